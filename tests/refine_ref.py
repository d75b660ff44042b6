"""NumPy restatement of the acquisition gradients and of the off-grid refinement rule (csrc/refine.hip).

The reference project answers with one of the candidates it was given (point_selector.py:197-207), so there is no reference
output to compare a refined point with: parity is pinned by this restatement on the Cholesky route, which is itself held to
central differences in long double (tests/test_refine_ref_cpu.py).  The product never imports this file.

For a query point x, k_n = exp(-1/2 sum_k (x_k - X_nk)^2 / ls_k^2) and g_nk = (X_nk - x_k) / ls_k^2:
    mu    = sum_n k_n alpha_n                  dmu_k  = sum_n k_n alpha_n g_nk
    v     = L^-1 k, var = KAPPA - |v|^2        w = L^-T v (= K^-1 k),  dvar_k = -2 sum_n k_n w_n g_nk
    sigma = sqrt(|var|)                        dsigma_k = sign(var) dvar_k / (2 sigma)        (0 when sigma == 0)
    LCB: acq = p0 sigma - mu                   dacq = p0 dsigma - dmu
    EI : imp = p0 - mu - p1, z = imp / sigma   dacq = -Phi(z) dmu + phi(z) dsigma   (sigma == 0: -dmu if imp > 0, else 0)
"""
import numpy as np
import scipy.linalg as sla
import scipy.special as sps

from oracle import gp_oracle as O

KAPPA = O.PRIOR_VAR   # diagonal of K = (1 + 1e-4) + 1e-6, also the prior variance the classes pass
C1 = 1e-4             # Armijo constant of the rule
DECIDED = 1e-7        # a point is decided when its smallest Armijo margin exceeds this
MAX_UNDECIDED = 4     # of 64

# the trajectory cases of the issue: make_problem(N, M, d), 64 starts, 12 iterations, box [0, 1]^d
CASES = [(300, 4096, 8), (700, 4096, 8), (512, 4096, 16)]
TABLE = [(64, 2048, 2), (300, 4096, 8), (700, 4096, 8), (512, 4096, 16)]   # the issue's table: 30 iterations, EI at min y
ACQS = ["lcb", "ei"]
N_STARTS, TRAJ_ITERS = 64, 12


def acq_kw(name, y, table=False):
    """Acquisition keywords of DeviceGP by name: LCB(4), or EI at the 0.1 quantile of y (min y for the issue's table)."""
    y = np.asarray(y, dtype=np.float64)
    if name == "lcb":
        return dict(acquisition="lcb", explore=4.0)
    return dict(acquisition="ei", f_best=float(np.min(y) if table else np.quantile(y, 0.1)), xi=0.0)


def _kernel(A, B, ls, dtype):
    A, B, ls = np.asarray(A, dtype=dtype), np.asarray(B, dtype=dtype), np.asarray(ls, dtype=dtype).reshape(-1)
    acc = np.zeros((A.shape[0], B.shape[0]), dtype=dtype)
    for k in range(A.shape[1]):
        acc += (A[:, k, None] - B[None, :, k]) ** 2 / ls[k] ** 2
    return np.exp(-acc / 2)


def _cholesky_any(K):
    """Left-looking Cholesky in the matrix's own dtype (numpy.linalg has no long double)."""
    n = K.shape[0]
    L = np.zeros_like(K)
    for j in range(n):
        c = K[j:, j] - L[j:, :j] @ L[j, :j]
        L[j:, j] = c / np.sqrt(c[0])
    return L


def _solve_lower_any(L, B):
    Y = np.array(B, dtype=L.dtype)
    for i in range(L.shape[0]):
        Y[i] = (Y[i] - L[i, :i] @ Y[:i]) / L[i, i]
    return Y


def _solve_upper_any(U, B):
    Y = np.array(B, dtype=U.dtype)
    for i in range(U.shape[0] - 1, -1, -1):
        Y[i] = (Y[i] - U[i, i + 1:] @ Y[i + 1:]) / U[i, i]
    return Y


class Model:
    """The factorised GP on (X, y): K = k(X, X) with KAPPA on the diagonal, Cholesky route, in float64 or long double."""

    def __init__(self, X, y, ls, dtype=np.float64):
        self.dtype = dtype
        self.X = np.asarray(X, dtype=dtype)
        self.ls = np.asarray(ls, dtype=dtype).reshape(-1)
        y = np.asarray(y, dtype=dtype).reshape(-1)
        K = _kernel(self.X, self.X, self.ls, dtype)
        K[np.diag_indices_from(K)] = dtype(KAPPA)
        if dtype == np.float64:
            self.L = np.linalg.cholesky(K)
            self.alpha = sla.cho_solve((self.L, True), y)
        else:
            self.L = _cholesky_any(K)
            self.alpha = _solve_upper_any(self.L.T, _solve_lower_any(self.L, y))

    def _lower(self, B):
        return sla.solve_triangular(self.L, B, lower=True, check_finite=False) if self.dtype == np.float64 \
            else _solve_lower_any(self.L, B)

    def _upper(self, B):
        return sla.solve_triangular(self.L.T, B, lower=False, check_finite=False) if self.dtype == np.float64 \
            else _solve_upper_any(self.L.T, B)

    def values(self, Q):
        """(mu, var) at the rows of Q."""
        k = _kernel(np.asarray(Q, dtype=self.dtype), self.X, self.ls, self.dtype)          # [P x N]
        v = self._lower(k.T)
        return k @ self.alpha, self.dtype(KAPPA) - np.einsum("np,np->p", v, v)

    def grad(self, Q, acquisition="lcb", explore=4.0, f_best=None, xi=0.0):
        """dict(mu, sigma, acq [P], dmu, dsigma, dacq [P x d]) at the rows of Q."""
        dt = self.dtype
        Q = np.asarray(Q, dtype=dt).reshape(-1, self.X.shape[1])
        k = _kernel(Q, self.X, self.ls, dt)                                                # [P x N]
        v = self._lower(k.T)
        w = self._upper(v).T                                                               # [P x N]
        g = (self.X[None, :, :] - Q[:, None, :]) / self.ls[None, None, :] ** 2             # [P x N x d]
        mu = k @ self.alpha
        var = dt(KAPPA) - np.einsum("np,np->p", v, v)
        dmu = np.einsum("pn,pnk->pk", k * self.alpha[None, :], g)
        dvar = -2 * np.einsum("pn,pnk->pk", k * w, g)
        sigma = np.sqrt(np.abs(var))
        with np.errstate(divide="ignore", invalid="ignore"):
            dsigma = np.where(sigma[:, None] == 0, dt(0), np.sign(var)[:, None] * dvar / (2 * sigma[:, None]))
        acq, cm, cs = acquisition_and_weights(mu, sigma, acquisition, explore, f_best, xi)
        return dict(mu=mu, sigma=sigma, acq=acq, dmu=dmu, dsigma=dsigma, dacq=cm[:, None] * dmu + cs[:, None] * dsigma)


def acquisition_and_weights(mu, sigma, acquisition="lcb", explore=4.0, f_best=None, xi=0.0):
    """(acq, cm, cs) with dacq = cm dmu + cs dsigma.  Phi and phi are evaluated in float64 (scipy has no long double)."""
    dt = mu.dtype.type
    if acquisition == "lcb":
        return dt(explore) * sigma - mu, np.full_like(mu, -1), np.full_like(mu, dt(explore))
    imp = dt(f_best) - mu - dt(xi)
    pos = sigma > 0
    with np.errstate(divide="ignore", invalid="ignore"):
        z = np.where(pos, imp / np.where(pos, sigma, 1), 0)
    cdf = (0.5 * sps.erfc(-np.asarray(z, dtype=np.float64) * 0.70710678118654752440)).astype(mu.dtype)
    pdf = np.exp(-z * z / 2) * dt(0.39894228040143267794)
    acq = np.where(pos, imp * cdf + sigma * pdf, np.where(sigma == 0, np.maximum(imp, 0), sigma))
    cm = np.where(pos, -cdf, np.where(imp > 0, dt(-1), dt(0)))
    cs = np.where(pos, pdf, dt(0))
    return acq, cm, cs


def posterior_grad(X, y, ls, Q, acquisition="lcb", explore=4.0, f_best=None, xi=0.0, dtype=np.float64):
    """Values and gradients at the rows of Q; dtype=np.longdouble for the long-double variant (N <= 300 is quick)."""
    return Model(X, y, ls, dtype).grad(Q, acquisition, explore, f_best, xi)


def central_differences(model, Q, h=1e-7, **acq):
    """dict(dmu, dsigma, dacq) [P x d] by central differences of the model's own values (long double: h = 1e-7)."""
    dt = model.dtype
    Q = np.asarray(Q, dtype=dt)
    P, d = Q.shape
    pts = np.repeat(Q[:, None, None, :], d, axis=1).repeat(2, axis=2)                      # [P x d x 2 x d]
    for k in range(d):
        pts[:, k, 0, k] += dt(h)
        pts[:, k, 1, k] -= dt(h)
    mu, var = model.values(pts.reshape(-1, d))
    sigma = np.sqrt(np.abs(var))
    a = acquisition_and_weights(mu, sigma, **acq)[0]
    out = {}
    for name, f in (("dmu", mu), ("dsigma", sigma), ("dacq", a)):
        f = f.reshape(P, d, 2)
        out[name] = (f[:, :, 0] - f[:, :, 1]) / (2 * dt(h))
    return out


def refine(X, y, ls, starts, lower, upper, acquisition="lcb", explore=4.0, f_best=None, xi=0.0, iters=30, step0=0.1,
           model=None):
    """The refinement rule of the issue, every start on its own (vectorised over the starts, float64):
        x <- clip(start); (f, g) there; acq0 = f; t <- step0 / max_k(|g_k| ls_k), frozen when that is 0 or not finite
        iters times: x' = clip(x + t g ls^2); accept iff x' != x, f' finite and f' >= f + C1 sum_k g_k (x'_k - x_k)
                     (the sum in index order); accepted: (x, f, g) <- (x', f', g'), t <- 2 t; rejected: t <- t / 2
    Returns dict(x, acq, acq0, accepted, pg, margin, best): margin = each point's smallest |f' - (f + C1 g . dx)| over its
    evaluated trials (inf when there was none), best = the first arg-max of the final values."""
    m = model or Model(X, y, ls)
    ls = np.asarray(ls, dtype=np.float64).reshape(-1)
    d = ls.size
    lo = np.broadcast_to(np.asarray(lower, dtype=np.float64).reshape(-1), (d,))
    hi = np.broadcast_to(np.asarray(upper, dtype=np.float64).reshape(-1), (d,))
    l2 = ls * ls
    akw = dict(acquisition=acquisition, explore=explore, f_best=f_best, xi=xi)

    def ev(Q):
        with np.errstate(all="ignore"):
            r = m.grad(Q, **akw)
        return r["acq"], r["dacq"]

    with np.errstate(invalid="ignore"):
        x = np.clip(np.array(np.asarray(starts, dtype=np.float64).reshape(-1, d)), lo, hi)
    P = x.shape[0]
    f, g = ev(x)
    acq0 = f.copy()
    with np.errstate(invalid="ignore"):
        mx = np.max(np.abs(g) * ls[None, :], axis=1)
    frozen = ~(np.isfinite(mx) & (mx > 0))
    with np.errstate(all="ignore"):
        t = np.where(frozen, 0.0, step0 / np.where(frozen, 1.0, mx))
    accepted = np.zeros(P, dtype=np.int32)
    margin = np.full(P, np.inf)
    for _ in range(int(iters)):
        with np.errstate(invalid="ignore"):
            xn = np.where(frozen[:, None], x, np.clip(x + t[:, None] * g * l2[None, :], lo, hi))
        fn, gn = ev(xn)
        s = np.zeros(P)
        with np.errstate(invalid="ignore"):
            for k in range(d):
                s = s + g[:, k] * (xn[:, k] - x[:, k])
            bar = f + C1 * s
            moved = np.any(xn != x, axis=1) & ~frozen
            ok = moved & np.isfinite(fn) & (fn >= bar)
            gap = np.abs(fn - bar)
        margin = np.where(~frozen, np.minimum(margin, np.where(np.isfinite(gap), gap, 0.0)), margin)
        x = np.where(ok[:, None], xn, x)
        g = np.where(ok[:, None], gn, g)
        f = np.where(ok, fn, f)
        t = np.where(ok, 2.0 * t, t / 2.0)
        accepted += ok.astype(np.int32)
    with np.errstate(invalid="ignore"):
        pg = np.max(np.abs(x - np.clip(x + g * l2[None, :], lo, hi)) / ls[None, :], axis=1)
    fin = np.where(np.isnan(f), -np.inf, f)
    best = int(np.flatnonzero(fin == fin.max())[0]) if np.any(~np.isnan(f)) else -1
    return dict(x=x, acq=f, acq0=acq0, accepted=accepted, pg=pg, margin=margin, best=best,
                nan_count=int(np.isnan(acq0).sum()))


def dense_acquisition(X, y, Xs, ls, acquisition="lcb", explore=4.0, f_best=None, xi=0.0, model=None):
    m = model or Model(X, y, ls)
    mu, var = m.values(Xs)
    return acquisition_and_weights(mu, np.sqrt(np.abs(var)), acquisition, explore, f_best, xi)[0]


def starts(X, y, Xs, ls, acquisition="lcb", explore=4.0, f_best=None, xi=0.0, n=N_STARTS, model=None):
    """(indices, rows of Xs, the dense acquisition) of the n candidates with the largest acquisition, stable order."""
    a = dense_acquisition(X, y, Xs, ls, acquisition, explore, f_best, xi, model)
    idx = np.argsort(-a, kind="stable")[:n]
    return idx, np.asarray(Xs, dtype=np.float64)[idx], a


def decided(ref):
    """Mask of the points whose every accept / reject decision had a margin above DECIDED; at most MAX_UNDECIDED of a case
    may fail that (they are left out of a trajectory comparison)."""
    mask = ref["margin"] > DECIDED
    assert (~mask).sum() <= MAX_UNDECIDED, f"{(~mask).sum()} undecided points, smallest margin {ref['margin'].min():.3g}"
    return mask
