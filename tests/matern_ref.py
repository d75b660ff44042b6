"""NumPy restatement of the Matern covariance families that the GPU computes (csrc/kernel_build.hip, csrc/ard_grad.hip), shared by
the Matern tests.  Not in the reference, which has the squared exponential only; pinned against long double in
tests/test_matern_ref_cpu.py the way hyper_ref.py is.

With r^2 = sum_k (x_k - x'_k)^2 / ls_k^2:
    "se"        k = exp(-r^2 / 2)                              g = k
    "matern32"  a = sqrt(3) r, k = (1 + a) exp(-a)             g = 3 exp(-a)
    "matern52"  a = sqrt(5) r, k = (1 + a + a^2 / 3) exp(-a)   g = 5/3 (1 + a) exp(-a)
and dk / dlog ls_k = g(r) (x_k - x'_k)^2 / ls_k^2 (nothing is divided by r).  The likelihoods are those of ard_fit_ref.py and
hyper_ref.py with g in the place of K0 inside the length-scale gradients; `scale` is the size of each cancelling sum, as there."""
import numpy as np
import scipy.linalg as sla

from hyper_ref import _profile

FAMILIES = ("se", "matern32", "matern52")
MATERN = ("matern32", "matern52")


def sqdist(X1, X2, ls, dtype=np.float64):
    """r^2 [n1 x n2], features added in index order."""
    X1, X2 = np.asarray(X1, dtype=dtype), np.asarray(X2, dtype=dtype)
    ls = np.asarray(ls, dtype=dtype).reshape(-1)
    r2 = np.zeros((len(X1), len(X2)), dtype=dtype)
    for k in range(X1.shape[1]):
        diff = X1[:, k, None] - X2[None, :, k]
        r2 += diff * diff / (ls[k] * ls[k])
    return r2


def of_r2(r2, family):
    """(k, g) as functions of r^2, in the dtype of r2."""
    t = r2.dtype.type
    if family == "se":
        k = np.exp(-r2 / t(2))
        return k, k
    if family == "matern32":
        a = np.sqrt(t(3) * r2)
        e = np.exp(-a)
        return (t(1) + a) * e, t(3) * e
    if family == "matern52":
        a = np.sqrt(t(5) * r2)
        e = np.exp(-a)
        return (t(1) + a + t(5) * r2 / t(3)) * e, t(5) / t(3) * (t(1) + a) * e
    raise ValueError(f"unknown family {family!r}")


def kernel(X1, X2, ls, family, dtype=np.float64):
    """k(X1, X2) [n1 x n2], unit prior variance, no diagonal term."""
    return of_r2(sqdist(X1, X2, ls, dtype), family)[0]


def gram(X, ls, family, jitter1, jitter2, dtype=np.float64):
    """K(X, X) with the diagonal (1 + jitter1) + jitter2, rounded in that order as the GPU does."""
    K = kernel(X, X, ls, family, dtype)
    t = K.dtype.type
    K[np.diag_indices_from(K)] = (t(1) + t(jitter1)) + t(jitter2)
    return K


def posterior(X, y, Xs, ls, family, jitter1=1e-4, jitter2=1e-6):
    """(mu [M], sigma [M]) by the Cholesky route: mu = K* K^-1 y, sigma = sqrt(|prior - |L^-1 K*^T|^2|), prior = the diagonal of K."""
    y = np.asarray(y, dtype=np.float64).reshape(-1)
    L = np.linalg.cholesky(gram(X, ls, family, jitter1, jitter2))
    Ks = kernel(Xs, X, ls, family)
    mu = Ks @ sla.cho_solve((L, True), y)
    v = sla.solve_triangular(L, Ks.T, lower=True)
    prior = (1.0 + jitter1) + jitter2
    return mu, np.sqrt(np.abs(prior - np.sum(v * v, axis=0)))


def posterior_longdouble(X, y, Xs, ls, family, jitter1=1e-4, jitter2=1e-6):
    """The same posterior with K, K*, the Cholesky factor and both triangular solves in np.longdouble."""
    ld = np.longdouble
    K = gram(X, ls, family, jitter1, jitter2, dtype=ld)
    N = len(K)
    L = np.zeros((N, N), dtype=ld)
    for j in range(N):
        L[j, j] = np.sqrt(K[j, j] - L[j, :j] @ L[j, :j])
        if j + 1 < N:
            L[j + 1:, j] = (K[j + 1:, j] - L[j + 1:, :j] @ L[j, :j]) / L[j, j]
    Ks = kernel(Xs, X, ls, family, dtype=ld)
    B = np.concatenate([np.asarray(y, dtype=ld).reshape(-1, 1), Ks.T], axis=1)   # L^-1 [y | K*^T] by forward substitution
    for i in range(N):
        B[i] = (B[i] - L[i, :i] @ B[:i]) / L[i, i]
    mu = B[:, 1:].T @ B[:, 0]
    prior = (ld(1) + ld(jitter1)) + ld(jitter2)
    return mu, np.sqrt(np.abs(prior - np.sum(B[:, 1:] * B[:, 1:], axis=0)))


def _length_scale_gradients(W, X, ls, family):
    """(g [d], scale [d]): 1/2 sum_ij W_ij g(r_ij) (x_ik - x_jk)^2 / ls_k^2 and the sum of the terms' absolute values."""
    X = np.asarray(X, dtype=np.float64)
    G = of_r2(sqdist(X, X, ls), family)[1]
    WG = W * G
    d = X.shape[1]
    g, sc = np.empty(d), np.empty(d)
    for k in range(d):
        diff = (X[:, k, None] - X[None, :, k]) / ls[k]
        dk = diff * diff
        g[k] = 0.5 * np.sum(WG * dk)
        sc[k] = 0.5 * np.sum(np.abs(WG * dk))
    return g, sc


def nlml_and_grad(X, y, ls, family, jitter=1e-4, with_scale=False):
    """ard_fit_ref.nlml_and_grad for a family: (NLML, gradient in log ls [d][, scale [d]]); NaN when K is not positive definite."""
    X = np.asarray(X, dtype=np.float64)
    y = np.asarray(y, dtype=np.float64).reshape(-1)
    ls = np.asarray(ls, dtype=np.float64).reshape(-1)
    N, d = X.shape
    try:
        L = np.linalg.cholesky(kernel(X, X, ls, family) + jitter * np.eye(N))
    except np.linalg.LinAlgError:
        nan = np.full(d, np.nan)
        return (np.nan, nan, nan) if with_scale else (np.nan, nan)
    alpha = sla.cho_solve((L, True), y)
    Kinv = sla.cho_solve((L, True), np.eye(N))
    f = 0.5 * (y @ alpha + 2.0 * np.sum(np.log(np.diag(L))) + N * np.log(2.0 * np.pi))
    g, sc = _length_scale_gradients(Kinv - np.outer(alpha, alpha), X, ls, family)
    return (f, g, sc) if with_scale else (f, g)


def nlml_hyper(X, y, ls, noise, family, fit_mean=True, fit_scale=True, with_scale=False):
    """hyper_ref.nlml_hyper for a family: (L, gradient [d + 1] in (log ls, log rho), m, s^2[, scale [d + 1]])."""
    X = np.asarray(X, dtype=np.float64)
    y = np.asarray(y, dtype=np.float64).reshape(-1)
    ls = np.asarray(ls, dtype=np.float64).reshape(-1)
    N, d = X.shape
    nan = np.full(d + 1, np.nan)
    bad = (np.nan, nan, np.nan, np.nan, nan) if with_scale else (np.nan, nan, np.nan, np.nan)
    try:
        L = np.linalg.cholesky(kernel(X, X, ls, family) + noise * np.eye(N))
    except np.linalg.LinAlgError:
        return bad
    a = sla.cho_solve((L, True), y)
    b = sla.cho_solve((L, True), np.ones(N))
    Kinv = sla.cho_solve((L, True), np.eye(N))
    m, r, alpha, ra, s2, one_b = _profile(y, a, b, fit_mean, fit_scale)
    if not (np.isfinite(one_b) and one_b > 0 and np.isfinite(s2) and s2 > 0):
        return bad
    f = 0.5 * (ra / s2 + N * np.log(s2) + 2.0 * np.sum(np.log(np.diag(L))) + N * np.log(2.0 * np.pi))
    g, sc = np.empty(d + 1), np.empty(d + 1)
    g[:d], sc[:d] = _length_scale_gradients(Kinv - np.outer(alpha, alpha) / s2, X, ls, family)
    tr, aa = np.trace(Kinv), alpha @ alpha / s2
    g[d] = 0.5 * noise * (tr - aa)
    sc[d] = 0.5 * noise * (tr + aa)
    return (f, g, float(m), float(s2), sc) if with_scale else (f, g, float(m), float(s2))


def mean_scale_longdouble(X, y, ls, noise, family, fit_mean=True, fit_scale=True, sweeps=4):
    """hyper_ref.mean_scale_longdouble for a family."""
    ld = np.longdouble
    N = len(X)
    Kt = kernel(X, X, ls, family, dtype=ld) + ld(noise) * np.eye(N, dtype=ld)
    L = np.linalg.cholesky(Kt.astype(np.float64))
    yl = np.asarray(y, dtype=ld).reshape(-1)

    def solve(rhs):
        x = np.zeros(N, dtype=ld)
        for _ in range(sweeps):
            x = x + sla.cho_solve((L, True), (rhs - Kt @ x).astype(np.float64)).astype(ld)
        return x

    m, _, _, _, s2, _ = _profile(yl, solve(yl), solve(np.ones(N, dtype=ld)), fit_mean, fit_scale)
    return m, s2


def objective(X, y, family, fit_mean=True, fit_scale=True):
    """(ls, noise) -> (value, gradient, mean, scale2): what ard_fit.fit_hyperparameters drives."""
    return lambda ls, noise: nlml_hyper(X, y, ls, noise, family, fit_mean, fit_scale)


def gp_problem(seed, N, d, family="matern52", ls_true=None, noise=0.05):
    """ard_fit_ref.gp_problem with the draw from the Matern prior: uniform points in [0, 1]^d, ARD length scales ls_true (default
    geomspace(0.3, 1.0, d)), unit signal variance, independent noise of standard deviation `noise`."""
    rng = np.random.default_rng(seed)
    ls_true = np.geomspace(0.3, 1.0, d) if ls_true is None else np.asarray(ls_true, dtype=np.float64)
    X = rng.uniform(0.0, 1.0, (N, d))
    K = kernel(X, X, ls_true, family) + 1e-8 * np.eye(N)
    y = np.linalg.cholesky(K) @ rng.standard_normal(N) + noise * rng.standard_normal(N)
    return X, y


# ---- cases shared by tests/test_gpu_matern.py and the CPU checks of their premises (tests/test_matern_ref_cpu.py) ---------
# selection: (N, M, d) of synthetic.make_problem whose two largest acquisition values are further apart than the tolerance
SELECTION_SHAPES = [(63, 1000, 3), (129, 1537, 3), (300, 4096, 8)]
EI_XI = 0.01
# the fit: seeds of gp_problem(seed, 200, 3, family, noise=0.01) whose optimum is interior and well conditioned - a 1e-9 relative
# perturbation of the gradient moves the fitted length scales of the CPU optimiser by < 1e-12 relative (both families)
FIT_SEEDS = [1, 3]
FIT_BOX = dict(ls0=[0.5] * 3, lower=[0.05] * 3, upper=[5.0] * 3)
