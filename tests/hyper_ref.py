"""NumPy restatement of the ML-II objective over all hyperparameters that the GPU computes (csrc/hyper.hip), shared by the
hyperparameter tests.

Model y ~ N(m 1, s^2 Kt), Kt = K0(ls) + rho I.  With a = Kt^-1 y and b = Kt^-1 1:
    m = (1 . a) / (1 . b) when the mean is fitted, else 0;  r = y - m;  alpha = a - m b
    s^2 = (r . alpha) / N when the scale is fitted, else 1
    L = 1/2 [(r . alpha) / s^2 + N log s^2 + log det Kt + N log 2 pi]
    dL / dlog ls_k = 1/2 sum_ij W_ij K0_ij (x_ik - x_jk)^2 / ls_k^2,   W = Kt^-1 - alpha alpha^T / s^2
    dL / dlog rho  = 1/2 rho (tr Kt^-1 - |alpha|^2 / s^2)
`scale` is the size of each cancelling sum (the tests' tolerance unit), as in ard_fit_ref: the absolute values of the terms for a
length scale, 1/2 rho (tr Kt^-1 + |alpha|^2 / s^2) for the noise.
Leave-one-out: mu_i = y_i - alpha_i / kappa_i, var_i = s^2 / kappa_i, kappa = diag Kt^-1."""
import numpy as np
import scipy.linalg as sla


def kernel(X, ls, dtype=np.float64):
    X = np.asarray(X, dtype=dtype)
    Xs = X / np.asarray(ls, dtype=dtype).reshape(-1)
    D2 = np.zeros((len(X), len(X)), dtype=dtype)
    for k in range(X.shape[1]):
        D2 += (Xs[:, k, None] - Xs[None, :, k]) ** 2
    return np.exp(-D2 / dtype(2)), Xs


def _profile(y, a, b, fit_mean, fit_scale):
    N = len(y)
    one_b = b.sum()
    m = a.sum() / one_b if fit_mean else y.dtype.type(0)
    r = y - m
    alpha = a - m * b
    ra = r @ alpha
    s2 = ra / N if fit_scale else y.dtype.type(1)
    return m, r, alpha, ra, s2, one_b


def nlml_hyper(X, y, ls, noise, fit_mean=True, fit_scale=True, with_scale=False, with_parts=False):
    """(L, gradient [d + 1] in (log ls, log rho), m, s^2[, scale [d + 1]]); NaN everywhere when Kt is not positive definite, when
    1 . b is not positive or when s^2 is not."""
    X = np.asarray(X, dtype=np.float64)
    y = np.asarray(y, dtype=np.float64).reshape(-1)
    ls = np.asarray(ls, dtype=np.float64).reshape(-1)
    N, d = X.shape
    nan = np.full(d + 1, np.nan)
    bad = (np.nan, nan, np.nan, np.nan, nan) if with_scale else (np.nan, nan, np.nan, np.nan)
    K0, Xs = kernel(X, ls)
    try:
        L = np.linalg.cholesky(K0 + noise * np.eye(N))
    except np.linalg.LinAlgError:
        return bad
    a = sla.cho_solve((L, True), y)
    b = sla.cho_solve((L, True), np.ones(N))
    Kinv = sla.cho_solve((L, True), np.eye(N))
    m, r, alpha, ra, s2, one_b = _profile(y, a, b, fit_mean, fit_scale)
    if not (np.isfinite(one_b) and one_b > 0 and np.isfinite(s2) and s2 > 0):
        return bad
    f = 0.5 * (ra / s2 + N * np.log(s2) + 2.0 * np.sum(np.log(np.diag(L))) + N * np.log(2.0 * np.pi))
    W = Kinv - np.outer(alpha, alpha) / s2
    WK = W * K0
    g, sc = np.empty(d + 1), np.empty(d + 1)
    for k in range(d):
        dk = (Xs[:, k, None] - Xs[None, :, k]) ** 2
        g[k] = 0.5 * np.sum(WK * dk)
        sc[k] = 0.5 * np.sum(np.abs(WK * dk))
    tr, aa = np.trace(Kinv), alpha @ alpha / s2
    g[d] = 0.5 * noise * (tr - aa)
    sc[d] = 0.5 * noise * (tr + aa)
    if with_parts:
        return dict(f=f, g=g, m=m, s2=s2, scale=sc, alpha=alpha, r=r, kinv_diag=np.diag(Kinv).copy())
    return (f, g, float(m), float(s2), sc) if with_scale else (f, g, float(m), float(s2))


def loo(X, y, ls, noise, fit_mean=True, fit_scale=True):
    """(mu_loo, var_loo, diag Kt^-1) with m and s^2 held at their fitted values."""
    p = nlml_hyper(X, y, ls, noise, fit_mean, fit_scale, with_parts=True)
    y = np.asarray(y, dtype=np.float64).reshape(-1)
    return y - p["alpha"] / p["kinv_diag"], p["s2"] / p["kinv_diag"], p["kinv_diag"]


def mean_scale_longdouble(X, y, ls, noise, fit_mean=True, fit_scale=True, sweeps=4):
    """(m, s^2) of the same formulas in np.longdouble: Kt is built in longdouble, a and b are the float64 Cholesky solves
    refined against longdouble residuals (each sweep gains a factor ~ cond(Kt) 2^-53), the sums are longdouble."""
    ld = np.longdouble
    K0, _ = kernel(X, ls, dtype=ld)
    N = len(K0)
    Kt = K0 + ld(noise) * np.eye(N, dtype=ld)
    L = np.linalg.cholesky(Kt.astype(np.float64))
    yl = np.asarray(y, dtype=ld).reshape(-1)

    def solve(rhs):
        x = np.zeros(N, dtype=ld)
        for _ in range(sweeps):
            res = rhs - Kt @ x
            x = x + sla.cho_solve((L, True), res.astype(np.float64)).astype(ld)
        return x

    a, b = solve(yl), solve(np.ones(N, dtype=ld))
    m, _, _, _, s2, _ = _profile(yl, a, b, fit_mean, fit_scale)
    return m, s2


def objective(X, y, fit_mean=True, fit_scale=True):
    """(ls, noise) -> (value, gradient, mean, scale2): what ard_fit.fit_hyperparameters drives."""
    return lambda ls, noise: nlml_hyper(X, y, ls, noise, fit_mean, fit_scale)
