"""NumPy reference of the ML-II objective the GPU computes (csrc/ard_grad.hip), shared by the ARD-fit tests.

K = K0 + jitter I, K0_ij = exp(-1/2 sum_k (x_ik - x_jk)^2 / l_k^2), alpha = K^-1 y, W = K^-1 - alpha alpha^T:
    NLML             = 1/2 (y . alpha + log det K + N log 2 pi)
    dNLML / dlog l_k = 1/2 sum_ij W_ij K0_ij (x_ik - x_jk)^2 / l_k^2
`scale[k]` = 1/2 sum_ij |W_ij K0_ij (x_ik - x_jk)^2 / l_k^2|: the size of the cancelling sum (the tests' tolerance unit)."""
import numpy as np
import scipy.linalg as sla

JITTER = 1e-4


def nlml_and_grad(X, y, ls, jitter=JITTER, with_scale=False):
    X = np.asarray(X, dtype=np.float64)
    y = np.asarray(y, dtype=np.float64).reshape(-1)
    ls = np.asarray(ls, dtype=np.float64).reshape(-1)
    N, d = X.shape
    Xs = X / ls
    D2 = np.zeros((N, N))
    for k in range(d):
        D2 += (Xs[:, k, None] - Xs[None, :, k]) ** 2
    K0 = np.exp(-0.5 * D2)
    try:
        L = np.linalg.cholesky(K0 + jitter * np.eye(N))
    except np.linalg.LinAlgError:
        nan = np.full(d, np.nan)
        return (np.nan, nan, nan) if with_scale else (np.nan, nan)
    alpha = sla.cho_solve((L, True), y)
    Kinv = sla.cho_solve((L, True), np.eye(N))
    W = Kinv - np.outer(alpha, alpha)
    f = 0.5 * (y @ alpha + 2.0 * np.sum(np.log(np.diag(L))) + N * np.log(2.0 * np.pi))
    WK = W * K0
    g, s = np.empty(d), np.empty(d)
    for k in range(d):
        dk = (Xs[:, k, None] - Xs[None, :, k]) ** 2
        g[k] = 0.5 * np.sum(WK * dk)
        s[k] = 0.5 * np.sum(np.abs(WK * dk))
    return (f, g, s) if with_scale else (f, g)


def gp_problem(seed, N, d, ls_true=None, noise=0.05):
    """A seeded draw of a GP with ARD length scales ls_true (default geomspace(0.3, 1.0, d)) at uniform points in [0, 1]^d."""
    rng = np.random.default_rng(seed)
    ls_true = np.geomspace(0.3, 1.0, d) if ls_true is None else np.asarray(ls_true, dtype=np.float64)
    X = rng.uniform(0.0, 1.0, (N, d))
    Xs = X / ls_true
    sq = np.sum(Xs * Xs, axis=1)
    K = np.exp(-0.5 * np.maximum(sq[:, None] + sq[None, :] - 2.0 * Xs @ Xs.T, 0.0)) + 1e-8 * np.eye(N)
    y = np.linalg.cholesky(K) @ rng.standard_normal(N) + noise * rng.standard_normal(N)
    return X, y
