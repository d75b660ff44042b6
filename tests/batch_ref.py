"""NumPy references for greedy q-point batch selection (csrc/batch.hip).

The reference project selects ONE point per iteration (point_selector.py:197-207), so there is no reference output to
compare a batch with: parity is pinned by the two restatements below, held to each other in tests/test_batch_ref_cpu.py.

  greedy_refit       what the feature MEANS: after every member the GP is refitted from scratch (fresh Cholesky) on the
                     observations plus the fantasy observations so far, the members chosen so far are masked, and the first
                     arg-max is taken.
  greedy_recurrence  what the kernel COMPUTES: the rank-one recurrence on the dense posterior of the original GP.
"""
import numpy as np
import scipy.linalg as sla

from oracle import gp_oracle as O

KAPPA = O.PRIOR_VAR   # diagonal of K = (1 + 1e-4) + 1e-6, also the prior variance the classes pass

# the problems and modes of the issue: make_problem(N, M, d), q = 8
PROBLEMS = [(64, 2048, 2), (300, 4096, 8), (700, 4096, 8), (512, 4096, 16)]
Q = 8
MODE_NAMES = ["lcb_believer", "ei_believer", "ei_liar_min", "lcb_liar_max"]


def mode(name, y):
    """(acquisition keywords of DeviceGP / host_binding, fantasy, lie) of a mode by name."""
    y = np.asarray(y, dtype=np.float64)
    return {
        "lcb_believer": (dict(acquisition="lcb", explore=4.0), "believer", None),
        "ei_believer": (dict(acquisition="ei", f_best=float(y.min()), xi=0.0), "believer", None),
        "ei_liar_min": (dict(acquisition="ei", f_best=float(y.min()), xi=0.0), "liar", float(y.min())),
        "lcb_liar_max": (dict(acquisition="lcb", explore=4.0), "liar", float(y.max())),
    }[name]


def kernel(A, B, ls):
    """k(A, B) without any jitter (the shape-coincidence quirk of point_selector.py:173 is not part of this feature)."""
    A, B = np.asarray(A, dtype=np.float64), np.asarray(B, dtype=np.float64)
    ls = np.asarray(ls, dtype=np.float64).reshape(-1)
    acc = np.zeros((A.shape[0], B.shape[0]))
    for k in range(A.shape[1]):
        acc += (A[:, k, None] - B[None, :, k]) ** 2 / ls[k] ** 2
    return np.exp(-0.5 * acc)


def acquisition(mu, sigma, acquisition="lcb", explore=4.0, f_best=None, xi=0.0):
    if acquisition == "lcb":
        return O.lcb(mu, sigma, explore)
    return O.expected_improvement(mu, sigma, f_best, xi)


def _pick(acq, chosen):
    """(first arg-max with the chosen masked, its value, the gap to the runner-up)."""
    a = np.array(acq, dtype=np.float64)
    a[chosen] = -np.inf
    i = int(np.flatnonzero(a == a.max())[0])
    rest = np.delete(a, i)
    gap = float(a[i] - rest.max()) if rest.size and np.isfinite(rest.max()) else np.inf
    return i, float(acq[i]), gap


def posterior(X, y, Xs, ls):
    """(mu, sigma) at Xs of the GP on (X, y), K = k(X, X) + KAPPA-diagonal: fresh Cholesky."""
    K = kernel(X, X, ls)
    K[np.diag_indices_from(K)] = KAPPA
    L = np.linalg.cholesky(K)
    Ks = kernel(X, Xs, ls)
    mu = Ks.T @ sla.cho_solve((L, True), np.asarray(y, dtype=np.float64))
    v = sla.solve_triangular(L, Ks, lower=True, check_finite=False)
    return mu, np.sqrt(np.abs(KAPPA - np.einsum("nm,nm->m", v, v)))


def greedy_refit(X, y, Xs, ls, q, acq_kw, fantasy="believer", lie=None):
    """dict(indices, values, gaps, mu, sigma): mu / sigma are the posterior the q-th member was chosen from."""
    Xa, ya = np.array(X, dtype=np.float64), np.array(y, dtype=np.float64).reshape(-1)
    Xs = np.asarray(Xs, dtype=np.float64)
    idx, val, gaps = [], [], []
    for j in range(q):
        mu, sigma = posterior(Xa, ya, Xs, ls)
        i, v, g = _pick(acquisition(mu, sigma, **acq_kw), idx)
        idx.append(i), val.append(v), gaps.append(g)
        yj = mu[i] if fantasy == "believer" else float(lie)
        Xa, ya = np.vstack([Xa, Xs[i: i + 1]]), np.append(ya, yj)
    return dict(indices=np.array(idx, dtype=np.int64), values=np.array(val), gaps=np.array(gaps), mu=mu, sigma=sigma)


def greedy_recurrence(X, y, Xs, ls, q, acq_kw, fantasy="believer", lie=None, prior_var=KAPPA):
    """The same batch by rank-one updates of the dense posterior of the ORIGINAL GP (the kernel's arithmetic):
        t_j(c) = k(c, x_j) - k_c . beta_j - sum_{i<j} t_i(c) t_i(x_j) / s_i,   beta_j = K^-1 k(X, x_j)
        s_j = var_j(x_j) - prior_var + KAPPA;   var' = var - t_j^2 / s_j;   mu' = mu + t_j (y_j - mu(x_j)) / s_j
    with the variance state carried as sigma = sqrt(|var|)."""
    X, Xs = np.asarray(X, dtype=np.float64), np.asarray(Xs, dtype=np.float64)
    K = kernel(X, X, ls)
    K[np.diag_indices_from(K)] = KAPPA
    L = np.linalg.cholesky(K)
    Ks = kernel(X, Xs, ls)
    mu = Ks.T @ sla.cho_solve((L, True), np.asarray(y, dtype=np.float64).reshape(-1))
    v = sla.solve_triangular(L, Ks, lower=True, check_finite=False)
    sigma = np.sqrt(np.abs(prior_var - np.einsum("nm,nm->m", v, v)))
    idx, val, gaps, T, S = [], [], [], [], []
    for j in range(q):
        i, a, g = _pick(acquisition(mu, sigma, **acq_kw), idx)
        idx.append(i), val.append(a), gaps.append(g)
        if j + 1 == q:
            break
        xj = Xs[i: i + 1]
        beta = sla.cho_solve((L, True), kernel(X, xj, ls)[:, 0])
        t = kernel(Xs, xj, ls)[:, 0] - Ks.T @ beta
        for ti, si in zip(T, S):
            t = t - ti * (ti[i] / si)
        s = sigma[i] ** 2 + (KAPPA - prior_var)
        yj = mu[i] if fantasy == "believer" else float(lie)
        mu = mu + t * ((yj - mu[i]) / s)
        sigma = np.sqrt(np.abs(sigma ** 2 - t * t / s))
        T.append(t), S.append(s)
    return dict(indices=np.array(idx, dtype=np.int64), values=np.array(val), gaps=np.array(gaps), mu=mu, sigma=sigma)
