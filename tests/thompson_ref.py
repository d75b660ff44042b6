"""NumPy restatement of Thompson sampling by pathwise posterior samples (include/gpbo.h).  The reference has
no such thing; like EI, qEI, batches and refinement the feature is pinned by its formulas written out once more:

    f_s(x) = g_s(x) + sum_n k0(x, x_n) v_s[n]
    g_s(x) = sqrt(2 / F) sum_f W[s,f] cos(2 pi t_f(x)),   t_f(x) = sum_k Omega[f,k] x_k / (2 pi ls_k) + phase[f]
    v_s    = K^-1 (y - g_s(X) - sqrt(kappa) E[s,:]),      K = k0(X,X) + kappa I

Every function takes xp = np.float64 (default) or np.longdouble: the type all arithmetic runs in.
"""
import functools

import numpy as np

from bayesian_optimisation_amd.thompson import first_distinct, thompson_draws as draws  # noqa: F401  (re-exported)

KAPPA = 1e-4 + 1e-6   # jitter1 + jitter2 of the classes


def _two_pi(xp):
    return xp(2) * np.arccos(xp(-1))


def feats(Xs, ls, omega, phase, xp=np.float64):
    """cos(2 pi t_f(x_c)), [M x F]."""
    Xs, ls, omega, phase = (np.asarray(a, dtype=xp) for a in (Xs, ls, omega, phase))
    tp = _two_pi(xp)
    t = (Xs / (tp * ls)[None, :]) @ omega.T + phase[None, :]
    return np.cos(tp * t)


def k0(A, B, ls, xp=np.float64):
    """exp(-1/2 sum_k (a_k - b_k)^2 / ls_k^2), [len(A) x len(B)]."""
    A, B, ls = (np.asarray(a, dtype=xp) for a in (A, B, ls))
    s = np.zeros((len(A), len(B)), dtype=xp)
    for k in range(A.shape[1]):
        diff = (A[:, k, None] - B[None, :, k]) / ls[k]
        s += diff * diff
    return np.exp(-s / xp(2))


def prior_paths(Xs, ls, omega, phase, W, xp=np.float64):
    """g_s at the rows of Xs, [S x M]."""
    W = np.asarray(W, dtype=xp)
    return (np.sqrt(xp(2) / xp(W.shape[1])) * (feats(Xs, ls, omega, phase, xp) @ W.T)).T


def residual(X, y, ls, omega, phase, W, E, kappa=KAPPA, xp=np.float64):
    """R[s] = y - g_s(X) - sqrt(kappa) E[s], [S x N]."""
    return np.asarray(y, dtype=xp)[None, :] - prior_paths(X, ls, omega, phase, W, xp) - np.sqrt(xp(kappa)) * np.asarray(E, dtype=xp)


def weights(X, y, ls, omega, phase, W, E, kappa=KAPPA, xp=np.float64):
    """v_s, [S x N].  fp64: np.linalg.solve.  long double: the fp64 solve plus four steps of iterative refinement with the
    residual in long double."""
    R = residual(X, y, ls, omega, phase, W, E, kappa, xp).T   # [N x S]
    K = k0(X, X, ls, xp) + xp(kappa) * np.eye(len(X), dtype=xp)
    K64 = K.astype(np.float64)
    V = np.linalg.solve(K64, R.astype(np.float64)).astype(xp)
    if xp is not np.float64:
        for _ in range(4):
            V = V + np.linalg.solve(K64, (R - K @ V).astype(np.float64)).astype(xp)
    return V.T


def paths(Xs, X, ls, omega, phase, W, V, xp=np.float64):
    """f_s at the rows of Xs, [S x M]; V = None: the prior paths alone."""
    f = prior_paths(Xs, ls, omega, phase, W, xp)
    if V is not None:
        # row by row through np.sum (pairwise), not through a BLAS product: with |V| ~ 10 the partial sums of the N terms
        # reach the hundreds, and an unspecified blocked summation order then costs a fifth of the bound below by itself
        k, V = k0(Xs, X, ls, xp), np.asarray(V, dtype=xp)
        f = f + np.stack([(k * V[s][None, :]).sum(axis=1) for s in range(len(V))])
    return f


def bound(Xs, ls, omega, phase, W, V, d):
    """The kernel-level tolerance [S x M], derived, not measured: an argument error of (d + 2) roundings times the cosine's
    slope 2 pi, a few ulp each for cos and exp, and the summations:
        tol[s,c] = (d + 8) 2^-53 (sqrt(2/F) sum_f |W[s,f]| (1 + 2 pi (sum_k |Omega[f,k] x_ck| / (2 pi ls_k) + |phase_f|))
                                  + sum_n |V[s,n]|)"""
    Xs, ls, omega, phase, W = (np.asarray(a, dtype=np.float64) for a in (Xs, ls, omega, phase, W))
    F = W.shape[1]
    A = (np.abs(Xs) / (2 * np.pi * ls)[None, :]) @ np.abs(omega).T + np.abs(phase)[None, :]   # [M x F]
    t = np.sqrt(2.0 / F) * (np.abs(W) @ (1.0 + 2 * np.pi * A).T)                              # [S x M]
    if V is not None:
        t = t + np.abs(np.asarray(V, dtype=np.float64)).sum(axis=1)[:, None]
    return (d + 8) * 2.0 ** -53 * t


def winners(f):
    """Per path: (first index of the arg-max of -f, the gap between the best and the runner-up value of -f)."""
    a = -np.asarray(f)
    idx = np.argmax(a, axis=1)   # first occurrence
    if a.shape[1] == 1:
        return idx, np.full(a.shape[0], np.inf)
    top = np.partition(a, -2, axis=1)[:, -2:]
    return idx, (top[:, 1] - top[:, 0]).astype(np.float64)


# The cases of the kernel test (N, M, d, F, S): the odd and the even observation tail, N at and around the 128 padding, M at
# and around the 512 candidates of a workgroup, a path count that is no multiple of the path group, the S maximum.
KERNEL_CASES = [(1, 1, 1, 1, 1), (5, 513, 3, 63, 2), (128, 511, 5, 2, 15), (127, 512, 2, 1000, 16), (129, 1025, 8, 257, 17),
                (300, 1537, 16, 64, 64), (2049, 4097, 8, 1025, 33)]


V_SEED = 0   # not chosen by its results: see test_thompson_ref_cpu.py for what every seed from 1 to 12 gave


def kernel_case(N, M, d, F, S, seed=7):
    """Inputs of one kernel case: observations and candidates of make_problem (N = 1: Sobol points, because make_problem
    normalises y by a zero standard deviation there), the draws of `seed`, V = 10 x unit normal from default_rng(V_SEED).
    With |V| ~ 10 the paths reach |f| ~ 300, where ONE ulp of f is already 0.05 of bound()."""
    from bayesian_optimisation_amd.synthetic import ard_length_scales, make_problem, sobol_points

    if N == 1:
        X, Xs, ls = sobol_points(0, 1, d), sobol_points(1, M, d), ard_length_scales(d)
    else:
        X, _, Xs, ls = make_problem(N, M, d)
    omega, phase, W, _ = draws(d, F, S, N, seed)
    V = 10.0 * np.random.default_rng(V_SEED).standard_normal((S, N))
    return X, Xs, ls, omega, phase, W, V


@functools.lru_cache(maxsize=None)
def kernel_reference(case):
    """The inputs of kernel_case(*case) with the long-double paths and the bound, with V and without: computed once and
    shared by the tests that need them (callers must not write to the arrays)."""
    N, M, d, F, S = case
    X, Xs, ls, omega, phase, W, V = kernel_case(*case)
    return dict(X=X, Xs=Xs, ls=ls, omega=omega, phase=phase, W=W, V=V,
                f=paths(Xs, X, ls, omega, phase, W, V, xp=np.longdouble), tol=bound(Xs, ls, omega, phase, W, V, d),
                f_prior=paths(Xs, X, ls, omega, phase, W, None, xp=np.longdouble),
                tol_prior=bound(Xs, ls, omega, phase, W, None, d))
