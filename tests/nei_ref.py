"""NumPy restatement of noisy expected improvement as the GPU computes it (csrc/nei.hip, include/gpbo.h), shared by the NEI
tests.  Not in the reference, which has no EI.  Everything in the units of the model; rho = jitter1 + jitter2, 0 < delta <= rho:

    K~  = k(X,X) with the diagonal (1 + jitter1) + jitter2 = L L^T,   U  = L^-T   (U U^T = K~^-1)
    K0d = k(X,X) with the diagonal 1 + delta             = L0 L0^T,  U0 = L0^-T  (the noise-free twin)
    B_s = U0 z_s,  g_s = K0d B_s,  r_s = y - g_s - sqrt(rho - delta) e_s,  A_s = B_s + U (U^T r_s),  F_s = K0d A_s
    best_s = min_i F_s[i];   mu_s(x) = k(x) . A_s;   sigma_0(x) = sqrt(|(1 + delta) - |U0^T k(x)|^2|)
    NEI(x) = (1 / S) sum_s EI(mu_s(x), sigma_0(x); best_s, xi), summed in index order

`dtype=np.longdouble` runs the same formulas with a column-by-column Cholesky and triangular inverse (as qei_ref.py does); the
float64 form uses LAPACK.  EI itself is evaluated in float64 in both (math.erfc has no long-double form; its inputs are rounded).
"""
import math

import numpy as np
import scipy.linalg as sla

import matern_ref as MR

LD = np.longdouble
HAVE_LONGDOUBLE = bool(np.finfo(LD).eps < 2e-19)
INFORMATIVE = 1e-6      # a value below this compares as 0 == 0
MAX_LEFT_OUT = 0.4      # at most this fraction of a case's candidates may be below it
JITTERS = (1e-4, 1e-6)  # the reference's frozen model


def _cholesky(A):
    n = A.shape[0]
    L = np.zeros_like(A)
    for j in range(n):
        c = A[j:, j] - L[j:, :j] @ L[j, :j]
        if not c[0] > 0:
            raise ValueError(f"pivot {j} is not positive: {float(c[0])!r}")
        L[j:, j] = c / np.sqrt(c[0])
    return L


def _inv_lower(L):
    """inv(L) of a lower triangular matrix, column by column (forward substitution on the identity)."""
    n = L.shape[0]
    Y = np.zeros_like(L)
    eye = np.eye(n, dtype=L.dtype)
    for i in range(n):
        Y[i] = (eye[i] - L[i, :i] @ Y[:i]) / L[i, i]
    return Y


def _factor(K):
    """U = L^-T of K = L L^T in K's dtype."""
    if K.dtype == np.float64:
        L = np.linalg.cholesky(K)
        return sla.solve_triangular(L, np.eye(len(K)), lower=True).T
    return _inv_lower(_cholesky(K)).T


def noise_sd(jitters, delta):
    """sqrt(rho - delta) as the callers of gpbo_nei_fantasies_f64 round it (float64)."""
    return float(np.sqrt(max((float(jitters[0]) + float(jitters[1])) - float(delta), 0.0)))


def fantasies(X, y, ls, Z, E, jitters=JITTERS, delta=1e-6, family="se", dtype=np.float64):
    """dict(A [S x N], F [S x N], best [S], U0, U, K0d, K) in `dtype`."""
    t = np.dtype(dtype).type
    y = np.asarray(y, dtype=np.float64).reshape(-1).astype(dtype)
    Z, E = np.asarray(Z, dtype=np.float64).astype(dtype), np.asarray(E, dtype=np.float64).astype(dtype)
    K = MR.gram(X, ls, family, jitters[0], jitters[1], dtype=dtype)
    K0d = MR.gram(X, ls, family, delta, 0.0, dtype=dtype)
    U, U0 = _factor(K), _factor(K0d)
    B = Z @ U0.T
    R = (y[None, :] - B @ K0d) - t(noise_sd(jitters, delta)) * E
    A = B + (R @ U) @ U.T
    F = A @ K0d
    return dict(A=A, F=F, best=F.min(axis=1), U0=U0, U=U, K0d=K0d, K=K)


def ei(mu, sigma, f_best, xi=0.0):
    """gpbo_acquisition(GPBO_ACQ_EI, ...) element by element in float64 (csrc/gpbo_internal.h)."""
    mu, sigma = np.asarray(mu, dtype=np.float64), np.asarray(sigma, dtype=np.float64)
    imp = float(f_best) - mu - float(xi)
    out = np.empty_like(mu)
    pos = sigma > 0.0
    with np.errstate(divide="ignore", invalid="ignore"):
        z = imp / sigma
        cdf = 0.5 * np.vectorize(math.erfc, otypes=[np.float64])(-z[pos] * 0.70710678118654752440) if pos.any() else np.empty(0)
        out[pos] = imp[pos] * cdf + sigma[pos] * (np.exp(-0.5 * z[pos] * z[pos]) * 0.39894228040143267794)
    out[~pos] = np.where(sigma[~pos] == 0.0, np.maximum(imp[~pos], 0.0), sigma[~pos])
    return out


def score(X, Xs, ls, fan, best=None, xi=0.0, delta=1e-6, family="se", dtype=np.float64):
    """dict(mu [S x M], sigma [M], nei [M], best [S]) as float64 arrays from fantasies() of the same dtype."""
    t = np.dtype(dtype).type
    Ks = MR.kernel(Xs, X, ls, family, dtype=dtype)          # [M x N]
    mu = (fan["A"] @ Ks.T).astype(np.float64)
    V = Ks @ fan["U0"]
    sigma = np.sqrt(np.abs((t(1) + t(delta)) - np.sum(V * V, axis=1))).astype(np.float64)
    best = np.asarray(fan["best"] if best is None else best, dtype=np.float64).reshape(-1)
    acc = np.zeros(len(Xs))
    for s in range(len(mu)):                                 # index order
        acc = acc + ei(mu[s], sigma, best[s], xi)
    return dict(mu=mu, sigma=sigma, nei=acc / len(mu), best=best)


def argmax_first(v):
    """First index of the maximum over the entries that are not NaN."""
    v = np.asarray(v, dtype=np.float64)
    return int(np.flatnonzero(v == np.nanmax(v))[0])


def top2_gap(v):
    s = np.sort(np.asarray(v, dtype=np.float64)[~np.isnan(v)])
    return float(s[-1] - s[-2]) if s.size > 1 else float("inf")


def quantile_best(fan, q=0.7):
    """The incumbents of the value tests: the q-quantile of each fantasy over the observations (float64)."""
    return np.quantile(np.asarray(fan["F"], dtype=np.float64), q, axis=1)


def informative(nei):
    """(mask of the candidates whose reference value is >= INFORMATIVE, fraction left out)."""
    nei = np.asarray(nei, dtype=np.float64)
    keep = nei >= INFORMATIVE
    return keep, 1.0 - float(np.mean(keep))


def candidates(seed, M, d):
    return np.random.default_rng(1000 + seed).uniform(0.0, 1.0, (M, d))


# ---- the value cases of tests/test_gpu_nei.py; tests/test_nei_ref_cpu.py asserts that each of them is informative -------------
# name: (problem seed, N, d, S, M, (jitter1, jitter2), family).  Every edge once: one observation, fewer than a k step of four,
# one short of / exactly / one past the padding granule of 128, three granules; d = 1 and the largest unrolled d; one fantasy,
# fewer than a column tile of 16, exactly one, one more, all four tiles; fewer candidates than a row tile, no multiple of the
# 256-candidate workgroup, more than one chunk of 512 with a ragged tail.
CASES = {
    "n1_d1_s1_m8": (1, 1, 1, 1, 8, (0.09, 0.0), "se"),
    "n5_d2_s3_m1000": (2, 5, 2, 3, 1000, (0.09, 0.0), "se"),
    "n40_d2_s16_m1537": (1, 40, 2, 16, 1537, (0.09, 0.0), "se"),
    "n40_d2_s16_m1000_seed2": (2, 40, 2, 16, 1000, (0.09, 0.0), "se"),
    "n40_d2_s17_m1000_seed3": (3, 40, 2, 17, 1000, (0.09, 0.0), "se"),
    "n127_d8_s64_m1000": (4, 127, 8, 64, 1000, (0.01, 0.0), "se"),
    "n128_d16_s16_m1537": (5, 128, 16, 16, 1537, (0.09, 0.0), "se"),
    "n129_d2_s17_m1537": (6, 129, 2, 17, 1537, (0.09, 0.0), "se"),
    "n129_d2_s3_m1000_reference_jitters": (7, 129, 2, 3, 1000, JITTERS, "se"),
    "n300_d8_s64_m1537": (8, 300, 8, 64, 1537, (0.09, 0.0), "se"),
    "n129_d1_s16_m8": (9, 129, 1, 16, 8, (0.09, 0.0), "se"),
    "n129_d2_s16_m1000_matern32": (10, 129, 2, 16, 1000, (0.09, 0.0), "matern32"),
    "n127_d8_s17_m1000_matern52": (11, 127, 8, 17, 1000, (0.09, 0.0), "matern52"),
}
DRAW_SEED = 0


def case_problem(name):
    """(X, y, ls, Xs, Z, E, jitters, family, S) of a value case.  The draws are nei_draws(N, S, DRAW_SEED)'s."""
    from ard_fit_ref import gp_problem
    from bayesian_optimisation_amd.nei import nei_draws

    seed, N, d, S, M, jitters, family = CASES[name]
    X, y = gp_problem(seed, N, d, noise=0.3)
    ls = np.geomspace(0.3, 1.0, d) if d > 1 else np.array([0.3])
    Z, E = nei_draws(N, S, DRAW_SEED)
    return X, y, ls, candidates(seed, M, d), Z, E, jitters, family, S


_case_cache = {}


def case_reference(name, longdouble=False):
    """The float64 restatement of a value case, computed once per process and shared by the tests (treat as read-only):
    dict(problem=..., fan=fantasies(), best=the 0.7-quantiles, score=score() with them); longdouble=True adds fan_ld."""
    if name not in _case_cache:
        X, y, ls, Xs, Z, E, jitters, family, S = case_problem(name)
        fan = fantasies(X, y, ls, Z, E, jitters, 1e-6, family)
        best = quantile_best(fan)
        _case_cache[name] = dict(problem=(X, y, ls, Xs, Z, E, jitters, family, S), fan=fan, best=best,
                                 score=score(X, Xs, ls, fan, best, 0.0, 1e-6, family))
    ref = _case_cache[name]
    if longdouble and "fan_ld" not in ref:
        X, y, ls, Xs, Z, E, jitters, family, S = ref["problem"]
        ref["fan_ld"] = fantasies(X, y, ls, Z, E, jitters, 1e-6, family, dtype=LD)
    return ref
