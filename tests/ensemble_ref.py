"""NumPy restatement of the ensemble scoring that the GPU computes (csrc/ensemble.hip), shared by the ard="marginal" tests, and
the cases and error bounds those tests use.

A model is (ls [d], jitter1, jitter2, y_mean m, y_scale s, weight w): the GP of (y - m) / s with K = k(X,X) + diagonal
(1 + jitter1) + jitter2 (a fitted model: jitter1 = rho, jitter2 = 0).  Per model the posterior is taken by the Cholesky route
(matern_ref.posterior); with mu_y = m + s mu, sigma_y = s sigma and shift = sum_s w_s m_s the accumulation is, per candidate,
    acq += w acquisition(kind, mu_y, sigma_y, p0, p1),   dm += w (mu_y - shift),   dv += w (sigma_y^2 + (mu_y - shift)^2)
    mean = shift + dm,   var = max(dv - dm^2, 0),   sd = sqrt(var)
in model order, the acquisition parameters in the units of y."""
import numpy as np
from scipy.special import erfc

import matern_ref as MR

LCB, EI = "lcb", "ei"


def acquisition(kind, mu, sigma, p0, p1=0.0):
    """LCB: p0 sigma - mu.  EI for minimisation: imp = p0 - mu - p1, imp Phi(z) + sigma phi(z), max(imp, 0) at sigma = 0."""
    mu, sigma = np.asarray(mu, dtype=np.float64), np.asarray(sigma, dtype=np.float64)
    if kind == LCB:
        return p0 * sigma - mu
    imp = p0 - mu - p1
    with np.errstate(divide="ignore", invalid="ignore"):
        z = imp / sigma
        val = imp * 0.5 * erfc(-z * 0.70710678118654752440) + sigma * np.exp(-0.5 * z * z) * 0.39894228040143267794
    return np.where(sigma > 0.0, val, np.where(sigma == 0.0, np.maximum(imp, 0.0), sigma))


def model_posteriors(X, y, Xs, models, family="se"):
    """[(mu_y [M], sigma_y [M])] per model, in the units of y."""
    y = np.asarray(y, dtype=np.float64).reshape(-1)
    Xs = np.asarray(Xs, dtype=np.float64)
    ok = np.all(np.isfinite(Xs), axis=1)   # a candidate with a NaN coordinate: NaN mean and sigma (SciPy refuses such rows)
    out = []
    for ls, j1, j2, m, s, _ in models:
        mu, sigma = np.full(len(Xs), np.nan), np.full(len(Xs), np.nan)
        mu[ok], sigma[ok] = MR.posterior(X, (y - m) / s, Xs[ok], ls, family, j1, j2)
        out.append((m + s * mu, s * sigma))
    return out


def fold(posteriors, models, kind, p0, p1=0.0):
    """dict(acq, mean, sd, var, best_idx, best_val, shift) of the accumulation over per-model (mu_y, sigma_y)."""
    w = np.array([mod[5] for mod in models], dtype=np.float64)
    shift = float(np.sum(w * np.array([mod[3] for mod in models], dtype=np.float64)))
    acq = dm = dv = 0.0
    for (mu_y, sigma_y), ws in zip(posteriors, w):
        d = mu_y - shift
        acq = acq + ws * acquisition(kind, mu_y, sigma_y, p0, p1)
        dm = dm + ws * d
        dv = dv + ws * (sigma_y * sigma_y + d * d)
    var = np.maximum(dv - dm * dm, 0.0)
    ok = ~np.isnan(acq)
    best = int(np.flatnonzero(ok & (acq == np.max(acq[ok])))[0]) if np.any(ok) else -1
    return dict(acq=acq, mean=shift + dm, sd=np.sqrt(var), var=var, best_idx=best,
                best_val=float(acq[best]) if best >= 0 else -np.inf, shift=shift)


def score(X, y, Xs, models, kind, p0, p1=0.0, family="se"):
    return fold(model_posteriors(X, y, Xs, models, family), models, kind, p0, p1)


# ---- error bounds of the GPU against this restatement, propagated from the per-model bounds the suite already holds
# (|mu - ref| <= 1e-10 max(1, |y~|_inf), |sigma - ref| <= 1e-9 in model units; tests/test_gpu_parity.py) -----------------------
MU_TOL, SIGMA_TOL = 1e-10, 1e-9


def _ynorm(y, mod):
    return max(1.0, float(np.max(np.abs((np.asarray(y, dtype=np.float64).reshape(-1) - mod[3]) / mod[4]))))


def acq_bound(y, models, kind, explore=None):
    """B = sum_s w_s s_s (e 1e-9 + 1e-10 max(1, |y~_s|_inf)): e = explore for LCB; e = 1 for EI, which is 1-Lipschitz in mu with a
    sigma-slope phi <= 0.4."""
    e = float(explore) if kind == LCB else 1.0
    return float(sum(mod[5] * mod[4] * (e * SIGMA_TOL + MU_TOL * _ynorm(y, mod)) for mod in models))


def mean_bound(y, models):
    return float(sum(mod[5] * mod[4] * MU_TOL * _ynorm(y, mod) for mod in models))


def var_bound(y, models, posteriors, shift):
    """2 sum_s w_s (2 sigma_y s_s 1e-9 + 2 |mu_y - shift| s_s 1e-10 max(1, |y~_s|_inf)) per candidate [M]."""
    b = 0.0
    for (mu_y, sigma_y), mod in zip(posteriors, models):
        b = b + mod[5] * (2.0 * sigma_y * mod[4] * SIGMA_TOL + 2.0 * np.abs(mu_y - shift) * mod[4] * MU_TOL * _ynorm(y, mod))
    return 2.0 * b


# ---- the cases of tests/test_gpu_ensemble.py; tests/test_ensemble_ref_cpu.py checks their premises on the CPU ----------------
EXPLORE, EI_XI = 4.0, 0.01
# (N, M, d, family): every N of {1, 7, 128, 129, 300}, every M of {1, 511, 513, 1000}, every d of {1, 3, 8, 16}, all three
# families at N = 129
CASES = [(1, 1, 1, "se"), (7, 511, 3, "se"), (128, 513, 8, "se"), (129, 1000, 16, "se"), (300, 1000, 3, "se"),
         (129, 513, 3, "matern32"), (129, 511, 8, "matern52"), (300, 1, 1, "se")]


def case_problem(N, M, d, seed=0):
    """(X, y, Xs, five fitted models): uniform points, a smooth y with an offset and a scale of its own, and five distinct
    (ls, rho >= 1e-4, m, s) around what a fit would give, with equal weights."""
    rng = np.random.default_rng(1000 * seed + 17 * N + d)
    X = rng.uniform(0.0, 1.0, (N, d))
    Xs = rng.uniform(0.0, 1.0, (M, d))
    f = np.sum(np.sin(3.0 * X + np.arange(d)), axis=1) / np.sqrt(d)
    y = 40.0 + 7.0 * (f + 0.05 * rng.standard_normal(N))
    m0, s0 = float(np.mean(y)), (float(np.std(y)) if N > 1 else 1.0)
    base = np.geomspace(0.4, 1.5, d)
    rhos = np.geomspace(1e-4, 3e-2, 5)
    models = [(base * f_ls, float(rhos[s]), 0.0, m0 + 0.1 * s0 * (s - 2), s0 * f_s, 0.2)
              for s, (f_ls, f_s) in enumerate(zip((0.7, 0.85, 1.0, 1.2, 1.5), (0.8, 1.3, 1.0, 0.9, 1.15)))]
    return X, y, Xs, models


def case_params(kind, y):
    """(p0, p1) of the case's acquisition in the units of y."""
    return (EXPLORE, 0.0) if kind == LCB else (float(np.min(y)), EI_XI)
