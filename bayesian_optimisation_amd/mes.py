"""Max-value entropy search: the sampling of the minimum's value and the parameter checks (NumPy only; both selector classes and
DeviceGP use it).

The kernels are in csrc/mes.hip; the formulas are stated in include/gpbo.h.  The library evaluates
log S(z) = sum_c log Phi((mu_c - z) / sigma_c) - the logarithm of Pr[m* > z] when the candidates are taken as independent - at
up to 64 levels per pass; everything here is arithmetic on those few numbers: the three levels z75 < z50 < z25 where S = 0.75, 0.5,
0.25 are bracketed, a Gumbel law is fitted to them (Wang & Jegelka 2017) and the minima m*_s are drawn from it.  The uniform draws are
default_rng(seed).random(S): one seed gives the same samples in DeviceGP, PointSelector, PointSelectorHost - on every rank of a
sharded call - and in the NumPy restatement of the tests.
"""
from __future__ import annotations

import numpy as np

from . import _lib
from .thompson import _integer

PROBS = (0.75, 0.5, 0.25)           # the survival levels of the fit, in the order of the quartiles returned
LO_SIGMAS = 10.0                    # lower bracket min_c(mu_c - 10 sigma_c): S >= 1 - M 7.7e-24
HI_SIGMAS = 0.6744897501960817      # upper bracket min_c(mu_c + 0.6745 sigma_c): one factor of S is Phi(-0.6745) = 0.25 there
LEVELS = 21
ROUNDS = 4
Y_STAR_RULES = ("gumbel", "thompson")


def mes_params(n_samples, seed, cap="observed") -> tuple:
    """(n_samples, seed, cap) as the C ABI and mes_uniforms take them; refuses what they refuse.  cap: "observed" (the smallest
    observation: the caller resolves it), None (no cap) or a finite number."""
    S, seed = _integer("n_samples", n_samples), _integer("seed", seed)
    if not 1 <= S <= _lib.MES_MAX_S:
        raise ValueError(f"n_samples must be in [1, {_lib.MES_MAX_S}], got {S}")
    if seed < 0:
        raise ValueError(f"seed must be non-negative, got {seed}")
    if cap is None or (isinstance(cap, str) and cap == "observed"):
        return S, seed, cap
    if isinstance(cap, (str, bool, np.bool_)) or not np.isscalar(cap) or not np.isfinite(float(cap)):
        raise ValueError(f"cap must be 'observed', None or a finite number, got {cap!r}")
    return S, seed, float(cap)


def mes_y_star(y_star, S: int):
    """The y_star argument of the MES calls: one of Y_STAR_RULES, or S finite values as a contiguous fp64 array (used verbatim)."""
    if isinstance(y_star, str):
        if y_star not in Y_STAR_RULES:
            raise ValueError(f"y_star must be one of {Y_STAR_RULES} or an array of n_samples values, got {y_star!r}")
        return y_star
    v = np.ascontiguousarray(np.asarray(y_star, dtype=np.float64).reshape(-1))
    if v.size != S or not np.all(np.isfinite(v)):
        raise ValueError(f"y_star must hold n_samples = {S} finite values")
    return v


def mes_uniforms(S: int, seed: int) -> np.ndarray:
    """The S uniform draws of the Gumbel samples, an exact 0 replaced by the next float (ln(-ln 0) is not finite)."""
    u = np.random.default_rng(seed).random(S)
    u[u == 0.0] = np.nextafter(0.0, 1.0)
    return u


def gumbel_quartiles(log_survival, lo: float, hi: float, levels: int = LEVELS, rounds: int = ROUNDS) -> tuple:
    """((z75, z50, z25), NaN count): the levels where S = 0.75, 0.5, 0.25.  log_survival: z [Q] -> (log S [Q], NaN count), log S
    decreasing in z; [lo, hi] must hold all three (S(lo) >= 0.75, S(hi) <= 0.25).  Each of `rounds` rounds is ONE call with
    3 x levels levels - `levels` evenly spaced in each quartile's bracket - after which the bracket is [the last level with
    log S >= log p, the next level]; the last round is interpolated linearly in log S."""
    lo, hi = float(lo), float(hi)
    if not (np.isfinite(lo) and np.isfinite(hi) and lo <= hi):
        raise ValueError(f"the brackets of the minimum's value must be finite with lo <= hi, got [{lo!r}, {hi!r}]")
    L = int(levels)
    logp = np.log(np.asarray(PROBS))
    br = np.tile(np.array([lo, hi]), (len(PROBS), 1))
    out, nan_count = np.empty(len(PROBS)), 0
    for r in range(int(rounds)):
        z = np.concatenate([np.linspace(a, b, L) for a, b in br])
        ls, n = log_survival(z)
        ls = np.asarray(ls, dtype=np.float64).reshape(len(PROBS), L)
        if r == 0:
            nan_count = int(n)
        for j in range(len(PROBS)):
            zj = z[j * L: (j + 1) * L]
            above = np.flatnonzero(ls[j] >= logp[j])
            k = min(int(above[-1]) if above.size else 0, L - 2)
            br[j] = zj[k], zj[k + 1]
            with np.errstate(invalid="ignore"):
                d = ls[j, k + 1] - ls[j, k]   # (-inf: a candidate with sigma = 0 sits on the next level; NaN: on both)
            t = (logp[j] - ls[j, k]) / d if d < 0.0 else 0.0
            out[j] = zj[k] + min(max(t, 0.0), 1.0) * (zj[k + 1] - zj[k])
    return out, nan_count


def sample_minima(quartiles, u, cap=None) -> np.ndarray:
    """m*_s [S] from the Gumbel law through the quartiles (z75, z50, z25) of the minimum: with w_p = -z_p,
    b = (w25 - w75) / (ln ln(4/3) - ln ln 4), a = w50 + b ln ln 2, m*_s = -(a - b ln(-ln u_s)).  z75 == z25: every sample is z50.
    cap (a number or None): m*_s <- min(m*_s, cap) - the minimum over the candidates is not above an observed value."""
    z75, z50, z25 = (float(v) for v in quartiles)
    u = np.asarray(u, dtype=np.float64).reshape(-1)
    if z75 == z25:
        m = np.full(u.shape, z50)
    else:
        w75, w50, w25 = -z75, -z50, -z25
        b = (w25 - w75) / (np.log(np.log(4.0 / 3.0)) - np.log(np.log(4.0)))
        a = w50 + b * np.log(np.log(2.0))
        m = -(a - b * np.log(-np.log(u)))
    return m if cap is None else np.minimum(m, float(cap))
