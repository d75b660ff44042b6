"""Noisy expected improvement: the random draws and the parameter checks (NumPy only; host_binding.py uses it without PyTorch).

The kernels are in csrc/nei.hip; the formulas are stated in include/gpbo.h.  The draws are INPUTS of the C ABI, so
one seed gives the same fantasies in DeviceGP, PointSelector, PointSelectorHost - on every rank of a sharded call - and in the
NumPy restatement of the tests.
"""
from __future__ import annotations

import numpy as np

from . import _lib
from .thompson import _integer

DELTA = 1e-6   # default nugget of the noise-free twin


def nei_draws(N: int, S: int, seed: int):
    """(Z [S x N], E [S x N]) unit normal: the prior draw and the noise draw of S fantasies over N observations.  THE ORDER OF
    THESE TWO CALLS IS PART OF THE CONTRACT.  Column n belongs to observation n in the CALLER's order."""
    rng = np.random.default_rng(seed)
    Z = rng.standard_normal((S, N))
    E = rng.standard_normal((S, N))
    return Z, E


def nei_params(n_fantasies, seed, xi=0.0, delta=DELTA, rho=None) -> tuple:
    """(n_fantasies, seed, xi, delta) as the C ABI and nei_draws take them; refuses what they refuse.  rho: the diagonal term
    jitter1 + jitter2 of the surrogate the fantasies are drawn from (None: not known yet)."""
    S, seed = _integer("n_fantasies", n_fantasies), _integer("seed", seed)
    if not 1 <= S <= _lib.NEI_MAX_S:
        raise ValueError(f"n_fantasies must be in [1, {_lib.NEI_MAX_S}], got {S}")
    if seed < 0:
        raise ValueError(f"seed must be non-negative, got {seed}")
    xi, delta = float(xi), float(delta)
    if not np.isfinite(xi):
        raise ValueError(f"xi must be finite, got {xi!r}")
    if not (np.isfinite(delta) and delta > 0.0):
        raise ValueError(f"delta must be positive and finite, got {delta!r}")
    if rho is not None and delta > float(rho):
        raise ValueError(f"delta = {delta!r} exceeds jitter1 + jitter2 = {float(rho)!r} of the surrogate: the noise would have a "
                         "negative variance")
    return S, seed, xi, delta


def nei_best(best, S: int):
    """The incumbents given in the place of the fantasies' minima: None, or S finite values as a contiguous fp64 array."""
    if best is None:
        return None
    b = np.ascontiguousarray(np.asarray(best, dtype=np.float64).reshape(-1))
    if b.size != S or not np.all(np.isfinite(b)):
        raise ValueError(f"best must hold {S} finite values (one incumbent per fantasy)")
    return b
