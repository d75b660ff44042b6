"""Thompson sampling by pathwise posterior samples: the random draws and the host-side selection rule.

NumPy only (host_binding.py uses it without PyTorch).  The kernels are in csrc/thompson.hip; the formulas are
stated in include/gpbo.h.  The random draws are INPUTS of the C ABI, so one seed gives the same sample paths in DeviceGP,
PointSelector, PointSelectorHost and the NumPy restatement of the tests.
"""
from __future__ import annotations

import numpy as np

from . import _lib


def thompson_draws(d: int, F: int, S: int, N: int, seed: int):
    """(omega [F x d], phase [F], W [S x F], E [S x N]) of S sample paths with F random Fourier features over N observations
    of d features.  THE ORDER OF THESE FOUR CALLS IS PART OF THE CONTRACT.  Column n of E belongs to observation n in the
    CALLER's order (DeviceGP permutes the columns when the surrogate was factorised in another order)."""
    rng = np.random.default_rng(seed)
    omega = rng.standard_normal((F, d))      # unit normal; the kernel divides by 2 pi ls_k
    phase = rng.uniform(0.0, 1.0, F)         # turns
    W = rng.standard_normal((S, F))
    E = rng.standard_normal((S, N))
    return omega, phase, W, E


def _integer(name: str, v) -> int:
    if isinstance(v, (bool, np.bool_)) or not isinstance(v, (int, np.integer)):
        raise ValueError(f"{name} must be an integer, got {v!r}")
    return int(v)


def path_params(n_paths, n_features, seed) -> tuple:
    """(n_paths, n_features, seed) as the C ABI and thompson_draws take them; refuses what they refuse."""
    n_paths, n_features, seed = _integer("n_paths", n_paths), _integer("n_features", n_features), _integer("seed", seed)
    if not 1 <= n_paths <= _lib.TS_MAX_PATHS:
        raise ValueError(f"n_paths must be in [1, {_lib.TS_MAX_PATHS}], got {n_paths}")
    if not 1 <= n_features <= _lib.TS_MAX_FEATURES:
        raise ValueError(f"n_features must be in [1, {_lib.TS_MAX_FEATURES}], got {n_features}")
    if seed < 0:
        raise ValueError(f"seed must be non-negative, got {seed}")
    return n_paths, n_features, seed


def select_params(q, n_paths, n_features, seed, M=None, d=None) -> tuple:
    """(q, n_paths, n_features, seed) of a select_thompson call; n_paths=None: min(TS_MAX_PATHS, 2 q)."""
    q = _integer("q", q)
    if not 1 <= q <= _lib.TS_MAX_PATHS:
        raise ValueError(f"q must be in [1, {_lib.TS_MAX_PATHS}], got {q}")
    if M is not None and q > int(M):
        raise ValueError(f"q = {q} exceeds the {int(M)} candidates")
    if d is not None and not 1 <= int(d) <= _lib.MAX_D:
        raise ValueError(f"Thompson sampling needs 1 <= d <= {_lib.MAX_D}, got d = {d}")
    if n_paths is None:
        n_paths = min(_lib.TS_MAX_PATHS, 2 * q)
    n_paths, n_features, seed = path_params(n_paths, n_features, seed)
    if n_paths < q:
        raise ValueError(f"n_paths = {n_paths} cannot give q = {q} points")
    return q, n_paths, n_features, seed


def first_distinct(indices, q: int) -> np.ndarray:
    """Positions (into `indices`, ascending) of the first q DISTINCT winners in path order; -1 entries (a path without a
    usable row) are skipped.  Fewer than q when the paths agree: the posterior has converged on those points."""
    seen, keep = set(), []
    for s, i in enumerate(np.asarray(indices, dtype=np.int64).reshape(-1).tolist()):
        if i < 0 or i in seen:
            continue
        seen.add(i)
        keep.append(s)
        if len(keep) == int(q):
            break
    return np.asarray(keep, dtype=np.int64)
