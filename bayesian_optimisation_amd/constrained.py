"""Constrained acquisitions in log space: the parameter checks, the limits and the incumbent rule (NumPy only; both selector
classes and DeviceGP use it).

The kernel is in csrc/constrained.hip; the formulas are stated in include/gpbo.h.  A constraint is a black-box
quantity g_c(x) with a GP of its own and an upper limit u_c; "feasible" means g_c(x) <= u_c for every c.  The library returns
    value(x) = base(x) + sum_c log Phi((u_c - mu_c(x)) / sigma_c(x)),     base: "none" (0), "ei" (log EI), "pi" (log PI)
and everything here is arithmetic on a handful of numbers around that call.
"""
from __future__ import annotations

import numpy as np

from . import _lib

BASES = tuple(_lib.CONS_BASE_IDS)   # "none", "ei", "pi"


def _finite_number(name: str, v) -> float:
    if isinstance(v, (str, bool, np.bool_)) or not np.isscalar(v) or not np.isfinite(float(v)):
        raise ValueError(f"{name} must be a finite number, got {v!r}")
    return float(v)


def cons_limits(upper, n_constraints=None) -> np.ndarray:
    """The limits as a contiguous fp64 [C]: 0 to CONS_MAX_C finite values, one per constraint."""
    u = np.ascontiguousarray(np.asarray([] if upper is None else upper, dtype=np.float64).reshape(-1))
    if u.size > _lib.CONS_MAX_C:
        raise ValueError(f"at most {_lib.CONS_MAX_C} constraints per call, got {u.size}")
    if n_constraints is not None and u.size != int(n_constraints):
        raise ValueError(f"upper must hold one limit per constraint ({int(n_constraints)}), got {u.size}")
    if not np.all(np.isfinite(u)):
        raise ValueError("every limit must be finite (a two-sided band is two constraints: g <= u and -g <= -l)")
    return u


def cons_params(base, f_best, xi, C: int) -> tuple:
    """(base id, f_best, xi) as the C ABI takes them; refuses what gpbo_constrained_acq_f64 refuses.  Without a base f_best and
    xi are not read (0.0 goes in)."""
    if not isinstance(base, str) or base not in _lib.CONS_BASE_IDS:
        raise ValueError(f"base must be one of {BASES}, got {base!r}")
    if base == "none":
        if C < 1:
            raise ValueError("the probability of feasibility needs at least one constraint")
        return _lib.CONS_BASE_NONE, 0.0, 0.0
    return _lib.CONS_BASE_IDS[base], _finite_number("f_best", f_best), _finite_number("xi", xi)


def incumbent_rule(f_best):
    """The f_best argument of the selector calls: "feasible" (the rule below) or a finite number, in the units of y."""
    if isinstance(f_best, str):
        if f_best != "feasible":
            raise ValueError(f"f_best must be 'feasible' or a finite number, got {f_best!r}")
        return f_best
    return _finite_number("f_best", f_best)


def _same_bits(a, b) -> bool:
    a, b = np.ascontiguousarray(a, dtype=np.float64), np.ascontiguousarray(b, dtype=np.float64)
    return a.shape == b.shape and a.tobytes() == b.tobytes()


def feasible_incumbent(points, values, cons_points, cons_values, upper):
    """The smallest objective observation among the observations at which EVERY constraint's own observation is <= its limit, or
    None when no observation is feasible (the caller then maximises the probability of feasibility alone: Gelbart's rule).
    points [N x d], values [N]: the objective's observations; cons_points / cons_values: those of every constraint; upper [C], in
    the units of cons_values.  The rule pairs observation i of the objective with observation i of every constraint, so all must
    hold the same points, bit for bit: ValueError otherwise (pass f_best as a number then).  A NaN observation is not feasible."""
    y = np.asarray(values, dtype=np.float64).reshape(-1)
    u = cons_limits(upper, len(cons_values))
    ok = ~np.isnan(y)
    for c, (Xc, yc) in enumerate(zip(cons_points, cons_values)):
        yc = np.asarray(yc, dtype=np.float64).reshape(-1)
        if yc.size != y.size or not _same_bits(np.asarray(points, dtype=np.float64).reshape(y.size, -1),
                                               np.asarray(Xc, dtype=np.float64).reshape(yc.size, -1)):
            raise ValueError(f"f_best='feasible' needs the same measured points in the objective and in constraint {c}, bit for "
                             "bit (observation i of each is taken as one evaluation): pass f_best as a number instead")
        with np.errstate(invalid="ignore"):
            ok &= yc <= u[c]
    return float(np.min(y[ok])) if np.any(ok) else None
