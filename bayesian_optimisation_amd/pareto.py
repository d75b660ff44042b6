"""Two objectives, both minimised: the Pareto front, the reference point, the dominated hypervolume and the parameter checks of
expected hypervolume improvement (NumPy only; both selector classes and DeviceGP use it).

The kernel is in csrc/ehvi.hip; the formulas are stated in include/gpbo.h.  A front is a float64 [P x 2] whose rows
(a_i, c_i) are strictly ascending in objective 1 and strictly descending in objective 2; the reference point r bounds the region
whose dominated area is measured, and every front point lies strictly below it in both coordinates.
"""
from __future__ import annotations

import numpy as np

from . import _lib

NADIR_MARGIN = 0.1   # reference_point("nadir"): the worst observation plus this share of the observed range, per objective


def _pairs(Y, name: str = "Y") -> np.ndarray:
    Y = np.asarray(Y, dtype=np.float64)
    if Y.size == 0:
        return np.empty((0, 2))
    if Y.ndim != 2 or Y.shape[1] != 2:
        raise ValueError(f"{name} must hold one row of two objective values per point, got shape {Y.shape}")
    return Y


def _ref_pair(ref) -> tuple:
    r = np.asarray(ref, dtype=np.float64).reshape(-1) if not isinstance(ref, str) else None
    if r is None or r.size != 2 or not np.all(np.isfinite(r)):
        raise ValueError(f"ref must be two finite numbers or 'nadir', got {ref!r}")
    return float(r[0]), float(r[1])


def pareto_front(Y, ref=None) -> np.ndarray:
    """The non-dominated rows of Y [n x 2] for minimisation, sorted: strictly ascending in column 0, strictly descending in
    column 1.  Rows holding a NaN or an infinity are dropped, a duplicate row is kept once, a row equal to another in one
    objective and worse in the other is dominated; with ref, rows not strictly below it in both objectives are dropped."""
    Y = _pairs(Y)
    keep = np.all(np.isfinite(Y), axis=1)
    if ref is not None:
        r = _ref_pair(ref)
        with np.errstate(invalid="ignore"):
            keep &= (Y[:, 0] < r[0]) & (Y[:, 1] < r[1])
    Y = Y[keep]
    Y = Y[np.lexsort((Y[:, 1], Y[:, 0]))]   # by objective 1, ties by objective 2
    out, low = [], np.inf
    for a, c in Y:
        if c < low:
            out.append((a, c))
            low = c
    return np.ascontiguousarray(np.array(out, dtype=np.float64).reshape(-1, 2))


def reference_point(Y, ref="nadir") -> tuple:
    """(r1, r2): ref itself when it is two finite numbers; "nadir": per objective the worst (largest) finite observation of Y plus
    NADIR_MARGIN of the observed range.  A zero range (or no finite row) gives no scale: ValueError, pass numbers."""
    if not (isinstance(ref, str) and ref == "nadir"):
        return _ref_pair(ref)
    Y = _pairs(Y)
    Y = Y[np.all(np.isfinite(Y), axis=1)]
    if Y.shape[0] == 0:
        raise ValueError("ref='nadir' needs at least one finite observation of both objectives: pass ref as two numbers")
    lo, hi = Y.min(axis=0), Y.max(axis=0)
    if not np.all(hi > lo):
        raise ValueError("ref='nadir' needs a non-zero observed range in both objectives (it sets the margin): pass ref as two "
                         "numbers")
    r = hi + NADIR_MARGIN * (hi - lo)
    return float(r[0]), float(r[1])


def check_front(front, ref) -> tuple:
    """(front as a contiguous fp64 [P x 2], (r1, r2)) as the C ABI takes them; refuses what gpbo_ehvi_acq_f64 refuses."""
    r = _ref_pair(ref)
    F = np.ascontiguousarray(_pairs([] if front is None else front, "front"))
    P = int(F.shape[0])
    if P > _lib.EHVI_MAX_P:
        raise ValueError(f"at most {_lib.EHVI_MAX_P} front points per call, got {P}")
    if not np.all(np.isfinite(F)):
        raise ValueError("every front value must be finite")
    if not (np.all(F[:, 0] < r[0]) and np.all(F[:, 1] < r[1])):
        raise ValueError("every front point must lie strictly below ref in both objectives (pareto_front(Y, ref) drops the others)")
    if P > 1 and not (np.all(np.diff(F[:, 0]) > 0) and np.all(np.diff(F[:, 1]) < 0)):
        raise ValueError("front must be strictly ascending in objective 1 and strictly descending in objective 2 "
                         "(pareto_front() returns that form)")
    return F, r


def hypervolume(front, ref) -> float:
    """The area below ref that the points of `front` dominate (any [n x 2]; its Pareto front below ref is taken first)."""
    r = _ref_pair(ref)
    F = pareto_front(front, r)
    if F.shape[0] == 0:
        return 0.0
    right = np.append(F[1:, 0], r[0])
    return float(np.sum((right - F[:, 0]) * (r[1] - F[:, 1])))


def _same_bits(a, b) -> bool:
    a, b = np.ascontiguousarray(a, dtype=np.float64), np.ascontiguousarray(b, dtype=np.float64)
    return a.shape == b.shape and a.tobytes() == b.tobytes()


def observed_pairs(points1, values1, points2, values2) -> np.ndarray:
    """[N x 2]: observation i of objective 1 beside observation i of objective 2.  The pairing takes observation i of each as
    one evaluation, so both must hold the same points, bit for bit: ValueError otherwise (pass front and ref explicitly then)."""
    y1, y2 = (np.asarray(v, dtype=np.float64).reshape(-1) for v in (values1, values2))
    if y1.size != y2.size or not _same_bits(np.asarray(points1, dtype=np.float64).reshape(y1.size, -1),
                                            np.asarray(points2, dtype=np.float64).reshape(y2.size, -1)):
        raise ValueError("the observed front needs the same measured points in both objectives, bit for bit (observation i of "
                         "each is taken as one evaluation): pass front and ref explicitly instead")
    return np.stack([y1, y2], axis=1)
