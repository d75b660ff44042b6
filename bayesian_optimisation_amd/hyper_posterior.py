"""Samples of the hyperparameter posterior: lockstep chains of coordinate-wise slice sampling (NumPy only).

Not in the reference, which scores every candidate under one length-scale choice (point_selector.py:104-163).  ard="marginal"
averages the acquisition over samples of the posterior of the hyperparameters instead (Snoek, Larochelle & Adams 2012); this
module draws them.

WHAT IS SAMPLED.  The variable is z = (log ls_1 ... log ls_d, log rho) inside the box [lower, upper] the ML-II fit searches.
The target density is exp(-L(z)) on that box, L the PROFILE likelihood the fit minimises - mean and signal variance at their
closed-form optima for each z, not integrated out - with a prior that is flat in z on the box (so log-uniform in the length
scales and the noise ratio) and zero outside it.  It is the profile-likelihood posterior of z, not the full Bayesian posterior of
all d + 3 hyperparameters.

THE METHOD.  C independent chains advance in lockstep, so that every evaluation of every chain at one step is ONE call
f_batch(Z [C x D]) -> L [C] (on the GPU: one launch of the wave-per-cell kernel, DeviceGP.nlml_hyper_cells).  A sweep visits the
D coordinates in a permutation drawn per sweep; each visit is one univariate slice-sampling update with stepping out and
shrinkage (Neal 2003, figs. 3 and 5) for all chains at once:
  * the slice level of a chain is L_cur - log(u), u uniform: a point is inside the slice when its L is finite and below the
    level; a value that is not finite (matrix not positive definite) counts as outside;
  * the interval of width `width` is placed at random around the current value and stepped out while its ends are inside the
    slice, at most MAX_STEP_OUT steps in all, divided at random between the two sides as Neal's limit requires; an end that
    reaches the box stops there (the density is zero beyond it);
  * a point drawn uniformly from the interval is accepted when inside the slice, otherwise the interval shrinks to it; a
    coordinate whose shrinkage has not ended after MAX_SHRINK trials keeps its value (counted in `kept`).
A chain that has finished a phase rides along with its current state - f_batch always receives C rows - and its value is
ignored.  Random numbers come from np.random.Generator(PCG64(seed)) and are always drawn for all C chains, so one seed and one
f_batch give one result; `min_margin`, the smallest |L - level| over every comparison that was made, says whether a
rounding-level difference between two implementations of f_batch could have changed a decision.
"""
from __future__ import annotations

from dataclasses import dataclass

import numpy as np

MAX_STEP_OUT = 8    # interval widenings per coordinate update, both sides together
MAX_SHRINK = 50     # shrinkage trials per coordinate update


@dataclass
class SampleResult:
    states: np.ndarray      # [C x D] final states z, inside the box
    values: np.ndarray      # [C] L at the final states (finite)
    n_batches: int          # calls of f_batch, the one at the start included
    min_margin: float       # smallest |L - slice level| over every comparison made (inf: none was made)
    kept: int               # coordinate updates that hit MAX_SHRINK and kept their value
    sweeps: int
    seed: int


def sample(f_batch, z0, lower, upper, sweeps: int, seed: int, width: float = 1.0) -> SampleResult:
    """`sweeps` sweeps of the chains started at z0 [C x D] (clipped into the box) under the density exp(-f_batch(z)) on
    lower <= z <= upper.  ValueError when the box is not finite and ordered, when width is not positive or when a chain starts
    where f_batch is not finite."""
    lo_b = np.asarray(lower, dtype=np.float64).reshape(-1)
    hi_b = np.asarray(upper, dtype=np.float64).reshape(-1)
    z = np.array(z0, dtype=np.float64, ndmin=2)
    C, D = z.shape
    if lo_b.size != D or hi_b.size != D:
        raise ValueError("z0, lower and upper must agree on the number of coordinates")
    if not (np.all(np.isfinite(lo_b)) and np.all(np.isfinite(hi_b)) and np.all(lo_b <= hi_b)):
        raise ValueError("the box must be finite with lower <= upper")
    width = float(width)
    if not (np.isfinite(width) and width > 0.0):
        raise ValueError(f"width must be positive and finite, got {width!r}")
    if int(sweeps) != sweeps or sweeps < 0:
        raise ValueError(f"sweeps must be a non-negative integer, got {sweeps!r}")
    z = np.minimum(np.maximum(z, lo_b), hi_b)
    rng = np.random.Generator(np.random.PCG64(int(seed)))
    stats = dict(batches=0, margin=np.inf, kept=0)

    def evaluate(Z):
        stats["batches"] += 1
        L = np.asarray(f_batch(Z), dtype=np.float64).reshape(-1)
        if L.size != C:
            raise ValueError(f"f_batch returned {L.size} values for {C} chains")
        return L

    def inside(L, level, active):
        """Which active chains' trial points are inside their slice; every comparison made is recorded in the margin."""
        fin = active & np.isfinite(L)
        if np.any(fin):
            stats["margin"] = min(stats["margin"], float(np.min(np.abs(L[fin] - level[fin]))))
        return fin & (L < level)

    Lcur = evaluate(z)
    if not np.all(np.isfinite(Lcur)):
        raise ValueError("the target is not finite at the start of every chain")
    for _ in range(int(sweeps)):
        for k in rng.permutation(D):
            x0 = z[:, k].copy()
            level = Lcur - np.log(rng.random(C))
            left = x0 - width * rng.random(C)
            right = left + width
            n_left = np.floor(MAX_STEP_OUT * rng.random(C)).astype(np.int64)   # Neal's J; the right side gets the rest
            n_right = MAX_STEP_OUT - 1 - n_left

            def step_out(end, budget, sign, bound):
                act = np.ones(C, dtype=bool)
                while True:
                    hit = act & (sign * (end - bound) >= 0.0)   # at or beyond the box: the end is the bound
                    end[hit] = bound
                    act &= ~hit & (budget > 0)
                    if not np.any(act):
                        return
                    Z = z.copy()
                    Z[act, k] = end[act]
                    ins = inside(evaluate(Z), level, act)
                    end[ins] += sign * width
                    budget[ins] -= 1
                    act &= ins

            step_out(left, n_left, -1.0, lo_b[k])
            step_out(right, n_right, +1.0, hi_b[k])
            left = np.maximum(left, lo_b[k])
            right = np.minimum(right, hi_b[k])
            act = np.ones(C, dtype=bool)
            for _trial in range(MAX_SHRINK):
                x1 = left + rng.random(C) * (right - left)
                Z = z.copy()
                Z[act, k] = x1[act]
                L = evaluate(Z)
                ins = inside(L, level, act)
                z[ins, k] = x1[ins]
                Lcur[ins] = L[ins]
                out = act & ~ins
                lower_side = out & (x1 < x0)
                left[lower_side] = x1[lower_side]
                upper_side = out & ~lower_side
                right[upper_side] = x1[upper_side]
                act = out
                if not np.any(act):
                    break
            stats["kept"] += int(np.sum(act))
    return SampleResult(states=z, values=Lcur, n_batches=stats["batches"], min_margin=float(stats["margin"]),
                        kept=stats["kept"], sweeps=int(sweeps), seed=int(seed))
