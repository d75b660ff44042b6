"""ML-II fitting of the ARD length scales: projected L-BFGS in log(length scale) inside a box (NumPy only).

Not in the reference, which planned it (point_selector.py:30 `hyperparam_obj`, :33 `gradient_steps`) and searches a
grid instead (:104-163).  The objective is any function ls -> (value, gradient with respect to log ls); the package
drives it with the negative log marginal likelihood and its gradient from the GPU (gp_device.LikelihoodFits over
DeviceGP.nlml_and_grad or the host-pointer binding's, csrc/ard_grad.hip).  Working in log ls keeps the length scales positive and makes the box [lower, upper] a box in the
optimisation variable.

The method (deterministic for a deterministic objective):
  * variables at a bound whose gradient points out of the box are held fixed for the step (the active set);
  * the direction on the others is the L-BFGS two-loop product with the last `memory` curvature pairs, restricted to
    the free variables; steepest descent when the memory is empty or the product is not a descent direction;
  * the step follows the projected path clip(z + t d) with Armijo backtracking (t halves); a value that is NaN or inf
    counts as +inf, so the search backs away from regions where K is not positive definite;
  * stops when the projected gradient's inf-norm is <= gtol ("gtol"), when an accepted step lowers the value by no more
    than ftol relative ("ftol"), when no step along steepest descent is accepted ("line_search"), or after max_iter
    iterations ("max_iter").
"""
from __future__ import annotations

from dataclasses import asdict, dataclass, field

import numpy as np

ARMIJO_C1 = 1e-4


@dataclass
class FitResult:
    ls: np.ndarray                  # fitted length scales [d]
    nlml: float                     # objective at ls
    trace: list = field(default_factory=list)   # objective at every accepted iterate, the start first (non-increasing)
    n_eval: int = 0                 # objective evaluations, the start included
    n_iter: int = 0                 # accepted steps
    converged: bool = False         # stopped by gtol or ftol
    reason: str = ""                # "gtol" | "ftol" | "line_search" | "max_iter"
    pg_norm: float = float("nan")   # inf-norm of the projected gradient (in log ls) at ls

    def as_dict(self) -> dict:
        d = asdict(self)
        d["ls"] = np.asarray(self.ls).tolist()
        d["trace"] = [float(v) for v in self.trace]
        return d


def _project(z, lo, hi):
    return np.minimum(np.maximum(z, lo), hi)


def _direction(g, free, S, Y):
    """-H g on the free variables (L-BFGS two-loop recursion, pairs restricted to the free variables)."""
    q = np.where(free, g, 0.0)
    pairs = []
    for s, y in zip(S, Y):
        s_f, y_f = np.where(free, s, 0.0), np.where(free, y, 0.0)
        sy = float(s_f @ y_f)
        if sy > 0.0:
            pairs.append((s_f, y_f, 1.0 / sy))
    if not pairs:
        return -q
    a = []
    for s_f, y_f, rho in reversed(pairs):
        ai = rho * float(s_f @ q)
        q = q - ai * y_f
        a.append(ai)
    s_f, y_f, _ = pairs[-1]
    q = q * (float(s_f @ y_f) / float(y_f @ y_f))
    for (s_f, y_f, rho), ai in zip(pairs, reversed(a)):
        b = rho * float(y_f @ q)
        q = q + (ai - b) * s_f
    return -np.where(free, q, 0.0)


def fit_length_scales(objective, ls0, lower, upper, max_iter: int = 100, gtol: float = 1e-5, ftol: float = 1e-12,
                      memory: int = 10, max_backtrack: int = 40) -> FitResult:
    """Minimise objective(ls) -> (value, d value / d log ls) over lower <= ls <= upper from ls0 (clipped into the box).
    Raises numpy.linalg.LinAlgError when the value at the start is not finite."""
    lo = np.log(np.asarray(lower, dtype=np.float64).reshape(-1))
    hi = np.log(np.asarray(upper, dtype=np.float64).reshape(-1))
    z = np.log(np.asarray(ls0, dtype=np.float64).reshape(-1))
    if not (lo.shape == hi.shape == z.shape) or z.size < 1:
        raise ValueError("ls0, lower and upper must hold one value per feature")
    if not (np.all(np.isfinite(lo)) and np.all(np.isfinite(hi)) and np.all(lo <= hi)):
        raise ValueError("the box must satisfy 0 < lower <= upper < inf")
    z = _project(z, lo, hi)

    def evaluate(zz):
        f, g = objective(np.exp(zz))
        f = float(f)
        g = np.asarray(g, dtype=np.float64).reshape(-1)
        if not np.isfinite(f) or not np.all(np.isfinite(g)):
            return np.inf, g
        return f, g

    f, g = evaluate(z)
    if not np.isfinite(f):
        raise np.linalg.LinAlgError("the likelihood is not finite at the starting length scales "
                                    "(covariance matrix not positive definite)")
    res = FitResult(ls=np.exp(z), nlml=f, trace=[f], n_eval=1)
    S, Y = [], []
    reason = "max_iter"
    while res.n_iter < max_iter:
        pg = z - _project(z - g, lo, hi)
        if float(np.max(np.abs(pg))) <= gtol:
            reason = "gtol"
            break
        free = ~(((z <= lo) & (g > 0.0)) | ((z >= hi) & (g < 0.0)))
        d = _direction(g, free, S, Y)
        if not float(d @ g) < 0.0:
            S, Y = [], []
            d = -np.where(free, g, 0.0)
        # without curvature pairs the first trial moves no log length scale by more than 1
        t = 1.0 if S else min(1.0, 1.0 / max(float(np.max(np.abs(d))), 1e-300))
        accepted = False
        for _ in range(max_backtrack):
            zt = _project(z + t * d, lo, hi)
            if np.array_equal(zt, z):
                break
            ft, gt = evaluate(zt)
            res.n_eval += 1
            if ft <= f + ARMIJO_C1 * float(g @ (zt - z)):
                accepted = True
                break
            t *= 0.5
        if not accepted:
            if S:                      # the quasi-Newton model misled the search: start again from steepest descent
                S, Y = [], []
                continue
            reason = "line_search"
            break
        s, yv = zt - z, gt - g
        if float(s @ yv) > 1e-10 * float(np.linalg.norm(s) * np.linalg.norm(yv)):
            S.append(s)
            Y.append(yv)
            if len(S) > memory:
                S.pop(0)
                Y.pop(0)
        f_prev = f
        z, f, g = zt, ft, gt
        res.n_iter += 1
        res.trace.append(f)
        if f_prev - f <= ftol * max(abs(f_prev), abs(f), 1.0):
            reason = "ftol"
            break
    res.ls, res.nlml, res.reason = np.exp(z), f, reason
    res.pg_norm = float(np.max(np.abs(z - _project(z - g, lo, hi))))
    res.converged = reason in ("gtol", "ftol")
    return res


@dataclass
class HyperFitResult(FitResult):
    """fit_hyperparameters: the FitResult of the joint fit (ls: the d length scales; pg_norm: over all d + 1 variables) and
    the rest of the fitted model y ~ N(mean 1, scale^2 (K0(ls) + noise I))."""
    noise: float = float("nan")     # fitted noise-to-signal ratio rho
    mean: float = float("nan")      # profiled constant mean m at (ls, noise), in the units of y
    scale: float = float("nan")     # profiled signal standard deviation s at (ls, noise), in the units of y


def fit_hyperparameters(objective, ls0, ls_lower, ls_upper, noise0, noise_lower, noise_upper, **opts) -> HyperFitResult:
    """Minimise objective(ls, noise) -> (value, gradient [d + 1] with respect to (log ls, log noise), mean, scale^2) over
    ls_lower <= ls <= ls_upper and noise_lower <= noise <= noise_upper: fit_length_scales on the concatenated positive vector
    (ls, noise), same method, same options (**opts), same errors.  mean and scale^2 are whatever the objective reports at a
    point (the package: the closed-form profile values of csrc/hyper.hip); those of the final point are returned."""
    ls0 = np.asarray(ls0, dtype=np.float64).reshape(-1)
    d = ls0.size
    cat = lambda v, s: np.concatenate([np.asarray(v, dtype=np.float64).reshape(-1), [float(s)]])   # noqa: E731
    if np.asarray(ls_lower).size != d or np.asarray(ls_upper).size != d:
        raise ValueError("ls0, ls_lower and ls_upper must hold one value per feature")
    seen = {}

    def joint(v):
        f, g, mean, scale2 = objective(v[:d].copy(), float(v[d]))
        seen[v.tobytes()] = (float(mean), float(scale2))
        return f, g

    r = fit_length_scales(joint, cat(ls0, noise0), cat(ls_lower, noise_lower), cat(ls_upper, noise_upper), **opts)
    mean, scale2 = seen[np.asarray(r.ls, dtype=np.float64).tobytes()]   # the final point is one that was evaluated
    return HyperFitResult(ls=r.ls[:d].copy(), nlml=r.nlml, trace=r.trace, n_eval=r.n_eval, n_iter=r.n_iter,
                          converged=r.converged, reason=r.reason, pg_norm=r.pg_norm, noise=float(r.ls[d]), mean=mean,
                          scale=float(np.sqrt(scale2)))
