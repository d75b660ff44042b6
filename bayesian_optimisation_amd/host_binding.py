"""The drop-in class bound through the host-pointer C entry points only: NumPy + ctypes, no PyTorch.

This is the ctypes stub a maintainer of the reference would write against include/gpbo.h
(the gpbo_*_host_f64 entry points): the arrays the reference already holds
(/root/reference/select_parameters.py:149-153, 285-289) go in as host pointers, `mean_func`, `cov_func`,
`acq_func_eval` and the selected index come back.  Every call allocates and frees its device buffers inside the
library, which costs a few milliseconds per step against the tensor-resident `PointSelector`; the numbers are the
same (same kernels).  Not available here: candidate sharding over several GPUs, the incremental factorisation,
fp32 / int8 screening - those need the device-pointer API behind `PointSelector`.
`PointSelectorHost` is `PointSelector` with two methods of its own - update_surrogate() and _score_acq(), one
gpbo_select_next_host_kern_f64 call with the update's model.SurrogateModel - between the shared prologue, epilogue and
_finish; `_GridOnly` supplies the likelihoods to the shared search and fits (gp_device.LikelihoodFits).
A process that uses both this binding and the PyTorch-based classes must `import torch` before its first call here
(bringing PyTorch's GPU context up after this library has initialised HIP was seen to dead-lock now and then; the
PyTorch-based classes refuse that order with a clear error).
"""
from __future__ import annotations

import ctypes as C
from contextlib import contextmanager

import numpy as np

from . import _lib
from .gp_device import NAN_ACQUISITION, LikelihoodFits, acq_params, fantasy_params, refine_box, refine_params
from .model import JITTER_ASSEMBLY, JITTER_KERNEL, SurrogateModel, need_se
from .point_selector import PointSelector


def _f64(a):
    return np.ascontiguousarray(a, dtype=np.float64)


def _problem(X, y, ls, Xs=None):
    """(X, y, ls, N, d) - with candidates (X, y, ls, Xs, N, d, M) - as contiguous fp64 arrays: the one shape check of the
    binding, made before anything touches the device."""
    X, y = _f64(X), _f64(y).reshape(-1)
    ls = _f64(np.asarray(ls, dtype=np.float64).reshape(-1))
    Xs = None if Xs is None else _f64(Xs)
    ok = X.ndim == 2 and ls.size == X.shape[1] and y.size == X.shape[0]
    if not ok or (Xs is not None and (Xs.ndim != 2 or Xs.shape[1] != X.shape[1])):
        raise ValueError("shapes: X (N, d), y (N,), ls (d,), Xs (M, d)")
    return (X, y, ls, *X.shape) if Xs is None else (X, y, ls, Xs, *X.shape, Xs.shape[0])


class _Result:
    """The gpbo_result record and the info word a host entry writes, and their decoding."""

    def __init__(self):
        self.res = (C.c_int64 * 4)()
        self.info = C.c_int32(0)
        self.info_ptr = C.byref(self.info)

    def decode(self) -> dict:
        best_val = float(np.frombuffer(self.res, dtype=np.float64, count=1)[0])
        return dict(best_val=best_val, best_idx=int(self.res[1]), nan_count=int(self.res[2]), info=int(self.info.value))


def nlml_grid(X, y, ls_cells, jitter: float = JITTER_KERNEL, lib=None, likelihood: str = "reference") -> np.ndarray:
    """-log marginal likelihood of every row of ls_cells [G x d]  (point_selector.py:111-156): float32 with the
    reference's det underflow (likelihood="reference") or fp64 with log det from the factor ("logdet")."""
    if likelihood not in ("reference", "logdet"):
        raise ValueError(f"likelihood must be 'reference' or 'logdet', got {likelihood!r}")
    lib = lib or _lib.load()
    X, y = _f64(X), _f64(y).reshape(-1)
    N, d = X.shape
    cells = _f64(np.asarray(ls_cells, dtype=np.float64).reshape(-1, d))
    logdet = likelihood == "logdet"
    out = np.empty(len(cells), dtype=np.float64 if logdet else np.float32)
    _lib.note_hip_use()
    fn = lib.gpbo_nlml_grid_logdet_host_f64 if logdet else lib.gpbo_nlml_grid_host_f64
    _lib.call(fn, X, y, N, d, cells, len(cells), float(jitter), out)
    return out


def nlml_and_grad(X, y, ls, jitter: float = JITTER_KERNEL, lib=None, kernel: str = "se"):
    """(NLML, d NLML / d log ls [d]) of K = k(X,X) + jitter I on host arrays: gpbo_nlml_grad_host_kern_f64 (factorisation and
    gradient kernel in one call).  NaN in every output when K is not positive definite.  d <= 16.  kernel: "se", "matern32" or
    "matern52"."""
    kid = _lib.kernel_id(kernel)
    lib = lib or _lib.load()
    X, y, ls, N, d = _problem(X, y, ls)
    out = np.empty(1 + d)
    _lib.note_hip_use()
    _lib.call(lib.gpbo_nlml_grad_host_kern_f64, X, y, N, d, ls, kid, float(jitter), out)
    return float(out[0]), out[1:].copy()


def nlml_hyper(X, y, ls, noise: float, fit_mean: bool = True, fit_scale: bool = True, lib=None, kernel: str = "se"):
    """(L, dL / d(log ls, log noise) [d + 1], mean, scale^2) of y ~ N(mean 1, scale^2 (k(X,X) + noise I)) on host arrays:
    gpbo_nlml_hyper_host_f64 (factorisation and the kernels of csrc/hyper.hip in one call).  NaN in every output when the
    matrix is not positive definite or scale^2 is not positive.  d <= 16.  kernel: "se", "matern32" or "matern52"."""
    kid = _lib.kernel_id(kernel)
    lib = lib or _lib.load()
    X, y, ls, N, d = _problem(X, y, ls)
    noise = float(noise)
    if d > _lib.MAX_D or not (np.isfinite(noise) and noise > 0.0) or not np.all(ls > 0):
        raise ValueError(f"nlml_hyper needs d <= {_lib.MAX_D}, positive length scales and a positive finite noise")
    flags = (_lib.HYPER_MEAN if fit_mean else 0) | (_lib.HYPER_SCALE if fit_scale else 0)
    out = np.empty(4 + d)
    _lib.note_hip_use()
    _lib.call(lib.gpbo_nlml_hyper_host_kern_f64, X, y, N, d, ls, kid, float(noise), flags, out)
    return float(out[0]), out[1: 2 + d].copy(), float(out[2 + d]), float(out[3 + d])


def select_next(X, y, ls, Xs, acquisition: str = "lcb", explore: float = 4.0, f_best=None, xi: float = 0.0,
                dense: bool = True, want_cov_meas: bool = False, chunk: int = 0, lib=None,
                jitter1: float = JITTER_KERNEL, jitter2: float = JITTER_ASSEMBLY, diag_add=None, kernel: str = "se") -> dict:
    """One surrogate step on host arrays.  Returns dict(best_val, best_idx, nan_count, info, mu, sigma, acq, cov_meas).
    jitter1 / jitter2: the two diagonal terms of the factorised matrix (prior variance (1 + jitter1) + jitter2); diag_add:
    None for the reference's N == M rule (squared exponential only: a Matern kernel has no such quirk), or the value itself.
    kernel: "se", "matern32" or "matern52"; a Matern step always takes the plain pass."""
    kid = _lib.kernel_id(kernel)
    lib = lib or _lib.load()
    X, y, ls, Xs, N, d, M = _problem(X, y, ls, Xs)
    kind, p0, p1 = acq_params(acquisition, explore, f_best, xi)
    mu, sigma, acq = (np.empty(M) if dense else None for _ in range(3))
    cov = np.empty((N, N)) if want_cov_meas else None
    out = _Result()
    if diag_add is None:
        diag_add = SurrogateModel(kernel, jitter1, jitter2).diag_add(Xs.shape, X.shape)   # point_selector.py:173 shape quirk
    _lib.note_hip_use()
    _lib.call(lib.gpbo_select_next_host_kern_f64, X, y, N, d, ls, kid, float(jitter1), float(jitter2), Xs, M, kind, p0, p1,
              float(diag_add), int(chunk), mu, sigma, acq, cov, out.res, out.info_ptr)
    return dict(out.decode(), mu=mu, sigma=sigma, acq=acq, cov_meas=cov)


def select_qei(X, y, ls, Xs, Z, f_best: float, xi: float = 0.0, chunk: int = 0, lib=None) -> dict:
    """q = 8 Monte-Carlo Expected Improvement on host arrays (gpbo_select_qei_host_f64): the candidates in consecutive
    batches of 8 (M a multiple of 8), Z [S x 8] the base samples.  Returns dict(best_val, best_idx: the first batch with
    the largest qEI, nan_count, info, qei [M / 8])."""
    lib = lib or _lib.load()
    X, y, ls, Xs, N, d, M = _problem(X, y, ls, Xs)
    Z = _f64(Z)
    qei = np.empty(M // 8)
    out = _Result()
    _lib.note_hip_use()
    _lib.call(lib.gpbo_select_qei_host_f64, X, y, N, d, ls, JITTER_KERNEL, JITTER_ASSEMBLY, Xs, M, float(f_best), float(xi), Z,
              len(Z), int(chunk), qei, out.res, out.info_ptr)
    return dict(out.decode(), qei=qei)


def select_batch(X, y, ls, Xs, q: int, acquisition: str = "lcb", explore: float = 4.0, f_best=None, xi: float = 0.0,
                 fantasy: str = "believer", lie=None, dense: bool = False, chunk: int = 0, lib=None) -> dict:
    """Greedy q-point batch on host arrays (gpbo_select_batch_host_f64).  Returns dict(indices, values, nan_count, info,
    mu, sigma); mu / sigma (dense=True) are the posterior the q-th member was chosen from."""
    lib = lib or _lib.load()
    X, y, ls, Xs, N, d, M = _problem(X, y, ls, Xs)
    q = int(q)
    if d > _lib.MAX_D or not 1 <= q <= min(_lib.BATCH_MAX_Q, M):
        raise ValueError(f"select_batch needs d <= {_lib.MAX_D} and q in [1, min({_lib.BATCH_MAX_Q}, M = {M})]")
    kind, p0, p1 = acq_params(acquisition, explore, f_best, xi)
    fkind, fl = fantasy_params(fantasy, lie)
    idx, val = np.full(q, -1, dtype=np.int64), np.full(q, np.nan)
    mu, sigma = (np.empty(M) if dense else None for _ in range(2))
    out = _Result()
    _lib.note_hip_use()
    _lib.call(lib.gpbo_select_batch_host_f64, X, y, N, d, ls, JITTER_KERNEL, JITTER_ASSEMBLY, Xs, M, kind, p0, p1, int(chunk),
              q, fkind, fl, idx, val, mu, sigma, out.res, out.info_ptr)
    r = out.decode()
    return dict(indices=idx, values=val, nan_count=r["nan_count"], info=r["info"], mu=mu, sigma=sigma)


def select_thompson(X, y, ls, Xs, q: int, n_paths=None, n_features: int = 2048, seed: int = 0, dense: bool = False,
                    lib=None) -> dict:
    """q points by Thompson sampling on host arrays (gpbo_thompson_host_f64: factorisation, path weights and the paths over
    all candidates in one call; the draws are thompson.thompson_draws(d, n_features, n_paths, N, seed)).  Returns
    dict(indices, values: the first q DISTINCT winners in path order - fewer than q when the paths agree -, all_indices,
    all_values, nan_counts [n_paths], info, f [n_paths x M] with dense=True)."""
    from .thompson import first_distinct, select_params, thompson_draws

    X, y, ls, Xs, N, d, M = _problem(X, y, ls, Xs)
    q, S, F, seed = select_params(q, n_paths, n_features, seed, M=M, d=d)
    lib = lib or _lib.load()
    omega, phase, W, E = (_f64(a) for a in thompson_draws(d, F, S, N, seed))
    idx, val, nan = np.full(S, -1, dtype=np.int64), np.full(S, np.nan), np.zeros(S, dtype=np.int64)
    f = np.empty((S, M)) if dense else None
    out = _Result()
    _lib.note_hip_use()
    _lib.call(lib.gpbo_thompson_host_f64, X, y, N, d, ls, JITTER_KERNEL, JITTER_ASSEMBLY, Xs, M, omega, phase, W, E, F, S, idx,
              val, nan, f, out.info_ptr)
    keep = first_distinct(idx, q)
    return dict(indices=idx[keep], values=val[keep], all_indices=idx, all_values=val, nan_counts=nan, info=out.decode()["info"],
                f=f)


def select_nei(X, y, ls, Xs, n_fantasies: int = 16, seed: int = 0, xi: float = 0.0, delta: float = 1e-6, best=None,
               dense: bool = True, dense_means: bool = False, chunk: int = 0, lib=None, jitter1: float = JITTER_KERNEL,
               jitter2: float = JITTER_ASSEMBLY, kernel: str = "se") -> dict:
    """Noisy expected improvement on host arrays (gpbo_nei_host_f64: the factorisation, its noise-free twin, the fantasies and
    the scoring in one call; the draws are nei.nei_draws(N, n_fantasies, seed)).  best: incumbents to use in the place of the
    fantasies' minima.  Returns dict(best_val, best_idx, nan_count, info, acq [M], sigma [M], mu [S x M] with dense_means=True,
    fantasy_best [S])."""
    from .nei import nei_best, nei_draws, nei_params

    kid = _lib.kernel_id(kernel)
    X, y, ls, Xs, N, d, M = _problem(X, y, ls, Xs)
    S, seed, xi, delta = nei_params(n_fantasies, seed, xi, delta, rho=float(jitter1) + float(jitter2))
    b = nei_best(best, S)
    if d > _lib.MAX_D:
        raise ValueError(f"noisy expected improvement needs d <= {_lib.MAX_D}, got d = {d}")
    lib = lib or _lib.load()
    Z, E = (_f64(a) for a in nei_draws(N, S, seed))
    acq, sigma = (np.empty(M) if dense else None for _ in range(2))
    mu = np.empty((S, M)) if dense_means else None
    fbest = np.empty(S)
    out = _Result()
    _lib.note_hip_use()
    _lib.call(lib.gpbo_nei_host_f64, X, y, N, d, ls, kid, float(jitter1), float(jitter2), delta, Xs, M, Z, E, S, xi, int(chunk),
              b, mu, sigma, acq, fbest, out.res, out.info_ptr)
    return dict(out.decode(), acq=acq, sigma=sigma, mu=mu, fantasy_best=fbest)


def _posterior_pair(mu, sigma):
    mu, sigma = _f64(mu).reshape(-1), _f64(sigma).reshape(-1)
    if mu.size < 1 or sigma.size != mu.size:
        raise ValueError("mu and sigma must hold one value per candidate (at least one)")
    return mu, sigma, int(mu.size)


def mes_log_survival(mu, sigma, z, lib=None) -> tuple:
    """(log S(z_q) = sum_c log Phi((mu_c - z_q) / sigma_c) [Q], the number of candidates skipped as NaN) on host arrays
    (gpbo_mes_log_survival_host_f64; Q <= 64 levels in one pass)."""
    mu, sigma, M = _posterior_pair(mu, sigma)
    z = _f64(z).reshape(-1)
    if not 1 <= z.size <= _lib.MES_MAX_LEVELS or not np.all(np.isfinite(z)):
        raise ValueError(f"z must hold 1 to {_lib.MES_MAX_LEVELS} finite levels")
    lib = lib or _lib.load()
    out, nan = np.empty(z.size), np.zeros(1, dtype=np.int64)
    _lib.note_hip_use()
    _lib.call(lib.gpbo_mes_log_survival_host_f64, mu, sigma, M, z, int(z.size), out, nan)
    return out, int(nan[0])


def mes_acq(mu, sigma, y_star, dense: bool = True, lib=None) -> dict:
    """Max-value entropy search on host arrays (gpbo_mes_acq_host_f64): MES(x) = mean_s h((mu - y_star_s) / sigma) over dense
    mu / sigma [M] and its first arg-max.  Returns dict(best_val, best_idx, nan_count, acq [M])."""
    from .mes import mes_y_star

    mu, sigma, M = _posterior_pair(mu, sigma)
    ys = _f64(y_star).reshape(-1)
    if not 1 <= ys.size <= _lib.MES_MAX_S:
        raise ValueError(f"y_star must hold 1 to {_lib.MES_MAX_S} values, got {ys.size}")
    ys = mes_y_star(ys, int(ys.size))
    lib = lib or _lib.load()
    acq = np.empty(M) if dense else None
    out = _Result()
    _lib.note_hip_use()
    _lib.call(lib.gpbo_mes_acq_host_f64, mu, sigma, M, ys, int(ys.size), acq, out.res)
    r = out.decode()
    return dict(best_val=r["best_val"], best_idx=r["best_idx"], nan_count=r["nan_count"], acq=acq)


def constrained_acq(mu, sigma, cons_mu, cons_sigma, upper, base: str = "ei", f_best=None, xi: float = 0.0, dense: bool = True,
                    lib=None) -> dict:
    """The constrained acquisitions on host arrays (gpbo_constrained_acq_host_f64): value = base + sum_c log Phi((upper_c -
    cons_mu_c) / cons_sigma_c) over dense posteriors and its first arg-max; base "ei", "pi" or "none" (mu / sigma may be None
    then).  cons_mu, cons_sigma: [C x M] (None or empty with no constraint).  Returns dict(best_val, best_idx, nan_count,
    value [M], log_feasibility [M])."""
    from .constrained import cons_limits, cons_params

    u = cons_limits(upper)
    C = int(u.size)
    bid, fb, xi = cons_params(base, f_best, xi, C)
    cm = cs = None
    if C > 0:
        cm, cs = _f64(cons_mu).reshape(C, -1), _f64(cons_sigma).reshape(C, -1)
        if cm.shape != cs.shape or cm.shape[1] < 1:
            raise ValueError("cons_mu and cons_sigma must hold one row of M values per limit")
    if bid == _lib.CONS_BASE_NONE:
        mu = sigma = None
        M = int(cm.shape[1])
    else:
        mu, sigma, M = _posterior_pair(mu, sigma)
        if C > 0 and cm.shape[1] != M:
            raise ValueError("cons_mu and cons_sigma must hold one row of M values per limit")
    lib = lib or _lib.load()
    val, feas = (np.empty(M), np.empty(M)) if dense else (None, None)
    out = _Result()
    _lib.note_hip_use()
    _lib.call(lib.gpbo_constrained_acq_host_f64, mu, sigma, M, bid, fb, xi, cm, cs, M, C, u, val, feas, out.res)
    r = out.decode()
    return dict(best_val=r["best_val"], best_idx=r["best_idx"], nan_count=r["nan_count"], value=val, log_feasibility=feas)


def ehvi_acq(mu1, sigma1, mu2, sigma2, front, ref, dense: bool = True, lib=None) -> dict:
    """Two-objective expected hypervolume improvement on host arrays (gpbo_ehvi_acq_host_f64): log EHVI over the dense posteriors
    of two minimised objectives and its first arg-max.  front [P x 2], ref (r1, r2): as DeviceGP.ehvi_on_posterior.  Returns
    dict(best_val, best_idx, nan_count, value [M])."""
    from .pareto import check_front

    F, r = check_front(front, ref)
    mu1, sigma1, M = _posterior_pair(mu1, sigma1)
    mu2, sigma2, M2 = _posterior_pair(mu2, sigma2)
    if M2 != M:
        raise ValueError("the two objectives' posteriors must hold one value per candidate each")
    lib = lib or _lib.load()
    val = np.empty(M) if dense else None
    out = _Result()
    _lib.note_hip_use()
    _lib.call(lib.gpbo_ehvi_acq_host_f64, mu1, sigma1, mu2, sigma2, M, F, int(F.shape[0]), r[0], r[1], val, out.res)
    res = out.decode()
    return dict(best_val=res["best_val"], best_idx=res["best_idx"], nan_count=res["nan_count"], value=val)


def refine(X, y, ls, starts, lower, upper, acquisition: str = "lcb", explore: float = 4.0, f_best=None, xi: float = 0.0,
           iters: int = 30, step0: float = 0.1, lib=None) -> dict:
    """Off-grid refinement on host arrays (gpbo_refine_host_f64: factorisation and refinement in one call).  Returns
    dict(x [P x d], acq, acq0, accepted, pg, best, best_val, nan_count, info)."""
    lib = lib or _lib.load()
    X, y, ls, N, d = _problem(X, y, ls)
    x = np.array(np.asarray(starts, dtype=np.float64).reshape(-1, d), dtype=np.float64, order="C")   # a copy: in / out
    P = x.shape[0]
    iters, step0 = refine_params(P, d, iters, step0)
    lo, hi = refine_box(lower, upper, d)
    kind, p0, p1 = acq_params(acquisition, explore, f_best, xi)
    acq, acq0, pg, accepted = np.empty(P), np.empty(P), np.empty(P), np.empty(P, dtype=np.int32)
    out = _Result()
    _lib.note_hip_use()
    _lib.call(lib.gpbo_refine_host_f64, X, y, N, d, ls, JITTER_KERNEL, JITTER_ASSEMBLY, x, P, lo, hi, kind, p0, p1, iters, step0,
              acq, acq0, accepted, pg, out.res, out.info_ptr)
    r = out.decode()
    return dict(x=x, acq=acq, acq0=acq0, accepted=accepted, pg=pg, best=r["best_idx"], best_val=r["best_val"],
                nan_count=r["nan_count"], info=r["info"])


class _GridOnly(LikelihoodFits):
    """What PointSelector.tune_kernel needs from its surrogate object: the likelihood grid (ard="grid"), the likelihood
    and its gradient (ard="gradient") or the likelihood over all hyperparameters (ard="hyper"), and the fits over them."""

    def __init__(self, lib):
        self.lib = lib

    def nlml_grid(self, X, y, ls_cells, jitter: float = JITTER_KERNEL, likelihood: str = "reference"):
        return nlml_grid(X, y, ls_cells, jitter, self.lib, likelihood)

    def nlml_and_grad(self, X, y, ls, jitter: float = JITTER_KERNEL, kernel: str = "se"):
        return nlml_and_grad(X, y, ls, jitter, self.lib, kernel)

    def nlml_hyper(self, X, y, ls, noise, fit_mean: bool = True, fit_scale: bool = True, kernel: str = "se"):
        return nlml_hyper(X, y, ls, noise, fit_mean, fit_scale, self.lib, kernel)

    @contextmanager
    def _fit_session(self, X, y):
        yield _f64(X), _f64(y).reshape(-1)   # made contiguous once for all evaluations


class PointSelectorHost(PointSelector):
    """`PointSelector` with the same attribute protocol (point_selector.py:13-207), on the host-pointer entry points."""

    def __init__(self, verbose: bool = False, chunk: int = 0, likelihood: str = "reference", ard: str = "grid",
                 noise0: float = 1e-2, noise_bounds=(1e-6, 1.0), kernel: str = "se"):
        if ard == "marginal":
            raise ValueError("ard='marginal' needs PointSelector, the device class (the ensemble of factorisations does not "
                             "outlive a host-pointer call)")
        super().__init__(device=None, verbose=verbose, shard_candidates=False, likelihood=likelihood, ard=ard, noise0=noise0,
                         noise_bounds=noise_bounds, kernel=kernel)
        self.lib = _lib.load()
        self._gp = _GridOnly(self.lib)
        self._chunk = int(chunk)
        self._inputs = None

    def _surrogate_inputs(self):
        self._need_update()
        return self._inputs

    def _factorised(self, r):
        """The result dict of a host call, or the error of a covariance matrix that is not positive definite."""
        if r["info"] != 0:
            raise np.linalg.LinAlgError(f"covariance matrix is not positive definite (pivot {r['info']} of {len(self._inputs[0])}); "
                                        "the reference's np.linalg.inv would raise or return garbage here")
        return r

    def _score(self, acquisition, want_cov_meas=False, **kw):
        """One host call with this update's model; the result dict with mu / sigma / acq / best_val in the units of y."""
        X, y, ls, Xs = self._inputs
        m = self._model
        r = self._factorised(select_next(X, m.to_model(y), ls, Xs, acquisition=acquisition, dense=True,
                                         want_cov_meas=want_cov_meas, chunk=self._chunk, lib=self.lib, jitter1=m.jitter1,
                                         jitter2=m.jitter2, diag_add=m.diag_add(Xs.shape, X.shape), kernel=m.kernel,
                                         **m.acq_kw(kw)))
        r.update(mu=m.mean_to_y(r["mu"]), sigma=m.sd_to_y(r["sigma"]), acq=m.acq_to_y(acquisition, r["acq"]),
                 best_val=float(m.acq_to_y(acquisition, r["best_val"])))
        return r

    def _score_acq(self, kind, **kw):
        r = self._score(kind, **kw)
        return r["acq"], (r["best_val"], r["best_idx"], r["nan_count"])

    _NEGATIVE_INDEX_IS_NAN = True

    def _not_in_hyper_mode(self, what: str):
        need_se(self._kernel, what)
        if self._ard == "hyper":
            raise ValueError(f"PointSelectorHost(ard='hyper') supports update_surrogate(), lower_confidence_bound() and "
                             f"expected_improvement(); {what} needs PointSelector")

    def loo(self):
        raise ValueError("loo() needs PointSelector (the factorisation does not outlive a host-pointer call)")

    def update_surrogate(self):
        """point_selector.py:42-102."""
        X, y, Xs, ls = self._begin_update()
        self._inputs = (X, y, ls, Xs)
        r = self._score("lcb", want_cov_meas=True, explore=4.0)
        self.cov_meas = r["cov_meas"]
        self.cov_pred = self.cov_meas_pred = None                         # not materialised on this route
        self.last_update = "factorise"
        self._publish(r["mu"], r["sigma"], r["acq"], (r["best_val"], r["best_idx"], r["nan_count"]))

    def q_expected_improvement(self, n_samples=512, seed=7, xi=0.0):
        """q = 8 Monte-Carlo Expected Improvement on the host-pointer route (same definition and return value as
        PointSelector.q_expected_improvement: the (8, ndim) multi-indices of the first batch with the largest qEI)."""
        self._not_in_hyper_mode("q_expected_improvement()")
        X, y, ls, Xs = self._surrogate_inputs()
        fd = [int(v) for v in self.feature_domain]
        M = int(np.prod(fd))
        if M % 8:
            raise ValueError("q_expected_improvement needs a candidate count that is a multiple of 8")
        Z = np.random.default_rng(seed).standard_normal((int(n_samples), 8))
        r = self._factorised(select_qei(X, y, ls, Xs, Z, float(np.min(y)), xi=xi, chunk=self._chunk, lib=self.lib))
        self.acq_func_eval = r["qei"]
        if r["nan_count"] > 0 or r["best_idx"] >= M // 8 or r["best_idx"] < 0:
            raise IndexError(NAN_ACQUISITION)
        flat = r["best_idx"] * 8 + np.arange(8)
        return np.stack(np.unravel_index(flat, fd), axis=1).astype(np.int64)

    def select_batch(self, q, acquisition="lcb", explore=4, xi=0.0, fantasy="believer", lie=None):
        """PointSelector.select_batch on the host-pointer route (gpbo_select_batch_host_f64: factorisation, plain pass and
        selection in one call): the same (q, ndim) multi-indices, the same errors."""
        self._not_in_hyper_mode("select_batch()")
        X, y, ls, Xs = self._surrogate_inputs()
        if Xs.shape == X.shape:
            raise ValueError("select_batch() does not support candidates of the observations' shape (the N == M quirk)")
        r = select_batch(X, y, ls, Xs, q, fantasy=fantasy, lie=lie, chunk=self._chunk, lib=self.lib,
                         **self._batch_acq(acquisition, explore, xi))
        if np.all(r["indices"] < 0):   # (with members chosen, info is the selection's own report)
            self._factorised(r)
        return self._batch_indices(r["indices"], r["nan_count"])

    def select_thompson(self, q, n_features=2048, seed=0):
        """PointSelector.select_thompson on the host-pointer route (gpbo_thompson_host_f64): the same (k, ndim) multi-indices
        for the same seed, the same errors."""
        self._not_in_hyper_mode("select_thompson()")
        X, y, ls, Xs = self._surrogate_inputs()
        r = self._factorised(select_thompson(X, y, ls, Xs, q, n_features=n_features, seed=seed, lib=self.lib))
        return self._batch_indices(r["indices"], int(np.sum(r["nan_counts"])))

    def _nei_scores(self, S, seed, xi, delta):
        """PointSelector.noisy_expected_improvement on the host-pointer route (gpbo_nei_host_f64): the same fantasies for the
        same seed, the same values."""
        X, y, ls, Xs = self._surrogate_inputs()
        m = self._model
        r = self._factorised(select_nei(X, m.to_model(y), ls, Xs, S, seed, xi=xi, delta=delta, chunk=self._chunk, lib=self.lib,
                                        jitter1=m.jitter1, jitter2=m.jitter2, kernel=m.kernel))
        return r["acq"], (r["best_val"], r["best_idx"], r["nan_count"]), r["fantasy_best"]

    def max_value_entropy_search(self, n_samples=16, seed=0, y_star="gumbel", cap="observed"):
        """PointSelector.max_value_entropy_search on the host-pointer route: the same samples for the same seed, the same
        index.  y_star: "gumbel" or n_samples values; "thompson" needs PointSelector (ValueError)."""
        if isinstance(y_star, str) and y_star == "thompson":
            raise ValueError("max_value_entropy_search(y_star='thompson') needs PointSelector (the sample paths are drawn on the "
                             "factorisation, which does not outlive a host-pointer call): use y_star='gumbel' or an array")
        return super().max_value_entropy_search(n_samples=n_samples, seed=seed, y_star=y_star, cap=cap)

    def _mes_scores(self, S, seed, y_star, cap):
        """PointSelector.max_value_entropy_search on the host-pointer route (gpbo_mes_log_survival_host_f64 /
        gpbo_mes_acq_host_f64 on mean_func / cov_func, taken back to the units of the model): the same samples for the same
        seed, the same values."""
        from . import mes as MES

        m = self._model
        mu = _f64(m.to_model(np.asarray(self.mean_func, dtype=np.float64))).reshape(-1)
        sigma = _f64(np.asarray(self.cov_func, dtype=np.float64) / m.y_scale if m.fitted else self.cov_func).reshape(-1)
        if isinstance(y_star, str):
            ok = ~(np.isnan(mu) | np.isnan(sigma))
            if not np.any(ok):
                raise IndexError(NAN_ACQUISITION)
            lo = float(np.min(mu[ok] - MES.LO_SIGMAS * sigma[ok]))
            hi = float(np.min(mu[ok] + MES.HI_SIGMAS * sigma[ok]))
            quartiles, _ = MES.gumbel_quartiles(lambda z: mes_log_survival(mu, sigma, z, self.lib), lo, hi)
            minima = MES.sample_minima(quartiles, MES.mes_uniforms(S, seed), cap)
        else:
            minima = y_star
        r = mes_acq(mu, sigma, minima, lib=self.lib)
        return r["acq"], (r["best_val"], r["best_idx"], r["nan_count"]), minima

    def _cons_posterior(self) -> tuple:
        """mean_func / cov_func taken back to the units of the model, as host arrays [M]."""
        m = self._model
        mu = _f64(m.to_model(np.asarray(self.mean_func, dtype=np.float64))).reshape(-1)
        sigma = _f64(np.asarray(self.cov_func, dtype=np.float64) / m.y_scale if m.fitted else self.cov_func).reshape(-1)
        return mu, sigma

    def _cons_scores(self, base, f_best, xi, posteriors, upper):
        """PointSelector._cons_scores on the host-pointer route (gpbo_constrained_acq_host_f64): the same values."""
        mu, sigma = self._cons_posterior()
        cm = np.stack([p[0] for p in posteriors]) if posteriors else None
        cs = np.stack([p[1] for p in posteriors]) if posteriors else None
        r = constrained_acq(mu, sigma, cm, cs, upper, base=base, f_best=f_best, xi=xi, lib=self.lib)
        return r["value"], r["log_feasibility"], (r["best_val"], r["best_idx"], r["nan_count"])

    def _ehvi_scores(self, posterior2, front, ref):
        """PointSelector._ehvi_scores on the host-pointer route (gpbo_ehvi_acq_host_f64): the same values."""
        mu1, sigma1 = self._cons_posterior()
        r = ehvi_acq(mu1, sigma1, posterior2[0], posterior2[1], front, ref, lib=self.lib)
        return r["value"], (r["best_val"], r["best_idx"], r["nan_count"])

    def refine_next(self, n_starts=64, iters=30, acquisition="lcb", explore=4, xi=0.0):
        """PointSelector.refine_next on the host-pointer route (gpbo_refine_host_f64): the same d coordinates, the same
        errors."""
        self._not_in_hyper_mode("refine_next()")
        X, y, ls, _ = self._surrogate_inputs()
        kw, starts, lo, hi = self._refine_inputs(n_starts, iters, acquisition, explore, xi)
        r = self._factorised(refine(X, y, ls, starts, lo, hi, iters=int(iters), lib=self.lib, **kw))
        if r["nan_count"] > 0 or r["best"] < 0:
            raise IndexError(NAN_ACQUISITION)
        return r["x"][r["best"]].copy()
