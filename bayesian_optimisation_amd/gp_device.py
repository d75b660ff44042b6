"""Device-resident GP surrogate: host orchestration of the libgpbo kernels.

PyTorch-ROCm is used here for device memory, streams and (in distributed.py) the process group -
plumbing only; every number is produced by the HIP kernels behind the C ABI (include/gpbo.h).

Mirrors the arithmetic of PointSelector.update_surrogate / lower_confidence_bound
(/root/reference/point_selector.py:76-98, 197-207) with the factorisation done once per BO step and
the candidates streamed in chunks.  There is no CPU path: without libgpbo.so or a GPU this raises.
The ML-II fits are written once, in `LikelihoodFits`, over a provider's nlml_and_grad() / nlml_hyper(): DeviceGP here (device
tensors, one input check and one factorise-into-fit-buffers step for both) and host_binding's host-pointer provider.
"""
from __future__ import annotations

import ctypes as C
from contextlib import contextmanager
from dataclasses import dataclass
from typing import Optional

import numpy as np

from . import _lib, ard_fit
from .model import JITTER_ASSEMBLY, JITTER_KERNEL, need_se  # noqa: F401  (the two jitters are part of this module's API)

# the IndexError of an acquisition with NaN in it: the reference's own failure, in NumPy's words (point_selector.py:207)
NAN_ACQUISITION = "index 0 is out of bounds for axis 0 with size 0 (acquisition contains NaN)"
PRIOR_VAR = (1.0 + JITTER_KERNEL) + JITTER_ASSEMBLY  # diagonal of cov_pred as the reference rounds it

DEFAULT_CHUNK = 1 << 17


def _torch():
    if _lib.hip_used_before_pytorch:
        # Seen on MI355X / ROCm 7: importing PyTorch and creating its GPU context AFTER this library has already
        # initialised HIP in the process (host-pointer binding used first) dead-locks now and then.  The other order
        # is the one every tensor-resident path takes and has never hung - so that is the only one allowed.
        raise _lib.GpboError(
            "libgpbo.so was used in this process before PyTorch was imported (PointSelectorHost / host_binding first). "
            "A process that needs both must `import torch` before its first use of bayesian_optimisation_amd.")
    import torch

    if not torch.cuda.is_available():
        raise _lib.GpboError("no GPU visible: the acquisition path runs only on the HIP kernels (no CPU fallback)")
    return torch


def acq_params(acquisition: str, explore: float = 4.0, f_best: Optional[float] = None, xi: float = 0.0) -> tuple:
    """(kind, p0, p1) of the C ABI for an acquisition by name (include/gpbo.h: GPBO_ACQ_*)."""
    if acquisition == "lcb":
        return _lib.ACQ_LCB, float(explore), 0.0
    if acquisition == "ei":
        if f_best is None:
            raise ValueError("EI needs f_best (the incumbent minimum)")
        return _lib.ACQ_EI, float(f_best), float(xi)
    raise ValueError(f"unknown acquisition {acquisition!r}")


def _round_up(n: int, granule: int = _lib.CHUNK_GRANULE) -> int:
    return (n + granule - 1) // granule * granule


@dataclass
class ScoreResult:
    best_val: float
    best_idx: int
    nan_count: int
    mu: Optional[object] = None      # torch fp64 device tensors [M] when dense=True
    sigma: Optional[object] = None
    acq: Optional[object] = None


@dataclass
class BatchResult:
    """What DeviceGP.select_batch returns: the q members in selection order."""
    indices: np.ndarray              # int64 [q], idx_offset + row of Xs; -1 from the first member that could not be chosen
    values: np.ndarray               # float64 [q], the acquisition of each member when it was chosen
    nan_count: int                   # > 0: the acquisition contains NaN (the reference raises IndexError)
    info: int                        # 0, or the 1-based member whose fantasy pivot s_j was not positive / not finite
    mu: Optional[object] = None      # torch fp64 device tensors [M]: the posterior the q-th member was chosen from
    sigma: Optional[object] = None


@dataclass
class GradResult:
    """What DeviceGP.posterior_grad returns: torch fp64 device tensors, values [P] and gradients in x [P x d]."""
    mu: object
    sigma: object
    acq: object
    dmu: object
    dsigma: object
    dacq: object


@dataclass
class RefineResult:
    """What DeviceGP.refine returns.  x / acq / acq0 / accepted / pg are device tensors, one row per start."""
    x: object                        # fp64 [P x d]: the refined points (inside the box)
    acq: object                      # fp64 [P]: the acquisition there
    acq0: object                     # fp64 [P]: the acquisition at the clipped start
    accepted: object                 # int32 [P]: accepted steps
    pg: object                       # fp64 [P]: projected-gradient norm max_k |x_k - clip(x_k + g_k ls_k^2)| / ls_k
    best: int                        # the LOWEST start with the largest final acquisition (-1: none)
    best_val: float
    nan_count: int                   # starts whose acq0 is NaN (they never move; the classes raise IndexError)
    grid_idx: Optional[int] = None   # select_refined(): score()'s arg-max over the candidates and its value
    grid_val: Optional[float] = None


@dataclass
class ThompsonPaths:
    """What DeviceGP.thompson_paths returns: S sample paths of the posterior as device tensors (include/gpbo.h).  Valid until
    the next factorise() / append() / load_state_dict() of the surrogate that made them."""
    omega: object                    # fp64 [F x d]
    phase: object                    # fp64 [F]
    W: object                        # fp64 [S x F]
    V: object                        # fp64 [S x Np]: v_s = K^-1 (y - g_s(X) - sqrt(kappa) E[s]), factorisation order
    n_paths: int
    n_features: int
    seed: int
    epoch: tuple = ()                # the factorisation they belong to


@dataclass
class ThompsonResult:
    """What DeviceGP.thompson_score / select_thompson return, one entry per path (select_thompson: per selected point)."""
    indices: np.ndarray              # int64: idx_offset + the lowest row minimising the path (-1: no usable row)
    values: np.ndarray               # float64: the acquisition -f_s there
    nan_counts: np.ndarray           # int64 [n_paths]: rows whose value is NaN, per path
    f: Optional[object] = None       # dense=True: torch fp64 device tensor [n_paths x M], the paths at the rows of Xs

    @property
    def nan_count(self) -> int:
        return int(np.sum(self.nan_counts))


@dataclass
class Fantasies:
    """What DeviceGP.fantasies returns: S samples of the latent function at the observed points and the noise-free twin they
    are scored with, as device tensors (include/gpbo.h).  Valid until the next factorise() / append() / load_state_dict() of
    the surrogate that made them."""
    A: object                        # fp64 [S x Np]: the weights, mu_s(x) = k(x) . A_s (zero on the padding)
    F: object                        # fp64 [S x Np]: the fantasy values at the observations (zero on the padding)
    best: object                     # fp64 [S]: min_{i < N} F_s[i], the incumbent of each fantasy
    K0d: object                      # fp64 [Np x Np]: the twin's matrix K0 + delta I
    U0: object                       # fp64 [Np x Np]: the twin's factor, U0 U0^T = K0d^-1
    n_fantasies: int
    seed: int
    delta: float
    epoch: tuple = ()                # the factorisation they belong to


@dataclass
class NeiResult:
    """What DeviceGP.score_nei / select_nei return."""
    best_val: float
    best_idx: int
    nan_count: int
    fantasy_best: object             # fp64 [S] device tensor: the incumbents the expected improvements were measured against
    acq: Optional[object] = None     # dense=True: torch fp64 device tensors, NEI [M] ...
    sigma: Optional[object] = None   # ... the twin's standard deviation [M] ...
    mu: Optional[object] = None      # ... and the S means [S x M]


@dataclass
class MesResult:
    """What DeviceGP.mes_on_posterior / select_mes return."""
    best_val: float
    best_idx: int
    nan_count: int
    acq: Optional[object] = None        # dense=True: torch fp64 device tensor, MES [M]
    y_star: Optional[np.ndarray] = None   # float64 [S]: the sampled minima the terms were measured against (units of the model)
    quartiles: Optional[np.ndarray] = None   # y_star="gumbel": (z75, z50, z25), the levels where Pr[m* > z] = 0.75, 0.5, 0.25
    mu: Optional[object] = None         # select_mes: the posterior the pass returned, fp64 [M] device tensors
    sigma: Optional[object] = None


@dataclass
class ConstrainedResult:
    """What DeviceGP.constrained_on_posterior / select_constrained return.  Every value is a LOGARITHM (-inf is a legal value)."""
    best_val: float
    best_idx: int
    nan_count: int
    base: str                                     # the base term that was used: "ei", "pi" or "none"
    value: Optional[object] = None                # dense=True: torch fp64 device tensors [M], base + log feasibility ...
    log_feasibility: Optional[object] = None      # ... and sum_c log Phi((u_c - mu_c) / sigma_c) alone
    f_best: Optional[float] = None                # the incumbent the base was measured against (None without a base)


@dataclass
class EhviResult:
    """What DeviceGP.ehvi_on_posterior / select_ehvi return.  Every value is a LOGARITHM (-inf is a legal value)."""
    best_val: float
    best_idx: int
    nan_count: int
    value: Optional[object] = None                # dense=True: torch fp64 device tensor [M], log EHVI
    front: Optional[np.ndarray] = None            # the front [P x 2] and the reference point (r1, r2) that were used
    ref: Optional[tuple] = None


def refine_params(P: int, d: int, iters: int, step0: float) -> tuple:
    """(iters, step0) as the C ABI takes them; refuses what gpbo_refine_f64 refuses (include/gpbo.h)."""
    if not 1 <= int(P) <= _lib.REFINE_MAX_P:
        raise ValueError(f"the number of points must be in [1, {_lib.REFINE_MAX_P}], got {P}")
    if not 1 <= int(d) <= _lib.MAX_D:
        raise ValueError(f"refinement needs 1 <= d <= {_lib.MAX_D}, got d = {d}")
    if int(iters) != iters or not 0 <= int(iters) <= 1000:
        raise ValueError(f"iters must be an integer in [0, 1000], got {iters!r}")
    step0 = float(step0)
    if not (np.isfinite(step0) and step0 > 0.0):
        raise ValueError(f"step0 must be positive and finite, got {step0!r}")
    return int(iters), step0


def refine_box(lower, upper, d: int) -> tuple:
    """(lower, upper) as contiguous fp64 host arrays of d finite values with lower <= upper (scalars are broadcast)."""
    lo = np.ascontiguousarray(np.broadcast_to(np.asarray(lower, dtype=np.float64).reshape(-1), (d,)))
    hi = np.ascontiguousarray(np.broadcast_to(np.asarray(upper, dtype=np.float64).reshape(-1), (d,)))
    if not (np.all(np.isfinite(lo)) and np.all(np.isfinite(hi)) and np.all(lo <= hi)):
        raise ValueError("the box needs finite bounds with lower <= upper in every coordinate")
    return lo, hi


def fantasy_params(fantasy: str, lie: Optional[float]) -> tuple:
    """(kind, lie) of the C ABI for a fantasy rule by name (include/gpbo.h: GPBO_FANTASY_*)."""
    if fantasy == "believer":
        return _lib.FANTASY_BELIEVER, 0.0
    if fantasy == "liar":
        if lie is None or not np.isfinite(float(lie)):
            raise ValueError("fantasy='liar' needs a finite lie (the constant every fantasy observation takes)")
        return _lib.FANTASY_LIE, float(lie)
    raise ValueError(f"fantasy must be 'believer' or 'liar', got {fantasy!r}")


class LikelihoodFits:
    """The ML-II fits (ard_fit.py) over a provider's nlml_and_grad() / nlml_hyper().  The provider's _fit_session(X, y) is a
    context manager around one fit: it yields the (X, y) every evaluation receives and cleans up behind the fit."""

    def fit_length_scales(self, X, y, ls0, lower, upper, jitter: float = JITTER_KERNEL, kernel: str = "se", **opts):
        """ML-II fit of the ARD length scales inside [lower, upper] from ls0 (ard_fit.fit_length_scales: projected L-BFGS
        in log ls, every evaluation one nlml_and_grad).  Returns the FitResult."""
        with self._fit_session(X, y) as (X, y):
            return ard_fit.fit_length_scales(lambda ls: self.nlml_and_grad(X, y, ls, jitter, kernel), ls0, lower, upper, **opts)

    def fit_hyperparameters(self, X, y, ls0, ls_lower, ls_upper, noise0: float = 1e-2, noise_lower: float = 1e-6,
                            noise_upper: float = 1.0, fit_mean: bool = True, fit_scale: bool = True, kernel: str = "se",
                            **opts):
        """ML-II fit of the length scales and the noise-to-signal ratio inside their boxes, mean and signal variance profiled
        out (ard_fit.fit_hyperparameters: projected L-BFGS in the d + 1 log variables, every evaluation one nlml_hyper).
        Returns the HyperFitResult."""
        with self._fit_session(X, y) as (X, y):
            return ard_fit.fit_hyperparameters(lambda ls, noise: self.nlml_hyper(X, y, ls, noise, fit_mean, fit_scale, kernel),
                                               ls0, ls_lower, ls_upper, noise0, noise_lower, noise_upper, **opts)


class DeviceSide:
    """What DeviceGP and ensemble.DeviceEnsemble share: the device and the chunk, uploads, the grow-only workspaces, the input
    checks and the pieces of an argument list that recur.  Tensors and arrays go into a library call as they are
    (_lib.Pointer); a call that returns a status goes through _lib.call."""

    def __init__(self, device=None, chunk: int = DEFAULT_CHUNK):
        torch = _torch()
        self.lib = _lib.load()
        self.torch = torch
        self.device = torch.device("cuda", torch.cuda.current_device()) if device is None else torch.device(device)
        if chunk % _lib.CHUNK_GRANULE:
            raise ValueError(f"chunk must be a multiple of {_lib.CHUNK_GRANULE}")
        self.chunk = int(chunk)
        self.N = self.Np = self.d = 0
        self.kernel = "se"           # covariance family of the held factorisation (_lib.KERNEL_IDS)

    def _stream(self):
        return C.c_void_p(self.torch.cuda.current_stream(self.device).cuda_stream)

    def _dev(self, arr):
        torch = self.torch
        if isinstance(arr, torch.Tensor):
            t = arr.to(device=self.device, dtype=torch.float64)
            return t if t.is_contiguous() else t.contiguous()
        return torch.from_numpy(np.ascontiguousarray(arr, dtype=np.float64)).to(self.device)

    @staticmethod
    def _ptr(t):
        """The address of a tensor as a c_void_p (tests and tools; the calls of this package pass the tensor itself)."""
        return C.c_void_p(t.data_ptr()) if t is not None else C.c_void_p(0)

    def _candidates(self, Xs):
        """(Xs as a contiguous fp64 device tensor, its row count); refuses anything but (M, d)."""
        Xsd = self._dev(Xs)
        if Xsd.dim() != 2 or int(Xsd.shape[1]) != self.d:
            raise ValueError("Xs must be (M, d) with the same d as X")
        return Xsd, int(Xsd.shape[0])

    def _chunk_for(self, M: int, granule: int = _lib.CHUNK_GRANULE) -> int:
        """self.chunk, but no more than M candidates need, in whole granules."""
        return _round_up(min(self.chunk, _round_up(M, granule)), granule)

    def _workspace(self, slot_name: str, nbytes: int, free_first: bool = False):
        """The workspace tensor kept in attribute `slot_name`, grown to hold nbytes (the answer of a size query; negative:
        the library refused the sizes).  free_first: the old buffer goes before the new one comes - for the slots that
        reach GiBs, where the two must not coexist."""
        if nbytes < 0:
            raise _lib.GpboError(f"{slot_name}: the workspace size query refused the sizes")
        w = getattr(self, slot_name)
        if w is None or w.numel() * 8 < nbytes:
            if free_first:
                w = None
                setattr(self, slot_name, None)
            w = self.torch.empty((nbytes + 7) // 8, dtype=self.torch.float64, device=self.device)
            setattr(self, slot_name, w)
        return w

    def _kid(self) -> int:
        return _lib.KERNEL_IDS[self.kernel]

    def _dense(self, M: int, dense: bool = True) -> tuple:
        """The three dense fp64 outputs [M] of a scoring call, or three times None."""
        if not dense:
            return None, None, None
        return tuple(self.torch.empty(M, dtype=self.torch.float64, device=self.device) for _ in range(3))

    def _problem(self, X, y, ls, d_limits, positive: bool = False, host_y: bool = False) -> tuple:
        """The one check of (X, y, length scales): (X on the device, y flat - on the device, or a host array with host_y -,
        N, d, the length scales as a contiguous host array or None when ls is None).  d_limits: (largest d, message with
        {d}) pairs, refused in that order; positive: the length scales must be positive."""
        Xd = self._dev(X)
        if Xd.dim() != 2:
            raise ValueError("X must be (N, d)")
        N, d = int(Xd.shape[0]), int(Xd.shape[1])
        for max_d, message in d_limits:
            if d > max_d:
                raise ValueError(message.format(d=d))
        if host_y:
            # (a tensor is what nlml_hyper_cells_fn has always taken; no copy of an array that is fp64 already)
            y = np.asarray(y.detach().cpu().numpy() if isinstance(y, self.torch.Tensor) else y, dtype=np.float64).reshape(-1)
        else:
            y = self._dev(y).reshape(-1)
        if (y.size if host_y else y.numel()) != N:
            raise ValueError("y must have one value per row of X")
        if ls is None:
            return Xd, y, N, d, None
        ls_h = np.ascontiguousarray(np.asarray(ls, dtype=np.float64).reshape(-1))
        if ls_h.size != d:
            raise ValueError(f"length scales: expected {d} values, got {ls_h.size}")
        if positive and not np.all(ls_h > 0):
            raise ValueError("length scales must be positive")
        return Xd, y, N, d, ls_h

    def _factorise_into(self, Xd, yd, N, d, ls_h, kid, jitter1, jitter2, Np, K, U, alpha, info, work=None, wbytes=None):
        """Enqueue gpbo_factorise_kern_f64 of (Xd, yd, ls_h) into K / U / alpha / info.  work: a workspace of wbytes as
        gpbo_factorise_workspace_bytes(Np) reports them, or None for this object's own grow-only slot _work_fact."""
        if work is None:
            wbytes = int(self.lib.gpbo_factorise_workspace_bytes(Np))
            work = self._workspace("_work_fact", wbytes)
        _lib.call(self.lib.gpbo_factorise_kern_f64, Xd, yd, N, d, ls_h, kid, jitter1, jitter2, Np, K, U, alpha, info, work,
                  wbytes, self._stream())

    def read_result(self, result_tensor) -> tuple:
        """(best value, best index, NaN count) of a gpbo_result record on the device (synchronises)."""
        r = result_tensor.cpu()
        best_val = float(r[:1].view(self.torch.float64)[0])
        return best_val, int(r[1]), int(r[2])


class DeviceGP(DeviceSide, LikelihoodFits):
    """One BO step's surrogate on one GPU: factorise once, then score any number of candidates."""

    def __init__(self, device=None, chunk: int = DEFAULT_CHUNK):
        super().__init__(device, chunk)
        torch = self.torch
        self.X = self.y = self.ls_h = None   # the observations and length scales of the last factorise() / load_state_dict()
        self.jitter1 = self.jitter2 = 0.0
        self.n_appended = 0
        self._owns_xy = False
        self.K = self.U = self.alpha = None
        # workspaces, kept from call to call and only ever grown (_workspace)
        self._work_post = self._work_fact = self._work_order = self._work_screen = self._work_rescore = None
        self._work_qei = self._work_ard = self._work_batch = self._work_refine = self._work_thompson = self._work_loo = None
        self._work_nei = self._work_mes = self._work_cons = self._work_ehvi = None
        self._epoch = 0              # counts factorise() / append() / load_state_dict(): ThompsonPaths belong to one of them
        self._order_flag = None      # device int32: factorise(order="fps") fell back to the arrival order
        self.U32, self.Np32, self._u32_valid = None, 0, False   # prepare_f32()
        self.U8, self._u8_valid = None, False                   # prepare_i8()
        self._screen_mu = self._screen_var = self._bound_ub = None
        self._fit_bufs = None
        self._keep = self._keep_ard = None   # inputs of the last enqueued call, alive until the stream has consumed them
        self.last_screen = None      # statistics of the last screened call (dict)
        self.perm = None             # factorise(order="fps"): device int64 [N], row of the factorisation -> the caller's row
        # the 32-byte result record and the factorisation's info word share one small buffer, so that a step can read
        # both back with a single device-to-host copy (each copy is a host synchronisation)
        self._status = torch.zeros(5, dtype=torch.int64, device=self.device)
        self._result = self._status[:4]
        self.info = self._status[4:5].view(torch.int32)[:1]
        self._profile = C.c_void_p(0)
        self.screen_cap = None       # fp32 screen: most survivors re-scored in fp64 before the plain fp64 pass takes over
        self.profile_active = True   # False: the next scoring calls record no events (bench.py samples every k-th step)

    # -- per-launch timing of the dominant kernel (bench.py) -----------------------------------------
    def enable_profile(self, capacity: int = 4096):
        p = C.c_void_p(0)
        _lib.call(self.lib.gpbo_profile_create, int(capacity), C.byref(p))
        self._profile = p

    def reset_profile(self):
        self.lib.gpbo_profile_reset(self._profile)

    def _read_profile(self, name):
        ms, n, c = C.c_double(0), C.c_int64(0), C.c_int64(0)
        _lib.call(getattr(self.lib, name), self._profile, C.byref(ms), C.byref(n), C.byref(c))
        return ms.value, n.value, c.value

    def read_profile(self):
        """(total ms, launches, candidates) summed over the recorded sigma/acquisition launches."""
        return self._read_profile("gpbo_profile_read")

    def read_profile_kstar(self):
        """(total ms, launches, candidates) of the K(X*,X) launches recorded beside the variance launches."""
        return self._read_profile("gpbo_profile_read_kstar")

    def read_profile_qei(self):
        """(total ms, launches, candidates) of the qEI launches recorded by score_qei()."""
        return self._read_profile("gpbo_profile_read_qei")

    # -- helpers -------------------------------------------------------------------------------
    def _head(self) -> tuple:
        """(X, N, Np, d, ls): the observations' run that opens the argument list of the calls on the held factorisation."""
        return self.X, self.N, self.Np, self.d, self.ls_h

    def _read(self, res_tuple) -> ScoreResult:
        """The synchronous form of what a score_async* call returned (reads the result record: synchronises)."""
        res, mu, sigma, acq = res_tuple
        v, i, n = self.read_result(res)
        return ScoreResult(v, i, n, mu, sigma, acq)

    # -- factorisation (once per BO step) ---------------------------------------------------------
    def factorise(self, X, y, ls, jitter1: float = JITTER_KERNEL, jitter2: float = JITTER_ASSEMBLY,
                  check: bool = True, order: str = "arrival", kernel: str = "se"):
        """K = k(X,X) + jitter; K = L L^T; U = L^-T; alpha = K^-1 y   (point_selector.py:79, 89-90).
        kernel: "se" (the reference's squared exponential), "matern32" or "matern52" (include/gpbo.h: GPBO_KERNEL_*; d <= 16,
        order="arrival").  score() / score_async(), kxx_host(), cov_meas_host(), cov_meas_pred_host(), loo(),
        acquisition_on_posterior() and fantasies() / score_nei() / select_nei() follow it; everything else of this class raises
        ValueError for a Matern surrogate.
        order="fps": the observations are factorised in their farthest-point order (gpbo_fps_order_f64: `bound_prefix()`
        members spread over the region the observations occupy, then the others in arrival order) instead of the order in
        which they arrived.  A GP's posterior does not depend on the order of its observations - every scoring call returns
        the same numbers within rounding - but score_bound() prunes by the FIRST observations of the factorisation, and a
        history sorted along an axis or begun inside one cluster is a poor prefix.  `perm` (device int64 [N]) maps a
        row of the factorisation to the caller's row; K / U / alpha / X / y of this object are in factorisation order
        (cov_meas_host() and observations_host() give the caller's order back)."""
        torch = self.torch
        if order not in ("arrival", "fps"):
            raise ValueError("order must be 'arrival' or 'fps'")
        kid = _lib.kernel_id(kernel)
        if kernel != "se" and order != "arrival":
            raise ValueError(f"order='fps' serves score_bound(), which is not available with kernel={kernel!r}")
        limits = [(_lib.MAX_D_ANY, f"d = {{d}} > {_lib.MAX_D_ANY} is not supported")]
        if kernel != "se":
            limits.append((_lib.MAX_D, f"kernel={kernel!r} needs d <= {_lib.MAX_D} (d = {{d}}): the any-d slow path is "
                                       "kernel='se' only"))
        Xd, yd, N, d, ls_h = self._problem(X, y, ls, limits)
        Np = int(self.lib.gpbo_padded_n(N))
        with torch.cuda.device(self.device):
            self.perm = None
            J = self.bound_prefix(Np)
            if order == "fps" and d <= _lib.MAX_D and J < N:
                # (fewer observations than one prefix, or the slow any-d kernels: the bound route is not taken anyway)
                wob = int(self.lib.gpbo_fps_order_workspace_bytes(N))
                self._workspace("_work_order", wob)
                perm = torch.empty(N, dtype=torch.int64, device=self.device)
                Xp, yp = torch.empty_like(Xd), torch.empty_like(yd)
                _lib.call(self.lib.gpbo_fps_order_f64, Xd, yd, N, d, ls_h, J, perm, Xp, yp, self._work_order, wob,
                          self._stream())
                # did the co-operative selection give up (a workgroup never scheduled) and install the arrival order?  The
                # flag stays on the device until somebody asks (order_fell_back(), last_screen): no synchronisation here
                if self._order_flag is None:
                    self._order_flag = torch.zeros(1, dtype=torch.int32, device=self.device)
                _lib.call(self.lib.gpbo_fps_order_status, self._work_order, N, self._order_flag, self._stream())
                Xd, yd, self.perm = Xp, yp, perm
            self.X, self.y, self.ls_h = Xd, yd, ls_h
            self.N, self.Np, self.d = N, Np, d
            self.jitter1, self.jitter2 = float(jitter1), float(jitter2)
            self.kernel = kernel
            self._owns_xy = False
            self.n_appended = 0  # columns of U built by append() since the last full factorisation
            self._epoch += 1
            if self.K is None or self.K.shape[0] != Np or self.U.shape[0] != Np:
                # the factor buffers (and the workspace) are kept from step to step: a BO loop refactorises
                # at the same padded size many times, and fresh 100-MB allocations cost more than the kernels
                self.K = torch.empty((Np, Np), dtype=torch.float64, device=self.device)
                self.U = torch.empty((Np, Np), dtype=torch.float64, device=self.device)
                self.alpha = torch.empty(Np, dtype=torch.float64, device=self.device)
                self._work_fact = None
            self._u32_valid = False
            self._u8_valid = False
            self._factorise_into(Xd, yd, N, d, ls_h, kid, jitter1, jitter2, Np, self.K, self.U, self.alpha, self.info)
            if check:
                info = int(self.info.item())  # synchronises
                if info != 0:
                    # the failing pivot as a row of the CALLER's arrays (gpbo_select_next_host_f64 reports the same row)
                    row = info if self.perm is None or info > N else int(self.perm[info - 1].item()) + 1
                    raise np.linalg.LinAlgError(
                        f"covariance matrix is not positive definite (pivot {row} of {N}); "
                        "the reference's np.linalg.inv would raise or return garbage here")
        return self

    BOUND_PREFIX_FRACTION = 16  # first pass over the first Np / 16 observations' columns (1/256 of the variance product);
                                # survivors get a second bound from four times as many before the fp64 kernels see them

    BOUND_MIN_JITTER = 1e-6     # score_bound(): smallest jitter1 + jitter2 the route is taken for (see score_async_bound)

    def bound_prefix(self, Np: Optional[int] = None) -> int:
        """First-level prefix length of score_bound() at this padded size (= the farthest-point members of order="fps")."""
        Np = self.Np if Np is None else int(Np)
        return max(128, (Np // self.BOUND_PREFIX_FRACTION) // 128 * 128)

    @property
    def order(self) -> str:
        return "arrival" if self.perm is None else "fps"

    def order_fell_back(self) -> bool:
        """True when factorise(order="fps") came back with the ARRIVAL order because the co-operative selection gave up (one of
        its workgroups was never scheduled: bounded waits, csrc/subset.hip).  Exact either way - but candidate shards of one
        step must hold the same factorisation, so PointSelector votes on this flag.  Reads one device word (synchronises)."""
        if self.perm is None or self._order_flag is None:
            return False
        return bool(int(self._order_flag.item()))

    def _perm_host(self):
        return None if self.perm is None else self.perm[: self.N].cpu().numpy()

    def observations_host(self):
        """(X [N x d], y [N]) in the CALLER's order (rows appended since the factorisation come last in both orders)."""
        Xf, yf = self.X[: self.N].cpu().numpy(), self.y[: self.N].cpu().numpy()
        p = self._perm_host()
        if p is None:
            return Xf, yf
        Xa, ya = np.empty_like(Xf), np.empty_like(yf)
        Xa[p], ya[p] = Xf, yf
        return Xa, ya

    def _need_unrolled_d(self, what: str):
        """d > 16 runs on the slow any-d kernels, which serve factorise() and score() only (point_selector.py:22: the
        reference's class takes any feature count; its call path is exactly those two)."""
        if self.d > _lib.MAX_D:
            raise ValueError(f"{what} needs d <= {_lib.MAX_D} (d = {self.d}): beyond that only factorise() and the plain fp64 "
                             "score() are available")

    # -- one more observation without refactorising ---------------------------------
    def _grow(self, Np_new: int):
        """Re-pad the factors into [Np_new x Np_new] buffers (identity on the new part of the diagonal)."""
        torch = self.torch
        Np = self.Np
        for name in ("K", "U"):
            old = getattr(self, name)
            new = torch.zeros((Np_new, Np_new), dtype=torch.float64, device=self.device)
            new[:Np, :Np] = old
            new.diagonal()[Np:] = 1.0
            setattr(self, name, new)
        alpha = torch.zeros(Np_new, dtype=torch.float64, device=self.device)
        alpha[:Np] = self.alpha
        self.alpha = alpha
        self.Np = Np_new
        self._work_post = None

    def append(self, x_new, y_new, check: bool = True):
        """Add one observation to the factorised surrogate in O(N^2): column N of U, alpha recomputed.
        The length scales and jitters stay those of the last factorise() - the caller decides when they may
        (the reference re-tunes them every iteration, point_selector.py:60-62, and then a full factorise() is due).
        An appended column goes through the explicit inverse factor (l = U^T k), so it carries cond(L) eps of
        relative error where the blocked Cholesky is backward stable: `n_appended` counts the columns built this way
        since the last full factorisation, for callers that want to refresh after a while (PointSelector does)."""
        need_se(self.kernel, "append()")
        self._need_unrolled_d("append()")
        torch = self.torch
        if self.N < 1:
            raise _lib.GpboError("append() needs a factorised surrogate")
        xn = self._dev(x_new).reshape(-1)
        if xn.numel() != self.d:
            raise ValueError(f"x_new: expected {self.d} coordinates, got {xn.numel()}")
        yn = self._dev(np.asarray([float(y_new)])) if not isinstance(y_new, torch.Tensor) else self._dev(y_new).reshape(-1)[:1]
        with torch.cuda.device(self.device):
            N = self.N
            if N + 1 > self.Np:
                self._grow(int(self.lib.gpbo_padded_n(N + 1)))
            if not self._owns_xy or self.X.shape[0] < N + 1:
                # private, padded copies: the caller's X / y tensors are never written to
                Xb = torch.zeros((self.Np, self.d), dtype=torch.float64, device=self.device)
                yb = torch.zeros(self.Np, dtype=torch.float64, device=self.device)
                Xb[:N] = self.X[:N]
                yb[:N] = self.y[:N]
                self.X, self.y, self._owns_xy = Xb, yb, True
            wbytes = int(self.lib.gpbo_append_workspace_bytes(self.Np))
            work = torch.empty(wbytes // 8, dtype=torch.float64, device=self.device)
            _lib.call(self.lib.gpbo_append_f64, self.X, self.y, N, self.d, self.ls_h, self.jitter1, self.jitter2, self.Np,
                      xn, yn, self.K, self.U, self.alpha, self.info, work, wbytes, self._stream())
            self._u32_valid = False
            self._u8_valid = False
            if check:
                info = int(self.info.item())  # synchronises
                if info != 0:
                    raise np.linalg.LinAlgError(
                        f"appended observation makes the covariance matrix numerically singular (pivot {info}); "
                        "call factorise() on the full data instead")
            else:
                torch.cuda.current_stream(self.device).synchronize()  # xn / yn / work must outlive the kernels
            if self.perm is not None:   # the new row is last in both orders
                self.perm = torch.cat([self.perm[:N], torch.tensor([N], dtype=torch.int64, device=self.device)])
            self.N = N + 1
            self.n_appended += 1
            self._epoch += 1
            del work
        return self

    # -- persistence across jobs: the DAG's select_parameters jobs are separate processes --------------------
    def state_dict(self) -> dict:
        """Host copy of everything append()/score() need (the N x N part of the factors, not the padding)."""
        need_se(self.kernel, "state_dict()")
        N = self.N
        st = dict(version=1, N=N, d=self.d, ls=np.array(self.ls_h), jitter1=self.jitter1, jitter2=self.jitter2,
                  n_appended=self.n_appended,
                  X=self.X[:N].cpu().numpy(), y=self.y[:N].cpu().numpy(), K=self.K[:N, :N].cpu().numpy(),
                  U=self.U[:N, :N].cpu().numpy(), alpha=self.alpha[:N].cpu().numpy())
        if self.perm is not None:   # everything above is in factorisation order; perm[i] = the caller's row of row i
            st["perm"] = self._perm_host()
        return st

    def load_state_dict(self, st: dict):
        need_se(self.kernel, "load_state_dict()")
        torch = self.torch
        if int(st.get("version", 0)) != 1:
            raise ValueError("unknown surrogate state version")
        N, d = int(st["N"]), int(st["d"])
        Np = int(self.lib.gpbo_padded_n(N))
        with torch.cuda.device(self.device):
            self.N, self.Np, self.d = N, Np, d
            self._epoch += 1
            self.ls_h = np.ascontiguousarray(np.asarray(st["ls"], dtype=np.float64).reshape(-1))
            self.jitter1, self.jitter2 = float(st["jitter1"]), float(st["jitter2"])
            self.n_appended = int(st["n_appended"]) if "n_appended" in st else 0
            self.X = torch.zeros((Np, d), dtype=torch.float64, device=self.device)
            self.y = torch.zeros(Np, dtype=torch.float64, device=self.device)
            self.X[:N] = self._dev(st["X"])
            self.y[:N] = self._dev(st["y"]).reshape(-1)
            self._owns_xy = True
            for name in ("K", "U"):
                m = torch.zeros((Np, Np), dtype=torch.float64, device=self.device)
                m[:N, :N] = self._dev(st[name])
                m.diagonal()[N:] = 1.0
                setattr(self, name, m)
            self.alpha = torch.zeros(Np, dtype=torch.float64, device=self.device)
            self.alpha[:N] = self._dev(st["alpha"]).reshape(-1)
            self.info.zero_()
            self.perm = None
            if "perm" in st and st["perm"] is not None:
                p = np.ascontiguousarray(np.asarray(st["perm"], dtype=np.int64).reshape(-1))
                if p.size != N or not np.array_equal(np.sort(p), np.arange(N)):
                    raise ValueError("surrogate state: perm is not a permutation of the observations")
                self.perm = torch.from_numpy(p).to(self.device)
            self._u32_valid = False
            self._u8_valid = False
            self._work_post = None
        return self

    def save_state(self, path: str):
        """Atomic: written to a temporary file in the same directory and renamed over `path`, so a job killed
        mid-write (or a concurrent reader) never sees a torn file."""
        import os
        import tempfile

        need_se(self.kernel, "save_state()")
        path = str(path)
        if not path.endswith(".npz"):
            path += ".npz"  # what np.savez would have appended
        fd, tmp = tempfile.mkstemp(prefix=".gpbo_state_", suffix=".tmp", dir=os.path.dirname(os.path.abspath(path)))
        try:
            with os.fdopen(fd, "wb") as f:
                np.savez(f, **self.state_dict())
            # mkstemp creates 0600; np.savez(path) honoured the umask - a follow-up job under another account of the
            # group must still be able to read the state, as it could before the atomic rename was introduced
            um = os.umask(0)
            os.umask(um)
            os.chmod(tmp, 0o666 & ~um)
            os.replace(tmp, path)
        except BaseException:
            if os.path.exists(tmp):
                os.unlink(tmp)
            raise

    def load_state(self, path: str):
        need_se(self.kernel, "load_state()")
        with np.load(path) as z:
            return self.load_state_dict({k: z[k] for k in z.files})

    # -- scoring ------------------------------------------------------------------------------------
    def _ensure_post_workspace(self, M):
        chunk = self._chunk_for(M)
        need = int(self.lib.gpbo_posterior_workspace_bytes(self.Np, chunk, M))
        self._workspace("_work_post", need)
        return chunk, need

    def score_async(self, Xs, acquisition: str = "lcb", explore: float = 4.0, f_best: Optional[float] = None,
                    xi: float = 0.0, dense: bool = False, idx_offset: int = 0, diag_add: float = 0.0,
                    prior_var: float = PRIOR_VAR):
        """Enqueue K(X*,X) + mu + sigma + acquisition + arg-max for all rows of Xs; no host sync.
        Returns (result_tensor[int64 x4 on device], mu, sigma, acq)."""
        torch = self.torch
        Xsd, M = self._candidates(Xs)
        kind, p0, p1 = acq_params(acquisition, explore, f_best, xi)
        if diag_add != 0.0 and self.perm is not None:
            # the N == M quirk (point_selector.py:173) adds to entry (i, i) of k(X, X*): candidate i against the caller's
            # observation i, which is not row i of a permuted factorisation
            raise ValueError("diag_add (the N == M shape quirk) needs factorise(order='arrival')")
        if diag_add != 0.0 and self.kernel != "se":
            raise ValueError(f"diag_add (the N == M shape quirk of the reference's kernel_rbf) is not available with "
                             f"kernel={self.kernel!r}")
        with torch.cuda.device(self.device):
            chunk, wbytes = self._ensure_post_workspace(M)
            mu, sigma, acq = self._dense(M, dense)
            _lib.call(self.lib.gpbo_posterior_acq_kern_f64, Xsd, M, *self._head(), self._kid(), self.U, self.alpha,
                      prior_var, kind, p0, p1, float(diag_add), int(idx_offset), chunk, mu, sigma, acq, self._result,
                      self._work_post, wbytes, self._profile if self.profile_active else None, self._stream())
        self._keep = Xsd  # keep the candidate tensor alive until the stream has consumed it
        return self._result, mu, sigma, acq

    # -- fp32-screened scoring (BASELINE config 4): fp32 variance product for all, fp64 re-score of the survivors ----
    SCREEN_TAU0 = 1e-4          # first guess of |var64 - var32|; checked and raised per call (gpbo_rescore_f64)
    SCREEN_SAMPLE = 1024        # about this many evenly strided non-survivors are re-scored as well, to check tau
    SCREEN_CHUNK64 = 1 << 14    # candidates per fp64 launch of the re-scoring

    def prepare_f32(self):
        """Round U to fp32 (re-padded to a multiple of 256) for the fp32 variance screen."""
        torch = self.torch
        Np32 = int(self.lib.gpbo_padded_n_f32(self.N))
        with torch.cuda.device(self.device):
            if self.U32 is None or self.U32.shape[0] != Np32:
                self.U32 = torch.empty((Np32, Np32), dtype=torch.float32, device=self.device)
            _lib.call(self.lib.gpbo_prepare_f32, self.U, None, self.Np, self.U32, None, Np32, self._stream())
        self.Np32 = Np32
        self._u32_valid = True
        return self

    def prepare_i8(self):
        """Column scales and int8 MFMA fragments of U for the int8-sliced variance screen (once per factorisation)."""
        torch = self.torch
        if self.Np > _lib.I8_MAX_N:
            raise _lib.GpboError(f"the int8-sliced screen needs N <= {_lib.I8_MAX_N} (int32 accumulators)")
        with torch.cuda.device(self.device):
            need = int(self.lib.gpbo_prepare_i8_bytes(self.Np))
            if need < 0:
                raise _lib.GpboError("gpbo_prepare_i8_bytes: invalid size")
            if self.U8 is None or self.U8.numel() < need:
                self.U8 = torch.empty(need, dtype=torch.uint8, device=self.device)
            _lib.call(self.lib.gpbo_prepare_i8, self.U, self.Np, self.U8, need, self._stream())
        self._u8_valid = True
        return self

    SCREEN_TAU0_I8 = 1e-9       # int8-sliced screen: |var64 - var_i8| is ~1e-11; checked per call like the fp32 one
    SCREEN_TAU0_I8C = 1e-3      # coarse int8 screen (three digits per operand): |var64 - var| ~ 2e-4 at N = 4096

    def _score_screened(self, mode, Xs, acquisition, explore, f_best, xi, dense, idx_offset, diag_add, prior_var):
        """A reduced-cost pass over all rows of Xs (mode "f32": fp32 matrix cores; "i8": int8 slices on the integer
        matrix cores), then the fp64 decision (gpbo_rescore_f64): the result record holds the fp64 kernels' maximum and
        its lowest index.  Dense outputs (mu exactly the fp64 path's; sigma / acq with the screen's variance) are
        float64 tensors.  Unlike score_async this call synchronises (the survivor count is read back).
        `last_screen` keeps the statistics of the call."""
        need_se(self.kernel, f"the {mode} screen (score_{mode}())")
        self._need_unrolled_d(f"the {mode} screen")
        torch = self.torch
        Xsd, M = self._candidates(Xs)
        kind, p0, p1 = acq_params(acquisition, explore, f_best, xi)
        if diag_add != 0.0:
            # N == M shape quirk (point_selector.py:173): gathered rows lose the index the quirk is keyed on
            self.last_screen = dict(fallback=True, reason="diag_add")
            return self.score_async(Xsd, acquisition, explore, f_best, xi, dense, idx_offset, diag_add, prior_var)
        if mode == "f32" and (not self._u32_valid or self.U32 is None):
            self.prepare_f32()
        if mode in ("i8", "i8c") and (not self._u8_valid or self.U8 is None):
            self.prepare_i8()
        with torch.cuda.device(self.device):
            if self._screen_mu is None or self._screen_mu.numel() < M:
                self._screen_mu = torch.empty(M, dtype=torch.float64, device=self.device)
                self._screen_var = torch.empty(M, dtype=torch.float64, device=self.device)
            mu, sigma, acq = self._dense(M, dense)
            mu_w = mu if dense else self._screen_mu
            prof = self._profile if self.profile_active else None
            if mode == "f32":
                chunk = self._chunk_for(M, 1024)
                need = int(self.lib.gpbo_posterior_workspace_bytes_f32(self.Np32, chunk, M))
            else:
                chunk = self._chunk_for(M)
                need = int(self.lib.gpbo_posterior_workspace_bytes_i8(self.Np, chunk, M))
            self._workspace("_work_screen", need, free_first=True)
            if mode == "f32":
                _lib.call(self.lib.gpbo_posterior_acq_f32, Xsd, M, self.X, self.N, self.Np32, self.d, self.ls_h, self.U32,
                          self.alpha, prior_var, kind, p0, p1, 0.0, int(idx_offset), chunk, mu_w, sigma, acq,
                          self._screen_var, self._result, self._work_screen, need, prof, self._stream())
                tau0 = float(self.SCREEN_TAU0)
            else:
                fn = self.lib.gpbo_posterior_acq_i8c if mode == "i8c" else self.lib.gpbo_posterior_acq_i8
                _lib.call(fn, Xsd, M, *self._head(), self.U8, self.alpha, prior_var, kind, p0, p1, int(idx_offset), chunk,
                          mu_w, sigma, acq, self._screen_var, self._result, self._work_screen, need, prof, self._stream())
                tau0 = float(self.SCREEN_TAU0_I8C if mode == "i8c" else self.SCREEN_TAU0_I8)
            cap = self.screen_cap if self.screen_cap else max(4096, min(M, max(M // 16, 1 << 16)))
            chunk64 = self.SCREEN_CHUNK64
            rbytes = int(self.lib.gpbo_rescore_workspace_bytes(self.Np, cap, chunk64))
            self._workspace("_work_rescore", rbytes)
            stats = _lib.ScreenStats()
            stride = max(1, M // self.SCREEN_SAMPLE)
            _lib.call(self.lib.gpbo_rescore_f64, Xsd, M, mu_w, self._screen_var, *self._head(), self.U, self.alpha,
                      prior_var, kind, p0, p1, int(idx_offset), tau0, stride, cap, chunk64, self._result, C.byref(stats),
                      self._work_rescore, rbytes, self._stream())
            self.last_screen = dict(mode=mode, survivors=int(stats.survivors), rescored=int(stats.rescored),
                                    rounds=int(stats.rounds), fallback=bool(stats.fallback), tau=float(stats.tau),
                                    err_max=float(stats.err_max), candidates=M)
        self._keep = Xsd
        if stats.fallback:
            # too many candidates could still be the maximum (or tau did not settle): the plain fp64 pass decides
            return self.score_async(Xsd, acquisition, explore, f_best, xi, dense, idx_offset, 0.0, prior_var)
        return self._result, mu, sigma, acq

    def score_async_f32(self, Xs, acquisition: str = "lcb", explore: float = 4.0, f_best: Optional[float] = None,
                        xi: float = 0.0, dense: bool = False, idx_offset: int = 0, diag_add: float = 0.0,
                        prior_var: float = PRIOR_VAR):
        """fp32 variance screen + fp64 decision (BASELINE config 4); see _score_screened."""
        return self._score_screened("f32", Xs, acquisition, explore, f_best, xi, dense, idx_offset, diag_add, prior_var)

    def score_async_i8(self, Xs, acquisition: str = "lcb", explore: float = 4.0, f_best: Optional[float] = None,
                       xi: float = 0.0, dense: bool = False, idx_offset: int = 0, diag_add: float = 0.0,
                       prior_var: float = PRIOR_VAR):
        """int8-sliced variance screen (|dsigma| ~ 1e-10) + fp64 decision; see _score_screened."""
        return self._score_screened("i8", Xs, acquisition, explore, f_best, xi, dense, idx_offset, diag_add, prior_var)

    def score_i8(self, Xs, **kw) -> ScoreResult:
        return self._read(self.score_async_i8(Xs, **kw))

    def score_async_i8c(self, Xs, acquisition: str = "lcb", explore: float = 4.0, f_best: Optional[float] = None,
                        xi: float = 0.0, dense: bool = False, idx_offset: int = 0, diag_add: float = 0.0,
                        prior_var: float = PRIOR_VAR):
        """Coarse int8 screen (three digits per operand, six slice products, |dsigma^2| ~ 2e-4) + fp64 decision: the
        cheapest pass that still leaves only a handful of candidates for the fp64 kernels; see _score_screened."""
        return self._score_screened("i8c", Xs, acquisition, explore, f_best, xi, dense, idx_offset, diag_add, prior_var)

    def score_i8c(self, Xs, **kw) -> ScoreResult:
        return self._read(self.score_async_i8c(Xs, **kw))

    def score_f32(self, Xs, **kw) -> ScoreResult:
        return self._read(self.score_async_f32(Xs, **kw))

    # -- prefix-bound screen: exact branch and bound, all fp64 ---------------------------------------------------
    ARD_KEEP_WORKSPACE_BYTES = 1 << 28   # the batched ARD workspace is dropped after a call when larger than this
    def score_async_bound(self, Xs, acquisition: str = "lcb", explore: float = 4.0, f_best: Optional[float] = None,
                          xi: float = 0.0, dense: bool = False, idx_offset: int = 0, diag_add: float = 0.0,
                          prior_var: float = PRIOR_VAR, prefix: Optional[int] = None, prefix2: Optional[int] = None):
        """The selected point WITHOUT the variance of every candidate - exact, all fp64.  The squared norm of the first J
        components of v_c = U^T k_c is the variance reduction from the first J observations alone, so
        sqrt(prior_var - |v_c[:J]|^2) >= cov_func_c and (both acquisitions increase with sigma) an UPPER bound of the
        acquisition follows at (J / N)^2 of the cost.  Candidates whose bound is below the best exact value of a sample
        cannot be the maximum nor tie with it; the others go through the fp64 kernels, which decide
        (gpbo_posterior_prefix_f64 + gpbo_bound_select_f64).  The mean is still computed for every candidate.
        Falls back to score_async when the bound cannot be used (dense outputs wanted, LCB with a negative weight, the
        N == M diagonal quirk, fewer than 3 column blocks) or does not separate the candidates (flat mean, ties).
        "The first J observations" are those of THIS object's factorisation: factorise(order="fps") puts J well-spread
        members first, so that the pruning does not depend on the order in which the observations arrived; with the
        default order the literal arrival prefix is used (exact as well; prunes little when the history is sorted or
        clustered).  Bounds and exact values come from the same U, the same K(X*,X) kernel and the same variance
        kernel: |v[:J]|^2 is a partial sum of the squares score() adds up.
        Synchronises; `last_screen` keeps the statistics."""
        need_se(self.kernel, "score_bound()")
        torch = self.torch
        if self.d > _lib.MAX_D:   # the slow any-d kernels serve the plain pass only
            self.last_screen = dict(mode="bound", fallback=True, reason="d > 16")
            return self.score_async(Xs, acquisition, explore, f_best, xi, dense, idx_offset, diag_add, prior_var)
        Xsd, M = self._candidates(Xs)
        kind, p0, p1 = acq_params(acquisition, explore, f_best, xi)
        J = int(prefix) if prefix else self.bound_prefix()
        J2 = int(prefix2) if prefix2 is not None else (4 * J if 8 * J <= self.Np else 0)   # second level: survivors only
        reason = None
        if dense:
            reason = "dense outputs"
        elif diag_add != 0.0:
            reason = "diag_add"
        elif kind == _lib.ACQ_LCB and not p0 >= 0.0:
            reason = "negative explore weight"
        elif J % 128 or J < 128 or 2 * J > self.Np:
            reason = "too few column blocks"
        elif not (self.jitter1 + self.jitter2 >= self.BOUND_MIN_JITTER
                  and prior_var >= (1.0 + self.jitter1) + self.jitter2 - 1e-15):
            # The plain pass takes sqrt(|var|) (point_selector.py:98): a NEGATIVE computed variance counts by its magnitude,
            # which no prefix can bound.  With K = k(X,X) + tau I and prior_var >= 1 + tau the true variance is >= tau
            # (a candidate on top of an observation: 2 tau - tau^2 (K^-1)_ii), so the computed one is negative only if its
            # rounding error exceeds tau; the route is taken for tau >= 1e-6 (the reference: 1.01e-4, errors seen: 1e-9).
            reason = "jitter too small for the |var| rule"
        if reason:
            self.last_screen = dict(mode="bound", fallback=True, reason=reason)
            return self.score_async(Xsd, acquisition, explore, f_best, xi, dense, idx_offset, diag_add, prior_var)
        with torch.cuda.device(self.device):
            chunk, wbytes = self._ensure_post_workspace(M)
            if self._bound_ub is None or self._bound_ub.numel() < M:
                self._bound_ub = torch.empty(M, dtype=torch.float64, device=self.device)
            _lib.call(self.lib.gpbo_posterior_prefix_f64, Xsd, M, *self._head(), self.U, self.alpha, prior_var, kind, p0, p1,
                      int(idx_offset), chunk, J, None, None, self._bound_ub, self._result, self._work_post, wbytes,
                      self._profile if self.profile_active else None, self._stream())
            # every first-level survivor may go on to the second-level bound (N/4 rows: 1/16 of a plain pass per candidate -
            # cheaper than falling back even if ALL of them survive); LCB(explore=10) on the headline workload leaves 256k
            # of 2^21: 24 ms through the second level against 518 ms through the plain pass (tools/bound_cap_probe.py)
            cap = self.screen_cap if self.screen_cap else max(4096, M)
            chunk64 = self.SCREEN_CHUNK64
            rbytes = int(self.lib.gpbo_rescore_workspace_bytes(self.Np, cap, chunk64))
            self._workspace("_work_rescore", rbytes)
            stats = _lib.ScreenStats()
            stride = max(1, M // self.SCREEN_SAMPLE)
            _lib.call(self.lib.gpbo_bound_select_f64, Xsd, M, self._bound_ub, *self._head(), self.U, self.alpha, prior_var,
                      kind, p0, p1, int(idx_offset), stride, cap, chunk64, J2, self._result, C.byref(stats),
                      self._work_rescore, rbytes, self._stream())
            self.last_screen = dict(mode="bound", order="arrival (fps fell back)" if self.order_fell_back() else self.order, prefix=J, prefix2=J2, survivors=int(stats.survivors),
                                    rescored=int(stats.rescored), rounds=int(stats.rounds), fallback=bool(stats.fallback),
                                    threshold=float(stats.tau), candidates=M)
        self._keep = Xsd
        if stats.fallback:
            return self.score_async(Xsd, acquisition, explore, f_best, xi, False, idx_offset, 0.0, prior_var)
        return self._result, None, None, None

    def score_bound(self, Xs, **kw) -> ScoreResult:
        return self._read(self.score_async_bound(Xs, **kw))

    # -- q = 8 Monte-Carlo Expected Improvement (BASELINE config 5) ---------------------------------------
    def score_qei_async(self, Xs, Z, f_best: float, xi: float = 0.0, dense: bool = False, batch_offset: int = 0,
                        prior_var: float = PRIOR_VAR):
        """Enqueue qEI over consecutive batches of 8 rows of Xs; Z = [S x 8] base samples; no host sync.
        Returns (result_tensor, qei or None); the result's best_idx is a BATCH index.
        Z must be finite: a host array is checked here, a device tensor is the caller's (the kernel skips the improvements
        a NaN sample makes NaN instead of reporting them: DESIGN.md 1, "qEI and NaN")."""
        need_se(self.kernel, "score_qei()")
        self._need_unrolled_d("qEI")
        torch = self.torch
        if isinstance(Z, np.ndarray) and not np.isfinite(Z).all():
            raise ValueError("qEI needs finite base samples Z")
        Xsd, Zd = self._dev(Xs), self._dev(Z)
        M, S = int(Xsd.shape[0]), int(Zd.shape[0])
        if M % 8 or int(Zd.shape[1]) != 8:
            raise ValueError("qEI needs M % 8 == 0 and base samples of shape (S, 8)")
        with torch.cuda.device(self.device):
            chunk = self._chunk_for(M)
            need = int(self.lib.gpbo_qei_workspace_bytes(self.Np, chunk, M))
            self._workspace("_work_qei", need)
            qei = torch.empty(M // 8, dtype=torch.float64, device=self.device) if dense else None
            _lib.call(self.lib.gpbo_posterior_qei_f64, Xsd, M, *self._head(), self.U, self.alpha, prior_var, float(f_best),
                      float(xi), Zd, S, int(batch_offset), chunk, qei, self._result, self._work_qei, need,
                      self._profile if self.profile_active else None, self._stream())
        self._keep = (Xsd, Zd)
        return self._result, qei

    def score_qei(self, Xs, Z, f_best: float, xi: float = 0.0, dense: bool = False, batch_offset: int = 0,
                  prior_var: float = PRIOR_VAR) -> ScoreResult:
        """qEI over consecutive batches of 8 rows of Xs; Z = [S x 8] base samples.  best_idx is a BATCH index."""
        res, qei = self.score_qei_async(Xs, Z, f_best, xi, dense, batch_offset, prior_var)
        v, i, n = self.read_result(res)
        return ScoreResult(v, i, n, None, None, qei)

    # -- greedy q-point batch by rank-one posterior updates (csrc/batch.hip) -------------------------
    def select_batch_on_posterior(self, Xs, mu, sigma, q: int, acquisition: str = "lcb", explore: float = 4.0,
                                  f_best: Optional[float] = None, xi: float = 0.0, fantasy: str = "believer",
                                  lie: Optional[float] = None, idx_offset: int = 0,
                                  prior_var: float = PRIOR_VAR) -> BatchResult:
        """The batch from dense device mu / sigma [M] of THIS surrogate at the rows of Xs (score(dense=True) without
        diag_add).  mu / sigma are updated in place: they leave as the posterior the q-th member was chosen from.
        One read-back (synchronises).  This is the call for a posterior the caller already holds on the device
        (PointSelector after update_surrogate()); select_batch() runs the plain pass first and then this.
        prior_var must be the one mu / sigma were scored with.
        EI keeps the f_best it is given for the whole batch: with fantasy="liar" and lie < f_best the later members are still
        scored against f_best, not against the lie (the NumPy reference of the tests, tests/batch_ref.py, does the same).
        A caller who wants the lie to count as the incumbent passes f_best = min(f_best, lie)."""
        need_se(self.kernel, "select_batch_on_posterior()")
        self._need_unrolled_d("select_batch()")
        torch = self.torch
        Xsd, M = self._candidates(Xs)
        q = int(q)
        if not 1 <= q <= min(_lib.BATCH_MAX_Q, M):
            raise ValueError(f"q must be in [1, min({_lib.BATCH_MAX_Q}, M = {M})], got {q}")
        kind, p0, p1 = acq_params(acquisition, explore, f_best, xi)
        fkind, fl = fantasy_params(fantasy, lie)
        for name, t in (("mu", mu), ("sigma", sigma)):
            if not (isinstance(t, torch.Tensor) and t.dtype == torch.float64 and t.is_contiguous() and t.numel() == M
                    and t.device == self.device):
                raise ValueError(f"{name} must be a contiguous fp64 tensor of {M} values on {self.device}")
        with torch.cuda.device(self.device):
            need = int(self.lib.gpbo_batch_workspace_bytes(self.Np, M, q))
            work = self._workspace("_work_batch", need)
            # members, values, the result record and the info word in one buffer: one device-to-host copy
            out = torch.zeros(2 * q + 5, dtype=torch.int64, device=self.device)
            idx, val, res, info = out[:q], out[q: 2 * q], out[2 * q: 2 * q + 4], out[2 * q + 4:]
            _lib.call(self.lib.gpbo_select_batch_f64, Xsd, M, *self._head(), self.U, self.alpha, self.jitter1, self.jitter2,
                      float(prior_var), kind, p0, p1, q, fkind, fl, mu, sigma, int(idx_offset), idx, val, res, info, work,
                      need, self._stream())
            h = out.cpu()   # synchronises: Xsd has been consumed
        return BatchResult(indices=h[:q].numpy().copy(), values=h[q: 2 * q].view(torch.float64).numpy().copy(),
                           nan_count=int(h[2 * q + 2]), info=int(h[2 * q + 4:].view(torch.int32)[0]), mu=mu, sigma=sigma)

    def select_batch(self, Xs, q: int, acquisition: str = "lcb", explore: float = 4.0, f_best: Optional[float] = None,
                     xi: float = 0.0, fantasy: str = "believer", lie: Optional[float] = None, idx_offset: int = 0,
                     diag_add: float = 0.0, prior_var: float = PRIOR_VAR) -> BatchResult:
        """q candidates to evaluate in parallel, chosen greedily: the first is score()'s, each further one the arg-max
        after conditioning the surrogate on a fantasy observation at the one before it - its current mean
        (fantasy="believer": Kriging believer, GP-BUCB under LCB) or the constant `lie` (fantasy="liar") - with the members
        chosen so far excluded.  Runs the dense plain pass, then gpbo_select_batch_f64: per member N kernel entries per
        candidate instead of the N^2 of a pass after append().  The factorisation (U, alpha, N) is not touched.
        d <= 16; not with the N == M shape quirk (diag_add)."""
        need_se(self.kernel, "select_batch()")
        if diag_add != 0.0:
            raise ValueError("select_batch() does not support diag_add (the N == M shape quirk)")
        self._need_unrolled_d("select_batch()")
        Xsd, M = self._candidates(Xs)
        fantasy_params(fantasy, lie)   # (refused before the N^2 pass is spent)
        if not 1 <= int(q) <= min(_lib.BATCH_MAX_Q, M):
            raise ValueError(f"q must be in [1, min({_lib.BATCH_MAX_Q}, M = {M})], got {q}")
        _, mu, sigma, _ = self.score_async(Xsd, acquisition, explore, f_best, xi, dense=True, idx_offset=idx_offset,
                                           prior_var=prior_var)
        return self.select_batch_on_posterior(Xsd, mu, sigma, q, acquisition, explore, f_best, xi, fantasy, lie, idx_offset,
                                              prior_var)

    # -- Thompson sampling by pathwise posterior samples (csrc/thompson.hip) ---------------------------
    def thompson_paths(self, n_paths: int, n_features: int = 2048, seed: int = 0) -> ThompsonPaths:
        """n_paths samples of the posterior FUNCTION (pathwise conditioning: a random-Fourier-feature draw of the prior plus
        the mean's own sum with v_s = K^-1 (y - g_s(X) - sqrt(kappa) E[s]) in the place of alpha).  The draws are
        thompson.thompson_draws(d, n_features, n_paths, N, seed); the columns of E follow the CALLER's order of the
        observations, so a seed gives the same paths under factorise(order="fps").  gpbo_thompson_weights_f64: enqueues
        only.  The paths stay valid until the next factorise() / append() / load_state_dict()."""
        from .thompson import path_params, thompson_draws

        need_se(self.kernel, "thompson_paths()")
        n_paths, n_features, seed = path_params(n_paths, n_features, seed)
        self._need_unrolled_d("thompson_paths()")
        if self.N < 1:
            raise _lib.GpboError("thompson_paths() needs a factorised surrogate")
        torch = self.torch
        omega, phase, W, E = thompson_draws(self.d, n_features, n_paths, self.N, seed)
        p = self._perm_host()
        if p is not None:
            E = E[:, p]   # row i of the factorisation is the caller's row p[i]
        with torch.cuda.device(self.device):
            om, ph, Wd, Ed = self._dev(omega), self._dev(phase), self._dev(W), self._dev(E)
            V = torch.empty((n_paths, self.Np), dtype=torch.float64, device=self.device)
            need = int(self.lib.gpbo_thompson_weights_workspace_bytes(self.Np, n_features, n_paths))
            work = self._workspace("_work_thompson", need)
            _lib.call(self.lib.gpbo_thompson_weights_f64, self.X, self.y, self.N, self.Np, self.d, self.ls_h, self.U,
                      self.jitter1, self.jitter2, om, ph, Wd, Ed, n_features, n_paths, V, work, need, self._stream())
        self._keep = Ed   # alive until the stream has consumed it
        return ThompsonPaths(om, ph, Wd, V, n_paths, n_features, seed, (id(self), self._epoch))

    def thompson_score(self, paths: ThompsonPaths, Xs, dense: bool = False, idx_offset: int = 0) -> ThompsonResult:
        """Every path at the rows of Xs in one launch (gpbo_thompson_paths_f64): per path the lowest row minimising it, the
        acquisition -f_s there and, with dense=True, the paths themselves [n_paths x M] on the device.  One read-back
        (synchronises).  IndexError when a value is NaN (a candidate with a non-finite coordinate), as the other
        acquisitions raise."""
        need_se(self.kernel, "thompson_score()")
        self._need_unrolled_d("thompson_score()")
        if not isinstance(paths, ThompsonPaths) or paths.epoch != (id(self), self._epoch):
            raise ValueError("these sample paths do not belong to the surrogate as it is now: call thompson_paths() again "
                             "after factorise() / append()")
        torch = self.torch
        Xsd, M = self._candidates(Xs)
        S, F = paths.n_paths, paths.n_features
        with torch.cuda.device(self.device):
            need = int(self.lib.gpbo_thompson_paths_workspace_bytes(self.Np, M, F, S))
            work = self._workspace("_work_thompson", need)
            f = torch.empty((S, M), dtype=torch.float64, device=self.device) if dense else None
            out = torch.zeros(3 * S, dtype=torch.int64, device=self.device)   # indices | values | NaN counts: one copy
            _lib.call(self.lib.gpbo_thompson_paths_f64, Xsd, M, *self._head(), paths.omega, paths.phase, paths.W, paths.V, F,
                      S, int(idx_offset), f, M, out[:S], out[S: 2 * S], out[2 * S:], work, need, self._stream())
            h = out.cpu()   # synchronises: Xsd has been consumed
        res = ThompsonResult(indices=h[:S].numpy().copy(), values=h[S: 2 * S].view(torch.float64).numpy().copy(),
                             nan_counts=h[2 * S:].numpy().copy(), f=f)
        if res.nan_counts.any():
            raise IndexError(NAN_ACQUISITION)
        return res

    def select_thompson(self, Xs, q: int, n_paths: Optional[int] = None, n_features: int = 2048, seed: int = 0,
                        idx_offset: int = 0) -> ThompsonResult:
        """q candidates to evaluate in parallel by Thompson sampling: the minimisers of independent posterior sample paths.
        n_paths (default min(64, 2 q)) paths are drawn and scored, and the first q DISTINCT winners in path order are
        returned - FEWER than q when the paths agree: that is the posterior saying it has converged on those points, and a
        caller who needs q points regardless tops the batch up with select_batch().  No variance pass is run.
        ValueError on bad q / n_paths / n_features / seed before any GPU work; IndexError when a value is NaN."""
        from .thompson import first_distinct, select_params

        need_se(self.kernel, "select_thompson()")
        self._need_unrolled_d("select_thompson()")
        Xsd, M = self._candidates(Xs)
        q, n_paths, n_features, seed = select_params(q, n_paths, n_features, seed, M=M, d=self.d)
        r = self.thompson_score(self.thompson_paths(n_paths, n_features, seed), Xsd, idx_offset=idx_offset)
        keep = first_distinct(r.indices, q)
        return ThompsonResult(indices=r.indices[keep], values=r.values[keep], nan_counts=r.nan_counts)

    # -- noisy expected improvement: EI averaged over fantasies of the incumbent (csrc/nei.hip) ----------
    def fantasies(self, n_fantasies: int = 16, seed: int = 0, delta: float = 1e-6) -> Fantasies:
        """n_fantasies samples of the LATENT function at the observed points from the posterior, and the noise-free twin
        (a second factorisation of the same X, ls and kernel with jitters (delta, 0)) they are scored with.  The model is
        latent covariance K0 + delta I plus noise of variance rho - delta, rho = jitter1 + jitter2 of this surrogate.  The
        draws are nei.nei_draws(N, n_fantasies, seed).  Needs factorise(order="arrival") and d <= 16; every kernel family.
        ValueError on bad parameters (delta > rho included) before any GPU work; LinAlgError when the twin is not positive
        definite.  Valid until the next factorise() / append() / load_state_dict()."""
        from .nei import nei_draws, nei_params

        S, seed, _, delta = nei_params(n_fantasies, seed, 0.0, delta, rho=self.jitter1 + self.jitter2)
        self._need_unrolled_d("fantasies()")
        if self.N < 1:
            raise _lib.GpboError("fantasies() needs a factorised surrogate")
        if self.perm is not None:
            raise ValueError("fantasies() needs factorise(order='arrival')")
        torch = self.torch
        Z, E = nei_draws(self.N, S, seed)
        N, Np = self.N, self.Np
        with torch.cuda.device(self.device):
            K0d = torch.empty((Np, Np), dtype=torch.float64, device=self.device)
            U0 = torch.empty((Np, Np), dtype=torch.float64, device=self.device)
            alpha0 = torch.empty(Np, dtype=torch.float64, device=self.device)
            info0 = torch.zeros(1, dtype=torch.int32, device=self.device)
            self._factorise_into(self.X, self.y, N, self.d, self.ls_h, self._kid(), delta, 0.0, Np, K0d, U0, alpha0, info0)
            Zd, Ed = self._dev(Z), self._dev(E)
            A = torch.empty((S, Np), dtype=torch.float64, device=self.device)
            F = torch.empty((S, Np), dtype=torch.float64, device=self.device)
            best = torch.empty(S, dtype=torch.float64, device=self.device)
            need = int(self.lib.gpbo_nei_fantasies_workspace_bytes(Np, S))
            wn = self._workspace("_work_nei", need)
            noise_sd = float(np.sqrt(max((self.jitter1 + self.jitter2) - delta, 0.0)))
            _lib.call(self.lib.gpbo_nei_fantasies_f64, K0d, U0, self.U, self.y, N, Np, Zd, Ed, noise_sd, S, A, F, best, wn,
                      need, self._stream())
            info = int(info0.item())   # synchronises: Zd and Ed have been consumed
        if info != 0:
            raise np.linalg.LinAlgError(f"the noise-free twin (k(X,X) + {delta!r} I) is not positive definite (pivot {info} of "
                                        f"{N}): raise delta")
        return Fantasies(A, F, best, K0d, U0, S, seed, delta, (id(self), self._epoch))

    def score_nei(self, fantasies: Fantasies, Xs, xi: float = 0.0, best=None, dense: bool = False,
                  idx_offset: int = 0, check: bool = True) -> NeiResult:
        """NEI(x) = mean_s EI(mu_s(x), sigma_0(x); best_s, xi) at the rows of Xs and its first arg-max
        (gpbo_posterior_nei_kern_f64: the variance pass on the twin, the S means from the pass's K(X*,X) image on the matrix
        cores).  best: S incumbents to use in the place of the fantasies' minima.  dense=True: also NEI [M], sigma_0 [M] and
        the means [S x M] on the device.  One read-back (synchronises).  A candidate with a NaN coordinate counts in
        nan_count and is never chosen; IndexError when no candidate is left (check=False: the caller looks at best_idx itself -
        a shard of a larger candidate set)."""
        from .nei import nei_best, nei_params

        if not isinstance(fantasies, Fantasies) or fantasies.epoch != (id(self), self._epoch):
            raise ValueError("these fantasies do not belong to the surrogate as it is now: call fantasies() again after "
                             "factorise() / append()")
        S = fantasies.n_fantasies
        _, _, xi, _ = nei_params(S, 0, xi)
        b = nei_best(best, S)
        torch = self.torch
        Xsd, M = self._candidates(Xs)
        with torch.cuda.device(self.device):
            bd = fantasies.best if b is None else self._dev(b)
            chunk = self._chunk_for(M)
            need = int(self.lib.gpbo_posterior_nei_workspace_bytes(self.Np, chunk, M, S))
            work = self._workspace("_work_nei", need)
            acq = sigma = mu = None
            if dense:
                acq = torch.empty(M, dtype=torch.float64, device=self.device)
                sigma = torch.empty(M, dtype=torch.float64, device=self.device)
                mu = torch.empty((S, M), dtype=torch.float64, device=self.device)
            _lib.call(self.lib.gpbo_posterior_nei_kern_f64, Xsd, M, *self._head(), self._kid(), fantasies.U0, fantasies.A, bd,
                      S, 1.0 + fantasies.delta, xi, int(idx_offset), chunk, mu, M, sigma, acq, self._result, work, need,
                      self._stream())
            v, i, n = self.read_result(self._result)   # synchronises: Xsd has been consumed
        if check and not int(idx_offset) <= i < int(idx_offset) + M:
            raise IndexError(NAN_ACQUISITION)
        return NeiResult(v, i, n, bd, acq, sigma, mu)

    def select_nei(self, Xs, n_fantasies: int = 16, seed: int = 0, xi: float = 0.0, delta: float = 1e-6,
                   dense: bool = False, idx_offset: int = 0, check: bool = True) -> NeiResult:
        """fantasies() and score_nei() in one call: the next point by noisy expected improvement."""
        from .nei import nei_params

        nei_params(n_fantasies, seed, xi, delta, rho=self.jitter1 + self.jitter2)   # (refused before any GPU work)
        Xsd, _ = self._candidates(Xs)
        return self.score_nei(self.fantasies(n_fantasies, seed, delta), Xsd, xi=xi, dense=dense, idx_offset=idx_offset,
                              check=check)

    # -- max-value entropy search on the dense posterior (csrc/mes.hip) --------------------------------
    def _posterior_pair(self, mu, sigma) -> tuple:
        """(mu, sigma as contiguous fp64 device tensors, M); refuses anything but two flat arrays of one length."""
        mud, sgd = self._dev(mu).reshape(-1), self._dev(sigma).reshape(-1)
        M = int(mud.numel())
        if M < 1 or int(sgd.numel()) != M:
            raise ValueError("mu and sigma must hold one value per candidate (at least one)")
        return mud, sgd, M

    def log_survival(self, mu, sigma, z) -> tuple:
        """(log S(z_q) = sum_c log Phi((mu_c - z_q) / sigma_c) as a float64 host array [Q], the number of candidates skipped
        because their mu or sigma is NaN) over dense mu / sigma [M] (gpbo_mes_log_survival_f64: one pass whatever Q <= 64; the
        edge rules are stated in include/gpbo.h).  Works without a factorisation.  One read-back (synchronises)."""
        torch = self.torch
        zh = np.ascontiguousarray(np.asarray(z, dtype=np.float64).reshape(-1))
        Q = int(zh.size)
        if not 1 <= Q <= _lib.MES_MAX_LEVELS or not np.all(np.isfinite(zh)):
            raise ValueError(f"z must hold 1 to {_lib.MES_MAX_LEVELS} finite levels")
        mud, sgd, M = self._posterior_pair(mu, sigma)
        with torch.cuda.device(self.device):
            work = self._workspace("_work_mes", _lib.MES_WORK_BYTES)
            out = torch.empty(Q + 1, dtype=torch.float64, device=self.device)   # log S [Q] | the NaN count (int64)
            _lib.call(self.lib.gpbo_mes_log_survival_f64, mud, sgd, M, zh, Q, out, out[Q:], work, _lib.MES_WORK_BYTES,
                      self._stream())
            h = out.cpu()   # synchronises: the levels have travelled by value, mud / sgd have been consumed
        return h[:Q].numpy().copy(), int(h[Q:].view(torch.int64)[0])

    def mes_on_posterior(self, mu, sigma, y_star, idx_offset: int = 0, dense: bool = True) -> MesResult:
        """MES(x) = mean_s h((mu(x) - y_star_s) / sigma(x)) over dense mu / sigma [M] and its first arg-max (gpbo_mes_acq_f64).
        y_star: 1 to 64 finite sampled minima, in the units of mu.  One read-back (synchronises)."""
        from .mes import mes_y_star

        torch = self.torch
        ys = np.ascontiguousarray(np.asarray(y_star, dtype=np.float64).reshape(-1))
        if not 1 <= ys.size <= _lib.MES_MAX_S:
            raise ValueError(f"y_star must hold 1 to {_lib.MES_MAX_S} values, got {ys.size}")
        ys = mes_y_star(ys, int(ys.size))
        mud, sgd, M = self._posterior_pair(mu, sigma)
        with torch.cuda.device(self.device):
            work = self._workspace("_work_mes", _lib.MES_WORK_BYTES)
            acq = torch.empty(M, dtype=torch.float64, device=self.device) if dense else None
            _lib.call(self.lib.gpbo_mes_acq_f64, mud, sgd, M, ys, int(ys.size), int(idx_offset), acq, self._result, work,
                      _lib.MES_WORK_BYTES, self._stream())
            v, i, n = self.read_result(self._result)   # synchronises
        return MesResult(v, i, n, acq, ys)

    def mes_minima(self, mu, sigma, Xs, S: int, seed: int, y_star, cap, log_survival=None, reduce_min=None) -> tuple:
        """(the S sampled minima m*_s [S] in the units of mu, the quartiles or None) for a MES call on the posterior (mu, sigma)
        of the candidates Xs.  y_star: "gumbel" (mes.gumbel_quartiles on log_survival(), mes.sample_minima with
        mes.mes_uniforms(S, seed)), "thompson" (m*_s = -val_out[s] of thompson_score with S paths and this seed: kernel='se'),
        or S values used verbatim.  cap: a number or None.  log_survival / reduce_min: what a sharded caller puts between the
        local pass and the fit (the rank-order sum of the partial log S, the MIN all-reduce of the brackets)."""
        from . import mes as MES

        y_star = MES.mes_y_star(y_star, S)
        if not isinstance(y_star, str):
            return y_star, None
        if y_star == "thompson":
            r = self.thompson_score(self.thompson_paths(S, seed=seed), Xs)
            return -np.asarray(r.values, dtype=np.float64), None   # (minima of actual paths: the cap is the Gumbel route's)
        torch = self.torch
        with torch.cuda.device(self.device):
            # the brackets: plumbing on the dense arrays (NaN candidates are skipped, as log S skips them)
            ok = ~(torch.isnan(mu) | torch.isnan(sigma))
            inf = torch.full_like(mu, float("inf"))
            lo_hi = torch.stack([torch.where(ok, mu - MES.LO_SIGMAS * sigma, inf).min(),
                                 torch.where(ok, mu + MES.HI_SIGMAS * sigma, inf).min()]).cpu().numpy()
        if reduce_min is not None:
            lo_hi = reduce_min(lo_hi)
        if not np.all(np.isfinite(lo_hi)):
            raise IndexError(NAN_ACQUISITION)   # no candidate with a usable posterior
        ls = log_survival if log_survival is not None else (lambda z: self.log_survival(mu, sigma, z))
        quartiles, _ = MES.gumbel_quartiles(ls, lo_hi[0], lo_hi[1])
        return MES.sample_minima(quartiles, MES.mes_uniforms(S, seed), cap), quartiles

    def select_mes(self, Xs, n_samples: int = 16, seed: int = 0, y_star="gumbel", cap="observed", dense: bool = False,
                   idx_offset: int = 0, prior_var: Optional[float] = None) -> MesResult:
        """The next point by max-value entropy search (Wang & Jegelka 2017): the unchanged fp64 pass for (mu, sigma)
        at the rows of Xs, n_samples samples of the minimum's VALUE, then MES and its first arg-max.  No trade-off parameter
        and no incumbent; every kernel family.  y_star: "gumbel" (the Gumbel fit to three quartiles of Pr[m* > z] under an
        independence approximation: four passes of gpbo_mes_log_survival_f64), "thompson" (the minima of n_samples posterior
        sample paths: kernel='se'), or n_samples values.  cap: "observed" (m*_s <= min(y): the paper's rule), a number or
        None.  prior_var: the pass's (default: that of this factorisation's jitters).  ValueError on bad parameters before any
        GPU work."""
        from .mes import mes_params, mes_y_star

        S, seed, cap = mes_params(n_samples, seed, cap)
        y_star = mes_y_star(y_star, S)
        if isinstance(y_star, str) and y_star == "thompson":
            need_se(self.kernel, "select_mes(y_star='thompson')")
        if self.N < 1:
            raise _lib.GpboError("select_mes() needs a factorised surrogate")
        Xsd, M = self._candidates(Xs)
        pv = (1.0 + self.jitter1) + self.jitter2 if prior_var is None else float(prior_var)
        s = self.score(Xsd, acquisition="lcb", explore=0.0, dense=True, prior_var=pv)
        if isinstance(cap, str):
            cap = float(self.y[: self.N].min().item())
        m, quartiles = self.mes_minima(s.mu, s.sigma, Xsd, S, seed, y_star, cap)
        r = self.mes_on_posterior(s.mu, s.sigma, m, idx_offset=idx_offset, dense=dense)
        r.quartiles, r.mu, r.sigma = quartiles, s.mu, s.sigma
        return r

    # -- constrained EI / PI / probability of feasibility in log space (csrc/constrained.hip) ------------
    def constrained_on_posterior(self, mu, sigma, cons_mu, cons_sigma, upper, base: str = "ei", f_best: Optional[float] = None,
                                 xi: float = 0.0, idx_offset: int = 0, dense: bool = True,
                                 ldc: Optional[int] = None) -> ConstrainedResult:
        """value(x) = base(x) + sum_c log Phi((upper_c - cons_mu_c(x)) / cons_sigma_c(x)) over dense posteriors and its first
        arg-max (gpbo_constrained_acq_f64; the formulas and edge rules are stated in include/gpbo.h).  base: "ei" (log sigma +
        log h(z): the logarithm of constrained expected improvement), "pi" (log Phi(z)) or "none" (the log-probability of
        feasibility alone; mu / sigma may be None).  mu, sigma [M]; cons_mu, cons_sigma [C x M] (None or empty with no
        constraint; with ldc: flat buffers whose row c starts at c ldc); upper [C].  f_best, xi: in the units of mu, needed
        with a base.  Works without a factorisation.  One read-back (synchronises)."""
        from .constrained import cons_limits, cons_params

        torch = self.torch
        u = cons_limits(upper)
        C = int(u.size)
        bid, fb, xi = cons_params(base, f_best, xi, C)
        if bid == _lib.CONS_BASE_NONE:
            mud = sgd = None
        else:
            mud, sgd, M = self._posterior_pair(mu, sigma)
        cmd = csd = None
        if C > 0:
            cmd, csd = self._dev(cons_mu), self._dev(cons_sigma)
            if ldc is None:
                cmd, csd = cmd.reshape(C, -1), csd.reshape(C, -1)
                ldc = int(cmd.shape[1])
                if bid == _lib.CONS_BASE_NONE:
                    M = ldc
                elif ldc != M:
                    raise ValueError("cons_mu and cons_sigma must hold one row of M values per limit (longer rows: pass ldc)")
            elif bid == _lib.CONS_BASE_NONE:
                raise ValueError("ldc needs a base (the candidate count is that of mu)")
            ldc = int(ldc)
            if ldc < M or M < 1 or int(cmd.numel()) < (C - 1) * ldc + M or csd.shape != cmd.shape:
                raise ValueError("cons_mu and cons_sigma must hold one row of at least M values per limit")
        with torch.cuda.device(self.device):
            work = self._workspace("_work_cons", _lib.CONS_WORK_BYTES)
            val = torch.empty(M, dtype=torch.float64, device=self.device) if dense else None
            feas = torch.empty(M, dtype=torch.float64, device=self.device) if dense else None
            _lib.call(self.lib.gpbo_constrained_acq_f64, mud, sgd, M, bid, fb, xi, cmd, csd, ldc if C > 0 else M, C, u,
                      int(idx_offset), val, feas, self._result, work, _lib.CONS_WORK_BYTES, self._stream())
            v, i, n = self.read_result(self._result)   # synchronises: cmd / csd have been consumed
        return ConstrainedResult(v, i, n, base, val, feas, None if bid == _lib.CONS_BASE_NONE else fb)

    def select_constrained(self, Xs, constraints=(), upper=(), base: str = "ei", f_best: Optional[float] = None,
                           xi: float = 0.0, dense: bool = False, idx_offset: int = 0) -> ConstrainedResult:
        """The next point by constrained expected improvement (base="ei"), constrained probability of improvement ("pi") or
        the probability of feasibility ("none"): this surrogate and every DeviceGP of `constraints` - each factorised on ITS
        quantity's observations, with any kernel family and model of its own - score the rows of Xs with the unchanged fp64
        pass, then constrained_on_posterior() combines them.  upper: one limit per constraint, in the units of its
        observations.  f_best: a number, or None for the smallest of this surrogate's observations among those at which every
        constraint's observation is within its limit (constrained.feasible_incumbent: the same points in all surrogates); if
        none is, the call maximises the probability of feasibility alone and the result's base says "none".  Every pass uses
        its own factorisation's prior variance ((1 + jitter1) + jitter2).  ValueError on bad parameters, on a constraint that is
        no DeviceGP or lives on another device, before any GPU work; GpboError for a surrogate that is not factorised."""
        from .constrained import cons_limits, cons_params, feasible_incumbent

        constraints = list(constraints)
        u = cons_limits(upper, len(constraints))
        cons_params(base, 0.0 if f_best is None else f_best, xi, len(constraints))
        for g in constraints:
            if not isinstance(g, DeviceGP) or g.device != self.device:
                raise ValueError(f"select_constrained(): every constraint must be a DeviceGP on {self.device}")
        for g in (self, *constraints):
            if g.N < 1:
                raise _lib.GpboError("select_constrained() needs a factorised surrogate for the objective and every constraint")
        if base != "none" and f_best is None:
            X0, y0 = self.observations_host()
            obs = [g.observations_host() for g in constraints]
            f_best = feasible_incumbent(X0, y0, [o[0] for o in obs], [o[1] for o in obs], u)
            if f_best is None:
                base = "none"
        Xsd, M = self._candidates(Xs)
        post = []
        for g in (*constraints, *(() if base == "none" else (self,))):
            pv = (1.0 + g.jitter1) + g.jitter2
            s = g.score(g._candidates(Xsd)[0], acquisition="lcb", explore=0.0, dense=True, prior_var=pv)
            post.append((s.mu, s.sigma))
        mu, sigma = post.pop() if base != "none" else (None, None)
        cm = self.torch.stack([p[0] for p in post]) if post else None
        cs = self.torch.stack([p[1] for p in post]) if post else None
        return self.constrained_on_posterior(mu, sigma, cm, cs, u, base=base, f_best=f_best, xi=xi, idx_offset=idx_offset,
                                             dense=dense)

    # -- two-objective expected hypervolume improvement in log space (csrc/ehvi.hip) --------------------
    def ehvi_on_posterior(self, mu1, sigma1, mu2, sigma2, front, ref, idx_offset: int = 0, dense: bool = True) -> EhviResult:
        """log EHVI(x) of two minimised, independent objectives over their dense posteriors and its first arg-max
        (gpbo_ehvi_acq_f64; the formula and edge rules are stated in include/gpbo.h).  mu1, sigma1, mu2, sigma2 [M]; front
        [P x 2]: rows (objective 1, objective 2), strictly ascending in the first and strictly descending in the second
        (pareto.pareto_front returns that form; None or empty: no front); ref: two finite numbers above every front point.  All in
        the units of the posteriors.  Works without a factorisation.  One read-back (synchronises)."""
        from .pareto import check_front

        torch = self.torch
        F, r = check_front(front, ref)
        m1, s1, M = self._posterior_pair(mu1, sigma1)
        m2, s2, M2 = self._posterior_pair(mu2, sigma2)
        if M2 != M:
            raise ValueError("the two objectives' posteriors must hold one value per candidate each")
        with torch.cuda.device(self.device):
            work = self._workspace("_work_ehvi", _lib.EHVI_WORK_BYTES)
            val = torch.empty(M, dtype=torch.float64, device=self.device) if dense else None
            _lib.call(self.lib.gpbo_ehvi_acq_f64, m1, s1, m2, s2, M, F, int(F.shape[0]), r[0], r[1], int(idx_offset), val,
                      self._result, work, _lib.EHVI_WORK_BYTES, self._stream())
            v, i, n = self.read_result(self._result)   # synchronises: the converted inputs have been consumed
        return EhviResult(v, i, n, val, F, r)

    def select_ehvi(self, Xs, other, front=None, ref="nadir", dense: bool = False, idx_offset: int = 0) -> EhviResult:
        """The next point by expected hypervolume improvement of two minimised objectives: this surrogate (objective 1) and
        `other` (objective 2) - each factorised on ITS objective's observations, with any kernel family and model of its own -
        score the rows of Xs with the unchanged fp64 pass, then ehvi_on_posterior() combines them.  front: [P x 2] in the units
        of the observations, or None for the Pareto front of the two surrogates' own observations (they must hold the same
        points, bit for bit: observation i of each is one evaluation).  ref: two numbers, or "nadir" (pareto.reference_point
        over those observations).  Every pass uses its own factorisation's prior variance ((1 + jitter1) + jitter2).  ValueError
        on bad parameters, on an `other` that is no DeviceGP or lives on another device, before any GPU work; GpboError for a
        surrogate that is not factorised."""
        from .pareto import check_front, observed_pairs, pareto_front, reference_point

        if not isinstance(other, DeviceGP) or other.device != self.device:
            raise ValueError(f"select_ehvi(): other must be a DeviceGP on {self.device}")
        if not (isinstance(ref, str) and ref == "nadir"):
            ref = reference_point(None, ref)
        if front is not None and isinstance(ref, tuple):
            check_front(front, ref)
        for g in (self, other):
            if g.N < 1:
                raise _lib.GpboError("select_ehvi() needs a factorised surrogate for both objectives")
        if front is None or isinstance(ref, str):
            Y = observed_pairs(*self.observations_host(), *other.observations_host())
            ref = reference_point(Y, ref)
            if front is None:
                front = pareto_front(Y, ref)
        F, r = check_front(front, ref)
        Xsd, M = self._candidates(Xs)
        post = []
        for g in (self, other):
            pv = (1.0 + g.jitter1) + g.jitter2
            s = g.score(g._candidates(Xsd)[0], acquisition="lcb", explore=0.0, dense=True, prior_var=pv)
            post.append((s.mu, s.sigma))
        return self.ehvi_on_posterior(post[0][0], post[0][1], post[1][0], post[1][1], F, r, idx_offset=idx_offset, dense=dense)

    # -- acquisition gradients and off-grid refinement (csrc/refine.hip) -------------------------------
    def _points(self, Xq, what: str):
        """(Xq as a contiguous fp64 device tensor [P x d], P) for the query-point calls."""
        Xd = self._dev(Xq)
        if Xd.dim() == 1:
            Xd = Xd.reshape(1, -1)
        if Xd.dim() != 2 or int(Xd.shape[1]) != self.d:
            raise ValueError(f"{what} must be (P, d) with the same d as X")
        return Xd, int(Xd.shape[0])

    def posterior_grad(self, Xq, acquisition: str = "lcb", explore: float = 4.0, f_best: Optional[float] = None,
                       xi: float = 0.0, prior_var: float = PRIOR_VAR) -> GradResult:
        """Posterior mean, standard deviation and acquisition at the rows of Xq [P x d] (P <= 4096) with their gradients in
        x (gpbo_posterior_grad_f64).  Query points, not candidates: the N == M quirk (diag_add) does not apply.  Works on
        the factorisation as it is (any order=, appended rows included).  Enqueues only; device tensors come back."""
        need_se(self.kernel, "posterior_grad()")
        self._need_unrolled_d("posterior_grad()")
        torch = self.torch
        Xd, P = self._points(Xq, "Xq")
        refine_params(P, self.d, 0, 1.0)
        kind, p0, p1 = acq_params(acquisition, explore, f_best, xi)
        with torch.cuda.device(self.device):
            need = int(self.lib.gpbo_posterior_grad_workspace_bytes(self.Np, P))
            work = self._workspace("_work_refine", need)
            vals = torch.empty((3, P), dtype=torch.float64, device=self.device)
            grads = torch.empty((3, P, self.d), dtype=torch.float64, device=self.device)
            _lib.call(self.lib.gpbo_posterior_grad_f64, Xd, P, *self._head(), self.U, self.alpha, float(prior_var), kind, p0,
                      p1, vals[0], vals[1], vals[2], grads[0], grads[1], grads[2], work, need, self._stream())
        self._keep = Xd
        return GradResult(vals[0], vals[1], vals[2], grads[0], grads[1], grads[2])

    def refine(self, starts, lower, upper, acquisition: str = "lcb", explore: float = 4.0, f_best: Optional[float] = None,
               xi: float = 0.0, iters: int = 30, step0: float = 0.1, prior_var: float = PRIOR_VAR) -> RefineResult:
        """Projected gradient ascent of the acquisition from every row of starts [P x d] (P <= 4096) inside the box
        [lower, upper] (gpbo_refine_f64; the rule is stated in include/gpbo.h): each start on its own, step doubled after an
        accepted trial and halved after a rejected one, iters trials.  All iters + 1 evaluations are enqueued at once;
        one read-back of the result record (synchronises).  Two calls give the same bits."""
        need_se(self.kernel, "refine()")
        self._need_unrolled_d("refine()")
        torch = self.torch
        Xd, P = self._points(starts, "starts")
        iters, step0 = refine_params(P, self.d, iters, step0)
        lo, hi = refine_box(lower, upper, self.d)
        kind, p0, p1 = acq_params(acquisition, explore, f_best, xi)
        with torch.cuda.device(self.device):
            x = Xd.clone()   # in: the starts, out: the refined points; the caller's tensor is never written to
            need = int(self.lib.gpbo_refine_workspace_bytes(self.Np, P))
            work = self._workspace("_work_refine", need)
            vals = torch.empty((3, P), dtype=torch.float64, device=self.device)
            accepted = torch.empty(P, dtype=torch.int32, device=self.device)
            res = torch.zeros(4, dtype=torch.int64, device=self.device)
            _lib.call(self.lib.gpbo_refine_f64, x, P, lo, hi, *self._head(), self.U, self.alpha, float(prior_var), kind, p0,
                      p1, iters, step0, vals[0], vals[1], accepted, vals[2], res, work, need, self._stream())
            v, i, n = self.read_result(res)   # synchronises
        return RefineResult(x=x, acq=vals[0], acq0=vals[1], accepted=accepted, pg=vals[2], best=i, best_val=v, nan_count=n)

    def select_refined(self, Xs, n_starts: int = 64, lower=None, upper=None, acquisition: str = "lcb", explore: float = 4.0,
                       f_best: Optional[float] = None, xi: float = 0.0, iters: int = 30, step0: float = 0.1,
                       prior_var: float = PRIOR_VAR) -> RefineResult:
        """The dense score() of the candidates Xs, then refine() from the n_starts candidates with the largest acquisition
        (stable descending sort: ties keep the lower index first).  lower / upper omitted: the per-feature minimum / maximum
        of Xs.  Returns refine()'s result with grid_idx / grid_val = score()'s arg-max and its value."""
        need_se(self.kernel, "select_refined()")
        self._need_unrolled_d("select_refined()")
        torch = self.torch
        Xsd, M = self._candidates(Xs)
        n_starts = int(n_starts)
        if not 1 <= n_starts <= min(_lib.REFINE_MAX_P, M):
            raise ValueError(f"n_starts must be in [1, min({_lib.REFINE_MAX_P}, M = {M})], got {n_starts}")
        refine_params(n_starts, self.d, iters, step0)
        if (lower is None) != (upper is None):
            raise ValueError("give both lower and upper, or neither")
        s = self.score(Xsd, acquisition=acquisition, explore=explore, f_best=f_best, xi=xi, dense=True, prior_var=prior_var)
        if s.nan_count > 0:
            raise IndexError(NAN_ACQUISITION)
        with torch.cuda.device(self.device):
            order = torch.sort(s.acq, descending=True, stable=True).indices[:n_starts]   # plumbing
            starts = Xsd[order].contiguous()
            if lower is None:
                lower, upper = Xsd.min(dim=0).values.cpu().numpy(), Xsd.max(dim=0).values.cpu().numpy()
        r = self.refine(starts, lower, upper, acquisition, explore, f_best, xi, iters, step0, prior_var)
        r.grid_idx, r.grid_val = s.best_idx, s.best_val
        return r

    @property
    def status(self):
        """Device int64[5]: the gpbo_result record of the last scoring call + the info word of the last factorisation
        (what distributed.allreduce_status gathers over the ranks)."""
        return self._status

    def read_result_and_info(self) -> tuple:
        """(best value, best index, NaN count, info of the last factorise/append) with one device-to-host copy."""
        r = self._status.cpu()  # synchronises
        best_val = float(r[:1].view(self.torch.float64)[0])
        return best_val, int(r[1]), int(r[2]), int(r[4:5].view(self.torch.int32)[0])

    def score(self, Xs, **kw) -> ScoreResult:
        return self._read(self.score_async(Xs, **kw))

    def acquisition_on_posterior(self, mu, sigma, acquisition: str = "lcb", explore: float = 4.0,
                                 f_best: Optional[float] = None, xi: float = 0.0, idx_offset: int = 0) -> ScoreResult:
        """Second acquisition on dense device mu/sigma (lower_confidence_bound(explore) after the fact)."""
        torch = self.torch
        M = int(mu.numel())
        kind, p0, p1 = acq_params(acquisition, explore, f_best, xi)
        with torch.cuda.device(self.device):
            acq = torch.empty(M, dtype=torch.float64, device=self.device)
            wbytes = int(self.lib.gpbo_acq_workspace_bytes())
            work = torch.empty(wbytes // 8 + 32, dtype=torch.float64, device=self.device)
            _lib.call(self.lib.gpbo_acq_argmax_f64, mu, sigma, M, kind, p0, p1, int(idx_offset), acq, self._result, work,
                      wbytes, self._stream())
            v, i, n = self.read_result(self._result)
        return ScoreResult(v, i, n, mu, sigma, acq)

    # -- ARD grid ------------------------------------------------------------------------------------
    ARD_KERNEL = "wave"  # N <= gpbo_nlml_grid_wave_max_n() (64): "wave" = a wave per cell, the matrix in registers (csrc/ard_wave.hip,
                         # round 5: 2,500 cells at N = 16 / 32 / 48 / 64, d = 2: 0.014 / 0.026 / 0.049 / 0.068 ms);
                         # "lds" = the workgroup-per-cell kernel of round 2 up to ARD_LDS_MAX_N, the fused kernel beyond (the
                         # routing until the end of round 5: 0.044 / 0.116 / 0.125 / 0.122 ms; tools/ard_lds_vs_fused.py).
                         # The float32 cells of the three kernels are equal.
    ARD_LDS_MAX_N = 32

    def nlml_grid(self, X, y, ls_cells, jitter: float = JITTER_KERNEL, likelihood: str = "reference") -> np.ndarray:
        """-log marginal likelihood of every row of ls_cells [G x d]  (point_selector.py:111-156), as a host array.

        likelihood="reference": the reference's value - float32, log det K taken as np.log(np.linalg.det(K)), which
        underflows to -inf beyond N ~ 100 (reproduced for parity).  likelihood="logdet": fp64, log det K = 2 sum log L_ii
        from the factor - finite at any N, NaN where a pivot is not positive (a documented departure)."""
        res = self.nlml_grid_device(X, y, ls_cells, jitter, likelihood).cpu().numpy()   # synchronises: the workspace is idle
        # the scratch slots can be GiBs (512 x (N + 16) x N x 8 bytes): kept between the calls of one search (a
        # coordinate-wise ARD search calls this once per axis and sweep) only while they are small
        if self._work_ard is not None and self._work_ard.numel() * 8 > self.ARD_KEEP_WORKSPACE_BYTES:
            self._work_ard = None
        return res

    def nlml_grid_device(self, X, y, ls_cells, jitter: float = JITTER_KERNEL, likelihood: str = "reference"):
        """The same grid left on the device (float32 / float64 tensor [G]); enqueues on the current stream, no read-back."""
        need_se(self.kernel, "nlml_grid()")   # (the grid kernels generate squared-exponential entries)
        if likelihood not in ("reference", "logdet"):
            raise ValueError(f"likelihood must be 'reference' or 'logdet', got {likelihood!r}")
        torch = self.torch
        Xd, yd = self._dev(X), self._dev(y).reshape(-1)
        N, d = int(Xd.shape[0]), int(Xd.shape[1])
        cells = ls_cells if isinstance(ls_cells, torch.Tensor) else np.asarray(ls_cells, dtype=np.float64).reshape(-1, d)
        cells = self._dev(cells).reshape(-1, d)
        G = int(cells.shape[0])
        logdet = likelihood == "logdet"
        with torch.cuda.device(self.device):
            wave = self.ARD_KERNEL == "wave" and N <= int(self.lib.gpbo_nlml_grid_wave_max_n())
            if wave:
                # the reference's own sizes: a wave per cell, the matrix in registers (csrc/ard_wave.hip), both likelihood modes;
                # pinned against the reference's float32 ties (golden g4_ard_n2) like the in-LDS kernel it replaced
                out = torch.empty(G, dtype=torch.float64 if logdet else torch.float32, device=self.device)
                fn = self.lib.gpbo_nlml_grid_wave_logdet_f64 if logdet else self.lib.gpbo_nlml_grid_wave_f64
                _lib.call(fn, Xd, yd, N, d, cells, G, float(jitter), out, self._stream())
            elif N > self.ARD_LDS_MAX_N or logdet:
                # one persistent workgroup per cell, the whole factorisation in one launch (csrc/ard.hip, round 5)
                out = torch.empty(G, dtype=torch.float64 if logdet else torch.float32, device=self.device)
                need = int(self.lib.gpbo_nlml_grid_batched_workspace_bytes(N, G))
                self._workspace("_work_ard", need, free_first=True)
                fn = self.lib.gpbo_nlml_grid_batched_logdet_f64 if logdet else self.lib.gpbo_nlml_grid_batched_f64
                _lib.call(fn, Xd, yd, N, d, cells, G, float(jitter), out, self._work_ard, need, self._stream())
            else:
                out = torch.empty(G, dtype=torch.float32, device=self.device)
                _lib.call(self.lib.gpbo_nlml_grid_f64, Xd, yd, N, d, cells, G, float(jitter), out, self._stream())
            self._keep_ard = (Xd, yd, cells)   # alive until the stream has consumed them
        return out

    # -- ML-II length-scale fitting (ard="gradient"; csrc/ard_grad.hip) --------------------------------------------
    def _fit_buffers(self, Np: int, d: int):
        """The fit's own factor buffers (K, U, alpha, info, workspaces): the surrogate's K / U / alpha stay untouched."""
        torch = self.torch
        fb = self._fit_bufs
        if fb is None or fb["Np"] != Np or fb["d"] < d:
            self._fit_bufs = None
            wf = int(self.lib.gpbo_factorise_workspace_bytes(Np))
            wg = int(self.lib.gpbo_nlml_grad_workspace_bytes(Np, d))
            if wg < 0:
                raise _lib.GpboError("gpbo_nlml_grad_workspace_bytes: invalid sizes")
            f64 = dict(dtype=torch.float64, device=self.device)
            fb = dict(Np=Np, d=d, K=torch.empty((Np, Np), **f64), U=torch.empty((Np, Np), **f64),
                      alpha=torch.empty(Np, **f64), out=torch.empty(1 + d, **f64),
                      info=torch.zeros(1, dtype=torch.int32, device=self.device),
                      work_fact=torch.empty((wf + 7) // 8, **f64), wf=wf, work_grad=torch.empty((wg + 7) // 8, **f64), wg=wg)
            self._fit_bufs = fb
        return fb

    def _fit_bytes(self) -> int:
        fb = self._fit_bufs or {}
        return sum(t.numel() * t.element_size() for t in fb.values() if isinstance(t, self.torch.Tensor))

    def _fit_problem(self, X, y, ls, kernel):
        """The input check of the two likelihood calls: (kernel id, X and y on the device, N, d, length scales on the host)."""
        kid = _lib.kernel_id(kernel)
        limit = (_lib.MAX_D, f"the likelihood gradient supports d <= {_lib.MAX_D}, got {{d}}")
        return (kid, *self._problem(X, y, ls, [limit], positive=True))

    def _fit_factorise(self, kid, Xd, yd, N, d, ls_h, jitter):
        """K = k(X,X) + jitter I factorised into the fit's own buffers (enqueued; inside torch.cuda.device(self.device)).
        Returns (buffers, padded N)."""
        Np = int(self.lib.gpbo_padded_n(N))
        fb = self._fit_buffers(Np, d)
        self._factorise_into(Xd, yd, N, d, ls_h, kid, float(jitter), 0.0, Np, fb["K"], fb["U"], fb["alpha"], fb["info"],
                             fb["work_fact"], fb["wf"])
        return fb, Np

    def nlml_and_grad(self, X, y, ls, jitter: float = JITTER_KERNEL, kernel: str = "se"):
        """(NLML, d NLML / d log ls [d]) of K = k(X,X) + jitter I - the "logdet" likelihood and its gradient - from a
        factorisation into the fit's own buffers (the surrogate held by this object is not touched).  NaN in every
        output when K is not positive definite.  d <= 16.  kernel: the covariance family k (factorise())."""
        kid, Xd, yd, N, d, ls_h = self._fit_problem(X, y, ls, kernel)
        with self.torch.cuda.device(self.device):
            fb, Np = self._fit_factorise(kid, Xd, yd, N, d, ls_h, jitter)
            _lib.call(self.lib.gpbo_nlml_grad_kern_f64, fb["U"], fb["alpha"], yd, Xd, N, Np, d, ls_h, kid, fb["info"],
                      fb["out"], fb["work_grad"], fb["wg"], self._stream())
            out = fb["out"][: 1 + d].cpu().numpy()   # synchronises
        return float(out[0]), out[1:].copy()

    @contextmanager
    def _fit_session(self, X, y):
        """X and y uploaded once for all evaluations of a fit; the fit's buffers are released afterwards when larger than
        ARD_KEEP_WORKSPACE_BYTES."""
        Xd, yd = self._dev(X), self._dev(y).reshape(-1)
        try:
            yield Xd, yd
        finally:
            if self._fit_bytes() > self.ARD_KEEP_WORKSPACE_BYTES:
                self._fit_bufs = None

    # -- ML-II over all hyperparameters (ard="hyper"; csrc/hyper.hip) and leave-one-out prediction ---------------------
    def nlml_hyper(self, X, y, ls, noise: float, fit_mean: bool = True, fit_scale: bool = True, kernel: str = "se"):
        """(L, dL / d(log ls, log noise) [d + 1], mean, scale^2) of the model y ~ N(mean 1, scale^2 (k(X,X) + noise I)) with
        mean and scale^2 at their closed-form optima (fit_mean / fit_scale False: held at 0 / 1): gpbo_nlml_hyper_f64 on a
        factorisation of the raw y with (jitter1, jitter2) = (noise, 0) in the fit's own buffers (the surrogate held by this
        object is not touched).  NaN in every output when the matrix is not positive definite or scale^2 is not positive
        (one observation, a constant y).  d <= 16.  kernel: the covariance family k (factorise())."""
        torch = self.torch
        kid, Xd, yd, N, d, ls_h = self._fit_problem(X, y, ls, kernel)
        noise = float(noise)
        if not (np.isfinite(noise) and noise > 0.0):
            raise ValueError(f"noise must be positive and finite, got {noise!r}")
        flags = (_lib.HYPER_MEAN if fit_mean else 0) | (_lib.HYPER_SCALE if fit_scale else 0)
        with torch.cuda.device(self.device):
            fb, Np = self._fit_factorise(kid, Xd, yd, N, d, ls_h, noise)
            if "work_hyper" not in fb:
                wh = int(self.lib.gpbo_nlml_hyper_workspace_bytes(Np, fb["d"]))
                if wh < 0:
                    raise _lib.GpboError("gpbo_nlml_hyper_workspace_bytes: invalid sizes")
                fb["work_hyper"] = torch.empty((wh + 7) // 8, dtype=torch.float64, device=self.device)
                fb["wh"] = wh
                fb["out_hyper"] = torch.empty(4 + fb["d"], dtype=torch.float64, device=self.device)
            _lib.call(self.lib.gpbo_nlml_hyper_kern_f64, fb["U"], fb["alpha"], yd, Xd, N, Np, d, ls_h, kid, noise, flags,
                      fb["info"], fb["out_hyper"], None, fb["work_hyper"], fb["wh"], self._stream())
            out = fb["out_hyper"][: 4 + d].cpu().numpy()   # synchronises
        return float(out[0]), out[1: 2 + d].copy(), float(out[2 + d]), float(out[3 + d])

    # -- the same likelihood at many cells (ard="marginal"; csrc/hyper_wave.hip) ------------------------------------------
    HYPER_CELLS_KERNELS = ("se", "matern32", "matern52")   # families with instances of the wave-per-cell kernel (all: none spills)

    def hyper_cells_route(self, N: int, kernel: str = "se") -> str:
        """"wave": one launch of gpbo_nlml_hyper_cells_f64 for all cells (N <= 64, a family with instances); "loop": one
        nlml_hyper() per cell."""
        return "wave" if N <= _lib.HYPER_CELLS_MAX_N and kernel in self.HYPER_CELLS_KERNELS else "loop"

    def nlml_hyper_cells_fn(self, X, y, fit_mean: bool = True, fit_scale: bool = True, kernel: str = "se", route=None):
        """cells [G x (d + 1)] -> [G x 3] for one (X, y), uploaded once: what a sampler calls once per step (nlml_hyper_cells
        describes the values).  route: None (hyper_cells_route), "wave" or "loop"."""
        torch = self.torch
        kid = _lib.kernel_id(kernel)
        limit = (_lib.MAX_D, f"the likelihood of hyperparameter cells supports d <= {_lib.MAX_D}, got {{d}}")
        Xd, y_h, N, d, _ = self._problem(X, y, None, [limit], host_y=True)
        route = self.hyper_cells_route(N, kernel) if route is None else route
        if route not in ("wave", "loop") or (route == "wave" and self.hyper_cells_route(N, kernel) != "wave"):
            raise ValueError(f"route {route!r} is not available for N = {N}, kernel={kernel!r}")
        flags = (_lib.HYPER_MEAN if fit_mean else 0) | (_lib.HYPER_SCALE if fit_scale else 0)
        # the kernel forms the profile from y . Kt^-1 y, 1 . Kt^-1 y and 1 . Kt^-1 1, which cancels like (mean / sd)^2 of the y
        # it is given: with a fitted mean it gets y - mean(y), and the shift goes back onto m (include/gpbo.h)
        shift = float(np.mean(y_h)) if fit_mean else 0.0
        yd = self._dev(y_h - shift) if route == "wave" else self._dev(y_h)

        def cells_ok(cells):
            c = np.ascontiguousarray(np.asarray(cells, dtype=np.float64))
            if c.ndim != 2 or c.shape[1] != d + 1 or c.shape[0] < 1:
                raise ValueError(f"cells must be [G x {d + 1}] rows (ls_1 ... ls_d, rho) with G >= 1")
            if not (np.all(np.isfinite(c)) and np.all(c[:, :d] > 0.0)):
                raise ValueError("cells must be finite with positive length scales")
            return c

        def wave(cells):
            c = cells_ok(cells)
            with torch.cuda.device(self.device):
                cd = torch.from_numpy(c).to(self.device)
                out = torch.empty((len(c), 3), dtype=torch.float64, device=self.device)
                _lib.call(self.lib.gpbo_nlml_hyper_cells_f64, Xd, yd, N, d, cd, len(c), kid, flags, out, self._stream())
                res = out.cpu().numpy()   # synchronises: the one read-back
            res[:, 1] += shift
            return res

        def loop(cells):
            c = cells_ok(cells)
            res = np.full((len(c), 3), np.nan)
            for g, row in enumerate(c):
                if row[d] > 0.0:   # (nlml_hyper refuses a noise that is not positive: such a cell is NaN)
                    f, _, m, s2 = self.nlml_hyper(Xd, yd, row[:d], row[d], fit_mean, fit_scale, kernel)
                    res[g] = (f, m, s2)
            return res

        return wave if route == "wave" else loop

    def nlml_hyper_cells(self, X, y, cells, fit_mean: bool = True, fit_scale: bool = True, kernel: str = "se", route=None):
        """[G x 3] host array (L, mean, scale^2) - nlml_hyper()'s value, mean and scale^2, no gradient - at every row
        (ls_1 ... ls_d, rho) of cells [G x (d + 1)].  N <= 64 and a family of HYPER_CELLS_KERNELS: one launch of the
        wave-per-cell kernel (csrc/hyper_wave.hip) and one read-back; otherwise nlml_hyper() cell by cell - the same values
        within rounding, one factorisation and one read-back per cell.  A row is NaN in all three entries where nlml_hyper()'s
        outputs are NaN (matrix not positive definite, scale^2 not positive); the loop also answers NaN for rho <= 0, which the
        kernel takes as it comes.  d <= 16; the surrogate held by this object is not touched."""
        return self.nlml_hyper_cells_fn(X, y, fit_mean, fit_scale, kernel, route)(cells)

    def loo(self, scale2: float = 1.0):
        """Leave-one-out prediction of every observation from the factorisation held by this object (gpbo_loo_f64: the diagonal
        of K^-1 is the row sums of squares of U, so nothing is refitted): device tensors (mu [N], var [N], kinv_diag [N]) in
        the CALLER's row order (factorise(order="fps") is undone), mu_i = y_i - alpha_i / kinv_diag_i and
        var_i = scale2 / kinv_diag_i in the units of the y that was factorised.  Enqueues only."""
        torch = self.torch
        if self.N < 1:
            raise _lib.GpboError("loo() needs a factorised surrogate")
        scale2 = float(scale2)
        if not (np.isfinite(scale2) and scale2 > 0.0):
            raise ValueError(f"scale2 must be positive and finite, got {scale2!r}")
        with torch.cuda.device(self.device):
            need = int(self.lib.gpbo_loo_workspace_bytes(self.Np))
            work = self._workspace("_work_loo", need)
            out = torch.empty((3, self.N), dtype=torch.float64, device=self.device)
            _lib.call(self.lib.gpbo_loo_f64, self.U, self.alpha, self.y, self.N, self.Np, scale2, out[0], out[1], out[2], work,
                      need, self._stream())
            if self.perm is not None:   # row i of the factorisation is the caller's row perm[i]
                back = torch.empty_like(out)
                back[:, self.perm[: self.N]] = out
                out = back
        return out[0], out[1], out[2]

    # -- dense covariance blocks for inspection (small problems only) --------------------------------------
    def cov_meas_host(self) -> np.ndarray:
        """cov_meas (point_selector.py:79) in the caller's order of the observations."""
        K = self.K[: self.N, : self.N].cpu().numpy()
        p = self._perm_host()
        if p is None:
            return K
        Ka = np.empty_like(K)
        Ka[np.ix_(p, p)] = K
        return Ka

    def kxx_host(self, P, ls, jitter1, jitter2) -> np.ndarray:
        """k(P,P) of the surrogate's covariance family with the reference's jitter, as a host array (used for `cov_pred` on small
        grids)."""
        torch = self.torch
        Pd = self._dev(P)
        n, d = int(Pd.shape[0]), int(Pd.shape[1])
        npad = int(self.lib.gpbo_padded_n(n))
        ls_h = np.ascontiguousarray(np.asarray(ls, dtype=np.float64).reshape(-1))
        with torch.cuda.device(self.device):
            Kp = torch.empty((npad, npad), dtype=torch.float64, device=self.device)
            _lib.call(self.lib.gpbo_kxx_kern_f64, Pd, n, d, ls_h, self._kid(), jitter1, jitter2, Kp, npad, self._stream())
            return Kp[:n, :n].cpu().numpy()

    def cov_meas_pred_host(self, Xs, diag_add: float = 0.0) -> np.ndarray:
        """K(X*, X) as an (M, N) host array  (point_selector.py:81); small problems only."""
        torch = self.torch
        Xsd = self._dev(Xs)
        M = int(Xsd.shape[0])
        ldk = _round_up(M)
        with torch.cuda.device(self.device):
            kst = torch.empty((self.Np, ldk), dtype=torch.float64, device=self.device)
            mup = torch.empty((self.Np // 64, ldk), dtype=torch.float64, device=self.device)
            xsc = torch.empty((self.Np, self.d), dtype=torch.float64, device=self.device)
            _lib.call(self.lib.gpbo_scale_points_f64, *self._head(), xsc, self._stream())
            _lib.call(self.lib.gpbo_kstar_mu_kern_f64, Xsd, M, xsc, self.N, self.Np, self.d, self.ls_h, self._kid(),
                      self.alpha, float(diag_add), 0, kst, ldk, mup, self._stream())
            Kf = kst[: self.N, :M].t().contiguous().cpu().numpy()
        p = self._perm_host()
        if p is None:
            return Kf
        Ka = np.empty_like(Kf)   # columns back in the caller's order of the observations
        Ka[:, p] = Kf
        return Ka
