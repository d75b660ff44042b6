"""Drop-in replacement for the reference's `PointSelector` running on the MI355X kernels.

Same attribute protocol and call sequence as /root/reference/point_selector.py:13-207 as driven by
/root/reference/select_parameters.py:146-157 and :282-293:

    ps = PointSelector(); ps.name = ...; ps.iteration = ...
    ps.measured_pts, ps.measured_vals, ps.feature_domain, ps.predicted_pts, ps.length_scales = ...
    ps.update_surrogate()
    idx = ps.lower_confidence_bound()          # np.ndarray[int64], one entry per feature axis
    ps.mean_func, ps.cov_func, ps.acq_func_eval, ps.kernel_params

Differences from the reference, all deliberate:
  * `cov_pred` (the M x M predictive covariance, :78) is never needed - only its diagonal is - and
    is materialised only when M <= COV_PRED_MAX_M; `cov_meas_pred` (:81) only when M*N is small.
  * Failures raise instead of returning garbage: numpy.linalg.LinAlgError when K is not positive
    definite, IndexError when the acquisition contains NaN (the reference's own failure at :207).
  * Extra, not in the reference: `precision="fp32"` / `"i8"` / `"i8c"` (fp64 factorisation and means; the N^2 variance
    product as an fp32 / int8-sliced / three-digit int8 SCREEN).  In these modes EVERY acquisition call - LCB with any
    `explore`, EI - returns the index the fp64 kernels decide (screen + fp64 re-score of the survivors with THAT
    acquisition), `mean_func` is the fp64 kernels' bit for bit, and `cov_func` / `acq_func_eval` are the SCREEN's:
    |cov_func - fp64| <= SCREEN_SIGMA_TOL[precision] (5e-3 for fp32 and i8c, 2e-9 for i8; also in `last_screen`), so the
    arg-max of `acq_func_eval` itself can differ from the returned index when two candidates are closer than that.
    A caller that plots or post-processes these arrays at the reference's 1e-8 should stay with precision="fp64".
    The screens' tolerance is verified per call on every re-scored candidate and a strided sample, not proven for each
    candidate: the route that is exact by construction is `dense_outputs=False` (the prefix bound).
    Also extra: `expected_improvement(xi)`, `noisy_expected_improvement()` (EI averaged over samples of the best latent value at
    the observed points instead of measured against min(measured_vals), the luckiest noise draw: INTEGRATION.md 9),
    `max_value_entropy_search()` (the information gained about the minimum's value: no incumbent, no trade-off parameter;
    INTEGRATION.md 10), `constrained_expected_improvement()` / `probability_of_feasibility()` (black-box constraints, each a
    selector object of its own; evaluated in log space) and `probability_of_improvement()`,
    `expected_hypervolume_improvement()` (two objectives, the second a selector object of its own),
    `q_expected_improvement()`, `select_thompson(q)` (q points as the minimisers of posterior sample paths), `select_batch(q)` (q points for parallel evaluation: greedy Kriging believer / GP-BUCB /
    constant liar), `refine_next()` (the next point off the grid: the best candidates polished by acquisition gradients), `dense_outputs=False` (next point only: the dense attributes stay None and the acquisition
    calls go through the exact prefix bound), `kernel_params` may be preset (then no
    ARD search runs), optional multi-GPU candidate sharding when torch.distributed is initialised,
    `incremental=True` / `state_path=...` (append new observations to the previous factorisation in O(N^2)
    while the length scales stay the same, within one process or across jobs through a state file), and
    `ard="gradient"` (fit the length scales by maximising the marginal likelihood with its gradient instead of the grid
    search; INTEGRATION.md "ARD fit modes"), and `ard="hyper"` (fit noise, signal variance and a constant mean together with
    the length scales; every attribute and acquisition value is then in the units of `measured_vals`: INTEGRATION.md
    "Fitting the whole model"), and `ard="marginal"` (that fit, then LCB / EI, `mean_func` and `cov_func` integrated over
    `n_models` samples of the hyperparameter posterior: INTEGRATION.md "Integrating over the hyperparameters").
Layout: what the surrogate IS besides its length scales (covariance family, diagonal terms, the units of y) is one record,
model.SurrogateModel, built once per update_surrogate() and read by every later call; what `length_scales` spans is one
model.LengthScaleSpace, which _select_kernel_params / tune_kernel / _fit_kernel ask for the middle, the box, the grid and the
shape of kernel_params.  update_surrogate()'s prologue and epilogue (_begin_update, _publish) and the tail of every
acquisition call (_finish) are shared with PointSelectorHost, which supplies its own "score this acquisition" (_score_acq).
There is no CPU implementation behind this class.
"""
from __future__ import annotations

import numpy as np

from . import distributed as D
from .gp_device import NAN_ACQUISITION, DeviceGP
from .model import LengthScaleSpace, SurrogateModel, need_se

COV_PRED_MAX_M = 4096          # cov_pred is M x M: 128 MiB at this size
COV_MEAS_PRED_MAX = 1 << 24    # entries of the (M, N) cross covariance kept for inspection
MAX_APPEND_ROWS = 64           # more new rows than this: a fresh factorisation is cheaper than row-by-row appends
MAX_APPENDED_COLUMNS = 256     # columns built by appends since the last full factorisation before a refresh is due
# |cov_func - fp64 sigma| of the screened precisions (asserted in tests/test_gpu_parity.py, test_gpu_i8.py, test_gpu_i8c.py)
SCREEN_SIGMA_TOL = {"fp32": 5e-3, "i8": 2e-9, "i8c": 5e-3}


def _plot_hooks():
    """The reference star-imports plot_utils (point_selector.py:4) and calls plot_ARD_LL{,_1d} from
    tune_kernel (:146,163).  If that module is importable (the DAG's working directory) use it."""
    try:
        import plot_utils  # type: ignore

        return getattr(plot_utils, "plot_ARD_LL", None), getattr(plot_utils, "plot_ARD_LL_1d", None)
    except Exception:  # noqa: BLE001 - plotting is a side output, never a reason to fail the step
        return None, None


class PointSelector:
    def __init__(self, device=None, verbose: bool = False, shard_candidates: bool = True, precision: str = "fp64",
                 incremental: bool = False, state_path=None, dense_outputs: bool = True, likelihood: str = "reference",
                 ard: str = "grid", noise0: float = 1e-2, noise_bounds=(1e-6, 1.0), kernel: str = "se", n_models: int = 16,
                 posterior_sweeps: int = 10, seed: int = 0):
        # attribute protocol of point_selector.py:15-40
        self.feature_domain = None
        self.predicted_pts = None
        self.measured_vals = []
        self.measured_pts = []
        self.mean_func = None
        self.cov_func = None
        self.acq_func_eval = None
        self.hyperparam_obj = []
        self.length_scales = None
        self.kernel_params = None
        self.gradient_steps = 0.001
        self.iteration = None
        self.name = None
        # cov_pred / cov_meas / cov_meas_pred (:38-40) are properties below: built on first access
        self._lazy = {}
        self._cov = {"cov_pred": None, "cov_meas": None, "cov_meas_pred": None}
        # build-specific
        self.nlogml = None
        self._device = device
        self._verbose = verbose
        self._shard = shard_candidates
        if precision not in ("fp64", "fp32", "i8", "i8c"):
            raise ValueError("precision must be 'fp64' (reference arithmetic), 'fp32', 'i8' or 'i8c' (fp64 factorisation, "
                             "means and decision; variance product screened in fp32 / in int8 slices / in three int8 digits)")
        self._precision = precision
        # likelihood="reference" (default): tune_kernel's grid holds the reference's float32 values, det underflow
        # included (point_selector.py:117-119: -inf beyond N ~ 100, where the search then returns its first cell);
        # "logdet" (not in the reference): fp64 grid with log det K from the Cholesky factor - finite at any N.
        if likelihood not in ("reference", "logdet"):
            raise ValueError("likelihood must be 'reference' (the reference's np.log(np.linalg.det(K))) or 'logdet'")
        self._likelihood = likelihood
        # ard="grid" (default): tune_kernel searches the length-scale grid as the reference does (point_selector.py:104-163);
        # "gradient" (not in the reference): ML-II fit of all d length scales at once inside the box the search axes span,
        # projected L-BFGS on the fp64 log-det likelihood and its gradient (ard_fit.py, csrc/ard_grad.hip)
        # "hyper" (not in the reference, whose model is frozen at unit signal variance, zero mean and a diagonal term of
        # 1e-4 + 1e-6): the same fit over d + 1 variables - the length scales and the noise-to-signal ratio rho, started at
        # noise0 inside noise_bounds - with the constant mean m and the signal variance s^2 at their closed-form optima
        # (csrc/hyper.hip).  The surrogate is then the GP of (y - m) / s with K = k(X,X) + rho I and prior variance 1 + rho,
        # and everything this class reports is mapped back to the units of y.
        # "marginal" (not in the reference): everything "hyper" does, then the acquisition INTEGRATED over the hyperparameter
        # posterior (Snoek, Larochelle & Adams 2012): n_models chains of slice sampling in (log ls, log rho), started at the
        # optimum and run for posterior_sweeps sweeps (hyper_posterior.py, every step one launch of csrc/hyper_wave.hip),
        # give an equal-weight ensemble of models (ensemble.py, csrc/ensemble.hip); mean_func / cov_func are the mean and the
        # standard deviation of the mixture of their predictions, LCB / EI the average of theirs.  One seed, one result.
        if ard not in ("grid", "gradient", "hyper", "marginal"):
            raise ValueError("ard must be 'grid' (the reference's grid search), 'gradient' (ML-II fit of the length scales), "
                             "'hyper' (ML-II fit of length scales, noise, signal variance and mean) or 'marginal' (that fit, "
                             "then the acquisition integrated over samples of the hyperparameter posterior)")
        self._ard = ard
        self._fits_model = ard in ("hyper", "marginal")   # the surrogate is a fitted model.SurrogateModel, in the units of y
        from ._lib import ENSEMBLE_MAX_S
        if int(n_models) != n_models or not 1 <= int(n_models) <= ENSEMBLE_MAX_S:
            raise ValueError(f"n_models must be an integer in [1, {ENSEMBLE_MAX_S}], got {n_models!r}")
        if int(posterior_sweeps) != posterior_sweeps or int(posterior_sweeps) < 0:
            raise ValueError(f"posterior_sweeps must be a non-negative integer, got {posterior_sweeps!r}")
        self._n_models, self._posterior_sweeps, self._seed = int(n_models), int(posterior_sweeps), int(seed)
        self.hyper_samples = None      # ard="marginal": the sampled models of the last update_surrogate() (dict)
        self._ens = None
        nlo, nhi = (float(v) for v in noise_bounds)
        if not (0.0 < nlo <= nhi < np.inf) or not nlo <= float(noise0) <= nhi:
            raise ValueError("noise_bounds must satisfy 0 < lower <= upper < inf and hold noise0")
        self._noise0, self._noise_bounds = float(noise0), (nlo, nhi)
        if self._fits_model:
            if precision != "fp64":
                raise ValueError(f"ard={ard!r} needs precision='fp64' (the screens are tuned to the reference's prior variance)")
            if incremental or state_path is not None:
                raise ValueError(f"ard={ard!r} refits the model at every update: incremental / state_path are not available")
            if not dense_outputs:
                raise ValueError(f"ard={ard!r} needs dense_outputs=True (the prefix bound assumes the reference's jitters)")
        # kernel="se" (default): the reference's squared exponential, every code path as it was.  "matern32" / "matern52" (not in
        # the reference, whose docs name them as its first planned improvement): the Matern families on the fp64 path -
        # factorisation, scoring, LCB / EI, loo() and the ML-II fits (ard="gradient" / "hyper", or preset kernel_params);
        # everything built on squared-exponential kernels of its own is refused here or at the call.
        from ._lib import kernel_id
        kernel_id(kernel)
        self._kernel = kernel
        self._model = SurrogateModel(kernel)   # rebuilt by every update_surrogate(): what the surrogate is, besides its length scales
        if kernel != "se":
            if ard == "grid":
                raise ValueError(f"kernel={kernel!r} with ard='grid': the grid kernels generate squared-exponential entries; use "
                                 "ard='gradient', ard='hyper' or ard='marginal' (preset kernel_params still skip the search)")
            if precision != "fp64":
                raise ValueError(f"kernel={kernel!r} needs precision='fp64', got precision={precision!r} (the screens build "
                                 "squared-exponential entries)")
            if incremental or state_path is not None:
                raise ValueError(f"kernel={kernel!r}: incremental / state_path are not available (append() and the state file "
                                 "are squared-exponential only)")
            if not dense_outputs:
                raise ValueError(f"kernel={kernel!r} needs dense_outputs=True (dense_outputs=False goes through the prefix "
                                 "bound, which is squared-exponential only)")
        self.noise = None              # ard="hyper": fitted noise-to-signal ratio rho (noise variance = rho y_scale^2)
        self.y_mean = None             # ard="hyper": fitted constant mean m, in the units of measured_vals
        self.y_scale = None            # ard="hyper": fitted signal standard deviation s, in the units of measured_vals
        self.last_fit = None           # ard="gradient" / "hyper": the last fit (ard_fit.FitResult.as_dict())
        # dense_outputs=False (not in the reference): a caller that needs the next point only.  mean_func / cov_func /
        # acq_func_eval stay None and the acquisition calls return the same multi-index through the exact prefix bound
        # (DeviceGP.score_bound: fp64 branch and bound, the full pass when the bound does not separate the candidates).
        self._dense = bool(dense_outputs)
        self._gp = None
        self._mu_dev = self._sigma_dev = None
        self._cand = None              # (this rank's candidates on the device, diag_add) of the last update_surrogate()
        self._cached = None  # (kind, p0, p1) -> (acq ndarray, flat index)
        self._preset_kernel_params = False
        self._ls_cells = None          # explicit [G x d] cell list for d > 2 (set_length_scale_cells)
        self.ard_sweeps = 2            # passes of the coordinate-wise search when length_scales holds d > 2 axes
        # consecutive iterations differ by one observed row (select_parameters.py:163,299)
        self._incremental = bool(incremental) or state_path is not None
        self._state_path = state_path
        self._inc = None               # (X, y, ls) of the factorisation held by self._gp
        self.last_update = None        # "factorise" | "append": what the last update_surrogate() did
        self.last_screen = None        # screened precisions: DeviceGP.last_screen of the last acquisition + sigma_abs_tol
        self.fantasy_best = None       # noisy_expected_improvement(): the incumbent of every fantasy [S], in the units of y
        self.sampled_minima = None     # max_value_entropy_search(): the sampled values of the minimum [S], in the units of y
        self.log_feasibility = None    # the constrained calls: the dense log-probability that every constraint holds
        self.constrained_base = None   # ... the base term that was used: "ei", "pi", or "none" (no feasible observation: the
        #                                probability of feasibility alone was maximised) ...
        self.constrained_incumbent = None   # ... and the incumbent it was measured against, in the units of y (None: no base)
        self.pareto_front = None       # expected_hypervolume_improvement(): the front [P x 2] that was used, in the units of y ...
        self.reference_point = None    # ... the reference point (r1, r2) ...
        self.hypervolume = None        # ... and the area below it that the front dominates

    # ------------------------------------------------------------------------------------------
    def _cov_get(self, name):
        make = self._lazy.pop(name, None)
        if make is not None:
            self._cov[name] = make()
        return self._cov[name]

    def _cov_set(self, name, value):
        self._lazy.pop(name, None)
        self._cov[name] = value

    cov_pred = property(lambda self: self._cov_get("cov_pred"), lambda self, v: self._cov_set("cov_pred", v),
                        doc="k(X*,X*) + 1e-6 I (point_selector.py:78); None above COV_PRED_MAX_M candidates")
    cov_meas = property(lambda self: self._cov_get("cov_meas"), lambda self, v: self._cov_set("cov_meas", v),
                        doc="k(X,X) + 1e-6 I (point_selector.py:79)")
    cov_meas_pred = property(lambda self: self._cov_get("cov_meas_pred"),
                             lambda self, v: self._cov_set("cov_meas_pred", v),
                             doc="k(X,X*).T (point_selector.py:81); None above COV_MEAS_PRED_MAX entries")

    def _need_update(self):
        if self._cached is None:
            raise RuntimeError("call update_surrogate() first")

    def _log(self, *a):
        if self._verbose:
            print(*a)

    def _world(self):
        if not self._shard:
            return 1, 0
        import torch.distributed as dist

        if dist.is_available() and dist.is_initialized():
            return dist.get_world_size(), dist.get_rank()
        return 1, 0

    def set_length_scale_cells(self, cells):
        """d > 2 (not in the reference, whose tune_kernel builds a 1-D or 2-D grid only, point_selector.py:122-163):
        an explicit list of length-scale vectors [G x d]; tune_kernel() evaluates the reference's likelihood
        (:111-120) in every cell on the GPU and keeps the FIRST minimum (np.argwhere(g == amin)[0], as :141,159)."""
        self.length_scales = None
        self._ls_cells = np.ascontiguousarray(np.asarray(cells, dtype=np.float64))
        if self._ls_cells.ndim != 2:
            raise ValueError("cells must be a [G x d] array of length-scale vectors")
        self._preset_kernel_params = False

    def set_kernel_params(self, kernel_params):
        """Preset length scales: update_surrogate() then skips the ARD grid search (needed for d > 2,
        where the reference's tune_kernel cannot run at all)."""
        self.kernel_params = np.asarray(kernel_params, dtype=np.float64)
        self._preset_kernel_params = True

    # ------------------------------------------------------------------------------------------
    def _begin_update(self):
        """The prologue of update_surrogate() (point_selector.py:42-73): (X, y, X*, length scales) as fp64 arrays, with the
        length scales chosen and the model record of this update built."""
        self.measured_pts = np.array(self.measured_pts)
        self.measured_vals = np.array(self.measured_vals)
        X = np.asarray(self.measured_pts, dtype=np.float64)
        y = np.asarray(self.measured_vals, dtype=np.float64)
        Xs = np.asarray(self.predicted_pts, dtype=np.float64)
        ls = self._select_kernel_params(X)
        # ard="hyper": the fitted model, the GP of (y - m) / s with K = k(X,X) + rho I; otherwise the reference's frozen one
        fit = (self.noise, 0.0, self.y_mean, self.y_scale, True) if self._fits_model else ()
        self._model = SurrogateModel(self._kernel, *fit)
        return X, y, Xs, ls

    def _publish(self, mu, sigma, acq, best):
        """The epilogue of update_surrogate() (:97-102), everything in the units of y: mean_func, cov_func, the LCB(4) entry
        of the acquisition cache, and measured_* back as lists."""
        fd = [int(v) for v in self.feature_domain]
        self.mean_func = mu.reshape(fd)                                   # :97
        self.cov_func = sigma.reshape(fd)                                 # :98 (a standard deviation)
        self._cached = {("lcb", 4.0, 0.0): (acq.reshape(fd), best)}
        self.measured_pts = self.measured_pts.tolist()                    # :101-102
        self.measured_vals = self.measured_vals.tolist()

    def update_surrogate(self):
        """point_selector.py:42-102."""
        X, y, Xs, ls = self._begin_update()
        model = self._model
        if self._gp is None:
            self._gp = DeviceGP(self._device)
        gp = self._gp
        self._factorise_or_append(gp, X, model.to_model(y), ls)           # :79, :89 (raises LinAlgError)

        M, N = len(Xs), len(X)
        diag_add = model.diag_add(Xs.shape, X.shape)                      # :173 shape-coincidence quirk
        world, rank = self._world()
        lo, hi = D.shard_bounds(M, world, rank)
        self._lo_hi = (lo, hi)
        self._cand = (gp._dev(Xs[lo:hi]), diag_add)   # this rank's candidates on the device: every later call scores these
        self._cov = {"cov_pred": None, "cov_meas": None, "cov_meas_pred": None}
        self._lazy = {"cov_meas": gp.cov_meas_host}
        self._mu_dev = self._sigma_dev = None
        if self._ard == "marginal":
            self._update_marginal(X, y, Xs, ls, lo, hi)
            return
        if not self._dense:
            self.mean_func = self.cov_func = self.acq_func_eval = None
            self._cached = {}
            self.measured_pts = self.measured_pts.tolist()
            self.measured_vals = self.measured_vals.tolist()
            return
        if self._precision != "fp64":   # screened variance product (fp32: BASELINE config 4's mode), fp64 decision
            res = self._score_screened("lcb", explore=4.0)
        else:
            res = gp.score(self._cand[0], acquisition="lcb", explore=4.0, dense=True, idx_offset=lo, diag_add=diag_add,
                           prior_var=model.prior_var)
        self._mu_dev, self._sigma_dev = res.mu, res.sigma                 # (in the units of the model)
        best = D.allreduce_argmax(res.best_val, res.best_idx, res.nan_count)
        # sharded: the three dense arrays are gathered on the device (one collective), then copied to the host once
        mu, sigma, acq = (t.cpu().numpy() for t in D.gather_concat_tensors([res.mu, res.sigma, res.acq], M))
        self._publish(model.mean_to_y(mu), model.sd_to_y(sigma), model.acq_to_y("lcb", acq), model.best_to_y("lcb", best))

        # The three covariance attributes of point_selector.py:38-40 are read by nobody on the reference's call path
        # (select_parameters.py reads mean_func / cov_func / acq_func_eval only): they are copied out of the device
        # on first access instead of on every call (the 2,500 x 2,500 cov_pred copy was 6.4 of 7.9 ms of a C1 step).
        self._lazy_cov_pred(gp, Xs, ls, model, diag_add)

    def _lazy_cov_pred(self, gp, Xs, ls, model, diag_add):
        M, N = len(Xs), gp.N
        if M * N <= COV_MEAS_PRED_MAX:
            self._lazy["cov_meas_pred"] = lambda: gp.cov_meas_pred_host(Xs, diag_add)
        if M <= COV_PRED_MAX_M:
            self._lazy["cov_pred"] = lambda: gp.kxx_host(Xs, ls, model.jitter1, model.jitter2)

    def _update_marginal(self, X, y, Xs, ls, lo, hi):
        """update_surrogate() with ard="marginal", behind the ML-II fit and the factorisation of its model (kernel_params,
        noise, y_mean, y_scale, last_fit, the cov_* attributes and loo() stay that model's): sample the hyperparameter
        posterior from the optimum, factorise the ensemble, publish the integrated mean_func / cov_func / LCB(4).  With
        several ranks every rank samples the same chains with the same deterministic kernels (as _fit_kernel): no collective
        before the arg-max."""
        from . import hyper_posterior
        from .ensemble import DeviceEnsemble

        gp, model, d = self._gp, self._model, X.shape[1]
        S = self._n_models
        if len(X) < 2:
            # one observation: nothing to sample from; the single model of the one-observation branch
            cells = np.concatenate([ls, [self.noise]])[None, :]
            prof = np.array([[np.nan, self.y_mean, self.y_scale ** 2]])
            counters = dict(n_batches=0, min_margin=float("inf"), kept=0)
        else:
            lower, upper, _ = self._space(d).box_and_start()
            zlo = np.log(np.concatenate([lower, [self._noise_bounds[0]]]))
            zhi = np.log(np.concatenate([upper, [self._noise_bounds[1]]]))
            cells_fn = gp.nlml_hyper_cells_fn(X, y, True, True, self._kernel)
            z0 = np.tile(np.log(np.concatenate([ls, [self.noise]])), (S, 1))
            r = hyper_posterior.sample(lambda Z: cells_fn(np.exp(Z))[:, 0], z0, zlo, zhi, self._posterior_sweeps, self._seed)
            cells = np.exp(r.states)
            prof = cells_fn(cells)   # (L, m, s^2) of the final states
            counters = dict(n_batches=r.n_batches + 1, min_margin=r.min_margin, kept=r.kept)
        n = len(cells)
        w = np.full(n, 1.0 / n)
        self.hyper_samples = dict(ls=cells[:, :d].copy(), noise=cells[:, d].copy(), y_mean=prof[:, 1].copy(),
                                  y_scale=np.sqrt(prof[:, 2]), weight=w, nlml=prof[:, 0].copy(),
                                  sweeps=self._posterior_sweeps, seed=self._seed, **counters)
        hs = self.hyper_samples
        models = [(hs["ls"][s], SurrogateModel(self._kernel, float(hs["noise"][s]), 0.0, float(hs["y_mean"][s]),
                                               float(hs["y_scale"][s]), True), float(w[s])) for s in range(n)]
        if self._ens is None:
            self._ens = DeviceEnsemble(self._device)
        self._ens.factorise(X, y, models)                                 # (raises LinAlgError naming the model)
        res = self._ens.score(self._cand[0], acquisition="lcb", explore=4.0, dense=True, idx_offset=lo)
        best = D.allreduce_argmax(res.best_val, res.best_idx, res.nan_count)
        mean, sd, acq = (t.cpu().numpy() for t in D.gather_concat_tensors([res.mean, res.sd, res.acq], len(Xs)))
        self._publish(mean, sd, acq, best)                                # (the ensemble reports in the units of y)
        self._lazy_cov_pred(gp, Xs, ls, model, 0.0)

    def _not_in_marginal_mode(self, what: str):
        if self._ard == "marginal":
            raise ValueError(f"{what} is not available with ard='marginal' (it works on one model's posterior): use "
                             "lower_confidence_bound() / expected_improvement(), or ard='hyper'")

    def _space(self, d: int) -> LengthScaleSpace:
        return LengthScaleSpace(self.length_scales, self._ls_cells, d)

    def _select_kernel_params(self, X) -> np.ndarray:
        """point_selector.py:60-73: preset, ARD grid search (n > 1) or the middle of each length-scale axis."""
        if self._fits_model and self._preset_kernel_params:
            raise ValueError(f"ard={self._ard!r} fits the length scales with the rest of the model: set_kernel_params() is not "
                             "available")
        if self._fits_model and len(X[:, 0]) < 2:
            # nothing to fit from one observation: the mean is that observation, unit scale, the starting noise
            self.noise, self.y_mean, self.y_scale = self._noise0, float(np.asarray(self.measured_vals, dtype=np.float64)[0]), 1.0
            self.last_fit = None
        if self._preset_kernel_params:
            pass
        elif len(X[:, 0]) > 1:                                           # :60
            self.tune_kernel()
        else:                                                            # :63-73
            self.kernel_params = self._space(X.shape[1]).middle()
        return np.asarray(self.kernel_params, dtype=np.float64).reshape(-1)

    def _factorise_or_append(self, gp, X, y, ls):
        """Full factorisation, or - with incremental=True / a state file - O(N^2) appends when the new data are
        the old data plus a few rows and the length scales are bit-identical to those of the held factors."""
        import os

        model = self._model
        appended = False
        world, rank = self._world()
        if self._incremental:
            if self._inc is None and self._state_path is not None and os.path.exists(self._state_path):
                try:
                    gp.load_state(self._state_path)
                    self._inc = (*gp.observations_host(), np.array(gp.ls_h))   # in the caller's order
                except Exception as exc:  # noqa: BLE001 - an unreadable state file only costs the shortcut
                    self._log(f"state file {self._state_path!r} ignored: {exc}")
                    self._inc = None
            can_append = False
            if self._inc is not None:
                X0, y0, ls0 = self._inc
                n0 = len(X0)
                can_append = (n0 < len(X) <= n0 + MAX_APPEND_ROWS and gp.N == n0 and X0.shape[1:] == X.shape[1:]
                              and gp.n_appended + (len(X) - n0) <= MAX_APPENDED_COLUMNS
                              and ls0.shape == ls.shape and np.array_equal(ls0, ls)
                              and gp.jitter1 == model.jitter1 and gp.jitter2 == model.jitter2
                              and np.array_equal(X[:n0], X0) and np.array_equal(y[:n0], y0)
                              # (a permuted factorisation cannot carry the N == M quirk, which is keyed on the arrival index)
                              and (gp.perm is None or np.shape(self.predicted_pts) != np.shape(X)))
            # the route is a collective decision: a rank that appends while another refactorises would hold factors
            # that differ at rounding level, and the lowest-index tie rule across shards assumes identical factors
            if D.all_agree(can_append) if self._shard else can_append:
                try:
                    for i in range(n0, len(X)):
                        gp.append(X[i], y[i])
                    appended = True
                except np.linalg.LinAlgError:
                    pass  # numerically singular through the update: the full route decides (and raises if so)
                if self._shard:
                    appended = D.all_agree(appended)
        if not appended:
            # next point only (dense_outputs=False): the acquisition calls prune by the first observations of the
            # factorisation (DeviceGP.score_bound), so those are chosen to cover the region whatever the order of the
            # history; not with the N == M quirk, which is keyed on the arrival index (:173)
            fps = not self._dense and np.shape(self.predicted_pts) != np.shape(X)
            gp.factorise(X, y, ls, model.jitter1, model.jitter2, check=True, order="fps" if fps else "arrival",
                         kernel=model.kernel)
            if fps and self._shard and self._world()[0] > 1:
                # the order is part of the factorisation: if the selection fell back to the arrival order on ANY rank, every
                # rank refactorises in arrival order (identical factors on all shards: the cross-shard tie rule needs them)
                if not D.all_agree(not gp.order_fell_back()):
                    gp.factorise(X, y, ls, model.jitter1, model.jitter2, check=True, order="arrival", kernel=model.kernel)
        self.last_update = "append" if appended else "factorise"
        if self._incremental:
            self._inc = (X.copy(), y.copy(), ls.copy())
            if self._state_path is not None and rank == 0:   # one writer; DeviceGP.save_state renames atomically
                gp.save_state(self._state_path)

    def _nlml_cells(self, X, y, cells) -> np.ndarray:
        """The likelihood of every grid cell; with several ranks each evaluates a contiguous block of cells
        (independent factorisations) and the float32 values are concatenated on every rank."""
        world, rank = self._world()
        kw = {} if self._likelihood == "reference" else {"likelihood": self._likelihood}
        if world == 1 or len(cells) < world:
            return self._gp.nlml_grid(X, y, cells, **kw)
        lo, hi = D.shard_bounds(len(cells), world, rank)
        return D.gather_concat(self._gp.nlml_grid(X, y, cells[lo:hi], **kw), len(cells))

    # ------------------------------------------------------------------------------------------
    def tune_kernel(self):
        """ARD grid search, point_selector.py:104-163: float32 nlml grid on the GPU, first row-major
        minimum on the host (np.argwhere(g == amin)[0]; NaN -> IndexError, as in the reference)."""
        X = np.asarray(self.measured_pts, dtype=np.float64)
        y = np.asarray(self.measured_vals, dtype=np.float64)
        plot2, plot1 = _plot_hooks()
        if self._gp is None:
            self._gp = DeviceGP(self._device)
        if self._ard in ("gradient", "hyper", "marginal"):
            self._fit_kernel(X, y)
            return
        space = self._space(X.shape[1])
        self.kernel_params, self.nlogml = space.search(lambda cells: self._nlml_cells(X, y, cells), int(self.ard_sweeps))
        plot = {"grid2": plot2, "grid1": plot1}.get(space.kind)          # :146, :163
        if plot is not None:
            try:
                plot(self.nlogml, self.kernel_params, self.length_scales, self.name, self.iteration)
            except Exception:  # noqa: BLE001
                pass

    def _fit_kernel(self, X, y):
        """tune_kernel with ard="gradient" / "hyper": box, start and the shape of kernel_params from the search space
        (LengthScaleSpace.box_and_start), the objective always the fp64 log-det likelihood: the reference's log(det K) is
        -inf beyond N ~ 100 and has no gradient.  hyperparam_obj (point_selector.py:30) receives the accepted likelihood
        values.  With several ranks every rank fits the same problem with the same deterministic kernels: no collective."""
        space = self._space(X.shape[1])
        lower, upper, ls0 = space.box_and_start()
        if self._fits_model:
            # the same box and start for the length scales; the noise-to-signal ratio joins them, mean and scale are profiled
            if np.ptp(y) == 0.0:
                raise np.linalg.LinAlgError("the likelihood is not finite: constant measured_vals leave no signal variance to fit")
            res = self._gp.fit_hyperparameters(X, y, ls0, lower, upper, self._noise0, *self._noise_bounds, kernel=self._kernel)
            self.noise, self.y_mean, self.y_scale = float(res.noise), float(res.mean), float(res.scale)
        else:
            res = self._gp.fit_length_scales(X, y, ls0, lower, upper, kernel=self._kernel)
        self.kernel_params = space.fitted(res.ls)
        self.hyperparam_obj = [float(v) for v in res.trace]
        self.nlogml = np.asarray(res.trace, dtype=np.float64)
        self.last_fit = res.as_dict()
        if self._fits_model:
            self.last_fit.update(y_mean=self.y_mean, y_scale=self.y_scale)
        self._log(f"ARD fit: {res.reason} after {res.n_iter} steps / {res.n_eval} evaluations, nlml {res.nlml:.12g}")

    # ------------------------------------------------------------------------------------------
    _NEGATIVE_INDEX_IS_NAN = False   # (PointSelectorHost: a negative arg-max index also raises the NaN IndexError)

    def _score_screened(self, kind, **kw):
        """A screen pass with this acquisition, then the fp64 kernels on every survivor; last_screen says how it went."""
        score = {"fp32": self._gp.score_f32, "i8": self._gp.score_i8, "i8c": self._gp.score_i8c}[self._precision]
        res = score(self._cand[0], acquisition=kind, dense=True, idx_offset=self._lo_hi[0], diag_add=self._cand[1], **kw)
        self.last_screen = dict(self._gp.last_screen, sigma_abs_tol=SCREEN_SIGMA_TOL[self._precision])
        return res

    def _score_acq(self, kind, **kw):
        """(acquisition values over all candidates [M] or None, (best value, flat index, NaN count)) of an acquisition that
        is not in the cache, in the units of y: what each class provides to _finish."""
        model, lo = self._model, self._lo_hi[0]
        if self._ard == "marginal":   # one more pass of the ensemble; its parameters and values are in the units of y
            res = self._ens.score(self._cand[0], acquisition=kind, dense=True, idx_offset=lo, **kw)
            best = D.allreduce_argmax(res.best_val, res.best_idx, res.nan_count)
            M = int(np.prod([int(v) for v in self.feature_domain]))
            return D.gather_concat_tensors([res.acq], M)[0].cpu().numpy(), best
        if not self._dense:
            res = self._gp.score_bound(self._cand[0], acquisition=kind, idx_offset=lo, diag_add=self._cand[1], **kw)
            return None, D.allreduce_argmax(res.best_val, res.best_idx, res.nan_count)
        if self._precision != "fp64":
            # screened precision: the stored sigma is the screen's, so the decision for THIS acquisition is made the
            # way the cached LCB(4) one was
            res = self._score_screened(kind, **kw)
        else:
            res = self._gp.acquisition_on_posterior(self._mu_dev, self._sigma_dev, acquisition=kind, idx_offset=lo,
                                                    **model.acq_kw(kw))
        best = D.allreduce_argmax(res.best_val, res.best_idx, res.nan_count)
        M = int(np.prod([int(v) for v in self.feature_domain]))
        return model.acq_to_y(kind, D.gather_concat_tensors([res.acq], M)[0].cpu().numpy()), model.best_to_y(kind, best)

    def _finish(self, key, kind, **kw):
        fd = [int(v) for v in self.feature_domain]
        if key not in self._cached:   # another acquisition on the same data: one more pass through the kernels
            acq, best = self._score_acq(kind, **kw)
            self._cached[key] = (None if acq is None else acq.reshape(fd), best)
        acq, (best_val, best_idx, nan_count) = self._cached[key][:2]
        self.acq_func_eval = acq
        if nan_count > 0 or best_idx >= int(np.prod(fd)) or (self._NEGATIVE_INDEX_IS_NAN and best_idx < 0):
            # the reference: amax is NaN, the comparison is empty, [0] raises (point_selector.py:207)
            raise IndexError(NAN_ACQUISITION)
        return np.array(np.unravel_index(best_idx, fd), dtype=np.int64)

    def lower_confidence_bound(self, explore=4):
        """point_selector.py:197-207: acq = explore*sigma - mu; first row-major arg-max as a multi-index."""
        self._need_update()
        return self._finish(("lcb", float(explore), 0.0), "lcb", explore=float(explore))

    def q_expected_improvement(self, n_samples=512, seed=7, xi=0.0):
        """Not in the reference: q = 8 Monte-Carlo Expected Improvement.  The candidates are grouped
        consecutively (row-major order of `predicted_pts`) into batches of 8; returns the (8, ndim) multi-indices
        of the first batch with the largest qEI, and leaves the per-batch values in `acq_func_eval` (1-D).
        Fixed base samples: default_rng(seed).standard_normal((n_samples, 8)).  Batches are sharded over the
        ranks like single candidates are."""
        self._not_in_marginal_mode("q_expected_improvement()")
        need_se(self._kernel, "q_expected_improvement()")
        self._need_update()
        fd = [int(v) for v in self.feature_domain]
        M = int(np.prod(fd))
        if M % 8:
            raise ValueError("q_expected_improvement needs a candidate count that is a multiple of 8")
        Z = np.random.default_rng(seed).standard_normal((int(n_samples), 8))
        f_best = float(np.min(np.asarray(self.measured_vals, dtype=np.float64)))
        Xs = np.asarray(self.predicted_pts, dtype=np.float64)
        world, rank = self._world()
        blo, bhi = D.shard_bounds(M // 8, world, rank)          # whole batches per rank, contiguous
        kw = self._model.acq_kw(dict(f_best=f_best, xi=float(xi)))
        res = self._gp.score_qei(Xs[blo * 8: bhi * 8], Z, kw["f_best"], xi=kw["xi"], dense=True, batch_offset=blo,
                                 prior_var=self._model.prior_var)
        best_val, best_idx, nan_count = D.allreduce_argmax(res.best_val, res.best_idx, res.nan_count)
        qei = self._model.acq_to_y("qei", D.gather_concat_tensors([res.acq], M // 8)[0].cpu().numpy())
        self.acq_func_eval = qei
        if nan_count > 0 or best_idx >= M // 8:
            raise IndexError(NAN_ACQUISITION)
        res.best_idx = best_idx
        flat = res.best_idx * 8 + np.arange(8)
        return np.stack(np.unravel_index(flat, fd), axis=1).astype(np.int64)

    def _batch_acq(self, acquisition, explore, xi):
        """Keyword arguments of the acquisition for a select_batch call (EI: f_best = min(measured_vals))."""
        if acquisition == "lcb":
            return dict(acquisition="lcb", explore=float(explore))
        if acquisition == "ei":
            return dict(acquisition="ei", f_best=float(np.min(np.asarray(self.measured_vals, dtype=np.float64))), xi=float(xi))
        raise ValueError(f"unknown acquisition {acquisition!r}")

    def _batch_indices(self, indices, nan_count):
        fd = [int(v) for v in self.feature_domain]
        if nan_count > 0 or np.any(indices < 0) or np.any(indices >= int(np.prod(fd))):
            raise IndexError(NAN_ACQUISITION)
        return np.stack(np.unravel_index(indices, fd), axis=1).astype(np.int64)

    def select_batch(self, q, acquisition="lcb", explore=4, xi=0.0, fantasy="believer", lie=None):
        """Not in the reference (one point per iteration): q points to evaluate in parallel, chosen greedily on the surrogate
        of the last update_surrogate().  The first is the acquisition's own arg-max; each further one is the arg-max after
        conditioning on a fantasy observation at the one before it - the current mean there (fantasy="believer": Kriging
        believer; under LCB this is GP-BUCB, only the variance shrinks) or the constant `lie` (fantasy="liar") - with the
        members chosen so far excluded (DeviceGP.select_batch).  acquisition: "lcb" (explore) or "ei"
        (f_best = min(measured_vals), xi).  Returns the (q, ndim) int64 multi-indices in selection order, the form
        q_expected_improvement() returns; IndexError when the acquisition contains NaN.  mean_func / cov_func /
        acq_func_eval stay as update_surrogate() set them (the selection works on copies of the device posterior).
        Needs precision="fp64", dense_outputs=True and candidates of another shape than the observations (the N == M
        quirk); candidates sharded over more than one rank are OUT OF SCOPE: NotImplementedError."""
        self._not_in_marginal_mode("select_batch()")
        need_se(self._kernel, "select_batch()")
        self._need_update()
        if self._precision != "fp64":
            raise ValueError("select_batch() needs precision='fp64' (a screened sigma cannot seed the updates)")
        if not self._dense:
            raise ValueError("select_batch() needs dense_outputs=True (it starts from the dense posterior)")
        if np.shape(self.predicted_pts) == np.shape(self.measured_pts):
            raise ValueError("select_batch() does not support candidates of the observations' shape (the N == M quirk)")
        if self._world()[0] > 1:
            raise NotImplementedError("select_batch() with candidates sharded over several ranks is not implemented")
        model = self._model
        # the candidates update_surrogate() left on the device: no second upload of M x d values
        r = self._gp.select_batch_on_posterior(self._cand[0], self._mu_dev.clone(), self._sigma_dev.clone(), int(q),
                                               fantasy=fantasy, lie=model.lie_to_model(lie), prior_var=model.prior_var,
                                               **model.acq_kw(self._batch_acq(acquisition, explore, xi)))
        return self._batch_indices(r.indices, r.nan_count)

    def select_thompson(self, q, n_features=2048, seed=0):
        """Not in the reference (one point per iteration): up to q points to evaluate in parallel by Thompson sampling on the
        surrogate of the last update_surrogate() - the minimisers of min(64, 2 q) independent sample paths of the posterior
        (pathwise conditioning on n_features random Fourier features, DeviceGP.select_thompson), the first q
        DISTINCT ones in path order.  Returns their (k, ndim) int64 multi-indices, k <= q: FEWER than q when the paths agree,
        which is the posterior saying it has converged there - top the batch up with select_batch().  One seed gives the
        same points here and in PointSelectorHost.  No variance pass is run, so every precision= and dense_outputs=False
        work; mean_func / cov_func / acq_func_eval stay as update_surrogate() set them.  IndexError when a candidate has a
        non-finite coordinate; candidates sharded over more than one rank are OUT OF SCOPE: NotImplementedError."""
        from .thompson import select_params

        self._not_in_marginal_mode("select_thompson()")
        need_se(self._kernel, "select_thompson()")
        self._need_update()
        Xs = np.asarray(self.predicted_pts, dtype=np.float64)
        Xs = Xs.reshape(len(Xs), -1)
        select_params(q, None, n_features, seed, M=len(Xs), d=Xs.shape[1])   # (refused before any GPU work)
        if self._world()[0] > 1:
            raise NotImplementedError("select_thompson() with candidates sharded over several ranks is not implemented")
        # the candidates update_surrogate() left on the device: no second upload of M x d values
        r = self._gp.select_thompson(self._cand[0], q, n_features=n_features, seed=seed)
        return self._batch_indices(r.indices, r.nan_count)

    def _refine_inputs(self, n_starts, iters, acquisition, explore, xi):
        """(acquisition keywords, starts [n x d], lower, upper) of a refine_next call: the n_starts candidates with the
        largest value of the class's own dense acquisition (stable order: ties keep the lower flat index first) and the
        bounding box of predicted_pts.  acq_func_eval and last_screen are left as they were.  Under a screened precision
        the ranking is the one the class's own acquisition methods use there: fp64 values on the screen's survivors (the
        top of the order), the screen's values below them; the refinement itself is always fp64."""
        from .gp_device import refine_params

        self._need_update()
        if not self._dense:
            raise ValueError("refine_next() needs dense_outputs=True (its starts come from the dense acquisition)")
        kw = self._batch_acq(acquisition, explore, xi)
        Xs = np.asarray(self.predicted_pts, dtype=np.float64)
        Xs = Xs.reshape(len(Xs), -1)
        n_starts = int(n_starts)
        if not 1 <= n_starts <= len(Xs):
            raise ValueError(f"n_starts must be in [1, M = {len(Xs)}], got {n_starts}")
        refine_params(n_starts, Xs.shape[1], iters, 0.1)
        key = ("lcb", kw["explore"], 0.0) if acquisition == "lcb" else ("ei", kw["f_best"], kw["xi"])
        keep = self.acq_func_eval, self.last_screen   # what _finish sets (last_screen: an uncached key under a screen)
        try:
            self._finish(key, acquisition, **{k: v for k, v in kw.items() if k != "acquisition"})   # IndexError on NaN
        finally:
            self.acq_func_eval, self.last_screen = keep
        acq = np.asarray(self._cached[key][0], dtype=np.float64).reshape(-1)
        order = np.argsort(-acq, kind="stable")[:n_starts]
        return kw, np.ascontiguousarray(Xs[order]), Xs.min(axis=0), Xs.max(axis=0)

    def refine_next(self, n_starts=64, iters=30, acquisition="lcb", explore=4, xi=0.0):
        """Not in the reference (whose lower_confidence_bound() answers with a grid index): the next point OFF the grid, as
        a float64 array of d coordinates.  The n_starts best candidates of the dense acquisition are refined by projected
        gradient ascent inside the bounding box of predicted_pts (DeviceGP.refine) and the best refined point
        is returned; call after update_surrogate().  acquisition: "lcb" (explore) or "ei" (f_best = min(measured_vals),
        xi).  mean_func / cov_func / acq_func_eval and every other attribute stay as they are; IndexError when the
        acquisition contains NaN.  With sharded candidates every rank refines the same global starts on the replicated
        factorisation (same bits on every rank, no collective)."""
        self._not_in_marginal_mode("refine_next()")
        need_se(self._kernel, "refine_next()")
        kw, starts, lo, hi = self._refine_inputs(n_starts, iters, acquisition, explore, xi)
        r = self._gp.refine(starts, lo, hi, iters=int(iters), prior_var=self._model.prior_var, **self._model.acq_kw(kw))
        if r.nan_count > 0 or r.best < 0:
            raise IndexError(NAN_ACQUISITION)
        return r.x[r.best].cpu().numpy().astype(np.float64)

    def loo(self):
        """Not in the reference: leave-one-out prediction of every observation from the surrogate of the last
        update_surrogate() - (mean [N], standard deviation [N], standardised residual [N]) as host arrays in the order of
        measured_pts, in the units of measured_vals.  Nothing is refitted: the diagonal of K^-1 comes from the factor
        (DeviceGP.loo).  The standard deviation is that of a NOISY observation at the left-out point (the model's K holds the
        noise), which is what the left-out value is compared with.  With ard="hyper" the residuals of a well-specified model are
        unit normal; the frozen model of the other modes is only calibrated for data that are already standardised."""
        self._need_update()
        mu, var, _ = self._gp.loo(1.0)
        mean = self._model.y_mean + self._model.y_scale * mu.cpu().numpy()   # (computed for every model, as it always was)
        sd = self._model.y_scale * np.sqrt(var.cpu().numpy())
        return mean, sd, (np.asarray(self.measured_vals, dtype=np.float64).reshape(-1) - mean) / sd

    def expected_improvement(self, xi=0.0):
        """Not in the reference (docs/README.md:363-365 'future work'): EI for minimisation,
        f_best = min(measured_vals)."""
        self._need_update()
        f_best = float(np.min(np.asarray(self.measured_vals, dtype=np.float64)))
        return self._finish(("ei", f_best, float(xi)), "ei", f_best=f_best, xi=float(xi))

    def _nei_scores(self, S, seed, xi, delta):
        """(NEI over all candidates [M], (best value, flat index, NaN count), the fantasies' incumbents [S]) in the units of the
        MODEL: what each class provides to noisy_expected_improvement()."""
        lo = self._lo_hi[0]
        r = self._gp.select_nei(self._cand[0], S, seed, xi=xi, delta=delta, dense=True, idx_offset=lo, check=False)
        best = D.allreduce_argmax(r.best_val, r.best_idx, r.nan_count)
        M = int(np.prod([int(v) for v in self.feature_domain]))
        return D.gather_concat_tensors([r.acq], M)[0].cpu().numpy(), best, r.fantasy_best.cpu().numpy()

    def noisy_expected_improvement(self, n_fantasies=16, seed=0, xi=0.0, delta=1e-6):
        """Not in the reference: noisy expected improvement (Letham, Karrer, Ottoni & Bakshy 2019) for minimisation.  The
        observations are noisy, so min(measured_vals) - the incumbent of expected_improvement() - is the luckiest noise draw and
        not the best function value.  Here n_fantasies samples of the latent function at the observed points are drawn from the
        posterior (DeviceGP.fantasies, DESIGN 4j: latent covariance k + delta, noise rho - delta with rho the model's diagonal
        term; delta in the units of the model, where the signal variance is 1), a noise-free model is conditioned on each, and
        the expected improvements - each against its own sample's minimum - are averaged.  Returns the multi-index as
        expected_improvement() does; acq_func_eval holds the values and fantasy_best [n_fantasies] the incumbents, both in the
        units of measured_vals.  One seed gives the same fantasies on every rank of a sharded call and in PointSelectorHost.
        Every model record and kernel= work; candidates of the observations' shape are scored without the N == M quirk.
        ard="marginal", a screened precision= and dense_outputs=False raise ValueError; IndexError when the acquisition
        contains NaN."""
        from .nei import nei_params

        self._not_in_marginal_mode("noisy_expected_improvement()")
        if self._precision != "fp64":
            raise ValueError(f"noisy_expected_improvement() needs precision='fp64', got precision={self._precision!r} (the "
                             "fantasies are conditioned on the fp64 posterior)")
        if not self._dense:
            raise ValueError("noisy_expected_improvement() needs dense_outputs=True (dense_outputs=False factorises the "
                             "observations in another order than the draws)")
        S, seed, xi, delta = nei_params(n_fantasies, seed, xi, delta)
        self._need_update()
        model = self._model
        nei_params(S, seed, xi, delta, rho=model.jitter1 + model.jitter2)
        key = ("nei", S, seed, xi, delta)
        if key not in self._cached:
            acq, best, fbest = self._nei_scores(S, seed, model.acq_kw(dict(xi=xi))["xi"], delta)
            fd = [int(v) for v in self.feature_domain]
            self._cached[key] = (model.acq_to_y("ei", acq).reshape(fd), model.best_to_y("ei", best), model.mean_to_y(fbest))
        self.fantasy_best = self._cached[key][2]
        return self._finish(key, "nei")

    def _mes_scores(self, S, seed, y_star, cap):
        """(MES over all candidates [M], (best value, flat index, NaN count), the sampled minima [S] in the units of the MODEL):
        what each class provides to max_value_entropy_search().  Sharded candidates: the brackets' minima are an exact MIN
        all-reduce and every round's partial log S is added in rank order, so every rank fits the same Gumbel law and draws the
        same samples (distributed.sum_in_rank_order; with one rank the identity)."""
        gp, mu, sigma, lo = self._gp, self._mu_dev, self._sigma_dev, self._lo_hi[0]
        if isinstance(y_star, str) and y_star == "thompson" and self._world()[0] > 1:
            raise NotImplementedError("max_value_entropy_search(y_star='thompson') with candidates sharded over several ranks is "
                                      "not implemented")
        m, _ = gp.mes_minima(mu, sigma, self._cand[0], S, seed, y_star, cap,
                             log_survival=lambda z: D.sum_in_rank_order(*gp.log_survival(mu, sigma, z)),
                             reduce_min=D.allreduce_min)
        r = gp.mes_on_posterior(mu, sigma, m, idx_offset=lo, dense=True)
        best = D.allreduce_argmax(r.best_val, r.best_idx, r.nan_count)
        M = int(np.prod([int(v) for v in self.feature_domain]))
        return D.gather_concat_tensors([r.acq], M)[0].cpu().numpy(), best, m

    def max_value_entropy_search(self, n_samples=16, seed=0, y_star="gumbel", cap="observed"):
        """Not in the reference: max-value entropy search (Wang & Jegelka 2017) for minimisation - the expected reduction of the
        entropy of the minimum's VALUE m* over the candidates, MES(x) = mean_s h((mu(x) - m*_s) / sigma(x)) with
        h(g) = g phi(g) / (2 Phi(g)) - log Phi(g).  No trade-off parameter and no incumbent, invariant under an affine map of
        measured_vals, and a function of the posterior update_surrogate() has left on the device: no variance pass, every
        kernel= and every model record.  y_star: how the n_samples minima are sampled - "gumbel" (a Gumbel law fitted to three
        quartiles of Pr[m* > z] under an independence approximation), "thompson" (the minima of n_samples posterior
        sample paths with this seed: kernel='se', one rank) or n_samples values in the units of measured_vals.  cap: "observed"
        (no Gumbel sample above min(measured_vals): the paper's rule), a number in the units of measured_vals, or None.
        Returns the multi-index as expected_improvement() does; acq_func_eval holds the values (unit-free) and sampled_minima
        [n_samples] the samples in the units of measured_vals.  One seed gives the same samples on every rank of a sharded call
        and in PointSelectorHost.  ard="marginal", a screened precision= and dense_outputs=False raise ValueError; IndexError
        when the acquisition contains NaN."""
        from .mes import mes_params, mes_y_star

        self._not_in_marginal_mode("max_value_entropy_search()")
        if self._precision != "fp64":
            raise ValueError(f"max_value_entropy_search() needs precision='fp64', got precision={self._precision!r} (the stored "
                             "sigma of a screened precision is the screen's)")
        if not self._dense:
            raise ValueError("max_value_entropy_search() needs dense_outputs=True (it works on the dense posterior)")
        S, seed, cap = mes_params(n_samples, seed, cap)
        y_star = mes_y_star(y_star, S)
        if isinstance(y_star, str) and y_star == "thompson":
            need_se(self._kernel, "max_value_entropy_search(y_star='thompson')")
        self._need_update()
        model = self._model
        key = ("mes", S, seed, y_star if isinstance(y_star, str) else tuple(y_star.tolist()), cap)
        if key not in self._cached:
            # everything below in the units of the model (MES itself has no unit)
            if isinstance(cap, str):
                cap_m = float(np.min(model.to_model(np.asarray(self.measured_vals, dtype=np.float64))))
            else:
                cap_m = None if cap is None else float(model.to_model(cap))
            ys = y_star if isinstance(y_star, str) else np.ascontiguousarray(model.to_model(y_star))
            acq, best, minima = self._mes_scores(S, seed, ys, cap_m)
            fd = [int(v) for v in self.feature_domain]
            self._cached[key] = (model.acq_to_y("mes", acq).reshape(fd), best, model.mean_to_y(minima))
        self.sampled_minima = self._cached[key][2]
        return self._finish(key, "mes")

    # -- constrained acquisitions in log space (csrc/constrained.hip) ------------------------------------------
    def _cons_refusals(self, what: str):
        self._not_in_marginal_mode(what)
        if self._precision != "fp64":
            raise ValueError(f"{what} needs precision='fp64', got precision={self._precision!r} (the stored sigma of a screened "
                             "precision is the screen's)")
        if not self._dense:
            raise ValueError(f"{what} needs dense_outputs=True (it works on the dense posterior)")

    def _cons_posterior(self) -> tuple:
        """(mu, sigma) of the last update_surrogate() over this rank's candidates in the units of the MODEL, in the form this
        class's _cons_scores takes them (here: the device tensors the pass left)."""
        return self._mu_dev, self._sigma_dev

    def _cons_scores(self, base, f_best, xi, posteriors, upper):
        """(value over all candidates [M], log-feasibility [M], (best value, flat index, NaN count)), everything in the units of
        the MODELS: what each class provides to _constrained().  posteriors: _cons_posterior() of every constraint."""
        gp, lo = self._gp, self._lo_hi[0]
        mu, sigma = self._cons_posterior()
        cm = gp.torch.stack([p[0] for p in posteriors]) if posteriors else None
        cs = gp.torch.stack([p[1] for p in posteriors]) if posteriors else None
        r = gp.constrained_on_posterior(mu, sigma, cm, cs, upper, base=base, f_best=f_best, xi=xi, idx_offset=lo, dense=True)
        best = D.allreduce_argmax(r.best_val, r.best_idx, r.nan_count)
        M = int(np.prod([int(v) for v in self.feature_domain]))
        val, feas = (t.cpu().numpy() for t in D.gather_concat_tensors([r.value, r.log_feasibility], M))
        return val, feas, best

    def _constrained(self, what, base, constraints, upper, xi, f_best):
        """The three constrained calls.  base: "ei", "pi" or "none"; f_best: "feasible" or a number in the units of
        measured_vals.  Refusals first, then "call update_surrogate() first", then the library."""
        from .constrained import _finite_number, cons_limits, cons_params, feasible_incumbent, incumbent_rule

        self._cons_refusals(what)
        constraints = list(constraints)
        for c in constraints:
            if type(c) is not type(self):
                raise ValueError(f"{what}: every constraint must be a {type(self).__name__} (holding that quantity's observations "
                                 f"as its measured_vals), got {type(c).__name__}")
            c._cons_refusals(what + " (a constraint)")
        u = cons_limits(upper, len(constraints))
        xi = _finite_number("xi", xi)
        if base != "none":
            f_best = incumbent_rule(f_best)
        cons_params(base, 0.0, xi, len(constraints))
        self._need_update()
        fd = [int(v) for v in self.feature_domain]
        Xs = np.ascontiguousarray(self.predicted_pts, dtype=np.float64)
        for k, c in enumerate(constraints):
            c._need_update()
            if ([int(v) for v in c.feature_domain] != fd or getattr(c, "_lo_hi", None) != getattr(self, "_lo_hi", None)
                    or np.ascontiguousarray(c.predicted_pts, dtype=np.float64).tobytes() != Xs.tobytes()):
                raise ValueError(f"{what}: constraint {k} was not updated on the same predicted_pts (feature_domain, the shard "
                                 "and every coordinate, bit for bit)")
        model = self._model
        if base == "none":
            f_best = None
        elif isinstance(f_best, str):   # "feasible"; with no constraint: min(measured_vals)
            f_best = feasible_incumbent(self.measured_pts, self.measured_vals, [c.measured_pts for c in constraints],
                                        [c.measured_vals for c in constraints], u)
            if f_best is None:
                base = "none"   # no feasible observation yet: maximise the probability of feasibility (Gelbart's rule)
        # everything below in the units of the models: each limit in its own constraint's, f_best and xi in the objective's
        u_m = np.array([float(c._model.to_model(u[k])) for k, c in enumerate(constraints)], dtype=np.float64)
        kw = model.acq_kw(dict(f_best=f_best, xi=xi))
        val, feas, best = self._cons_scores(base, kw["f_best"], kw["xi"], [c._cons_posterior() for c in constraints], u_m)
        kind = {"ei": "log_cei", "pi": "log_pi", "none": "log_pof"}[base]
        key = ("constrained",)   # never reused: the constraints' posteriors are not part of this object's cache
        self._cached[key] = (model.acq_to_y(kind, val).reshape(fd), model.best_to_y(kind, best))
        self.log_feasibility = feas.reshape(fd)
        self.constrained_base, self.constrained_incumbent = base, f_best
        return self._finish(key, kind)

    def probability_of_improvement(self, xi=0.0, f_best=None):
        """Not in the reference (whose docs name it as a wish): probability of improvement for minimisation,
        Phi(((f_best - mu) - xi) / sigma), evaluated as its LOGARITHM (it does not underflow: log Phi(-40) = -804.6, where Phi
        itself is 0 in fp64 and every candidate would tie).  f_best: a number in the units of measured_vals, default
        min(measured_vals).  Returns the multi-index as expected_improvement() does; acq_func_eval holds log PI (unit-free).  A
        function of the posterior update_surrogate() has left on the device: every kernel= and every model record.
        ard="marginal", a screened precision= and dense_outputs=False raise ValueError; IndexError when a value is NaN."""
        from .constrained import _finite_number

        self._cons_refusals("probability_of_improvement()")
        # (no constraint: the feasible incumbent of _constrained IS min(measured_vals))
        f_best = "feasible" if f_best is None else _finite_number("f_best", f_best)
        return self._constrained("probability_of_improvement()", "pi", [], [], xi, f_best)

    def constrained_expected_improvement(self, constraints, upper, xi=0.0, f_best="feasible"):
        """Not in the reference: constrained expected improvement (Gardner et al. 2014; Gelbart, Snoek & Adams 2014) for
        minimisation under black-box constraints g_c(x) <= upper[c] - EI times the probability that every constraint holds,
        evaluated as log EI + sum_c log Phi((upper_c - mu_c) / sigma_c): the plain product is exactly 0 a few dozen standard
        deviations inside the infeasible region, where every candidate would tie.  constraints: selector objects of this
        class, one per constraint, each holding that quantity's observations as its measured_vals - with a kernel=, ard= and
        model of its own - whose update_surrogate() has run on the same predicted_pts.  upper: one limit per constraint, in
        the units of that selector's measured_vals (a two-sided band: two constraints, g <= u and -g <= -l).  f_best:
        "feasible" (the smallest of measured_vals among the observations at which every constraint's observation is within
        its limit: all selectors must hold the same measured_pts; if no observation is feasible the call maximises the
        probability of feasibility alone and constrained_base says "none") or a number in the units of measured_vals.
        Returns the multi-index as expected_improvement() does; acq_func_eval holds the LOG values (log of the units of
        measured_vals; -inf is a legal value), log_feasibility the dense log-probability of feasibility, constrained_base the
        base that was used and constrained_incumbent f_best.  ard="marginal", a screened precision= and dense_outputs=False
        raise ValueError, for this object and for every constraint; IndexError when a value is NaN."""
        return self._constrained("constrained_expected_improvement()", "ei", constraints, upper, xi, f_best)

    def probability_of_feasibility(self, constraints, upper):
        """Not in the reference: the point at which all constraints are most likely to hold, by
        sum_c log Phi((upper_c - mu_c) / sigma_c) (acq_func_eval and log_feasibility; unit-free).  constraints, upper and the
        refusals: as constrained_expected_improvement().  This object's own posterior is not read."""
        return self._constrained("probability_of_feasibility()", "none", constraints, upper, 0.0, None)

    # -- two-objective expected hypervolume improvement in log space (csrc/ehvi.hip) ---------------------------
    def _ehvi_scores(self, posterior2, front, ref):
        """(log EHVI over all candidates [M], (best value, flat index, NaN count)), everything in the units of the MODELS: what
        each class provides to expected_hypervolume_improvement().  posterior2: _cons_posterior() of the second objective."""
        gp, lo = self._gp, self._lo_hi[0]
        mu1, sigma1 = self._cons_posterior()
        r = gp.ehvi_on_posterior(mu1, sigma1, posterior2[0], posterior2[1], front, ref, idx_offset=lo, dense=True)
        best = D.allreduce_argmax(r.best_val, r.best_idx, r.nan_count)
        M = int(np.prod([int(v) for v in self.feature_domain]))
        (val,) = (t.cpu().numpy() for t in D.gather_concat_tensors([r.value], M))
        return val, best

    def expected_hypervolume_improvement(self, other, ref="nadir", front="observed"):
        """Not in the reference: expected hypervolume improvement (Emmerich et al. 2006, 2016) for TWO minimised objectives - the
        expected growth of the area below the reference point that the Pareto front dominates - evaluated as its LOGARITHM: the
        plain value is exactly 0 wherever both objectives are a few dozen standard deviations from improving, where every
        candidate would tie.  This object holds objective 1's observations as its measured_vals; other: a selector object of
        this class holding objective 2's - with a kernel=, ard= and model of its own - whose update_surrogate() has run on the
        same predicted_pts.  The objectives are taken as independent.  ref: two numbers in the units of the two measured_vals,
        or "nadir": per objective the worst observation plus 10 % of the observed range (ValueError when a range is zero: pass
        numbers).  front: "observed" (the Pareto front of the observed pairs below ref: both selectors must hold the same
        measured_pts, bit for bit) or a [P x 2] array in the form pareto.pareto_front() returns, at most 128 points.
        Returns the multi-index as expected_improvement() does; acq_func_eval holds log EHVI (log of the product of the two
        units; -inf is a legal value), pareto_front, reference_point and hypervolume what was used, in the units of y.
        ard="marginal", a screened precision= and dense_outputs=False raise ValueError, for this object and for other;
        IndexError when a value is NaN.  To add black-box constraints, add log_feasibility of a constrained call to
        acq_func_eval."""
        from .pareto import check_front, hypervolume, observed_pairs, pareto_front, reference_point

        what = "expected_hypervolume_improvement()"
        self._cons_refusals(what)
        if type(other) is not type(self):
            raise ValueError(f"{what}: the second objective must be a {type(self).__name__} (holding its observations as its "
                             f"measured_vals), got {type(other).__name__}")
        other._cons_refusals(what + " (the second objective)")
        nadir = isinstance(ref, str) and ref == "nadir"
        if not nadir:
            ref = reference_point(None, ref)
        observed = isinstance(front, str)
        if observed and front != "observed":
            raise ValueError(f"front must be 'observed' or a [P x 2] array, got {front!r}")
        if not observed and not nadir:
            check_front(front, ref)
        self._need_update()
        other._need_update()
        fd = [int(v) for v in self.feature_domain]
        Xs = np.ascontiguousarray(self.predicted_pts, dtype=np.float64)
        if ([int(v) for v in other.feature_domain] != fd or getattr(other, "_lo_hi", None) != getattr(self, "_lo_hi", None)
                or np.ascontiguousarray(other.predicted_pts, dtype=np.float64).tobytes() != Xs.tobytes()):
            raise ValueError(f"{what}: the second objective was not updated on the same predicted_pts (feature_domain, the shard "
                             "and every coordinate, bit for bit)")
        if observed or nadir:
            Y = observed_pairs(self.measured_pts, self.measured_vals, other.measured_pts, other.measured_vals)
            ref = reference_point(Y, ref)
        F, r = check_front(pareto_front(Y, ref) if observed else front, ref)
        # everything below in the units of the models: each coordinate in its own objective's
        m1, m2 = self._model, other._model
        F_m = np.stack([np.asarray(m1.to_model(F[:, 0]), dtype=np.float64), np.asarray(m2.to_model(F[:, 1]), dtype=np.float64)],
                       axis=1)
        r_m = (float(m1.to_model(r[0])), float(m2.to_model(r[1])))
        val, best = self._ehvi_scores(other._cons_posterior(), F_m, r_m)

        def to_y(v):   # log of an area: + log y_scale of each objective
            return m2.acq_to_y("log_ehvi", m1.acq_to_y("log_ehvi", v))

        key = ("ehvi",)   # never reused: the second objective's posterior is not part of this object's cache
        self._cached[key] = (to_y(val).reshape(fd), (float(to_y(best[0])),) + tuple(best[1:]))
        self.pareto_front, self.reference_point, self.hypervolume = F, r, hypervolume(F, r)
        return self._finish(key, "log_ehvi")
