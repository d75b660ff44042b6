"""An ensemble of surrogates on one GPU: the acquisition integrated over samples of the hyperparameter posterior.

Not in the reference, which scores under one frozen model (point_selector.py:63-101).  S models share the observations and the
covariance family and differ in (length scales, noise ratio, mean, scale); `DeviceEnsemble.factorise` factorises each with the
kernels every other route uses (gpbo_factorise_kern_f64) into stacked buffers, `DeviceEnsemble.score` is one call of
gpbo_ensemble_acq_f64 (csrc/ensemble.hip): per model the fp64 posterior pass, then one fold kernel, in index order - the
weighted mean of the models' acquisitions, and the mean and standard deviation of the mixture of their predictive
distributions, everything in the units of y.  PyTorch is plumbing only, as in gp_device.py; there is no CPU path.
"""
from __future__ import annotations

from dataclasses import dataclass
from typing import Optional

import numpy as np

from . import _lib
from .gp_device import DEFAULT_CHUNK, DeviceSide, acq_params

ENSEMBLE_MAX_BYTES = 8 << 30   # cap on the stacked inverse factors, S * Np^2 * 8 bytes (S = 16 at N = 8192)


@dataclass
class EnsembleResult:
    best_val: float                  # the largest integrated acquisition, in the units of y
    best_idx: int                    # idx_offset + the LOWEST row of Xs attaining it
    nan_count: int                   # candidates whose integrated acquisition is NaN (not part of the arg-max)
    mean: Optional[object] = None    # dense=True: torch fp64 device tensors [M]: mean of the mixture,
    sd: Optional[object] = None      # its standard deviation,
    acq: Optional[object] = None     # the integrated acquisition


class DeviceEnsemble(DeviceSide):
    def __init__(self, device=None, chunk: int = DEFAULT_CHUNK):
        super().__init__(device, chunk)
        self.S = 0
        self.X = self.U = self.alpha = self.info = None
        self.ls_h = self.model_h = None      # host [S x d], [S x 4] = (weight, prior variance, y_mean, y_scale)
        self._K = self._work_fact = self._work = None
        self._result = self.torch.zeros(4, dtype=self.torch.int64, device=self.device)
        self._keep = None

    def factorise(self, X, y, models):
        """models: a list of (length scales [d], model.SurrogateModel, weight >= 0), 1 <= S <= 64, one covariance family.
        Model s is factorised as gpbo_factorise_kern_f64 does for (model.to_model(y), ls, model.jitter1, model.jitter2).
        numpy.linalg.LinAlgError naming the first model whose matrix is not positive definite; ValueError when the stacked
        inverse factors would exceed ENSEMBLE_MAX_BYTES or d > 16."""
        torch = self.torch
        S = len(models)
        if not 1 <= S <= _lib.ENSEMBLE_MAX_S:
            raise ValueError(f"an ensemble holds 1 to {_lib.ENSEMBLE_MAX_S} models, got {S}")
        limit = (_lib.MAX_D, f"an ensemble needs d <= {_lib.MAX_D}, got d = {{d}}")
        Xd, y_h, N, d, _ = self._problem(X, y, None, [limit], host_y=True)   # (the [S x d] length scales: checked below)
        kernels = {m.kernel for _, m, _ in models}
        if len(kernels) != 1:
            raise ValueError(f"the models of an ensemble share one covariance family, got {sorted(kernels)}")
        kernel = kernels.pop()
        kid = _lib.kernel_id(kernel)
        ls_h = np.ascontiguousarray(np.stack([np.asarray(ls, dtype=np.float64).reshape(-1) for ls, _, _ in models]))
        if ls_h.shape != (S, d) or not np.all(ls_h > 0.0):
            raise ValueError(f"every model needs {d} positive length scales")
        model_h = np.ascontiguousarray(np.array([[float(w), m.prior_var, m.y_mean, m.y_scale] for _, m, w in models]))
        if not (np.all(np.isfinite(model_h)) and np.all(model_h[:, 0] >= 0.0) and model_h[:, 0].sum() > 0.0
                and np.all(model_h[:, 3] > 0.0)):
            raise ValueError("weights must be finite and >= 0 with a positive sum, scales positive")
        Np = int(self.lib.gpbo_padded_n(N))
        if S * Np * Np * 8 > ENSEMBLE_MAX_BYTES:
            raise ValueError(f"{S} models at N = {N}: the stacked inverse factors need {S * Np * Np * 8} bytes, more than "
                             f"ENSEMBLE_MAX_BYTES = {ENSEMBLE_MAX_BYTES}")
        with torch.cuda.device(self.device):
            f64 = dict(dtype=torch.float64, device=self.device)
            if self.U is None or tuple(self.U.shape) != (S, Np, Np):
                self.U = self._K = None
                self.U = torch.empty((S, Np, Np), **f64)
                self.alpha = torch.empty((S, Np), **f64)
                self._K = torch.empty((Np, Np), **f64)
            self.info = torch.zeros(S, dtype=torch.int32, device=self.device)
            wf = int(self.lib.gpbo_factorise_workspace_bytes(Np))
            work = self._workspace("_work_fact", wf)
            ys = self._dev(np.stack([m.to_model(y_h) for _, m, _ in models]))   # [S x N], each in its model's units
            for s, (_, m, _) in enumerate(models):
                self._factorise_into(Xd, ys[s], N, d, ls_h[s], kid, float(m.jitter1), float(m.jitter2), Np, self._K,
                                     self.U[s], self.alpha[s], self.info[s:s + 1], work, wf)
            info = self.info.cpu().numpy()   # synchronises
        self.X, self.S, self.N, self.Np, self.d, self.kernel = Xd, S, N, Np, d, kernel
        self.ls_h, self.model_h = ls_h, model_h
        if np.any(info != 0):
            s = int(np.flatnonzero(info)[0])
            self.S = 0
            raise np.linalg.LinAlgError(f"model {s} of the ensemble: covariance matrix is not positive definite "
                                        f"(pivot {int(info[s])} of {N})")
        return self

    def score(self, Xs, acquisition: str = "lcb", explore: float = 4.0, f_best: Optional[float] = None, xi: float = 0.0,
              dense: bool = False, idx_offset: int = 0) -> EnsembleResult:
        """The integrated acquisition over the rows of Xs and its first arg-max; explore / f_best / xi in the units of y.
        dense=True also returns the mixture's mean and standard deviation and the acquisition as device tensors [M]."""
        torch = self.torch
        if self.S < 1:
            raise _lib.GpboError("score() needs a factorised ensemble")
        Xsd, M = self._candidates(Xs)
        kind, p0, p1 = acq_params(acquisition, explore, f_best, xi)
        chunk = self._chunk_for(M)
        with torch.cuda.device(self.device):
            need = int(self.lib.gpbo_ensemble_workspace_bytes(self.Np, chunk, M))
            work = self._workspace("_work", need, free_first=True)
            mean, sd, acq = self._dense(M, dense)
            _lib.call(self.lib.gpbo_ensemble_acq_f64, Xsd, M, self.X, self.N, self.Np, self.d, self.S, self.ls_h, self._kid(),
                      self.U, self.alpha, self.model_h, kind, p0, p1, int(idx_offset), chunk, mean, sd, acq, self._result,
                      work, need, self._stream())
            v, i, n = self.read_result(self._result)   # synchronises
        return EnsembleResult(v, i, n, mean, sd, acq)
