"""The surrogate model as one record, and the length-scale search space as one description (NumPy only).

`SurrogateModel` is what the selector classes know about the GP besides its length scales: the covariance family, the two
diagonal terms and the affine map between the units of y and those the kernels work in.  The reference's frozen model is
SurrogateModel("se") - 1e-4 + 1e-6 on the diagonal, zero mean, unit scale; ard="hyper" fits SurrogateModel(kernel, rho, 0.0,
m, s, fitted=True): the GP of (y - m) / s with K = k(X,X) + rho I.  A model that is not fitted maps nothing:
every map returns its argument ITSELF, so no -0.0 becomes +0.0 on the way.
`LengthScaleSpace` is what `length_scales` / set_length_scale_cells() span for d features (point_selector.py:60-73, 104-163).
"""
from __future__ import annotations

from dataclasses import dataclass

import numpy as np

JITTER_KERNEL = 1e-4    # point_selector.py:193
JITTER_ASSEMBLY = 1e-6  # point_selector.py:78-79


def need_se(kernel: str, what: str):
    """The calls that build covariance entries with squared-exponential kernels of their own refuse a surrogate of another
    family (each is a follow-up of its own: DESIGN.md 4g)."""
    if kernel != "se":
        raise ValueError(f"{what} is not available with kernel={kernel!r}: it supports kernel='se' only")


@dataclass(frozen=True)
class SurrogateModel:
    kernel: str = "se"
    jitter1: float = JITTER_KERNEL     # on the diagonal of k(X,X) (fitted: the noise-to-signal ratio rho)
    jitter2: float = JITTER_ASSEMBLY   # added when the covariance blocks are assembled (fitted: 0)
    y_mean: float = 0.0                # m, in the units of y
    y_scale: float = 1.0               # s, in the units of y
    fitted: bool = False

    @property
    def prior_var(self) -> float:
        """Diagonal of cov_pred: the variance of an OBSERVATION at a point nothing is known about, as the reference rounds
        it ((1 + 1e-4) + 1e-6; fitted: 1 + rho)."""
        return (1.0 + self.jitter1) + self.jitter2

    def diag_add(self, xs_shape, x_shape) -> float:
        """point_selector.py:173: kernel_rbf adds 1e-4 to the diagonal of k(X*, X) when the two shapes coincide - a quirk of
        the reference's squared exponential, not of a fitted model or a Matern kernel."""
        return JITTER_KERNEL if tuple(xs_shape) == tuple(x_shape) and not self.fitted and self.kernel == "se" else 0.0

    # -- the units of y -> the units of the model ----------------------------------------------------------------------
    def to_model(self, y):
        return (np.asarray(y, dtype=np.float64) - self.y_mean) / self.y_scale if self.fitted else y

    def acq_kw(self, kw: dict) -> dict:
        """Acquisition keywords given in the units of y, as the kernels take them: EI's f_best and xi are standardised."""
        if not self.fitted:
            return kw
        kw = dict(kw)
        if kw.get("f_best") is not None:
            kw["f_best"] = float(self.to_model(kw["f_best"]))
        if "xi" in kw:
            kw["xi"] = float(kw["xi"]) / self.y_scale
        return kw

    def lie_to_model(self, lie):
        """A fantasy observation is a value of y (None and the non-finite markers pass through)."""
        return float(self.to_model(lie)) if self.fitted and lie is not None and np.isfinite(float(lie)) else lie

    # -- the units of the model -> the units of y ----------------------------------------------------------------------
    def mean_to_y(self, mu):
        return self.y_mean + self.y_scale * mu if self.fitted else mu

    def sd_to_y(self, sigma):
        return self.y_scale * sigma if self.fitted else sigma

    def acq_to_y(self, kind: str, acq):
        """LCB = s acq - m (explore s sigma - (m + s mu)), EI / qEI = s acq.  Both maps increase, so the arg-max and its
        tie rule are those of the kernels.  "mes" (max-value entropy search) has no unit: an entropy of a ratio.  The
        constrained acquisitions are LOGARITHMS: "log_cei" = log EI_model + log s (a probability of feasibility has no unit),
        "log_pi" and "log_pof" are logarithms of probabilities and have none; "log_ehvi" is the logarithm of an AREA, the product
        of two objectives' units: each objective's model adds its own log s (the caller applies both)."""
        if not self.fitted or kind in ("mes", "log_pi", "log_pof"):
            return acq
        if kind in ("log_cei", "log_ehvi"):
            return acq + float(np.log(self.y_scale))
        return self.y_scale * acq - self.y_mean if kind == "lcb" else self.y_scale * acq

    def best_to_y(self, kind: str, best):
        """The (value, index, NaN count) record of an arg-max with its value in the units of y."""
        return (float(self.acq_to_y(kind, best[0])),) + tuple(best[1:]) if self.fitted else best


def _first_min(g) -> np.ndarray:
    """np.argwhere(g == np.amin(g))[0] (point_selector.py:141, 159): the first row-major minimum; IndexError on NaN."""
    return np.argwhere(g == np.amin(g))[0]


class LengthScaleSpace:
    """kind "cells": an explicit [G x d] list (any d); "sweep": one axis per feature, d > 2, searched one axis at a time;
    "grid2": two axes, the reference's full grid (:122-146; `len(length_scales) == 2` is read as two axes, as there);
    "grid1": `length_scales` is the one axis itself, and a tuned kernel_params has the shape (1, 1) of :161."""

    def __init__(self, length_scales, cells, d: int):
        self.d, self.cells, self.axes = int(d), cells, None
        if cells is not None:
            self.kind, self.shape = "cells", (self.d,)
        elif d > 2 or len(length_scales) == 2:
            self.axes = [np.asarray(a, dtype=np.float64).reshape(-1) for a in length_scales]
            self.kind, self.shape = "sweep" if d > 2 else "grid2", (len(self.axes),)
        else:
            self.axes = [np.asarray(length_scales, dtype=np.float64).reshape(-1)]
            self.kind, self.shape = "grid1", (1, 1)

    def _check(self):
        if self.cells is not None and self.cells.shape[1] != self.d:
            raise ValueError(f"length-scale cells have {self.cells.shape[1]} columns, the observations {self.d}")
        if self.cells is None and len(self.axes) != self.d:
            raise ValueError(f"length_scales must hold one axis per feature ({self.d}), got {len(self.axes)}")

    def middle(self) -> np.ndarray:
        """The reference's choice when it cannot tune (:63-73): the middle cell / the middle of every axis, as an fp64 vector."""
        if self.cells is not None:
            return np.array(self.cells[len(self.cells) // 2])
        return np.array([a[len(a) // 2] for a in self.axes])

    def box_and_start(self) -> tuple:
        """(lower, upper, start) of a likelihood fit: each feature's [min, max] of its axis (of its column of the cell
        list) and the middle."""
        self._check()
        cols = self.axes if self.cells is None else self.cells.T
        return np.array([a.min() for a in cols]), np.array([a.max() for a in cols]), self.middle()

    def fitted(self, ls) -> np.ndarray:
        """Fitted length scales in the shape the grid route gives kernel_params for this space."""
        return np.asarray(ls, dtype=np.float64).reshape(self.shape)

    def search(self, nlml, sweeps: int = 2) -> tuple:
        """(kernel_params, nlogml) of the grid search over nlml(cells [G x d]) -> [G], the first minimum winning: every cell
        of the list; `sweeps` passes over the axes from the middle of every axis (d > 2: the full grid has prod(G_k) cells;
        nlogml is then the last grid of each axis); or the reference's full 1-D / 2-D grid."""
        self._check()
        if self.kind == "cells":
            g = nlml(self.cells)
            return np.array(self.cells[_first_min(g)[0]]), g
        if self.kind == "sweep":
            ls, grids = self.middle(), [None] * self.d
            for _ in range(sweeps):
                for k, a in enumerate(self.axes):
                    cells = np.tile(ls, (len(a), 1))
                    cells[:, k] = a
                    grids[k] = nlml(cells)
                    ls[k] = a[_first_min(grids[k])[0]]
            return ls, grids
        cells = np.stack(np.meshgrid(*self.axes, indexing="ij"), -1).reshape(-1, self.d)
        g = nlml(cells).reshape([len(a) for a in self.axes])
        return np.array([a[i] for a, i in zip(self.axes, _first_min(g))]).reshape(self.shape), g
