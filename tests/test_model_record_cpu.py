"""The surrogate-model record (bayesian_optimisation_amd/model.py) on its own: no GPU, no library.  The prior variance as the
kernels and the oracle round it, the identity of every map of a model that is not fitted, the affine maps of a fitted one
 and the N == M rule."""
import dataclasses
import itertools

import numpy as np
import pytest

from bayesian_optimisation_amd import gp_device
from bayesian_optimisation_amd.model import JITTER_KERNEL, SurrogateModel, need_se
from oracle import gp_oracle as O

M_, S_ = 40.0, 7.0


def _fitted(rho=3e-2, kernel="se"):
    return SurrogateModel(kernel, rho, 0.0, M_, S_, fitted=True)


def test_frozen_prior_var_is_the_kernels_and_the_oracles_bit_for_bit():
    frozen = SurrogateModel()
    assert (frozen.kernel, frozen.jitter1, frozen.jitter2, frozen.y_mean, frozen.y_scale, frozen.fitted) == \
        ("se", 1e-4, 1e-6, 0.0, 1.0, False)
    assert frozen.prior_var.hex() == gp_device.PRIOR_VAR.hex() == O.PRIOR_VAR.hex()
    assert SurrogateModel("matern52").prior_var.hex() == gp_device.PRIOR_VAR.hex()
    with pytest.raises(dataclasses.FrozenInstanceError):
        frozen.jitter1 = 0.5                                            # a frozen dataclass


@pytest.mark.parametrize("rho", [1e-6, 1e-4, 3e-2, 1.0])
def test_fitted_prior_var_is_one_plus_rho_bit_for_bit(rho):
    assert _fitted(rho).prior_var.hex() == (1.0 + rho).hex()


@pytest.mark.parametrize("kernel", ["se", "matern32", "matern52"])
def test_every_map_of_a_model_that_is_not_fitted_returns_its_argument_itself(kernel):
    m = SurrogateModel(kernel)
    a = np.array([-0.0, np.nan, np.inf, -np.inf, 1.5])
    before = a.tobytes()
    assert m.to_model(a) is a and m.mean_to_y(a) is a and m.sd_to_y(a) is a
    for kind in ("lcb", "ei", "qei"):
        assert m.acq_to_y(kind, a) is a
        best = (2.5, 3, 0)
        assert m.best_to_y(kind, best) is best
    kw = dict(f_best=-0.0, xi=0.25)
    assert m.acq_kw(kw) is kw and kw == dict(f_best=-0.0, xi=0.25)
    for lie in (None, 45.0, np.inf):
        assert m.lie_to_model(lie) is lie
    assert a.tobytes() == before


def test_fitted_maps_are_those_of_the_units_convention():
    m = _fitted()
    mu, sigma, acq = np.array([-0.0, 0.5, -2.0]), np.array([0.0, 0.25, 1.0]), np.array([-1.0, 0.0, 3.0])
    y = np.array([33.0, 40.0, 54.0])
    assert np.array_equal(m.to_model(y), (y - M_) / S_)
    assert np.array_equal(m.mean_to_y(mu), M_ + S_ * mu)                 # mean = m + s mu
    assert np.array_equal(m.sd_to_y(sigma), S_ * sigma)                  # sd = s sigma
    assert np.array_equal(m.acq_to_y("lcb", acq), S_ * acq - M_)         # LCB = s acq - m
    for kind in ("ei", "qei"):
        assert np.array_equal(m.acq_to_y(kind, acq), S_ * acq)           # EI, qEI = s acq
    assert m.best_to_y("lcb", (3.0, 7, 0)) == (S_ * 3.0 - M_, 7, 0) and m.best_to_y("ei", (3.0, 7, 0)) == (S_ * 3.0, 7, 0)
    assert m.acq_kw(dict(f_best=33.0, xi=0.7, explore=4.0)) == dict(f_best=(33.0 - M_) / S_, xi=0.7 / S_, explore=4.0)
    assert m.acq_kw(dict(explore=2.0)) == dict(explore=2.0)              # LCB: explore has no unit
    assert m.acq_kw(dict(f_best=None, xi=0.7)) == dict(f_best=None, xi=0.7 / S_)
    assert m.lie_to_model(45.0) == (45.0 - M_) / S_
    assert m.lie_to_model(None) is None                                  # ... and only a finite lie is mapped
    for lie in (np.inf, -np.inf):
        assert m.lie_to_model(lie) == lie
    assert np.isnan(m.lie_to_model(np.nan))


@pytest.mark.parametrize("same_shape,fitted,kernel", itertools.product([True, False], [True, False], ["se", "matern32", "matern52"]))
def test_diag_add_truth_table(same_shape, fitted, kernel):
    m = _fitted(kernel=kernel) if fitted else SurrogateModel(kernel)
    xs_shape = (50, 2) if same_shape else (64, 2)
    want = JITTER_KERNEL if same_shape and not fitted and kernel == "se" else 0.0
    assert m.diag_add(xs_shape, (50, 2)) == want
    assert m.diag_add(np.zeros(xs_shape).shape, [50, 2]) == want         # (a shape is a shape, tuple or list)


def test_one_refusal_text_for_the_squared_exponential_only_calls():
    need_se("se", "select_batch()")
    with pytest.raises(ValueError, match=r"select_batch\(\) is not available with kernel='matern32': it supports kernel='se' only"):
        need_se("matern32", "select_batch()")
