"""The NumPy restatement of the ensemble scoring (tests/ensemble_ref.py) against itself, and the premises of the GPU cases that
compare selected indices (tests/test_gpu_ensemble.py): no GPU needed."""
import numpy as np
import pytest

import ensemble_ref as E
import matern_ref as MR


def _single():
    X, y, Xs, _ = E.case_problem(129, 513, 3)
    y = (y - 40.0) / 7.0
    ls = np.array([0.5, 0.8, 1.1])
    return X, y, Xs, ls


@pytest.mark.parametrize("kind", [E.LCB, E.EI])
def test_one_model_of_weight_one_is_the_single_model_formulas(kind):
    X, y, Xs, ls = _single()
    mu, sigma = MR.posterior(X, y, Xs, ls, "se", 1e-4, 1e-6)
    p0, p1 = E.case_params(kind, y)
    r = E.score(X, y, Xs, [(ls, 1e-4, 1e-6, 0.0, 1.0, 1.0)], kind, p0, p1)
    assert np.array_equal(r["acq"], E.acquisition(kind, mu, sigma, p0, p1)) and np.array_equal(r["mean"], mu)
    np.testing.assert_allclose(r["sd"], sigma, rtol=0, atol=1e-12)   # sqrt((sigma^2 + mu^2) - mu^2)
    assert r["best_idx"] == int(np.argmax(r["acq"])) and r["best_val"] == r["acq"].max()
    # the units of y: the same model of 40 + 7 y reports 40 + 7 mu, 7 sigma
    r7 = E.score(X, 40.0 + 7.0 * y, Xs, [(ls, 1e-4, 1e-6, 40.0, 7.0, 1.0)], kind, *E.case_params(kind, 40.0 + 7.0 * y)[:1],
                 7.0 * p1)
    np.testing.assert_allclose(r7["mean"], 40.0 + 7.0 * mu, rtol=1e-13)
    np.testing.assert_allclose(r7["sd"], 7.0 * sigma, rtol=0, atol=1e-10)
    assert r7["best_idx"] == r["best_idx"]


def test_expected_improvement_edge_cases():
    assert E.acquisition(E.EI, 1.0, 0.0, 2.0, 0.25) == 0.75 and E.acquisition(E.EI, 3.0, 0.0, 2.0) == 0.0
    assert np.isnan(E.acquisition(E.EI, 1.0, np.nan, 2.0)) and np.isnan(E.acquisition(E.LCB, np.nan, 1.0, 4.0))
    assert E.acquisition(E.EI, 0.0, 1.0, 0.0) == pytest.approx(0.39894228040143267794, rel=1e-15)


@pytest.mark.parametrize("kind", [E.LCB, E.EI])
def test_duplicating_every_model_with_half_its_weight_changes_nothing_beyond_rounding(kind):
    X, y, Xs, models = E.case_problem(129, 513, 3)
    p0, p1 = E.case_params(kind, y)
    a = E.score(X, y, Xs, models, kind, p0, p1)
    twice = [m[:5] + (0.5 * m[5],) for m in models for _ in range(2)]
    b = E.score(X, y, Xs, twice, kind, p0, p1)
    scale = np.max(np.abs(a["acq"]))
    np.testing.assert_allclose(b["acq"], a["acq"], rtol=0, atol=1e-14 * scale)
    np.testing.assert_allclose(b["mean"], a["mean"], rtol=1e-14)
    np.testing.assert_allclose(b["var"], a["var"], rtol=0, atol=1e-13 * np.max(a["var"]))
    assert b["best_idx"] == a["best_idx"]


def test_a_nan_candidate_is_left_out_of_the_arg_max():
    X, y, Xs, models = E.case_problem(7, 511, 3)
    Xs = Xs.copy()
    Xs[5, 1] = np.nan
    r = E.score(X, y, Xs, models, E.LCB, E.EXPLORE)
    assert np.isnan(r["acq"][5]) and np.sum(np.isnan(r["acq"])) == 1 and r["best_idx"] != 5


def test_the_mixture_variance_holds_the_spread_of_the_means():
    """Two models that agree on sigma and differ in the mean by 2 delta: var = sigma^2 + delta^2."""
    post = [(np.array([1.0, 5.0]), np.array([0.5, 0.1])), (np.array([3.0, 5.0]), np.array([0.5, 0.1]))]
    models = [(None, 0.0, 0.0, 10.0, 1.0, 0.5), (None, 0.0, 0.0, 20.0, 1.0, 0.5)]
    r = E.fold(post, models, E.LCB, 0.0)
    np.testing.assert_allclose(r["mean"], [2.0, 5.0], rtol=1e-15)
    np.testing.assert_allclose(r["var"], [0.25 + 1.0, 0.01], rtol=1e-12)
    assert r["shift"] == 15.0


@pytest.mark.parametrize("N,M,d,family", E.CASES)
@pytest.mark.parametrize("kind", [E.LCB, E.EI])
def test_the_top_two_of_every_gpu_case_are_further_apart_than_twice_its_bound(N, M, d, family, kind):
    """The GPU test asserts the restatement's arg-max: the runner-up must be out of reach of both sides' error."""
    X, y, Xs, models = E.case_problem(N, M, d)
    assert len({tuple(m[0]) for m in models}) == 5 and min(m[1] for m in models) >= 1e-4 and abs(sum(m[5] for m in models) - 1) < 1e-15
    p0, p1 = E.case_params(kind, y)
    r = E.score(X, y, Xs, models, kind, p0, p1, family)
    B = E.acq_bound(y, models, kind, E.EXPLORE)
    assert np.all(np.isfinite(r["acq"])) and 0.0 < B < 1e-6
    if M > 1:
        top = np.sort(r["acq"])[-2:]
        print(f"N {N} M {M} d {d} {family} {kind}: gap {top[1] - top[0]:.3e}, bound {B:.3e}")
        assert top[1] - top[0] > 2.0 * B
