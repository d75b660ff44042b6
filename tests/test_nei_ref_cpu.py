"""CPU-only checks of the NumPy restatement of noisy expected improvement (tests/nei_ref.py) that the GPU tests compare with:
its float64 form against its long-double form, the law of the fantasies, the degenerate cases in which it must reduce to plain
EI, and the premise of every GPU value case - that the compared values are not 0 == 0."""
import numpy as np
import pytest

import matern_ref as MR
import nei_ref as R
from ard_fit_ref import gp_problem
from bayesian_optimisation_amd.nei import nei_draws
from oracle import gp_oracle as O

needs_longdouble = pytest.mark.skipif(not R.HAVE_LONGDOUBLE, reason="np.longdouble is 64 bits here")


def _problem(seed, N, d, M=300, S=8):
    X, y = gp_problem(seed, N, d, noise=0.3)
    ls = np.geomspace(0.3, 1.0, d) if d > 1 else np.array([0.3])
    Z, E = nei_draws(N, S, 0)
    return X, y, ls, R.candidates(seed, M, d), Z, E


# The GPU is held to |dmu| <= 1e-9 max(1, |F|), |dsigma| <= 1e-8, |dF| <= 1e-9 max(1, |y|) of THIS float64 restatement:
# the restatement itself must be ten times closer to its long-double form, or those tolerances would measure the restatement.
# A is ill-conditioned by construction (U0 z with |U0| ~ 1 / sqrt(delta)): its distance is only required to be small against
# max |A|, and the GPU test then takes ten times the distance measured on its own case.
@needs_longdouble
@pytest.mark.parametrize("seed,N,d,jitters", [(1, 40, 2, (0.09, 0.0)), (2, 129, 2, (0.09, 0.0)), (3, 129, 8, (0.01, 0.0)),
                                              (4, 129, 2, (1e-4, 1e-6))])
def test_float64_restatement_agrees_with_its_long_double_form(seed, N, d, jitters):
    X, y, ls, Xs, Z, E = _problem(seed, N, d)
    f64 = R.fantasies(X, y, ls, Z, E, jitters)
    fld = R.fantasies(X, y, ls, Z, E, jitters, dtype=R.LD)
    best = R.quantile_best(f64)
    s64 = R.score(X, Xs, ls, f64, best)
    sld = R.score(X, Xs, ls, fld, best, dtype=R.LD)
    fmax = max(1.0, float(np.abs(f64["F"]).max()))
    d_mu = float(np.abs(s64["mu"] - sld["mu"]).max())
    d_sigma = float(np.abs(s64["sigma"] - sld["sigma"]).max())
    d_F = float(np.abs(f64["F"] - fld["F"]).max())
    d_A = float(np.abs(f64["A"] - fld["A"]).max() / np.abs(fld["A"]).max())
    d_nei = float(np.abs(s64["nei"] - sld["nei"]).max())
    print(f"N = {N}, d = {d}, rho = {sum(jitters):g}: |dmu| {d_mu:.2e}, |dsigma| {d_sigma:.2e}, |dF| {d_F:.2e}, "
          f"|dA| / max|A| {d_A:.2e} (max|A| {float(np.abs(fld['A']).max()):.3g}), |dNEI| {d_nei:.2e}")
    assert d_mu <= 1e-10 * fmax
    assert d_sigma <= 1e-9
    assert d_F <= 1e-10 * max(1.0, float(np.abs(y).max()))
    assert d_nei <= 1e-9 * fmax
    assert d_A <= 1e-8


@pytest.mark.parametrize("jitters,family", [((0.09, 0.0), "se"), ((1e-4, 1e-6), "se"), ((0.09, 0.0), "matern52")])
def test_the_fantasies_have_the_posterior_law_of_the_latent_values(jitters, family):
    """F = mean + M_z z + M_e e is linear in the draws: the maps are read off by feeding unit vectors.  Required:
    M_z M_z^T + (rho - delta) M_e M_e^T = K0d - K0d K~^-1 K0d and mean = K0d K~^-1 y, to 1e-10 of the largest entry."""
    dtype = R.LD if R.HAVE_LONGDOUBLE else np.float64
    N, delta = 40, 1e-6
    X, y = gp_problem(1, N, 2, noise=0.3)
    ls = np.array([0.3, 1.0])
    eye, zero = np.eye(N), np.zeros((N, N))
    mean = R.fantasies(X, y, ls, zero[:1], zero[:1], jitters, delta, family, dtype)
    Fz = R.fantasies(X, 0.0 * y, ls, eye, zero, jitters, delta, family, dtype)["F"]     # row s = M_z e_s
    Fe = R.fantasies(X, 0.0 * y, ls, zero, eye, jitters, delta, family, dtype)["F"]     # row s = sqrt(rho - delta) M_e e_s
    K, K0d = mean["K"], mean["K0d"]
    Kinv = mean["U"] @ mean["U"].T
    want_cov = K0d - K0d @ Kinv @ K0d
    want_mean = K0d @ Kinv @ y.astype(dtype)
    got_cov = Fz.T @ Fz + Fe.T @ Fe
    assert float(np.abs(got_cov - want_cov).max()) <= 1e-10 * float(np.abs(want_cov).max())
    assert float(np.abs(mean["F"][0] - want_mean).max()) <= 1e-10 * float(np.abs(want_mean).max())
    # ... and the covariance is not trivially zero: the latent values are uncertain where the noise is not negligible
    assert float(np.abs(want_cov).max()) > 1e-3 * sum(jitters)


@pytest.mark.parametrize("family", ["se", "matern32"])
def test_rho_equal_delta_every_fantasy_is_y_and_nei_is_plain_ei(family):
    rho = 0.09
    X, y, ls, Xs, Z, E = _problem(2, 40, 2)
    fan = R.fantasies(X, y, ls, Z, E, (rho, 0.0), rho, family)
    assert float(np.abs(fan["F"] - y[None, :]).max()) <= 1e-10 * max(1.0, float(np.abs(y).max()))
    sc = R.score(X, Xs, ls, fan, delta=rho, family=family)
    mu, sigma = MR.posterior(X, y, Xs, ls, family, rho, 0.0)
    want = O.expected_improvement(mu, sigma, float(y.min()))
    assert float(np.abs(sc["nei"] - want).max()) <= 1e-9
    assert want.max() > R.INFORMATIVE


def test_one_fantasy_with_a_given_incumbent_is_ei_at_that_incumbent():
    X, y, ls, Xs, Z, E = _problem(3, 40, 2, S=1)
    fan = R.fantasies(X, y, ls, Z, E, (0.09, 0.0))
    b = float(np.quantile(fan["F"][0], 0.7))
    sc = R.score(X, Xs, ls, fan, best=[b], xi=0.01)
    assert np.array_equal(sc["nei"], R.ei(sc["mu"][0], sc["sigma"], b, 0.01))
    assert float(np.abs(sc["nei"] - O.expected_improvement(sc["mu"][0], sc["sigma"], b, 0.01)).max()) <= 1e-14
    assert sc["nei"].max() > R.INFORMATIVE


def test_ei_restates_the_device_function_at_its_corners():
    mu = np.array([0.0, 0.5, -0.5, 0.0, 0.0])
    sigma = np.array([0.0, 0.0, 0.0, np.nan, 1.0])
    got = R.ei(mu, sigma, 0.0)
    assert got[0] == 0.0 and got[1] == 0.0 and got[2] == 0.5 and np.isnan(got[3])
    assert abs(got[4] - 0.39894228040143267794) <= 1e-16
    assert np.isnan(R.ei(np.array([np.nan]), np.array([1.0]), 0.0)[0])


@pytest.mark.parametrize("name", sorted(R.CASES))
def test_every_gpu_value_case_is_informative(name):
    """With the incumbents at the 0.7-quantile of each fantasy at most 40 % of a case's candidates have a reference value below
    1e-6 (those are left out of the comparison).  If a case fails this, change its input, not the cap."""
    ref = R.case_reference(name)
    keep, left_out = R.informative(ref["score"]["nei"])
    print(f"{name}: {100 * left_out:.1f} % of {keep.size} candidates left out")
    assert np.isfinite(ref["score"]["nei"]).all()
    assert left_out <= R.MAX_LEFT_OUT
    assert keep.sum() >= 5


def test_with_the_row_minima_few_values_are_informative():
    """Why the value tests do not use the fantasies' own minima: most candidates then have NEI < 1e-6."""
    for name in ("n40_d2_s16_m1537", "n40_d2_s16_m1000_seed2"):
        ref = R.case_reference(name)
        X, y, ls, Xs, Z, E, jitters, family, S = ref["problem"]
        _, left_out = R.informative(R.score(X, Xs, ls, ref["fan"], None, 0.0, 1e-6, family)["nei"])
        assert left_out > R.MAX_LEFT_OUT


def nei_and_ei_choices(seed=2):
    """(index NEI picks, index EI with f_best = min(y) picks, NEI values, EI values) on the issue's 40-point problem."""
    X, y = gp_problem(seed, 40, 2, noise=0.3)
    ls, Xs = np.array([0.3, 1.0]), R.candidates(seed, 1600, 2)
    Z, E = nei_draws(40, 16, 0)
    fan = R.fantasies(X, y, ls, Z, E, (0.09, 0.0))
    nei = R.score(X, Xs, ls, fan)["nei"]
    mu, sigma = MR.posterior(X, y, Xs, ls, "se", 0.09, 0.0)
    ei = O.expected_improvement(mu, sigma, float(y.min()))
    return R.argmax_first(nei), R.argmax_first(ei), nei, ei, y, fan


def test_nei_and_min_y_ei_pick_different_candidates():
    i_nei, i_ei, nei, ei, y, fan = nei_and_ei_choices()
    assert i_nei != i_ei
    assert R.top2_gap(nei) > 1e-7 and R.top2_gap(ei) > 1e-7
    # min(y) is the luckiest noise draw: every fantasy's incumbent lies above it
    assert float(fan["best"].min()) > float(y.min())
