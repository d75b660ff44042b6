"""CPU-only checks of the NumPy / SciPy restatement of max-value entropy search (tests/mes_ref.py) and of the package's own
host-side rule (bayesian_optimisation_amd/mes.py): the terms against 60-digit values (tests/golden/mes_terms.npz, written by
tests/golden/make_mes_golden.py), the quartile rule against its closed form on one candidate and against log S itself on 1,000,
the Gumbel samples, the cap, the degenerate width, the edge rules."""
import os

import numpy as np
import pytest
from scipy import special as sp

import mes_ref as R
from bayesian_optimisation_amd import mes as MES

EPS = np.finfo(np.float64).eps
GOLD = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "mes_terms.npz"))


def test_the_fixture_covers_the_range_and_the_far_tail():
    g = GOLD["gamma"]
    assert g.size == 2004 and g[:2001].min() == -40.0 and g[:2001].max() == 40.0
    assert set(g[2001:].tolist()) == {-1e2, -1e3, -1e4}
    assert np.all(np.isfinite(GOLD["h"])) and np.all(GOLD["h"] >= 0.0) and np.all(GOLD["log_ndtr"] <= 0.0)
    assert abs(GOLD["h"][np.flatnonzero(g == 0.0)[0]] - np.log(2.0)) <= 2 * EPS   # h(0) = -log(1/2)


def test_h_matches_60_digit_values():
    g, want = GOLD["gamma"], GOLD["h"]
    err = np.abs(R.h(g) - want)
    unit = EPS * (np.maximum(1.0, np.where(g < 0.0, 0.5 * g * g, 0.0)) + np.abs(want))
    worst = float(np.max(err / unit))
    print(f"h: worst error {worst:.2f} units of eps (max(1, gamma^2/2 for gamma<0) + |h|)")
    assert worst <= 8.0


def test_log_ndtr_matches_60_digit_values():
    g, want = GOLD["gamma"], GOLD["log_ndtr"]
    err = np.abs(R.log_ndtr(g) - want)
    assert np.all(err <= 8.0 * EPS * np.abs(want)), float(np.max(err / np.maximum(np.abs(want), 1e-300)) / EPS)


def test_limits_and_nan_of_h():
    out = R.h(np.array([np.nan, np.inf, -np.inf, 0.0]))
    assert np.isnan(out[0]) and out[1] == 0.0 and out[2] == np.inf and abs(out[3] - np.log(2.0)) <= 2 * EPS


def _one(mu, sigma):
    return lambda z: R.log_survival(np.array([mu]), np.array([sigma]), z)


@pytest.mark.parametrize("mu,sigma", [(1.5, 0.3), (-20.0, 4.0), (3.0, 1e-3)])
def test_one_candidate_has_the_closed_form_quartiles(mu, sigma):
    """S(z) = Phi((mu - z) / sigma): z_p = mu - sigma Phi^-1(p); the upper bracket IS z25 here (the last level)."""
    lo, hi = R.brackets([mu], [sigma])
    want = mu - sigma * sp.ndtri(np.array(R.PROBS))
    got = R.quartiles(lambda z: _one(mu, sigma)(z)[0], lo, hi)
    np.testing.assert_allclose(got, want, rtol=1e-8)
    pkg, n = MES.gumbel_quartiles(_one(mu, sigma), lo, hi)
    assert n == 0 and np.array_equal(pkg, got)   # the package's rule is this rule, bit for bit


def _cloud(M=1000, seed=3):
    rng = np.random.default_rng(seed)
    return rng.standard_normal(M), np.exp(rng.uniform(np.log(0.05), np.log(1.5), M))


def test_quartiles_of_a_thousand_candidates_solve_log_s():
    mu, sigma = _cloud()
    lo, hi = R.brackets(mu, sigma)
    calls = []

    def ls(z):
        calls.append(len(z))
        return R.log_survival(mu, sigma, z)

    q, n = MES.gumbel_quartiles(ls, lo, hi)
    assert calls == [63] * 4 and n == 0                       # four rounds of 3 x 21 levels
    assert q[0] < q[1] < q[2]                                 # z75 < z50 < z25
    resid = np.abs(R.log_survival(mu, sigma, q)[0] - np.log(np.array(R.PROBS)))
    print("|log S(z_p) - log p| =", resid)
    assert np.all(resid <= 1e-6)
    assert np.array_equal(q, R.quartiles(lambda z: R.log_survival(mu, sigma, z)[0], lo, hi))
    # the brackets hold what the rule says they hold
    s_lo, s_hi = np.exp(R.log_survival(mu, sigma, [lo, hi])[0])
    assert s_lo >= 0.75 and s_hi <= 0.25


def test_gumbel_samples_follow_the_fitted_law():
    q = np.array([-2.4, -2.0, -1.7])
    u = R.uniforms(64, 5)
    m = MES.sample_minima(q, MES.mes_uniforms(64, 5))
    assert np.array_equal(MES.mes_uniforms(64, 5), u) and np.array_equal(m, R.gumbel_samples(q, u))
    # two parameters through three levels: the law's median is z50 and its interquartile range is z25 - z75 (u = p gives the
    # law's own level of Pr[m* > z] = p, since w = -m* has Pr[w < -z_p] = p)
    back = MES.sample_minima(q, np.array(R.PROBS))
    np.testing.assert_allclose([back[1], back[2] - back[0]], [q[1], q[2] - q[0]], rtol=1e-13)
    assert np.all(np.diff(m[np.argsort(u)]) <= 0.0)           # larger u, larger maximum of -f, smaller minimum


def test_cap_and_degenerate_width():
    q = np.array([-2.4, -2.0, -1.7])
    u = MES.mes_uniforms(32, 1)
    free = MES.sample_minima(q, u)
    capped = MES.sample_minima(q, u, cap=-2.0)
    assert np.any(free > -2.0) and np.array_equal(capped, np.minimum(free, -2.0))
    assert np.array_equal(MES.sample_minima([0.5, 0.5, 0.5], u), np.full(32, 0.5))
    assert np.array_equal(MES.sample_minima([0.5, 0.5, 0.5], u, cap=0.25), np.full(32, 0.25))
    assert np.array_equal(R.gumbel_samples([0.5, 0.5, 0.5], u), np.full(32, 0.5))
    # an exact zero among the draws is replaced by the next float
    assert np.all(MES.mes_uniforms(64, 0) > 0.0) and np.all(MES.mes_uniforms(64, 0) < 1.0)


def test_a_point_mass_has_a_degenerate_fit():
    """Every candidate with sigma = 0: log S steps from 0 to -inf at the smallest mean; the three levels coincide within the
    last round's spacing and the samples are that value."""
    mu, sigma = np.array([0.7, 0.3, 0.9]), np.zeros(3)
    lo, hi = R.brackets(mu, sigma)
    assert lo == hi == 0.3
    q, _ = MES.gumbel_quartiles(lambda z: R.log_survival(mu, sigma, z), lo, hi)
    assert np.array_equal(q, [0.3, 0.3, 0.3])
    assert np.array_equal(MES.sample_minima(q, MES.mes_uniforms(4, 0)), np.full(4, 0.3))


def test_edge_rules_of_the_restatement():
    mu = np.array([0.0, 1.0, np.nan, 2.0, -1.0])
    sigma = np.array([1.0, 0.0, 1.0, np.nan, 0.0])
    z = np.array([0.5, -2.0])
    ls, n = R.log_survival(mu, sigma, z)
    assert n == 2
    assert ls[0] == -np.inf                                   # candidate 4: sigma = 0 and mu = -1 <= 0.5
    assert ls[1] == R.log_ndtr(2.0)                        # both point masses above -2: only candidate 0 contributes
    acq, _ = R.acquisition(mu, sigma, [-0.5, -1.0])
    assert np.isnan(acq[2]) and np.isnan(acq[3]) and acq[1] == 0.0 and acq[4] == 0.0 and acq[0] > 0.0
    assert R.first_argmax(acq) == (0, 2)
    assert R.first_argmax(np.array([np.nan, 1.0, 1.0])) == (1, 1) and R.first_argmax(np.array([np.nan])) == (-1, 1)


def test_parameter_checks():
    assert MES.mes_params(16, 0) == (16, 0, "observed") and MES.mes_params(np.int64(64), 3, None) == (64, 3, None)
    assert MES.mes_params(1, 0, -0.5) == (1, 0, -0.5)
    for bad in (dict(n_samples=0), dict(n_samples=65), dict(n_samples=2.0), dict(n_samples=True), dict(seed=-1), dict(seed=0.5),
                dict(cap=float("nan")), dict(cap=float("inf")), dict(cap="min"), dict(cap=[1.0])):
        kw = dict(n_samples=16, seed=0)
        kw.update(bad)
        with pytest.raises(ValueError):
            MES.mes_params(**kw)
    assert MES.mes_y_star("gumbel", 4) == "gumbel" and MES.mes_y_star("thompson", 4) == "thompson"
    assert np.array_equal(MES.mes_y_star([1, 2, 3], 3), [1.0, 2.0, 3.0])
    for bad in ("sobol", [1.0, 2.0], [1.0, np.nan, 0.0], [1.0, np.inf, 0.0]):
        with pytest.raises(ValueError):
            MES.mes_y_star(bad, 3)
    with pytest.raises(ValueError):
        MES.gumbel_quartiles(lambda z: (z, 0), 1.0, 0.0)
    with pytest.raises(ValueError):
        MES.gumbel_quartiles(lambda z: (z, 0), float("-inf"), 0.0)
