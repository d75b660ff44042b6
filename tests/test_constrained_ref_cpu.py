"""CPU-only checks of the NumPy / SciPy restatement of the constrained acquisitions (tests/constrained_ref.py) and of the package's
own host-side rules (bayesian_optimisation_amd/constrained.py): log h against 60-digit values (tests/golden/cons_terms.npz,
written by tests/golden/make_constrained_golden.py), the value against the logarithm of the plain product where that product
exists, monotonicity in the constraints, the edge rules, the limits and the incumbent rule.

Measured here (SciPy 1.15, x86-64), in units of eps (max(1, z^2 / 2 for z < 0) + |log h|): the fp64 forms of include/gpbo.h are
within 0.75 (z >= 0), 0.61 (-1 <= z < 0), 2.63 (-1e3 < z < -1; the worst point is z = -11.84) and 0.52 (z <= -1e3) units of the
fixture; the long-double forms of the restatement (no erfc: a continued fraction and a series) within 0.45 units everywhere,
which is the rounding of their fp64 result."""
import os

import numpy as np
import pytest
from scipy import special as sp

import constrained_ref as R
from bayesian_optimisation_amd import constrained as CONS

EPS = np.finfo(np.float64).eps
HERE = os.path.dirname(os.path.abspath(__file__))
GOLD = np.load(os.path.join(HERE, "golden", "cons_terms.npz"))
MES_GOLD = np.load(os.path.join(HERE, "golden", "mes_terms.npz"))
FP64_BOUND = 2.84   # the worst value the fp64 forms were measured at when the formula was chosen; here 2.63 (see above)


def test_the_fixture_covers_the_range_the_branch_edges_and_the_far_tail():
    z, lh = GOLD["z"], GOLD["log_h"]
    assert z.size == 2007 and z[:2001].min() == -40.0 and z[:2001].max() == 40.0
    assert z[2001:].tolist() == [-1e2, -3e2, -999.0, -1e3, -1e4, -1e6]
    assert np.all(np.isfinite(lh))
    assert abs(lh[np.flatnonzero(z == 0.0)[0]] + 0.5 * np.log(2.0 * np.pi)) <= 2 * EPS          # h(0) = phi(0)
    assert abs(lh[np.flatnonzero(z == 40.0)[0]] - np.log(40.0)) <= 2 * EPS * np.log(40.0)      # h(z) -> z
    assert set(R.log_h_branch(z).tolist()) == {0, 1, 2, 3} and R.log_h_branch(np.array([-1e3, -999.0, -1.0])).tolist() == [3, 2, 1]
    # plain EI is gone where the logarithm is an ordinary number: the reason for the formula
    with np.errstate(under="ignore"):
        plain = np.exp(-0.5 * 39.0 ** 2) / np.sqrt(2 * np.pi) - 39.0 * sp.ndtr(-39.0)
    assert plain == 0.0 and -770.0 < lh[np.flatnonzero(z == -39.0)[0]] < -760.0


def test_fp64_log_h_stays_within_its_measured_bound_of_60_digit_values():
    z, want = GOLD["z"], GOLD["log_h"]
    worst = R.fixture_worst(R.log_h, z, want, R.log_h_branch(z))
    print("log h, fp64 forms: worst error per branch (z >= 0, [-1, 0), (-1e3, -1), <= -1e3) "
          + ", ".join(f"{w:.2f}" for w in worst) + " units of eps (max(1, z^2/2 for z<0) + |log h|)")
    assert max(worst) <= FP64_BOUND


def test_the_long_double_forms_are_a_reference_between_the_fixture_points():
    z = GOLD["z"]
    worst_h = R.fixture_worst(R.log_h_hp, z, GOLD["log_h"], R.log_h_branch(z))
    worst_p = R.fixture_worst(R.log_ndtr_hp, MES_GOLD["gamma"], MES_GOLD["log_ndtr"])
    print("long-double forms: log h per branch " + ", ".join(f"{w:.2f}" for w in worst_h) + f"; log Phi {worst_p[0]:.2f} units")
    assert max(worst_h) <= 0.5 and worst_p[0] <= 0.5
    # ... and the fp64 log Phi of the header, restated, is within the 8 units the device's own is held to
    assert R.fixture_worst(R.log_ndtr64, MES_GOLD["gamma"], MES_GOLD["log_ndtr"])[0] <= 8.0


def test_limits_and_nan_of_the_terms():
    for fn in (R.log_h, R.log_h_hp):
        out = fn(np.array([np.nan, np.inf, -np.inf]))
        assert np.isnan(out[0]) and out[1] == np.inf and out[2] == -np.inf
    for fn in (R.log_ndtr64, R.log_ndtr_hp):
        out = fn(np.array([np.nan, np.inf, -np.inf]))
        assert np.isnan(out[0]) and out[1] == 0.0 and out[2] == -np.inf


def _posteriors(rng, M, C, spread):
    mu, sigma = rng.normal(0.0, spread, M), np.exp(rng.uniform(np.log(0.05), np.log(3.0), M))
    cm, cs = rng.normal(0.0, spread, (C, M)), np.exp(rng.uniform(np.log(0.05), np.log(3.0), (C, M)))
    return mu, sigma, cm, cs, rng.normal(0.0, 1.0, C)


@pytest.mark.parametrize("base", [R.BASE_NONE, R.BASE_EI, R.BASE_PI])
@pytest.mark.parametrize("C", [0, 1, 3, 8])
def test_value_is_the_log_of_the_plain_product_where_that_exists(base, C):
    if base == R.BASE_NONE and C == 0:
        return   # (no such call)
    rng = np.random.default_rng(100 + 10 * base + C)
    mu, sigma, cm, cs, u = _posteriors(rng, 4000, C, 2.0)
    f_best, xi = -0.3, 0.01
    v, feas = R.value(mu, sigma, cm, cs, u, base, f_best, xi, hp=False)
    with np.errstate(all="ignore"):
        z = ((f_best - mu) - xi) / sigma
        plain = np.ones_like(mu)
        if base == R.BASE_EI:
            plain = sigma * (np.exp(-0.5 * z * z) / np.sqrt(2.0 * np.pi) + z * sp.ndtr(z))
        elif base == R.BASE_PI:
            plain = sp.ndtr(z)
        for c in range(C):
            plain = plain * sp.ndtr((u[c] - cm[c]) / cs[c])
    ok = plain > 1e-280
    assert ok.sum() > 400
    # the restatement: 8 units of each term's scale.  The plain forms are the weaker side: a CDF carries the rounding of its
    # argument, eps gamma^2 / 2 of a factor (inside the 8 units), and plain EI below 0 adds phi and z Phi - each with a relative
    # error of (z^2 / 2 + 4) eps from exp's and erfc's arguments - to a sum of about phi / (z^2 + 1): (z^2 + 8) (z^2 + 2) eps
    bound = R.value_bound(mu, sigma, cm, cs, u, base, f_best, xi, 8.0, 8.0)
    if base == R.BASE_EI:
        bound = bound + np.where(z < 0.0, EPS * (z * z + 8.0) * (z * z + 2.0), 8.0 * EPS)
    assert np.all(np.abs(v[ok] - np.log(plain[ok])) <= bound[ok])
    assert np.all(feas <= 0.0)


def test_adding_a_constraint_never_raises_a_value():
    rng = np.random.default_rng(7)
    mu, sigma, cm, cs, u = _posteriors(rng, 3000, 8, 30.0)
    for hp in (False, True):
        prev = R.value(mu, sigma, cm[:0], cs[:0], u[:0], R.BASE_EI, 0.2, 0.0, hp)[0]
        for C in range(1, 9):
            v = R.value(mu, sigma, cm[:C], cs[:C], u[:C], R.BASE_EI, 0.2, 0.0, hp)[0]
            assert np.all(v <= prev)
            prev = v
    assert np.all(np.isfinite(prev)) and prev.min() < -1e3   # far inside the infeasible region, still ordered


def test_the_underflow_case_keeps_its_order_in_log_space():
    M, C = 500, 8
    rng = np.random.default_rng(3)
    cm, cs = rng.uniform(30.0, 60.0, (C, M)), np.ones((C, M))
    cm[:, 123] = 30.0                                  # the least infeasible candidate
    with np.errstate(under="ignore"):
        plain = np.prod(sp.ndtr((0.0 - cm) / cs), axis=0)
    assert np.all(plain == 0.0)                        # every candidate ties at exactly 0
    v, _ = R.value(None, None, cm, cs, np.zeros(C), R.BASE_NONE)
    assert np.all(np.isfinite(v)) and R.first_argmax(v)[1] == 123


def test_edge_rules_of_the_value():
    nan, inf = np.nan, np.inf
    mu, sigma = np.array([0.0, nan, 0.0, 0.0, 1.0, -1.0]), np.array([1.0, 1.0, nan, 0.0, 0.0, 0.0])
    for hp in (False, True):
        ei, _ = R.value(mu, sigma, None, None, [], R.BASE_EI, 0.0, 0.0, hp)
        pi, _ = R.value(mu, sigma, None, None, [], R.BASE_PI, 0.0, 0.0, hp)
        assert np.isnan(ei[1]) and np.isnan(ei[2]) and ei[3] == -inf and ei[4] == -inf and ei[5] == 0.0   # log(max(imp, 0))
        assert np.isnan(pi[1]) and np.isnan(pi[2]) and pi[3] == -inf and pi[4] == -inf and pi[5] == 0.0
        cm, cs = np.array([[0.0, 1.0, 1.0 + 1e-12, nan, 0.0]]), np.array([[0.0, 0.0, 0.0, 0.0, nan]])
        v, feas = R.value(None, None, cm, cs, [1.0], R.BASE_NONE, hp=hp)
        assert v.tolist()[:3] == [0.0, 0.0, -inf] and np.isnan(v[3]) and np.isnan(v[4]) and np.array_equal(v, feas, equal_nan=True)
    assert R.first_argmax([nan, -inf, -inf], 5) == (-inf, 6, 1)          # -inf is a legal value; NaN is never chosen
    assert R.first_argmax([nan, nan]) == (-inf, np.iinfo(np.int64).max, 2)
    assert R.first_argmax([1.0, 2.0, 2.0, nan], 1 << 33) == (2.0, (1 << 33) + 1, 1)


def test_limits_and_parameters_of_the_package():
    u = CONS.cons_limits([1, 2.5])
    assert u.dtype == np.float64 and u.flags.c_contiguous and u.tolist() == [1.0, 2.5]
    assert CONS.cons_limits(None).size == 0 and CONS.cons_limits([], 0).size == 0 and CONS.cons_limits(np.zeros(8)).size == 8
    for bad in (np.zeros(9), [np.nan], [np.inf], [0.0, -np.inf]):
        with pytest.raises(ValueError):
            CONS.cons_limits(bad)
    with pytest.raises(ValueError, match="one limit per constraint"):
        CONS.cons_limits([1.0], 2)
    assert CONS.cons_params("none", None, None, 2) == (0, 0.0, 0.0)
    assert CONS.cons_params("ei", 1, 0.5, 0) == (1, 1.0, 0.5) and CONS.cons_params("pi", -2.0, 0, 3) == (2, -2.0, 0.0)
    for args in (("none", 0.0, 0.0, 0), ("lcb", 0.0, 0.0, 1), (1, 0.0, 0.0, 1), ("ei", None, 0.0, 1), ("ei", np.nan, 0.0, 1),
                 ("pi", 0.0, np.inf, 1), ("ei", "feasible", 0.0, 1), ("ei", True, 0.0, 1)):
        with pytest.raises(ValueError):
            CONS.cons_params(*args)
    assert CONS.incumbent_rule("feasible") == "feasible" and CONS.incumbent_rule(3) == 3.0
    for bad in ("best", None, np.nan, [1.0]):
        with pytest.raises(ValueError):
            CONS.incumbent_rule(bad)


def test_the_incumbent_rule():
    rng = np.random.default_rng(11)
    X = rng.uniform(size=(12, 2))
    y, g0, g1 = rng.normal(size=12), rng.normal(size=12), rng.normal(size=12)
    u = [0.3, 0.1]
    g0[np.argmin(y)] = 10.0                            # the smallest observation of all is not feasible
    feasible = (g0 <= u[0]) & (g1 <= u[1])
    assert 1 < feasible.sum() < 12
    for F in (CONS.feasible_incumbent, R.feasible_incumbent):
        # the smallest objective value of the feasible subset: not the smallest observation
        got = F(X, y, [X.copy(), X.tolist()], [g0, g1.tolist()], u)
        assert got == y[feasible].min() and got > y.min()
        assert F(X, y, [], [], []) == y.min()                                       # no constraint: the plain incumbent
        assert F(X, y, [X], [g0], [g0.min()]) == y[np.argmin(g0)]                   # <= : the limit itself is feasible
        assert F(X, y, [X, X], [g0, g1], [g0.min() - 1.0, 10.0]) is None            # none feasible
        ynan = y.copy()
        ynan[np.flatnonzero(feasible)[0]] = np.nan                                  # a NaN observation is not feasible
        assert F(X, ynan, [X, X], [g0, g1], u) == np.nanmin(np.where(feasible, ynan, np.nan))
        # mismatched measured points: one bit, the order, the count
        X1 = X.copy()
        X1[5, 1] = np.nextafter(X1[5, 1], 2.0)
        for Xc, gc in ((X1, g0), (X[::-1], g0), (X[:11], g0[:11])):
            with pytest.raises(ValueError):
                F(X, y, [X, Xc], [g1, gc], u)
    gnan = g0.copy()
    gnan[:] = np.nan
    assert CONS.feasible_incumbent(X, y, [X], [gnan], [0.0]) is None                # a NaN constraint value is not feasible
