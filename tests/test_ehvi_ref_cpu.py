"""The restatement of two-objective expected hypervolume improvement (tests/ehvi_ref.py) and the NumPy helpers of the package
(bayesian_optimisation_amd/pareto.py), on the CPU: the 60-digit fixture, the fp64 log form in units of its bound, the strip sum
against the geometry and against Monte Carlo, the properties of the value, the edge rules.

U = 4 for SciPy's log h (tests/test_constrained_ref_cpu.py measures 2.84 units of eps (max(1, z^2 / 2 for z < 0) + |log h|) against
60-digit values); the GPU tests use 10.5 for the device's.  Measured here: see the printed lines and DESIGN.md 4p."""
import os

import numpy as np
import pytest

import ehvi_ref as R
from bayesian_optimisation_amd import pareto as PF

EPS = R.EPS
HERE = os.path.dirname(os.path.abspath(__file__))
PATH = os.path.join(HERE, "golden", "ehvi_cases.npz")
GOLD = np.load(PATH)
U_CPU = 4.0
REL_CAP = 1e-10


def _fixture(k):
    sel = GOLD["fid"] == k
    return [GOLD[n][sel] for n in ("mu1", "s1", "mu2", "s2")], GOLD[f"front_{k}"], tuple(GOLD["ref"][k]), GOLD["want"][sel]


def _random_front(rng, P, step=None):
    step = step if step is not None else float(np.exp(rng.uniform(np.log(1e-3), np.log(3.0))))
    a, c = np.cumsum(step * (1.0 + rng.random(P))), -np.cumsum(step * (1.0 + rng.random(P)))
    return np.stack([a, c], axis=1).reshape(-1, 2), (float(a[-1] if P else 0.0) + rng.uniform(0.1, 2.0), rng.uniform(0.1, 2.0))


def _random_candidates(rng, F, ref, M, spread=30.0):
    lo1, lo2 = (F[0, 0], F[-1, 1]) if len(F) else (ref[0] - 1.0, ref[1] - 1.0)
    w = rng.choice([0.5, 3.0, spread], M)
    return (lo1 - w + rng.random(M) * (ref[0] - lo1 + 2 * w), np.exp(rng.uniform(np.log(0.01), np.log(2.0), M)),
            lo2 - w + rng.random(M) * (ref[1] - lo2 + 2 * w), np.exp(rng.uniform(np.log(0.01), np.log(2.0), M)))


def test_the_fixture_covers_what_it_should_and_the_long_double_form_is_within_its_rounding():
    """|value_ld - 60-digit value| <= eps max(1, |value|): half of it is the one rounding to fp64, the other half is far more than
    the long-double evaluation needs (2^-11 eps per operation, amplified by at most z^2 / 2 <= |value| in the deep tail)."""
    assert os.path.getsize(PATH) < 100 * 1024
    n = GOLD["ref"].shape[0]
    assert sorted({GOLD[f"front_{k}"].shape[0] for k in range(n)}) == [0, 1, 2, 7, 128] and GOLD["want"].size >= 300
    steps, zeros, worst = [], 0, 0.0
    for k in range(n):
        a, F, ref, want = _fixture(k)
        PF.check_front(F, ref)                                   # every fixture front is one the library accepts
        if len(F) > 1:
            steps += [np.diff(F[:, 0]).min(), np.diff(F[:, 0]).max()]
        zeros += int(np.sum((R.plain(*a, F, ref) == 0.0) & np.isfinite(want)))
        got = R.value_ld(*a, F, ref)
        fin = np.isfinite(want)
        assert np.array_equal(got[~fin], want[~fin]) and np.all(want[~fin] == -np.inf)
        worst = max(worst, float(np.max(np.abs(got[fin] - want[fin]) / (EPS * np.maximum(1.0, np.abs(want[fin]))))))
    print(f"long-double form against 60 digits: worst {worst:.3f} eps max(1, |value|); plain sum exactly 0 with a finite logarithm "
          f"at {zeros} of {GOLD['want'].size} cases; front spacings {min(steps):.2e} .. {max(steps):.2e}")
    assert worst <= 1.0 and zeros >= 80 and 1e-3 <= min(steps) < 2.1e-3 and max(steps) >= 10.0


def test_the_fp64_form_is_within_its_bound_of_the_long_double_form():
    """The fixture cases, 60 random fronts of 1 - 20 points (spacings 1e-3 .. 6, means up to 30 away) and 10 fronts of spacing
    1e-3.  The bound itself must stay <= 1e-10 max(1, |value|)."""
    rng = np.random.default_rng(11)
    cases = [_fixture(k)[:3] for k in range(GOLD["ref"].shape[0])]
    for j in range(70):
        F, ref = _random_front(rng, int(rng.integers(1, 21)), None if j < 60 else 1.0e-3)
        cases.append((_random_candidates(rng, F, ref, 100), F, ref))
    worst = worst_eps = worst_bound = 0.0
    for a, F, ref in cases:
        T = R.terms_ld(*a, F, ref)
        want, got, bound = R.value_ld(*a, F, ref, T), R.value64(*a, F, ref), R.value_bound(*a, F, ref, U_CPU, T)
        fin = np.isfinite(want)
        scale = np.maximum(1.0, np.abs(want[fin]))
        assert np.array_equal(got[~fin], want[~fin], equal_nan=True)
        worst = max(worst, float(np.max(np.abs(got[fin] - want[fin]) / bound[fin])))
        worst_eps = max(worst_eps, float(np.max(np.abs(got[fin] - want[fin]) / (EPS * scale))))
        worst_bound = max(worst_bound, float(np.max(bound[fin] / scale)))
    print(f"fp64 form against the long-double form: worst {worst:.3f} of value_bound(U = {U_CPU}), {worst_eps:.2f} eps max(1, |value|); "
          f"worst bound {worst_bound:.2e} max(1, |value|)")
    assert worst <= 1.0 and worst_bound <= REL_CAP


def test_at_zero_sigma_the_strip_sum_is_the_hypervolume_gain():
    rng = np.random.default_rng(12)
    for P in (0, 1, 5, 20):
        F, ref = _random_front(rng, P, 0.3)
        mu1, mu2 = rng.uniform(-1.0, ref[0] + 0.5, 300), rng.uniform(F[-1, 1] - 1.0 if P else -1.0, ref[1] + 0.5, 300)
        zero = np.zeros(300)
        got, log_got = R.plain(mu1, zero, mu2, zero, F, ref), R.value_ld(mu1, zero, mu2, zero, F, ref)
        hv0 = R.hypervolume(F, ref)
        assert abs(PF.hypervolume(F, ref) - hv0) <= 4.0 * (P + 1) * EPS * hv0
        for j in range(300):
            both = np.vstack([F, [mu1[j], mu2[j]]])
            hv1 = R.hypervolume(both, ref)
            assert abs(PF.hypervolume(both, ref) - hv1) <= 4.0 * (P + 2) * EPS * hv1
            assert abs(got[j] - (hv1 - hv0)) <= 4.0 * (P + 2) * EPS * hv1, (P, j)     # two areas of P + 2 rectangles, subtracted
            assert abs(got[j] - R.improvement(mu1[j], mu2[j], F, ref)) <= 4.0 * (P + 2) * EPS * hv1
        ok = got > 4.0 * (P + 2) * EPS * (hv0 + got) * 1e4
        assert ok.sum() > 30 and np.all(np.abs(np.exp(log_got[ok]) - got[ok]) <= 1e-10 * got[ok])
        assert np.all(log_got[got == 0.0] == -np.inf)


def test_the_strip_sum_is_the_monte_carlo_mean_of_the_hypervolume_gain():
    rng = np.random.default_rng(13)
    n = 2_000_000
    e1, e2 = rng.standard_normal(n), rng.standard_normal(n)
    for P, (m1, s1, m2, s2) in ((0, (0.2, 0.5, -0.1, 0.8)), (3, (1.0, 0.7, -1.2, 0.6)), (6, (2.5, 1.5, -0.5, 0.3))):
        F, ref = _random_front(rng, P, 0.5)
        gain = R.improvement(m1 + s1 * e1, m2 + s2 * e2, F, ref)
        mean, se = float(gain.mean()), float(gain.std(ddof=1) / np.sqrt(n))
        got = float(R.plain([m1], [s1], [m2], [s2], F, ref)[0])
        print(f"P = {P}: strip sum {got:.6f}, Monte Carlo {mean:.6f} +- {se:.6f}")
        assert got > 1e-3 and abs(got - mean) <= 5.0 * se
        assert abs(float(R.value_ld([m1], [s1], [m2], [s2], F, ref)[0]) - np.log(got)) <= 1e-12


def test_the_log_value_is_the_logarithm_of_the_plain_sum_where_that_has_not_underflowed():
    """Wherever the plain sum exceeds 1e-280.  The plain form loses bits the log form keeps - phi + z Phi cancels like z^2 below
    z ~ -5 (z^2 eps <= 4e-13 down to the underflow at -38), and a narrow strip is a difference of nearly equal numbers - so the
    two agree to 1e-6 (1 + |value|), not to rounding."""
    rng = np.random.default_rng(14)
    seen = 0
    for _ in range(30):
        F, ref = _random_front(rng, int(rng.integers(0, 21)))
        a = _random_candidates(rng, F, ref, 200)
        p, v = R.plain(*a, F, ref), R.value64(*a, F, ref)
        big = p > 1e-280
        seen += int(big.sum())
        assert np.all(np.abs(v[big] - np.log(p[big])) <= 1e-6 * (1.0 + np.abs(v[big])))
        assert np.all(np.isfinite(v))
    assert seen > 2000


def test_a_further_front_point_never_raises_and_a_wider_reference_point_never_lowers_a_value():
    rng = np.random.default_rng(15)
    for _ in range(20):
        F, ref = _random_front(rng, int(rng.integers(1, 12)), 0.4)
        a = _random_candidates(rng, F, ref, 200, spread=8.0)
        T = R.terms_ld(*a, F, ref)
        v, b = R.value64(*a, F, ref), R.value_bound(*a, F, ref, U_CPU, T)
        extra = [rng.uniform(F[0, 0] - 1.0, ref[0]), rng.uniform(F[-1, 1] - 1.0, ref[1])]
        F2 = PF.pareto_front(np.vstack([F, extra]), ref)         # (the new point may be dominated, or dominate some)
        v2, b2 = R.value64(*a, F2, ref), R.value_bound(*a, F2, ref, U_CPU)
        assert np.all(v2 <= v + b + b2)
        wide = (ref[0] + rng.uniform(0.0, 2.0), ref[1] + rng.uniform(0.0, 2.0))
        v3, b3 = R.value64(*a, F, wide), R.value_bound(*a, F, wide, U_CPU)
        assert np.all(v3 >= v - b - b3)
        assert np.any(v2 < v - b - b2) or not PF.hypervolume(F2, ref) > PF.hypervolume(F, ref)


def test_the_selection_is_invariant_under_affine_maps_of_the_objectives():
    """y_j -> a_j + b_j y_j, b_j > 0, of posteriors, front and reference point: the value shifts by log b_1 + log b_2.  With
    powers of two and a = 0 every standardised argument keeps its bits, so the shift holds to a few roundings; with general
    (a, b) the arguments move by the rounding of the mapped inputs, and the selection is compared where the top two are apart."""
    rng = np.random.default_rng(16)
    F, ref = _random_front(rng, 9, 0.3)
    mu1, s1, mu2, s2 = _random_candidates(rng, F, ref, 500, spread=6.0)
    v = R.value64(mu1, s1, mu2, s2, F, ref)
    for b1, b2 in ((4.0, 0.5), (0.125, 1024.0)):
        w = R.value64(b1 * mu1, b1 * s1, b2 * mu2, b2 * s2, F * [b1, b2], (b1 * ref[0], b2 * ref[1]))
        shift = np.log(b1) + np.log(b2)
        assert np.all(np.abs(w - (v + shift)) <= 8.0 * EPS * (np.abs(v) + abs(shift) + 20.0))
        assert R.first_argmax(w)[1] == R.first_argmax(v)[1]
    (a1, b1), (a2, b2) = (3.7, 1.9), (-250.0, 40.0)
    w = R.value64(a1 + b1 * mu1, b1 * s1, a2 + b2 * mu2, b2 * s2, F * [b1, b2] + [a1, a2], (a1 + b1 * ref[0], a2 + b2 * ref[1]))
    top = np.sort(v)[-2:]
    assert top[1] - top[0] > 1e-6 and R.first_argmax(w)[1] == R.first_argmax(v)[1]
    assert np.all(np.abs(w - (v + np.log(b1) + np.log(b2))) <= 1e-8 * (1.0 + np.abs(v)))


def test_edge_rules():
    F, ref = np.array([[0.0, 1.0], [1.0, 0.0]]), (2.0, 2.0)
    one = np.ones(1)
    for form in (R.value64, R.value_ld):
        for k in range(4):
            a = [0.5 * one, one.copy(), 0.5 * one, one.copy()]
            a[k][0] = np.nan
            assert np.isnan(form(*a, F, ref)[0])
        assert np.isnan(form([np.nan], [0.0], [0.5], [1.0], F, ref)[0])               # NaN beside sigma = 0: NaN
        # sigma = 0 in both: the gain of the mean, (2 - 0.5) (1 - 0.5) - dominated part: strips [.., 0] x, [0, 1], [1, 2]
        assert abs(np.exp(form([0.5], [0.0], [0.5], [0.0], F, ref)[0]) - 0.5 * 0.5) <= 4 * EPS
        assert abs(np.exp(form([-1.0], [0.0], [-1.0], [0.0], F, ref)[0]) - (1.0 * 3.0 + 1.0 * 2.0 + 1.0 * 1.0)) <= 32 * EPS
        # nothing to gain: -inf, not NaN - beyond r in one objective, or dominated; ON an edge counts as no gain
        for m1, m2 in ((2.0, 0.0), (3.0, -5.0), (-5.0, 2.0), (1.0, 1.0), (1.5, 0.5)):
            assert form([m1], [0.0], [m2], [0.0], F, ref)[0] == -np.inf
        assert form([3.0], [0.0], [0.0], [1.0], F, ref)[0] == -np.inf and form([0.0], [1.0], [2.0], [0.0], F, ref)[0] == -np.inf
        # sigma = 0 in objective 1 only, mu1 between the front points: strips 1 and 2 remain; strip 0 is -inf, not NaN
        got = form([0.5], [0.0], [0.3], [0.7], F, ref)[0]
        assert abs(got - np.log(R.plain([0.5], [0.0], [0.3], [0.7], F, ref)[0])) <= 1e-12
        # 60 sigma away in both: finite where the plain sum is 0
        assert np.isfinite(form([50.0], [0.8], [70.0], [1.1], F, ref)[0]) and R.plain([50.0], [0.8], [70.0], [1.1], F, ref)[0] == 0.0
    v = np.array([np.nan, -np.inf, 3.0, np.nan, 3.0])
    assert R.first_argmax(v, 10) == (3.0, 12, 2) and R.first_argmax(np.full(4, -np.inf), 5) == (-np.inf, 5, 0)


def test_pareto_helpers():
    rng = np.random.default_rng(17)
    for n in (1, 2, 10, 200):
        Y = np.round(rng.standard_normal((n, 2)), 1)             # rounded: equal coordinates and duplicate rows occur
        ref = (1.0, 1.2)
        for r in (None, ref):
            F = PF.pareto_front(Y, r)
            assert np.array_equal(F, R.pareto_front(Y, r)) and F.flags["C_CONTIGUOUS"] and F.dtype == np.float64
            assert np.all(np.diff(F[:, 0]) > 0) and np.all(np.diff(F[:, 1]) < 0)
        assert abs(PF.hypervolume(Y, ref) - R.hypervolume(Y, ref)) <= 4.0 * (n + 1) * EPS * max(R.hypervolume(Y, ref), 1.0)
    Y = np.array([[0.0, 1.0], [1.0, 0.0], [0.0, 1.0], [1.0, 1.0], [np.nan, -5.0], [-5.0, np.nan], [0.5, np.inf], [-np.inf, 0.2],
                  [3.0, -1.0], [0.0, 2.0], [2.0, 0.0]])
    assert PF.pareto_front(Y).tolist() == [[0.0, 1.0], [1.0, 0.0], [3.0, -1.0]]     # duplicates once; dominated, NaN, inf rows dropped
    assert PF.pareto_front(Y, (3.0, 3.0)).tolist() == [[0.0, 1.0], [1.0, 0.0]]      # a row ON the reference point is beyond it
    assert PF.pareto_front(Y, (0.0, 3.0)).shape == (0, 2) and PF.pareto_front([]).shape == (0, 2)
    assert PF.hypervolume(Y, (3.0, 3.0)) == 3.0 * 2.0 + 2.0 * 1.0 and PF.hypervolume([], (1.0, 1.0)) == 0.0
    assert PF.reference_point(Y, (2.0, 3)) == (2.0, 3.0) and PF.reference_point(None, [1.5, 2.5]) == (1.5, 2.5)
    assert PF.reference_point(Y, "nadir") == (3.0 + 0.1 * 3.0, 2.0 + 0.1 * 3.0) == R.nadir(Y)   # finite rows only
    for bad in ("worst", (1.0,), (1.0, np.nan), (np.inf, 1.0), (1.0, 2.0, 3.0), None):
        with pytest.raises(ValueError):
            PF.reference_point(Y, bad)
    for flat in ([[1.0, 2.0]], [[1.0, 2.0], [3.0, 2.0]], [[np.nan, 1.0]], []):
        with pytest.raises(ValueError, match="pass ref as two numbers"):
            PF.reference_point(flat, "nadir")
    with pytest.raises(ValueError):
        PF.pareto_front(np.zeros((3, 3)))
    ok = [[0.0, 1.0], [1.0, 0.0]]
    F, r = PF.check_front(ok, (2.0, 2.0))
    assert F.shape == (2, 2) and r == (2.0, 2.0) and PF.check_front(None, (0.0, 0.0))[0].shape == (0, 2)
    big = np.stack([np.arange(129.0), -np.arange(129.0)], axis=1)
    assert PF.check_front(big[:128], (200.0, 1.0))[0].shape == (128, 2)
    for front, ref in ((big, (200.0, 1.0)), (ok, (1.0, 2.0)), (ok, (2.0, 1.0)), (ok[::-1], (2.0, 2.0)), ([[0.0, 1.0], [0.0, 0.0]], (2.0, 2.0)),
                       ([[0.0, 1.0], [1.0, 1.0]], (2.0, 2.0)), ([[0.0, np.nan]], (2.0, 2.0)), ([[-np.inf, 0.0]], (2.0, 2.0)),
                       (ok, (np.inf, 2.0)), (ok, "nadir"), (np.zeros((2, 3)), (2.0, 2.0))):
        with pytest.raises(ValueError):
            PF.check_front(front, ref)
    X = rng.random((5, 2))
    assert PF.observed_pairs(X, np.arange(5.0), X.copy(), -np.arange(5.0)).tolist() == [[k, -k] for k in range(5)]
    for X2, y2 in ((X + 1e-12, np.arange(5.0)), (X[:4], np.arange(4.0)), (X, np.arange(4.0))):
        with pytest.raises(ValueError, match="same measured points"):
            PF.observed_pairs(X, np.arange(5.0), X2, y2)
