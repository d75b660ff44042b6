"""Noisy expected improvement on the GPU (csrc/nei.hip; DeviceGP.fantasies / score_nei / select_nei,
PointSelector.noisy_expected_improvement, PointSelectorHost.noisy_expected_improvement, gpbo_nei_host_f64) against
tests/nei_ref.py, the NumPy restatement (the reference project has no EI), whose own accuracy tests/test_nei_ref_cpu.py pins.
Tolerances: the project's - |dmu_s| <= 1e-9 max(1, |F|_inf), |dsigma_0| <= 1e-8, |dNEI| <= 1e-8 max(1, |F|_inf) -
on the candidates whose reference value is >= 1e-6, with the incumbents at the 0.7-quantile of each fantasy so that most are."""
import numpy as np
import pytest
import torch  # noqa: F401  (before the host-pointer binding initialises HIP)

pytestmark = pytest.mark.gpu

import nei_ref as R  # noqa: E402
from ard_fit_ref import gp_problem  # noqa: E402
from bayesian_optimisation_amd import DeviceGP, PointSelector, PointSelectorHost  # noqa: E402
from bayesian_optimisation_amd import host_binding as H  # noqa: E402
from bayesian_optimisation_amd.nei import nei_draws  # noqa: E402
from test_nei_ref_cpu import nei_and_ei_choices  # noqa: E402

DEV = "cuda:0"
OFFSET = 10 ** 9 + 7
DELTA = 1e-6
_GPS = {}


def _surrogate(name, chunk=None):
    """(DeviceGP, its Fantasies) of a value case, made once per (case, chunk) and shared (nothing in the tests changes them)."""
    key = (name, chunk)
    if key not in _GPS:
        X, y, ls, Xs, Z, E, jitters, family, S = R.case_reference(name)["problem"]
        gp = DeviceGP(device=DEV) if chunk is None else DeviceGP(device=DEV, chunk=chunk)
        gp.factorise(X, y, ls, jitters[0], jitters[1], kernel=family)
        _GPS[key] = (gp, gp.fantasies(S, seed=R.DRAW_SEED, delta=DELTA))
    return _GPS[key]


# ---- score_nei against the restatement ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(R.CASES))
def test_score_nei_matches_the_restatement(name):
    ref = R.case_reference(name)
    X, y, ls, Xs, Z, E, jitters, family, S = ref["problem"]
    gp, fan = _surrogate(name)
    r = gp.score_nei(fan, Xs, best=ref["best"], dense=True)
    want = ref["score"]
    mu, sigma, nei = r.mu.cpu().numpy(), r.sigma.cpu().numpy(), r.acq.cpu().numpy()
    fmax = max(1.0, float(np.abs(ref["fan"]["F"]).max()))
    keep, left_out = R.informative(want["nei"])
    d_mu, d_sigma = float(np.abs(mu - want["mu"]).max()), float(np.abs(sigma - want["sigma"]).max())
    d_nei = float(np.abs(nei - want["nei"])[keep].max())
    gap = R.top2_gap(want["nei"])
    print(f"{name}: |dmu| {d_mu:.2e} (bound {1e-9 * fmax:.2e}), |dsigma| {d_sigma:.2e}, |dNEI| {d_nei:.2e} over {int(keep.sum())} of "
          f"{keep.size} candidates (bound {1e-8 * fmax:.2e}), top-2 gap {gap:.2e}")
    assert mu.shape == (S, len(Xs)) and left_out <= R.MAX_LEFT_OUT
    assert d_mu <= 1e-9 * fmax
    assert d_sigma <= 1e-8
    assert d_nei <= 1e-8 * fmax
    assert r.nan_count == 0
    assert np.array_equal(r.fantasy_best.cpu().numpy(), ref["best"])
    if gap > 1e-7:
        assert r.best_idx == R.argmax_first(want["nei"])
    assert r.best_idx == R.argmax_first(nei) and r.best_val == nei[r.best_idx]      # the record is the dense output's own arg-max
    # dense=False gives the same record
    q = gp.score_nei(fan, Xs, best=ref["best"])
    assert (q.best_val, q.best_idx, q.nan_count) == (r.best_val, r.best_idx, 0) and q.acq is None and q.mu is None


# ---- fantasies against the restatement ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["n1_d1_s1_m8", "n127_d8_s64_m1000", "n128_d16_s16_m1537", "n129_d2_s17_m1537",
                                  "n300_d8_s64_m1537"])
def test_fantasies_match_the_restatement(name):
    ref = R.case_reference(name, longdouble=R.HAVE_LONGDOUBLE)
    X, y, ls, Xs, Z, E, jitters, family, S = ref["problem"]
    N = len(X)
    gp, fan = _surrogate(name)
    A, F, best = fan.A.cpu().numpy(), fan.F.cpu().numpy(), fan.best.cpu().numpy()
    want = ref["fan"]
    ymax = max(1.0, float(np.abs(y).max()))
    d_F, d_best = float(np.abs(F[:, :N] - want["F"]).max()), float(np.abs(best - want["best"]).max())
    print(f"{name}: |dF| {d_F:.2e}, |dbest| {d_best:.2e} (bound {1e-9 * ymax:.2e})")
    assert A.shape == F.shape == (S, gp.Np) and best.shape == (S,)
    assert d_F <= 1e-9 * ymax and d_best <= 1e-9 * ymax
    assert np.array_equal(best, F[:, :N].min(axis=1))                        # the minimum of the values it reports
    assert np.all(A[:, N:] == 0.0) and np.all(F[:, N:] == 0.0)               # the padding is exactly zero
    if R.HAVE_LONGDOUBLE:
        # A against the long-double form, relative to max |A|: within ten times the float64 restatement's own distance
        ld = ref["fan_ld"]["A"]
        amax = float(np.abs(ld).max())
        d_ref = float(np.abs(want["A"] - ld).max()) / amax
        d_dev = float(np.abs(A[:, :N] - ld).max()) / amax
        print(f"{name}: |dA| / max|A| device {d_dev:.2e}, restatement {d_ref:.2e} (max|A| {amax:.3g})")
        assert d_dev <= 10 * d_ref


@pytest.mark.parametrize("N", [5, 127, 129])
def test_the_incumbent_ignores_the_padding(N):
    """y > 0: every fantasy value is positive, so a padding zero would win the minimum."""
    X, y = gp_problem(12, N, 2, noise=0.3)
    y = y - y.min() + 5.0
    ls = np.array([0.3, 1.0])
    gp = DeviceGP(device=DEV).factorise(X, y, ls, 0.09, 0.0)
    fan = gp.fantasies(16, seed=1)
    F, best = fan.F.cpu().numpy(), fan.best.cpu().numpy()
    assert gp.Np > N and np.all(F[:, N:] == 0.0)
    assert np.all(best > 1.0) and np.array_equal(best, F[:, :N].min(axis=1))
    Z, E = nei_draws(N, 16, 1)
    want = R.fantasies(X, y, ls, Z, E, (0.09, 0.0))["best"]
    assert float(np.abs(best - want).max()) <= 1e-9 * float(np.abs(y).max())


# ---- bit properties ----------------------------------------------------------------------------------------------------------
def test_chunking_repetition_and_index_offset_do_not_change_a_bit():
    name = "n129_d2_s17_m1537"
    ref = R.case_reference(name)
    Xs = ref["problem"][3]
    (g512, f512), (g2048, f2048) = _surrogate(name, 512), _surrogate(name, 2048)
    assert torch.equal(f512.A, f2048.A) and torch.equal(f512.best, f2048.best)
    a = g512.score_nei(f512, Xs, best=ref["best"], dense=True)       # four chunks, the last one ragged
    b = g2048.score_nei(f2048, Xs, best=ref["best"], dense=True)     # one chunk
    for u, v in ((a.acq, b.acq), (a.mu, b.mu), (a.sigma, b.sigma)):
        assert np.array_equal(u.cpu().numpy(), v.cpu().numpy())
    assert (a.best_val, a.best_idx, a.nan_count) == (b.best_val, b.best_idx, b.nan_count)
    c = g512.score_nei(f512, Xs, best=ref["best"], dense=True)       # two calls: the same bits
    assert torch.equal(a.acq, c.acq) and torch.equal(a.mu, c.mu) and (a.best_val, a.best_idx) == (c.best_val, c.best_idx)
    o = g512.score_nei(f512, Xs, best=ref["best"], dense=True, idx_offset=OFFSET)
    assert torch.equal(a.acq, o.acq) and o.best_idx == a.best_idx + OFFSET and o.best_val == a.best_val
    # the fantasies themselves: two calls, the same bits
    again = g512.fantasies(f512.n_fantasies, seed=R.DRAW_SEED, delta=DELTA)
    assert torch.equal(again.A, f512.A) and torch.equal(again.F, f512.F) and torch.equal(again.best, f512.best)


# ---- special values ----------------------------------------------------------------------------------------------------------
def test_nan_candidates_and_exact_ties():
    name = "n40_d2_s16_m1537"
    ref = R.case_reference(name)
    Xs = ref["problem"][3]
    gp, fan = _surrogate(name, 512)
    base = gp.score_nei(fan, Xs, best=ref["best"], dense=True)
    i = base.best_idx
    # the best candidate with a NaN coordinate: counted once, never chosen, NaN in its own dense entries only
    Xn = Xs.copy()
    Xn[i, 1] = np.nan
    r = gp.score_nei(fan, Xn, best=ref["best"], dense=True)
    acq = r.acq.cpu().numpy()
    assert r.nan_count == 1 and r.best_idx != i and np.isnan(acq[i]) and np.isnan(r.mu.cpu().numpy()[:, i]).all()
    others = np.delete(np.arange(len(Xs)), i)
    assert np.array_equal(acq[others], base.acq.cpu().numpy()[others])
    assert r.best_idx == R.argmax_first(acq)
    # every candidate NaN: nothing to choose
    with pytest.raises(IndexError):
        gp.score_nei(fan, np.full((700, 2), np.nan), best=ref["best"])
    # an exact tie from duplicated rows resolves to the lower index, across workgroups and chunks
    for lo, hi in ((3, 1500), (300, 301), (i, 1536)):
        Xt = Xs.copy()
        Xt[lo] = Xs[i]
        Xt[hi] = Xs[i]
        t = gp.score_nei(fan, Xt, best=ref["best"], dense=True)
        ta = t.acq.cpu().numpy()
        assert ta[lo] == ta[hi] == base.best_val
        assert t.best_idx == min(lo, i) and t.nan_count == 0


# ---- rho = delta: plain EI ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("family", ["se", "matern52"])
def test_rho_equal_delta_is_plain_ei_with_the_smallest_observation(family):
    rho = 0.09
    X, y = gp_problem(2, 40, 2, noise=0.3)
    ls, Xs = np.array([0.3, 1.0]), R.candidates(2, 1537, 2)
    gp = DeviceGP(device=DEV, chunk=1024).factorise(X, y, ls, rho, 0.0, kernel=family)
    r = gp.select_nei(Xs, n_fantasies=17, seed=3, delta=rho, dense=True)
    F = gp.fantasies(17, seed=3, delta=rho).F.cpu().numpy()
    assert float(np.abs(F[:, :40] - y[None, :]).max()) <= 1e-9 * max(1.0, float(np.abs(y).max()))
    e = gp.score(Xs, acquisition="ei", f_best=float(y.min()), dense=True, prior_var=1.0 + rho)
    d = float(np.abs(r.acq.cpu().numpy() - e.acq.cpu().numpy()).max())
    print(f"{family}: |NEI - EI| {d:.2e}, largest EI {e.best_val:.3g}")
    assert e.best_val > R.INFORMATIVE
    assert d <= 1e-8
    assert r.best_idx == e.best_idx
    with pytest.raises(ValueError):
        gp.fantasies(16, delta=0.1)       # delta > rho


# ---- where the two incumbents disagree ---------------------------------------------------------------------------------------
def test_the_device_picks_the_restatements_candidate_where_nei_and_min_y_ei_differ():
    i_nei, i_ei, nei, ei, y, _ = nei_and_ei_choices()
    X, _ = gp_problem(2, 40, 2, noise=0.3)
    Xs = R.candidates(2, 1600, 2)
    gp = DeviceGP(device=DEV).factorise(X, y, np.array([0.3, 1.0]), 0.09, 0.0)
    r = gp.select_nei(Xs, n_fantasies=16, seed=0, dense=True)
    e = gp.score(Xs, acquisition="ei", f_best=float(y.min()), prior_var=1.09)
    assert i_nei != i_ei and r.best_idx == i_nei and e.best_idx == i_ei
    assert float(np.abs(r.acq.cpu().numpy() - nei).max()) <= 1e-8 * max(1.0, float(np.abs(y).max()))


# ---- the drop-in classes -----------------------------------------------------------------------------------------------------
FD = [40, 40]
AXES = [np.geomspace(0.05, 5.0, 16)] * 2
XI = 0.01
_RUNS = {}


def _data():
    X, y = gp_problem(2, 40, 2, noise=0.3)
    g = (np.arange(40) + 0.5) / 40
    return X, y, np.stack(np.meshgrid(g, g, indexing="ij"), -1).reshape(-1, 2)


def _run(cls, scaled=False, **kw):
    """One updated selector per (class, options, scaling of y) with its NEI choice, shared by the tests below."""
    key = (cls.__name__, scaled, tuple(sorted(kw.items())))
    if key not in _RUNS:
        X, y, Xs = _data()
        ps = cls(**kw)
        ps.name, ps.iteration = "T", 0
        ps.measured_pts, ps.measured_vals = X, 40.0 + 7.0 * y if scaled else y
        ps.feature_domain, ps.predicted_pts, ps.length_scales = FD, Xs, AXES
        ps.update_surrogate()
        idx = ps.noisy_expected_improvement(n_fantasies=16, seed=0, xi=XI * (7.0 if scaled else 1.0))   # (xi is a value of y)
        _RUNS[key] = (ps, idx, ps.acq_func_eval.copy(), ps.fantasy_best.copy())
    return _RUNS[key]


def _restated(ps, y, xi):
    """(NEI in the units of y [M], the incumbents in the units of y [S], |F|_inf in the units of the model) of the
    restatement for the model a selector holds."""
    X, _, Xs = _data()
    m = ps._model
    ls = np.asarray(ps.kernel_params, dtype=np.float64).reshape(-1)
    Z, E = nei_draws(len(X), 16, 0)
    fan = R.fantasies(X, (y - m.y_mean) / m.y_scale, ls, Z, E, (m.jitter1, m.jitter2), DELTA, m.kernel)
    sc = R.score(X, Xs, ls, fan, None, xi / m.y_scale, DELTA, m.kernel)
    return m.y_scale * sc["nei"], m.y_mean + m.y_scale * fan["best"], max(1.0, float(np.abs(fan["F"]).max()))


@pytest.mark.parametrize("cls,kw", [(PointSelector, dict(ard="hyper")), (PointSelector, {}), (PointSelectorHost, dict(ard="hyper")),
                                    (PointSelector, dict(ard="hyper", kernel="matern52")), (PointSelector, dict(ard="gradient"))])
def test_the_selector_classes_report_the_restatements_nei(cls, kw):
    _, y, _ = _data()
    ps, idx, acq, fbest = _run(cls, **kw)
    want, want_best, fmax = _restated(ps, y, XI)
    s = ps._model.y_scale
    d_acq, d_best = float(np.abs(acq.ravel() - want).max()), float(np.abs(fbest - want_best).max())
    gap = R.top2_gap(want)
    print(f"{cls.__name__} {kw}: |dNEI| {d_acq:.2e} (bound {1e-8 * fmax * s:.2e}), |dbest| {d_best:.2e}, top-2 gap {gap:.2e}, largest "
          f"{want.max():.3g}, rho {ps._model.jitter1 + ps._model.jitter2:.3g}")
    assert acq.shape == tuple(FD) and fbest.shape == (16,) and want.max() > R.INFORMATIVE
    assert d_acq <= 1e-8 * fmax * s and d_best <= 1e-9 * fmax * s
    assert gap > 1e-7 * s, "the restatement does not decide this case"
    assert int(np.ravel_multi_index(tuple(idx), FD)) == R.argmax_first(want)
    # a second call is served from the cache; another seed is another acquisition
    assert np.array_equal(ps.noisy_expected_improvement(n_fantasies=16, seed=0, xi=XI), idx)
    assert np.array_equal(ps.acq_func_eval, acq)
    ps.noisy_expected_improvement(n_fantasies=16, seed=1, xi=XI)
    assert not np.array_equal(ps.acq_func_eval, acq)
    ps.noisy_expected_improvement(n_fantasies=16, seed=0, xi=XI)   # (leave the shared selector as it was found)


def test_the_selection_does_not_depend_on_the_units_of_y():
    a, ia, acq_a, best_a = _run(PointSelector, ard="hyper")
    b, ib, acq_b, best_b = _run(PointSelector, scaled=True, ard="hyper")
    d_acq = float(np.abs(acq_b - 7.0 * acq_a).max() / np.abs(acq_b).max())
    d_best = float(np.abs(best_b - (40.0 + 7.0 * best_a)).max() / np.abs(best_b).max())
    print(f"y -> 40 + 7 y: |acq' - 7 acq| / max {d_acq:.2e}, |best' - (40 + 7 best)| / max {d_best:.2e}; rho {a.noise:.6g} / "
          f"{b.noise:.6g}")
    assert np.array_equal(ia, ib)
    assert d_acq <= 1e-9
    assert d_best <= 1e-9


def test_host_and_device_classes_agree():
    ps, idx, acq, fbest = _run(PointSelector, ard="hyper")
    ph, idh, acq_h, fbest_h = _run(PointSelectorHost, ard="hyper")
    assert np.array_equal(idx, idh)
    np.testing.assert_allclose(acq_h, acq, rtol=0, atol=1e-9 * float(np.abs(acq).max()))
    np.testing.assert_allclose(fbest_h, fbest, rtol=0, atol=1e-9 * float(np.abs(fbest).max()))
    # the other acquisitions of both classes are untouched by the call
    assert np.array_equal(ph.expected_improvement(), ps.expected_improvement())


def test_host_binding_returns_the_device_path_bit_for_bit_on_one_model():
    name = "n129_d2_s17_m1537"
    ref = R.case_reference(name)
    X, y, ls, Xs, Z, E, jitters, family, S = ref["problem"]
    gp, fan = _surrogate(name, 512)
    r = gp.score_nei(fan, Xs, best=ref["best"], dense=True)
    h = H.select_nei(X, y, ls, Xs, S, R.DRAW_SEED, best=ref["best"], dense_means=True, chunk=512, jitter1=jitters[0],
                     jitter2=jitters[1])
    assert h["info"] == 0 and (h["best_val"], h["best_idx"], h["nan_count"]) == (r.best_val, r.best_idx, 0)
    assert np.array_equal(h["acq"], r.acq.cpu().numpy()) and np.array_equal(h["mu"], r.mu.cpu().numpy())
    assert np.array_equal(h["sigma"], r.sigma.cpu().numpy()) and np.array_equal(h["fantasy_best"], ref["best"])
    h2 = H.select_nei(X, y, ls, Xs, S, R.DRAW_SEED, jitter1=jitters[0], jitter2=jitters[1])
    assert np.array_equal(h2["fantasy_best"], fan.best.cpu().numpy())


def test_stale_fantasies_are_refused():
    X, y = gp_problem(2, 40, 2, noise=0.3)
    ls, Xs = np.array([0.3, 1.0]), R.candidates(2, 100, 2)
    gp = DeviceGP(device=DEV).factorise(X, y, ls, 0.09, 0.0)
    fan = gp.fantasies(4)
    gp.score_nei(fan, Xs)
    gp.factorise(X, y, ls, 0.09, 0.0)
    with pytest.raises(ValueError, match="fantasies"):
        gp.score_nei(fan, Xs)
    with pytest.raises(ValueError, match="order"):
        DeviceGP(device=DEV).factorise(*gp_problem(3, 300, 2), ls, 0.09, 0.0, order="fps").fantasies(4)
