"""Max-value entropy search on the GPU (csrc/mes.hip; DeviceGP.log_survival / mes_on_posterior / select_mes,
PointSelector.max_value_entropy_search, PointSelectorHost.max_value_entropy_search, the two host entries) against tests/mes_ref.py,
the NumPy / SciPy restatement, whose own accuracy tests/test_mes_ref_cpu.py pins against 60-digit values.
Bounds: log S within 64 eps sum_c |log Phi(gamma_c)| per level (a few ulps per term, about 22 adds in the fixed tree); MES within
8 eps (max(1, gamma^2 / 2 for gamma < 0) + |h|), the maximum over the S terms of a candidate.
Sizes: M = 1, 255 (one partial workgroup), 257 (two), 262,145 (more than 1024 workgroups: the grid-stride loop runs)."""
import numpy as np
import pytest
import torch  # noqa: F401  (before the host-pointer binding initialises HIP)

pytestmark = pytest.mark.gpu

import mes_ref as R  # noqa: E402
from ard_fit_ref import gp_problem  # noqa: E402
from bayesian_optimisation_amd import DeviceGP, PointSelector, PointSelectorHost  # noqa: E402
from bayesian_optimisation_amd import host_binding as H  # noqa: E402

DEV = "cuda:0"
EPS = np.finfo(np.float64).eps
SIZES = [1, 255, 257, 262145]
OFFSET = 10 ** 9 + 7
_GP, _SURV, _ACQ = [], {}, {}


def _gp():
    if not _GP:
        _GP.append(DeviceGP(device=DEV))   # both kernels work on dense arrays: no factorisation
    return _GP[0]


# ---- the log-survival kernel -------------------------------------------------------------------------------------------------
def _survival_case(M):
    """(mu, sigma, 64 levels, log S, its error unit, the NaN count) once per size: gamma over [-40, 40] (sigma >= 0.1, means and
    levels in [-2, 2]); from 9 candidates on two point masses (sigma = 0) at 1.2 and 1.6 - the levels below 1.2 have both on
    the right side, the others are -inf - and two NaN candidates."""
    if M not in _SURV:
        rng = np.random.default_rng(M)
        mu, sigma = rng.uniform(-2.0, 2.0, M), np.exp(rng.uniform(np.log(0.1), np.log(2.0), M))
        if M == 1:
            # ONE term is held to 64 eps |log Phi| itself, which no plain fp64 form meets for gamma above about 8 (log Phi ~ -erfc / 2
            # moves by gamma^2 / 2 eps with the rounding of its argument): a wide candidate, |gamma| <= 2.5 at every level
            sigma[0] = 1.75
        if M > 8:
            sigma[[3, 7]], mu[[3, 7]] = 0.0, [1.6, 1.2]
            mu[5], sigma[M - 1] = np.nan, np.nan
        z = np.linspace(-2.0, 2.0, 64)
        z[10] = 1.2                                    # a level ON a point mass: mu > z is false there
        want, n = R.log_survival(mu, sigma, z)
        _SURV[M] = (mu, sigma, z, want, R.log_survival_scale(mu, sigma, z), n)
    return _SURV[M]


@pytest.mark.parametrize("Q", [1, 63, 64])
@pytest.mark.parametrize("M", SIZES)
def test_log_survival_matches_the_restatement(M, Q):
    mu, sigma, z, want, unit, n_nan = _survival_case(M)
    gp = _gp()
    mud, sgd = gp._dev(mu), gp._dev(sigma)
    got, n = gp.log_survival(mud, sgd, z[:Q])
    fin = np.isfinite(want[:Q])
    worst = float(np.max(np.abs(got[fin] - want[:Q][fin]) / (EPS * unit[:Q][fin]))) if fin.any() else 0.0
    print(f"M = {M}, Q = {Q}: worst |dlog S| = {worst:.2f} units of eps sum|log Phi| (bound 64), {int((~fin).sum())} levels -inf, "
          f"{n} NaN candidates")
    assert got.shape == (Q,) and n == n_nan == (2 if M > 8 else 0)
    assert np.array_equal(np.isfinite(got), fin) and np.all(got[~fin] == -np.inf)
    if M > 8:
        assert fin[0] and (Q == 1 or not fin[10])               # below both point masses finite, on / above one of them -inf
    assert worst <= 64.0
    # the same bits from a second call and from a call on another stream
    again, n2 = gp.log_survival(mud, sgd, z[:Q])
    assert again.tobytes() == got.tobytes() and n2 == n
    side = torch.cuda.Stream(device=DEV)
    side.wait_stream(torch.cuda.current_stream(DEV))
    with torch.cuda.stream(side):
        other, n3 = gp.log_survival(mud, sgd, z[:Q])
    torch.cuda.current_stream(DEV).wait_stream(side)
    assert other.tobytes() == got.tobytes() and n3 == n


def test_log_survival_on_host_arrays_is_the_device_path():
    mu, sigma, z, want, unit, n_nan = _survival_case(257)
    got, n = H.mes_log_survival(mu, sigma, z[:63])
    dev, nd = _gp().log_survival(mu, sigma, z[:63])
    assert got.tobytes() == dev.tobytes() and n == nd == n_nan


# ---- the acquisition kernel --------------------------------------------------------------------------------------------------
def _acq_case(M):
    """(mu, sigma, 64 samples, h of every (candidate, sample) [M x 64], its error unit [M x 64]) once per size.  Means and
    samples in [-2, 2], sigma >= 0.1: gamma covers [-40, 40], all three branches of the term (about a tenth of the pairs in
    [-1, 0], a third below -1).  From 17 candidates on: candidates ON the branch points for sample 0 (gamma = 0, its two
    neighbours, and -1 with its two neighbours); a planted winner (the lowest mean by far: gamma ~ -150, h ~ 5.5 against at most
    4.2 at gamma = -40) at index M // 2 and its exact copy at M // 2 + 3 - two equal winners -, a candidate with sigma = 0 and
    two NaN candidates.  M = 1: one candidate in the middle of the samples, so that its 64 terms take all three branches."""
    if M not in _ACQ:
        rng = np.random.default_rng(1000 + M)
        mu, sigma = rng.uniform(-2.0, 2.0, M), np.exp(rng.uniform(np.log(0.1), np.log(2.0), M))
        ys = rng.uniform(-2.0, 2.0, 64)
        ys[0] = 0.25                                           # (S = 1 uses this one alone: means on both sides of it)
        if M == 1:
            mu[0], sigma[0] = float(np.median(ys)), 0.5
        if M > 16:
            w = M // 2
            mu[[w, w + 3]], sigma[[w, w + 3]] = -30.0, 0.2
            sigma[1] = 0.0
            mu[2], sigma[M - 2] = np.nan, np.nan
            sigma[8:14] = 1.0                                  # gamma for sample 0 is mu - ys[0] exactly
            mu[8:11] = ys[0], np.nextafter(ys[0], 3.0), np.nextafter(ys[0], -3.0)
            mu[11:14] = ys[0] - 1.0, np.nextafter(ys[0] - 1.0, 3.0), np.nextafter(ys[0] - 1.0, -3.0)
        with np.errstate(all="ignore"):
            g = (mu[:, None] - ys[None, :]) / np.where(sigma == 0.0, 1.0, sigma)[:, None]
        _ACQ[M] = (mu, sigma, ys, R.h(g), R.h_scale(g), g)
    return _ACQ[M]


def _acq_reference(M, S):
    mu, sigma, ys, hh, unit, _ = _acq_case(M)
    want = np.sum(hh[:, :S], axis=1) / S
    want = np.where(sigma == 0.0, 0.0, want)
    want[np.isnan(mu) | np.isnan(sigma)] = np.nan
    return want, np.max(unit[:, :S], axis=1)


def _undecided(want, unit):
    """The restatement's top-two gap does not exceed the tolerance of the two values: the index is not compared."""
    ok = ~np.isnan(want)
    v = np.sort(np.unique(want[ok]))
    if v.size < 2:
        return False
    top = np.flatnonzero(ok & (want >= v[-2]))
    return bool(v[-1] - v[-2] <= 2 * 8.0 * EPS * np.max(unit[top]))


@pytest.mark.parametrize("S", [1, 16, 64])
@pytest.mark.parametrize("M", SIZES)
def test_acquisition_matches_the_restatement(M, S):
    mu, sigma, ys, _, _, g = _acq_case(M)
    want, unit = _acq_reference(M, S)
    gp = _gp()
    mud, sgd = gp._dev(mu), gp._dev(sigma)
    r = gp.mes_on_posterior(mud, sgd, ys[:S], idx_offset=OFFSET)
    acq = r.acq.cpu().numpy()
    ok = ~np.isnan(want)
    worst = float(np.max(np.abs(acq[ok] - want[ok]) / (EPS * unit[ok])))
    gs = g[ok][:, :S]
    mid, low = (gs >= -1.0) & (gs <= 0.0), gs < -1.0
    # per branch: the candidates ALL of whose S terms take it (no term of another branch hides an error of this one)
    pure = {name: np.flatnonzero(np.all(m, axis=1)) for name, m in (("high", gs > 0.0), ("mid", mid), ("low", low))}
    per = {k: (float(np.max(np.abs(acq[ok][v] - want[ok][v]) / (EPS * unit[ok][v]))) if v.size else None) for k, v in pure.items()}
    print(f"M = {M}, S = {S}: worst |dMES| = {worst:.2f} units of eps (max(1, gamma^2/2) + |h|) (bound 8); largest {np.nanmax(want):.4g}; "
          f"pairs in [-1, 0]: {int(mid.sum())}, below -1: {int(low.sum())} of {gs.size}; candidates with every term in one branch "
          f"(worst units): " + ", ".join(f"{k} {v.size} ({per[k] if per[k] is None else round(per[k], 2)})" for k, v in pure.items()))
    if M > 16:
        assert mid.sum() >= gs.size // 20 and low.sum() >= gs.size // 5      # the middle and the low branch are really run
    assert np.array_equal(np.isnan(acq), ~ok) and r.nan_count == int((~ok).sum()) == (2 if M > 16 else 0)
    assert worst <= 8.0
    assert np.all(acq[ok] >= 0.0) and np.array_equal(r.y_star, ys[:S])
    if M > 16:
        assert acq[1] == 0.0                                                        # sigma = 0
        assert acq[M // 2] == acq[M // 2 + 3]                                       # two equal winners: the lower index
    first, _ = R.first_argmax(acq)
    assert r.best_idx == OFFSET + first and r.best_val == acq[first]                # the record is the dense output's own arg-max
    if not _undecided(want, unit):
        assert first == R.first_argmax(want)[0] == (M // 2 if M > 16 else 0)
    # the repeat is bit-equal; without the dense store the same record; another offset moves the index only
    q = gp.mes_on_posterior(mud, sgd, ys[:S], idx_offset=OFFSET)
    assert q.acq.cpu().numpy().tobytes() == acq.tobytes() and (q.best_val, q.best_idx, q.nan_count) == (r.best_val, r.best_idx, r.nan_count)
    p = gp.mes_on_posterior(mud, sgd, ys[:S], idx_offset=5, dense=False)
    assert p.acq is None and (p.best_val, p.best_idx, p.nan_count) == (r.best_val, 5 + first, r.nan_count)


def test_a_unique_winner_is_found_and_all_nan_leaves_none():
    mu, sigma, ys = _acq_case(257)[:3]
    mu, sigma = mu.copy(), sigma.copy()
    mu[200], sigma[200] = -60.0, 0.2                                                 # below the two planted copies
    gp = _gp()
    r = gp.mes_on_posterior(mu, sigma, ys[:16])
    assert r.best_idx == 200 == R.first_argmax(R.acquisition(mu, sigma, ys[:16])[0])[0]
    e = gp.mes_on_posterior(np.full(300, np.nan), sigma[:1].repeat(300), ys[:16], idx_offset=7)
    assert e.nan_count == 300 and not 7 <= e.best_idx < 307
    hst = H.mes_acq(mu, sigma, ys[:16])
    assert hst["best_idx"] == 200 and hst["acq"].tobytes() == r.acq.cpu().numpy().tobytes() and hst["nan_count"] == r.nan_count


def test_at_most_one_case_in_twenty_is_left_undecided():
    cases = [(M, S) for M in SIZES for S in (1, 16, 64)]
    left = sum(_undecided(*_acq_reference(M, S)) for M, S in cases)
    assert 20 * left <= len(cases), (left, len(cases))


# ---- end to end ----------------------------------------------------------------------------------------------------------------
FD = [50, 50]
AXES = [np.geomspace(0.05, 5.0, 16)] * 2
_E2E, _RUNS = {}, {}


def _data():
    X, y = gp_problem(2, 40, 2, noise=0.3)
    g = (np.arange(50) + 0.5) / 50
    return X, y, np.stack(np.meshgrid(g, g, indexing="ij"), -1).reshape(-1, 2)


def _selector(cls, **kw):
    key = (cls.__name__, tuple(sorted(kw.items())))
    if key not in _RUNS:
        X, y, Xs = _data()
        ps = cls(**kw)
        ps.name, ps.iteration = "T", 0
        ps.measured_pts, ps.measured_vals = X, 40.0 + 7.0 * y
        ps.feature_domain, ps.predicted_pts, ps.length_scales = FD, Xs, AXES
        ps.update_surrogate()
        _RUNS[key] = ps
    return _RUNS[key]


def _surrogate(case):
    """(DeviceGP, candidates on the device, prior variance, min(y) in the units of the model): the frozen record with each
    family, or the record ard="hyper" has fitted."""
    if case not in _E2E:
        X, y, Xs = _data()
        if case == "hyper":
            ps = _selector(PointSelector, ard="hyper")
            m = ps._model
            _E2E[case] = (ps._gp, ps._cand[0], m.prior_var, float(np.min(m.to_model(np.asarray(ps.measured_vals)))))
        else:
            gp = DeviceGP(device=DEV).factorise(X, y, [0.3, 0.5], kernel=case)
            _E2E[case] = (gp, gp._dev(Xs), None, float(y.min()))
    return _E2E[case]


def _close(a, b, width):
    return float(np.max(np.abs(np.asarray(a) - np.asarray(b)))) <= 1e-9 * width


@pytest.mark.parametrize("case", ["se", "matern32", "matern52", "hyper"])
def test_select_mes_is_the_restatement_on_the_pass_own_posterior(case):
    gp, Xsd, pv, ymin = _surrogate(case)
    r = gp.select_mes(Xsd, n_samples=16, seed=3, dense=True, prior_var=pv)
    mu, sigma = r.mu.cpu().numpy(), r.sigma.cpu().numpy()
    idx, acq, m, q = R.select(mu, sigma, 16, 3, cap=ymin)
    lo, hi = R.brackets(mu, sigma)
    _, unit = R.acquisition(mu, sigma, m)
    print(f"{case}: quartiles {r.quartiles} (restated {q}), brackets [{lo:.4g}, {hi:.4g}], min(y) {ymin:.4g}, samples in "
          f"[{r.y_star.min():.4g}, {r.y_star.max():.4g}], index {r.best_idx} (restated {idx})")
    assert q[0] < q[1] < q[2] and mu.shape == (2500,) and r.nan_count == 0
    assert _close(r.quartiles, q, hi - lo) and _close(r.y_star, m, hi - lo)
    assert np.all(r.y_star <= ymin)
    assert not _undecided(acq, unit), "the restatement does not decide this case"
    assert r.best_idx == idx and r.best_val == float(r.acq[idx].item())
    # a y_star array is used verbatim; no cap: the free samples
    given = np.linspace(ymin - 1.0, ymin, 5)
    v = gp.select_mes(Xsd, n_samples=5, y_star=given, dense=True, prior_var=pv)
    assert np.array_equal(v.y_star, given) and v.quartiles is None
    assert v.best_idx == R.first_argmax(R.acquisition(mu, sigma, given)[0])[0]
    free = gp.select_mes(Xsd, n_samples=16, seed=3, cap=None, prior_var=pv)
    assert _close(free.y_star, R.gumbel_samples(q, R.uniforms(16, 3)), hi - lo) and free.acq is None


def test_thompson_samples_are_the_minima_of_the_paths():
    gp, Xsd, pv, _ = _surrogate("se")
    r = gp.select_mes(Xsd, n_samples=8, seed=11, y_star="thompson", dense=True)
    ts = gp.thompson_score(gp.thompson_paths(8, seed=11), Xsd)
    assert np.array_equal(r.y_star, -ts.values) and r.quartiles is None
    want, _ = R.acquisition(r.mu.cpu().numpy(), r.sigma.cpu().numpy(), -ts.values)
    assert r.best_idx == R.first_argmax(want)[0]
    with pytest.raises(ValueError, match="kernel='se' only"):
        _surrogate("matern52")[0].select_mes(_surrogate("matern52")[1], y_star="thompson")


# ---- through the selector classes ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kw", [dict(ard="hyper"), {}, dict(ard="hyper", kernel="matern52")], ids=["hyper", "frozen", "hyper-matern52"])
def test_the_selector_class_reports_the_restatements_choice(kw, monkeypatch):
    ps = _selector(PointSelector, **kw)
    idx = ps.max_value_entropy_search(n_samples=16, seed=0)
    acq, minima = ps.acq_func_eval.copy(), ps.sampled_minima.copy()
    mu, sigma = ps._mu_dev.cpu().numpy(), ps._sigma_dev.cpu().numpy()       # in the units of the model
    m = ps._model
    ymin = float(np.min(m.to_model(np.asarray(ps.measured_vals, dtype=np.float64))))
    want_idx, want, samples, q = R.select(mu, sigma, 16, 0, cap=ymin)
    lo, hi = R.brackets(mu, sigma)
    _, unit = R.acquisition(mu, sigma, samples)
    assert acq.shape == tuple(FD) and minima.shape == (16,)
    assert np.array_equal(idx, np.unravel_index(int(np.argmax(acq)), FD))
    assert _close(minima, m.mean_to_y(samples), (hi - lo) * m.y_scale)
    assert np.all(minima <= np.min(ps.measured_vals) + 1e-9 * (hi - lo) * m.y_scale)
    assert not _undecided(want, unit) and int(np.ravel_multi_index(tuple(idx), FD)) == want_idx
    # a second call is served from the cache: no kernel runs
    monkeypatch.setattr(ps._gp, "mes_on_posterior", None)
    monkeypatch.setattr(ps._gp, "log_survival", None)
    assert np.array_equal(ps.max_value_entropy_search(n_samples=16, seed=0), idx) and np.array_equal(ps.acq_func_eval, acq)
    monkeypatch.undo()
    ps.max_value_entropy_search(n_samples=16, seed=1)
    assert not np.array_equal(ps.sampled_minima, minima)
    # the lower confidence bound of the update is still served as it was
    assert ps.lower_confidence_bound().shape == (2,)


def test_host_and_device_classes_agree():
    ps, ph = _selector(PointSelector, ard="hyper"), _selector(PointSelectorHost, ard="hyper")
    idx = ps.max_value_entropy_search(n_samples=16, seed=0)
    acq, minima = ps.acq_func_eval.copy(), ps.sampled_minima.copy()
    idh = ph.max_value_entropy_search(n_samples=16, seed=0)
    mu, sigma = ps._mu_dev.cpu().numpy(), ps._sigma_dev.cpu().numpy()
    m = ps._model
    _, unit = R.acquisition(mu, sigma, (minima - m.y_mean) / m.y_scale)
    worst = float(np.max(np.abs(ph.acq_func_eval.ravel() - acq.ravel()) / (EPS * unit)))
    lo, hi = R.brackets(mu, sigma)
    print(f"host against device: worst |dMES| {worst:.2f} units of eps (max(1, gamma^2/2) + |h|) (bound 8)")
    assert np.array_equal(idh, idx)
    assert _close(ph.sampled_minima, minima, (hi - lo) * m.y_scale)
    assert worst <= 8.0


def test_nan_in_the_posterior_raises_the_reference_error():
    ps = _selector(PointSelector)
    keep = ps._mu_dev
    try:
        ps._mu_dev = keep.clone()
        ps._mu_dev[17] = float("nan")
        with pytest.raises(IndexError, match="NaN"):
            ps.max_value_entropy_search(n_samples=4, seed=99)
    finally:
        ps._mu_dev = keep
