"""Acquisition gradients and off-grid refinement on the GPU (csrc/refine.hip; DeviceGP.posterior_grad / refine /
select_refined, PointSelector.refine_next, PointSelectorHost.refine_next) against tests/refine_ref.py, the NumPy restatement
on the Cholesky route (the reference project has no such step), and against the library's own score().

Tolerances are the project's fp64 ones: |dmu| <= 1e-9 max(1, |y|_inf), |dsigma| <= 1e-8, |dacq| <= 1e-8 max(1, |y|_inf);
a gradient entry gets the same figure divided by ls_k (d k_n / d x_k = k_n g_nk with |k_n g_nk| <= e^-1/2 / ls_k).
Trajectories (12 iterations, decided points only): identical `accepted`, |dx_k| / ls_k <= 1e-4, |dacq| <= 1e-5 - 10x and
3x what errors of the full value / gradient tolerances, injected into every evaluation of the NumPy rule, moved it.

Every test prints its measured maxima before it asserts."""
import functools

import numpy as np
import pytest
import torch  # noqa: F401  (before the host-pointer binding initialises HIP)

pytestmark = pytest.mark.gpu

import refine_ref as R  # noqa: E402
from bayesian_optimisation_amd import DeviceGP, PointSelector, PointSelectorHost  # noqa: E402
from bayesian_optimisation_amd.synthetic import make_problem  # noqa: E402

GRAD_SHAPES = [(1, 1), (2, 3), (63, 2), (64, 2), (65, 5), (128, 8), (129, 3), (300, 8), (700, 8), (512, 16)]
GRAD_P = [1, 63, 64, 65, 200]


@functools.lru_cache(maxsize=None)
def _problem(N, M, d):
    X, y, Xs, ls = make_problem(max(N, 8), M, d)   # (y of fewer than 8 rows: a slice, the generator scales by the sample's spread)
    return X[:N], y[:N], Xs, ls


@functools.lru_cache(maxsize=None)
def _model(N, M, d):
    X, y, _, ls = _problem(N, M, d)
    return R.Model(X, y, ls)


@functools.lru_cache(maxsize=None)
def _gp(N, M, d):
    X, y, _, ls = _problem(N, M, d)
    return DeviceGP(device="cuda:0").factorise(X, y, ls)


def _np(t):
    return t.cpu().numpy()


# ---- 1. gradients against refine_ref ---------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _grad_case(N, d, name):
    """(the 200 query points, refine_ref's values and gradients there, the acquisition keywords)."""
    X, y, Xs, ls = _problem(N, 256, d)
    Q = Xs[:200].copy()
    Q[0] = X[0]                    # an observation itself: k = 1 exactly
    Q[1] = np.ones(d)              # a corner of the box
    Q[2] = X[0] + 50.0 * ls        # 50 length scales away: mu = 0, sigma = sqrt(prior), no gradient
    kw = R.acq_kw(name, y)
    return Q, _model(N, 256, d).grad(Q, **kw), kw


@pytest.mark.parametrize("name", R.ACQS)
@pytest.mark.parametrize("P", GRAD_P)
@pytest.mark.parametrize("N,d", GRAD_SHAPES)
def test_gradients_match_the_numpy_restatement(N, d, P, name):
    X, y, Xs, ls = _problem(N, 256, d)
    Q, ref, kw = _grad_case(N, d, name)
    g = _gp(N, 256, d).posterior_grad(Q[:P], **kw)
    ymax = max(1.0, float(np.abs(y).max()))
    tmu, tsig = 1e-9 * ymax, 1e-8
    tdacq = (kw["explore"] * tsig + tmu) if name == "lcb" else (tsig + tmu)
    err = {k: np.abs(_np(getattr(g, k)) - ref[k][:P]) for k in ("mu", "sigma", "acq", "dmu", "dsigma", "dacq")}
    print(f"N={N} d={d} P={P} {name}: " + " ".join(
        f"{k} {(v * (ls[None, :] if v.ndim == 2 else 1.0)).max():.3g}" for k, v in err.items()) + "  (gradients times ls)")
    assert err["mu"].max() <= tmu and err["sigma"].max() <= tsig and err["acq"].max() <= 1e-8 * ymax
    assert np.all(err["dmu"] <= tmu / ls[None, :])
    assert np.all(err["dsigma"] <= tsig / ls[None, :])
    assert np.all(err["dacq"] <= tdacq / ls[None, :])
    if P >= 3:   # the far point: the prior itself
        assert _np(g.mu)[2] == 0.0 and _np(g.sigma)[2] == np.sqrt(R.KAPPA)
        assert not np.any(_np(g.dmu)[2]) and not np.any(_np(g.dsigma)[2]) and not np.any(_np(g.dacq)[2])


@pytest.mark.parametrize("d", [1, 3, 8])
def test_a_point_on_the_observation_has_k_of_exactly_one(d):
    """N = 1 with the query on the observation: the kernel entry is exp(-0) = 1 in the difference form (the expanded-distance
    form leaves a rounding residue under the exponential), every other term of the sum is a zero of the padding, so mu is
    alpha_0 bit for bit; and the gradient of mu, alpha_0 k_0 g_0k with g_0k = 0, is exactly zero."""
    X, y, _, ls = _problem(1, 256, d)
    gp = _gp(1, 256, d)
    g = gp.posterior_grad(X[:1].copy())
    assert _np(g.mu)[0] == _np(gp.alpha)[0] != 0.0
    assert not np.any(_np(g.dmu)[0])


# ---- 2. trajectories: the six cases of the issue, 64 starts, 12 iterations, decided points only ---------------------------------
@functools.lru_cache(maxsize=None)
def _trajectory(N, M, d, name):
    X, y, Xs, ls = _problem(N, M, d)
    kw = R.acq_kw(name, y)
    m = _model(N, M, d)
    _, S, _ = R.starts(X, y, Xs, ls, model=m, **kw)
    ref = R.refine(X, y, ls, S, 0.0, 1.0, iters=R.TRAJ_ITERS, model=m, **kw)
    return S, ref, R.decided(ref), kw


def _check_trajectory(r, ref, mask, ls, what):
    x, acq, accepted = _np(r.x), _np(r.acq), _np(r.accepted)
    dx = np.abs(x - ref["x"]) / ls[None, :]
    da = np.abs(acq - ref["acq"])
    same = accepted == ref["accepted"]
    print(f"{what}: {int(mask.sum())} decided (smallest margin {ref['margin'][mask].min():.3g}), accepted {accepted.min()}.."
          f"{accepted.max()}, identical on {int(same[mask].sum())}; |dx|/ls {dx[mask].max():.3g}, |dacq| {da[mask].max():.3g}")
    assert np.all(same[mask])
    assert dx[mask].max() <= 1e-4
    assert da[mask].max() <= 1e-5


@pytest.mark.parametrize("name", R.ACQS)
@pytest.mark.parametrize("N,M,d", R.CASES)
def test_trajectories_match_the_numpy_rule(N, M, d, name):
    _, _, _, ls = _problem(N, M, d)
    S, ref, mask, kw = _trajectory(N, M, d, name)
    r = _gp(N, M, d).refine(S, 0.0, 1.0, iters=R.TRAJ_ITERS, **kw)
    assert r.nan_count == 0 and r.best == ref["best"]
    assert abs(r.best_val - ref["acq"].max()) <= 1e-5
    _check_trajectory(r, ref, mask, ls, f"N={N} d={d} {name}")


# ---- 3. properties at the default 30 iterations ------------------------------------------------------------------------------
@pytest.mark.parametrize("name", R.ACQS)
@pytest.mark.parametrize("N,M,d", [(64, 2048, 2), (129, 1024, 3), (300, 4096, 8)])
def test_properties_at_thirty_iterations(N, M, d, name):
    X, y, Xs, ls = _problem(N, M, d)
    kw = R.acq_kw(name, y)
    gp = _gp(N, M, d)
    r = gp.select_refined(Xs, n_starts=64, **kw)
    lo, hi = Xs.min(axis=0), Xs.max(axis=0)
    x, acq, acq0 = _np(r.x), _np(r.acq), _np(r.acq0)
    assert np.all((x >= lo[None, :]) & (x <= hi[None, :]))
    assert np.all(acq >= acq0)
    grid = gp.score(Xs, dense=True, **kw)
    ga = _np(grid.acq)
    order = np.argsort(-ga, kind="stable")[:64]
    tol = 1e-8 * max(1.0, float(np.abs(y).max()))
    at_x = _np(gp.score(x, dense=True, **kw).acq)
    print(f"N={N} d={d} {name}: grid best {grid.best_val:.6g} -> refined best {r.best_val:.6g}; |acq0 - score| "
          f"{np.abs(acq0 - ga[order]).max():.3g}, |acq - score(x)| {np.abs(acq - at_x).max():.3g}, pg {_np(r.pg).min():.2g} .. "
          f"{_np(r.pg).max():.2g}, accepted {_np(r.accepted).min()}..{_np(r.accepted).max()}")
    assert np.abs(acq0 - ga[order]).max() <= tol      # the new kernels against the existing ones, at the starts ...
    assert np.abs(acq - at_x).max() <= tol            # ... and at the refined points
    assert r.best == int(np.flatnonzero(acq == acq.max())[0]) and r.best_val == acq.max() and r.nan_count == 0
    assert (r.grid_idx, r.grid_val) == (grid.best_idx, grid.best_val) and r.grid_idx == order[0]
    assert r.best_val >= r.grid_val


# ---- 4. same bits; other factorisations of the same observation set ---------------------------------------------------------------
def test_two_calls_give_the_same_bits_and_other_factorisations_agree():
    N, M, d, name = 300, 4096, 8, "lcb"
    X, y, Xs, ls = _problem(N, M, d)
    S, ref, mask, kw = _trajectory(N, M, d, name)
    gp = _gp(N, M, d)
    a, b = gp.refine(S, 0.0, 1.0, iters=30, **kw), gp.refine(S, 0.0, 1.0, iters=30, **kw)
    for k in ("x", "acq", "acq0", "accepted", "pg"):
        assert torch.equal(getattr(a, k), getattr(b, k)), k
    assert (a.best, a.best_val, a.nan_count) == (b.best, b.best_val, b.nan_count)
    fps = DeviceGP(device="cuda:0").factorise(X, y, ls, order="fps")
    assert fps.order == "fps"
    _check_trajectory(fps.refine(S, 0.0, 1.0, iters=R.TRAJ_ITERS, **kw), ref, mask, ls, "order='fps'")
    app = DeviceGP(device="cuda:0").factorise(X[:-3], y[:-3], ls)
    for i in range(N - 3, N):
        app.append(X[i], y[i])
    _check_trajectory(app.refine(S, 0.0, 1.0, iters=R.TRAJ_ITERS, **kw), ref, mask, ls, "three append()s")


# ---- 5. edges ------------------------------------------------------------------------------------------------------------------
def test_one_start_and_the_largest_set():
    X, y, Xs, ls = _problem(64, 4096, 2)
    gp, m = _gp(64, 4096, 2), _model(64, 4096, 2)
    tol = 1e-8 * max(1.0, float(np.abs(y).max()))
    ref = R.refine(X, y, ls, Xs, 0.0, 1.0, iters=6, model=m)
    one = gp.refine(Xs[0], 0.0, 1.0, iters=6)
    assert one.x.shape == (1, 2) and one.best == 0 and one.nan_count == 0
    assert int(one.accepted[0]) == ref["accepted"][0] and abs(float(one.acq[0]) - ref["acq"][0]) <= 1e-5
    r = gp.refine(Xs, 0.0, 1.0, iters=6)
    x, acq, acq0 = _np(r.x), _np(r.acq), _np(r.acq0)
    assert x.shape == (4096, 2) and np.all((x >= 0.0) & (x <= 1.0)) and np.all(acq >= acq0) and r.nan_count == 0
    assert np.abs(acq0 - ref["acq0"]).max() <= tol
    assert r.best == int(np.flatnonzero(acq == acq.max())[0]) and r.best_val == acq.max()
    dec = ref["margin"] > R.DECIDED
    print(f"P=4096: {int(dec.sum())} decided, |dx|/ls {(np.abs(x - ref['x']) / ls)[dec].max():.3g}")
    assert np.array_equal(_np(r.accepted)[dec], ref["accepted"][dec])
    assert (np.abs(x - ref["x"]) / ls[None, :])[dec].max() <= 1e-4 and np.abs(acq - ref["acq"])[dec].max() <= 1e-5


def test_edges_of_the_rule():
    X, y, Xs, ls = _problem(64, 2048, 2)
    gp = _gp(64, 2048, 2)
    S = Xs[:6].copy()
    S[1] = [1.7, -0.3]
    r0 = gp.refine(S, 0.0, 1.0, iters=0)
    assert np.array_equal(_np(r0.x), np.clip(S, 0.0, 1.0))        # iters = 0: the clipped starts (one outside the box)
    assert torch.equal(r0.acq, r0.acq0) and not np.any(_np(r0.accepted))
    pin = gp.refine(S, [0.0, 0.25], [1.0, 0.25], iters=10)
    assert np.all(_np(pin.x)[:, 1] == 0.25) and np.all(_np(pin.acq) >= _np(pin.acq0))
    S[2, 0] = np.nan
    r = gp.refine(S, 0.0, 1.0, iters=10)
    x = _np(r.x)
    assert r.nan_count == 1 and np.isnan(x[2, 0]) and x[2, 1] == S[2, 1] and int(r.accepted[2]) == 0
    assert np.isnan(_np(r.acq)[2]) and np.isnan(_np(r.acq0)[2]) and np.isnan(_np(r.pg)[2])
    ok = [0, 1, 3, 4, 5]
    assert r.best in ok and np.all(np.isfinite(_np(r.acq)[ok])) and torch.equal(r.x[ok], gp.refine(S[ok], 0.0, 1.0, iters=10).x)
    g = gp.posterior_grad(S)
    assert all(np.all(np.isnan(_np(getattr(g, k))[2])) for k in ("mu", "sigma", "acq", "dmu", "dsigma", "dacq"))
    with pytest.raises(ValueError):
        gp.refine(np.zeros((4097, 2)), 0.0, 1.0)
    with pytest.raises(ValueError):
        gp.posterior_grad(np.zeros((4097, 2)))
    for bad in (dict(lower=1.0, upper=0.0), dict(lower=0.0, upper=np.inf), dict(lower=0.0, upper=1.0, iters=-1),
                dict(lower=0.0, upper=1.0, iters=1001), dict(lower=0.0, upper=1.0, step0=0.0),
                dict(lower=0.0, upper=1.0, step0=np.nan), dict(lower=0.0, upper=1.0, acquisition="ucb")):
        with pytest.raises(ValueError):
            gp.refine(S, **bad)
    X17, y17, Xs17, ls17 = _problem(20, 64, 17)
    g17 = DeviceGP(device="cuda:0").factorise(X17, y17, ls17)
    for call in (lambda: g17.refine(Xs17[:4], 0.0, 1.0), lambda: g17.posterior_grad(Xs17[:4]),
                 lambda: g17.select_refined(Xs17, n_starts=4)):
        with pytest.raises(ValueError):
            call()


# ---- 6. the classes ------------------------------------------------------------------------------------------------------------
def _selector(cls, X, y, Xs, ls, fd):
    ps = cls()
    ps.measured_pts, ps.measured_vals, ps.predicted_pts, ps.feature_domain = X, y, Xs, fd
    ps.set_kernel_params(ls)
    ps.update_surrogate()
    return ps


@pytest.mark.parametrize("cls", [PointSelector, PointSelectorHost])
@pytest.mark.parametrize("N,M,d", [(64, 2048, 2), (300, 4096, 8)])
def test_selector_classes_refine_next(N, M, d, cls):
    X, y, Xs, ls = _problem(N, M, d)
    fd = [64, M // 64]
    ps = _selector(cls, X, y, Xs, ls, fd)
    idx0 = ps.lower_confidence_bound()
    keep = {k: np.array(getattr(ps, k)) for k in ("mean_func", "cov_func", "acq_func_eval", "kernel_params", "measured_pts",
                                                  "measured_vals", "predicted_pts")}
    gp = _gp(N, M, d)
    for kw, call in ((R.acq_kw("lcb", y), dict()), (R.acq_kw("ei", y, table=True), dict(acquisition="ei"))):
        x = ps.refine_next(**call)
        assert isinstance(x, np.ndarray) and x.dtype == np.float64 and x.shape == (d,)
        assert np.all((x >= Xs.min(axis=0)) & (x <= Xs.max(axis=0)))
        here, grid = float(gp.score(x[None, :], dense=True, **kw).acq[0]), gp.score(Xs, **kw).best_val
        print(f"{cls.__name__} N={N} d={d} {kw['acquisition']}: grid {grid:.6g} -> refined {here:.6g}")
        assert here >= grid
        for k, v in keep.items():
            assert np.array_equal(np.array(getattr(ps, k)), v), k
    assert np.array_equal(ps.lower_confidence_bound(), idx0)
    assert np.array_equal(idx0, np.unravel_index(int(np.argmax(keep["acq_func_eval"])), fd))
    with pytest.raises(ValueError):
        ps.refine_next(n_starts=0)


def test_refine_next_under_a_screened_precision_leaves_last_screen():
    """An acquisition that the class has not cached yet runs the screen again for the ranking of the starts; last_screen
    and acq_func_eval stay the last acquisition method's, and the refined point (always fp64) is no worse than the grid's."""
    N, M, d = 300, 4096, 8
    X, y, Xs, ls = _problem(N, M, d)
    ps = _selector(lambda: PointSelector(precision="i8"), X, y, Xs, ls, [64, M // 64])
    ps.lower_confidence_bound()
    screen, acq = dict(ps.last_screen), np.array(ps.acq_func_eval)
    kw = R.acq_kw("ei", y, table=True)
    x = ps.refine_next(acquisition="ei")
    assert ps.last_screen == screen and np.array_equal(ps.acq_func_eval, acq)
    gp = _gp(N, M, d)
    assert float(gp.score(x[None, :], dense=True, **kw).acq[0]) >= gp.score(Xs, **kw).best_val


@pytest.mark.parametrize("cls", [PointSelector, PointSelectorHost])
def test_selector_classes_raise_on_nan(cls):
    X, y, Xs, ls = _problem(64, 2048, 2)
    Xn = Xs.copy()
    Xn[5, 1] = np.nan
    ps = _selector(cls, X, y, Xn, ls, [64, 32])
    with pytest.raises(IndexError):
        ps.refine_next()
