"""PointSelector(ard="marginal") end to end: the ML-II model of ard="hyper" unchanged, a sampled ensemble in `hyper_samples`, the
published arrays equal to the NumPy restatement (tests/ensemble_ref.py) on those samples, selections invariant under affine maps of
y, and the documented refusals."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

import ensemble_ref as E  # noqa: E402
from ard_fit_ref import gp_problem  # noqa: E402
from bayesian_optimisation_amd.point_selector import PointSelector  # noqa: E402

FD = [40, 40]
AXES = [np.geomspace(0.05, 5.0, 16)] * 2
S = 8
_RUNS = {}


def _data():
    X, y = gp_problem(3, 40, 2, noise=0.05)
    g = (np.arange(40) + 0.5) / 40
    return X, y, np.stack(np.meshgrid(g, g, indexing="ij"), -1).reshape(-1, 2)


def _selector(y, X=None, **kw):
    X0, _, Xs = _data()
    ps = PointSelector(**kw)
    ps.name, ps.iteration = "T", 0
    ps.measured_pts, ps.measured_vals = (X0 if X is None else X), y
    ps.feature_domain, ps.predicted_pts, ps.length_scales = FD, Xs, AXES
    ps.update_surrogate()
    return ps


def _run(tag):
    """One updated selector per (mode, scaling of y), shared by the tests below."""
    if tag not in _RUNS:
        mode, scaled = tag
        y = _data()[1]
        kw = dict(n_models=S) if mode == "marginal" else {}
        _RUNS[tag] = _selector(40.0 + 7.0 * y if scaled else y, ard=mode, **kw)
    return _RUNS[tag]


def _models(hs):
    return [(hs["ls"][s], float(hs["noise"][s]), 0.0, float(hs["y_mean"][s]), float(hs["y_scale"][s]), float(hs["weight"][s]))
            for s in range(len(hs["weight"]))]


@pytest.mark.parametrize("scaled", [False, True])
def test_published_arrays_are_the_restatement_on_the_sampled_models(scaled):
    X, y, Xs = _data()
    y = 40.0 + 7.0 * y if scaled else y
    ps, hyper = _run(("marginal", scaled)), _run(("hyper", scaled))
    hs = ps.hyper_samples
    # the ML-II model is ard="hyper"'s, unchanged
    assert np.array_equal(np.asarray(ps.kernel_params), np.asarray(hyper.kernel_params)) and ps.noise == hyper.noise
    assert ps.y_mean == hyper.y_mean and ps.y_scale == hyper.y_scale and ps.last_fit == hyper.last_fit
    for a, b in zip(ps.loo(), hyper.loo()):
        assert np.array_equal(a, b)
    assert np.array_equal(ps.cov_meas, hyper.cov_meas)
    # shapes and the box
    assert hs["ls"].shape == (S, 2) and all(hs[k].shape == (S,) for k in ("noise", "y_mean", "y_scale", "weight", "nlml"))
    assert np.all(hs["ls"] >= 0.05) and np.all(hs["ls"] <= 5.0) and np.all(hs["noise"] >= 1e-6) and np.all(hs["noise"] <= 1.0)
    assert np.all(hs["weight"] == 1.0 / S) and np.all(np.isfinite(hs["nlml"])) and np.all(hs["nlml"] >= ps.last_fit["nlml"] - 1e-4)
    assert hs["n_batches"] > 10 and hs["min_margin"] > 0.0 and hs["sweeps"] == 10 and hs["seed"] == 0 and hs["kept"] == 0
    assert len({tuple(r) for r in hs["ls"]}) == S                      # the chains have parted
    assert ps.mean_func.shape == ps.cov_func.shape == tuple(FD)
    print(f"scaled {scaled}: {hs['n_batches']} batches, min margin {hs['min_margin']:.2e}, ls {hs['ls'].min(axis=0)} .. "
          f"{hs['ls'].max(axis=0)}, noise {hs['noise'].min():.2e} .. {hs['noise'].max():.2e}")
    models = _models(hs)
    post = E.model_posteriors(X, y, Xs, models)
    for kind, call in ((E.LCB, lambda: ps.lower_confidence_bound()), (E.EI, lambda: ps.expected_improvement(xi=0.01 * (7 if scaled else 1)))):
        p0, p1 = (4.0, 0.0) if kind == E.LCB else (float(np.min(y)), 0.01 * (7 if scaled else 1))
        ref = E.fold(post, models, kind, p0, p1)
        idx = call()
        B = E.acq_bound(y, models, kind, 4.0)
        top = np.sort(ref["acq"])[-2:]
        err = np.max(np.abs(ps.acq_func_eval.ravel() - ref["acq"]))
        print(f"    {kind}: |acq - ref| {err:.2e} (bound {B:.2e}), top-two gap {top[1] - top[0]:.2e}")
        assert err <= B
        assert top[1] - top[0] > 2.0 * B and int(np.ravel_multi_index(tuple(idx), FD)) == ref["best_idx"]
    ref = E.fold(post, models, E.LCB, 4.0)
    assert np.max(np.abs(ps.mean_func.ravel() - ref["mean"])) <= E.mean_bound(y, models)
    assert np.all(np.abs(ps.cov_func.ravel() ** 2 - ref["var"]) <= E.var_bound(y, models, post, ref["shift"]))
    # integrating widens the error bars where the sampled models disagree
    assert np.mean(ps.cov_func) > 0.0 and not np.array_equal(ps.cov_func, hyper.cov_func)


def test_the_mode_is_invariant_under_affine_maps_of_y():
    a, b = _run(("marginal", False)), _run(("marginal", True))
    print(f"min margins {a.hyper_samples['min_margin']:.2e} / {b.hyper_samples['min_margin']:.2e}, batches "
          f"{a.hyper_samples['n_batches']} / {b.hyper_samples['n_batches']}, max |d ls| / ls "
          f"{np.max(np.abs(b.hyper_samples['ls'] / a.hyper_samples['ls'] - 1)):.2e}, mean_func "
          f"{np.max(np.abs(b.mean_func - (40.0 + 7.0 * a.mean_func))) / np.max(np.abs(b.mean_func)):.2e}")
    assert np.array_equal(a.lower_confidence_bound(), b.lower_confidence_bound())
    assert np.array_equal(a.expected_improvement(xi=0.01), b.expected_improvement(xi=0.07))
    assert np.max(np.abs(b.mean_func - (40.0 + 7.0 * a.mean_func))) <= 1e-6 * np.max(np.abs(b.mean_func))


def test_the_same_seed_gives_the_same_ensemble_and_another_seed_another():
    y = _data()[1]
    a = _run(("marginal", False))
    b = _selector(y, ard="marginal", n_models=S)
    assert all(np.array_equal(a.hyper_samples[k], b.hyper_samples[k]) for k in ("ls", "noise", "y_mean", "y_scale", "nlml"))
    assert np.array_equal(a.mean_func, b.mean_func) and np.array_equal(a.cov_func, b.cov_func)
    c = _selector(y, ard="marginal", n_models=S, seed=1)
    assert not np.array_equal(a.hyper_samples["ls"], c.hyper_samples["ls"])
    z = _selector(y, ard="marginal", n_models=3, posterior_sweeps=0)   # no sweep: three copies of the optimum = ard="hyper"
    h = _run(("hyper", False))
    np.testing.assert_allclose(z.hyper_samples["ls"], np.tile(np.asarray(h.kernel_params).reshape(-1), (3, 1)), rtol=1e-14)
    np.testing.assert_allclose(z.hyper_samples["noise"], h.noise, rtol=1e-14)   # (exp(log(.)) of the optimum)
    np.testing.assert_allclose(z.mean_func, h.mean_func, rtol=0, atol=1e-9 * max(1.0, float(np.max(np.abs(y)))))
    np.testing.assert_allclose(z.cov_func, h.cov_func, rtol=0, atol=1e-8 * h.y_scale)


def test_refusals_name_the_mode_and_the_edge_cases_follow_hyper():
    ps = _run(("marginal", False))
    for call in (lambda: ps.q_expected_improvement(), lambda: ps.select_batch(2), lambda: ps.select_thompson(2),
                 lambda: ps.refine_next()):
        with pytest.raises(ValueError, match="ard='marginal'"):
            call()
    X, y, Xs = _data()
    one = _selector(y[:1] + 40.0, X=X[:1], ard="marginal", n_models=S, noise0=2e-2)
    assert one.noise == 2e-2 and one.y_mean == y[0] + 40.0 and one.y_scale == 1.0 and one.last_fit is None
    assert one.hyper_samples["ls"].shape == (1, 2) and one.hyper_samples["weight"][0] == 1.0 and one.hyper_samples["n_batches"] == 0
    np.testing.assert_allclose(one.mean_func, y[0] + 40.0, rtol=0, atol=1e-12)
    assert one.lower_confidence_bound().shape == (2,)
    with pytest.raises(np.linalg.LinAlgError):
        _selector(np.full(5, 3.0), X=X[:5], ard="marginal")
    pk = PointSelector(ard="marginal")
    pk.set_kernel_params([0.5, 0.5])
    pk.measured_pts, pk.measured_vals, pk.feature_domain, pk.predicted_pts, pk.length_scales = X, y, FD, Xs, AXES
    with pytest.raises(ValueError):
        pk.update_surrogate()
