"""ML-II length-scale fitting on the GPU: the likelihood gradient kernel (csrc/ard_grad.hip) against the NumPy reference
(tests/ard_fit_ref.py), its edge cases, the device fit against the CPU optimiser, and the drop-in class with
ard="gradient" end to end."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

from ard_fit_ref import gp_problem, nlml_and_grad as ref_nlml_and_grad  # noqa: E402
from bayesian_optimisation_amd import DeviceGP, host_binding  # noqa: E402
from bayesian_optimisation_amd.ard_fit import fit_length_scales  # noqa: E402
from bayesian_optimisation_amd.host_binding import PointSelectorHost  # noqa: E402
from bayesian_optimisation_amd.point_selector import PointSelector  # noqa: E402
from bayesian_optimisation_amd.synthetic import ard_length_scales, make_problem, rff_objective, sobol_points  # noqa: E402
from oracle import gp_oracle as O  # noqa: E402

_GP = {}


def _gp():
    if "gp" not in _GP:
        _GP["gp"] = DeviceGP(device="cuda:0")
    return _GP["gp"]


def _problem(N, d):
    """Sobol points and a smooth objective (the surrogate sizes' inputs: tests/test_gpu_ard_large_n.py)."""
    X = sobol_points(0, N, d)
    return X, rff_objective(X, ard_length_scales(d)), ard_length_scales(d)


# the padding edges (N = 63 / 64 / 65 around a 64-row tile, 127 / 128 / 129 around the 128 padding granule), one
# observation, every compiled d at least once among 1 / 2 / 3 / 8 / 16, and the surrogate sizes
PAIRS = [(1, 1), (2, 2), (63, 3), (64, 8), (65, 1), (127, 16), (128, 2), (129, 3), (300, 8), (1030, 16), (2048, 8),
         (4096, 3)]


@pytest.mark.parametrize("N,d", PAIRS)
def test_value_and_gradient_match_the_numpy_reference(N, d):
    X, y, ls = _problem(N, d)
    f, g = _gp().nlml_and_grad(X, y, ls)
    fr, gr, scale = ref_nlml_and_grad(X, y, ls, with_scale=True)
    assert f == pytest.approx(fr, rel=1e-10, abs=0)
    assert g.shape == (d,)
    if N == 1:
        assert np.all(g == 0.0)
    assert np.all(np.abs(g - gr) <= 1e-7 * scale), (g, gr, scale)


@pytest.mark.parametrize("N,d", [(65, 2), (300, 8)])
def test_value_is_the_logdet_likelihood_of_the_grid(N, d):
    X, y, ls = _problem(N, d)
    f, _ = _gp().nlml_and_grad(X, y, ls)
    grid = _gp().nlml_grid(X, y, ls[None], likelihood="logdet")
    assert f == pytest.approx(float(grid[0]), rel=1e-10, abs=0)


def test_two_calls_give_the_same_bits_and_leave_the_surrogate_alone():
    X, y, ls = _problem(1030, 8)
    gp = DeviceGP(device="cuda:0")
    gp.factorise(X[:200], y[:200], ls)
    U0, a0 = gp.U.clone(), gp.alpha.clone()
    f1, g1 = gp.nlml_and_grad(X, y, ls)
    f2, g2 = gp.nlml_and_grad(X, y, ls)
    assert f1 == f2 and np.array_equal(g1, g2)
    assert gp.N == 200 and bool((gp.U == U0).all()) and bool((gp.alpha == a0).all())


def test_not_positive_definite_gives_nan_everywhere():
    X, y, ls = _problem(100, 2)
    f, g = _gp().nlml_and_grad(X, y, ls, jitter=-0.5)
    assert np.isnan(f) and np.all(np.isnan(g))
    fh, gh = host_binding.nlml_and_grad(X, y, ls, jitter=-0.5)
    assert np.isnan(fh) and np.all(np.isnan(gh))


def test_host_entry_matches_the_device_entry():
    X, y, ls = _problem(300, 3)
    f, g = _gp().nlml_and_grad(X, y, ls)
    fh, gh = host_binding.nlml_and_grad(X, y, ls)
    assert fh == pytest.approx(f, rel=1e-13, abs=0)
    np.testing.assert_allclose(gh, g, rtol=1e-12, atol=0)


# seeds whose optimum is interior and well conditioned: a 1e-9 relative perturbation of the gradient moves the fitted
# length scales of the CPU optimiser by < 1e-12 relative
@pytest.mark.parametrize("seed", [21, 25])
def test_device_fit_follows_the_cpu_optimiser(seed):
    X, y = gp_problem(seed, 200, 3, noise=0.01)
    box = dict(ls0=[0.5] * 3, lower=[0.05] * 3, upper=[5.0] * 3)
    cpu = fit_length_scales(lambda ls: ref_nlml_and_grad(X, y, ls), **box)
    dev = _gp().fit_length_scales(X, y, **box)
    assert dev.converged and cpu.converged
    assert dev.nlml == pytest.approx(cpu.nlml, rel=1e-8, abs=0)
    np.testing.assert_allclose(dev.ls, cpu.ls, rtol=1e-4)
    assert np.all(np.diff(dev.trace) <= 0.0)


def _selector(cls, X, y, Xs, fd, length_scales, **kw):
    ps = cls(**kw)
    ps.name, ps.iteration = "T", 0
    ps.measured_pts, ps.measured_vals = X, y
    ps.feature_domain = fd
    ps.predicted_pts = Xs
    ps.length_scales = length_scales
    ps.update_surrogate()
    return ps, ps.lower_confidence_bound()


def _check_fit(ps, X, y, Xs, idx, lower, upper, shape):
    kp = np.asarray(ps.kernel_params)
    assert kp.shape == shape
    ls = kp.reshape(-1)
    assert np.all(ls >= lower * (1 - 1e-12)) and np.all(ls <= upper * (1 + 1e-12))
    tr = np.asarray(ps.hyperparam_obj)
    assert len(tr) >= 2 and np.all(np.diff(tr) <= 0.0) and np.array_equal(tr, ps.nlogml)
    assert ps.last_fit["n_eval"] >= len(tr) and ps.last_fit["nlml"] == tr[-1]
    assert tr[-1] == pytest.approx(O.nlml_cells_logdet(X, y, ls[None])[0], rel=1e-9, abs=0)
    acq = O.lcb(*O.posterior_chol(X, y, Xs, ls), 4)
    flat = int(np.ravel_multi_index(tuple(idx), ps.feature_domain))
    assert flat == int(np.flatnonzero(acq == acq.max())[0])


@pytest.mark.parametrize("name", ["g2_n20_tr", "g11_2d_n64"])
def test_point_selector_gradient_mode_on_golden_inputs(golden, name):
    g = golden(name)
    fd = [int(v) for v in g["feature_domain"]]
    ps, idx = _selector(PointSelector, g["X"], g["y"], g["Xs"], fd, g["length_scales"], ard="gradient")
    axes = np.atleast_2d(g["length_scales"])
    shape = (1, 1) if g["X"].shape[1] == 1 else (2,)
    _check_fit(ps, g["X"], g["y"], g["Xs"], idx, axes.min(axis=1), axes.max(axis=1), shape)
    if name == "g11_2d_n64":
        ph, idh = _selector(PointSelectorHost, g["X"], g["y"], g["Xs"], fd, g["length_scales"], ard="gradient")
        np.testing.assert_allclose(np.asarray(ph.kernel_params), np.asarray(ps.kernel_params), rtol=1e-10, atol=0)
        assert np.array_equal(idh, idx)


def test_point_selector_gradient_mode_d8_beats_the_coordinate_search():
    X, y, Xs, _ = make_problem(512, 4096, 8)
    axes = [np.geomspace(0.05, 5.0, 16)] * 8
    fd = [4096]
    ps, idx = _selector(PointSelector, X, y, Xs, fd, axes, ard="gradient")
    _check_fit(ps, X, y, Xs, idx, np.full(8, 0.05), np.full(8, 5.0), (8,))
    cs, _ = _selector(PointSelector, X, y, Xs, fd, axes, likelihood="logdet")
    grid_nlml = O.nlml_cells_logdet(X, y, np.asarray(cs.kernel_params)[None])[0]
    assert ps.hyperparam_obj[-1] <= grid_nlml, (ps.hyperparam_obj[-1], grid_nlml)
