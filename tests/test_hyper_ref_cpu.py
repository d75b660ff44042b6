"""The NumPy restatement of the hyperparameter likelihood (tests/hyper_ref.py) checked against itself - central differences,
the length-scale-only objective it extends, the identity the GPU path re-uses ard_grad.hip by, leave-one-out refits, affine
invariance - and ard_fit.fit_hyperparameters driven by it.  No GPU."""
import numpy as np
import pytest

import hyper_ref as H
from ard_fit_ref import gp_problem, nlml_and_grad as ref_nlml_and_grad
from bayesian_optimisation_amd.ard_fit import HyperFitResult, fit_hyperparameters, fit_length_scales

FLAGS = [(False, False), (True, False), (False, True), (True, True)]


def _problem(N, d, seed=5):
    X, y = gp_problem(seed, N, d, noise=0.05)
    return X, 3.0 + 2.0 * y, np.geomspace(0.4, 0.9, d)


@pytest.mark.parametrize("fit_mean,fit_scale", FLAGS)
@pytest.mark.parametrize("N,d", [(2, 2), (65, 3), (200, 3)])
def test_gradient_matches_central_differences(N, d, fit_mean, fit_scale):
    X, y, ls = _problem(N, d)
    noise, h = 3e-2, 1e-5
    f, g, m, s2, scale = H.nlml_hyper(X, y, ls, noise, fit_mean, fit_scale, with_scale=True)
    z = np.log(np.concatenate([ls, [noise]]))
    num = np.empty(d + 1)
    for k in range(d + 1):
        e = np.zeros(d + 1)
        e[k] = h
        fp = H.nlml_hyper(X, y, np.exp(z + e)[:d], np.exp(z + e)[d], fit_mean, fit_scale)[0]
        fm = H.nlml_hyper(X, y, np.exp(z - e)[:d], np.exp(z - e)[d], fit_mean, fit_scale)[0]
        num[k] = (fp - fm) / (2 * h)
    print("max |g - num| / scale", np.max(np.abs(g - num) / scale))
    assert np.all(np.abs(g - num) <= 1e-6 * scale), (g, num, scale)


@pytest.mark.parametrize("N,d", [(2, 2), (65, 3), (200, 3)])
def test_no_flags_at_the_old_jitter_is_the_old_objective(N, d):
    X, y, ls = _problem(N, d)
    f, g, m, s2 = H.nlml_hyper(X, y, ls, 1e-4, False, False)
    fr, gr, sr = ref_nlml_and_grad(X, y, ls, jitter=1e-4, with_scale=True)
    assert m == 0.0 and s2 == 1.0
    assert f == pytest.approx(fr, rel=1e-10, abs=0)
    assert np.all(np.abs(g[:d] - gr) <= 1e-10 * sr)


@pytest.mark.parametrize("fit_mean,fit_scale", FLAGS)
def test_length_scale_gradients_are_the_old_kernel_on_the_standardised_pair(fit_mean, fit_scale):
    """What lets csrc/hyper.hip call gpbo_nlml_grad_f64 unchanged: on y' = r / s (whose alpha is alpha / s) the old objective has
    the same d gradients and the value L - 1/2 N log s^2."""
    X, y, ls = _problem(200, 3)
    noise = 3e-2
    p = H.nlml_hyper(X, y, ls, noise, fit_mean, fit_scale, with_parts=True)
    s = np.sqrt(p["s2"])
    fr, gr, sr = ref_nlml_and_grad(X, p["r"] / s, ls, jitter=noise, with_scale=True)
    assert np.all(np.abs(p["g"][:3] - gr) <= 1e-10 * sr)
    assert fr + 0.5 * len(y) * np.log(p["s2"]) == pytest.approx(p["f"], rel=1e-12, abs=0)


def test_leave_one_out_matches_n_refits():
    X, y, ls = _problem(40, 3)
    noise = 3e-2
    p = H.nlml_hyper(X, y, ls, noise, with_parts=True)
    mu, var, _ = H.loo(X, y, ls, noise)
    K0, _ = H.kernel(X, ls)
    Kt = K0 + noise * np.eye(40)
    for i in range(40):
        keep = np.arange(40) != i
        sol = np.linalg.solve(Kt[np.ix_(keep, keep)], np.stack([y[keep] - p["m"], Kt[keep, i]], axis=1))
        mu_i = p["m"] + Kt[i, keep] @ sol[:, 0]
        var_i = p["s2"] * (Kt[i, i] - Kt[i, keep] @ sol[:, 1])
        assert mu[i] == pytest.approx(mu_i, rel=1e-10, abs=1e-10)
        assert var[i] == pytest.approx(var_i, rel=1e-10, abs=1e-10)


def test_affine_maps_of_y_leave_the_gradients_and_shift_the_value():
    X, y, ls = _problem(200, 3)
    f, g, m, s2, scale = H.nlml_hyper(X, y, ls, 3e-2, with_scale=True)
    f2, g2, m2, s22 = H.nlml_hyper(X, 40.0 + 7.0 * y, ls, 3e-2)
    assert np.all(np.abs(g - g2) <= 1e-9 * scale)
    assert f2 - len(y) * np.log(7.0) == pytest.approx(f, rel=1e-10, abs=0)
    assert m2 == pytest.approx(40.0 + 7.0 * m, rel=1e-10) and s22 == pytest.approx(49.0 * s2, rel=1e-9)


def test_not_positive_definite_and_degenerate_profiles_give_nan():
    X, y, ls = _problem(20, 2)
    X[1] = X[0]
    f, g, m, s2 = H.nlml_hyper(X, y, ls, 1e-300)
    assert np.isnan(f) and np.all(np.isnan(g)) and np.isnan(m) and np.isnan(s2)
    f, g, m, s2 = H.nlml_hyper(X[:1], y[:1], ls, 1e-2)          # one observation, both flags: s^2 = 0
    assert np.isnan(f) and np.all(np.isnan(g))
    f, g, m, s2 = H.nlml_hyper(X[:1], y[:1], ls, 1e-2, True, False)
    assert np.isfinite(f) and np.all(np.isfinite(g)) and m == pytest.approx(y[0]) and s2 == 1.0


BOX = dict(ls0=[0.5] * 3, ls_lower=[0.05] * 3, ls_upper=[5.0] * 3, noise0=1e-2, noise_lower=1e-6, noise_upper=1.0)


@pytest.mark.parametrize("seed", [3, 7, 21, 25])
def test_fit_recovers_the_noise_and_beats_the_length_scale_only_fit(seed):
    X, y0 = gp_problem(seed, 200, 3, noise=0.05)
    y = 40.0 + 7.0 * y0
    res = fit_hyperparameters(H.objective(X, y), **BOX)
    assert isinstance(res, HyperFitResult) and res.converged, res.reason
    assert np.all(np.diff(res.trace) <= 0.0)
    assert np.all(res.ls > 0.05) and np.all(res.ls < 5.0) and 1e-6 < res.noise < 1.0
    sd = np.sqrt(res.noise) * res.scale
    print(f"seed {seed}: nlml {res.nlml:.6f}, noise sd {sd:.4f} (true 0.35), {res.n_iter} steps, {res.n_eval} evaluations, "
          f"{res.reason}")
    assert abs(sd - 0.35) <= 0.2 * 0.35
    f, g, m, s2 = H.nlml_hyper(X, y, res.ls, res.noise)
    assert res.nlml == f and res.mean == m and res.scale == np.sqrt(s2)
    # the length-scale-only model on the data standardised by hand, in the units of y: + N log std(y)
    ys = (y - y.mean()) / y.std()
    old = fit_length_scales(lambda ls: ref_nlml_and_grad(X, ys, ls), [0.5] * 3, [0.05] * 3, [5.0] * 3)
    assert res.nlml < old.nlml + len(y) * np.log(y.std()), (res.nlml, old.nlml + len(y) * np.log(y.std()))


def test_fit_refuses_a_constant_y_and_bad_boxes():
    X, y0 = gp_problem(3, 30, 2)
    # (a power of two: a = 2 b and m = 2 hold exactly, so r = 0 and s^2 = 0 without a rounding residue)
    with pytest.raises(np.linalg.LinAlgError):
        fit_hyperparameters(H.objective(X, np.full(30, 2.0)), [0.5] * 2, [0.05] * 2, [5.0] * 2, 1e-2, 1e-6, 1.0)
    with pytest.raises(ValueError):
        fit_hyperparameters(H.objective(X, y0), [0.5] * 2, [0.05] * 3, [5.0] * 2, 1e-2, 1e-6, 1.0)
    with pytest.raises(ValueError):
        fit_hyperparameters(H.objective(X, y0), [0.5] * 2, [0.05] * 2, [5.0] * 2, 1e-2, 0.0, 1.0)
