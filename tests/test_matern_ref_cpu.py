"""The NumPy restatement of the Matern families (tests/matern_ref.py) checked against long double: the kernels' closed forms, the
likelihood gradient by central differences of a long-double value, the posterior by a long-double Cholesky.  No GPU."""
import numpy as np
import pytest

import matern_ref as MR
from ard_fit_ref import nlml_and_grad as se_nlml_and_grad
from bayesian_optimisation_amd.synthetic import make_problem

LD = np.longdouble
EPS = float(np.finfo(np.float64).eps) / 2   # unit roundoff

# (N, M, d) of tests/test_gpu_matern.py's posterior cases
SHAPES = [(1, 1, 1), (2, 513, 2), (63, 1000, 3), (64, 512, 8), (65, 1025, 1), (127, 700, 16), (128, 511, 2), (129, 1537, 3),
          (300, 4096, 8)]


@pytest.mark.parametrize("family", MR.FAMILIES)
@pytest.mark.parametrize("N,M,d", SHAPES)
def test_unit_diagonal_symmetry_and_positive_definiteness(family, N, M, d):
    X, _, _, ls = make_problem(N, M, d)
    K = MR.kernel(X, X, ls, family)
    assert np.all(np.diag(K) == 1.0)
    assert np.array_equal(K, K.T)
    assert np.all(K > 0.0) and np.all(K <= 1.0)
    np.linalg.cholesky(MR.gram(X, ls, family, 1e-4, 1e-6))   # raises when not positive definite
    assert MR.kernel(X[:1], X[:1], ls, family)[0, 0] == 1.0


@pytest.mark.parametrize("family", MR.FAMILIES)
@pytest.mark.parametrize("d", [1, 3, 8, 16])
def test_kernels_match_their_closed_forms_in_long_double(family, d):
    """float64 against the same closed form evaluated in long double from the same float64 inputs.  Bound: r^2 is a sum of d
    terms of three roundings each, relative error <= (d + 3) u; the square root halves it and the Matern argument's constant
    adds one; |a dk/da| <= max a^2 exp(-a) = 0.54 (0.37 for the squared exponential's r^2 / 2 exp(-r^2 / 2)); four more roundings
    on values <= 1.35 in the polynomial, the exponential and the product."""
    X, _, Xs, ls = make_problem(70, 300, d)
    for A, B in ((X, X), (Xs, X)):
        k64 = MR.kernel(A, B, ls, family)
        kld = MR.kernel(A, B, ls, family, dtype=LD)
        err = float(np.max(np.abs(k64.astype(LD) - kld)))
        print(f"{family} d {d}: max |k64 - k_ld| = {err:.2e}")
        assert err <= (0.54 * (d + 3) + 6) * EPS


def _nlml_longdouble(X, y, ls, family, jitter):
    K = MR.kernel(X, X, ls, family, dtype=LD) + LD(jitter) * np.eye(len(X), dtype=LD)
    N = len(K)
    L = np.zeros((N, N), dtype=LD)
    for j in range(N):
        L[j, j] = np.sqrt(K[j, j] - L[j, :j] @ L[j, :j])
        if j + 1 < N:
            L[j + 1:, j] = (K[j + 1:, j] - L[j + 1:, :j] @ L[j, :j]) / L[j, j]
    z = np.asarray(y, dtype=LD).copy()
    for i in range(N):
        z[i] = (z[i] - L[i, :i] @ z[:i]) / L[i, i]
    return LD(0.5) * (z @ z + LD(2) * np.sum(np.log(np.diag(L))) + N * np.log(LD(2) * np.pi))


@pytest.mark.parametrize("family", MR.FAMILIES)
@pytest.mark.parametrize("N,d", [(65, 3), (129, 8)])
def test_gradient_matches_long_double_central_differences_of_the_value(family, N, d):
    """Step and bound of tests/test_hyper_ref_cpu.py: h = 1e-5 in log ls, |g - num| <= 1e-6 of the cancelling sum."""
    X, y0 = MR.gp_problem(5, N, d, family if family != "se" else "matern52")
    y, ls, h = 3.0 + 2.0 * y0, np.geomspace(0.4, 0.9, d), 1e-5
    f, g, scale = MR.nlml_and_grad(X, y, ls, family, jitter=3e-2, with_scale=True)
    assert float(abs(LD(f) - _nlml_longdouble(X, y, ls, family, 3e-2))) <= 1e-12 * abs(f)
    num = np.empty(d)
    for k in range(d):
        e = np.zeros(d, dtype=LD)
        e[k] = h
        fp = _nlml_longdouble(X, y, np.exp(np.log(ls.astype(LD)) + e), family, 3e-2)
        fm = _nlml_longdouble(X, y, np.exp(np.log(ls.astype(LD)) - e), family, 3e-2)
        num[k] = float((fp - fm) / (2 * LD(h)))
    print(f"{family} N {N} d {d}: max |g - num| / scale = {np.max(np.abs(g - num) / scale):.2e}")
    assert np.all(np.abs(g - num) <= 1e-6 * scale), (g, num, scale)


def test_squared_exponential_family_is_the_existing_reference():
    X, y0 = MR.gp_problem(5, 65, 3)
    ls = np.geomspace(0.4, 0.9, 3)
    f, g, s = MR.nlml_and_grad(X, y0, ls, "se", with_scale=True)
    fr, gr, sr = se_nlml_and_grad(X, y0, ls, with_scale=True)
    assert f == pytest.approx(fr, rel=1e-12, abs=0) and np.all(np.abs(g - gr) <= 1e-10 * sr)


@pytest.mark.parametrize("family", MR.MATERN)
@pytest.mark.parametrize("fit_mean,fit_scale", [(False, False), (True, True)])
def test_hyper_gradient_matches_central_differences(family, fit_mean, fit_scale):
    """tests/test_hyper_ref_cpu.py::test_gradient_matches_central_differences for the Matern families."""
    X, y0 = MR.gp_problem(5, 65, 3, family)
    y, ls, noise, h, d = 3.0 + 2.0 * y0, np.geomspace(0.4, 0.9, 3), 3e-2, 1e-5, 3
    f, g, m, s2, scale = MR.nlml_hyper(X, y, ls, noise, family, fit_mean, fit_scale, with_scale=True)
    z = np.log(np.concatenate([ls, [noise]]))
    num = np.empty(d + 1)
    for k in range(d + 1):
        e = np.zeros(d + 1)
        e[k] = h
        fp = MR.nlml_hyper(X, y, np.exp(z + e)[:d], np.exp(z + e)[d], family, fit_mean, fit_scale)[0]
        fm = MR.nlml_hyper(X, y, np.exp(z - e)[:d], np.exp(z - e)[d], family, fit_mean, fit_scale)[0]
        num[k] = (fp - fm) / (2 * h)
    assert np.all(np.abs(g - num) <= 1e-6 * scale), (g, num, scale)
    if not (fit_mean or fit_scale):   # no flags at a jitter: the length-scale-only objective
        fr, gr, sr = MR.nlml_and_grad(X, y, ls, family, jitter=noise, with_scale=True)
        assert f == pytest.approx(fr, rel=1e-12, abs=0) and np.all(np.abs(g[:d] - gr) <= 1e-10 * sr)


@pytest.mark.parametrize("family", MR.MATERN)
@pytest.mark.parametrize("N,M,d", SHAPES)
def test_posterior_matches_a_long_double_cholesky(family, N, M, d):
    """The float64 restatement may use a hundredth of what tests/test_gpu_matern.py allows the GPU (1e-10 max(1, |y|) on the mean,
    1e-9 on sigma), so that it does not eat that budget: 1e-12 max(1, |y|) and 1e-11.  (Measured: 4e-13 and 7e-14 at most.)"""
    X, y, Xs, ls = make_problem(N, M, d)
    Xs = Xs[:: max(1, M // 256)]   # the long-double solves are slow: every 16th candidate at the largest shape
    mu, sig = MR.posterior(X, y, Xs, ls, family)
    mul, sigl = MR.posterior_longdouble(X, y, Xs, ls, family)
    em, es = float(np.max(np.abs(mu - mul))), float(np.max(np.abs(sig - sigl)))
    print(f"{family} N {N} M {M} d {d}: |dmu| {em:.2e}, |dsigma| {es:.2e}")
    assert em <= 1e-12 * max(1.0, float(np.max(np.abs(y)))) and es <= 1e-11


def test_gp_problem_is_seeded_and_draws_from_the_matern_prior():
    X, y = MR.gp_problem(3, 200, 3, noise=0.01)
    X2, y2 = MR.gp_problem(3, 200, 3, noise=0.01)
    assert np.array_equal(X, X2) and np.array_equal(y, y2) and X.shape == (200, 3) and y.shape == (200,)
    assert 0.3 < np.std(y) < 2.0


# ---- the premises of tests/test_gpu_matern.py that need no GPU ---------------------------------------------------------------
@pytest.mark.parametrize("family", MR.MATERN)
@pytest.mark.parametrize("N,M,d", MR.SELECTION_SHAPES)
def test_selection_shapes_have_a_top_two_gap_beyond_the_tolerance(family, N, M, d):
    from oracle import gp_oracle as O

    X, y, Xs, ls = make_problem(N, M, d)
    mu, sig = MR.posterior(X, y, Xs, ls, family)
    tol = 1e-8 * max(1.0, float(np.max(np.abs(y))))
    for acq in (O.lcb(mu, sig, 4), O.expected_improvement(mu, sig, float(np.min(y)), MR.EI_XI)):
        top = np.sort(acq)[-2:]
        assert top[1] - top[0] > 100 * tol, (top, tol)


@pytest.mark.parametrize("family", MR.MATERN)
@pytest.mark.parametrize("seed", MR.FIT_SEEDS)
def test_fit_seeds_have_an_interior_well_conditioned_optimum(family, seed):
    from bayesian_optimisation_amd.ard_fit import fit_length_scales

    X, y = MR.gp_problem(seed, 200, 3, family, noise=0.01)
    cpu = fit_length_scales(lambda ls: MR.nlml_and_grad(X, y, ls, family), **MR.FIT_BOX)
    u = np.where(np.random.default_rng(0).random(3) < 0.5, -1.0, 1.0)

    def perturbed(ls):
        f, g = MR.nlml_and_grad(X, y, ls, family)
        return f, g * (1.0 + 1e-9 * u)

    per = fit_length_scales(perturbed, **MR.FIT_BOX)
    assert cpu.converged and per.converged
    assert np.all(cpu.ls > 0.05 * 1.01) and np.all(cpu.ls < 5.0 / 1.01)
    shift = float(np.max(np.abs(per.ls / cpu.ls - 1.0)))
    print(f"{family} seed {seed}: ls {cpu.ls}, shift {shift:.2e}, evaluations {cpu.n_eval} / {per.n_eval}")
    assert shift < 1e-12
