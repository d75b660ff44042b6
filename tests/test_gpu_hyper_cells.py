"""The likelihood over all hyperparameters at MANY cells in one launch (csrc/hyper_wave.hip, DeviceGP.nlml_hyper_cells) against
the NumPy restatements (tests/hyper_ref.py, tests/matern_ref.py): every compiled size and feature count, both ends of the noise
range, all four flag pairs, the three covariance families, cell counts around a partly filled workgroup, the NaN rule, the
per-cell route beyond 64 observations, and the sampler of hyper_posterior.py driven by the kernel against the same sampler
driven by the restatement."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

import hyper_ref as H  # noqa: E402
import matern_ref as MR  # noqa: E402
from ard_fit_ref import gp_problem  # noqa: E402
from bayesian_optimisation_amd import DeviceGP  # noqa: E402
from bayesian_optimisation_amd.ard_fit import fit_hyperparameters  # noqa: E402
from bayesian_optimisation_amd.hyper_posterior import sample  # noqa: E402
from bayesian_optimisation_amd.synthetic import ard_length_scales, rff_objective, sobol_points  # noqa: E402

_GP = {}


def _gp():
    if "gp" not in _GP:
        _GP["gp"] = DeviceGP(device="cuda:0")
    return _GP["gp"]


def _problem(N, d):
    """The inputs of tests/test_gpu_hyper.py::_problem, with the offset and scale of a y that is not standardised."""
    X = sobol_points(0, N, d)
    return X, 40.0 + 7.0 * rff_objective(X, ard_length_scales(d)), ard_length_scales(d)


def _cells(ls, rho, G=5):
    """G cells with distinct length scales around ls at one noise ratio."""
    f = np.geomspace(0.7, 1.4, G) if G > 1 else np.ones(1)
    return np.concatenate([ls[None, :] * f[:, None], np.full((G, 1), rho)], axis=1)


# every NMAX (16 / 32 / 48 / 64) at its edge and one past the one before, every compiled D (2 / 4 / 8 / 16) and d below it
PAIRS = [(1, 1), (2, 2), (15, 3), (16, 8), (17, 1), (32, 16), (33, 2), (48, 4), (49, 8), (63, 16), (64, 2)]
ALL_FLAGS = [(False, False), (True, False), (False, True), (True, True)]
CASES = [(N, d, rho, fm, fs, "se") for N, d in PAIRS for rho in (1e-4, 3e-2)
         for fm, fs in (ALL_FLAGS if (N, d) in ((33, 2), (49, 8)) else [(True, True)])]
CASES += [(N, d, rho, True, True, fam) for N, d in ((33, 2), (49, 8)) for rho in (1e-4, 3e-2) for fam in MR.MATERN]

# mean and scale^2 against the restatement in np.longdouble, as the relative distances of tests/test_gpu_hyper.py:
# |m - m_ld| / max(|m_ld|, s_ld) and |s2 - s2_ld| / s2_ld.  REF_DIST: the float64 restatement's own largest distance over the
# five cells of every case of CASES, per noise level (m, s2), computed on the CPU; the bound is ten times that.  (The value L
# itself: largest relative distance from the restatement 1.04e-11, at N = 64, d = 2, rho = 1e-4, for a bound of 1e-10.)
# Measured (restatement / device on an MI355X):
#   rho 1e-4: m 8.64e-14 (N = 64, d = 2) / 6.47e-14 (N = 33, d = 2),  s2 1.03e-12 (N = 64, d = 2) / 1.17e-12 (N = 64, d = 2)
#   rho 3e-2: m 1.33e-15 (N = 64, d = 2) / 3.13e-16 (N = 15, d = 3),  s2 4.37e-15 (N = 48, d = 4) / 1.28e-15 (N = 48, d = 4)
REF_DIST = {1e-4: (8.64e-14, 1.03e-12), 3e-2: (1.33e-15, 4.37e-15)}


def _dist(m, s2, ml, sl):
    return float(abs(m - ml) / max(abs(ml), np.sqrt(sl))), float(abs(s2 - sl) / sl)


def _reference(X, y, cell, d, fm, fs, family):
    if family == "se":
        r = H.nlml_hyper(X, y, cell[:d], cell[d], fm, fs)
        ml, sl = H.mean_scale_longdouble(X, y, cell[:d], cell[d], fm, fs)
    else:
        r = MR.nlml_hyper(X, y, cell[:d], cell[d], family, fm, fs)
        ml, sl = MR.mean_scale_longdouble(X, y, cell[:d], cell[d], family, fm, fs)
    return r[0], r[2], r[3], ml, sl


def restatement_distances():
    """{rho: (largest m distance, largest s2 distance, where)} of the float64 restatement over CASES: what REF_DIST records
    (python -c "import test_gpu_hyper_cells as t; print(t.restatement_distances())" on any machine)."""
    out = {}
    for N, d, rho, fm, fs, family in CASES:
        X, y, ls = _problem(N, d)
        if N == 1 and fs:
            fs = False
        for cell in _cells(ls, rho):
            _, m, s2, ml, sl = _reference(X, y, cell, d, fm, fs, family)
            dm, ds = _dist(m, s2, ml, sl)
            cur = out.get(rho, (0.0, 0.0, None, None))
            out[rho] = (max(cur[0], dm), max(cur[1], ds), (N, d) if dm > cur[0] else cur[2], (N, d) if ds > cur[1] else cur[3])
    return out


@pytest.mark.parametrize("N,d,rho,fit_mean,fit_scale,family", CASES)
def test_value_mean_and_scale_match_the_restatement(N, d, rho, fit_mean, fit_scale, family):
    X, y, ls = _problem(N, d)
    cells = _cells(ls, rho)
    out = _gp().nlml_hyper_cells(X, y, cells, fit_mean, fit_scale, kernel=family)
    assert out.shape == (5, 3) and _gp().hyper_cells_route(N, family) == "wave"
    if N == 1 and fit_scale:   # the residual is zero: no signal variance to profile
        assert np.all(np.isnan(out))
        fit_scale = False
        out = _gp().nlml_hyper_cells(X, y, cells, fit_mean, fit_scale, kernel=family)
    assert np.all(np.isfinite(out))
    worst = [0.0, 0.0, 0.0]
    for cell, (f, m, s2) in zip(cells, out):
        fr, mr, s2r, ml, sl = _reference(X, y, cell, d, fit_mean, fit_scale, family)
        assert f == pytest.approx(fr, rel=1e-10, abs=0)
        if not fit_mean:
            assert m == 0.0
        if not fit_scale:
            assert s2 == 1.0
        dm, ds = _dist(m, s2, ml, sl)
        worst = [max(worst[0], abs(f - fr) / abs(fr)), max(worst[1], dm), max(worst[2], ds)]
        assert dm <= 10 * REF_DIST[rho][0] and ds <= 10 * REF_DIST[rho][1], (dm, ds, _dist(mr, s2r, ml, sl))
    print(f"N {N} d {d} rho {rho} flags {int(fit_mean)}{int(fit_scale)} {family}: value rel {worst[0]:.2e}, "
          f"distance from longdouble m {worst[1]:.2e} s2 {worst[2]:.2e}")


@pytest.mark.parametrize("G", [1, 4, 5, 1027])
def test_cell_counts_around_a_partly_filled_workgroup(G):
    """Four cells per workgroup: 1 and 5 leave three waves of the last workgroup without a cell, 1027 = 256 x 4 + 3 one; every
    cell has its own length scales and noise, and a sample of them is compared with the restatement."""
    N, d = 33, 2
    X, y, ls = _problem(N, d)
    rng = np.random.default_rng(G)
    cells = np.concatenate([ls[None, :] * np.exp(rng.uniform(-0.7, 0.7, (G, d))), np.exp(rng.uniform(np.log(1e-4), np.log(3e-2), (G, 1)))],
                           axis=1)
    out = _gp().nlml_hyper_cells(X, y, cells)
    assert out.shape == (G, 3) and np.all(np.isfinite(out))
    for g in sorted({0, G // 3, G // 2, G - 2 if G > 1 else 0, G - 1}):
        fr, _, mr, s2r = H.nlml_hyper(X, y, cells[g, :d], cells[g, d])
        assert out[g, 0] == pytest.approx(fr, rel=1e-10, abs=0)
        assert out[g, 1] == pytest.approx(mr, rel=1e-9) and out[g, 2] == pytest.approx(s2r, rel=1e-9)
    # a cell's values do not depend on its place in the launch
    assert np.array_equal(_gp().nlml_hyper_cells(X, y, cells[::-1].copy())[::-1], out)


def test_a_cell_that_is_not_positive_definite_is_nan_and_its_neighbours_are_untouched():
    N, d = 33, 2
    X, y, ls = _problem(N, d)
    cells = _cells(ls, 3e-2, 9)
    good = _gp().nlml_hyper_cells(X, y, cells)
    bad = cells.copy()
    bad[4, d] = -0.5   # K0 - 0.5 I has negative eigenvalues at 33 points in the unit square
    assert np.any(np.isnan(H.nlml_hyper(X, y, bad[4, :d], -0.5)[0]))
    out = _gp().nlml_hyper_cells(X, y, bad)
    assert np.all(np.isnan(out[4]))
    keep = np.arange(9) != 4
    assert np.array_equal(out[keep], good[keep])
    # a constant y leaves no signal variance: NaN with the scale fitted, finite without
    const = np.full(N, 3.0)
    assert np.all(np.isnan(_gp().nlml_hyper_cells(X, const, cells)))
    fixed = _gp().nlml_hyper_cells(X, const, cells, fit_scale=False)
    assert np.all(np.isfinite(fixed)) and np.all(fixed[:, 1] == pytest.approx(3.0, rel=1e-12)) and np.all(fixed[:, 2] == 1.0)


@pytest.mark.parametrize("d", [1, 3, 16])
@pytest.mark.parametrize("N", [1, 16, 17, 33, 48, 49, 64])
def test_without_a_profile_the_cells_kernel_is_the_grid_kernel_up_to_the_order_of_one_sum(N, d):
    """Both kernels are built on csrc/wave_cell.h.  With flags = 0, the squared exponential and rho = jitter the cells kernel
    factors the same matrix by the same instructions as the grid kernel in its log-det mode, so every z_c and the log det are
    the same numbers; the grid kernel then sums the N terms z_c^2 >= 0 in column order and the cells kernel by a butterfly.
    Each order is within (N - 1) 2^-53 relative of the exact sum and the rest of the value costs a few roundings:
        |L_cells - L_grid| <= 64 * 2^-52 * (quad + |logdet| + N log 2 pi),   quad, logdet: tests/hyper_ref.py.
    Both sides of every compiled size (48 / 49: the row index that is no mask, lanes beyond NMAX), padded features, a feature
    count that is no power of two and the widest one; five cells: a partly filled second workgroup."""
    rho, log2pi = 1e-4, np.log(2.0 * np.pi)
    X, y, ls = _problem(N, d)
    cells = _cells(ls, rho)
    assert _gp().ARD_KERNEL == "wave" and _gp().hyper_cells_route(N) == "wave"
    out = _gp().nlml_hyper_cells(X, y, cells, fit_mean=False, fit_scale=False)
    grid = _gp().nlml_grid(X, y, cells[:, :d], jitter=rho, likelihood="logdet")
    assert out.shape == (5, 3) and grid.shape == (5,) and grid.dtype == np.float64
    assert np.all(out[:, 1] == 0.0) and np.all(out[:, 2] == 1.0)
    worst = 0.0
    for cell, lc, lg in zip(cells, out[:, 0], grid):
        p = H.nlml_hyper(X, y, cell[:d], rho, False, False, with_parts=True)
        quad = float(p["r"] @ p["alpha"])
        logdet = float(np.linalg.slogdet(H.kernel(X, cell[:d])[0] + rho * np.eye(N))[1])
        bound = 64 * 2.0 ** -52 * (quad + abs(logdet) + N * log2pi)
        worst = max(worst, abs(lc - lg) / bound)
        assert np.isfinite(lc) and np.isfinite(lg) and abs(lc - lg) <= bound, (lc, lg, bound)
    print(f"N {N} d {d}: largest |L_cells - L_grid| / bound {worst:.3f}")


def test_two_launches_give_the_same_bits_and_leave_the_surrogate_alone():
    X, y, ls = _problem(64, 2)
    gp = DeviceGP(device="cuda:0")
    gp.factorise(X[:40], y[:40], ls)
    U0, a0 = gp.U.clone(), gp.alpha.clone()
    cells = _cells(ls, 1e-4, 37)
    a, b = gp.nlml_hyper_cells(X, y, cells), gp.nlml_hyper_cells(X, y, cells)
    assert np.array_equal(a, b)
    assert gp.N == 40 and bool((gp.U == U0).all()) and bool((gp.alpha == a0).all())


@pytest.mark.parametrize("N,d", [(65, 3), (130, 2)])
def test_more_than_64_observations_take_the_per_cell_route(N, d):
    X, y, ls = _problem(N, d)
    cells = _cells(ls, 3e-2, 3)
    assert _gp().hyper_cells_route(N) == "loop"
    out = _gp().nlml_hyper_cells(X, y, cells)
    for cell, (f, m, s2) in zip(cells, out):
        fr, _, mr, s2r = H.nlml_hyper(X, y, cell[:d], cell[d])
        assert f == pytest.approx(fr, rel=1e-10, abs=0) and m == pytest.approx(mr, rel=1e-9) and s2 == pytest.approx(s2r, rel=1e-9)
    with pytest.raises(ValueError):
        _gp().nlml_hyper_cells(X, y, cells, route="wave")


def test_the_two_routes_agree_at_64_observations():
    X, y, ls = _problem(64, 2)
    cells = np.concatenate([_cells(ls, 1e-4, 3), _cells(ls, 3e-2, 3)])
    wave = _gp().nlml_hyper_cells(X, y, cells, route="wave")
    loop = _gp().nlml_hyper_cells(X, y, cells, route="loop")
    np.testing.assert_allclose(loop[:, 0], wave[:, 0], rtol=1e-10, atol=0)
    np.testing.assert_allclose(loop[:, 1:], wave[:, 1:], rtol=1e-9, atol=0)
    bad = cells.copy()
    bad[1, 2] = -0.5
    assert np.all(np.isnan(_gp().nlml_hyper_cells(X, y, bad, route="loop")[1]))


def test_refusals():
    X, y, ls = _problem(20, 2)
    for cells in (np.ones((3, 2)), np.ones(3), np.zeros((0, 3)), np.array([[0.5, -0.5, 1e-2]]), np.array([[0.5, np.nan, 1e-2]])):
        with pytest.raises(ValueError):
            _gp().nlml_hyper_cells(X, y, cells)
    with pytest.raises(ValueError):
        _gp().nlml_hyper_cells(X, y[:-1], np.ones((1, 3)))
    with pytest.raises(ValueError):
        _gp().nlml_hyper_cells(X, y, np.ones((1, 3)), kernel="rq")
    with pytest.raises(ValueError):
        _gp().nlml_hyper_cells(np.ones((5, 17)), np.arange(5.0), np.ones((1, 18)))


# ---- the sampler driven by the kernel -----------------------------------------------------------------------------------
BOX = dict(ls0=[0.5] * 2, ls_lower=[0.05] * 2, ls_upper=[5.0] * 2, noise0=1e-2, noise_lower=1e-6, noise_upper=1.0)
ZLO, ZHI = np.log([0.05, 0.05, 1e-6]), np.log([5.0, 5.0, 1.0])


@pytest.mark.parametrize("seed", [0, 1])
def test_the_sampler_on_the_device_follows_the_cpu_driven_run(seed):
    """gp_problem(seed, 20, 2, noise=0.05), 16 chains from the CPU fit's optimum, 3 sweeps: the CPU-driven run's smallest
    |L - slice level| is 1.5e-3 / 6.1e-3 for the seeds 0 / 1 (88 batches each; asserted > 1e-6), six orders above the two likelihoods'
    difference, so both runs take the same decisions: equal batch counts, states equal to rtol 1e-9."""
    X, y = gp_problem(seed, 20, 2, noise=0.05)
    fit = fit_hyperparameters(H.objective(X, y), **BOX)
    z0 = np.tile(np.log(np.concatenate([fit.ls, [fit.noise]])), (16, 1))

    def cpu(Z):
        return np.array([H.nlml_hyper(X, y, np.exp(z[:2]), float(np.exp(z[2])))[0] for z in Z])

    fn = _gp().nlml_hyper_cells_fn(X, y)
    rc = sample(cpu, z0, ZLO, ZHI, 3, seed)
    rd = sample(lambda Z: fn(np.exp(Z))[:, 0], z0, ZLO, ZHI, 3, seed)
    print(f"seed {seed}: {rc.n_batches} batches, min margin cpu {rc.min_margin:.2e} device {rd.min_margin:.2e}, "
          f"max |dz| {np.max(np.abs(rd.states - rc.states)):.2e}")
    assert rc.min_margin > 1e-6
    assert rd.n_batches == rc.n_batches and rd.kept == rc.kept
    np.testing.assert_allclose(rd.states, rc.states, rtol=1e-9, atol=0)
    np.testing.assert_allclose(rd.values, rc.values, rtol=1e-10, atol=0)
    assert np.std(rd.states[:, 2]) > 0.05   # the chains have left the optimum
