"""The Matern 3/2 and 5/2 covariance families on the GPU (csrc/kernel_build.hip, csrc/ard_grad.hip) against the NumPy restatement
(tests/matern_ref.py): covariance entries, the posterior at the kernels' edges, selection, bit identities, failures, the
likelihood gradient, the likelihood over all hyperparameters, the device fit, and the drop-in classes end to end."""
import ctypes as C

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

import matern_ref as MR  # noqa: E402
from bayesian_optimisation_amd import DeviceGP, _lib, host_binding  # noqa: E402
from bayesian_optimisation_amd.ard_fit import fit_length_scales  # noqa: E402
from bayesian_optimisation_amd.host_binding import PointSelectorHost  # noqa: E402
from bayesian_optimisation_amd.point_selector import PointSelector  # noqa: E402
from bayesian_optimisation_amd.synthetic import ard_length_scales, make_problem, rff_objective, sobol_points  # noqa: E402
from oracle import gp_oracle as O  # noqa: E402

FAMILIES = list(MR.MATERN)
_GP = {}
_REF = {}


def _gp():
    if "gp" not in _GP:
        _GP["gp"] = DeviceGP(device="cuda:0")
    return _GP["gp"]


def _first_argmax(a):
    return int(np.flatnonzero(a == np.max(a))[0])


def _posterior_ref(family, N, M, d):
    """(X, y, Xs, ls, mu, sigma) of make_problem(N, M, d), computed once per case and never changed."""
    key = (family, N, M, d)
    if key not in _REF:
        X, y, Xs, ls = make_problem(N, M, d)
        _REF[key] = (X, y, Xs, ls, *MR.posterior(X, y, Xs, ls, family))
    return _REF[key]


# ---- entries ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("family", FAMILIES)
@pytest.mark.parametrize("d", list(range(1, 17)))
def test_covariance_entries_match_the_restatement(family, d):
    """5e-15 absolute, the bound the squared-exponential entries hold in tests/test_gpu_parity.py: entries are <= 1 and
    max_a a^2 exp(-a) = 0.54, so a few ulp of error in a stay far below it."""
    X, y, Xs, ls = make_problem(70, 300, d)
    gp = DeviceGP(chunk=512).factorise(X, y, ls, kernel=family)
    Kxx, Ksx = gp.cov_meas_host(), gp.cov_meas_pred_host(Xs)
    rxx, rsx = MR.gram(X, ls, family, 1e-4, 1e-6), MR.kernel(Xs, X, ls, family)
    print(f"{family} d {d}: K(X,X) {np.max(np.abs(Kxx - rxx)):.2e}, K(X*,X) {np.max(np.abs(Ksx - rsx)):.2e}")
    np.testing.assert_allclose(Kxx, rxx, rtol=0, atol=5e-15)
    np.testing.assert_allclose(Ksx, rsx, rtol=0, atol=5e-15)
    assert np.array_equal(Kxx, Kxx.T)                                   # bitwise symmetric
    assert np.all(np.diag(Kxx) == (1.0 + 1e-4) + 1e-6)                  # k(x, x) = 1 exactly, then the two jitters in order
    Kself = gp.cov_meas_pred_host(X)                                    # candidates on top of the observations
    assert np.all(np.diag(Kself) == 1.0)
    np.testing.assert_allclose(gp.kxx_host(Xs[:40], ls, 1e-4, 1e-6), MR.gram(Xs[:40], ls, family, 1e-4, 1e-6), rtol=0, atol=5e-15)


# ---- the posterior at the kernel's edges: the odd observation tail, the 64-row slice, the 128 padding granule, the 512 chunk
# granule +- 1, several chunks, the second candidate of a thread missing ----------------------------------------------------------
EDGES = [(1, 1, 1, 512), (2, 513, 2, 512), (63, 1000, 3, 512), (64, 512, 8, 512), (65, 1025, 1, 512), (127, 700, 16, 512),
         (128, 511, 2, 512), (129, 1537, 3, 1024), (300, 4096, 8, 1024)]


@pytest.mark.parametrize("family", FAMILIES)
@pytest.mark.parametrize("N,M,d,chunk", EDGES)
def test_posterior_at_the_kernel_edges(family, N, M, d, chunk):
    """|dmu| <= 1e-10 max(1, |y|), |dsigma| <= 1e-9: the bounds of test_fused_path_vs_oracle_ragged_sizes (cond(K) of both Matern
    families at these shapes is at most 4.9e5, against 5.5e5 for the squared exponential)."""
    X, y, Xs, ls, mu_o, sig_o = _posterior_ref(family, N, M, d)
    gp = DeviceGP(chunk=chunk).factorise(X, y, ls, kernel=family)
    assert gp.kernel == family
    r = gp.score(Xs, dense=True, idx_offset=1000)
    mu, sig, acq = r.mu.cpu().numpy(), r.sigma.cpu().numpy(), r.acq.cpu().numpy()
    print(f"{family} N {N} M {M} d {d}: |dmu| {np.max(np.abs(mu - mu_o)):.2e}, |dsigma| {np.max(np.abs(sig - sig_o)):.2e}")
    assert np.max(np.abs(mu - mu_o)) <= 1e-10 * max(1.0, np.abs(y).max())
    assert np.max(np.abs(sig - sig_o)) <= 1e-9
    assert r.nan_count == 0 and r.best_idx == 1000 + _first_argmax(acq) and r.best_val == acq.max()
    # leave-one-out needs no kernel entries: it follows the factorisation
    mu_l, var_l, kd = (t.cpu().numpy() for t in gp.loo())
    kinv = np.diag(np.linalg.inv(MR.gram(X, ls, family, 1e-4, 1e-6)))
    np.testing.assert_allclose(kd, kinv, rtol=1e-6, atol=0)


# ---- selection ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("family", FAMILIES)
@pytest.mark.parametrize("N,M,d", MR.SELECTION_SHAPES)
def test_selection_matches_the_reference_acquisition(family, N, M, d):
    """LCB(4) and EI within 1e-8 max(1, |y|) of the reference's, and the reference's first arg-max (its top-two gap exceeds that
    bound at these shapes: tests/test_matern_ref_cpu.py)."""
    X, y, Xs, ls, mu_o, sig_o = _posterior_ref(family, N, M, d)
    tol = 1e-8 * max(1.0, float(np.abs(y).max()))
    gp = DeviceGP(chunk=1024).factorise(X, y, ls, kernel=family)
    f_best = float(y.min())
    for r, acq_o in ((gp.score(Xs, acquisition="lcb", explore=4.0, dense=True), O.lcb(mu_o, sig_o, 4)),
                     (gp.score(Xs, acquisition="ei", f_best=f_best, xi=MR.EI_XI, dense=True),
                      O.expected_improvement(mu_o, sig_o, f_best, MR.EI_XI))):
        acq = r.acq.cpu().numpy()
        print(f"{family} N {N} M {M} d {d}: |dacq| {np.max(np.abs(acq - acq_o)):.2e} (bound {tol:.2e})")
        assert np.max(np.abs(acq - acq_o)) <= tol
        top = np.sort(acq_o)[-2:]
        assert top[1] - top[0] > tol
        assert r.best_idx == _first_argmax(acq_o) and r.nan_count == 0
    # the second acquisition on the dense posterior (no kernel entries) agrees with the fused one
    s = gp.score(Xs, dense=True)
    e = gp.acquisition_on_posterior(s.mu, s.sigma, acquisition="ei", f_best=f_best, xi=MR.EI_XI)
    assert e.best_idx == _first_argmax(O.expected_improvement(mu_o, sig_o, f_best, MR.EI_XI))


# ---- bit identities ------------------------------------------------------------------------------------------------------------
def test_squared_exponential_through_the_new_entry_points_gives_todays_bits():
    """factorise(kernel="se") + score() - gpbo_factorise_kern_f64 / gpbo_posterior_acq_kern_f64 with id 0 - against the entry
    points without a kernel argument, called directly."""
    import torch

    X, y, Xs, ls = make_problem(300, 4096, 8)
    gp = DeviceGP(chunk=1024).factorise(X, y, ls, kernel="se")
    r = gp.score(Xs, dense=True)
    lib, dev = gp.lib, gp.device
    N, M, d, Np = 300, 4096, 8, gp.Np
    f64 = dict(dtype=torch.float64, device=dev)
    Xd, yd, Xsd = gp._dev(X), gp._dev(y), gp._dev(Xs)
    K, U, alpha = torch.empty((Np, Np), **f64), torch.empty((Np, Np), **f64), torch.empty(Np, **f64)
    info = torch.zeros(1, dtype=torch.int32, device=dev)
    res = torch.zeros(4, dtype=torch.int64, device=dev)
    mu, sig, acq = (torch.empty(M, **f64) for _ in range(3))
    wf = int(lib.gpbo_factorise_workspace_bytes(Np))
    wp = int(lib.gpbo_posterior_workspace_bytes(Np, 1024, M))
    work = torch.empty((max(wf, wp) + 7) // 8, **f64)
    lsp = np.ascontiguousarray(ls, dtype=np.float64)
    p = lambda t: C.c_void_p(t.data_ptr())   # noqa: E731
    st = gp._stream()
    _lib.check(lib.gpbo_factorise_f64(p(Xd), p(yd), N, d, lsp.ctypes.data_as(C.c_void_p), 1e-4, 1e-6, Np, p(K), p(U), p(alpha),
                                      p(info), p(work), wf, st), "gpbo_factorise_f64")
    _lib.check(lib.gpbo_posterior_acq_f64(p(Xsd), M, p(Xd), N, Np, d, lsp.ctypes.data_as(C.c_void_p), p(U), p(alpha),
                                          (1.0 + 1e-4) + 1e-6, 0, 4.0, 0.0, 0.0, 0, 1024, p(mu), p(sig), p(acq), p(res), p(work),
                                          wp, None, st), "gpbo_posterior_acq_f64")
    torch.cuda.synchronize()
    assert int(info.item()) == 0
    assert bool((K == gp.K).all()) and bool((U == gp.U).all()) and bool((alpha == gp.alpha).all())
    assert bool((mu == r.mu).all()) and bool((sig == r.sigma).all()) and bool((acq == r.acq).all())
    v, i, n = gp.read_result(res)
    assert (v, i, n) == (r.best_val, r.best_idx, r.nan_count)
    # ... and the default keeps it: no kernel argument at all
    r0 = DeviceGP(chunk=1024).factorise(X, y, ls).score(Xs, dense=True)
    assert bool((r0.acq == r.acq).all()) and r0.best_idx == r.best_idx


@pytest.mark.parametrize("family", FAMILIES)
def test_chunk_invariance(family):
    X, y, Xs, ls = make_problem(129, 4096, 3)
    a = DeviceGP(chunk=512).factorise(X, y, ls, kernel=family).score(Xs, dense=True)
    b = DeviceGP(chunk=4096).factorise(X, y, ls, kernel=family).score(Xs, dense=True)
    for name in ("mu", "sigma", "acq"):
        assert bool((getattr(a, name) == getattr(b, name)).all()), name
    assert a.best_idx == b.best_idx and a.best_val == b.best_val


# ---- failures ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("family", FAMILIES)
def test_failures_are_reported(family):
    X, y, Xs, ls = make_problem(20, 600, 3)
    Xs = Xs.copy()
    Xs[17, 1] = np.nan
    gp = DeviceGP(chunk=512).factorise(X, y, ls, kernel=family)
    r = gp.score(Xs, dense=True)
    acq = r.acq.cpu().numpy()
    assert r.nan_count == 1 and np.isnan(acq[17]) and r.best_idx != 17 and np.all(np.isfinite(np.delete(acq, 17)))
    Xd = np.zeros((4, 2))
    Xd[:, 0] = [0.0, 0.0, 1.0, 1.0]   # duplicated rows, and a negative jitter to break definiteness
    with pytest.raises(np.linalg.LinAlgError):
        DeviceGP().factorise(Xd, np.ones(4), np.array([1.0, 1.0]), jitter1=-1e-3, jitter2=0.0, kernel=family)
    # what stays squared-exponential only says so, naming the kernel
    for call in (lambda: gp.append(X[0], 0.0), lambda: gp.score_f32(Xs), lambda: gp.score_i8(Xs), lambda: gp.score_i8c(Xs),
                 lambda: gp.score_bound(Xs), lambda: gp.score_qei(Xs[:8], np.zeros((4, 8)), 0.0), lambda: gp.select_batch(Xs, 2),
                 lambda: gp.thompson_paths(2), lambda: gp.select_thompson(Xs, 2), lambda: gp.posterior_grad(Xs[:4]),
                 lambda: gp.refine(Xs[:4], 0.0, 1.0), lambda: gp.select_refined(Xs, 4), lambda: gp.nlml_grid(X, y, ls[None]),
                 lambda: gp.state_dict(), lambda: gp.save_state("s.npz"), lambda: gp.load_state("s.npz"),
                 lambda: gp.score(Xs, diag_add=1e-4)):
        with pytest.raises(ValueError) as e:
            call()
        assert family in str(e.value)
    with pytest.raises(ValueError):
        DeviceGP().factorise(np.zeros((3, 17)), np.zeros(3), np.ones(17), kernel=family)
    with pytest.raises(ValueError):
        DeviceGP().factorise(X, y, ls, kernel="rbf")


# ---- the likelihood gradient -------------------------------------------------------------------------------------------------
def _problem(N, d):
    """The inputs of tests/test_gpu_ard_fit.py::_problem."""
    X = sobol_points(0, N, d)
    return X, rff_objective(X, ard_length_scales(d)), ard_length_scales(d)


PAIRS = [(1, 1), (2, 2), (63, 3), (64, 8), (65, 1), (127, 16), (128, 2), (129, 3), (300, 8)]


@pytest.mark.parametrize("family", FAMILIES)
@pytest.mark.parametrize("N,d", PAIRS)
def test_value_and_gradient_match_the_restatement(family, N, d):
    """The bounds of tests/test_gpu_ard_fit.py; two calls give the same bits."""
    X, y, ls = _problem(N, d)
    f, g = _gp().nlml_and_grad(X, y, ls, kernel=family)
    fr, gr, scale = MR.nlml_and_grad(X, y, ls, family, with_scale=True)
    print(f"{family} N {N} d {d}: value rel {abs(f - fr) / abs(fr):.2e}, gradient / scale "
          f"{np.max(np.abs(g - gr) / np.maximum(scale, 1e-300)):.2e}")
    assert f == pytest.approx(fr, rel=1e-10, abs=0)
    assert g.shape == (d,)
    if N == 1:
        assert np.all(g == 0.0)
    assert np.all(np.abs(g - gr) <= 1e-7 * scale), (g, gr, scale)
    f2, g2 = _gp().nlml_and_grad(X, y, ls, kernel=family)
    assert f == f2 and np.array_equal(g, g2)


@pytest.mark.parametrize("family", FAMILIES)
def test_gradient_edge_cases(family):
    X, y, ls = _problem(100, 2)
    f, g = _gp().nlml_and_grad(X, y, ls, jitter=-0.5, kernel=family)   # not positive definite: NaN everywhere
    assert np.isnan(f) and np.all(np.isnan(g))
    fh, gh = host_binding.nlml_and_grad(X, y, ls, jitter=-0.5, kernel=family)
    assert np.isnan(fh) and np.all(np.isnan(gh))
    X, y, ls = _problem(300, 3)
    f, g = _gp().nlml_and_grad(X, y, ls, kernel=family)
    fh, gh = host_binding.nlml_and_grad(X, y, ls, kernel=family)
    assert fh == pytest.approx(f, rel=1e-13, abs=0)
    np.testing.assert_allclose(gh, g, rtol=1e-12, atol=0)
    # the squared exponential through the same entry: today's bits
    assert _gp().nlml_and_grad(X, y, ls, kernel="se")[0] == _gp().nlml_and_grad(X, y, ls)[0]


# ---- the likelihood over all hyperparameters ---------------------------------------------------------------------------------
# mean and scale^2 against the restatement in np.longdouble, as the relative distances of tests/test_gpu_hyper.py.  REF_DIST: the
# float64 restatement's own largest distance over the cases below, per family and noise level (m, s2), measured on the CPU; the
# bound is ten times that.
REF_DIST = {"matern32": {1e-4: (6.72e-14, 1.50e-13), 3e-2: (2.81e-15, 6.53e-16)},
            "matern52": {1e-4: (1.77e-13, 5.47e-13), 3e-2: (1.63e-15, 1.67e-15)}}


def _dist(m, s2, ml, sl):
    return float(abs(m - ml) / max(abs(ml), np.sqrt(sl))), float(abs(s2 - sl) / sl)


@pytest.mark.parametrize("family", FAMILIES)
@pytest.mark.parametrize("noise", [1e-4, 3e-2])
@pytest.mark.parametrize("N,d", PAIRS)
def test_hyper_value_gradient_mean_and_scale_match_the_restatement(family, N, d, noise):
    X, y, ls = _problem(N, d)
    fit_scale = N > 1   # (one observation leaves no signal variance to profile: NaN, as tests/test_gpu_hyper.py checks)
    f, g, m, s2 = _gp().nlml_hyper(X, y, ls, noise, True, fit_scale, kernel=family)
    fr, gr, mr, s2r, scale = MR.nlml_hyper(X, y, ls, noise, family, True, fit_scale, with_scale=True)
    assert g.shape == (d + 1,)
    assert f == pytest.approx(fr, rel=1e-10, abs=0)
    assert np.all(np.abs(g - gr) <= 1e-7 * scale), (g, gr, scale)
    ml, sl = MR.mean_scale_longdouble(X, y, ls, noise, family, True, fit_scale)
    dm, ds = _dist(m, s2, ml, sl)
    rm, rs = _dist(mr, s2r, ml, sl)
    print(f"{family} N {N} d {d} noise {noise}: value rel {abs(f - fr) / abs(fr):.2e}, gradient / scale "
          f"{np.max(np.abs(g - gr) / np.maximum(scale, 1e-300)):.2e}; from longdouble: m device {dm:.2e} restatement {rm:.2e}, s2 device {ds:.2e} "
          f"restatement {rs:.2e}")
    if not fit_scale:
        assert s2 == 1.0
    assert dm <= 10 * REF_DIST[family][noise][0] and ds <= 10 * REF_DIST[family][noise][1], (dm, ds, rm, rs)
    r2 = _gp().nlml_hyper(X, y, ls, noise, True, fit_scale, kernel=family)
    assert r2[0] == f and np.array_equal(r2[1], g) and r2[2:] == (m, s2)


@pytest.mark.parametrize("family", FAMILIES)
def test_hyper_host_entry_matches_the_device_entry(family):
    X, y, ls = _problem(300, 3)
    f, g, m, s2 = _gp().nlml_hyper(X, y, ls, 3e-2, kernel=family)
    fh, gh, mh, s2h = host_binding.nlml_hyper(X, y, ls, 3e-2, kernel=family)
    assert fh == pytest.approx(f, rel=1e-13, abs=0)
    np.testing.assert_allclose(gh, g, rtol=1e-12, atol=0)
    np.testing.assert_allclose([mh, s2h], [m, s2], rtol=1e-12, atol=0)


# ---- the device fit ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("family", FAMILIES)
@pytest.mark.parametrize("seed", MR.FIT_SEEDS)
def test_device_fit_follows_the_cpu_optimiser(family, seed):
    """Seeds by the criterion of tests/test_gpu_ard_fit.py (checked on the CPU in tests/test_matern_ref_cpu.py)."""
    X, y = MR.gp_problem(seed, 200, 3, family, noise=0.01)
    cpu = fit_length_scales(lambda ls: MR.nlml_and_grad(X, y, ls, family), **MR.FIT_BOX)
    dev = _gp().fit_length_scales(X, y, kernel=family, **MR.FIT_BOX)
    print(f"{family} seed {seed}: nlml rel {abs(dev.nlml / cpu.nlml - 1):.2e}, ls rel {np.max(np.abs(dev.ls / cpu.ls - 1)):.2e}, "
          f"evaluations {dev.n_eval} / {cpu.n_eval}")
    assert dev.converged and cpu.converged
    assert dev.nlml == pytest.approx(cpu.nlml, rel=1e-8, abs=0)
    np.testing.assert_allclose(dev.ls, cpu.ls, rtol=1e-4)
    assert np.all(np.diff(dev.trace) <= 0.0)


# ---- the drop-in classes -------------------------------------------------------------------------------------------------------
FD = [50, 50]
AXES = [np.geomspace(0.05, 5.0, 16)] * 2


def _data():
    X, y, _, _ = make_problem(40, 1, 2)
    g = (np.arange(50) + 0.5) / 50
    return X, y, np.stack(np.meshgrid(g, g, indexing="ij"), -1).reshape(-1, 2)


def _selector(cls, **kw):
    X, y, Xs = _data()
    ps = cls(**kw)
    ps.name, ps.iteration = "T", 0
    ps.measured_pts, ps.measured_vals = X, y
    ps.feature_domain = FD
    ps.predicted_pts = Xs
    ps.length_scales = AXES
    ps.update_surrogate()
    return ps, ps.lower_confidence_bound()


@pytest.mark.parametrize("ard", ["gradient", "hyper"])
def test_point_selector_with_a_matern_kernel_end_to_end(ard):
    family = "matern52"
    X, y, Xs = _data()
    ps, idx = _selector(PointSelector, kernel=family, ard=ard)
    ls = np.asarray(ps.kernel_params).reshape(-1)
    assert ls.shape == (2,) and np.all(ls >= 0.05) and np.all(ls <= 5.0) and ps.last_fit["converged"]
    if ard == "hyper":
        rho, m, s = ps.noise, ps.y_mean, ps.y_scale
        fr = MR.nlml_hyper(X, y, ls, rho, family)
        assert ps.hyperparam_obj[-1] == pytest.approx(fr[0], rel=1e-9, abs=0)
        assert m == pytest.approx(fr[2], rel=1e-9) and s ** 2 == pytest.approx(fr[3], rel=1e-9)
        mu0, sig0 = MR.posterior(X, (y - m) / s, Xs, ls, family, rho, 0.0)
        mu, sig = m + s * mu0, s * sig0
    else:
        s = 1.0
        assert ps.hyperparam_obj[-1] == pytest.approx(MR.nlml_and_grad(X, y, ls, family)[0], rel=1e-9, abs=0)
        mu, sig = MR.posterior(X, y, Xs, ls, family)
    ys = max(1.0, float(np.max(np.abs(y))))
    print(f"{ard}: ls {ls}, noise {ps.noise}, |dmu| {np.max(np.abs(ps.mean_func.ravel() - mu)):.2e} (bound {1e-9 * ys:.2e}), "
          f"|dsigma| {np.max(np.abs(ps.cov_func.ravel() - sig)):.2e} (bound {1e-8 * s:.2e})")
    assert np.max(np.abs(ps.mean_func.ravel() - mu)) <= 1e-9 * ys          # the tolerances of tests/test_gpu_hyper.py
    assert np.max(np.abs(ps.cov_func.ravel() - sig)) <= 1e-8 * s
    assert np.max(np.abs(ps.acq_func_eval.ravel() - O.lcb(mu, sig, 4))) <= 1e-8 * ys
    assert int(np.ravel_multi_index(tuple(idx), FD)) == _first_argmax(ps.acq_func_eval.ravel())
    f_best = float(np.min(y))
    ide = ps.expected_improvement(xi=0.01)
    assert np.max(np.abs(ps.acq_func_eval.ravel() - O.expected_improvement(mu, sig, f_best, 0.01))) <= 1e-8 * ys
    assert int(np.ravel_multi_index(tuple(ide), FD)) == _first_argmax(ps.acq_func_eval.ravel())
    # every attribute works: the covariance blocks are the family's, leave-one-out follows the factorisation
    j1, j2 = (ps.noise, 0.0) if ard == "hyper" else (1e-4, 1e-6)
    np.testing.assert_allclose(ps.cov_meas, MR.gram(X, ls, family, j1, j2), rtol=0, atol=5e-15)
    np.testing.assert_allclose(ps.cov_meas_pred, MR.kernel(Xs, X, ls, family), rtol=0, atol=5e-15)
    np.testing.assert_allclose(ps.cov_pred, MR.gram(Xs, ls, family, j1, j2), rtol=0, atol=5e-15)
    mean, sd, z = ps.loo()
    assert mean.shape == sd.shape == z.shape == (40,) and np.all(np.isfinite(z)) and np.all(sd > 0)
    # the host-pointer class agrees
    ph, idh = _selector(PointSelectorHost, kernel=family, ard=ard)
    np.testing.assert_allclose(np.asarray(ph.kernel_params), np.asarray(ps.kernel_params), rtol=1e-10, atol=0)
    np.testing.assert_allclose(ph.mean_func, ps.mean_func, rtol=0, atol=1e-9 * ys)
    assert np.array_equal(idh, ps.lower_confidence_bound()) and np.array_equal(ph.expected_improvement(xi=0.01), ide)
    # the four unsupported methods raise, naming the kernel
    for sel in (ps, ph):
        for call in (lambda: sel.q_expected_improvement(), lambda: sel.select_batch(2), lambda: sel.select_thompson(2),
                     lambda: sel.refine_next()):
            with pytest.raises(ValueError) as e:
                call()
            assert family in str(e.value)


def test_point_selector_with_preset_kernel_params_and_no_quirk():
    """Preset length scales skip the search; candidates of the observations' shape carry no N == M quirk with a Matern kernel."""
    X, y, _, ls = make_problem(40, 40, 2)
    Xs = sobol_points(40, 40, 2)
    ps = PointSelector(kernel="matern32", ard="gradient")
    ps.measured_pts, ps.measured_vals, ps.feature_domain, ps.predicted_pts = X, y, [40], Xs
    ps.set_kernel_params(ls)
    ps.update_surrogate()
    mu, sig = MR.posterior(X, y, Xs, ls, "matern32")
    assert np.max(np.abs(ps.mean_func - mu)) <= 1e-10 * max(1.0, np.abs(y).max()) and np.max(np.abs(ps.cov_func - sig)) <= 1e-9
    np.testing.assert_allclose(ps.cov_meas_pred, MR.kernel(Xs, X, ls, "matern32"), rtol=0, atol=5e-15)
