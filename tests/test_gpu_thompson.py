"""Thompson sampling by pathwise posterior samples on the GPU (csrc/thompson.hip; DeviceGP.thompson_paths / thompson_score /
select_thompson, PointSelector.select_thompson, PointSelectorHost.select_thompson, gpbo_thompson_host_f64) against
tests/thompson_ref.py, the NumPy restatement in long double (the reference project has no sample paths), and against the
library's own mean.  Kernel-level tolerance: thompson_ref.bound(), derived; end to end: the project's fp64 tolerance for the
mean, 1e-9 max(1, |R|_inf), with the residual R in the place of y."""
import ctypes as C
import functools

import numpy as np
import pytest
import torch  # noqa: F401  (before the host-pointer binding initialises HIP)

pytestmark = pytest.mark.gpu

import thompson_ref as T  # noqa: E402
from bayesian_optimisation_amd import DeviceGP, PointSelector, PointSelectorHost, _lib  # noqa: E402
from bayesian_optimisation_amd import host_binding as H  # noqa: E402
from bayesian_optimisation_amd.synthetic import make_problem  # noqa: E402

DEV = "cuda:0"
OFFSET = 10 ** 9 + 7


def _t(a):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.float64)).to(DEV)


def _p(t):
    return C.c_void_p(t.data_ptr()) if t is not None else C.c_void_p(0)


def _paths_call(X, Xs, ls, omega, phase, W, V, ldf=None, idx_offset=0, dense=True):
    """gpbo_thompson_paths_f64 through ctypes.  V: None, a host [S x N] array (padded here) or a device [S x Np] tensor.
    Returns (f [S x M] or None, idx, val, nan) as host arrays; the columns of f_out beyond M must stay untouched."""
    lib = _lib.load()
    N, d = X.shape
    M, (S, F) = len(Xs), W.shape
    Np = int(lib.gpbo_padded_n(N))
    if V is not None and not isinstance(V, torch.Tensor):
        Vp = np.zeros((S, Np))
        Vp[:, :N] = V
        V = _t(Vp)
    ldf = M if ldf is None else ldf
    Xd, Xsd, om, ph, Wd = _t(X), _t(Xs), _t(omega), _t(phase), _t(W)
    lsh = np.ascontiguousarray(ls, dtype=np.float64)
    need = int(lib.gpbo_thompson_paths_workspace_bytes(Np, M, F, S))
    assert need > 0
    work = torch.empty(need // 8, dtype=torch.float64, device=DEV)
    f = torch.full((S, ldf), -777.0, dtype=torch.float64, device=DEV) if dense else None
    out = torch.zeros(3 * S, dtype=torch.int64, device=DEV)
    st = lib.gpbo_thompson_paths_f64(_p(Xsd), M, _p(Xd), N, Np, d, lsh.ctypes.data_as(C.c_void_p), _p(om), _p(ph), _p(Wd), _p(V),
                                     F, S, idx_offset, _p(f), ldf, _p(out[:S]), _p(out[S: 2 * S]), _p(out[2 * S:]), _p(work),
                                     need, None)
    assert st == 0
    torch.cuda.synchronize()
    h = out.cpu()
    fh = None
    if dense:
        fh = f.cpu().numpy()
        assert np.all(fh[:, M:] == -777.0)
        fh = fh[:, :M]
    return fh, h[:S].numpy().copy(), h[S: 2 * S].view(torch.float64).numpy().copy(), h[2 * S:].numpy().copy()


def _check_paths(what, got, fld, tol, idx_offset=0):
    """The dense output against the long-double paths, then the winners - the figures first, then the assertions."""
    f, idx, val, nan = got
    err = np.abs(f - fld).astype(np.float64)
    want, gap = T.winners(fld.astype(np.float64))
    print(f"{what}: max |f - f_ld| / tol = {np.max(err / tol):.3g} (tol up to {tol.max():.3g}), smallest winner gap "
          f"{gap.min():.3g}")
    assert np.all(err <= tol)
    assert np.all(nan == 0)
    assert np.all(gap > 2 * tol.max()), "the restatement does not decide every path of this case: change its seed"
    assert np.array_equal(idx, want + idx_offset)
    S = len(idx)
    assert np.array_equal(val, -f[np.arange(S), idx - idx_offset])   # bit for bit


# ---- the kernel against the restatement, V given ---------------------------------------------------------------------------
@pytest.mark.parametrize("case", T.KERNEL_CASES, ids=lambda c: "-".join(map(str, c)))
def test_paths_kernel_matches_the_long_double_restatement(case):
    r = T.kernel_reference(case)
    a = (r["X"], r["Xs"], r["ls"], r["omega"], r["phase"], r["W"])
    _check_paths(f"{case} V given", _paths_call(*a, r["V"], idx_offset=OFFSET), r["f"], r["tol"], OFFSET)
    # V = NULL: the prior paths alone, against feats @ W^T
    _check_paths(f"{case} V = NULL", _paths_call(*a, None), r["f_prior"], r["tol_prior"])


@pytest.mark.parametrize("case", [(129, 1025, 8, 257, 17), (5, 513, 3, 63, 2)], ids=lambda c: "-".join(map(str, c)))
def test_dense_output_with_a_leading_dimension_beyond_m_and_without_one(case):
    r = T.kernel_reference(case)
    a = (r["X"], r["Xs"], r["ls"], r["omega"], r["phase"], r["W"], r["V"])
    wide = _paths_call(*a, ldf=case[1] + 37)
    _check_paths(f"{case} ldf = M + 37", wide, r["f"], r["tol"])
    plain = _paths_call(*a)
    assert np.array_equal(wide[0], plain[0]) and np.array_equal(wide[1], plain[1]) and np.array_equal(wide[2], plain[2])
    none = _paths_call(*a, dense=False)
    assert none[0] is None and np.array_equal(none[1], plain[1]) and np.array_equal(none[2], plain[2])


def test_ties_go_to_the_lowest_index():
    """Every candidate twice (Xs stacked on itself): each winner stays below M."""
    case = (129, 1025, 8, 257, 17)
    r = T.kernel_reference(case)
    Xs2 = np.concatenate([r["Xs"], r["Xs"]])
    f, idx, val, nan = _paths_call(r["X"], Xs2, r["ls"], r["omega"], r["phase"], r["W"], r["V"])
    M = case[1]
    assert np.array_equal(f[:, :M], f[:, M:])
    want, _ = T.winners(r["f"].astype(np.float64))
    assert np.all(idx < M) and np.array_equal(idx, want) and np.all(nan == 0)


# ---- NaN -------------------------------------------------------------------------------------------------------------------
def test_a_candidate_with_a_nan_coordinate_is_counted_and_never_chosen():
    case = (129, 1025, 8, 257, 17)
    r = T.kernel_reference(case)
    want, _ = T.winners(r["f"].astype(np.float64))
    bad = int(want[0])                       # the row path 0 would choose
    Xs = r["Xs"].copy()
    Xs[bad, 3] = np.nan
    f, idx, val, nan = _paths_call(r["X"], Xs, r["ls"], r["omega"], r["phase"], r["W"], r["V"])
    assert np.all(nan == 1)
    assert np.all(np.isnan(f[:, bad])) and np.isfinite(np.delete(f, bad, axis=1)).all()
    masked = r["f"].astype(np.float64).copy()
    masked[:, bad] = np.inf
    assert np.all(idx != bad) and np.array_equal(idx, T.winners(masked)[0])
    Xs[bad, 3] = np.inf                      # an infinite coordinate is no better
    assert np.all(_paths_call(r["X"], Xs, r["ls"], r["omega"], r["phase"], r["W"], r["V"])[3] == 1)
    # all rows NaN: nothing is usable
    f, idx, val, nan = _paths_call(r["X"], np.full((3, 8), np.nan), r["ls"], r["omega"], r["phase"], r["W"], r["V"])
    assert np.all(idx == -1) and np.all(nan == 3) and np.all(np.isnan(val)) and np.all(np.isnan(f))
    # the Python layer raises, as the other acquisitions do
    X, y, _, ls = make_problem(129, 8, 8)
    gp = DeviceGP(device=DEV).factorise(X, y, ls)
    with pytest.raises(IndexError):
        gp.thompson_score(gp.thompson_paths(4, 64, 1), Xs)
    with pytest.raises(IndexError):
        gp.select_thompson(Xs, 2, n_features=64)


# ---- against the library's own mean ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("N,M,d", [(200, 3000, 8), (129, 700, 3)])
def test_one_path_without_features_and_with_alpha_is_the_mean(N, M, d):
    """S = 1, W = 0, V = alpha: the kernel entries are the fp64 path's own arithmetic, so f is the plain pass's mean within the
    bound of test_kstar_mu (another summation order)."""
    X, y, Xs, ls = make_problem(N, M, d)
    gp = DeviceGP(device=DEV).factorise(X, y, ls)
    mu = gp.score(Xs, dense=True).mu.cpu().numpy()
    omega, phase, W, _ = T.draws(d, 8, 1, N, 0)
    f, idx, val, nan = _paths_call(X, Xs, ls, omega, phase, np.zeros_like(W), gp.alpha.reshape(1, -1).contiguous())
    err = np.max(np.abs(f[0] - mu))
    bound = 1e-13 * max(1.0, float(gp.alpha.abs().sum().item()))
    print(f"N={N} M={M} d={d}: max |f - mu| = {err:.3g}, bound {bound:.3g}")
    assert err <= bound
    assert idx[0] == int(np.argmin(f[0])) and nan[0] == 0


# ---- end to end: weights + paths through DeviceGP --------------------------------------------------------------------------
E2E = [(5, 513, 3), (127, 512, 2), (129, 1025, 8), (300, 1537, 16), (700, 2048, 8)]


@functools.lru_cache(maxsize=None)
def _e2e_ref(N, M, d, F=512, S=16, seed=7):
    X, y, Xs, ls = make_problem(N, M, d)
    omega, phase, W, E = T.draws(d, F, S, N, seed)
    V = T.weights(X, y, ls, omega, phase, W, E, xp=np.longdouble)
    R = T.residual(X, y, ls, omega, phase, W, E)
    return dict(X=X, y=y, Xs=Xs, ls=ls, E=E, V=V, f=T.paths(Xs, X, ls, omega, phase, W, V, xp=np.longdouble),
                tol=1e-9 * max(1.0, float(np.abs(R).max())))


@pytest.mark.parametrize("order", ["arrival", "fps"])
@pytest.mark.parametrize("N,M,d", E2E)
def test_device_gp_paths_match_the_restatement_end_to_end(N, M, d, order):
    r = _e2e_ref(N, M, d)
    X, y, Xs, E = r["X"], r["y"], r["Xs"], r["E"]
    gp = DeviceGP(device=DEV).factorise(X, y, r["ls"], order=order)
    paths = gp.thompson_paths(16, 512, 7)
    res = gp.thompson_score(paths, Xs, dense=True)
    f = res.f.cpu().numpy()
    err = float(np.max(np.abs(f - r["f"])))
    # the interpolation identity on the device output: f_s(X_n) + kappa v_s[n] + sqrt(kappa) E[s,n] == y_n
    Xf, yf = gp.X[:N].cpu().numpy(), gp.y[:N].cpu().numpy()          # factorisation order
    p = np.arange(N) if gp.perm is None else gp.perm.cpu().numpy()
    fx = gp.thompson_score(paths, Xf, dense=True).f.cpu().numpy()
    V = paths.V.cpu().numpy()
    ident = float(np.max(np.abs(fx + T.KAPPA * V[:, :N] + np.sqrt(T.KAPPA) * E[:, p] - yf[None, :])))
    print(f"N={N} M={M} d={d} {order} (perm: {gp.perm is not None}): max |f - f_ld| = {err:.3g} (tolerance {r['tol']:.3g}), "
          f"identity {ident:.3g}")
    if order == "fps" and N >= 129:   # the ordering really permutes these problems, so the columns of E are permuted too
        assert gp.perm is not None and not np.array_equal(p, np.arange(N))
    assert err <= r["tol"]
    assert ident <= 1e-10 * r["tol"] / 1e-9
    assert np.all(V[:, N:] == 0.0)                                   # zero on the padding
    want, gap = T.winners(r["f"].astype(np.float64))
    decided = gap > 2 * r["tol"]
    assert decided.any() and np.array_equal(res.indices[decided], want[decided])
    assert np.all(res.nan_counts == 0)


def test_determinism_and_seeds():
    X, y, Xs, ls = make_problem(300, 1537, 16)
    gp = DeviceGP(device=DEV).factorise(X, y, ls)
    a = gp.thompson_score(gp.thompson_paths(16, 512, 7), Xs, dense=True)
    b = gp.thompson_score(gp.thompson_paths(16, 512, 7), Xs, dense=True)
    assert torch.equal(a.f, b.f) and np.array_equal(a.indices, b.indices) and np.array_equal(a.values, b.values)
    c = gp.thompson_score(gp.thompson_paths(16, 512, 8), Xs, dense=True)
    assert not torch.equal(a.f, c.f)
    # paths belong to one factorisation
    stale = gp.thompson_paths(4, 64, 0)
    gp.factorise(X, y, ls)
    with pytest.raises(ValueError):
        gp.thompson_score(stale, Xs)
    # select_thompson: the first q distinct winners in path order, no more than q
    s = gp.select_thompson(Xs, 4, n_features=512, seed=7)
    allp = gp.thompson_score(gp.thompson_paths(8, 512, 7), Xs)
    keep = T.first_distinct(allp.indices, 4)
    assert np.array_equal(s.indices, allp.indices[keep]) and len(set(s.indices.tolist())) == len(s.indices) <= 4
    assert s.nan_count == 0 and np.array_equal(s.values, allp.values[keep])


# ---- the classes -------------------------------------------------------------------------------------------------------------
def _selector(cls, X, y, Xs, ls, fd):
    ps = cls()
    ps.measured_pts, ps.measured_vals, ps.predicted_pts, ps.feature_domain = X, y, Xs, fd
    ps.set_kernel_params(ls)
    ps.update_surrogate()
    return ps


@functools.lru_cache(maxsize=None)
def _class_ref(N, M, d, q, F, seed):
    X, y, Xs, ls = make_problem(N, M, d)
    S = min(64, 2 * q)
    omega, phase, W, E = T.draws(d, F, S, N, seed)
    V = T.weights(X, y, ls, omega, phase, W, E, xp=np.longdouble)
    f = T.paths(Xs, X, ls, omega, phase, W, V, xp=np.longdouble).astype(np.float64)
    idx, gap = T.winners(f)
    tol = 1e-9 * max(1.0, float(np.abs(T.residual(X, y, ls, omega, phase, W, E)).max()))
    return X, y, Xs, ls, idx, bool(np.all(gap > 2 * tol))


@pytest.mark.parametrize("N,M,d,fd", [(129, 1024, 8, [64, 16]), (300, 1536, 16, [64, 24])])
def test_selector_classes_agree_with_each_other_and_the_restatement(N, M, d, fd):
    q, F, seed = 4, 512, 7
    X, y, Xs, ls, idx, decided = _class_ref(N, M, d, q, F, seed)
    assert decided, "the restatement does not decide every path of this case: change its seed"
    want = np.stack(np.unravel_index(idx[T.first_distinct(idx, q)], fd), axis=1)
    got = []
    for cls in (PointSelector, PointSelectorHost):
        ps = _selector(cls, X, y, Xs, ls, fd)
        mean0, cov0, lcb0 = ps.mean_func.copy(), ps.cov_func.copy(), ps.lower_confidence_bound()
        pts = ps.select_thompson(q, n_features=F, seed=seed)
        assert pts.dtype == np.int64 and pts.ndim == 2 and pts.shape[1] == 2 and 1 <= len(pts) <= q
        assert np.array_equal(pts, want)
        assert np.array_equal(ps.mean_func, mean0) and np.array_equal(ps.cov_func, cov0)
        assert np.array_equal(ps.lower_confidence_bound(), lcb0)
        with pytest.raises(ValueError):
            ps.select_thompson(0)
        got.append(pts)
    assert np.array_equal(got[0], got[1])


def test_c_host_entry_equals_the_device_route_bit_for_bit():
    N, M, d, F, S = 129, 1025, 8, 257, 17
    X, y, Xs, ls = make_problem(N, M, d)
    gp = DeviceGP(device=DEV).factorise(X, y, ls)
    dv = gp.thompson_score(gp.thompson_paths(S, F, 7), Xs, dense=True)
    h = H.select_thompson(X, y, ls, Xs, 8, n_paths=S, n_features=F, seed=7, dense=True)
    assert h["info"] == 0 and np.all(h["nan_counts"] == 0)
    assert np.array_equal(h["all_indices"], dv.indices) and np.array_equal(h["all_values"], dv.values)
    assert np.array_equal(h["f"], dv.f.cpu().numpy())
    keep = T.first_distinct(dv.indices, 8)
    assert np.array_equal(h["indices"], dv.indices[keep])
