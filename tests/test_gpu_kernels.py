"""Kernel-level parity on the MI355X: every C-ABI entry point of libgpbo against the CPU oracle /
NumPy-LAPACK on the same seeded inputs.  All calls go through ctypes -> libgpbo.so."""
import ctypes as C

import numpy as np
import pytest
import scipy.linalg as sla

pytestmark = pytest.mark.gpu

from bayesian_optimisation_amd import _lib  # noqa: E402
from bayesian_optimisation_amd.synthetic import make_problem  # noqa: E402
from oracle import gp_oracle as O  # noqa: E402


@pytest.fixture(scope="module")
def env():
    import torch

    assert torch.cuda.is_available(), "GPU tests need a GPU"
    lib = _lib.load()
    dev = torch.device("cuda", 0)

    class Env:
        pass

    e = Env()
    e.torch, e.lib, e.dev = torch, lib, dev
    e.stream = lambda: C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
    e.to = lambda a: torch.from_numpy(np.ascontiguousarray(a, dtype=np.float64)).to(dev)
    e.p = lambda t: C.c_void_p(t.data_ptr())
    e.hp = lambda a: a.ctypes.data_as(C.c_void_p)
    return e


def _spd(n, seed, cond_jitter=1e-2):
    rng = np.random.default_rng(seed)
    A = rng.standard_normal((n, n))
    return A @ A.T / n + cond_jitter * np.eye(n)


@pytest.mark.parametrize("transB,batch,lower", [(0, 1, 0), (1, 1, 0), (0, 3, 0), (1, 2, 1)])
def test_gemm_f64(env, transB, batch, lower):
    t, lib = env.torch, env.lib
    rng = np.random.default_rng(5)
    M, N, K = 192, 128, 80
    if lower:
        N = M
    A = rng.standard_normal((batch, M, K))
    B = rng.standard_normal((batch, N, K) if transB else (batch, K, N))
    Cm = rng.standard_normal((batch, M, N))
    dA, dB, dC = env.to(A), env.to(B), env.to(Cm)
    alpha, beta = -0.75, 0.5
    st = lib.gpbo_gemm_f64(transB, M, N, K, alpha, env.p(dA), K, M * K, env.p(dB), (K if transB else N),
                           B.shape[1] * B.shape[2], beta, env.p(dC), N, M * N, batch, lower, env.stream())
    assert st == 0
    got = dC.cpu().numpy()
    ref = alpha * (A @ (B.transpose(0, 2, 1) if transB else B)) + beta * Cm
    if lower:
        mask = np.kron(np.tril(np.ones((M // 64, N // 64))), np.ones((64, 64))).astype(bool)
        assert np.array_equal(got[:, ~mask], Cm[:, ~mask])  # skipped tiles untouched
        np.testing.assert_allclose(got[:, mask], ref[:, mask], rtol=0, atol=1e-12)
    else:
        np.testing.assert_allclose(got, ref, rtol=0, atol=1e-12)


@pytest.mark.parametrize("N,d", [(1, 1), (37, 2), (100, 3), (256, 8), (300, 16)])
def test_kxx(env, N, d):
    t, lib = env.torch, env.lib
    rng = np.random.default_rng(N)
    X = rng.uniform(0, 1, (N, d))
    ls = np.geomspace(0.2, 2.0, d)
    Np = int(lib.gpbo_padded_n(N))
    K = t.full((Np, Np), 7.0, dtype=t.float64, device=env.dev)
    dX = env.to(X)
    assert lib.gpbo_kxx_f64(env.p(dX), N, d, env.hp(ls), 1e-4, 1e-6, env.p(K), Np, env.stream()) == 0
    got = K.cpu().numpy()
    ref = O.kernel_rbf(X, X, ls) + 1e-6 * np.eye(N)
    np.testing.assert_allclose(got[:N, :N], ref, rtol=0, atol=5e-15)
    assert np.array_equal(np.diag(got[:N, :N]), np.full(N, O.PRIOR_VAR))  # (1 + 1e-4) + 1e-6 exactly
    pad = got.copy()
    pad[:N, :N] = 0
    expect = np.zeros_like(pad)
    expect[np.arange(N, Np), np.arange(N, Np)] = 1.0
    assert np.array_equal(pad, expect)


# >= 4096: two block columns per trailing update;  192: the second level of the inverse is the ragged pair alone (no full pair)
@pytest.mark.parametrize("n", [128, 192, 256, 384, 640, 1024, 4096, 4288])
def test_potrf_trtri_alpha(env, n):
    t, lib = env.torch, env.lib
    A = _spd(n, n)
    y = np.random.default_rng(1).standard_normal(n - 5)
    N = n - 5  # last 5 rows/cols play the identity padding
    A[N:, :] = 0
    A[:, N:] = 0
    A[np.arange(N, n), np.arange(N, n)] = 1.0
    dA = env.to(A)
    dinv = t.empty((n // 64, 64, 64), dtype=t.float64, device=env.dev)
    info = t.ones(1, dtype=t.int32, device=env.dev)
    assert lib.gpbo_potrf_f64(env.p(dA), n, env.p(dinv), env.p(info), env.stream()) == 0
    assert int(info.item()) == 0
    L = np.tril(dA.cpu().numpy())
    Lref = np.linalg.cholesky(A)
    np.testing.assert_allclose(L, Lref, rtol=0, atol=1e-12)
    for j in range(n // 64):
        blk = Lref[j * 64:(j + 1) * 64, j * 64:(j + 1) * 64]
        np.testing.assert_allclose(dinv[j].cpu().numpy() @ blk, np.eye(64), rtol=0, atol=1e-11)
    U = t.empty((n, n), dtype=t.float64, device=env.dev)
    work = t.empty((n, n), dtype=t.float64, device=env.dev)
    Ld = env.to(L)
    assert lib.gpbo_trtri_f64(env.p(Ld), env.p(dinv), n, env.p(U), env.p(work), env.stream()) == 0
    Ug = U.cpu().numpy()
    Uref = sla.solve_triangular(Lref, np.eye(n), lower=True).T
    scale = np.abs(Uref).max()
    np.testing.assert_allclose(Ug, Uref, rtol=0, atol=1e-11 * scale)
    assert np.array_equal(np.tril(Ug, -1), np.zeros((n, n)))
    tmp = t.empty(n, dtype=t.float64, device=env.dev)
    alpha = t.full((n,), 3.0, dtype=t.float64, device=env.dev)
    dy = env.to(y)
    assert lib.gpbo_alpha_f64(env.p(U), env.p(dy), N, n, env.p(tmp), env.p(alpha), env.stream()) == 0
    aref = sla.cho_solve((Lref[:N, :N], True), y)
    got = alpha.cpu().numpy()
    np.testing.assert_allclose(got[:N], aref, rtol=0, atol=1e-10 * np.abs(aref).max())
    assert np.array_equal(got[N:], np.zeros(n - N))


def test_potrf_reports_non_positive_definite(env):
    t, lib = env.torch, env.lib
    n = 256
    A = _spd(n, 3)
    A[150, 150] = -1.0
    dA = env.to(A)
    dinv = t.empty((n // 64, 64, 64), dtype=t.float64, device=env.dev)
    info = t.zeros(1, dtype=t.int32, device=env.dev)
    assert lib.gpbo_potrf_f64(env.p(dA), n, env.p(dinv), env.p(info), env.stream()) == 0
    assert int(info.item()) == 151  # LAPACK convention: 1-based column of the failing pivot


@pytest.mark.parametrize("N,M,d", [(5, 50, 1), (32, 1000, 2), (200, 1300, 8), (130, 700, 16)])
def test_kstar_mu(env, N, M, d):
    t, lib = env.torch, env.lib
    rng = np.random.default_rng(N + M)
    X = rng.uniform(0, 1, (N, d))
    Xs = rng.uniform(0, 1, (M, d))
    Xs[3] = X[min(2, N - 1)]  # a candidate that coincides with an observed point
    ls = np.geomspace(0.3, 1.5, d)
    Np = int(lib.gpbo_padded_n(N))
    alpha = np.zeros(Np)
    alpha[:N] = rng.standard_normal(N)
    ldk = (M + 511) // 512 * 512
    kst = t.full((Np, ldk), np.nan, dtype=t.float64, device=env.dev)
    mup = t.full((Np // 64, ldk), np.nan, dtype=t.float64, device=env.dev)
    dXs, dX, dal = env.to(Xs), env.to(X), env.to(alpha)  # keep the device buffers alive across the call
    dXsc = t.full((Np, d), np.nan, dtype=t.float64, device=env.dev)
    assert lib.gpbo_scale_points_f64(env.p(dX), N, Np, d, env.hp(ls), env.p(dXsc), env.stream()) == 0
    xsc = dXsc.cpu().numpy()
    np.testing.assert_allclose(xsc[:N], X / (ls * np.sqrt(2.0)), rtol=5e-16, atol=0)
    assert np.array_equal(xsc[N:], np.zeros((Np - N, d)))
    st = lib.gpbo_kstar_mu_f64(env.p(dXs), M, env.p(dXsc), N, Np, d, env.hp(ls), env.p(dal),
                               0.0, 0, env.p(kst), ldk, env.p(mup), env.stream())
    assert st == 0
    got = kst.cpu().numpy()
    ref = O.kernel_rbf(X, Xs, ls)
    np.testing.assert_allclose(got[:N, :M], ref, rtol=0, atol=5e-15)
    assert got[min(2, N - 1), 3] == 1.0
    assert np.array_equal(got[N:, :ldk], np.zeros((Np - N, ldk)))
    assert np.isfinite(got).all()
    mu = mup.cpu().numpy().sum(0)[:M]
    np.testing.assert_allclose(mu, ref.T @ alpha[:N], rtol=0, atol=1e-13 * max(1.0, np.abs(alpha).sum()))


def test_nlml_grid_matches_golden(env, golden):
    from bayesian_optimisation_amd import DeviceGP

    gp = DeviceGP()
    for name in ["g1_m32", "g4_ard_n2", "g2_n5_a", "g2_n20_tr", "g2_n12_a"]:
        g = golden(name)
        lsg = g["length_scales"]
        if lsg.ndim == 2:
            cells = np.stack(np.meshgrid(lsg[0], lsg[1], indexing="ij"), -1).reshape(-1, 2)
        else:
            cells = lsg.reshape(-1, 1)
        out = gp.nlml_grid(g["X"], g["y"], cells).reshape(g["nlogml"].shape)
        assert out.dtype == np.float32
        np.testing.assert_allclose(out, g["nlogml"], rtol=2e-6, atol=0)
        assert np.array_equal(np.argwhere(out == out.min())[0], np.argwhere(g["nlogml"] == g["nlogml"].min())[0])


def test_nlml_grid_det_underflow_like_reference(env):
    """N = 120, tiny length scale cells: det underflows in the reference -> -inf; large ones stay finite."""
    from bayesian_optimisation_amd import DeviceGP

    X, y, _, _ = make_problem(120, 8, 2)
    cells = np.array([[0.01, 0.01], [5.0, 5.0], [0.3, 0.3]])
    ref = O.nlml_grid(X, y, [np.array([0.01, 5.0, 0.3]), np.array([0.01, 5.0, 0.3])])
    out = DeviceGP().nlml_grid(X, y, cells)
    for k in range(3):
        r = ref[k, k]
        if np.isfinite(r):
            assert abs(out[k] - r) <= 1e-5 * abs(r) + 1e-3
        else:
            assert out[k] == r or (np.isnan(r) and np.isnan(out[k]))


@pytest.mark.parametrize("N", [129, 150, 176, 177, 230])
def test_nlml_grid_large_n(env, N):
    """In-LDS kernel up to N = 64 by default (it can go to 176), the batched blocked Cholesky beyond.  Same float32
    values / -inf pattern as the reference's formula on both routes."""
    from bayesian_optimisation_amd import DeviceGP

    X, y, _, _ = make_problem(N, 8, 2)
    a1, a2 = np.array([0.02, 0.3, 4.0]), np.array([0.05, 0.5])
    cells = np.stack(np.meshgrid(a1, a2, indexing="ij"), -1).reshape(-1, 2)
    ref = O.nlml_grid(X, y, [a1, a2]).ravel()
    out = DeviceGP().nlml_grid(X, y, cells)
    assert out.dtype == np.float32 and out.shape == ref.shape
    for o, r in zip(out, ref):
        if np.isfinite(r):
            assert abs(o - r) <= 1e-5 * abs(r) + 1e-3
        else:
            assert (np.isnan(r) and np.isnan(o)) or o == r


def _nlml_direct(gp, X, y, cells, batched):
    """The two grid entry points called directly (DeviceGP.nlml_grid picks by N)."""
    import ctypes as C

    torch = gp.torch
    Xd, yd, cd = gp._dev(X), gp._dev(y), gp._dev(cells)
    N, d, G = X.shape[0], X.shape[1], cells.shape[0]
    out = torch.empty(G, dtype=torch.float32, device=gp.device)
    if batched:
        need = int(gp.lib.gpbo_nlml_grid_batched_workspace_bytes(N, G))
        work = torch.empty(need // 8 + 1, dtype=torch.float64, device=gp.device)
        st = gp.lib.gpbo_nlml_grid_batched_f64(gp._ptr(Xd), gp._ptr(yd), N, d, gp._ptr(cd), G, 1e-4, gp._ptr(out),
                                               gp._ptr(work), need, gp._stream())
    else:
        st = gp.lib.gpbo_nlml_grid_f64(gp._ptr(Xd), gp._ptr(yd), N, d, gp._ptr(cd), G, 1e-4, gp._ptr(out), gp._stream())
    assert st == 0
    return out.cpu().numpy()


@pytest.mark.parametrize("N,d", [(2, 2), (63, 1), (64, 3), (65, 2), (150, 8), (176, 2)])
def test_nlml_batched_cholesky_agrees_with_the_in_lds_kernel(env, N, d):
    """Same cells through both routes (the batched blocked Cholesky takes over above N = 176): float32 values equal to
    rounding, identical first minimum."""
    from bayesian_optimisation_amd import DeviceGP

    X, y, _, _ = make_problem(N, 8, d)
    rng = np.random.default_rng(N)
    cells = np.exp(rng.uniform(np.log(0.02), np.log(3.0), size=(70, d)))
    gp = DeviceGP()
    a, b = _nlml_direct(gp, X, y, cells, batched=False), _nlml_direct(gp, X, y, cells, batched=True)
    fin = np.isfinite(a)
    assert np.array_equal(fin, np.isfinite(b)) and np.array_equal(a[~fin], b[~fin], equal_nan=True)
    np.testing.assert_allclose(b[fin], a[fin], rtol=3e-6, atol=1e-4)


def _nlml_wave(gp, X, y, cells, jitter=1e-4):
    torch = gp.torch
    Xd, yd, cd = gp._dev(X), gp._dev(y), gp._dev(cells)
    out = torch.empty(cells.shape[0], dtype=torch.float32, device=gp.device)
    st = gp.lib.gpbo_nlml_grid_wave_f64(gp._ptr(Xd), gp._ptr(yd), X.shape[0], X.shape[1], gp._ptr(cd), cells.shape[0], jitter,
                                        gp._ptr(out), gp._stream())
    assert st == 0
    return out.cpu().numpy()


@pytest.mark.parametrize("N", [1, 2, 3, 7, 15, 16, 17, 24, 31, 32, 33, 40, 47, 48, 49, 57, 63, 64])
@pytest.mark.parametrize("d", [1, 2, 3, 5, 8, 11, 16])
def test_nlml_wave_kernel_vs_oracle_and_the_in_lds_kernel(env, N, d):
    """The wave-per-cell kernel of the reference's own sizes (csrc/ard_wave.hip, N <= 64): the reference's formula (oracle
    nlml_cells: inv + det) to float32 rounding, the in-LDS kernel's values, the same first minimum, the log-det mode against
    the oracle's Cholesky form; every template instance (16 / 32 / 48 / 64 rows x 2 / 4 / 8 / 16 features), cell counts that do
    not fill the last workgroup."""
    from bayesian_optimisation_amd import DeviceGP

    X, y, _, _ = make_problem(N, 8, d)
    rng = np.random.default_rng(100 * N + d)
    G = int(rng.integers(1, 400))
    cells = np.exp(rng.uniform(np.log(0.05), np.log(5.0), size=(G, d)))
    gp = DeviceGP()
    w = _nlml_wave(gp, X, y, cells)
    a = _nlml_direct(gp, X, y, cells, batched=False)
    ref = O.nlml_cells(X, y, cells)
    assert w.dtype == np.float32 and np.isfinite(w).all() and np.isfinite(ref).all()
    np.testing.assert_allclose(w, ref, rtol=3e-6, atol=1e-5)
    np.testing.assert_allclose(w, a, rtol=3e-6, atol=1e-5)
    if G == 1 or np.ptp(np.sort(ref)[:2]) > 1e-4 * max(1.0, abs(ref.min())):
        assert int(np.argmin(w)) == int(np.argmin(ref))
    # DeviceGP routes these sizes to it, in both likelihood modes
    np.testing.assert_array_equal(gp.nlml_grid(X, y, cells), w)
    ld = gp.nlml_grid(X, y, cells, likelihood="logdet")
    want = O.nlml_cells_logdet(X, y, cells)
    assert ld.dtype == np.float64
    np.testing.assert_allclose(ld, want, rtol=1e-10, atol=1e-9 * N)


def test_nlml_wave_kernel_edge_cases(env):
    """A pivot that is not positive gives NaN (the reference's log(det < 0)), NaN observations give NaN, and 2,600 cells that
    are 200 copies of 13 give the bits of the first copy."""
    from bayesian_optimisation_amd import DeviceGP

    gp = DeviceGP()
    rng = np.random.default_rng(5)
    X = rng.uniform(0, 1, (20, 3))
    y = rng.standard_normal(20)
    cells = np.array([[0.5, 0.5, 0.5], [2.0, 1.0, 3.0]])
    assert np.isnan(_nlml_wave(gp, X, y, cells, jitter=-2.0)).all()      # K - 2 I: the first pivot is -1
    assert np.isfinite(_nlml_wave(gp, X, y, cells)).all()
    Xn = rng.uniform(0, 1, (12, 2))
    yn = rng.standard_normal(12)
    yn[5] = np.nan
    assert np.isnan(_nlml_wave(gp, Xn, yn, np.array([[0.3, 0.3]]))).all()
    Xd_ = 0.5 + 0.02 * rng.standard_normal((32, 16))
    yd_ = 0.1 * rng.standard_normal(32)
    base = np.exp(rng.uniform(np.log(0.02), np.log(20.0), size=(13, 16)))
    for rep in range(3):
        o = _nlml_wave(gp, Xd_, yd_, np.tile(base, (200, 1))).reshape(200, 13)
        assert np.array_equal(o, np.tile(o[0], (200, 1)), equal_nan=True), rep


@pytest.mark.parametrize("N,d,G", [(300, 2, 90), (512, 3, 64), (700, 8, 40), (1030, 2, 12)])
def test_nlml_batched_large_n_vs_oracle(env, N, d, G):
    """Beyond the LDS kernel: the reference's formula (inv + det, oracle nlml_cells) where its det is a normal number,
    its -inf where det underflows; everywhere the Cholesky form of the same quantity."""
    from bayesian_optimisation_amd import DeviceGP

    X, y, _, _ = make_problem(N, 8, d)
    rng = np.random.default_rng(N + d)
    cells = np.exp(rng.uniform(np.log(0.01), np.log(0.4), size=(G, d)))
    cells[0] = 3.0   # a smooth cell: det underflows in the reference
    out = DeviceGP().nlml_grid(X, y, cells)
    assert out.dtype == np.float32 and out.shape == (G,)
    ref = O.nlml_cells(X, y, cells)
    stable = O.nlml_cells_stable(X, y, cells)
    assert np.isneginf(out[0]) or np.isnan(out[0])
    n_fin = 0
    for o, r, s in zip(out, ref, stable):
        if np.isfinite(s):
            assert abs(o - s) <= 3e-6 * abs(s) + 1e-3
        else:
            assert o == s or (np.isnan(o) and np.isnan(s))
        if np.isfinite(r) and np.isfinite(s) and abs(r - s) <= 1e-3 * abs(s):   # LU det still accurate here
            assert abs(o - r) <= 1e-5 * abs(r) + 1e-2
            n_fin += 1
    assert n_fin >= 1
    fin = np.isfinite(stable)
    if fin.all():
        assert int(np.flatnonzero(out == out.min())[0]) == int(np.flatnonzero(stable.astype(np.float32) == stable.astype(np.float32).min())[0])


# ---- round 5: the one-launch grid (a persistent workgroup per cell) and the log-det likelihood mode ----------------------
@pytest.mark.parametrize("N,d,G", [(300, 2, 60), (512, 8, 48), (1030, 2, 12), (1030, 8, 10), (700, 5, 24)])
def test_nlml_logdet_mode_vs_oracle(env, N, d, G):
    """likelihood="logdet" (not in the reference, whose np.log(np.linalg.det(K)) is -inf at these sizes): fp64 values of
    0.5 (|L^-1 y|^2 + 2 sum log L_ii + N log 2 pi) against the oracle's Cholesky restatement, rtol 1e-10; every cell finite;
    the reference mode of the same kernel on the same cells keeps the reference's -inf pattern."""
    from bayesian_optimisation_amd import DeviceGP

    X, y, _, _ = make_problem(N, 8, d)
    rng = np.random.default_rng(N * 31 + d)
    cells = np.exp(rng.uniform(np.log(0.05), np.log(3.0), size=(G, d)))
    gp = DeviceGP()
    out = gp.nlml_grid(X, y, cells, likelihood="logdet")
    assert out.dtype == np.float64 and out.shape == (G,) and np.isfinite(out).all()
    want = O.nlml_cells_logdet(X, y, cells)
    np.testing.assert_allclose(out, want, rtol=1e-10, atol=0)
    assert int(np.argmin(out)) == int(np.argmin(want))
    ref_mode = gp.nlml_grid(X, y, cells)
    stable = O.nlml_cells_stable(X, y, cells)
    fin = np.isfinite(stable)
    assert np.array_equal(np.isfinite(ref_mode), fin)
    np.testing.assert_allclose(ref_mode[fin], stable[fin].astype(np.float32), rtol=3e-6)
    assert np.array_equal(ref_mode[~fin], stable[~fin].astype(np.float32))
    # wherever the reference's determinant is a normal number the two modes are the same quantity
    np.testing.assert_allclose(out[fin], ref_mode[fin], rtol=3e-6)


@pytest.mark.parametrize("N", [1, 2, 17, 63, 64, 65, 127, 128, 129, 191, 192, 193, 257])
@pytest.mark.parametrize("d", [1, 3, 4, 5, 9, 16])
def test_nlml_one_launch_grid_every_panel_edge_and_feature_bucket(env, N, d):
    """Ragged sizes around the 64-column panels and the 32-row blocks, every feature bucket of the kernel (2 / 4 / 8 / 16):
    the log-det mode against the oracle, the reference mode against the in-LDS kernel's route where that exists."""
    from bayesian_optimisation_amd import DeviceGP

    X, y, _, _ = make_problem(N, 8, d)
    rng = np.random.default_rng(N * 7 + d)
    cells = np.exp(rng.uniform(np.log(0.1), np.log(2.0), size=(9, d)))
    gp = DeviceGP()
    out = gp.nlml_grid(X, y, cells, likelihood="logdet")
    np.testing.assert_allclose(out, O.nlml_cells_logdet(X, y, cells), rtol=1e-10, atol=1e-11)
    b = _nlml_direct(gp, X, y, cells, batched=True)
    stable = O.nlml_cells_stable(X, y, cells)
    fin = np.isfinite(stable)
    assert np.array_equal(np.isfinite(b), fin)
    np.testing.assert_allclose(b[fin], stable[fin], rtol=3e-6, atol=1e-5)


def test_nlml_one_launch_grid_more_cells_than_workgroups(env):
    """2,600 cells on 512 persistent workgroups: every workgroup takes several cells in turn (its scratch slot, its LDS
    and its reductions are reused); cell g of the output is cell g of the input."""
    from bayesian_optimisation_amd import DeviceGP

    X, y, _, _ = make_problem(150, 8, 3)
    rng = np.random.default_rng(11)
    base = np.exp(rng.uniform(np.log(0.1), np.log(2.0), size=(13, 3)))
    cells = np.tile(base, (200, 1))
    out = DeviceGP().nlml_grid(X, y, cells, likelihood="logdet")
    want = O.nlml_cells_logdet(X, y, base)
    np.testing.assert_allclose(out.reshape(200, 13), np.tile(want, (200, 1)), rtol=1e-10)
    assert np.array_equal(out.reshape(200, 13), np.tile(out[:13], (200, 1)))     # the same cell gives the same bits anywhere


def test_nlml_logdet_mode_reports_a_failed_pivot_as_nan(env):
    """K = k(X,X) + jitter I with jitter = -0.5 is not positive definite: NaN in that cell (the reference's log of a
    negative determinant is NaN too), the cells of a second call unaffected."""
    from bayesian_optimisation_amd import DeviceGP

    X, y, _, _ = make_problem(200, 8, 2)
    cells = np.array([[0.3, 0.3], [1.0, 2.0], [0.05, 0.05]])
    gp = DeviceGP()
    bad = gp.nlml_grid(X, y, cells, jitter=-0.5, likelihood="logdet")
    assert np.isnan(bad).all()
    assert np.isnan(gp.nlml_grid(X, y, cells, jitter=-0.5)).all()
    good = gp.nlml_grid(X, y, cells, likelihood="logdet")
    np.testing.assert_allclose(good, O.nlml_cells_logdet(X, y, cells), rtol=1e-10)


def test_nlml_logdet_host_entry_point_equals_the_device_one(env):
    from bayesian_optimisation_amd import DeviceGP
    from bayesian_optimisation_amd import host_binding as H

    X, y, _, _ = make_problem(333, 8, 6)
    cells = np.exp(np.random.default_rng(2).uniform(np.log(0.1), np.log(2.0), size=(20, 6)))
    a = DeviceGP().nlml_grid(X, y, cells, likelihood="logdet")
    b = H.nlml_grid(X, y, cells, likelihood="logdet")
    assert b.dtype == np.float64 and np.array_equal(a, b)
    with pytest.raises(ValueError):
        H.nlml_grid(X, y, cells, likelihood="det")


@pytest.mark.parametrize("N,d", [(63, 16), (32, 16), (64, 9), (150, 16)])
def test_nlml_grid_is_deterministic_when_the_chip_is_full(env, N, d):
    """2,600 cells that are 200 copies of 13: every copy must give the bits of the first, in both kernels and both modes, run
    after run.  Round 5's randomised sweep (tools/fuzz_ard.py) found the in-LDS kernel returning a different value for ~2 %
    of such cells at d = 16 - hipcc had emitted the barrier at the head of its elimination loop without waiting for the wave's
    own LDS writes (gpbo_syncthreads in gpbo_internal.h); a few cells alone never showed it."""
    from bayesian_optimisation_amd import DeviceGP

    rng = np.random.default_rng(N + d)
    X = 0.5 + 0.02 * rng.standard_normal((N, d))
    y = 0.1 * rng.standard_normal(N)
    base = np.exp(rng.uniform(np.log(0.02), np.log(20.0), size=(13, d)))
    cells = np.tile(base, (200, 1))
    gp = DeviceGP()
    want = O.nlml_cells_logdet(X, y, base)
    for rep in range(3):
        for mode in ("reference", "logdet"):
            out = gp.nlml_grid(X, y, cells, likelihood=mode).reshape(200, 13)
            assert np.array_equal(out, np.tile(out[0], (200, 1)), equal_nan=True), (rep, mode, int((out != out[0]).sum()))
        np.testing.assert_allclose(out[0], want, rtol=1e-9, atol=1e-9 * N)   # (the three terms cancel: values near 0 occur)
        if N <= 176:
            a = _nlml_direct(gp, X, y, cells, batched=False).reshape(200, 13)
            assert np.array_equal(a, np.tile(a[0], (200, 1)), equal_nan=True), (rep, "in-LDS", int((a != a[0]).sum()))
