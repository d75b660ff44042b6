"""The int8-sliced variance screens (csrc/ozaki.hip: gpbo_posterior_acq_i8 and its coarse variant gpbo_posterior_acq_i8c)
against the exact integer emulation of tests/ozaki_ref.py.  "Everything after the two roundings is exact integer
arithmetic": the screen's |v|^2 is a function of its operands that the host predicts to the rounding of one fp64 sum.

Calls go to the C ABI (not DeviceGP.score_i8, whose fp64 fallback could hand back the fp64 pass's dense values), with
prior_var = 0.0, so that var_out = -|v|^2 exactly and a tiny planted column is not drowned by 1.000101.  The K* the emulator
sees is the image gpbo_kstar_mu_f64 writes for the same inputs (cov_entry.h: the same bits in both kernels).

  a  K* digit probe        U = 0.5 at (n0, n0) alone: v = T_k(c, n0) 2^-39, bit for bit
  b  U digit/scale probe   unit K* rows, one carry pattern per row of U: v = rint(U_nj 2^(46-e_j)) 2^(e_j-46), bit for bit
  c  whole products        |(-var_out) - ssq_ref| <= tol = 2^-53 ((Np + 4) ssq_ref + 12 sum_j |v_j| S_j)  (derived in
                           ozaki_ref.py; tests/test_ozaki_ref_cpu.py shows that plausible defects miss it by >= 100 tol)
  d  chunk invariance      on the planted operands, bit for bit
"""
import ctypes as C

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

import ozaki_ref as R  # noqa: E402
from bayesian_optimisation_amd import _lib  # noqa: E402

PASSES = {"i8": ("gpbo_posterior_acq_i8", False), "i8c": ("gpbo_posterior_acq_i8c", True)}
EXPLORE = 2.5   # LCB; the mean is not the subject here


@pytest.fixture(scope="module")
def env():
    import torch

    assert torch.cuda.is_available(), "GPU tests need a GPU"

    class Env:
        pass

    e = Env()
    e.torch, e.lib, e.dev = torch, _lib.load(), torch.device("cuda", 0)
    e.stream = lambda: C.c_void_p(torch.cuda.current_stream(e.dev).cuda_stream)
    e.to = lambda a: torch.from_numpy(np.ascontiguousarray(a, dtype=np.float64)).to(e.dev)
    e.nan = lambda *shape: torch.full(shape, np.nan, dtype=torch.float64, device=e.dev)
    return e


class Surrogate:
    """Device copies of one set of operands: X [N x d], alpha [Np], U [Np x Np] and the int8 image of U."""

    def __init__(self, env, X, N, Np, d, ls, alpha, U):
        t, lib = env.torch, env.lib
        assert Np == int(lib.gpbo_padded_n(N))
        self.env, self.N, self.Np, self.d = env, N, Np, d
        self.ls = np.ascontiguousarray(ls, dtype=np.float64)
        self.X = X if t.is_tensor(X) else env.to(X)
        self.alpha = alpha if t.is_tensor(alpha) else env.to(alpha)
        self.U = U if t.is_tensor(U) else env.to(U)
        assert tuple(self.U.shape) == (Np, Np) and self.alpha.numel() == Np
        need = int(lib.gpbo_prepare_i8_bytes(Np))
        assert need > 0
        self.u8 = t.empty(need, dtype=t.uint8, device=env.dev)
        assert lib.gpbo_prepare_i8(self.U, Np, self.u8, need, env.stream()) == 0

    def kstar(self, Xs):
        """(K* [M x Np], mean partials [Np / 64 x M]) of gpbo_kstar_mu_f64."""
        env, lib = self.env, self.env.lib
        M = len(Xs)
        ldk = (M + 511) // 512 * 512
        xsc, kst, mup = env.nan(self.Np, self.d), env.nan(self.Np, ldk), env.nan(self.Np // 64, ldk)
        dXs = env.to(Xs)
        assert lib.gpbo_scale_points_f64(self.X, self.N, self.Np, self.d, self.ls, xsc, env.stream()) == 0
        assert lib.gpbo_kstar_mu_f64(dXs, M, xsc, self.N, self.Np, self.d, self.ls, self.alpha, 0.0, 0, kst, ldk, mup,
                                     env.stream()) == 0
        Ks = np.ascontiguousarray(kst.cpu().numpy()[:, :M].T)
        assert np.isfinite(Ks).all() and not Ks[:, self.N:].any()
        return Ks, mup.cpu().numpy()[:, :M]

    def screen(self, which, Xs, chunk):
        """dict(mu, sigma, acq, var) of one pass with prior_var = 0.0 and LCB."""
        env, t, lib = self.env, self.env.torch, self.env.lib
        M = len(Xs)
        need = int(lib.gpbo_posterior_workspace_bytes_i8(self.Np, chunk, M))
        assert need > 0
        work = t.empty(need, dtype=t.uint8, device=env.dev)
        result = t.zeros(4, dtype=t.int64, device=env.dev)
        out = {k: env.nan(M) for k in ("mu", "sigma", "acq", "var")}
        dXs = env.to(Xs)
        st = getattr(lib, PASSES[which][0])(dXs, M, self.X, self.N, self.Np, self.d, self.ls, self.u8, self.alpha, 0.0,
                                            _lib.ACQ_LCB, EXPLORE, 0.0, 0, chunk, out["mu"], out["sigma"], out["acq"],
                                            out["var"], result, work, need, None, env.stream())
        assert st == 0
        out = {k: v.cpu().numpy() for k, v in out.items()}
        assert int(result.cpu().numpy()[2]) == 0   # nan_count
        return out


def _probe(env, p):
    alpha = np.zeros(p["Np"])
    alpha[:p["N"]] = np.random.default_rng(p["Np"]).standard_normal(p["N"])
    return Surrogate(env, p["X"], p["N"], p["Np"], p["d"], p["ls"], alpha, p["U"])


# ---- a: K* digits ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n0", R.PROBE_A_ROWS)
def test_kstar_digit_probe(env, n0):
    """Rows n0 cover every lane group, k half and k block of the fragment layout and the last real row; 600 candidates in
    chunks of 512 leave a ragged 128-row and 256-row tile.  No tolerance: every partial sum of the chain is exact."""
    p = R.probe_a(n0)
    g = _probe(env, p)
    Ks, _ = g.kstar(p["Xs"])
    k = Ks[:, n0]
    assert (k == 1.0).any() and (k == 0.0).any() and ((k > 0.0) & (k < 2.0 ** -39)).any() and ((k > 0.5) & (k < 1.0)).any()
    Tk = np.rint(k * 2.0 ** 38)
    full = g.screen("i8", p["Xs"], 512)
    assert np.array_equal(-full["var"], (Tk * 2.0 ** -39) ** 2)
    D = R.digits(Tk.astype(np.int64), R.NK)
    coarse = g.screen("i8c", p["Xs"], 512)
    assert np.array_equal(-coarse["var"], ((D[0] * 2.0 ** 32 + D[1] * 2.0 ** 24 + D[2] * 2.0 ** 16) * 2.0 ** -39) ** 2)


# ---- b: U digits and column scales ------------------------------------------------------------------------------------
@pytest.mark.parametrize("Np", [128, 256])
@pytest.mark.parametrize("shift", R.PROBE_B_SHIFTS)
def test_u_digit_and_column_scale_probe(env, Np, shift):
    p = R.probe_b(Np, shift)
    g = _probe(env, p)
    N, M = p["N"], p["M"]
    Ks, _ = g.kstar(p["Xs"])
    unit = np.zeros((M, Np))
    unit[np.arange(M), np.arange(M) % N] = 1.0
    assert np.array_equal(Ks, unit)   # k == 1.0 once, exact zeros elsewhere (t > 708 is flushed)
    Tu, e = R.quantise_u(p["U"])
    Du = R.digits(Tu, R.NU)
    T3 = Du[0] * 2.0 ** 40 + Du[1] * 2.0 ** 32 + Du[2] * 2.0 ** 24   # what the coarse pass keeps of T_u
    rows = np.arange(M) % N
    on_pin_row = rows == 0
    for which, T in (("i8", Tu.astype(np.float64)), ("i8c", T3)):
        vals = T * 2.0 ** (e - R.U_BITS)[None, :]
        assert np.all(np.count_nonzero(vals[1:], axis=1) <= 1)
        expect = (vals ** 2).sum(axis=1)[rows]   # rows n >= 1: one squared value (or none), nothing to round
        got = -g.screen(which, p["Xs"], 512)["var"]
        assert np.array_equal(got[~on_pin_row], expect[~on_pin_row])
        ref = R.emulate(Ks[on_pin_row], p["U"], PASSES[which][1])   # row 0, the pins: a sum over all columns
        assert np.all(np.abs(got[on_pin_row] - ref["ssq"]) <= ref["tol"])


# ---- c: whole products ------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def cases(env):
    """Per case: the operands on the device, the K* image and, per pass, the emulation - computed once."""
    cache = {}

    def get(case):
        if case not in cache:
            c = R.case_inputs(case)
            if c["kind"] == "factor":
                from bayesian_optimisation_amd import DeviceGP

                gp = DeviceGP(chunk=c["chunk"]).factorise(c["X"], c["y"], c["ls"])
                assert gp.Np == c["Np"]
                g = Surrogate(env, gp.X, c["N"], c["Np"], c["d"], c["ls"], gp.alpha, gp.U)
                g.keep = gp
            else:
                g = Surrogate(env, c["X"], c["N"], c["Np"], c["d"], c["ls"], c["alpha"], c["U"])
            Ks, mup = g.kstar(c["Xs"])
            Kd, Ud, e = R.operands(Ks, g.U.cpu().numpy())
            ref = {which: R.emulate_digits(Kd, Ud, e, coarse) for which, (_, coarse) in PASSES.items()}
            cache[case] = (c, g, mup, ref)
        return cache[case]

    return get


@pytest.mark.parametrize("case", sorted(R.CASES))
@pytest.mark.parametrize("which", sorted(PASSES))
def test_whole_product_against_the_emulator(env, cases, case, which):
    """Case 4 (sixteen column blocks) is the only one that reaches the column-group launch of the full pass and
    split_finish_kernel with S = 8.  The largest error / tol of each case is printed before the assertion."""
    c, g, mup, ref = cases(case)
    r = ref[which]
    out = g.screen(which, c["Xs"], c["chunk"])
    err = np.abs(-out["var"] - r["ssq"])
    worst = int(np.argmax(err / r["tol"]))
    print(f"case {case} {which}: max error / tol = {(err / r['tol']).max():.3g} (candidate {worst}: ssq {r['ssq'][worst]:.17g}, "
          f"error {err[worst]:.3g}, tol {r['tol'][worst]:.3g}); ssq in [{r['ssq'].min():.3g}, {r['ssq'].max():.3g}]")
    assert np.all(err <= r["tol"])
    if case == 2:   # the epilogue behind the split launch
        mu = np.zeros(c["M"])
        for s in range(mup.shape[0]):
            mu = mu + mup[s]
        assert np.array_equal(out["mu"], mu)
        sig = np.sqrt(np.abs(out["var"]))
        assert np.all(np.abs(out["sigma"] - sig) <= np.spacing(sig))
        assert np.array_equal(out["acq"], EXPLORE * out["sigma"] - out["mu"])


# ---- d: chunk and tile invariance -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("which", sorted(PASSES))
def test_chunk_invariance_on_planted_operands(env, cases, which):
    c, g, _, _ = cases(2)
    a = g.screen(which, c["Xs"], 512)
    b = g.screen(which, c["Xs"], 1024)
    assert np.array_equal(a["var"], b["var"])
