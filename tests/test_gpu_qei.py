"""The q = 8 Monte-Carlo qEI route (gpbo_posterior_qei_f64: the GRAM form of sigma_acq_kernel + qei_kernel, through
DeviceGP.score_qei) where its value is NOT zero, and at the edges of the route.

With f_best = min(y) most batches of the suite's Sobol problems have qEI exactly 0 on the device and in any reference,
whatever Sigma_b, the Gram partials or the 8 x 8 Cholesky were.  Every value comparison here therefore takes the incumbent
from the ORACLE's posterior mean (a quantile in [0.5, 0.9]) and first passes `qei_ref.assert_informative`: every compared
batch has a reference value >= 1e-6.  The inputs are built in tests/qei_cases.py; tests/test_qei_ref_cpu.py checks the same
condition on them without a GPU.  Only the tests whose subject IS the zero (all-zero acquisition, ties) are exempt.

References: tests/qei_ref.py (np.longdouble) for N <= about 300, oracle.gp_oracle.qei_mc (fp64) above.
Tolerance: the suite's for this route, 1e-9 max(1, max|y|).  Measured on an MI355X over the edge cases, the N = 1 case and the
degenerate batches (every value printed by the tests, run with -s):
    largest |device - long double| = 1.7e-13   (N = 64, M = 512, d = 3, S = 1; 8.5e-14 on the degenerate batches, <= 1.5e-14
                                                on every other case; a later tightening starts from 16 x this: another
                                                summation order, another box)
    largest |oracle - long double| = 1.4e-13   (the same case; 1.0e-13 on the degenerate batches, <= 1e-14 elsewhere)
At N = 2048 (fp64 oracle only): |device - oracle| <= 7.4e-13; grouped against ungrouped launches <= 1.3e-14.

Contracts read from the kernel and pinned here:
  * a NaN coordinate in ONE candidate makes exactly its batch NaN (dense output), counts once in nan_count, and leaves the
    arg-max to the other batches;
  * the base samples Z must be finite: a host array with a NaN is refused (ValueError); a device tensor is not checked, and
    what the kernel then computes (finite values, nan_count 0: NOT the oracle's NaN) is pinned in
    test_qei_nan_in_the_base_samples_contract, which says why;
  * the all-zero acquisition (the normal late-BO state) returns best_val 0.0 at best_idx = batch_offset + 0;
  * equal values: the lowest batch index wins, whatever the chunking."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

import qei_cases as C  # noqa: E402
import qei_ref as R  # noqa: E402
from bayesian_optimisation_amd import DeviceGP  # noqa: E402
from bayesian_optimisation_amd.synthetic import make_problem  # noqa: E402
from oracle import gp_oracle as O  # noqa: E402


def _first_argmax(a):
    return int(np.flatnonzero(a == a.max())[0])


def _tol(y):
    return 1e-9 * max(1.0, float(np.abs(y).max()))


def _score(c, chunk=512, **kw):
    gp = DeviceGP(chunk=chunk).factorise(c["X"], c["y"], c["ls"])
    kw.setdefault("xi", c.get("xi", 0.0))
    kw.setdefault("batch_offset", c.get("batch_offset", 0))
    r = gp.score_qei(c["Xs"], c["Z"], c["f_best"], dense=True, **kw)
    return r, r.acq.cpu().numpy()


def _check(r, got, ref, y, offset, what):
    """Values against an informative reference, the result record against the dense output, the reference's arg-max."""
    R.assert_informative(ref)
    err = float(np.max(np.abs(got - ref)))
    print(f"[qei] {what}: max |device - reference| = {err:.3e}, smallest reference value {ref.min():.3e}")
    assert r.nan_count == 0 and got.shape == ref.shape
    assert err <= _tol(y)
    assert r.best_idx == offset + _first_argmax(got) and r.best_val == got.max()
    top2 = np.sort(ref)[-2:] if len(ref) > 1 else np.array([-np.inf, ref[0]])
    if top2[1] - top2[0] > 1e-7:
        assert r.best_idx - offset == _first_argmax(ref)


# ---- values: the shapes of test_qei_vs_oracle and the N = 2048 sub-sample with an informative incumbent -------------------
@pytest.mark.parametrize("xi", C.XIS)
@pytest.mark.parametrize("N,M,d,chunk,S", C.EXISTING)
def test_qei_existing_shapes_informative_incumbent_vs_oracle(N, M, d, chunk, S, xi):
    c = C.existing_case(N, M, d, S)
    r, got = _score(c, chunk, xi=xi, batch_offset=5)
    _check(r, got, O.qei_mc(c["X"], c["y"], c["Xs"], c["ls"], c["Z"], c["f_best"], xi), c["y"], 5, f"N={N} xi={xi} vs oracle")


def test_qei_n300_informative_incumbent_vs_longdouble():
    c = C.existing_case(300, 2048, 8, 512)
    r, got = _score(c, 1024, xi=0.05, batch_offset=5)
    ref, _, name = R.reference(c["X"], c["y"], c["Xs"], c["ls"], c["Z"], c["f_best"], 0.05)
    _check(r, got, ref, c["y"], 5, f"N=300 xi=0.05 vs {name}")


@pytest.mark.parametrize("xi", C.XIS)
def test_qei_n2048_subsample_informative_incumbent_vs_oracle(xi):
    """BASELINE config 5's N and d: the incumbent is the oracle's median mean on the random part of the sub-sample; the
    device's top 8 are added to what is compared (they are the largest values, and assert_informative sees them too)."""
    M = 1 << 13
    c = C.n2048_case(M)
    rand = C.random_batches(M // 8, 48, 5)
    c["f_best"] = C.subsample_incumbent(c, C.rows_of(rand))
    r, got = _score(c, 1 << 12, xi=xi)
    assert r.nan_count == 0 and r.best_idx == _first_argmax(got) and r.best_val == got.max()
    batches = np.unique(np.concatenate([rand, np.argsort(got)[-8:]]))
    ref = O.qei_mc(c["X"], c["y"], c["Xs"][C.rows_of(batches)], c["ls"], c["Z"], c["f_best"], xi)
    R.assert_informative(ref)
    err = float(np.max(np.abs(got[batches] - ref)))
    print(f"[qei] N=2048 xi={xi} vs oracle: max |device - reference| = {err:.3e}, smallest reference value {ref.min():.3e}")
    assert err <= _tol(c["y"])
    top2 = np.sort(ref)[-2:]
    if top2[1] - top2[0] > 1e-7:
        assert batches[_first_argmax(ref)] == r.best_idx


# ---- edges against the long-double reference, chunk 512 -------------------------------------------------------------------
def _edge(c, what):
    ref, lam, name = R.reference(c["X"], c["y"], c["Xs"], c["ls"], c["Z"], c["f_best"], c["xi"])
    ora = O.qei_mc(c["X"], c["y"], c["Xs"], c["ls"], c["Z"], c["f_best"], c["xi"])
    print(f"[qei] {what}: max |oracle - {name}| = {float(np.max(np.abs(ora - ref))):.3e}, smallest eigenvalue {lam.min():.3e}")
    r, got = _score(c, 512)
    _check(r, got, ref, c["y"], c["batch_offset"], f"{what} vs {name}")
    return r, got


@pytest.mark.parametrize("edge", C.EDGES, ids=lambda e: "N{}_M{}_d{}_S{}".format(*e[:4]))
def test_qei_edge_shapes_vs_longdouble(edge):
    _edge(C.edge_case(*edge), "edge N={} M={} d={} S={} xi={}".format(*edge[:5]))


def test_qei_single_observation_vs_longdouble():
    _edge(C.n1_case(), "N=1")


def test_qei_refuses_d17_and_a_ragged_batch():
    X, y, Xs, ls = make_problem(20, 64, 17)
    gp = DeviceGP().factorise(X, y, ls)
    with pytest.raises(ValueError):
        gp.score_qei(Xs, O.qei_base_samples(8), 0.0)
    X, y, Xs, ls = make_problem(20, 64, 4)
    gp = DeviceGP().factorise(X, y, ls)
    for M in (63, 7, 60):
        with pytest.raises(ValueError):
            gp.score_qei(Xs[:M], O.qei_base_samples(8), 0.0)
    with pytest.raises(ValueError):
        gp.score_qei(Xs, np.zeros((8, 7)), 0.0)


# ---- degenerate batches ---------------------------------------------------------------------------------------------------
def test_qei_degenerate_batches_vs_longdouble():
    """Eight identical candidates / eight observed rows / eight candidates 1e-7 apart / 4 + 4 copies: Sigma_b is positive
    definite (its smallest eigenvalue is the prior's jitter), so no batch is NaN and the values agree."""
    c = C.degenerate_case()
    c["batch_offset"] = 0
    r, got = _edge(c, "degenerate batches")
    assert r.nan_count == 0 and np.isfinite(got[list(C.DEGENERATE)]).all()


@pytest.mark.parametrize("where", ["anywhere", "at_the_maximum"])
def test_qei_nan_coordinate_in_one_candidate(where):
    c = C.nan_case()
    ref, _, name = R.reference(c["X"], c["y"], c["Xs"], c["ls"], c["Z"], c["f_best"], 0.0)
    R.assert_informative(ref)
    order = np.argsort(ref)
    assert ref[order[-1]] - ref[order[-2]] > 1e-7 and ref[order[-2]] - ref[order[-3]] > 1e-7   # a property of the input
    b = int(order[-1]) if where == "at_the_maximum" else (37 if order[-1] != 37 else 38)
    c["Xs"][8 * b + 3, 2] = np.nan
    r, got = _score(c, 512, batch_offset=11)
    assert r.nan_count == 1 and np.flatnonzero(np.isnan(got)).tolist() == [b]
    rest = np.delete(np.arange(len(ref)), b)
    err = float(np.max(np.abs(got[rest] - ref[rest])))
    print(f"[qei] NaN candidate {where} vs {name}: max |device - reference| = {err:.3e}")
    assert err <= _tol(c["y"])
    want = int(order[-1]) if where == "anywhere" else int(order[-2])
    assert r.best_idx == 11 + want and r.best_val == got[want] == np.nanmax(got)


def test_qei_nan_in_the_base_samples_contract():
    """Z is the caller's constant and must be finite.  A host array is checked (ValueError).  A device tensor is not read
    back (score_qei_async stays without a host synchronisation), and qei_kernel does not look for a NaN in it: its maximum
    over the batch skips NaN comparisons, so a NaN z_sk leaves candidates k..7 out of sample s (row j of L_b z_s sums over
    z_s0..z_sj).  Every batch then comes back finite with nan_count == 0 - NOT the oracle's NaN.  That arithmetic is pinned
    here against the long-double reference with the same rule (skip_nan), so that a change of it is a decision, not an
    accident; DESIGN.md 1 ("qEI and NaN") has the finding and the alternative."""
    import torch

    c = C.nan_case()
    gp = DeviceGP(chunk=512).factorise(c["X"], c["y"], c["ls"])
    for s_, k in ((5, 0), (127, 7), (64, 3)):
        Z = c["Z"].copy()
        Z[s_, k] = np.nan
        with pytest.raises(ValueError):
            gp.score_qei(c["Xs"], Z, c["f_best"], dense=True)
        assert np.isnan(O.qei_mc(c["X"], c["y"], c["Xs"][:8], c["ls"], Z, c["f_best"])).all()      # the oracle's answer
        r = gp.score_qei(c["Xs"], torch.from_numpy(Z).to(gp.device), c["f_best"], dense=True)
        got = r.acq.cpu().numpy()
        if R.HAVE_LONGDOUBLE:
            ref, _ = R.qei_longdouble(c["X"], c["y"], c["Xs"], c["ls"], Z, c["f_best"], skip_nan=True)
            R.assert_informative(ref)
            err = float(np.max(np.abs(got - ref)))
            print(f"[qei] NaN base sample ({s_}, {k}) vs longdouble with the kernel's rule: max |device - reference| = {err:.3e}")
            assert err <= _tol(c["y"])
        assert r.nan_count == 0 and np.isfinite(got).all()
        assert r.best_idx == _first_argmax(got) and r.best_val == got.max()


# ---- zeros and ties (exempt from assert_informative: the zero is the subject) ----------------------------------------------
def test_qei_all_zero_acquisition_returns_the_first_batch():
    X, y, Xs, ls = make_problem(100, 1536, 6)
    gp = DeviceGP(chunk=512).factorise(X, y, ls)
    r = gp.score_qei(Xs, O.qei_base_samples(512, 8, 7), float(y.min()) - 50.0, dense=True, batch_offset=77)
    got = r.acq.cpu().numpy()
    assert got.shape == (192,) and np.array_equal(got, np.zeros(192)) and not np.signbit(got).any()
    assert r.best_val == 0.0 and r.best_idx == 77 and r.nan_count == 0
    assert gp.score_qei(Xs, O.qei_base_samples(512, 8, 7), float(y.min()) - 50.0, batch_offset=77).best_idx == 77   # not dense


def test_qei_ties_go_to_the_lowest_batch_index_whatever_the_chunk():
    c = C.tie_case()
    res = {}
    for chunk in (512, 1024):
        r, got = _score(c, chunk, batch_offset=9)
        vals = got[c["copies"]]
        assert np.all(vals == vals[0]) and vals.tobytes() == np.repeat(vals[:1], len(vals)).tobytes()   # bit-equal copies
        assert got.max() == vals[0] and r.best_val == vals[0]
        assert r.best_idx == 9 + min(c["copies"]) and r.nan_count == 0
        res[chunk] = (r.best_idx, r.best_val, got)
    assert res[512][:2] == res[1024][:2] and np.array_equal(res[512][2], res[1024][2])


# ---- the grouped Gram launch below full size --------------------------------------------------------------------------------
@pytest.mark.parametrize("N", [2048, 1921])
def test_qei_column_groups_ragged_tiles_agree_with_the_ungrouped_launch_and_the_oracle(N):
    """M = 41,224 candidates in one call (>= 32,768, Np = 2048: eight column groups per candidate tile), chunk 16,384: the last
    chunk has 34 candidate tiles, not a multiple of 8, so workgroups of the grouped launch leave through `tile_x >= ntile`.
    The same candidates in two calls below 32,768 run ungrouped.  N = 1921 is the first size that pads to Np = 2048: rows and
    columns >= N contribute nothing."""
    c = C.grouped_case(N)
    M = C.GROUPED_M
    rand = C.grouped_random_batches()
    f_best = C.subsample_incumbent(c, C.rows_of(rand))
    gp = DeviceGP(chunk=1 << 14).factorise(c["X"], c["y"], c["ls"])
    assert gp.Np == 2048
    big = gp.score_qei(c["Xs"], c["Z"], f_best, dense=True)                                     # grouped
    got = big.acq.cpu().numpy()
    h = 20608
    a = gp.score_qei(c["Xs"][:h], c["Z"], f_best, dense=True)                                   # ungrouped
    b = gp.score_qei(c["Xs"][h:], c["Z"], f_best, dense=True, batch_offset=h // 8)
    two = np.concatenate([a.acq.cpu().numpy(), b.acq.cpu().numpy()])
    assert big.nan_count == a.nan_count == b.nan_count == 0 and got.shape == two.shape == (M // 8,)
    print(f"[qei] grouped N={N}: max |grouped - ungrouped| = {float(np.max(np.abs(got - two))):.3e}")
    assert np.max(np.abs(got - two)) <= 1e-12
    assert big.best_idx == _first_argmax(got) and big.best_val == got.max()
    top2 = np.sort(got)[-2:]
    assert top2[1] - top2[0] > 1e-10            # a property of the input: the two launches cannot disagree on a near-tie
    best2 = max([(a.best_val, -a.best_idx), (b.best_val, -b.best_idx)])
    assert big.best_idx == -best2[1] and abs(big.best_val - best2[0]) <= 1e-12
    other = DeviceGP(chunk=1 << 13).factorise(c["X"], c["y"], c["ls"]).score_qei(c["Xs"], c["Z"], f_best, dense=True)
    assert np.array_equal(other.acq.cpu().numpy(), got) and (other.best_idx, other.best_val) == (big.best_idx, big.best_val)
    batches = np.unique(np.concatenate([rand, np.argsort(got)[-8:]]))
    ref = O.qei_mc(c["X"], c["y"], c["Xs"][C.rows_of(batches)], c["ls"], c["Z"], f_best)
    R.assert_informative(ref)
    err = float(np.max(np.abs(got[batches] - ref)))
    print(f"[qei] grouped N={N} vs oracle: max |device - reference| = {err:.3e}, smallest reference value {ref.min():.3e}")
    assert err <= _tol(c["y"])
    t2 = np.sort(ref)[-2:]
    if t2[1] - t2[0] > 1e-7:
        assert batches[_first_argmax(ref)] == big.best_idx


# ---- a fixed sample of the randomised sweep tools/fuzz_qei.py ---------------------------------------------------------------
@pytest.mark.parametrize("seed", C.FUZZ_SEEDS)
def test_qei_random_case_vs_oracle(seed):
    c = C.fuzz_qei.draw_case(seed)
    ref = O.qei_mc(c["X"], c["y"], c["Xs"], c["ls"], c["Z"], c["f_best"], c["xi"])
    R.assert_informative(ref)
    assert C.fuzz_qei.check_case(c, ref) == []
