"""The references of the qEI tests, checked without a GPU:

  * tests/qei_ref.py (long double) is pinned to oracle.gp_oracle.qei_mc (fp64): on every input of tests/test_gpu_qei.py that
    is compared with the long-double reference the two agree to 1e-12 (measured: at most 1.4e-14 at N <= 300);
  * every input of the GPU tests that carries a value comparison is INFORMATIVE (qei_ref.assert_informative): no compared
    batch has a reference value below 1e-6, so none of those comparisons is 0 == 0;
  * what the reference is sensitive to: dropping the off-diagonals of Sigma_b, losing one 128-column partial of V, flipping
    the sign of xi each move the reference by far more than the GPU tests' tolerance on the inputs those tests use - a
    kernel with such a fault cannot pass them."""
import numpy as np
import pytest
import scipy.linalg as sla

import qei_cases as C
import qei_ref as R
from oracle import gp_oracle as O


def _both(c, xi=None):
    xi = c.get("xi", 0.0) if xi is None else xi
    ref, lam, name = R.reference(c["X"], c["y"], c["Xs"], c["ls"], c["Z"], c["f_best"], xi)
    ora = O.qei_mc(c["X"], c["y"], c["Xs"], c["ls"], c["Z"], c["f_best"], xi)
    return ref, lam, ora


def test_assert_informative_rejects_zeros_and_nans():
    R.assert_informative(np.array([1e-6, 0.3]))
    for bad in ([0.0, 0.3], [0.3, 9.9e-7], [0.3, np.nan], []):
        with pytest.raises(AssertionError):
            R.assert_informative(np.array(bad))


@pytest.mark.parametrize("edge", C.EDGES, ids=lambda e: "N{}_M{}_d{}_S{}".format(*e[:4]))
def test_edge_inputs_longdouble_vs_oracle_and_informative(edge):
    ref, lam, ora = _both(C.edge_case(*edge))
    R.assert_informative(ref)
    assert np.max(np.abs(ref - ora)) <= 1e-12
    assert lam.min() >= 1.0e-4          # the prior's jitter bounds Sigma_b from below


def test_n1_input_longdouble_vs_oracle_and_informative():
    ref, lam, ora = _both(C.n1_case())
    R.assert_informative(ref)
    assert np.max(np.abs(ref - ora)) <= 1e-12 and lam.min() >= 1.0e-4


def test_degenerate_batches_are_positive_definite_and_informative():
    """Eight identical candidates, eight observed rows, eight candidates 1e-7 apart, 4 + 4 copies: Sigma_b keeps the prior's
    jitter 1.01e-4 as its smallest eigenvalue (never less), both references factorise it and agree."""
    c = C.degenerate_case()
    ref, lam, ora = _both(c)
    R.assert_informative(ref)
    assert np.max(np.abs(ref - ora)) <= 1e-12
    for b, kind in C.DEGENERATE.items():
        assert 1.0e-4 <= lam[b] <= 2.03e-4, (kind, lam[b])
        if kind != "observed":          # exact copies / near copies: the jitter itself
            assert abs(lam[b] - 1.01e-4) <= 1e-8, (kind, lam[b])
    assert np.delete(lam, list(C.DEGENERATE)).min() > 2.03e-4      # the planted batches ARE the extreme ones


def test_nan_test_input_is_informative():
    c = C.nan_case()
    ref, _, ora = _both(c)
    R.assert_informative(ref)
    assert np.max(np.abs(ref - ora)) <= 1e-12


def test_nan_and_tie_inputs_have_a_clear_first_and_second_maximum():
    """What the NaN and tie tests of the GPU file assume of their inputs, on the reference alone."""
    c = C.nan_case()
    top3 = np.sort(O.qei_mc(c["X"], c["y"], c["Xs"], c["ls"], c["Z"], c["f_best"]))[-3:]
    assert top3[2] - top3[1] > 1e-7 and top3[1] - top3[0] > 1e-7
    t = C.tie_case()
    assert t["top2_gap"] > 1e-7 and len(t["copies"]) >= 3
    ref = O.qei_mc(t["X"], t["y"], t["Xs"], t["ls"], t["Z"], t["f_best"])
    assert np.all(ref[t["copies"]] == ref.max()) and np.sum(ref == ref.max()) == len(t["copies"])


@pytest.mark.parametrize("N,M,d,chunk,S", C.EXISTING)
@pytest.mark.parametrize("xi", C.XIS)
def test_existing_shapes_with_the_median_incumbent_are_informative(N, M, d, chunk, S, xi):
    c = C.existing_case(N, M, d, S)
    ora = O.qei_mc(c["X"], c["y"], c["Xs"], c["ls"], c["Z"], c["f_best"], xi)
    R.assert_informative(ora)
    # ... where the incumbent the earlier tests use is not: the reason these cases exist
    if N == 300:
        assert np.sum(O.qei_mc(c["X"], c["y"], c["Xs"], c["ls"], c["Z"], float(c["y"].min())) == 0.0) > 100


def test_existing_shape_n300_longdouble_vs_oracle():
    c = C.existing_case(300, 2048, 8, 512)
    ref, _, ora = _both(c, 0.05)
    assert np.max(np.abs(ref - ora)) <= 1e-12


@pytest.mark.parametrize("what,M,n_random,seed", [("parity", 1 << 13, 48, 5), ("fullsize", 1 << 20, 256, 5)])
def test_n2048_subsamples_with_the_median_incumbent_are_informative(what, M, n_random, seed):
    """The random part of the sub-samples of test_config5_shape_qei_n2048_subsampled and
    test_config5_full_size_qei_n2048_m2e20, and of test_gpu_qei's N = 2048 case (the device's top batches, which those tests
    add, are the largest values: assert_informative sees them when the GPU test runs)."""
    c = C.n2048_case(M)
    batches = np.sort(np.random.default_rng(seed).choice(M // 8, n_random, replace=False))
    rows = C.rows_of(batches)
    f_best = C.subsample_incumbent(c, rows)
    for xi in C.XIS:
        R.assert_informative(O.qei_mc(c["X"], c["y"], c["Xs"][rows], c["ls"], c["Z"], f_best, xi))


@pytest.mark.parametrize("N", [2048, 1921])
def test_grouped_launch_subsample_is_informative(N):
    c = C.grouped_case(N)
    rows = C.rows_of(C.grouped_random_batches())
    R.assert_informative(O.qei_mc(c["X"], c["y"], c["Xs"][rows], c["ls"], c["Z"], C.subsample_incumbent(c, rows)))


@pytest.mark.parametrize("seed", C.FUZZ_SEEDS)
def test_fuzz_sample_is_informative(seed):
    c = C.fuzz_qei.draw_case(seed)
    N, d = c["X"].shape
    assert 1 <= N <= 400 and 1 <= d <= 16 and len(c["Xs"]) % 8 == 0 and len(c["Xs"]) <= 3000 and 1 <= len(c["Z"]) <= 600
    assert c["chunk"] in (512, 1024) and c["xi"] in (0.0, 0.01, 0.05) and 0.5 <= c["quantile"] <= 0.9 and len(c["planted"]) <= 3
    ref = O.qei_mc(c["X"], c["y"], c["Xs"], c["ls"], c["Z"], c["f_best"], c["xi"])
    R.assert_informative(ref)
    assert np.array_equal(ref, c["ref"])


def test_fuzz_sample_covers_the_degenerate_kinds():
    kinds = {k for s in C.FUZZ_SEEDS for _, k in C.fuzz_qei.draw_case(s)["planted"]}
    assert kinds == set(C.fuzz_qei.DEGENERATE_KINDS)


# ---- what an informative incumbent buys: deliberate errors in a restatement move the values far beyond the tolerance ------
def _qei_with_fault(c, fault, xi):
    X, y, Xs, ls, Z, f_best = (c[k] for k in ("X", "y", "Xs", "ls", "Z", "f_best"))
    _, L, alpha = O.factorise(X, y, ls)
    out = np.empty(len(Xs) // 8)
    for b in range(len(out)):
        P = Xs[b * 8:(b + 1) * 8]
        d2 = np.zeros((len(X), 8))
        for k in range(X.shape[1]):
            d2 += (X[:, k, None] - P[None, :, k]) ** 2 / ls[k] ** 2
        ksx = np.exp(-0.5 * d2)
        V = sla.solve_triangular(L, ksx, lower=True, check_finite=False)
        if fault == "partial":                      # one 128-column partial of V V^T lost: the last one
            V = V[: (len(X) - 1) // 128 * 128]
        p2 = np.zeros((8, 8))
        for k in range(X.shape[1]):
            p2 += (P[:, k, None] - P[None, :, k]) ** 2 / ls[k] ** 2
        Sig = np.exp(-0.5 * p2)
        Sig[np.arange(8), np.arange(8)] = O.PRIOR_VAR
        Sig = Sig - V.T @ V
        if fault == "offdiag":
            Sig = np.diag(np.diag(Sig))
        f = (ksx.T @ alpha)[None, :] + Z @ np.linalg.cholesky(Sig).T
        out[b] = np.mean(np.maximum(0.0, np.max(f_best - (-xi if fault == "xi_sign" else xi) - f, axis=1)))
    return out


@pytest.mark.parametrize("fault", ["offdiag", "partial", "xi_sign"])
def test_deliberate_errors_are_visible_at_the_tolerance_of_the_gpu_tests(fault):
    c = C.existing_case(300, 2048, 8, 512)
    tol = 1e-9 * max(1.0, float(np.abs(c["y"]).max()))
    good = O.qei_mc(c["X"], c["y"], c["Xs"], c["ls"], c["Z"], c["f_best"], 0.05)
    assert np.max(np.abs(_qei_with_fault(c, None, 0.05) - good)) <= 1e-12       # the restatement itself is right
    moved = np.abs(_qei_with_fault(c, fault, 0.05) - good) > tol
    assert moved.sum() >= len(good) // 2, (fault, int(moved.sum()))
    # ... and with the incumbent of the earlier tests most batches cannot see it: 0 == 0
    c0 = dict(c, f_best=float(c["y"].min()))
    good0 = O.qei_mc(c0["X"], c0["y"], c0["Xs"], c0["ls"], c0["Z"], c0["f_best"], 0.05)
    assert (np.abs(_qei_with_fault(c0, fault, 0.05) - good0) > tol).sum() < moved.sum()
