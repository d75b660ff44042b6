"""The host emulation of the int8-sliced variance product (tests/ozaki_ref.py) is itself tested here, without a GPU:
its digits against the kernel's documented extraction method, its error against an extended-precision product within the
project's written bounds, and - so that the GPU comparison against it (tests/test_gpu_i8_exact.py) cannot be vacuous - the
sensitivity of that comparison's own operands to four plausible kernel defects."""
import numpy as np
import pytest

import ozaki_ref as R
from bayesian_optimisation_amd.synthetic import make_problem


@pytest.mark.parametrize("s,bits", [(R.NK, R.K_BITS), (R.NU, R.U_BITS)])
def test_digits_two_ways(s, bits):
    """The modular definition against `T + 0x80..80 byte by byte, xor 0x80 below the top digit`, in Python integers."""
    top = 2 ** bits
    vals = [t for t in R.CARRY_T if abs(t) <= top] + [top, -top, top - 1, 1 - top]
    vals += [int(t) for t in np.random.default_rng(s).integers(-top, top + 1, 100000)]
    D = np.stack(R.digits(np.array(vals, dtype=np.int64), s), axis=1)
    assert D.min() >= -128 and D.max() <= 127
    w = 256 ** np.arange(s - 1, -1, -1, dtype=np.int64)
    assert np.array_equal(D.astype(np.int64) @ w, np.array(vals, dtype=np.int64))
    byt = np.array([R.digits_bytewise(t, s) for t in vals], dtype=np.float64)
    assert np.array_equal(D, byt)
    assert R.digits_bytewise(top, s)[0] == 64 and not any(R.digits_bytewise(top, s)[1:])   # k == 1.0, |u| -> 2^e


def test_builders_are_what_they_say():
    """The planted matrices quantise back to the planted integers and exponents; the probe's special columns too."""
    for Np, seed in ((128, 31), (256, 62)):
        U, T, e = R.planted_u(Np, seed)
        Tq, eq = R.quantise_u(U)
        assert np.array_equal(Tq, T) and np.array_equal(eq, e)
        assert np.isnan(U[np.tril_indices(Np, -1)]).all() and e.min() >= -40 and e.max() <= 40
    for Np in (128, 256):
        for s in R.PROBE_B_SHIFTS:
            p = R.probe_b(Np, s)
            Tq, eq = R.quantise_u(p["U"])
            assert np.abs(Tq).max() <= 2 ** 46 and np.all(np.count_nonzero(Tq[1:], axis=1) <= 1)
            assert eq[Np - 1] == 0 and not Tq[:, Np - 1].any()
            if Np - 3 - s >= 1:
                e0 = -40 + (np.arange(Np) + s) % 81
                assert eq[Np - 2] == e0[Np - 2] + 1 and Tq[Np - 2 - s, Np - 2] == -(2 ** 45)
                assert eq[Np - 3] == e0[Np - 3] and Tq[Np - 3 - s, Np - 3] == 2 ** 46
            R.digits(Tq, R.NU)   # fits six digits (asserted inside)


@pytest.fixture(scope="module")
def benchmark_like():
    """make_problem(N, 64, 8), the first eight candidates on observations: (K*, U, extended-precision |K* U|^2)."""
    out = {}
    for N in (256, 1024):
        X, y, Xs, ls = make_problem(N, 64, 8)
        Xs = Xs.copy()
        Xs[:8] = X[:8]
        U = R.host_factor(X, y, ls)
        Ks = R.host_kstar(X, Xs, ls, R.padded(N))
        vref = Ks.astype(np.longdouble) @ U.astype(np.longdouble)
        out[N] = (Ks, U, (vref * vref).sum(axis=1))
    return out


@pytest.mark.parametrize("N", [256, 1024])
@pytest.mark.parametrize("coarse,bound", [(False, 2.5e-10), (True, 1e-3)])
def test_emulation_error_against_an_extended_precision_product(benchmark_like, N, coarse, bound):
    """Bounds: the `err_max` bound of tests/test_gpu_i8.py (full pass) and the coarse screen's 1e-3.  Measured: 4.6e-12 /
    6.7e-12 (full, N = 256 / 1024) and 8.3e-6 / 2.6e-5 (coarse)."""
    Ks, U, ref = benchmark_like[N]
    r = R.emulate(Ks, U, coarse)
    err = float(np.abs(r["ssq"].astype(np.longdouble) - ref).max())
    print(f"N={N} coarse={coarse}: max |ssq - ref| = {err:.3g}, max tol = {r['tol'].max():.3g}")
    assert err <= bound
    assert r["tol"].max() <= 1e-2 * bound   #the emulator's own uncertainty is far below what it is compared with


@pytest.fixture(scope="module")
def case_digits():
    cache = {}

    def get(case):
        if case not in cache:
            c = R.case_inputs(case, M=64 if case == 4 else None)
            U = c["U"] if c["U"] is not None else R.host_factor(c["X"], c["y"], c["ls"])
            cache[case] = R.operands(R.host_kstar(c["X"], c["Xs"], c["ls"], c["Np"]), U)
        return cache[case]

    return get


@pytest.mark.parametrize("case", sorted(R.CASES))
@pytest.mark.parametrize("coarse", [False, True])
@pytest.mark.parametrize("mutant", ["drop_last_diagonal", "abs_lowest_k_digit", "scale_exponent_plus_one"])
def test_whole_product_cases_are_sensitive(case_digits, case, coarse, mutant):
    """A condition on the operands of test_gpu_i8_exact's whole-product cases: each mutant of the emulator moves at least
    one candidate by 100 tolerances or more, so a kernel with that defect cannot pass there."""
    Kd, Ud, e = case_digits(case)
    good = R.emulate_digits(Kd, Ud, e, coarse)
    nk, nd = (3, 3) if coarse else (R.NK, 6)
    if mutant == "drop_last_diagonal":       # diagonal 5 (full), diagonal 2 (coarse)
        bad = R.emulate_digits(Kd, Ud, e, coarse, keep=set(range(nd - 1)))
    elif mutant == "abs_lowest_k_digit":     # a wrong sign handling of the lowest digit of K* the pass reads
        Km = list(Kd)
        Km[nk - 1] = np.abs(Km[nk - 1])
        bad = R.emulate_digits(Km, Ud, e, coarse)
    else:                                    # a wrong column scale on the last 128-column block
        em = e.copy()
        em[-128:] += 1
        bad = R.emulate_digits(Kd, Ud, em, coarse)
    ratio = np.abs(bad["ssq"] - good["ssq"]) / good["tol"]
    print(f"case {case} coarse={coarse} {mutant}: max |d ssq| / tol = {ratio.max():.3g}")
    assert ratio.max() >= 100.0
