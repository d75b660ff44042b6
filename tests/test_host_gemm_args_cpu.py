"""The host check of the fp64 GEMM (csrc/gemm_f64.hip, contract in include/gpbo.h), without a GPU.

Every refusal is GPBO_ERR_ARG before anything is launched, so the pointers are dummies that are never dereferenced.  Each
case changes ONE thing of a call that satisfies every rule (tests/gemm_cases.py: BASE, the in-place BASE_ALIAS, the
triangular BASE_TRI1 / BASE_TRI2), so that a refusal cannot be credited to another rule; tests/test_gpu_gemm.py runs the same four calls on
real buffers and sees GPBO_OK, which is what makes "the other arguments are valid" more than a reading."""
import ctypes as C

import pytest

from bayesian_optimisation_amd import _lib
from gemm_cases import BASE, BASE_ALIAS, BASE_TRI1, BASE_TRI2

ERR_ARG, OK = -1, 0


@pytest.fixture(scope="module")
def call():
    lib = _lib.load()
    buf = (C.c_char * 1024)()
    base = (C.addressof(buf) + 255) & ~255   # 256-byte aligned like a device allocation; never dereferenced

    def run(args, entry="gpbo_gemm_tri_f64"):
        a = dict(args)
        A, B, Cc = base + a["a_off"], base + a["b_off"], base + a["c_off"]   # (offsets reach past buf: addresses only)
        head = (a["transB"], a["M"], a["N"], a["K"], 1.0, C.c_void_p(A), a["lda"], a["strideA"], C.c_void_p(B), a["ldb"],
                a["strideB"], 0.0, C.c_void_p(Cc), a["ldc"], a["strideC"], a["batch"], a["lower_only"])
        if entry == "gpbo_gemm_f64":
            return lib.gpbo_gemm_f64(*head, None)
        return lib.gpbo_gemm_tri_f64(*head, a["tri"], a["tile"], None)

    return run


REFUSED = {
    # the rules the launcher had
    "M % 64": dict(BASE, M=96),
    "N % 64": dict(BASE, N=160),
    "K % 16": dict(BASE, K=24),
    "K == 0 with M > 0": dict(BASE, K=0),
    "odd lda": dict(BASE, lda=41),
    "odd ldb": dict(BASE, ldb=37),
    "A offset by 8 bytes": dict(BASE, a_off=8),
    "B offset by 8 bytes": dict(BASE, b_off=BASE["b_off"] + 8),
    "batch = 65536": dict(BASE, batch=65536),
    "tri = 3": dict(BASE_TRI1, tri=3),
    "tri = -1": dict(BASE_TRI1, tri=-1),
    "tri = 1 with transB = 1": dict(BASE_TRI1, transB=1),
    "tri = 1 with K != N": dict(BASE_TRI1, K=64),
    "tri = 2 with K != M": dict(BASE_TRI2, K=64),
    # the new ones
    "lda < K": dict(BASE, lda=30),
    "ldb < K (transB = 1)": dict(BASE, ldb=30),
    "ldb < N (transB = 0)": dict(BASE_TRI1, ldb=126),
    "ldc < N": dict(BASE, ldc=190),
    "odd strideA with batch > 1": dict(BASE, strideA=128 * 40 + 5),
    "odd strideB with batch > 1": dict(BASE, strideB=192 * 36 + 3),
    "C == B": dict(BASE, c_off=BASE["b_off"]),
    "C == A with N = 192": dict(BASE, c_off=0),
    "C == A with N = 128": dict(BASE_ALIAS, N=128),
    "C == A with ldc != lda": dict(BASE_ALIAS, ldc=72),   # (row tiles of C would then lie over other row tiles of A)
    "tile = 16": dict(BASE, tile=16),
    "tile = 128": dict(BASE, tile=128),
    "tile = -32": dict(BASE, tile=-32),
    "tile = 32 in place": dict(BASE_ALIAS, tile=32),
}


@pytest.mark.parametrize("what", sorted(REFUSED))
def test_refused(call, what):
    assert call(REFUSED[what]) == ERR_ARG, what


def test_cases_differ_from_a_valid_call_in_one_respect():
    """The table above is what it says: every case is one of the four valid calls with a single field changed."""
    bases = (BASE, BASE_ALIAS, BASE_TRI1, BASE_TRI2)
    for what, case in REFUSED.items():
        assert min(sum(case[k] != b[k] for k in b) for b in bases) == 1, what


@pytest.mark.parametrize("entry", ["gpbo_gemm_f64", "gpbo_gemm_tri_f64"])
def test_the_rules_hold_for_both_exports(call, entry):
    """One shared launcher: gpbo_gemm_f64 (no tri, no tile) refuses what gpbo_gemm_tri_f64 refuses."""
    for what in ("lda < K", "ldb < K (transB = 1)", "ldc < N", "odd strideA with batch > 1", "odd strideB with batch > 1", "C == B",
                 "C == A with N = 192", "odd lda", "A offset by 8 bytes", "batch = 65536", "K % 16"):
        assert call(REFUSED[what], entry) == ERR_ARG, what


def test_empty_products_are_ok_with_null_pointers():
    lib = _lib.load()
    for M, N, batch in ((0, 64, 1), (64, 0, 1), (64, 64, 0), (0, 0, 0), (-64, 64, 1)):
        assert lib.gpbo_gemm_f64(0, M, N, 16, 1.0, None, 0, 0, None, 0, 0, 0.0, None, 0, 0, batch, 0, None) == OK
        for tile in (0, 32, 64):
            assert lib.gpbo_gemm_tri_f64(1, M, N, 16, 1.0, None, 0, 0, None, 0, 0, 0.0, None, 0, 0, batch, 0, 0, tile, None) == OK


def test_null_pointers_are_refused_when_there_is_work():
    lib = _lib.load()
    buf = (C.c_char * 1024)()
    base = (C.addressof(buf) + 255) & ~255
    pa, pb, pc = C.c_void_p(base), C.c_void_p(base + 256), C.c_void_p(base + 512)   # distinct: the alias rule is not in play
    for A, B, Cc in ((None, pb, pc), (pa, None, pc), (pa, pb, None)):
        assert lib.gpbo_gemm_tri_f64(1, 64, 64, 16, 1.0, A, 16, 0, B, 16, 0, 0.0, Cc, 64, 0, 1, 0, 0, 0, None) == ERR_ARG
