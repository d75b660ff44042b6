"""The fp64 matrix-core GEMM (csrc/gemm_f64.hip) on the MI355X, directly and in both tile variants, through
gpbo_gemm_tri_f64 (ctypes -> libgpbo.so).

Exact inputs: A, B and C hold integers of [-8, 8], alpha is one of 1, -1, -0.75 and beta one of 0, 1, 0.5.  With K <= 512 every
partial sum is an integer far below 2^53 and the scalings are by dyadic numbers, so alpha * A @ op(B) + beta * C is exact in
NumPy float64 and exact on the device in any summation order: the comparison is np.array_equal, there is no tolerance.

Sentinels: every operand has a leading dimension larger than its row length, a gap between batch members and a pointer
offset into its allocation.  Everything that is not an element of a matrix holds one NaN bit pattern: a read of A's or B's
padding shows up as a NaN in C, and C's padding must come back bit for bit."""
import ctypes as C
import itertools

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

from bayesian_optimisation_amd import _lib  # noqa: E402
from gemm_cases import BASE, BASE_ALIAS, BASE_TRI1, BASE_TRI2  # noqa: E402

SENTINEL = np.uint64(0x7FF80BAD0BAD0BAD)   # a quiet NaN with a payload of its own
TAIL = 32                                   # sentinel elements behind the last row
ALPHAS, BETAS = (1.0, -1.0, -0.75), (0.0, 1.0, 0.5)


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
    e.to = lambda a: torch.from_numpy(a).to(dev)
    return e


class Operand:
    """`nb` matrices [rows x rowlen] inside one flat allocation: first element at `off`, rows `ld` apart, matrices `stride`
    apart (0: one shared matrix); everything else is SENTINEL."""

    def __init__(self, rows, rowlen, nb, pad, gap, off, shared=False, tail=TAIL):
        self.rows, self.rowlen, self.off, self.ld = rows, rowlen, off, rowlen + pad
        self.nb = 1 if shared else nb
        self.stride = 0 if shared else rows * self.ld + gap
        self.size = off + (self.nb - 1) * self.stride + rows * self.ld + tail
        self.h = np.full(self.size, SENTINEL, dtype=np.uint64).view(np.float64)

    def mats(self, flat):   # the nb matrices of a flat array of this layout, as one strided view [nb x rows x rowlen]
        assert flat.size == self.size and flat.itemsize == 8
        return np.lib.stride_tricks.as_strided(flat[self.off:], shape=(self.nb, self.rows, self.rowlen),
                                               strides=(8 * self.stride, 8 * self.ld, 8))

    def set(self, values):   # [nb x rows x rowlen]
        self.mats(self.h)[...] = values
        return self

    def payload(self, keep=True):   # which elements of the allocation belong to a matrix (and to `keep` [rows x rowlen] of it)
        m = np.zeros(self.size, dtype=np.uint64)
        self.mats(m)[...] = keep
        return m.astype(bool)

    def gather(self, flat):
        return self.mats(flat).copy()


def _ints(rng, shape):
    return rng.integers(-8, 9, size=shape).astype(np.float64)


def _launch(env, transB, M, N, K, alpha, dA, opA, dB, opB, beta, dC, opC, batch, lower, tri, tile):
    return env.lib.gpbo_gemm_tri_f64(transB, M, N, K, alpha, C.c_void_p(dA.data_ptr() + 8 * opA.off), opA.ld, opA.stride,
                                     C.c_void_p(dB.data_ptr() + 8 * opB.off), opB.ld, opB.stride, beta,
                                     C.c_void_p(dC.data_ptr() + 8 * opC.off), opC.ld, opC.stride, batch, lower, tri, tile,
                                     env.stream())


def _reference(transB, alpha, A, B, beta, Cm):
    prod = A @ (B.transpose(0, 2, 1) if transB else B)   # (a shared operand broadcasts over the batch)
    return alpha * prod + (beta * Cm if beta != 0.0 else 0.0)


def _block_lower_mask(M, N):
    return np.kron(np.tril(np.ones((M // 64, N // 64))), np.ones((64, 64))).astype(bool)


def check(env, transB, M, N, K, tile, batch=1, scalars=((-0.75, 0.5),), lower=0, tri=0, share_a=False, share_b=False, A=None, B=None,
          c_values=None, layout_c=(6, 7, 4), seed=0):
    """One set of operands, one launch per (alpha, beta); returns the device results [len(scalars) x batch x M x N]."""
    rng = np.random.default_rng([seed, M, N, K, transB, tile, batch])
    opA = Operand(M, K, batch, 6, 12, 6, share_a)
    brows, blen = (N, K) if transB else (K, N)
    opB = Operand(brows, blen, batch, 10, 20, 10, share_b)
    opC = Operand(M, N, batch, *layout_c, tail=TAIL if any(layout_c) else 0)   # (0, 0, 0): dense, nothing around it
    A = _ints(rng, (opA.nb, M, K)) if A is None else A
    B = _ints(rng, (opB.nb, brows, blen)) if B is None else B
    Cm = _ints(rng, (batch, M, N)) if c_values is None else c_values
    opA.set(A), opB.set(B), opC.set(Cm)
    dA, dB = env.to(opA.h), env.to(opB.h)
    keep = _block_lower_mask(M, N) if lower else np.ones((M, N), dtype=bool)
    written = opC.payload(keep)
    before = opC.h.view(np.uint64)
    results = []
    for alpha, beta in scalars:
        dC = env.to(opC.h)
        assert _launch(env, transB, M, N, K, alpha, dA, opA, dB, opB, beta, dC, opC, batch, lower, tri, tile) == 0
        got = dC.cpu().numpy()
        what = (transB, M, N, K, tile, batch, alpha, beta, lower, tri)
        # nothing but the tiles of C is written: padding, gaps, the words before and behind, skipped tiles - bit for bit
        assert np.array_equal(got.view(np.uint64)[~written], before[~written]), what
        g = opC.gather(got)
        ref = _reference(transB, alpha, A, B, beta, Cm)
        assert not np.isnan(g[:, keep]).any(), what       # a NaN here is a read of A's or B's padding (or of C at beta == 0)
        assert np.array_equal(g[:, keep], ref[:, keep]), what
        results.append(g)
    # the operands themselves are read only
    assert np.array_equal(dA.cpu().numpy().view(np.uint64), opA.h.view(np.uint64))
    assert np.array_equal(dB.cpu().numpy().view(np.uint64), opB.h.view(np.uint64))
    return results


ALL_SCALARS = tuple(itertools.product(ALPHAS, BETAS))


@pytest.mark.parametrize("transB", [0, 1])
@pytest.mark.parametrize("tile", [32, 64])
@pytest.mark.parametrize("M,N", [(64, 64), (192, 64), (64, 192), (128, 192)])
def test_rectangles(env, M, N, tile, transB):
    """M != N tells the column tile index from the row tile index; 192 is three tiles of 64 and six of 32.  Every alpha and beta."""
    check(env, transB, M, N, 48, tile, scalars=ALL_SCALARS)


@pytest.mark.parametrize("transB", [0, 1])
@pytest.mark.parametrize("tile", [32, 64])
@pytest.mark.parametrize("K", [16, 32, 48, 80])
def test_k_tiles(env, K, tile, transB):
    """K = 16 is a single k tile: the register prefetch must not load a second one (it would read the NaN behind the rows of A,
    or the NaN row behind B).  48 and 80 are odd tile counts."""
    check(env, transB, 128, 64, K, tile, scalars=((1.0, 0.0), (-0.75, 0.5)))


@pytest.mark.parametrize("transB", [0, 1])
@pytest.mark.parametrize("tile", [32, 64])
@pytest.mark.parametrize("share", ["none", "A", "B"])
def test_batch_of_three(env, share, tile, transB):
    """Gapped strides for all three operands (odd for C, which the contract allows, in rows of odd length); strideA = 0 or
    strideB = 0 is one shared operand, as the triangular inverse's callers pass it."""
    check(env, transB, 128, 64, 32, tile, batch=3, share_a=share == "A", share_b=share == "B", layout_c=(5, 7, 3),
          scalars=((-1.0, 1.0), (-0.75, 0.0)))


@pytest.mark.parametrize("transB", [0, 1])
@pytest.mark.parametrize("tile", [32, 64])
def test_beta_zero_does_not_read_c(env, tile, transB):
    """C holds NaN and infinities of both signs: with beta == 0 the result is the plain product, no NaN (0 * Inf) in it."""
    M, N = 128, 192
    Cm = np.tile(np.array([np.nan, np.inf, -np.inf]), 2 * M * N // 3 + 1)[:2 * M * N].reshape(2, M, N)
    for alpha in ALPHAS:
        check(env, transB, M, N, 32, tile, batch=2, scalars=((alpha, 0.0),), c_values=Cm)


@pytest.mark.parametrize("transB", [0, 1])
@pytest.mark.parametrize("tile", [32, 64])
@pytest.mark.parametrize("M,N", [(192, 192), (192, 128)])
def test_lower_only(env, M, N, tile, transB):
    """The 64 x 64 blocks strictly above the block diagonal are untouched bit for bit in BOTH variants (the skip is at 64
    granularity when the tile is 32); every other element is exact - the upper halves of the diagonal blocks included, and
    over the whole k range."""
    check(env, transB, M, N, 80, tile, batch=2, lower=1, scalars=((-1.0, 1.0), (-0.75, 0.5), (1.0, 0.0)))


def _lower_triangular(rng, n):
    L = np.tril(_ints(rng, (1, n, n)))
    d = np.arange(n)
    L[0, d, d] = rng.choice([-8.0, -3.0, -1.0, 1.0, 2.0, 7.0], size=n)   # a diagonal without zeros
    L[0][np.tril(np.ones((n, n), dtype=bool), -1) & (L[0] == 0)] = 5.0    # ... and none below it: every term counts
    return L


@pytest.mark.parametrize("tile", [32, 64])
@pytest.mark.parametrize("M,N", [(128, 128), (192, 192), (64, 192)])
def test_tri_1_b_lower_triangular(env, M, N, tile):
    """tri = 1 (transB = 0, K == N, B lower triangular): the k range of column tile bx starts at bx T - the result is the
    dense product.  With T = 32 at N = 192 the range starts inside a 64 block; starting one tile late drops the diagonal tile."""
    B = _lower_triangular(np.random.default_rng(N + tile), N)
    for batch, share in ((1, False), (2, True)):
        check(env, 0, M, N, N, tile, batch=batch, tri=1, B=B, share_b=share, scalars=((1.0, 0.0), (-0.75, 0.5)))


@pytest.mark.parametrize("tile", [32, 64])
@pytest.mark.parametrize("M,N", [(128, 128), (192, 192), (192, 64)])
def test_tri_2_a_lower_triangular(env, M, N, tile):
    """tri = 2 (K == M, A lower triangular): the k range of row tile by ends at (by + 1) T, and at K for the last one."""
    A = _lower_triangular(np.random.default_rng(M + tile + 1), M)
    for transB in (0, 1):   # (the triangular inverse uses transB = 0; nothing forbids the other)
        for batch, share in ((1, False), (2, True)):
            check(env, transB, M, N, M, tile, batch=batch, tri=2, A=A, share_a=share, scalars=((-1.0, 0.0), (-0.75, 0.5)))


@pytest.mark.parametrize("tri", [1, 2])
@pytest.mark.parametrize("tile", [32, 64])
def test_tri_reads_nothing_of_the_zero_blocks(env, tri, tile):
    """What makes tri worth having: the 64 x 64 blocks of the triangular operand strictly above its block diagonal are never
    read, in either variant (they hold NaN here; np.tril of the reference treats them as the zeros they stand for)."""
    n = 192
    rng = np.random.default_rng(tri + tile)
    L = _lower_triangular(rng, n)
    poisoned = L.copy()
    poisoned[0][~_block_lower_mask(n, n)] = np.nan
    opA, opB, opC = Operand(n, n, 1, 6, 12, 6), Operand(n, n, 1, 10, 20, 10), Operand(n, n, 1, 6, 7, 4)
    other = _ints(rng, (1, n, n))
    A, B = (other, L) if tri == 1 else (L, other)
    opA.set(other if tri == 1 else poisoned), opB.set(poisoned if tri == 1 else other)
    dA, dB, dC = env.to(opA.h), env.to(opB.h), env.to(opC.h)
    assert _launch(env, 0, n, n, n, 1.0, dA, opA, dB, opB, 0.0, dC, opC, 1, 0, tri, tile) == 0
    assert np.array_equal(opC.gather(dC.cpu().numpy()), A @ B)


@pytest.mark.parametrize("tile", [0, 64])
def test_in_place_panel_solve(env, tile):
    """C == A, transB = 1, N = K = 64, M = 192, lda == ldc: the panel solve of the factorisation, with an integer block in the
    place of the inverse.  Bit for bit the out-of-place result."""
    M, N, K = 192, 64, 64
    rng = np.random.default_rng(64 + tile)
    opA, opB, opC = Operand(M, K, 1, 6, 12, 6), Operand(N, K, 1, 10, 20, 10), Operand(M, N, 1, 6, 12, 6)
    A, B = _ints(rng, (1, M, K)), _ints(rng, (1, N, K))
    opA.set(A), opB.set(B), opC.set(_ints(rng, (1, M, N)))
    dA, dB, dC = env.to(opA.h), env.to(opB.h), env.to(opC.h)
    assert _launch(env, 1, M, N, K, 1.0, dA, opA, dB, opB, 0.0, dC, opC, 1, 0, 0, tile) == 0
    out_of_place = dC.cpu().numpy()
    assert _launch(env, 1, M, N, K, 1.0, dA, opA, dB, opB, 0.0, dA, opA, 1, 0, 0, tile) == 0
    in_place = dA.cpu().numpy()
    assert np.array_equal(opA.gather(in_place), A @ B.transpose(0, 2, 1))
    pay = opA.payload()
    assert np.array_equal(in_place.view(np.uint64)[pay], out_of_place.view(np.uint64)[pay])
    assert np.array_equal(in_place.view(np.uint64)[~pay], opA.h.view(np.uint64)[~pay])   # the padding of the panel


def _threshold(env, transB, M, N, batch, lower):
    """tile = 0 about the library's switch between the variants; A strided with gaps, B shared, C dense (its size is the point)."""
    check(env, transB, M, N, 16, 0, batch=batch, lower=lower, share_b=True, layout_c=(0, 0, 0), scalars=((-0.75, 0.5),))


@pytest.mark.parametrize("transB", [0, 1])
@pytest.mark.parametrize("batch", [2047, 2048])
def test_own_choice_at_the_threshold(env, batch, transB):
    """M = N = 64: 2047 tiles of 64 x 64 take the 32 x 32 variant, 2048 the 64 x 64 one.  Both exact."""
    _threshold(env, transB, 64, 64, batch, 0)


@pytest.mark.parametrize("transB", [0, 1])
@pytest.mark.parametrize("batch", [682, 683])
def test_own_choice_at_the_threshold_lower_only(env, batch, transB):
    """M = N = 128 with lower_only: three tiles of 64 x 64 per matrix are counted, 2046 and 2049 in all."""
    _threshold(env, transB, 128, 128, batch, 1)


@pytest.mark.parametrize("transB", [0, 1])
@pytest.mark.parametrize("tile", [32, 64])
def test_rounding(env, tile, transB):
    """Standard-normal operands against a np.longdouble reference.  The bound is the standard one for a K-term fused sum in any
    order followed by the scaling by alpha and the fused beta * C: K + 2 roundings,
    |got - exact| <= (K + 2) 2^-53 (|alpha| |A| @ |op(B)| + |beta| |C|) element-wise.  Derived, not measured."""
    M, N, K, alpha, beta = 128, 192, 80, -0.75, 0.5
    rng = np.random.default_rng(80 + tile + transB)
    A, B = rng.standard_normal((1, M, K)), rng.standard_normal((1, N, K) if transB else (1, K, N))
    Cm = rng.standard_normal((1, M, N))
    opA, opB, opC = Operand(M, K, 1, 6, 12, 6).set(A), Operand(*B.shape[1:], 1, 10, 20, 10).set(B), Operand(M, N, 1, 6, 7, 4).set(Cm)
    dA, dB, dC = env.to(opA.h), env.to(opB.h), env.to(opC.h)
    assert _launch(env, transB, M, N, K, alpha, dA, opA, dB, opB, beta, dC, opC, 1, 0, 0, tile) == 0
    got = opC.gather(dC.cpu().numpy())[0]
    opB_ = B[0].T if transB else B[0]
    ld = np.longdouble
    ref = ld(alpha) * (A[0].astype(ld) @ opB_.astype(ld)) + ld(beta) * Cm[0].astype(ld)
    bound = (K + 2) * 2.0 ** -53 * (abs(alpha) * (np.abs(A[0]) @ np.abs(opB_)) + abs(beta) * np.abs(Cm[0]))
    err = np.abs(got.astype(ld) - ref)
    print(f"rounding tile={tile} transB={transB}: max err / bound = {float(np.max(err / bound)):.3g}")
    assert np.all(err <= bound)


@pytest.mark.parametrize("name,case", [("BASE", BASE), ("BASE_ALIAS", BASE_ALIAS), ("BASE_TRI1", BASE_TRI1), ("BASE_TRI2", BASE_TRI2),
                                       ("odd strides, batch 1", dict(BASE, batch=1, strideA=5, strideB=7))])
def test_valid_calls_of_the_host_check_are_accepted(env, name, case):
    """The calls that tests/test_host_gemm_args_cpu.py breaks one rule at a time are accepted as they stand (on zeros: the
    status is the point), and so is an odd stride that batch == 1 never uses."""
    t, c = env.torch, case
    brows = c["N"] if c["transB"] else c["K"]
    def alloc(rows, ld, stride):
        return t.zeros(c["batch"] * stride + rows * ld + 64, dtype=t.float64, device=env.dev)
    dA, dB = alloc(c["M"], c["lda"], c["strideA"]), alloc(brows, c["ldb"], c["strideB"])
    dC = dA if c["c_off"] == c["a_off"] else alloc(c["M"], c["ldc"], c["strideC"])
    rc = env.lib.gpbo_gemm_tri_f64(c["transB"], c["M"], c["N"], c["K"], 1.0, C.c_void_p(dA.data_ptr()), c["lda"], c["strideA"],
                                   C.c_void_p(dB.data_ptr()), c["ldb"], c["strideB"], 0.0, C.c_void_p(dC.data_ptr()), c["ldc"],
                                   c["strideC"], c["batch"], c["lower_only"], c["tri"], c["tile"], env.stream())
    assert rc == 0, name
    t.cuda.synchronize()
    assert not bool(t.isnan(dC).any())
