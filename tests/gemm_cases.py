"""Four calls of the fp64 GEMM (include/gpbo.h: gpbo_gemm_tri_f64) that satisfy every rule of its host check.

tests/test_host_gemm_args_cpu.py breaks one rule at a time starting from these and expects GPBO_ERR_ARG;
tests/test_gpu_gemm.py runs them unchanged on real buffers and expects GPBO_OK.  a_off / b_off / c_off are byte offsets
of the three operands from one 256-byte-aligned base (equal offsets = aliased operands)."""

# transB = 1: A [128 x 32] in rows of 40, B [192 x 32] in rows of 36, C [128 x 192] in rows of 200, two gapped matrices each
BASE = dict(transB=1, M=128, N=192, K=32, lda=40, strideA=128 * 40 + 6, ldb=36, strideB=192 * 36 + 2, ldc=200,
            strideC=128 * 200 + 1, batch=2, lower_only=0, tri=0, tile=0, a_off=0, b_off=1 << 20, c_off=2 << 20)
# the in-place panel solve of the factorisation: C == A, N == K == 64, one leading dimension
BASE_ALIAS = dict(BASE, M=192, N=64, K=64, lda=200, ldb=64, ldc=200, strideA=0, strideB=0, strideC=0, batch=1, c_off=0)
# the two triangular products of the triangular inverse: transB = 0, the triangular operand square
BASE_TRI1 = dict(BASE, transB=0, M=64, N=128, K=128, lda=130, ldb=130, ldc=130, strideA=0, strideB=0, strideC=0, batch=1,
                 tri=1)
BASE_TRI2 = dict(BASE, transB=0, M=128, N=64, K=128, lda=130, ldb=66, ldc=66, strideA=0, strideB=0, strideC=0, batch=1,
                 tri=2)
