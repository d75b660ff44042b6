// Gradient of the log marginal likelihood with respect to the log length scales (ML-II fitting of the ARD kernel).
//
// The reference declares `hyperparam_obj` and `gradient_steps` (point_selector.py:30, :33) for a gradient fit it never
// built; its tune_kernel searches a grid (:104-163).  From a factorisation of K = K0 + jitter I made by
// gpbo_factorise_f64 (U = L^-T, alpha = K^-1 y):
//     NLML              = 1/2 (y . alpha + log det K + N log 2 pi),   log det K = -2 sum_i log U_ii
//     dNLML / dlog l_k  = 1/2 sum_ij W_ij K0_ij (x_ik - x_jk)^2 / l_k^2,   W = K^-1 - alpha alpha^T
// With the points scaled by 1 / (l sqrt 2) (gpbo_scale_points_f64: K0_ij = exp(-sum_k d_k^2), d = the scaled difference)
// the k-th term is W_ij K0_ij 2 d_k^2, so the gradient is sum_ij W_ij K0_ij d_k^2.
//
// nlml_grad_kernel: one workgroup per 64 x 64 tile (I, J), I >= J, of the lower block triangle of K^-1 = U U^T, the
// blocks wholly inside the padding not launched.  The tile is U[I rows] U[J rows]^T on the matrix cores
// (v_mfma_f64_16x16x4_f64); U is upper triangular, so only k >= 64 I contributes, up to N rounded up to 16 (U is the
// identity on the padding, zero beyond column N in the leading rows): about Np^3 / 3 flop in all.  Both operands are
// row-major [rows x k], the TRANSB = 1 staging of gemm_f64.hip with its register prefetch.  Tiles are numbered by
// increasing I, so the longest products are dispatched first.  The epilogue works on the accumulators in registers:
// W_ij, K0_ij regenerated from the scaled points in LDS (exp_neg.h), d partial sums, rows or columns >= N masked,
// off-diagonal tiles counted twice; the workgroup's d sums go to its own slot of a slab in the workspace.
// nlml_grad_finish_kernel (one workgroup) adds the slab in a fixed order and writes out[0] = NLML, out[1 + k] = the
// gradient: no atomics, so two calls give the same bits.  info != 0 (K not positive definite): every output NaN.
// Other covariance families (gpbo_nlml_grad_kern_f64): dk / dlog l_k = g(r) (x_ik - x_jk)^2 / l_k^2 with g = k for the squared
// exponential, 3 exp(-a) for Matern 3/2 and 5/3 (1 + a) exp(-a) for Matern 5/2, so only the factor the epilogue regenerates
// changes; in the scaled coordinates s = r^2 / 2, a = sqrt(6 s) or sqrt(10 s).  Nothing is divided by r.
#include "cov_entry.h"

namespace {

constexpr int GT = 64;      // tile edge
constexpr int GBK = 16;     // k depth of one staged tile
constexpr int GLDA = 17;    // As[m][k] / Bs[n][k] row stride (doubles), as gemm_f64.hip

// tile t -> (I, J), t = I (I + 1) / 2 + J, 0 <= J <= I
__device__ __forceinline__ void tile_of(int64_t t, int &I, int &J) {
    int i = (int)((sqrt(8.0 * (double)t + 1.0) - 1.0) * 0.5);
    while ((int64_t)(i + 1) * (i + 2) / 2 <= t) ++i;
    while ((int64_t)i * (i + 1) / 2 > t) --i;
    I = i;
    J = (int)(t - (int64_t)i * (i + 1) / 2);
}

// g(r) of the family from s = r^2 / 2 (see the header)
template <int KERN>
__device__ __forceinline__ double dlog_factor(double s, const double *tab) {
    if constexpr (KERN == GPBO_KERNEL_SE) {
        return exp_neg(s, tab);
    } else if constexpr (KERN == GPBO_KERNEL_MATERN32) {
        return 3.0 * exp_neg(sqrt_nonneg(6.0 * s), tab);
    } else {
        const double a = sqrt_nonneg(10.0 * s);
        return (5.0 / 3.0) * ((1.0 + a) * exp_neg(a, tab));
    }
}

// The body of the tile kernels below, one per family (inlined into each: the squared-exponential kernel keeps its name and its
// instructions).
template <int D, int KERN>
__device__ __forceinline__ void nlml_grad_tile(const double *__restrict__ U, const double *__restrict__ alpha,
                                               const double *__restrict__ Xsc, int N, int Np, double *__restrict__ slab) {
    __shared__ double As[GT * GLDA];
    __shared__ double Bs[GT * GLDA];
    __shared__ double xr[GT * D], xc[GT * D];   // scaled points of the tile's rows (block I) and columns (block J)
    __shared__ double ar[GT], ac[GT];           // alpha of the same
    __shared__ double tab[GPBO_EXP_E];
    __shared__ double red[4][D];

    int I, J;
    tile_of(blockIdx.x, I, J);
    const int tid = threadIdx.x;
    const int lane = tid & 63, wid = tid >> 6;
    const int wr = wid >> 1, wc = wid & 1;
    const int l15 = lane & 15, l4 = lane >> 4;
    const int r0 = I * GT, c0 = J * GT;

    for (int e = tid; e < GT * D; e += 256) {
        xr[e] = Xsc[(int64_t)r0 * D + e];
        xc[e] = Xsc[(int64_t)c0 * D + e];
    }
    if (tid < GT) ar[tid] = alpha[r0 + tid];
    else if (tid < 2 * GT) ac[tid - GT] = alpha[c0 + tid - GT];
    else if (tid < 2 * GT + GPBO_EXP_E) cov_stage_tab(tab, tid - 2 * GT);

    const double *A = U + (int64_t)r0 * Np;
    const double *B = U + (int64_t)c0 * Np;
    d4_t acc[2][2];
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int j = 0; j < 2; ++j) acc[i][j] = d4_t{0.0, 0.0, 0.0, 0.0};

    // staging: thread -> row tid / 4, 4 doubles at k = (tid % 4) * 4 of both operands
    const int sr = tid >> 2, sk = (tid & 3) * 4;
    d2_t a0, a1, b0, b1;
    auto gload = [&](int k0) {
        const d2_t *ap = reinterpret_cast<const d2_t *>(A + (int64_t)sr * Np + k0 + sk);
        const d2_t *bp = reinterpret_cast<const d2_t *>(B + (int64_t)sr * Np + k0 + sk);
        a0 = ap[0]; a1 = ap[1];
        b0 = bp[0]; b1 = bp[1];
    };
    const int kbeg = r0;                        // U[i][k] = 0 for k < i: nothing below the row block's first column
    const int kend = (N + GBK - 1) / GBK * GBK; // and nothing beyond column N in the rows that count
    gload(kbeg);
    for (int k0 = kbeg; k0 < kend; k0 += GBK) {
        gpbo_syncthreads();   // previous tile consumed
        As[sr * GLDA + sk + 0] = a0.x; As[sr * GLDA + sk + 1] = a0.y;
        As[sr * GLDA + sk + 2] = a1.x; As[sr * GLDA + sk + 3] = a1.y;
        Bs[sr * GLDA + sk + 0] = b0.x; Bs[sr * GLDA + sk + 1] = b0.y;
        Bs[sr * GLDA + sk + 2] = b1.x; Bs[sr * GLDA + sk + 3] = b1.y;
        gpbo_syncthreads();
        if (k0 + GBK < kend) gload(k0 + GBK);
#pragma unroll
        for (int kk = 0; kk < GBK; kk += 4) {
            double af[2], bf[2];
#pragma unroll
            for (int i = 0; i < 2; ++i) af[i] = As[(wr * 32 + i * 16 + l15) * GLDA + kk + l4];
#pragma unroll
            for (int j = 0; j < 2; ++j) bf[j] = Bs[(wc * 32 + j * 16 + l15) * GLDA + kk + l4];
#pragma unroll
            for (int i = 0; i < 2; ++i)
#pragma unroll
                for (int j = 0; j < 2; ++j) acc[i][j] = mfma_f64_16x16x4(af[i], bf[j], acc[i][j]);
        }
    }
    // (the point / alpha / table loads above are published by the loop's barriers: the loop runs at least once)

    // epilogue: f64 C/D layout, row = (lane >> 4) + 4 reg, col = lane & 15 of each 16 x 16 block
    double g[D];
#pragma unroll
    for (int k = 0; k < D; ++k) g[k] = 0.0;
#pragma unroll
    for (int j = 0; j < 2; ++j) {
        const int lc = wc * 32 + j * 16 + l15;
        if (c0 + lc >= N) continue;
        double xj[D];
#pragma unroll
        for (int k = 0; k < D; ++k) xj[k] = xc[lc * D + k];
        const double aj = ac[lc];
#pragma unroll
        for (int i = 0; i < 2; ++i)
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int lr = wr * 32 + i * 16 + l4 + 4 * r;
                if (r0 + lr >= N) continue;
                double dd[D], s = 0.0;
#pragma unroll
                for (int k = 0; k < D; ++k) {
                    const double t = xr[lr * D + k] - xj[k];
                    dd[k] = t * t;
                    s += dd[k];
                }
                const double w = acc[i][j][r] - ar[lr] * aj;
                const double wk = w * dlog_factor<KERN>(s, tab);
#pragma unroll
                for (int k = 0; k < D; ++k) g[k] = fma(wk, dd[k], g[k]);
            }
    }
    // fixed-order reduction: butterfly within the wave (every lane ends with the same bits), then the four waves
#pragma unroll
    for (int off = 32; off > 0; off >>= 1)
#pragma unroll
        for (int k = 0; k < D; ++k) g[k] += __shfl_xor(g[k], off);
    if (lane == 0) {
#pragma unroll
        for (int k = 0; k < D; ++k) red[wid][k] = g[k];
    }
    gpbo_syncthreads();
    if (tid < D) {
        const double s = ((red[0][tid] + red[1][tid]) + red[2][tid]) + red[3][tid];
        slab[(int64_t)blockIdx.x * D + tid] = (I == J) ? s : 2.0 * s;   // (J, I) is the same sum
    }
}

template <int D>
__global__ __launch_bounds__(256) void nlml_grad_kernel(const double *__restrict__ U, const double *__restrict__ alpha,
                                                        const double *__restrict__ Xsc, int N, int Np,
                                                        double *__restrict__ slab) {
    nlml_grad_tile<D, GPBO_KERNEL_SE>(U, alpha, Xsc, N, Np, slab);
}

// the same tiles with a Matern factor in the epilogue (gpbo_nlml_grad_kern_f64)
template <int D, int KERN>
__global__ __launch_bounds__(256) void nlml_grad_matern_kernel(const double *__restrict__ U, const double *__restrict__ alpha,
                                                               const double *__restrict__ Xsc, int N, int Np,
                                                               double *__restrict__ slab) {
    static_assert(KERN == GPBO_KERNEL_MATERN32 || KERN == GPBO_KERNEL_MATERN52, "a Matern family");
    nlml_grad_tile<D, KERN>(U, alpha, Xsc, N, Np, slab);
}

// out[0] = NLML from diag(U) and y . alpha; out[1 + k] = sum of the slab's column k, tiles in order
__global__ __launch_bounds__(256) void nlml_grad_finish_kernel(const double *__restrict__ slab, int64_t tiles, int d,
                                                               const double *__restrict__ U,
                                                               const double *__restrict__ alpha,
                                                               const double *__restrict__ y, int64_t N, int64_t Np,
                                                               const int32_t *__restrict__ info, double *__restrict__ out) {
    __shared__ double s_a[256], s_b[256];
    const int tid = threadIdx.x;
    const bool bad = *info != 0;
    double ld = 0.0, q = 0.0;
    for (int64_t i = tid; i < N; i += 256) {
        ld -= log(U[i * Np + i]);
        q = fma(y[i], alpha[i], q);
    }
    s_a[tid] = ld;
    s_b[tid] = q;
    gpbo_syncthreads();
    for (int off = 128; off > 0; off >>= 1) {
        if (tid < off) { s_a[tid] += s_a[tid + off]; s_b[tid] += s_b[tid + off]; }
        gpbo_syncthreads();
    }
    if (tid == 0) {
        const double nlml = 0.5 * ((s_b[0] + 2.0 * s_a[0]) + (double)N * 1.8378770664093453);  // log(2 pi)
        out[0] = bad ? __builtin_nan("") : nlml;
    }
    for (int k = 0; k < d; ++k) {
        gpbo_syncthreads();   // the previous round's result has been read
        double s = 0.0;
        for (int64_t t = tid; t < tiles; t += 256) s += slab[t * d + k];
        s_a[tid] = s;
        gpbo_syncthreads();
        for (int off = 128; off > 0; off >>= 1) {
            if (tid < off) s_a[tid] += s_a[tid + off];
            gpbo_syncthreads();
        }
        if (tid == 0) out[1 + k] = bad ? __builtin_nan("") : s_a[0];
    }
}

int64_t grad_tiles(int64_t N) {
    const int64_t nb = (N + GT - 1) / GT;   // row blocks that hold an observation
    return nb * (nb + 1) / 2;
}

int64_t align256(int64_t b) { return (b + 255) / 256 * 256; }

}  // namespace

extern "C" int64_t gpbo_nlml_grad_workspace_bytes(int64_t Np, int32_t d) {
    if (Np < GPBO_NPAD || Np % GPBO_NPAD || d < 1 || d > GPBO_MAX_D) return GPBO_ERR_ARG;
    // scaled points [Np x d], then the slab [tiles x d] (at most Np / 64 row blocks)
    return align256((int64_t)sizeof(double) * Np * d) + align256((int64_t)sizeof(double) * grad_tiles(Np) * d);
}

extern "C" int gpbo_nlml_grad_f64(const double *U, const double *alpha, const double *y, const double *X, int64_t N,
                                  int64_t Np, int32_t d, const double *ls_host, const int32_t *info, double *out,
                                  void *work, int64_t work_bytes, void *stream) {
    return gpbo_nlml_grad_kern_f64(U, alpha, y, X, N, Np, d, ls_host, GPBO_KERNEL_SE, info, out, work, work_bytes, stream);
}

extern "C" int gpbo_nlml_grad_kern_f64(const double *U, const double *alpha, const double *y, const double *X, int64_t N,
                                       int64_t Np, int32_t d, const double *ls_host, int32_t kernel, const int32_t *info,
                                       double *out, void *work, int64_t work_bytes, void *stream) {
    if (!U || !alpha || !y || !X || !ls_host || !info || !out || !work) return GPBO_ERR_ARG;
    if (!kernel_ok(kernel, d)) return GPBO_ERR_ARG;
    if (N < 1 || Np != gpbo_padded_n(N) || Np > (1 << 20) || d < 1 || d > GPBO_MAX_D) return GPBO_ERR_ARG;
    for (int k = 0; k < d; ++k)
        if (!(ls_host[k] > 0.0)) return GPBO_ERR_ARG;
    if (((uintptr_t)U | (uintptr_t)work) & 15) return GPBO_ERR_ARG;
    if (work_bytes < gpbo_nlml_grad_workspace_bytes(Np, d)) return GPBO_ERR_WORKSPACE;
    double *Xsc = reinterpret_cast<double *>(work);
    double *slab = reinterpret_cast<double *>(reinterpret_cast<char *>(work) + align256((int64_t)sizeof(double) * Np * d));
    const int64_t tiles = grad_tiles(N);
    hipStream_t st = gpbo_stream(stream);
    int rc = gpbo_scale_points_launch(X, N, Np, d, ls_host, Xsc, nullptr, stream);
    if (rc != GPBO_OK) return rc;
#define GRAD_LAUNCH(DD, KK)                                                                                                      \
    hipLaunchKernelGGL((nlml_grad_matern_kernel<DD, KK>), dim3((unsigned)tiles), dim3(256), 0, st, U, alpha, Xsc, (int)N, (int)Np, \
                       slab)
#define CALL(DD)                                                                   \
    if (kernel == GPBO_KERNEL_MATERN32) GRAD_LAUNCH(DD, GPBO_KERNEL_MATERN32);     \
    else if (kernel == GPBO_KERNEL_MATERN52) GRAD_LAUNCH(DD, GPBO_KERNEL_MATERN52); \
    else hipLaunchKernelGGL(nlml_grad_kernel<DD>, dim3((unsigned)tiles), dim3(256), 0, st, U, alpha, Xsc, (int)N, (int)Np, slab)
    GPBO_FOR_D(d, CALL)
#undef CALL
#undef GRAD_LAUNCH
    hipLaunchKernelGGL(nlml_grad_finish_kernel, dim3(1), dim3(256), 0, st, slab, tiles, (int)d, U, alpha, y, N, Np, info,
                       out);
    GPBO_CHECK_LAUNCH();
    return GPBO_OK;
}
