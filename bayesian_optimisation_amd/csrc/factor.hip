// Factorisation of K + sigma^2 I: blocked right-looking Cholesky, block-recursive
// inverse of the Cholesky factor, and alpha = K^-1 y.
//
// The reference inverts cov_meas with np.linalg.inv (/root/reference/point_selector.py:89) and uses
// the inverse twice (:90-91).  Here K = L L^T once per BO step; U = L^-T is formed explicitly so the
// per-candidate variance becomes a dense triangular product on the matrix cores
// (sigma_acq.hip) instead of a sequential triangular solve per candidate.
#include "gpbo_internal.h"
#include "potrf_diag64.h"

#include <cstdio>
#include <cstdlib>
#include <mutex>

int gpbo_gemm_launch(int transB, int64_t M, int64_t N, int64_t K, double alpha, const double *A, int64_t lda,
                     int64_t strideA, const double *B, int64_t ldb, int64_t strideB, double beta, double *C,
                     int64_t ldc, int64_t strideC, int batch, int lower_only, hipStream_t st);

namespace {

constexpr int NB = GPBO_NB;  // 64
constexpr int LDS_LD = NB + 1;

using gpbo_pd::LDM;
using gpbo_pd::readlane_f64;
using gpbo_pd::rsqrt_refined;

__global__ __launch_bounds__(256) void potrf_diag_kernel(double *__restrict__ K, int64_t ld, int jb,
                                                         double *__restrict__ dinv, int32_t *__restrict__ info,
                                                         int64_t strideK, int64_t strideD /* batch = gridDim.x */) {
    __shared__ double M[2 * NB * LDM];  // rows 0..63: A -> L (lower);  rows 64..127: I -> L^-T (upper)
    K += (int64_t)blockIdx.x * strideK;      // batched use (the ARD grid): one matrix per workgroup
    dinv += (int64_t)blockIdx.x * strideD;
    if (strideK) info += blockIdx.x;
    const int tid = threadIdx.x;
    double *Kd = K + ((int64_t)jb * NB) * ld + (int64_t)jb * NB;
    for (int e = tid; e < NB * NB; e += 256) {
        const int r = e >> 6, c = e & 63;
        M[r * LDM + c] = (c <= r) ? Kd[(int64_t)r * ld + c] : 0.0;
        M[(NB + r) * LDM + c] = (c == r) ? 1.0 : 0.0;
    }
    __syncthreads();

    const int first_bad = gpbo_pd::potrf_diag64_lds(M, tid);
    if (tid == 0 && first_bad) atomicCAS(info, 0, jb * NB + first_bad);
    double *dv = dinv + (int64_t)jb * NB * NB;
    for (int e = tid; e < NB * NB; e += 256) {
        const int r = e >> 6, c = e & 63;
        if (c <= r) Kd[(int64_t)r * ld + c] = M[r * LDM + c];
        dv[e] = (c <= r) ? M[(NB + c) * LDM + r] : 0.0;   // inv(L)[r][c] = (L^-T)[c][r]
    }
}

// W <- block-diagonal of dinv, zero elsewhere.   grid (Np/64, Np/64), block 256.
__global__ __launch_bounds__(256) void init_w_kernel(const double *__restrict__ dinv, double *__restrict__ W,
                                                     int64_t Np) {
    const int bi = blockIdx.y, bj = blockIdx.x;
    double *Wb = W + ((int64_t)bi * NB) * Np + (int64_t)bj * NB;
    const double *dv = dinv + (int64_t)bi * NB * NB;
    for (int e = threadIdx.x; e < NB * NB; e += 256) {
        const int r = e >> 6, c = e & 63;
        Wb[(int64_t)r * Np + c] = (bi == bj) ? dv[e] : 0.0;
    }
}

// U = W^T restricted to the upper triangle (W is lower triangular): 64x64 tiles through LDS.
__global__ __launch_bounds__(256) void transpose_upper_kernel(const double *__restrict__ W, double *__restrict__ U,
                                                              int64_t Np) {
    __shared__ double tile[NB * LDS_LD];
    const int bi = blockIdx.y, bj = blockIdx.x;  // output tile (bi, bj) of U = input tile (bj, bi) of W
    double *Ub = U + ((int64_t)bi * NB) * Np + (int64_t)bj * NB;
    if (bj < bi) {  // strictly below the diagonal: zeros
        for (int e = threadIdx.x; e < NB * NB; e += 256) Ub[(int64_t)(e >> 6) * Np + (e & 63)] = 0.0;
        return;
    }
    const double *Wb = W + ((int64_t)bj * NB) * Np + (int64_t)bi * NB;
    for (int e = threadIdx.x; e < NB * NB; e += 256) tile[(e >> 6) * LDS_LD + (e & 63)] = Wb[(int64_t)(e >> 6) * Np + (e & 63)];
    __syncthreads();
    for (int e = threadIdx.x; e < NB * NB; e += 256) {
        const int r = e >> 6, c = e & 63;
        double v = tile[c * LDS_LD + r];
        if (bi == bj && c < r) v = 0.0;
        Ub[(int64_t)r * Np + c] = v;
    }
}

// tmp_i = sum_{m<=i} U[m][i] y_m   (= (L^-1 y)_i).  Block = 16 columns (one 128-byte line per row of U) x 64 row
// groups: lane -> column lane&15, row group 4*wave + lane>>4 takes m = rg, rg+64, ...; fixed-order LDS reduction.
// (Np/16 workgroups: with 64 columns per workgroup a 4096-point problem kept only 64 of the 256 CUs busy.)
__global__ __launch_bounds__(1024) void utv_kernel(const double *__restrict__ U, const double *__restrict__ y,
                                                   int64_t N, int64_t Np, double *__restrict__ tmp) {
    __shared__ double part[64][17];
    const int lane = threadIdx.x & 63, col = lane & 15;
    const int rg = (threadIdx.x >> 6) * 4 + (lane >> 4);
    const int64_t i = (int64_t)blockIdx.x * 16 + col;
    double s = 0.0;
    const int64_t mend = (i < N ? i : N - 1);
    for (int64_t m = rg; m <= mend; m += 64) s = fma(U[m * Np + i], y[m], s);
    part[rg][col] = s;
    __syncthreads();
    if (threadIdx.x < 16) {
        double r = 0.0;
        for (int k = 0; k < 64; ++k) r += part[k][threadIdx.x];
        tmp[(int64_t)blockIdx.x * 16 + threadIdx.x] = r;
    }
}

// alpha_m = sum_{i>=m} U[m][i] tmp_i.  One wave per row m, lanes stride over i, fixed-order reduce.
__global__ __launch_bounds__(256) void uv_kernel(const double *__restrict__ U, const double *__restrict__ tmp,
                                                 int64_t N, int64_t Np, double *__restrict__ alpha) {
    const int lane = threadIdx.x & 63;
    const int64_t m = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (m >= Np) return;
    double s = 0.0;
    if (m < N) {
        for (int64_t i = (m & ~63LL) + lane; i < Np; i += 64)
            if (i >= m) s = fma(U[m * Np + i], tmp[i], s);
    }
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) s += __shfl_xor(s, off);
    if (lane == 0) alpha[m] = (m < N) ? s : 0.0;
}

__global__ void zero_i32_kernel(int32_t *p) { *p = 0; }

}  // namespace

// Helper stream for the look-ahead of the Cholesky (one per device, created on first use, kept for the life of the
// process; nothing is retained about the caller's buffers).
struct LookAhead {
    hipStream_t stream;
    hipEvent_t panel_done, rest_done;
};

// (round-2 chain only - gpbo_potrf_f64 and GPBO_FACTOR_OLD=1: ONE such factorisation per device at a time; two callers on
//  different streams would re-record the same pair of events.  The fused factorisation of round 3 has no helper stream.)
static LookAhead *lookahead_for_current_device() {
    static LookAhead *tab[64] = {nullptr};
    static std::mutex mu;
    std::lock_guard<std::mutex> g(mu);
    int dev = 0;
    if (hipGetDevice(&dev) != hipSuccess || dev < 0 || dev >= 64) return nullptr;
    if (!tab[dev]) {
        LookAhead *h = new LookAhead;
        bool ok = hipStreamCreateWithFlags(&h->stream, hipStreamNonBlocking) == hipSuccess;
        ok = ok && hipEventCreateWithFlags(&h->panel_done, hipEventDisableTiming) == hipSuccess;
        ok = ok && hipEventCreateWithFlags(&h->rest_done, hipEventDisableTiming) == hipSuccess;
        if (!ok) { delete h; return nullptr; }
        tab[dev] = h;
    }
    return tab[dev];
}

// info_is_zero: the caller has already cleared *info on this stream (gpbo_factorise_f64 does it in the K(X,X) build)
static int potrf_run(double *Kp, int64_t Np, double *dinv, int32_t *info, bool info_is_zero, void *stream) {
    if (!Kp || !dinv || !info || Np < NB || Np % NB) return GPBO_ERR_ARG;
    hipStream_t st = gpbo_stream(stream);
    if (!info_is_zero) hipLaunchKernelGGL(zero_i32_kernel, dim3(1), dim3(1), 0, st, info);
    const int nb = (int)(Np / NB);
    // Block columns per trailing update.  With one column per update (rank 64) every step reads and writes the whole
    // trailing matrix for 128 flops per 16 bytes: HBM-bound from N ~ 2048 up (N = 8192: 67 GB of traffic, 8.4 ms for
    // 1.8e11 flop).  Groups of four columns are factorised left-looking inside the group (narrow updates of one block
    // column, K = 64..192) and applied to the rest in one rank-256 update: a quarter of the traffic.  Small problems
    // keep one column per update - their launches are latency-bound and the narrow updates would sit on the
    // critical path with a longer K loop.  Measured (whole factorisation, ms, G = 1 / 2 / 4 / 8):
    // N = 2048: 1.36 / 1.37 / 1.45 / 1.62;  N = 4096: 3.77 / 3.63 / 3.76 / 4.10;  N = 8192: 17.1 / 15.3 / 15.1 / 15.9.
    const int G = (Np >= 8192) ? 4 : (Np >= 4096) ? 2 : 1;
    // Look-ahead (N >= 8192): the trailing update of a group is cut in two - the block columns of the NEXT group, applied
    // on the caller's stream so that their diagonal blocks and panels (64 launches of ~15 + ~8 us at N = 4096: sequential,
    // one workgroup wide) can start at once, and everything to the right of them, applied on a helper stream meanwhile.
    // Events: panel_done (caller -> helper: the group's panel is final), rest_done (helper -> caller: the columns the next
    // update of the caller touches are no longer being written).  Fork and join inside this call: still capturable.
    // Measured on MI355X (GPBO_NO_LOOKAHEAD=1 against 0, whole factorisation): N = 2048: 1.17 -> 1.49 ms, N = 4096:
    // 3.18 -> 3.44 ms (two events and two waits per group cost more than the ~25 us of diagonal block + panel they hide),
    // N = 8192: 12.9 -> 12.3 ms - so it is used from N = 8192 up only.
    static const bool la_env = !env_flag("GPBO_NO_LOOKAHEAD");
    LookAhead *la = (Np >= 8192 && la_env) ? lookahead_for_current_device() : nullptr;
    bool rest_pending = false;  // a helper-stream update has been issued and not yet waited for
    for (int j0 = 0; j0 < nb; j0 += G) {
        const int gend = (j0 + G < nb) ? j0 + G : nb;
        for (int j = j0; j < gend; ++j) {
            const int c = j - j0;  // block columns of this group already factorised
            if (c > 0) {
                // block column j, rows j.. :  -= L[j.., j0..j-1] * L[j, j0..j-1]^T
                const int64_t rows = Np - (int64_t)j * NB;
                const double *Lrows = Kp + (int64_t)j * NB * Np + (int64_t)j0 * NB;
                double *Acol = Kp + (int64_t)j * NB * Np + (int64_t)j * NB;
                int rc = gpbo_gemm_launch(1, rows, NB, (int64_t)NB * c, -1.0, Lrows, Np, 0, Lrows, Np, 0, 1.0, Acol, Np, 0,
                                          1, 0, st);
                if (rc != GPBO_OK) return rc;
            }
            hipLaunchKernelGGL(potrf_diag_kernel, dim3(1), dim3(256), 0, st, Kp, Np, j, dinv, info, (int64_t)0, (int64_t)0);
            GPBO_CHECK_LAUNCH();
            const int64_t rest = Np - (int64_t)(j + 1) * NB;
            if (rest <= 0) break;
            double *panel = Kp + (int64_t)(j + 1) * NB * Np + (int64_t)j * NB;  // [rest x 64]
            // panel <- panel * inv(L_jj)^T      (in place: each 64x64 tile is read whole before it is written)
            int rc = gpbo_gemm_launch(1, rest, NB, NB, 1.0, panel, Np, 0, dinv + (int64_t)j * NB * NB, NB, 0, 0.0, panel,
                                      Np, 0, 1, 0, st);
            if (rc != GPBO_OK) return rc;
        }
        const int64_t restg = Np - (int64_t)gend * NB;
        if (restg <= 0) break;
        // trailing lower triangle beyond the group -= P * P^T,  P = rows gend.., block columns j0..gend-1
        const double *P = Kp + (int64_t)gend * NB * Np + (int64_t)j0 * NB;
        double *trail = Kp + (int64_t)gend * NB * Np + (int64_t)gend * NB;
        const int64_t kdim = (int64_t)NB * (gend - j0);
        const int gend2 = (gend + G < nb) ? gend + G : nb;
        const int64_t ncols_a = (int64_t)(gend2 - gend) * NB, rest_b = restg - ncols_a;
        if (!la || rest_b <= 0) {
            if (rest_pending) {  // the helper's last update wrote this region
                if (hipStreamWaitEvent(st, la->rest_done, 0) != hipSuccess) return GPBO_ERR_LAUNCH;
                rest_pending = false;
            }
            int rc = gpbo_gemm_launch(1, restg, restg, kdim, -1.0, P, Np, 0, P, Np, 0, 1.0, trail, Np, 0, 1, 1, st);
            if (rc != GPBO_OK) return rc;
            continue;
        }
        if (hipEventRecord(la->panel_done, st) != hipSuccess) return GPBO_ERR_LAUNCH;
        // (a) the next group's block columns, all rows below: on the caller's stream, after the helper's previous update
        if (rest_pending && hipStreamWaitEvent(st, la->rest_done, 0) != hipSuccess) return GPBO_ERR_LAUNCH;
        int rc = gpbo_gemm_launch(1, restg, ncols_a, kdim, -1.0, P, Np, 0, P, Np, 0, 1.0, trail, Np, 0, 1, 0, st);
        if (rc != GPBO_OK) return rc;
        // (b) the lower triangle to the right of them: helper stream (in order behind its previous update)
        if (hipStreamWaitEvent(la->stream, la->panel_done, 0) != hipSuccess) return GPBO_ERR_LAUNCH;
        const double *Pb = P + ncols_a * Np;
        double *trail_b = trail + ncols_a * Np + ncols_a;
        rc = gpbo_gemm_launch(1, rest_b, rest_b, kdim, -1.0, Pb, Np, 0, Pb, Np, 0, 1.0, trail_b, Np, 0, 1, 1, la->stream);
        if (rc != GPBO_OK) return rc;
        if (hipEventRecord(la->rest_done, la->stream) != hipSuccess) return GPBO_ERR_LAUNCH;
        rest_pending = true;
    }
    if (rest_pending && hipStreamWaitEvent(st, la->rest_done, 0) != hipSuccess) return GPBO_ERR_LAUNCH;  // join
    return GPBO_OK;
}

extern "C" int gpbo_potrf_f64(double *Kp, int64_t Np, double *dinv, int32_t *info, void *stream) {
    return potrf_run(Kp, Np, dinv, info, false, stream);
}

int gpbo_launch_transpose_upper(const double *W, int64_t Np, double *U, hipStream_t st) {
    dim3 grid((unsigned)(Np / NB), (unsigned)(Np / NB));
    hipLaunchKernelGGL(transpose_upper_kernel, grid, dim3(256), 0, st, W, U, Np);
    GPBO_CHECK_LAUNCH();
    return GPBO_OK;
}

extern "C" int gpbo_trtri_f64(const double *L, const double *dinv, int64_t Np, double *U, double *work,
                              void *stream) {
    if (!L || !dinv || !U || !work || Np < NB || Np % NB) return GPBO_ERR_ARG;
    hipStream_t st = gpbo_stream(stream);
    double *W = work;
    double *T = U;  // scratch until the final transpose
    dim3 g2((unsigned)(Np / NB), (unsigned)(Np / NB));
    hipLaunchKernelGGL(init_w_kernel, g2, dim3(256), 0, st, dinv, W, Np);
    GPBO_CHECK_LAUNCH();
    for (int64_t s = NB; s < Np; s <<= 1) {
        const int64_t full = Np / (2 * s);       // complete pairs (s, s)
        const int64_t rem = Np - full * 2 * s;   // what is left after them
        const int64_t stride = 2 * s * (Np + 1);
        if (full > 0) {
            // T21 = L21 * W11 ; W21 = -W22 * T21      (block (p): rows o+s.., cols o.., o = 2ps)
            // (W11 and W22 are lower triangular: the zero halves of the k ranges are skipped, tri = 1 / 2)
            int rc = gpbo_gemm_launch_tri(0, s, s, s, 1.0, L + s * Np, Np, stride, W, Np, stride, 0.0, T + s * Np, Np,
                                          stride, (int)full, 0, 1, st);
            if (rc != GPBO_OK) return rc;
            rc = gpbo_gemm_launch_tri(0, s, s, s, -1.0, W + s * Np + s, Np, stride, T + s * Np, Np, stride, 0.0,
                                      W + s * Np, Np, stride, (int)full, 0, 2, st);
            if (rc != GPBO_OK) return rc;
        }
        if (rem > s) {  // ragged last pair: W11 is s x s, W22 is m2 x m2 with m2 = rem - s < s
            const int64_t o = full * 2 * s, m2 = rem - s;
            const double *L21 = L + (o + s) * Np + o;
            int rc = gpbo_gemm_launch(0, m2, s, s, 1.0, L21, Np, 0, W + o * Np + o, Np, 0, 0.0, T + (o + s) * Np + o, Np,
                                      0, 1, 0, st);
            if (rc != GPBO_OK) return rc;
            rc = gpbo_gemm_launch(0, m2, s, m2, -1.0, W + (o + s) * Np + o + s, Np, 0, T + (o + s) * Np + o, Np, 0, 0.0,
                                  W + (o + s) * Np + o, Np, 0, 1, 0, st);
            if (rc != GPBO_OK) return rc;
        }
    }
    return gpbo_launch_transpose_upper(W, Np, U, st);
}

extern "C" int gpbo_alpha_f64(const double *U, const double *y, int64_t N, int64_t Np, double *tmp, double *alpha,
                              void *stream) {
    if (!U || !y || !tmp || !alpha || N < 1 || Np < N || Np % NB) return GPBO_ERR_ARG;
    hipStream_t st = gpbo_stream(stream);
    hipLaunchKernelGGL(utv_kernel, dim3((unsigned)(Np / 16)), dim3(1024), 0, st, U, y, N, Np, tmp);
    hipLaunchKernelGGL(uv_kernel, dim3((unsigned)((Np + 3) / 4)), dim3(256), 0, st, U, tmp, N, Np, alpha);
    GPBO_CHECK_LAUNCH();
    return GPBO_OK;
}

extern "C" int64_t gpbo_factorise_workspace_bytes(int64_t Np) {
    // L [Np*Np] + trtri work [Np*Np] + dinv [Np*64] + tmp [Np]
    return (int64_t)sizeof(double) * (2 * Np * Np + Np * NB + Np);
}

extern "C" int gpbo_factorise_f64(const double *X, const double *y, int64_t N, int32_t d, const double *ls_host,
                                  double jitter1, double jitter2, int64_t Np, double *Kp, double *U, double *alpha,
                                  int32_t *info, void *work, int64_t work_bytes, void *stream) {
    return gpbo_factorise_kern_f64(X, y, N, d, ls_host, GPBO_KERNEL_SE, jitter1, jitter2, Np, Kp, U, alpha, info, work, work_bytes,
                                   stream);
}

// (the covariance family reaches the K(X,X) build only: everything after it works on the matrix)
extern "C" int gpbo_factorise_kern_f64(const double *X, const double *y, int64_t N, int32_t d, const double *ls_host,
                                       int32_t kernel, double jitter1, double jitter2, int64_t Np, double *Kp, double *U,
                                       double *alpha, int32_t *info, void *work, int64_t work_bytes, void *stream) {
    if (!X || !y || !Kp || !U || !alpha || !info || !work) return GPBO_ERR_ARG;
    if (!kernel_ok(kernel, d)) return GPBO_ERR_ARG;
    if (Np != gpbo_padded_n(N)) return GPBO_ERR_ARG;
    if (work_bytes < gpbo_factorise_workspace_bytes(Np)) return GPBO_ERR_WORKSPACE;
    double *L = reinterpret_cast<double *>(work);
    double *W = L + Np * Np;
    double *dinv = W + Np * Np;
    double *tmp = dinv + Np * NB;
    // Round 3: one sweep of row operations over the stacked matrix S = [K | 0] (cholinv.hip) leaves inv(L) in its right
    // half; U is its transpose.  The two-pass chain of round 2 (blocked Cholesky, then the block-recursive triangular
    // inverse) stays behind GPBO_FACTOR_OLD=1 for A/B runs and behind gpbo_potrf_f64 / gpbo_trtri_f64.
    static const bool old_chain = env_flag("GPBO_FACTOR_OLD");
    // (the fused sweep's plan stops at Np = 32768 - 32-bit tile offsets; beyond, the two-pass chain, which has no such cap)
    if (!old_chain && Np <= GPBO_CHOLINV_MAX_NP) {
        double *S = L;  // [Np x 2 Np]: the same 2 Np^2 doubles
        int rc = gpbo_kxx_launch(X, N, d, ls_host, kernel, jitter1, jitter2, Kp, Np, S, 2 * Np, info, stream);
        if (rc != GPBO_OK) return rc;
        // GPBO_CI_OPTS="win,far_k,far_kind,defer+1,group_from+1,small_w": schedule choices of the plan for A/B runs (cholinv_plan.h)
        static int env_opt[7] = {0, 0, 0, 0, 0, 0, 0};
        static const bool have_env_opt = [] {
            const char *e = env_str("GPBO_CI_OPTS");
            return e && sscanf(e, "%d,%d,%d,%d,%d,%d", &env_opt[0], &env_opt[1], &env_opt[2], &env_opt[3], &env_opt[5], &env_opt[6]) >= 1;
        }();
        rc = gpbo_cholinv_run(S, 2 * Np, Np, info, have_env_opt ? env_opt : nullptr, gpbo_stream(stream));
        if (rc != GPBO_OK) return rc;
        rc = gpbo_launch_transpose_w(S + Np, 2 * Np, Np, U, gpbo_stream(stream));
        if (rc != GPBO_OK) return rc;
        return gpbo_alpha_f64(U, y, N, Np, tmp, alpha, stream);
    }
    // one launch builds K twice (Kp stays as the reference's cov_meas, L is factorised in place) and clears info
    int rc = gpbo_kxx_launch(X, N, d, ls_host, kernel, jitter1, jitter2, Kp, Np, L, Np, info, stream);
    if (rc != GPBO_OK) return rc;
    rc = potrf_run(L, Np, dinv, info, true, stream);
    if (rc != GPBO_OK) return rc;
    rc = gpbo_trtri_f64(L, dinv, Np, U, W, stream);
    if (rc != GPBO_OK) return rc;
    return gpbo_alpha_f64(U, y, N, Np, tmp, alpha, stream);
}
