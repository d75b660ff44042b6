// Noisy expected improvement: EI averaged over fantasies of the incumbent (Letham, Karrer, Ottoni & Bakshy 2019;
// not in the reference, which has no EI at all: its point_selector.py:197-207 is the lower confidence bound).
//
// The observations are noisy, so min(y) is the luckiest noise draw and not the best function value.  With K~ = K0 + rho I the
// factorised matrix, 0 < delta <= rho a nugget and K0d = K0 + delta I the covariance of the LATENT function (the noise then has
// variance rho - delta: the sum is K~ again), S samples of the latent values at the observed points are drawn from the posterior,
// a noise-free model is conditioned on each, and the S expected improvements - each against its own sample's incumbent - are
// averaged.  All S conditioned models share K0d, hence one variance pass; only their means differ.
//
// gpbo_nei_fantasies_f64 (once per factorisation and set of draws; rows = fantasies, [64 x Np], five dense products on the
// matrix cores through gpbo_gemm_launch_tri, U0 U0^T = K0d^-1 and U U^T = K~^-1):
//     nei_pack_kernel      Zp = Z, zero on the padding
//     gemm  B = Zp U0^T    B_s = U0 z_s, so cov(K0d B_s) = K0d exactly and K0d^-1 g_s = B_s by construction (no solve)
//     gemm  G = B K0d      the prior draw g_s at X
//     nei_resid_kernel     R = (y - G) - sqrt(rho - delta) E
//     gemm  T = R U,  gemm  W = T U^T      K~^-1 r_s, the two products gpbo_alpha_f64 makes for one vector
//     nei_sum_kernel       A = B + W        (the weights of fantasy s: mu_s(x) = k(x) . A_s)
//     gemm  F = A K0d      the fantasy values at X: mean K0d K~^-1 y, covariance K0d - K0d K~^-1 K0d
//     nei_rowmin_kernel    best_s = min_{i < N} F_s[i]  (the padding is not read)
// gpbo_posterior_nei_kern_f64 (per candidate set) drives the fp64 pass of every other scoring entry, unchanged, one chunk at a
// time with U0 for the variance; after a chunk's variance launch its K(X*,X)^T image is still in the pass's workspace, and
//     nei_kernel           reads the image ONCE: mu_s for 64 (from 33 fantasies on: 32) candidates x 16 CT fantasies per wave on
//                          v_mfma_f64_16x16x4_f64, then
//                          in registers EI per (candidate, fantasy), the sum over the fantasies, the dense stores, the NaN count
//                          and the workgroup's arg-max record
// Sums run in a fixed order (k ascending in one wave, no split-k; fantasy lanes by a butterfly, column tiles in index order), only
// the integer NaN counter is atomic: two calls give the same bits, and a candidate's means do not depend on the chunk
// (sigma_0 is the pass's own: see gpbo_posterior_nei_kern_f64).
#include "gpbo_internal.h"

#include <cmath>

namespace {

constexpr int NEI_TILE_MIN = 128;                 // fewest candidates per workgroup: four waves of two 16-candidate row tiles
constexpr int64_t NEI_MAX_M = (int64_t)1 << 40;

inline int padded_fantasies(int32_t S) { return (int)align_up(S, 16); }
// candidates per workgroup of nei_kernel: four waves of four row tiles, of two from three column tiles on (the accumulators
// of 4 x 4 tiles leave room for one wave per SIMD only)
inline int nei_tile(int Sp) { return Sp / 16 >= 3 ? 128 : 256; }

// At[n][s] = A[s][n] (zero for s >= S and n >= N): the B operand of nei_kernel, 16 fantasies of one observation contiguous.
// best_p[s] = best[s] (0 for s >= S).  grid ceil(Np Sp / 256), block 256.
__global__ __launch_bounds__(256) void nei_prep_kernel(const double *__restrict__ A, const double *__restrict__ best, int S,
                                                       int Sp, int64_t N, int64_t Np, double *__restrict__ At,
                                                       double *__restrict__ best_p) {
    const int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (e < Sp) best_p[e] = (e < S) ? best[e] : 0.0;
    if (e >= Np * Sp) return;
    const int64_t n = e / Sp;
    const int s = (int)(e - n * Sp);
    At[e] = (s < S && n < N) ? A[(int64_t)s * Np + n] : 0.0;
}

// The hot kernel.  grid ceil(Mc / (64 NEI_ROWS)), block 256.  KsT [Np x ldk]: row n = observation n, column c = candidate c of the
// chunk, rows >= N zero (gpbo_kstar_mu_kern_f64).  A wave owns 16 NEI_ROWS consecutive candidates (NEI_ROWS row tiles of 16: four,
// or two where CT >= 3 - 4 x 4 accumulator tiles would leave one wave per SIMD, measured 2.86 against 1.53 ms per 2^17
// candidates at N = 4096, S = 64) and all 16 CT fantasies:
//     acc[i][t] += KsT[k .. k + 4)[16 candidates of tile i]^T  x  At[k .. k + 4)[16 fantasies of tile t]
// A operand: lane l reads candidate l & 15 of observation row k + (l >> 4): 128 contiguous bytes per row and tile, 512 (256) per
// row and wave.  B operand: At, 2 MB at most, from the cache.  nk = N rounded up to 4 (the rows beyond N are zero on both sides).
// Register r of acc[i][t] in lane l is candidate 16 i + (l >> 4) + 4 r, fantasy 16 t + (l & 15).
// nan0: the pass's own mean with A_0 as its alpha, NaN exactly where a candidate has a NaN coordinate (the image holds zeros
// there: kstar_mu_kernel) - such a candidate is NaN in every fantasy, counts once and is never chosen.
template <int CT, int NEI_ROWS>
__global__ __launch_bounds__(256) void nei_kernel(const double *__restrict__ KsT, int64_t ldk, int nk,
                                                  const double *__restrict__ At, int Sp, const double *__restrict__ best_p, int S,
                                                  double xi, const double *__restrict__ nan0, const double *__restrict__ sigma,
                                                  int64_t Mc, int64_t idx_base, double *__restrict__ mu_out, int64_t ldm,
                                                  double *__restrict__ acq_out, double *__restrict__ part_val,
                                                  int64_t *__restrict__ part_idx, unsigned long long *__restrict__ nan_count) {
    __shared__ double s_val[4];
    __shared__ int64_t s_idx[4];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int l15 = lane & 15, l4 = lane >> 4;
    constexpr int NEI_WAVE = 16 * NEI_ROWS;   // candidates per wave
    constexpr int NEI_UNROLL = 4;
    const int64_t c0 = ((int64_t)blockIdx.x * 4 + wave) * NEI_WAVE;
    d4_t acc[NEI_ROWS][CT];
#pragma unroll
    for (int i = 0; i < NEI_ROWS; ++i)
#pragma unroll
        for (int t = 0; t < CT; ++t) acc[i][t] = d4_t{0.0, 0.0, 0.0, 0.0};
    const double *a_ptr = KsT + (int64_t)l4 * ldk + c0 + l15;
    const double *b_ptr = At + (int64_t)l4 * Sp + l15;
    // NEI_UNROLL k steps per trip, their loads issued before the first product: the loop is bound by the latency of the image's
    // loads, and the compiler does not unroll it when asked by a pragma; the tail in single steps (same order: k ascending)
    int k = 0;
    for (; k + 4 * NEI_UNROLL <= nk; k += 4 * NEI_UNROLL) {
        double a[NEI_UNROLL][NEI_ROWS], b[NEI_UNROLL][CT];
#pragma unroll
        for (int u = 0; u < NEI_UNROLL; ++u) {
#pragma unroll
            for (int i = 0; i < NEI_ROWS; ++i) a[u][i] = a_ptr[(int64_t)(4 * u) * ldk + i * 16];
#pragma unroll
            for (int t = 0; t < CT; ++t) b[u][t] = b_ptr[(int64_t)(4 * u) * Sp + t * 16];
        }
#pragma unroll
        for (int u = 0; u < NEI_UNROLL; ++u)
#pragma unroll
            for (int i = 0; i < NEI_ROWS; ++i)
#pragma unroll
                for (int t = 0; t < CT; ++t) acc[i][t] = mfma_f64_16x16x4(a[u][i], b[u][t], acc[i][t]);
        a_ptr += 4 * NEI_UNROLL * ldk;
        b_ptr += 4 * NEI_UNROLL * (int64_t)Sp;
    }
    for (; k < nk; k += 4) {
        double a[NEI_ROWS], b[CT];
#pragma unroll
        for (int i = 0; i < NEI_ROWS; ++i) a[i] = a_ptr[i * 16];
#pragma unroll
        for (int t = 0; t < CT; ++t) b[t] = b_ptr[t * 16];
#pragma unroll
        for (int i = 0; i < NEI_ROWS; ++i)
#pragma unroll
            for (int t = 0; t < CT; ++t) acc[i][t] = mfma_f64_16x16x4(a[i], b[t], acc[i][t]);
        a_ptr += 4 * ldk;
        b_ptr += 4 * (int64_t)Sp;
    }
    double bs[CT];
#pragma unroll
    for (int t = 0; t < CT; ++t) bs[t] = best_p[t * 16 + l15];
    // EI per (candidate, fantasy); the 16 fantasy lanes by a butterfly (every lane of the group ends with the same bits), the
    // column tiles in index order; then lane l & 15 = 4 i + r keeps candidate 16 i + (l >> 4) + 4 r for the stores and the arg-max
    double mine = 0.0;
#pragma unroll
    for (int i = 0; i < NEI_ROWS; ++i)
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const int64_t c = c0 + i * 16 + l4 + 4 * r;
            const bool valid = c < Mc;
            const double sg = valid ? sigma[c] : 0.0;
            const double flag = valid ? nan0[c] : 0.0;
            double sum = 0.0;
#pragma unroll
            for (int t = 0; t < CT; ++t) {
                const int s = t * 16 + l15;
                const double m = (flag != flag) ? flag : acc[i][t][r];
                if (mu_out && valid && s < S) mu_out[(int64_t)s * ldm + c] = m;
                double e = gpbo_acquisition(GPBO_ACQ_EI, m, sg, bs[t], xi);
                e = (s < S) ? e : 0.0;   // a padded fantasy has weight 0
#pragma unroll
                for (int off = 1; off < 16; off <<= 1) e += __shfl_xor(e, off);
                sum += e;
            }
            if (l15 == 4 * i + r) mine = sum / (double)S;
        }
    const int64_t c = c0 + (l15 >> 2) * 16 + l4 + 4 * (l15 & 3);
    const bool valid = l15 < 4 * NEI_ROWS && c < Mc;
    if (valid && acq_out) acq_out[c] = mine;
    const bool is_nan = valid && (mine != mine);
    gpbo_count_nan(is_nan, lane, nan_count);
    double bv = (valid && !is_nan) ? mine : gpbo_none::val;
    int64_t bi = (valid && !is_nan) ? idx_base + c : gpbo_none::idx;
    gpbo_argmax_post(bv, bi, lane, wave, s_val, s_idx);
    gpbo_syncthreads();
    if (tid == 0) {
        gpbo_argmax_fold(s_val, s_idx, 4, bv, bi);
        part_val[blockIdx.x] = bv;
        part_idx[blockIdx.x] = bi;
    }
}

// Zp[s][n] = Z[s][n], zero on the padding (rows s >= S, columns n >= N).  grid ceil(64 Np / 256), block 256.
__global__ __launch_bounds__(256) void nei_pack_kernel(const double *__restrict__ Z, int S, int64_t N, int64_t Np,
                                                       double *__restrict__ Zp) {
    const int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (e >= 64 * Np) return;
    const int64_t s = e / Np, n = e - s * Np;
    Zp[e] = (s < S && n < N) ? Z[s * N + n] : 0.0;
}

// R[s][n] = (y[n] - G[s][n]) - sd E[s][n] in place of G, zero on the padding.  grid ceil(64 Np / 256), block 256.
__global__ __launch_bounds__(256) void nei_resid_kernel(const double *__restrict__ y, const double *__restrict__ E, int S,
                                                        int64_t N, int64_t Np, double sd, double *__restrict__ GR) {
    const int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (e >= 64 * Np) return;
    const int64_t s = e / Np, n = e - s * Np;
    GR[e] = (s < S && n < N) ? (y[n] - GR[e]) - sd * E[s * N + n] : 0.0;
}

// A = B + W in place of B (all 64 rows: the next product reads them), and the first S rows to A_out.
__global__ __launch_bounds__(256) void nei_sum_kernel(double *__restrict__ B, const double *__restrict__ W, int S, int64_t Np,
                                                      double *__restrict__ A_out) {
    const int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (e >= 64 * Np) return;
    const double a = B[e] + W[e];
    B[e] = a;
    if (e < (int64_t)S * Np) A_out[e] = a;
}

// A workgroup per fantasy: F_out[s] = F[s] (padding included: zeros) and best[s] = min over the N observations, the padding
// NOT read for the minimum (a padding zero would win over positive values).  grid S, block 256.
__global__ __launch_bounds__(256) void nei_rowmin_kernel(const double *__restrict__ F, int64_t N, int64_t Np,
                                                         double *__restrict__ F_out, double *__restrict__ best) {
    __shared__ double s_min[4];
    const int tid = threadIdx.x, lane = tid & 63;
    const int64_t s = blockIdx.x;
    double m = __builtin_huge_val();
    for (int64_t n = tid; n < Np; n += 256) {
        const double f = F[s * Np + n];
        F_out[s * Np + n] = f;
        if (n < N) m = fmin(m, f);
    }
#pragma unroll
    for (int off = 1; off < 64; off <<= 1) m = fmin(m, __shfl_xor(m, off));
    if (lane == 0) s_min[tid >> 6] = m;
    gpbo_syncthreads();
    if (tid == 0) best[s] = fmin(fmin(s_min[0], s_min[1]), fmin(s_min[2], s_min[3]));
}

struct FantasyLayout {   // three [64 x Np] matrices
    double *P, *Q, *R;
    int64_t total;
    FantasyLayout(void *work, int64_t Np) {
        Carver c(work);
        P = c.take<double>(64 * Np);
        Q = c.take<double>(64 * Np);
        R = c.take<double>(64 * Np);
        total = c.total();
    }
};

struct NeiLayout {
    void *post_work;   // the workspace of a one-chunk fp64 pass, post bytes
    double *at, *best, *nan0, *sigma, *pval;
    int64_t *pidx;
    unsigned long long *nan;
    gpbo_result *res;   // the pass's own result record: not reported
    int64_t post, total;
    NeiLayout(void *work, int64_t Np, int64_t chunk, int64_t M, int32_t S) {
        Carver c(work);
        post = gpbo_posterior_workspace_bytes_split(Np, chunk, M < chunk ? M : chunk, 1);   // one chunk per call
        const int64_t nparts = (M + NEI_TILE_MIN - 1) / NEI_TILE_MIN;   // (capacity: the wider tile writes fewer)
        post_work = c.take_bytes(post);
        at = c.take<double>(Np * padded_fantasies(S));
        best = c.take<double>(GPBO_NEI_MAX_S);
        nan0 = c.take<double>(M);
        sigma = c.take<double>(M);
        pval = c.take<double>(nparts);
        pidx = c.take<int64_t>(nparts);
        nan = c.take<unsigned long long>(32);   // 256 bytes
        res = static_cast<gpbo_result *>(c.take_bytes(256));
        total = c.total();
    }
};

bool fantasies_ok(int32_t S) { return S >= 1 && S <= GPBO_NEI_MAX_S; }
bool is_finite(double v) { return v - v == 0.0; }

// nei_kernel on the image of the chunk that starts at candidate `start`.
struct NeiRun {
    int64_t N;
    const double *At, *best_p, *nan0, *sigma;
    int S, Sp;
    double xi;
    int64_t idx_offset;
    double *mu_out;
    int64_t ldm;
    double *acq_out, *part_val;
    int64_t *part_idx;
    unsigned long long *nan_count;
};

int nei_chunk(const NeiRun &r, int64_t start, int64_t Mc, const double *KsT, int64_t ldk, hipStream_t st) {
    const int tile = nei_tile(r.Sp);
    const dim3 grid((unsigned)((Mc + tile - 1) / tile));
    const int nk = (int)align_up(r.N, 4);
    const int64_t p0 = start / tile;   // (chunks are multiples of 512 candidates: the records of a call are contiguous)
#define GPBO_NEI_LAUNCH(CT, ROWS)                                                                                               \
    hipLaunchKernelGGL((nei_kernel<CT, ROWS>), grid, dim3(256), 0, st, KsT, ldk, nk, r.At, r.Sp, r.best_p, r.S, r.xi, r.nan0 + start, \
                       r.sigma + start, Mc, r.idx_offset + start, r.mu_out ? r.mu_out + start : nullptr, r.ldm,                 \
                       r.acq_out ? r.acq_out + start : nullptr, r.part_val + p0, r.part_idx + p0, r.nan_count)
    switch (r.Sp / 16) {
        case 1: GPBO_NEI_LAUNCH(1, 4); break;
        case 2: GPBO_NEI_LAUNCH(2, 4); break;
        case 3: GPBO_NEI_LAUNCH(3, 2); break;
        default: GPBO_NEI_LAUNCH(4, 2); break;
    }
#undef GPBO_NEI_LAUNCH
    GPBO_CHECK_LAUNCH();
    return GPBO_OK;
}

}  // namespace

extern "C" int64_t gpbo_nei_fantasies_workspace_bytes(int64_t Np, int32_t S) {
    if (!np_ok(Np) || Np > (1 << 20) || !fantasies_ok(S)) return GPBO_ERR_ARG;
    return FantasyLayout(nullptr, Np).total;
}

extern "C" int gpbo_nei_fantasies_f64(const double *K0d, const double *U0, const double *U, const double *y, int64_t N,
                                      int64_t Np, const double *Z, const double *E, double noise_sd, int32_t S, double *A_out,
                                      double *F_out, double *best_out, void *work, int64_t work_bytes, void *stream) {
    if (!K0d || !U0 || !U || !y || !Z || !E || !A_out || !F_out || !best_out || !work) return GPBO_ERR_ARG;
    if (!fantasies_ok(S) || N < 1 || !np_ok(Np) || Np > (1 << 20) || N > Np) return GPBO_ERR_ARG;
    if (!(noise_sd >= 0.0) || !is_finite(noise_sd)) return GPBO_ERR_ARG;
    if (!aligned_to(K0d, 16) || !aligned_to(U0, 16) || !aligned_to(U, 16)) return GPBO_ERR_ARG;   // the GEMM's B operands
    const FantasyLayout L(work, Np);
    if (work_bytes < L.total || !aligned_to(work, 256)) return GPBO_ERR_WORKSPACE;
    hipStream_t st = gpbo_stream(stream);
    double *P = L.P, *Q = L.Q, *R = L.R;
    const dim3 grid((unsigned)((64 * Np + 255) / 256));
    hipLaunchKernelGGL(nei_pack_kernel, grid, dim3(256), 0, st, Z, (int)S, N, Np, P);
    GPBO_CHECK_LAUNCH();
    // (U0, U upper triangular, K0d symmetric with the identity on its padding; every product runs dense)
    int rc = gpbo_gemm_launch_tri(1, 64, Np, Np, 1.0, P, Np, 0, U0, Np, 0, 0.0, Q, Np, 0, 1, 0, 0, st);    // B = Zp U0^T
    if (rc != GPBO_OK) return rc;
    rc = gpbo_gemm_launch_tri(0, 64, Np, Np, 1.0, Q, Np, 0, K0d, Np, 0, 0.0, P, Np, 0, 1, 0, 0, st);       // G = B K0d
    if (rc != GPBO_OK) return rc;
    hipLaunchKernelGGL(nei_resid_kernel, grid, dim3(256), 0, st, y, E, (int)S, N, Np, noise_sd, P);       // R in place of G
    GPBO_CHECK_LAUNCH();
    rc = gpbo_gemm_launch_tri(0, 64, Np, Np, 1.0, P, Np, 0, U, Np, 0, 0.0, R, Np, 0, 1, 0, 0, st);         // T = R U
    if (rc != GPBO_OK) return rc;
    rc = gpbo_gemm_launch_tri(1, 64, Np, Np, 1.0, R, Np, 0, U, Np, 0, 0.0, P, Np, 0, 1, 0, 0, st);         // W = T U^T
    if (rc != GPBO_OK) return rc;
    hipLaunchKernelGGL(nei_sum_kernel, grid, dim3(256), 0, st, Q, P, (int)S, Np, A_out);                  // A = B + W
    GPBO_CHECK_LAUNCH();
    rc = gpbo_gemm_launch_tri(0, 64, Np, Np, 1.0, Q, Np, 0, K0d, Np, 0, 0.0, P, Np, 0, 1, 0, 0, st);       // F = A K0d
    if (rc != GPBO_OK) return rc;
    hipLaunchKernelGGL(nei_rowmin_kernel, dim3((unsigned)S), dim3(256), 0, st, P, N, Np, F_out, best_out);
    GPBO_CHECK_LAUNCH();
    return GPBO_OK;
}

extern "C" int64_t gpbo_posterior_nei_workspace_bytes(int64_t Np, int64_t chunk, int64_t M, int32_t S) {
    if (gpbo_posterior_workspace_bytes_split(Np, chunk, M, 1) < 0 || M > NEI_MAX_M || !fantasies_ok(S)) return GPBO_ERR_ARG;
    return NeiLayout(nullptr, Np, chunk, M, S).total;
}

extern "C" int gpbo_posterior_nei_kern_f64(const double *Xs, int64_t M, const double *X, int64_t N, int64_t Np, int32_t d,
                                           const double *ls_host, int32_t kernel, const double *U0, const double *A,
                                           const double *best, int32_t S, double prior_var, double xi, int64_t idx_offset,
                                           int64_t chunk, double *mu_out, int64_t ldm, double *sigma_out, double *acq_out,
                                           gpbo_result *result, void *work, int64_t work_bytes, void *stream) {
    if (!Xs || !X || !ls_host || !U0 || !A || !best || !result || !work) return GPBO_ERR_ARG;
    if (!fantasies_ok(S) || d < 1 || d > GPBO_MAX_D || !kernel_ok(kernel, d)) return GPBO_ERR_ARG;
    if (M < 1 || M > NEI_MAX_M || N < 1 || Np != gpbo_padded_n(N) || Np > (1 << 20)) return GPBO_ERR_ARG;
    if (!chunk_ok(chunk) || !length_scales_ok(ls_host, d)) return GPBO_ERR_ARG;
    if (!(prior_var > 0.0) || !is_finite(prior_var) || !is_finite(xi) || (mu_out && ldm < M)) return GPBO_ERR_ARG;
    if (!aligned_to(U0, 16)) return GPBO_ERR_ARG;
    if (!aligned_to(work, 256)) return GPBO_ERR_WORKSPACE;
    const NeiLayout L(work, Np, chunk, M, S);
    if (work_bytes < L.total) return GPBO_ERR_WORKSPACE;
    hipStream_t st = gpbo_stream(stream);
    double *At = L.at, *best_p = L.best, *nan0 = L.nan0;
    double *sigma = sigma_out ? sigma_out : L.sigma;
    unsigned long long *nan_count = L.nan;
    gpbo_result *scratch = L.res;
    const int Sp = padded_fantasies(S);
    if (hipMemsetAsync(nan_count, 0, sizeof(unsigned long long), st) != hipSuccess) return GPBO_ERR_LAUNCH;
    hipLaunchKernelGGL(nei_prep_kernel, dim3((unsigned)((Np * Sp + 255) / 256)), dim3(256), 0, st, A, best, (int)S, Sp, N, Np, At,
                       best_p);
    GPBO_CHECK_LAUNCH();
    NeiRun run = {N, At, best_p, nan0, sigma, (int)S, Sp, xi, idx_offset, mu_out, ldm, acq_out, L.pval, L.pidx, nan_count};
    // The pass with the twin's factor, one chunk per call: sigma_0 of the chunk's candidates, its own mean with A_0 as alpha -
    // which marks the candidates with a NaN coordinate - and, left behind in its workspace, the chunk's K(X*,X)^T image.  The
    // pass's acquisition and arg-max are not used (LCB with explore 0 is the cheapest it has).
    // (The pass chooses the column groups of its variance kernel by the candidates of the CALL - here the chunk - from 32,768
    // candidates and N > 1,920 on: across that line sigma_0 differs by the rounding of another summation order, 1e-16 relative.
    // The means never depend on the chunk.)
    const GpModel gp = {X, N, Np, d, ls_host, U0, A, prior_var, kernel};
    for (int64_t s = 0; s < M; s += chunk) {
        const int64_t Mc = (M - s < chunk) ? (M - s) : chunk;
        int rc = gpbo_posterior_acq_f64_split(Xs + s * d, Mc, gp, {GPBO_ACQ_LCB, 0.0, 0.0}, 0.0, idx_offset + s, chunk,
                                              {nan0 + s, sigma + s, nullptr, nullptr}, scratch, L.post_work, L.post, nullptr, 1, 0,
                                              stream);
        if (rc != GPBO_OK) return rc;
        rc = nei_chunk(run, s, Mc, gpbo_posterior_chunk_image(L.post_work, Np, chunk, Mc), chunk, st);
        if (rc != GPBO_OK) return rc;
    }
    const int tile = nei_tile(Sp);
    return gpbo_launch_argmax_finish(run.part_val, run.part_idx, (M + tile - 1) / tile, nan_count, result, st);
}
