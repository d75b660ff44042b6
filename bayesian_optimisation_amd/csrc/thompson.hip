// Thompson sampling by pathwise posterior samples (not in the reference, whose acquisition is a function of
// (mean_func, cov_func) alone: its point_selector.py:197-207).
//
// Pathwise conditioning (Wilson et al. 2020, "Efficiently sampling functions from Gaussian process posteriors") writes a
// sample of the posterior FUNCTION at any point x as
//     f_s(x) = g_s(x) + sum_n k0(x, x_n) v_s[n]
//     g_s(x) = sqrt(2 / F) sum_f W[s,f] cos(2 pi t_f(x)),   t_f(x) = sum_k Omega[f,k] x_k / (2 pi ls_k) + phase[f]   (turns)
//     v_s    = K^-1 (y - g_s(X) - sqrt(kappa) E[s,:]),      kappa = jitter1 + jitter2,  K = k0(X,X) + kappa I
// g_s is a random-Fourier-feature draw of the ARD-SE prior, the second term is the mean's own sum with v_s in the place of
// alpha.  The random draws (Omega, phase, W, E) are INPUTS (as Z is for gpbo_posterior_qei_f64).  Per candidate the N kernel
// entries and the F feature cosines are generated once, in registers, and shared by all S paths; nothing of K(X*,X) is
// stored and no variance pass is needed.
//
// gpbo_thompson_weights_f64 (once per factorisation and set of draws):
//     thompson_paths_kernel    G = g_s(X): the hot kernel itself with the observations as its points and no V
//     thompson_resid_kernel    R = (y - G) - sqrt(kappa) E, rows padded to 64
//     gemm  T = R U, gemm  V = T U^T    (the two dense products of refine.hip; U = L^-T, so U U^T = K^-1)
// gpbo_thompson_paths_f64 (per candidate set): one launch over all M candidates plus a finish
//     thompson_prep_kernel     Om = Omega / (2 pi ls), W and V transposed to [F x Sp] / [N x Sp]: the values of all paths of a
//                              group for one feature / observation are contiguous and wave-uniform (scalar loads)
//     thompson_paths_kernel    every candidate: f_s, the optional dense output, NaN counts, block arg-max of -f_s per path
//     thompson_finish_kernel   per path: the lowest row attaining the maximum over the blocks
// Sums run in a fixed order, only the integer NaN counters use atomics: two calls give the same bits.
#include "gpbo_internal.h"

#include <cmath>
#include <limits>

#include "cov_entry.h"

namespace {

struct TsScale {
    double isc[GPBO_MAX_D];   // 1 / (ls_k sqrt 2): the scoring form of cov_entry.h
    double tl[GPBO_MAX_D];    // 2 pi ls_k
};

constexpr int TS_CANDS = 512;          // candidates per workgroup: 256 threads, two adjacent candidates each
constexpr int TS_GROUP = 16;           // paths per launch row (accumulators per candidate in registers)
constexpr int TS_GROUP_SMALL = 4;      // ... for S <= 4
constexpr int64_t TS_MAX_M = (int64_t)1 << 31;

inline int group_of(int32_t S) { return S <= TS_GROUP_SMALL ? TS_GROUP_SMALL : TS_GROUP; }
inline int64_t padded_paths(int32_t S) { return align_up(S, group_of(S)); }

// cos(2 pi t) for an angle t in turns, full fp64 accuracy (1.7 ulp of 1 against a long-double cosine over 2 * 10^6 angles in
// [-8, 8]; exact at the quarter turns).  r = t - rint(t) is exact, cos(2 pi r) = sin(2 pi q) with q = 1/4 - |r| in
// [-1/4, 1/4], and sin(2 pi q) = q P(q^2) by the Taylor series to (2 pi q)^21 (the next term is 1.3e-18 at the ends).
// 19 fp64 instructions where cospi() compiled to 85 (its own reduction and a two-branch select): -DGPBO_TS_COSPI builds
// that form for A/B runs (tools/bench_thompson.py).
__device__ __forceinline__ double cos_turns(double t) {
#ifdef GPBO_TS_COSPI
    return cospi(2.0 * t);
#else
    const double r = t - rint(t);
    const double q = 0.25 - fabs(r);
    const double z = q * q;
    double p = 1.13092374825179628e-03;
    p = fma(p, z, -1.20315859421206272e-02);
    p = fma(p, z, 1.04229162208139839e-01);
    p = fma(p, z, -7.18122301778500560e-01);
    p = fma(p, z, 3.81995258484828204e+00);
    p = fma(p, z, -1.50946425768229897e+01);
    p = fma(p, z, 4.20586939448976551e+01);
    p = fma(p, z, -7.67058597530613895e+01);
    p = fma(p, z, 8.16052492760750567e+01);
    p = fma(p, z, -4.13417022403997620e+01);
    p = fma(p, z, 6.28318530717958623e+00);
    return q * p;
#endif
}

// Om[f][k] = Omega[f][k] / (2 pi ls_k);  Wt[f][s] = W[s][f];  Vt[n][s] = V[s][n]  (zero for s >= S).  grid-stride free:
// grid ceil(max(F d, F Sp, N Sp) / 256), block 256.
__global__ __launch_bounds__(256) void thompson_prep_kernel(const double *__restrict__ omega, const double *__restrict__ W,
                                                            const double *__restrict__ V, int F, int S, int Sp, int d, int N,
                                                            int64_t Np, TsScale sc, double *__restrict__ Om,
                                                            double *__restrict__ Wt, double *__restrict__ Vt) {
    const int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (e < (int64_t)F * d) Om[e] = omega[e] / sc.tl[e % d];
    if (e < (int64_t)F * Sp) {
        const int64_t f = e / Sp;
        const int s = (int)(e - f * Sp);
        Wt[e] = (s < S) ? W[(int64_t)s * F + f] : 0.0;
    }
    if (V && e < (int64_t)N * Sp) {
        const int64_t n = e / Sp;
        const int s = (int)(e - n * Sp);
        Vt[e] = (s < S) ? V[(int64_t)s * Np + n] : 0.0;
    }
}

// The hot kernel.  grid (ceil(M / 512), Sp / G), block 256.  A thread owns two adjacent candidates and G path accumulators
// for each.  First the F features: the angle in turns by an FMA chain from the phase (omega rows, the phase and the W column
// of the group are wave-uniform: scalar loads), cos_turns(t) (the reduction is exact in turns), G multiply-adds per candidate
// against scalar operands; the sums are scaled by sqrt(2 / F) once.  Then the N observations in the difference form on
// coordinates pre-scaled by 1 / (ls sqrt 2) with exp_neg() - the fp64 path's own arithmetic - and G multiply-adds against
// the V row of the observation.  N = 0 (no V): the prior paths alone.  A row with a non-finite coordinate is NaN in every
// path.  part_val == null: no arg-max (the weights call wants the dense output only).
template <int D, int G>
__global__ __launch_bounds__(256) void thompson_paths_kernel(
    const double *__restrict__ Xs, int64_t M, const double *__restrict__ Xsc, int N, TsScale sc,
    const double *__restrict__ Vt, const double *__restrict__ Om, const double *__restrict__ phase,
    const double *__restrict__ Wt, int F, int S, int Sp, double amp, int64_t idx_offset, double *__restrict__ f_out,
    int64_t ldf, double *__restrict__ part_val, int64_t *__restrict__ part_idx, int64_t nblk,
    unsigned long long *__restrict__ nan_count) {
    __shared__ double tab[GPBO_EXP_E];
    __shared__ double s_val[4][G];
    __shared__ int64_t s_idx[4][G];
    const int tid = threadIdx.x, lane = tid & 63;
    cov_stage_tab(tab, tid);
    const int g0 = blockIdx.y * G;
    const int64_t c0 = ((int64_t)blockIdx.x * 256 + tid) * 2;
    const bool va = c0 < M, vb = c0 + 1 < M;
    double fa[G], fb[G];
#pragma unroll
    for (int g = 0; g < G; ++g) fa[g] = fb[g] = 0.0;
    bool fin_a = true, fin_b = true;
    {
        double xa[D], xb[D];
#pragma unroll
        for (int k = 0; k < D; ++k) {
            xa[k] = va ? Xs[c0 * D + k] : 0.0;
            xb[k] = vb ? Xs[(c0 + 1) * D + k] : 0.0;
            fin_a = fin_a && (xa[k] - xa[k] == 0.0);
            fin_b = fin_b && (xb[k] - xb[k] == 0.0);
        }
        for (int f = 0; f < F; ++f) {
            const double *om = Om + (int64_t)f * D;    // wave-uniform -> scalar loads
            const double *w = Wt + (int64_t)f * Sp + g0;
            double ta = phase[f], tb = ta;
#pragma unroll
            for (int k = 0; k < D; ++k) {
                const double o = om[k];
                ta = fma(o, xa[k], ta);
                tb = fma(o, xb[k], tb);
            }
            const double ca = cos_turns(ta), cb = cos_turns(tb);
#pragma unroll
            for (int g = 0; g < G; ++g) {
                const double wg = w[g];
                fa[g] = fma(ca, wg, fa[g]);
                fb[g] = fma(cb, wg, fb[g]);
            }
        }
#pragma unroll
        for (int g = 0; g < G; ++g) {
            fa[g] *= amp;
            fb[g] *= amp;
        }
#pragma unroll
        for (int k = 0; k < D; ++k) {
            xa[k] *= sc.isc[k];
            xb[k] *= sc.isc[k];
        }
        gpbo_syncthreads();   // tab
        for (int n = 0; n < N; ++n) {
            const double *xo = Xsc + (int64_t)n * D;   // wave-uniform -> scalar loads
            const double *v = Vt + (int64_t)n * Sp + g0;
            double sa = 0.0, sb = 0.0;   // cov_s2 of cov_entry.h, written out (see there)
#pragma unroll
            for (int k = 0; k < D; ++k) {
                const double o = xo[k];
                const double da = xa[k] - o, db = xb[k] - o;
                sa = fma(da, da, sa);
                sb = fma(db, db, sb);
            }
            const double ka = cov_from_s<GPBO_KERNEL_SE>(sa, tab), kb = cov_from_s<GPBO_KERNEL_SE>(sb, tab);
#pragma unroll
            for (int g = 0; g < G; ++g) {
                const double vg = v[g];
                fa[g] = fma(ka, vg, fa[g]);
                fb[g] = fma(kb, vg, fb[g]);
            }
        }
    }
    const double nan = __builtin_nan("");
#pragma unroll
    for (int g = 0; g < G; ++g) {
        const int s = g0 + g;
        if (s < S) {   // uniform
            const double a = fin_a ? fa[g] : nan, b = fin_b ? fb[g] : nan;   // (exp_neg returns 0 for a NaN argument)
            if (f_out) {
                if (va) f_out[(int64_t)s * ldf + c0] = a;
                if (vb) f_out[(int64_t)s * ldf + c0 + 1] = b;
            }
            if (part_val) {
                const bool nan_a = va && (a != a), nan_b = vb && (b != b);
                const unsigned long long mask_a = __ballot(nan_a), mask_b = __ballot(nan_b);
                if (lane == 0 && (mask_a | mask_b))
                    atomicAdd(nan_count + s, (unsigned long long)(__popcll(mask_a) + __popcll(mask_b)));
                const bool use_a = va && !nan_a, use_b = vb && !nan_b;
                double bv = use_a ? -a : gpbo_none::val;
                int64_t bi = use_a ? idx_offset + c0 : gpbo_none::idx;
                if (use_b && gpbo_better(-b, idx_offset + c0 + 1, bv, bi)) { bv = -b; bi = idx_offset + c0 + 1; }
                gpbo_argmax_post(bv, bi, lane, tid >> 6, &s_val[0][g], &s_idx[0][g], G);
            }
        }
    }
    if (!part_val) return;
    gpbo_syncthreads();
    if (tid < G && g0 + tid < S) {   // a thread per path folds the waves' entries of that path
        double bv;
        int64_t bi;
        gpbo_argmax_fold(&s_val[0][tid], &s_idx[0][tid], 4, bv, bi, G);
        part_val[(int64_t)(g0 + tid) * nblk + blockIdx.x] = bv;
        part_idx[(int64_t)(g0 + tid) * nblk + blockIdx.x] = bi;
    }
}

// A workgroup per path: the block records of that path in a fixed order.  grid S, block 256.
__global__ __launch_bounds__(256) void thompson_finish_kernel(const double *__restrict__ part_val,
                                                              const int64_t *__restrict__ part_idx, int64_t nblk,
                                                              const unsigned long long *__restrict__ nan_count,
                                                              int64_t *__restrict__ idx_out, double *__restrict__ val_out,
                                                              int64_t *__restrict__ nan_out) {
    __shared__ double s_val[4];
    __shared__ int64_t s_idx[4];
    const int tid = threadIdx.x, lane = tid & 63;
    const int64_t s = blockIdx.x;
    double bv = gpbo_none::val;
    int64_t bi = gpbo_none::idx;
    for (int64_t p = tid; p < nblk; p += 256) {
        const double v = part_val[s * nblk + p];
        const int64_t i = part_idx[s * nblk + p];
        if (gpbo_better(v, i, bv, bi)) { bv = v; bi = i; }
    }
    gpbo_argmax_post(bv, bi, lane, tid >> 6, s_val, s_idx);
    gpbo_syncthreads();
    if (tid == 0) {
        gpbo_argmax_fold(s_val, s_idx, 4, bv, bi);
        idx_out[s] = (bi == gpbo_none::idx) ? -1 : bi;
        val_out[s] = (bi == gpbo_none::idx) ? __builtin_nan("") : bv;
        nan_out[s] = (int64_t)nan_count[s];
    }
}

// R[s][n] = (y[n] - G[s][n]) - sqrt(kappa) E[s][n], zero on the padding (rows s >= S, columns n >= N).
// grid ceil(S64 Np / 256), block 256.
__global__ __launch_bounds__(256) void thompson_resid_kernel(const double *__restrict__ y, const double *__restrict__ Gm,
                                                             const double *__restrict__ E, int S, int64_t S64, int64_t N,
                                                             int64_t Np, double sk, double *__restrict__ R) {
    const int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (e >= S64 * Np) return;
    const int64_t s = e / Np, n = e - s * Np;
    R[e] = (s < S && n < N) ? (y[n] - Gm[e]) - sk * E[s * N + n] : 0.0;
}

struct PathsLayout {
    double *xsc, *vt, *om, *wt, *part_val;
    int64_t *part_idx;
    unsigned long long *nan;
    int64_t Sp, nblk, total;
    PathsLayout(void *work, int64_t Np, int64_t M, int32_t F, int32_t S) {
        Carver c(work);
        Sp = padded_paths(S);
        nblk = (M + TS_CANDS - 1) / TS_CANDS;
        xsc = c.take<double>(Np * GPBO_MAX_D);
        vt = c.take<double>(Np * Sp);
        om = c.take<double>((int64_t)F * GPBO_MAX_D);
        wt = c.take<double>((int64_t)F * Sp);
        part_val = c.take<double>(Sp * nblk);
        part_idx = c.take<int64_t>(Sp * nblk);
        nan = c.take<unsigned long long>(Sp);
        total = c.total();
    }
};

struct WeightsLayout {
    double *a, *b;   // G = g_s(X), then T = R U;  R, then V with its rows padded to 64
    void *paths;     // the workspace of the inner paths call over the Np observations
    int64_t S64, total;
    WeightsLayout(void *work, int64_t Np, int32_t F, int32_t S) {
        Carver c(work);
        S64 = align_up(S, 64);
        a = c.take<double>(S64 * Np);
        b = c.take<double>(S64 * Np);
        c.take_bytes(3 * align_up(8 * GPBO_TS_MAX_PATHS, 256));   // the arg-max outputs of the inner paths call (unused)
        paths = c.take_bytes(PathsLayout(nullptr, Np, Np, F, S).total);
        total = c.total();
    }
};

bool draws_ok(int32_t F, int32_t S) { return F >= 1 && F <= GPBO_TS_MAX_FEATURES && S >= 1 && S <= GPBO_TS_MAX_PATHS; }
bool sizes_ok(int64_t Np, int32_t F, int32_t S) { return np_ok(Np) && Np <= (1 << 20) && draws_ok(F, S); }

template <int D>
void launch_paths(int G, dim3 grid, hipStream_t st, const double *Xs, int64_t M, const double *Xsc, int N, const TsScale &sc,
                  const double *Vt, const double *Om, const double *phase, const double *Wt, int F, int S, int Sp, double amp,
                  int64_t idx_offset, double *f_out, int64_t ldf, double *part_val, int64_t *part_idx, int64_t nblk,
                  unsigned long long *nan_count) {
    if (G == TS_GROUP_SMALL)
        hipLaunchKernelGGL((thompson_paths_kernel<D, TS_GROUP_SMALL>), grid, dim3(256), 0, st, Xs, M, Xsc, N, sc, Vt, Om, phase,
                           Wt, F, S, Sp, amp, idx_offset, f_out, ldf, part_val, part_idx, nblk, nan_count);
    else
        hipLaunchKernelGGL((thompson_paths_kernel<D, TS_GROUP>), grid, dim3(256), 0, st, Xs, M, Xsc, N, sc, Vt, Om, phase, Wt,
                           F, S, Sp, amp, idx_offset, f_out, ldf, part_val, part_idx, nblk, nan_count);
}

// The launches of gpbo_thompson_paths_f64 once its arguments have been checked.  want_argmax = false: f_out only.
int run_paths(const double *Xs, int64_t M, const double *X, int64_t N, int64_t Np, int32_t d, const double *ls_host,
              const double *omega, const double *phase, const double *W, const double *V, int32_t F, int32_t S,
              int64_t idx_offset, double *f_out, int64_t ldf, int64_t *idx_out, double *val_out, int64_t *nan_out,
              bool want_argmax, void *work, void *stream) {
    const PathsLayout L(work, Np, M, F, S);
    hipStream_t st = gpbo_stream(stream);
    TsScale sc;
    for (int k = 0; k < GPBO_MAX_D; ++k) sc.isc[k] = sc.tl[k] = 1.0;
    (void)length_scale_scalings(ls_host, d, nullptr, sc.isc);   // (cannot refuse: the arguments have been checked)
    for (int k = 0; k < d; ++k) sc.tl[k] = 6.283185307179586477 * ls_host[k];
    const int Sp = (int)L.Sp, G = group_of(S);
    const int Nk = V ? (int)N : 0;
    if (V) {
        int rc = gpbo_scale_points_launch(X, N, Np, d, ls_host, L.xsc, nullptr, stream);
        if (rc != GPBO_OK) return rc;
    }
    if (want_argmax && hipMemsetAsync(L.nan, 0, 8 * (size_t)Sp, st) != hipSuccess) return GPBO_ERR_LAUNCH;
    int64_t prep = (int64_t)F * (Sp > d ? Sp : d);
    if ((int64_t)Nk * Sp > prep) prep = (int64_t)Nk * Sp;
    hipLaunchKernelGGL(thompson_prep_kernel, dim3((unsigned)((prep + 255) / 256)), dim3(256), 0, st, omega, W, V, (int)F, (int)S,
                       Sp, (int)d, Nk, Np, sc, L.om, L.wt, L.vt);
    GPBO_CHECK_LAUNCH();
    const dim3 grid((unsigned)L.nblk, (unsigned)(Sp / G));
    const double amp = sqrt(2.0 / (double)F);
#define CALL(DD)                                                                                                                  \
    launch_paths<DD>(G, grid, st, Xs, M, L.xsc, Nk, sc, L.vt, L.om, phase, L.wt, (int)F, (int)S, Sp, amp, idx_offset, f_out, ldf, \
                     want_argmax ? L.part_val : nullptr, L.part_idx, L.nblk, L.nan)
    GPBO_FOR_D(d, CALL)
#undef CALL
    GPBO_CHECK_LAUNCH();
    if (!want_argmax) return GPBO_OK;
    hipLaunchKernelGGL(thompson_finish_kernel, dim3((unsigned)S), dim3(256), 0, st, L.part_val, L.part_idx, L.nblk, L.nan,
                       idx_out, val_out, nan_out);
    GPBO_CHECK_LAUNCH();
    return GPBO_OK;
}

bool model_ok(const double *X, int64_t N, int64_t Np, int32_t d, const double *ls_host, int32_t F, int32_t S) {
    if (!X || !ls_host) return false;
    if (d < 1 || d > GPBO_MAX_D || N < 1 || !sizes_ok(Np, F, S) || N > Np) return false;
    return length_scales_ok(ls_host, d);
}

}  // namespace

extern "C" int64_t gpbo_thompson_paths_workspace_bytes(int64_t Np, int64_t M, int32_t F, int32_t S) {
    if (!sizes_ok(Np, F, S) || M < 1 || M > TS_MAX_M) return GPBO_ERR_ARG;
    return PathsLayout(nullptr, Np, M, F, S).total;
}

extern "C" int64_t gpbo_thompson_weights_workspace_bytes(int64_t Np, int32_t F, int32_t S) {
    if (!sizes_ok(Np, F, S)) return GPBO_ERR_ARG;
    return WeightsLayout(nullptr, Np, F, S).total;
}

extern "C" int gpbo_thompson_paths_f64(const double *Xs, int64_t M, const double *X, int64_t N, int64_t Np, int32_t d,
                                       const double *ls_host, const double *omega, const double *phase, const double *W,
                                       const double *V, int32_t F, int32_t S, int64_t idx_offset, double *f_out, int64_t ldf,
                                       int64_t *idx_out, double *val_out, int64_t *nan_out, void *work, int64_t work_bytes,
                                       void *stream) {
    if (!Xs || !omega || !phase || !W || !idx_out || !val_out || !nan_out || !work) return GPBO_ERR_ARG;
    if (!model_ok(X, N, Np, d, ls_host, F, S) || M < 1 || M > TS_MAX_M || (f_out && ldf < M)) return GPBO_ERR_ARG;
    if (work_bytes < PathsLayout(nullptr, Np, M, F, S).total || !aligned_to(work, 256)) return GPBO_ERR_WORKSPACE;
    return run_paths(Xs, M, X, N, Np, d, ls_host, omega, phase, W, V, F, S, idx_offset, f_out, ldf, idx_out, val_out, nan_out,
                     true, work, stream);
}

extern "C" int gpbo_thompson_weights_f64(const double *X, const double *y, int64_t N, int64_t Np, int32_t d,
                                         const double *ls_host, const double *U, double jitter1, double jitter2,
                                         const double *omega, const double *phase, const double *W, const double *E, int32_t F,
                                         int32_t S, double *V, void *work, int64_t work_bytes, void *stream) {
    if (!y || !U || !omega || !phase || !W || !E || !V || !work) return GPBO_ERR_ARG;
    if (!model_ok(X, N, Np, d, ls_host, F, S)) return GPBO_ERR_ARG;
    if (!aligned_to(U, 16)) return GPBO_ERR_ARG;   // the GEMM's B operand; refused here so that nothing is enqueued first
    const double kappa = jitter1 + jitter2;
    if (!(kappa >= 0.0) || !std::isfinite(kappa)) return GPBO_ERR_ARG;
    const WeightsLayout L(work, Np, F, S);
    if (work_bytes < L.total || !aligned_to(work, 256)) return GPBO_ERR_WORKSPACE;
    hipStream_t st = gpbo_stream(stream);
    double *A = L.a, *B = L.b;
    // G = g_s(X) [S x Np] (columns n >= N are not written and not read)
    int rc = run_paths(X, N, X, N, Np, d, ls_host, omega, phase, W, nullptr, F, S, 0, A, Np, nullptr, nullptr, nullptr, false,
                       L.paths, stream);
    if (rc != GPBO_OK) return rc;
    hipLaunchKernelGGL(thompson_resid_kernel, dim3((unsigned)((L.S64 * Np + 255) / 256)), dim3(256), 0, st, y, A, E, (int)S,
                       L.S64, N, Np, sqrt(kappa), B);
    GPBO_CHECK_LAUNCH();
    // U is upper triangular; both products run dense (the GEMM's triangular skips are for the lower case)
    rc = gpbo_gemm_launch_tri(0, L.S64, Np, Np, 1.0, B, Np, 0, U, Np, 0, 0.0, A, Np, 0, 1, 0, 0, st);
    if (rc != GPBO_OK) return rc;
    rc = gpbo_gemm_launch_tri(1, L.S64, Np, Np, 1.0, A, Np, 0, U, Np, 0, 0.0, B, Np, 0, 1, 0, 0, st);
    if (rc != GPBO_OK) return rc;
    if (hipMemcpyAsync(V, B, 8 * (size_t)S * (size_t)Np, hipMemcpyDeviceToDevice, st) != hipSuccess) return GPBO_ERR_LAUNCH;
    return GPBO_OK;
}
