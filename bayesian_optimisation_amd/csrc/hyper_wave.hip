// The ard="hyper" likelihood of MANY hyperparameter cells in one launch (N <= 64): one WAVE per cell, the matrix in registers.
//
// A cell is (ls_1 ... ls_d, rho); the model is the one of hyper.hip: y ~ N(m 1, s^2 Kt), Kt = K0(ls) + rho I, mean and scale
// profiled out in closed form.  hyper.hip evaluates one cell per call from a factorisation in memory (five launches and a host
// round trip): a sampler of the hyperparameter posterior (hyper_posterior.py) needs the VALUE only, at a few dozen cells per
// step, and at the sizes where the posterior is broad enough to matter (N <= 64) a cell's whole matrix fits the registers of one
// wave.  The kernel is nlml_wave_kernel of ard_wave.hip - lane i holds row i of Kt, the column steps of a right-looking
// Cholesky are unrolled, pivot and multipliers travel by v_readlane - with TWO right-hand sides riding along instead of one:
// y and the vector of ones.  Forward substitution in the same steps leaves zy = L^-1 y and z1 = L^-1 1 entry by entry, and
//     A = zy . zy = y^T Kt^-1 y,   B = z1 . zy = 1^T Kt^-1 y,   C = z1 . z1 = 1^T Kt^-1 1
// are all the profile needs:
//     m   = B / C                       (0 without GPBO_HYPER_MEAN)
//     q   = A - 2 m B + m^2 C           = (y - m 1)^T Kt^-1 (y - m 1)
//     s^2 = q / N                       (1 without GPBO_HYPER_SCALE)
//     L   = 1/2 [q / s^2 + N log s^2 + log det Kt + N log 2 pi]
// NaN in all three outputs when a pivot is not positive and finite, when C is not positive and finite or when s^2 is not (one
// observation with both flags, a constant y, rho <= 0 on a matrix that needs it): the rule of gpbo_nlml_hyper_f64.
// The covariance family is a template parameter as in kxx_kernel (kernel_build.hip), with that kernel's entry formulas on the
// table-driven exp(-t) and the Goldschmidt sqrt of exp_neg.h.  Rows / columns beyond N are the identity (pivot 1, log 1 = 0,
// both right-hand sides 0), lanes beyond NMAX idle.  NMAX = 16 / 32 / 48 / 64, D = 2 / 4 / 8 / 16.
// The three sums are butterflies over the lanes; no atomics, one fixed order: two launches give the same bits.
#include "gpbo_internal.h"
#include "exp_neg.h"
#include "potrf_diag64.h"

#include <cmath>

namespace {

using gpbo_pd::readlane_f64;
using gpbo_pd::rsqrt_refined;

template <int NMAX, int D, int KERN>
__global__ __launch_bounds__(256, NMAX > 32 ? 2 : (D == 16 ? 3 : 4)) void hyper_wave_kernel(
    const double *__restrict__ X, const double *__restrict__ y, int N, int d, const double *__restrict__ cells, int G, int flags,
    double *__restrict__ out) {
    __shared__ double tab[GPBO_EXP_E];
    __shared__ double Xs[NMAX * D];   // the observations, padded with zeros to NMAX rows of D features (the same for the four cells)
    __shared__ double ys[NMAX];
    if (threadIdx.x < GPBO_EXP_E) tab[threadIdx.x] = kExp2Tab256[threadIdx.x * (256 / GPBO_EXP_E)];
    for (int e = threadIdx.x; e < NMAX * D; e += 256) {
        const int r = e / D, q = e % D;   // (D is a power of two)
        Xs[e] = (r < N && q < d) ? X[r * d + q] : 0.0;
    }
    if (threadIdx.x < NMAX) ys[threadIdx.x] = ((int)threadIdx.x < N) ? y[threadIdx.x] : 0.0;
    gpbo_syncthreads();
    const int lane = threadIdx.x & 63;
    const int g = (int)blockIdx.x * 4 + __builtin_amdgcn_readfirstlane((int)threadIdx.x >> 6);   // this wave's cell
    if (g >= G) return;

    const int li = ((NMAX & (NMAX - 1)) == 0) ? (lane & (NMAX - 1)) : (lane >= NMAX ? lane - NMAX : lane);   // a row < NMAX for every lane
    const double *cell = cells + (int64_t)g * (d + 1);
    const double rho = cell[d];                                                   // wave-uniform
    double il2[D], xi[D];
#pragma unroll
    for (int k = 0; k < D; ++k) {
        const double l = (k < d) ? cell[k] : 1.0;                                 // wave-uniform
        il2[k] = (k < d) ? 1.0 / (l * l) : 0.0;
        xi[k] = Xs[li * D + k];                                                   // this lane's row
    }
    // Kt[i][k] for the lane's row i: column k's coordinates are wave-uniform (one LDS address for the wave)
    double x[NMAX];
#pragma unroll
    for (int k = 0; k < NMAX; ++k) {
        double a = 0.0;
#pragma unroll
        for (int q = 0; q < D; ++q) {
            const double diff = Xs[k * D + q] - xi[q];
            a = fma(diff * diff, il2[q], a);
        }
        double v;
        if constexpr (KERN == GPBO_KERNEL_SE) {
            v = exp_neg(0.5 * a, tab);
        } else if constexpr (KERN == GPBO_KERNEL_MATERN32) {
            const double t = sqrt_nonneg(3.0 * a);
            v = (1.0 + t) * exp_neg(t, tab);
        } else {
            const double t = sqrt_nonneg(5.0 * a);
            v = ((1.0 + t) + t * t / 3.0) * exp_neg(t, tab);
        }
        if (k == lane) v += rho;
        if (lane >= N || k >= N) v = (k == lane) ? 1.0 : 0.0;
        x[k] = v;
        // two entries in flight at a time (nlml_wave_kernel: left to itself the scheduler starts all NMAX chains at once)
        if (k & 1) __builtin_amdgcn_sched_barrier(0);
    }
    // (plain loads and selects, as in nlml_wave_kernel: one conditional expression there cost 124 spilled registers)
    double by = ys[li];
    if (lane >= NMAX) by = 0.0;
    double b1 = 1.0;
    if (lane >= N) b1 = 0.0;

    double zyl = 0.0, z1l = 0.0, lcc = 1.0;           // lane c keeps (L^-1 y)_c, (L^-1 1)_c and L[c][c]
    bool bad = false;
#pragma unroll
    for (int c = 0; c < NMAX; ++c) {
        const double piv = readlane_f64(x[c], c);
        bad |= !(piv > 0.0) | !(piv < 1.0e300);
        const double r = rsqrt_refined(piv);
        const double lc = x[c] * r;                   // lane i >= c: L[i][c]
        if (lane == c) lcc = lc;                      // L[c][c], for log det
        const double zy = readlane_f64(by, c) * r;    // (L^-1 y)_c
        const double z1 = readlane_f64(b1, c) * r;    // (L^-1 1)_c
        // (kept per lane and summed after the loop: three wave-uniform accumulators here are sunk behind the whole elimination
        //  by the compiler, which then holds every column's multipliers alive for them - 238 registers at NMAX = 48 for 123)
        if (lane == c) { zyl = zy; z1l = z1; }
        by = fma(-lc, zy, by);
        b1 = fma(-lc, z1, b1);
#pragma unroll
        for (int k = c + 1; k < NMAX; ++k) x[k] = fma(-lc, readlane_f64(lc, k), x[k]);
    }
    double logdet = log(lcc);                         // one log per lane, all at once (1 on the padded lanes)
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) logdet += __shfl_xor(logdet, off);
    logdet *= 2.0;
    double A = zyl * zyl, B = z1l * zyl, Cc = z1l * z1l;   // zero on the padded lanes
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
        A += __shfl_xor(A, off);
        B += __shfl_xor(B, off);
        Cc += __shfl_xor(Cc, off);
    }
    if (lane == 0) {
        const double inf = __builtin_huge_val();
        const double m = (flags & GPBO_HYPER_MEAN) ? B / Cc : 0.0;
        const double q = fma(m * m, Cc, fma(-2.0 * m, B, A));
        const double s2 = (flags & GPBO_HYPER_SCALE) ? q / (double)N : 1.0;
        double L = 0.5 * (q / s2 + (double)N * log(s2) + logdet + (double)N * 1.8378770664093453);   // log(2 pi)
        double mo = m, so = s2;
        if (bad || !(Cc > 0.0 && Cc < inf) || !(s2 > 0.0 && s2 < inf)) L = mo = so = __builtin_nan("");
        out[(int64_t)g * 3 + 0] = L;
        out[(int64_t)g * 3 + 1] = mo;
        out[(int64_t)g * 3 + 2] = so;
    }
}

template <int NMAX, int KERN>
int launch_d(const double *X, const double *y, int64_t N, int32_t d, const double *cells, int64_t G, int32_t flags, double *out,
             hipStream_t st) {
    const unsigned grid = (unsigned)((G + 3) / 4);
#define GPBO_HYPER_WAVE_LAUNCH(DD)                                                                                          \
    hipLaunchKernelGGL((hyper_wave_kernel<NMAX, DD, KERN>), dim3(grid), dim3(256), 0, st, X, y, (int)N, (int)d, cells, (int)G, \
                       (int)flags, out)
    if (d <= 2) GPBO_HYPER_WAVE_LAUNCH(2);
    else if (d <= 4) GPBO_HYPER_WAVE_LAUNCH(4);
    else if (d <= 8) GPBO_HYPER_WAVE_LAUNCH(8);
    else GPBO_HYPER_WAVE_LAUNCH(16);
#undef GPBO_HYPER_WAVE_LAUNCH
    GPBO_CHECK_LAUNCH();
    return GPBO_OK;
}

template <int KERN>
int launch_n(const double *X, const double *y, int64_t N, int32_t d, const double *cells, int64_t G, int32_t flags, double *out,
             hipStream_t st) {
    if (N <= 16) return launch_d<16, KERN>(X, y, N, d, cells, G, flags, out, st);
    if (N <= 32) return launch_d<32, KERN>(X, y, N, d, cells, G, flags, out, st);
    if (N <= 48) return launch_d<48, KERN>(X, y, N, d, cells, G, flags, out, st);
    return launch_d<64, KERN>(X, y, N, d, cells, G, flags, out, st);
}

}  // namespace

static_assert(GPBO_HYPER_CELLS_MAX_N == 64, "a cell's rows are the lanes of one wave");

// y: pass y - mean(y) when the mean is fitted and add the shift back to m (out[1]): q is formed as A - 2 m B + m^2 C, which
// cancels like (mean / sd)^2 of the y given here.  Kt, hence L and s^2, do not see the shift.
extern "C" int gpbo_nlml_hyper_cells_f64(const double *X, const double *y, int64_t N, int32_t d, const double *cells, int64_t G,
                                         int32_t kernel, int32_t flags, double *out, void *stream) {
    if (!X || !y || !cells || !out || N < 1 || N > GPBO_HYPER_CELLS_MAX_N || d < 1 || d > GPBO_MAX_D || G < 1 || G > (1 << 28))
        return GPBO_ERR_ARG;
    if (!kernel_ok(kernel, d) || (flags & ~(GPBO_HYPER_MEAN | GPBO_HYPER_SCALE))) return GPBO_ERR_ARG;
    hipStream_t st = gpbo_stream(stream);
    if (kernel == GPBO_KERNEL_MATERN32) return launch_n<GPBO_KERNEL_MATERN32>(X, y, N, d, cells, G, flags, out, st);
    if (kernel == GPBO_KERNEL_MATERN52) return launch_n<GPBO_KERNEL_MATERN52>(X, y, N, d, cells, G, flags, out, st);
    return launch_n<GPBO_KERNEL_SE>(X, y, N, d, cells, G, flags, out, st);
}
