// ARD likelihood grid at the reference's OWN sizes (N <= 64 observations): one WAVE per grid cell, the matrix in registers.
//
// Replaces PointSelector.tune_kernel / eval_log_marginal (/root/reference/point_selector.py:104-163) like ard.hip does:
//     nlml = 0.5 * (y^T inv(K) y + log(det(K)) + N log(2 pi)),  K = kernel_rbf(X, X) (1e-4 jitter, :116,193), float32.
// The in-LDS kernel of round 2 (ard.hip, nlml_grid_kernel: a workgroup per cell, one barrier and one LDS round trip per
// column, index arithmetic with integer divisions, library exp / sqrt / division) needs 0.116 ms for the reference's 50 x 50
// grid at N = 32; the DAG runs exactly this shape once per iteration.  Here the wave-per-cell core of wave_cell.h factors
// K with y riding along as its one right-hand side, and y^T inv(K) y is accumulated column by column as the z_c appear.
// det under- / overflow of the reference (np.log(np.linalg.det(K)), :117-119) as in ard.hip: log(exp(logdet)); the second
// likelihood mode (fp64, log det straight from the factor: gpbo.h) is a kernel argument.
// Measured (one MI355X, 2,500 cells, d = 2 / 8 / 16, ms): N = 16: 0.014 / 0.016 / 0.023, N = 32: 0.026 / 0.031 / 0.038
// (in-LDS kernel: 0.044 and 0.116 at d = 2), N = 48: 0.049 / 0.065 / 0.075, N = 64: 0.068 / 0.083 / 0.096 (the fused kernel of
// ard.hip, which serves every larger N: 0.122 / 0.140 / 0.178); the float32 cells of all three kernels are equal.
#include "wave_cell.h"

#ifndef GPBO_WAVE_MAX_N
#define GPBO_WAVE_MAX_N 64
#endif

namespace {

namespace wc = gpbo_wave;

template <int NMAX, int D>
__global__ GPBO_WAVE_BOUNDS(NMAX, D) void nlml_wave_kernel(const double *__restrict__ X, const double *__restrict__ y, int N, int d,
                                                           const double *__restrict__ ls_cells, int G, double jitter,
                                                           void *__restrict__ out, int logdet_mode) {
    __shared__ double tab[GPBO_EXP_E], Xs[NMAX * D], ys[NMAX];
    const int g = wc::stage<NMAX, D>(tab, Xs, ys, X, y, N, d);
    if (g >= G) return;
    const int lane = threadIdx.x & 63, li = wc::row_of<NMAX>(lane);
    double x[NMAX], lcc, quad = 0.0;
    wc::build_row<NMAX, D, GPBO_KERNEL_SE>(x, tab, Xs, ls_cells + (int64_t)g * d, jitter, N, d, lane, li);
    double b[1] = {wc::load_rhs<NMAX>(ys, lane, li)};
    // (in column order, wave-uniform: this order is part of the float32 and float64 cells' bits)
    const bool bad = wc::eliminate<NMAX, 1>(x, b, lcc, lane, [&](int, const double(&z)[1]) { quad = fma(z[0], z[0], quad); });
    const double logdet = 2.0 * wc::wave_sum(log(lcc));
    if (lane == 0) {
        // reference mode: the reference takes log of a det that under- / overflows
        const double ld = logdet_mode ? logdet : log(exp(logdet));
        double nlml = 0.5 * (quad + ld + (double)N * 1.8378770664093453);   // log(2 pi)
        if (bad) nlml = __builtin_nan("");            // not positive definite: the reference's log(det < 0) is NaN
        if (logdet_mode) reinterpret_cast<double *>(out)[g] = nlml;
        else reinterpret_cast<float *>(out)[g] = (float)nlml;
    }
}

}  // namespace

constexpr int WAVE_MAX_N = GPBO_WAVE_MAX_N;
extern "C" int gpbo_nlml_grid_wave_max_n(void) { return WAVE_MAX_N; }

static int wave_run(const double *X, const double *y, int64_t N, int32_t d, const double *ls_cells, int64_t G, double jitter,
                    void *out, int mode, void *stream) {
    if (!X || !y || !ls_cells || !out || N < 1 || N > WAVE_MAX_N || d < 1 || d > GPBO_MAX_D || G < 1 || G > (1 << 30))
        return GPBO_ERR_ARG;
    hipStream_t st = gpbo_stream(stream);
    return wc::dispatch<WAVE_MAX_N>(N, d, [&](auto nmax, auto dd) -> int {
        hipLaunchKernelGGL((nlml_wave_kernel<nmax(), dd()>), dim3(wc::grid_of(G)), dim3(256), 0, st, X, y, (int)N, (int)d, ls_cells,
                           (int)G, jitter, out, mode);
        GPBO_CHECK_LAUNCH();
        return GPBO_OK;
    });
}

extern "C" int gpbo_nlml_grid_wave_f64(const double *X, const double *y, int64_t N, int32_t d, const double *ls_cells,
                                       int64_t G, double jitter, float *out, void *stream) {
    return wave_run(X, y, N, d, ls_cells, G, jitter, out, 0, stream);
}

extern "C" int gpbo_nlml_grid_wave_logdet_f64(const double *X, const double *y, int64_t N, int32_t d, const double *ls_cells,
                                              int64_t G, double jitter, double *out, void *stream) {
    return wave_run(X, y, N, d, ls_cells, G, jitter, out, 1, stream);
}
