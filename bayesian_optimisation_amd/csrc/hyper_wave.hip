// The ard="hyper" likelihood of MANY hyperparameter cells in one launch (N <= 64): one WAVE per cell, the matrix in registers.
//
// A cell is (ls_1 ... ls_d, rho); the model is the one of hyper.hip: y ~ N(m 1, s^2 Kt), Kt = K0(ls) + rho I, mean and scale
// profiled out in closed form.  hyper.hip evaluates one cell per call from a factorisation in memory (five launches and a host
// round trip): a sampler of the hyperparameter posterior (hyper_posterior.py) needs the VALUE only, at a few dozen cells per
// step, and at the sizes where the posterior is broad enough to matter (N <= 64) a cell's whole matrix fits the registers of one
// wave.  The kernel is the wave-per-cell core of wave_cell.h, which nlml_wave_kernel (ard_wave.hip) runs with one right-hand
// side, with TWO riding along: y and the vector of ones.  It leaves zy = L^-1 y and z1 = L^-1 1 entry by entry, and
//     A = zy . zy = y^T Kt^-1 y,   B = z1 . zy = 1^T Kt^-1 y,   C = z1 . z1 = 1^T Kt^-1 1
// are all the profile needs:
//     m   = B / C                       (0 without GPBO_HYPER_MEAN)
//     q   = A - 2 m B + m^2 C           = (y - m 1)^T Kt^-1 (y - m 1)
//     s^2 = q / N                       (1 without GPBO_HYPER_SCALE)
//     L   = 1/2 [q / s^2 + N log s^2 + log det Kt + N log 2 pi]
// NaN in all three outputs when a pivot is not positive and finite, when C is not positive and finite or when s^2 is not (one
// observation with both flags, a constant y, rho <= 0 on a matrix that needs it): the rule of gpbo_nlml_hyper_f64.
// The covariance family is a template parameter as in kxx_kernel (kernel_build.hip); both right-hand sides are 0 beyond N.
// The three sums are butterflies over the lanes; no atomics, one fixed order: two launches give the same bits.
#include "wave_cell.h"

namespace {

namespace wc = gpbo_wave;

template <int NMAX, int D, int KERN>
__global__ GPBO_WAVE_BOUNDS(NMAX, D) void hyper_wave_kernel(
    const double *__restrict__ X, const double *__restrict__ y, int N, int d, const double *__restrict__ cells, int G, int flags,
    double *__restrict__ out) {
    __shared__ double tab[GPBO_EXP_E], Xs[NMAX * D], ys[NMAX];
    const int g = wc::stage<NMAX, D>(tab, Xs, ys, X, y, N, d);
    if (g >= G) return;
    const int lane = threadIdx.x & 63, li = wc::row_of<NMAX>(lane);
    const double *cell = cells + (int64_t)g * (d + 1);
    double x[NMAX], lcc;
    wc::build_row<NMAX, D, KERN>(x, tab, Xs, cell, cell[d], N, d, lane, li);   // Kt = K0(ls) + rho I
    double b[2] = {wc::load_rhs<NMAX>(ys, lane, li), 1.0};                      // y and the ones
    if (lane >= N) b[1] = 0.0;
    // lane c keeps (L^-1 y)_c and (L^-1 1)_c, summed after the loop (eliminate(): wave-uniform accumulators cost registers here)
    double zyl = 0.0, z1l = 0.0;
    const bool bad = wc::eliminate<NMAX, 2>(x, b, lcc, lane, [&](int c, const double(&z)[2]) {
        if (lane == c) { zyl = z[0]; z1l = z[1]; }
    });
    const double logdet = 2.0 * wc::wave_sum(log(lcc));
    const double A = wc::wave_sum(zyl * zyl), B = wc::wave_sum(z1l * zyl), Cc = wc::wave_sum(z1l * z1l);   // zero on the padded lanes
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

template <int KERN>
int launch(const double *X, const double *y, int64_t N, int32_t d, const double *cells, int64_t G, int32_t flags, double *out,
           hipStream_t st) {
    return wc::dispatch<GPBO_HYPER_CELLS_MAX_N>(N, d, [&](auto nmax, auto dd) -> int {
        hipLaunchKernelGGL((hyper_wave_kernel<nmax(), dd(), KERN>), dim3(wc::grid_of(G)), dim3(256), 0, st, X, y, (int)N, (int)d,
                           cells, (int)G, (int)flags, out);
        GPBO_CHECK_LAUNCH();
        return GPBO_OK;
    });
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
    if (kernel == GPBO_KERNEL_MATERN32) return launch<GPBO_KERNEL_MATERN32>(X, y, N, d, cells, G, flags, out, st);
    if (kernel == GPBO_KERNEL_MATERN52) return launch<GPBO_KERNEL_MATERN52>(X, y, N, d, cells, G, flags, out, st);
    return launch<GPBO_KERNEL_SE>(X, y, N, d, cells, G, flags, out, st);
}
