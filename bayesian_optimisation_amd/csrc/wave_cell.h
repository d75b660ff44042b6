// One WAVE per cell, the cell's matrix in registers: the core shared by nlml_wave_kernel (ard_wave.hip) and hyper_wave_kernel
// (hyper_wave.hip).  Lane i holds row i of K = K0(ls) + diag I (x[k] = K[i][k], k < NMAX), the column steps of a right-looking
// Cholesky are fully unrolled, the pivot and the multipliers L[k][c] travel by v_readlane, and NRHS right-hand sides ride along
// (b -> z = L^-1 b by forward substitution in the same steps): no LDS traffic beyond the exp table and the observations, no
// barrier after the first, four cells per workgroup.  Work per cell: NMAX^2 / 2 wave instructions (+ two readlanes each); the
// upper triangle is carried along unused (lanes i < k hold garbage in x[k]; nothing reads it).  Rows / columns beyond N are the
// identity (pivot 1, log 1 = 0), lanes beyond NMAX idle.  NMAX = 16 / 32 / 48 / 64, D = 2 / 4 / 8 / 16.
// The core owns the staging, the row build, the elimination, the butterfly and the NMAX x D ladder.  What a kernel does with a
// column's z - and in WHICH ORDER it sums - is the kernel's: that order is part of its output bits (eliminate()'s hook).
// The register allocation of these kernels is fragile; the notes at build_row(), load_rhs() and eliminate() say what was paid.
#pragma once
#include "cov_entry.h"
#include "potrf_diag64.h"

#include <cmath>
#include <type_traits>

namespace gpbo_wave {

using gpbo_pd::readlane_f64;
using gpbo_pd::rsqrt_refined;

constexpr int CELLS = 4;   // waves, hence cells, per workgroup of 256
// workgroups per CU the register budget allows: 128 / 168 / 256 registers per lane for 4 / 3 / 2
#define GPBO_WAVE_BOUNDS(NMAX, D) __launch_bounds__(256, (NMAX) > 32 ? 2 : ((D) == 16 ? 3 : 4))

// Fills the exp table, Xs [NMAX x D] (the observations padded with zeros, the same for the four cells) and ys [NMAX], passes the
// kernel's one barrier and returns this wave's cell (which may be >= G: the caller returns then).
template <int NMAX, int D>
__device__ __forceinline__ int stage(double *tab, double *Xs, double *ys, const double *__restrict__ X, const double *__restrict__ y,
                                     int N, int d) {
    cov_stage_tab(tab, threadIdx.x);
    for (int e = threadIdx.x; e < NMAX * D; e += 256) {
        const int r = e / D, q = e % D;   // (D is a power of two)
        Xs[e] = (r < N && q < d) ? X[r * d + q] : 0.0;
    }
    if (threadIdx.x < NMAX) ys[threadIdx.x] = ((int)threadIdx.x < N) ? y[threadIdx.x] : 0.0;
    gpbo_syncthreads();
    return (int)blockIdx.x * CELLS + __builtin_amdgcn_readfirstlane((int)threadIdx.x >> 6);
}

// a row < NMAX for every lane (NMAX = 48 is no power of two)
template <int NMAX>
__device__ __forceinline__ int row_of(int lane) {
    return ((NMAX & (NMAX - 1)) == 0) ? (lane & (NMAX - 1)) : (lane >= NMAX ? lane - NMAX : lane);
}

// x[k] = (K0(ls) + diag I)[i][k] for the lane's row i = li; ls: the cell's d length scales (wave-uniform).  Column k's coordinates
// are wave-uniform too (one LDS address for the wave).  The entries are cov_r2 / cov_from_r2_tab (cov_entry.h): kxx_kernel's
// formulas on the table-driven exp(-t) and the Goldschmidt sqrt of exp_neg.h.
template <int NMAX, int D, int KERN>
__device__ __forceinline__ void build_row(double (&x)[NMAX], const double *tab, const double *Xs, const double *__restrict__ ls,
                                          double diag, int N, int d, int lane, int li) {
    double il2[D], xi[D];
#pragma unroll
    for (int k = 0; k < D; ++k) {
        const double l = (k < d) ? ls[k] : 1.0;
        il2[k] = (k < d) ? 1.0 / (l * l) : 0.0;
        xi[k] = Xs[li * D + k];
    }
#pragma unroll
    for (int k = 0; k < NMAX; ++k) {
        double v = cov_from_r2_tab<KERN>(cov_r2<D>(Xs + k * D, xi, il2), tab);
        if (k == lane) v += diag;
        if (lane >= N || k >= N) v = (k == lane) ? 1.0 : 0.0;
        x[k] = v;
        // two entries in flight at a time: left to itself the scheduler starts all NMAX chains at once (264 registers)
        if (k & 1) __builtin_amdgcn_sched_barrier(0);
    }
}

// The lane's entry of y (0 on the lanes beyond NMAX).  A plain load and a select: written as one conditional expression, the
// register allocation of the WHOLE kernel collapses - 124 spilled registers at NMAX = 32 - and the launch moves 157 MB of scratch.
template <int NMAX>
__device__ __forceinline__ double load_rhs(const double *ys, int lane, int li) {
    double b = ys[li];
    if (lane >= NMAX) b = 0.0;
    return b;
}

// The elimination: x becomes L (lane i >= c: x[c] = L[i][c]), b becomes garbage, lcc = L[c][c] on lane c (1 on the lanes beyond
// NMAX).  column(c, z) is called once per column, in column order, with z[j] = (L^-1 b_j)_c, wave-uniform.  A hook that
// accumulates wave-uniform values can be sunk behind the whole elimination by the compiler, which then holds every column's
// multipliers alive for it (three such sums: 238 registers at NMAX = 48 for 123); keeping z on lane c and summing afterwards
// (wave_sum) is the way out.  Returns true when a pivot was not positive and finite.
template <int NMAX, int NRHS, class F>
__device__ __forceinline__ bool eliminate(double (&x)[NMAX], double (&b)[NRHS], double &lcc, int lane, F &&column) {
    bool bad = false;
    lcc = 1.0;
#pragma unroll
    for (int c = 0; c < NMAX; ++c) {
        const double piv = readlane_f64(x[c], c);
        bad |= !(piv > 0.0) | !(piv < 1.0e300);
        const double r = rsqrt_refined(piv);
        const double lc = x[c] * r;
        if (lane == c) lcc = lc;
        double z[NRHS];   // z_c = (b_c - sum_{k<c} L[c][k] z_k) / L[c][c]
#pragma unroll
        for (int j = 0; j < NRHS; ++j) z[j] = readlane_f64(b[j], c) * r;
        column(c, z);
#pragma unroll
        for (int j = 0; j < NRHS; ++j) b[j] = fma(-lc, z[j], b[j]);
        // the next pivot's entry x[c + 1] is updated LAST (its multiplier read first): in column order the schedule changes with
        // it - 1 to 3 % slower at NMAX <= 32 (60 % more hazard wait states at NMAX = 16), 1 % faster at NMAX >= 48
        double l1 = 0.0;
        if (c + 1 < NMAX) l1 = readlane_f64(lc, c + 1);
#pragma unroll
        for (int k = c + 2; k < NMAX; ++k) x[k] = fma(-lc, readlane_f64(lc, k), x[k]);
        if (c + 1 < NMAX) x[c + 1] = fma(-lc, l1, x[c + 1]);
    }
    return bad;
}

// the sum over the 64 lanes, in every lane: one fixed order (log det = 2 wave_sum(log(lcc)): one log per lane, all at once)
__device__ __forceinline__ double wave_sum(double v) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off);
    return v;
}

inline unsigned grid_of(int64_t G) { return (unsigned)((G + CELLS - 1) / CELLS); }

// launch(integral_constant NMAX, integral_constant D) for the smallest instance that holds N <= MAXN observations of d features
template <int MAXN, class F>
int dispatch(int64_t N, int32_t d, F &&launch) {
    auto with_d = [&](auto nmax) {
        if (d <= 2) return launch(nmax, std::integral_constant<int, 2>{});
        if (d <= 4) return launch(nmax, std::integral_constant<int, 4>{});
        if (d <= 8) return launch(nmax, std::integral_constant<int, 8>{});
        return launch(nmax, std::integral_constant<int, 16>{});
    };
    if (N <= 16) return with_d(std::integral_constant<int, 16>{});
    if (N <= 32) return with_d(std::integral_constant<int, 32>{});
    if constexpr (MAXN > 32) {
        if (N <= 48) return with_d(std::integral_constant<int, 48>{});
        return with_d(std::integral_constant<int, 64>{});
    }
    return GPBO_ERR_ARG;
}

}  // namespace gpbo_wave
