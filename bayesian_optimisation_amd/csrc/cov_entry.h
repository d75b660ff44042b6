// The covariance entry, ONCE: every kernel that needs k(x, x') - in either of the library's two forms - gets the distance and
// the family formula from here, so that an entry has the same bits wherever it is computed (the mean of the fp32 / int8
// screens is the fp64 path's, append() reproduces a column of K as the factorisation saw it, the batch pivot is exp(-0) = 1,
// the Thompson paths use the fp64 path's arithmetic).  The loops around these calls, the order of the sums over the
// observations, the stores, the HAS_DIAG quirk and the NaN poisoning belong to the kernels.
//   scoring form        coordinates pre-scaled by 1 / (ls_k sqrt 2):  s = sum_k fma(d_k, d_k, s) = r^2 / 2,  cov_from_s(s, tab)
//   factorisation form  raw coordinates:  acc = sum_k fma(diff_k diff_k, il2_k, acc) = r^2,  cov_from_r2(acc) by the library's
//                       exp / sqrt (K(X,X) and its columns), cov_from_r2_tab(acc, tab) by exp_neg.h (the likelihood kernels)
// -ffp-contract=off: nothing is contracted across these function boundaries that was not contracted inside the kernels.
// Different formulas ON PURPOSE, not served from here:
//   dlog_factor (ard_grad.hip)           a derivative: g(r), summed per feature by a plain s += dd[k]
//   kstar_mu_anyd_kernel                 (x - o) * isc, scaled AFTER the subtraction, and the library's exp (any-d slow path)
//   kstar_mfma.hip                       the expanded distance |a|^2 + |b|^2 - 2 a.b on the matrix cores and a shorter exp: its
//                                        error is absolute; it feeds the prefix bound, never an answer
//   subset.hip                           farthest-point distances in units of ls (FpsLs::isc = 1 / ls), never exponentiated
// The SAME formulas, still written out in a kernel because a call there changes that kernel's generated code:
//   the scaled load x[k] = (valid ? Xs[c D + k] : 0) * isc[k] with its NaN flags (kstar_mu_kernel, kstar_slices_kernel,
//   batch_downdate_kernel), the 2 x 1 sum of thompson_paths_kernel, the scale-on-the-fly sum of refine_ks_kernel, the r^2 sum of
//   nlml_fused_kernel, and the r^2 sum over a run-time d (kxx_anyd_kernel, batch_pivot_kernel, append_kvec_kernel,
//   nlml_grid_kernel, qei_kernel).  Whoever changes cov_s* or cov_r2 changes those loops with them.
#pragma once
#include "gpbo_internal.h"
#include "exp_neg.h"

// ---- the length scales as kernel arguments (filled by length_scale_scalings(), host_driver.h; entries k >= d are zero) ----
struct CovIl2 {
    double il2[GPBO_MAX_D];  // 1 / ls_k^2, computed on the host in fp64
};
struct CovIsc {
    double isc[GPBO_MAX_D];  // 1 / (ls_k sqrt 2): coordinates scaled by this give exp(-sum diff^2)
};
struct CovLs {
    double il2[GPBO_MAX_D];
    double isc[GPBO_MAX_D];
};

// tab[0 .. E) in LDS, by the threads i = 0 .. E - 1 of the caller's choice; the caller's barrier publishes it
__device__ __forceinline__ void cov_stage_tab(double *tab, int i) {
    if (i < GPBO_EXP_E) tab[i] = kExp2Tab256[i * (256 / GPBO_EXP_E)];
}

// ---- scoring form ------------------------------------------------------------------------------------------------------
// s = r^2 / 2 of one scaled point against one scaled row
template <int D>
__device__ __forceinline__ double cov_s(const double (&x)[D], const double *xo) {
    double s = 0.0;
#pragma unroll
    for (int k = 0; k < D; ++k) {
        const double dd = x[k] - xo[k];
        s = fma(dd, dd, s);
    }
    return s;
}
// two points against one row
template <int D>
__device__ __forceinline__ void cov_s2(const double (&xa)[D], const double (&xb)[D], const double *xo, double &sa, double &sb) {
    sa = 0.0, sb = 0.0;
#pragma unroll
    for (int k = 0; k < D; ++k) {
        const double o = xo[k];
        const double da = xa[k] - o, db = xb[k] - o;
        sa = fma(da, da, sa);
        sb = fma(db, db, sb);
    }
}
// two points against two rows: four independent chains.  DEPTH < D: a timing variant's truncated sum (wrong by design)
template <int D, int DEPTH = D>
__device__ __forceinline__ void cov_s4(const double (&xa)[D], const double (&xb)[D], const double *xo0, const double *xo1,
                                       double &s00, double &s01, double &s10, double &s11) {
    s00 = 0.0, s01 = 0.0, s10 = 0.0, s11 = 0.0;
#pragma unroll
    for (int k = 0; k < DEPTH; ++k) {
        const double o0 = xo0[k], o1 = xo1[k];
        const double d00 = xa[k] - o0, d01 = xb[k] - o0, d10 = xa[k] - o1, d11 = xb[k] - o1;
        s00 = fma(d00, d00, s00);
        s01 = fma(d01, d01, s01);
        s10 = fma(d10, d10, s10);
        s11 = fma(d11, d11, s11);
    }
}
// the entry from s = r^2 / 2: a = sqrt(6 s) (Matern 3/2) or sqrt(10 s) (5/2, where a^2 / 3 = 10/3 s needs no square)
template <int KERN>
__device__ __forceinline__ double cov_from_s(double s, const double *tab) {
    if constexpr (KERN == GPBO_KERNEL_SE) {
        return exp_neg(s, tab);
    } else if constexpr (KERN == GPBO_KERNEL_MATERN32) {
        const double a = sqrt_nonneg(6.0 * s);
        return (1.0 + a) * exp_neg(a, tab);
    } else {
        static_assert(KERN == GPBO_KERNEL_MATERN52, "a covariance family");
        const double a = sqrt_nonneg(10.0 * s);
        return ((1.0 + a) + (10.0 / 3.0) * s) * exp_neg(a, tab);
    }
}

// ---- factorisation form ------------------------------------------------------------------------------------------------
// r^2 = sum_k (a_k - b_k)^2 / ls_k^2 in the reference's order per entry: subtract, square, scale, sum in index order.
// The same bits for (a, b) and (b, a).
template <int D>
__device__ __forceinline__ double cov_r2(const double *a, const double *b, const double *il2) {
    double acc = 0.0;
#pragma unroll
    for (int k = 0; k < D; ++k) {
        const double diff = a[k] - b[k];
        acc = fma(diff * diff, il2[k], acc);
    }
    return acc;
}
// the entry from r^2 by the library's exp and sqrt: K(X,X) as the factorisation sees it
template <int KERN>
__device__ __forceinline__ double cov_from_r2(double acc) {
    if constexpr (KERN == GPBO_KERNEL_SE) {
        return exp(-0.5 * acc);
    } else if constexpr (KERN == GPBO_KERNEL_MATERN32) {
        const double a = sqrt(3.0 * acc);
        return (1.0 + a) * exp(-a);
    } else {
        static_assert(KERN == GPBO_KERNEL_MATERN52, "a covariance family");
        const double a = sqrt(5.0 * acc);
        return ((1.0 + a) + a * a / 3.0) * exp(-a);
    }
}
// the same formulas on the table-driven exp(-t) and the Goldschmidt sqrt of exp_neg.h: the likelihood kernels
template <int KERN>
__device__ __forceinline__ double cov_from_r2_tab(double acc, const double *tab) {
    if constexpr (KERN == GPBO_KERNEL_SE) {
        return exp_neg(0.5 * acc, tab);
    } else if constexpr (KERN == GPBO_KERNEL_MATERN32) {
        const double a = sqrt_nonneg(3.0 * acc);
        return (1.0 + a) * exp_neg(a, tab);
    } else {
        static_assert(KERN == GPBO_KERNEL_MATERN52, "a covariance family");
        const double a = sqrt_nonneg(5.0 * acc);
        return ((1.0 + a) + a * a / 3.0) * exp_neg(a, tab);
    }
}
