// Scalar arithmetic of the constrained acquisitions in log space (constrained.hip): log h with h(z) = phi(z) + z Phi(z)
// - expected improvement is sigma h(z) - in three branches of which none cancels beyond what its bound states, and the terms of
// one candidate built from it and from mes_log_ndtr (mes_math.h).  t = -z / sqrt 2:
//   z >= -1          log(phi(z) + z Phi(z)) with the plain forms: both terms are positive from 0 on, and on [-1, 0) h >= 0.083
//                    while the terms stay below 0.4 - at most 2.3 bits are cancelled
//   -1e3 < z < -1    h = phi(z) (1 + z Phi / phi) and Phi / phi = sqrt(pi / 2) erfcx(t):
//                                                   -t^2 - log(2 pi) / 2 + log1p(-sqrt(pi) t erfcx(t))
//                    (h itself underflows at z ~ -38.5; the argument of log1p tends to -1 like 1 / z^2, so its rounding error is
//                    amplified by z^2 - the eps z^2 / 2 of the bound below)
//   z <= -1e3        the argument of log1p is within 1e-6 of -1 and erfcx has no bits left for it; the asymptotic series
//                    sqrt(pi) t erfcx(t) = 1 - u + 3 u^2 - 15 u^3 + ..., u = 1 / (2 t^2) = 1 / z^2 (next term 105 u^4 <= 1e-22 u):
//                                                   -t^2 - log(2 pi) / 2 + log(u (1 - 3 u (1 - 5 u)))
// Against 60-digit values at 2,001 points on [-40, 40] and at -1e2, -3e2, -999, -1e3, -1e4, -1e6 (tests/golden/cons_terms.npz) these
// forms, evaluated in fp64 with SciPy, stay within 2.84 units of eps (max(1, z^2 / 2 for z < 0) + |log h|); the device's own are
// measured in tests/test_gpu_constrained.py.
#pragma once
#include "../../include/gpbo.h"
#include "mes_math.h"

#define CONS_HALF_LOG_2PI 0.91893853320467274178   /* log(2 pi) / 2 */
#define CONS_SQRTPI 1.77245385090551602730         /* sqrt pi */

// log h(z); NaN for NaN, +inf at +inf, -inf at -inf
__device__ __forceinline__ double cons_log_h(double z) {
    if (z >= -1.0) {
        const double pdf = exp(-0.5 * z * z) * MES_RSQRT2PI;
        const double cdf = 0.5 * erfc(-z * MES_RSQRT2);
        return log(pdf + z * cdf);
    }
    const double t = -z * MES_RSQRT2;
    if (z > -1.0e3) return (-(t * t) - CONS_HALF_LOG_2PI) + log1p(-(CONS_SQRTPI * t) * erfcx(t));
    const double u = 1.0 / (2.0 * (t * t));   // (z NaN: every comparison above is false, and NaN comes out here)
    return (-(t * t) - CONS_HALF_LOG_2PI) + log(u * (1.0 - 3.0 * u * (1.0 - 5.0 * u)));
}

// log Pr[g <= upper] of one constraint with posterior (mu, sigma): NaN for a NaN input; sigma == 0: certain, either way
__device__ __forceinline__ double cons_feasible_term(double mu, double sigma, double upper) {
    if (mu != mu || sigma != sigma) return __builtin_nan("");
    if (sigma == 0.0) return mu <= upper ? 0.0 : -__builtin_huge_val();
    return mes_log_ndtr((upper - mu) / sigma);
}

// The base term of a candidate with objective posterior (mu, sigma), base GPBO_CONS_BASE_EI or GPBO_CONS_BASE_PI:
//   EI  log sigma + log h(z)      sigma == 0: log(max(imp, 0))
//   PI  log Phi(z)                sigma == 0: 0 where imp > 0, else -inf
// with imp = (f_best - mu) - xi and z = imp / sigma; NaN for a NaN input.
__device__ __forceinline__ double cons_base_term(int base, double mu, double sigma, double f_best, double xi) {
    if (mu != mu || sigma != sigma) return __builtin_nan("");
    const double imp = (f_best - mu) - xi;
    if (sigma == 0.0) {
        if (base == GPBO_CONS_BASE_PI) return imp > 0.0 ? 0.0 : -__builtin_huge_val();
        return log(fmax(imp, 0.0));
    }
    const double z = imp / sigma;
    return base == GPBO_CONS_BASE_PI ? mes_log_ndtr(z) : log(sigma) + cons_log_h(z);
}
