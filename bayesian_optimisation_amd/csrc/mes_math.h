// Scalar arithmetic of max-value entropy search (mes.hip): log Phi and the entropy term h, each in three branches
// of which none cancels beyond what its bound states.  Used by the two kernels of mes.hip; log Phi also by cons_math.h (constrained.hip).
//   gamma > 0         Phi = 1 - erfc(gamma / sqrt 2) / 2 is close to 1:       log1p(-erfc(gamma / sqrt 2) / 2)
//   -1 <= gamma <= 0  Phi = erfc(-gamma / sqrt 2) / 2, in [0.158, 0.5]:       log(erfc(-gamma / sqrt 2) / 2)
//   gamma < -1        t = -gamma / sqrt 2, Phi = exp(-t^2) erfcx(t) / 2 (Phi itself underflows at gamma ~ -38):
//                                                                             -t^2 + log(erfcx(t) / 2)
// h(gamma) = gamma phi(gamma) / (2 Phi(gamma)) - log Phi(gamma) >= 0.  Below -1 both terms of the plain form grow like gamma^2 / 2
// and cancel; with phi / Phi = sqrt(2 / pi) / erfcx(t) the t^2 of the two terms is taken together FIRST:
//   h = (t^2 - t / (sqrt(pi) erfcx(t))) - log(erfcx(t) / 2)
// whose bracket tends to -1/2 with a rounding error of eps t^2.  Against 60-digit values at 2,001 points on [-40, 40] and at -1e2,
// -1e3, -1e4 (tests/golden/mes_terms.npz) these forms, evaluated in fp64 with SciPy, stay within 2.24 units of
// eps (max(1, gamma^2 / 2 for gamma < 0) + |h|); the device's own are measured in tests/test_gpu_mes.py.
#pragma once
#include <hip/hip_runtime.h>

#define MES_RSQRT2 0.70710678118654752440     /* 1 / sqrt 2 */
#define MES_RSQRT2PI 0.39894228040143267794   /* 1 / sqrt(2 pi) */
#define MES_RSQRTPI 0.56418958354775628695    /* 1 / sqrt pi */

// log Phi(gamma); NaN for NaN, 0 at +inf, -inf at -inf
__device__ __forceinline__ double mes_log_ndtr(double g) {
    if (g > 0.0) return log1p(-0.5 * erfc(g * MES_RSQRT2));
    if (g >= -1.0) return log(0.5 * erfc(-g * MES_RSQRT2));
    const double t = -g * MES_RSQRT2;
    return -(t * t) + log(0.5 * erfcx(t));   // (g NaN: every comparison above is false, and NaN comes out here)
}

// h(gamma) = gamma phi / (2 Phi) - log Phi; NaN for NaN, the limits 0 at +inf and +inf at -inf (inf * 0 otherwise)
__device__ __forceinline__ double mes_term(double g) {
    if (g - g != 0.0 && g == g) return g > 0.0 ? 0.0 : __builtin_huge_val();
    if (g >= -1.0) {
        const double pdf = exp(-0.5 * g * g) * MES_RSQRT2PI;
        if (g > 0.0) {
            const double q = 0.5 * erfc(g * MES_RSQRT2);   // 1 - Phi
            return g * pdf / (2.0 * (1.0 - q)) - log1p(-q);
        }
        const double cdf = 0.5 * erfc(-g * MES_RSQRT2);
        return g * pdf / (2.0 * cdf) - log(cdf);
    }
    const double t = -g * MES_RSQRT2;
    const double ex = erfcx(t);
    return (t * t - t * MES_RSQRTPI / ex) - log(0.5 * ex);
}
