// Scalar arithmetic of two-objective expected hypervolume improvement in log space (ehvi.hip), built on cons_log_h
// (cons_math.h).  For one objective with posterior (mu, sigma) and a level a,
//     g(a) = E[(a - f)+] = sigma h((a - mu) / sigma)   (sigma > 0),      max(a - mu, 0)   (sigma == 0),
// and G = log g.  A strip of the sum is [g1(a') - g1(a)] g2(c) with a < a'; in logarithms
//     G1(a') + log(1 - exp(G1(a) - G1(a'))) + G2(c)
// and the strips are added by a one-pass running-maximum logsumexp (EhviSum).
#pragma once
#include "cons_math.h"

// G(level): log sigma + log h(z), z = (level - mu) / sigma - one subtraction, then ONE division; sigma == 0: log(max(level - mu, 0)).
// log_sigma = log(sigma) is the caller's (one logarithm per objective and candidate, not per strip); not read when sigma == 0.
__device__ __forceinline__ double ehvi_log_g(double level, double mu, double sigma, double log_sigma) {
    if (sigma == 0.0) return log(fmax(level - mu, 0.0));
    return log_sigma + cons_log_h((level - mu) / sigma);
}

// log(1 - exp(d)) for d <= 0 in the two usual branches (d > -log 2: 1 - exp(d) is small and expm1 keeps its bits; else exp(d) is
// small and log1p does); -inf for d >= 0 - a strip whose two levels give the same G to the last bit has no width left in fp64
__device__ __forceinline__ double ehvi_log1mexp(double d) {
    if (d >= 0.0) return -__builtin_huge_val();
    return d > -0.69314718055994530942 ? log(-expm1(d)) : log1p(-exp(d));
}

// One strip: G1 at its right edge (g1n) and left edge (g1p; the first strip has none: first), G2 at its ceiling.  A strip whose
// g1n or g2 is -inf is -inf, not NaN (g1p <= g1n is then -inf too, and the difference of the two would be NaN).
__device__ __forceinline__ double ehvi_strip(bool first, double g1p, double g1n, double g2) {
    const double ninf = -__builtin_huge_val();
    if (g1n == ninf || g2 == ninf) return ninf;
    return first ? g1n + g2 : (g1n + ehvi_log1mexp(g1p - g1n)) + g2;
}

// Running-maximum logsumexp of the strips, in the order they are added: value = m + log(s), s = sum exp(t - m).
struct EhviSum {
    double m = -__builtin_huge_val(), s = 0.0;
    __device__ __forceinline__ void add(double t) {
        if (t == -__builtin_huge_val()) return;
        if (t > m) {
            s = s * exp(m - t) + 1.0;
            m = t;
        } else {
            s += exp(t - m);   // (t NaN: s becomes NaN and stays so)
        }
    }
    __device__ __forceinline__ double value() const { return m + log(s); }   // no strip above -inf: -inf + log 0 = -inf
};
