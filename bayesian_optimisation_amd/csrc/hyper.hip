// The marginal likelihood over ALL hyperparameters of the surrogate (ML-II: ard="hyper"), and leave-one-out prediction.
//
// The reference fixes the signal variance at 1, the mean at 0 and the diagonal term at 1e-4 + 1e-6 (point_selector.py:78-79,
// :193) and fits the length scales only.  Here the model is y ~ N(m 1, s^2 Kt), Kt = K0(ls) + rho I, rho > 0 the
// noise-to-signal ratio.  Mean and scale have closed forms given (ls, rho), so the optimiser sees d + 1 variables.  From a
// factorisation of Kt made by gpbo_factorise_f64 with (jitter1, jitter2) = (rho, 0) and the raw y - U = L^-T, a = Kt^-1 y -
// and b = Kt^-1 1 (one more gpbo_alpha_f64 on a vector of ones):
//     m      = (1 . a) / (1 . b)  (0 without GPBO_HYPER_MEAN),  r = y - m,  alpha = a - m b
//     s^2    = (r . alpha) / N    (1 without GPBO_HYPER_SCALE)
//     L      = 1/2 [(r . alpha) / s^2 + N log s^2 + log det Kt + N log 2 pi]
//     dL / dlog ls_k = 1/2 sum_ij W_ij K0_ij (x_ik - x_jk)^2 / ls_k^2,   W = Kt^-1 - alpha alpha^T / s^2
//     dL / dlog rho  = 1/2 rho (tr Kt^-1 - |alpha|^2 / s^2),   tr Kt^-1 = sum_i kappa_i,  kappa_i = sum_{j >= i} U_ij^2
// (no derivative of m or s^2 appears: both are stationary points of L).  gpbo_nlml_grad_f64 called with alpha / s and r / s
// returns exactly those d length-scale gradients and L - 1/2 N log s^2, so csrc/ard_grad.hip is used as it is.
// kappa_i is also the diagonal of Kt^-1, which makes leave-one-out prediction free (gpbo_loo_f64):
//     mu_loo_i = y_i - alpha_i / kappa_i,   var_loo_i = s^2 / kappa_i.
//
// Launches of gpbo_nlml_hyper_f64, all on the caller's stream:
//     hyper_rowsum_kernel    kappa [N] from the upper triangle of U: a wave per row, only j >= i and only rows < N are read
//                            (the padding of U holds the identity and must not be counted); also writes the vector of ones
//     gpbo_alpha_f64         b = U (U^T 1)   (factor.hip)
//     hyper_profile_kernel   one workgroup: 1 . a, 1 . b, tr Kt^-1; m, then r . alpha and |alpha|^2 summed directly
//                            (not as y . a - (1 . a)^2 / (1 . b), which cancels when y has a large offset);
//                            alpha / s and r / s as [Np] vectors, zero on the padding
//     gpbo_nlml_grad_f64     the d length-scale gradients and the value without 1/2 N log s^2   (ard_grad.hip)
//     hyper_finish_kernel    out [d + 4]; every entry NaN when info != 0, 1 . b or s^2 not positive and finite
// No atomics, every sum in a fixed order: two calls give the same bits.
#include "gpbo_internal.h"

namespace {

constexpr int PROFILE_THREADS = 1024;
constexpr int PROFILE_WAVES = PROFILE_THREADS / 64;

// kappa_i = sum_{j = i}^{N - 1} U_ij^2 for the rows i < N; ones_i = 1 (optional).  One wave per row, four rows per workgroup;
// lane l adds the columns (i & ~63) + l + 64 t in increasing t, then a butterfly: a fixed order.  No barrier in this kernel.
__global__ __launch_bounds__(256) void hyper_rowsum_kernel(const double *__restrict__ U, int64_t N, int64_t Np,
                                                           double *__restrict__ kappa, double *__restrict__ ones) {
    const int lane = threadIdx.x & 63;
    const int64_t i = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (i >= N) return;
    const double *u = U + i * Np;
    double s0 = 0.0, s1 = 0.0, s2 = 0.0, s3 = 0.0;
    for (int64_t j = (i & ~(int64_t)63) + lane; j < N; j += 256) {
        // (j + 64 t < N <= Np: inside the row)
        const double v0 = (j >= i) ? u[j] : 0.0;
        const double v1 = (j + 64 < N) ? u[j + 64] : 0.0;
        const double v2 = (j + 128 < N) ? u[j + 128] : 0.0;
        const double v3 = (j + 192 < N) ? u[j + 192] : 0.0;
        s0 = fma(v0, v0, s0);
        s1 = fma(v1, v1, s1);
        s2 = fma(v2, v2, s2);
        s3 = fma(v3, v3, s3);
    }
    double s = (s0 + s1) + (s2 + s3);
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) s += __shfl_xor(s, off);
    if (lane == 0) {
        kappa[i] = s;
        if (ones) ones[i] = 1.0;
    }
}

// Sum of v over the workgroup in a fixed order, the same bits in every thread: butterfly in the wave, then the waves in order.
__device__ __forceinline__ double profile_sum(double v, double *red) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off);
    gpbo_syncthreads();   // the previous sum has been read
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
    gpbo_syncthreads();
    double s = 0.0;
#pragma unroll
    for (int w = 0; w < PROFILE_WAVES; ++w) s += red[w];
    return s;
}

// scal: [0] m, [1] s^2, [2] |alpha|^2 / s^2, [3] tr Kt^-1, [4] 1 . b
__global__ __launch_bounds__(PROFILE_THREADS) void hyper_profile_kernel(const double *__restrict__ a, const double *__restrict__ b,
                                                                        const double *__restrict__ y,
                                                                        const double *__restrict__ kappa, int64_t N, int64_t Np,
                                                                        int flags, double *__restrict__ alpha_std,
                                                                        double *__restrict__ r_std,
                                                                        double *__restrict__ alpha_std_out,
                                                                        double *__restrict__ scal) {
    __shared__ double red[PROFILE_WAVES];
    const int tid = threadIdx.x;
    double sa = 0.0, sb = 0.0, str = 0.0;
    for (int64_t i = tid; i < N; i += PROFILE_THREADS) {
        sa += a[i];
        sb += b[i];
        str += kappa[i];
    }
    sa = profile_sum(sa, red);
    sb = profile_sum(sb, red);
    str = profile_sum(str, red);
    const double m = (flags & GPBO_HYPER_MEAN) ? sa / sb : 0.0;
    double ra = 0.0, aa = 0.0;
    for (int64_t i = tid; i < N; i += PROFILE_THREADS) {
        const double al = a[i] - m * b[i];
        ra = fma(y[i] - m, al, ra);
        aa = fma(al, al, aa);
    }
    ra = profile_sum(ra, red);
    aa = profile_sum(aa, red);
    // (without the mean this is y . a itself)
    const double s2 = (flags & GPBO_HYPER_SCALE) ? ra / (double)N : 1.0;
    const double s = sqrt(s2);
    for (int64_t i = tid; i < Np; i += PROFILE_THREADS) {
        double al = 0.0, r = 0.0;
        if (i < N) {
            al = (a[i] - m * b[i]) / s;
            r = (y[i] - m) / s;
        }
        alpha_std[i] = al;
        r_std[i] = r;
        if (alpha_std_out) alpha_std_out[i] = al;
    }
    if (tid == 0) {
        scal[0] = m;
        scal[1] = s2;
        scal[2] = aa / s2;
        scal[3] = str;
        scal[4] = sb;
    }
}

// out[0] = L, out[1 .. d] = the length-scale gradients, out[1 + d] = dL / dlog rho, out[2 + d] = m, out[3 + d] = s^2
__global__ __launch_bounds__(64) void hyper_finish_kernel(const double *__restrict__ gout, const double *__restrict__ scal, int d,
                                                          int64_t N, double rho, const int32_t *__restrict__ info,
                                                          double *__restrict__ out) {
    const int k = threadIdx.x;
    if (k >= d + 4) return;
    const double m = scal[0], s2 = scal[1], sb = scal[4];
    const double inf = __builtin_huge_val();
    const bool bad = *info != 0 || !(sb > 0.0 && sb < inf) || !(s2 > 0.0 && s2 < inf);
    double v;
    if (k == 0) v = gout[0] + 0.5 * (double)N * log(s2);
    else if (k <= d) v = gout[k];
    else if (k == d + 1) v = 0.5 * rho * (scal[3] - scal[2]);
    else if (k == d + 2) v = m;
    else v = s2;
    out[k] = bad ? __builtin_nan("") : v;
}

// mu_loo_i = y_i - alpha_i / kappa_i, var_loo_i = scale2 / kappa_i, kinv_diag_i = kappa_i; each output optional
__global__ __launch_bounds__(256) void loo_kernel(const double *__restrict__ kappa, const double *__restrict__ alpha,
                                                  const double *__restrict__ y, int64_t N, double scale2,
                                                  double *__restrict__ mu_out, double *__restrict__ var_out,
                                                  double *__restrict__ kinv_out) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= N) return;
    const double k = kappa[i];
    if (mu_out) mu_out[i] = y[i] - alpha[i] / k;
    if (var_out) var_out[i] = scale2 / k;
    if (kinv_out) kinv_out[i] = k;
}

int64_t align256(int64_t b) { return (b + 255) / 256 * 256; }

bool positive_finite(double v) { return v > 0.0 && v < __builtin_huge_val(); }

// the workspace of gpbo_nlml_hyper_f64: the gradient's own, then six [Np] vectors and the scalars
struct HyperLayout {
    void *grad_work;
    double *kappa, *ones, *tmp, *b, *alpha_std, *r_std, *scal, *gout;
    int64_t wgrad, total;
    HyperLayout(void *work, int64_t Np, int32_t d) {
        Carver c(work);
        wgrad = gpbo_nlml_grad_workspace_bytes(Np, d);
        grad_work = c.take_bytes(wgrad);
        kappa = c.take<double>(Np);
        ones = c.take<double>(Np);
        tmp = c.take<double>(Np);
        b = c.take<double>(Np);
        alpha_std = c.take<double>(Np);   // alpha / s
        r_std = c.take<double>(Np);       // r / s
        scal = c.take<double>(32);
        gout = c.take<double>(32);        // the gradient's out
        total = c.total();
    }
};

int launch_rowsum(const double *U, int64_t N, int64_t Np, double *kappa, double *ones, hipStream_t st) {
    hipLaunchKernelGGL(hyper_rowsum_kernel, dim3((unsigned)((N + 3) / 4)), dim3(256), 0, st, U, N, Np, kappa, ones);
    GPBO_CHECK_LAUNCH();
    return GPBO_OK;
}

}  // namespace

extern "C" int64_t gpbo_nlml_hyper_workspace_bytes(int64_t Np, int32_t d) {
    if (gpbo_nlml_grad_workspace_bytes(Np, d) < 0) return GPBO_ERR_ARG;
    return HyperLayout(nullptr, Np, d).total;
}

extern "C" int gpbo_nlml_hyper_f64(const double *U, const double *alpha, const double *y, const double *X, int64_t N,
                                   int64_t Np, int32_t d, const double *ls_host, double noise, int32_t flags,
                                   const int32_t *info, double *out, double *alpha_std_out, void *work, int64_t work_bytes,
                                   void *stream) {
    return gpbo_nlml_hyper_kern_f64(U, alpha, y, X, N, Np, d, ls_host, GPBO_KERNEL_SE, noise, flags, info, out, alpha_std_out, work,
                                    work_bytes, stream);
}

// The profiled mean and scale, the noise gradient and the finish never see the covariance function: the family only travels
// to the length-scale gradients (gpbo_nlml_grad_kern_f64).
extern "C" int gpbo_nlml_hyper_kern_f64(const double *U, const double *alpha, const double *y, const double *X, int64_t N,
                                        int64_t Np, int32_t d, const double *ls_host, int32_t kernel, double noise,
                                        int32_t flags, const int32_t *info, double *out, double *alpha_std_out, void *work,
                                        int64_t work_bytes, void *stream) {
    if (!U || !alpha || !y || !X || !ls_host || !info || !out || !work) return GPBO_ERR_ARG;
    if (!kernel_ok(kernel, d)) return GPBO_ERR_ARG;
    if (N < 1 || Np != gpbo_padded_n(N) || Np > (1 << 20) || d < 1 || d > GPBO_MAX_D) return GPBO_ERR_ARG;
    if (!positive_finite(noise) || (flags & ~(GPBO_HYPER_MEAN | GPBO_HYPER_SCALE))) return GPBO_ERR_ARG;
    if (!length_scales_ok(ls_host, d)) return GPBO_ERR_ARG;
    if (!aligned_to(U, 16) || !aligned_to(work, 16)) return GPBO_ERR_ARG;
    const HyperLayout L(work, Np, d);
    if (work_bytes < L.total) return GPBO_ERR_WORKSPACE;
    hipStream_t st = gpbo_stream(stream);
    int rc = launch_rowsum(U, N, Np, L.kappa, L.ones, st);
    if (rc != GPBO_OK) return rc;
    rc = gpbo_alpha_f64(U, L.ones, N, Np, L.tmp, L.b, stream);
    if (rc != GPBO_OK) return rc;
    hipLaunchKernelGGL(hyper_profile_kernel, dim3(1), dim3(PROFILE_THREADS), 0, st, alpha, L.b, y, L.kappa, N, Np, (int)flags,
                       L.alpha_std, L.r_std, alpha_std_out, L.scal);
    GPBO_CHECK_LAUNCH();
    rc = gpbo_nlml_grad_kern_f64(U, L.alpha_std, L.r_std, X, N, Np, d, ls_host, kernel, info, L.gout, L.grad_work, L.wgrad, stream);
    if (rc != GPBO_OK) return rc;
    hipLaunchKernelGGL(hyper_finish_kernel, dim3(1), dim3(64), 0, st, L.gout, L.scal, (int)d, N, noise, info, out);
    GPBO_CHECK_LAUNCH();
    return GPBO_OK;
}

extern "C" int64_t gpbo_loo_workspace_bytes(int64_t Np) {
    if (Np < GPBO_NPAD || Np % GPBO_NPAD) return GPBO_ERR_ARG;
    return align256((int64_t)sizeof(double) * Np);
}

extern "C" int gpbo_loo_f64(const double *U, const double *alpha, const double *y, int64_t N, int64_t Np, double scale2,
                            double *mu_out, double *var_out, double *kinv_diag_out, void *work, int64_t work_bytes,
                            void *stream) {
    if (!U || !alpha || !y || !work) return GPBO_ERR_ARG;
    if (N < 1 || Np != gpbo_padded_n(N) || !positive_finite(scale2)) return GPBO_ERR_ARG;
    if (!aligned_to(U, 16) || !aligned_to(work, 16)) return GPBO_ERR_ARG;
    if (work_bytes < gpbo_loo_workspace_bytes(Np)) return GPBO_ERR_WORKSPACE;
    double *kappa = reinterpret_cast<double *>(work);
    hipStream_t st = gpbo_stream(stream);
    const int rc = launch_rowsum(U, N, Np, kappa, nullptr, st);
    if (rc != GPBO_OK) return rc;
    hipLaunchKernelGGL(loo_kernel, dim3((unsigned)((N + 255) / 256)), dim3(256), 0, st, kappa, alpha, y, N, scale2, mu_out,
                       var_out, kinv_diag_out);
    GPBO_CHECK_LAUNCH();
    return GPBO_OK;
}
