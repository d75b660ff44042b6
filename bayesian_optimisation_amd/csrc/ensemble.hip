// Candidates scored under an ENSEMBLE of surrogates: the acquisition integrated over samples of the hyperparameter posterior
// (ard="marginal"; Snoek, Larochelle & Adams 2012).  Not in the reference, which scores under one frozen model
// (point_selector.py:63-101).
//
// S models share the observations and the covariance family and differ in (ls_s, rho_s, m_s, s_s): model s is y ~ N(m_s 1,
// s_s^2 (K0(ls_s) + rho_s I)), held as the factorisation of the standardised (y - m_s) / s_s.  For each model in index order
//   gpbo_posterior_acq_f64_split  the fp64 pass of every other scoring entry, unchanged: the model's dense mu, sigma (model
//                                 units) into the workspace
//   ensemble_fold_kernel          one thread per candidate: mu_y = m_s + s_s mu, sigma_y = s_s sigma and, with
//                                 shift = sum_s w_s m_s from the host,
//                                     acq += w_s acquisition(kind, mu_y, sigma_y, p0, p1)
//                                     dm  += w_s (mu_y - shift)
//                                     dv  += w_s (sigma_y^2 + (mu_y - shift)^2)
//                                 (the first model stores instead of adding: no clearing pass, and one model of weight 1 leaves
//                                 the pass's own bits).  The moments are taken about `shift` so that dv - dm^2 does not cancel
//                                 like (mean / sd)^2 of y.  Traffic per candidate and model: mu and sigma read, three
//                                 accumulators read and written - 64 bytes (40 for the first model).
// The LAST model's instance also finishes: mean = shift + dm, sd = sqrt(max(dv - dm^2, 0)), the dense stores, the NaN count and the
// workgroup's arg-max record (gpbo_argmax_post / _fold); gpbo_launch_argmax_finish folds the records.  A candidate belongs to a
// fixed thread of a fixed workgroup whatever the chunk of the per-model pass, whose values do not depend on the chunk either:
// the same bits from call to call and for any chunk.
#include "gpbo_internal.h"

#include <cmath>

namespace {

constexpr int FOLD_BLOCKS_MAX = 1024;

template <bool FIRST, bool LAST>
__global__ __launch_bounds__(256) void ensemble_fold_kernel(const double *__restrict__ mu, const double *__restrict__ sigma,
                                                            int64_t M, double w, double y_mean, double y_scale, double shift,
                                                            int acq_kind, double p0, double p1, double *__restrict__ acc_acq,
                                                            double *__restrict__ acc_dm, double *__restrict__ acc_dv,
                                                            int64_t idx_base, double *__restrict__ mean_out,
                                                            double *__restrict__ sd_out, double *__restrict__ acq_out,
                                                            double *__restrict__ part_val, int64_t *__restrict__ part_idx,
                                                            unsigned long long *__restrict__ nan_count) {
    __shared__ double s_val[4];
    __shared__ int64_t s_idx[4];
    const int tid = threadIdx.x, lane = tid & 63;
    double bv = gpbo_none::val;
    int64_t bi = gpbo_none::idx;
    // (every lane of a wave makes the same number of trips: the ballot inside gpbo_count_nan sees whole waves)
    const int64_t stride = (int64_t)gridDim.x * 256;
    for (int64_t c0 = (int64_t)blockIdx.x * 256; c0 < M; c0 += stride) {
        const int64_t c = c0 + tid;
        const bool valid = c < M;
        double a = 0.0;
        if (valid) {
            const double mu_y = y_mean + y_scale * mu[c];
            const double sigma_y = y_scale * sigma[c];
            const double dmu = mu_y - shift;
            a = w * gpbo_acquisition(acq_kind, mu_y, sigma_y, p0, p1);
            double dm = w * dmu;
            double dv = w * (sigma_y * sigma_y + dmu * dmu);
            if (!FIRST) {
                a = acc_acq[c] + a;
                dm = acc_dm[c] + dm;
                dv = acc_dv[c] + dv;
            }
            if (!LAST) {
                acc_acq[c] = a;
                acc_dm[c] = dm;
                acc_dv[c] = dv;
            } else {
                if (mean_out) mean_out[c] = shift + dm;
                const double var = dv - dm * dm;
                if (sd_out) sd_out[c] = sqrt(var < 0.0 ? 0.0 : var);   // (not fmax: a NaN candidate stays NaN)
                if (acq_out) acq_out[c] = a;
            }
        }
        if (LAST) {
            const bool is_nan = valid && (a != a);
            gpbo_count_nan(is_nan, lane, nan_count);
            if (valid && !is_nan && gpbo_better(a, idx_base + c, bv, bi)) { bv = a; bi = idx_base + c; }
        }
    }
    if (LAST) {
        gpbo_argmax_post(bv, bi, lane, tid >> 6, s_val, s_idx);
        gpbo_syncthreads();
        if (tid == 0) {
            gpbo_argmax_fold(s_val, s_idx, 4, bv, bi);
            part_val[blockIdx.x] = bv;
            part_idx[blockIdx.x] = bi;
        }
    }
}

static_assert(FOLD_BLOCKS_MAX * 8 % 256 == 0, "the partial records are carved in whole 256-byte granules");
struct EnsembleLayout {
    void *post_work;   // the workspace of the per-model fp64 pass, post bytes
    double *mu, *sigma, *acc_acq, *acc_dm, *acc_dv, *pval;
    int64_t *pidx;
    unsigned long long *nan;
    gpbo_result *res;   // the per-model pass's own result record: not reported
    int64_t post, total;
    EnsembleLayout(void *work, int64_t Np, int64_t chunk, int64_t M) {
        Carver c(work);
        post = gpbo_posterior_workspace_bytes_split(Np, chunk, M, 1);
        post_work = c.take_bytes(post);
        mu = c.take<double>(M);
        sigma = c.take<double>(M);
        acc_acq = c.take<double>(M);
        acc_dm = c.take<double>(M);
        acc_dv = c.take<double>(M);
        pval = c.take<double>(FOLD_BLOCKS_MAX);
        pidx = c.take<int64_t>(FOLD_BLOCKS_MAX);
        nan = c.take<unsigned long long>(32);   // 256 bytes
        res = static_cast<gpbo_result *>(c.take_bytes(256));
        total = c.total();
    }
};

bool positive_finite(double v) { return v > 0.0 && v < __builtin_huge_val(); }

}  // namespace

extern "C" int64_t gpbo_ensemble_workspace_bytes(int64_t Np, int64_t chunk, int64_t M) {
    if (gpbo_posterior_workspace_bytes_split(Np, chunk, M, 1) < 0 || M > ((int64_t)1 << 40)) return GPBO_ERR_ARG;
    return EnsembleLayout(nullptr, Np, chunk, M).total;
}

extern "C" int gpbo_ensemble_acq_f64(const double *Xs, int64_t M, const double *X, int64_t N, int64_t Np, int32_t d, int32_t S,
                                     const double *ls_host, int32_t kernel, const double *U, const double *alpha,
                                     const double *model_host, int32_t acq_kind, double p0, double p1, int64_t idx_offset,
                                     int64_t chunk, double *mean_out, double *sd_out, double *acq_out, gpbo_result *result,
                                     void *work, int64_t work_bytes, void *stream) {
    if (!Xs || !X || !ls_host || !U || !alpha || !model_host || !result || !work) return GPBO_ERR_ARG;
    if (S < 1 || S > GPBO_ENSEMBLE_MAX_S || d < 1 || d > GPBO_MAX_D || !kernel_ok(kernel, d)) return GPBO_ERR_ARG;
    if (M < 1 || M > ((int64_t)1 << 40) || N < 1 || Np != gpbo_padded_n(N) || Np > (1 << 20)) return GPBO_ERR_ARG;
    if (!chunk_ok(chunk) || !acq_kind_ok(acq_kind)) return GPBO_ERR_ARG;
    if (!length_scales_ok(ls_host, S * d)) return GPBO_ERR_ARG;
    double wsum = 0.0, shift = 0.0;
    for (int s = 0; s < S; ++s) {
        const double *m = model_host + 4 * s;
        if (!(m[0] >= 0.0 && m[0] < __builtin_huge_val()) || !positive_finite(m[1]) || !(fabs(m[2]) < __builtin_huge_val()) ||
            !positive_finite(m[3]))
            return GPBO_ERR_ARG;
        wsum += m[0];
        shift += m[0] * m[2];
    }
    if (!(wsum > 0.0)) return GPBO_ERR_ARG;
    if (!aligned_to(U, 16)) return GPBO_ERR_ARG;
    if (!aligned_to(work, 256)) return GPBO_ERR_WORKSPACE;
    const EnsembleLayout L(work, Np, chunk, M);
    if (work_bytes < L.total) return GPBO_ERR_WORKSPACE;
    hipStream_t st = gpbo_stream(stream);
    if (hipMemsetAsync(L.nan, 0, sizeof(unsigned long long), st) != hipSuccess) return GPBO_ERR_LAUNCH;
    int64_t nblk = (M + 255) / 256;
    if (nblk > FOLD_BLOCKS_MAX) nblk = FOLD_BLOCKS_MAX;
    for (int s = 0; s < S; ++s) {
        const double *m = model_host + 4 * s;
        const GpModel gp = {X, N, Np, d, ls_host + (int64_t)s * d, U + (int64_t)s * Np * Np, alpha + (int64_t)s * Np, m[1], kernel};
        // (the pass's own acquisition and arg-max, in model units, are not used: LCB with explore 0 is the cheapest it has)
        int rc = gpbo_posterior_acq_f64_split(Xs, M, gp, {GPBO_ACQ_LCB, 0.0, 0.0}, 0.0, idx_offset, chunk,
                                              {L.mu, L.sigma, nullptr, nullptr}, L.res, L.post_work, L.post, nullptr, 1, 0, stream);
        if (rc != GPBO_OK) return rc;
        const bool first = s == 0, last = s == S - 1;
#define GPBO_FOLD_LAUNCH(F, LL)                                                                                                          \
    hipLaunchKernelGGL((ensemble_fold_kernel<F, LL>), dim3((unsigned)nblk), dim3(256), 0, st, L.mu, L.sigma, M, m[0], m[2], m[3], shift, \
                       (int)acq_kind, p0, p1, L.acc_acq, L.acc_dm, L.acc_dv, idx_offset, mean_out, sd_out, acq_out, L.pval, L.pidx,      \
                       L.nan)
        if (first && last) GPBO_FOLD_LAUNCH(true, true);
        else if (first) GPBO_FOLD_LAUNCH(true, false);
        else if (last) GPBO_FOLD_LAUNCH(false, true);
        else GPBO_FOLD_LAUNCH(false, false);
#undef GPBO_FOLD_LAUNCH
        GPBO_CHECK_LAUNCH();
    }
    return gpbo_launch_argmax_finish(L.pval, L.pidx, nblk, L.nan, result, st);
}
