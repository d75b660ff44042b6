// Greedy q-point batch selection by rank-one posterior updates (not in the reference, which selects one
// point per iteration: /root/reference/point_selector.py:197-207).
//
// Once the dense posterior (mu, sigma) of a candidate set exists, conditioning the GP on one more (fantasy) observation at
// the chosen candidate x_j needs no N^2 work per candidate:
//     t_j(c)  = k(c, x_j) - k_c . beta_j - sum_{i<j} t_i(c) t_i(x_j) / s_i        beta_j = K^-1 k(X, x_j) = U (U^T k_j)
//     s_j     = var_j(x_j) - prior_var + ((1 + jitter1) + jitter2)
//     var'(c) = var(c) - t_j(c)^2 / s_j        mu'(c) = mu(c) + t_j(c) (y_j - mu(x_j)) / s_j
// k_c . beta_j is the sum kstar_mu_kernel (kernel_build.hip) forms for the mean with beta_j in place of alpha: N entries of
// K(X*,X) per candidate, generated in registers and never stored.  x_j is itself a candidate, so t_i(x_j) is an element of a
// stored vector, and the factorisation is only read.  y_j = mu(x_j) (Kriging believer: the mean stays, GP-BUCB under LCB) or
// a constant (constant liar).
//
// Per added member, all on the caller's stream and without a host round trip:
//     batch_pivot_kernel     x_j gathered through the index the previous step left on the device, k_j, the step's scalars
//     gpbo_alpha_f64         beta_j (the two U-products of the factorisation, factor.hip)
//     batch_downdate_kernel  every candidate: t_j, mu, sigma, acquisition, block arg-max without the members chosen so far
//     argmax_finish_kernel   the next member (sigma_acq.hip: lowest index on ties, NaN counted)
//     batch_record_kernel    idx_out / val_out, the guards
#include "cov_entry.h"

#include <cmath>
#include <limits>

namespace {

// What one step hands to the next, on the device.
struct BatchRec {
    int64_t idx[GPBO_BATCH_MAX_Q];  // member j as an index into Xs (without idx_offset); -1: none was chosen
    double s[GPBO_BATCH_MAX_Q];     // s_j
    double r[GPBO_BATCH_MAX_Q];     // of the step in hand: t_i(x_j) / s_i, i < j
    double xj[GPBO_MAX_D];          // x_j scaled by isc
    double g;                       // (y_j - mu(x_j)) / s_j
    int64_t nan_total;              // largest NaN count any step reported
    int32_t bad;                    // no further member: NaN acquisition, failed pivot, or nothing left to choose
    int32_t pad;
};

// k_j[n] = k(x_n, x_j) in the factorisation's own order (0 on the padding), the scaled x_j and the scalars of step j.
// grid ceil(Np / 256), block 256.  A member that does not exist (idx < 0: see batch_record_kernel) gives k_j = 0.
__global__ __launch_bounds__(256) void batch_pivot_kernel(const double *__restrict__ Xs, int64_t M,
                                                          const double *__restrict__ X, int N, int Np, int d, CovLs ls,
                                                          const double *__restrict__ mu, const double *__restrict__ sigma,
                                                          const double *__restrict__ T, int64_t ldt, int j,
                                                          double kappa_minus_prior, int fantasy, double lie,
                                                          BatchRec *__restrict__ rec, double *__restrict__ kj,
                                                          unsigned long long *__restrict__ nan_count,
                                                          int32_t *__restrict__ info) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    int64_t idx = rec->idx[j];
    const bool none = idx < 0 || idx >= M;
    if (none) idx = 0;   // every gather below stays inside Xs / mu / sigma / T
    const double *xj = Xs + idx * d;
    if (i < Np) {
        double v = 0.0;
        if (i < N && !none) {
            double acc = 0.0;   // cov_r2 over a run-time d, written out: k_j is a column of K as the factorisation saw it
            for (int k = 0; k < d; ++k) {
                const double diff = X[(int64_t)i * d + k] - xj[k];
                acc = fma(diff * diff, ls.il2[k], acc);
            }
            v = cov_from_r2<GPBO_KERNEL_SE>(acc);
        }
        kj[i] = v;
    }
    if (i != 0) return;
    *nan_count = 0ull;
    if (none || rec->bad) return;   // a batch that has ended (NaN acquisition): s, r, g and *info stay as its last step left them
    for (int k = 0; k < d; ++k) rec->xj[k] = xj[k] * ls.isc[k];
    const double sg = sigma[idx], m = mu[idx];
    const double s = sg * sg + kappa_minus_prior;
    const bool ok = s > 0.0 && s <= std::numeric_limits<double>::max();   // false for NaN
    rec->s[j] = s;
    for (int p = 0; p < j; ++p) rec->r[p] = T[(int64_t)p * ldt + idx] / rec->s[p];
    rec->g = (ok && fantasy == GPBO_FANTASY_LIE) ? (lie - m) / s : 0.0;
    if (!ok) {
        rec->bad = 1;
        if (*info == 0) *info = j + 1;
    }
}

// One launch per added member over all M candidates.  grid ceil(M / 512), block 256: a thread owns two adjacent candidates,
// coordinates pre-scaled in registers, and walks the N observations two at a time in the difference form (four independent
// distance / exp chains; observation rows and beta are wave-uniform and arrive through the scalar cache).  The expanded-
// distance MFMA form is not used here: t at and near x_j must be accurate (exp(-0) = 1 exactly at the pivot).
// No atomics in the sums (the NaN counter is an integer), fixed order everywhere: two calls give the same bits.
template <int D>
__global__ __launch_bounds__(256) void batch_downdate_kernel(const double *__restrict__ Xs, int64_t M,
                                                             const double *__restrict__ Xsc, int N, CovLs ls,
                                                             const double *__restrict__ beta,
                                                             const BatchRec *__restrict__ rec, int j,
                                                             double *__restrict__ T, int64_t ldt, double *__restrict__ mu,
                                                             double *__restrict__ sigma, int acq_kind, double p0, double p1,
                                                             int64_t idx_offset, double *__restrict__ part_val,
                                                             int64_t *__restrict__ part_idx,
                                                             unsigned long long *__restrict__ nan_count) {
    __shared__ double tab[GPBO_EXP_E];
    __shared__ double s_val[4];
    __shared__ int64_t s_idx[4];
    const int tid = threadIdx.x, lane = tid & 63;
    if (rec->bad) {   // uniform over the launch: nothing is updated, nothing can be chosen
        if (tid == 0) {
            part_val[blockIdx.x] = gpbo_none::val;
            part_idx[blockIdx.x] = gpbo_none::idx;
        }
        return;
    }
    cov_stage_tab(tab, tid);
    const int64_t c0 = ((int64_t)blockIdx.x * 256 + tid) * 2;
    const bool va = c0 < M, vb = c0 + 1 < M;
    double xa[D], xb[D];
#pragma unroll
    for (int k = 0; k < D; ++k) {
        xa[k] = (va ? Xs[c0 * D + k] : 0.0) * ls.isc[k];
        xb[k] = (vb ? Xs[(c0 + 1) * D + k] : 0.0) * ls.isc[k];
    }
    gpbo_syncthreads();
    double ta0 = 0.0, ta1 = 0.0, tb0 = 0.0, tb1 = 0.0;
    int n = 0;
    for (; n + 1 < N; n += 2) {
        const double *xo0 = Xsc + (int64_t)n * D;  // wave-uniform rows -> scalar loads
        const double *xo1 = xo0 + D;
        double s00, s01, s10, s11;
        cov_s4<D>(xa, xb, xo0, xo1, s00, s01, s10, s11);
        const double b0 = beta[n], b1 = beta[n + 1];
        ta0 = fma(cov_from_s<GPBO_KERNEL_SE>(s00, tab), b0, ta0);
        tb0 = fma(cov_from_s<GPBO_KERNEL_SE>(s01, tab), b0, tb0);
        ta1 = fma(cov_from_s<GPBO_KERNEL_SE>(s10, tab), b1, ta1);
        tb1 = fma(cov_from_s<GPBO_KERNEL_SE>(s11, tab), b1, tb1);
    }
    if (n < N) {  // odd tail
        const double *xo = Xsc + (int64_t)n * D;
        double sa, sb;
        cov_s2<D>(xa, xb, xo, sa, sb);
        const double bn = beta[n];
        ta0 = fma(cov_from_s<GPBO_KERNEL_SE>(sa, tab), bn, ta0);
        tb0 = fma(cov_from_s<GPBO_KERNEL_SE>(sb, tab), bn, tb0);
    }
    // t_j = k(c, x_j) - k_c . beta_j - sum_{i<j} t_i(c) r_i
    double pa, pb;
    cov_s2<D>(xa, xb, rec->xj, pa, pb);
    double t_a = cov_from_s<GPBO_KERNEL_SE>(pa, tab) - (ta0 + ta1), t_b = cov_from_s<GPBO_KERNEL_SE>(pb, tab) - (tb0 + tb1);
    if (va) {   // (c0 is even and ldt is: 16-byte pieces; column c0 + 1 < ldt exists even when candidate c0 + 1 does not)
        for (int p = 0; p < j; ++p) {
            const d2_t tp = *reinterpret_cast<const d2_t *>(T + (int64_t)p * ldt + c0);
            const double r = rec->r[p];
            t_a = fma(-tp.x, r, t_a);
            t_b = fma(-tp.y, r, t_b);
        }
        *reinterpret_cast<d2_t *>(T + (int64_t)j * ldt + c0) = d2_t{t_a, t_b};
    }
    const double s = rec->s[j], g = rec->g;
    double acq_a = 0.0, acq_b = 0.0;
    if (va) {
        const double sg = sigma[c0];
        const double m = mu[c0] + t_a * g, sn = sqrt(fabs(sg * sg - t_a * t_a / s));
        mu[c0] = m;
        sigma[c0] = sn;
        acq_a = gpbo_acquisition(acq_kind, m, sn, p0, p1);
    }
    if (vb) {
        const double sg = sigma[c0 + 1];
        const double m = mu[c0 + 1] + t_b * g, sn = sqrt(fabs(sg * sg - t_b * t_b / s));
        mu[c0 + 1] = m;
        sigma[c0 + 1] = sn;
        acq_b = gpbo_acquisition(acq_kind, m, sn, p0, p1);
    }
    const bool nan_a = va && (acq_a != acq_a), nan_b = vb && (acq_b != acq_b);
    bool use_a = va && !nan_a, use_b = vb && !nan_b;
    for (int p = 0; p <= j; ++p) {   // the members chosen so far leave the maximum
        const int64_t ci = rec->idx[p];
        if (ci == c0) use_a = false;
        if (ci == c0 + 1) use_b = false;
    }
    const unsigned long long mask_a = __ballot(nan_a), mask_b = __ballot(nan_b);
    if (lane == 0 && (mask_a | mask_b)) atomicAdd(nan_count, (unsigned long long)(__popcll(mask_a) + __popcll(mask_b)));
    double bv = use_a ? acq_a : gpbo_none::val;
    int64_t bi = use_a ? idx_offset + c0 : gpbo_none::idx;
    if (use_b && gpbo_better(acq_b, idx_offset + c0 + 1, bv, bi)) { bv = acq_b; bi = idx_offset + c0 + 1; }
    gpbo_argmax_post(bv, bi, lane, tid >> 6, s_val, s_idx);
    gpbo_syncthreads();
    if (tid == 0) {
        gpbo_argmax_fold(s_val, s_idx, 4, bv, bi);
        part_val[blockIdx.x] = bv;
        part_idx[blockIdx.x] = bi;
    }
}

// Member j from the arg-max record of its step; the guards.  One thread.
//   nothing chosen (every candidate NaN or already a member, or an earlier guard)  ->  idx_out[j] = -1, val_out[j] = NaN
//   NaN acquisition anywhere (the caller raises)                                    ->  every LATER member is -1
__global__ void batch_record_kernel(gpbo_result *__restrict__ result, int j, int64_t idx_offset, BatchRec *__restrict__ rec,
                                    int64_t *__restrict__ idx_out, double *__restrict__ val_out) {
    if (result->nan_count > rec->nan_total) rec->nan_total = result->nan_count;
    const int64_t bi = result->best_idx;
    if (rec->bad || bi == gpbo_none::idx) {
        rec->bad = 1;
        rec->idx[j] = -1;
        idx_out[j] = -1;
        val_out[j] = __builtin_nan("");
        result->best_idx = -1;
        result->best_val = __builtin_nan("");
    } else {
        rec->idx[j] = bi - idx_offset;
        idx_out[j] = bi;
        val_out[j] = result->best_val;
    }
    if (rec->nan_total > 0) rec->bad = 1;
    result->nan_count = rec->nan_total;
}

struct Layout {
    BatchRec *rec;
    unsigned long long *nan;
    void *acq;   // gpbo_acq_workspace_bytes() for member 0's arg-max
    double *part_val;
    int64_t *part_idx;
    double *xsc, *kj, *tmp, *beta, *t;
    int64_t total, ldt, nblk;
    Layout(void *work, int64_t Np, int64_t M, int32_t q) {
        Carver c(work);
        nblk = (M + 511) / 512;
        ldt = align_up(M, 2);
        rec = c.take<BatchRec>(1);
        nan = c.take<unsigned long long>(32);   // 256 bytes
        acq = c.take_bytes(gpbo_acq_workspace_bytes());
        part_val = c.take<double>(nblk);
        part_idx = c.take<int64_t>(nblk);
        xsc = c.take<double>(Np * GPBO_MAX_D);
        kj = c.take<double>(Np);
        tmp = c.take<double>(Np);
        beta = c.take<double>(Np);
        t = c.take<double>(ldt * (q > 1 ? q - 1 : 1));
        total = c.total();
    }
};

bool sizes_ok(int64_t Np, int64_t M, int32_t q) {
    return np_ok(Np) && Np <= (1 << 20) && M >= 1 && M <= ((int64_t)1 << 40) && q >= 1 && q <= GPBO_BATCH_MAX_Q && q <= M;
}

}  // namespace

extern "C" int64_t gpbo_batch_workspace_bytes(int64_t Np, int64_t M, int32_t q) {
    if (!sizes_ok(Np, M, q)) return GPBO_ERR_ARG;
    return Layout(nullptr, Np, M, q).total;
}

extern "C" int gpbo_select_batch_f64(const double *Xs, int64_t M, const double *X, int64_t N, int64_t Np, int32_t d,
                                     const double *ls_host, const double *U, const double *alpha, double jitter1,
                                     double jitter2, double prior_var, int32_t acq_kind, double p0, double p1, int32_t q,
                                     int32_t fantasy, double lie, double *mu, double *sigma, int64_t idx_offset,
                                     int64_t *idx_out, double *val_out, gpbo_result *result, int32_t *info, void *work,
                                     int64_t work_bytes, void *stream) {
    if (!Xs || !X || !ls_host || !U || !alpha || !mu || !sigma || !idx_out || !val_out || !result || !info || !work)
        return GPBO_ERR_ARG;
    if (N < 1 || Np < N || d < 1 || d > GPBO_MAX_D || !sizes_ok(Np, M, q)) return GPBO_ERR_ARG;
    if (!acq_kind_ok(acq_kind) || !length_scales_ok(ls_host, d)) return GPBO_ERR_ARG;
    if (fantasy != GPBO_FANTASY_BELIEVER && fantasy != GPBO_FANTASY_LIE) return GPBO_ERR_ARG;
    if (fantasy == GPBO_FANTASY_LIE && !std::isfinite(lie)) return GPBO_ERR_ARG;
    if (!std::isfinite(prior_var) || !std::isfinite(jitter1) || !std::isfinite(jitter2)) return GPBO_ERR_ARG;
    const Layout L(work, Np, M, q);
    if (work_bytes < L.total || !aligned_to(work, 256)) return GPBO_ERR_WORKSPACE;

    CovLs ls;
    for (int k = 0; k < GPBO_MAX_D; ++k) ls.il2[k] = ls.isc[k] = 0.0;
    (void)length_scale_scalings(ls_host, d, ls.il2, ls.isc);   // (cannot refuse: length_scales_ok above has)
    hipStream_t st = gpbo_stream(stream);
    const double kappa_minus_prior = ((1.0 + jitter1) + jitter2) - prior_var;   // 0 for the prior_var the classes pass

    if (hipMemsetAsync(L.rec, 0, sizeof(BatchRec), st) != hipSuccess || hipMemsetAsync(info, 0, sizeof(int32_t), st) != hipSuccess)
        return GPBO_ERR_LAUNCH;
    // member 0: the arg-max of the posterior as it came in (the plain pass's own acquisition on the same mu / sigma)
    int rc = gpbo_acq_argmax_f64(mu, sigma, M, acq_kind, p0, p1, idx_offset, nullptr, result, L.acq,
                                 gpbo_acq_workspace_bytes(), stream);
    if (rc != GPBO_OK) return rc;
    hipLaunchKernelGGL(batch_record_kernel, dim3(1), dim3(1), 0, st, result, 0, idx_offset, L.rec, idx_out, val_out);
    GPBO_CHECK_LAUNCH();
    if (q == 1) return GPBO_OK;
    rc = gpbo_scale_points_launch(X, N, Np, d, ls_host, L.xsc, nullptr, stream);
    if (rc != GPBO_OK) return rc;
    for (int j = 0; j + 1 < q; ++j) {
        hipLaunchKernelGGL(batch_pivot_kernel, dim3((unsigned)((Np + 255) / 256)), dim3(256), 0, st, Xs, M, X, (int)N, (int)Np,
                           (int)d, ls, mu, sigma, L.t, L.ldt, j, kappa_minus_prior, (int)fantasy, lie, L.rec, L.kj, L.nan, info);
        GPBO_CHECK_LAUNCH();
        rc = gpbo_alpha_f64(U, L.kj, N, Np, L.tmp, L.beta, stream);
        if (rc != GPBO_OK) return rc;
#define CALL(DD)                                                                                                                     \
    hipLaunchKernelGGL(batch_downdate_kernel<DD>, dim3((unsigned)L.nblk), dim3(256), 0, st, Xs, M, L.xsc, (int)N, ls, L.beta, L.rec, \
                       j, L.t, L.ldt, mu, sigma, (int)acq_kind, p0, p1, idx_offset, L.part_val, L.part_idx, L.nan)
        GPBO_FOR_D(d, CALL)
#undef CALL
        GPBO_CHECK_LAUNCH();
        rc = gpbo_launch_argmax_finish(L.part_val, L.part_idx, L.nblk, L.nan, result, st);
        if (rc != GPBO_OK) return rc;
        hipLaunchKernelGGL(batch_record_kernel, dim3(1), dim3(1), 0, st, result, j + 1, idx_offset, L.rec, idx_out, val_out);
        GPBO_CHECK_LAUNCH();
    }
    return GPBO_OK;
}
