// Constrained expected improvement, probability of improvement and probability of feasibility on the dense posterior, in LOG
// space (Gardner et al. 2014, Gelbart, Snoek & Adams 2014; not in the reference, whose docs name probability of
// improvement as a wish).  For a candidate with objective posterior (mu, sigma) and C >= 0 constraint posteriors (mu_c, sigma_c)
// with upper limits u_c - feasible means g_c(x) <= u_c, every constraint a GP of its own, taken as independent:
//     feas(x)  = sum_{c < C} log Phi((u_c - mu_c) / sigma_c)                   (added in index order, c = 0 first, from 0)
//     value(x) = base(x) + feas(x),   base = 0 | log sigma + log h(z) | log Phi(z),   z = ((f_best - mu) - xi) / sigma
// (cons_math.h).  The plain product of C normal CDFs is exactly 0 as soon as the candidates are a few dozen standard deviations
// inside the infeasible region - the normal state at the start of a constrained run - and every candidate then ties; the sum of
// logarithms keeps their order.  A function of dense (mu, sigma) arrays alone: no covariance entry, every kernel family, every
// model record.
//     constrained_acq_kernel    the shape of mes_acq_kernel (mes.hip): min(ceil(M / 256), 1024) workgroups of 256 threads,
//                               grid-striding; a thread loads its candidate's 2 + 2 C values (consecutive threads, consecutive
//                               addresses in every array), the limits and scalars arrive by value in the kernel-argument record
//                               (uniform: scalar registers); the optional dense stores; the workgroup's arg-max record, folded
//                               by gpbo_launch_argmax_finish
// Edge rules (restated in tests/constrained_ref.py): a NaN in any input the call reads gives value NaN, counted once in nan_count
// and never chosen; sigma_c == 0 is certain either way (0 or -inf); sigma == 0: EI log(max(imp, 0)), PI 0 where imp > 0 else -inf;
// -inf is a legal value that beats the empty record, so an all -inf input returns its lowest index.
// No sum crosses candidates; the grid depends on M alone; only the integer NaN counter is atomic: two calls give the same bits.
#include "gpbo_internal.h"
#include "cons_math.h"

namespace {

constexpr int CONS_MAX_BLOCKS = 1024;

struct ConsArgs {
    double upper[GPBO_CONS_MAX_C];
    double f_best, xi;
    int32_t base, C;
};

// grid min(ceil(M / 256), 1024), block 256.  Every trip of the candidate loop is taken by the whole workgroup (gpbo_count_nan is a
// wave-wide ballot), the tail masked by `valid`.  mu / sigma are read only when the base needs them, row c of cons_mu / cons_sigma
// only for c < C.
__global__ __launch_bounds__(256) void constrained_acq_kernel(const double *__restrict__ mu, const double *__restrict__ sigma,
                                                              int64_t M, const double *__restrict__ cons_mu,
                                                              const double *__restrict__ cons_sigma, int64_t ldc, ConsArgs a,
                                                              int64_t idx_base, double *__restrict__ val_out,
                                                              double *__restrict__ feas_out, double *__restrict__ part_val,
                                                              int64_t *__restrict__ part_idx,
                                                              unsigned long long *__restrict__ nan_count) {
    __shared__ double s_val[4];
    __shared__ int64_t s_idx[4];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    double bv = gpbo_none::val;
    int64_t bi = gpbo_none::idx;
    for (int64_t b = (int64_t)blockIdx.x * 256; b < M; b += (int64_t)gridDim.x * 256) {
        const int64_t c = b + tid;
        const bool valid = c < M;
        double v = 0.0;
        if (valid) {
            double feas = 0.0;
            for (int k = 0; k < a.C; ++k)
                feas += cons_feasible_term(cons_mu[(int64_t)k * ldc + c], cons_sigma[(int64_t)k * ldc + c], a.upper[k]);
            const double base = a.base == GPBO_CONS_BASE_NONE ? 0.0 : cons_base_term(a.base, mu[c], sigma[c], a.f_best, a.xi);
            v = base + feas;
            if (val_out) val_out[c] = v;
            if (feas_out) feas_out[c] = feas;
        }
        const bool is_nan = valid && (v != v);
        gpbo_count_nan(is_nan, lane, nan_count);
        if (valid && !is_nan && gpbo_better(v, idx_base + c, bv, bi)) {
            bv = v;
            bi = idx_base + c;
        }
    }
    gpbo_argmax_post(bv, bi, lane, wave, s_val, s_idx);
    gpbo_syncthreads();
    if (tid == 0) {
        gpbo_argmax_fold(s_val, s_idx, 4, bv, bi);
        part_val[blockIdx.x] = bv;
        part_idx[blockIdx.x] = bi;
    }
}

struct ConsLayout {   // the arg-max records of at most 1024 workgroups, then the NaN counter
    double *pval;
    int64_t *pidx;
    unsigned long long *nan;
    int64_t total;
    explicit ConsLayout(void *work) {
        Carver c(work);
        pval = c.take<double>(CONS_MAX_BLOCKS);
        pidx = c.take<int64_t>(CONS_MAX_BLOCKS);
        nan = c.take<unsigned long long>(32);   // 256 bytes
        total = c.total();
    }
};

}  // namespace

extern "C" int gpbo_constrained_acq_f64(const double *mu, const double *sigma, int64_t M, int32_t base, double f_best, double xi,
                                        const double *cons_mu, const double *cons_sigma, int64_t ldc, int32_t C,
                                        const double *upper_host, int64_t idx_offset, double *val_out, double *feas_out,
                                        gpbo_result *result, void *work, int64_t work_bytes, void *stream) {
    if (!cons_args_ok(mu, sigma, M, base, f_best, xi, cons_mu, cons_sigma, ldc, C, upper_host) || !result || !work)
        return GPBO_ERR_ARG;
    static_assert(GPBO_CONS_WORK_BYTES % 256 == 0, "the workspace is a whole number of 256-byte regions");
    if (!aligned_to(work, 256) || work_bytes < GPBO_CONS_WORK_BYTES || ConsLayout(nullptr).total > GPBO_CONS_WORK_BYTES)
        return GPBO_ERR_WORKSPACE;
    const ConsLayout L(work);
    hipStream_t st = gpbo_stream(stream);
    ConsArgs a;
    for (int k = 0; k < GPBO_CONS_MAX_C; ++k) a.upper[k] = k < C ? upper_host[k] : 0.0;
    const bool reads = base != GPBO_CONS_BASE_NONE;
    a.f_best = reads ? f_best : 0.0, a.xi = reads ? xi : 0.0, a.base = base, a.C = C;
    if (hipMemsetAsync(L.nan, 0, sizeof(unsigned long long), st) != hipSuccess) return GPBO_ERR_LAUNCH;
    const int64_t want = (M + 255) / 256;
    const int nblk = (int)(want > CONS_MAX_BLOCKS ? CONS_MAX_BLOCKS : want);
    hipLaunchKernelGGL(constrained_acq_kernel, dim3((unsigned)nblk), dim3(256), 0, st, mu, sigma, M, cons_mu, cons_sigma, ldc, a,
                       idx_offset, val_out, feas_out, L.pval, L.pidx, L.nan);
    GPBO_CHECK_LAUNCH();
    return gpbo_launch_argmax_finish(L.pval, L.pidx, nblk, L.nan, result, st);
}
