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
//     ConsScore    an instance of dense_acq_kernel (dense_acq.h: the candidate loop, the NaN count, the arg-max record, the
//                  launch).  A thread loads its candidate's 2 + 2 C values (consecutive threads, consecutive addresses in every
//                  array), the limits and scalars arrive by value in the kernel-argument record (uniform: scalar registers); the
//                  optional dense stores
// Edge rules (restated in tests/constrained_ref.py): a NaN in any input the call reads gives value NaN, counted once in nan_count
// and never chosen; sigma_c == 0 is certain either way (0 or -inf); sigma == 0: EI log(max(imp, 0)), PI 0 where imp > 0 else -inf;
// -inf is a legal value that beats the empty record, so an all -inf input returns its lowest index.
// No sum crosses candidates; the grid depends on M alone; only the integer NaN counter is atomic: two calls give the same bits.
#include "dense_acq.h"
#include "cons_math.h"

namespace {

// mu / sigma are read only when the base needs them, row k of cons_mu / cons_sigma only for k < C.
struct ConsScore {
    const double *__restrict__ mu, *__restrict__ sigma, *__restrict__ cons_mu, *__restrict__ cons_sigma;
    int64_t ldc;
    double *__restrict__ val_out, *__restrict__ feas_out;
    double upper[GPBO_CONS_MAX_C];
    double f_best, xi;
    int32_t base, C;
    __device__ __forceinline__ double operator()(int64_t c) const {
        double feas = 0.0;
        for (int k = 0; k < C; ++k) feas += cons_feasible_term(cons_mu[(int64_t)k * ldc + c], cons_sigma[(int64_t)k * ldc + c], upper[k]);
        const double b = base == GPBO_CONS_BASE_NONE ? 0.0 : cons_base_term(base, mu[c], sigma[c], f_best, xi);
        const double v = b + feas;
        if (val_out) val_out[c] = v;
        if (feas_out) feas_out[c] = feas;
        return v;
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
    if (!DenseAcqScratch::fits(work, work_bytes, GPBO_CONS_WORK_BYTES)) return GPBO_ERR_WORKSPACE;
    ConsScore sc;
    sc.mu = mu, sc.sigma = sigma, sc.cons_mu = cons_mu, sc.cons_sigma = cons_sigma, sc.ldc = ldc;
    sc.val_out = val_out, sc.feas_out = feas_out;
    for (int k = 0; k < GPBO_CONS_MAX_C; ++k) sc.upper[k] = k < C ? upper_host[k] : 0.0;
    const bool reads = base != GPBO_CONS_BASE_NONE;
    sc.f_best = reads ? f_best : 0.0, sc.xi = reads ? xi : 0.0, sc.base = base, sc.C = C;
    return dense_acq_launch(M, sc, idx_offset, DenseAcqScratch(work), result, gpbo_stream(stream));
}
