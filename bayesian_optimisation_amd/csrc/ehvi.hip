// Two-objective expected hypervolume improvement on the dense posteriors, in LOG space (Emmerich, Giannakoglou &
// Naujoks 2006, Emmerich, Yang, Deutz et al. 2016; not in the reference).  Both objectives are minimised, each a GP of its own,
// taken as independent: a candidate has (mu1, sigma1) and (mu2, sigma2).  The front holds P >= 0 points (a_i, c_i), i = 1..P,
// strictly ascending in objective 1 and strictly descending in objective 2, all strictly below the reference point r = (r1, r2);
// a_{P+1} = r1, c_0 = r2.  With g(a) = E[(a - f)+] per objective and G = log g (ehvi_math.h), the region below r is cut into
// vertical strips at the a_i, strip i with the ceiling c_i:
//     EHVI  = sum_{i = 0..P} [g1(a_{i+1}) - g1(a_i)] g2(c_i),       g1(a_0) := 0
//     value = logsumexp_{i = 0..P} (G1(a_{i+1}) + log(1 - exp(G1(a_i) - G1(a_{i+1}))) + G2(c_i))        (i = 0 first, no subtraction)
// The plain sum is exactly 0 wherever both objectives are a few dozen standard deviations from improving - every candidate then
// ties; the logarithm is finite there and keeps the order.  A function of dense (mu, sigma) arrays alone: no covariance entry,
// every kernel family, every model record.
//     EhviScore    an instance of dense_acq_kernel (dense_acq.h: the candidate loop, the NaN count, the arg-max record, the
//                  launch).  A thread loads its candidate's 4 values (consecutive threads, consecutive addresses in every
//                  array); the strip edges and ceilings arrive by value in the kernel-argument record (uniform, read with a
//                  uniform index: scalar loads into scalar registers, no LDS and no vector register per front point); G1 at an
//                  edge is evaluated once and carried to the next strip; the running-maximum logsumexp lives in two registers;
//                  the optional dense store
// Edge rules (restated in tests/ehvi_ref.py): a NaN in any of a candidate's four values gives value NaN, counted once in
// nan_count and never chosen; sigma == 0 uses max(level - mu, 0); -inf is a legal value that beats the empty record, so an
// all -inf input returns its lowest index; ties go to the lowest index.
// No sum crosses candidates; the grid depends on M alone; only the integer NaN counter is atomic: two calls give the same bits.
#include "dense_acq.h"
#include "ehvi_math.h"

namespace {

struct EhviScore {   // 2,112 bytes of the kernel-argument record
    const double *__restrict__ mu1, *__restrict__ sigma1, *__restrict__ mu2, *__restrict__ sigma2;
    double *__restrict__ val_out;
    double edge[GPBO_EHVI_MAX_P + 1];   // a_1 .. a_P, r1: the right edge of strip i
    double ceil[GPBO_EHVI_MAX_P + 1];   // r2, c_1 .. c_P: the ceiling of strip i
    int32_t P, pad;
    __device__ __forceinline__ double operator()(int64_t c) const {
        const double m1 = mu1[c], s1 = sigma1[c], m2 = mu2[c], s2 = sigma2[c];
        double v;
        if (m1 != m1 || s1 != s1 || m2 != m2 || s2 != s2) {
            v = __builtin_nan("");
        } else {
            const double ls1 = log(s1), ls2 = log(s2);
            EhviSum sum;
            double g1p = 0.0;
            for (int i = 0; i <= P; ++i) {
                const double g1n = ehvi_log_g(edge[i], m1, s1, ls1);
                sum.add(ehvi_strip(i == 0, g1p, g1n, ehvi_log_g(ceil[i], m2, s2, ls2)));
                g1p = g1n;
            }
            v = sum.value();
        }
        if (val_out) val_out[c] = v;
        return v;
    }
};

}  // namespace

extern "C" int gpbo_ehvi_acq_f64(const double *mu1, const double *sigma1, const double *mu2, const double *sigma2, int64_t M,
                                 const double *front_host, int32_t P, double ref1, double ref2, int64_t idx_offset, double *val_out,
                                 gpbo_result *result, void *work, int64_t work_bytes, void *stream) {
    if (!ehvi_args_ok(mu1, sigma1, mu2, sigma2, M, front_host, P, ref1, ref2) || !result || !work) return GPBO_ERR_ARG;
    static_assert(GPBO_EHVI_WORK_BYTES % 256 == 0, "the workspace is a whole number of 256-byte regions");
    if (!DenseAcqScratch::fits(work, work_bytes, GPBO_EHVI_WORK_BYTES)) return GPBO_ERR_WORKSPACE;
    EhviScore sc;
    sc.mu1 = mu1, sc.sigma1 = sigma1, sc.mu2 = mu2, sc.sigma2 = sigma2, sc.val_out = val_out;
    for (int i = 0; i <= GPBO_EHVI_MAX_P; ++i) {
        sc.edge[i] = i < P ? front_host[2 * i] : (i == P ? ref1 : 0.0);
        sc.ceil[i] = i == 0 ? ref2 : (i <= P ? front_host[2 * (i - 1) + 1] : 0.0);
    }
    sc.P = P, sc.pad = 0;
    return dense_acq_launch(M, sc, idx_offset, DenseAcqScratch(work), result, gpbo_stream(stream));
}
