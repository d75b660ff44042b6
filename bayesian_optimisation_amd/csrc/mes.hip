// Max-value entropy search on the dense posterior (Wang & Jegelka 2017; not in the reference, which has the lower
// confidence bound only: its point_selector.py:197-207).  For minimisation, with m* the minimum of the latent function over the
// candidates and gamma_s(x) = (mu(x) - m*_s) / sigma(x) for S sampled minima:
//     MES(x) = (1 / S) sum_s h(gamma_s),   h(gamma) = gamma phi(gamma) / (2 Phi(gamma)) - log Phi(gamma) >= 0     (mes_math.h)
// No trade-off parameter, invariant under y -> a + b y, and a function of (mu, sigma) alone: both kernels read the dense posterior
// a scoring pass has left on the device and build no covariance entry - every kernel family and every model record.
//
// gpbo_mes_log_survival_f64 serves the sampling of m* (the Gumbel route of the paper; the fit itself is host arithmetic on three
// numbers, bayesian_optimisation_amd/mes.py): under an independence approximation
//     log S(z) = log Pr[m* > z] = sum_c log Phi((mu_c - z) / sigma_c)
// at Q <= 64 levels z in ONE pass over the candidates:
//     mes_log_survival_kernel   dense_acq_blocks(M) workgroups of 256 threads, grid-striding; a thread loads (mu_c, sigma_c)
//                               once and adds its term to one fp64 accumulator PER LEVEL, all in registers; the levels arrive by
//                               value in the kernel-argument record (uniform: scalar registers)
//     mes_survival_finish_kernel  adds the workgroups' partial sums in index order and publishes the NaN count
// gpbo_mes_acq_f64:
//     MesScore                  an instance of dense_acq_kernel (dense_acq.h: the candidate loop, the NaN count, the arg-max
//                               record, the launch): per candidate the S terms in index order, divided by S, the optional dense
//                               store; the sampled minima arrive by value in the kernel-argument record (uniform: scalar registers)
// Edge rules (restated in tests/mes_ref.py):
//     mu or sigma NaN   log S: the candidate is skipped and counted.  Acquisition: NaN, counted once in nan_count, never chosen.
//     sigma == 0        log S: the term is 0 where mu > z and -inf otherwise.  Acquisition: 0 (nothing to learn there).
// Sums run in a fixed order - a thread's candidates ascending, the xor butterfly inside a wave, the four waves in wave order, the
// workgroups in index order - and the grid depends on M alone: two calls give the same bits.  No floating-point atomics; only the
// integer NaN counter is atomic (gpbo_count_nan).
#include "dense_acq.h"
#include "mes_math.h"

namespace {

struct MesLevels {
    double z[GPBO_MES_MAX_LEVELS];
};

// One candidate's term of log S(z).  NOT inlined: the level loop of mes_log_survival_kernel is unrolled (its accumulators are
// registers), and 64 inlined copies of erfc / erfcx / log / log1p were 312 KB of code - the compiler then declined to unroll and
// put the accumulators in scratch.  As a call the kernel of 64 levels is 22 KB, holds 169 registers and needs no scratch (the
// register allocation crosses the call: the accumulators stay where the callee does not write).
__device__ __attribute__((noinline)) double mes_survival_term(double mu, double sigma, double z) {
    if (sigma == 0.0) return mu > z ? 0.0 : -__builtin_huge_val();
    return mes_log_ndtr((mu - z) / sigma);
}

// part[blockIdx.x * Q + q] = sum over this workgroup's candidates of log Phi((mu_c - z_q) / sigma_c), q < Q <= QCAP = 64.
// ONE instance: instances with 8 and 32 accumulators (67 / 103 registers against 169) were measured at 0.88 and 1.11 x 10^11 terms
// per second against 1.05 here - the kernel is bound by fp64 issue at every occupancy, fewer accumulators buy nothing.
// grid dense_acq_blocks(M), block 256.  Every trip of the candidate loop is taken by the whole workgroup (gpbo_count_nan
// is a wave-wide ballot), the tail masked by `valid`.
__global__ __launch_bounds__(256) void mes_log_survival_kernel(const double *__restrict__ mu, const double *__restrict__ sigma,
                                                               int64_t M, MesLevels lv, int Q, double *__restrict__ part,
                                                               unsigned long long *__restrict__ nan_count) {
    constexpr int QCAP = GPBO_MES_MAX_LEVELS;
    __shared__ double s_part[4][QCAP];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    double acc[QCAP];
#pragma unroll
    for (int q = 0; q < QCAP; ++q) acc[q] = 0.0;
    for (int64_t b = (int64_t)blockIdx.x * 256; b < M; b += (int64_t)gridDim.x * 256) {
        const int64_t c = b + tid;
        const bool valid = c < M;
        const double m = valid ? mu[c] : 0.0;
        const double s = valid ? sigma[c] : 1.0;
        const bool is_nan = valid && (m != m || s != s);
        gpbo_count_nan(is_nan, lane, nan_count);
        if (valid && !is_nan) {
#pragma unroll
            for (int q = 0; q < QCAP; ++q)
                if (q < Q) acc[q] += mes_survival_term(m, s, lv.z[q]);
        }
    }
#pragma unroll
    for (int q = 0; q < QCAP; ++q) {
        double a = acc[q];
#pragma unroll
        for (int off = 1; off < 64; off <<= 1) a += __shfl_xor(a, off);
        if (lane == 0) s_part[wave][q] = a;
    }
    gpbo_syncthreads();
    if (tid < Q) part[(int64_t)blockIdx.x * Q + tid] = ((s_part[0][tid] + s_part[1][tid]) + s_part[2][tid]) + s_part[3][tid];
}

// out[q] = sum over the workgroups, in index order, of part[w * Q + q]; nan_out = the NaN count.  grid 1, block 64.
__global__ __launch_bounds__(64) void mes_survival_finish_kernel(const double *__restrict__ part, int nblk, int Q,
                                                                 const unsigned long long *__restrict__ nan_count,
                                                                 double *__restrict__ out, int64_t *__restrict__ nan_out) {
    const int q = threadIdx.x;
    if (q < Q) {
        double a = 0.0;
#pragma unroll 8
        for (int w = 0; w < nblk; ++w) a += part[(int64_t)w * Q + q];
        out[q] = a;
    }
    if (q == 0) nan_out[0] = (int64_t)nan_count[0];
}

// MES of one candidate over dense mu / sigma.
struct MesScore {
    const double *__restrict__ mu, *__restrict__ sigma;
    double *__restrict__ acq_out;
    double y[GPBO_MES_MAX_S];
    int32_t S, pad;
    __device__ __forceinline__ double operator()(int64_t c) const {
        const double m = mu[c], sg = sigma[c];
        double a = 0.0;
        if (m != m || sg != sg) {
            a = __builtin_nan("");
        } else if (sg != 0.0) {
            double sum = 0.0;
            for (int s = 0; s < S; ++s) sum += mes_term((m - y[s]) / sg);
            a = sum / (double)S;
        }
        if (acq_out) acq_out[c] = a;
        return a;
    }
};

struct MesLayout {   // the partial sums of at most DENSE_ACQ_MAX_BLOCKS workgroups x 64 levels, then the arg-max scratch
    Carver carve;
    double *part;
    DenseAcqScratch acq;
    explicit MesLayout(void *work)
        : carve(work), part(carve.take<double>((int64_t)DENSE_ACQ_MAX_BLOCKS * GPBO_MES_MAX_LEVELS)), acq(carve) {}
};

int mes_workspace(const void *work, int64_t work_bytes) {
    static_assert(GPBO_MES_WORK_BYTES % 256 == 0, "the workspace is a whole number of 256-byte regions");
    if (!aligned_to(work, 256) || work_bytes < GPBO_MES_WORK_BYTES) return GPBO_ERR_WORKSPACE;
    return MesLayout(nullptr).carve.total() <= GPBO_MES_WORK_BYTES ? GPBO_OK : GPBO_ERR_WORKSPACE;
}

}  // namespace

extern "C" int gpbo_mes_log_survival_f64(const double *mu, const double *sigma, int64_t M, const double *z_host, int32_t Q,
                                         double *out, int64_t *nan_out, void *work, int64_t work_bytes, void *stream) {
    if (!mu || !sigma || !z_host || !out || !nan_out || !work) return GPBO_ERR_ARG;
    if (!mes_values_ok(M, z_host, Q, GPBO_MES_MAX_LEVELS)) return GPBO_ERR_ARG;
    const int rc = mes_workspace(work, work_bytes);
    if (rc != GPBO_OK) return rc;
    const MesLayout L(work);
    hipStream_t st = gpbo_stream(stream);
    MesLevels lv;
    for (int q = 0; q < GPBO_MES_MAX_LEVELS; ++q) lv.z[q] = q < Q ? z_host[q] : 0.0;
    if (hipMemsetAsync(L.acq.nan, 0, sizeof(unsigned long long), st) != hipSuccess) return GPBO_ERR_LAUNCH;
    const int nblk = dense_acq_blocks(M);
    hipLaunchKernelGGL(mes_log_survival_kernel, dim3((unsigned)nblk), dim3(256), 0, st, mu, sigma, M, lv, (int)Q, L.part, L.acq.nan);
    GPBO_CHECK_LAUNCH();
    hipLaunchKernelGGL(mes_survival_finish_kernel, dim3(1), dim3(64), 0, st, L.part, nblk, (int)Q, L.acq.nan, out, nan_out);
    GPBO_CHECK_LAUNCH();
    return GPBO_OK;
}

extern "C" int gpbo_mes_acq_f64(const double *mu, const double *sigma, int64_t M, const double *ystar_host, int32_t S,
                                int64_t idx_offset, double *acq_out, gpbo_result *result, void *work, int64_t work_bytes,
                                void *stream) {
    if (!mu || !sigma || !ystar_host || !result || !work) return GPBO_ERR_ARG;
    if (!mes_values_ok(M, ystar_host, S, GPBO_MES_MAX_S)) return GPBO_ERR_ARG;
    const int rc = mes_workspace(work, work_bytes);
    if (rc != GPBO_OK) return rc;
    MesScore sc;
    sc.mu = mu, sc.sigma = sigma, sc.acq_out = acq_out;
    for (int s = 0; s < GPBO_MES_MAX_S; ++s) sc.y[s] = s < S ? ystar_host[s] : 0.0;
    sc.S = S, sc.pad = 0;
    return dense_acq_launch(M, sc, idx_offset, MesLayout(work).acq, result, gpbo_stream(stream));
}
