// One candidate loop and one launch for every acquisition that is a function of dense posterior arrays already on the device
// (DESIGN.md 4q): EI / LCB on (mu, sigma) (sigma_acq.hip), max-value entropy search (mes.hip), the constrained acquisitions
// (constrained.hip), two-objective expected hypervolume improvement (ehvi.hip).  An acquisition is a Score: a struct with
//     __device__ __forceinline__ double operator()(int64_t c) const
// that returns candidate c's value and makes its own optional dense stores.  It is called for c < M only, and it travels BY VALUE
// in the kernel-argument record with everything it needs - array pointers, uniform tables, scalars: what it reads with a uniform
// index is a scalar load into scalar registers, no LDS and no vector register per entry.  Everything else is written once here:
//     dense_acq_kernel   min(ceil(M / 256), DENSE_ACQ_MAX_BLOCKS) workgroups of 256 threads, grid-striding (consecutive threads,
//                        consecutive candidates); a NaN value is counted (one atomicAdd per wave that has any) and never chosen;
//                        the workgroup's arg-max record, ties to the lower index, gpbo_none where it has no candidate
//     DenseAcqScratch    the records of the workgroups and the NaN counter, carved from the caller's workspace
//     dense_acq_launch   counter reset, launch, gpbo_launch_argmax_finish (sigma_acq.hip): the gpbo_result record
// No sum crosses candidates, the grid depends on M alone, only the integer NaN counter is atomic: two calls give the same bits.
#pragma once
#include "gpbo_internal.h"

constexpr int DENSE_ACQ_MAX_BLOCKS = 1024;

inline int dense_acq_blocks(int64_t M) {
    const int64_t want = (M + 255) / 256;
    return (int)(want > DENSE_ACQ_MAX_BLOCKS ? DENSE_ACQ_MAX_BLOCKS : want);
}

// grid dense_acq_blocks(M), block 256.  Every trip of the candidate loop is taken by the whole workgroup (gpbo_count_nan is a
// wave-wide ballot), the tail masked by `valid`.
template <class Score>
__global__ __launch_bounds__(256) void dense_acq_kernel(int64_t M, Score sc, int64_t idx_base, double *__restrict__ part_val,
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
        if (valid) v = sc(c);
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

struct DenseAcqScratch {   // 16,640 bytes: the arg-max records of at most DENSE_ACQ_MAX_BLOCKS workgroups, then the NaN counter
    double *pval;
    int64_t *pidx;
    unsigned long long *nan;
    explicit DenseAcqScratch(Carver &c)
        : pval(c.take<double>(DENSE_ACQ_MAX_BLOCKS)), pidx(c.take<int64_t>(DENSE_ACQ_MAX_BLOCKS)),
          nan(c.take<unsigned long long>(32)) {}   // 256 bytes
    explicit DenseAcqScratch(void *work) {   // ... from the start of `work`
        Carver c(work);
        *this = DenseAcqScratch(c);
    }
    static int64_t bytes() {
        Carver c(nullptr);
        const DenseAcqScratch s(c);
        return c.total();
    }
    // the scratch as the whole of a workspace of the constant size `fixed` (a multiple of 256 that holds it)
    static bool fits(const void *work, int64_t work_bytes, int64_t fixed) {
        return aligned_to(work, 256) && work_bytes >= fixed && bytes() <= fixed;
    }
};

// enqueue only: result holds the first arg-max of sc over the M candidates (index + idx_offset) and the NaN count
template <class Score>
int dense_acq_launch(int64_t M, const Score &sc, int64_t idx_offset, const DenseAcqScratch &L, gpbo_result *result,
                     hipStream_t st) {
    if (hipMemsetAsync(L.nan, 0, sizeof(unsigned long long), st) != hipSuccess) return GPBO_ERR_LAUNCH;
    const int nblk = dense_acq_blocks(M);
    hipLaunchKernelGGL(dense_acq_kernel<Score>, dim3((unsigned)nblk), dim3(256), 0, st, M, sc, idx_offset, L.pval, L.pidx, L.nan);
    GPBO_CHECK_LAUNCH();
    return gpbo_launch_argmax_finish(L.pval, L.pidx, nblk, L.nan, result, st);
}
