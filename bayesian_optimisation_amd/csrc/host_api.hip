// Host-pointer entry points: one call = one SELECT_PARAMETERS surrogate step.
//
// The reference's boundary is a Python attribute protocol fed with NumPy arrays
// (the reference's select_parameters.py:146-158, 282-294 -> point_selector.py:42-102, 197-207).
// The functions of this file take exactly those arrays as plain host pointers, so a maintainer can bind the GPU path
// with ctypes + NumPy alone (no PyTorch, no device-memory handling on the caller's side): device buffers are
// allocated, filled, used and released inside the call, on the library's own stream.
//   gpbo_select_next_host_f64      = update_surrogate() after the length scales are chosen + the acquisition arg-max
//   gpbo_select_qei_host_f64       = the same step with q = 8 Monte-Carlo qEI as the acquisition
//   gpbo_select_batch_host_f64     = the same step, then q points for parallel evaluation (not in the reference; batch.hip)
//   gpbo_thompson_host_f64         = the factorisation, then q points as minimisers of posterior sample paths (thompson.hip)
//   gpbo_nei_host_f64              = the factorisation and its noise-free twin, then noisy expected improvement (nei.hip)
//   gpbo_mes_log_survival_host_f64 / gpbo_mes_acq_host_f64 = max-value entropy search on a dense posterior the caller holds (mes.hip)
//   gpbo_constrained_acq_host_f64  = constrained EI / PI / probability of feasibility on dense posteriors the caller holds (constrained.hip)
//   gpbo_ehvi_acq_host_f64         = two-objective expected hypervolume improvement on dense posteriors the caller holds (ehvi.hip)
//   gpbo_refine_host_f64           = the factorisation, then gradient refinement of given starts off the grid (refine.hip)
//   gpbo_nlml_grid_host_f64        = tune_kernel()'s likelihood grid (float32, the reference's det underflow)
//   gpbo_nlml_grid_logdet_host_f64 = the same grid in fp64 with log det from the factor
//   gpbo_nlml_grad_host_f64        = the likelihood and its gradient in the log length scales (ard="gradient")
//   gpbo_nlml_hyper_host_f64       = the likelihood over length scales, noise, signal variance and mean (ard="hyper"; hyper.hip)
//   gpbo_select_next_host_kern_f64 / gpbo_nlml_grad_host_kern_f64 / gpbo_nlml_hyper_host_kern_f64 = the same three with a
//                                    covariance family (GPBO_KERNEL_*): it rides in the Surrogate, which hands it to the factorisation
// Every factorising entry reads: own checks, own buffers, Surrogate (below), own calls, own read-backs.
#include "gpbo_internal.h"

#include <algorithm>
#include <vector>

namespace {

// Device allocations of one call, released on every exit path.
struct DeviceArena {
    std::vector<void *> ptrs;
    hipStream_t stream = nullptr;
    bool ok = true;
    DeviceArena() { ok = hipStreamCreateWithFlags(&stream, hipStreamNonBlocking) == hipSuccess; }
    ~DeviceArena() {
        if (stream) {
            (void)hipStreamSynchronize(stream);
            (void)hipStreamDestroy(stream);
        }
        for (void *p : ptrs) (void)hipFree(p);
    }
    template <typename T>
    T *alloc(int64_t count) {
        void *p = nullptr;
        if (count < 1) count = 1;
        if (hipMalloc(&p, sizeof(T) * (size_t)count) != hipSuccess) {
            ok = false;
            return nullptr;
        }
        ptrs.push_back(p);
        return reinterpret_cast<T *>(p);
    }
    bool h2d(void *dst, const void *src, size_t bytes) {
        return hipMemcpyAsync(dst, src, bytes, hipMemcpyHostToDevice, stream) == hipSuccess;
    }
    bool d2h(void *dst, const void *src, size_t bytes) {
        return hipMemcpyAsync(dst, src, bytes, hipMemcpyDeviceToHost, stream) == hipSuccess;
    }
    bool sync() { return hipStreamSynchronize(stream) == hipSuccess; }
    void *st() const { return reinterpret_cast<void *>(stream); }
};

// The factorised surrogate of one call: what every factorising entry opens with.  The sizes come first (they feed the entry's
// own refusals, made before the arena exists); then two steps, because gpbo_select_next_host_f64 re-points X / y between the
// upload and the factorisation.
struct Surrogate {
    const int64_t N, Np, wfact;   // observations, padded, the bytes the factorisation needs of `work`
    const int32_t d;
    const int32_t kernel;   // GPBO_KERNEL_*: the family of the factorised matrix
    double *X = nullptr, *y = nullptr, *K = nullptr, *U = nullptr, *alpha = nullptr;
    int32_t *info = nullptr;
    char *work = nullptr;   // the factorisation's workspace is dead once U and alpha exist: the entry's own calls reuse it
    Surrogate(int64_t N_, int32_t d_, int32_t kernel_ = GPBO_KERNEL_SE)
        : N(N_), Np(gpbo_padded_n(N_)), wfact(gpbo_factorise_workspace_bytes(Np)), d(d_), kernel(kernel_) {}
    int64_t work_bytes(int64_t own) const { return wfact > own ? wfact : own; }   // (the entry adds its own slack)
    // Step 1, after the entry's own allocations: the buffers, GPBO_ERR_WORKSPACE if ANY allocation of the call failed, and
    // only then the first copies of the call: X and y.
    int stage(DeviceArena &A, const double *hX, const double *hy, int64_t wbytes) {
        X = A.alloc<double>(N * d), y = A.alloc<double>(N);
        K = A.alloc<double>(Np * Np), U = A.alloc<double>(Np * Np), alpha = A.alloc<double>(Np);
        info = A.alloc<int32_t>(1);
        work = A.alloc<char>(wbytes);
        if (!A.ok) return GPBO_ERR_WORKSPACE;
        return A.h2d(X, hX, sizeof(double) * N * d) && A.h2d(y, hy, sizeof(double) * N) ? GPBO_OK : GPBO_ERR_LAUNCH;
    }
    // The factorisation, enqueued (gpbo_nlml_grad_host_f64 stops here: its kernel reads `info` on the device).
    int factorise(DeviceArena &A, const double *ls, double jitter1, double jitter2) {
        return gpbo_factorise_kern_f64(X, y, N, d, ls, kernel, jitter1, jitter2, Np, K, U, alpha, info, work, wfact, A.st());
    }
    // Step 2: the factorisation, its info word on the host, the stream idle.  *info_out != 0: not positive definite - the
    // entry fills its own outputs for that exit.
    int factorise_sync(DeviceArena &A, const double *ls, double jitter1, double jitter2, int32_t *info_out) {
        const int rc = factorise(A, ls, jitter1, jitter2);
        if (rc != GPBO_OK) return rc;
        return A.d2h(info_out, info, sizeof(int32_t)) && A.sync() ? GPBO_OK : GPBO_ERR_LAUNCH;
    }
};

// What the entries on dense posteriors the caller holds on the HOST open and close with (MES, the constrained acquisitions, EHVI;
// no factorisation), after their own refusals: the arena; every input as rows of M values, ld apart on the host and packed on the
// device; every output the caller asked for (dense values, the result record: whatever the device entry writes); the constant
// workspace.  The entry returns rc unless it is GPBO_OK, calls its device entry on in[] / out[] / work, and returns finish(status).
struct DenseCall : DeviceArena {
    struct In { const double *host; int64_t rows, ld; };
    struct Out { void *host; size_t bytes; };
    In ins[4] = {};   // (an unused slot is a null host pointer: no buffer, no copy)
    Out outs[3] = {};
    double *in[4] = {};
    void *out[3] = {};
    char *work = nullptr;
    int rc = GPBO_ERR_ARG;   // more inputs or outputs than slots
    DenseCall(int64_t M, std::initializer_list<In> il, std::initializer_list<Out> ol, int64_t work_bytes) {
        if (il.size() > 4 || ol.size() > 3) return;
        std::copy(il.begin(), il.end(), ins), std::copy(ol.begin(), ol.end(), outs);
        rc = open(M, work_bytes);
    }
    int open(int64_t M, int64_t work_bytes) {
        if (!ok) return GPBO_ERR_LAUNCH;
        for (int k = 0; k < 4; ++k) in[k] = ins[k].host && ins[k].rows > 0 ? alloc<double>(ins[k].rows * M) : nullptr;
        for (int k = 0; k < 3; ++k) out[k] = outs[k].host ? alloc<char>((int64_t)outs[k].bytes) : nullptr;
        work = alloc<char>(work_bytes);   // (hipMalloc: 256-byte aligned)
        if (!ok) return GPBO_ERR_WORKSPACE;   // if ANY allocation failed
        for (int k = 0; k < 4; ++k)
            for (int64_t r = 0; in[k] && r < ins[k].rows; ++r)
                if (!h2d(in[k] + r * M, ins[k].host + r * ins[k].ld, sizeof(double) * M)) return GPBO_ERR_LAUNCH;
        return GPBO_OK;
    }
    template <class T = double>
    T *o(int k) const { return static_cast<T *>(out[k]); }
    int finish(int status) {   // the read-backs and the wait
        if (status != GPBO_OK) return status;
        bool okc = true;
        for (int k = 0; k < 3; ++k)
            if (out[k]) okc = okc && d2h(outs[k].host, out[k], outs[k].bytes);
        return okc && sync() ? GPBO_OK : GPBO_ERR_LAUNCH;
    }
};

// diagonal of cov_pred as the reference rounds it
inline double prior_variance(double jitter1, double jitter2) { return (1.0 + jitter1) + jitter2; }

}  // namespace

extern "C" int gpbo_select_next_host_f64(const double *X, const double *y, int64_t N, int32_t d, const double *ls,
                                         double jitter1, double jitter2, const double *Xs, int64_t M, int32_t acq_kind,
                                         double p0, double p1, double diag_add, int64_t chunk, double *mu_out,
                                         double *sigma_out, double *acq_out, double *cov_meas_out, gpbo_result *result,
                                         int32_t *info) {
    return gpbo_select_next_host_kern_f64(X, y, N, d, ls, GPBO_KERNEL_SE, jitter1, jitter2, Xs, M, acq_kind, p0, p1, diag_add, chunk,
                                          mu_out, sigma_out, acq_out, cov_meas_out, result, info);
}

extern "C" int gpbo_select_next_host_kern_f64(const double *X, const double *y, int64_t N, int32_t d, const double *ls,
                                              int32_t kernel, double jitter1, double jitter2, const double *Xs, int64_t M,
                                              int32_t acq_kind, double p0, double p1, double diag_add, int64_t chunk,
                                              double *mu_out, double *sigma_out, double *acq_out, double *cov_meas_out,
                                              gpbo_result *result, int32_t *info) {
    if (!X || !y || !ls || !Xs || !result || !info) return GPBO_ERR_ARG;
    if (!kernel_ok(kernel, d, diag_add)) return GPBO_ERR_ARG;
    if (N < 1 || M < 1 || d < 1 || d > GPBO_MAX_D_ANY) return GPBO_ERR_ARG;
    if (!acq_kind_ok(acq_kind)) return GPBO_ERR_ARG;
    if (chunk == 0) chunk = (int64_t)1 << 17;
    if (!chunk_ok(chunk) || !length_scales_ok(ls, d)) return GPBO_ERR_ARG;
    chunk = clamp_chunk(chunk, M);
    Surrogate G(N, d, kernel);
    const int64_t Np = G.Np;
    const int64_t wpost = gpbo_posterior_workspace_bytes(Np, chunk, M);
    if (wpost < 0) return GPBO_ERR_ARG;

    DeviceArena A;
    if (!A.ok) return GPBO_ERR_LAUNCH;
    double *dXs = A.alloc<double>(M * d);
    gpbo_result *dres = A.alloc<gpbo_result>(1);
    const bool dense = mu_out || sigma_out || acq_out;
    double *dmu = dense ? A.alloc<double>(M) : nullptr;
    double *dsig = dense ? A.alloc<double>(M) : nullptr;
    double *dacq = dense ? A.alloc<double>(M) : nullptr;
    // A caller that asks for the next point only (no dense arrays) gets it by branch and bound on the exact prefix bound
    // (same point, same NaN count, the plain pass when the bound does not separate the candidates); the same
    // rule and the same prefix lengths as DeviceGP.score_bound.
    // (jitter: with K = k(X,X) + tau I the true variance is >= tau, so the plain pass's sqrt(|var|) never reflects a
    //  negative value unless its rounding error exceeds tau - the one case a prefix cannot bound; DeviceGP.BOUND_MIN_JITTER)
    // (squared exponential only: the bound builds its mean with the entries of kstar_mfma.hip; a Matern family takes the plain pass)
    const bool bound_route = kernel == GPBO_KERNEL_SE && !dense && diag_add == 0.0 && M >= 32768 && Np >= 1024 && d <= GPBO_MAX_D &&
                             (acq_kind == GPBO_ACQ_EI || p0 >= 0.0) && jitter1 + jitter2 >= 1e-6;
    const int64_t J1 = (Np / 16) / 128 * 128 < 128 ? 128 : (Np / 16) / 128 * 128, J2 = (8 * J1 <= Np) ? 4 * J1 : 0;
    // every first-level survivor may go on to the second-level bound (1/16 of a plain pass per candidate); the plain pass
    // takes over when more than M / 8 reach the fp64 kernels (rescore.hip)
    const int64_t bcap = M < 4096 ? 4096 : M;
    const int64_t bchunk = 1 << 14;
    const int64_t wresc = bound_route ? gpbo_rescore_workspace_bytes(Np, bcap, bchunk) : 0;
    if (wresc < 0) return GPBO_ERR_ARG;
    double *dub = bound_route ? A.alloc<double>(M) : nullptr;
    char *dresc = bound_route ? A.alloc<char>(wresc + 256) : nullptr;
    // the bound prunes by the FIRST J1 observations of the factorised problem: factorise the farthest-point order of the
    // observations (subset.hip), so that the pruning does not depend on the order in which they arrived.  cov_meas_out is
    // the reference's matrix in ARRIVAL order: a caller who wants it gets the arrival-order factorisation.
    const bool fps_order = bound_route && J1 < N && !cov_meas_out;
    const int64_t word = fps_order ? gpbo_fps_order_workspace_bytes(N) : 0;
    int64_t *dperm = fps_order ? A.alloc<int64_t>(N) : nullptr;
    double *dXp = fps_order ? A.alloc<double>(N * d) : nullptr;
    double *dyp = fps_order ? A.alloc<double>(N) : nullptr;
    char *dword = fps_order ? A.alloc<char>(word + 256) : nullptr;
    int rc = G.stage(A, X, y, G.work_bytes(wpost) + 256);
    if (rc != GPBO_OK) return rc;
    if (!A.h2d(dXs, Xs, sizeof(double) * M * d)) return GPBO_ERR_LAUNCH;
    if (fps_order) {
        char *wo = reinterpret_cast<char *>(((uintptr_t)dword + 255) & ~(uintptr_t)255);
        rc = gpbo_fps_order_f64(G.X, G.y, N, d, ls, J1, dperm, dXp, dyp, wo, word, A.st());
        if (rc != GPBO_OK) return rc;
        G.X = dXp;   // the factorisation and every later pass read the observations in this order
        G.y = dyp;
    }
    rc = G.factorise_sync(A, ls, jitter1, jitter2, info);
    if (rc != GPBO_OK) return rc;
    if (cov_meas_out) {  // the reference's cov_meas attribute (point_selector.py:79), N x N without the padding
        if (hipMemcpy2DAsync(cov_meas_out, sizeof(double) * N, G.K, sizeof(double) * Np, sizeof(double) * N, (size_t)N,
                             hipMemcpyDeviceToHost, A.stream) != hipSuccess)
            return GPBO_ERR_LAUNCH;
    }
    if (*info != 0) {  // not positive definite: nothing to score (the reference's inv() raises or returns garbage)
        if (fps_order && *info >= 1 && *info <= N) {   // report the failing observation by its ARRIVAL index, as documented
            int64_t row = 0;
            if (!A.d2h(&row, dperm + (*info - 1), sizeof(int64_t)) || !A.sync()) return GPBO_ERR_LAUNCH;
            *info = (int32_t)(row + 1);
        }
        *result = {0.0, -1, 0, 0};
        return A.sync() ? GPBO_OK : GPBO_ERR_LAUNCH;
    }
    const double prior_var = prior_variance(jitter1, jitter2);
    bool decided = false;
    if (bound_route) {
        rc = gpbo_posterior_prefix_f64(dXs, M, G.X, N, Np, d, ls, G.U, G.alpha, prior_var, acq_kind, p0, p1, 0, chunk, J1,
                                       nullptr, nullptr, dub, dres, G.work, wpost, nullptr, A.st());
        if (rc != GPBO_OK) return rc;
        gpbo_screen_stats stats;
        char *wr = reinterpret_cast<char *>(((uintptr_t)dresc + 255) & ~(uintptr_t)255);
        int64_t stride = M / 1024;
        if (stride < 1) stride = 1;
        rc = gpbo_bound_select_f64(dXs, M, dub, G.X, N, Np, d, ls, G.U, G.alpha, prior_var, acq_kind, p0, p1, 0, stride, bcap,
                                   bchunk, J2, dres, &stats, wr, wresc, A.st());
        if (rc != GPBO_OK) return rc;
        decided = !stats.fallback;
    }
    if (!decided) {
        rc = gpbo_posterior_acq_kern_f64(dXs, M, G.X, N, Np, d, ls, kernel, G.U, G.alpha, prior_var, acq_kind, p0, p1, diag_add, 0,
                                         chunk, dmu, dsig, dacq, dres, G.work, wpost, nullptr, A.st());
        if (rc != GPBO_OK) return rc;
    }
    bool okc = A.d2h(result, dres, sizeof(gpbo_result));
    if (mu_out) okc = okc && A.d2h(mu_out, dmu, sizeof(double) * M);
    if (sigma_out) okc = okc && A.d2h(sigma_out, dsig, sizeof(double) * M);
    if (acq_out) okc = okc && A.d2h(acq_out, dacq, sizeof(double) * M);
    return okc && A.sync() ? GPBO_OK : GPBO_ERR_LAUNCH;
}

// q = 8 Monte-Carlo qEI on host arrays (same conventions as gpbo_select_next_host_f64; Z: [S x 8] base samples)
extern "C" int gpbo_select_qei_host_f64(const double *X, const double *y, int64_t N, int32_t d, const double *ls,
                                        double jitter1, double jitter2, const double *Xs, int64_t M, double f_best,
                                        double xi, const double *Z, int32_t S, int64_t chunk, double *qei_out,
                                        gpbo_result *result, int32_t *info) {
    if (!X || !y || !ls || !Xs || !Z || !result || !info) return GPBO_ERR_ARG;
    if (N < 1 || M < 8 || M % 8 || d < 1 || d > GPBO_MAX_D || S < 1) return GPBO_ERR_ARG;
    if (chunk == 0) chunk = (int64_t)1 << 15;
    if (!chunk_ok(chunk) || !length_scales_ok(ls, d)) return GPBO_ERR_ARG;
    chunk = clamp_chunk(chunk, M);
    Surrogate G(N, d);
    const int64_t Np = G.Np;
    const int64_t wq = gpbo_qei_workspace_bytes(Np, chunk, M);
    if (wq < 0) return GPBO_ERR_ARG;

    DeviceArena A;
    if (!A.ok) return GPBO_ERR_LAUNCH;
    double *dXs = A.alloc<double>(M * d), *dZ = A.alloc<double>((int64_t)S * 8);
    gpbo_result *dres = A.alloc<gpbo_result>(1);
    double *dq = qei_out ? A.alloc<double>(M / 8) : nullptr;
    int rc = G.stage(A, X, y, G.work_bytes(wq) + 256);
    if (rc != GPBO_OK) return rc;
    if (!A.h2d(dXs, Xs, sizeof(double) * M * d) || !A.h2d(dZ, Z, sizeof(double) * S * 8)) return GPBO_ERR_LAUNCH;
    rc = G.factorise_sync(A, ls, jitter1, jitter2, info);
    if (rc != GPBO_OK) return rc;
    if (*info != 0) {  // not positive definite: nothing to score
        *result = {0.0, -1, 0, 0};
        return GPBO_OK;
    }
    rc = gpbo_posterior_qei_f64(dXs, M, G.X, N, Np, d, ls, G.U, G.alpha, prior_variance(jitter1, jitter2), f_best, xi, dZ, S, 0,
                                chunk, dq, dres, G.work, wq, nullptr, A.st());
    if (rc != GPBO_OK) return rc;
    bool okc = A.d2h(result, dres, sizeof(gpbo_result));
    if (qei_out) okc = okc && A.d2h(qei_out, dq, sizeof(double) * (M / 8));
    return okc && A.sync() ? GPBO_OK : GPBO_ERR_LAUNCH;
}

// Greedy q-point batch on host arrays: factorisation + the dense plain pass + gpbo_select_batch_f64 (csrc/batch.hip).
extern "C" int gpbo_select_batch_host_f64(const double *X, const double *y, int64_t N, int32_t d, const double *ls,
                                          double jitter1, double jitter2, const double *Xs, int64_t M, int32_t acq_kind,
                                          double p0, double p1, int64_t chunk, int32_t q, int32_t fantasy, double lie,
                                          int64_t *idx_out, double *val_out, double *mu_out, double *sigma_out,
                                          gpbo_result *result, int32_t *info) {
    if (!X || !y || !ls || !Xs || !idx_out || !val_out || !result || !info) return GPBO_ERR_ARG;
    if (N < 1 || M < 1 || d < 1 || d > GPBO_MAX_D || q < 1 || q > GPBO_BATCH_MAX_Q || q > M) return GPBO_ERR_ARG;
    if (!acq_kind_ok(acq_kind)) return GPBO_ERR_ARG;
    if (fantasy != GPBO_FANTASY_BELIEVER && fantasy != GPBO_FANTASY_LIE) return GPBO_ERR_ARG;
    if (fantasy == GPBO_FANTASY_LIE && !(lie - lie == 0.0)) return GPBO_ERR_ARG;   // not finite
    if (chunk == 0) chunk = (int64_t)1 << 17;
    if (!chunk_ok(chunk) || !length_scales_ok(ls, d)) return GPBO_ERR_ARG;
    chunk = clamp_chunk(chunk, M);
    Surrogate G(N, d);
    const int64_t Np = G.Np;
    const int64_t wpost = gpbo_posterior_workspace_bytes(Np, chunk, M);
    const int64_t wbatch = gpbo_batch_workspace_bytes(Np, M, q);
    if (wpost < 0 || wbatch < 0) return GPBO_ERR_ARG;

    DeviceArena A;
    if (!A.ok) return GPBO_ERR_LAUNCH;
    double *dXs = A.alloc<double>(M * d);
    gpbo_result *dres = A.alloc<gpbo_result>(1);
    char *dbatch = A.alloc<char>(wbatch);   // (hipMalloc: 256-byte aligned)
    double *dmu = A.alloc<double>(M), *dsig = A.alloc<double>(M), *dval = A.alloc<double>(q);
    int64_t *didx = A.alloc<int64_t>(q);
    int rc = G.stage(A, X, y, G.work_bytes(wpost) + 256);
    if (rc != GPBO_OK) return rc;
    if (!A.h2d(dXs, Xs, sizeof(double) * M * d)) return GPBO_ERR_LAUNCH;
    rc = G.factorise_sync(A, ls, jitter1, jitter2, info);
    if (rc != GPBO_OK) return rc;
    if (*info != 0) {  // not positive definite: nothing to select from
        *result = {0.0, -1, 0, 0};
        for (int32_t j = 0; j < q; ++j) idx_out[j] = -1;
        return GPBO_OK;
    }
    const double prior_var = prior_variance(jitter1, jitter2);
    rc = gpbo_posterior_acq_f64(dXs, M, G.X, N, Np, d, ls, G.U, G.alpha, prior_var, acq_kind, p0, p1, 0.0, 0, chunk, dmu, dsig,
                                nullptr, dres, G.work, wpost, nullptr, A.st());
    if (rc != GPBO_OK) return rc;
    rc = gpbo_select_batch_f64(dXs, M, G.X, N, Np, d, ls, G.U, G.alpha, jitter1, jitter2, prior_var, acq_kind, p0, p1, q, fantasy,
                               lie, dmu, dsig, 0, didx, dval, dres, G.info, dbatch, wbatch, A.st());
    if (rc != GPBO_OK) return rc;
    bool okc = A.d2h(result, dres, sizeof(gpbo_result)) && A.d2h(info, G.info, sizeof(int32_t)) &&
               A.d2h(idx_out, didx, sizeof(int64_t) * q) && A.d2h(val_out, dval, sizeof(double) * q);
    if (mu_out) okc = okc && A.d2h(mu_out, dmu, sizeof(double) * M);
    if (sigma_out) okc = okc && A.d2h(sigma_out, dsig, sizeof(double) * M);
    return okc && A.sync() ? GPBO_OK : GPBO_ERR_LAUNCH;
}

// Thompson sampling on host arrays: factorisation + gpbo_thompson_weights_f64 + gpbo_thompson_paths_f64 (csrc/thompson.hip).
extern "C" int gpbo_thompson_host_f64(const double *X, const double *y, int64_t N, int32_t d, const double *ls, double jitter1,
                                      double jitter2, const double *Xs, int64_t M, const double *omega, const double *phase,
                                      const double *W, const double *E, int32_t F, int32_t S, int64_t *idx_out,
                                      double *val_out, int64_t *nan_out, double *f_out, int32_t *info) {
    if (!X || !y || !ls || !Xs || !omega || !phase || !W || !E || !idx_out || !val_out || !nan_out || !info)
        return GPBO_ERR_ARG;
    if (N < 1 || M < 1 || d < 1 || d > GPBO_MAX_D || !length_scales_ok(ls, d)) return GPBO_ERR_ARG;
    if (!(jitter1 + jitter2 >= 0.0)) return GPBO_ERR_ARG;
    Surrogate G(N, d);
    const int64_t Np = G.Np;
    const int64_t wwts = gpbo_thompson_weights_workspace_bytes(Np, F, S);
    const int64_t wpaths = gpbo_thompson_paths_workspace_bytes(Np, M, F, S);
    if (wwts < 0 || wpaths < 0) return GPBO_ERR_ARG;   // F, S, M out of range

    DeviceArena A;
    if (!A.ok) return GPBO_ERR_LAUNCH;
    double *dXs = A.alloc<double>(M * d);
    double *dom = A.alloc<double>((int64_t)F * d), *dph = A.alloc<double>(F), *dW = A.alloc<double>((int64_t)S * F);
    double *dE = A.alloc<double>((int64_t)S * N), *dV = A.alloc<double>((int64_t)S * Np);
    int64_t *dout = A.alloc<int64_t>(3 * (int64_t)S);   // idx | val | nan
    double *df = f_out ? A.alloc<double>((int64_t)S * M) : nullptr;
    // one workspace serves the three calls in turn (hipMalloc: 256-byte aligned)
    int rc = G.stage(A, X, y, G.work_bytes(wwts > wpaths ? wwts : wpaths));
    if (rc != GPBO_OK) return rc;
    if (!A.h2d(dXs, Xs, sizeof(double) * M * d) || !A.h2d(dom, omega, sizeof(double) * F * d) ||
        !A.h2d(dph, phase, sizeof(double) * F) || !A.h2d(dW, W, sizeof(double) * S * F) ||
        !A.h2d(dE, E, sizeof(double) * S * N))
        return GPBO_ERR_LAUNCH;
    rc = G.factorise_sync(A, ls, jitter1, jitter2, info);
    if (rc != GPBO_OK) return rc;
    if (*info != 0) {  // not positive definite: no posterior to sample from
        for (int32_t s = 0; s < S; ++s) {
            idx_out[s] = -1;
            val_out[s] = __builtin_nan("");
            nan_out[s] = 0;
        }
        return GPBO_OK;
    }
    rc = gpbo_thompson_weights_f64(G.X, G.y, N, Np, d, ls, G.U, jitter1, jitter2, dom, dph, dW, dE, F, S, dV, G.work, wwts,
                                   A.st());
    if (rc != GPBO_OK) return rc;
    rc = gpbo_thompson_paths_f64(dXs, M, G.X, N, Np, d, ls, dom, dph, dW, dV, F, S, 0, df, M, dout,
                                 reinterpret_cast<double *>(dout + S), dout + 2 * (int64_t)S, G.work, wpaths, A.st());
    if (rc != GPBO_OK) return rc;
    bool okc = A.d2h(idx_out, dout, sizeof(int64_t) * S) && A.d2h(val_out, dout + S, sizeof(double) * S) &&
               A.d2h(nan_out, dout + 2 * (int64_t)S, sizeof(int64_t) * S);
    if (f_out) okc = okc && A.d2h(f_out, df, sizeof(double) * S * M);
    return okc && A.sync() ? GPBO_OK : GPBO_ERR_LAUNCH;
}

// Noisy expected improvement on host arrays: the factorisation, its noise-free twin (jitters (delta, 0)), gpbo_nei_fantasies_f64 and
// gpbo_posterior_nei_kern_f64 (csrc/nei.hip).
extern "C" int gpbo_nei_host_f64(const double *X, const double *y, int64_t N, int32_t d, const double *ls, int32_t kernel,
                                 double jitter1, double jitter2, double delta, const double *Xs, int64_t M, const double *Z,
                                 const double *E, int32_t S, double xi, int64_t chunk, const double *best_in, double *mu_out,
                                 double *sigma_out, double *acq_out, double *best_out, gpbo_result *result, int32_t *info) {
    if (!X || !y || !ls || !Xs || !Z || !E || !result || !info) return GPBO_ERR_ARG;
    if (N < 1 || M < 1 || d < 1 || d > GPBO_MAX_D || !kernel_ok(kernel, d) || !length_scales_ok(ls, d)) return GPBO_ERR_ARG;
    const double rho = jitter1 + jitter2;
    if (!(delta > 0.0) || !(delta <= rho) || !(rho < __builtin_huge_val()) || !(xi - xi == 0.0)) return GPBO_ERR_ARG;
    if (chunk == 0) chunk = (int64_t)1 << 17;
    if (!chunk_ok(chunk)) return GPBO_ERR_ARG;
    chunk = clamp_chunk(chunk, M);
    Surrogate G(N, d, kernel);
    const int64_t Np = G.Np;
    const int64_t wfan = gpbo_nei_fantasies_workspace_bytes(Np, S);
    const int64_t wnei = gpbo_posterior_nei_workspace_bytes(Np, chunk, M, S);
    if (wfan < 0 || wnei < 0) return GPBO_ERR_ARG;   // S, M out of range

    DeviceArena A;
    if (!A.ok) return GPBO_ERR_LAUNCH;
    double *dXs = A.alloc<double>(M * d);
    double *dZ = A.alloc<double>((int64_t)S * N), *dE = A.alloc<double>((int64_t)S * N);
    double *dA = A.alloc<double>((int64_t)S * Np), *dF = A.alloc<double>((int64_t)S * Np), *dbest = A.alloc<double>(S);
    double *dK0 = A.alloc<double>(Np * Np), *dU0 = A.alloc<double>(Np * Np), *dalpha0 = A.alloc<double>(Np);
    int32_t *dinfo0 = A.alloc<int32_t>(1);
    gpbo_result *dres = A.alloc<gpbo_result>(1);
    double *dmu = mu_out ? A.alloc<double>((int64_t)S * M) : nullptr;
    double *dsig = sigma_out ? A.alloc<double>(M) : nullptr;
    double *dacq = acq_out ? A.alloc<double>(M) : nullptr;
    // one workspace serves the four calls in turn (hipMalloc: 256-byte aligned)
    int rc = G.stage(A, X, y, G.work_bytes(wfan > wnei ? wfan : wnei));
    if (rc != GPBO_OK) return rc;
    if (!A.h2d(dXs, Xs, sizeof(double) * M * d) || !A.h2d(dZ, Z, sizeof(double) * S * N) || !A.h2d(dE, E, sizeof(double) * S * N))
        return GPBO_ERR_LAUNCH;
    rc = G.factorise(A, ls, jitter1, jitter2);
    if (rc != GPBO_OK) return rc;
    int32_t info0 = 0;
    rc = gpbo_factorise_kern_f64(G.X, G.y, N, d, ls, kernel, delta, 0.0, Np, dK0, dU0, dalpha0, dinfo0, G.work, G.wfact, A.st());
    if (rc != GPBO_OK) return rc;
    if (!A.d2h(info, G.info, sizeof(int32_t)) || !A.d2h(&info0, dinfo0, sizeof(int32_t)) || !A.sync()) return GPBO_ERR_LAUNCH;
    if (*info == 0) *info = info0;
    if (*info != 0) {  // not positive definite: nothing to sample from
        *result = {0.0, -1, 0, 0};
        return GPBO_OK;
    }
    rc = gpbo_nei_fantasies_f64(dK0, dU0, G.U, G.y, N, Np, dZ, dE, sqrt(rho - delta), S, dA, dF, dbest, G.work, wfan, A.st());
    if (rc != GPBO_OK) return rc;
    if (best_in && !A.h2d(dbest, best_in, sizeof(double) * S)) return GPBO_ERR_LAUNCH;
    rc = gpbo_posterior_nei_kern_f64(dXs, M, G.X, N, Np, d, ls, kernel, dU0, dA, dbest, S, 1.0 + delta, xi, 0, chunk, dmu, M, dsig,
                                     dacq, dres, G.work, wnei, A.st());
    if (rc != GPBO_OK) return rc;
    bool okc = A.d2h(result, dres, sizeof(gpbo_result));
    if (mu_out) okc = okc && A.d2h(mu_out, dmu, sizeof(double) * S * M);
    if (sigma_out) okc = okc && A.d2h(sigma_out, dsig, sizeof(double) * M);
    if (acq_out) okc = okc && A.d2h(acq_out, dacq, sizeof(double) * M);
    if (best_out) okc = okc && A.d2h(best_out, dbest, sizeof(double) * S);
    return okc && A.sync() ? GPBO_OK : GPBO_ERR_LAUNCH;
}

// Max-value entropy search on host arrays (csrc/mes.hip): the two calls work on a dense posterior (mu, sigma) the caller already
// holds (DenseCall, above).  The refusals are the device entries' own (mes_values_ok, host_driver.h), made before the arena exists.
extern "C" int gpbo_mes_log_survival_host_f64(const double *mu, const double *sigma, int64_t M, const double *z, int32_t Q,
                                              double *out, int64_t *nan_out) {
    if (!mu || !sigma || !z || !out || !nan_out || !mes_values_ok(M, z, Q, GPBO_MES_MAX_LEVELS)) return GPBO_ERR_ARG;
    DenseCall D(M, {{mu, 1, M}, {sigma, 1, M}}, {{out, sizeof(double) * Q}, {nan_out, sizeof(int64_t)}}, GPBO_MES_WORK_BYTES);
    if (D.rc != GPBO_OK) return D.rc;
    return D.finish(gpbo_mes_log_survival_f64(D.in[0], D.in[1], M, z, Q, D.o(0), D.o<int64_t>(1), D.work, GPBO_MES_WORK_BYTES,
                                              D.st()));
}

extern "C" int gpbo_mes_acq_host_f64(const double *mu, const double *sigma, int64_t M, const double *ystar, int32_t S,
                                     double *acq_out, gpbo_result *result) {
    if (!mu || !sigma || !ystar || !result || !mes_values_ok(M, ystar, S, GPBO_MES_MAX_S)) return GPBO_ERR_ARG;
    DenseCall D(M, {{mu, 1, M}, {sigma, 1, M}}, {{acq_out, sizeof(double) * M}, {result, sizeof(gpbo_result)}}, GPBO_MES_WORK_BYTES);
    if (D.rc != GPBO_OK) return D.rc;
    return D.finish(gpbo_mes_acq_f64(D.in[0], D.in[1], M, ystar, S, 0, D.o(0), D.o<gpbo_result>(1), D.work, GPBO_MES_WORK_BYTES,
                                     D.st()));
}

// The constrained acquisitions on host arrays (csrc/constrained.hip): the objective's dense posterior (read only with a base) and
// the C constraints' [C x ldc].  The refusals are the device entry's own (cons_args_ok, host_driver.h), made before the arena
// exists; the rows are uploaded without their padding (ldc = M on the device).
extern "C" int gpbo_constrained_acq_host_f64(const double *mu, const double *sigma, int64_t M, int32_t base, double f_best,
                                             double xi, const double *cons_mu, const double *cons_sigma, int64_t ldc, int32_t C,
                                             const double *upper, double *val_out, double *feas_out, gpbo_result *result) {
    if (!cons_args_ok(mu, sigma, M, base, f_best, xi, cons_mu, cons_sigma, ldc, C, upper) || !result) return GPBO_ERR_ARG;
    const int64_t own = base != GPBO_CONS_BASE_NONE;
    DenseCall D(M, {{mu, own, M}, {sigma, own, M}, {cons_mu, C, ldc}, {cons_sigma, C, ldc}},
                {{val_out, sizeof(double) * M}, {feas_out, sizeof(double) * M}, {result, sizeof(gpbo_result)}}, GPBO_CONS_WORK_BYTES);
    if (D.rc != GPBO_OK) return D.rc;
    return D.finish(gpbo_constrained_acq_f64(D.in[0], D.in[1], M, base, f_best, xi, D.in[2], D.in[3], M, C, upper, 0, D.o(0), D.o(1),
                                             D.o<gpbo_result>(2), D.work, GPBO_CONS_WORK_BYTES, D.st()));
}

// Two-objective expected hypervolume improvement on host arrays (csrc/ehvi.hip): the two objectives' dense posteriors.  The
// refusals are the device entry's own (ehvi_args_ok, host_driver.h), made before the arena exists.
extern "C" int gpbo_ehvi_acq_host_f64(const double *mu1, const double *sigma1, const double *mu2, const double *sigma2, int64_t M,
                                      const double *front, int32_t P, double ref1, double ref2, double *val_out,
                                      gpbo_result *result) {
    if (!ehvi_args_ok(mu1, sigma1, mu2, sigma2, M, front, P, ref1, ref2) || !result) return GPBO_ERR_ARG;
    DenseCall D(M, {{mu1, 1, M}, {sigma1, 1, M}, {mu2, 1, M}, {sigma2, 1, M}},
                {{val_out, sizeof(double) * M}, {result, sizeof(gpbo_result)}}, GPBO_EHVI_WORK_BYTES);
    if (D.rc != GPBO_OK) return D.rc;
    return D.finish(gpbo_ehvi_acq_f64(D.in[0], D.in[1], D.in[2], D.in[3], M, front, P, ref1, ref2, 0, D.o(0), D.o<gpbo_result>(1),
                                      D.work, GPBO_EHVI_WORK_BYTES, D.st()));
}

// Off-grid refinement on host arrays: factorisation + gpbo_refine_f64 (csrc/refine.hip).
extern "C" int gpbo_refine_host_f64(const double *X, const double *y, int64_t N, int32_t d, const double *ls, double jitter1,
                                    double jitter2, double *Xq, int64_t P, const double *lower, const double *upper,
                                    int32_t acq_kind, double p0, double p1, int32_t iters, double step0, double *acq_out,
                                    double *acq0_out, int32_t *accepted_out, double *pg_out, gpbo_result *result,
                                    int32_t *info) {
    if (!X || !y || !ls || !Xq || !lower || !upper || !result || !info) return GPBO_ERR_ARG;
    if (N < 1 || d < 1 || d > GPBO_MAX_D || P < 1 || P > GPBO_REFINE_MAX_P) return GPBO_ERR_ARG;
    if (!acq_kind_ok(acq_kind) || !length_scales_ok(ls, d)) return GPBO_ERR_ARG;
    if (iters < 0 || iters > 1000 || !(step0 > 0.0) || !(step0 - step0 == 0.0)) return GPBO_ERR_ARG;
    for (int k = 0; k < d; ++k)
        if (!(lower[k] - lower[k] == 0.0) || !(upper[k] - upper[k] == 0.0) || lower[k] > upper[k]) return GPBO_ERR_ARG;
    Surrogate G(N, d);
    const int64_t Np = G.Np;
    const int64_t wref = gpbo_refine_workspace_bytes(Np, P);
    if (wref < 0) return GPBO_ERR_ARG;

    DeviceArena A;
    if (!A.ok) return GPBO_ERR_LAUNCH;
    double *dXq = A.alloc<double>(P * d);
    gpbo_result *dres = A.alloc<gpbo_result>(1);
    double *dacq = A.alloc<double>(P), *dacq0 = A.alloc<double>(P), *dpg = A.alloc<double>(P);
    int32_t *dacc = A.alloc<int32_t>(P);
    int rc = G.stage(A, X, y, G.work_bytes(wref));   // (hipMalloc: 256-byte aligned)
    if (rc != GPBO_OK) return rc;
    if (!A.h2d(dXq, Xq, sizeof(double) * P * d)) return GPBO_ERR_LAUNCH;
    rc = G.factorise_sync(A, ls, jitter1, jitter2, info);
    if (rc != GPBO_OK) return rc;
    if (*info != 0) {  // not positive definite: nothing to refine on
        *result = {0.0, -1, 0, 0};
        return GPBO_OK;
    }
    rc = gpbo_refine_f64(dXq, P, lower, upper, G.X, N, Np, d, ls, G.U, G.alpha, prior_variance(jitter1, jitter2), acq_kind, p0,
                         p1, iters, step0, dacq, dacq0, dacc, dpg, dres, G.work, wref, A.st());
    if (rc != GPBO_OK) return rc;
    bool okc = A.d2h(result, dres, sizeof(gpbo_result)) && A.d2h(Xq, dXq, sizeof(double) * P * d);
    if (acq_out) okc = okc && A.d2h(acq_out, dacq, sizeof(double) * P);
    if (acq0_out) okc = okc && A.d2h(acq0_out, dacq0, sizeof(double) * P);
    if (accepted_out) okc = okc && A.d2h(accepted_out, dacc, sizeof(int32_t) * P);
    if (pg_out) okc = okc && A.d2h(pg_out, dpg, sizeof(double) * P);
    return okc && A.sync() ? GPBO_OK : GPBO_ERR_LAUNCH;
}

// mode 0: the reference's float32 likelihood; mode 1: fp64, log det from the factor (gpbo.h)
static int nlml_grid_host(const double *X, const double *y, int64_t N, int32_t d, const double *ls_cells, int64_t G,
                          double jitter, void *out, int mode) {
    if (!X || !y || !ls_cells || !out || N < 1 || d < 1 || d > GPBO_MAX_D || G < 1 || G > (1 << 30))
        return GPBO_ERR_ARG;
    for (int64_t e = 0; e < G * d; ++e)
        if (!(ls_cells[e] > 0.0)) return GPBO_ERR_ARG;
    DeviceArena A;
    if (!A.ok) return GPBO_ERR_LAUNCH;
    const size_t osz = mode ? sizeof(double) : sizeof(float);
    double *dX = A.alloc<double>(N * d), *dy = A.alloc<double>(N);
    char *dout = A.alloc<char>((int64_t)(G * osz));
    if (!A.ok) return GPBO_ERR_WORKSPACE;
    if (!A.h2d(dX, X, sizeof(double) * N * d) || !A.h2d(dy, y, sizeof(double) * N)) return GPBO_ERR_LAUNCH;
    int rc;
    double *dcells = A.alloc<double>(G * d);
    if (!A.ok) return GPBO_ERR_WORKSPACE;
    if (!A.h2d(dcells, ls_cells, sizeof(double) * G * d)) return GPBO_ERR_LAUNCH;
    if (N <= gpbo_nlml_grid_wave_max_n()) {   // the wave-per-cell kernel (the same switch as the tensor-resident binding)
        rc = mode ? gpbo_nlml_grid_wave_logdet_f64(dX, dy, N, d, dcells, G, jitter, reinterpret_cast<double *>(dout), A.st())
                  : gpbo_nlml_grid_wave_f64(dX, dy, N, d, dcells, G, jitter, reinterpret_cast<float *>(dout), A.st());
        if (rc != GPBO_OK) return rc;
    } else {         // one persistent workgroup per cell, the whole factorisation in one launch
        const int64_t wb = gpbo_nlml_grid_batched_workspace_bytes(N, G);
        if (wb < 0) return GPBO_ERR_ARG;
        char *dwork = A.alloc<char>(wb);
        if (!A.ok) return GPBO_ERR_WORKSPACE;
        rc = mode ? gpbo_nlml_grid_batched_logdet_f64(dX, dy, N, d, dcells, G, jitter, reinterpret_cast<double *>(dout), dwork, wb, A.st())
                  : gpbo_nlml_grid_batched_f64(dX, dy, N, d, dcells, G, jitter, reinterpret_cast<float *>(dout), dwork, wb, A.st());
        if (rc != GPBO_OK) return rc;
    }
    return A.d2h(out, dout, G * osz) && A.sync() ? GPBO_OK : GPBO_ERR_LAUNCH;
}

extern "C" int gpbo_nlml_grid_host_f64(const double *X, const double *y, int64_t N, int32_t d, const double *ls_cells,
                                       int64_t G, double jitter, float *out) {
    return nlml_grid_host(X, y, N, d, ls_cells, G, jitter, out, 0);
}

extern "C" int gpbo_nlml_grid_logdet_host_f64(const double *X, const double *y, int64_t N, int32_t d,
                                              const double *ls_cells, int64_t G, double jitter, double *out) {
    return nlml_grid_host(X, y, N, d, ls_cells, G, jitter, out, 1);
}

extern "C" int gpbo_nlml_grad_host_f64(const double *X, const double *y, int64_t N, int32_t d, const double *ls,
                                       double jitter, double *out) {
    return gpbo_nlml_grad_host_kern_f64(X, y, N, d, ls, GPBO_KERNEL_SE, jitter, out);
}

extern "C" int gpbo_nlml_grad_host_kern_f64(const double *X, const double *y, int64_t N, int32_t d, const double *ls,
                                            int32_t kernel, double jitter, double *out) {
    if (!X || !y || !ls || !out || !kernel_ok(kernel, d)) return GPBO_ERR_ARG;
    if (N < 1 || d < 1 || d > GPBO_MAX_D || !length_scales_ok(ls, d)) return GPBO_ERR_ARG;
    Surrogate G(N, d, kernel);
    const int64_t wgrad = gpbo_nlml_grad_workspace_bytes(G.Np, d);
    if (wgrad < 0) return GPBO_ERR_ARG;

    DeviceArena A;
    if (!A.ok) return GPBO_ERR_LAUNCH;
    double *dout = A.alloc<double>(1 + d);
    char *dwg = A.alloc<char>(wgrad);   // (the gradient has a workspace of its own)
    int rc = G.stage(A, X, y, G.wfact);
    if (rc != GPBO_OK) return rc;
    rc = G.factorise(A, ls, jitter, 0.0);   // info stays on the device: the gradient kernel answers NaN for it
    if (rc != GPBO_OK) return rc;
    rc = gpbo_nlml_grad_kern_f64(G.U, G.alpha, G.y, G.X, N, G.Np, d, ls, kernel, G.info, dout, dwg, wgrad, A.st());
    if (rc != GPBO_OK) return rc;
    return A.d2h(out, dout, sizeof(double) * (1 + d)) && A.sync() ? GPBO_OK : GPBO_ERR_LAUNCH;
}

extern "C" int gpbo_nlml_hyper_host_f64(const double *X, const double *y, int64_t N, int32_t d, const double *ls, double noise,
                                        int32_t flags, double *out) {
    return gpbo_nlml_hyper_host_kern_f64(X, y, N, d, ls, GPBO_KERNEL_SE, noise, flags, out);
}

extern "C" int gpbo_nlml_hyper_host_kern_f64(const double *X, const double *y, int64_t N, int32_t d, const double *ls,
                                             int32_t kernel, double noise, int32_t flags, double *out) {
    if (!X || !y || !ls || !out || !kernel_ok(kernel, d)) return GPBO_ERR_ARG;
    if (N < 1 || d < 1 || d > GPBO_MAX_D || !length_scales_ok(ls, d)) return GPBO_ERR_ARG;
    if (!(noise > 0.0 && noise < __builtin_huge_val()) || (flags & ~(GPBO_HYPER_MEAN | GPBO_HYPER_SCALE))) return GPBO_ERR_ARG;
    Surrogate G(N, d, kernel);
    const int64_t whyp = gpbo_nlml_hyper_workspace_bytes(G.Np, d);
    if (whyp < 0) return GPBO_ERR_ARG;

    DeviceArena A;
    if (!A.ok) return GPBO_ERR_LAUNCH;
    double *dout = A.alloc<double>(4 + d);
    char *dwh = A.alloc<char>(whyp);   // (a workspace of its own, as the gradient's; hipMalloc: 256-byte aligned)
    int rc = G.stage(A, X, y, G.wfact);
    if (rc != GPBO_OK) return rc;
    rc = G.factorise(A, ls, noise, 0.0);   // info stays on the device: the finish kernel answers NaN for it
    if (rc != GPBO_OK) return rc;
    rc = gpbo_nlml_hyper_kern_f64(G.U, G.alpha, G.y, G.X, N, G.Np, d, ls, kernel, noise, flags, G.info, dout, nullptr, dwh, whyp,
                                  A.st());
    if (rc != GPBO_OK) return rc;
    return A.d2h(out, dout, sizeof(double) * (4 + d)) && A.sync() ? GPBO_OK : GPBO_ERR_LAUNCH;
}
