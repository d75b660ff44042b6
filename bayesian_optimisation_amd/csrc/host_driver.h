// Host-side plumbing shared by the scoring drivers (sigma_acq.hip, posterior_f32.hip, ozaki.hip, rescore.hip, host_api.hip)
// and the launchers below them: size arithmetic, the workspace carver, the argument refusals, environment switches, the
// profile-slot bookkeeping, the dense outputs of a chunk, the model / acquisition views, the length-scale scalings, the
// dispatch over d.
// Host only: no device code in this file.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stdlib.h>

#include "../../include/gpbo.h"

#pragma GCC visibility push(hidden)   // nothing here is part of the library's interface

// ---- sizes -------------------------------------------------------------------------------------------------------------
inline int64_t align_up(int64_t v, int64_t a) { return (v + a - 1) / a * a; }
inline int64_t round_up_granule(int64_t M) { return align_up(M, GPBO_CHUNK_GRANULE); }
// no more chunk than M candidates need
inline int64_t clamp_chunk(int64_t chunk, int64_t M) {
    const int64_t need = round_up_granule(M);
    return chunk > need ? need : chunk;
}

// ---- a workspace as consecutive 256-byte aligned regions.  Every layout is a struct of typed pointers that ONE function carves
// in region order: with a null base it only counts (the *_workspace_bytes query returns total()), with `work` it hands out the
// pointers the kernels get, so the type and count of the size pass are those of the pointer.
class Carver {
    char *base_;
    int64_t off_ = 0;

public:
    explicit Carver(void *base) : base_(static_cast<char *>(base)) {}
    void *take_bytes(int64_t n) {   // a nested workspace or an opaque region
        void *p = base_ ? base_ + off_ : nullptr;
        off_ += align_up(n, 256);
        return p;
    }
    template <class T>
    T *take(int64_t count) { return static_cast<T *>(take_bytes((int64_t)sizeof(T) * count)); }
    int64_t total() const { return off_; }
};

// ---- refusals (each entry point keeps its own order of checks: GPBO_ERR_ARG before GPBO_ERR_WORKSPACE before any HIP call)
inline bool chunk_ok(int64_t chunk) {
    return chunk >= GPBO_CHUNK_GRANULE && chunk % GPBO_CHUNK_GRANULE == 0 && chunk <= GPBO_CHUNK_MAX;
}
inline bool acq_kind_ok(int32_t kind) { return kind == GPBO_ACQ_LCB || kind == GPBO_ACQ_EI; }
// a covariance family (GPBO_KERNEL_*) and what goes with it: the Matern kernels exist for the unrolled feature counts only and
// never carry the N == M diagonal quirk (a shape coincidence of the reference's kernel_rbf)
inline bool kernel_ok(int32_t kernel, int32_t d, double diag_add = 0.0) {
    if (kernel == GPBO_KERNEL_SE) return true;
    if (kernel != GPBO_KERNEL_MATERN32 && kernel != GPBO_KERNEL_MATERN52) return false;
    return d <= GPBO_MAX_D && diag_add == 0.0;
}
inline bool np_ok(int64_t Np) { return Np >= GPBO_NPAD && Np % GPBO_NPAD == 0; }   // a padded size of the fp64 / int8 routes
inline bool aligned_to(const void *p, uintptr_t a) { return ((uintptr_t)p & (a - 1)) == 0; }
inline bool length_scales_ok(const double *ls, int d) {
    for (int k = 0; k < d; ++k)
        if (!(ls[k] > 0.0)) return false;
    return true;
}

// max-value entropy search (mes.hip and its host entries in host_api.hip): 1 <= M <= 2^40 candidates and 1 <= n <= n_max values
// that travel by value (levels or sampled minima), each finite
inline bool mes_values_ok(int64_t M, const double *v_host, int32_t n, int32_t n_max) {
    if (M < 1 || M > ((int64_t)1 << 40) || n < 1 || n > n_max) return false;
    for (int32_t i = 0; i < n; ++i)
        if (!(v_host[i] - v_host[i] == 0.0)) return false;
    return true;
}

// the constrained acquisitions (constrained.hip and its host entry in host_api.hip): 1 <= M <= 2^40 candidates, one of the three
// bases, 0 <= C <= GPBO_CONS_MAX_C constraints (at least one when there is no base) in rows of ldc >= M values, finite limits, a
// finite f_best and xi where the base reads them; mu / sigma may be null only without a base, cons_* / upper only with C == 0
inline bool cons_args_ok(const double *mu, const double *sigma, int64_t M, int32_t base, double f_best, double xi,
                         const double *cons_mu, const double *cons_sigma, int64_t ldc, int32_t C, const double *upper_host) {
    if (M < 1 || M > ((int64_t)1 << 40) || ldc < M || C < 0 || C > GPBO_CONS_MAX_C) return false;
    if (base != GPBO_CONS_BASE_NONE && base != GPBO_CONS_BASE_EI && base != GPBO_CONS_BASE_PI) return false;
    if (base == GPBO_CONS_BASE_NONE ? C == 0 : (!mu || !sigma || !(f_best - f_best == 0.0) || !(xi - xi == 0.0))) return false;
    if (C > 0 && (!cons_mu || !cons_sigma || !upper_host)) return false;
    for (int32_t c = 0; c < C; ++c)
        if (!(upper_host[c] - upper_host[c] == 0.0)) return false;
    return true;
}

// two-objective expected hypervolume improvement (ehvi.hip and its host entry in host_api.hip): 1 <= M <= 2^40 candidates, a
// finite reference point, 0 <= P <= GPBO_EHVI_MAX_P front points (a_i, c_i) in rows of front_host [P x 2] - every value finite,
// a strictly ascending, c strictly descending, every point strictly below the reference point; front_host may be null only with
// P == 0
inline bool ehvi_args_ok(const double *mu1, const double *sigma1, const double *mu2, const double *sigma2, int64_t M,
                         const double *front_host, int32_t P, double ref1, double ref2) {
    if (M < 1 || M > ((int64_t)1 << 40) || P < 0 || P > GPBO_EHVI_MAX_P || !mu1 || !sigma1 || !mu2 || !sigma2) return false;
    if (!(ref1 - ref1 == 0.0) || !(ref2 - ref2 == 0.0) || (P > 0 && !front_host)) return false;
    for (int32_t i = 0; i < P; ++i) {
        const double a = front_host[2 * i], c = front_host[2 * i + 1];
        if (!(a - a == 0.0) || !(c - c == 0.0) || !(a < ref1) || !(c < ref2)) return false;
        if (i > 0 && (!(front_host[2 * i - 2] < a) || !(front_host[2 * i - 1] > c))) return false;
    }
    return true;
}

// ---- the length scales as the kernels take them: il2[k] = 1 / ls_k^2 (cov_r2, cov_entry.h), isc[k] = 1 / (ls_k sqrt 2)
// (the scoring form of cov_entry.h), k < d; either may be null.  EXACTLY these expressions: the values feed kernels whose
// outputs are compared bit for bit.  The entries k >= d are the caller's.  false: a length scale that is not positive.
inline bool length_scale_scalings(const double *ls_host, int d, double *il2, double *isc) {
    for (int k = 0; k < d; ++k) {
        const double l = ls_host[k];
        if (!(l > 0.0)) return false;
        if (il2) il2[k] = 1.0 / (l * l);
        if (isc) isc[k] = 1.0 / (l * 1.4142135623730950488);
    }
    return true;
}

// ---- one kernel instance per feature count: CALL(1) ... CALL(GPBO_MAX_D) by the run-time d, inside a function that returns a
// status.  Every dispatch over d goes through it.
#define GPBO_FOR_D(d, CALL)           \
    switch ((d)) {                    \
        case 1: CALL(1); break;       \
        case 2: CALL(2); break;       \
        case 3: CALL(3); break;       \
        case 4: CALL(4); break;       \
        case 5: CALL(5); break;       \
        case 6: CALL(6); break;       \
        case 7: CALL(7); break;       \
        case 8: CALL(8); break;       \
        case 9: CALL(9); break;       \
        case 10: CALL(10); break;     \
        case 11: CALL(11); break;     \
        case 12: CALL(12); break;     \
        case 13: CALL(13); break;     \
        case 14: CALL(14); break;     \
        case 15: CALL(15); break;     \
        case 16: CALL(16); break;     \
        default: return GPBO_ERR_ARG; \
    }
static_assert(GPBO_MAX_D == 16, "GPBO_FOR_D lists the feature counts 1 ... GPBO_MAX_D");

// ---- environment switches (include/gpbo.h lists them; a caller that wants one read per process keeps it in a static const)
inline const char *env_str(const char *name) { return getenv(name); }
inline int env_int(const char *name, int dflt) {
    const char *e = env_str(name);
    return e ? atoi(e) : dflt;
}
inline bool env_flag(const char *name) { return env_int(name, 0) != 0; }

// Column groups of the fp64 variance kernel (sigma_acq.hip) for a call of M candidates, 1 = none: a rule of the PROBLEM
// (N, candidates of the call), never of the chunking, so results stay chunk-size invariant bit for bit.  GPBO_F64_GROUPS=1
// switches it off (A/B runs).  Both drivers of that kernel ask here.
inline int f64_column_groups(int64_t M, int64_t Np) {
    static const int g = env_int("GPBO_F64_GROUPS", 8);
    return (g > 1 && g <= 16 && M >= 32768 && Np / GPBO_NPAD >= 2 * g) ? g : 1;
}

// ---- the model and the acquisition, filled once at each extern "C" entry ----------------------------------------------------
struct GpModel {
    const double *X;   // [N x d] observations (device)
    int64_t N, Np;
    int32_t d;
    const double *ls_host;
    const double *U;   // (L^-1)^T in fp64; null on the routes that bring their own copy of it (int8 slices)
    const double *alpha;
    double prior_var;
    int32_t kernel;    // GPBO_KERNEL_*; a driver that does not set it gets 0 = the squared exponential
};
struct Acquisition {
    int32_t kind;   // GPBO_ACQ_*
    double p0, p1;
};

// ---- dense outputs of a call (each optional); at(s): those of the chunk that starts at candidate s, null stays null ------------
struct DenseOut {
    double *mu, *sigma, *acq, *var;
    static double *shift(double *p, int64_t s) { return p ? p + s : nullptr; }
    DenseOut at(int64_t s) const { return {shift(mu, s), shift(sigma, s), shift(acq, s), shift(var, s)}; }
};

// ---- profile slots ---------------------------------------------------------------------------------------------------------
// One slot of a gpbo_profile per chunk:  [kbegin |] K(X*,X) | begin | variance launch | end [| qEI launch | qend].  The launches
// of a call form one chain on the stream, so the event in front of the variance launch ends the K(X*,X) interval, and that
// interval begins at the previous slot's end event (kmode 2: chunks after the first) or at kbegin (kmode 1).  A full or
// absent profile turns every call into a no-op that succeeds.  Every method returns false when hipEventRecord fails.
class ProfileRecorder {
    gpbo_profile *p_;
    bool prev_recorded_ = false;   // the previous chunk's variance launch has an end event in the slot before
    bool rec_ = false;             // the slot in hand is recorded (decided at begin())
    bool open() const { return p_ && p_->count < p_->capacity; }
    static bool mark(void *ev, hipStream_t st) { return hipEventRecord(reinterpret_cast<hipEvent_t>(ev), st) == hipSuccess; }

public:
    explicit ProfileRecorder(gpbo_profile *p) : p_(p) {}
    // in front of the K(X*,X) launch of the next slot.  timed = false: the launch is not on the variance launches' stream
    // (kmode 0).  may_chain = false: first chunk of a call, or a driver with another launch between `end` and here.
    bool kstar(hipStream_t st, bool may_chain, bool timed = true) {
        if (!open()) return true;
        const int i = p_->count;
        if (!timed) {
            p_->kmode[i] = 0;
            return true;
        }
        const bool chained = may_chain && i > 0 && prev_recorded_;
        p_->kmode[i] = chained ? 2 : 1;
        return chained || mark(p_->kbegin[i], st);
    }
    // in front of the variance launch
    bool begin(hipStream_t st) {
        rec_ = open();
        return !rec_ || mark(p_->begin[p_->count], st);
    }
    // behind the variance launch; the slot stays in hand (a qEI launch follows)
    bool end_open(hipStream_t st) { return !rec_ || mark(p_->end[p_->count], st); }
    // behind the variance launch: the slot is complete
    bool end(hipStream_t st, int64_t cands) {
        if (!end_open(st)) return false;
        close(cands);
        return true;
    }
    // behind the qEI launch: the slot is complete
    bool qend(hipStream_t st, int64_t cands) {
        if (rec_) {
            if (!mark(p_->qend[p_->count], st)) return false;
            p_->qmode[p_->count] = 1;
        }
        close(cands);
        return true;
    }

private:
    void close(int64_t cands) {
        if (rec_) {
            p_->cands[p_->count] = cands;
            ++p_->count;
        }
        prev_recorded_ = rec_;
    }
};

#pragma GCC visibility pop
