// Off-grid refinement of selected points by acquisition gradients (not in the reference, which only ever
// answers with one of the candidates it was given: /root/reference/point_selector.py:197-207).
//
// For a query point x, with k_n = exp(-1/2 sum_k (x_k - X_nk)^2 / ls_k^2) and g_nk = (X_nk - x_k) / ls_k^2:
//     mu    = sum_n k_n alpha_n                    dmu_k  = sum_n k_n alpha_n g_nk
//     v     = U^T k,  var = prior_var - |v|^2      w = U v (= K^-1 k),   dvar_k = -2 sum_n k_n w_n g_nk
//     sigma = sqrt(|var|)                          dsigma_k = sign(var) dvar_k / (2 sigma)        (0 when sigma == 0)
//     LCB: acq = p0 sigma - mu                     dacq = p0 dsigma - dmu
//     EI : imp = p0 - mu - p1, z = imp / sigma     dacq = -Phi(z) dmu + phi(z) dsigma   (sigma == 0: -dmu if imp > 0, else 0)
//
// One evaluation of P points is four launches on the caller's stream (Pp = P rounded up to 64):
//     refine_ks_kernel         Ks [Pp x Np], POINT-major (row p = the k_n of point p, zeros on the padding): the GEMM takes a
//                              row-major A only, and with the points as rows both products below are plain calls of it
//     gemm  Vt = Ks U          (row p = v of point p)
//     gemm  Wt = Vt U^T        (row p = w of point p)
//     refine_grad_step_kernel  a workgroup per point: the 2 + 2 d sums over n, then thread 0 finishes the point - value,
//                              gradient and, when refining, the accept / reject decision and the next trial point
// Refinement (gpbo_refine_f64) is projected gradient ascent with a doubling / halving step, every start on its own:
//     x <- clip(start);  t <- step0 / max_k(|g_k| ls_k)   (the first trial moves no coordinate by more than step0 length scales)
//     iters times:  x' = clip(x + t g ls^2);  accept iff x' != x, f' finite and f' >= f + 1e-4 g . (x' - x)  (then t <- 2 t),
//                   else t <- t / 2
// All iters + 1 evaluations are enqueued without a host round trip; the per-point state lives in a device record.  No random
// numbers, no atomics, fixed summation orders: two calls give the same bits.
#include "gpbo_internal.h"

#include <cmath>
#include <limits>

#include "cov_entry.h"

namespace {

struct RefineBox {
    double lo[GPBO_MAX_D], hi[GPBO_MAX_D];
    double ls[GPBO_MAX_D];   // ls_k
    double l2[GPBO_MAX_D];   // ls_k^2
    double il2[GPBO_MAX_D];  // 1 / ls_k^2
    double isc[GPBO_MAX_D];  // 1 / (ls_k sqrt 2): the scoring form of cov_entry.h
};

// The state of one start, on the device from the first launch of a call to the last.
struct RefinePoint {
    double x[GPBO_MAX_D];   // the accepted point
    double g[GPBO_MAX_D];   // dacq there
    double f, acq0, t;
    int32_t accepted, frozen;
};

enum { MODE_EVAL = 0, MODE_START = 1, MODE_STEP = 2 };

constexpr double kArmijo = 1e-4;
constexpr int KS_POINTS = 8;   // points per workgroup of refine_ks_kernel (Pp is a multiple of 64)

__device__ __forceinline__ double clip(double v, double lo, double hi) {   // NaN stays NaN (as numpy.clip)
    return v < lo ? lo : (v > hi ? hi : v);
}

// Ks[p][n] for 256 observations x KS_POINTS points per workgroup: the observation's scaled row stays in registers, the
// points' coordinates are wave-uniform.  Difference form on coordinates pre-scaled by 1 / (ls sqrt 2): exp(-0) = 1 exactly
// when a point sits on an observation.  grid (ceil(Np / 256), Pp / KS_POINTS), block 256.
template <int D>
__global__ __launch_bounds__(256) void refine_ks_kernel(const double *__restrict__ pts, int P, const double *__restrict__ Xsc,
                                                        int N, int Np, RefineBox box, double *__restrict__ Ks) {
    __shared__ double tab[GPBO_EXP_E];
    const int tid = threadIdx.x;
    cov_stage_tab(tab, tid);
    const int n = blockIdx.x * 256 + tid;
    double xo[D];
#pragma unroll
    for (int k = 0; k < D; ++k) xo[k] = (n < N) ? Xsc[(int64_t)n * D + k] : 0.0;
    gpbo_syncthreads();
    if (n >= Np) return;
    const int p0 = blockIdx.y * KS_POINTS;
    for (int i = 0; i < KS_POINTS; ++i) {
        const int p = p0 + i;
        double v = 0.0;
        if (p < P && n < N) {
            const double *xp = pts + (int64_t)p * D;   // wave-uniform
            double s = 0.0;   // cov_s of cov_entry.h on a point scaled on the fly, written out (see there)
#pragma unroll
            for (int k = 0; k < D; ++k) {
                const double df = xp[k] * box.isc[k] - xo[k];
                s = fma(df, df, s);
            }
            v = cov_from_s<GPBO_KERNEL_SE>(s, tab);
        }
        Ks[(int64_t)p * Np + n] = v;
    }
}

// What thread 0 needs of the acquisition at one point: value and gradient from the reduced sums.
template <int D>
__device__ __forceinline__ void value_and_gradient(int kind, double p0, double p1, double prior_var, double mu, double vv,
                                                   const double *dmu, const double *dkw, bool finite_x, double *sigma_out,
                                                   double *acq_out, double *dsigma, double *dacq) {
    const double var = prior_var - vv;
    const double sigma = sqrt(fabs(var));
    double acq = gpbo_acquisition(kind, mu, sigma, p0, p1);
    const double sgn = var < 0.0 ? -1.0 : 1.0;
    double cm, cs;   // dacq = cm dmu + cs dsigma
    if (kind == GPBO_ACQ_LCB) {
        cm = -1.0;
        cs = p0;
    } else {
        const double imp = p0 - mu - p1;
        if (sigma > 0.0) {
            const double z = imp / sigma;
            cm = -(0.5 * erfc(-z * 0.70710678118654752440));
            cs = exp(-0.5 * z * z) * 0.39894228040143267794;
        } else {
            cm = (imp > 0.0) ? -1.0 : 0.0;
            cs = 0.0;
        }
    }
    const double nan = __builtin_nan("");
#pragma unroll
    for (int k = 0; k < D; ++k) {
        const double dvar = -2.0 * dkw[k];
        const double ds = (sigma == 0.0) ? 0.0 : sgn * dvar / (2.0 * sigma);
        dsigma[k] = finite_x ? ds : nan;
        dacq[k] = finite_x ? cm * dmu[k] + cs * ds : nan;
    }
    if (!finite_x) acq = nan;   // exp_neg returns 0 for a NaN argument: a point with a non-finite coordinate is poisoned here
    *sigma_out = finite_x ? sigma : nan;
    *acq_out = acq;
}

// One workgroup of 256 threads per point.  Threads stride over n (coalesced rows of Ks / Wt / Vt, alpha; the rows of X
// come from L2) with 2 + 2 D partial sums in registers; wave reduction by a fixed butterfly, the four waves through LDS in
// a fixed order; thread 0 finishes the point.  grid P, block 256.
//   MODE_EVAL : the six outputs of gpbo_posterior_grad_f64 (each optional)
//   MODE_START: pts = the clipped starts; records (x, f, g), acq0, the first step length, and writes the first trial
//   MODE_STEP : pts = the trials; accept / reject, the next step length, and the next trial
template <int D>
__global__ __launch_bounds__(256) void refine_grad_step_kernel(
    const double *__restrict__ Ks, const double *__restrict__ Vt, const double *__restrict__ Wt, int Np,
    const double *__restrict__ alpha, const double *__restrict__ X, int N, const double *pts /* may be `trial` */, RefineBox box,
    double prior_var, int kind, double p0, double p1, int mode, double step0, RefinePoint *__restrict__ rec,
    double *trial, double *__restrict__ mu_out, double *__restrict__ sigma_out, double *__restrict__ acq_out,
    double *__restrict__ dmu_out, double *__restrict__ dsigma_out, double *__restrict__ dacq_out) {
    constexpr int S = 2 + 2 * D;
    __shared__ double part[4][S];
    const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
    const int p = blockIdx.x;
    const double *ks = Ks + (int64_t)p * Np, *vt = Vt + (int64_t)p * Np, *wt = Wt + (int64_t)p * Np;
    double xq[D];
#pragma unroll
    for (int k = 0; k < D; ++k) xq[k] = pts[(int64_t)p * D + k];
    double mu = 0.0, vv = 0.0, dmu[D], dkw[D];
#pragma unroll
    for (int k = 0; k < D; ++k) dmu[k] = dkw[k] = 0.0;
    for (int n = tid; n < Np; n += 256) {
        const double v = vt[n];
        vv = fma(v, v, vv);
        if (n < N) {
            const double kn = ks[n];
            const double ka = kn * alpha[n], kw = kn * wt[n];
            mu += ka;
            const double *xo = X + (int64_t)n * D;
#pragma unroll
            for (int k = 0; k < D; ++k) {
                const double g = (xo[k] - xq[k]) * box.il2[k];
                dmu[k] = fma(ka, g, dmu[k]);
                dkw[k] = fma(kw, g, dkw[k]);
            }
        }
    }
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) {
        mu += __shfl_xor(mu, off);
        vv += __shfl_xor(vv, off);
#pragma unroll
        for (int k = 0; k < D; ++k) {
            dmu[k] += __shfl_xor(dmu[k], off);
            dkw[k] += __shfl_xor(dkw[k], off);
        }
    }
    if (lane == 0) {
        part[wid][0] = mu;
        part[wid][1] = vv;
#pragma unroll
        for (int k = 0; k < D; ++k) {
            part[wid][2 + k] = dmu[k];
            part[wid][2 + D + k] = dkw[k];
        }
    }
    gpbo_syncthreads();
    if (tid != 0) return;
    mu = ((part[0][0] + part[1][0]) + part[2][0]) + part[3][0];
    vv = ((part[0][1] + part[1][1]) + part[2][1]) + part[3][1];
    bool finite_x = true;
#pragma unroll
    for (int k = 0; k < D; ++k) {
        dmu[k] = ((part[0][2 + k] + part[1][2 + k]) + part[2][2 + k]) + part[3][2 + k];
        dkw[k] = ((part[0][2 + D + k] + part[1][2 + D + k]) + part[2][2 + D + k]) + part[3][2 + D + k];
        finite_x = finite_x && (xq[k] - xq[k] == 0.0);
    }
    const double nan = __builtin_nan("");
    double sigma, f, dsig[D], g[D];
    value_and_gradient<D>(kind, p0, p1, prior_var, mu, vv, dmu, dkw, finite_x, &sigma, &f, dsig, g);
    if (mode == MODE_EVAL) {
        if (mu_out) mu_out[p] = finite_x ? mu : nan;
        if (sigma_out) sigma_out[p] = sigma;
        if (acq_out) acq_out[p] = f;
#pragma unroll
        for (int k = 0; k < D; ++k) {
            if (dmu_out) dmu_out[(int64_t)p * D + k] = finite_x ? dmu[k] : nan;
            if (dsigma_out) dsigma_out[(int64_t)p * D + k] = dsig[k];
            if (dacq_out) dacq_out[(int64_t)p * D + k] = g[k];
        }
        return;
    }
    RefinePoint *r = rec + p;
    double t, x[D];
    if (mode == MODE_START) {
        double m = 0.0;
        bool fin = true;
#pragma unroll
        for (int k = 0; k < D; ++k) {
            const double a = fabs(g[k]) * box.ls[k];
            fin = fin && (a - a == 0.0);
            if (a > m) m = a;
            x[k] = xq[k];
            r->x[k] = xq[k];
            r->g[k] = g[k];
        }
        const bool frozen = !fin || !(m > 0.0);
        t = frozen ? 0.0 : step0 / m;
        r->f = f;
        r->acq0 = f;
        r->accepted = 0;
        r->frozen = frozen ? 1 : 0;
    } else {
        const double f0 = r->f;
        double gx[D], s = 0.0;
        bool moved = false;
#pragma unroll
        for (int k = 0; k < D; ++k) {
            x[k] = r->x[k];
            gx[k] = r->g[k];
            moved = moved || (xq[k] != x[k]);
            s = s + gx[k] * (xq[k] - x[k]);
        }
        const bool accept = !r->frozen && moved && (f - f == 0.0) && f >= f0 + kArmijo * s;
        t = r->t;
        if (accept) {
#pragma unroll
            for (int k = 0; k < D; ++k) {
                x[k] = xq[k];
                r->x[k] = xq[k];
                r->g[k] = g[k];
            }
            r->f = f;
            r->accepted += 1;
            t = 2.0 * t;
        } else {
#pragma unroll
            for (int k = 0; k < D; ++k) g[k] = gx[k];
            t = t / 2.0;
        }
    }
    r->t = t;
    const bool frozen = r->frozen != 0;
#pragma unroll
    for (int k = 0; k < D; ++k)
        trial[(int64_t)p * D + k] = frozen ? x[k] : clip(x[k] + t * g[k] * box.l2[k], box.lo[k], box.hi[k]);
}

// trial[p] = clip(start[p]).  grid ceil(P d / 256), block 256.
__global__ __launch_bounds__(256) void refine_init_kernel(const double *__restrict__ Xq, int P, int d, RefineBox box,
                                                          double *__restrict__ trial) {
    const int e = blockIdx.x * 256 + threadIdx.x;
    if (e >= P * d) return;
    const int k = e % d;
    trial[e] = clip(Xq[e], box.lo[k], box.hi[k]);
}

// One workgroup: the outputs of every point, the projected-gradient norm, then the first-index arg-max of the final values
// (NaN counted by acq0: such a start never moved).
__global__ __launch_bounds__(256) void refine_finish_kernel(const RefinePoint *__restrict__ rec, int P, int d, RefineBox box,
                                                            double *__restrict__ Xq, double *__restrict__ acq_out,
                                                            double *__restrict__ acq0_out, int32_t *__restrict__ accepted_out,
                                                            double *__restrict__ pg_out, gpbo_result *__restrict__ result) {
    __shared__ double s_val[4];
    __shared__ int64_t s_idx[4], s_nan[4];
    const int tid = threadIdx.x, lane = tid & 63;
    double bv = gpbo_none::val;
    int64_t bi = gpbo_none::idx, nans = 0;
    for (int p = tid; p < P; p += 256) {
        const RefinePoint *r = rec + p;
        double pg = 0.0;
        bool bad = false;
        for (int k = 0; k < d; ++k) {
            const double x = r->x[k];
            const double v = fabs(x - clip(x + r->g[k] * box.l2[k], box.lo[k], box.hi[k])) / box.ls[k];
            bad = bad || (v != v);
            if (v > pg) pg = v;
            Xq[(int64_t)p * d + k] = x;
        }
        if (bad) pg = __builtin_nan("");
        const double f = r->f, f0 = r->acq0;
        if (acq_out) acq_out[p] = f;
        if (acq0_out) acq0_out[p] = f0;
        if (accepted_out) accepted_out[p] = r->accepted;
        if (pg_out) pg_out[p] = pg;
        if (f0 != f0) ++nans;
        if (f == f && gpbo_better(f, p, bv, bi)) { bv = f; bi = p; }
    }
#pragma unroll
    for (int off = 1; off < 64; off <<= 1) nans += __shfl_xor(nans, off);
    if (lane == 0) s_nan[tid >> 6] = nans;
    gpbo_argmax_post(bv, bi, lane, tid >> 6, s_val, s_idx);
    gpbo_syncthreads();
    if (tid == 0) {
        for (int w = 1; w < 4; ++w) nans += s_nan[w];
        gpbo_argmax_fold(s_val, s_idx, 4, bv, bi);
        result->best_val = (bi == gpbo_none::idx) ? __builtin_nan("") : bv;
        result->best_idx = (bi == gpbo_none::idx) ? -1 : bi;
        result->nan_count = nans;
        result->reserved = 0;
    }
}

struct Layout {
    double *xsc, *ks, *vt, *wt;
    RefinePoint *rec;   // the stepping state: null in the workspace of the gradient call
    double *trial;
    int64_t Pp, total;
    Layout(void *work, int64_t Np, int64_t P, bool stepping) {
        Carver c(work);
        Pp = align_up(P, 64);
        xsc = c.take<double>(Np * GPBO_MAX_D);
        ks = c.take<double>(Pp * Np);
        vt = c.take<double>(Pp * Np);
        wt = c.take<double>(Pp * Np);
        rec = stepping ? c.take<RefinePoint>(Pp) : nullptr;
        trial = stepping ? c.take<double>(Pp * GPBO_MAX_D) : nullptr;
        total = c.total();
    }
};

bool sizes_ok(int64_t Np, int64_t P) { return np_ok(Np) && Np <= (1 << 20) && P >= 1 && P <= GPBO_REFINE_MAX_P; }

bool make_box(const double *ls_host, const double *lower, const double *upper, int d, RefineBox *box) {
    for (int k = 0; k < GPBO_MAX_D; ++k) {
        box->lo[k] = box->hi[k] = 0.0;
        box->ls[k] = box->l2[k] = box->il2[k] = box->isc[k] = 1.0;
    }
    if (!length_scale_scalings(ls_host, d, box->il2, box->isc)) return false;
    for (int k = 0; k < d; ++k) {
        const double l = ls_host[k];
        box->ls[k] = l;
        box->l2[k] = l * l;
        if (lower) {
            if (!std::isfinite(lower[k]) || !std::isfinite(upper[k]) || lower[k] > upper[k]) return false;
            box->lo[k] = lower[k];
            box->hi[k] = upper[k];
        }
    }
    return true;
}

struct Eval {
    const double *X, *U, *alpha;
    int N, Np, P, Pp, d;
    RefineBox box;
    double prior_var, p0, p1;
    int kind;
    double *Xsc, *Ks, *Vt, *Wt;
    hipStream_t st;
};

// The four launches of one evaluation at the points `pts` [P x d].
int evaluate(const Eval &e, const double *pts, int mode, double step0, RefinePoint *rec, double *trial, double *mu_out,
             double *sigma_out, double *acq_out, double *dmu_out, double *dsigma_out, double *dacq_out) {
    const dim3 kgrid((unsigned)((e.Np + 255) / 256), (unsigned)(e.Pp / KS_POINTS));
#define KS(DD) hipLaunchKernelGGL(refine_ks_kernel<DD>, kgrid, dim3(256), 0, e.st, pts, e.P, e.Xsc, e.N, e.Np, e.box, e.Ks)
#define GS(DD)                                                                                                              \
    hipLaunchKernelGGL(refine_grad_step_kernel<DD>, dim3((unsigned)e.P), dim3(256), 0, e.st, e.Ks, e.Vt, e.Wt, e.Np, e.alpha,  \
                       e.X, e.N, pts, e.box, e.prior_var, e.kind, e.p0, e.p1, mode, step0, rec, trial, mu_out, sigma_out,     \
                       acq_out, dmu_out, dsigma_out, dacq_out)
    GPBO_FOR_D(e.d, KS)
    GPBO_CHECK_LAUNCH();
    // U is upper triangular; both products run dense (the GEMM's triangular skips are for the lower case)
    int rc = gpbo_gemm_launch_tri(0, e.Pp, e.Np, e.Np, 1.0, e.Ks, e.Np, 0, e.U, e.Np, 0, 0.0, e.Vt, e.Np, 0, 1, 0, 0, e.st);
    if (rc != GPBO_OK) return rc;
    rc = gpbo_gemm_launch_tri(1, e.Pp, e.Np, e.Np, 1.0, e.Vt, e.Np, 0, e.U, e.Np, 0, 0.0, e.Wt, e.Np, 0, 1, 0, 0, e.st);
    if (rc != GPBO_OK) return rc;
    GPBO_FOR_D(e.d, GS)
    GPBO_CHECK_LAUNCH();
#undef KS
#undef GS
    return GPBO_OK;
}

int make_eval(Eval *e, const Layout &L, const double *X, int64_t N, int64_t Np, int64_t P, int32_t d, const double *ls_host,
              const double *U, const double *alpha, double prior_var, int32_t acq_kind, double p0, double p1, void *stream) {
    e->X = X; e->U = U; e->alpha = alpha;
    e->N = (int)N; e->Np = (int)Np; e->P = (int)P; e->Pp = (int)L.Pp; e->d = (int)d;
    e->prior_var = prior_var; e->p0 = p0; e->p1 = p1; e->kind = (int)acq_kind;
    e->Xsc = L.xsc; e->Ks = L.ks; e->Vt = L.vt; e->Wt = L.wt;
    e->st = gpbo_stream(stream);
    return gpbo_scale_points_launch(X, N, Np, d, ls_host, e->Xsc, nullptr, stream);
}

bool model_ok(const double *X, int64_t N, int64_t Np, int32_t d, const double *ls_host, const double *U, const double *alpha,
              double prior_var, int32_t acq_kind, int64_t P) {
    if (!X || !ls_host || !U || !alpha) return false;
    if (!aligned_to(U, 16)) return false;   // the GEMM's B operand; refused here so that nothing is enqueued first
    if (d < 1 || d > GPBO_MAX_D || N < 1 || !sizes_ok(Np, P) || Np != gpbo_padded_n(N)) return false;
    return acq_kind_ok(acq_kind) && length_scales_ok(ls_host, d) && std::isfinite(prior_var);
}

}  // namespace

extern "C" int64_t gpbo_posterior_grad_workspace_bytes(int64_t Np, int64_t P) {
    if (!sizes_ok(Np, P)) return GPBO_ERR_ARG;
    return Layout(nullptr, Np, P, false).total;
}

extern "C" int64_t gpbo_refine_workspace_bytes(int64_t Np, int64_t P) {
    if (!sizes_ok(Np, P)) return GPBO_ERR_ARG;
    return Layout(nullptr, Np, P, true).total;
}

extern "C" int gpbo_posterior_grad_f64(const double *Xq, int64_t P, const double *X, int64_t N, int64_t Np, int32_t d,
                                       const double *ls_host, const double *U, const double *alpha, double prior_var,
                                       int32_t acq_kind, double p0, double p1, double *mu_out, double *sigma_out,
                                       double *acq_out, double *dmu_out, double *dsigma_out, double *dacq_out, void *work,
                                       int64_t work_bytes, void *stream) {
    if (!Xq || !work || !model_ok(X, N, Np, d, ls_host, U, alpha, prior_var, acq_kind, P)) return GPBO_ERR_ARG;
    const Layout L(work, Np, P, false);
    if (work_bytes < L.total || !aligned_to(work, 256)) return GPBO_ERR_WORKSPACE;
    Eval e;
    if (!make_box(ls_host, nullptr, nullptr, d, &e.box)) return GPBO_ERR_ARG;
    int rc = make_eval(&e, L, X, N, Np, P, d, ls_host, U, alpha, prior_var, acq_kind, p0, p1, stream);
    if (rc != GPBO_OK) return rc;
    return evaluate(e, Xq, MODE_EVAL, 0.0, nullptr, nullptr, mu_out, sigma_out, acq_out, dmu_out, dsigma_out, dacq_out);
}

extern "C" int gpbo_refine_f64(double *Xq, int64_t P, const double *lower_host, const double *upper_host, const double *X,
                               int64_t N, int64_t Np, int32_t d, const double *ls_host, const double *U, const double *alpha,
                               double prior_var, int32_t acq_kind, double p0, double p1, int32_t iters, double step0,
                               double *acq_out, double *acq0_out, int32_t *accepted_out, double *pg_out, gpbo_result *result,
                               void *work, int64_t work_bytes, void *stream) {
    if (!Xq || !lower_host || !upper_host || !result || !work) return GPBO_ERR_ARG;
    if (!model_ok(X, N, Np, d, ls_host, U, alpha, prior_var, acq_kind, P)) return GPBO_ERR_ARG;
    if (iters < 0 || iters > 1000 || !(step0 > 0.0) || !std::isfinite(step0)) return GPBO_ERR_ARG;
    const Layout L(work, Np, P, true);
    Eval e;
    if (!make_box(ls_host, lower_host, upper_host, d, &e.box)) return GPBO_ERR_ARG;
    if (work_bytes < L.total || !aligned_to(work, 256)) return GPBO_ERR_WORKSPACE;
    int rc = make_eval(&e, L, X, N, Np, P, d, ls_host, U, alpha, prior_var, acq_kind, p0, p1, stream);
    if (rc != GPBO_OK) return rc;
    hipLaunchKernelGGL(refine_init_kernel, dim3((unsigned)((P * d + 255) / 256)), dim3(256), 0, e.st, Xq, (int)P, (int)d, e.box,
                       L.trial);
    GPBO_CHECK_LAUNCH();
    for (int it = 0; it <= iters; ++it) {
        rc = evaluate(e, L.trial, it == 0 ? MODE_START : MODE_STEP, step0, L.rec, L.trial, nullptr, nullptr, nullptr, nullptr,
                      nullptr, nullptr);
        if (rc != GPBO_OK) return rc;
    }
    hipLaunchKernelGGL(refine_finish_kernel, dim3(1), dim3(256), 0, e.st, L.rec, (int)P, (int)d, e.box, Xq, acq_out, acq0_out,
                       accepted_out, pg_out, result);
    GPBO_CHECK_LAUNCH();
    return GPBO_OK;
}
