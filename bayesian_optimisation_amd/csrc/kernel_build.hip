// ARD squared-exponential covariance builds (SURVEY.md §2.2 K1, K2+K5).
//
// Replaces PointSelector.kernel_rbf (/root/reference/point_selector.py:166-195): the reference
// broadcasts an (n1, n2, d) temporary; here one thread owns a column (a candidate, or an observed
// point for K(X,X)), keeps its d coordinates in VGPRs, and walks the other set of points, whose
// coordinates are wave-uniform and therefore travel through the scalar cache into SGPRs.
// K(X,X) follows the reference's order per entry: subtract, square, scale by 1/ls_k^2 (the reference
// divides by ls_k^2; multiplying by the host-rounded reciprocal differs by <= 1 ulp per term), sum over
// features in index order, times -0.5, exp.  K(X*,X) - M x N entries, the fp64-issue-bound kernel - uses
// coordinates pre-scaled by 1/(ls_k sqrt 2) and its own exp(-t); both agree with the reference's values
// to a few ulp (tests: 5e-15 absolute on entries <= 1).
// Both kernels take the covariance family as a template parameter (GPBO_KERNEL_*, include/gpbo.h): the squared-exponential
// instances are the code above unchanged, the Matern instances replace the exponential of the accumulated distance by
// (1 + a) exp(-a) or (1 + a + a^2 / 3) exp(-a), a = sqrt(3) r or sqrt(5) r.
#include "cov_entry.h"

#include <cstdlib>
#include <vector>

// ---------------------------------------------------------------------------------------------
// K1: Kp[Np x Np] = k(X, X) with diagonal (1 + j1) + j2; identity on the padding.
// grid (ceil(Np/256), Np/8), block 256: thread = column j, block row-slice of 8 rows (the chains of one
// entry are ~45 dependent fp64 instructions, so parallelism over rows matters more than reuse of xj).
// ---------------------------------------------------------------------------------------------
template <int D, int KERN>
__global__ __launch_bounds__(256) void kxx_kernel(const double *__restrict__ X, int N, CovLs ls, double j1,
                                                  double j2, double *__restrict__ K, int Np,
                                                  double *__restrict__ K2 /* optional second copy (the one the
                                                  factorisation overwrites), row stride ld2; ld2 >= 2 Np: the stacked
                                                  matrix [K | 0] of cholinv.hip, zeros written here too */, int ld2,
                                                  int32_t *__restrict__ info0 /* optional:
                                                  zeroed here, saving the factorisation a launch */) {
    const int j = blockIdx.x * 256 + threadIdx.x;
    if (info0 && blockIdx.x == 0 && blockIdx.y == 0 && threadIdx.x == 0) *info0 = 0;
    if (j >= Np) return;
    const int i0 = blockIdx.y * 8;
    double xj[D];
#pragma unroll
    for (int k = 0; k < D; ++k) xj[k] = (j < N) ? X[(int64_t)j * D + k] : 0.0;
    for (int i = i0; i < i0 + 8; ++i) {
        double v;
        if (i < N) {  // wave-uniform
            v = cov_from_r2<KERN>(cov_r2<D>(xj, X + (int64_t)i * D, ls.il2));   // r^2: the same bits for (i, j) and (j, i)
            if (i == j) v = (v + j1) + j2;  // reference: kernel_rbf adds 1e-4 (:193), assembly adds 1e-6 (:79)
            if (j >= N) v = 0.0;
        } else {
            v = (i == j) ? 1.0 : 0.0;
        }
        K[(int64_t)i * Np + j] = v;
        if (K2) {
            K2[(int64_t)i * ld2 + j] = v;
            if (ld2 >= 2 * Np) K2[(int64_t)i * ld2 + Np + j] = 0.0;
        }
    }
}

// ---------------------------------------------------------------------------------------------
// K2+K5: KsT[n][c] = k(x_n, x*_c) for one candidate chunk, plus per-slice partial means.
// grid (ldk_used/512, Np/64), block 256: thread = two adjacent candidates (16-byte stores, two
// independent exp chains), blockIdx.y = slice of 64 observations.
// Coordinates are pre-scaled by 1/(ls_k sqrt 2) (the candidates here, the observations by
// scale_points_kernel), so an entry is exp(-sum_k (a_k - b_k)^2): 2 fp64 instructions per feature.
// ---------------------------------------------------------------------------------------------
constexpr int KS_SLICE = GPBO_KS_SLICE;

typedef float f2_t __attribute__((ext_vector_type(2)));
// two adjacent candidates' entries of one K*^T row: 16 B (fp64) or, rounded once to fp32, 8 B (the fp32 screen)
// NT: the non-temporal hint on the rows of K*^T.  Measured on MI355X (same box, tools/ab_kstar.sh): at N = 4096 a
// 2^17-candidate slab is 4.3 GB - nothing of it survives in the 256-MiB Infinity Cache until the variance kernel reads it,
// and with the hint the build runs 0.966 -> 0.807 ms (4.5 -> 5.3 TB/s); at N = 512 (537 MB) the variance kernel still
// finds part of the slab on chip and the hint costs it 2 % for a 2 % shorter build: the host picks by slab size.
template <bool NT>
__device__ __forceinline__ void store_pair(double *p, double a, double b) {
    if (NT) __builtin_nontemporal_store(d2_t{a, b}, reinterpret_cast<d2_t *>(p));
    else *reinterpret_cast<d2_t *>(p) = d2_t{a, b};
}
template <bool NT>
__device__ __forceinline__ void store_pair(float *p, double a, double b) {
    if (NT) __builtin_nontemporal_store(f2_t{(float)a, (float)b}, reinterpret_cast<f2_t *>(p));
    else *reinterpret_cast<f2_t *>(p) = f2_t{(float)a, (float)b};
}

// TK = double: the fp64 path.  TK = float (gpbo_kstar_mu_mixed): entries and means are computed exactly as in the
// fp64 path - the mean partials are the same doubles bit for bit - and only the stored K*^T is rounded to fp32
// (relative error <= 2^-24 per entry) for the fp32 variance screen.
// KERN: cov_from_s<KERN> (cov_entry.h).  The HAS_DIAG quirk belongs to the reference's kernel_rbf: squared exponential only.
// BESIDE = false: grid (ldk_used/512, Np/64), one slice of 64 observations per workgroup.
// BESIDE = true: the form that runs on the compute units of a variance launch (sigma_acq.hip: K(X*,X) of chunk c + 1 beside
// the variance kernel of chunk c).  A variance workgroup leaves 64 of a SIMD's 512 registers and 4 KiB of LDS free, so this
// form is held to 64 VGPRs (waves-per-EU 8) and is instantiated only where that costs neither a spill nor scratch
// (KSTAR_BESIDE_MAX_D).  Its grid is (ldk_used/512, gy) with gy chosen by the launcher so that there is one workgroup per
// compute unit at the most, each walking the slices blockIdx.y, blockIdx.y + gy, ...: once the workgroups are resident nothing
// is pending that could take a freed compute unit ahead of the next variance workgroup.  Per entry the same instructions and
// over n the same order as the other form, hence the same bits.
template <int D, int VARIANT, bool HAS_DIAG, bool BESIDE, typename TK, bool NT, int KERN = GPBO_KERNEL_SE>
__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(BESIDE ? 8 : 0, BESIDE ? 8 : 0)))
void kstar_mu_kernel(const double *__restrict__ Xs, int64_t Mc,
                                                       const double *__restrict__ Xsc, int N, CovLs ls,
                                                       const double *__restrict__ alpha, double diag_add,
                                                       int64_t cand_base, TK *__restrict__ KsT, int64_t ldk,
                                                       double *__restrict__ mu_part,
                                                       int store_rows /* rows n >= store_rows are not stored (multiple of 64):
                                                                         the prefix-bound screen needs the mean of all N
                                                                         observations but K*^T of the first few only */,
                                                       int nslices /* BESIDE: Np / 64 (the grid no longer says) */) {
    static_assert(KERN == GPBO_KERNEL_SE || (!HAS_DIAG && VARIANT == 0), "the quirk and the timing variants are SE-only");
    static_assert(!BESIDE || (VARIANT == 0 && !HAS_DIAG && KERN == GPBO_KERNEL_SE), "the co-resident form: the plain build only");
    static_assert(!BESIDE || sizeof(TK) == sizeof(double), "the co-resident form: fp64 rows (one byte offset serves K*^T and mu_part)");
    __shared__ double tab[GPBO_EXP_E];
    cov_stage_tab(tab, threadIdx.x);
    const int64_t c0 = ((int64_t)blockIdx.x * 256 + threadIdx.x) * 2;
    double xa[D], xb[D];   // (the scaled load stays written out: see cov_entry.h)
#pragma unroll
    for (int k = 0; k < D; ++k) {
        xa[k] = ((c0 < Mc) ? Xs[c0 * D + k] : 0.0) * ls.isc[k];
        xb[k] = ((c0 + 1 < Mc) ? Xs[(c0 + 1) * D + k] : 0.0) * ls.isc[k];
    }
    __syncthreads();
    bool nan_a = false, nan_b = false;  // NaN candidate coordinates: the reference's k is NaN, hence mu and the acquisition
#pragma unroll
    for (int k = 0; k < D; ++k) {
        nan_a = nan_a || (xa[k] != xa[k]);
        nan_b = nan_b || (xb[k] != xb[k]);
    }
    // BESIDE: rows are addressed as a wave-uniform base plus the thread's 32-bit byte offset (a row is at most 2^24 entries), which
    // keeps the 64-bit c0 and a 64-bit pointer per thread out of the loop: three registers of the 64
    const unsigned voff = ((unsigned)blockIdx.x * 256u + threadIdx.x) * 2u * (unsigned)sizeof(TK);
    auto at = [&](auto *row) { return BESIDE ? reinterpret_cast<decltype(row)>(reinterpret_cast<char *>(row) + voff) : row; };
    int by = blockIdx.y;
    do {   // (BESIDE: the slices of this workgroup; else the one slice)
    const int n0 = by * KS_SLICE;
    double mua = 0.0, mub = 0.0;
    TK *out = KsT + (int64_t)n0 * ldk + (BESIDE ? 0 : c0);
    const bool do_store = n0 < store_rows;   // workgroup-uniform
    int nend = n0 + KS_SLICE;
    if (nend > N) nend = N;  // observations beyond N are padding: exact zeros, written below
    // two observations per trip: four independent distance/exp chains per thread (the loop is bound by the
    // latency of dependent fp64 instructions, not by their count).  BESIDE: one observation per trip throughout (the tail's
    // form below: two chains, the registers of the other two are what the cap takes) - per entry the same instructions, and the
    // mean partials add up in the same order over n either way.
    int n = n0;
    if (!BESIDE) for (; n + 1 < nend; n += 2) {
        const double *xo0 = Xsc + (int64_t)n * D;  // wave-uniform rows -> scalar loads
        const double *xo1 = xo0 + D;
        double s00, s01, s10, s11;
        cov_s4<D, (VARIANT == 3 ? 1 : D)>(xa, xb, xo0, xo1, s00, s01, s10, s11);
        double k00, k01, k10, k11;
        if (VARIANT == 3) { k00 = s00; k01 = s01; k10 = s10; k11 = s11; }
        else {
            k00 = cov_from_s<KERN>(s00, tab); k01 = cov_from_s<KERN>(s01, tab);
            k10 = cov_from_s<KERN>(s10, tab); k11 = cov_from_s<KERN>(s11, tab);
        }
        if (HAS_DIAG) {  // N == M shape-coincidence quirk (point_selector.py:173,191-193)
            if ((int64_t)n == cand_base + c0) k00 += diag_add;
            if ((int64_t)n == cand_base + c0 + 1) k01 += diag_add;
            if ((int64_t)n + 1 == cand_base + c0) k10 += diag_add;
            if ((int64_t)n + 1 == cand_base + c0 + 1) k11 += diag_add;
        }
        const double a0 = alpha[n], a1 = alpha[n + 1];
        mua = fma(k00, a0, mua);
        mub = fma(k01, a0, mub);
        mua = fma(k10, a1, mua);
        mub = fma(k11, a1, mub);
        if (VARIANT != 1) {
            if (do_store) {
                store_pair<NT>(at(out), k00, k01);
                store_pair<NT>(at(out + ldk), k10, k11);
            }
        } else {
            mua += (k00 + k10) * 1e-300;
            mub += (k01 + k11) * 1e-300;
        }
        out += 2 * ldk;
    }
    if (n < nend) do {  // odd tail
        const double *xo = Xsc + (int64_t)n * D;
        double sa, sb;
        cov_s2<D>(xa, xb, xo, sa, sb);
        double ka = cov_from_s<KERN>(sa, tab), kb = cov_from_s<KERN>(sb, tab);
        if (HAS_DIAG) {
            if ((int64_t)n == cand_base + c0) ka += diag_add;
            if ((int64_t)n == cand_base + c0 + 1) kb += diag_add;
        }
        const double an = alpha[n];
        mua = fma(ka, an, mua);
        mub = fma(kb, an, mub);
        if (do_store) store_pair<NT>(at(out), ka, kb);
        out += ldk;
        ++n;
    } while (BESIDE && n < nend);
    for (n = (nend > n0 ? nend : n0); n < n0 + KS_SLICE; ++n) {
        if (do_store) store_pair<NT>(at(out), 0.0, 0.0);
        out += ldk;
    }
    d2_t m = {nan_a ? __builtin_nan("") : mua, nan_b ? __builtin_nan("") : mub};
    *reinterpret_cast<d2_t *>(at(mu_part + (int64_t)by * ldk + (BESIDE ? 0 : c0))) = m;
    by += gridDim.y;
    } while (BESIDE && by < nslices);
}

// Xsc[n][k] = X[n][k] / (ls_k sqrt 2), rows n >= N zero.   One thread per element.
__global__ __launch_bounds__(256) void scale_points_kernel(const double *__restrict__ X, int64_t N, int64_t Np, int d,
                                                          CovLs ls, double *__restrict__ Xsc,
                                                          unsigned long long *__restrict__ zero_word /* optional:
                                                          cleared here (the posterior's NaN counter), saving a memset */) {
    const int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (zero_word && e == 0) *zero_word = 0ull;
    if (e >= Np * d) return;
    const int64_t n = e / d;
    const int k = (int)(e - n * d);
    Xsc[e] = (n < N) ? X[e] * ls.isc[k] : 0.0;
}

// ---------------------------------------------------------------------------------------------
// Any feature count (d > GPBO_MAX_D): the reference's class is "agnostic to the dimensionality of the feature space"
// (/root/reference/point_selector.py:22, the broadcast at :180-189).  Slow path: coordinates are re-read from memory in
// every distance instead of living in unrolled registers, the length scales come from device memory, exp() is the
// library's.  Same layouts and semantics as kxx_kernel / kstar_mu_kernel; serves the fp64 route (factorise, score).
// ---------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void kxx_anyd_kernel(const double *__restrict__ X, int N, int d,
                                                       const double *__restrict__ il2, double j1, double j2,
                                                       double *__restrict__ K, int Np, double *__restrict__ K2, int ld2,
                                                       int32_t *__restrict__ info0) {
    const int j = blockIdx.x * 256 + threadIdx.x;
    if (info0 && blockIdx.x == 0 && blockIdx.y == 0 && threadIdx.x == 0) *info0 = 0;
    if (j >= Np) return;
    const int i0 = blockIdx.y * 8;
    for (int i = i0; i < i0 + 8; ++i) {
        double v;
        if (i < N) {
            double acc = 0.0;   // cov_r2 / cov_from_r2<SE> of cov_entry.h over a run-time d: the any-d slow path keeps its copy
            if (j < N) {
                for (int k = 0; k < d; ++k) {
                    const double diff = X[(int64_t)j * d + k] - X[(int64_t)i * d + k];
                    acc = fma(diff * diff, il2[k], acc);
                }
            }
            v = exp(-0.5 * acc);
            if (i == j) v = (v + j1) + j2;
            if (j >= N) v = 0.0;
        } else {
            v = (i == j) ? 1.0 : 0.0;
        }
        K[(int64_t)i * Np + j] = v;
        if (K2) {
            K2[(int64_t)i * ld2 + j] = v;
            if (ld2 >= 2 * Np) K2[(int64_t)i * ld2 + Np + j] = 0.0;
        }
    }
}

// grid (used / 256, Np / 64), block 256: thread = one candidate, blockIdx.y = slice of 64 observations
__global__ __launch_bounds__(256) void kstar_mu_anyd_kernel(const double *__restrict__ Xs, int64_t Mc,
                                                            const double *__restrict__ X, int N, int d,
                                                            const double *__restrict__ isc,
                                                            const double *__restrict__ alpha, double diag_add,
                                                            int64_t cand_base, double *__restrict__ KsT, int64_t ldk,
                                                            double *__restrict__ mu_part) {
    const int64_t c = (int64_t)blockIdx.x * 256 + threadIdx.x;
    const int n0 = blockIdx.y * KS_SLICE;
    const bool valid = c < Mc;
    double mu = 0.0;
    for (int n = n0; n < n0 + KS_SLICE; ++n) {
        double kv = 0.0;
        if (n < N && valid) {
            double t = 0.0;
            for (int k = 0; k < d; ++k) {
                const double df = (Xs[c * d + k] - X[(int64_t)n * d + k]) * isc[k];   // NaN coordinates poison the row
                t = fma(df, df, t);
            }
            kv = exp(-t);
            if (diag_add != 0.0 && (int64_t)n == cand_base + c) kv += diag_add;
            mu = fma(kv, alpha[n], mu);
        }
        KsT[(int64_t)n * ldk + c] = kv;
    }
    mu_part[(int64_t)blockIdx.y * ldk + c] = mu;
}

// length-scale factors of an any-d call in a stream-ordered device allocation: [0, d) = 1 / ls^2, [d, 2 d) = 1 / (ls sqrt 2)
static int make_ls_anyd(const double *ls_host, int d, hipStream_t st, double **dev_out) {
    if (!ls_host || d < 1 || d > GPBO_MAX_D_ANY) return GPBO_ERR_ARG;
    std::vector<double> h(2 * (size_t)d);
    if (!length_scale_scalings(ls_host, d, h.data(), h.data() + d)) return GPBO_ERR_ARG;
    double *p = nullptr;
    if (hipMallocAsync(reinterpret_cast<void **>(&p), sizeof(double) * 2 * d, st) != hipSuccess) return GPBO_ERR_LAUNCH;
    // (pageable source: the runtime stages the bytes before the call returns, so `h` may go out of scope)
    if (hipMemcpyAsync(p, h.data(), sizeof(double) * 2 * d, hipMemcpyHostToDevice, st) != hipSuccess ||
        hipStreamSynchronize(st) != hipSuccess) {
        (void)hipFreeAsync(p, st);
        return GPBO_ERR_LAUNCH;
    }
    *dev_out = p;
    return GPBO_OK;
}

int gpbo_kstar_mu_anyd(const double *Xs, int64_t Mc, const double *X, int64_t N, int64_t Np, int32_t d, const double *ls_host,
                       const double *alpha, double diag_add, int64_t cand_base, double *KsT, int64_t ldk, double *mu_part,
                       void *stream) {
    if (!Xs || !X || !alpha || !KsT || !mu_part) return GPBO_ERR_ARG;
    if (Mc < 1 || N < 1 || Np < N || Np % 128 != 0 || ldk % GPBO_CHUNK_GRANULE != 0 || Mc > ldk) return GPBO_ERR_ARG;
    hipStream_t st = gpbo_stream(stream);
    double *lsd = nullptr;
    int rc = make_ls_anyd(ls_host, d, st, &lsd);
    if (rc != GPBO_OK) return rc;
    const int64_t used = round_up_granule(Mc);
    hipLaunchKernelGGL(kstar_mu_anyd_kernel, dim3((unsigned)(used / 256), (unsigned)(Np / KS_SLICE)), dim3(256), 0, st, Xs, Mc, X,
                       (int)N, (int)d, lsd + d, alpha, diag_add, cand_base, KsT, ldk, mu_part);
    const bool ok = hipGetLastError() == hipSuccess;
    (void)hipFreeAsync(lsd, st);
    return ok ? GPBO_OK : GPBO_ERR_LAUNCH;
}

static int make_ls(const double *ls_host, int d, CovLs *out) {
    if (!ls_host || d < 1 || d > GPBO_MAX_D) return GPBO_ERR_ARG;
    for (int k = 0; k < GPBO_MAX_D; ++k) out->il2[k] = out->isc[k] = 0.0;
    return length_scale_scalings(ls_host, d, out->il2, out->isc) ? GPBO_OK : GPBO_ERR_ARG;
}

int gpbo_kxx_launch(const double *X, int64_t N, int32_t d, const double *ls_host, int32_t kernel, double jitter1,
                    double jitter2, double *Kp, int64_t Np, double *K2, int64_t ld2, int32_t *info0, void *stream) {
    if (!X || !Kp || N < 1 || Np < N || Np % 64 != 0 || Np > (1 << 20)) return GPBO_ERR_ARG;
    if (!kernel_ok(kernel, d)) return GPBO_ERR_ARG;
    if (K2 && (ld2 < Np || ld2 > (1 << 21))) return GPBO_ERR_ARG;
    if (d > GPBO_MAX_D) {  // any feature count: the slow path
        hipStream_t st = gpbo_stream(stream);
        double *lsd = nullptr;
        int rc0 = make_ls_anyd(ls_host, d, st, &lsd);
        if (rc0 != GPBO_OK) return rc0;
        dim3 g((unsigned)((Np + 255) / 256), (unsigned)(Np / 8));
        hipLaunchKernelGGL(kxx_anyd_kernel, g, dim3(256), 0, st, X, (int)N, (int)d, lsd, jitter1, jitter2, Kp, (int)Np, K2,
                           (int)ld2, info0);
        const bool ok = hipGetLastError() == hipSuccess;
        (void)hipFreeAsync(lsd, st);
        return ok ? GPBO_OK : GPBO_ERR_LAUNCH;
    }
    CovLs ls;
    int rc = make_ls(ls_host, d, &ls);
    if (rc != GPBO_OK) return rc;
    dim3 grid((unsigned)((Np + 255) / 256), (unsigned)(Np / 8));
#define KXX_LAUNCH(DD, KK)                                                                                                   \
    hipLaunchKernelGGL((kxx_kernel<DD, KK>), grid, dim3(256), 0, gpbo_stream(stream), X, (int)N, ls, jitter1, jitter2, Kp, (int)Np, \
                       K2, (int)ld2, info0)
#define CALL(DD)                                                                  \
    if (kernel == GPBO_KERNEL_MATERN32) KXX_LAUNCH(DD, GPBO_KERNEL_MATERN32);     \
    else if (kernel == GPBO_KERNEL_MATERN52) KXX_LAUNCH(DD, GPBO_KERNEL_MATERN52); \
    else KXX_LAUNCH(DD, GPBO_KERNEL_SE)
    GPBO_FOR_D(d, CALL)
#undef CALL
#undef KXX_LAUNCH
    GPBO_CHECK_LAUNCH();
    return GPBO_OK;
}

extern "C" int gpbo_kxx_f64(const double *X, int64_t N, int32_t d, const double *ls_host, double jitter1,
                            double jitter2, double *Kp, int64_t Np, void *stream) {
    return gpbo_kxx_kern_f64(X, N, d, ls_host, GPBO_KERNEL_SE, jitter1, jitter2, Kp, Np, stream);
}

extern "C" int gpbo_kxx_kern_f64(const double *X, int64_t N, int32_t d, const double *ls_host, int32_t kernel, double jitter1,
                                 double jitter2, double *Kp, int64_t Np, void *stream) {
    return gpbo_kxx_launch(X, N, d, ls_host, kernel, jitter1, jitter2, Kp, Np, nullptr, 0, nullptr, stream);
}

int gpbo_scale_points_launch(const double *X, int64_t N, int64_t Np, int32_t d, const double *ls_host, double *Xsc,
                             unsigned long long *zero_word, void *stream) {
    if (!X || !Xsc || N < 1 || Np < N) return GPBO_ERR_ARG;
    CovLs ls;
    int rc = make_ls(ls_host, d, &ls);
    if (rc != GPBO_OK) return rc;
    const int64_t tot = Np * d;
    hipLaunchKernelGGL(scale_points_kernel, dim3((unsigned)((tot + 255) / 256)), dim3(256), 0, gpbo_stream(stream), X, N,
                       Np, (int)d, ls, Xsc, zero_word);
    GPBO_CHECK_LAUNCH();
    return GPBO_OK;
}

extern "C" int gpbo_scale_points_f64(const double *X, int64_t N, int64_t Np, int32_t d, const double *ls_host,
                                     double *Xsc, void *stream) {
    return gpbo_scale_points_launch(X, N, Np, d, ls_host, Xsc, nullptr, stream);
}

extern "C" int gpbo_kstar_mu_f64(const double *Xs, int64_t Mc, const double *Xsc, int64_t N, int64_t Np, int32_t d,
                                 const double *ls_host, const double *alpha, double diag_add, int64_t cand_base,
                                 double *KsT, int64_t ldk, double *mu_part, void *stream) {
    return gpbo_kstar_mu_kern_f64(Xs, Mc, Xsc, N, Np, d, ls_host, GPBO_KERNEL_SE, alpha, diag_add, cand_base, KsT, ldk, mu_part,
                                  stream);
}

extern "C" int gpbo_kstar_mu_kern_f64(const double *Xs, int64_t Mc, const double *Xsc, int64_t N, int64_t Np, int32_t d,
                                      const double *ls_host, int32_t kernel, const double *alpha, double diag_add,
                                      int64_t cand_base, double *KsT, int64_t ldk, double *mu_part, void *stream) {
    // GPBO_KSTAR_BESIDE=1: this stand-alone entry launches the co-resident form (tests and A/B runs compare it with the shipped one)
    static const bool beside_env = env_flag("GPBO_KSTAR_BESIDE");
    return gpbo_kstar_mu_rows(Xs, Mc, Xsc, N, Np, d, ls_host, kernel, alpha, diag_add, cand_base, KsT, ldk, mu_part, Np, beside_env,
                              stream);
}

// The co-resident form of kstar_mu_kernel (BESIDE) exists for the feature counts at which the 64-register cap costs no spill and
// no scratch (hipcc -Rpass-analysis=kernel-resource-usage; DESIGN.md 8b lists them), for the squared exponential without the
// N == M quirk, with fp64 stores.
constexpr int KSTAR_BESIDE_MAX_D = 9;
static int compute_units() {
    int dev = 0, cus = 0;
    if (hipGetDevice(&dev) != hipSuccess || hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess) return 0;
    return cus;
}
// ... and a launch is bounded to one workgroup per compute unit only while its candidate blocks (512 candidates each) are no more
// than the compute units: a larger chunk keeps the in-order path
bool gpbo_kstar_beside_ok(int32_t d, int32_t kernel, double diag_add, int64_t chunk) {
    return d >= 1 && d <= KSTAR_BESIDE_MAX_D && kernel == GPBO_KERNEL_SE && diag_add == 0.0 &&
           round_up_granule(chunk) / 512 <= compute_units();
}

namespace {
template <int DD>
void launch_kstar_beside(bool nt, dim3 grid, hipStream_t st, const double *Xs, int64_t Mc, const double *Xsc, int N, const CovLs &ls,
                         const double *alpha, int64_t cand_base, double *KsT, int64_t ldk, double *mu_part, int store_rows,
                         int nslices) {
    if constexpr (DD <= KSTAR_BESIDE_MAX_D) {
        if (nt)
            hipLaunchKernelGGL((kstar_mu_kernel<DD, 0, false, true, double, true>), grid, dim3(256), 0, st, Xs, Mc, Xsc, N, ls,
                               alpha, 0.0, cand_base, KsT, ldk, mu_part, store_rows, nslices);
        else
            hipLaunchKernelGGL((kstar_mu_kernel<DD, 0, false, true, double, false>), grid, dim3(256), 0, st, Xs, Mc, Xsc, N, ls,
                               alpha, 0.0, cand_base, KsT, ldk, mu_part, store_rows, nslices);
    }
}
}  // namespace

// store_rows: only rows n < store_rows of K*^T are written (a multiple of 64; Np = everything); the mean partials always
// cover all N observations.
// beside != 0: the co-resident form where gpbo_kstar_beside_ok() says it exists (the same bits), the shipped form elsewhere.
int gpbo_kstar_mu_rows(const double *Xs, int64_t Mc, const double *Xsc, int64_t N, int64_t Np, int32_t d,
                       const double *ls_host, int32_t kernel, const double *alpha, double diag_add, int64_t cand_base,
                       double *KsT, int64_t ldk, double *mu_part, int64_t store_rows, int beside, void *stream) {
    if (!Xs || !Xsc || !alpha || !KsT || !mu_part) return GPBO_ERR_ARG;
    if (!kernel_ok(kernel, d, diag_add)) return GPBO_ERR_ARG;
    if (store_rows < 0 || store_rows > Np || store_rows % KS_SLICE) return GPBO_ERR_ARG;
    if (Mc < 1 || N < 1 || Np < N || Np % 128 != 0 || ldk % GPBO_CHUNK_GRANULE != 0 || Mc > ldk)
        return GPBO_ERR_ARG;
    CovLs ls;
    int rc = make_ls(ls_host, d, &ls);
    if (rc != GPBO_OK) return rc;
    const int64_t used = round_up_granule(Mc);
    dim3 grid((unsigned)(used / 512), (unsigned)(Np / KS_SLICE));
    const int nslices = (int)(Np / KS_SLICE);
    // Timing-only variants (1 = no stores, 3 = stores with a trivial body; wrong results) exist only in a diagnostics
    // build (GPBO_DIAG=1 bayesian_optimisation_amd/csrc/build.sh); the shipped library has no switch into them.
#ifdef GPBO_DIAGNOSTICS
    static const int variant = env_int("GPBO_KSTAR_VARIANT", 0);
#else
    constexpr int variant = 0;
#endif
    const bool nt = (int64_t)sizeof(double) * store_rows * ldk > ((int64_t)1 << 30);  // slab beyond what the Infinity Cache keeps
    if (beside && variant == 0 && gpbo_kstar_beside_ok(d, kernel, diag_add, Mc)) {
        // one workgroup per compute unit at the most (see kstar_mu_kernel): the slices are dealt out over cus / nbx rows of them
        int gy = (int)(compute_units() / (used / 512));
        if (gy > nslices) gy = nslices;
#ifdef GPBO_BESIDE_FULL_GRID   // (A/B builds: every slice its own workgroup, the unbounded grid of DESIGN.md 8b)
        gy = nslices;
#endif
        const dim3 gb((unsigned)(used / 512), (unsigned)gy);
#define CALL(DD)                                                                                                        \
    launch_kstar_beside<DD>(nt, gb, gpbo_stream(stream), Xs, Mc, Xsc, (int)N, ls, alpha, cand_base, KsT, ldk, mu_part, \
                            (int)store_rows, nslices)
        GPBO_FOR_D(d, CALL)
#undef CALL
        GPBO_CHECK_LAUNCH();
        return GPBO_OK;
    }
#define KSTAR_LAUNCH1(DD, V, H, NTF)                                                                                  \
    hipLaunchKernelGGL((kstar_mu_kernel<DD, V, H, false, double, NTF>), grid, dim3(256), 0, gpbo_stream(stream), Xs, Mc, Xsc, (int)N, \
                       ls, alpha, diag_add, cand_base, KsT, ldk, mu_part, (int)store_rows, nslices)
#define KSTAR_LAUNCH(DD, V, H) \
    do { if (nt) KSTAR_LAUNCH1(DD, V, H, true); else KSTAR_LAUNCH1(DD, V, H, false); } while (0)
#define KSTAR_MATERN1(DD, NTF, KK)                                                                                                \
    hipLaunchKernelGGL((kstar_mu_kernel<DD, 0, false, false, double, NTF, KK>), grid, dim3(256), 0, gpbo_stream(stream), Xs, Mc, Xsc, (int)N, \
                       ls, alpha, 0.0, cand_base, KsT, ldk, mu_part, (int)store_rows, nslices)
#define KSTAR_MATERN(DD, KK) \
    do { if (nt) KSTAR_MATERN1(DD, true, KK); else KSTAR_MATERN1(DD, false, KK); } while (0)
#ifdef GPBO_DIAGNOSTICS
#define CALL(DD)                                                                    \
    if (kernel == GPBO_KERNEL_MATERN32) KSTAR_MATERN(DD, GPBO_KERNEL_MATERN32);     \
    else if (kernel == GPBO_KERNEL_MATERN52) KSTAR_MATERN(DD, GPBO_KERNEL_MATERN52); \
    else if (diag_add != 0.0) KSTAR_LAUNCH(DD, 0, true);                            \
    else if (variant == 1) KSTAR_LAUNCH(DD, 1, false);                              \
    else if (variant == 3) KSTAR_LAUNCH(DD, 3, false);                              \
    else KSTAR_LAUNCH(DD, 0, false)
#else
#define CALL(DD)                                                                    \
    if (kernel == GPBO_KERNEL_MATERN32) KSTAR_MATERN(DD, GPBO_KERNEL_MATERN32);     \
    else if (kernel == GPBO_KERNEL_MATERN52) KSTAR_MATERN(DD, GPBO_KERNEL_MATERN52); \
    else if (diag_add != 0.0) KSTAR_LAUNCH(DD, 0, true);                            \
    else KSTAR_LAUNCH(DD, 0, false)
#endif
    (void)variant;
    GPBO_FOR_D(d, CALL)
#undef CALL
    GPBO_CHECK_LAUNCH();
    return GPBO_OK;
}

// Same build with K*^T stored in fp32 (rows of `ldk` floats, Np rows, Np a multiple of 64) and the mean partials in
// fp64: the front end of the fp32 variance screen (posterior_f32.hip).
int gpbo_kstar_mu_mixed(const double *Xs, int64_t Mc, const double *Xsc, int64_t N, int64_t Np, int32_t d,
                        const double *ls_host, const double *alpha, double diag_add, int64_t cand_base, float *KsT,
                        int64_t ldk, double *mu_part, void *stream) {
    if (!Xs || !Xsc || !alpha || !KsT || !mu_part) return GPBO_ERR_ARG;
    if (Mc < 1 || N < 1 || Np < N || Np % KS_SLICE != 0 || ldk % GPBO_CHUNK_GRANULE != 0 || Mc > ldk) return GPBO_ERR_ARG;
    CovLs ls;
    int rc = make_ls(ls_host, d, &ls);
    if (rc != GPBO_OK) return rc;
    const int64_t used = round_up_granule(Mc);
    dim3 grid((unsigned)(used / 512), (unsigned)(Np / KS_SLICE));
    const bool nt = (int64_t)sizeof(float) * Np * ldk > ((int64_t)1 << 30);
#define CALL(DD)                                                                                                     \
    if (diag_add != 0.0)                                                                                             \
        hipLaunchKernelGGL((kstar_mu_kernel<DD, 0, true, false, float, false>), grid, dim3(256), 0, gpbo_stream(stream), Xs, Mc,  \
                           Xsc, (int)N, ls, alpha, diag_add, cand_base, KsT, ldk, mu_part, (int)Np, (int)(Np / KS_SLICE));                 \
    else if (nt)                                                                                                     \
        hipLaunchKernelGGL((kstar_mu_kernel<DD, 0, false, false, float, true>), grid, dim3(256), 0, gpbo_stream(stream), Xs, Mc,  \
                           Xsc, (int)N, ls, alpha, diag_add, cand_base, KsT, ldk, mu_part, (int)Np, (int)(Np / KS_SLICE));                 \
    else                                                                                                             \
        hipLaunchKernelGGL((kstar_mu_kernel<DD, 0, false, false, float, false>), grid, dim3(256), 0, gpbo_stream(stream), Xs, Mc, \
                           Xsc, (int)N, ls, alpha, diag_add, cand_base, KsT, ldk, mu_part, (int)Np, (int)(Np / KS_SLICE))
    GPBO_FOR_D(d, CALL)
#undef CALL
    GPBO_CHECK_LAUNCH();
    return GPBO_OK;
}
