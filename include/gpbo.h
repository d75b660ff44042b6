/*
 * gpbo.h - C ABI of libgpbo: the MI355X (gfx950) GP-surrogate acquisition path.
 *
 * The reference has no FFI: its boundary is the Python attribute protocol between
 * select_parameters.py:146-157 / 282-293 and class PointSelector (point_selector.py:13-207).
 * bayesian_optimisation_amd.PointSelector keeps that protocol and binds the entry points below
 * through ctypes.  Each entry point names the reference code it replaces.
 *
 * Conventions
 *   - every pointer is a DEVICE pointer unless its name ends in _host; all buffers are
 *     caller-allocated and caller-owned, nothing is retained across calls;
 *   - `stream` is a hipStream_t passed as void* (NULL = the default stream); calls only enqueue
 *     work on it and never synchronise, so they may be captured into a hipGraph;
 *   - matrices are row-major fp64; observation-sized dimensions are padded to
 *     Np = gpbo_padded_n(N) (a multiple of 128): the padding carries the identity in K/L/U and
 *     zeros in y/alpha, so results on the leading N entries are those of the unpadded problem;
 *   - return value: GPBO_OK or a negative GPBO_ERR_* (no exceptions cross the ABI).  Numerical
 *     failures that are only known on the device (non-positive Cholesky pivot, NaN acquisition)
 *     are reported through the device-side `info` / `result` words the caller reads back.
 */
#ifndef GPBO_H
#define GPBO_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define GPBO_VERSION 151 /* 0.5.1 (symbols added since, backward compatible: gpbo_ehvi_acq_f64 / gpbo_ehvi_acq_host_f64, two-objective expected hypervolume improvement in log space; gpbo_constrained_acq_f64 / gpbo_constrained_acq_host_f64, constrained expected improvement, probability of improvement and probability of feasibility in log space; gpbo_mes_log_survival_f64 / gpbo_mes_acq_f64 / gpbo_mes_log_survival_host_f64 / gpbo_mes_acq_host_f64, max-value entropy search on the dense posterior; gpbo_nei_fantasies_workspace_bytes / gpbo_nei_fantasies_f64 / gpbo_posterior_nei_workspace_bytes / gpbo_posterior_nei_kern_f64 / gpbo_nei_host_f64, noisy expected improvement; gpbo_kxx_kern_f64 / gpbo_kstar_mu_kern_f64 / gpbo_factorise_kern_f64 / gpbo_posterior_acq_kern_f64 / gpbo_nlml_grad_kern_f64 / gpbo_nlml_hyper_kern_f64 / gpbo_select_next_host_kern_f64 / gpbo_nlml_grad_host_kern_f64 / gpbo_nlml_hyper_host_kern_f64, the Matern 3/2 and 5/2 covariance families on the fp64 path; gpbo_nlml_hyper_workspace_bytes / gpbo_nlml_hyper_f64 / gpbo_nlml_hyper_host_f64 / gpbo_loo_workspace_bytes / gpbo_loo_f64, the likelihood over noise, signal variance and mean with the length scales, and leave-one-out prediction; gpbo_thompson_weights_workspace_bytes / gpbo_thompson_weights_f64 / gpbo_thompson_paths_workspace_bytes / gpbo_thompson_paths_f64 / gpbo_thompson_host_f64, Thompson sampling by pathwise posterior samples; gpbo_posterior_grad_workspace_bytes / gpbo_posterior_grad_f64 / gpbo_refine_workspace_bytes / gpbo_refine_f64 / gpbo_refine_host_f64, acquisition gradients and off-grid refinement; gpbo_batch_workspace_bytes / gpbo_select_batch_f64 / gpbo_select_batch_host_f64, greedy q-point batch selection; gpbo_nlml_grad_workspace_bytes / gpbo_nlml_grad_f64 / gpbo_nlml_grad_host_f64, the likelihood gradient for ML-II length-scale fitting): + gpbo_nlml_grid_wave_f64 / _wave_logdet_f64 (the likelihood grid of N <= 64 observations, a wave per cell); 0.5.0: the likelihood grid of any N in one launch (one workgroup per cell), a second likelihood mode (log det from the factor: gpbo_nlml_grid_*logdet*) */

/* Environment switches the SHIPPED library reads (each once per process; none changes a result beyond the rounding of a
 * different summation order, none is needed for normal use - they select between measured alternatives for A/B runs):
 *   GPBO_F64_GROUPS=g     column groups of the fp64 variance kernel for large calls (default 8: one per XCD)
 *   GPBO_OVERLAP=0        never build K(X*,X) of chunk c + 1 on a second stream beside the variance launch of chunk c (the default
 *                         does where the co-resident K(X*,X) form exists - d <= 9, squared exponential - and the call takes the
 *                         grouped variance launch: -1.0 % per headline step); any other value: for every call of several chunks
 *   GPBO_KSTAR_BESIDE=1   gpbo_kstar_mu_f64 / gpbo_kstar_mu_kern_f64 launch the co-resident form (the same bits; tests, A/B runs)
 *   GPBO_PREFIX_VALU=1    the prefix bound's first-level mean from the difference-form kernel instead of the MFMA one
 *   GPBO_FACTOR_OLD=1     the round-2 factorisation chain (Cholesky + triangular inverse) instead of the fused sweep
 *   GPBO_NO_LOOKAHEAD=1   that chain without its helper stream
 *   GPBO_CI_OPTS=a,b,c,d  launch-plan options of the fused sweep (csrc/cholinv_plan.h)
 * Read only by DIAGNOSTICS builds (-DGPBO_DIAGNOSTICS: tools/build_variant.sh, never the shipped library; some produce
 * wrong results on purpose to time a phase): GPBO_KSTAR_VARIANT, GPBO_SIGMA_VARIANT, GPBO_CI_STAMPS, GPBO_FPS_MUTE (fault
 * injection), GPBO_FPS_SHAPE, and the compile-time GPBO_ARD_SKIP / GPBO_ARD_STAMPS of csrc/ard.hip. */

#define GPBO_OK 0
#define GPBO_ERR_ARG (-1)      /* null pointer, bad size/alignment, unsupported d */
#define GPBO_ERR_LAUNCH (-2)   /* HIP reported a launch/runtime error */
#define GPBO_ERR_WORKSPACE (-3) /* workspace too small */

#define GPBO_MAX_D 16          /* compile-time-unrolled feature counts 1..16 (every route) */
#define GPBO_MAX_D_ANY 1024    /* fp64 route only (kxx, factorise, posterior_acq_f64, select_next_host): any d up to this, slow path */
#define GPBO_NPAD 128          /* observation padding granule (column-block width of the variance kernel) */
#define GPBO_CHUNK_GRANULE 512 /* candidate-chunk granule */
#define GPBO_CHUNK_MAX (1 << 24) /* largest chunk (16-row tile offsets inside K*^T are 32-bit element offsets) */

/* Covariance families (the `kernel` argument of the gpbo_*_kern_f64 entry points; every other entry is the squared exponential).
 * r^2 = sum_k (x_k - x'_k)^2 / ls_k^2 with the ARD length scales; all three have unit prior variance, k(x, x) = 1 exactly. */
#define GPBO_KERNEL_SE 0       /* k = exp(-r^2 / 2): the reference's kernel_rbf (point_selector.py:166-195) */
#define GPBO_KERNEL_MATERN32 1 /* a = sqrt(3) r, k = (1 + a) exp(-a)             (not in the reference) */
#define GPBO_KERNEL_MATERN52 2 /* a = sqrt(5) r, k = (1 + a + a^2 / 3) exp(-a)   (not in the reference) */

#define GPBO_ACQ_LCB 0 /* acq = p0*sigma - mu            (point_selector.py:204, p0 = explore) */
#define GPBO_ACQ_EI 1  /* acq = EI for minimisation, p0 = f_best, p1 = xi (not in the reference) */

/* Result record written by gpbo_posterior_acq_f64 (device memory, 32 bytes). */
typedef struct gpbo_result {
    double best_val;   /* max acquisition over the candidates given to this call          */
    int64_t best_idx;  /* LOWEST global index attaining it (point_selector.py:207 tie rule) */
    int64_t nan_count; /* number of candidates whose acquisition is NaN (reference: IndexError) */
    int64_t reserved;
} gpbo_result;

/* Optional timing of the dominant kernel (sigma/acquisition) and of the K(X*,X) build: hipEvents recorded on
 * the caller's stream by gpbo_posterior_acq_f64 when a profile is passed.  The launches of one call form a chain
 * K*(0), variance(0), K*(1), variance(1), ... on one stream, so one event per boundary serves as the end of one
 * launch and the beginning of the next (an event record costs a few microseconds of idle GPU).  Host-side object. */
typedef struct gpbo_profile {
    int32_t capacity, count;
    void **begin, **end;   /* hipEvent_t before / after each variance/acquisition launch */
    int64_t *cands;        /* candidates processed by each recorded launch */
    void **kbegin;         /* hipEvent_t before the K(X*,X) launch of the slot (used when kmode == 1) */
    int32_t *kmode;        /* K(X*,X) launch of the slot: 0 not timed, 1 kbegin[i]..begin[i], 2 end[i-1]..begin[i] */
    void **qend;           /* gpbo_posterior_qei_f64: hipEvent_t after the qEI launch of the slot (end[i]..qend[i]) */
    int32_t *qmode;        /* 1: the slot has a qEI interval */
} gpbo_profile;
int gpbo_profile_create(int32_t capacity, gpbo_profile **out);
void gpbo_profile_reset(gpbo_profile *p);
/* Waits for the recorded events; sums elapsed ms, launches and candidates over all recorded launches. */
int gpbo_profile_read(gpbo_profile *p, double *total_ms_host, int64_t *launches_host, int64_t *cands_host);
/* Same for the K(X*,X) launches (fp64 path). */
int gpbo_profile_read_kstar(gpbo_profile *p, double *total_ms_host, int64_t *launches_host, int64_t *cands_host);
/* Same for the qEI launches (gpbo_posterior_qei_f64 with a profile). */
int gpbo_profile_read_qei(gpbo_profile *p, double *total_ms_host, int64_t *launches_host, int64_t *cands_host);
void gpbo_profile_destroy(gpbo_profile *p);

int gpbo_version(void);
const char *gpbo_strerror(int status);
int64_t gpbo_padded_n(int64_t N);

/* K1 - replaces kernel_rbf(X, X) + jitter assembly (point_selector.py:166-195 with :79, :116).
 * Kp[Np x Np]: leading N x N = exp(-1/2 sum_k (x_ik-x_jk)^2 / ls_k^2), diagonal = (1 + jitter1) + jitter2
 * (the reference adds 1e-4 inside kernel_rbf and 1e-6 at assembly, in that order); padding = identity.
 * X: [N x d] row-major, ls: [d] length scales (kernel_params). */
int gpbo_kxx_f64(const double *X, int64_t N, int32_t d, const double *ls_host, double jitter1, double jitter2,
                 double *Kp, int64_t Np, void *stream);

/* K4 - replaces np.linalg.inv(cov_meas) (point_selector.py:89) by a blocked right-looking Cholesky.
 * In place: lower triangle of Kp becomes L (upper triangle is left untouched). dinv [Np/64][64][64]
 * receives the inverses of the diagonal blocks of L. info (device int32): 0, or 1-based column of the
 * first non-positive / non-finite pivot.  Np: any multiple of 64. */
int gpbo_potrf_f64(double *Kp, int64_t Np, double *dinv, int32_t *info, void *stream);

/* U = (L^-1)^T, upper triangular, [Np x Np] row-major (strict lower triangle zero-filled).
 * work: Np*Np doubles. Together with gpbo_potrf_f64 this is the factorisation the posterior uses. */
int gpbo_trtri_f64(const double *L, const double *dinv, int64_t Np, double *U, double *work, void *stream);

/* K4, round 3 - the same inverse (point_selector.py:89) in ONE sweep: fused Cholesky + inverse factor by row
 * operations on the stacked matrix S = [A | W], [Np x ld] row-major with ld >= 2 Np (csrc/cholinv.hip).
 * In: columns [0, Np) = the symmetric positive definite matrix (both triangles), columns [Np, 2 Np) = zeros.
 * Out: columns [Np, 2 Np) = inv(L), lower triangular (U of gpbo_trtri_f64 is its transpose); the upper block triangle
 * of columns [0, Np) holds L^T except on its 128 x 128 diagonal blocks, which keep their last Schur complements.
 * info as gpbo_potrf_f64.  Np: a multiple of 128.  opt: NULL, or int32[7] {win, far_k, far_kind (3: 128 x 128 tiles,
 * 4: 256 x 128), defer + 1, max_launches, group_from + 1, small_w (64 or 32)}, 0 = default: schedule choices (csrc/cholinv_plan.h) and, for tests, the
 * first max_launches launches of the plan only.  The first call for a size uploads its plan (synchronous). */
int gpbo_cholinv_f64(double *S, int64_t ld, int64_t Np, int32_t *info, const int32_t *opt, void *stream);
/* The launch plan of gpbo_cholinv_f64 as data (no GPU needed; tests/test_cholinv_plan_cpu.py executes it with NumPy).
 * opt: as above (max_launches ignored).  *n_launch / *n_tile: in = capacity of launches[] / tiles[] in entries (ignored
 * when the array is NULL), out = entries of the plan.  launches: 5 words each {pair or -1, workgroups of PAIR(pair),
 * first tile, tiles, tiles per workgroup}; tiles: 8 words each {kind (2: 64 x w, 3: 128 x 128, 4: 256 x 128), k0, K, row0, col0, r1, wlim, w (kind 2: 64 or 32)}:
 * S[row0.., col0..] -= sum over source rows [k0, k0 + K) of S[k, row0..]^T S[k, col0..], rows < r1, live columns only. */
int gpbo_cholinv_plan(int64_t Np, const int32_t *opt, int64_t *n_launch, int64_t *n_tile, int32_t *launches, int32_t *tiles);
/* One launch = the PAIR workgroups of `pair` (< 0: none) + the given tiles (host array, format above; `group`
 * consecutive tiles per workgroup), `reps` times;
 * synchronous.  For tests of a tile kind by itself and tools/bench_ci_jobs.py.  info is not cleared here. */
int gpbo_cholinv_tiles_f64(double *S, int64_t ld, int64_t Np, int32_t *info, int32_t pair, const int32_t *tiles,
                           int64_t ntile, int32_t group, int32_t reps, void *stream);

/* alpha = K^-1 y = U (U^T y)   (point_selector.py:90 `inv @ measured_vals`).
 * y: [N]; alpha: [Np] (zero on the padding); tmp: [Np]. */
int gpbo_alpha_f64(const double *U, const double *y, int64_t N, int64_t Np, double *tmp, double *alpha,
                   void *stream);

/* One call = kxx + cholinv + transpose + alpha (round 2: kxx + potrf + trtri + alpha).  work: gpbo_factorise_workspace_bytes(Np) bytes.
 * Outputs: Kp keeps K (the reference's `cov_meas`, point_selector.py:79; L lives in the workspace),
 * U [Np x Np], alpha [Np], info (device int32, as gpbo_potrf_f64). */
int64_t gpbo_factorise_workspace_bytes(int64_t Np);
int gpbo_factorise_f64(const double *X, const double *y, int64_t N, int32_t d, const double *ls_host,
                       double jitter1, double jitter2, int64_t Np, double *Kp, double *U, double *alpha,
                       int32_t *info, void *work, int64_t work_bytes, void *stream);

/* Append one observation to an existing factorisation in O(N^2) instead of refactorising (SURVEY.md §8f rank 4:
 * consecutive BO iterations differ by one observed row, select_parameters.py:163,299, while
 * point_selector.py:89 inverts the whole matrix again).  Valid only while the length scales and jitters are
 * those the factors were built with.  In place, N -> N+1:
 *   X [>= N+1 rows x d], y [>= N+1]: row N receives x_new / y_new (device pointers to d and 1 doubles);
 *   U [Np x Np]: column N is written (U' = [U, -U l/lambda; 0, 1/lambda], l = U^T k, lambda^2 = K_NN - l.l);
 *   alpha [Np]: recomputed as U'(U'^T y');   Kp [Np x Np] or NULL: row and column N of K.
 * Needs N + 1 <= Np (Np a multiple of 64; the caller re-pads into larger buffers when the padding is used up:
 * identity on the new diagonal).  info (device int32): 0, or N+1 when the new pivot is not positive - U and alpha are
 * then unchanged (the surrogate of the N old observations stays valid) and the caller refactorises.  work: gpbo_append_workspace_bytes(Np).
 * (To FANTASISE observations - a batch of q points chosen one after the other - gpbo_select_batch_f64 below is the cheaper
 * way: it updates a dense posterior in O(N) per candidate and member and leaves the factorisation alone.) */
int64_t gpbo_append_workspace_bytes(int64_t Np);
int gpbo_append_f64(double *X, double *y, int64_t N, int32_t d, const double *ls_host, double jitter1,
                    double jitter2, int64_t Np, const double *x_new, const double *y_new, double *Kp, double *U,
                    double *alpha, int32_t *info, void *work, int64_t work_bytes, void *stream);

/* Xsc[Np x d] = X / (ls sqrt 2) (rows >= N zero): the pre-scaled observations gpbo_kstar_mu_f64 reads. */
int gpbo_scale_points_f64(const double *X, int64_t N, int64_t Np, int32_t d, const double *ls_host, double *Xsc,
                          void *stream);

/* K2+K5 - replaces kernel_rbf(X, X*).T and the mean product (point_selector.py:81, :90).
 * Builds the transposed cross-covariance chunk KsT[Np x ldk] (row n = observation n, column c =
 * candidate c of the chunk; rows n >= N are zero) and per-64-observation partial sums of
 * mu_c = sum_n k(x*_c, x_n) alpha_n into mu_part[(Np/64) x ldk].
 * Xs: [Mc x d] candidates of this chunk (unscaled); Xsc: output of gpbo_scale_points_f64;
 * Mc <= ldk, ldk a multiple of 512.
 * diag_add / cand_base: when the caller's full candidate set has the SAME SHAPE as X the reference
 * adds 1e-4 where observation index == global candidate index (point_selector.py:173,191-193);
 * pass diag_add = 0 otherwise. */
int gpbo_kstar_mu_f64(const double *Xs, int64_t Mc, const double *Xsc, int64_t N, int64_t Np, int32_t d,
                      const double *ls_host, const double *alpha, double diag_add, int64_t cand_base,
                      double *KsT, int64_t ldk, double *mu_part, void *stream);

/* K5..K8, whole candidate set of this rank: chunks of `chunk` candidates through gpbo_kstar_mu_f64 and
 * the fused sigma/acquisition/argmax kernel (point_selector.py:90-98, :204-207).
 *   sigma_c = sqrt(|prior_var - |U^T k_c|^2|)     (abs and sqrt as at :98; "cov_func" is a std-dev)
 *   acq_c   = LCB or EI;  result = first-index argmax over c in [0, M), reported as idx_offset + c.
 * mu_out / sigma_out / acq_out: optional dense [M] outputs (NULL to skip).
 * work: gpbo_posterior_workspace_bytes(Np, chunk, M) bytes. */
int64_t gpbo_posterior_workspace_bytes(int64_t Np, int64_t chunk, int64_t M);
int gpbo_posterior_acq_f64(const double *Xs, int64_t M, const double *X, int64_t N, int64_t Np, int32_t d,
                           const double *ls_host, const double *U, const double *alpha, double prior_var,
                           int32_t acq_kind, double p0, double p1, double diag_add, int64_t idx_offset,
                           int64_t chunk, double *mu_out, double *sigma_out, double *acq_out,
                           gpbo_result *result, void *work, int64_t work_bytes, gpbo_profile *prof /* or NULL */,
                           void *stream);

/* q = 8 Monte-Carlo Expected Improvement over consecutive batches of 8 candidates (BASELINE config 5; not in the
 * reference).  qEI_b = mean_s max(0, max_j(f_best - xi - (mu_b + chol(Sigma_b) z_s)_j)); Z: [S x 8] fixed base
 * samples (device); M a multiple of 8 (chunks must not split a batch: chunk is a multiple of 512).
 * result.best_idx = batch_offset + index of the first batch attaining the maximum; qei_out: optional [M/8]. */
int64_t gpbo_qei_workspace_bytes(int64_t Np, int64_t chunk, int64_t M);
int gpbo_posterior_qei_f64(const double *Xs, int64_t M, const double *X, int64_t N, int64_t Np, int32_t d,
                           const double *ls_host, const double *U, const double *alpha, double prior_var, double f_best,
                           double xi, const double *Z, int32_t S, int64_t batch_offset, int64_t chunk, double *qei_out,
                           gpbo_result *result, void *work, int64_t work_bytes, gpbo_profile *prof /* or NULL */,
                           void *stream);

/* fp32-screened scoring (BASELINE config 4).  The factorisation stays fp64; U is rounded to fp32 once per step
 * (gpbo_prepare_f32, re-padded to Np32 = gpbo_padded_n_f32(N), a multiple of 256; alpha32 may be NULL).
 * gpbo_posterior_acq_f32 = the screen over all M candidates: K(X*,X) entries and the mean in fp64 exactly as in the
 * fp64 path (mu_out is the fp64 path's mean bit for bit), K*^T stored in fp32, the N^2-per-candidate triangular
 * product on the fp32 matrix cores.  Dense outputs are doubles holding fp32-accurate values; var_out is the signed
 * prior_var - |v|^2 the screen decides on.  alpha: the fp64 alpha of the factorisation.  chunk: a multiple of 1024.
 * result: the screen's own arg-max (NOT final - see gpbo_rescore_f64). */
int64_t gpbo_padded_n_f32(int64_t N);
int gpbo_prepare_f32(const double *U, const double *alpha, int64_t Np, float *U32, float *alpha32, int64_t Np32,
                     void *stream);
int64_t gpbo_posterior_workspace_bytes_f32(int64_t Np32, int64_t chunk, int64_t M);
int gpbo_posterior_acq_f32(const double *Xs, int64_t M, const double *X, int64_t N, int64_t Np32, int32_t d,
                           const double *ls_host, const float *U32, const double *alpha, double prior_var,
                           int32_t acq_kind, double p0, double p1, double diag_add, int64_t idx_offset, int64_t chunk,
                           double *mu_out, double *sigma_out, double *acq_out, double *var_out, gpbo_result *result,
                           void *work, int64_t work_bytes, gpbo_profile *prof /* or NULL */, void *stream);

/* The decision behind the screen: the selected point must be the fp64 path's (point_selector.py:204-207: first index
 * of the maximum).  Given the screen's dense mu [M] and var32 [M]: every candidate whose acquisition could still reach
 * the best lower bound when its variance is off by up to tau - plus every sample_stride-th candidate - is gathered and
 * re-scored through the fp64 kernels (gpbo_posterior_acq_f64 on the gathered rows); result = fp64 maximum over those,
 * lowest original index on ties, idx_offset added.  tau starts at tau0 and is CHECKED on every call: the largest
 * |var64 - var32| on the re-scored set must stay below tau / 4, else tau is raised and the selection repeated.
 * stats_host->fallback = 1 (result untouched) when more than `cap` candidates survive or tau does not settle in four
 * rounds: the caller then runs gpbo_posterior_acq_f64 over all candidates.  This call synchronises `stream` (it
 * reads the survivor count back); not supported with the N == M diagonal quirk (diag_add != 0: use the fp64 path). */
typedef struct gpbo_screen_stats {
    int64_t survivors; /* candidates selected in the last round (may exceed cap when fallback is set) */
    int64_t rescored;  /* candidates pushed through the fp64 kernels, all rounds */
    int32_t rounds;
    int32_t fallback;
    double tau;        /* variance tolerance of the last round */
    double err_max;    /* largest |sigma64^2 - |var32|| seen on the last round's re-scored set */
} gpbo_screen_stats;
int64_t gpbo_rescore_workspace_bytes(int64_t Np, int64_t cap, int64_t chunk64);
int gpbo_rescore_f64(const double *Xs, int64_t M, const double *mu, const double *var32, const double *X, int64_t N,
                     int64_t Np, int32_t d, const double *ls_host, const double *U, const double *alpha,
                     double prior_var, int32_t acq_kind, double p0, double p1, int64_t idx_offset, double tau0,
                     int64_t sample_stride, int64_t cap, int64_t chunk64, gpbo_result *result,
                     gpbo_screen_stats *stats_host, void *work, int64_t work_bytes, void *stream);

/* Prefix-bound screen: exact branch and bound, everything in fp64 (csrc/sigma_acq.hip, csrc/rescore.hip).
 * |U^T k_c|^2 summed over the FIRST n_prefix components is a lower bound of the whole sum - it is the variance reduction
 * from the first n_prefix observations alone - so  sigma_ub = sqrt(|prior_var - partial|) >= cov_func_c  and, both
 * acquisitions being increasing in sigma (LCB for explore >= 0), acq_ub_c >= acq_func_eval_c (point_selector.py:98,204).
 * gpbo_posterior_prefix_f64: one pass over all candidates - the mean over all N observations (exactly the fp64 path's),
 * the variance product over the first n_prefix columns only ((n_prefix / Np)^2 of the work; n_prefix a multiple of 128).
 * Same workspace as gpbo_posterior_acq_f64; `result` receives the arg-max of the BOUNDS (not the answer).
 * gpbo_bound_select_f64: the strided sample goes through the fp64 kernels (a lower bound of the maximum), every
 * candidate whose bound reaches it survives and is re-scored by the fp64 kernels, which decide (maximum, lowest index,
 * NaN count as the plain pass); too many survivors -> stats->fallback = 1 and the caller runs gpbo_posterior_acq_f64.
 * work: gpbo_rescore_workspace_bytes(Np, cap, chunk64).  This call synchronises the stream.
 * When the bound is one: U, X, alpha must be ONE factorisation (the same the plain pass would use): the bound's |v[:J]|^2 is
 * then a partial sum of the squares gpbo_posterior_acq_f64 adds up.  The plain pass takes sqrt(|var|) (point_selector.py:98),
 * and a NEGATIVE computed variance - possible only when its rounding error exceeds the jitter tau of K = k(X,X) + tau I,
 * since the true variance is >= tau for prior_var >= 1 + tau - is the one value a prefix cannot bound: callers take this route
 * for tau >= 1e-6 (DeviceGP.BOUND_MIN_JITTER, gpbo_select_next_host_f64) and the plain pass otherwise. */
int gpbo_posterior_prefix_f64(const double *Xs, int64_t M, const double *X, int64_t N, int64_t Np, int32_t d,
                              const double *ls_host, const double *U, const double *alpha, double prior_var,
                              int32_t acq_kind, double p0, double p1, int64_t idx_offset, int64_t chunk, int64_t n_prefix,
                              double *mu_out, double *sigma_ub_out, double *acq_ub_out, gpbo_result *result, void *work,
                              int64_t work_bytes, gpbo_profile *prof /* or NULL */, void *stream);
int gpbo_bound_select_f64(const double *Xs, int64_t M, const double *acq_ub, const double *X, int64_t N, int64_t Np,
                          int32_t d, const double *ls_host, const double *U, const double *alpha, double prior_var,
                          int32_t acq_kind, double p0, double p1, int64_t idx_offset, int64_t sample_stride, int64_t cap,
                          int64_t chunk64, int64_t n_prefix2 /* 0, or a longer prefix (multiple of 128) that tightens the
                          bounds of the survivors before they are re-scored */, gpbo_result *result,
                          gpbo_screen_stats *stats_host, void *work, int64_t work_bytes, void *stream);

/* Order independence of that bound (csrc/subset.hip; version 140, replaces the gpbo_*_subset_f64 calls of 130): which
 * observations come FIRST decides how much the prefix prunes, and a history sorted along an axis or started inside one
 * cluster is a bad prefix.  gpbo_fps_order_f64 writes a permutation of the observations - J members by farthest-point
 * sampling in length-scale units (first member: the observation farthest from the centroid; then the one farthest from
 * the members so far; ties to the lowest index), then every other observation in index order - and gathers X / y in that
 * order.  The caller factorises the PERMUTED problem (a GP's posterior does not depend on the order of its observations:
 * same mean_func / cov_func within rounding, point_selector.py:89-98) and runs every pass - gpbo_posterior_acq_f64 as
 * well as the two calls above - on that one factorisation, so the bound's |v[:J]|^2 is a partial sum of the squares the
 * plain pass itself adds up, whatever the history.
 * perm_out [N] int64, Xp_out [N x d], yp_out [N] (both optional; y may be NULL when yp_out is): device memory;
 * 1 <= J <= N, d <= GPBO_MAX_D; work: gpbo_fps_order_workspace_bytes(N) bytes, 256-byte aligned. */
int64_t gpbo_fps_order_workspace_bytes(int64_t N);
int gpbo_fps_order_f64(const double *X, const double *y, int64_t N, int32_t d, const double *ls_host, int64_t J,
                       int64_t *perm_out, double *Xp_out, double *yp_out, void *work, int64_t work_bytes, void *stream);
/* The selection runs on up to 16 co-operating workgroups that wait for each other with BOUNDED polls; should one of them
 * never be scheduled the others give up after about a second and the ARRIVAL order is installed (exact as well, it only
 * prunes less).  gpbo_fps_order_status writes 1 into *fell_back (device int32) when the last gpbo_fps_order_f64 on this
 * workspace ended that way, else 0 - a caller whose peers must hold the same factorisation (candidate shards) checks it. */
int gpbo_fps_order_status(const void *work, int64_t N, int32_t *fell_back, void *stream);

/* int8-sliced variance screen (Ozaki-style splitting on the integer matrix cores, csrc/ozaki.hip): same role and
 * outputs as gpbo_posterior_acq_f32 - mean exactly the fp64 path's, variance from 20 exact int8 slice products
 * (|dsigma| ~ 1e-10 at N = 4096), decision by gpbo_rescore_f64 - at N <= GPBO_I8_MAX_N (int32 accumulators).
 * gpbo_prepare_i8: once per factorisation, U -> column scales + int8 MFMA fragments in `u8`
 * (gpbo_prepare_i8_bytes(Np) bytes, 256-byte aligned).  chunk: a multiple of 512.  No N == M diagonal quirk. */
#define GPBO_I8_MAX_N 16384
int64_t gpbo_prepare_i8_bytes(int64_t Np);
int gpbo_prepare_i8(const double *U, int64_t Np, void *u8, int64_t u8_bytes, void *stream);
int64_t gpbo_posterior_workspace_bytes_i8(int64_t Np, int64_t chunk, int64_t M);
int gpbo_posterior_acq_i8(const double *Xs, int64_t M, const double *X, int64_t N, int64_t Np, int32_t d,
                          const double *ls_host, const void *u8, const double *alpha, double prior_var,
                          int32_t acq_kind, double p0, double p1, int64_t idx_offset, int64_t chunk, double *mu_out,
                          double *sigma_out, double *acq_out, double *var_out, gpbo_result *result, void *work,
                          int64_t work_bytes, gpbo_profile *prof /* or NULL */, void *stream);
/* Coarse variant of the same screen: the three leading digits of both operands, SIX slice products, 256-row tiles
 * (|dsigma^2| ~ 2e-4 at N = 4096: start gpbo_rescore_f64 with tau0 ~ 1e-3).  Same arguments, buffers and workspace
 * size as gpbo_posterior_acq_i8 (it reads slices 0-2 of the same `u8`); the mean is still the fp64 path's. */
int gpbo_posterior_acq_i8c(const double *Xs, int64_t M, const double *X, int64_t N, int64_t Np, int32_t d,
                           const double *ls_host, const void *u8, const double *alpha, double prior_var,
                           int32_t acq_kind, double p0, double p1, int64_t idx_offset, int64_t chunk, double *mu_out,
                           double *sigma_out, double *acq_out, double *var_out, gpbo_result *result, void *work,
                           int64_t work_bytes, gpbo_profile *prof /* or NULL */, void *stream);

/* K7+K8 on a posterior already on the device: acq = LCB/EI of (mu, sigma), first-index arg-max
 * (point_selector.py:204-207).  Used for a second acquisition on the same surrogate.
 * work: gpbo_acq_workspace_bytes() bytes, 256-byte aligned. */
int64_t gpbo_acq_workspace_bytes(void);
int gpbo_acq_argmax_f64(const double *mu, const double *sigma, int64_t M, int32_t acq_kind, double p0, double p1,
                        int64_t idx_offset, double *acq_out, gpbo_result *result, void *work, int64_t work_bytes,
                        void *stream);

/* Greedy q-point batch selection by rank-one posterior updates (csrc/batch.hip; not in the reference, which
 * selects one point per iteration).  Member 0 is the arg-max of the posterior as given; every further member is the arg-max
 * after conditioning the GP on a FANTASY observation y_j at the member before it, members chosen so far excluded:
 *   t_j(c) = k(c, x_j) - k_c . beta_j - sum_{i<j} t_i(c) t_i(x_j) / s_i,   beta_j = U (U^T k(X, x_j))
 *   s_j = var_j(x_j) - prior_var + ((1 + jitter1) + jitter2);  var'(c) = var(c) - t_j(c)^2 / s_j;  mu'(c) = mu(c) + t_j(c) (y_j - mu(x_j)) / s_j
 * N kernel entries per candidate and member instead of the N^2 of a variance pass; the factorisation (U, alpha, X) is only
 * read.  GPBO_FANTASY_BELIEVER: y_j = the current mean at x_j (Kriging believer; GP-BUCB under LCB: only the variance
 * shrinks); GPBO_FANTASY_LIE: y_j = lie (constant liar).
 *   mu / sigma [M]: IN the dense outputs of gpbo_posterior_acq_f64 for the same Xs (diag_add = 0; the variance state is
 *     sigma^2), OUT the posterior the q-th member was chosen from;
 *   idx_out [q]: the members in selection order as idx_offset + row of Xs (the first equals the plain pass's arg-max);
 *     val_out [q]: their acquisition values at selection time;
 *   result: the record of the last member, nan_count = the largest NaN count of any step.  nan_count > 0 (the caller raises):
 *     every LATER member is -1 (value NaN);  info (device int32): 0, or the 1-based member whose s_j was not positive or not
 *     finite - that member's successors are -1 as well, mu / sigma stay as they were before the failed step;
 *   alpha: the factorisation's (not read today: the mean arrives in mu; kept with the model's other arguments);
 *   1 <= q <= GPBO_BATCH_MAX_Q, q <= M, d <= GPBO_MAX_D, Np = gpbo_padded_n(N); work: gpbo_batch_workspace_bytes(Np, M, q)
 *   bytes (negative: invalid sizes), 256-byte aligned.  Enqueues only, never synchronises; no atomics in the sums: two
 *   calls give the same bits.
 * gpbo_select_batch_host_f64: factorisation + plain pass + selection on host arrays (conventions of
 *   gpbo_select_next_host_f64; idx_out_host / val_out_host [q], mu_out_host / sigma_out_host optional [M]; info_host: the
 *   failing pivot of the factorisation - then every member is -1 - or the failing member as above). */
#define GPBO_BATCH_MAX_Q 64
#define GPBO_FANTASY_BELIEVER 0 /* y_j = the current mean at x_j */
#define GPBO_FANTASY_LIE 1      /* y_j = lie */
int64_t gpbo_batch_workspace_bytes(int64_t Np, int64_t M, int32_t q);
int gpbo_select_batch_f64(const double *Xs, int64_t M, const double *X, int64_t N, int64_t Np, int32_t d,
                          const double *ls_host, const double *U, const double *alpha, double jitter1, double jitter2,
                          double prior_var, int32_t acq_kind, double p0, double p1, int32_t q, int32_t fantasy, double lie,
                          double *mu /* in/out [M] */, double *sigma /* in/out [M] */, int64_t idx_offset,
                          int64_t *idx_out /* [q] */, double *val_out /* [q] */, gpbo_result *result, int32_t *info,
                          void *work, int64_t work_bytes, void *stream);
int gpbo_select_batch_host_f64(const double *X_host, const double *y_host, int64_t N, int32_t d, const double *ls_host,
                               double jitter1, double jitter2, const double *Xs_host, int64_t M, int32_t acq_kind,
                               double p0, double p1, int64_t chunk, int32_t q, int32_t fantasy, double lie,
                               int64_t *idx_out_host, double *val_out_host, double *mu_out_host, double *sigma_out_host,
                               gpbo_result *result_host, int32_t *info_host);

/* Acquisition gradients and off-grid refinement of selected points (csrc/refine.hip; not in the reference, which
 * answers with one of the candidates it was given).  For a query point x, k_n = k(x, X_n), g_nk = (X_nk - x_k) / ls_k^2:
 *   mu = sum_n k_n alpha_n, dmu_k = sum_n k_n alpha_n g_nk;  v = U^T k, var = prior_var - |v|^2, w = U v,
 *   dvar_k = -2 sum_n k_n w_n g_nk;  sigma = sqrt(|var|), dsigma_k = sign(var) dvar_k / (2 sigma) (0 when sigma == 0);
 *   LCB: dacq = p0 dsigma - dmu;  EI: dacq = -Phi(z) dmu + phi(z) dsigma (sigma == 0: -dmu if imp > 0, else 0).
 * gpbo_posterior_grad_f64: value and gradient at the P rows of Xq [P x d] (not candidates: no diag_add); mu_out / sigma_out /
 *   acq_out [P] and dmu_out / dsigma_out / dacq_out [P x d], each optional.  A row with a non-finite coordinate gives NaN
 *   in every output.  Four launches: K(Xq, X) point-major, the two dense products with U on the matrix cores, the sums.
 * gpbo_refine_f64: projected gradient ascent of the acquisition inside the box [lower, upper], every start on its own:
 *   x <- clip(start), (f, g) there, acq0 = f, t <- step0 / max_k(|g_k| ls_k) (frozen when that is 0 or not finite);
 *   iters times: x' = clip(x + t g ls^2); accepted iff x' != x, f' finite and f' >= f + 1e-4 sum_k g_k (x'_k - x_k) - then
 *   (x, f, g) <- (x', f', g'), t <- 2 t - else t <- t / 2.
 *   Xq [P x d]: IN the starts, OUT the refined points;  acq_out / acq0_out / pg_out (double) and accepted_out (int32), [P],
 *   each optional: the final value, the value at the clipped start, the projected-gradient norm
 *   max_k |x_k - clip(x_k + g_k ls_k^2)| / ls_k, the number of accepted steps;  result: the largest final value, the LOWEST
 *   start attaining it, nan_count = starts whose acq0 is NaN (such a start never moves and reports NaN; the caller raises).
 *   All iters + 1 evaluations are enqueued without a host round trip; no atomics, no random numbers: two calls give the
 *   same bits.
 * 1 <= P <= GPBO_REFINE_MAX_P, 1 <= d <= GPBO_MAX_D, Np = gpbo_padded_n(N), ls > 0, finite lower <= upper, 0 <= iters <= 1000,
 *   finite step0 > 0, U 16-byte aligned (GPBO_ERR_ARG otherwise, before any launch);  work: gpbo_posterior_grad_workspace_bytes(Np, P) /
 *   gpbo_refine_workspace_bytes(Np, P) bytes (negative: invalid sizes), 256-byte aligned (GPBO_ERR_WORKSPACE).
 * gpbo_refine_host_f64: factorisation + refinement on host arrays (conventions of gpbo_select_batch_host_f64: X, y, N, d,
 *   ls, jitter1, jitter2; prior_var = (1 + jitter1) + jitter2);  Xq_host [P x d] in / out, the four optional [P] host
 *   outputs;  info_host: 0, or the failing pivot of the factorisation - then nothing is refined and best_idx = -1. */
#define GPBO_REFINE_MAX_P 4096
int64_t gpbo_posterior_grad_workspace_bytes(int64_t Np, int64_t P);
int gpbo_posterior_grad_f64(const double *Xq, int64_t P, const double *X, int64_t N, int64_t Np, int32_t d,
                            const double *ls_host, const double *U, const double *alpha, double prior_var, int32_t acq_kind,
                            double p0, double p1, double *mu_out, double *sigma_out, double *acq_out /* [P] */,
                            double *dmu_out, double *dsigma_out, double *dacq_out /* [P x d] */, void *work,
                            int64_t work_bytes, void *stream);
int64_t gpbo_refine_workspace_bytes(int64_t Np, int64_t P);
int gpbo_refine_f64(double *Xq /* in: starts, out: refined points [P x d] */, int64_t P, const double *lower_host,
                    const double *upper_host, const double *X, int64_t N, int64_t Np, int32_t d, const double *ls_host,
                    const double *U, const double *alpha, double prior_var, int32_t acq_kind, double p0, double p1,
                    int32_t iters, double step0, double *acq_out, double *acq0_out, int32_t *accepted_out, double *pg_out,
                    gpbo_result *result, void *work, int64_t work_bytes, void *stream);
int gpbo_refine_host_f64(const double *X_host, const double *y_host, int64_t N, int32_t d, const double *ls_host,
                         double jitter1, double jitter2, double *Xq_host /* in / out [P x d] */, int64_t P,
                         const double *lower_host, const double *upper_host, int32_t acq_kind, double p0, double p1,
                         int32_t iters, double step0, double *acq_out_host, double *acq0_out_host,
                         int32_t *accepted_out_host, double *pg_out_host, gpbo_result *result_host, int32_t *info_host);

/* Thompson sampling by pathwise posterior samples (csrc/thompson.hip; not in the reference, whose acquisitions
 * are functions of (mean_func, cov_func)).  Pathwise conditioning (Wilson et al. 2020) writes a sample of the posterior
 * FUNCTION as
 *   f_s(x) = g_s(x) + sum_n k0(x, x_n) v_s[n],   g_s(x) = sqrt(2 / F) sum_f W[s,f] cos(2 pi t_f(x)),
 *   t_f(x) = sum_k Omega[f,k] x_k / (2 pi ls_k) + phase[f] (turns),   v_s = K^-1 (y - g_s(X) - sqrt(kappa) E[s,:]),
 *   kappa = jitter1 + jitter2,  K = k0(X,X) + kappa I (the matrix the factorisation inverts).
 * The random draws are INPUTS (device arrays, as Z is for gpbo_posterior_qei_f64): omega [F x d] unit normal, phase [F]
 * uniform in [0, 1), W [S x F] and E [S x N] unit normal; column n of E belongs to row n of X as given to the call.
 * gpbo_thompson_weights_f64: V [S x Np] = the v_s (zero on the padding) from a factorisation's X, y, U and the jitters it was
 *   made with: g_s(X) by the paths kernel itself, the residual, then the two dense products with U (U U^T = K^-1) on the
 *   matrix cores.  U 16-byte aligned.  Once per factorisation and set of draws.
 * gpbo_thompson_paths_f64: every path at the M rows of Xs in one launch plus a finish; nothing of K(X*,X) is stored, the
 *   N kernel entries and F cosines of a candidate are generated once and shared by all S paths.  The acquisition of path s
 *   is -f_s (the project minimises the objective and maximises acquisitions):
 *   idx_out[s] = idx_offset + the LOWEST row attaining max_c -f_s(c), or -1 when no row is usable; val_out[s] = that maximum
 *   (NaN when none); nan_out[s] = rows whose value is NaN - a row with a non-finite coordinate is NaN in every path and is
 *   never chosen.  f_out: optional dense [S x ldf] (row s = path s, ldf >= M).  V == NULL: the prior paths g_s alone (X is
 *   then not read, but must still be non-null: GPBO_ERR_ARG).  Kernel entries: the fp64 path's own arithmetic - with W = 0, S = 1, V = alpha the output is the mean.
 * 1 <= d <= GPBO_MAX_D, 1 <= F <= GPBO_TS_MAX_FEATURES, 1 <= S <= GPBO_TS_MAX_PATHS, 1 <= M <= 2^31, ls > 0, Np a multiple of
 *   GPBO_NPAD, 1 <= N <= Np (GPBO_ERR_ARG otherwise, before any launch);  work: gpbo_thompson_weights_workspace_bytes(Np, F, S)
 *   / gpbo_thompson_paths_workspace_bytes(Np, M, F, S) bytes (negative: invalid sizes), 256-byte aligned (GPBO_ERR_WORKSPACE).
 *   Both calls only enqueue and never synchronise; sums run in a fixed order and only the integer NaN counters use atomics:
 *   two calls give the same bits.
 * gpbo_thompson_host_f64: factorisation + weights + paths on host arrays (conventions of gpbo_select_batch_host_f64: X, y, N,
 *   d, ls, jitter1, jitter2, Xs, M; the four draw arrays on the host);  idx_out_host / val_out_host / nan_out_host [S],
 *   f_out_host optional [S x M];  info_host: 0, or the failing pivot of the factorisation - then every index is -1. */
#define GPBO_TS_MAX_PATHS 64
#define GPBO_TS_MAX_FEATURES 16384
int64_t gpbo_thompson_weights_workspace_bytes(int64_t Np, int32_t F, int32_t S);
int gpbo_thompson_weights_f64(const double *X, const double *y, int64_t N, int64_t Np, int32_t d, const double *ls_host,
                              const double *U, double jitter1, double jitter2, const double *omega /* [F x d] */,
                              const double *phase /* [F] */, const double *W /* [S x F] */, const double *E /* [S x N] */,
                              int32_t F, int32_t S, double *V /* out [S x Np], zero on the padding */, void *work,
                              int64_t work_bytes, void *stream);
int64_t gpbo_thompson_paths_workspace_bytes(int64_t Np, int64_t M, int32_t F, int32_t S);
int gpbo_thompson_paths_f64(const double *Xs, int64_t M, const double *X, int64_t N, int64_t Np, int32_t d,
                            const double *ls_host, const double *omega, const double *phase, const double *W,
                            const double *V /* [S x Np], or NULL: the prior paths g_s alone */, int32_t F, int32_t S,
                            int64_t idx_offset, double *f_out /* optional [S x ldf] */, int64_t ldf,
                            int64_t *idx_out /* [S] */, double *val_out /* [S] */, int64_t *nan_out /* [S] */, void *work,
                            int64_t work_bytes, void *stream);
int gpbo_thompson_host_f64(const double *X_host, const double *y_host, int64_t N, int32_t d, const double *ls_host,
                           double jitter1, double jitter2, const double *Xs_host, int64_t M, const double *omega_host,
                           const double *phase_host, const double *W_host, const double *E_host, int32_t F, int32_t S,
                           int64_t *idx_out_host, double *val_out_host, int64_t *nan_out_host,
                           double *f_out_host /* optional [S x M] */, int32_t *info_host);

/* ---- Host-pointer entry points: the reference's call sequence on NumPy-style arrays, no device handling by the
 * caller (device buffers and a private stream live inside the call).  What a ctypes stub in the reference binds.
 *
 * gpbo_select_next_host_f64 = PointSelector.update_surrogate() once kernel_params are chosen + the acquisition
 * arg-max (point_selector.py:76-98, 197-207; caller: select_parameters.py:149-158, 285-294):
 *   X [N x d], y [N], ls [d] (kernel_params), Xs [M x d] (predicted_pts, row-major grid) - host, fp64;
 *   jitter1 / jitter2 = 1e-4 / 1e-6 for the reference's arithmetic; acq_kind / p0 / p1 as gpbo_posterior_acq_f64;
 *   diag_add = 1e-4 when Xs has the same shape as X (point_selector.py:173), else 0; chunk = 0 for the default;
 *   mu_out / sigma_out / acq_out: optional host [M] (mean_func, cov_func, acq_func_eval before reshaping);
 *   cov_meas_out: optional host [N x N] (the cov_meas attribute);
 *   result (host): best value, lowest flat index attaining it, NaN count (> 0: the reference raises IndexError);
 *   info (host): 0, or the 1-based failing pivot (the reference's inv() raises LinAlgError or returns garbage) -
 *   then nothing is scored and result->best_idx = -1.
 * gpbo_nlml_grid_host_f64 = tune_kernel()'s float32 likelihood grid (point_selector.py:104-163): ls_cells [G x d]
 *   host, out [G] host float32; any N (the wave-per-cell kernel up to 64 observations, the one-launch workgroup-per-cell
 *   kernel beyond). */
/* (When mu_out, sigma_out and acq_out are all NULL, M >= 32768, N > 896 and the acquisition increases with sigma, the next
 * point is found by branch and bound on the exact prefix bound - gpbo_posterior_prefix_f64 / gpbo_bound_select_f64 below -
 * instead of computing every variance: same index and NaN count, the value within 1e-12 relative of the plain pass.) */
int gpbo_select_next_host_f64(const double *X_host, const double *y_host, int64_t N, int32_t d, const double *ls_host,
                              double jitter1, double jitter2, const double *Xs_host, int64_t M, int32_t acq_kind,
                              double p0, double p1, double diag_add, int64_t chunk, double *mu_out_host,
                              double *sigma_out_host, double *acq_out_host, double *cov_meas_out_host,
                              gpbo_result *result_host, int32_t *info_host);
/* q = 8 Monte-Carlo qEI on host arrays (gpbo_posterior_qei_f64 behind the same device handling): Z_host [S x 8] base
 * samples, M a multiple of 8; qei_out_host optional [M/8]; result->best_idx = first batch with the largest qEI. */
int gpbo_select_qei_host_f64(const double *X_host, const double *y_host, int64_t N, int32_t d, const double *ls_host,
                             double jitter1, double jitter2, const double *Xs_host, int64_t M, double f_best, double xi,
                             const double *Z_host, int32_t S, int64_t chunk, double *qei_out_host,
                             gpbo_result *result_host, int32_t *info_host);
int gpbo_nlml_grid_host_f64(const double *X_host, const double *y_host, int64_t N, int32_t d,
                            const double *ls_cells_host, int64_t G, double jitter, float *out_host);
/* the log-det likelihood mode (gpbo_nlml_grid_batched_logdet_f64) on host arrays: out_host [G] fp64 */
int gpbo_nlml_grid_logdet_host_f64(const double *X_host, const double *y_host, int64_t N, int32_t d,
                                   const double *ls_cells_host, int64_t G, double jitter, double *out_host);

/* K9 - replaces tune_kernel / eval_log_marginal (point_selector.py:104-163): float32 grid of
 * nlml = 0.5 (y^T K^-1 y + log det K + N log 2pi), K = k(X,X) + jitter I, one value per grid cell.
 * ls_cells: [G x d] length scales of each cell (device); out: [G] float32 (device).
 * N <= gpbo_nlml_grid_max_n() (the bordered matrix is factorised in LDS). */
int gpbo_nlml_grid_max_n(void);
int gpbo_nlml_grid_f64(const double *X, const double *y, int64_t N, int32_t d, const double *ls_cells, int64_t G,
                       double jitter, float *out, void *stream);

/* The same grid at the reference's own sizes, N <= gpbo_nlml_grid_wave_max_n() (= 64): one WAVE per cell, the cell's
 * matrix in registers (lane = row), the column steps unrolled with v_readlane broadcasts, y as a right-hand side
 * (csrc/ard_wave.hip; ABI 151).  Same arguments and the same value per cell as gpbo_nlml_grid_f64 up to the rounding
 * of another elimination order; a pivot that is not positive gives NaN (the reference's log(det < 0)).
 * ..._wave_logdet_f64: the second likelihood mode (fp64 output, log det K straight from the factor: see below). */
int gpbo_nlml_grid_wave_max_n(void);
int gpbo_nlml_grid_wave_f64(const double *X, const double *y, int64_t N, int32_t d, const double *ls_cells, int64_t G,
                            double jitter, float *out, void *stream);
int gpbo_nlml_grid_wave_logdet_f64(const double *X, const double *y, int64_t N, int32_t d, const double *ls_cells,
                                   int64_t G, double jitter, double *out, void *stream);

/* The same grid for ANY N, one launch: a persistent workgroup per cell runs a left-looking blocked Cholesky of the
 * cell's K (entries generated on the fly, the factor kept in MFMA fragment order in a scratch slot of the workspace,
 * y carried as one more row so that y^T K^-1 y = |L^-1 y|^2).  Same value per cell as gpbo_nlml_grid_f64 up to the
 * rounding of a blocked elimination order.  work: ..._workspace_bytes(N, G), 256-byte aligned.
 *
 * Two likelihood modes (INTEGRATION.md "ARD likelihood modes"):
 *   gpbo_nlml_grid_batched_f64         the REFERENCE's value: float32, log det K evaluated as log(exp(logdet)) because
 *                                      point_selector.py:118 takes np.log(np.linalg.det(K)) - det underflows to 0 beyond
 *                                      N ~ 100 and the cell becomes -inf (reproduced on purpose: parity);
 *   gpbo_nlml_grid_batched_logdet_f64  a documented DEPARTURE for the sizes where that is useless: fp64 output,
 *                                      log det K = 2 sum log L_ii straight from the factor (finite at any N), NaN when a
 *                                      pivot is not positive.  Any N >= 1 (small N included). */
int64_t gpbo_nlml_grid_batched_workspace_bytes(int64_t N, int64_t G);
int gpbo_nlml_grid_batched_f64(const double *X, const double *y, int64_t N, int32_t d, const double *ls_cells,
                               int64_t G, double jitter, float *out, void *work, int64_t work_bytes, void *stream);
int gpbo_nlml_grid_batched_logdet_f64(const double *X, const double *y, int64_t N, int32_t d, const double *ls_cells,
                                      int64_t G, double jitter, double *out, void *work, int64_t work_bytes,
                                      void *stream);

/* One cell of the same grid for any N, from a factorisation made with (jitter1, jitter2) = (1e-4, 0):
 * log det K = -2 sum log U_ii, y^T K^-1 y = y . alpha; NaN when info != 0 (the reference's log of a negative det). */
int gpbo_nlml_cell_f64(const double *U, const double *alpha, const double *y, int64_t N, int64_t Np,
                       const int32_t *info, float *out, void *stream);

/* ML-II length-scale fitting (not in the reference: point_selector.py:30 / :33 declare `hyperparam_obj` and `gradient_steps`
 * for a gradient fit that was never built).  From a factorisation of K = K0 + jitter I made by gpbo_factorise_f64 with
 * (jitter1, jitter2) = (jitter, 0) - U, alpha, info - and the same X [N x d] (device), y, ls_host:
 *   out[0]     = NLML = 1/2 (y . alpha + log det K + N log 2 pi), log det K = -2 sum log U_ii (the "logdet" likelihood)
 *   out[1 + k] = dNLML / dlog ls_k = 1/2 sum_ij W_ij K0_ij (x_ik - x_jk)^2 / ls_k^2,   W = K^-1 - alpha alpha^T
 * out: [1 + d] doubles, device; all NaN when info != 0.  K^-1 = U U^T is never formed: its lower block triangle is
 * produced 64 x 64 tile by tile on the matrix cores and consumed in registers (csrc/ard_grad.hip).  The sum is reduced in
 * a fixed order (no atomics): two calls give the same bits.  Np = gpbo_padded_n(N), 1 <= d <= GPBO_MAX_D, ls > 0;
 * work: gpbo_nlml_grad_workspace_bytes(Np, d) bytes (negative: invalid sizes), 16-byte aligned.
 * gpbo_nlml_grad_host_f64: factorisation + gradient on host arrays in one call (device buffers inside the call). */
int64_t gpbo_nlml_grad_workspace_bytes(int64_t Np, int32_t d);
int gpbo_nlml_grad_f64(const double *U, const double *alpha, const double *y, const double *X, int64_t N, int64_t Np,
                       int32_t d, const double *ls_host, const int32_t *info, double *out, void *work, int64_t work_bytes,
                       void *stream);
int gpbo_nlml_grad_host_f64(const double *X_host, const double *y_host, int64_t N, int32_t d, const double *ls_host,
                            double jitter, double *out_host);

/* ML-II over ALL hyperparameters (ard="hyper"; not in the reference, whose model is frozen at unit signal variance, zero mean and a
 * diagonal term of 1e-4 + 1e-6: point_selector.py:78-79, :193).  Model: y ~ N(m 1, s^2 Kt), Kt = K0(ls) + noise I, noise > 0 the
 * noise-to-signal ratio; mean and scale are profiled out in closed form, so the optimiser sees log ls and log noise.  From a
 * factorisation made by gpbo_factorise_f64 with (jitter1, jitter2) = (noise, 0) and the RAW y - U, alpha = a = Kt^-1 y, info -
 * and b = Kt^-1 1 (computed inside the call):
 *   m = (1 . a) / (1 . b) with GPBO_HYPER_MEAN, else 0;  r = y - m;  alpha' = a - m b;
 *   s^2 = (r . alpha') / N with GPBO_HYPER_SCALE, else 1;
 *   out[0]         = L = 1/2 [(r . alpha') / s^2 + N log s^2 + log det Kt + N log 2 pi]
 *   out[1 + k]     = dL / dlog ls_k = 1/2 sum_ij W_ij K0_ij (x_ik - x_jk)^2 / ls_k^2,  W = Kt^-1 - alpha' alpha'^T / s^2,  k < d
 *   out[1 + d]     = dL / dlog noise = 1/2 noise (tr Kt^-1 - |alpha'|^2 / s^2),  tr Kt^-1 = sum_i sum_{j >= i} U_ij^2 over rows i < N
 *   out[2 + d]     = m;   out[3 + d] = s^2
 * out: [d + 4] doubles, device; every entry NaN when *info != 0, when 1 . b is not positive and finite or when s^2 is not (one
 * observation with both flags, a constant y).  alpha_std_out: optional [Np], receives alpha' / s (zero on the padding) - the
 * alpha of a factorisation of (y - m) / s with the same U.  The length-scale gradients come from gpbo_nlml_grad_f64 on
 * (alpha' / s, r / s).  Np = gpbo_padded_n(N), 1 <= d <= GPBO_MAX_D, ls > 0, noise positive and finite, flags a combination of the
 * two bits, U and work 16-byte aligned (GPBO_ERR_ARG otherwise, before any launch);  work: gpbo_nlml_hyper_workspace_bytes(Np, d)
 * bytes (negative: invalid sizes; GPBO_ERR_WORKSPACE when too small).  Enqueues only, never synchronises; no atomics, every sum
 * in a fixed order: two calls give the same bits.
 * gpbo_nlml_hyper_host_f64: factorisation + the above on host arrays in one call (out_host [d + 4]).
 * gpbo_loo_f64: leave-one-out prediction from a factorisation (U, alpha) of y: kappa_i = (K^-1)_ii = sum_{j >= i} U_ij^2,
 *   mu_out[i] = y_i - alpha_i / kappa_i, var_out[i] = scale2 / kappa_i, kinv_diag_out[i] = kappa_i; each output optional [N];
 *   scale2 positive and finite; work: gpbo_loo_workspace_bytes(Np) bytes, 16-byte aligned. */
#define GPBO_HYPER_MEAN 1  /* fit the constant mean m */
#define GPBO_HYPER_SCALE 2 /* fit the signal variance s^2 */
int64_t gpbo_nlml_hyper_workspace_bytes(int64_t Np, int32_t d);
int gpbo_nlml_hyper_f64(const double *U, const double *alpha, const double *y, const double *X, int64_t N, int64_t Np,
                        int32_t d, const double *ls_host, double noise, int32_t flags, const int32_t *info,
                        double *out /* [d + 4] */, double *alpha_std_out /* optional [Np] */, void *work, int64_t work_bytes,
                        void *stream);
int gpbo_nlml_hyper_host_f64(const double *X_host, const double *y_host, int64_t N, int32_t d, const double *ls_host,
                             double noise, int32_t flags, double *out_host /* [d + 4] */);
int64_t gpbo_loo_workspace_bytes(int64_t Np);
int gpbo_loo_f64(const double *U, const double *alpha, const double *y, int64_t N, int64_t Np, double scale2, double *mu_out,
                 double *var_out, double *kinv_diag_out, void *work, int64_t work_bytes, void *stream);

/* ---- The Matern covariance families (not in the reference, whose docs/README.md names them as its first planned improvement).
 * Each entry below is its squared-exponential twin with `int32_t kernel` (GPBO_KERNEL_*) inserted after ls_host; the twin is a
 * one-line forward with GPBO_KERNEL_SE, so kernel = 0 gives the twin's results bit for bit.  Workspaces are those of the twins
 * (the same *_workspace_bytes queries).  With r^2 = sum_k (x_k - x'_k)^2 / ls_k^2:
 *   GPBO_KERNEL_MATERN32   a = sqrt(3) r,  k = (1 + a) exp(-a),             dk / dlog ls_k = 3 exp(-a) (x_k - x'_k)^2 / ls_k^2
 *   GPBO_KERNEL_MATERN52   a = sqrt(5) r,  k = (1 + a + a^2 / 3) exp(-a),   dk / dlog ls_k = 5/3 (1 + a) exp(-a) (x_k - x'_k)^2 / ls_k^2
 * (nothing is divided by r: coincident points need no special case).  Only three kernels evaluate covariance entries - K(X,X),
 * K(X*,X) and the epilogue of the likelihood gradient - so the factorisation, alpha, the variance product, the acquisitions, the
 * arg-max, the profiled mean and scale of gpbo_nlml_hyper_f64 and gpbo_loo_f64 serve every family unchanged.  The diagonal of
 * K(X,X) is (1 + jitter1) + jitter2 as for the squared exponential.
 * Refused with GPBO_ERR_ARG before any HIP call: a kernel id outside {0, 1, 2}; a Matern id with d > GPBO_MAX_D (the any-d slow
 * path is squared-exponential only); a Matern id with diag_add != 0 (the N == M quirk reproduces a shape coincidence of the
 * reference's kernel_rbf and belongs to that kernel alone).  gpbo_select_next_host_kern_f64 with a Matern id always takes the
 * plain pass (the prefix bound builds its mean with squared-exponential entries).  Everything else of the ABI - append, the
 * fp32 / int8 screens, the prefix bound, qEI, batches, Thompson sampling, refinement, the likelihood grids - is
 * squared-exponential only. */
int gpbo_kxx_kern_f64(const double *X, int64_t N, int32_t d, const double *ls_host, int32_t kernel, double jitter1, double jitter2,
                      double *Kp, int64_t Np, void *stream);
int gpbo_kstar_mu_kern_f64(const double *Xs, int64_t Mc, const double *Xsc, int64_t N, int64_t Np, int32_t d,
                           const double *ls_host, int32_t kernel, const double *alpha, double diag_add, int64_t cand_base,
                           double *KsT, int64_t ldk, double *mu_part, void *stream);
int gpbo_factorise_kern_f64(const double *X, const double *y, int64_t N, int32_t d, const double *ls_host, int32_t kernel,
                            double jitter1, double jitter2, int64_t Np, double *Kp, double *U, double *alpha, int32_t *info,
                            void *work, int64_t work_bytes, void *stream);
int gpbo_posterior_acq_kern_f64(const double *Xs, int64_t M, const double *X, int64_t N, int64_t Np, int32_t d,
                                const double *ls_host, int32_t kernel, const double *U, const double *alpha, double prior_var,
                                int32_t acq_kind, double p0, double p1, double diag_add, int64_t idx_offset, int64_t chunk,
                                double *mu_out, double *sigma_out, double *acq_out, gpbo_result *result, void *work,
                                int64_t work_bytes, gpbo_profile *prof /* or NULL */, void *stream);
int gpbo_nlml_grad_kern_f64(const double *U, const double *alpha, const double *y, const double *X, int64_t N, int64_t Np,
                            int32_t d, const double *ls_host, int32_t kernel, const int32_t *info, double *out, void *work,
                            int64_t work_bytes, void *stream);
int gpbo_nlml_hyper_kern_f64(const double *U, const double *alpha, const double *y, const double *X, int64_t N, int64_t Np,
                             int32_t d, const double *ls_host, int32_t kernel, double noise, int32_t flags, const int32_t *info,
                             double *out /* [d + 4] */, double *alpha_std_out /* optional [Np] */, void *work,
                             int64_t work_bytes, void *stream);
int gpbo_select_next_host_kern_f64(const double *X_host, const double *y_host, int64_t N, int32_t d, const double *ls_host,
                                   int32_t kernel, double jitter1, double jitter2, const double *Xs_host, int64_t M,
                                   int32_t acq_kind, double p0, double p1, double diag_add, int64_t chunk, double *mu_out_host,
                                   double *sigma_out_host, double *acq_out_host, double *cov_meas_out_host,
                                   gpbo_result *result_host, int32_t *info_host);
int gpbo_nlml_grad_host_kern_f64(const double *X_host, const double *y_host, int64_t N, int32_t d, const double *ls_host,
                                 int32_t kernel, double jitter, double *out_host);
int gpbo_nlml_hyper_host_kern_f64(const double *X_host, const double *y_host, int64_t N, int32_t d, const double *ls_host,
                                  int32_t kernel, double noise, int32_t flags, double *out_host /* [d + 4] */);

/* ---- The acquisition integrated over the hyperparameter posterior (ard="marginal"; Snoek, Larochelle & Adams 2012; not in the
 * reference).  Two pieces: the likelihood of gpbo_nlml_hyper_f64 at MANY cells in one launch, which a sampler of exp(-L) drives, and
 * the scoring of candidates under an ensemble of the sampled models.
 *
 * gpbo_nlml_hyper_cells_f64 (csrc/hyper_wave.hip): cells [G x (d + 1)] doubles on the device, row g = (ls_1 ... ls_d, rho);
 *   out [G x 3] doubles on the device, row g = (L, m, s^2) with the meaning of out[0], out[2 + d], out[3 + d] of
 *   gpbo_nlml_hyper_f64 at (ls, noise = rho); no gradient.  One wave per cell, the cell's matrix in registers:
 *   1 <= N <= GPBO_HYPER_CELLS_MAX_N, 1 <= d <= GPBO_MAX_D, 1 <= G <= 2^28, kernel a GPBO_KERNEL_*, flags a combination of
 *   GPBO_HYPER_MEAN | GPBO_HYPER_SCALE (GPBO_ERR_ARG otherwise, before any launch).  A row is NaN in all three entries when a pivot
 *   of K0(ls) + rho I is not positive and finite, when 1 . Kt^-1 1 is not or when s^2 is not; the other rows do not see it.
 *   y: the profile is formed from y . Kt^-1 y, 1 . Kt^-1 y and 1 . Kt^-1 1, which cancels like (mean / sd)^2 of the y passed in:
 *   with GPBO_HYPER_MEAN pass y - mean(y) and add the shift back to m (L and s^2 do not see it).  Enqueues only; no atomics: two
 *   launches give the same bits.
 *
 * gpbo_ensemble_acq_f64 (csrc/ensemble.hip): S models that share (X, N, d, kernel) score M candidates in one call.
 *   U [S][Np][Np] and alpha [S][Np]: model s as gpbo_factorise_kern_f64 writes it for ((y - m_s) / s_s, ls_s, jitter1 = rho_s,
 *   jitter2 = 0);  ls_host [S x d];  model_host [S x 4] = (weight w_s >= 0, prior_var = 1 + rho_s, y_mean m_s, y_scale s_s > 0);
 *   p0, p1: the acquisition parameters in the units of y (LCB: explore, -; EI: f_best, xi).
 *   For each model in index order the fp64 pass of gpbo_posterior_acq_kern_f64 writes the model's dense mu, sigma into the
 *   workspace and one kernel folds them, with mu_y = m_s + s_s mu, sigma_y = s_s sigma and shift = sum_s w_s m_s, into
 *       acq += w_s acquisition(kind, mu_y, sigma_y, p0, p1),   dm += w_s (mu_y - shift),   dv += w_s (sigma_y^2 + (mu_y - shift)^2)
 *   after the last model: mean_out = shift + dm, sd_out = sqrt(max(dv - dm^2, 0)), acq_out = acq (each optional, [M]) and the
 *   first arg-max of acq over the candidates that are not NaN (result->nan_count counts those that are; ties to the lower index).
 *   Every sum in a fixed order, nothing atomic but that count: the same bits from call to call and for any chunk.
 *   1 <= S <= GPBO_ENSEMBLE_MAX_S, 1 <= d <= GPBO_MAX_D, Np = gpbo_padded_n(N), chunk as for gpbo_posterior_acq_f64, weights
 *   finite and >= 0 with a positive sum, y_scale and prior_var positive and finite, U 16-byte aligned (GPBO_ERR_ARG otherwise,
 *   before any launch);  work: gpbo_ensemble_workspace_bytes(Np, chunk, M) bytes (negative: invalid sizes), 256-byte aligned
 *   (GPBO_ERR_WORKSPACE).  Enqueues only; info of the factorisations is the caller's to check. */
#define GPBO_HYPER_CELLS_MAX_N 64
#define GPBO_ENSEMBLE_MAX_S 64
int gpbo_nlml_hyper_cells_f64(const double *X, const double *y, int64_t N, int32_t d, const double *cells /* [G x (d + 1)] */,
                              int64_t G, int32_t kernel, int32_t flags, double *out /* [G x 3] */, void *stream);
int64_t gpbo_ensemble_workspace_bytes(int64_t Np, int64_t chunk, int64_t M);
int gpbo_ensemble_acq_f64(const double *Xs, int64_t M, const double *X, int64_t N, int64_t Np, int32_t d, int32_t S,
                          const double *ls_host /* [S x d] */, int32_t kernel, const double *U /* [S][Np][Np] */,
                          const double *alpha /* [S][Np] */, const double *model_host /* [S x 4] */, int32_t acq_kind, double p0,
                          double p1, int64_t idx_offset, int64_t chunk, double *mean_out, double *sd_out, double *acq_out,
                          gpbo_result *result, void *work, int64_t work_bytes, void *stream);

/* ---- Noisy expected improvement: EI averaged over fantasies of the incumbent (csrc/nei.hip; Letham, Karrer, Ottoni &
 * Bakshy 2019; not in the reference).  Everything in the units of the model.  rho = jitter1 + jitter2 of the factorisation (U,
 * K~ = K0 + rho I), 0 < delta <= rho the nugget of the noise-free TWIN: a second factorisation of the same X, ls and kernel with
 * jitters (delta, 0), of which K0d (its Kp = K0 + delta I) and U0 (U0 U0^T = K0d^-1) are used.
 *
 * gpbo_nei_fantasies_f64: S samples of the latent function at the observed points from the posterior.  Z, E [S x N] unit normal
 *   draws (device; column n belongs to row n of the factorised X), noise_sd = sqrt(rho - delta):
 *     B_s = U0 z_s,  g_s = K0d B_s,  r_s = y - g_s - noise_sd e_s,  A_s = B_s + K~^-1 r_s,  F_s = K0d A_s,  best_s = min_{i < N} F_s[i]
 *   (cov g = K0d exactly and K0d^-1 g_s = B_s by construction: no solve with the ill-conditioned K0d).  F_s has mean K0d K~^-1 y and
 *   covariance K0d - K0d K~^-1 K0d; with rho = delta every F_s is y.  A_out, F_out [S x Np] (zero on the padding), best_out [S].
 *   Five dense products of [64 x Np] with [Np x Np] on the matrix cores; the minimum does not read the padding.
 * gpbo_posterior_nei_kern_f64: NEI(x) = (1 / S) sum_s EI(mu_s(x), sigma_0(x); best_s, xi) over the M rows of Xs, with
 *   mu_s(x) = k(x) . A_s and sigma_0 the variance pass of gpbo_posterior_acq_kern_f64 on U0 with prior_var (= 1 + delta), EI as
 *   GPBO_ACQ_EI; first arg-max, NaN rule and tie rule as every other acquisition (a candidate with a NaN coordinate counts once
 *   in nan_count and is never chosen).  The means come from the K(X*,X)^T image the pass has built for its variance launch, read
 *   once, all S of them on the matrix cores: about one EI pass whatever S, and no covariance entry of its own - every
 *   kernel family.  A [S x Np] and best [S]: device (best need not be the row minima).  mu_out: optional dense [S x ldm],
 *   ldm >= M; sigma_out, acq_out: optional [M].  The sums run in a fixed order, k ascending in one wave: the same bits from call
 *   to call, and means that do not depend on the chunk.  sigma_0 comes from one call of the pass per chunk, which chooses the
 *   column groups of its variance kernel by the candidates of that call: the same bits for any chunk except across the line of
 *   32,768 candidates per chunk at N > 1,920, where it differs by the rounding of another summation order.
 * 1 <= S <= GPBO_NEI_MAX_S, 1 <= d <= GPBO_MAX_D, Np = gpbo_padded_n(N), chunk as for gpbo_posterior_acq_f64, ls > 0, prior_var
 *   positive and finite, xi and noise_sd finite, noise_sd >= 0, K0d / U0 / U 16-byte aligned (GPBO_ERR_ARG otherwise, before any HIP
 *   call);  work: gpbo_nei_fantasies_workspace_bytes(Np, S) / gpbo_posterior_nei_workspace_bytes(Np, chunk, M, S) bytes (negative:
 *   invalid sizes), 256-byte aligned (GPBO_ERR_WORKSPACE).  Both calls only enqueue; only the integer NaN counter is atomic.
 * gpbo_nei_host_f64: both factorisations + fantasies + scoring on host arrays (conventions of gpbo_select_next_host_kern_f64: X,
 *   y, N, d, ls, kernel, jitter1, jitter2, Xs, M, chunk = 0 for the default);  Z_host, E_host [S x N];  best_in_host: NULL for
 *   the row minima, or [S] incumbents to use instead;  mu_out_host optional [S x M], sigma_out_host / acq_out_host optional [M],
 *   best_out_host optional [S] (the incumbents used);  info_host: 0, or the failing pivot of either factorisation - then nothing
 *   is scored and best_idx = -1.  0 < delta <= jitter1 + jitter2 (GPBO_ERR_ARG). */
#define GPBO_NEI_MAX_S 64
int64_t gpbo_nei_fantasies_workspace_bytes(int64_t Np, int32_t S);
int gpbo_nei_fantasies_f64(const double *K0d, const double *U0, const double *U, const double *y, int64_t N, int64_t Np,
                           const double *Z /* [S x N] */, const double *E /* [S x N] */, double noise_sd, int32_t S,
                           double *A_out /* [S x Np], zero on the padding */, double *F_out /* [S x Np] */,
                           double *best_out /* [S] */, void *work, int64_t work_bytes, void *stream);
int64_t gpbo_posterior_nei_workspace_bytes(int64_t Np, int64_t chunk, int64_t M, int32_t S);
int gpbo_posterior_nei_kern_f64(const double *Xs, int64_t M, const double *X, int64_t N, int64_t Np, int32_t d,
                                const double *ls_host, int32_t kernel, const double *U0, const double *A /* [S x Np] */,
                                const double *best /* [S], device */, int32_t S, double prior_var, double xi, int64_t idx_offset,
                                int64_t chunk, double *mu_out /* optional [S x ldm] */, int64_t ldm, double *sigma_out,
                                double *acq_out, gpbo_result *result, void *work, int64_t work_bytes, void *stream);
int gpbo_nei_host_f64(const double *X_host, const double *y_host, int64_t N, int32_t d, const double *ls_host, int32_t kernel,
                      double jitter1, double jitter2, double delta, const double *Xs_host, int64_t M, const double *Z_host,
                      const double *E_host, int32_t S, double xi, int64_t chunk, const double *best_in_host,
                      double *mu_out_host, double *sigma_out_host, double *acq_out_host, double *best_out_host,
                      gpbo_result *result_host, int32_t *info_host);

/* ---- Max-value entropy search on the dense posterior (csrc/mes.hip; Wang & Jegelka 2017; not in the reference).
 * For minimisation.  m* is the minimum of the latent function over the candidates; with S sampled minima m*_s and
 * gamma_s(x) = (mu(x) - m*_s) / sigma(x),
 *     MES(x) = (1 / S) sum_s h(gamma_s),   h(gamma) = gamma phi(gamma) / (2 Phi(gamma)) - log Phi(gamma) >= 0.
 * No trade-off parameter and no incumbent; invariant under y -> a + b y (mu, sigma and the samples in ONE unit, any unit); a
 * function of (mu, sigma) alone, so both calls read dense device arrays a scoring pass has left and build no covariance entry:
 * every kernel family, every model record.  h and log Phi are evaluated in three branches (csrc/mes_math.h), t = -gamma / sqrt 2:
 *     gamma > 0          log Phi = log1p(-erfc(gamma / sqrt 2) / 2),     h = gamma phi / (2 Phi) - log Phi
 *     -1 <= gamma <= 0   log Phi = log(erfc(t) / 2),                     h = gamma phi / (2 Phi) - log Phi
 *     gamma < -1         log Phi = -t^2 + log(erfcx(t) / 2),             h = (t^2 - t / (sqrt(pi) erfcx(t))) - log(erfcx(t) / 2)
 *   (below -1 both terms of the plain h grow like gamma^2 / 2 and cancel, and Phi underflows at gamma ~ -38); against 60-digit
 *   values the error stays within a few units of eps (max(1, gamma^2 / 2 for gamma < 0) + |h|).
 *
 * gpbo_mes_log_survival_f64: out[q] = log S(z_q) = sum_c log Phi((mu_c - z_q) / sigma_c), q < Q - the logarithm of Pr[m* > z_q]
 *   when the candidates are taken as independent - at Q levels in ONE pass over the M candidates, and nan_out[0] = the number of
 *   candidates skipped.  It serves the sampling of m*: the caller brackets the three levels where S = 0.75, 0.5, 0.25, fits a
 *   Gumbel law to them and draws the m*_s from it (bayesian_optimisation_amd/mes.py; the draws are the caller's, as everywhere in
 *   this ABI).  z_host [Q] travels by value.
 * gpbo_mes_acq_f64: MES over the M candidates and its first arg-max; the S terms are added in index order and divided by S.
 *   ystar_host [S]: the sampled minima, by value.  acq_out: optional dense [M].  result: as every other acquisition (best_idx =
 *   idx_offset + the LOWEST candidate attaining the maximum).
 * Edge rules: a candidate whose mu or sigma is NaN is skipped by log S and counted in nan_out; its acquisition is NaN, it counts
 *   once in nan_count and is never chosen.  sigma == 0: the term of log S is 0 where mu > z and -inf otherwise; the acquisition
 *   is 0.  (sigma is a standard deviation: >= 0.)
 * Sums run in a fixed order (a thread's candidates ascending, a butterfly inside a wave, waves in wave order, workgroups in index
 *   order) on a grid that depends on M alone: two calls give the same bits.  Only the integer NaN counter is atomic.
 * 1 <= M <= 2^40, 1 <= Q <= GPBO_MES_MAX_LEVELS, 1 <= S <= GPBO_MES_MAX_S, every level and sample finite, no null pointer
 *   but acq_out (GPBO_ERR_ARG otherwise);  work: GPBO_MES_WORK_BYTES bytes - a constant: 1024 x 64 partial sums and the arg-max
 *   records - 256-byte aligned (GPBO_ERR_WORKSPACE otherwise);  all of it before any HIP call.  Both calls only enqueue.
 * gpbo_mes_log_survival_host_f64 / gpbo_mes_acq_host_f64: the same two on host arrays (conventions of the other *_host entries:
 *   device buffers are allocated, filled, used and released inside the call, on a stream of its own; synchronous). */
#define GPBO_MES_MAX_LEVELS 64
#define GPBO_MES_MAX_S 64
#define GPBO_MES_WORK_BYTES 1048576
int gpbo_mes_log_survival_f64(const double *mu, const double *sigma, int64_t M, const double *z_host, int32_t Q,
                              double *out /* device [Q] */, int64_t *nan_out /* device [1] */, void *work, int64_t work_bytes,
                              void *stream);
int gpbo_mes_acq_f64(const double *mu, const double *sigma, int64_t M, const double *ystar_host, int32_t S, int64_t idx_offset,
                     double *acq_out /* optional [M] */, gpbo_result *result, void *work, int64_t work_bytes, void *stream);
int gpbo_mes_log_survival_host_f64(const double *mu_host, const double *sigma_host, int64_t M, const double *z_host, int32_t Q,
                                   double *out_host, int64_t *nan_out_host);
int gpbo_mes_acq_host_f64(const double *mu_host, const double *sigma_host, int64_t M, const double *ystar_host, int32_t S,
                          double *acq_out_host, gpbo_result *result_host);

/* ---- Constrained expected improvement, probability of improvement and probability of feasibility on the dense posterior, in
 * LOG space (csrc/constrained.hip; Gardner et al. 2014, Gelbart, Snoek & Adams 2014; not in the reference).  For
 * minimisation.  A candidate has the objective's posterior (mu, sigma) and C >= 0 constraint posteriors (mu_c, sigma_c), each
 * from a GP of its own, with upper limits u_c: feasible means g_c(x) <= u_c for every c, the constraints taken as independent.
 *     feas(x)  = sum_{c < C} log Phi((u_c - mu_c) / sigma_c)        (added in index order, c = 0 first, starting from 0)
 *     value(x) = base(x) + feas(x)
 *     base = 0                                                      GPBO_CONS_BASE_NONE: the probability of feasibility alone
 *          = log sigma + log h(z),  h(z) = phi(z) + z Phi(z)        GPBO_CONS_BASE_EI:   log of constrained expected improvement
 *          = log Phi(z)                                             GPBO_CONS_BASE_PI:   log of constrained probability of improvement
 *     z = ((f_best - mu) - xi) / sigma
 *   Every standardised argument is formed as written: subtractions, then ONE division.  The plain product of CDFs is exactly 0
 *   once the candidates are a few dozen standard deviations inside the infeasible region, and plain EI below z ~ -38.5; the
 *   logarithms keep the order.  log Phi as for max-value entropy search above; log h in three branches (csrc/cons_math.h),
 *   t = -z / sqrt 2, u = 1 / (2 t^2):
 *     z >= -1           log(phi(z) + z Phi(z))
 *     -1e3 < z < -1     -t^2 - log(2 pi) / 2 + log1p(-sqrt(pi) t erfcx(t))
 *     z <= -1e3         -t^2 - log(2 pi) / 2 + log(u (1 - 3 u (1 - 5 u)))
 *   against 60-digit values the error stays within a few units of eps (max(1, z^2 / 2 for z < 0) + |log h|).
 * mu, sigma [M]: read only with a base (may be null with GPBO_CONS_BASE_NONE).  cons_mu, cons_sigma: [C x ldc], row c the
 *   posterior of constraint c over the M candidates, ldc >= M (may be null with C == 0).  upper_host [C]: the limits, by value,
 *   in the units of cons_mu.  All of (mu, sigma, f_best, xi) in ONE unit, any unit.
 * val_out, feas_out: optional dense [M], value and feas; the result does not depend on their presence.  result: as every other
 *   acquisition (best_idx = idx_offset + the LOWEST candidate attaining the maximum).
 * Edge rules: a NaN in any value of a candidate the call reads makes its value NaN; it counts once in nan_count and is never
 *   chosen.  sigma_c == 0: the term is 0 where mu_c <= u_c and -inf otherwise.  sigma == 0, imp = (f_best - mu) - xi: EI gives
 *   log(max(imp, 0)), PI gives 0 where imp > 0 and -inf otherwise.  -inf is a legal value: when every candidate is -inf the lowest
 *   index is returned with best_val = -inf and nan_count untouched.  (sigma is a standard deviation: >= 0.)
 * No sum crosses candidates, the grid depends on M alone, only the integer NaN counter is atomic: two calls give the same bits.
 * 1 <= M <= 2^40, base one of the three, 0 <= C <= GPBO_CONS_MAX_C and C >= 1 without a base, ldc >= M, every limit finite,
 *   f_best and xi finite when there is a base, no null pointer but those named above (GPBO_ERR_ARG otherwise);  work:
 *   GPBO_CONS_WORK_BYTES bytes - a constant: the arg-max records of 1024 workgroups and the counter - 256-byte aligned
 *   (GPBO_ERR_WORKSPACE otherwise);  all of it before any HIP call.  The call only enqueues.
 * gpbo_constrained_acq_host_f64: the same on host arrays (conventions of the other *_host entries: device buffers are allocated,
 *   filled, used and released inside the call, on a stream of its own; synchronous; idx_offset = 0). */
#define GPBO_CONS_BASE_NONE 0
#define GPBO_CONS_BASE_EI 1
#define GPBO_CONS_BASE_PI 2
#define GPBO_CONS_MAX_C 8
#define GPBO_CONS_WORK_BYTES 16640
int gpbo_constrained_acq_f64(const double *mu, const double *sigma, int64_t M, int32_t base, double f_best, double xi,
                             const double *cons_mu, const double *cons_sigma, int64_t ldc, int32_t C, const double *upper_host,
                             int64_t idx_offset, double *val_out /* optional [M] */, double *feas_out /* optional [M] */,
                             gpbo_result *result, void *work, int64_t work_bytes, void *stream);
int gpbo_constrained_acq_host_f64(const double *mu_host, const double *sigma_host, int64_t M, int32_t base, double f_best,
                                  double xi, const double *cons_mu_host, const double *cons_sigma_host, int64_t ldc, int32_t C,
                                  const double *upper_host, double *val_out_host, double *feas_out_host,
                                  gpbo_result *result_host);

/* ---- Two-objective expected hypervolume improvement on the dense posteriors, in LOG space (csrc/ehvi.hip, DESIGN.md 4p;
 * Emmerich, Giannakoglou & Naujoks 2006; Emmerich, Yang, Deutz et al. 2016; not in the reference).  BOTH objectives are
 * minimised, each modelled by a GP of its own, taken as independent: a candidate has (mu1, sigma1) and (mu2, sigma2).  The
 * reference point is r = (ref1, ref2).  The front holds P >= 0 points (a_i, c_i), i = 1..P, strictly ascending in objective 1
 * and strictly descending in objective 2, every value finite, every point strictly below r in both coordinates; a_{P+1} = ref1,
 * c_0 = ref2.  For one objective and a level a
 *     g(a) = E[(a - f)+] = sigma h((a - mu) / sigma),  h(z) = phi(z) + z Phi(z)     (sigma > 0)
 *          = max(a - mu, 0)                                                         (sigma == 0)
 *     G(a) = log g(a) = log sigma + log h(z)           (log h: the three branches of the constrained acquisitions above)
 * and the region below r, cut into vertical strips at the a_i (strip i has the non-dominated ceiling c_i), gives
 *     EHVI  = sum_{i = 0..P} [g1(a_{i+1}) - g1(a_i)] g2(c_i),        g1(a_0) := 0      (every term >= 0)
 *     value = logsumexp_{i = 0..P} (G1(a_{i+1}) + log(1 - exp(G1(a_i) - G1(a_{i+1}))) + G2(c_i))
 *   Every z is formed as written: one subtraction, then ONE division.  The strips are added in index order, i = 0 first, by a
 *   one-pass running-maximum logsumexp; the i = 0 strip has no subtraction; log(1 - exp(d)) is log(-expm1(d)) for d > -log 2
 *   and log1p(-exp(d)) below, and -inf for d >= 0 (two levels whose G agree to the last bit).  A strip whose G1(a_{i+1}) or
 *   G2(c_i) is -inf is -inf, not NaN.  The plain sum is exactly 0 wherever both objectives are a few dozen standard deviations
 *   from improving; the logarithm is finite there and keeps the order.  Under y_j -> alpha_j + beta_j y_j (beta_j > 0) of the
 *   posteriors, the front and r, the value shifts by log beta_1 + log beta_2.
 * mu1, sigma1, mu2, sigma2 [M] (device).  front_host [P x 2], rows (a_i, c_i), read on the host during the call and passed to
 *   the kernel by value (may be null with P == 0).
 * val_out: optional dense [M]; the result does not depend on its presence.  result: as every other acquisition (best_idx =
 *   idx_offset + the LOWEST candidate attaining the maximum).
 * Edge rules: a NaN in any of a candidate's four values makes its value NaN; it counts once in nan_count and is never chosen.
 *   sigma == 0 uses max(a - mu, 0).  -inf is a legal value that beats the empty record: when every candidate is -inf the lowest
 *   index is returned with best_val = -inf and nan_count untouched.  Ties go to the lowest index.  (mu is finite or NaN, sigma a
 *   standard deviation: >= 0.)
 * No sum crosses candidates, the grid depends on M alone, only the integer NaN counter is atomic: two calls give the same bits.
 * 1 <= M <= 2^40, 0 <= P <= GPBO_EHVI_MAX_P, ref1 / ref2 finite, the front as stated above, no null pointer but val_out (and
 *   front_host with P == 0) (GPBO_ERR_ARG otherwise);  work: GPBO_EHVI_WORK_BYTES bytes - a constant: the arg-max records of
 *   1024 workgroups and the counter - 256-byte aligned (GPBO_ERR_WORKSPACE otherwise);  all of it before any HIP call.  The
 *   call only enqueues.
 * gpbo_ehvi_acq_host_f64: the same on host arrays (conventions of the other *_host entries: device buffers are allocated,
 *   filled, used and released inside the call, on a stream of its own; synchronous; idx_offset = 0). */
#define GPBO_EHVI_MAX_P 128
#define GPBO_EHVI_WORK_BYTES 16640
int gpbo_ehvi_acq_f64(const double *mu1, const double *sigma1, const double *mu2, const double *sigma2, int64_t M,
                      const double *front_host /* [P x 2] */, int32_t P, double ref1, double ref2, int64_t idx_offset,
                      double *val_out /* optional [M] */, gpbo_result *result, void *work, int64_t work_bytes, void *stream);
int gpbo_ehvi_acq_host_f64(const double *mu1_host, const double *sigma1_host, const double *mu2_host, const double *sigma2_host,
                           int64_t M, const double *front_host, int32_t P, double ref1, double ref2, double *val_out_host,
                           gpbo_result *result_host);

/* Strided-batched fp64 MFMA GEMM used by the factorisation (exported for tests):
 * C_b = alpha * A_b * op(B_b) + beta * C_b, row-major, M and N multiples of 64, K a multiple of 16;
 * transB = 0: B is [K x N]; transB = 1: B is [N x K].  lower_only = 1 skips 64x64 tiles strictly above
 * the block diagonal (SYRK-style update of a lower triangle).  M, N or batch <= 0 is an empty product: GPBO_OK,
 * nothing is read.  beta == 0: C is written and never read (it may hold NaN).
 * The contract, checked on the host (GPBO_ERR_ARG before anything is launched):
 *  - A and B are 16-byte aligned; lda, ldb are even, and so are strideA, strideB when batch > 1 (16-byte loads);
 *  - each leading dimension is at least the row length: lda >= K, ldb >= (transB ? K : N), ldc >= N;
 *  - K > 0; batch <= 65535; M / 32 and N / 32 <= 65535;
 *  - C may alias A only with N == 64 and ldc == lda (one workgroup then owns a whole 64-row tile, which it
 *    reads completely before it writes: the in-place panel solve of the factorisation); C may never alias B.
 *    Operands that overlap in any other way are the caller's error and are not detected. */
int gpbo_gemm_f64(int32_t transB, int64_t M, int64_t N, int64_t K, double alpha, const double *A, int64_t lda,
                  int64_t strideA, const double *B, int64_t ldb, int64_t strideB, double beta, double *C,
                  int64_t ldc, int64_t strideC, int32_t batch, int32_t lower_only, void *stream);

/* The same product with the two choices the library otherwise makes itself (exported for tests):
 * tri = 0: dense;  1: B [K x N] is lower triangular (transB = 0, K == N): the k range of a column tile starts at the
 * tile's first column;  2: A [M x K] is lower triangular (K == M): the k range of a row tile ends at the tile's last
 * row (the two products of each level of gpbo_trtri_f64; the 64 x 64 blocks of the zero triangle that lie strictly above
 * the block diagonal are not read).
 * tile = 0: the library's own rule (32 x 32 tiles below 2048 tiles of 64 x 64, 64 x 64 from there up and in place);
 * 32 or 64: that variant (32 is refused when C aliases A).  Otherwise the contract of gpbo_gemm_f64. */
int gpbo_gemm_tri_f64(int32_t transB, int64_t M, int64_t N, int64_t K, double alpha, const double *A, int64_t lda,
                      int64_t strideA, const double *B, int64_t ldb, int64_t strideB, double beta, double *C,
                      int64_t ldc, int64_t strideC, int32_t batch, int32_t lower_only, int32_t tri, int32_t tile,
                      void *stream);

#ifdef __cplusplus
}
#endif
#endif /* GPBO_H */
