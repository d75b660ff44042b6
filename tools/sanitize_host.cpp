// Host-side sanitizer job: driver for a build of libgpbo's HOST code - every translation unit of csrc/
// compiled with `-fsanitize=address,undefined -fno-gpu-sanitize` (host code instrumented; tools/sanitize_host.sh) - on a machine WITHOUT a GPU.
// It exercises what runs on the host before any kernel is launched:
//   * the launch planner of the fused factorisation (cholinv_plan.h through gpbo_cholinv_plan) for every padded size
//     128 ... 16,384 with the option sets the tests and the product use, checking each plan's tiles for well-formedness;
//   * the argument validation of every compute entry point (the bad-argument table of tests/test_abi_cpu.py, plus
//     all-NULL calls), which must return an error code before touching a pointer or the HIP runtime.
// Sanitizers are for this CPU build only (no GPU AddressSanitizer on the pool).  Prints "sanitize_host ok: ..." and exits 0;
// a sanitizer finding aborts with its report (-fno-sanitize-recover).
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "../include/gpbo.h"

static int fails = 0;
#define EXPECT(cond)                                                  \
    do {                                                              \
        if (!(cond)) {                                                \
            std::fprintf(stderr, "FAILED %s:%d: %s\n", __FILE__, __LINE__, #cond); \
            ++fails;                                                  \
        }                                                             \
    } while (0)

static long plans = 0, tiles_seen = 0;

static void run_plan(int64_t Np, const int32_t *opt) {
    int64_t nl = 0, nt = 0;
    int rc = gpbo_cholinv_plan(Np, opt, &nl, &nt, nullptr, nullptr);
    EXPECT(rc == GPBO_OK);
    if (rc != GPBO_OK) return;
    EXPECT(nl >= 1 && nt >= 0);
    // exact-size arrays: an off-by-one write of the export loop lands in ASan's red zone
    std::vector<int32_t> L((size_t)(5 * nl)), T((size_t)(8 * nt));
    int64_t cl = nl, ct = nt;
    rc = gpbo_cholinv_plan(Np, opt, &cl, &ct, L.data(), T.empty() ? nullptr : T.data());
    EXPECT(rc == GPBO_OK && cl == nl && ct == nt);
    if (nt > 1) {  // one entry short: refused, nothing written past the end
        std::vector<int32_t> Ts((size_t)(8 * (nt - 1)));
        int64_t c2 = nl, c3 = nt - 1;
        EXPECT(gpbo_cholinv_plan(Np, opt, &c2, &c3, L.data(), Ts.data()) == GPBO_ERR_WORKSPACE);
    }
    int64_t covered = 0;
    int pairs = 0;
    for (int64_t i = 0; i < nl; ++i) {
        const int32_t *l = &L[(size_t)(5 * i)];
        EXPECT(l[2] >= 0 && l[3] >= 0 && (int64_t)l[2] + l[3] <= nt && l[4] >= 1);
        EXPECT(l[1] + l[3] > 0);
        if (l[1] > 0) {
            EXPECT(l[0] == pairs);
            ++pairs;
        }
        covered += l[3];
    }
    EXPECT(pairs == Np / 128);
    EXPECT(covered == nt);
    for (int64_t i = 0; i < nt; ++i) {
        const int32_t *t = &T[(size_t)(8 * i)];
        const int th = t[0] == 2 ? 64 : t[0] == 3 ? 128 : t[0] == 4 ? 256 : 0;
        const int tw = t[0] == 2 ? (t[7] == 32 ? 32 : 64) : 128;
        EXPECT(th != 0);
        EXPECT(t[1] >= 0 && t[2] >= 32 && t[2] % 32 == 0 && t[1] + t[2] <= t[3]);   // source rows are finished rows
        EXPECT(t[3] % 64 == 0 && t[3] < Np && t[5] > t[3] && t[5] <= Np);
        EXPECT(t[4] >= 0 && t[4] % tw == 0 && (int64_t)t[4] + tw <= 2 * Np);
        EXPECT(t[6] >= 0 && t[6] <= Np);
    }
    ++plans;
    tiles_seen += nt;
}

int main() {
    EXPECT(gpbo_version() == GPBO_VERSION);
    EXPECT(gpbo_strerror(GPBO_ERR_ARG) != nullptr && gpbo_strerror(-99) != nullptr && gpbo_strerror(0) != nullptr);
    for (int64_t n = -3; n < 70000; n += 97) {
        const int64_t p = gpbo_padded_n(n);
        if (n >= 1) EXPECT(p >= n && p % GPBO_NPAD == 0 && p - n < GPBO_NPAD);
    }

    // ---- planner: every size, default options; the option sets of tests/test_cholinv_plan_cpu.py at every size they fit
    static const int32_t OPTS[][7] = {
        {1, 128, 3, 1, 0, 0, 0}, {2, 256, 4, 2, 0, 0, 0}, {3, 384, 3, 2, 0, 0, 0}, {1, 256, 4, 1, 0, 0, 0},
        {2, 512, 4, 3, 0, 0, 0}, {3, 256, 4, 3, 0, 0, 0}, {1, 128, 3, 1, 0, 2, 0}, {1, 256, 3, 3, 0, 0, 64},
        {1, 384, 3, 3, 0, 0, 64}, {1, 256, 3, 3, 0, 0, 32}, {4, 768, 3, 1, 0, 5, 32},
    };
    for (int64_t Np = 128; Np <= 16384; Np += 128) {
        run_plan(Np, nullptr);
        if (Np <= 4096 || Np % 2048 == 0)
            for (const auto &o : OPTS) run_plan(Np, o);
    }
    {  // refused before any planning: sizes, a far rank that is no multiple of 128, a tile width that does not exist
        int64_t a = 0, b = 0;
        EXPECT(gpbo_cholinv_plan(100, nullptr, &a, &b, nullptr, nullptr) == GPBO_ERR_ARG);
        EXPECT(gpbo_cholinv_plan(0, nullptr, &a, &b, nullptr, nullptr) == GPBO_ERR_ARG);
        EXPECT(gpbo_cholinv_plan(-128, nullptr, &a, &b, nullptr, nullptr) == GPBO_ERR_ARG);
        EXPECT(gpbo_cholinv_plan((int64_t)1 << 40, nullptr, &a, &b, nullptr, nullptr) == GPBO_ERR_ARG);
        EXPECT(gpbo_cholinv_plan(32768 + 128, nullptr, &a, &b, nullptr, nullptr) == GPBO_ERR_ARG);
        EXPECT(gpbo_cholinv_plan(1024, nullptr, nullptr, &b, nullptr, nullptr) == GPBO_ERR_ARG);
        const int32_t bad1[7] = {0, 200, 0, 0, 0, 0, 0}, bad2[7] = {0, 0, 0, 0, 0, 0, 48}, bad3[7] = {65, 0, 0, 0, 0, 0, 0},
                      bad4[7] = {0, 0, 9, 0, 0, 0, 0}, bad5[7] = {0, 1 << 30, 0, 0, 0, 0, 0};
        for (const int32_t *o : {bad1, bad2, bad3, bad4, bad5}) EXPECT(gpbo_cholinv_plan(1024, o, &a, &b, nullptr, nullptr) == GPBO_ERR_ARG);
    }

    // ---- argument validation: the table of tests/test_abi_cpu.py::test_size_contracts_are_checked_on_the_host -------------
    alignas(256) static char buf[1024];
    void *p = buf;            // aligned like a device allocation; never dereferenced by a call that is refused
    double *pd = reinterpret_cast<double *>(buf);
    int32_t *pi = reinterpret_cast<int32_t *>(buf);
    double ls[16];
    for (double &v : ls) v = 0.5;
    EXPECT(gpbo_kxx_f64(nullptr, 4, 2, nullptr, 1e-4, 1e-6, nullptr, 128, nullptr) == GPBO_ERR_ARG);
    EXPECT(gpbo_posterior_workspace_bytes(100, 512, 10) == -1);
    EXPECT(gpbo_posterior_workspace_bytes(128, 500, 10) == -1);
    EXPECT(gpbo_posterior_workspace_bytes(128, 512, 1000) > 128 * 512 * 8);
    EXPECT(gpbo_factorise_workspace_bytes(256) == 8 * (2 * 256 * 256 + 256 * 64 + 256));
    EXPECT(gpbo_factorise_f64(pd, pd, 100, 2, ls, 1e-4, 1e-6, 256, pd, pd, pd, pi, p, (int64_t)1 << 40, nullptr) == GPBO_ERR_ARG);
    EXPECT(gpbo_factorise_f64(pd, pd, 100, 2, ls, 1e-4, 1e-6, 128, pd, pd, pd, pi, p, 8, nullptr) == GPBO_ERR_WORKSPACE);
    EXPECT(gpbo_append_f64(pd, pd, 128, 2, ls, 1e-4, 1e-6, 128, pd, pd, nullptr, pd, pd, pi, p, 1 << 30, nullptr) == GPBO_ERR_ARG);
    EXPECT(gpbo_append_f64(pd, pd, 10, 17, ls, 1e-4, 1e-6, 128, pd, pd, nullptr, pd, pd, pi, p, 1 << 30, nullptr) == GPBO_ERR_ARG);
    const double bad_ls[2] = {0.5, 0.0};
    EXPECT(gpbo_append_f64(pd, pd, 10, 2, bad_ls, 1e-4, 1e-6, 128, pd, pd, nullptr, pd, pd, pi, p, 1 << 30, nullptr) == GPBO_ERR_ARG);
    EXPECT(gpbo_append_f64(pd, pd, 10, 2, ls, 1e-4, 1e-6, 128, pd, pd, nullptr, pd, pd, pi, p, 8, nullptr) == GPBO_ERR_WORKSPACE);
    EXPECT(gpbo_append_workspace_bytes(128) == 8 * (3 * 128 + 8));
    auto post = [&](int64_t Np, int64_t chunk, int kind, int64_t wbytes) {
        return gpbo_posterior_acq_f64(pd, 1000, pd, 100, Np, 2, ls, pd, pd, 1.0, kind, 4.0, 0.0, 0.0, 0, chunk, nullptr, nullptr,
                                      nullptr, reinterpret_cast<gpbo_result *>(p), p, wbytes, nullptr, nullptr);
    };
    EXPECT(post(100, 512, 0, (int64_t)1 << 40) == GPBO_ERR_ARG);
    EXPECT(post(128, 500, 0, (int64_t)1 << 40) == GPBO_ERR_ARG);
    EXPECT(post(128, 512, 7, (int64_t)1 << 40) == GPBO_ERR_ARG);
    EXPECT(post(128, (int64_t)1 << 25, 0, (int64_t)1 << 40) == GPBO_ERR_ARG);
    EXPECT(post(128, 512, 0, 8) == GPBO_ERR_WORKSPACE);
    // batch selection (tests/test_batch_abi_cpu.py): q range, q > M, d, fantasy rule, a NaN lie, the workspace one byte short
    auto batch = [&](int64_t M, int32_t d, int32_t q, int32_t fantasy, double lie, int64_t wbytes) {
        return gpbo_select_batch_f64(pd, M, pd, 100, 128, d, ls, pd, pd, 1e-4, 1e-6, 1.000101, 0, 4.0, 0.0, q, fantasy, lie, pd, pd,
                                     0, reinterpret_cast<int64_t *>(p), pd, reinterpret_cast<gpbo_result *>(p), pi, p, wbytes, nullptr);
    };
    const int64_t wb = gpbo_batch_workspace_bytes(128, 1000, 8);
    EXPECT(wb > 0 && gpbo_batch_workspace_bytes(128, 1000, 65) == -1 && gpbo_batch_workspace_bytes(100, 1000, 8) == -1);
    EXPECT(batch(1000, 2, 0, 0, 0.0, wb) == GPBO_ERR_ARG && batch(1000, 2, 65, 0, 0.0, wb) == GPBO_ERR_ARG);
    EXPECT(batch(7, 2, 8, 0, 0.0, (int64_t)1 << 40) == GPBO_ERR_ARG && batch(1000, 17, 8, 0, 0.0, wb) == GPBO_ERR_ARG);
    EXPECT(batch(1000, 2, 8, 2, 0.0, wb) == GPBO_ERR_ARG && batch(1000, 2, 8, 1, __builtin_nan(""), wb) == GPBO_ERR_ARG);
    EXPECT(batch(1000, 2, 8, 0, 0.0, wb - 1) == GPBO_ERR_WORKSPACE);
    // refinement (tests/test_refine_abi_cpu.py): P range, d, Np against N, a box upside down, iters, step0, the workspace one byte short
    {
        const double lo[2] = {0.0, 0.0}, hi[2] = {1.0, 1.0}, up[2] = {0.0, -1.0};
        auto refine = [&](int64_t P, int64_t Np, int32_t d, const double *h, int32_t iters, double step0, int64_t wbytes) {
            return gpbo_refine_f64(pd, P, lo, h, pd, 100, Np, d, ls, pd, pd, 1.000101, 0, 4.0, 0.0, iters, step0, nullptr, nullptr,
                                   nullptr, nullptr, reinterpret_cast<gpbo_result *>(p), p, wbytes, nullptr);
        };
        const int64_t wr = gpbo_refine_workspace_bytes(128, 8), wg = gpbo_posterior_grad_workspace_bytes(128, 8);
        EXPECT(wr > wg && wg > 0 && gpbo_refine_workspace_bytes(128, 4097) == -1 && gpbo_posterior_grad_workspace_bytes(100, 8) == -1);
        EXPECT(refine(0, 128, 2, hi, 30, 0.1, wr) == GPBO_ERR_ARG && refine(4097, 128, 2, hi, 30, 0.1, wr) == GPBO_ERR_ARG);
        EXPECT(refine(8, 256, 2, hi, 30, 0.1, wr) == GPBO_ERR_ARG && refine(8, 128, 17, hi, 30, 0.1, wr) == GPBO_ERR_ARG);
        EXPECT(refine(8, 128, 2, up, 30, 0.1, wr) == GPBO_ERR_ARG && refine(8, 128, 2, hi, 1001, 0.1, wr) == GPBO_ERR_ARG);
        EXPECT(refine(8, 128, 2, hi, 30, __builtin_nan(""), wr) == GPBO_ERR_ARG && refine(8, 128, 2, hi, 30, 0.0, wr) == GPBO_ERR_ARG);
        EXPECT(refine(8, 128, 2, hi, 30, 0.1, wr - 1) == GPBO_ERR_WORKSPACE);
        EXPECT(gpbo_posterior_grad_f64(pd, 8, pd, 100, 128, 2, ls, pd, pd, 1.000101, 0, 4.0, 0.0, nullptr, nullptr, nullptr, nullptr,
                                       nullptr, nullptr, p, wg - 1, nullptr) == GPBO_ERR_WORKSPACE);
        EXPECT(gpbo_posterior_grad_f64(pd, 8, pd, 100, 128, 2, ls, pd, pd, 1.000101, 7, 4.0, 0.0, nullptr, nullptr, nullptr, nullptr,
                                       nullptr, nullptr, p, wg, nullptr) == GPBO_ERR_ARG);
    }
    // Thompson sampling (tests/test_thompson_abi_cpu.py): the ranges of F, S, d, M, the dense output's leading dimension, the
    // workspaces one byte short; V == NULL alone is legal and reaches the workspace check
    {
        int64_t *pl = reinterpret_cast<int64_t *>(p);
        int32_t info_t = 0;
        auto paths = [&](int64_t M, int32_t d, int32_t F, int32_t S, const double *V, double *f_out, int64_t ldf, int64_t wbytes) {
            return gpbo_thompson_paths_f64(pd, M, pd, 100, 128, d, ls, pd, pd, pd, V, F, S, 0, f_out, ldf, pl, pd, pl, p, wbytes,
                                           nullptr);
        };
        auto weights = [&](int64_t N, int64_t Np, int32_t F, int32_t S, double j1, int64_t wbytes) {
            return gpbo_thompson_weights_f64(pd, pd, N, Np, 2, ls, pd, j1, 1e-6, pd, pd, pd, pd, F, S, pd, p, wbytes, nullptr);
        };
        const int64_t wp = gpbo_thompson_paths_workspace_bytes(128, 1000, 64, 16), ww = gpbo_thompson_weights_workspace_bytes(128, 64, 16);
        EXPECT(wp > 0 && ww > wp && gpbo_thompson_paths_workspace_bytes(128, 0, 64, 16) == -1 &&
               gpbo_thompson_weights_workspace_bytes(128, 16385, 16) == -1 && gpbo_thompson_paths_workspace_bytes(100, 1000, 64, 16) == -1);
        EXPECT(paths(0, 2, 64, 16, pd, nullptr, 0, wp) == GPBO_ERR_ARG && paths(1000, 17, 64, 16, pd, nullptr, 0, wp) == GPBO_ERR_ARG);
        EXPECT(paths(1000, 2, 0, 16, pd, nullptr, 0, wp) == GPBO_ERR_ARG && paths(1000, 2, 64, 65, pd, nullptr, 0, wp) == GPBO_ERR_ARG);
        EXPECT(paths(1000, 2, 64, 16, pd, pd, 999, wp) == GPBO_ERR_ARG);
        EXPECT(paths(1000, 2, 64, 16, pd, nullptr, 0, wp - 1) == GPBO_ERR_WORKSPACE);
        EXPECT(paths(1000, 2, 64, 16, nullptr, nullptr, 0, wp - 1) == GPBO_ERR_WORKSPACE);
        EXPECT(weights(129, 128, 64, 16, 1e-4, ww) == GPBO_ERR_ARG && weights(100, 100, 64, 16, 1e-4, ww) == GPBO_ERR_ARG);
        EXPECT(weights(100, 128, 64, 0, 1e-4, ww) == GPBO_ERR_ARG && weights(100, 128, 64, 16, -1.0, ww) == GPBO_ERR_ARG);
        EXPECT(weights(100, 128, 64, 16, 1e-4, ww - 1) == GPBO_ERR_WORKSPACE);
        EXPECT(gpbo_thompson_host_f64(nullptr, nullptr, 0, 0, nullptr, 0, 0, nullptr, 0, nullptr, nullptr, nullptr, nullptr, 0, 0, nullptr,
                                      nullptr, nullptr, nullptr, &info_t) == GPBO_ERR_ARG);
    }
    // noisy expected improvement (tests/test_nei_abi_cpu.py): the ranges of S, d, the chunk, the dense means' leading dimension,
    // the noise's standard deviation, the workspaces one byte short
    {
        gpbo_result res_n;
        int32_t info_n = 0;
        auto score = [&](int64_t M, int32_t d, int32_t S, int64_t chunk, double *mu, int64_t ldm, int64_t wbytes) {
            return gpbo_posterior_nei_kern_f64(pd, M, pd, 100, 128, d, ls, 0, pd, pd, pd, S, 1.000001, 0.0, 0, chunk, mu, ldm, nullptr,
                                               nullptr, &res_n, p, wbytes, nullptr);
        };
        auto fantasies = [&](int64_t N, int64_t Np, int32_t S, double sd, int64_t wbytes) {
            return gpbo_nei_fantasies_f64(pd, pd, pd, pd, N, Np, pd, pd, sd, S, pd, pd, pd, p, wbytes, nullptr);
        };
        const int64_t wn = gpbo_posterior_nei_workspace_bytes(128, 512, 1000, 16), wf = gpbo_nei_fantasies_workspace_bytes(128, 16);
        EXPECT(wn > 0 && wf > 0 && gpbo_posterior_nei_workspace_bytes(128, 512, 1000, 65) == -1 &&
               gpbo_posterior_nei_workspace_bytes(128, 500, 1000, 16) == -1 && gpbo_nei_fantasies_workspace_bytes(100, 16) == -1);
        EXPECT(score(1000, 2, 0, 512, nullptr, 0, wn) == GPBO_ERR_ARG && score(1000, 2, 65, 512, nullptr, 0, wn) == GPBO_ERR_ARG);
        EXPECT(score(1000, 17, 16, 512, nullptr, 0, wn) == GPBO_ERR_ARG && score(1000, 2, 16, 500, nullptr, 0, wn) == GPBO_ERR_ARG);
        EXPECT(score(0, 2, 16, 512, nullptr, 0, wn) == GPBO_ERR_ARG && score(1000, 2, 16, 512, pd, 999, wn) == GPBO_ERR_ARG);
        EXPECT(score(1000, 2, 16, 512, nullptr, 0, wn - 1) == GPBO_ERR_WORKSPACE);
        EXPECT(fantasies(129, 128, 16, 0.3, wf) == GPBO_ERR_ARG && fantasies(100, 128, 65, 0.3, wf) == GPBO_ERR_ARG);
        EXPECT(fantasies(100, 128, 16, -0.1, wf) == GPBO_ERR_ARG && fantasies(100, 128, 16, 0.0, wf - 1) == GPBO_ERR_WORKSPACE);
        EXPECT(gpbo_nei_host_f64(pd, pd, 100, 2, ls, 0, 0.09, 0.0, 0.1, pd, 1000, pd, pd, 16, 0.0, 0, nullptr, nullptr, nullptr, nullptr,
                                 nullptr, &res_n, &info_n) == GPBO_ERR_ARG);   // delta > rho
        EXPECT(gpbo_nei_host_f64(pd, pd, 100, 2, ls, 0, 0.09, 0.0, 1e-6, pd, 1000, pd, pd, 65, 0.0, 0, nullptr, nullptr, nullptr, nullptr,
                                 nullptr, &res_n, &info_n) == GPBO_ERR_ARG);
    }
    // max-value entropy search (tests/test_mes_abi_cpu.py): the ranges of M, Q and S, the values that travel by value read on
    // the host (only the first Q / S of them), the constant workspace one byte short or misaligned
    {
        gpbo_result res_m;
        int64_t nan_m = 0;
        double lv[64], bad[3] = {0.0, 1.0, __builtin_nan("")};
        for (int q = 0; q < 64; ++q) lv[q] = -1.0 + q / 32.0;
        auto surv = [&](int64_t M, const double *z, int32_t Q, void *w, int64_t wbytes) {
            return gpbo_mes_log_survival_f64(pd, pd, M, z, Q, pd, reinterpret_cast<int64_t *>(pd), w, wbytes, nullptr);
        };
        auto acq = [&](int64_t M, const double *y, int32_t S, void *w, int64_t wbytes) {
            return gpbo_mes_acq_f64(pd, pd, M, y, S, 0, nullptr, &res_m, w, wbytes, nullptr);
        };
        const int64_t wm = GPBO_MES_WORK_BYTES;
        EXPECT(surv(0, lv, 63, p, wm) == GPBO_ERR_ARG && surv(((int64_t)1 << 40) + 1, lv, 63, p, wm) == GPBO_ERR_ARG);
        EXPECT(surv(1000, lv, 0, p, wm) == GPBO_ERR_ARG && surv(1000, lv, 65, p, wm) == GPBO_ERR_ARG);
        EXPECT(surv(1000, bad, 3, p, wm) == GPBO_ERR_ARG && surv(1000, bad, 2, p, wm - 1) == GPBO_ERR_WORKSPACE);
        EXPECT(surv(1000, lv, 64, p, wm - 1) == GPBO_ERR_WORKSPACE && surv(1000, lv, 64, static_cast<char *>(p) + 8, wm) == GPBO_ERR_WORKSPACE);
        EXPECT(surv(1000, nullptr, 1, p, wm) == GPBO_ERR_ARG && surv(1000, lv, 1, nullptr, wm) == GPBO_ERR_ARG);
        EXPECT(acq(0, lv, 16, p, wm) == GPBO_ERR_ARG && acq(1000, lv, 0, p, wm) == GPBO_ERR_ARG && acq(1000, lv, 65, p, wm) == GPBO_ERR_ARG);
        EXPECT(acq(1000, bad, 3, p, wm) == GPBO_ERR_ARG && acq(1000, lv, 64, p, wm - 1) == GPBO_ERR_WORKSPACE);
        EXPECT(gpbo_mes_log_survival_host_f64(pd, pd, 10, bad, 3, pd, &nan_m) == GPBO_ERR_ARG);
        EXPECT(gpbo_mes_log_survival_host_f64(pd, pd, 10, lv, 65, pd, &nan_m) == GPBO_ERR_ARG);
        EXPECT(gpbo_mes_acq_host_f64(pd, pd, 0, lv, 16, nullptr, &res_m) == GPBO_ERR_ARG);
        EXPECT(gpbo_mes_acq_host_f64(pd, pd, 10, bad, 3, nullptr, &res_m) == GPBO_ERR_ARG);
    }
    // the constrained acquisitions (tests/test_constrained_abi_cpu.py): the ranges of M, base, C and ldc, the limits read on the
    // host (only the first C of them), f_best / xi only with a base, the constant workspace one byte short or misaligned
    {
        gpbo_result res_c;
        double up[8] = {0.0, 0.5, -0.5, 1.0, 2.0, -2.0, 0.25, 0.75}, bad[3] = {0.0, 1.0, __builtin_nan("")};
        const double nan = __builtin_nan("");
        auto cons = [&](int64_t M, int32_t base, double fb, int64_t ldc, int32_t Cn, const double *u, void *w, int64_t wbytes) {
            return gpbo_constrained_acq_f64(pd, pd, M, base, fb, 0.0, pd, pd, ldc, Cn, u, 0, nullptr, nullptr, &res_c, w, wbytes, nullptr);
        };
        const int64_t wc = GPBO_CONS_WORK_BYTES;
        EXPECT(cons(0, GPBO_CONS_BASE_EI, 0.0, 10, 3, up, p, wc) == GPBO_ERR_ARG && cons(((int64_t)1 << 40) + 1, GPBO_CONS_BASE_EI, 0.0, (int64_t)1 << 41, 3, up, p, wc) == GPBO_ERR_ARG);
        EXPECT(cons(1000, 3, 0.0, 1000, 3, up, p, wc) == GPBO_ERR_ARG && cons(1000, GPBO_CONS_BASE_NONE, 0.0, 1000, 0, up, p, wc) == GPBO_ERR_ARG);
        EXPECT(cons(1000, GPBO_CONS_BASE_PI, 0.0, 1000, 9, up, p, wc) == GPBO_ERR_ARG && cons(1000, GPBO_CONS_BASE_PI, 0.0, 999, 3, up, p, wc) == GPBO_ERR_ARG);
        EXPECT(cons(1000, GPBO_CONS_BASE_EI, 0.0, 1000, 3, bad, p, wc) == GPBO_ERR_ARG && cons(1000, GPBO_CONS_BASE_EI, 0.0, 1000, 2, bad, p, wc - 1) == GPBO_ERR_WORKSPACE);
        EXPECT(cons(1000, GPBO_CONS_BASE_EI, nan, 1000, 3, up, p, wc) == GPBO_ERR_ARG && cons(1000, GPBO_CONS_BASE_NONE, nan, 1000, 3, up, p, wc - 1) == GPBO_ERR_WORKSPACE);
        EXPECT(cons(1000, GPBO_CONS_BASE_EI, 0.0, 1037, 8, up, static_cast<char *>(p) + 8, wc) == GPBO_ERR_WORKSPACE);
        EXPECT(cons(1000, GPBO_CONS_BASE_EI, 0.0, 1000, 0, nullptr, p, wc - 1) == GPBO_ERR_WORKSPACE && cons(1000, GPBO_CONS_BASE_EI, 0.0, 1000, 1, nullptr, p, wc) == GPBO_ERR_ARG);
        EXPECT(gpbo_constrained_acq_host_f64(pd, pd, 10, GPBO_CONS_BASE_EI, 0.0, 0.0, pd, pd, 10, 3, bad, nullptr, nullptr, &res_c) == GPBO_ERR_ARG);
        EXPECT(gpbo_constrained_acq_host_f64(pd, pd, 10, GPBO_CONS_BASE_NONE, 0.0, 0.0, nullptr, nullptr, 10, 0, nullptr, nullptr, nullptr, &res_c) == GPBO_ERR_ARG);
    }
    // two-objective expected hypervolume improvement (tests/test_ehvi_abi_cpu.py): the ranges of M and P, the front read on the
    // host (only its first P rows: finite, ordered, strictly below the reference point), the reference point, the null pointers,
    // the constant workspace one byte short or misaligned
    {
        gpbo_result res_e;
        const double nan = __builtin_nan(""), inf = __builtin_huge_val();
        double fr[6] = {0.0, 2.0, 1.0, 1.0, 2.0, 0.0}, big[2 * (GPBO_EHVI_MAX_P + 1)];
        double nanf[6] = {0.0, 2.0, 1.0, nan, 2.0, 0.0}, asc[6] = {0.0, 2.0, 0.0, 1.0, 2.0, 0.0}, desc[6] = {0.0, 2.0, 1.0, 2.0, 2.0, 0.0};
        for (int i = 0; i <= GPBO_EHVI_MAX_P; ++i) big[2 * i] = i, big[2 * i + 1] = -i;
        auto ehvi = [&](int64_t M, const double *f, int32_t Pn, double r1, double r2, void *w, int64_t wbytes) {
            return gpbo_ehvi_acq_f64(pd, pd, pd, pd, M, f, Pn, r1, r2, 0, nullptr, &res_e, w, wbytes, nullptr);
        };
        const int64_t we = GPBO_EHVI_WORK_BYTES;
        EXPECT(ehvi(0, fr, 3, 3.0, 3.0, p, we) == GPBO_ERR_ARG && ehvi(((int64_t)1 << 40) + 1, fr, 3, 3.0, 3.0, p, we) == GPBO_ERR_ARG);
        EXPECT(ehvi(1000, fr, -1, 3.0, 3.0, p, we) == GPBO_ERR_ARG && ehvi(1000, big, GPBO_EHVI_MAX_P + 1, 1e3, 1e3, p, we) == GPBO_ERR_ARG);
        EXPECT(ehvi(1000, big, GPBO_EHVI_MAX_P, 1e3, 1e3, p, we - 1) == GPBO_ERR_WORKSPACE && ehvi((int64_t)1 << 40, fr, 3, 3.0, 3.0, p, we - 1) == GPBO_ERR_WORKSPACE);
        EXPECT(ehvi(1000, nanf, 3, 3.0, 3.0, p, we) == GPBO_ERR_ARG && ehvi(1000, nanf, 1, 3.0, 3.0, p, we - 1) == GPBO_ERR_WORKSPACE);
        EXPECT(ehvi(1000, asc, 3, 3.0, 3.0, p, we) == GPBO_ERR_ARG && ehvi(1000, desc, 3, 3.0, 3.0, p, we) == GPBO_ERR_ARG);
        EXPECT(ehvi(1000, fr, 3, 2.0, 3.0, p, we) == GPBO_ERR_ARG && ehvi(1000, fr, 3, 3.0, 2.0, p, we) == GPBO_ERR_ARG);
        EXPECT(ehvi(1000, fr, 3, nan, 3.0, p, we) == GPBO_ERR_ARG && ehvi(1000, fr, 0, 3.0, inf, p, we) == GPBO_ERR_ARG);
        EXPECT(ehvi(1000, nullptr, 1, 3.0, 3.0, p, we) == GPBO_ERR_ARG && ehvi(1000, nullptr, 0, 3.0, 3.0, p, we - 1) == GPBO_ERR_WORKSPACE);
        EXPECT(ehvi(1000, fr, 3, 3.0, 3.0, static_cast<char *>(p) + 8, we) == GPBO_ERR_WORKSPACE && ehvi(1000, fr, 3, 3.0, 3.0, nullptr, we) == GPBO_ERR_ARG);
        EXPECT(gpbo_ehvi_acq_f64(nullptr, pd, pd, pd, 10, fr, 3, 3.0, 3.0, 0, nullptr, &res_e, p, we, nullptr) == GPBO_ERR_ARG);
        EXPECT(gpbo_ehvi_acq_f64(pd, pd, pd, pd, 10, fr, 3, 3.0, 3.0, 0, nullptr, nullptr, p, we, nullptr) == GPBO_ERR_ARG);
        EXPECT(gpbo_ehvi_acq_host_f64(pd, pd, pd, pd, 10, nanf, 3, 3.0, 3.0, nullptr, &res_e) == GPBO_ERR_ARG);
        EXPECT(gpbo_ehvi_acq_host_f64(pd, pd, pd, nullptr, 10, fr, 3, 3.0, 3.0, nullptr, &res_e) == GPBO_ERR_ARG);
    }
    // the likelihood of many hyperparameter cells and the ensemble pass (tests/test_marginal_abi_cpu.py): the size limits, the
    // model table read on the host (weights, scales, every model's length scales), the workspace one byte short
    {
        EXPECT(gpbo_nlml_hyper_cells_f64(pd, pd, 65, 2, pd, 4, 0, 3, pd, nullptr) == GPBO_ERR_ARG);
        EXPECT(gpbo_nlml_hyper_cells_f64(pd, pd, 20, 17, pd, 4, 0, 3, pd, nullptr) == GPBO_ERR_ARG);
        EXPECT(gpbo_nlml_hyper_cells_f64(pd, pd, 20, 2, pd, 0, 0, 3, pd, nullptr) == GPBO_ERR_ARG);
        EXPECT(gpbo_nlml_hyper_cells_f64(pd, pd, 20, 2, pd, 4, 3, 3, pd, nullptr) == GPBO_ERR_ARG);
        EXPECT(gpbo_nlml_hyper_cells_f64(pd, pd, 20, 2, pd, 4, 0, 4, pd, nullptr) == GPBO_ERR_ARG);
        double lss[GPBO_ENSEMBLE_MAX_S * 2], model[GPBO_ENSEMBLE_MAX_S * 4];
        for (int s = 0; s < GPBO_ENSEMBLE_MAX_S; ++s) {
            lss[2 * s] = lss[2 * s + 1] = 0.5;
            model[4 * s] = 1.0 / GPBO_ENSEMBLE_MAX_S, model[4 * s + 1] = 1.01, model[4 * s + 2] = 40.0, model[4 * s + 3] = 7.0;
        }
        const int64_t we = gpbo_ensemble_workspace_bytes(128, 512, 1000);
        auto ens = [&](int32_t S, int32_t d, int64_t wbytes) {
            return gpbo_ensemble_acq_f64(pd, 1000, pd, 100, 128, d, S, lss, 0, pd, pd, model, 0, 4.0, 0.0, 0, 512, nullptr, nullptr,
                                         nullptr, reinterpret_cast<gpbo_result *>(p), p, wbytes, nullptr);
        };
        EXPECT(we > gpbo_posterior_workspace_bytes(128, 512, 1000) && gpbo_ensemble_workspace_bytes(100, 512, 1000) == -1);
        EXPECT(ens(0, 2, we) == GPBO_ERR_ARG && ens(GPBO_ENSEMBLE_MAX_S + 1, 2, we) == GPBO_ERR_ARG && ens(4, 17, we) == GPBO_ERR_ARG);
        EXPECT(ens(GPBO_ENSEMBLE_MAX_S, 2, we - 1) == GPBO_ERR_WORKSPACE);   // (reads all 64 rows of both tables)
        model[4 * 63] = -0.25;
        EXPECT(ens(GPBO_ENSEMBLE_MAX_S, 2, we) == GPBO_ERR_ARG && ens(63, 2, we - 1) == GPBO_ERR_WORKSPACE);
        model[4 * 63] = 0.25;
        lss[2 * 63 + 1] = 0.0;
        EXPECT(ens(GPBO_ENSEMBLE_MAX_S, 2, we) == GPBO_ERR_ARG);
    }
    EXPECT(gpbo_potrf_f64(pd, 100, pd, pi, nullptr) == GPBO_ERR_ARG);
    EXPECT(gpbo_trtri_f64(pd, pd, 100, pd, pd, nullptr) == GPBO_ERR_ARG);
    EXPECT(gpbo_nlml_grid_f64(pd, pd, 177, 2, pd, 4, 1e-4, reinterpret_cast<float *>(p), nullptr) == GPBO_ERR_ARG);
    // the fp64 GEMM (tests/test_host_gemm_args_cpu.py has every rule): short leading dimensions, an odd batch stride, the
    // alias rule, an unknown tile; the empty product is fine with no pointers at all
    {
        double *pa = pd, *pb = pd + 32, *pc = pd + 64;   // distinct, 16-byte aligned, never dereferenced
        auto gemm = [&](int64_t N, int64_t lda, int64_t ldc, int64_t sA, const double *A, const double *B, double *Cc, int32_t batch,
                        int32_t tile) {
            return gpbo_gemm_tri_f64(1, 64, N, 64, 1.0, A, lda, sA, B, 64, 0, 0.0, Cc, ldc, 64 * ldc, batch, 0, 0, tile, nullptr);
        };
        EXPECT(gemm(64, 62, 64, 0, pa, pb, pc, 1, 0) == GPBO_ERR_ARG && gemm(128, 64, 126, 0, pa, pb, pc, 1, 0) == GPBO_ERR_ARG);
        EXPECT(gemm(64, 64, 64, 4097, pa, pb, pc, 2, 0) == GPBO_ERR_ARG);
        EXPECT(gemm(64, 64, 64, 0, pa, pb, pb, 1, 0) == GPBO_ERR_ARG && gemm(128, 64, 128, 0, pa, pb, pa, 1, 0) == GPBO_ERR_ARG);
        EXPECT(gemm(64, 64, 64, 0, pa, pb, pa, 1, 32) == GPBO_ERR_ARG && gemm(64, 64, 64, 0, pa, pb, pc, 1, 16) == GPBO_ERR_ARG);
        EXPECT(gpbo_gemm_f64(0, 64, 64, 16, 1.0, pa, 14, 0, pb, 64, 0, 0.0, pc, 64, 0, 1, 0, nullptr) == GPBO_ERR_ARG);
        EXPECT(gpbo_gemm_tri_f64(0, 0, 64, 16, 1.0, nullptr, 0, 0, nullptr, 0, 0, 0.0, nullptr, 0, 0, 1, 0, 0, 0, nullptr) == GPBO_OK);
    }
    // the fused factorisation: S must be 16-byte aligned (LDS-DMA reads it in 16-byte pieces), ld even and >= 2 Np
    EXPECT(gpbo_cholinv_f64(pd + 1, 512, 256, pi, nullptr, nullptr) == GPBO_ERR_ARG);
    EXPECT(gpbo_cholinv_f64(pd, 511, 256, pi, nullptr, nullptr) == GPBO_ERR_ARG);
    EXPECT(gpbo_cholinv_f64(pd, 256, 256, pi, nullptr, nullptr) == GPBO_ERR_ARG);
    EXPECT(gpbo_cholinv_f64(pd, 512, 200, pi, nullptr, nullptr) == GPBO_ERR_ARG);
    EXPECT(gpbo_cholinv_f64(pd, 2 * 32896, 32896, pi, nullptr, nullptr) == GPBO_ERR_ARG);
    {
        const int32_t tile_bad[8] = {3, 0, 100, 128, 0, 256, 0, 0};  // rank not a multiple of 32
        EXPECT(gpbo_cholinv_tiles_f64(pd, 512, 256, pi, -1, tile_bad, 1, 1, 1, nullptr) == GPBO_ERR_ARG);
        EXPECT(gpbo_cholinv_tiles_f64(pd, 512, 256, pi, 5, nullptr, 0, 1, 1, nullptr) == GPBO_ERR_ARG);  // pair beyond Np
        EXPECT(gpbo_cholinv_tiles_f64(pd, 512, 256, pi, -1, nullptr, 0, 1, 1, nullptr) == GPBO_ERR_ARG);  // nothing to do
    }
    // the workspace carves with a null base (csrc/host_driver.h: Carver): every size query over the argument sets of
    // tests/test_workspace_sizes_cpu.py, refused values included - whole 256-byte granules, or a refusal
    {
        const int64_t NP[] = {128, 256, 384, 4096, 32768, 0, 100}, CHUNK[] = {512, 1024, 131072, 0, 500};
        const int64_t MM[] = {1, 511, 512, 513, 131073, 0}, CAP[] = {1, 4096, 131073, 0};
        const int32_t QS[] = {1, 2, 16, 64, 0, 65}, FS[] = {1, 1000, 16384, 0, 16385}, DS[] = {1, 8, 16, 0, 17};
        const int64_t PS[] = {1, 64, 4096, 0, 4097};
        long queries = 0;
        auto granules = [&](int64_t b) {
            EXPECT(b == GPBO_ERR_ARG || (b > 0 && b % 256 == 0));
            ++queries;
        };
        granules(gpbo_acq_workspace_bytes());
        for (int64_t Np : NP) {
            granules(gpbo_prepare_i8_bytes(Np));
            granules(gpbo_loo_workspace_bytes(Np));
            granules(gpbo_fps_order_workspace_bytes(Np + 2));
            EXPECT(gpbo_factorise_workspace_bytes(Np) >= 0 && gpbo_append_workspace_bytes(Np) != 0);
            for (int64_t chunk : CHUNK)
                for (int64_t M : MM) {
                    granules(gpbo_posterior_workspace_bytes(Np, chunk, M));
                    granules(gpbo_qei_workspace_bytes(Np, chunk, M));
                    granules(gpbo_posterior_workspace_bytes_f32(Np, chunk, M));
                    granules(gpbo_posterior_workspace_bytes_i8(Np, chunk, M));
                    granules(gpbo_ensemble_workspace_bytes(Np, chunk, M));
                    for (int32_t S : QS) granules(gpbo_posterior_nei_workspace_bytes(Np, chunk, M, S));
                }
            for (int64_t chunk : CHUNK)
                for (int64_t cap : CAP) granules(gpbo_rescore_workspace_bytes(Np, cap, chunk));
            for (int32_t S : QS) {
                granules(gpbo_nei_fantasies_workspace_bytes(Np, S));
                for (int64_t M : MM) granules(gpbo_batch_workspace_bytes(Np, M, S));
                for (int32_t F : FS) {
                    granules(gpbo_thompson_weights_workspace_bytes(Np, F, S));
                    for (int64_t M : MM) granules(gpbo_thompson_paths_workspace_bytes(Np, M, F, S));
                }
            }
            for (int64_t P : PS) {
                granules(gpbo_posterior_grad_workspace_bytes(Np, P));
                granules(gpbo_refine_workspace_bytes(Np, P));
            }
            for (int32_t d : DS) {
                granules(gpbo_nlml_grad_workspace_bytes(Np, d));
                granules(gpbo_nlml_hyper_workspace_bytes(Np, d));
            }
        }
        EXPECT(queries == 1 + 7 * 625);
    }
    // host-pointer entry points: refused before the first HIP call
    gpbo_result res;
    int32_t info_h = 0;
    EXPECT(gpbo_select_next_host_f64(nullptr, nullptr, 0, 0, nullptr, 0, 0, nullptr, 0, 0, 0, 0, 0, 0, nullptr, nullptr, nullptr,
                                     nullptr, &res, &info_h) == GPBO_ERR_ARG);
    EXPECT(gpbo_select_qei_host_f64(nullptr, nullptr, 0, 0, nullptr, 0, 0, nullptr, 0, 0, 0, nullptr, 0, 0, nullptr, &res,
                                    &info_h) == GPBO_ERR_ARG);
    EXPECT(gpbo_nlml_grid_host_f64(nullptr, nullptr, 0, 0, nullptr, 0, 0, nullptr) == GPBO_ERR_ARG);
    EXPECT(gpbo_nlml_grid_logdet_host_f64(nullptr, nullptr, 0, 0, nullptr, 0, 0, nullptr) == GPBO_ERR_ARG);
    EXPECT(gpbo_nlml_grad_host_f64(nullptr, nullptr, 0, 0, nullptr, 0, nullptr) == GPBO_ERR_ARG);
    EXPECT(gpbo_select_batch_host_f64(nullptr, nullptr, 0, 0, nullptr, 0, 0, nullptr, 0, 0, 0, 0, 0, 0, 0, 0, nullptr, nullptr,
                                      nullptr, nullptr, &res, &info_h) == GPBO_ERR_ARG);
    EXPECT(gpbo_refine_host_f64(nullptr, nullptr, 0, 0, nullptr, 0, 0, nullptr, 0, nullptr, nullptr, 0, 0, 0, 0, 0, nullptr,
                                nullptr, nullptr, nullptr, &res, &info_h) == GPBO_ERR_ARG);
    if (fails) {
        std::fprintf(stderr, "sanitize_host: %d check(s) failed\n", fails);
        return 1;
    }
    std::printf("sanitize_host ok: %ld plans (%ld tiles) built and checked, argument tables refused on the host\n", plans, tiles_seen);
    return 0;
}
