"""Cost and effect of noisy expected improvement (DeviceGP.fantasies / score_nei, csrc/nei.hip), recorded - nothing is asserted.
Device-event times around the C calls alone (inputs on the device, no read-back inside the window), warm-up first, the routes
alternated ROUNDS times; medians, with every sample reported.
  headline  d = 8, N = 4096, M = 2^21, S = 16 and 64 on one surrogate:
      ei_ms         gpbo_posterior_acq_kern_f64 with EI, no dense outputs: the pass every acquisition call makes
      ei_parent_ms  the same call in --parent-lib (a library built from the parent commit, loaded beside this one), when given
      nei_score_ms  gpbo_posterior_nei_kern_f64: the pass on the twin + nei_kernel per chunk + the finish
      twin_pass_ms  gpbo_posterior_acq_kern_f64 on the twin's factor with dense mu / sigma: the part of nei_score_ms that is not new
      nei_kernel_ms_per_chunk = (nei_score_ms - twin_pass_ms) / chunks: nei_kernel (and 1 / chunks of the prep and finish
                    launches) per chunk of 2^17 candidates; image_GBps = N * 2^17 * 8 bytes over that time, beside 8 TB/s
      fantasies_ms  gpbo_nei_fantasies_f64;  twin_ms  the second factorisation (both once per factorisation)
      select_nei_over_ei = (nei_score_ms + fantasies_ms + twin_ms) / ei_ms
  small     the fantasies entry and the twin factorisation at N = 512 and 4096 (S = 16); the reference's shape - N = 32, d = 2,
            50 x 50 candidates - through PointSelector: expected_improvement() and noisy_expected_improvement() (wall clock)
  quality   --quality: 25-step BO loops on a noisy random-Fourier-feature objective in d = 2 (noise sd 0.3, fixed length scales
            (0.3, 1.0), rho = 0.09, 5 starting points, 1,500 uniform candidates, 20 seeds), EI with f_best = min(y) against NEI
            (S = 16): regret = the objective's noise-free value at the visited point with the smallest posterior mean minus the
            smallest noise-free value over the candidates, and the number of distinct points visited
usage: python tools/bench_nei.py [--rounds 5] [--parent-lib ab_libs/parent.so] [--quality] [--skip-headline]
                                 [--out profiles/nei_bench_line.json]"""
import argparse
import ctypes as C
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402
import torch  # noqa: E402

from bayesian_optimisation_amd import DeviceGP, PointSelector, _lib  # noqa: E402
from bayesian_optimisation_amd.synthetic import make_problem  # noqa: E402

N, M, D, CHUNK = 4096, 1 << 21, 8, 1 << 17
HBM_GBPS = 8000.0


def timed(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    out = fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b), out


def spread(v):
    return dict(median=statistics.median(v), min=min(v), max=max(v), all=[round(x, 4) for x in v])


def twin_factorise(gp, delta=1e-6):
    """A callable that factorises the twin into buffers of its own (what DeviceGP.fantasies enqueues first)."""
    lib, p = gp.lib, gp._ptr
    K0 = torch.empty((gp.Np, gp.Np), dtype=torch.float64, device=gp.device)
    U0, a0 = torch.empty_like(K0), torch.empty(gp.Np, dtype=torch.float64, device=gp.device)
    info = torch.zeros(1, dtype=torch.int32, device=gp.device)
    wb = int(lib.gpbo_factorise_workspace_bytes(gp.Np))
    work = torch.empty(wb // 8 + 1, dtype=torch.float64, device=gp.device)
    lsp = gp.ls_h.ctypes.data_as(C.c_void_p)

    def run():
        _lib.check(lib.gpbo_factorise_kern_f64(p(gp.X), p(gp.y), gp.N, gp.d, lsp, gp._kid(), delta, 0.0, gp.Np, p(K0), p(U0), p(a0),
                                               p(info), p(work), wb, gp._stream()), "twin")
    return run


def headline(S, rounds, gp, Xsd, parent):
    lib, p = gp.lib, gp._ptr
    lsp = gp.ls_h.ctypes.data_as(C.c_void_p)
    fan = gp.fantasies(S, seed=0)
    res = torch.zeros(4, dtype=torch.int64, device=gp.device)
    wpost = int(lib.gpbo_posterior_workspace_bytes(gp.Np, CHUNK, M))
    wnei = int(lib.gpbo_posterior_nei_workspace_bytes(gp.Np, CHUNK, M, S))
    wfan = int(lib.gpbo_nei_fantasies_workspace_bytes(gp.Np, S))
    work = torch.empty(max(wpost, wnei, wfan) // 8 + 1, dtype=torch.float64, device=gp.device)
    mu, sg = (torch.empty(M, dtype=torch.float64, device=gp.device) for _ in range(2))
    Z, E = (torch.randn((S, gp.N), dtype=torch.float64, device=gp.device) for _ in range(2))
    A, F = (torch.empty((S, gp.Np), dtype=torch.float64, device=gp.device) for _ in range(2))
    best = torch.empty(S, dtype=torch.float64, device=gp.device)
    f_best = float(gp.y.min().item())
    noise_sd = float(np.sqrt(gp.jitter1 + gp.jitter2 - fan.delta))

    def ei(l=lib):
        st = l.gpbo_posterior_acq_kern_f64(p(Xsd), M, p(gp.X), gp.N, gp.Np, D, lsp, 0, p(gp.U), p(gp.alpha), 1.0 + gp.jitter1 + gp.jitter2,
                                           _lib.ACQ_EI, f_best, 0.0, 0.0, 0, CHUNK, None, None, None, p(res), p(work), wpost, None,
                                           gp._stream())
        assert st == 0

    def ei_parent():
        fn = parent.gpbo_posterior_acq_kern_f64
        fn.restype, fn.argtypes = _lib.SIGNATURES["gpbo_posterior_acq_kern_f64"]
        ei(parent)

    def twin_pass():
        st = lib.gpbo_posterior_acq_kern_f64(p(Xsd), M, p(gp.X), gp.N, gp.Np, D, lsp, 0, p(fan.U0), p(fan.A), 1.0 + fan.delta,
                                             _lib.ACQ_LCB, 0.0, 0.0, 0.0, 0, CHUNK, p(mu), p(sg), None, p(res), p(work), wpost, None,
                                             gp._stream())
        assert st == 0

    def nei_score():
        st = lib.gpbo_posterior_nei_kern_f64(p(Xsd), M, p(gp.X), gp.N, gp.Np, D, lsp, 0, p(fan.U0), p(fan.A), p(fan.best), S,
                                             1.0 + fan.delta, 0.0, 0, CHUNK, None, M, None, None, p(res), p(work), wnei, gp._stream())
        assert st == 0

    def fantasies():
        st = lib.gpbo_nei_fantasies_f64(p(fan.K0d), p(fan.U0), p(gp.U), p(gp.y), gp.N, gp.Np, p(Z), p(E), noise_sd, S, p(A), p(F),
                                        p(best), p(work), wfan, gp._stream())
        assert st == 0

    twin = twin_factorise(gp)
    routes = dict(ei=ei, twin_pass=twin_pass, nei_score=nei_score, fantasies=fantasies, twin=twin)
    if parent is not None:
        routes["ei_parent"] = ei_parent
    for fn in routes.values():   # warm-up: every shape and code object of the timed window
        fn()
    torch.cuda.synchronize()
    t = {k: [] for k in routes}
    for _ in range(rounds):
        for k, fn in routes.items():
            t[k].append(timed(fn)[0])
    out = {k + "_ms": spread(v) for k, v in t.items()}
    med = {k: statistics.median(v) for k, v in t.items()}
    chunks = M // CHUNK
    per_chunk = (med["nei_score"] - med["twin_pass"]) / chunks
    out.update(S=S, chunks=chunks, nei_kernel_ms_per_chunk=per_chunk,
               image_GBps=N * CHUNK * 8 / 1e9 / (per_chunk / 1e3) if per_chunk > 0 else None, hbm_GBps=HBM_GBPS,
               nei_score_over_ei=med["nei_score"] / med["ei"],
               select_nei_over_ei=(med["nei_score"] + med["fantasies"] + med["twin"]) / med["ei"])
    if parent is not None:
        out["select_nei_over_parent_ei"] = (med["nei_score"] + med["fantasies"] + med["twin"]) / med["ei_parent"]
        out["ei_over_parent_ei"] = med["ei"] / med["ei_parent"]
    return out


def small(rounds):
    out = {}
    for n in (512, 4096):
        X, y, _, ls = make_problem(n, 8, D)
        gp = DeviceGP(chunk=CHUNK).factorise(X, y, ls, 0.09, 0.0)
        twin = twin_factorise(gp)
        twin(), gp.fantasies(16)
        torch.cuda.synchronize()
        tt = [timed(twin)[0] for _ in range(rounds)]
        tf = []
        for _ in range(rounds):   # (wall clock of the whole method minus the twin: the draws' upload is part of it)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            gp.fantasies(16)
            torch.cuda.synchronize()
            tf.append((time.perf_counter() - t0) * 1e3)
        out[f"N{n}"] = dict(twin_ms=spread(tt), fantasies_method_wall_ms=spread(tf))
    # the reference's shape through the drop-in class
    rng = np.random.default_rng(0)
    X = rng.uniform(0, 1, (32, 2))
    y = np.sin(6 * X[:, 0]) * np.cos(4 * X[:, 1]) + 0.3 * rng.standard_normal(32)
    g = (np.arange(50) + 0.5) / 50
    ps = PointSelector()
    ps.measured_pts, ps.measured_vals, ps.feature_domain = X, y, [50, 50]
    ps.predicted_pts = np.stack(np.meshgrid(g, g, indexing="ij"), -1).reshape(-1, 2)
    ps.set_kernel_params([0.3, 0.3])
    te, tn = [], []
    for r in range(rounds + 1):
        ps.update_surrogate()
        t0 = time.perf_counter()
        ps.expected_improvement(xi=1e-3 * r)          # (another key every round: never served from the cache)
        t1 = time.perf_counter()
        ps.noisy_expected_improvement(seed=r)
        t2 = time.perf_counter()
        if r:
            te.append((t1 - t0) * 1e3)
            tn.append((t2 - t1) * 1e3)
    out["reference_shape_N32_d2_50x50"] = dict(expected_improvement_wall_ms=spread(te), noisy_expected_improvement_wall_ms=spread(tn))
    return out


def quality(seeds=20, steps=25, n_cand=1500, n0=5, noise=0.3):
    ls, rho = np.array([0.3, 1.0]), 0.09
    rows = {"ei": [], "nei": []}
    gp = DeviceGP()
    for seed in range(seeds):
        rng = np.random.default_rng(100 + seed)
        Xs = rng.uniform(0, 1, (n_cand, 2))
        om = rng.standard_normal((256, 2)) / ls[None, :]
        ph, w = rng.uniform(0, 2 * np.pi, 256), rng.standard_normal(256)
        f = np.sqrt(2.0 / 256) * (np.cos(Xs @ om.T + ph[None, :]) @ w)          # the noise-free objective at the candidates
        eps = noise * rng.standard_normal((steps + n0, n_cand))                  # the noise of evaluation t at candidate c
        start = rng.choice(n_cand, n0, replace=False)
        for how in ("ei", "nei"):
            visited = list(start)
            for t in range(steps):
                idx = np.asarray(visited)
                yv = f[idx] + eps[np.arange(len(idx)), idx]
                gp.factorise(Xs[idx], yv, ls, rho, 0.0)
                if how == "ei":
                    nxt = gp.score(Xs, acquisition="ei", f_best=float(yv.min()), prior_var=1.0 + rho).best_idx
                else:
                    nxt = gp.select_nei(Xs, n_fantasies=16, seed=t).best_idx
                visited.append(int(nxt))
            idx = np.asarray(visited)
            yv = f[idx] + eps[np.arange(len(idx)), idx]
            gp.factorise(Xs[idx], yv, ls, rho, 0.0)
            mu = gp.score(Xs[idx], acquisition="lcb", explore=0.0, dense=True, prior_var=1.0 + rho).mu.cpu().numpy()
            rows[how].append(dict(regret=float(f[idx[int(np.argmin(mu))]] - f.min()), distinct=len(set(visited))))
    return {how: dict(mean_regret=float(np.mean([r["regret"] for r in v])), median_regret=float(np.median([r["regret"] for r in v])),
                      mean_distinct=float(np.mean([r["distinct"] for r in v])), regrets=[round(r["regret"], 4) for r in v],
                      distinct=[r["distinct"] for r in v]) for how, v in rows.items()} | dict(
        seeds=seeds, steps=steps, candidates=n_cand, start_points=n0, noise_sd=noise, rho=rho, ls=ls.tolist(), n_fantasies=16)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--parent-lib", default=None)
    ap.add_argument("--quality", action="store_true")
    ap.add_argument("--skip-headline", action="store_true")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "nei_bench_line.json"))
    a = ap.parse_args()
    line = dict(tool="tools/bench_nei.py", device=torch.cuda.get_device_name(0), rounds=a.rounds)
    if not a.skip_headline:
        parent = C.CDLL(os.path.abspath(a.parent_lib)) if a.parent_lib else None
        X, y, Xs, ls = make_problem(N, M, D)
        gp = DeviceGP(chunk=CHUNK).factorise(X, y, ls, 0.09, 0.0)
        Xsd = gp._dev(Xs)
        line["headline"] = dict(N=N, M=M, d=D, chunk=CHUNK, rho=0.09, delta=1e-6, parent_lib=a.parent_lib,
                                runs=[headline(S, a.rounds, gp, Xsd, parent) for S in (16, 64)])
        del gp, Xsd
        torch.cuda.empty_cache()
    line["small"] = small(a.rounds)
    if a.quality:
        line["quality"] = quality()
    with open(a.out, "w") as fh:
        json.dump(line, fh, indent=1)
        fh.write("\n")
    print(json.dumps(line))


if __name__ == "__main__":
    main()
