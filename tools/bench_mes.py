"""Cost and effect of max-value entropy search (DeviceGP.log_survival / mes_on_posterior, csrc/mes.hip), recorded - nothing is
asserted.  Device-event times around the C calls alone (inputs on the device, no read-back inside the window), warm-up first, the
routes alternated ROUNDS times; medians, with every sample reported.
  headline  d = 8, N = 4096, M = 2^21 on one surrogate, on the posterior (mu, sigma) its dense pass has left on the device:
      survival_q63_ms  gpbo_mes_log_survival_f64 with 63 levels (one round of the quartile search; a call makes four)
      acq_ms           gpbo_mes_acq_f64 with the dense store, S = 16 and 64
      ei_ms            gpbo_acq_argmax_f64 with EI and the dense store over the same M: the pass PointSelector makes for another
                       acquisition on an existing posterior (sigma_acq.hip is the parent commit's, byte for byte; --parent-lib
                       times a library built from the parent beside it)
      mes_call_wall_ms the selection on an existing posterior: brackets, four rounds, samples, MES with the dense store, read-back
                       of the 32-byte record (DeviceGP.mes_minima + mes_on_posterior; wall clock).  The dense values stay on the device.
      mes_call_with_readback_wall_ms  the same plus the copy of the dense values to the host (8 M bytes), which
                       PointSelector.max_value_entropy_search() makes for acq_func_eval
      dense_step_ms    the dense scoring pass itself (DeviceGP.score(dense=True)): what update_surrogate() pays before any of it
      terms_per_s / GBps: log Phi (or h) evaluations per second and the bytes of mu, sigma and the dense store per second, beside
                       the chip's 8 TB/s: which of VALU issue and memory the kernel sits at
  quality   --quality: the 25-step BO loops of tools/bench_nei.py (noisy random-Fourier-feature objective in d = 2, noise sd 0.3,
            fixed length scales (0.3, 1.0), rho = 0.09, 5 starting points, 1,500 uniform candidates, 20 seeds) for EI with
            f_best = min(y), NEI (S = 16) and MES (S = 16, Gumbel samples, cap = min(y)) side by side: regret = the objective's
            noise-free value at the visited point with the smallest posterior mean minus the smallest noise-free value over the
            candidates, and the number of distinct points visited
usage: python tools/bench_mes.py [--rounds 5] [--parent-lib ab_libs/parent.so] [--quality] [--skip-headline]
                                 [--out profiles/mes_bench_line.json]"""
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

from bayesian_optimisation_amd import DeviceGP, _lib  # noqa: E402
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


def headline(rounds, parent):
    X, y, Xs, ls = make_problem(N, M, D)
    gp = DeviceGP(chunk=CHUNK).factorise(X, y, ls, 0.09, 0.0)
    Xsd = gp._dev(Xs)
    lib, p = gp.lib, gp._ptr
    pv = 1.0 + 0.09
    s = gp.score(Xsd, acquisition="lcb", explore=0.0, dense=True, prior_var=pv)
    mu, sg = s.mu, s.sigma
    f_best = float(gp.y[: gp.N].min().item())
    work = torch.empty(_lib.MES_WORK_BYTES // 8, dtype=torch.float64, device=gp.device)
    acq = torch.empty(M, dtype=torch.float64, device=gp.device)
    out = torch.empty(65, dtype=torch.float64, device=gp.device)
    res = torch.zeros(4, dtype=torch.int64, device=gp.device)
    lo = float((mu - 10.0 * sg).min().item())
    hi = float((mu + 0.6744897501960817 * sg).min().item())
    z = np.ascontiguousarray(np.concatenate([np.linspace(lo, hi, 21)] * 3))
    ys = np.ascontiguousarray(np.linspace(lo, hi, 64)[::-1] * 0.5 + 0.5 * lo)

    def survival(Q):
        def run():
            st = lib.gpbo_mes_log_survival_f64(p(mu), p(sg), M, z[:Q].ctypes.data_as(C.c_void_p), Q, p(out), p(out[64:]), p(work),
                                               _lib.MES_WORK_BYTES, gp._stream())
            assert st == 0
        return run

    def mes(S):
        def run():
            st = lib.gpbo_mes_acq_f64(p(mu), p(sg), M, ys[:S].ctypes.data_as(C.c_void_p), S, 0, p(acq), p(res), p(work),
                                      _lib.MES_WORK_BYTES, gp._stream())
            assert st == 0
        return run

    def ei(l=lib):
        def run():
            wb = int(l.gpbo_acq_workspace_bytes())
            st = l.gpbo_acq_argmax_f64(p(mu), p(sg), M, _lib.ACQ_EI, f_best, 0.0, 0, p(acq), p(res), p(work), wb, gp._stream())
            assert st == 0
        return run

    routes = dict(survival_q63=survival(63), acq_s16=mes(16), acq_s64=mes(64), ei=ei())
    if parent is not None:
        for name in ("gpbo_acq_argmax_f64", "gpbo_acq_workspace_bytes"):
            fn = getattr(parent, name)
            fn.restype, fn.argtypes = _lib.SIGNATURES[name]
        routes["ei_parent"] = ei(parent)
    for fn in routes.values():   # warm-up: every code object of the timed window
        fn()
    torch.cuda.synchronize()
    t = {k: [] for k in routes}
    for _ in range(rounds):
        for k, fn in routes.items():
            t[k].append(timed(fn)[0])
    line = {k + "_ms": spread(v) for k, v in t.items()}
    med = {k: statistics.median(v) for k, v in t.items()}
    for k, terms, nbytes in (("survival_q63", 63 * M, 16 * M), ("acq_s16", 16 * M, 24 * M), ("acq_s64", 64 * M, 24 * M),
                             ("ei", M, 24 * M)):
        line[k + "_terms_per_s"] = terms / (med[k] / 1e3)
        line[k + "_GBps"] = nbytes / 1e9 / (med[k] / 1e3)
    # the whole call on an existing posterior, and the dense step in front of it (wall clock, synchronised)
    cap = f_best
    wall, back, dense = [], [], []
    for r in range(rounds + 1):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        m, _ = gp.mes_minima(mu, sg, Xsd, 16, r, "gumbel", cap)
        res_mes = gp.mes_on_posterior(mu, sg, m)
        tb = time.perf_counter()
        res_mes.acq.cpu().numpy()
        t1 = time.perf_counter()
        gp.score(Xsd, acquisition="lcb", explore=4.0, dense=True, prior_var=pv)
        torch.cuda.synchronize()
        t2 = time.perf_counter()
        if r:
            wall.append((tb - t0) * 1e3)
            back.append((t1 - t0) * 1e3)
            dense.append((t2 - t1) * 1e3)
    line.update(mes_call_wall_ms=spread(wall), mes_call_with_readback_wall_ms=spread(back), dense_step_ms=spread(dense), N=N, M=M, d=D, chunk=CHUNK, rho=0.09,
                hbm_GBps=HBM_GBPS, parent_lib=None if parent is None else parent._name)
    return line


def quality(seeds=20, steps=25, n_cand=1500, n0=5, noise=0.3):
    ls, rho = np.array([0.3, 1.0]), 0.09
    rows = {"ei": [], "nei": [], "mes": []}
    gp = DeviceGP()
    for seed in range(seeds):
        rng = np.random.default_rng(100 + seed)
        Xs = rng.uniform(0, 1, (n_cand, 2))
        om = rng.standard_normal((256, 2)) / ls[None, :]
        ph, w = rng.uniform(0, 2 * np.pi, 256), rng.standard_normal(256)
        f = np.sqrt(2.0 / 256) * (np.cos(Xs @ om.T + ph[None, :]) @ w)          # the noise-free objective at the candidates
        eps = noise * rng.standard_normal((steps + n0, n_cand))                  # the noise of evaluation t at candidate c
        start = rng.choice(n_cand, n0, replace=False)
        for how in rows:
            visited = list(start)
            for t in range(steps):
                idx = np.asarray(visited)
                yv = f[idx] + eps[np.arange(len(idx)), idx]
                gp.factorise(Xs[idx], yv, ls, rho, 0.0)
                if how == "ei":
                    nxt = gp.score(Xs, acquisition="ei", f_best=float(yv.min()), prior_var=1.0 + rho).best_idx
                elif how == "nei":
                    nxt = gp.select_nei(Xs, n_fantasies=16, seed=t).best_idx
                else:
                    nxt = gp.select_mes(Xs, n_samples=16, seed=t).best_idx
                visited.append(int(nxt))
            idx = np.asarray(visited)
            yv = f[idx] + eps[np.arange(len(idx)), idx]
            gp.factorise(Xs[idx], yv, ls, rho, 0.0)
            mu = gp.score(Xs[idx], acquisition="lcb", explore=0.0, dense=True, prior_var=1.0 + rho).mu.cpu().numpy()
            rows[how].append(dict(regret=float(f[idx[int(np.argmin(mu))]] - f.min()), distinct=len(set(visited))))
    return {how: dict(mean_regret=float(np.mean([r["regret"] for r in v])), median_regret=float(np.median([r["regret"] for r in v])),
                      mean_distinct=float(np.mean([r["distinct"] for r in v])), regrets=[round(r["regret"], 4) for r in v],
                      distinct=[r["distinct"] for r in v]) for how, v in rows.items()} | dict(
        seeds=seeds, steps=steps, candidates=n_cand, start_points=n0, noise_sd=noise, rho=rho, ls=ls.tolist(), n_samples=16)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--parent-lib", default=None)
    ap.add_argument("--quality", action="store_true")
    ap.add_argument("--skip-headline", action="store_true")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "mes_bench_line.json"))
    a = ap.parse_args()
    line = dict(tool="tools/bench_mes.py", device=torch.cuda.get_device_name(0), rounds=a.rounds)
    if not a.skip_headline:
        parent = C.CDLL(os.path.abspath(a.parent_lib)) if a.parent_lib else None
        line["headline"] = headline(a.rounds, parent)
        torch.cuda.empty_cache()
    if a.quality:
        line["quality"] = quality()
    with open(a.out, "w") as fh:
        json.dump(line, fh, indent=1)
        fh.write("\n")
    print(json.dumps(line))


if __name__ == "__main__":
    main()
