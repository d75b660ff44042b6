"""Cost and effect of two-objective expected hypervolume improvement in log space (DeviceGP.ehvi_on_posterior / select_ehvi,
csrc/ehvi.hip), recorded - nothing is asserted.
  headline  M = 2^21 candidates on synthetic dense posteriors on the device (the kernel reads nothing else): means in [-2, 2],
            sigma in [0.05, 2], fronts of P points spread evenly over [-1.5, 1.5]^2 below r = (2, 2), so every branch of log h
            runs.  Device-event times around the C call alone (no read-back inside the window), warm-up first, the routes
            alternated ROUNDS times; medians, with every sample reported.
      ehvi_p{0,8,32,128}_ms  gpbo_ehvi_acq_f64 with its dense store, P front points (P + 1 strips, 2 (P + 1) log h)
      cons_c8_ms             gpbo_constrained_acq_f64, base EI, C = 8, both dense stores, over the same arrays  } the neighbours
      mes_s16_ms             gpbo_mes_acq_f64, S = 16, dense store, over the same mu / sigma                   } it is shaped like
      *_log_h_per_s          log h evaluations per second; *_strips_per_s strips per second (a strip: 2 log h, one log(1 - exp),
                             one exp of the running sum); the neighbours' *_terms_per_s: their log-terms (1 + C, S) per second
      *_GBps                 bytes read and written per second, beside the chip's 8 TB/s
  quality   --quality: closed loops on a 2-d toy with TWO objectives, 20 seeds, 25 steps from 5 starting points, 1,500 uniform
            candidates: both objectives are random-Fourier-feature draws (length scales (0.3, 1.0)), observed with noise sd 0.05.
            Surrogates with fixed length scales and rho = 0.0025.  The reference point is fixed per seed: per objective the
            largest noise-free value over the candidates plus 10 % of the range.  "ehvi": DeviceGP.select_ehvi (the front of the
            noisy observations); "weighted_ei": ONE surrogate on 0.5 y1 + 0.5 y2 with EI against its smallest observation;
            "random": uniform candidates.  Reported: the hypervolume the noise-free values of the visited points dominate at
            the end, as a share of what the whole candidate set dominates.
usage: python tools/bench_ehvi.py [--rounds 5] [--quality] [--skip-headline] [--out profiles/ehvi_bench_line.json]"""
import argparse
import ctypes as C
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402
import torch  # noqa: E402

from bayesian_optimisation_amd import DeviceGP, _lib  # noqa: E402
from bayesian_optimisation_amd.pareto import hypervolume  # noqa: E402

M = 1 << 21
HBM_GBPS = 8000.0
COUNTS = (0, 8, 32, 128)


def timed(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b)


def spread(v):
    return dict(median=statistics.median(v), min=min(v), max=max(v), all=[round(x, 4) for x in v])


def headline(rounds):
    gp = DeviceGP()
    lib, p = gp.lib, gp._ptr
    rng = np.random.default_rng(0)
    mu, sg = gp._dev(rng.uniform(-2.0, 2.0, M)), gp._dev(np.exp(rng.uniform(np.log(0.05), np.log(2.0), M)))
    cm, cs = gp._dev(rng.uniform(-2.0, 2.0, (8, M))), gp._dev(np.exp(rng.uniform(np.log(0.05), np.log(2.0), (8, M))))
    upper = np.ascontiguousarray(rng.uniform(-0.5, 0.5, 8))
    ys = np.ascontiguousarray(np.linspace(-2.0, 2.0, 16))
    fronts = {P: np.ascontiguousarray(np.stack([np.linspace(-1.5, 1.5, P), np.linspace(1.5, -1.5, P)], axis=1)) for P in COUNTS}
    val, feas = (torch.empty(M, dtype=torch.float64, device=gp.device) for _ in range(2))
    res = torch.zeros(4, dtype=torch.int64, device=gp.device)
    work = torch.empty(_lib.MES_WORK_BYTES // 8, dtype=torch.float64, device=gp.device)

    def ehvi(P):
        def run():
            st = lib.gpbo_ehvi_acq_f64(p(mu), p(sg), p(cm[0]), p(cs[0]), M, fronts[P].ctypes.data_as(C.c_void_p), P, 2.0, 2.0, 0,
                                       p(val), p(res), p(work), _lib.EHVI_WORK_BYTES, gp._stream())
            assert st == 0
        return run

    def cons():
        st = lib.gpbo_constrained_acq_f64(p(mu), p(sg), M, _lib.CONS_BASE_EI, 0.0, 0.01, p(cm), p(cs), M, 8,
                                          upper.ctypes.data_as(C.c_void_p), 0, p(val), p(feas), p(res), p(work),
                                          _lib.CONS_WORK_BYTES, gp._stream())
        assert st == 0

    def mes():
        st = lib.gpbo_mes_acq_f64(p(mu), p(sg), M, ys.ctypes.data_as(C.c_void_p), 16, 0, p(val), p(res), p(work),
                                  _lib.MES_WORK_BYTES, gp._stream())
        assert st == 0

    routes = {f"ehvi_p{P}": ehvi(P) for P in COUNTS}
    routes.update(cons_c8=cons, mes_s16=mes)
    for fn in routes.values():   # warm-up: every code object of the timed window
        fn()
    torch.cuda.synchronize()
    t = {k: [] for k in routes}
    for _ in range(rounds):
        for k, fn in routes.items():
            t[k].append(timed(fn))
    line = {k + "_ms": spread(v) for k, v in t.items()}
    med = {k: statistics.median(v) / 1e3 for k, v in t.items()}
    for P in COUNTS:
        k = f"ehvi_p{P}"
        line[k + "_log_h_per_s"] = 2 * (P + 1) * M / med[k]
        line[k + "_strips_per_s"] = (P + 1) * M / med[k]
        line[k + "_GBps"] = 5 * 8 * M / 1e9 / med[k]
    line["cons_c8_terms_per_s"], line["cons_c8_GBps"] = 9 * M / med["cons_c8"], (2 + 16 + 2) * 8 * M / 1e9 / med["cons_c8"]
    line["mes_s16_terms_per_s"], line["mes_s16_GBps"] = 16 * M / med["mes_s16"], 3 * 8 * M / 1e9 / med["mes_s16"]
    line.update(M=M, hbm_GBps=HBM_GBPS, nan_count=int(res.cpu()[2]))
    return line


def _rff(rng, Xs, ls):
    om = rng.standard_normal((256, 2)) / ls[None, :]
    ph, w = rng.uniform(0, 2 * np.pi, 256), rng.standard_normal(256)
    return np.sqrt(2.0 / 256) * (np.cos(Xs @ om.T + ph[None, :]) @ w)


def quality(seeds=20, steps=25, n_cand=1500, n0=5, noise=0.05):
    ls, rho = np.array([0.3, 1.0]), 0.0025
    rows = {"ehvi": [], "weighted_ei": [], "random": []}
    g1, g2 = DeviceGP(), DeviceGP()
    for seed in range(seeds):
        rng = np.random.default_rng(200 + seed)
        Xs = rng.uniform(0, 1, (n_cand, 2))
        F = np.stack([_rff(rng, Xs, ls), _rff(rng, Xs, ls)], axis=1)          # noise-free objectives at the candidates
        ref = tuple(float(v) for v in F.max(axis=0) + 0.1 * (F.max(axis=0) - F.min(axis=0)))
        total = hypervolume(F, ref)
        eps = noise * rng.standard_normal((2, steps + n0, n_cand))
        start = rng.choice(n_cand, n0, replace=False)
        pick = rng.choice(n_cand, steps, replace=False)
        for how in rows:
            visited = list(start)
            for s in range(steps):
                idx = np.asarray(visited)
                k = np.arange(len(idx))
                y1, y2 = F[idx, 0] + eps[0, k, idx], F[idx, 1] + eps[1, k, idx]
                if how == "ehvi":
                    g1.factorise(Xs[idx], y1, ls, rho, 0.0)
                    g2.factorise(Xs[idx], y2, ls, rho, 0.0)
                    nxt = g1.select_ehvi(Xs, g2, ref=ref).best_idx
                elif how == "weighted_ei":
                    y = 0.5 * y1 + 0.5 * y2
                    g1.factorise(Xs[idx], y, ls, rho, 0.0)
                    nxt = g1.score(Xs, acquisition="ei", f_best=float(y.min()), prior_var=1.0 + rho).best_idx
                else:
                    nxt = pick[s]
                visited.append(int(nxt))
            rows[how].append(dict(share=hypervolume(F[np.asarray(visited)], ref) / total, distinct=len(set(visited))))
    out = {}
    for how, v in rows.items():
        sh = [r["share"] for r in v]
        out[how] = dict(mean_hypervolume_share=float(np.mean(sh)), median_hypervolume_share=float(np.median(sh)),
                        min_hypervolume_share=float(np.min(sh)), mean_distinct=float(np.mean([r["distinct"] for r in v])),
                        shares=[round(x, 4) for x in sh])
    return out | dict(seeds=seeds, steps=steps, candidates=n_cand, start_points=n0, noise_sd=noise, rho=rho, ls=ls.tolist(),
                      reference_point="largest noise-free value over the candidates + 10 % of the range, per objective",
                      share_of="the hypervolume the whole candidate set dominates")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--quality", action="store_true")
    ap.add_argument("--skip-headline", action="store_true")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "ehvi_bench_line.json"))
    a = ap.parse_args()
    line = dict(tool="tools/bench_ehvi.py", device=torch.cuda.get_device_name(0), rounds=a.rounds)
    if not a.skip_headline:
        line["headline"] = headline(a.rounds)
        torch.cuda.empty_cache()
    if a.quality:
        line["quality"] = quality()
    with open(a.out, "w") as fh:
        json.dump(line, fh, indent=1)
        fh.write("\n")
    print(json.dumps(line))


if __name__ == "__main__":
    main()
