"""Cost and effect of the constrained acquisitions in log space (DeviceGP.constrained_on_posterior / select_constrained,
csrc/constrained.hip), recorded - nothing is asserted.
  headline  M = 2^21 candidates on synthetic dense posteriors on the device (the kernel reads nothing else): z and every gamma
            spread over [-40, 40], so all branches of log h and log Phi run.  Device-event times around the C call alone (no
            read-back inside the window), warm-up first, the routes alternated ROUNDS times; medians, with every sample reported.
      cons_c{0,1,4,8}_ms   gpbo_constrained_acq_f64, base EI, both dense stores, C constraints
      pof_c8_ms            the same without a base (the probability of feasibility alone), C = 8
      mes_s16_ms           gpbo_mes_acq_f64 with S = 16 and its dense store over the same mu / sigma: the neighbour it is shaped like
      terms_per_s / GBps   log-terms (1 + C) per second and the bytes read and written per second, beside the chip's 8 TB/s: which
                           of VALU issue and memory the kernel sits at
  quality   --quality: closed loops on a 2-d toy with ONE constraint, 20 seeds, 25 steps from 5 starting points, 1,500 uniform
            candidates: the objective f and the constraint g are random-Fourier-feature draws (length scales (0.3, 1.0)), both
            observed with noise sd 0.1; feasible means g(x) <= the median of g over the candidates (half of them).  Two
            surrogates with fixed length scales and rho = 0.01.  "cei": DeviceGP.select_constrained (feasible incumbent, the
            probability of feasibility alone while no observation is feasible); "ei": plain EI on the objective with
            f_best = min(y), blind to the constraint.  Reported: the share of the 25 evaluations that are truly feasible
            (noise-free g), and the feasible regret = the smallest noise-free f among the truly feasible visited points minus the
            smallest noise-free f among the feasible candidates (runs that visit no feasible point are counted apart).
usage: python tools/bench_constrained.py [--rounds 5] [--quality] [--skip-headline] [--out profiles/constrained_bench_line.json]"""
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

M = 1 << 21
HBM_GBPS = 8000.0


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
    val, feas = (torch.empty(M, dtype=torch.float64, device=gp.device) for _ in range(2))
    res = torch.zeros(4, dtype=torch.int64, device=gp.device)
    work = torch.empty(_lib.MES_WORK_BYTES // 8, dtype=torch.float64, device=gp.device)

    def cons(Cn, base):
        def run():
            st = lib.gpbo_constrained_acq_f64(p(mu), p(sg), M, base, 0.0, 0.01, p(cm), p(cs), M, Cn, upper.ctypes.data_as(C.c_void_p),
                                              0, p(val), p(feas), p(res), p(work), _lib.CONS_WORK_BYTES, gp._stream())
            assert st == 0
        return run

    def mes():
        st = lib.gpbo_mes_acq_f64(p(mu), p(sg), M, ys.ctypes.data_as(C.c_void_p), 16, 0, p(val), p(res), p(work),
                                  _lib.MES_WORK_BYTES, gp._stream())
        assert st == 0

    routes = {f"cons_c{c}": cons(c, _lib.CONS_BASE_EI) for c in (0, 1, 4, 8)}
    routes.update(pof_c8=cons(8, _lib.CONS_BASE_NONE), mes_s16=mes)
    for fn in routes.values():   # warm-up: every code object of the timed window
        fn()
    torch.cuda.synchronize()
    t = {k: [] for k in routes}
    for _ in range(rounds):
        for k, fn in routes.items():
            t[k].append(timed(fn))
    line = {k + "_ms": spread(v) for k, v in t.items()}
    med = {k: statistics.median(v) for k, v in t.items()}
    shapes = {f"cons_c{c}": (1 + c, (2 + 2 * c + 2) * 8 * M) for c in (0, 1, 4, 8)}
    shapes.update(pof_c8=(8, (16 + 2) * 8 * M), mes_s16=(16, 3 * 8 * M))
    for k, (terms, nbytes) in shapes.items():
        line[k + "_terms_per_s"] = terms * M / (med[k] / 1e3)
        line[k + "_GBps"] = nbytes / 1e9 / (med[k] / 1e3)
    line.update(M=M, hbm_GBps=HBM_GBPS, nan_count=int(res.cpu()[2]))
    return line


def _rff(rng, Xs, ls):
    om = rng.standard_normal((256, 2)) / ls[None, :]
    ph, w = rng.uniform(0, 2 * np.pi, 256), rng.standard_normal(256)
    return np.sqrt(2.0 / 256) * (np.cos(Xs @ om.T + ph[None, :]) @ w)


def quality(seeds=20, steps=25, n_cand=1500, n0=5, noise=0.1):
    ls, rho = np.array([0.3, 1.0]), 0.01
    rows = {"cei": [], "ei": []}
    gp, gc = DeviceGP(), DeviceGP()
    for seed in range(seeds):
        rng = np.random.default_rng(100 + seed)
        Xs = rng.uniform(0, 1, (n_cand, 2))
        f, g = _rff(rng, Xs, ls), _rff(rng, Xs, ls)          # noise-free objective and constraint at the candidates
        u = float(np.median(g))
        ok = g <= u
        eps_f, eps_g = (noise * rng.standard_normal((steps + n0, n_cand)) for _ in range(2))
        start = rng.choice(n_cand, n0, replace=False)
        for how in rows:
            visited, fallbacks = list(start), 0
            for _ in range(steps):
                idx = np.asarray(visited)
                yv, gv = f[idx] + eps_f[np.arange(len(idx)), idx], g[idx] + eps_g[np.arange(len(idx)), idx]
                gp.factorise(Xs[idx], yv, ls, rho, 0.0)
                if how == "ei":
                    nxt = gp.score(Xs, acquisition="ei", f_best=float(yv.min()), prior_var=1.0 + rho).best_idx
                else:
                    gc.factorise(Xs[idx], gv, ls, rho, 0.0)
                    r = gp.select_constrained(Xs, [gc], [u])
                    nxt, fallbacks = r.best_idx, fallbacks + (r.base == "none")
                visited.append(int(nxt))
            new = np.asarray(visited[n0:])
            feas_new = new[ok[new]]
            rows[how].append(dict(share=float(ok[new].mean()), fallbacks=fallbacks, distinct=len(set(visited)),
                                  regret=float(f[feas_new].min() - f[ok].min()) if feas_new.size else None))
    out = {}
    for how, v in rows.items():
        reg = [r["regret"] for r in v if r["regret"] is not None]
        out[how] = dict(mean_feasible_share=float(np.mean([r["share"] for r in v])),
                        mean_feasible_regret=float(np.mean(reg)) if reg else None,
                        median_feasible_regret=float(np.median(reg)) if reg else None,
                        runs_without_a_feasible_evaluation=len(v) - len(reg),
                        mean_distinct=float(np.mean([r["distinct"] for r in v])),
                        steps_on_feasibility_alone=int(sum(r["fallbacks"] for r in v)),
                        shares=[round(r["share"], 3) for r in v],
                        regrets=[None if r["regret"] is None else round(r["regret"], 4) for r in v])
    return out | dict(seeds=seeds, steps=steps, candidates=n_cand, start_points=n0, noise_sd=noise, rho=rho, ls=ls.tolist(),
                      limit="median of g over the candidates")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--quality", action="store_true")
    ap.add_argument("--skip-headline", action="store_true")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "constrained_bench_line.json"))
    a = ap.parse_args()
    line = dict(tool="tools/bench_constrained.py", device=torch.cuda.get_device_name(0), rounds=a.rounds)
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
