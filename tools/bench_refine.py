"""Cost of off-grid refinement (DeviceGP.refine, csrc/refine.hip) beside the dense score() of the same shape: 64 and 1024
starts x 30 iterations (31 evaluations of four launches each).  Device-event times, warm-up first, refine and score
alternated ROUNDS times in one process on one GPU; medians reported, every sample kept.
  --trace-one: one refine call of --starts starts and nothing else timed (the program of a kernel-trace run)
usage: python tools/bench_refine.py [--rounds 7] [--shapes headline,c2] [--out profiles/refine_bench_line.json]"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402
import torch  # noqa: E402

from bayesian_optimisation_amd import DeviceGP  # noqa: E402
from bayesian_optimisation_amd.synthetic import make_problem  # noqa: E402

SHAPES = {"headline": (4096, 1 << 21, 8), "c2": (512, 1 << 20, 8)}   # (N, M, d); c2 = BASELINE configs[1]
STARTS = (64, 1024)
ITERS = 30


def timed(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    out = fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b), out


def setup(name):
    N, M, d = SHAPES[name]
    X, y, Xs, ls = make_problem(N, M, d)
    gp = DeviceGP()
    Xsd = gp._dev(Xs)
    gp.factorise(gp._dev(X), gp._dev(y), ls)
    base = gp.score(Xsd, dense=True)
    order = torch.sort(base.acq, descending=True, stable=True).indices
    return gp, Xsd, order, base, (N, M, d)


def bench(name, rounds):
    gp, Xsd, order, base, (N, M, d) = setup(name)
    starts = {p: Xsd[order[:p]].contiguous() for p in STARTS}
    for p in STARTS:   # warm-up: every shape and code object of the timed window
        gp.refine(starts[p], 0.0, 1.0, iters=ITERS)
    gp.score(Xsd, dense=True)
    t_ref, t_score, last = {p: [] for p in STARTS}, [], {}
    for _ in range(rounds):
        for p in STARTS:
            t, r = timed(lambda: gp.refine(starts[p], 0.0, 1.0, iters=ITERS))
            t_ref[p].append(t)
            last[p] = r
        t_score.append(timed(lambda: gp.score(Xsd, dense=True))[0])
    med = statistics.median
    Np = gp.Np
    line = dict(shape=name, N=N, M=M, d=d, iters=ITERS, rounds=rounds, dense_score_ms=med(t_score), dense_score_ms_all=t_score,
                grid_best=base.best_val, device=torch.cuda.get_device_name(0))
    for p in STARTS:
        ms, r = med(t_ref[p]), last[p]
        evals = ITERS + 1
        Pp = (p + 63) // 64 * 64
        line[f"refine_{p}"] = dict(
            ms=ms, ms_all=t_ref[p], ms_per_evaluation=ms / evals, fraction_of_dense_score=ms / med(t_score),
            gemm_tflops=4.0 * Pp * Np * Np * evals / (ms * 1e-3) / 1e12,       # both dense products, as if they were all of the call
            u_read_gbs=2.0 * 8 * Np * Np * evals / (ms * 1e-3) / 1e9,           # two reads of U per evaluation
            refined_best=r.best_val, accepted_min=int(r.accepted.min()), accepted_max=int(r.accepted.max()),
            pg_max=float(r.pg.max()), every_start_improved=bool((r.acq >= r.acq0).all()))
    print(json.dumps(line), flush=True)
    return line


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--shapes", default="headline,c2")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "refine_bench_line.json"))
    ap.add_argument("--trace-one", action="store_true")
    ap.add_argument("--starts", type=int, default=64)
    a = ap.parse_args()
    if a.trace_one:
        gp, Xsd, order, _, _ = setup(a.shapes.split(",")[0])
        s = Xsd[order[: a.starts]].contiguous()
        gp.refine(s, 0.0, 1.0, iters=ITERS)
        torch.cuda.synchronize()
        sys.exit(0)
    if a.rounds < 5:
        sys.exit("at least five alternations")
    lines = [bench(s, a.rounds) for s in a.shapes.split(",")]
    with open(a.out, "w") as f:
        json.dump(dict(tool="tools/bench_refine.py", results=lines), f, indent=1)
        f.write("\n")
