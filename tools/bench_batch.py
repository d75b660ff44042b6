"""Per-member cost of greedy batch selection (DeviceGP.select_batch, csrc/batch.hip) against the only route the library
offered before it: append(x_j, y_j) + score(dense=True) per member.  Device-event times, warm-up first, the two routes
alternated ROUNDS times in one process on one GPU; medians reported.
  per added member of select_batch = (events around gpbo_select_batch_f64 at q = 8  -  the same at q = 1) / 7
  parent route per member          = events around one append() + one dense score() (the surrogate refactorised, untimed,
                                     and one untimed append before each sample, so that every sample appends to the same
                                     N + 1 observations and never pays for re-padding the factors)
usage: python tools/bench_batch.py [--rounds 5] [--shapes headline,c2] [--out profiles/batch_bench_line.json]"""
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
Q = 8
VALU_PER_PAIR = {8: 36.25}    # vector instructions per (candidate, observation) pair in batch_downdate_kernel<8>'s loop, from the ISA
ISSUE_CEILING = 33e12         # fp64 lane-instructions per second


def timed(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    out = fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b), out


def bench(name, rounds):
    N, M, d = SHAPES[name]
    X, y, Xs, ls = make_problem(N, M, d)
    gp, slow = DeviceGP(), DeviceGP()
    Xd, yd, Xsd = gp._dev(X), gp._dev(y), gp._dev(Xs)
    gp.factorise(Xd, yd, ls)
    base = gp.score(Xsd, dense=True)
    mu0, sig0 = base.mu.clone(), base.sigma.clone()

    def batch(q):
        mu, sig = mu0.clone(), sig0.clone()
        return timed(lambda: gp.select_batch_on_posterior(Xsd, mu, sig, q))

    def parent(i):
        slow.factorise(Xd, yd, ls)
        slow.append(Xsd[i ^ 1], mu0[(i ^ 1): (i ^ 1) + 1], check=False)   # untimed: may re-pad the factors (N == Np)
        torch.cuda.synchronize()
        t_app, _ = timed(lambda: slow.append(Xsd[i], mu0[i: i + 1], check=False))
        t_score, _ = timed(lambda: slow.score_async(Xsd, dense=True))
        return t_app, t_score

    first = int(base.best_idx)
    batch(Q), batch(1), parent(first)   # warm-up: every shape and code object of the timed window
    t8, t1, ta, ts = [], [], [], []
    members = None
    for _ in range(rounds):
        t, r = batch(Q)
        t8.append(t)
        members = r.indices.tolist()
        t1.append(batch(1)[0])
        a, s = parent(first)
        ta.append(a)
        ts.append(s)
    med = statistics.median
    per_member = (med(t8) - med(t1)) / (Q - 1)
    parent_ms = med(ta) + med(ts)
    pairs = float(N) * M
    line = dict(shape=name, N=N, M=M, d=d, q=Q, rounds=rounds, members=members,
                select_batch_q8_ms=med(t8), select_batch_q1_ms=med(t1), select_batch_per_added_member_ms=per_member,
                select_batch_per_added_member_ms_all=[(a - b) / (Q - 1) for a, b in zip(t8, t1)],
                parent_append_ms=med(ta), parent_dense_score_ms=med(ts), parent_per_member_ms=parent_ms,
                parent_per_member_ms_all=[a + s for a, s in zip(ta, ts)], ratio=parent_ms / per_member,
                valu_per_pair=VALU_PER_PAIR.get(d),
                fraction_of_issue_ceiling=(pairs * VALU_PER_PAIR[d] / (per_member * 1e-3) / ISSUE_CEILING) if d in VALU_PER_PAIR else None,
                device=torch.cuda.get_device_name(0))
    print(json.dumps(line), flush=True)
    return line


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--shapes", default="headline,c2")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "batch_bench_line.json"))
    a = ap.parse_args()
    if a.rounds < 5:
        sys.exit("at least five alternations")
    lines = [bench(s, a.rounds) for s in a.shapes.split(",")]
    with open(a.out, "w") as f:
        json.dump(dict(tool="tools/bench_batch.py", results=lines), f, indent=1)
        f.write("\n")
