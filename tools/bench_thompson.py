"""Cost of Thompson sampling by pathwise posterior samples (DeviceGP.thompson_paths / thompson_score, csrc/thompson.hip) at
the headline shape, beside select_batch(q = 16) on the same surrogate in the same process, for scale.  Device-event times
around the two C calls alone (inputs already on the device, no read-back inside the window), warm-up first, the routes
alternated ROUNDS times; medians, with every sample and the spread reported.
  weights_ms  gpbo_thompson_weights_f64: g_s(X), the residual, the two products with U           (once per factorisation)
  paths_ms    gpbo_thompson_paths_f64: prep + the launch over all M candidates + the finish      (per candidate set)
  valu_issue_fraction = M (N v_obs + F v_feat) ceil(S / 16) / paths time / ISSUE_CEILING, with v_obs / v_feat the vector
                instructions per (candidate, observation) / (candidate, feature) in the loops of thompson_paths_kernel<8, 16>,
                counted in its ISA
  select_batch_q16_ms  the dense plain pass + gpbo_select_batch_f64 (q = 16): what 16 parallel points cost before
A library built with another cosine (tools/build_variant.sh ts_cospi thompson -DGPBO_TS_COSPI) is measured by running this
tool once more with GPBO_LIB=ab_libs/ts_cospi.so --label cospi --no-batch --append: its lines join those of the file.
The two instruction counts are read off the ISA by hand and hold for d = 8 and the 16-path instance only; they go stale when
the kernel changes, so the file records them with that caveat and a changed kernel needs them counted again.
usage: python tools/bench_thompson.py [--rounds 5] [--paths 16,64] [--label shipped] [--out profiles/thompson_bench_line.json]
                                      [--no-batch] [--append]"""
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
from bayesian_optimisation_amd.synthetic import make_problem  # noqa: E402
from bayesian_optimisation_amd.thompson import thompson_draws  # noqa: E402

N, M, D, F = 4096, 1 << 21, 8, 2048
# vector instructions per two candidates in the loops of thompson_paths_kernel<8, 16> (ISA of this tree: 103 per observation,
# 79 per feature - 16 of each pair's share are the multiply-adds into the 16 path accumulators)
VALU_PER_OBS, VALU_PER_FEATURE = 103 / 2, 79 / 2
ISSUE_CEILING = 33e12              # fp64 lane-instructions per second


def timed(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    out = fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b), out


def spread(v):
    return dict(median=statistics.median(v), min=min(v), max=max(v), all=v)


def bench(S, rounds, gp, Xsd, with_batch, label):
    lib, p = gp.lib, gp._ptr
    omega, phase, W, E = (gp._dev(a) for a in thompson_draws(D, F, S, N, 0))
    V = torch.empty((S, gp.Np), dtype=torch.float64, device=gp.device)
    ww = int(lib.gpbo_thompson_weights_workspace_bytes(gp.Np, F, S))
    wp = int(lib.gpbo_thompson_paths_workspace_bytes(gp.Np, M, F, S))
    work = torch.empty(max(ww, wp) // 8, dtype=torch.float64, device=gp.device)
    out = torch.zeros(3 * S, dtype=torch.int64, device=gp.device)
    lsp = gp.ls_h.ctypes.data_as(C.c_void_p)

    def weights():
        _lib.check(lib.gpbo_thompson_weights_f64(p(gp.X), p(gp.y), N, gp.Np, D, lsp, p(gp.U), gp.jitter1, gp.jitter2, p(omega),
                                                 p(phase), p(W), p(E), F, S, p(V), p(work), ww, gp._stream()), "weights")

    def paths():
        _lib.check(lib.gpbo_thompson_paths_f64(p(Xsd), M, p(gp.X), N, gp.Np, D, lsp, p(omega), p(phase), p(W), p(V), F, S, 0, None,
                                               0, p(out[:S]), p(out[S: 2 * S]), p(out[2 * S:]), p(work), wp, gp._stream()), "paths")

    def batch():
        return gp.select_batch(Xsd, 16)

    weights(), paths()                       # warm-up: every shape and code object of the timed window
    if with_batch:
        batch()
    torch.cuda.synchronize()
    tw, tp, tb = [], [], []
    for _ in range(rounds):
        tw.append(timed(weights)[0])
        tp.append(timed(paths)[0])
        if with_batch:
            tb.append(timed(batch)[0])
    h = out.cpu()
    idx = h[:S].numpy()
    passes = -(-S // 16)
    lane_instr = float(M) * (N * VALU_PER_OBS + F * VALU_PER_FEATURE) * passes
    med = statistics.median(tp)
    line = dict(label=label, N=N, M=M, d=D, F=F, S=S, rounds=rounds, weights_ms=spread(tw), paths_ms=spread(tp),
                distinct_winners=int(len(set(idx.tolist()))), nan_total=int(h[2 * S:].sum()),
                generated_entries=float(M) * (N + F) * passes, paths_ms_per_point=med / S,
                device=torch.cuda.get_device_name(0))
    if label == "shipped":   # (the instruction counts are those of the shipped kernel)
        line.update(valu_per_observation=VALU_PER_OBS, valu_per_feature=VALU_PER_FEATURE,
                    valu_counts="hand-counted in the ISA of thompson_paths_kernel<8, 16>; recount when the kernel changes",
                    valu_issue_fraction=lane_instr / (med * 1e-3) / ISSUE_CEILING)
    if with_batch:
        line["select_batch_q16_ms"] = spread(tb)
    print(json.dumps(line), flush=True)
    return line


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--paths", default="16,64")
    ap.add_argument("--label", default="shipped")
    ap.add_argument("--no-batch", action="store_true")
    ap.add_argument("--append", action="store_true", help="keep the lines already in --out")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "thompson_bench_line.json"))
    a = ap.parse_args()
    if a.rounds < 5:
        sys.exit("at least five alternations")
    X, y, Xs, ls = make_problem(N, M, D)
    gp = DeviceGP()
    gp.factorise(gp._dev(X), gp._dev(y), ls)
    Xsd = gp._dev(Xs)
    lines = [bench(int(s), a.rounds, gp, Xsd, not a.no_batch and i == 0, a.label) for i, s in enumerate(a.paths.split(","))]
    for line in lines:
        line["library"] = os.path.basename(_lib.LIB_PATH)
    if a.append and os.path.exists(a.out):
        with open(a.out) as f:
            lines = json.load(f)["results"] + lines
    with open(a.out, "w") as f:
        json.dump(dict(tool="tools/bench_thompson.py", results=lines), f, indent=1)
        f.write("\n")
