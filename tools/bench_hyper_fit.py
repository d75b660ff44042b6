"""ML-II over all hyperparameters on the GPU (ard="hyper"): one JSON line.

  eval[N]   d = 8 at N = 512 / 4096 on synthetic.make_problem: milliseconds per DeviceGP.nlml_hyper evaluation (host wall,
            read-back included) beside DeviceGP.nlml_and_grad - the length-scale-only evaluation of ard="gradient", which this
            mode leaves as it was - on the same box; by device events after warm-up: the factorisation, the whole
            gpbo_nlml_hyper_f64 call, the gpbo_nlml_grad_f64 call it contains, and their difference added_ms = the launches
            this mode adds (row sums over half of U, one [Np] product pair for K^-1 1, profile, finish)
  fit[N]    the whole fit (DeviceGP.fit_hyperparameters, box [0.05, 5]^8 x [1e-6, 1], start 0.5 / 1e-2): evaluations,
            milliseconds, final value, fitted noise / mean / scale
usage: python tools/bench_hyper_fit.py [--sizes 512,4096] [--reps R] [--out profiles/hyper_fit_bench_line.json]"""
import argparse
import ctypes as C
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402
import torch  # noqa: E402

from bayesian_optimisation_amd import DeviceGP  # noqa: E402
from bayesian_optimisation_amd.synthetic import make_problem  # noqa: E402

D = 8
NOISE = 1e-2


def event_ms(fn, reps):
    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    s.record()
    for _ in range(reps):
        fn()
    e.record()
    e.synchronize()
    return s.elapsed_time(e) / reps


def wall_ms(fn, reps):
    torch.cuda.synchronize()
    t = time.perf_counter()
    for _ in range(reps):
        fn()
    return (time.perf_counter() - t) * 1e3 / reps


def eval_times(gp, N, reps):
    X, y, _, ls = make_problem(N, 8, D)
    Xd, yd = gp._dev(X), gp._dev(y)
    gp.nlml_and_grad(Xd, yd, ls, NOISE)     # warm-up: buffers, the factorisation's plan for this size
    gp.nlml_hyper(Xd, yd, ls, NOISE)
    fb, lib, st = gp._fit_bufs, gp.lib, gp._stream()
    Np = fb["Np"]
    lsp = np.ascontiguousarray(ls).ctypes.data_as(C.c_void_p)

    def fact():
        rc = lib.gpbo_factorise_f64(gp._ptr(Xd), gp._ptr(yd), N, D, lsp, NOISE, 0.0, Np, gp._ptr(fb["K"]), gp._ptr(fb["U"]),
                                    gp._ptr(fb["alpha"]), gp._ptr(fb["info"]), gp._ptr(fb["work_fact"]), fb["wf"], st)
        assert rc == 0, rc

    def grad():
        rc = lib.gpbo_nlml_grad_f64(gp._ptr(fb["U"]), gp._ptr(fb["alpha"]), gp._ptr(yd), gp._ptr(Xd), N, Np, D, lsp,
                                    gp._ptr(fb["info"]), gp._ptr(fb["out"]), gp._ptr(fb["work_grad"]), fb["wg"], st)
        assert rc == 0, rc

    def hyper():
        rc = lib.gpbo_nlml_hyper_f64(gp._ptr(fb["U"]), gp._ptr(fb["alpha"]), gp._ptr(yd), gp._ptr(Xd), N, Np, D, lsp, NOISE, 3,
                                     gp._ptr(fb["info"]), gp._ptr(fb["out_hyper"]), None, gp._ptr(fb["work_hyper"]), fb["wh"], st)
        assert rc == 0, rc

    fact(); grad(); hyper()
    torch.cuda.synchronize()
    f_ms, g_ms, h_ms = event_ms(fact, reps), event_ms(grad, reps), event_ms(hyper, reps)
    return dict(N=N, d=D, nlml_hyper_eval_ms=round(wall_ms(lambda: gp.nlml_hyper(Xd, yd, ls, NOISE), reps), 4),
                nlml_and_grad_eval_ms=round(wall_ms(lambda: gp.nlml_and_grad(Xd, yd, ls, NOISE), reps), 4),
                factorise_ms=round(f_ms, 4), hyper_call_ms=round(h_ms, 4), grad_call_ms=round(g_ms, 4),
                added_ms=round(h_ms - g_ms, 4), added_over_factorise=round((h_ms - g_ms) / f_ms, 4))


def fit(gp, N):
    X, y, _, _ = make_problem(N, 8, D)
    box = dict(ls0=[0.5] * D, ls_lower=[0.05] * D, ls_upper=[5.0] * D, noise0=1e-2, noise_lower=1e-6, noise_upper=1.0)
    gp.nlml_hyper(X, y, np.full(D, 0.5), 1e-2)   # warm-up at this size
    torch.cuda.synchronize()
    t = time.perf_counter()
    r = gp.fit_hyperparameters(X, y, **box)
    ms = (time.perf_counter() - t) * 1e3
    return dict(N=N, d=D, evals=r.n_eval, iters=r.n_iter, ms=round(ms, 2), nlml=r.nlml, reason=r.reason, pg_norm=r.pg_norm,
                noise=r.noise, mean=r.mean, scale=r.scale, ls=np.asarray(r.ls).tolist())


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="512,4096")
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    gp = DeviceGP(device="cuda:0")
    sizes = [int(n) for n in a.sizes.split(",") if n]
    out = dict(metric="hyper_fit", device=torch.cuda.get_device_name(0), eval=[eval_times(gp, n, a.reps) for n in sizes],
               fit=[fit(gp, n) for n in sizes])
    line = json.dumps(out)
    print(line, flush=True)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
