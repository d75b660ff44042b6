"""ML-II length-scale fitting on the GPU (ard="gradient"): one JSON line.

  kernel[N]   the likelihood-gradient call (gpbo_nlml_grad_f64: point scaling + nlml_grad_kernel + finish) and the
              factorisation (gpbo_factorise_f64) at N = 512 / 2048 / 4096 / 8192, d = 8, by device events after warm-up;
              roofline of the gradient call against the 78.6 TFLOP/s fp64 matrix peak, flop counted from the tiles
              actually launched (2 * 64 * 64 * (N rounded up to 16 - 64 I) per 64 x 64 tile (I, J), I >= J) and, for
              comparison, from the triangular count N^3 / 3; eval_ms = one DeviceGP.nlml_and_grad (host wall, read-back
              included)
  fit[N]      d = 8 at N = 512 / 2048 / 4096 on synthetic.make_problem, axes geomspace(0.05, 5, 16) per feature: the
              gradient fit (PointSelector(ard="gradient").tune_kernel: evaluations, ms, final NLML) beside the log-det
              coordinate search with 2 sweeps (PointSelector(likelihood="logdet").tune_kernel: ms, NLML at its choice)
usage: python tools/bench_ard_fit.py [--kernel-only] [--sizes 512,2048,...] [--reps R]"""
import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402
import torch  # noqa: E402

from bayesian_optimisation_amd import DeviceGP  # noqa: E402
from bayesian_optimisation_amd.point_selector import PointSelector  # noqa: E402
from bayesian_optimisation_amd.synthetic import make_problem  # noqa: E402

PEAK_TFLOPS = 78.6
D = 8


def tile_flop(N):
    nb = -(-N // 64)
    kend = -(-N // 16) * 16
    return sum((I + 1) * 2.0 * 64 * 64 * (kend - 64 * I) for I in range(nb)), nb * (nb + 1) // 2


def event_ms(fn, reps):
    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    s.record()
    for _ in range(reps):
        fn()
    e.record()
    e.synchronize()
    return s.elapsed_time(e) / reps


def kernel_times(gp, N, reps):
    X, y, _, ls = make_problem(N, 8, D)
    Xd, yd = gp._dev(X), gp._dev(y)
    gp.nlml_and_grad(Xd, yd, ls)        # warm-up: buffers, the factorisation's plan for this size
    fb, lib, st = gp._fit_bufs, gp.lib, gp._stream()
    Np = fb["Np"]
    lsp = np.ascontiguousarray(ls).ctypes.data_as(__import__("ctypes").c_void_p)

    def fact():
        rc = lib.gpbo_factorise_f64(gp._ptr(Xd), gp._ptr(yd), N, D, lsp, 1e-4, 0.0, Np, gp._ptr(fb["K"]), gp._ptr(fb["U"]),
                                    gp._ptr(fb["alpha"]), gp._ptr(fb["info"]), gp._ptr(fb["work_fact"]), fb["wf"], st)
        assert rc == 0, rc

    def grad():
        rc = lib.gpbo_nlml_grad_f64(gp._ptr(fb["U"]), gp._ptr(fb["alpha"]), gp._ptr(yd), gp._ptr(Xd), N, Np, D, lsp,
                                    gp._ptr(fb["info"]), gp._ptr(fb["out"]), gp._ptr(fb["work_grad"]), fb["wg"], st)
        assert rc == 0, rc

    fact(); grad()
    torch.cuda.synchronize()
    f_ms, g_ms = event_ms(fact, reps), event_ms(grad, reps)
    t = time.perf_counter()
    for _ in range(reps):
        gp.nlml_and_grad(Xd, yd, ls)
    eval_ms = (time.perf_counter() - t) * 1e3 / reps
    flop, tiles = tile_flop(N)
    tri = N ** 3 / 3.0
    return dict(N=N, d=D, tiles=tiles, factorise_ms=round(f_ms, 4), grad_ms=round(g_ms, 4), eval_ms=round(eval_ms, 4),
                grad_tile_tflops=round(flop / g_ms / 1e9, 3), grad_frac_of_peak_tiles=round(flop / g_ms / 1e9 / PEAK_TFLOPS, 4),
                grad_frac_of_peak_triangular=round(tri / g_ms / 1e9 / PEAK_TFLOPS, 4))


def selector(gp, X, y, axes, **kw):
    ps = PointSelector(**kw)
    ps._gp = gp
    ps.measured_pts, ps.measured_vals, ps.length_scales = X, y, axes
    return ps


def fit_vs_search(gp, N):
    X, y, _, _ = make_problem(N, 8, D)
    axes = [np.geomspace(0.05, 5.0, 16)] * D
    # warm-up of both routes at this size (first-call costs: plan upload, workspaces)
    gp.nlml_and_grad(X, y, np.full(D, 0.5))
    gp.nlml_grid(X, y, np.full((16, D), 0.5), likelihood="logdet")
    ps = selector(gp, X, y, axes, ard="gradient")
    torch.cuda.synchronize()
    t = time.perf_counter()
    ps.tune_kernel()
    fit_ms = (time.perf_counter() - t) * 1e3
    cs = selector(gp, X, y, axes, likelihood="logdet")
    torch.cuda.synchronize()
    t = time.perf_counter()
    cs.tune_kernel()
    cs_ms = (time.perf_counter() - t) * 1e3
    cs_nlml, _ = gp.nlml_and_grad(X, y, np.asarray(cs.kernel_params))
    lf = ps.last_fit
    return dict(N=N, d=D, fit=dict(evals=lf["n_eval"], iters=lf["n_iter"], ms=round(fit_ms, 2), nlml=lf["nlml"],
                                   reason=lf["reason"], pg_norm=lf["pg_norm"]),
                coordinate_search=dict(sweeps=2, launches=2 * D, cells=2 * D * 16, ms=round(cs_ms, 2), nlml=cs_nlml))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--kernel-only", action="store_true")
    ap.add_argument("--sizes", default="512,2048,4096,8192")
    ap.add_argument("--fit-sizes", default="512,2048,4096")
    ap.add_argument("--reps", type=int, default=10)
    a = ap.parse_args()
    gp = DeviceGP(device="cuda:0")
    out = dict(metric="ard_fit", device=torch.cuda.get_device_name(0), peak_fp64_matrix_tflops=PEAK_TFLOPS,
               kernel=[kernel_times(gp, int(n), a.reps) for n in a.sizes.split(",") if n])
    if not a.kernel_only:
        out["fit"] = [fit_vs_search(gp, int(n)) for n in a.fit_sizes.split(",") if n]
    print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
