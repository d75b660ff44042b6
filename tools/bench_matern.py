"""The Matern 3/2 and 5/2 covariance families on the GPU beside the squared exponential: one JSON line.

  step[family]   d = 8, N = 4096, 2^21 candidates in chunks of 2^17 (the headline shape of bench.py) through DeviceGP.score():
                 milliseconds per step (host wall, result read back), and from the profile events of the same steps the
                 K(X*,X) launch - the only launch that differs between the families - and the variance launch, which does not
  eval[family]   one DeviceGP.nlml_and_grad and one DeviceGP.nlml_hyper evaluation (host wall, read-back included) at N = 512
                 and 4096, d = 8
  fit            data drawn from the Matern-5/2 prior (tests/matern_ref.gp_problem, N = 200, d = 3, noise 0.05, five seeds):
                 the ard="hyper" fit (DeviceGP.fit_hyperparameters, box [0.05, 5]^3 x [1e-6, 1], start 0.5 / 1e-2) with
                 kernel="matern52" against kernel="se": final NLML and the recovered noise standard deviation
Every figure: five repetitions after a warm-up, reported as [min, median, max].
usage: python tools/bench_matern.py [--out profiles/matern_bench_line.json] [--label shipped] [--kstar-only] [--append]
       GPBO_LIB=ab_libs/matern_sqrt_lib.so python tools/bench_matern.py --label sqrt_lib --kstar-only --append
       (tools/build_variant.sh matern_sqrt_lib kernel_build -DGPBO_MATERN_SQRT_LIB: the library's sqrt in the Matern arms)"""
import argparse
import json
import os
import sys
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, "tests"))
import numpy as np  # noqa: E402
import torch  # noqa: E402

from bayesian_optimisation_amd import DeviceGP  # noqa: E402
from bayesian_optimisation_amd.synthetic import make_problem  # noqa: E402

D = 8
FAMILIES = ("se", "matern32", "matern52")
REPS = 5


def spread(v):
    v = sorted(float(x) for x in v)
    return [round(v[0], 4), round(v[len(v) // 2], 4), round(v[-1], 4)]


def wall_ms(fn):
    torch.cuda.synchronize()
    t = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t) * 1e3


def steps(N, M, chunk, kstar_only):
    X, y, Xs, ls = make_problem(N, M, D)
    out = {}
    gp = DeviceGP(device="cuda:0", chunk=chunk)
    gp.enable_profile(4096)
    Xsd = gp._dev(Xs)
    for fam in FAMILIES:
        gp.factorise(X, y, ls, kernel=fam)
        gp.score(Xsd)   # warm-up
        step, kstar, var = [], [], []
        for _ in range(REPS):
            gp.reset_profile()
            step.append(wall_ms(lambda: gp.score(Xsd)))
            k_ms, k_n, _ = gp.read_profile_kstar()
            v_ms, v_n, _ = gp.read_profile()
            kstar.append(k_ms / max(k_n, 1))
            var.append(v_ms / max(v_n, 1))
        out[fam] = dict(kstar_launch_ms=spread(kstar))
        if not kstar_only:
            out[fam].update(step_ms=spread(step), variance_launch_ms=spread(var))
    return dict(N=N, d=D, candidates=M, chunk=chunk, **out)


def evals(N):
    X, y, _, ls = make_problem(N, 8, D)
    gp = DeviceGP(device="cuda:0")
    Xd, yd = gp._dev(X), gp._dev(y)
    out = {}
    for fam in FAMILIES:
        gp.nlml_and_grad(Xd, yd, ls, 1e-2, kernel=fam)   # warm-up
        gp.nlml_hyper(Xd, yd, ls, 1e-2, kernel=fam)
        out[fam] = dict(nlml_and_grad_ms=spread(wall_ms(lambda: gp.nlml_and_grad(Xd, yd, ls, 1e-2, kernel=fam)) for _ in range(REPS)),
                        nlml_hyper_ms=spread(wall_ms(lambda: gp.nlml_hyper(Xd, yd, ls, 1e-2, kernel=fam)) for _ in range(REPS)))
    return dict(N=N, d=D, **out)


def fits():
    import matern_ref as MR

    gp = DeviceGP(device="cuda:0")
    rows = []
    for seed in range(1, 6):
        X, y = MR.gp_problem(seed, 200, 3, "matern52", noise=0.05)
        row = dict(seed=seed)
        for fam in ("matern52", "se"):
            r = gp.fit_hyperparameters(X, y, [0.5] * 3, [0.05] * 3, [5.0] * 3, 1e-2, 1e-6, 1.0, kernel=fam)
            row[fam] = dict(nlml=round(float(r.nlml), 6), noise_sd=round(float(np.sqrt(r.noise) * r.scale), 5),
                            ls=[round(float(v), 4) for v in r.ls], evaluations=int(r.n_eval), converged=bool(r.converged))
        row["nlml_se_minus_matern52"] = round(row["se"]["nlml"] - row["matern52"]["nlml"], 6)
        rows.append(row)
    return dict(data="matern_ref.gp_problem(seed, 200, 3, 'matern52', noise=0.05)", true_noise_sd=0.05, seeds=rows,
                nlml_se_minus_matern52=spread(r["nlml_se_minus_matern52"] for r in rows),
                noise_sd_matern52=spread(r["matern52"]["noise_sd"] for r in rows),
                noise_sd_se=spread(r["se"]["noise_sd"] for r in rows))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "matern_bench_line.json"))
    ap.add_argument("--label", default="shipped")
    ap.add_argument("--kstar-only", action="store_true")
    ap.add_argument("--append", action="store_true")
    a = ap.parse_args()
    line = dict(device=torch.cuda.get_device_name(0), library=os.environ.get("GPBO_LIB", "libgpbo.so"), spread="[min, median, max] of 5",
                step=steps(4096, 1 << 21, 1 << 17, a.kstar_only))
    if not a.kstar_only:
        line["eval"] = [evals(512), evals(4096)]
        line["fit"] = fits()
    doc = {}
    if a.append and os.path.exists(a.out):
        doc = json.load(open(a.out))
    doc[a.label] = line
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(doc, f, indent=1)
        f.write("\n")
    print(json.dumps({a.label: line}))


if __name__ == "__main__":
    main()
