"""The acquisition integrated over the hyperparameter posterior (ard="marginal"): one JSON line.

  cells[]    gpbo_nlml_hyper_cells_f64 (csrc/hyper_wave.hip) at G = 16 and 2,500 cells, N = 16 / 32 / 48 / 64, d = 2 and 8:
             milliseconds per launch by device events; beside it gpbo_nlml_grid_wave_logdet_f64 (csrc/ard_wave.hip, the kernel it
             extends by one right-hand side) on the same box and shape; the host wall time of DeviceGP.nlml_hyper_cells through
             the kernel (upload, launch, read-back) and through the per-cell loop, per call of G = 16 cells
  update     update_surrogate() at the reference's shape (N = 32, d = 2, 50 x 50 candidates) with ard="marginal" and, in
             alternation, ard="hyper": median host milliseconds; the marginal update split into the ML-II fit, the sampling
             (with its batch count), the S factorisations and the ensemble pass
  scale      the ensemble pass at d = 8, N = 4096, M = 2^21, S = 8 beside eight single score() calls on the same box
  quality    CPU only (tests/hyper_ref.py, tests/ensemble_ref.py): gp_problem(seed, 2020, 2, noise=0.05), the first 20 points
             observed and 2,000 held out, five seeds: mean log predictive density of the held-out values under the integrated
             posterior (the mixture of 16 sampled models) and under the ML-II model alone
usage: python tools/bench_marginal.py [--parts cells,update,scale,quality] [--reps R] [--out profiles/marginal_bench_line.json]"""
import argparse
import ctypes as C
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np  # noqa: E402


def event_ms(torch, fn, reps):
    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    fn()
    torch.cuda.synchronize()
    s.record()
    for _ in range(reps):
        fn()
    e.record()
    e.synchronize()
    return s.elapsed_time(e) / reps


def wall_ms(torch, fn, reps):
    fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(reps):
        t = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        ts.append((time.perf_counter() - t) * 1e3)
    return float(np.median(ts))


def part_cells(reps):
    import torch
    from bayesian_optimisation_amd import DeviceGP
    from bayesian_optimisation_amd.synthetic import make_problem

    gp = DeviceGP(device="cuda:0")
    lib, st = gp.lib, gp._stream()
    rows = []
    for d in (2, 8):
        for N in (16, 32, 48, 64):
            X, y, _, ls = make_problem(N, 8, d)
            Xd, yd = gp._dev(X), gp._dev(y - y.mean())
            for G in (16, 2500):
                rng = np.random.default_rng(G)
                cells = np.concatenate([ls[None, :] * np.exp(rng.uniform(-0.5, 0.5, (G, d))), np.full((G, 1), 1e-2)], axis=1)
                cd, lsd = gp._dev(cells), gp._dev(np.ascontiguousarray(cells[:, :d]))
                out3 = torch.empty((G, 3), dtype=torch.float64, device=gp.device)
                out1 = torch.empty(G, dtype=torch.float64, device=gp.device)

                def hyper():
                    rc = lib.gpbo_nlml_hyper_cells_f64(gp._ptr(Xd), gp._ptr(yd), N, d, gp._ptr(cd), G, 0, 3, gp._ptr(out3), st)
                    assert rc == 0, rc

                def grid():
                    rc = lib.gpbo_nlml_grid_wave_logdet_f64(gp._ptr(Xd), gp._ptr(yd), N, d, gp._ptr(lsd), G, 1e-2, gp._ptr(out1), st)
                    assert rc == 0, rc

                row = dict(N=N, d=d, G=G, hyper_cells_ms=round(event_ms(torch, hyper, reps), 5),
                           grid_wave_logdet_ms=round(event_ms(torch, grid, reps), 5))
                row["ratio"] = round(row["hyper_cells_ms"] / row["grid_wave_logdet_ms"], 3)
                if G == 16:
                    row["wave_call_wall_ms"] = round(wall_ms(torch, lambda: gp.nlml_hyper_cells(Xd, y, cells, route="wave"), reps), 4)
                    row["loop_call_wall_ms"] = round(wall_ms(torch, lambda: gp.nlml_hyper_cells(Xd, y, cells, route="loop"), 3), 4)
                rows.append(row)
    return rows


def part_update(reps):
    import torch
    from ard_fit_ref import gp_problem
    from bayesian_optimisation_amd import DeviceEnsemble, DeviceGP, PointSelector, hyper_posterior
    from bayesian_optimisation_amd.model import SurrogateModel

    N, d, S = 32, 2, 16
    X, y = gp_problem(0, N, d, noise=0.05)
    g = (np.arange(50) + 0.5) / 50
    Xs = np.stack(np.meshgrid(g, g, indexing="ij"), -1).reshape(-1, 2)
    axes = [np.geomspace(0.05, 5.0, 50)] * 2

    def selector(mode):
        ps = PointSelector(ard=mode)
        ps.feature_domain, ps.predicted_pts, ps.length_scales = [50, 50], Xs, axes
        return ps

    sel = {m: selector(m) for m in ("marginal", "hyper")}
    times = {m: [] for m in sel}
    for r in range(reps + 1):
        for m, ps in sel.items():   # in alternation
            ps.measured_pts, ps.measured_vals = X, y
            torch.cuda.synchronize()
            t = time.perf_counter()
            ps.update_surrogate()
            ps.lower_confidence_bound()
            torch.cuda.synchronize()
            if r:
                times[m].append((time.perf_counter() - t) * 1e3)
    hs = sel["marginal"].hyper_samples
    # the pieces of the marginal update, timed on their own
    gp = DeviceGP(device="cuda:0")
    box = dict(ls0=[0.5] * d, ls_lower=[0.05] * d, ls_upper=[5.0] * d, noise0=1e-2, noise_lower=1e-6, noise_upper=1.0)
    fit = gp.fit_hyperparameters(X, y, **box)
    fit_ms = wall_ms(torch, lambda: gp.fit_hyperparameters(X, y, **box), reps)
    fn = gp.nlml_hyper_cells_fn(X, y)
    z0 = np.tile(np.log(np.concatenate([fit.ls, [fit.noise]])), (S, 1))
    zlo, zhi = np.log([0.05] * d + [1e-6]), np.log([5.0] * d + [1.0])
    run = lambda: hyper_posterior.sample(lambda Z: fn(np.exp(Z))[:, 0], z0, zlo, zhi, 10, 0)   # noqa: E731
    res = run()
    sample_ms = wall_ms(torch, run, reps)
    prof = fn(np.exp(res.states))
    cells = np.exp(res.states)
    models = [(cells[s, :d], SurrogateModel("se", float(cells[s, d]), 0.0, float(prof[s, 1]), float(np.sqrt(prof[s, 2])), True), 1.0 / S)
              for s in range(S)]
    ens = DeviceEnsemble(device="cuda:0")
    fact_ms = wall_ms(torch, lambda: ens.factorise(X, y, models), reps)
    Xsd = ens._dev(Xs)
    score_ms = wall_ms(torch, lambda: ens.score(Xsd, dense=True), reps)
    return dict(N=N, d=d, M=len(Xs), n_models=S, sweeps=10, marginal_update_ms=round(float(np.median(times["marginal"])), 3),
                hyper_update_ms=round(float(np.median(times["hyper"])), 3), batches=int(hs["n_batches"]),
                min_margin=float(hs["min_margin"]), fit_ms=round(fit_ms, 3), fit_evals=int(fit.n_eval),
                sampling_ms=round(sample_ms, 3), sampling_batches=int(res.n_batches),
                ms_per_batch=round(sample_ms / res.n_batches, 4), factorise_ms=round(fact_ms, 3), ensemble_pass_ms=round(score_ms, 3))


def part_scale(reps):
    import torch
    from bayesian_optimisation_amd import DeviceEnsemble, DeviceGP
    from bayesian_optimisation_amd.model import SurrogateModel
    from bayesian_optimisation_amd.synthetic import make_problem

    N, M, d, S = 4096, 1 << 21, 8, 8
    X, y, Xs, ls = make_problem(N, M, d)
    f = np.geomspace(0.8, 1.25, S)
    models = [(ls * f[s], SurrogateModel("se", 1e-2 * f[s], 0.0, float(y.mean()), float(y.std()) * f[s], True), 1.0 / S) for s in range(S)]
    ens = DeviceEnsemble(device="cuda:0").factorise(X, y, models)
    Xsd = ens._dev(Xs)
    ens_ms = wall_ms(torch, lambda: ens.score(Xsd, dense=True), reps)
    gp = DeviceGP(device="cuda:0").factorise(X, models[0][1].to_model(y), ls, 1e-2, 0.0)
    one_ms = wall_ms(torch, lambda: gp.score(Xsd, dense=True, prior_var=1.01), reps)
    return dict(N=N, M=M, d=d, S=S, ensemble_pass_ms=round(ens_ms, 2), single_score_ms=round(one_ms, 2),
                eight_single_scores_ms=round(8 * one_ms, 2), fold_and_overhead_ms_per_model=round((ens_ms - S * one_ms) / S, 3),
                fold_bytes_per_candidate_and_model=64)


def part_quality():
    import ensemble_ref as E
    import hyper_ref as H
    from ard_fit_ref import gp_problem
    from bayesian_optimisation_amd import hyper_posterior
    from bayesian_optimisation_amd.ard_fit import fit_hyperparameters

    box = dict(ls0=[0.5] * 2, ls_lower=[0.05] * 2, ls_upper=[5.0] * 2, noise0=1e-2, noise_lower=1e-6, noise_upper=1.0)
    zlo, zhi = np.log([0.05, 0.05, 1e-6]), np.log([5.0, 5.0, 1.0])
    rows = []
    for seed in range(5):
        Xa, ya = gp_problem(seed, 2020, 2, noise=0.05)
        X, y, Xt, yt = Xa[:20], ya[:20], Xa[20:], ya[20:]
        fit = fit_hyperparameters(H.objective(X, y), **box)
        f = lambda Z: np.array([H.nlml_hyper(X, y, np.exp(z[:2]), float(np.exp(z[2])))[0] for z in Z])   # noqa: E731
        r = hyper_posterior.sample(f, np.tile(np.log(np.concatenate([fit.ls, [fit.noise]])), (16, 1)), zlo, zhi, 10, 0)
        models = []
        for z in r.states:
            _, _, m, s2 = H.nlml_hyper(X, y, np.exp(z[:2]), float(np.exp(z[2])))
            models.append((np.exp(z[:2]), float(np.exp(z[2])), 0.0, m, float(np.sqrt(s2)), 1.0 / 16))
        ml2 = [(fit.ls, fit.noise, 0.0, fit.mean, fit.scale, 1.0)]

        def lpd(mods):
            dens = 0.0
            for (mu, sd), mod in zip(E.model_posteriors(X, y, Xt, mods), mods):
                dens = dens + mod[5] * np.exp(-0.5 * ((yt - mu) / sd) ** 2) / (sd * np.sqrt(2.0 * np.pi))
            return float(np.mean(np.log(dens)))

        rows.append(dict(seed=seed, batches=r.n_batches, min_margin=r.min_margin, mlpd_marginal=round(lpd(models), 4),
                         mlpd_hyper=round(lpd(ml2), 4)))
    return rows


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parts", default="cells,update,scale,quality")
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    parts = [p for p in a.parts.split(",") if p]
    out = dict(metric="marginal")
    if set(parts) & {"cells", "update", "scale"}:
        import torch
        out["device"] = torch.cuda.get_device_name(0)
    if "cells" in parts:
        out["cells"] = part_cells(a.reps)
    if "update" in parts:
        out["update"] = part_update(a.reps)
    if "scale" in parts:
        out["scale"] = part_scale(max(2, a.reps // 5))
    if "quality" in parts:
        out["quality"] = part_quality()
    line = json.dumps(out)
    print(line, flush=True)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
