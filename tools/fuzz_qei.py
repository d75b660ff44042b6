"""Randomised sweep of the q = 8 Monte-Carlo qEI route (DeviceGP.score_qei: the GRAM form of sigma_acq_kernel + qei_kernel)
against the fp64 oracle (oracle.gp_oracle.qei_mc): random N in [1, 400], d in [1, 16], M a multiple of 8 up to 3000, chunk
512 / 1024, S in [1, 600] base samples, xi in {0, 0.01, 0.05}, a non-zero batch offset, and up to three batches replaced by
degenerate ones (eight identical candidates / eight observed rows / eight candidates 1e-7 apart / four copies of an
observation + four of a candidate).  The incumbent is a quantile in [0.5, 0.9] of the ORACLE's posterior mean, so that the
values compared are not zeros; a draw whose reference has a batch below 1e-6 is drawn again.
The bar: |device - oracle| <= 1e-9 max(1, max|y|) on every batch, nan_count == 0, best_idx / best_val = the first maximum of
the dense output, and the oracle's arg-max when its top two differ by more than 1e-7.
tests/test_gpu_qei.py runs seeds 0..15 of `draw_case`.
usage: python tools/fuzz_qei.py [seconds] [first seed]"""
import os
import sys
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if REPO not in sys.path:
    sys.path.insert(0, REPO)
import numpy as np

from oracle import gp_oracle as O

DEGENERATE_KINDS = ("identical", "observed", "near", "copies")


def degenerate_batch(kind, X, Xs, b, base=None, obs=0):
    """Replace batch b of Xs (rows 8b .. 8b+7) in place by a degenerate batch built from candidate row `base` of Xs (default:
    the batch's first) and observation row `obs` of X.  All four are positive definite in exact arithmetic: the smallest
    eigenvalue of Sigma_b stays at or above the prior's jitter, 1.01e-4."""
    N, d = X.shape
    rows = slice(8 * b, 8 * b + 8)
    cand = Xs[8 * b if base is None else base].copy()
    if kind == "identical":          # eight identical candidates
        Xs[rows] = cand
    elif kind == "observed":         # the batch equal to eight observed rows (repeated where N < 8)
        Xs[rows] = X[(obs + np.arange(8)) % N]
    elif kind == "near":             # eight candidates 1e-7 apart
        Xs[rows] = cand + 1e-7 * np.arange(8)[:, None] * np.ones(d)
    elif kind == "copies":           # four copies of an observation + four copies of a candidate
        Xs[8 * b:8 * b + 4] = X[obs]
        Xs[8 * b + 4:8 * b + 8] = cand
    else:
        raise ValueError(kind)


def oracle_mean(X, y, Xs, ls):
    """The oracle's posterior mean at Xs (no same-shape jitter quirk, as qei_mc forms it per batch)."""
    _, _, alpha = O.factorise(X, y, ls)
    d2 = np.zeros((len(X), len(Xs)))
    for k in range(X.shape[1]):
        d2 += (X[:, k, None] - Xs[None, :, k]) ** 2 / ls[k] ** 2
    return np.exp(-0.5 * d2).T @ alpha


def plant(kind, X, y, Xs, ls, b):
    """A degenerate batch that still says something: built from the candidate of batch b with the lowest oracle mean and the
    observation with the lowest y, so that an incumbent at or above the median of the mean leaves its qEI positive."""
    mu = oracle_mean(X, y, Xs[8 * b:8 * b + 8], ls)
    degenerate_batch(kind, X, Xs, b, base=8 * b + int(np.argmin(mu)), obs=int(np.argmin(y)))


def oracle_incumbent(X, y, Xs, ls, quantile):
    """A quantile of the oracle's posterior mean at the candidates (the incumbent never comes from the device)."""
    return float(np.quantile(oracle_mean(X, y, Xs, ls), quantile))


def _draw(rng):
    N = int(rng.integers(1, 401))
    d = int(rng.integers(1, 17))
    M = 8 * int(rng.integers(1, 376))
    chunk = int(rng.choice([512, 1024]))
    S = int(rng.integers(1, 601))
    xi = float(rng.choice([0.0, 0.01, 0.05]))
    quantile = float(rng.uniform(0.5, 0.9))
    X = rng.uniform(0, 1, (N, d))
    Xs = rng.uniform(0, 1, (M, d))
    ls = np.exp(rng.uniform(np.log(0.1), np.log(2.0), d))
    y = np.sin(X @ rng.standard_normal(d) * 3.0) * float(rng.choice([1.0, 50.0])) + 0.01 * rng.standard_normal(N)
    planted = []
    for b in sorted(set(int(v) for v in rng.integers(0, M // 8, int(rng.integers(0, 4))))):
        kind = str(rng.choice(DEGENERATE_KINDS))
        plant(kind, X, y, Xs, ls, b)
        planted.append((b, kind))
    c = dict(X=X, y=y, Xs=Xs, ls=ls, Z=rng.standard_normal((S, 8)), xi=xi, chunk=chunk, quantile=quantile,
             f_best=oracle_incumbent(X, y, Xs, ls, quantile), batch_offset=int(rng.integers(1, 1 << 40)), planted=planted)
    c["ref"] = O.qei_mc(X, y, Xs, ls, c["Z"], c["f_best"], xi)
    return c


def draw_case(seed):
    """One seeded case: dict(X, y, Xs, ls, Z, f_best, xi, chunk, batch_offset, planted=[(batch, kind), ...], ref=the oracle's
    values, attempt).  A draw whose REFERENCE has a batch below 1e-6 is drawn again (a few per cent of them: eight random
    candidates that all lie well above the incumbent): the input changes, never the threshold, and the device is not asked."""
    for attempt in range(64):
        c = _draw(np.random.default_rng(31000 + seed if attempt == 0 else [31000 + seed, attempt]))
        if np.isfinite(c["ref"]).all() and c["ref"].min() >= 1e-6:
            c["attempt"] = attempt
            return c
    raise RuntimeError(f"seed {seed}: no informative case in 64 draws")


def check_case(c, ref=None):
    """Score the case on the device and compare with the oracle; returns the list of what is wrong (empty = pass)."""
    from bayesian_optimisation_amd import DeviceGP

    if ref is None:
        ref = c["ref"]
    wrong = []
    if not (np.isfinite(ref).all() and ref.min() >= 1e-6):
        wrong.append(f"generator: reference has a batch below 1e-6 (min {ref.min():.3e})")
    gp = DeviceGP(chunk=c["chunk"]).factorise(c["X"], c["y"], c["ls"])
    r = gp.score_qei(c["Xs"], c["Z"], c["f_best"], xi=c["xi"], dense=True, batch_offset=c["batch_offset"])
    got = r.acq.cpu().numpy()
    err = float(np.max(np.abs(got - ref)))
    if not err <= 1e-9 * max(1.0, float(np.abs(c["y"]).max())):
        wrong.append(f"max |device - oracle| = {err:.3e} at batch {int(np.nanargmax(np.abs(got - ref)))}")
    if r.nan_count != 0:
        wrong.append(f"nan_count = {r.nan_count}")
    first = int(np.flatnonzero(got == got.max())[0]) if np.isfinite(got).all() else -1
    if r.best_idx != c["batch_offset"] + first or r.best_val != got.max():
        wrong.append(f"result ({r.best_val}, {r.best_idx}) is not the first maximum of the dense output ({got.max()}, {first})")
    top2 = np.sort(ref)[-2:] if len(ref) > 1 else np.array([-np.inf, ref[0]])
    if top2[1] - top2[0] > 1e-7 and r.best_idx - c["batch_offset"] != int(np.flatnonzero(ref == ref.max())[0]):
        wrong.append(f"arg-max {r.best_idx - c['batch_offset']} is not the oracle's {int(np.argmax(ref))}")
    return wrong


def main():
    budget = float(sys.argv[1]) if len(sys.argv) > 1 else 60.0
    seed = int(sys.argv[2]) if len(sys.argv) > 2 else 16
    t_end = time.time() + budget
    n_cases = n_fail = 0
    while time.time() < t_end:
        c = draw_case(seed)
        tag = f"seed={seed} N={c['X'].shape[0]} d={c['X'].shape[1]} M={len(c['Xs'])} S={len(c['Z'])} xi={c['xi']} " \
              f"chunk={c['chunk']} planted={c['planted']}"
        try:
            wrong = check_case(c)
        except Exception as exc:  # noqa: BLE001
            wrong = [f"{type(exc).__name__}: {exc}"]
        n_cases += 1
        if wrong:
            n_fail += 1
            print("FAIL", tag, wrong, flush=True)
        seed += 1
        if n_cases % 25 == 0:
            print(f"... {n_cases} cases, {n_fail} failures", flush=True)
    print(f"fuzz_qei: {n_cases} cases, {n_fail} failures (next seed {seed})")
    return 1 if n_fail else 0


if __name__ == "__main__":
    sys.exit(main())
