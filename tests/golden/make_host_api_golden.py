"""What every host-pointer entry point (csrc/host_api.hip, through bayesian_optimisation_amd.host_binding) computes, as bits.

tests/golden/host_api_*.npz were recorded on an MI355X from the library as it was BEFORE the entries shared one prologue
(the parent commit's build, loaded through GPBO_LIB):

    GPBO_LIB=<parent libgpbo.so> python tests/golden/make_host_api_golden.py [DIR]

Every case is computed twice and one that is not reproducible is not written.  tests/test_gpu_host_api.py imports CASES
from here and compares bit for bit.  Inputs: synthetic.make_problem at
  (N, d, M) = (5, 1, 24)      one observation block, the smallest qEI / batch / refinement problem
              (37, 2, 1000)   the reference's own size
              (130, 8, 1000)  past the 128 -> 256 padding edge
  d20         select_next at d = 20, (N, M) = (37, 1000): the any-d kernels
  bound       make_problem(1300, 50000, 6) without dense outputs: the bound route in farthest-point order
Keys are "<entry>.<field>" of the dict the binding returns (fields that are None are left out)."""
import functools
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(os.path.dirname(HERE))
if REPO not in sys.path:
    sys.path.insert(0, REPO)

PROBLEMS = {"n5_d1_m24": (5, 24, 1), "n37_d2_m1000": (37, 1000, 2), "n130_d8_m1000": (130, 1000, 8)}   # make_problem(N, M, d)


def _put(out, entry, r):
    for k, v in r.items():
        if v is not None:
            out[f"{entry}.{k}"] = np.asarray(v)


def _entries(N, M, d):
    from bayesian_optimisation_amd import host_binding as H
    from bayesian_optimisation_amd.synthetic import make_problem

    X, y, Xs, ls = make_problem(N, M, d)
    out = {}
    _put(out, "next_lcb", H.select_next(X, y, ls, Xs, want_cov_meas=True))
    _put(out, "next_ei", H.select_next(X, y, ls, Xs, acquisition="ei", f_best=float(y.min()), xi=0.01, want_cov_meas=True))
    Z = np.random.default_rng(7).standard_normal((64, 8))
    _put(out, "qei", H.select_qei(X, y, ls, Xs, Z, float(np.median(y))))
    _put(out, "batch_believer", H.select_batch(X, y, ls, Xs, 4, dense=True))
    _put(out, "batch_liar", H.select_batch(X, y, ls, Xs, 4, fantasy="liar", lie=float(y.min()), dense=True))
    _put(out, "thompson", H.select_thompson(X, y, ls, Xs, 2, n_features=64, dense=True))
    _put(out, "refine", H.refine(X, y, ls, Xs[:8], Xs.min(axis=0), Xs.max(axis=0), iters=5))
    cells = np.array([0.5, 0.7, 1.0, 1.4, 2.0, 3.0])[:, None] * ls[None, :]
    out["nlml_grid.reference"] = H.nlml_grid(X, y, cells)
    out["nlml_grid.logdet"] = H.nlml_grid(X, y, cells, likelihood="logdet")
    nlml, grad = H.nlml_and_grad(X, y, ls)
    out["nlml_and_grad"] = np.concatenate([[nlml], grad])
    return out


def _d20():
    from bayesian_optimisation_amd import host_binding as H
    from bayesian_optimisation_amd.synthetic import make_problem

    out = {}
    _put(out, "next_lcb", H.select_next(*_reordered(make_problem(37, 1000, 20))))
    return out


def _bound():
    from bayesian_optimisation_amd import host_binding as H
    from bayesian_optimisation_amd.synthetic import make_problem

    r = H.select_next(*_reordered(make_problem(1300, 50000, 6)), dense=False)
    return {f"next_lcb.{k}": np.asarray(r[k]) for k in ("best_idx", "best_val", "nan_count")}


def _reordered(problem):
    X, y, Xs, ls = problem   # make_problem's order -> select_next's
    return X, y, ls, Xs


CASES = {**{name: functools.partial(_entries, *nmd) for name, nmd in PROBLEMS.items()}, "d20": _d20, "bound": _bound}


def same_bits(a, b) -> bool:
    a, b = np.asarray(a), np.asarray(b)
    return a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()


def path(case, golden=HERE):
    return os.path.join(golden, f"host_api_{case}.npz")


if __name__ == "__main__":
    golden = os.path.abspath(sys.argv[1]) if len(sys.argv) > 1 else HERE
    os.makedirs(golden, exist_ok=True)
    bad = 0
    for case in sorted(CASES):
        first, second = CASES[case](), CASES[case]()
        if set(first) != set(second) or not all(same_bits(first[k], second[k]) for k in first):
            print(f"NOT REPRODUCIBLE: {case}", [k for k in first if not same_bits(first[k], second[k])])
            bad += 1
            continue
        np.savez_compressed(path(case, golden), **first)
        print(f"{case}: wrote {os.path.getsize(path(case, golden))} bytes, {len(first)} arrays", flush=True)
    sys.exit(1 if bad else 0)
