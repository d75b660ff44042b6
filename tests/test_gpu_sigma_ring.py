"""Every ring phase of the fp64 variance kernel's tile loop (csrc/sigma_acq.hip), bit for bit against recorded results.

The k tiles of `sigma_acq_kernel` go through a ring of three LDS stages.  The full tiles (left of the diagonal block of U)
run three at a time from ring position 0 with fragment addresses that are compile-time constants; up to two tiles in front
of such a run, up to two behind it and the diagonal block go through the form that takes the ring position at run time.
Column block jb has 8 jb full tiles and the position at its start depends on everything before it, so which tiles take
which form changes from block to block.  tests/test_gpu_sigma_bits.py (N = 384 and 2048) does not reach every combination;
the sizes here do, at 1,024 candidates and d = 8 (Sobol problems of bayesian_optimisation_amd/synthetic.py):

  N = 128    one column block, no full tile at all
  N = 256, 640, 896, 1152    2, 5, 7 and 9 column blocks with runs of 8 to 64 full tiles.  A plain launch has
             4 jb (jb + 1) tiles in front of block jb, so its blocks start at ring position 0 or 2 only: no tile or one
             in front of the runs of three, none or one behind them.  Position 1 (two tiles in front) and two tiles
             behind occur in the launches of eight column groups, which test_gpu_sigma_bits.py's n2048 takes
  bound      N = 1152, score_bound after factorise(order="fps"): the prefix mode (ncb > 0) and the column-split launches
             S > 1 of the re-scoring, whose column blocks come in boustrophedon order
  qei        N = 1152, score_qei(dense=True) with f_best = median(y): the GRAM instantiation
  chunks     N = 1152 scored in one chunk of 1,024 and in two of 512: the same bits, and the recorded ones

tests/golden/sigma_ring_*.npz were recorded on an MI355X from the library as it was BEFORE the loop took this form (the
parent commit's build, loaded through GPBO_LIB: `GPBO_LIB=<parent libgpbo.so> python tests/test_gpu_sigma_ring.py --record`,
which computes every case twice and refuses to write a case that is not reproducible).  Every comparison is
np.array_equal / ==: no tolerance."""
import functools
import json
import os
import sys

import numpy as np
import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if REPO not in sys.path:
    sys.path.insert(0, REPO)
GOLDEN = os.path.join(REPO, "tests", "golden")

pytestmark = pytest.mark.gpu

M, D = 1024, 8
DENSE_N = (128, 256, 640, 896, 1152)


def _record_of(r):
    return np.array([r.best_val, float(r.best_idx), float(r.nan_count)])


@functools.lru_cache(maxsize=None)
def _problem(N):
    from bayesian_optimisation_amd.synthetic import make_problem

    return make_problem(N, M, D)


def _dense_lcb(N, chunk=None):
    from bayesian_optimisation_amd import DeviceGP

    X, y, Xs, ls = _problem(N)
    gp = (DeviceGP(chunk=chunk) if chunk else DeviceGP()).factorise(X, y, ls)
    r = gp.score(Xs, dense=True, acquisition="lcb", explore=4.0)
    return {"mu": r.mu.cpu().numpy(), "sigma": r.sigma.cpu().numpy(), "acq": r.acq.cpu().numpy(), "result": _record_of(r)}


def _bound():
    from bayesian_optimisation_amd import DeviceGP

    X, y, Xs, ls = _problem(1152)
    gp = DeviceGP().factorise(X, y, ls, order="fps")
    r = gp.score_bound(Xs)
    return {"result": _record_of(r), "screen": np.array(json.dumps(gp.last_screen, sort_keys=True))}


def _qei():
    from bayesian_optimisation_amd import DeviceGP

    X, y, Xs, ls = _problem(1152)
    gp = DeviceGP().factorise(X, y, ls)
    Z = np.random.default_rng(7).standard_normal((64, 8))
    r = gp.score_qei(Xs, Z, f_best=float(np.median(y)), dense=True)
    return {"qei": r.acq.cpu().numpy(), "result": _record_of(r)}


CASES = {**{f"n{N}": functools.partial(_dense_lcb, N) for N in DENSE_N}, "bound": _bound, "qei": _qei}


def _same(a, b):
    a, b = np.asarray(a), np.asarray(b)
    if a.dtype.kind in "US":
        return json.loads(str(a)) == json.loads(str(b))
    return a.shape == b.shape and np.array_equal(a, b)


def _load(name):
    return dict(np.load(os.path.join(GOLDEN, f"sigma_ring_{name}.npz"), allow_pickle=False))


def _assert_recorded(name, got):
    want = _load(name)
    assert set(got) == set(want), name
    for key in sorted(want):
        if not _same(got[key], want[key]):
            a, b = np.asarray(got[key]), np.asarray(want[key])
            detail = (f"{int(np.sum(a != b))} of {a.size} entries differ, max |diff| {np.max(np.abs(a - b)):.3e}"
                      if a.dtype.kind == "f" and a.shape == b.shape else f"{a} != {b}")
            pytest.fail(f"sigma_ring_{name}.npz[{key}]: {detail}")


@pytest.mark.parametrize("case", sorted(CASES))
def test_every_ring_phase_gives_the_recorded_bits(case):
    _assert_recorded(case, CASES[case]())


def test_the_chunk_size_does_not_change_the_bits():
    one, two = _dense_lcb(1152, chunk=1024), _dense_lcb(1152, chunk=512)
    for key in sorted(one):
        assert _same(one[key], two[key]), key
    _assert_recorded("n1152", two)


def _record(check_only=False):
    bad = 0
    for case in sorted(CASES):
        first, second = CASES[case](), CASES[case]()
        if not all(_same(first[k], second[k]) for k in first):
            print(f"NOT REPRODUCIBLE: {case}")
            bad += 1
            continue
        path = os.path.join(GOLDEN, f"sigma_ring_{case}.npz")
        if check_only:
            want = _load(case)
            same = set(want) == set(first) and all(_same(first[k], want[k]) for k in want)
            print(f"{case}: {'equal' if same else 'DIFFERENT'}")
            bad += 0 if same else 1
        else:
            np.savez_compressed(path, **first)
            print(f"{case}: wrote {os.path.getsize(path)} bytes", {k: np.asarray(v).shape for k, v in first.items()})
    return bad


if __name__ == "__main__":
    # --record [DIR]: write the fixtures (to DIR instead of tests/golden); --check: compare without pytest
    if len(sys.argv) > 2:
        GOLDEN = os.path.abspath(sys.argv[2])
        os.makedirs(GOLDEN, exist_ok=True)
    sys.exit(1 if _record(check_only=sys.argv[1:2] == ["--check"]) else 0)
