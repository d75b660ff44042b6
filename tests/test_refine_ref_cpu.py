"""The NumPy restatement of the acquisition gradients and the refinement rule (tests/refine_ref.py) held to itself, without a
GPU: the analytic gradients against central differences in long double, float64 against long double, the gains of the
issue's table, and that the trajectory cases of tests/test_gpu_refine.py are decided."""
import functools

import numpy as np
import pytest

import refine_ref as R
from bayesian_optimisation_amd.synthetic import make_problem


@functools.lru_cache(maxsize=None)
def _problem(N, M, d):
    return make_problem(N, M, d)


@functools.lru_cache(maxsize=None)
def _model(N, M, d):
    X, y, _, ls = _problem(N, M, d)
    return R.Model(X, y, ls)


@pytest.mark.parametrize("N,d", [(64, 2), (300, 8), (512, 16)])
def test_gradients_equal_central_differences_in_long_double(N, d):
    """48 Sobol points; bound 1e-8 (measured when the rule was specified: <= 6.1e-10)."""
    X, y, Xs, ls = _problem(N, 4096, d)
    Q = Xs[:48]
    ml = R.Model(X, y, ls, np.longdouble)
    for name in R.ACQS:
        kw = R.acq_kw(name, y, table=True)
        g = _model(N, 4096, d).grad(Q, **kw)
        cd = R.central_differences(ml, Q, h=1e-7, **kw)
        for key in ("dmu", "dsigma", "dacq"):
            err = float(np.max(np.abs(g[key] - cd[key])))
            print(f"N={N} d={d} {name} {key}: max |analytic - central difference| {err:.3g}, max |gradient| {np.abs(g[key]).max():.3g}")
            assert err <= 1e-8


@pytest.mark.parametrize("N,d", [(64, 2), (300, 8)])
def test_float64_and_long_double_agree(N, d):
    """Bound: the float64 solves carry cond_2(K) eps of relative error, with the condition number of the matrix that was
    actually factorised (cond_2(L)^2: 2.7e5 at (64, 2), 2.6e3 at (300, 8) - not the worst case N / jitter, which is three
    orders wider), against the largest entry of the quantity: 6e-11 and 6e-13 times that entry.  A restatement wrong in
    the tenth digit fails.  Measured when the rule was specified: <= 4.1e-12 on gradients of size ~10."""
    X, y, Xs, ls = _problem(N, 4096, d)
    Q = Xs[:48]
    cond = float(np.linalg.cond(_model(N, 4096, d).L)) ** 2
    for name in R.ACQS:
        kw = R.acq_kw(name, y, table=True)
        a, b = R.posterior_grad(X, y, ls, Q, **kw), R.posterior_grad(X, y, ls, Q, dtype=np.longdouble, **kw)
        for key in ("mu", "sigma", "acq", "dmu", "dsigma", "dacq"):
            err = float(np.max(np.abs(a[key] - b[key])))
            tol = cond * np.finfo(np.float64).eps * max(1.0, float(np.abs(a[key]).max()))
            print(f"N={N} d={d} {name} {key}: {err:.3g} (bound {tol:.3g})")
            assert err <= tol


@pytest.mark.parametrize("name", R.ACQS)
@pytest.mark.parametrize("N,M,d", R.TABLE)
def test_every_start_of_the_table_improves(N, M, d, name):
    """64 best grid candidates, 30 iterations inside [0, 1]^d, EI at f_best = min y: every start gains."""
    X, y, Xs, ls = _problem(N, M, d)
    kw = R.acq_kw(name, y, table=True)
    m = _model(N, M, d)
    idx, S, a = R.starts(X, y, Xs, ls, model=m, **kw)
    assert idx[0] == int(np.flatnonzero(a == a.max())[0])
    r = R.refine(X, y, ls, S, 0.0, 1.0, iters=30, model=m, **kw)
    # the starts are inside the box: the clipped start is the candidate (two BLAS calls of different shapes: rounding only)
    assert np.max(np.abs(r["acq0"] - a[idx])) <= 1e-12 * max(1.0, np.abs(y).max())
    print(f"N={N} d={d} {name}: grid best {a.max():.4g} -> refined best {r['acq'].max():.4g}, smallest gain "
          f"{(r['acq'] - r['acq0']).min():.3g}, pg {r['pg'].min():.2g} .. {r['pg'].max():.2g}")
    assert np.all(r["acq"] > r["acq0"])
    assert np.all((r["x"] >= 0.0) & (r["x"] <= 1.0))
    assert r["best"] == int(np.flatnonzero(r["acq"] == r["acq"].max())[0]) and r["nan_count"] == 0


@pytest.mark.parametrize("name", R.ACQS)
@pytest.mark.parametrize("N,M,d", R.CASES)
def test_the_trajectory_cases_are_decided(N, M, d, name):
    """At 12 iterations every accept / reject decision of (nearly) every start has an Armijo margin above 1e-7, so the
    GPU's trajectory can be held to this one decision by decision."""
    X, y, Xs, ls = _problem(N, M, d)
    kw = R.acq_kw(name, y)
    m = _model(N, M, d)
    _, S, _ = R.starts(X, y, Xs, ls, model=m, **kw)
    r = R.refine(X, y, ls, S, 0.0, 1.0, iters=R.TRAJ_ITERS, model=m, **kw)
    mask = R.decided(r)
    print(f"N={N} d={d} {name}: {int(mask.sum())} of {len(mask)} decided, smallest margin {r['margin'].min():.3g}")
    assert mask.sum() >= R.N_STARTS - R.MAX_UNDECIDED


def test_the_rule_at_its_edges():
    X, y, Xs, ls = _problem(64, 2048, 2)
    m = _model(64, 2048, 2)
    S = Xs[:6].copy()
    S[1] = [1.7, -0.3]          # outside the box: clipped
    S[2, 0] = np.nan            # never moves, reports NaN
    r0 = R.refine(X, y, ls, S, 0.0, 1.0, iters=0, model=m)
    assert np.array_equal(r0["x"][[0, 1]], np.clip(S[[0, 1]], 0.0, 1.0)) and np.array_equal(r0["acq"][:2], r0["acq0"][:2])
    r = R.refine(X, y, ls, S, [0.0, 0.25], [1.0, 0.25], iters=10, model=m)
    assert np.all(r["x"][[0, 1, 3, 4, 5], 1] == 0.25)               # lower == upper pins the coordinate
    assert r["nan_count"] == 1 and np.isnan(r["acq"][2]) and np.isnan(r["acq0"][2]) and r["accepted"][2] == 0
    assert np.isnan(r["x"][2, 0]) and r["best"] != 2
    # 50 length scales away: the prior, no gradient, a frozen point
    far = R.refine(X, y, ls, np.array([[0.5 + 50 * ls[0], 0.5]]), -100.0, 100.0, iters=5, model=m)
    assert far["accepted"][0] == 0 and far["acq"][0] == 4.0 * np.sqrt(R.KAPPA) and far["pg"][0] == 0.0
