"""CPU-only: the maths of the NumPy restatement of Thompson sampling (tests/thompson_ref.py) - the restatement is what the
GPU tests compare the kernels with, so its own properties are pinned here: the interpolation identity of pathwise
conditioning, the posterior moments against the oracle, the derived tolerance against long double, and the selection rule."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import thompson_ref as T  # noqa: E402
from bayesian_optimisation_amd.synthetic import make_problem  # noqa: E402
from oracle import gp_oracle as O  # noqa: E402


@pytest.mark.parametrize("N,d", [(5, 3), (127, 2), (129, 8), (300, 16)])
def test_interpolation_identity(N, d):
    """f_s(X_n) + kappa v_s[n] + sqrt(kappa) E[s,n] == y_n, exactly for ANY number of features: conditioning is exact on
    whatever prior sample it is given.  (Observed: <= 1.2e-12.)"""
    X, y, _, ls = make_problem(N, 64, d)
    omega, phase, W, E = T.draws(d, 96, 8, N, 3)
    V = T.weights(X, y, ls, omega, phase, W, E)
    R = T.residual(X, y, ls, omega, phase, W, E)
    f = T.paths(X, X, ls, omega, phase, W, V)
    err = np.max(np.abs(f + T.KAPPA * V + np.sqrt(T.KAPPA) * E - y[None, :]))
    print(f"N={N} d={d}: identity error {err:.3g}, |R|_inf {np.abs(R).max():.3g}")
    assert err <= 1e-10 * max(1.0, np.abs(R).max())


@pytest.mark.parametrize("N,M,d,F,S,seed", [(20, 96, 2, 4096, 4096, 11), (200, 96, 8, 2048, 2048, 5)])
def test_posterior_moments_against_the_oracle(N, M, d, F, S, seed):
    """Mean and variance over S paths against oracle.gp_oracle.posterior_chol (N != M: no diagonal quirk).  The mean is
    unbiased (standard error std / sqrt(S)); the variance carries the O(1 / sqrt F) error of the feature approximation of
    the prior.  Fixed seeds: deterministic.  (Observed: 1.7 and 2.9 standard errors; 8.5e-4 and 3.6e-2.)"""
    X, y, Xs, ls = make_problem(N, M, d)
    omega, phase, W, E = T.draws(d, F, S, N, seed)
    f = T.paths(Xs, X, ls, omega, phase, W, T.weights(X, y, ls, omega, phase, W, E))
    mu, sigma = O.posterior_chol(X, y, Xs, ls)
    z = np.abs(f.mean(axis=0) - mu) / (f.std(axis=0, ddof=1) / np.sqrt(S))
    dv = np.abs(f.var(axis=0, ddof=1) - sigma ** 2)
    print(f"N={N}: mean off by {z.max():.2f} standard errors, variance off by {dv.max():.3g} (bound {3 / np.sqrt(F):.3g})")
    assert z.max() <= 4.5
    assert dv.max() <= 3.0 / np.sqrt(F)


@pytest.mark.parametrize("case", T.KERNEL_CASES, ids=lambda c: "-".join(map(str, c)))
def test_fp64_restatement_stays_far_inside_the_derived_bound(case):
    """fp64 NumPy against long double on every case of the kernel test, with V and without (the prior paths alone): at most
    0.15 x tol.  The GPU kernel is held to 1.0 x tol; it differs from this restatement by its summation order (one chain over
    N and over F where NumPy sums pairwise or in blocks), its contracted multiply-adds, a 1-ulp exp and its own cosine, so
    the restatement's own share of the bound has to leave it most of the bound: a factor of 6 here.
    The figure is not a worst case - the restatement makes d + 4 or more roundings in the angle alone (x / (2 pi ls): two, the
    product with Omega^T: d or more, + phase, 2 pi t) where the bound allows d + 8 aligned ones for angle, cosine and sums
    together - but what independent roundings leave of it.  Observed: with V at most 0.093 over the generator seeds 1 .. 12
    for V (the figure sits at the rounding of |f| ~ 300 itself, one ulp of which is 0.05 x tol, and moves with the draw; half
    of those seeds exceed 0.06 on some case), without V at most 0.107 (case (128, 511, 5, 2, 15): two features, nothing
    averages)."""
    r = T.kernel_reference(case)
    X, Xs, ls, omega, phase, W = (r[k] for k in ("X", "Xs", "ls", "omega", "phase", "W"))
    for Vv, fld, tol in ((r["V"], r["f"], r["tol"]), (None, r["f_prior"], r["tol_prior"])):
        f64 = T.paths(Xs, X, ls, omega, phase, W, Vv)
        ratio = float(np.max(np.abs(f64 - fld) / tol))
        print(f"{case} V={'given' if Vv is not None else 'None'}: max |f64 - fld| / tol = {ratio:.3g}")
        assert ratio <= 0.15


def test_long_double_weights_solve_the_system():
    X, y, _, ls = make_problem(129, 8, 8)
    omega, phase, W, E = T.draws(8, 64, 4, 129, 1)
    V = T.weights(X, y, ls, omega, phase, W, E, xp=np.longdouble)
    R = T.residual(X, y, ls, omega, phase, W, E, xp=np.longdouble)
    K = T.k0(X, X, ls, np.longdouble) + np.longdouble(T.KAPPA) * np.eye(129, dtype=np.longdouble)
    assert float(np.max(np.abs(V @ K - R))) <= 1e-14 * float(np.abs(R).max())
    V64 = T.weights(X, y, ls, omega, phase, W, E)
    assert np.max(np.abs(V64 - V.astype(np.float64))) <= 1e-9 * np.abs(V64).max() * 1e3   # cond(K) ~ 1e6


def test_selection_rule_first_q_distinct_winners_in_path_order():
    """DeviceGP.select_thompson's host logic with the device call replaced by the restatement."""
    X, y, Xs, ls = make_problem(40, 300, 2)
    omega, phase, W, E = T.draws(2, 256, 16, 40, 0)
    f = T.paths(Xs, X, ls, omega, phase, W, T.weights(X, y, ls, omega, phase, W, E))
    idx, _ = T.winners(f)
    keep = T.first_distinct(idx, 4)
    chosen = idx[keep]
    assert len(set(chosen.tolist())) == len(chosen) <= 4
    # path order: every kept path is the first one with its winner, and nothing distinct was skipped before the last kept
    seen = []
    for s in range(int(keep[-1]) + 1):
        if idx[s] not in seen:
            seen.append(int(idx[s]))
    assert chosen.tolist() == seen[: len(chosen)]
    # paths that agree give fewer than q points; -1 (no usable row) is never a point
    assert T.first_distinct(np.array([7, 7, 7, 7]), 3).tolist() == [0]
    assert T.first_distinct(np.array([5, -1, 5, 2, -1, 9]), 3).tolist() == [0, 3, 5]
    assert T.first_distinct(np.array([5, 3, 5, 2]), 2).tolist() == [0, 1]
    assert T.first_distinct(np.array([-1, -1]), 2).size == 0


def test_draws_are_the_contracted_sequence():
    omega, phase, W, E = T.draws(3, 5, 2, 4, 9)
    rng = np.random.default_rng(9)
    assert np.array_equal(omega, rng.standard_normal((5, 3))) and np.array_equal(phase, rng.uniform(0.0, 1.0, 5))
    assert np.array_equal(W, rng.standard_normal((2, 5))) and np.array_equal(E, rng.standard_normal((2, 4)))
    assert np.all((phase >= 0) & (phase < 1))
