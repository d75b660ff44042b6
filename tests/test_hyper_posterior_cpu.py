"""The sampler of the hyperparameter posterior (bayesian_optimisation_amd/hyper_posterior.py) on the CPU: it is NumPy only, so
what it samples is checked here against densities whose moments are known - a correlated Gaussian in closed form, and the
profile-likelihood posterior of tests/hyper_ref.py by quadrature - and its bookkeeping against its documentation."""
import numpy as np
import pytest

import hyper_ref as H
from ard_fit_ref import gp_problem
from bayesian_optimisation_amd.hyper_posterior import MAX_SHRINK, sample

A = np.array([[1.0, 0.6, 0.3], [0.6, 1.5, -0.4], [0.3, -0.4, 0.8]])   # covariance of the Gaussian target
P = np.linalg.inv(A)
MODE = np.array([0.5, -1.0, 0.25])


def gauss(Z):
    return 0.5 * np.einsum("ci,ij,cj->c", Z - MODE, P, Z - MODE)


def test_the_same_seed_gives_the_same_states_and_counters():
    z0 = np.tile(MODE, (32, 1))
    a = sample(gauss, z0, [-10] * 3, [10] * 3, 5, seed=3)
    b = sample(gauss, z0, [-10] * 3, [10] * 3, 5, seed=3)
    c = sample(gauss, z0, [-10] * 3, [10] * 3, 5, seed=4)
    assert np.array_equal(a.states, b.states) and np.array_equal(a.values, b.values)
    assert (a.n_batches, a.min_margin, a.kept) == (b.n_batches, b.min_margin, b.kept)
    assert not np.array_equal(a.states, c.states)
    assert np.array_equal(a.values, gauss(a.states))            # the values belong to the states
    assert a.n_batches > 1 + 5 * 3 and 0.0 < a.min_margin < np.inf and a.sweeps == 5 and a.seed == 3


def test_every_batch_has_one_row_per_chain_and_every_state_stays_inside_the_box():
    lower, upper = np.array([0.0, -1.5, 0.0]), np.array([1.0, -0.5, 0.5])   # a box that cuts the Gaussian on every side
    seen = []

    def f(Z):
        seen.append(Z.copy())
        return gauss(Z)

    r = sample(f, np.tile(MODE, (64, 1)), lower, upper, 10, seed=0, width=2.0)   # (wider than the box: every end is clipped)
    assert len(seen) == r.n_batches and all(Z.shape == (64, 3) for Z in seen)
    for Z in seen:
        assert np.all(Z >= lower) and np.all(Z <= upper)
    assert np.all(r.states >= lower) and np.all(r.states <= upper)
    assert np.std(r.states[:, 0]) > 0.1                                        # and they move


def test_values_that_are_not_finite_are_never_accepted():
    """NaN inside a ball, +inf in a slab: no chain ever rests there, and the margin ignores those comparisons."""
    def f(Z):
        L = gauss(Z)
        L[np.sum((Z - (MODE + 1.0)) ** 2, axis=1) < 0.5] = np.nan
        L[Z[:, 1] > 0.5] = np.inf
        return L

    r = sample(f, np.tile(MODE, (128, 1)), [-10] * 3, [10] * 3, 10, seed=1)
    assert np.all(np.isfinite(r.values)) and np.all(np.isfinite(f(r.states))) and np.isfinite(r.min_margin)
    with pytest.raises(ValueError):
        sample(f, np.tile(MODE + 1.0, (4, 1)), [-10] * 3, [10] * 3, 1, seed=0)   # a start where the target is NaN


def test_a_coordinate_whose_shrinkage_does_not_end_keeps_its_value():
    """A target that is finite at the start only: every trial is outside, the chains stay, `kept` counts the updates."""
    z0 = np.tile(MODE, (8, 1))

    def f(Z):
        return np.where(np.all(Z == MODE, axis=1), 0.0, np.nan)

    r = sample(f, z0, [-10] * 3, [10] * 3, 2, seed=0)
    assert np.array_equal(r.states, z0) and r.kept == 8 * 3 * 2
    assert r.n_batches == 1 + 2 * 3 * (2 + MAX_SHRINK)   # per update: one step-out trial per side, then MAX_SHRINK draws


def test_refusals():
    z0 = np.tile(MODE, (4, 1))
    for kw in (dict(lower=[-10] * 2, upper=[10] * 3), dict(lower=[1] * 3, upper=[0] * 3), dict(lower=[-np.inf] * 3, upper=[1] * 3)):
        with pytest.raises(ValueError):
            sample(gauss, z0, sweeps=1, seed=0, **kw)
    for kw in (dict(width=0.0), dict(width=np.nan)):
        with pytest.raises(ValueError):
            sample(gauss, z0, [-10] * 3, [10] * 3, 1, 0, **kw)
    with pytest.raises(ValueError):
        sample(gauss, z0, [-10] * 3, [10] * 3, -1, 0)
    with pytest.raises(ValueError):
        sample(lambda Z: gauss(Z)[:-1], z0, [-10] * 3, [10] * 3, 1, 0)


@pytest.mark.parametrize("seed", [0, 1, 2])
def test_the_moments_of_a_correlated_gaussian(seed):
    """512 independent chains from the mode, 20 sweeps: the mean over the chains has the standard error sqrt(A_kk / 512)
    exactly (the chains are independent), and it is within four of them; so is every variance within four of its own,
    A_kk sqrt(2 / 511).  Measured |mean - mode| / se for the seeds 0 / 1 / 2: at most 1.15 / 0.55 / 1.15; 985 / 988 / 977 batches."""
    r = sample(gauss, np.tile(MODE, (512, 1)), [-10] * 3, [10] * 3, 20, seed=seed)
    se = np.sqrt(np.diag(A) / 512)
    dev = np.abs(r.states.mean(axis=0) - MODE) / se
    print(f"seed {seed}: {r.n_batches} batches, |mean - mode| / se {dev}, min margin {r.min_margin:.2e}, kept {r.kept}")
    assert np.all(dev <= 4.0) and r.kept == 0
    var = r.states.var(axis=0, ddof=1)
    assert np.all(np.abs(var - np.diag(A)) <= 4.0 * np.diag(A) * np.sqrt(2.0 / 511))


# ---- the profile-likelihood posterior of a small GP problem against quadrature ----------------------------------------------
LOWER, UPPER = np.log([0.05, 1e-4]), np.log([5.0, 1.0])   # z = (log ls, log rho)


def _batched_profile_likelihood(X, y):
    """hyper_ref.nlml_hyper's value for many (ls, rho) at once (d = 1): the same formulas on stacked matrices."""
    N = len(y)
    D2 = (X[:, 0, None] - X[None, :, 0]) ** 2

    def f(Z):
        ls, rho = np.exp(Z[:, 0]), np.exp(Z[:, 1])
        K = np.exp(-0.5 * D2[None] / (ls * ls)[:, None, None]) + rho[:, None, None] * np.eye(N)[None]
        Lc = np.linalg.cholesky(K)
        ab = np.linalg.solve(K, np.stack([np.broadcast_to(y, (len(Z), N)), np.ones((len(Z), N))], axis=2))
        a, b = ab[:, :, 0], ab[:, :, 1]
        m = a.sum(axis=1) / b.sum(axis=1)
        ra = np.einsum("ci,ci->c", y[None] - m[:, None], a - m[:, None] * b)
        s2 = ra / N
        return 0.5 * (ra / s2 + N * np.log(s2) + 2.0 * np.log(np.diagonal(Lc, axis1=1, axis2=2)).sum(axis=1) + N * np.log(2 * np.pi))
    return f


@pytest.mark.parametrize("seed", [0, 1])
def test_the_profile_likelihood_posterior_against_quadrature(seed):
    """gp_problem(seed, 20, 1, noise=0.05): the means of log ls and log rho over 512 chains (from the mode of the grid, 20
    sweeps) against a 200 x 200 midpoint quadrature of exp(-L) on the same box, within four standard errors
    sqrt(var_quadrature / 512)."""
    X, y = gp_problem(seed, 20, 1, noise=0.05)
    f = _batched_profile_likelihood(X, y)
    for z in (np.array([[-1.0, -3.0]]), np.array([[0.5, -6.0]])):   # the batched form is the restatement's
        assert f(z)[0] == pytest.approx(H.nlml_hyper(X, y, np.exp(z[0, :1]), float(np.exp(z[0, 1])))[0], rel=1e-11)
    n = 200
    axes = [lo + (np.arange(n) + 0.5) * (hi - lo) / n for lo, hi in zip(LOWER, UPPER)]
    G = np.stack(np.meshgrid(*axes, indexing="ij"), -1).reshape(-1, 2)
    Lg = f(G)
    p = np.exp(-(Lg - Lg.min()))
    p /= p.sum()
    mean = p @ G
    var = p @ (G - mean) ** 2
    r = sample(f, np.tile(G[np.argmin(Lg)], (512, 1)), LOWER, UPPER, 20, seed=seed)
    se = np.sqrt(var / 512)
    dev = np.abs(r.states.mean(axis=0) - mean) / se
    print(f"seed {seed}: quadrature mean {mean}, sd {np.sqrt(var)}; chains mean {r.states.mean(axis=0)}, |diff| / se {dev}, "
          f"{r.n_batches} batches, kept {r.kept}")
    assert np.all(dev <= 4.0)
