"""The two NumPy statements of greedy q-point batch selection (tests/batch_ref.py) held to each other: refitting the
augmented GP from scratch per member against the rank-one recurrence the kernel implements (csrc/batch.hip).  The GPU
tests compare the library with greedy_refit; this file shows, without a GPU, that the recurrence IS the refit - and that the
inputs decide something: every step's top-2 gap is far above the deviations, and the q members are distinct."""
import numpy as np
import pytest

import batch_ref as R
from bayesian_optimisation_amd.synthetic import make_problem


@pytest.mark.parametrize("name", R.MODE_NAMES)
@pytest.mark.parametrize("N,M,d", R.PROBLEMS)
def test_recurrence_equals_refit(N, M, d, name):
    X, y, Xs, ls = make_problem(N, M, d)
    acq_kw, fantasy, lie = R.mode(name, y)
    a = R.greedy_refit(X, y, Xs, ls, R.Q, acq_kw, fantasy, lie)
    b = R.greedy_recurrence(X, y, Xs, ls, R.Q, acq_kw, fantasy, lie)
    dmu, dsig = np.max(np.abs(a["mu"] - b["mu"])), np.max(np.abs(a["sigma"] - b["sigma"]))
    print(f"N={N} M={M} d={d} {name}: idx {a['indices'].tolist()} min gap {a['gaps'].min():.3g} dmu {dmu:.3g} dsigma {dsig:.3g} "
          f"min sigma {a['sigma'].min():.3g}")
    # the inputs are informative
    assert a["gaps"].min() >= 1e-5 and b["gaps"].min() >= 1e-5
    assert len(set(a["indices"].tolist())) == R.Q
    assert np.array_equal(a["indices"], b["indices"])
    assert dmu <= 1e-9 * max(1.0, np.abs(y).max())
    assert dsig <= 1e-8
    assert np.allclose(a["values"], b["values"], rtol=0, atol=1e-8 * max(1.0, np.abs(y).max()))


def test_believer_leaves_the_mean_alone_and_shrinks_the_variance():
    X, y, Xs, ls = make_problem(64, 2048, 2)
    acq_kw, fantasy, lie = R.mode("lcb_believer", y)
    mu0, sig0 = R.posterior(X, y, Xs, ls)
    b = R.greedy_recurrence(X, y, Xs, ls, 4, acq_kw, fantasy, lie)
    assert np.array_equal(b["mu"], mu0)
    assert np.all(b["sigma"] <= sig0 + 1e-15) and b["sigma"][b["indices"][:3]].max() < 0.02
