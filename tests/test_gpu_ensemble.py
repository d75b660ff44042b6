"""Candidates scored under an ensemble of surrogates on the GPU (csrc/ensemble.hip, DeviceEnsemble) against the single-model path
it is built on - bit for bit - and against the NumPy restatement (tests/ensemble_ref.py) within bounds propagated from the
per-model bounds the suite already holds; the premises of the index comparisons are checked on the CPU in
tests/test_ensemble_ref_cpu.py."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

import ensemble_ref as E  # noqa: E402
from bayesian_optimisation_amd import DeviceEnsemble, DeviceGP, ensemble  # noqa: E402
from bayesian_optimisation_amd.model import SurrogateModel  # noqa: E402
from bayesian_optimisation_amd.synthetic import make_problem  # noqa: E402

_REF = {}


def _np(t):
    return t.cpu().numpy()


def _fitted(models, family="se"):
    """ensemble_ref's model tuples as DeviceEnsemble takes them."""
    return [(ls, SurrogateModel(family, j1, j2, m, s, True), w) for ls, j1, j2, m, s, w in models]


def _case(N, M, d, family):
    """One problem and its restatement posteriors per (N, M, d, family), shared by the LCB and the EI test and left unchanged."""
    key = (N, M, d, family)
    if key not in _REF:
        X, y, Xs, models = E.case_problem(N, M, d)
        _REF[key] = (X, y, Xs, models, E.model_posteriors(X, y, Xs, models, family))
    return _REF[key]


@pytest.mark.parametrize("kind", [E.LCB, E.EI])
def test_one_unfitted_model_of_weight_one_is_the_single_model_pass_bit_for_bit(kind):
    X, y, Xs, ls = make_problem(130, 1000, 3)
    kw = dict(explore=4.0) if kind == E.LCB else dict(f_best=float(np.min(y)), xi=0.01)
    one = DeviceGP(device="cuda:0").factorise(X, y, ls).score(Xs, acquisition=kind, dense=True, idx_offset=7, **kw)
    ens = DeviceEnsemble(device="cuda:0").factorise(X, y, [(ls, SurrogateModel("se"), 1.0)])
    r = ens.score(Xs, acquisition=kind, dense=True, idx_offset=7, **kw)
    assert np.array_equal(_np(r.acq), _np(one.acq)) and np.array_equal(_np(r.mean), _np(one.mu))
    assert (r.best_val, r.best_idx, r.nan_count) == (one.best_val, one.best_idx, one.nan_count) and r.nan_count == 0
    np.testing.assert_allclose(_np(r.sd), _np(one.sigma), rtol=0, atol=1e-12)   # sqrt((sigma^2 + mu^2) - mu^2)
    lean = ens.score(Xs, acquisition=kind, idx_offset=7, **kw)                  # no dense outputs: the same record
    assert lean.mean is None and (lean.best_val, lean.best_idx, lean.nan_count) == (r.best_val, r.best_idx, 0)


@pytest.mark.parametrize("N,M,d,family", E.CASES)
@pytest.mark.parametrize("kind", [E.LCB, E.EI])
def test_five_fitted_models_match_the_restatement(N, M, d, family, kind):
    X, y, Xs, models, post = _case(N, M, d, family)
    p0, p1 = E.case_params(kind, y)
    ref = E.fold(post, models, kind, p0, p1)
    kw = dict(explore=p0) if kind == E.LCB else dict(f_best=p0, xi=p1)
    r = DeviceEnsemble(device="cuda:0").factorise(X, y, _fitted(models, family)).score(Xs, acquisition=kind, dense=True, **kw)
    acq, mean, sd = _np(r.acq), _np(r.mean), _np(r.sd)
    B, Bm, Bv = E.acq_bound(y, models, kind, E.EXPLORE), E.mean_bound(y, models), E.var_bound(y, models, post, ref["shift"])
    ea, em, ev = np.max(np.abs(acq - ref["acq"])), np.max(np.abs(mean - ref["mean"])), np.max(np.abs(sd * sd - ref["var"]) / Bv)
    print(f"N {N} M {M} d {d} {family} {kind}: |acq - ref| {ea:.2e} (bound {B:.2e}), |mean - ref| {em:.2e} (bound {Bm:.2e}), "
          f"|var - ref| / bound {ev:.2e}")
    assert ea <= B and em <= Bm and ev <= 1.0
    assert r.nan_count == 0 and r.best_idx == ref["best_idx"] and abs(r.best_val - ref["best_val"]) <= B
    assert r.best_val == acq[r.best_idx] and r.best_idx == int(np.argmax(acq))


def test_the_chunk_and_a_second_call_change_no_bit():
    X, y, Xs, models, _ = _case(129, 1000, 16, "se")
    runs = []
    for chunk in (512, 4096, 4096):
        ens = DeviceEnsemble(device="cuda:0", chunk=chunk).factorise(X, y, _fitted(models))
        r = ens.score(Xs, acquisition="ei", f_best=float(np.min(y)), xi=E.EI_XI, dense=True)
        runs.append((r.best_val, r.best_idx, r.nan_count, _np(r.acq), _np(r.mean), _np(r.sd)))
        if len(runs) == 3:   # and again on the same object
            r = ens.score(Xs, acquisition="ei", f_best=float(np.min(y)), xi=E.EI_XI, dense=True)
            runs.append((r.best_val, r.best_idx, r.nan_count, _np(r.acq), _np(r.mean), _np(r.sd)))
    for other in runs[1:]:
        assert other[:3] == runs[0][:3]
        assert all(np.array_equal(a, b) for a, b in zip(other[3:], runs[0][3:]))


def test_a_nan_candidate_is_counted_and_does_not_poison_its_neighbours():
    X, y, Xs, models, _ = _case(7, 511, 3, "se")
    ens = DeviceEnsemble(device="cuda:0").factorise(X, y, _fitted(models))
    clean = ens.score(Xs, dense=True)
    clean = (clean.best_idx, _np(clean.acq), _np(clean.mean), _np(clean.sd))
    bad = Xs.copy()
    hit = (clean[0] + 1) % len(Xs)   # next to the winner
    bad[hit, 1] = np.nan
    r = ens.score(bad, dense=True)
    assert r.nan_count == 1 and r.best_idx == clean[0]
    keep = np.arange(len(Xs)) != hit
    for got, want in zip((_np(r.acq), _np(r.mean), _np(r.sd)), clean[1:]):
        assert np.isnan(got[hit]) and np.array_equal(got[keep], want[keep])
    bad[clean[0], 0] = np.nan        # the winner itself: the runner-up takes over
    r2 = ens.score(bad, dense=True)
    assert r2.nan_count == 2 and r2.best_idx == int(np.nanargmax(_np(r2.acq))) and r2.best_idx != clean[0]


def test_weights_need_not_be_equal():
    X, y, Xs, models, post = _case(128, 513, 8, "se")
    w = np.array([0.5, 0.0, 0.25, 0.125, 0.125])
    weighted = [m[:5] + (float(wi),) for m, wi in zip(models, w)]
    ref = E.fold(post, weighted, E.LCB, E.EXPLORE)
    r = DeviceEnsemble(device="cuda:0").factorise(X, y, _fitted(weighted)).score(Xs, dense=True)
    assert np.max(np.abs(_np(r.acq) - ref["acq"])) <= E.acq_bound(y, weighted, E.LCB, E.EXPLORE)
    assert np.max(np.abs(_np(r.mean) - ref["mean"])) <= E.mean_bound(y, weighted)


def test_refusals(monkeypatch):
    X, y, Xs, models, _ = _case(7, 511, 3, "se")
    ens = DeviceEnsemble(device="cuda:0")
    with pytest.raises(ensemble._lib.GpboError):
        ens.score(Xs)                                            # nothing factorised
    broken = list(models)
    broken[3] = broken[3][:1] + (-1.0,) + broken[3][2:]          # rho = -1: a negative diagonal
    with pytest.raises(np.linalg.LinAlgError, match="model 3"):
        ens.factorise(X, y, _fitted(broken))
    with pytest.raises(ensemble._lib.GpboError):
        ens.score(Xs)                                            # and the failed ensemble is not scored
    for bad in ([], _fitted(models) * 13, _fitted(models[:2]) + _fitted(models[2:], "matern32"),
                [(m[0][:2], m[1], m[2]) for m in _fitted(models)], [(m[0], m[1], -0.2) for m in _fitted(models)]):
        with pytest.raises(ValueError):
            ens.factorise(X, y, bad)
    with pytest.raises(ValueError, match="d <= 16"):
        ens.factorise(np.ones((3, 17)), np.arange(3.0), [(np.ones(17), SurrogateModel("se"), 1.0)])
    monkeypatch.setattr(ensemble, "ENSEMBLE_MAX_BYTES", 5 * 128 * 128 * 8 - 1)
    with pytest.raises(ValueError, match="ENSEMBLE_MAX_BYTES"):
        ens.factorise(X, y, _fitted(models))
    monkeypatch.undo()
    ens.factorise(X, y, _fitted(models))
    with pytest.raises(ValueError):
        ens.score(Xs[:, :2])
    with pytest.raises(ValueError):
        ens.score(Xs, acquisition="ei")                          # EI needs f_best
