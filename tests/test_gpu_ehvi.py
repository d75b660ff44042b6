"""Two-objective expected hypervolume improvement in log space on the GPU (csrc/ehvi.hip; DeviceGP.ehvi_on_posterior /
select_ehvi, expected_hypervolume_improvement() of PointSelector and PointSelectorHost, the host entry) against tests/ehvi_ref.py,
the NumPy / SciPy restatement, whose own accuracy tests/test_ehvi_ref_cpu.py pins against 60-digit values.

Bound: ehvi_ref.value_bound with U = 10.5 units of eps (max(1, z^2 / 2 for z < 0) + |log h|) for every log h - what
tests/test_gpu_constrained.py holds the device's log h to - against the long-double form of the restatement.  As a condition on
the test itself, every candidate's bound stays <= 1e-10 max(1, |value|): a loose bound cannot hide a failure.
Sizes: M = 1, 255 (one partial workgroup), 256, 257 (two), 262,147 (1024 x 256 + 3: the grid-stride loop takes a second trip in
which the last workgroup that has one is ragged); P = 0, 1, 2, 7 (spacing 1e-3), 128.  The large size repeats the 601 distinct
candidates of the small ones (601 is prime: a candidate meets every lane), so one long-double reference per P serves every size."""
import os

import numpy as np
import pytest
import torch  # noqa: F401  (before the host-pointer binding initialises HIP)

pytestmark = pytest.mark.gpu

import ehvi_ref as R  # noqa: E402
import matern_ref as MR  # noqa: E402
from bayesian_optimisation_amd import DeviceGP, EhviResult, PointSelector, PointSelectorHost  # noqa: E402
from bayesian_optimisation_amd import host_binding as H  # noqa: E402

DEV = "cuda:0"
EPS = np.finfo(np.float64).eps
HERE = os.path.dirname(os.path.abspath(__file__))
GOLD = np.load(os.path.join(HERE, "golden", "ehvi_cases.npz"))
U = 10.5
REL_CAP = 1e-10
SIZES = [1, 255, 256, 257, 262147]
COUNTS = [0, 1, 2, 7, 128]
OFFSETS = [0, (1 << 33) + 5]
K = 601
_GP, _FRONTS, _BASE, _WANT = [], {}, [], {}


def _gp():
    if not _GP:
        _GP.append(DeviceGP(device=DEV))   # the kernel works on dense arrays: no factorisation
    return _GP[0]


def _record(r):
    return r.best_val, r.best_idx, r.nan_count


def _front(P):
    """(front [P x 2], ref): spacing 1e-3 .. 2e-3 at P = 7, 0.02 .. 0.04 at P = 128, 0.5 .. 1 below."""
    if P not in _FRONTS:
        rng = np.random.default_rng(7000 + P)
        step = {7: 1.0e-3, 128: 0.02}.get(P, 0.5)
        a, c = np.cumsum(step * (1.0 + rng.random(P))), -np.cumsum(step * (1.0 + rng.random(P)))
        _FRONTS[P] = (np.stack([a, c], axis=1).reshape(-1, 2), (float(a[-1] if P else 0.0) + 0.4, 0.3))
    return _FRONTS[P]


def _base():
    """The K distinct candidates: means up to 4 around the fronts, sigma in [0.05, 2]; 1 - 3: sigma = 0 in objective 1, 2, both,
    inside the box; 4: sigma = 0 beyond r (the value is -inf); 5 - 24: 40 to 60 sigma beyond r in both objectives."""
    if not _BASE:
        rng = np.random.default_rng(99)
        mu1, mu2 = rng.uniform(-4.0, 7.0, K), rng.uniform(-6.0, 4.0, K)
        s1, s2 = (np.exp(rng.uniform(np.log(0.05), np.log(2.0), K)) for _ in range(2))
        s1[[1, 3, 4]], s2[[2, 3]] = 0.0, 0.0
        mu1[1:4], mu2[1:4], mu1[4] = -0.25, -0.4, 9.0
        mu1[5:25], mu2[5:25] = 7.0 + rng.uniform(40.0, 60.0, 20) * s1[5:25], 0.3 + rng.uniform(40.0, 60.0, 20) * s2[5:25]
        _BASE.append((mu1, s1, mu2, s2))
    return _BASE[0]


def _want(P):
    """(value_ld, bound) over the K base candidates: once per P."""
    if P not in _WANT:
        F, ref = _front(P)
        T = R.terms_ld(*_base(), F, ref)
        _WANT[P] = (R.value_ld(*_base(), F, ref, T), R.value_bound(*_base(), F, ref, U, T))
    return _WANT[P]


def _held(got, want, bound, what):
    """got against want within bound; -inf and NaN exactly where want has them; the bound itself within REL_CAP."""
    fin = np.isfinite(want)
    assert np.array_equal(got[~fin], want[~fin], equal_nan=True), what
    assert np.all(bound[fin] <= REL_CAP * np.maximum(1.0, np.abs(want[fin]))), what
    worst = float(np.max(np.abs(got[fin] - want[fin]) / bound[fin])) if fin.any() else 0.0
    print(f"{what}: worst |dvalue| = {worst:.3f} of its bound over {int(fin.sum())} candidates, worst bound "
          f"{float(np.max(bound[fin] / np.maximum(1.0, np.abs(want[fin])))) if fin.any() else 0.0:.2e} max(1, |value|); "
          f"{int((~fin).sum())} at -inf / NaN")
    assert worst <= 1.0, what


# ---- the 60-digit fixture ---------------------------------------------------------------------------------------------------------
def test_the_fixture_cases_match_60_digit_values():
    gp = _gp()
    for k in range(GOLD["ref"].shape[0]):
        F, ref, sel = GOLD[f"front_{k}"], tuple(GOLD["ref"][k]), GOLD["fid"] == k
        a = [GOLD[n][sel] for n in ("mu1", "s1", "mu2", "s2")]
        r = gp.ehvi_on_posterior(*a, F, ref)
        _held(r.value.cpu().numpy(), GOLD["want"][sel], R.value_bound(*a, F, ref, U), f"fixture front {k} (P = {F.shape[0]})")
        assert r.nan_count == 0 and r.best_idx == R.first_argmax(r.value.cpu().numpy())[1]


# ---- sizes and front sizes --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("P", COUNTS)
@pytest.mark.parametrize("M", SIZES)
def test_values_and_record_match_the_restatement(M, P):
    gp = _gp()
    F, ref = _front(P)
    k = np.arange(M) % K
    dev = [gp._dev(a[k]) for a in _base()]
    want, bound = (a[k] for a in _want(P))
    r = gp.ehvi_on_posterior(*dev, F, ref, idx_offset=OFFSETS[1])
    assert isinstance(r, EhviResult) and r.ref == ref and np.array_equal(r.front, F)
    val = r.value.cpu().numpy()
    assert val.shape == (M,) and r.nan_count == 0 and not np.isnan(val).any()
    _held(val, want, bound, f"M = {M}, P = {P}")
    if M > 24:
        assert np.all(np.isfinite(val[1:4])) and val[4] == -np.inf and np.all(np.isfinite(val[5:25]))
    # the record is the dense output's own first arg-max, moved by idx_offset; where the restatement decides, its choice
    best, first, _ = R.first_argmax(val)
    assert _record(r) == (best, OFFSETS[1] + first, 0) and first < K
    order = np.argsort(-want[:K], kind="stable")
    if M > 1 and want[order[0]] - want[order[1]] > bound[order[0]] + bound[order[1]]:
        assert first == order[0]
    # the same bits from a second call; the same record without the dense output and at another offset
    q = gp.ehvi_on_posterior(*dev, F, ref, idx_offset=OFFSETS[1])
    assert q.value.cpu().numpy().tobytes() == val.tobytes() and _record(q) == _record(r)
    p = gp.ehvi_on_posterior(*dev, F, ref, idx_offset=OFFSETS[0], dense=False)
    assert p.value is None and _record(p) == (best, first, 0)


def test_host_entry_is_the_device_path():
    a = [v[:257] for v in _base()]
    for P in (0, 7, 128):
        F, ref = _front(P)
        d = _gp().ehvi_on_posterior(*a, F, ref)
        h = H.ehvi_acq(*a, F, ref)
        assert h["value"].tobytes() == d.value.cpu().numpy().tobytes()
        assert (h["best_val"], h["best_idx"], h["nan_count"]) == _record(d)
        n = H.ehvi_acq(*a, F, ref, dense=False)
        assert n["value"] is None and (n["best_val"], n["best_idx"], n["nan_count"]) == _record(d)


# ---- edges --------------------------------------------------------------------------------------------------------------------------
def test_a_nan_in_any_array_is_counted_once_and_never_chosen():
    M = 300
    gp = _gp()
    F, ref = _front(2)
    base = [v[25: 25 + M].copy() for v in _base()]
    clean = gp.ehvi_on_posterior(*base, F, ref, idx_offset=7)
    assert clean.nan_count == 0
    j = clean.best_idx - 7                                    # the NaN goes where the best candidate is
    for a in range(4):
        arrays = [x.copy() for x in base]
        arrays[a][j] = np.nan
        r = gp.ehvi_on_posterior(*arrays, F, ref, idx_offset=7)
        v = r.value.cpu().numpy()
        assert r.nan_count == 1 and np.isnan(v[j]) and np.isnan(v).sum() == 1, a
        assert r.best_idx != 7 + j and 7 <= r.best_idx < 7 + M and r.best_val == np.nanmax(v)
    # NaN in all four arrays of ONE candidate: still one; NaN beside sigma = 0: NaN, not the certain answer
    arrays = [x.copy() for x in base]
    for a in range(4):
        arrays[a][j] = np.nan
    p, q = [i for i in (10, 11, 12) if i != j][:2]
    arrays[1][p], arrays[0][p] = 0.0, np.nan                  # sigma1 = 0, mu1 NaN
    arrays[3][q], arrays[2][q] = 0.0, np.nan                  # sigma2 = 0, mu2 NaN
    r = gp.ehvi_on_posterior(*arrays, F, ref)
    assert r.nan_count == 3 and np.flatnonzero(np.isnan(r.value.cpu().numpy())).tolist() == sorted([j, p, q])
    e = gp.ehvi_on_posterior(np.full(M, np.nan), np.ones(M), np.zeros(M), np.ones(M), F, ref, idx_offset=7)
    assert e.nan_count == M and not 7 <= e.best_idx < 7 + M   # every candidate NaN: the empty record


def test_zero_sigma_is_the_hypervolume_gain_of_the_mean():
    """sigma1 = sigma2 = 0: exp(value) is hypervolume(front + mu) - hypervolume(front); one of them 0: the strip sum with
    max(a - mu, 0) in that objective (the restatement)."""
    rng = np.random.default_rng(3)
    M = 200
    F, ref = _front(7)
    mu1, mu2 = rng.uniform(-0.02, 0.03, M), rng.uniform(-0.03, 0.02, M)   # around the staircase of the front
    s = np.exp(rng.uniform(np.log(0.05), np.log(2.0), M))
    zero = np.zeros(M)
    gain = R.improvement(mu1, mu2, F, ref)
    want = R.value_ld(mu1, zero, mu2, zero, F, ref)
    ok = gain > 0.0
    # (the restatement IS the gain: tests/test_ehvi_ref_cpu.py; here only that the two agree on where it is 0)
    assert np.array_equal(want == -np.inf, ~ok) and ok.sum() > 50 and (~ok).sum() > 10
    box = R.improvement(mu1, mu2, F[:0], ref)                 # the whole rectangle [mu, r]: what the strips' edges are cut from
    assert np.all(np.abs(np.exp(want[ok]) - gain[ok]) <= 16.0 * EPS * gain[ok] * (1.0 + np.abs(want[ok])) + EPS * box[ok])
    for a in ((mu1, zero, mu2, zero), (mu1, zero, mu2, s), (mu1, s, mu2, zero)):
        v = _gp().ehvi_on_posterior(*a, F, ref).value.cpu().numpy()
        T = R.terms_ld(*a, F, ref)
        _held(v, R.value_ld(*a, F, ref, T), R.value_bound(*a, F, ref, U, T), "one sigma zero")


@pytest.mark.parametrize("M", [257, 262147])
def test_all_minus_inf_returns_the_lowest_index(M):
    gp = _gp()
    F, ref = _front(2)
    for off in OFFSETS:
        r = gp.ehvi_on_posterior(np.full(M, ref[0] + 1.0), np.zeros(M), np.zeros(M), np.ones(M), F, ref, idx_offset=off)
        assert _record(r) == (-np.inf, off, 0) and torch.all(r.value == -np.inf).item()
    r = gp.ehvi_on_posterior(np.zeros(M), np.ones(M), np.full(M, ref[1]), np.zeros(M), F, ref, dense=False)   # ON r2: no gain
    assert _record(r) == (-np.inf, 0, 0)


@pytest.mark.parametrize("P", [0, 7])
def test_the_first_of_planted_exact_ties_wins(P):
    M = 262147
    F, ref = _front(P)
    mu1, s1, mu2, s2 = np.full(M, 3.0), np.full(M, 0.7), np.full(M, 2.0), np.full(M, 0.3)
    top = [70, 300, 65536 + 9, M - 1]                         # another wave, another workgroup, the second trip of the loop
    mu1[top], mu2[top] = 0.5, -0.5
    r = _gp().ehvi_on_posterior(mu1, s1, mu2, s2, F, ref, idx_offset=OFFSETS[1])
    v = r.value.cpu().numpy()
    assert np.unique(v).size == 2 and np.flatnonzero(v == v.max()).tolist() == top
    assert _record(r) == (v.max(), OFFSETS[1] + 70, 0)


@pytest.mark.parametrize("P", [0, 7, 128])
def test_the_plain_sum_underflows_and_the_logarithm_does_not(P):
    """What the log form exists for: every candidate at least 40 standard deviations from improving in BOTH objectives.  The plain
    fp64 strip sum is exactly 0 for every candidate, so a plain-space implementation sees M equal values and returns candidate
    0; in log space the unique best candidate is found, with a finite value."""
    M, winner = 1000, 613
    rng = np.random.default_rng(8)
    F, ref = _front(P)
    s1, s2 = (np.exp(rng.uniform(np.log(0.1), np.log(1.0), M)) for _ in range(2))
    k1, k2 = rng.uniform(43.0, 60.0, M), rng.uniform(43.0, 60.0, M)
    k1[winner] = k2[winner] = 40.5
    s1[winner] = s2[winner] = 0.5
    mu1, mu2 = ref[0] + k1 * s1, ref[1] + k2 * s2
    assert ((ref[0] - mu1) / s1).max() <= -40.0 and ((ref[1] - mu2) / s2).max() <= -40.0
    assert np.all(R.plain(mu1, s1, mu2, s2, F, ref) == 0.0)
    r = _gp().ehvi_on_posterior(mu1, s1, mu2, s2, F, ref)
    v = r.value.cpu().numpy()
    T = R.terms_ld(mu1, s1, mu2, s2, F, ref)
    want = R.value_ld(mu1, s1, mu2, s2, F, ref, T)
    assert np.all(np.isfinite(v)) and v.max() < -1600.0 and np.unique(v).size > M // 2
    assert r.best_idx == winner == R.first_argmax(want)[1] and r.best_val == v[winner] and r.nan_count == 0
    assert np.sort(want)[-1] - np.sort(want)[-2] > 1.0        # the best is unique, by far more than any rounding
    _held(v, want, R.value_bound(mu1, s1, mu2, s2, F, ref, U, T), f"underflow, P = {P}")


# ---- end to end ---------------------------------------------------------------------------------------------------------------------
FD = [24, 25]
AXES = [np.geomspace(0.05, 5.0, 16)] * 2
KINDS = {"se-preset": dict(kernel="se"), "matern52-hyper": dict(kernel="matern52", ard="hyper")}
MIXED = ("se-preset", "matern52-hyper")
_RUNS = {}


def _data():
    """N = 40 uniform points in [0, 1]^2 and TWO draws of a GP with length scales (0.3, 0.6) at them, each with noise 0.05; a
    24 x 25 grid of candidates."""
    rng = np.random.default_rng(0)
    X = rng.uniform(0.0, 1.0, (40, 2))
    Xn = X / np.array([0.3, 0.6])
    sq = np.sum(Xn * Xn, axis=1)
    L = np.linalg.cholesky(np.exp(-0.5 * np.maximum(sq[:, None] + sq[None, :] - 2.0 * Xn @ Xn.T, 0.0)) + 1e-8 * np.eye(40))
    f = [L @ rng.standard_normal(40) + 0.05 * rng.standard_normal(40) for _ in range(2)]
    a, b = (np.arange(24) + 0.5) / 24, (np.arange(25) + 0.5) / 25
    return X, f, np.stack(np.meshgrid(a, b, indexing="ij"), -1).reshape(-1, 2)


def _values(kinds, affine=None):
    """The two objectives' observations: a frozen model ("se-preset": zero mean, unit signal variance) gets its draw as it is, a
    fitted one gets 40 + 7 f (objective 1) or 3 + 2 f (objective 2); affine = (a, b): every FITTED objective holds a + b y."""
    f = _data()[1]
    ys = []
    for k, kind in enumerate(kinds):
        y = f[k] if kind == "se-preset" else ((40.0, 3.0)[k] + (7.0, 2.0)[k] * f[k])
        ys.append(y if affine is None or kind == "se-preset" else affine[0] + affine[1] * y)
    return ys


def _pair(cls, kinds=MIXED, affine=None, **extra):
    """(objective 1, objective 2) selector objects of the given kinds, updated once."""
    key = (cls.__name__, kinds, affine, tuple(sorted(extra.items())))
    if key not in _RUNS:
        X, _, Xs = _data()
        out = []
        for kind, y in zip(kinds, _values(kinds, affine)):
            ps = cls(**KINDS[kind], **extra)
            ps.name, ps.iteration = "T", 0
            ps.measured_pts, ps.measured_vals = X, y
            ps.feature_domain, ps.predicted_pts, ps.length_scales = FD, Xs, AXES
            if kind == "se-preset":
                ps.set_kernel_params([0.3, 0.6])
            ps.update_surrogate()
            out.append(ps)
        _RUNS[key] = out
    return _RUNS[key]


def _to_model(ps, v):
    m = ps._model
    return (np.asarray(v, dtype=np.float64) - m.y_mean) / m.y_scale if m.fitted else np.asarray(v, dtype=np.float64)


def _shift(pair):
    return sum(float(np.log(ps._model.y_scale)) if ps._model.fitted else 0.0 for ps in pair)


def _model_inputs(pair, posterior, F, ref):
    """(mu1, sigma1, mu2, sigma2, front, ref) in the units of the MODELS, from posterior(selector) -> (mu, sigma)."""
    (m1, s1), (m2, s2) = posterior(pair[0]), posterior(pair[1])
    F_m = np.stack([_to_model(pair[0], F[:, 0]), _to_model(pair[1], F[:, 1])], axis=1)
    return m1, s1, m2, s2, F_m, (float(_to_model(pair[0], ref[0])), float(_to_model(pair[1], ref[1])))


def _device_posterior(ps):
    return ps._mu_dev.cpu().numpy(), ps._sigma_dev.cpu().numpy()


def _public_posterior(ps):   # from the public attributes, in the units of the model
    m = ps._model
    if not m.fitted:
        return np.asarray(ps.mean_func, dtype=np.float64).ravel(), np.asarray(ps.cov_func, dtype=np.float64).ravel()
    return (np.asarray(ps.mean_func).ravel() - m.y_mean) / m.y_scale, np.asarray(ps.cov_func).ravel() / m.y_scale


def _reference_posterior(ps):
    """The CPU reference posterior of the model the selector holds (tests/matern_ref.py: Cholesky route in NumPy)."""
    m = ps._model
    X, Xs = np.asarray(ps.measured_pts, dtype=np.float64), np.asarray(ps.predicted_pts, dtype=np.float64)
    return MR.posterior(X, _to_model(ps, ps.measured_vals), Xs, np.asarray(ps.kernel_params, dtype=np.float64).reshape(-1),
                        m.kernel, m.jitter1, m.jitter2)


def _observed(pair):
    Y = np.stack([np.asarray(ps.measured_vals, dtype=np.float64) for ps in pair], axis=1)
    ref = R.nadir(Y)
    return Y, R.pareto_front(Y, ref), ref


def _held_in_y(acq, args, shift, what):
    T = R.terms_ld(*args)
    want = R.value_ld(*args, T)
    bound = R.value_bound(*args, U, T) + 2.0 * EPS * (np.abs(want) + abs(shift))
    _held(acq.ravel() - shift, want, bound, what)
    return want


@pytest.mark.parametrize("kinds", [MIXED, MIXED[::-1]])
def test_selector_end_to_end(kinds):
    pair = _pair(PointSelector, kinds)
    obj, other = pair
    Y, F, ref = _observed(pair)
    idx = obj.expected_hypervolume_improvement(other)
    acq = obj.acq_func_eval.copy()
    flat = int(np.ravel_multi_index(tuple(idx), FD))
    assert acq.shape == tuple(FD) and np.array_equal(idx, np.unravel_index(int(np.argmax(acq)), FD))
    assert np.array_equal(obj.pareto_front, F) and obj.reference_point == ref and 2 <= F.shape[0] <= 40
    assert abs(obj.hypervolume - R.hypervolume(Y, ref)) <= 8.0 * EPS * F.shape[0] * R.hypervolume(Y, ref) and obj.hypervolume > 0.0
    # the dense values: the restatement fed the device's own posteriors (the posterior itself is pinned elsewhere)
    shift = _shift(pair)
    _held_in_y(acq, _model_inputs(pair, _device_posterior, F, ref), shift, f"{kinds}: log EHVI on the device's posteriors")
    print(f"{kinds}: P = {F.shape[0]}, ref {ref}, log EHVI in [{acq.min():.4g}, {acq.max():.4g}], index {idx.tolist()}")
    # the selected point: the restatement's on the CPU reference posterior, whose top two are apart
    cpu = R.value_ld(*_model_inputs(pair, _reference_posterior, F, ref))
    top = np.sort(cpu)[-2:]
    print(f"{kinds}: top-two gap of the reference {top[1] - top[0]:.3e}")
    assert top[1] - top[0] > 1e-6
    assert flat == R.first_argmax(cpu)[1]
    # DeviceGP.select_ehvi on the selectors' own surrogates, in the units of the models: the same point
    args = _model_inputs(pair, _device_posterior, F, ref)
    r = obj._gp.select_ehvi(obj._cand[0], other._gp, front=args[4], ref=args[5], dense=True)
    assert r.best_idx == flat and r.nan_count == 0
    assert np.all(np.abs(r.value.cpu().numpy() - (acq.ravel() - shift)) <= 4.0 * EPS * (np.abs(acq.ravel()) + abs(shift)))
    with pytest.raises(ValueError, match="must be a DeviceGP"):
        obj._gp.select_ehvi(obj._cand[0], other)               # (a selector object is not its surrogate)
    # an explicit front and reference point are the observed ones; the call is not served from a cache
    assert np.array_equal(obj.expected_hypervolume_improvement(other, ref=ref, front=F), idx)
    assert obj.acq_func_eval.tobytes() == acq.tobytes()
    wide = (ref[0] + 1.0, ref[1] + 1.0)
    obj.expected_hypervolume_improvement(other, ref=wide)
    grown = obj.acq_func_eval - acq                           # (every bound of this file is <= REL_CAP max(1, |value|))
    assert np.all(grown >= -2.0 * REL_CAP * np.maximum(1.0, np.abs(acq))) and grown.max() > 1e-3
    assert obj.reference_point == wide and obj.hypervolume > R.hypervolume(Y, ref)
    # no front and r far away: the sum of the two log expected improvements against r (one strip, no subtraction)
    far = (float(Y[:, 0].max()) + 5.0, float(Y[:, 1].max()) + 5.0)
    obj.expected_hypervolume_improvement(other, ref=far, front=np.empty((0, 2)))
    box = obj.acq_func_eval.copy()
    assert obj.pareto_front.shape == (0, 2) and obj.hypervolume == 0.0
    obj.constrained_expected_improvement([], [], f_best=far[0])
    other.constrained_expected_improvement([], [], f_best=far[1])
    e1, e2 = obj.acq_func_eval, other.acq_func_eval
    assert np.all(np.abs(box - (e1 + e2)) <= 4.0 * EPS * (np.abs(e1) + np.abs(e2) + abs(shift) + 1.0))
    # mismatches are refused: other measured points under the observed front (explicit ones still work), other candidates
    keep = other.measured_pts
    try:
        other.measured_pts = (np.asarray(keep, dtype=np.float64) + 1e-9).tolist()
        with pytest.raises(ValueError, match="same measured points"):
            obj.expected_hypervolume_improvement(other)
        with pytest.raises(ValueError, match="same measured points"):
            obj.expected_hypervolume_improvement(other, front=F)         # (ref="nadir" needs the pairs too)
        assert np.array_equal(obj.expected_hypervolume_improvement(other, ref=ref, front=F), idx)
    finally:
        other.measured_pts = keep
    keep = other.predicted_pts
    try:
        other.predicted_pts = np.asarray(keep) + 1e-12
        with pytest.raises(ValueError, match="same predicted_pts"):
            obj.expected_hypervolume_improvement(other)
    finally:
        other.predicted_pts = keep
    with pytest.raises(ValueError, match="must be a PointSelector"):
        obj.expected_hypervolume_improvement(_pair(PointSelectorHost, kinds)[1])
    assert obj.lower_confidence_bound().shape == (2,)         # the update's own acquisition is still served


@pytest.mark.parametrize("kinds", [MIXED, MIXED[::-1]])
def test_values_shift_by_log_b_under_an_affine_map_of_an_objective(kinds):
    """ard="hyper" fits mean and scale: the fitted objective given as a + b y, with the observed front and the nadir point moving
    with it, is the same problem, and log EHVI - the logarithm of an area - moves by log b.  The two fits follow the same path up
    to rounding (the profiled likelihood is invariant), so the posteriors in the units of the models agree to about 1e-9; the
    value moves by at most (|z| + 2) times the change of an argument per factor, |z| <= 40 here: 1e-6 relative."""
    a, b = -250.0, 40.0
    p1, p2 = _pair(PointSelector, kinds), _pair(PointSelector, kinds, affine=(a, b))
    i1 = p1[0].expected_hypervolume_improvement(p1[1])
    v1, hv1 = p1[0].acq_func_eval.copy(), p1[0].hypervolume
    i2 = p2[0].expected_hypervolume_improvement(p2[1])
    v2, hv2 = p2[0].acq_func_eval, p2[0].hypervolume
    print(f"affine map of the fitted objective {kinds}: |dvalue - log b| {np.max(np.abs(v2 - v1 - np.log(b))):.3e}")
    assert np.array_equal(i1, i2) and p1[0].pareto_front.shape == p2[0].pareto_front.shape
    assert abs(hv2 - b * hv1) <= 1e-9 * b * hv1
    assert np.all(np.abs(v2 - v1 - np.log(b)) <= 1e-6 * (1.0 + np.abs(v1)))


@pytest.mark.parametrize("kinds", [("se-preset", "se-preset"), MIXED])
def test_host_and_device_classes_agree(kinds):
    """The host class runs the same kernel on mean_func / cov_func taken back to the units of the model.  Two frozen models map
    nothing: the same bits.  With a fitted objective its dense values are held to the restatement fed ITS OWN inputs (recomputed
    here from the public mean_func / cov_func), the selected point is the device class's, and every standardised argument and log
    sigma lies within ARG_CAP = 1e-9 of the device class's (the two classes' fits are pinned to each other at 1e-10 relative and
    their mean_func at 1e-9 by tests/test_gpu_matern.py; a wrong conversion moves the arguments by order 1)."""
    ARG_CAP = 1e-9
    dev, hst = _pair(PointSelector, kinds), _pair(PointSelectorHost, kinds)
    idx = dev[0].expected_hypervolume_improvement(dev[1])
    v = dev[0].acq_func_eval.copy()
    idh = hst[0].expected_hypervolume_improvement(hst[1])
    vh = hst[0].acq_func_eval
    assert np.array_equal(idx, idh) and np.array_equal(hst[0].pareto_front, dev[0].pareto_front)
    assert hst[0].reference_point == dev[0].reference_point and hst[0].hypervolume == dev[0].hypervolume
    if kinds == ("se-preset", "se-preset"):
        assert all(np.array_equal(h.mean_func, d.mean_func) and np.array_equal(h.cov_func, d.cov_func) for h, d in zip(hst, dev))
        assert vh.tobytes() == v.tobytes()
        return
    _, F, ref = _observed(dev)
    ah, ad = _model_inputs(hst, _public_posterior, F, ref), _model_inputs(dev, _device_posterior, F, ref)
    _held_in_y(vh, ah, _shift(hst), "host class against the restatement on its own inputs")

    def arguments(a):
        m1, s1, m2, s2, F_m, r_m = a
        e, c = R.strips(F_m, r_m)
        return np.concatenate([((e[:, None] - m1) / s1).ravel(), ((c[:, None] - m2) / s2).ravel(), np.log(s1), np.log(s2)])

    moved = float(np.abs(arguments(ah) - arguments(ad)).max())
    print(f"{kinds}: largest change of an argument host - device {moved:.2e} (cap {ARG_CAP:.0e}); |dlog EHVI| {np.abs(vh - v).max():.2e}")
    assert moved <= ARG_CAP and abs(_shift(hst) - _shift(dev)) <= ARG_CAP


# ---- candidates sharded over two ranks on one GPU -------------------------------------------------------------------------------
def _sharded_worker(rank, world, port, q):
    import torch.distributed as dist

    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        pair = _pair(PointSelector, ("se-preset", "se-preset"), device=DEV)
        idx = pair[0].expected_hypervolume_improvement(pair[1])
        q.put((rank, idx.tolist(), pair[0].acq_func_eval.tobytes(), pair[0]._lo_hi))
    finally:
        dist.destroy_process_group()


def test_two_ranks_sharing_the_gpu_return_the_single_process_answer():
    import socket

    import torch.multiprocessing as mp

    pair = _pair(PointSelector, ("se-preset", "se-preset"))
    idx = pair[0].expected_hypervolume_improvement(pair[1])
    acq = pair[0].acq_func_eval.tobytes()
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    port = s.getsockname()[1]
    s.close()
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    procs = [ctx.Process(target=_sharded_worker, args=(r, 2, port, q)) for r in range(2)]
    for p in procs:
        p.start()
    res = [q.get(timeout=300) for _ in procs]
    for p in procs:
        p.join(120)
        assert p.exitcode == 0
    assert sorted(r[3] for r in res) == [(0, 300), (300, 600)]
    for _, i, a, _ in res:
        assert i == idx.tolist() and a == acq
