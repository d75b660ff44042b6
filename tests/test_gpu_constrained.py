"""The constrained acquisitions in log space on the GPU (csrc/constrained.hip; DeviceGP.constrained_on_posterior /
select_constrained, the three methods of PointSelector and PointSelectorHost, the host entry) against tests/constrained_ref.py, the
NumPy / SciPy restatement, whose own accuracy tests/test_constrained_ref_cpu.py pins against 60-digit values.

Bounds, in units of eps (max(1, a^2 / 2 for a < 0) + |term|) of a term with standardised argument a:
    log Phi   8 units: what tests/test_gpu_mes.py holds mes_log_ndtr to on this hardware
    log h     FOUR TIMES the worst value the fp64 restatement shows against tests/golden/cons_terms.npz on the CPU, computed when
              this module is imported (2.63 with SciPy 1.15: a bound of 10.5).  The factor covers the device's erfcx / log1p / log
              differing from SciPy's by a few ulp each.
    a value   the bounds of its terms added, 2 eps |log sigma|, and max(C, 1) eps sum |terms| for the additions
              (constrained_ref.value_bound), against the long-double form of the restatement (within 0.45 units of the fixtures).
Measured on an MI355X (the test prints them): see DESIGN.md 4o.
Sizes: M = 1, 255 (one partial workgroup), 256, 257 (two), 262,147 (1024 x 256 + 3: the grid-stride loop takes a second trip in
which the last workgroup that has one is ragged)."""
import os

import numpy as np
import pytest
import torch  # noqa: F401  (before the host-pointer binding initialises HIP)

pytestmark = pytest.mark.gpu

import constrained_ref as R  # noqa: E402
import matern_ref as MR  # noqa: E402
from bayesian_optimisation_amd import ConstrainedResult, DeviceGP, PointSelector, PointSelectorHost  # noqa: E402
from bayesian_optimisation_amd import host_binding as H  # noqa: E402

DEV = "cuda:0"
EPS = np.finfo(np.float64).eps
HERE = os.path.dirname(os.path.abspath(__file__))
GOLD = np.load(os.path.join(HERE, "golden", "cons_terms.npz"))
MES_GOLD = np.load(os.path.join(HERE, "golden", "mes_terms.npz"))
UNITS_NDTR = 8.0
UNITS_H = 4.0 * max(R.fixture_worst(R.log_h, GOLD["z"], GOLD["log_h"]))
SIZES = [1, 255, 256, 257, 262147]
OFFSETS = [0, (1 << 33) + 5]
BASES = {"none": R.BASE_NONE, "ei": R.BASE_EI, "pi": R.BASE_PI}
F_BEST, XI = 0.0, 0.01
_GP, _CASES = [], {}


def _gp():
    if not _GP:
        _GP.append(DeviceGP(device=DEV))   # the kernel works on dense arrays: no factorisation
    return _GP[0]


def _record(r):
    return r.best_val, r.best_idx, r.nan_count


# ---- the terms at the 60-digit fixtures -------------------------------------------------------------------------------------------
def test_the_terms_match_60_digit_values():
    """sigma = 1, f_best = xi = 0 and mu = -z make the standardised argument z itself, and log sigma = 0 adds nothing: the value
    IS the term.  z and gamma: 2,001 points on [-40, 40] and -1e2 ... -1e6 / -1e2, -1e3, -1e4."""
    gp = _gp()
    z, want = GOLD["z"], GOLD["log_h"]
    got = gp.constrained_on_posterior(-z, np.ones_like(z), None, None, [], base="ei", f_best=0.0, xi=0.0).value.cpu().numpy()
    err = np.abs(got - want) / (EPS * R.term_scale(z, want))
    br = R.log_h_branch(z)
    per = [float(err[br == b].max()) for b in range(4)]
    print(f"log h on the device: worst error per branch (z >= 0, [-1, 0), (-1e3, -1), <= -1e3) "
          + ", ".join(f"{w:.2f}" for w in per) + f" units of eps (max(1, z^2/2 for z<0) + |log h|); bound {UNITS_H:.2f} = 4 x the "
          f"fp64 restatement's {UNITS_H / 4:.2f}")
    assert 8.0 <= UNITS_H <= 4.0 * 2.84 and max(per) <= UNITS_H
    g, wantp = MES_GOLD["gamma"], MES_GOLD["log_ndtr"]
    one = np.ones_like(g)
    as_base = gp.constrained_on_posterior(-g, one, None, None, [], base="pi", f_best=0.0, xi=0.0).value.cpu().numpy()
    as_cons = gp.constrained_on_posterior(None, None, -g[None, :], one[None, :], [0.0], base="none")
    errp = np.abs(as_base - wantp) / (EPS * R.term_scale(g, wantp))
    print(f"log Phi on the device: worst error {errp.max():.2f} units (bound {UNITS_NDTR:.0f}), at gamma = {g[errp.argmax()]:.4g}")
    assert errp.max() <= UNITS_NDTR
    assert as_cons.value.cpu().numpy().tobytes() == as_base.tobytes() == as_cons.log_feasibility.cpu().numpy().tobytes()


# ---- sizes, constraint counts, bases ------------------------------------------------------------------------------------------------
def _case(M):
    """(mu, sigma, cons_mu [8 x M], cons_sigma [8 x M], upper [8]) once per size: means in [-2, 2], sigma in [0.05, 2], so that z
    and every gamma cover [-40, 40] and beyond.  From 17 candidates on: sigma = 0 on each side of its rule for the objective
    (1: imp > 0, 2: imp < 0) and for constraint 0 (3: within the limit, 4: beyond it, 5: ON it), and two exact copies of one
    candidate, M // 2 and M // 2 + 3 (equal values whatever the base)."""
    if M not in _CASES:
        rng = np.random.default_rng(4000 + M)
        mu, sigma = rng.uniform(-2.0, 2.0, M), np.exp(rng.uniform(np.log(0.05), np.log(2.0), M))
        cm, cs = rng.uniform(-2.0, 2.0, (8, M)), np.exp(rng.uniform(np.log(0.05), np.log(2.0), (8, M)))
        u = rng.uniform(-0.5, 0.5, 8)
        if M > 16:
            sigma[1], mu[1], sigma[2], mu[2] = 0.0, -0.5, 0.0, 0.5
            cs[0, 3:6], cm[0, 3:6] = 0.0, [u[0] - 0.25, u[0] + 0.25, u[0]]
            w = M // 2
            mu[w + 3], sigma[w + 3], cm[:, w + 3], cs[:, w + 3] = mu[w], sigma[w], cm[:, w], cs[:, w]
        _CASES[M] = (mu, sigma, cm, cs, u)
    return _CASES[M]


def _checked(M):
    """The candidates whose dense values are compared with the long-double restatement: all of them, or at the large size (where
    the restatement would take seconds) both ends and a stride through the rest."""
    return np.arange(M) if M < 5000 else np.unique(np.concatenate([np.arange(700), np.arange(M - 700, M), np.arange(0, M, 431)]))


@pytest.mark.parametrize("base", ["none", "ei", "pi"])
@pytest.mark.parametrize("C", [0, 1, 3, 8])
@pytest.mark.parametrize("M", SIZES)
def test_values_and_record_match_the_restatement(M, C, base):
    if base == "none" and C == 0:
        with pytest.raises(ValueError):
            _gp().constrained_on_posterior(None, None, None, None, [], base="none")
        return
    mu, sigma, cm, cs, u = _case(M)
    cm, cs, u = cm[:C], cs[:C], u[:C]
    gp = _gp()
    mud, sgd, cmd, csd = gp._dev(mu), gp._dev(sigma), gp._dev(cm), gp._dev(cs)
    kw = dict(base=base, f_best=F_BEST, xi=XI)
    r = gp.constrained_on_posterior(mud, sgd, cmd, csd, u, idx_offset=OFFSETS[1], **kw)
    assert isinstance(r, ConstrainedResult) and r.base == base
    val, feas = r.value.cpu().numpy(), r.log_feasibility.cpu().numpy()
    k = _checked(M)
    sub = (mu[k], sigma[k], cm[:, k], cs[:, k], u, BASES[base], F_BEST, XI)
    want, want_feas = R.value(*sub)
    bound = R.value_bound(*sub, UNITS_NDTR, UNITS_H)
    fin = np.isfinite(want)
    with np.errstate(invalid="ignore"):
        worst = float(np.max(np.abs(val[k][fin] - want[fin]) / bound[fin]))
    print(f"M = {M}, C = {C}, base {base}: worst |dvalue| = {worst:.3f} of its bound over {int(fin.sum())} candidates; values in "
          f"[{want[fin].min():.4g}, {want[fin].max():.4g}], {int((~fin).sum())} at -inf")
    assert val.shape == feas.shape == (M,) and r.nan_count == 0 and not np.isnan(val).any()
    assert np.array_equal(val[k][~fin], want[~fin]) and np.all(want[~fin] == -np.inf)      # -inf exactly where the rules say
    assert worst <= 1.0
    ffin = np.isfinite(want_feas)
    fbound = R.value_bound(None, None, cm[:, k], cs[:, k], u, R.BASE_NONE, 0.0, 0.0, UNITS_NDTR, UNITS_H) if C else np.ones(k.size)
    assert np.array_equal(feas[k][~ffin], want_feas[~ffin]) and np.all(np.abs(feas[k][ffin] - want_feas[ffin]) <= fbound[ffin])
    assert np.all(feas <= 0.0) and (C > 0 or not feas.any())
    if base == "none":
        assert val.tobytes() == feas.tobytes()                                             # 0 + feas is feas
    if M > 16:
        if base == "ei":
            assert np.isfinite(val[1]) == np.isfinite(feas[1]) and val[2] == -np.inf       # sigma = 0: log(max(imp, 0))
        if base == "pi":
            assert val[1] == feas[1] and val[2] == -np.inf                                 # sigma = 0: 0 where imp > 0
        if C > 0:
            assert feas[4] == -np.inf and val[4] == -np.inf and np.isfinite(feas[[3, 5]]).all()   # sigma_c = 0: mu_c <= u_c or not
        assert val[M // 2] == val[M // 2 + 3]
    # the record is the dense output's own first arg-max, moved by idx_offset; where the restatement decides, its choice
    best, first, _ = R.first_argmax(val)
    assert _record(r) == (best, OFFSETS[1] + first, 0)
    if k.size == M:
        order = np.argsort(-want, kind="stable")
        if M > 1 and want[order[0]] - want[order[1]] > bound[order[0]] + bound[order[1]]:
            assert first == order[0]
    # the same bits from a second call; the same record without the dense outputs, at another offset, and from rows ldc apart
    q = gp.constrained_on_posterior(mud, sgd, cmd, csd, u, idx_offset=OFFSETS[1], **kw)
    assert q.value.cpu().numpy().tobytes() == val.tobytes() and q.log_feasibility.cpu().numpy().tobytes() == feas.tobytes()
    assert _record(q) == _record(r)
    p = gp.constrained_on_posterior(mud, sgd, cmd, csd, u, idx_offset=OFFSETS[0], dense=False, **kw)
    assert p.value is None and p.log_feasibility is None and _record(p) == (best, first, 0)
    if C > 0 and base != "none":
        ldc = M + 37
        wide = np.full((C, ldc), np.nan)                                                   # (a read of the padding would show)
        wide_s = wide.copy()
        wide[:, :M], wide_s[:, :M] = cm, cs
        s = gp.constrained_on_posterior(mud, sgd, wide.reshape(-1), wide_s.reshape(-1), u, idx_offset=OFFSETS[1], ldc=ldc, **kw)
        assert s.value.cpu().numpy().tobytes() == val.tobytes() and _record(s) == _record(r)


def test_host_entry_is_the_device_path():
    mu, sigma, cm, cs, u = _case(257)
    for base, C in (("ei", 3), ("pi", 0), ("none", 8), ("ei", 0)):
        d = _gp().constrained_on_posterior(mu, sigma, cm[:C], cs[:C], u[:C], base=base, f_best=F_BEST, xi=XI)
        h = H.constrained_acq(mu, sigma, cm[:C], cs[:C], u[:C], base=base, f_best=F_BEST, xi=XI)
        assert h["value"].tobytes() == d.value.cpu().numpy().tobytes()
        assert h["log_feasibility"].tobytes() == d.log_feasibility.cpu().numpy().tobytes()
        assert (h["best_val"], h["best_idx"], h["nan_count"]) == _record(d)
        n = H.constrained_acq(mu, sigma, cm[:C], cs[:C], u[:C], base=base, f_best=F_BEST, xi=XI, dense=False)
        assert n["value"] is None and (n["best_val"], n["best_idx"], n["nan_count"]) == _record(d)
    # rows longer than M are refused on both routes unless the device route is told their stride
    wide, wide_s = np.zeros((3, 260)), np.ones((3, 260))
    for call in (_gp().constrained_on_posterior, H.constrained_acq):
        with pytest.raises(ValueError, match="M values per limit"):
            call(mu, sigma, wide, wide_s, u[:3], base="ei", f_best=F_BEST, xi=XI)


# ---- edges --------------------------------------------------------------------------------------------------------------------------
def test_a_nan_in_any_array_is_counted_once_and_never_chosen():
    M, C = 300, 3
    rng = np.random.default_rng(5)
    base_arrays = [rng.uniform(-1.0, 1.0, M), np.full(M, 0.5)] + [rng.uniform(-1.0, 1.0, M) for _ in range(C)] \
        + [np.full(M, 0.5) for _ in range(C)]
    u = np.zeros(C)
    gp = _gp()

    def run(arrays, base):
        mu, sigma = arrays[:2]
        cm, cs = np.stack(arrays[2: 2 + C]), np.stack(arrays[2 + C:])
        return gp.constrained_on_posterior(mu, sigma, cm, cs, u, base=base, f_best=0.0, xi=0.0, idx_offset=7)

    clean = run(base_arrays, "ei")
    assert clean.nan_count == 0
    j = clean.best_idx - 7                                    # the NaN goes where the best candidate is
    for a in range(2 + 2 * C):
        for base in ("ei", "pi", "none"):
            arrays = [x.copy() for x in base_arrays]
            arrays[a][j] = np.nan
            r = run(arrays, base)
            v = r.value.cpu().numpy()
            if base == "none" and a < 2:                      # without a base the objective's posterior is not read
                assert r.nan_count == 0 and not np.isnan(v).any()
                continue
            assert r.nan_count == 1 and np.isnan(v[j]) and np.isnan(v).sum() == 1, (a, base)
            assert r.best_idx != 7 + j and 7 <= r.best_idx < 7 + M and r.best_val == np.nanmax(v)
            assert np.isnan(r.log_feasibility.cpu().numpy()[j]) == (a >= 2)
    # NaN in several arrays of ONE candidate: still one; NaN beside sigma = 0: NaN, not the certain answer
    arrays = [x.copy() for x in base_arrays]
    for a in range(2 + 2 * C):
        arrays[a][j] = np.nan
    p, q = [i for i in (10, 11, 12) if i != j][:2]
    arrays[1][p], arrays[0][p] = 0.0, np.nan                  # sigma = 0, mu NaN
    arrays[2 + C][q], arrays[2][q] = 0.0, np.nan              # sigma_0 = 0, mu_0 NaN
    r = run(arrays, "ei")
    assert r.nan_count == 3 and np.flatnonzero(np.isnan(r.value.cpu().numpy())).tolist() == sorted([j, p, q])
    # every candidate NaN: the empty record
    e = gp.constrained_on_posterior(np.full(M, np.nan), np.ones(M), None, None, [], base="pi", f_best=0.0, idx_offset=7)
    assert e.nan_count == M and not 7 <= e.best_idx < 7 + M


@pytest.mark.parametrize("M", [257, 262147])
def test_all_minus_inf_returns_the_lowest_index(M):
    gp = _gp()
    cm, cs = np.ones((2, M)), np.zeros((2, M))                # certainly beyond the limit 0
    for off in OFFSETS:
        r = gp.constrained_on_posterior(np.zeros(M), np.ones(M), cm, cs, [0.0, 0.0], base="ei", f_best=0.0, idx_offset=off)
        assert _record(r) == (-np.inf, off, 0) and torch.all(r.value == -np.inf).item()
    r = gp.constrained_on_posterior(np.ones(M), np.zeros(M), None, None, [], base="pi", f_best=0.0, dense=False)   # imp < 0
    assert _record(r) == (-np.inf, 0, 0)


@pytest.mark.parametrize("base", ["none", "ei", "pi"])
def test_the_first_of_planted_exact_ties_wins(base):
    M = 262147
    mu, sigma, cm, cs = np.full(M, 1.0), np.full(M, 0.7), np.full((2, M), 0.5), np.full((2, M), 0.3)
    top = [70, 300, 65536 + 9, M - 1]                         # another wave, another workgroup, the second trip of the loop
    mu[top], cm[:, top] = -1.0, -0.5
    r = _gp().constrained_on_posterior(mu, sigma, cm, cs, [0.0, 0.1], base=base, f_best=0.0, xi=0.0, idx_offset=OFFSETS[1])
    v = r.value.cpu().numpy()
    assert np.unique(v).size == 2 and np.flatnonzero(v == v.max()).tolist() == top
    assert _record(r) == (v.max(), OFFSETS[1] + 70, 0)


@pytest.mark.parametrize("base", ["none", "ei"])
def test_the_plain_product_underflows_and_the_logarithm_does_not(base):
    """What the feature exists for: eight constraints, every candidate at least 30 standard deviations inside the infeasible
    region.  The plain product of the CDFs is exactly 0 for every candidate, so a plain-product implementation sees M equal
    values and returns candidate 0; in log space the least infeasible candidate is found."""
    from scipy import special as sp

    M, C, winner = 1000, 8, 613
    rng = np.random.default_rng(8)
    cs = np.exp(rng.uniform(np.log(0.1), np.log(1.0), (C, M)))
    gamma = -rng.uniform(31.5, 60.0, (C, M))
    gamma[:, winner] = -30.5
    u = rng.uniform(-1.0, 1.0, C)
    cm = u[:, None] - gamma * cs
    with np.errstate(all="ignore"):
        g = (u[:, None] - cm) / cs                            # as the kernel forms it
        plain = np.prod(sp.ndtr(g), axis=0) * (1.0 if base == "none" else 0.3)
    assert g.max() <= -30.0 and np.all(plain == 0.0)
    r = _gp().constrained_on_posterior(np.zeros(M), np.ones(M), cm, cs, u, base=base, f_best=0.0, xi=0.0)
    v = r.value.cpu().numpy()
    want, _ = R.value(np.zeros(M), np.ones(M), cm, cs, u, BASES[base], 0.0, 0.0)
    assert np.all(np.isfinite(v)) and v.max() < -3000.0 and np.unique(v).size > M // 2
    assert r.best_idx == winner == R.first_argmax(want)[1] and r.best_val == v[winner] and r.nan_count == 0
    assert np.all(np.abs(v - want) <= R.value_bound(np.zeros(M), np.ones(M), cm, cs, u, BASES[base], 0.0, 0.0, UNITS_NDTR, UNITS_H))


# ---- end to end ---------------------------------------------------------------------------------------------------------------------
FD = [24, 25]
AXES = [np.geomspace(0.05, 5.0, 16)] * 2
SEED = 0     # chosen on the CPU (tests/matern_ref.py posteriors; the fit of "matern52-hyper" by ard_fit on matern_ref.objective): the
#              top-two gaps of log cEI are 0.13 / 0.058 and those of log EI 0.034 / 0.078 for the two cases, the feasible incumbent
#              is not the smallest observation (14 of 40 feasible), and the constrained choice is not the unconstrained one
XI_Y = 0.01
_RUNS = {}
CASES = {"se-preset": dict(kernel="se"), "matern52-hyper": dict(kernel="matern52", ard="hyper")}


def _data(case, seed=SEED):
    """gp_problem-style data (tests/ard_fit_ref.py): N = 40 uniform points in [0, 1]^2 and THREE draws of a GP with length scales
    (0.3, 0.6) at them - the objective and two constraints -, each with noise 0.05; a 24 x 25 grid of candidates; the limits at
    the constraints' 60 % quantiles (about a third of the observations feasible).  The frozen model of "se-preset" (zero mean, unit
    signal variance) gets the draws as they are, the fitted one of "matern52-hyper" gets them in units of their own."""
    rng = np.random.default_rng(seed)
    X = rng.uniform(0.0, 1.0, (40, 2))
    Xn = X / np.array([0.3, 0.6])
    sq = np.sum(Xn * Xn, axis=1)
    L = np.linalg.cholesky(np.exp(-0.5 * np.maximum(sq[:, None] + sq[None, :] - 2.0 * Xn @ Xn.T, 0.0)) + 1e-8 * np.eye(40))
    f = [L @ rng.standard_normal(40) + 0.05 * rng.standard_normal(40) for _ in range(3)]
    ys = [f[0], f[1], -f[2]] if case == "se-preset" else [40.0 + 7.0 * f[0], f[1], 3.0 - 2.0 * f[2]]
    a, b = (np.arange(24) + 0.5) / 24, (np.arange(25) + 0.5) / 25
    Xs = np.stack(np.meshgrid(a, b, indexing="ij"), -1).reshape(-1, 2)
    return X, ys, Xs, [float(np.quantile(ys[1], 0.6)), float(np.quantile(ys[2], 0.6))]


def _selectors(cls, case, affine=None, **extra):
    """(objective, constraint 0, constraint 1) of a case, updated once.  affine = (a, b): the constraints hold a + b g."""
    key = (cls.__name__, case, affine, tuple(sorted(extra.items())))
    if key not in _RUNS:
        X, ys, Xs, _ = _data(case)
        out = []
        for k, y in enumerate(ys):
            ps = cls(**CASES[case], **extra)
            ps.name, ps.iteration = "T", 0
            ps.measured_pts, ps.measured_vals = X, (y if affine is None or k == 0 else affine[0] + affine[1] * y)
            ps.feature_domain, ps.predicted_pts, ps.length_scales = FD, Xs, AXES
            if case == "se-preset":
                ps.set_kernel_params([0.3, 0.6])
            ps.update_surrogate()
            out.append(ps)
        _RUNS[key] = out
    return _RUNS[key]


def _model_inputs(sel, upper, posterior):
    """(mu, sigma, cons_mu, cons_sigma, limits, f_best, xi) in the units of the MODELS, from posterior(selector) -> (mu, sigma)."""
    obj, cons = sel[0], sel[1:]
    X = np.asarray(obj.measured_pts, dtype=np.float64)
    fb = R.feasible_incumbent(X, obj.measured_vals, [X] * len(cons), [c.measured_vals for c in cons], upper)
    m = obj._model
    mu, sigma = posterior(obj)
    post = [posterior(c) for c in cons]
    u_m = np.array([float(c._model.to_model(u)) for c, u in zip(cons, upper)])
    return (mu, sigma, np.stack([p[0] for p in post]), np.stack([p[1] for p in post]), u_m, float(m.to_model(fb)),
            XI_Y / m.y_scale), fb


def _device_posterior(ps):
    return ps._mu_dev.cpu().numpy(), ps._sigma_dev.cpu().numpy()


def _reference_posterior(ps):
    """The CPU reference posterior of the model the selector holds (tests/matern_ref.py: Cholesky route in NumPy)."""
    m = ps._model
    X, Xs = np.asarray(ps.measured_pts, dtype=np.float64), np.asarray(ps.predicted_pts, dtype=np.float64)
    y = m.to_model(np.asarray(ps.measured_vals, dtype=np.float64))
    return MR.posterior(X, y, Xs, np.asarray(ps.kernel_params, dtype=np.float64).reshape(-1), m.kernel, m.jitter1, m.jitter2)


@pytest.mark.parametrize("case", list(CASES))
def test_selector_end_to_end(case):
    sel = _selectors(PointSelector, case)
    obj, cons = sel[0], sel[1:]
    upper = _data(case)[3]
    idx = obj.constrained_expected_improvement(cons, upper, xi=XI_Y)
    acq, feas = obj.acq_func_eval.copy(), obj.log_feasibility.copy()
    shift = float(np.log(obj._model.y_scale)) if obj._model.fitted else 0.0
    # the dense values: the restatement fed the device's own posteriors (the posterior itself is pinned elsewhere)
    args, fb = _model_inputs(sel, upper, _device_posterior)
    want, want_feas = R.value(*args[:5], R.BASE_EI, *args[5:])
    bound = R.value_bound(*args[:5], R.BASE_EI, *args[5:], UNITS_NDTR, UNITS_H) + 2.0 * EPS * (np.abs(want) + abs(shift))
    worst = float(np.max(np.abs(acq.ravel() - (want + shift)) / bound))
    print(f"{case}: worst |dlog cEI| = {worst:.3f} of its bound; log cEI in [{acq.min():.4g}, {acq.max():.4g}], log feasibility in "
          f"[{feas.min():.4g}, {feas.max():.4g}], incumbent {fb:.6g} (min y {np.min(obj.measured_vals):.6g}), index {idx.tolist()}")
    assert acq.shape == feas.shape == tuple(FD) and worst <= 1.0
    assert np.all(np.abs(feas.ravel() - want_feas) <= R.value_bound(None, None, *args[2:5], R.BASE_NONE, 0.0, 0.0, UNITS_NDTR, UNITS_H))
    assert obj.constrained_base == "ei" and obj.constrained_incumbent == fb and fb > np.min(obj.measured_vals)
    assert np.array_equal(idx, np.unravel_index(int(np.argmax(acq)), FD))
    # the selected point: the restatement's on the CPU reference posterior, whose top two are apart
    ref_args, _ = _model_inputs(sel, upper, _reference_posterior)
    ref = R.value(*ref_args[:5], R.BASE_EI, *ref_args[5:])[0]
    top = np.sort(ref)[-2:]
    print(f"{case}: top-two gap of the reference {top[1] - top[0]:.3e}")
    assert top[1] - top[0] > 1e-6
    assert int(np.ravel_multi_index(tuple(idx), FD)) == R.first_argmax(ref)[1]
    # DeviceGP.select_constrained on the selectors' own surrogates: the same point
    r = obj._gp.select_constrained(obj._cand[0], [c._gp for c in cons], [float(c._model.to_model(u)) for c, u in zip(cons, upper)],
                                   f_best=ref_args[5], xi=ref_args[6], dense=True)
    assert r.best_idx == int(np.ravel_multi_index(tuple(idx), FD)) and r.nan_count == 0 and r.base == "ei"
    with pytest.raises(ValueError, match="must be a DeviceGP"):
        obj._gp.select_constrained(obj._cand[0], [cons[0]], [0.0])     # (a selector object is not its surrogate)
    # the other two calls: each the restatement's choice on the device posterior, unit-free values
    for call, base, a in ((lambda: obj.probability_of_feasibility(cons, upper), R.BASE_NONE, args[:5] + (0.0, 0.0)),
                          (lambda: obj.probability_of_improvement(xi=XI_Y), R.BASE_PI,
                           (args[0], args[1], None, None, [], float(obj._model.to_model(np.min(obj.measured_vals))), args[6]))):
        i = call()
        w = R.value(*a[:5], base, *a[5:])[0]
        b = R.value_bound(*a[:5], base, *a[5:], UNITS_NDTR, UNITS_H)
        assert np.all(np.abs(obj.acq_func_eval.ravel() - w) <= b) and np.all(obj.acq_func_eval <= 0.0)
        assert np.array_equal(i, np.unravel_index(int(np.argmax(obj.acq_func_eval)), FD))
        assert obj.constrained_base == ("none" if base == R.BASE_NONE else "pi")
    # no constraint, base EI: the point expected_improvement() selects (the same incumbent, the plain form's own arg-max)
    i0 = obj.constrained_expected_improvement([], [], xi=XI_Y)
    log_ei = obj.acq_func_eval.copy()
    assert obj.constrained_incumbent == np.min(obj.measured_vals) and not obj.log_feasibility.any()
    i1 = obj.expected_improvement(xi=XI_Y)
    ei = obj.acq_func_eval
    assert np.array_equal(i0, i1) and not np.array_equal(i0, idx)      # (the constraints move the choice on these data)
    big = ei > 1e-200
    assert np.all(np.abs(log_ei[big] - np.log(ei[big])) <= 1e-6 * (1.0 + np.abs(log_ei[big])))   # (plain EI cancels below z ~ -5)
    # no feasible observation: Gelbart's rule, said in the attributes
    low = [float(np.min(c.measured_vals)) - 1.0 for c in cons]
    i2 = obj.constrained_expected_improvement(cons, low, xi=XI_Y)
    assert obj.constrained_base == "none" and obj.constrained_incumbent is None
    assert np.array_equal(obj.acq_func_eval, obj.log_feasibility) and np.array_equal(i2, obj.probability_of_feasibility(cons, low))
    # mismatches are refused: other candidates, other measured points under the feasible rule (a number still works)
    X = np.asarray(cons[0].measured_pts, dtype=np.float64)
    keep = cons[0].measured_pts
    try:
        cons[0].measured_pts = (X + 1e-9).tolist()
        with pytest.raises(ValueError, match="same measured points"):
            obj.constrained_expected_improvement(cons, upper)
        assert np.array_equal(obj.constrained_expected_improvement(cons, upper, xi=XI_Y, f_best=fb), idx)
    finally:
        cons[0].measured_pts = keep
    keep = cons[1].predicted_pts
    try:
        cons[1].predicted_pts = np.asarray(keep) + 1e-12
        with pytest.raises(ValueError, match="same predicted_pts"):
            obj.constrained_expected_improvement(cons, upper)
    finally:
        cons[1].predicted_pts = keep
    assert obj.lower_confidence_bound().shape == (2,)         # the update's own acquisition is still served


def test_limits_and_values_are_invariant_under_an_affine_map_of_the_constraint_data():
    """ard="hyper" fits mean and scale: a constraint given as a + b g with the limit a + b u is the same constraint.  The two fits
    follow the same path up to rounding (the profiled likelihood is invariant), so the posteriors in the units of the models
    agree to about 1e-9; a term moves by (|gamma| + 1) times the change of its argument, |gamma| <= 40 here: 1e-6 relative."""
    a, b = -250.0, 40.0
    upper = _data("matern52-hyper")[3]
    sel, sel2 = _selectors(PointSelector, "matern52-hyper"), _selectors(PointSelector, "matern52-hyper", affine=(a, b))
    i1 = sel[0].constrained_expected_improvement(sel[1:], upper, xi=XI_Y)
    v1, f1 = sel[0].acq_func_eval.copy(), sel[0].log_feasibility.copy()
    i2 = sel2[0].constrained_expected_improvement(sel2[1:], [a + b * u for u in upper], xi=XI_Y)
    v2, f2 = sel2[0].acq_func_eval, sel2[0].log_feasibility
    print(f"affine map of the constraints: |dvalue| {np.max(np.abs(v1 - v2)):.3e}, |dlog feasibility| {np.max(np.abs(f1 - f2)):.3e}")
    assert np.array_equal(i1, i2)
    assert np.all(np.abs(v1 - v2) <= 1e-6 * (1.0 + np.abs(v1))) and np.all(np.abs(f1 - f2) <= 1e-6 * (1.0 + np.abs(f1)))


@pytest.mark.parametrize("case", list(CASES))
def test_host_and_device_classes_agree(case):
    """The host class runs the same kernel on mean_func / cov_func taken back to the units of the model.  Its dense values are held
    to the restatement fed the DEVICE class's posteriors, by the bounds above plus a FIXED allowance for its inputs: every
    standardised argument and log sigma, recomputed here from the host class's public mean_func / cov_func, must lie within
    ARG_CAP = 1e-9 of the device class's.  (Why 1e-9: the two classes' fits are pinned to each other at 1e-10 relative and their
    mean_func at 1e-9 by tests/test_gpu_matern.py, and the round trip through the units of y costs a few eps (|m| / s + |mu|) /
    sigma, about 1e-13 here; 1.4e-14 was measured.  A wrong conversion - a missing division by y_scale, a wrong to_model - moves
    the arguments by order 1.)  An argument a that moves by da moves log Phi by at most (|a| + 1) da and log h by at most
    (|a| + 2) da (the slopes phi / Phi and Phi / h), log sigma by its own change.  The frozen model maps nothing: same bits."""
    ARG_CAP = 1e-9
    upper = _data(case)[3]
    sel, hst = _selectors(PointSelector, case), _selectors(PointSelectorHost, case)
    idx = sel[0].constrained_expected_improvement(sel[1:], upper, xi=XI_Y)
    v, f = sel[0].acq_func_eval.copy(), sel[0].log_feasibility.copy()
    idh = hst[0].constrained_expected_improvement(hst[1:], upper, xi=XI_Y)
    vh, fh = hst[0].acq_func_eval, hst[0].log_feasibility
    assert np.array_equal(idx, idh) and hst[0].constrained_base == "ei" and hst[0].constrained_incumbent == sel[0].constrained_incumbent
    if case == "se-preset":
        assert all(np.array_equal(h.mean_func, d.mean_func) and np.array_equal(h.cov_func, d.cov_func) for h, d in zip(hst, sel))
        assert vh.tobytes() == v.tobytes() and fh.tobytes() == f.tobytes()
        return

    def host_posterior(ps):   # from the public attributes, in the units of the model
        m = ps._model
        return (np.asarray(ps.mean_func).ravel() - m.y_mean) / m.y_scale, np.asarray(ps.cov_func).ravel() / m.y_scale

    def arguments(a):
        mu, sigma, cm, cs, u_m, fb, xi = a
        return ((fb - mu) - xi) / sigma, (u_m[:, None] - cm) / cs, np.log(sigma)

    ad, _ = _model_inputs(sel, upper, _device_posterior)
    ah, _ = _model_inputs(hst, upper, host_posterior)
    (zd, gd, ld), (zh, gh, lh) = arguments(ad), arguments(ah)
    moved_args = max(np.abs(zd - zh).max(), np.abs(gd - gh).max(), np.abs(ld - lh).max())
    shift = float(np.log(sel[0]._model.y_scale))
    want, want_f = R.value(*ad[:5], R.BASE_EI, *ad[5:])
    bound = R.value_bound(*ad[:5], R.BASE_EI, *ad[5:], UNITS_NDTR, UNITS_H) + 2.0 * EPS * (np.abs(want) + abs(shift))
    allowed_f = np.sum((np.abs(gd) + 1.0 + ARG_CAP) * ARG_CAP, axis=0)
    allowed = allowed_f + (np.abs(zd) + 2.0 + ARG_CAP) * ARG_CAP + 2.0 * ARG_CAP   # (log sigma, and log y_scale of the other fit)
    worst = float(np.max(np.abs(vh.ravel() - (want + shift)) / (bound + allowed)))
    print(f"{case}: host class against the restatement on the device class's posterior, worst |dlog cEI| {worst:.3e} of its bound; "
          f"largest change of an argument {moved_args:.2e} (cap {ARG_CAP:.0e}); |dlog cEI| host - device {np.abs(vh - v).max():.2e}")
    assert moved_args <= ARG_CAP and abs(np.log(hst[0]._model.y_scale) - shift) <= ARG_CAP
    fbound = R.value_bound(None, None, *ad[2:5], R.BASE_NONE, 0.0, 0.0, UNITS_NDTR, UNITS_H)
    assert worst <= 1.0 and np.all(np.abs(fh.ravel() - want_f) <= fbound + allowed_f)


# ---- candidates sharded over two ranks on one GPU -------------------------------------------------------------------------------
def _sharded_worker(rank, world, port, q):
    import torch.distributed as dist

    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        sel = _selectors(PointSelector, "se-preset", device=DEV)
        idx = sel[0].constrained_expected_improvement(sel[1:], _data("se-preset")[3], xi=XI_Y)
        q.put((rank, idx.tolist(), sel[0].acq_func_eval.tobytes(), sel[0].log_feasibility.tobytes(), sel[0]._lo_hi))
    finally:
        dist.destroy_process_group()


def test_two_ranks_sharing_the_gpu_return_the_single_process_answer():
    import socket

    import torch.multiprocessing as mp

    sel = _selectors(PointSelector, "se-preset")
    idx = sel[0].constrained_expected_improvement(sel[1:], _data("se-preset")[3], xi=XI_Y)
    acq, feas = sel[0].acq_func_eval.tobytes(), sel[0].log_feasibility.tobytes()
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
    assert sorted(r[4] for r in res) == [(0, 300), (300, 600)]
    for _, i, a, f, _ in res:
        assert i == idx.tolist() and a == acq and f == feas
