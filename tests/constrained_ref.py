"""NumPy / SciPy restatement of the constrained acquisitions in log space (csrc/constrained.hip, csrc/cons_math.h,
bayesian_optimisation_amd/constrained.py): log h, the terms, the value, the edge rules and the incumbent rule, written from
include/gpbo.h and independently of the package (nothing here imports bayesian_optimisation_amd).

    feas(x)  = sum_{c < C} log Phi((u_c - mu_c) / sigma_c)             (added in index order, c = 0 first, from 0)
    value(x) = base(x) + feas(x),  base = 0 | log sigma + log h(z) | log Phi(z),  z = ((f_best - mu) - xi) / sigma
Two forms of every term: the fp64 one of the header (SciPy erfc / erfcx / log1p: `log_h`, and `log_ndtr64` for log Phi), whose
error against the 60-digit fixtures is what the tests measure, and a high-precision one without mpmath (`log_h_hp`,
`log_ndtr_hp`: x86 long double, a continued fraction and a series instead of erfc) for the places where a test needs a reference
BETWEEN the fixtures' points.
Edge rules: a NaN in any input the call reads gives NaN; sigma_c == 0: 0 where mu_c <= u_c, else -inf; sigma == 0: EI
log(max(imp, 0)), PI 0 where imp > 0 else -inf.
"""
import numpy as np
from scipy import special as sp

EPS = np.finfo(np.float64).eps
BASE_NONE, BASE_EI, BASE_PI = 0, 1, 2
HALF_LOG_2PI = 0.5 * np.log(2.0 * np.pi)


def log_ndtr64(g):
    """log Phi in the three fp64 branches of include/gpbo.h (what mes_log_ndtr evaluates)."""
    g = np.asarray(g, dtype=np.float64)
    out = np.empty_like(g)
    with np.errstate(all="ignore"):
        hi, mid, lo = g > 0.0, (g <= 0.0) & (g >= -1.0), ~(g >= -1.0)
        out[hi] = np.log1p(-0.5 * sp.erfc(g[hi] / np.sqrt(2.0)))
        out[mid] = np.log(0.5 * sp.erfc(-g[mid] / np.sqrt(2.0)))
        t = -g[lo] / np.sqrt(2.0)
        out[lo] = -(t * t) + np.log(0.5 * sp.erfcx(t))
    return out


def log_h_branch(z):
    """0: z >= 0 and 1: -1 <= z < 0 (the plain form, reported apart: only below 0 do its terms cancel), 2: -1e3 < z < -1,
    3: z <= -1e3."""
    z = np.asarray(z, dtype=np.float64)
    return np.where(z >= 0.0, 0, np.where(z >= -1.0, 1, np.where(z > -1.0e3, 2, 3)))


def log_h(z):
    """log(phi(z) + z Phi(z)) in the three fp64 branches of include/gpbo.h."""
    z = np.asarray(z, dtype=np.float64)
    out = np.empty_like(z)
    with np.errstate(all="ignore"):
        top, mid, low = z >= -1.0, (z < -1.0) & (z > -1.0e3), ~(z > -1.0e3)
        zt = z[top]
        out[top] = np.log(np.exp(-0.5 * zt * zt) / np.sqrt(2.0 * np.pi) + zt * (0.5 * sp.erfc(-zt / np.sqrt(2.0))))
        t = -z[mid] / np.sqrt(2.0)
        out[mid] = (-(t * t) - HALF_LOG_2PI) + np.log1p(-(np.sqrt(np.pi) * t) * sp.erfcx(t))
        t = -z[low] / np.sqrt(2.0)
        u = 1.0 / (2.0 * (t * t))
        out[low] = (-(t * t) - HALF_LOG_2PI) + np.log(u * (1.0 - 3.0 * u * (1.0 - 5.0 * u)))
    return out


_LD = np.longdouble
_HALF_LOG_2PI_LD = _LD("0.918938533204672741780329736405617639861")
_SQRT_2PI_LD = _LD("2.506628274631000502415765284811045253007")
_CF_TERMS = 400


def _cf_K(x):
    """K = 1 / (x + 2 / (x + 3 / (x + ...))) for x >= 1 in long double: Laplace's continued fraction of the Mills ratio,
    Phi(-x) / phi(x) = 1 / (x + K), evaluated backwards from _CF_TERMS levels (at x = 1 the tail is below
    exp(-2 sqrt(2 _CF_TERMS)) ~ 3e-25; every quantity is positive: nothing cancels)."""
    K = np.zeros_like(x)
    for n in range(_CF_TERMS, 1, -1):
        K = _LD(n) / (x + K)
    return _LD(1.0) / (x + K)


def _ndtr_small(z):
    """Phi(z) for |z| <= 1 in long double: (1 + erf(z / sqrt 2)) / 2 with erf(x) = 2 / sqrt(pi) sum_n (-1)^n x^(2n+1) / (n! (2n+1)),
    |x| <= 0.7072: 40 terms, the largest of them x itself."""
    x = z / np.sqrt(_LD(2.0))
    s, p = np.zeros_like(x), x.copy()          # p = (-1)^n x^(2n+1) / n!
    for n in range(40):
        s = s + p / _LD(2 * n + 1)
        p = -p * x * x / _LD(n + 1)
    return (1 + 2 * s / np.sqrt(_LD("3.141592653589793238462643383279502884197"))) / 2


def _hp(z, want_h):
    """log h (want_h) or log Phi in long double without erfc / erfcx, rounded to fp64 once.  x = |z|, phi = phi(z):
        z < -1      Phi = phi / (x + K):    log Phi = log phi - log(x + K);   h = phi K / (x + K): log h = log phi + log K - log(x + K)
        |z| <= 1    Phi by the series:      log Phi;                          log(phi + z Phi)
        z > 1       1 - Phi = phi / (x + K): log1p(-phi / (x + K));           log(phi + z (1 - phi / (x + K)))"""
    z = np.asarray(z, dtype=np.float64)
    zl = z.astype(_LD)
    out = np.full(z.shape, np.nan, dtype=_LD)
    with np.errstate(all="ignore"):
        log_phi = -(zl * zl) / 2 - _HALF_LOG_2PI_LD
        low, mid, top = z < -1.0, np.abs(z) <= 1.0, z > 1.0
        x = -zl[low]
        K = _cf_K(x)
        out[low] = log_phi[low] + (np.log(K) if want_h else 0) - np.log(x + K)
        cdf = _ndtr_small(zl[mid])
        out[mid] = np.log(np.exp(log_phi[mid]) + zl[mid] * cdf) if want_h else np.log(cdf)
        x = zl[top]
        tail = np.exp(log_phi[top]) / (x + _cf_K(x))
        out[top] = np.log(np.exp(log_phi[top]) + x * (1 - tail)) if want_h else np.log1p(-tail)
    return out.astype(np.float64)


def log_h_hp(z):
    """log h to well below one unit of its scale, at any z (NaN for NaN)."""
    return _hp(z, True)


def log_ndtr_hp(g):
    """log Phi to well below one unit of its scale, at any gamma (NaN for NaN)."""
    return _hp(g, False)


def term_scale(arg, term):
    """What the error of a term is measured in: max(1, arg^2 / 2 for arg < 0) + |term| (below -1 the -arg^2 / 2 of the term is
    formed from a rounded argument)."""
    arg, term = np.asarray(arg, dtype=np.float64), np.asarray(term, dtype=np.float64)
    with np.errstate(all="ignore"):
        return np.maximum(1.0, np.where(arg < 0.0, 0.5 * arg * arg, 0.0)) + np.abs(term)


def fixture_worst(fn, arg, want, branch=None) -> list:
    """The worst error of fn(arg) against the 60-digit `want`, in units of eps term_scale; per branch id when given."""
    err = np.abs(fn(arg) - want) / (EPS * term_scale(arg, want))
    if branch is None:
        return [float(err.max())]
    return [float(err[branch == b].max()) for b in range(int(branch.max()) + 1)]


def feasible_terms(cons_mu, cons_sigma, upper, log_ndtr=log_ndtr_hp):
    """([C x M] terms log Phi((u_c - mu_c) / sigma_c) with the edge rules, [C x M] their standardised arguments)."""
    cm, cs = np.atleast_2d(np.asarray(cons_mu, dtype=np.float64)), np.atleast_2d(np.asarray(cons_sigma, dtype=np.float64))
    u = np.asarray(upper, dtype=np.float64).reshape(-1, 1)
    bad = np.isnan(cm) | np.isnan(cs)
    zero = (cs == 0.0) & ~bad
    with np.errstate(all="ignore"):
        g = (u - cm) / np.where(zero | bad, 1.0, cs)
        t = log_ndtr(g)
        t = np.where(zero, np.where(cm <= u, 0.0, -np.inf), t)
    return np.where(bad, np.nan, t), g


def base_term(base, mu, sigma, f_best, xi, hp=True):
    """([M] base term with the edge rules, [M] z); BASE_NONE: zeros."""
    if base == BASE_NONE:
        return 0.0, None
    mu, sigma = np.asarray(mu, dtype=np.float64).reshape(-1), np.asarray(sigma, dtype=np.float64).reshape(-1)
    bad = np.isnan(mu) | np.isnan(sigma)
    zero = (sigma == 0.0) & ~bad
    with np.errstate(all="ignore"):
        imp = (f_best - mu) - xi
        z = imp / np.where(zero | bad, 1.0, sigma)
        if base == BASE_PI:
            b = (log_ndtr_hp if hp else log_ndtr64)(z)
            b = np.where(zero, np.where(imp > 0.0, 0.0, -np.inf), b)
        else:
            b = np.log(sigma) + (log_h_hp if hp else log_h)(z)
            b = np.where(zero, np.log(np.maximum(imp, 0.0)), b)
    return np.where(bad, np.nan, b), z


def value(mu, sigma, cons_mu, cons_sigma, upper, base=BASE_EI, f_best=0.0, xi=0.0, hp=True):
    """(value [M], feas [M]) as the header defines them: feas added in index order from 0, then base + feas."""
    C = len(np.asarray(upper).reshape(-1))
    b, _ = base_term(base, mu, sigma, f_best, xi, hp)
    if C == 0:
        return np.asarray(b, dtype=np.float64) + 0.0, np.zeros_like(np.asarray(b, dtype=np.float64))
    t, _ = feasible_terms(cons_mu, cons_sigma, upper, log_ndtr_hp if hp else log_ndtr64)
    feas = np.zeros(t.shape[1])
    with np.errstate(all="ignore"):
        for c in range(C):
            feas = feas + t[c]
        return b + feas, feas


def value_bound(mu, sigma, cons_mu, cons_sigma, upper, base, f_best, xi, units_ndtr, units_h):
    """The absolute error allowed to a computed value against value(hp=True): units_ndtr units of each log Phi term's scale,
    units_h units of log h's, 2 eps |log sigma| (a logarithm rounded once here and once there), and max(C, 1) eps sum |terms| for
    the roundings of the additions (at most C + 1 of them, eps / 2 of a partial sum each)."""
    C = len(np.asarray(upper).reshape(-1))
    b, z = base_term(base, mu, sigma, f_best, xi)
    bound, mass = 0.0, 0.0
    with np.errstate(all="ignore"):
        if base == BASE_PI:
            bound, mass = units_ndtr * EPS * term_scale(z, b), np.abs(b)
        elif base == BASE_EI:
            sg = np.asarray(sigma, dtype=np.float64).reshape(-1)
            zero = sg == 0.0                                   # there the base is log(max(imp, 0)): one logarithm, twice rounded
            ls = np.log(np.where(zero, 1.0, sg))
            lh = np.where(zero, 0.0, b - ls)
            bound = np.where(zero, 2.0 * EPS * np.abs(b), units_h * EPS * term_scale(z, lh) + 2.0 * EPS * np.abs(ls))
            mass = np.where(zero, np.abs(b), np.abs(ls) + np.abs(lh))
        if C:
            t, g = feasible_terms(cons_mu, cons_sigma, upper)
            bound = bound + np.sum(units_ndtr * EPS * term_scale(g, t), axis=0)
            mass = mass + np.sum(np.abs(t), axis=0)
        return bound + max(C, 1) * EPS * mass


def first_argmax(v, idx_offset=0):
    """(best value, index, NaN count) under the library's rule: NaN never chosen, -inf legal, ties to the lowest index."""
    v = np.asarray(v, dtype=np.float64).reshape(-1)
    ok = ~np.isnan(v)
    if not ok.any():
        return -np.inf, np.iinfo(np.int64).max, int((~ok).sum())
    best = v[ok].max()
    return float(best), int(idx_offset) + int(np.flatnonzero(ok & (v == best))[0]), int((~ok).sum())


def feasible_incumbent(points, values, cons_points, cons_values, upper):
    """min of `values` over the observations at which every constraint's observation is <= its limit; None when there is none;
    ValueError when the points of a constraint are not those of the objective, bit for bit."""
    X, y = np.asarray(points, dtype=np.float64), np.asarray(values, dtype=np.float64).reshape(-1)
    ok = ~np.isnan(y)
    for Xc, yc, u in zip(cons_points, cons_values, np.asarray(upper, dtype=np.float64).reshape(-1)):
        Xc, yc = np.asarray(Xc, dtype=np.float64), np.asarray(yc, dtype=np.float64).reshape(-1)
        if Xc.shape != X.shape or not np.array_equal(Xc.view(np.int64), X.view(np.int64)) or yc.size != y.size:
            raise ValueError("the constraint's measured points are not the objective's")
        with np.errstate(invalid="ignore"):
            ok &= yc <= u
    return float(y[ok].min()) if ok.any() else None
