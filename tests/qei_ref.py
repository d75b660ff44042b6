"""High-precision reference of the q = 8 Monte-Carlo qEI (csrc/sigma_acq.hip: the GRAM form of sigma_acq_kernel + qei_kernel),
shared by the qEI tests.  Plain NumPy in np.longdouble (x87 extended: 64-bit mantissa), restating oracle.gp_oracle.qei_mc:

    K       = k(X, X) with the reference's diagonal (1 + 1e-4) + 1e-6,  K = L L^T (column Cholesky),  alpha = K^-1 y
    V_b     = L^-1 k(X, P_b) by forward substitution, mu_b = k(X, P_b)^T alpha   (no "same shape" jitter quirk: N == 8 is plain)
    Sigma_b = K_bb - V_b^T V_b with PRIOR_VAR on the diagonal,  L_b = chol(Sigma_b)
    qEI_b   = mean_s max(0, max_j (f_best - xi - (mu_b + L_b z_s)_j))

The Cholesky and the substitution are Python loops over N: meant for N <= about 300 (a fraction of a second); above that the
tests compare with the fp64 oracle.  Where long double is only 64 bits (HAVE_LONGDOUBLE False) `reference` IS the fp64 oracle
and says so through its third return value; nothing fails.

`assert_informative(ref)`: the condition every value comparison of the qEI tests carries.  With f_best = min(y) most batches
of a late-BO problem have qEI exactly 0 on the device and in any reference, whatever Sigma_b was, so a comparison proves
nothing; the tests take the incumbent from the ORACLE's posterior mean (a quantile in [0.5, 0.9]) and require every compared
batch to have a reference value >= INFORMATIVE."""
import numpy as np
import scipy.linalg as sla

from oracle import gp_oracle as O

LD = np.longdouble
HAVE_LONGDOUBLE = bool(np.finfo(LD).eps < 2e-19)
INFORMATIVE = 1e-6
Q = 8


def assert_informative(ref):
    """Every compared batch has a reference qEI >= 1e-6 (change the input, not the threshold)."""
    ref = np.asarray(ref, dtype=np.float64)
    assert ref.size > 0 and np.isfinite(ref).all(), "reference qEI is not finite"
    small = np.flatnonzero(ref < INFORMATIVE)
    assert small.size == 0, f"{small.size} of {ref.size} compared batches have reference qEI < {INFORMATIVE:g} " \
                            f"(smallest {ref.min():.3e} at batch {int(np.argmin(ref))}): the comparison would be 0 == 0"


def _gram(A, B, ls):
    acc = np.zeros((A.shape[0], B.shape[0]), dtype=LD)
    for k in range(A.shape[1]):
        acc += (A[:, k, None] - B[None, :, k]) ** 2 / ls[k] ** 2
    return np.exp(LD(-0.5) * acc)


def _cholesky(A):
    """Lower Cholesky factor, column by column; ValueError where a pivot is not positive."""
    n = A.shape[0]
    L = np.zeros_like(A)
    for j in range(n):
        c = A[j:, j] - L[j:, :j] @ L[j, :j]
        if not c[0] > 0:
            raise ValueError(f"pivot {j} is not positive: {float(c[0])!r}")
        L[j:, j] = c / np.sqrt(c[0])
    return L


def _solve_lower(L, B):
    Y = np.zeros_like(B)
    for i in range(L.shape[0]):
        Y[i] = (B[i] - L[i, :i] @ Y[:i]) / L[i, i]
    return Y


def _solve_upper(U, B):
    Y = np.zeros_like(B)
    for i in range(U.shape[0] - 1, -1, -1):
        Y[i] = (B[i] - U[i, i + 1:] @ Y[i + 1:]) / U[i, i]
    return Y


def qei_longdouble(X, y, Xs, ls, Z, f_best, xi=0.0, skip_nan=False):
    """(qEI per batch as fp64, smallest eigenvalue of each Sigma_b as fp64), all arithmetic in np.longdouble.
    skip_nan: a NaN improvement never raises a sample's maximum (what qei_kernel does with a NaN base sample: z_sk reaches
    candidates k..7 only, L_b being lower triangular) instead of making the value NaN (what the oracle does)."""
    X, Xs, Z = (np.asarray(a, dtype=np.float64).astype(LD) for a in (X, Xs, Z))
    y = np.asarray(y, dtype=np.float64).reshape(-1).astype(LD)
    ls = np.asarray(ls, dtype=np.float64).reshape(-1).astype(LD)
    N, M = X.shape[0], Xs.shape[0]
    assert M % Q == 0 and Z.shape[1] == Q
    prior = LD(O.PRIOR_VAR)
    K = _gram(X, X, ls)
    K[np.arange(N), np.arange(N)] = prior
    L = _cholesky(K)
    alpha = _solve_upper(L.T, _solve_lower(L, y[:, None]))[:, 0]
    Ks = _gram(X, Xs, ls)                       # (N, M)
    mu = Ks.T @ alpha
    V = _solve_lower(L, Ks)
    out, lam = np.empty(M // Q), np.empty(M // Q)
    thr = LD(f_best) - LD(xi)
    for b in range(M // Q):
        sl = slice(b * Q, (b + 1) * Q)
        Kbb = _gram(Xs[sl], Xs[sl], ls)
        Kbb[np.arange(Q), np.arange(Q)] = prior
        Sig = Kbb - V[:, sl].T @ V[:, sl]
        lam[b] = np.linalg.eigvalsh(Sig.astype(np.float64)).min()
        Lb = _cholesky(Sig)
        f = mu[None, sl] + np.stack([Z[:, :j + 1] @ Lb[j, :j + 1] for j in range(Q)], axis=1)   # row j of L_b z_s: z_s0..z_sj only
        if skip_nan:
            with np.errstate(invalid="ignore"):
                out[b] = float(np.mean(np.fmax(LD(0), np.fmax.reduce(thr - f, axis=1))))
        else:
            out[b] = float(np.mean(np.maximum(LD(0), np.max(thr - f, axis=1))))
    return out, lam


def min_eig_f64(X, y, Xs, ls):
    """Smallest eigenvalue of every Sigma_b from the fp64 oracle's pieces (the fall-back of `reference`, and large N)."""
    X, Xs = np.asarray(X, dtype=np.float64), np.asarray(Xs, dtype=np.float64)
    lsq = np.asarray(ls, dtype=np.float64).reshape(-1)
    _, L, _ = O.factorise(X, y, ls)
    lam = np.empty(len(Xs) // Q)
    for b in range(len(lam)):
        P = Xs[b * Q:(b + 1) * Q]
        d2 = np.zeros((len(X), Q))
        for k in range(X.shape[1]):
            d2 += (X[:, k, None] - P[None, :, k]) ** 2 / lsq[k] ** 2
        V = sla.solve_triangular(L, np.exp(-0.5 * d2), lower=True, check_finite=False)
        p2 = np.zeros((Q, Q))
        for k in range(X.shape[1]):
            p2 += (P[:, k, None] - P[None, :, k]) ** 2 / lsq[k] ** 2
        Kbb = np.exp(-0.5 * p2)
        Kbb[np.arange(Q), np.arange(Q)] = O.PRIOR_VAR
        lam[b] = np.linalg.eigvalsh(Kbb - V.T @ V).min()
    return lam


def reference(X, y, Xs, ls, Z, f_best, xi=0.0):
    """(values, smallest eigenvalues, name): the long-double reference, or - where long double is 64 bits - the fp64 oracle."""
    if HAVE_LONGDOUBLE:
        v, lam = qei_longdouble(X, y, Xs, ls, Z, f_best, xi)
        return v, lam, "longdouble"
    return O.qei_mc(X, y, Xs, ls, Z, f_best, xi), min_eig_f64(X, y, Xs, ls), "oracle-fp64 (long double is 64 bits here)"


def oracle_mean(X, y, Xs, ls):
    """Posterior mean of the fp64 oracle at Xs WITHOUT the reference's N == M jitter quirk (as qei_mc forms it per batch)."""
    X, Xs = np.asarray(X, dtype=np.float64), np.asarray(Xs, dtype=np.float64)
    lsq = np.asarray(ls, dtype=np.float64).reshape(-1)
    _, _, alpha = O.factorise(X, y, ls)
    d2 = np.zeros((len(X), len(Xs)))
    for k in range(X.shape[1]):
        d2 += (X[:, k, None] - Xs[None, :, k]) ** 2 / lsq[k] ** 2
    return np.exp(-0.5 * d2).T @ alpha


def incumbent(X, y, Xs, ls, quantile=0.5):
    """f_best from the reference side only: a quantile in [0.5, 0.9] of the oracle's posterior mean at the compared candidates
    (NaN candidates, which the NaN tests plant, are left out)."""
    assert 0.5 <= quantile <= 0.9
    mu = oracle_mean(X, y, Xs, ls)
    return float(np.quantile(mu[np.isfinite(mu)], quantile))
