"""Exact host emulation of the int8-sliced variance product, from the mathematics in the header of csrc/ozaki.hip
(NumPy only; not the kernel's code), and the operands the CPU and GPU tests of that product share.

    e_j  = frexp exponent of max_{i<=j} |U_ij|  (0 for an all-zero column)
    T_k  = rint(k 2^38),  T_u = rint(U_ij 2^(46 - e_j))            (half to even; below the diagonal: zero)
    T    = sum_a D_a 256^(n-1-a),  D_a in [-128, 127]               (five digits of T_k, six of T_u)
    G_g  = sum_{a+b=g} K_a U_b                                       (exact integers, |G_g| < 2^31)
    v_j  = 2^e_j sum_g 2^(-12-8g) G_g                                (added from the smallest diagonal up, each add rounded)
    ssq  = sum_j v_j^2
Full pass: a < 5, b < 6, g <= 5 (20 products).  Coarse pass: a, b < 3, g <= 2 (6 products).

Everything up to G_g is exact, so the device's |v|^2 can differ from `ssq` only by the rounding of the v_j chain (at most
six roundings, each <= 2^-53 S_j with S_j = 2^e_j sum_g 2^(-12-8g) |G_g|), of the squares and of one fp64 sum over Np
columns in an order this module does not know:
    tol = 2^-53 ((Np + 4) ssq + 12 sum_j |v_j| S_j).
"""
import numpy as np

from bayesian_optimisation_amd.synthetic import make_problem
from oracle import gp_oracle as O

NK, NU = 5, 6            # digits of T_k, T_u
K_BITS, U_BITS = 38, 46  # T_k = rint(k 2^38), T_u = rint(u 2^(46 - e))
T_MAX = 2 ** 46 - 1      # largest |T| a planted entry may have (a column maximum just below 2^e rounds to 2^46)

_CARRY_POS = [
    1, 127, 128, 129, 255, 256, 257, 0x7F7F, 0x7F80, 0x8080, 0x8081, 0x7F7F7F, 0x808080, 0x7F7F7F7F, 0x7F807F80,
    0x80808080, 0x80808081, 0xFFFFFFFF, 0x100000000, 0x7F7F7F7F7F, 0x8080808080, 0x807F7F7F7F, 0x00FFFFFFFFFF,
    0x007F807F807F, 0x008080808080, 0x008080808081, 0x00807F7F7F7F, 0x017F7F7F7F7F, 0x3F7F7F7F7F7F, 0x3F7F7F7F7F80,
    0x3F8080808080, 0x3F807F7F7F7F, 63 * 2 ** 40 + 0x7F7F7F7F7F, 63 * 2 ** 40 + 0x8080808080, 2 ** 45 - 1, 2 ** 45,
    2 ** 45 + 1, 2 ** 46 - 129, 2 ** 46 - 128, 2 ** 46 - 1,
] + [2 ** k for k in (7, 15, 23, 31, 39)] + [2 ** k - 1 for k in (15, 23, 31, 39, 40)] + [2 ** k + 1 for k in (8, 16, 24, 32, 40)]
# byte patterns that carry through several digits, values next to a power of two, both signs
CARRY_T = [0] + [s * t for t in sorted(set(_CARRY_POS)) for s in (1, -1)]
assert all(abs(t) <= T_MAX for t in CARRY_T)


# ---- digits ---------------------------------------------------------------------------------------------------------------
def digits(T, s):
    """Balanced base-256 digits of an int64 array, most significant first: T = sum_a D_a 256^(s-1-a), D_a in [-128, 127]
    (as tools/ozaki_error.py: digits).  Raises if T does not fit s digits."""
    r = np.asarray(T, dtype=np.int64).copy()
    out = []
    for _ in range(s):
        lo = ((r + 128) % 256) - 128
        out.append(lo.astype(np.float64))
        r = (r - lo) // 256
    assert np.all(r == 0), "top digit overflow"
    return out[::-1]


def digits_bytewise(T, s):
    """The same digits of ONE Python integer by the method the comments on digits4 / digits4_k describe: the bytes of
    T + 0x80..80 (0x80 in every byte below the top one), xor 0x80 below the top, the top byte as it is (two's complement)."""
    off = sum(0x80 << (8 * i) for i in range(s - 1))
    tp = (int(T) + off) & ((1 << (8 * s)) - 1)
    out = []
    for i in range(s - 1, -1, -1):
        b = (tp >> (8 * i)) & 0xFF
        if i < s - 1:
            b ^= 0x80
        out.append(b - 256 if b >= 128 else b)
    return out


# ---- the two roundings ------------------------------------------------------------------------------------------------
def _upper(U):
    U = np.asarray(U, dtype=np.float64)
    n = U.shape[0]
    return np.where(np.arange(n)[:, None] <= np.arange(n)[None, :], U, 0.0)   # below the diagonal: zero, whatever is stored


def column_exponents(U):
    m = np.abs(_upper(U)).max(axis=0)
    assert np.all((m == 0.0) | ((m >= 2.0 ** -200) & (m <= 2.0 ** 200))), "column maxima outside [2^-200, 2^200]"
    return np.frexp(m)[1].astype(np.int64)   # frexp(0) = (0, 0)


def quantise_u(U):
    """(T_u [Np x Np] int64, e [Np] int64)"""
    e = column_exponents(U)
    T = np.rint(_upper(U) * 2.0 ** (U_BITS - e)[None, :])   # a power-of-two scaling is exact; rint rounds half to even
    return T.astype(np.int64), e


def quantise_k(Ks):
    return np.rint(np.asarray(Ks, dtype=np.float64) * 2.0 ** K_BITS).astype(np.int64)


def operands(Ks, U):
    """Ks [M x Np] (candidate c, observation n), U [Np x Np] -> (K digits [5] of [M x Np], U digits [6] of [Np x Np], e)."""
    Tu, e = quantise_u(U)
    return digits(quantise_k(Ks), NK), digits(Tu, NU), e


# ---- slice products and recombination ---------------------------------------------------------------------------------
def diagonals(Kd, Ud, ndiag):
    """G_g = sum_{a+b=g} K_a U_b for g < ndiag over the digits given (float64 matmuls of integers below 2^53: exact)."""
    n = Kd[0].shape[1]
    assert n * 2 ** 14 * min(len(Kd), len(Ud)) < 2 ** 53
    G = [np.zeros((Kd[0].shape[0], Ud[0].shape[1])) for _ in range(ndiag)]
    for a in range(len(Kd)):
        for b in range(len(Ud)):
            if a + b < ndiag:
                G[a + b] += Kd[a] @ Ud[b]
    for g in G:
        assert np.abs(g).max() < 2.0 ** 31, "a diagonal leaves the int32 accumulators"
    return G


def recombine(G, e, keep=None):
    """v_j and S_j from the diagonals (`keep`: the diagonals that take part, default all).  Each term G_g 2^(-12-8g) is
    exact, so a rounded add is the kernel's fma; the power-of-two column scale is exact."""
    v = np.zeros_like(G[0])
    S = np.zeros_like(G[0])
    for g in reversed(range(len(G))):
        if keep is not None and g not in keep:
            continue
        w = 2.0 ** (-12 - 8 * g)
        v = v + G[g] * w
        S = S + np.abs(G[g]) * w
    sc = 2.0 ** np.asarray(e, dtype=np.float64)[None, :]
    return v * sc, S * sc


def sum_squares(v, S):
    """(ssq, tol) per candidate; the sum of squares in extended precision, so that `tol` is all the device's."""
    n = v.shape[1]
    vl = v.astype(np.longdouble)
    ssq = (vl * vl).sum(axis=1).astype(np.float64)
    tol = 2.0 ** -53 * ((n + 4) * ssq + 12.0 * (np.abs(v) * S).sum(axis=1))
    return ssq, tol


def emulate(Ks, U, coarse=False):
    """The variance product of gpbo_posterior_acq_i8 (coarse: gpbo_posterior_acq_i8c): dict(ssq, tol, v, S)."""
    Kd, Ud, e = operands(Ks, U)
    return emulate_digits(Kd, Ud, e, coarse)


def emulate_digits(Kd, Ud, e, coarse=False, keep=None):
    if coarse:
        G = diagonals(Kd[:3], Ud[:3], 3)
    else:
        G = diagonals(Kd[:NK], Ud[:NU], 6)
    v, S = recombine(G, e, keep)
    ssq, tol = sum_squares(v, S)
    return dict(ssq=ssq, tol=tol, v=v, S=S)


# ---- operands shared by the CPU and the GPU tests ---------------------------------------------------------------------
PROBE_A_N, PROBE_A_M, PROBE_A_ROWS = 129, 600, (0, 15, 16, 31, 32, 63, 64, 128)
PROBE_B_SHIFTS = (0, 1, 31, 32, 33, 63, 64, 127)


def probe_a(n0):
    """K* digit probe: U = 0.5 at (n0, n0) alone, so e = 0, T_u = 2^45 (the single digit 32) and
    v = T_k(c, n0) 2^-39 exactly.  dict(N, Np, d, X, Xs, ls, U): candidates 0 .. 45 length scales from X[n0], every
    tenth one on an observation (k == 1.0 at n0 among them); beyond sqrt(2 708) length scales k == 0.0."""
    N, M, Np = PROBE_A_N, PROBE_A_M, 256
    X = np.linspace(0.0, 1.0, N)[:, None]
    Xs = X[n0, 0] + np.linspace(0.0, 45.0, M)[:, None]
    on = np.arange(0, M, 10)
    Xs[on, 0] = X[(n0 + 3 * np.arange(len(on))) % N, 0]
    U = np.zeros((Np, Np))
    U[n0, n0] = 0.5
    return dict(N=N, Np=Np, d=1, M=M, X=X, Xs=Xs, ls=np.ones(1), U=U)


def probe_b(Np, shift):
    """U digit and column-scale probe.  Observations 100 length scales apart, candidate c on observation c mod N: every K*
    row is a unit vector (T_k = 2^38, the single digit 64) and v_j = rint(U_nj 2^(46-e_j)) 2^(e_j-46) exactly.
    Row 0: one pin per column (it fixes e_j, cycling through -40 .. 40); row n >= 1: one carry pattern at column n + shift.
    The last column is all zero; where there is room, one column's maximum is exactly a power of two and one's the double
    just below one (pattern entries, no pin)."""
    N, M = Np, Np + 1
    rng = np.random.default_rng(1000 * Np + shift)
    e = -40 + (np.arange(Np) + shift) % 81
    pin = rng.integers(2 ** 45, 2 ** 46, Np) * rng.choice([-1, 1], Np)
    U = np.zeros((Np, Np))
    U[0] = pin.astype(np.float64) * 2.0 ** (e - U_BITS)
    for n in range(1, Np - shift):
        j = n + shift
        T = CARRY_T[(n - 1 + 5 * shift) % len(CARRY_T)]
        assert abs(T) <= T_MAX
        U[n, j] = float(T) * 2.0 ** (int(e[j]) - U_BITS)
    U[:, Np - 1] = 0.0
    if Np - 3 - shift >= 1:
        jp, jn = Np - 2, Np - 3
        U[:, jp] = 0.0
        U[:, jn] = 0.0
        U[jp - shift, jp] = -(2.0 ** int(e[jp]))                       # e = e[jp] + 1, T = -2^45
        U[jn - shift, jn] = np.nextafter(2.0 ** int(e[jn]), 0.0)       # e = e[jn],     T = rint(2^46 - 2^-7) = 2^46
    X = 100.0 * np.arange(N, dtype=np.float64)[:, None]
    Xs = X[np.arange(M) % N].copy()
    return dict(N=N, Np=Np, d=1, M=M, X=X, Xs=Xs, ls=np.ones(1), U=U)


def planted_u(Np, seed):
    """Dense upper-triangular U of planted fixed-point values: (U, T [Np x Np] int64, e [Np]).  Column exponents from
    [-40, 40]; entries T 2^(e_j - 46) with T uniform in [-(2^46 - 1), 2^46 - 1], a tenth of them from CARRY_T; one pin per
    column with 2^45 <= |T| fixes e_j; NaN below the diagonal (never read)."""
    rng = np.random.default_rng(seed)
    e = rng.integers(-40, 41, Np)
    T = rng.integers(-T_MAX, T_MAX + 1, (Np, Np))
    carry = rng.random((Np, Np)) < 0.1
    T[carry] = rng.choice(np.array(CARRY_T, dtype=np.int64), int(carry.sum()))
    cols = np.arange(Np)
    rows = (rng.random(Np) * (cols + 1)).astype(np.int64)
    T[rows, cols] = rng.integers(2 ** 45, T_MAX + 1, Np) * rng.choice([-1, 1], Np)
    T = np.triu(T)
    assert np.abs(T).max() <= T_MAX
    U = T.astype(np.float64) * 2.0 ** (e - U_BITS)[None, :]
    U[np.tril_indices(Np, -1)] = np.nan
    return U, T, e


#   case: (U, N, d, M, chunk)
CASES = {1: ("planted", 100, 3, 300, 512),     # Np = 128
         2: ("planted", 129, 1, 1030, 512),    # Np = 256, three chunks, ragged last tile
         3: ("factor", 256, 8, 600, 512),      # first 16 candidates on observations
         4: ("factor", 2048, 8, 300, 512)}     # sixteen column blocks: the column-group launch


def padded(N):
    return (N + 127) // 128 * 128


def case_inputs(case, M=None):
    """dict(kind, N, Np, d, M, chunk, X, y, Xs, ls, alpha, U): U is None for a real factor (the GPU test takes the
    device's, the CPU test host_factor())."""
    kind, N, d, M0, chunk = CASES[case]
    M = M0 if M is None else M
    X, y, Xs, ls = make_problem(N, M, d)
    Np = padded(N)
    alpha = np.zeros(Np)
    alpha[:N] = np.random.default_rng(77 + case).standard_normal(N)
    U = None
    if kind == "planted":
        U = planted_u(Np, 31 * case)[0]
    elif case == 3:
        Xs = Xs.copy()
        Xs[:16] = X[:16]
    return dict(kind=kind, N=N, Np=Np, d=d, M=M, chunk=chunk, X=X, y=y, Xs=Xs, ls=ls, alpha=alpha, U=U)


def host_factor(X, y, ls):
    """U = L^-T of the oracle's factorisation, identity on the padding: [Np x Np]."""
    import scipy.linalg as sla

    N = len(X)
    Np = padded(N)
    _, L, _ = O.factorise(X, y, ls)
    U = np.eye(Np)
    U[:N, :N] = sla.solve_triangular(L, np.eye(N), lower=True).T
    return U


def host_kstar(X, Xs, ls, Np):
    """K* [M x Np] on the host (the CPU tests' stand-in for the device's KsT image): zero on the padding."""
    assert len(Xs) != len(X)   # (kernel_rbf adds the reference's 1e-4 diagonal when the two shapes coincide)
    Ks = np.zeros((len(Xs), Np))
    Ks[:, :len(X)] = O.kernel_rbf(Xs, X, ls)
    return Ks
