"""Writes tests/golden/mes_terms.npz: log Phi(gamma) and h(gamma) = gamma phi(gamma) / (2 Phi(gamma)) - log Phi(gamma) of max-value
entropy search (csrc/mes_math.h) at 60 digits with mpmath, rounded to float64.  gamma: 2001 points on [-40, 40] and -1e2, -1e3,
-1e4.  The tests read the fixture and never mpmath.      usage: python tests/golden/make_mes_golden.py"""
import os

import mpmath as mp
import numpy as np

mp.mp.dps = 60


def log_ndtr(g):
    # erfc of a large argument in mpmath keeps its relative accuracy (no underflow); above 0, 1 - Phi falls below 1e-60 from
    # gamma ~ 16 on, so the logarithm is taken of 1 + (-(1 - Phi))
    if g > 0:
        return mp.log1p(-mp.erfc(g / mp.sqrt(2)) / 2)
    return mp.log(mp.erfc(-g / mp.sqrt(2)) / 2)


def h(g):
    lp = log_ndtr(g)
    log_pdf = -g * g / 2 - mp.log(2 * mp.pi) / 2
    return g * mp.exp(log_pdf - lp) / 2 - lp


def main():
    gamma = np.concatenate([np.linspace(-40.0, 40.0, 2001), [-1e2, -1e3, -1e4]])
    lp = np.array([float(log_ndtr(mp.mpf(float(g)))) for g in gamma])
    hh = np.array([float(h(mp.mpf(float(g)))) for g in gamma])
    out = os.path.join(os.path.dirname(os.path.abspath(__file__)), "mes_terms.npz")
    np.savez(out, gamma=gamma, log_ndtr=lp, h=hh)
    print(out, gamma.size, "points")


if __name__ == "__main__":
    main()
