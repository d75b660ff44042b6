"""Writes tests/golden/cons_terms.npz: log h(z), h(z) = phi(z) + z Phi(z) - expected improvement is sigma h(z) - of the constrained
acquisitions (csrc/cons_math.h) at 60 digits with mpmath, rounded to float64.  z: 2001 points on [-40, 40] and -1e2, -3e2, -999,
-1e3, -1e4, -1e6.  (log Phi is in mes_terms.npz.)  The tests read the fixture and never mpmath.
usage: python tests/golden/make_constrained_golden.py"""
import os

import mpmath as mp
import numpy as np

mp.mp.dps = 60


def log_h(z):
    # h = phi (1 + z Phi / phi): for z << 0 the bracket is ~ 1 / z^2 and its sum loses log10(z^2) of the 60 digits (12 at -1e6);
    # erfc of a large argument in mpmath keeps its relative accuracy (no underflow), so the ratio Phi / phi is formed first
    log_pdf = -z * z / 2 - mp.log(2 * mp.pi) / 2
    if z >= 0:
        return mp.log(mp.exp(log_pdf) + z * (1 - mp.erfc(z / mp.sqrt(2)) / 2))
    ratio = mp.erfc(-z / mp.sqrt(2)) / 2 / mp.exp(log_pdf)   # Phi / phi, of order 1 / |z|
    return log_pdf + mp.log(1 + z * ratio)


def main():
    z = np.concatenate([np.linspace(-40.0, 40.0, 2001), [-1e2, -3e2, -999.0, -1e3, -1e4, -1e6]])
    lh = np.array([float(log_h(mp.mpf(float(v)))) for v in z])
    out = os.path.join(os.path.dirname(os.path.abspath(__file__)), "cons_terms.npz")
    np.savez(out, z=z, log_h=lh)
    print(out, z.size, "points")


if __name__ == "__main__":
    main()
