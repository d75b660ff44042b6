"""Writes tests/golden/ehvi_cases.npz: log EHVI of two minimised objectives at 60 digits (mpmath 1.3.0), rounded to fp64 once.

    python tests/golden/make_ehvi_golden.py

Eight fronts - P = 0, 1, 2, 7 (spacings 1e-3, about 1, and 10) and 128 (spacings 1e-3 and 0.05) - with 40 candidates each: means
spread up to 30 around the front with sigma log-uniform in [0.01, 2], candidates 40 to 60 sigma beyond the reference point in both
objectives (the plain fp64 sum is exactly 0 there), and a few with sigma == 0 in one objective or both.  The tests read the file and
never mpmath.  Keys: front_<k> [P x 2], ref [8 x 2], and per case fid, mu1, s1, mu2, s2, want (log EHVI; -inf where EHVI is 0).
"""
import os

import mpmath as mp
import numpy as np

mp.mp.dps = 60
PER_FRONT = 40


def make_front(rng, P, step):
    a = np.cumsum(step * (1.0 + rng.random(P)))
    c = -np.cumsum(step * (1.0 + rng.random(P)))
    F = np.stack([a, c], axis=1).reshape(-1, 2)
    span = max(step * max(P, 1), 0.5)
    ref = (float(a[-1] if P else 0.0) + 0.37 * span, 0.41 * span)
    return F, ref


def g(level, mu, sigma):
    level, mu, sigma = mp.mpf(level), mp.mpf(mu), mp.mpf(sigma)
    if sigma == 0:
        return max(level - mu, mp.mpf(0))
    z = (level - mu) / sigma
    return sigma * (mp.npdf(z) + z * mp.ncdf(z))


def log_ehvi(mu1, s1, mu2, s2, F, ref):
    edge = [float(v) for v in F[:, 0]] + [ref[0]]
    ceil = [ref[1]] + [float(v) for v in F[:, 1]]
    total, prev = mp.mpf(0), mp.mpf(0)
    for a, c in zip(edge, ceil):
        g1 = g(a, mu1, s1)
        total += (g1 - prev) * g(c, mu2, s2)
        prev = g1
    return float(mp.log(total)) if total > 0 else -np.inf


def main():
    rng = np.random.default_rng(20260416)
    shapes = [(0, 1.0), (1, 1.0), (2, 0.7), (7, 1.0e-3), (7, 1.0), (7, 10.0), (128, 1.0e-3), (128, 0.05)]
    out, refs, rows = {}, [], []
    for k, (P, step) in enumerate(shapes):
        F, ref = make_front(rng, P, step)
        out[f"front_{k}"] = F
        refs.append(ref)
        lo1, lo2 = (F[0, 0], F[-1, 1]) if P else (ref[0] - 1.0, ref[1] - 1.0)
        for j in range(PER_FRONT):
            s1, s2 = (float(np.exp(rng.uniform(np.log(0.01), np.log(2.0)))) for _ in range(2))
            if j < 24:      # around the front, up to 30 away
                spread = (0.5, 3.0, 30.0)[j % 3]
                mu1, mu2 = rng.uniform(lo1 - spread, ref[0] + spread), rng.uniform(lo2 - spread, ref[1] + spread)
            elif j < 34:    # 40 to 60 sigma beyond the reference point in both objectives
                mu1, mu2 = ref[0] + rng.uniform(40.0, 60.0) * s1, ref[1] + rng.uniform(40.0, 60.0) * s2
            else:           # sigma == 0 in one objective or both
                mu1, mu2 = rng.uniform(lo1 - 0.5, ref[0] + 0.2), rng.uniform(lo2 - 0.5, ref[1] + 0.2)
                s1, s2 = (0.0, s2) if j % 3 == 0 else ((s1, 0.0) if j % 3 == 1 else (0.0, 0.0))
            rows.append((k, mu1, s1, mu2, s2, log_ehvi(mu1, s1, mu2, s2, F, ref)))
    rows = np.array(rows, dtype=np.float64)
    out.update(ref=np.array(refs), fid=rows[:, 0].astype(np.int32), mu1=rows[:, 1], s1=rows[:, 2], mu2=rows[:, 3], s2=rows[:, 4],
               want=rows[:, 5])
    np.savez_compressed(os.path.join(os.path.dirname(os.path.abspath(__file__)), "ehvi_cases.npz"), **out)


if __name__ == "__main__":
    main()
