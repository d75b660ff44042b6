"""Diagnostic (needs a diagnostics build of the library, loaded through GPBO_LIB; GPBO_SIGMA_VARIANT = 6, 9, 11, 12, 13 or 15:
the product loop, or the timing variants 1 / 3 / 4 / 5 / 7, with per-tile stamps): per-tile s_memtime stamps of the variance
kernel's LAST launch at a shape that takes the column-group launches (N >= 2048, M >= 32768).  Prints the median
duration of a FULL k tile (left of the diagonal block) and of a diagonal tile, in stamp ticks, over all workgroups.
Stamped builds are compared with each other only (a stamp costs wave cycles).
usage: GPBO_LIB=ab_libs/diag_sigma.so GPBO_SIGMA_VARIANT=6 python tools/tile_stamps_groups.py [N]"""
import os, sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
from bayesian_optimisation_amd import DeviceGP
from bayesian_optimisation_amd.synthetic import make_problem

N = int(sys.argv[1]) if len(sys.argv) > 1 else 4096
chunk, xg = 1 << 17, 8
M = 2 * chunk
X, y, Xs, ls = make_problem(N, M, 8)
gp = DeviceGP(chunk=chunk).factorise(X, y, ls)
for _ in range(2):
    gp.score(Xs)
nJ = gp.Np // 128
assert nJ >= 2 * xg
nwg = chunk // 256 * xg
raw = gp._work_post[: nwg * 1024].cpu().numpy().reshape(nwg, 1024)   # the stamps of the last chunk lie in chunk buffer 0
full, diag = [], []
for wg in range(nwg):
    sp = (wg >> 3) % xg
    kinds = []
    for r in range(nJ // xg):
        jb = r * xg + ((xg - 1 - sp) if (r & 1) else sp)
        kinds += [True] * (8 * jb) + [False] * 8
    T = len(kinds)
    d = np.diff(raw[wg, :T])
    kk = np.array(kinds[:-1])
    full.append(d[kk][4:])      # (the first tiles of a workgroup start beside the prologue of the others)
    diag.append(d[~kk])
full, diag = np.concatenate(full), np.concatenate(diag)
print(f"variant {os.environ.get('GPBO_SIGMA_VARIANT')}: N={N} workgroups={nwg} full tiles: median {np.median(full):.0f} "
      f"mean {np.mean(full):.0f} p10 {np.percentile(full, 10):.0f} p90 {np.percentile(full, 90):.0f} ticks; "
      f"diagonal tiles: median {np.median(diag):.0f}")
sp0 = raw[raw[:, 1001] > 0]
if len(sp0):
    T0 = 8 * sum(r * xg + ((xg - 1) if (r & 1) else 0) + 1 for r in range(nJ // xg))
    ratio = (sp0[:, T0 - 1] - sp0[:, 0]) / (sp0[:, 1001] - sp0[:, 1000])
    print(f"stamp ticks per 100-MHz tick: median {np.median(ratio):.3f}")
