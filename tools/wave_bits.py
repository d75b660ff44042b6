"""The bits of the two wave-per-cell likelihood kernels (csrc/ard_wave.hip, csrc/hyper_wave.hip over csrc/wave_cell.h), as one
JSON object of SHA-256 digests of the output bytes: the before / after record of a change that must not move a number.  Run it
once per library on the same machine (GPBO_LIB=<library> selects it, as in every tool) and compare the outputs key for key.

  grid.*    gpbo_nlml_grid_wave_f64 (float32 cells) and gpbo_nlml_grid_wave_logdet_f64 (float64), squared exponential
  cells.*   gpbo_nlml_hyper_cells_f64, the three covariance families, the four flag pairs
at N = 1 ... 64 on both sides of every compiled size, every compiled feature count and d below it, G = 1, 5 and 2,500 cells; one
cell of every call is not positive definite (a NaN length scale in the grid, rho = -1.5 in the cells).  Inputs:
synthetic.make_problem(N, 8, d) and a seeded cell table; nothing outside the repository is read.

    python tools/wave_bits.py [output.json]        (prints the object; also written to output.json when given)
"""
import hashlib
import json
import os
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
import numpy as np  # noqa: E402
import torch  # noqa: E402

from bayesian_optimisation_amd import DeviceGP  # noqa: E402
from bayesian_optimisation_amd.synthetic import make_problem  # noqa: E402

NS = (1, 2, 15, 16, 17, 31, 32, 33, 47, 48, 49, 63, 64)
DS = {0: (1, 2, 3, 4, 5, 8, 9, 16), 1: (1, 4, 16), 2: (1, 4, 16)}   # kernel id (se, matern32, matern52) -> feature counts
GS = (1, 5, 2500)
JITTER = 1e-4
FINITE = [0, 0]   # (finite values, values) over all outputs: reported, so that a run of NaNs alone cannot pass for agreement


def digest(t):
    a = np.ascontiguousarray(t.cpu().numpy())
    FINITE[0] += int(np.isfinite(a).sum())
    FINITE[1] += a.size
    return f"{a.dtype}{list(a.shape)}:{hashlib.sha256(a.tobytes()).hexdigest()}"


def main():
    gp = DeviceGP(device="cuda:0")
    lib, st, f64 = gp.lib, gp._stream(), dict(dtype=torch.float64, device=gp.device)
    out = {}
    for N in NS:
        for kid, ds in DS.items():
            for d in ds:
                X, y, _, ls = make_problem(N, 8, d)
                Xd, yd = gp._dev(X), gp._dev(y)
                for G in GS:
                    rng = np.random.default_rng([N, d, G])
                    cells = np.concatenate([ls[None, :] * np.exp(rng.uniform(-0.5, 0.5, (G, d))),
                                            np.exp(rng.uniform(np.log(1e-4), np.log(3e-2), (G, 1)))], axis=1)
                    grid = np.ascontiguousarray(cells[:, :d])
                    cells[G // 2, d] = -1.5          # K0 - 1.5 I: the first pivot is negative
                    grid[G // 2, 0] = np.nan         # every entry of the row build is NaN
                    cd, gd = gp._dev(cells), gp._dev(grid)
                    if kid == 0:
                        for name, fn, dtype in (("f32", lib.gpbo_nlml_grid_wave_f64, torch.float32),
                                                ("logdet", lib.gpbo_nlml_grid_wave_logdet_f64, torch.float64)):
                            o = torch.full((G,), 7.0, dtype=dtype, device=gp.device)
                            rc = fn(gp._ptr(Xd), gp._ptr(yd), N, d, gp._ptr(gd), G, JITTER, gp._ptr(o), st)
                            assert rc == 0, rc
                            out[f"grid.{name}.N{N}.d{d}.G{G}"] = digest(o)
                    for flags in range(4):
                        o = torch.full((G, 3), 7.0, **f64)
                        rc = lib.gpbo_nlml_hyper_cells_f64(gp._ptr(Xd), gp._ptr(yd), N, d, gp._ptr(cd), G, kid, flags, gp._ptr(o), st)
                        assert rc == 0, rc
                        out[f"cells.k{kid}.f{flags}.N{N}.d{d}.G{G}"] = digest(o)
    out["finite_values_of"] = FINITE
    text = json.dumps(out, indent=1, sort_keys=True)
    print(text)
    if len(sys.argv) > 1:
        with open(sys.argv[1], "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
