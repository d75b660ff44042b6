"""CPU-only checks of what ard="marginal" adds at the boundary: the new entry points are declared, bound and refuse bad arguments
on the host; the size limits are mirrored in Python; the selector classes refuse what the mode does not support; the wave-per-cell
kernel of csrc/hyper_wave.hip keeps its matrix in registers."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from bayesian_optimisation_amd import _lib

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("gpbo_nlml_hyper_cells_f64", "gpbo_ensemble_workspace_bytes", "gpbo_ensemble_acq_f64")


def _aligned():
    buf = (C.c_char * 1024)()
    return buf, C.c_void_p((C.addressof(buf) + 255) & ~255)   # 256-byte aligned like a device allocation; never dereferenced


def test_the_new_entry_points_are_declared_exported_and_bound():
    src = open(os.path.join(REPO, "include", "gpbo.h")).read()
    lib = _lib.load()            # (first: the loader binds the library to PyTorch's HIP runtime)
    raw = C.CDLL(_lib.LIB_PATH)
    for name in NEW:
        assert re.search(r"\b" + name + r"\s*\(", src), f"{name} is not declared in include/gpbo.h"
        assert hasattr(raw, name) and name in _lib.SIGNATURES
    assert lib.gpbo_version() == 151
    defs = {k: int(v) for k, v in re.findall(r"#define\s+(GPBO_[A-Z_]+)\s+\(?(-?\d+)\)?", src)}
    assert defs["GPBO_HYPER_CELLS_MAX_N"] == _lib.HYPER_CELLS_MAX_N == 64
    assert defs["GPBO_ENSEMBLE_MAX_S"] == _lib.ENSEMBLE_MAX_S == 64
    # no new function of no arguments that returns int (test_every_compute_entry_point_rejects_null_arguments would call it)
    assert all(_lib.SIGNATURES[n][1] for n in NEW)


def test_all_null_arguments_are_refused():
    lib = _lib.load()
    for name in ("gpbo_nlml_hyper_cells_f64", "gpbo_ensemble_acq_f64"):
        res, args = _lib.SIGNATURES[name]
        assert res is C.c_int
        a = [None if t is C.c_void_p else (0.0 if t is C.c_double else 0) for t in args]
        assert getattr(lib, name)(*a) == -1, name
    assert lib.gpbo_ensemble_workspace_bytes(0, 0, 0) == -1


def test_size_contracts_of_the_cells_likelihood():
    lib = _lib.load()
    _, p = _aligned()

    def cells(N=20, d=2, G=4, kernel=0, flags=3):
        return lib.gpbo_nlml_hyper_cells_f64(p, p, N, d, p, G, kernel, flags, p, None)

    assert cells(N=65) == -1 and cells(N=0) == -1
    assert cells(d=17) == -1 and cells(d=0) == -1
    assert cells(G=0) == -1 and cells(G=(1 << 28) + 1) == -1
    assert cells(kernel=3) == -1 and cells(kernel=-1) == -1
    assert cells(flags=4) == -1


def test_size_contracts_of_the_ensemble():
    lib = _lib.load()
    _, p = _aligned()
    S_MAX = _lib.ENSEMBLE_MAX_S
    ls = (C.c_double * (16 * (S_MAX + 1)))(*([0.5] * (16 * (S_MAX + 1))))
    model = np.ascontiguousarray(np.tile([1.0 / 4, 1.01, 40.0, 7.0], (S_MAX + 1, 1)))
    need = lib.gpbo_ensemble_workspace_bytes(128, 512, 1000)
    assert need > lib.gpbo_posterior_workspace_bytes(128, 512, 1000) + 5 * 8 * 1000
    assert lib.gpbo_ensemble_workspace_bytes(100, 512, 1000) == -1 and lib.gpbo_ensemble_workspace_bytes(128, 500, 1000) == -1
    assert lib.gpbo_ensemble_workspace_bytes(128, 512, 0) == -1

    def ens(S=4, N=100, Np=128, d=2, M=1000, chunk=512, kind=0, kernel=0, mod=model, lsp=ls, work=p, wbytes=need, U=p):
        return lib.gpbo_ensemble_acq_f64(p, M, p, N, Np, d, S, C.cast(lsp, C.c_void_p), kernel, U, p,
                                         mod.ctypes.data_as(C.c_void_p), kind, 4.0, 0.0, 0, chunk, None, None, None, p, work,
                                         wbytes, None)

    assert ens(S=0) == -1 and ens(S=S_MAX + 1) == -1
    assert ens(d=17) == -1 and ens(d=0) == -1
    assert ens(Np=256) == -1 and ens(M=0) == -1 and ens(chunk=500) == -1 and ens(kind=7) == -1 and ens(kernel=3) == -1
    neg = model.copy()
    neg[2, 0] = -0.25
    assert ens(mod=neg) == -1                                   # a negative weight
    zero = model.copy()
    zero[:, 0] = 0.0
    assert ens(mod=zero) == -1                                  # no weight at all
    for col, v in ((1, 0.0), (3, 0.0), (3, -1.0), (2, np.inf), (0, np.nan)):
        bad = model.copy()
        bad[1, col] = v
        assert ens(mod=bad) == -1, (col, v)
    bad_ls = (C.c_double * 32)(*([0.5] * 5 + [0.0] + [0.5] * 26))
    assert ens(lsp=bad_ls) == -1                                # a length scale of model 2 that is not positive
    assert ens(U=C.c_void_p(p.value + 8)) == -1                 # U is read by 16-byte pieces
    assert ens(wbytes=need - 1) == -3 and ens(wbytes=8) == -3   # a short workspace
    assert ens(work=C.c_void_p(p.value + 128)) == -3            # or one that is not 256-byte aligned


def test_constructor_refusals_of_the_marginal_mode():
    from bayesian_optimisation_amd import PointSelector, PointSelectorHost

    for kw in (dict(precision="fp32"), dict(incremental=True), dict(state_path="s.npz"), dict(dense_outputs=False)):
        with pytest.raises(ValueError, match="marginal"):
            PointSelector(ard="marginal", **kw)
    for kw in (dict(n_models=0), dict(n_models=65), dict(n_models=2.5), dict(posterior_sweeps=-1)):
        with pytest.raises(ValueError):
            PointSelector(ard="marginal", **kw)
    with pytest.raises(ValueError, match="PointSelector"):
        PointSelectorHost(ard="marginal")
    ps = PointSelector(ard="marginal", n_models=8, posterior_sweeps=3, seed=5)
    assert ps.hyper_samples is None and ps.noise is None
    for call, name in ((lambda: ps.q_expected_improvement(), "q_expected_improvement"), (lambda: ps.select_batch(2), "select_batch"),
                       (lambda: ps.select_thompson(2), "select_thompson"), (lambda: ps.refine_next(), "refine_next")):
        with pytest.raises(ValueError, match="ard='marginal'") as e:
            call()
        assert name in str(e.value)
    with pytest.raises(ValueError):
        PointSelector(ard="integrated")
    # the other modes keep their constructor and take the new keywords without using them
    assert PointSelector(ard="hyper", n_models=4)._ard == "hyper" and PointSelector()._ard == "grid"


@pytest.fixture(scope="module")
def assembly(tmp_path_factory):
    """gfx950 assembly of the two new translation units, compiled once for the tests below: {unit: path}."""
    import sys

    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    if not os.path.exists(hipcc):
        pytest.skip("no hipcc in this environment")
    sys.path.insert(0, os.path.join(REPO, "tools"))
    import check_barriers as cb

    out = str(tmp_path_factory.mktemp("asm"))
    return cb, {unit: cb.assemble(unit, out) for unit in ("hyper_wave", "ensemble")}


def test_the_new_translation_units_are_built_and_checked_for_barriers(assembly):
    cb, paths = assembly
    build = open(os.path.join(REPO, "bayesian_optimisation_amd", "csrc", "build.sh")).read()
    barriers = 0
    for unit, path in paths.items():
        assert unit in cb.UNITS and f" {unit} " in build and f"build/{unit}.o" in build
        found, n = cb.check_file(path)
        assert found == [], found
        barriers += n
    assert barriers >= 48 + 2   # one per hyper_wave instance, one per finishing instance of the fold kernel


def test_the_wave_per_cell_hyper_likelihood_keeps_its_matrix_in_registers(assembly):
    """csrc/hyper_wave.hip holds a cell's matrix in registers like csrc/ard_wave.hip, whose allocation proved fragile; here the
    three sums of the profile, written as wave-uniform accumulators inside the elimination, doubled the registers (238 for 123
    at NMAX = 48) and spilled at NMAX = 32 and 64.  No instance may need more than a few bytes of scratch, and every family has
    its instances: 4 sizes x 4 feature counts x 3 families."""
    s = open(assembly[1]["hyper_wave"]).read()
    sizes = {re.search(r"\.name:\s+(\S+)", b).group(1): int(re.search(r"\.private_segment_fixed_size:\s+(\d+)", b).group(1))
             for b in s.split("  - .agpr_count:")[1:]}
    waves = {k: v for k, v in sizes.items() if "hyper_wave_kernel" in k}
    assert len(waves) == 48, sorted(sizes)
    assert max(waves.values()) <= 16, waves
