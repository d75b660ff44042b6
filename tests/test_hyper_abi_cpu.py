"""CPU-only checks of the hyperparameter boundary (csrc/hyper.hip): the contracts of gpbo_nlml_hyper_f64 /
gpbo_nlml_hyper_host_f64 / gpbo_loo_f64 and of the two workspace queries are refused on the host before anything is launched,
the Python layers refuse bad arguments without a GPU, a fresh hyper.hip compiles for gfx950 without scratch and is one of the
units whose barriers are checked."""
import ctypes as C
import os
import re
import shutil
import sys

import numpy as np
import pytest

from bayesian_optimisation_amd import _lib

sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools"))
import check_barriers as cb  # noqa: E402

needs_hipcc = pytest.mark.skipif(shutil.which(cb.HIPCC) is None and not os.path.exists(cb.HIPCC), reason="hipcc not installed")


def _fake_pointer():
    buf = (C.c_char * 1024)()
    return buf, C.c_void_p((C.addressof(buf) + 255) & ~255)   # 256-byte aligned like a device allocation; never dereferenced


def test_workspace_queries():
    lib = _lib.load()
    wh, wl, wg = lib.gpbo_nlml_hyper_workspace_bytes, lib.gpbo_loo_workspace_bytes, lib.gpbo_nlml_grad_workspace_bytes
    for Np in (128, 256, 4096, 8192):
        for d in (1, 8, 16):
            assert wh(Np, d) >= wg(Np, d) + 6 * 8 * Np and wh(Np, d) % 256 == 0   # the gradient's own + six [Np] vectors
        assert wl(Np) >= 8 * Np
    for Np in (0, 100, 64, -128):
        assert wh(Np, 2) == -1 and wl(Np) == -1
    assert wh(128, 0) == -1 and wh(128, 17) == -1


def test_likelihood_entry_point_checks_its_contracts_on_the_host():
    lib = _lib.load()
    buf, p = _fake_pointer()
    ls = (C.c_double * 16)(*([0.5] * 16))
    lsp = C.cast(ls, C.c_void_p)
    need = lib.gpbo_nlml_hyper_workspace_bytes(128, 2)

    def call(U=p, alpha=p, y=p, X=p, N=100, Np=128, d=2, lsp=lsp, noise=1e-2, flags=3, info=p, out=p, astd=None, work=p,
             wbytes=need):
        return lib.gpbo_nlml_hyper_f64(U, alpha, y, X, N, Np, d, lsp, noise, flags, info, out, astd, work, wbytes, None)

    for name in ("U", "alpha", "y", "X", "lsp", "info", "out", "work"):
        assert call(**{name: None}) == -1, name
    for noise in (0.0, -1e-3, float("nan"), float("inf")):
        assert call(noise=noise) == -1, noise
    for flags in (4, 8, 7, -1):
        assert call(flags=flags) == -1, flags
    assert call(d=0) == -1 and call(d=17) == -1
    assert call(Np=256) == -1 and call(Np=100) == -1 and call(N=129) == -1 and call(N=0) == -1
    for bad in ((0.5, 0.0), (-1.0, 0.5), (0.5, float("nan"))):
        assert call(lsp=C.cast((C.c_double * 2)(*bad), C.c_void_p)) == -1, bad
    assert call(U=C.c_void_p(p.value + 8)) == -1 and call(work=C.c_void_p(p.value + 8)) == -1
    # a workspace one byte short: after the arguments, before any HIP call; the optional output changes nothing
    assert call(wbytes=need - 1) == -3 and call(wbytes=0) == -3 and call(astd=p, wbytes=need - 1) == -3
    for flags in (0, 1, 2, 3):
        assert call(flags=flags, wbytes=need - 1) == -3   # every legal flag combination gets as far as the workspace check
    del buf


def test_host_entry_point_checks_its_contracts_on_the_host():
    lib = _lib.load()
    buf, p = _fake_pointer()
    ls = (C.c_double * 16)(*([0.5] * 16))
    lsp = C.cast(ls, C.c_void_p)

    def call(X=p, y=p, N=100, d=2, lsp=lsp, noise=1e-2, flags=3, out=p):
        return lib.gpbo_nlml_hyper_host_f64(X, y, N, d, lsp, noise, flags, out)

    for name in ("X", "y", "lsp", "out"):
        assert call(**{name: None}) == -1, name
    assert call(N=0) == -1 and call(d=0) == -1 and call(d=17) == -1
    for noise in (0.0, -1.0, float("nan"), float("inf")):
        assert call(noise=noise) == -1
    assert call(flags=4) == -1 and call(flags=-1) == -1
    assert call(lsp=C.cast((C.c_double * 2)(0.5, 0.0), C.c_void_p)) == -1
    del buf


def test_leave_one_out_entry_point_checks_its_contracts_on_the_host():
    lib = _lib.load()
    buf, p = _fake_pointer()
    need = lib.gpbo_loo_workspace_bytes(128)

    def call(U=p, alpha=p, y=p, N=100, Np=128, scale2=1.0, mu=p, var=None, kd=None, work=p, wbytes=need):
        return lib.gpbo_loo_f64(U, alpha, y, N, Np, scale2, mu, var, kd, work, wbytes, None)

    for name in ("U", "alpha", "y", "work"):
        assert call(**{name: None}) == -1, name
    assert call(N=0) == -1 and call(N=129) == -1 and call(Np=256) == -1 and call(Np=100) == -1
    for s2 in (0.0, -1.0, float("nan"), float("inf")):
        assert call(scale2=s2) == -1
    assert call(U=C.c_void_p(p.value + 8)) == -1 and call(work=C.c_void_p(p.value + 8)) == -1
    assert call(wbytes=need - 1) == -3 and call(mu=None, wbytes=need - 1) == -3   # (every output is optional)
    del buf


def test_python_constants_and_prototypes_match_the_header():
    repo = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    src = open(os.path.join(repo, "include", "gpbo.h")).read()
    defs = {k: int(v) for k, v in re.findall(r"#define\s+(GPBO_[A-Z_]+)\s+\(?(-?\d+)\)?", src)}
    assert defs["GPBO_HYPER_MEAN"] == _lib.HYPER_MEAN == 1 and defs["GPBO_HYPER_SCALE"] == _lib.HYPER_SCALE == 2
    assert defs["GPBO_VERSION"] == 151 and _lib.load().gpbo_version() == 151
    for name in ("gpbo_nlml_hyper_workspace_bytes", "gpbo_nlml_hyper_f64", "gpbo_nlml_hyper_host_f64", "gpbo_loo_workspace_bytes",
                 "gpbo_loo_f64"):
        assert name in _lib.SIGNATURES and name in src


def test_python_layers_refuse_bad_arguments_without_a_gpu():
    from bayesian_optimisation_amd import host_binding as H
    from bayesian_optimisation_amd.host_binding import PointSelectorHost
    from bayesian_optimisation_amd.point_selector import PointSelector

    X, y = np.zeros((4, 2)), np.zeros(4)
    with pytest.raises(ValueError):
        H.nlml_hyper(X, y, [1.0], 1e-2)                          # shapes
    for noise in (0.0, -1.0, float("nan"), float("inf")):
        with pytest.raises(ValueError):
            H.nlml_hyper(X, y, [1.0, 1.0], noise)
    with pytest.raises(ValueError):
        H.nlml_hyper(np.zeros((4, 17)), y, np.ones(17), 1e-2)     # d = 17
    with pytest.raises(ValueError):
        H.nlml_hyper(X, y, [1.0, 0.0], 1e-2)
    for kw in (dict(precision="fp32"), dict(incremental=True), dict(state_path="s.npz"), dict(dense_outputs=False),
               dict(noise0=0.0), dict(noise0=2.0), dict(noise_bounds=(0.0, 1.0)), dict(noise_bounds=(1.0, 1e-6))):
        with pytest.raises(ValueError):
            PointSelector(ard="hyper", **kw)
    with pytest.raises(ValueError):
        PointSelector(ard="everything")
    ps = PointSelectorHost(ard="hyper")
    assert ps.noise is None and ps.y_mean is None and ps.y_scale is None
    for call in (lambda: ps.select_batch(2), lambda: ps.select_thompson(2), lambda: ps.refine_next(),
                 lambda: ps.q_expected_improvement(), lambda: ps.loo()):
        with pytest.raises(ValueError):
            call()


@needs_hipcc
def test_a_fresh_hyper_unit_compiles_for_gfx950_without_scratch(tmp_path):
    asm = open(cb.assemble("hyper", str(tmp_path))).read()
    sizes = {re.search(r"\.name:\s+(\S+)", b).group(1): int(re.search(r"\.private_segment_fixed_size:\s+(\d+)", b).group(1))
             for b in asm.split("  - .agpr_count:")[1:]}
    for kernel in ("hyper_rowsum_kernel", "hyper_profile_kernel", "hyper_finish_kernel", "loo_kernel"):
        assert any(kernel in k for k in sizes), sorted(sizes)
    assert max(sizes.values()) == 0, sizes
    assert "global_atomic" not in asm and "flat_atomic" not in asm   # no atomics in any sum


@needs_hipcc
def test_the_unit_is_barrier_checked(capsys):
    assert "hyper" in cb.UNITS
    rc = cb.main(["hyper"])
    out = capsys.readouterr().out
    assert rc == 0, out
    assert "0 reachable" in out
