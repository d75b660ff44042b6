"""CPU-only checks of the Thompson-sampling boundary (csrc/thompson.hip): the size contracts of gpbo_thompson_weights_f64 /
gpbo_thompson_paths_f64 / gpbo_thompson_host_f64 and of the two workspace queries are refused on the host before anything is
launched, the Python layers refuse bad arguments without a GPU, and no instance of the compiled hot kernel needs scratch or
has a barrier reachable with an LDS write in flight."""
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
    wp, ww = lib.gpbo_thompson_paths_workspace_bytes, lib.gpbo_thompson_weights_workspace_bytes
    assert wp(128, 1000, 64, 16) > 0 and ww(128, 64, 16) > 0
    assert wp(4096, 1 << 21, 2048, 64) > 0 and ww(4096, 2048, 64) > 0
    for S in (0, 65):
        assert wp(128, 1000, 64, S) == -1 and ww(128, 64, S) == -1
    for F in (0, 16385):
        assert wp(128, 1000, F, 16) == -1 and ww(128, F, 16) == -1
    assert wp(100, 1000, 64, 16) == -1 and ww(100, 64, 16) == -1 and wp(0, 1000, 64, 16) == -1      # Np granule
    assert wp(128, 0, 64, 16) == -1 and wp(128, -5, 64, 16) == -1                                   # M < 1
    assert wp(128, 1000, 16384, 64) > 0 and ww(128, 16384, 64) > 0                                  # the maxima are legal
    prev_p = prev_w = 0
    for S in range(1, 65):
        p, w = wp(256, 4096, 512, S), ww(256, 512, S)
        assert p >= prev_p and w >= prev_w and p % 256 == 0 and w % 256 == 0
        prev_p, prev_w = p, w
    # the weights workspace holds a paths workspace for the observations as points
    assert ww(256, 512, 16) > wp(256, 256, 512, 16)


def test_paths_entry_point_checks_its_size_contracts_on_the_host():
    lib = _lib.load()
    buf, p = _fake_pointer()
    ls = (C.c_double * 16)(*([0.5] * 16))
    lsp = C.cast(ls, C.c_void_p)
    need = lib.gpbo_thompson_paths_workspace_bytes(128, 1000, 64, 16)

    def call(M=1000, N=100, Np=128, d=2, lsp=lsp, V=p, F=64, S=16, f_out=None, ldf=0, idx=p, work=p, wbytes=need):
        return lib.gpbo_thompson_paths_f64(p, M, p, N, Np, d, lsp, p, p, p, V, F, S, 0, f_out, ldf, idx, p, p, work, wbytes, None)

    assert call(d=0) == -1 and call(d=17) == -1
    assert call(F=0) == -1 and call(F=16385) == -1
    assert call(S=0) == -1 and call(S=65) == -1
    assert call(M=0) == -1
    assert call(f_out=p, ldf=999) == -1                         # a dense output narrower than M
    bad = (C.c_double * 2)(0.5, 0.0)
    assert call(lsp=C.cast(bad, C.c_void_p)) == -1
    nan = (C.c_double * 2)(0.5, float("nan"))
    assert call(lsp=C.cast(nan, C.c_void_p)) == -1
    assert call(Np=100) == -1 and call(N=129) == -1 and call(N=0) == -1   # Np granule, N > Np
    assert call(idx=None) == -1 and call(work=None) == -1 and call(lsp=None) == -1
    # a workspace one byte short, or not 256-byte aligned: after the arguments, before any HIP call
    assert call(wbytes=need - 1) == -3
    assert call(work=C.c_void_p(p.value + 8)) == -3
    assert call(f_out=p, ldf=1000, wbytes=need - 1) == -3
    # V == NULL alone is legal (the prior paths): it gets as far as the workspace check
    assert call(V=None, wbytes=need - 1) == -3
    del buf


def test_weights_entry_point_checks_its_size_contracts_on_the_host():
    lib = _lib.load()
    buf, p = _fake_pointer()
    ls = (C.c_double * 16)(*([0.5] * 16))
    lsp = C.cast(ls, C.c_void_p)
    need = lib.gpbo_thompson_weights_workspace_bytes(128, 64, 16)

    def call(N=100, Np=128, d=2, lsp=lsp, U=p, j1=1e-4, j2=1e-6, F=64, S=16, V=p, work=p, wbytes=need):
        return lib.gpbo_thompson_weights_f64(p, p, N, Np, d, lsp, U, j1, j2, p, p, p, p, F, S, V, work, wbytes, None)

    assert call(d=0) == -1 and call(d=17) == -1
    assert call(F=0) == -1 and call(F=16385) == -1 and call(S=0) == -1 and call(S=65) == -1
    assert call(Np=100) == -1 and call(N=129) == -1 and call(N=0) == -1
    bad = (C.c_double * 2)(0.0, 0.5)
    assert call(lsp=C.cast(bad, C.c_void_p)) == -1
    assert call(V=None) == -1 and call(U=None) == -1 and call(work=None) == -1
    assert call(U=C.c_void_p(p.value + 8)) == -1                # the GEMM's operand must be 16-byte aligned
    assert call(j1=-1.0) == -1 and call(j1=float("nan")) == -1  # kappa = jitter1 + jitter2 is a variance
    assert call(wbytes=need - 1) == -3
    assert call(work=C.c_void_p(p.value + 8)) == -3
    del buf


def test_host_entry_point_checks_its_size_contracts_on_the_host():
    lib = _lib.load()
    buf, p = _fake_pointer()
    ls = (C.c_double * 16)(*([0.5] * 16))
    lsp = C.cast(ls, C.c_void_p)

    def call(M=1000, N=100, d=2, lsp=lsp, F=64, S=16, idx=p, info=p):
        return lib.gpbo_thompson_host_f64(p, p, N, d, lsp, 1e-4, 1e-6, p, M, p, p, p, p, F, S, idx, p, p, None, info)

    assert call(d=0) == -1 and call(d=17) == -1
    assert call(F=0) == -1 and call(F=16385) == -1 and call(S=0) == -1 and call(S=65) == -1
    assert call(M=0) == -1 and call(N=0) == -1
    bad = (C.c_double * 2)(0.5, -1.0)
    assert call(lsp=C.cast(bad, C.c_void_p)) == -1
    assert call(idx=None) == -1 and call(info=None) == -1
    del buf


def test_python_constants_match_the_header():
    repo = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    src = open(os.path.join(repo, "include", "gpbo.h")).read()
    defs = {k: int(v) for k, v in re.findall(r"#define\s+(GPBO_[A-Z_]+)\s+\(?(-?\d+)\)?", src)}
    assert defs["GPBO_TS_MAX_PATHS"] == _lib.TS_MAX_PATHS == 64
    assert defs["GPBO_TS_MAX_FEATURES"] == _lib.TS_MAX_FEATURES == 16384
    assert defs["GPBO_VERSION"] == 151 and _lib.load().gpbo_version() == 151
    for name in ("gpbo_thompson_weights_workspace_bytes", "gpbo_thompson_weights_f64", "gpbo_thompson_paths_workspace_bytes",
                 "gpbo_thompson_paths_f64", "gpbo_thompson_host_f64"):
        assert name in _lib.SIGNATURES and name in src


def test_python_layers_refuse_bad_arguments_without_a_gpu():
    from bayesian_optimisation_amd import host_binding as H
    from bayesian_optimisation_amd import thompson as TS

    assert TS.select_params(4, None, 2048, 0) == (4, 8, 2048, 0)
    assert TS.select_params(40, None, 64, 3)[1] == 64            # n_paths defaults to min(64, 2 q)
    assert TS.path_params(np.int64(3), 16384, 0) == (3, 16384, 0)
    for bad in (dict(q=0), dict(q=65), dict(q=2.0), dict(q=True), dict(q="2"), dict(q=3, n_paths=2), dict(q=2, n_paths=0),
                dict(q=2, n_paths=65), dict(q=2, n_paths=4.0), dict(q=2, n_features=0), dict(q=2, n_features=16385),
                dict(q=2, n_features=2048.0), dict(q=2, seed=-1), dict(q=2, seed=1.5), dict(q=2, seed=None)):
        kw = dict(n_paths=None, n_features=2048, seed=0)
        kw.update(bad)
        with pytest.raises(ValueError):
            TS.select_params(**kw)
    X, y, Xs = np.zeros((4, 2)), np.zeros(4), np.zeros((10, 2))
    for kw in (dict(q=0), dict(q=11), dict(q=2, n_paths=1), dict(q=2, n_features=0), dict(q=2, seed=0.5), dict(q=2.5)):
        with pytest.raises(ValueError):
            H.select_thompson(X, y, [1.0, 1.0], Xs, **kw)
    with pytest.raises(ValueError):
        H.select_thompson(np.zeros((4, 17)), y, np.ones(17), np.zeros((10, 17)), q=2)                # d = 17
    with pytest.raises(ValueError):
        H.select_thompson(X, y, [1.0, 1.0], np.zeros((10, 3)), q=2)                                  # shapes


def _kernel_sizes(asm):
    return {re.search(r"\.name:\s+(\S+)", b).group(1): int(re.search(r"\.private_segment_fixed_size:\s+(\d+)", b).group(1))
            for b in asm.split("  - .agpr_count:")[1:]}


@needs_hipcc
def test_no_instance_of_the_paths_kernel_needs_scratch(tmp_path):
    """A fresh csrc/thompson.hip compiles for gfx950 and no instance of the hot kernel (d = 1 .. 16 x the two path-group
    sizes) spills: two candidates' coordinates and 2 x 16 path accumulators stay in registers."""
    sizes = _kernel_sizes(open(cb.assemble("thompson", str(tmp_path))).read())
    hot = {k: v for k, v in sizes.items() if "thompson_paths_kernel" in k}
    assert len(hot) == 32, sorted(sizes)
    for D in range(1, 17):
        for G in (4, 16):
            assert any(f"ILi{D}ELi{G}E" in k for k in hot), (D, G)
    assert max(hot.values()) == 0, hot
    assert max(sizes.values()) == 0, sizes
    for other in ("thompson_prep_kernel", "thompson_finish_kernel", "thompson_resid_kernel"):
        assert any(other in k for k in sizes)


@needs_hipcc
def test_no_barrier_of_the_thompson_kernels_is_reachable_with_an_lds_write_in_flight(capsys):
    assert "thompson" in cb.UNITS
    rc = cb.main(["thompson"])
    out = capsys.readouterr().out
    assert rc == 0, out
    assert "0 reachable" in out
