"""CPU-only checks of the batch-selection boundary (csrc/batch.hip): the size contracts of gpbo_select_batch_f64 /
gpbo_select_batch_host_f64 / gpbo_batch_workspace_bytes are refused on the host before anything is launched, and the
compiled hot kernel needs no scratch and has no barrier reachable with an LDS write in flight."""
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


def test_workspace_query():
    lib = _lib.load()
    ws = lib.gpbo_batch_workspace_bytes
    assert ws(128, 1000, 8) > 0
    assert ws(128, 1000, 0) == -1 and ws(128, 1000, 65) == -1 and ws(128, 7, 8) == -1      # q < 1, q > 64, q > M
    assert ws(100, 1000, 8) == -1 and ws(0, 1000, 8) == -1 and ws(128, 0, 1) == -1         # Np granule, empty sets
    # the slab of stored t vectors: (q - 1) rows of M doubles
    assert ws(4096, 1 << 21, 8) - ws(4096, 1 << 21, 2) == 6 * 8 * (1 << 21)
    assert ws(4096, 1 << 21, 64) >= 63 * 8 * (1 << 21)
    prev = 0
    for q in range(1, 65):
        b = ws(256, 4096, q)
        assert b >= prev and b % 256 == 0
        prev = b


def test_device_entry_point_checks_its_size_contracts_on_the_host():
    lib = _lib.load()
    buf, p = _fake_pointer()
    ls = (C.c_double * 16)(*([0.5] * 16))
    lsp = C.cast(ls, C.c_void_p)
    need = lib.gpbo_batch_workspace_bytes(128, 1000, 8)

    def call(M=1000, N=100, Np=128, d=2, lsp=lsp, kind=0, q=8, fantasy=0, lie=0.0, work=p, wbytes=need):
        return lib.gpbo_select_batch_f64(p, M, p, N, Np, d, lsp, p, p, 1e-4, 1e-6, 1.000101, kind, 4.0, 0.0, q, fantasy, lie,
                                         p, p, 0, p, p, p, p, work, wbytes, None)

    assert call(q=0) == -1
    assert call(q=65) == -1
    assert call(M=7, wbytes=1 << 40) == -1                      # q > M
    assert call(d=17) == -1 and call(d=0) == -1
    assert call(kind=7) == -1 and call(fantasy=2) == -1 and call(fantasy=-1) == -1
    assert call(fantasy=1, lie=float("nan")) == -1 and call(fantasy=1, lie=float("inf")) == -1
    assert call(Np=100) == -1 and call(N=129) == -1             # Np granule, N > Np
    bad = (C.c_double * 2)(0.5, 0.0)
    assert call(lsp=C.cast(bad, C.c_void_p)) == -1
    assert call(work=None) == -1
    # a workspace one byte short, or not 256-byte aligned
    assert call(wbytes=need - 1) == -3
    assert call(work=C.c_void_p(p.value + 8)) == -3
    # (a NaN lie is only refused where it would be used)
    assert call(fantasy=0, lie=float("nan"), wbytes=need - 1) == -3
    del buf


def test_host_entry_point_checks_its_size_contracts_on_the_host():
    lib = _lib.load()
    buf, p = _fake_pointer()
    ls = (C.c_double * 16)(*([0.5] * 16))
    lsp = C.cast(ls, C.c_void_p)

    def call(M=1000, N=100, d=2, kind=0, chunk=0, q=8, fantasy=0, lie=0.0):
        return lib.gpbo_select_batch_host_f64(p, p, N, d, lsp, 1e-4, 1e-6, p, M, kind, 4.0, 0.0, chunk, q, fantasy, lie, p, p,
                                              None, None, p, p)

    assert call(q=0) == -1 and call(q=65) == -1 and call(M=7) == -1
    assert call(d=17) == -1 and call(kind=7) == -1 and call(fantasy=2) == -1
    assert call(fantasy=1, lie=float("nan")) == -1
    assert call(chunk=500) == -1 and call(N=0) == -1
    del buf


def test_python_constants_match_the_header():
    repo = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    src = open(os.path.join(repo, "include", "gpbo.h")).read()
    defs = {k: int(v) for k, v in re.findall(r"#define\s+(GPBO_[A-Z_]+)\s+\(?(-?\d+)\)?", src)}
    assert defs["GPBO_BATCH_MAX_Q"] == _lib.BATCH_MAX_Q == 64
    assert defs["GPBO_FANTASY_BELIEVER"] == _lib.FANTASY_BELIEVER and defs["GPBO_FANTASY_LIE"] == _lib.FANTASY_LIE
    assert defs["GPBO_VERSION"] == 151


def test_python_layer_refuses_bad_arguments_without_a_gpu():
    from bayesian_optimisation_amd import host_binding as H
    from bayesian_optimisation_amd.gp_device import fantasy_params

    assert fantasy_params("believer", None) == (0, 0.0) and fantasy_params("liar", -1.5) == (1, -1.5)
    for bad in (("liar", None), ("liar", float("nan")), ("truth", 0.0)):
        with pytest.raises(ValueError):
            fantasy_params(*bad)
    X, y, Xs = np.zeros((4, 2)), np.zeros(4), np.zeros((10, 2))
    for kw in (dict(q=0), dict(q=11), dict(q=65), dict(q=2, fantasy="liar")):
        with pytest.raises(ValueError):
            H.select_batch(X, y, [1.0, 1.0], Xs, **kw)
    with pytest.raises(ValueError):
        H.select_batch(np.zeros((4, 17)), y, np.ones(17), np.zeros((10, 17)), q=2)


@needs_hipcc
def test_the_downdate_kernel_needs_no_scratch(tmp_path):
    """A fresh csrc/batch.hip compiles for gfx950 and no instance of the hot kernel (d = 1 .. 16) spills: the loop keeps two
    candidates' scaled coordinates and four distance / exp chains in registers."""
    s = open(cb.assemble("batch", str(tmp_path))).read()
    sizes = {re.search(r"\.name:\s+(\S+)", b).group(1): int(re.search(r"\.private_segment_fixed_size:\s+(\d+)", b).group(1))
             for b in s.split("  - .agpr_count:")[1:]}
    down = {k: v for k, v in sizes.items() if "batch_downdate_kernel" in k}
    assert len(down) == 16, sorted(sizes)
    assert max(down.values()) == 0, down
    assert any("batch_pivot_kernel" in k for k in sizes)


@needs_hipcc
def test_no_barrier_of_the_batch_kernels_is_reachable_with_an_lds_write_in_flight(capsys):
    assert "batch" in cb.UNITS
    rc = cb.main(["batch"])
    out = capsys.readouterr().out
    assert rc == 0, out
    assert "0 reachable" in out
