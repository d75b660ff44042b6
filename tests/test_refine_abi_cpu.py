"""CPU-only checks of the refinement boundary (csrc/refine.hip): the size contracts of gpbo_posterior_grad_f64 /
gpbo_refine_f64 / gpbo_refine_host_f64 and the two workspace queries are refused on the host before anything is launched, the
Python layer refuses the same without a GPU, and the compiled kernels need no scratch and have no barrier reachable with an
LDS write in flight."""
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


def _doubles(*v):
    a = (C.c_double * len(v))(*v)
    return a, C.cast(a, C.c_void_p)


def test_workspace_queries():
    lib = _lib.load()
    for ws in (lib.gpbo_posterior_grad_workspace_bytes, lib.gpbo_refine_workspace_bytes):
        assert ws(128, 1) > 0 and ws(4096, 4096) > 3 * 8 * 4096 * 4096
        assert ws(128, 0) == -1 and ws(128, 4097) == -1 and ws(128, -5) == -1       # P < 1, P > GPBO_REFINE_MAX_P
        assert ws(100, 8) == -1 and ws(0, 8) == -1 and ws(-128, 8) == -1            # Np granule, empty
        prev = 0
        for P in (1, 2, 63, 64, 65, 128, 200, 1024, 4095, 4096):
            b = ws(256, P)
            assert b >= prev and b % 256 == 0
            prev = b
        assert ws(256, 1) == ws(256, 64) < ws(256, 65)                              # whole tiles of 64 points
    # the three point-major slabs, and the stepping state on top of them
    assert lib.gpbo_posterior_grad_workspace_bytes(4096, 128) - lib.gpbo_posterior_grad_workspace_bytes(4096, 64) == 3 * 8 * 64 * 4096
    assert lib.gpbo_refine_workspace_bytes(256, 64) > lib.gpbo_posterior_grad_workspace_bytes(256, 64)


def test_device_entry_points_check_their_contracts_on_the_host():
    lib = _lib.load()
    buf, p = _fake_pointer()
    ls, lsp = _doubles(*([0.5] * 16))
    lo, lop = _doubles(*([0.0] * 16))
    hi, hip = _doubles(*([1.0] * 16))
    need_g, need_r = lib.gpbo_posterior_grad_workspace_bytes(128, 8), lib.gpbo_refine_workspace_bytes(128, 8)

    def grad(Xq=p, P=8, X=p, N=100, Np=128, d=2, lsp=lsp, U=p, alpha=p, prior=1.000101, kind=0, work=p, wbytes=need_g):
        return lib.gpbo_posterior_grad_f64(Xq, P, X, N, Np, d, lsp, U, alpha, prior, kind, 4.0, 0.0, None, None, None, None,
                                           None, None, work, wbytes, None)

    def refine(Xq=p, P=8, lop=lop, hip=hip, X=p, N=100, Np=128, d=2, lsp=lsp, U=p, alpha=p, kind=0, iters=30, step0=0.1,
               result=p, work=p, wbytes=need_r):
        return lib.gpbo_refine_f64(Xq, P, lop, hip, X, N, Np, d, lsp, U, alpha, 1.000101, kind, 4.0, 0.0, iters, step0, None,
                                   None, None, None, result, work, wbytes, None)

    _, bad_ls = _doubles(0.5, 0.0)
    _, neg_ls = _doubles(0.5, -1.0)
    for call in (grad, refine):
        assert call(P=0) == -1 and call(P=4097) == -1
        assert call(d=0) == -1 and call(d=17) == -1
        assert call(Np=100) == -1 and call(Np=256) == -1 and call(N=129) == -1 and call(N=0) == -1   # Np is not gpbo_padded_n(N)
        assert call(lsp=bad_ls) == -1 and call(lsp=neg_ls) == -1
        assert call(kind=7) == -1 and call(kind=-1) == -1
        for name in ("Xq", "X", "lsp", "U", "alpha", "work"):
            assert call(**{name: None}) == -1, name
        assert call(U=C.c_void_p(p.value + 8)) == -1         # the GEMM's operand: refused here, before anything is enqueued
    assert refine(lop=None) == -1 and refine(hip=None) == -1 and refine(result=None) == -1
    _, lo_above = _doubles(0.0, 1.5)
    _, inf_hi = _doubles(1.0, float("inf"))
    _, nan_lo = _doubles(float("nan"), 0.0)
    assert refine(lop=lo_above) == -1 and refine(hip=inf_hi) == -1 and refine(lop=nan_lo) == -1
    assert refine(iters=-1) == -1 and refine(iters=1001) == -1
    assert refine(step0=0.0) == -1 and refine(step0=-0.1) == -1 and refine(step0=float("inf")) == -1 and refine(step0=float("nan")) == -1
    # a workspace one byte short, or not 256-byte aligned
    off = C.c_void_p(p.value + 8)
    assert grad(wbytes=need_g - 1) == -3 and grad(work=off) == -3
    assert refine(wbytes=need_r - 1) == -3 and refine(work=off) == -3
    assert refine(wbytes=need_g) == -3                       # the stepping state needs more than the gradient call
    assert refine(iters=-1, wbytes=0) == -1                  # arguments are refused before the workspace
    del buf


def test_host_entry_point_checks_its_contracts_on_the_host():
    lib = _lib.load()
    buf, p = _fake_pointer()
    ls, lsp = _doubles(*([0.5] * 16))
    lo, lop = _doubles(*([0.0] * 16))
    hi, hip = _doubles(*([1.0] * 16))

    def call(X=p, y=p, N=100, d=2, lsp=lsp, Xq=p, P=8, lop=lop, hip=hip, kind=0, iters=30, step0=0.1, result=p, info=p):
        return lib.gpbo_refine_host_f64(X, y, N, d, lsp, 1e-4, 1e-6, Xq, P, lop, hip, kind, 4.0, 0.0, iters, step0, None, None,
                                        None, None, result, info)

    assert call(P=0) == -1 and call(P=4097) == -1 and call(d=0) == -1 and call(d=17) == -1 and call(N=0) == -1
    assert call(kind=7) == -1 and call(iters=-1) == -1 and call(iters=1001) == -1
    assert call(step0=0.0) == -1 and call(step0=float("nan")) == -1 and call(step0=float("inf")) == -1
    _, bad_ls = _doubles(0.5, 0.0)
    _, neg_ls = _doubles(0.5, -1.0)
    _, lo_above = _doubles(0.0, 1.5)
    _, inf_hi = _doubles(1.0, float("inf"))
    _, nan_lo = _doubles(float("nan"), 0.0)
    assert call(lsp=bad_ls) == -1 and call(lsp=neg_ls) == -1
    assert call(lop=lo_above) == -1 and call(hip=inf_hi) == -1 and call(lop=nan_lo) == -1
    for name in ("X", "y", "lsp", "Xq", "lop", "hip", "result", "info"):
        assert call(**{name: None}) == -1, name
    del buf


def test_python_constants_match_the_header():
    repo = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    src = open(os.path.join(repo, "include", "gpbo.h")).read()
    defs = {k: int(v) for k, v in re.findall(r"#define\s+(GPBO_[A-Z_]+)\s+\(?(-?\d+)\)?", src)}
    assert defs["GPBO_REFINE_MAX_P"] == _lib.REFINE_MAX_P == 4096
    assert defs["GPBO_MAX_D"] == _lib.MAX_D == 16
    assert defs["GPBO_VERSION"] == 151
    for name in ("gpbo_posterior_grad_workspace_bytes", "gpbo_posterior_grad_f64", "gpbo_refine_workspace_bytes",
                 "gpbo_refine_f64", "gpbo_refine_host_f64"):
        assert name in _lib.SIGNATURES and re.search(r"\b%s\(" % name, src)


def test_python_layer_refuses_bad_arguments_without_a_gpu():
    import bayesian_optimisation_amd as B
    from bayesian_optimisation_amd import host_binding as H
    from bayesian_optimisation_amd.gp_device import refine_box, refine_params

    assert {"GradResult", "RefineResult"} <= set(B.__all__)
    assert refine_params(64, 8, 30, 0.1) == (30, 0.1) and refine_params(4096, 16, 0, 1) == (0, 1.0)
    for bad in ((0, 8, 30, 0.1), (4097, 8, 30, 0.1), (8, 17, 30, 0.1), (8, 0, 30, 0.1), (8, 8, -1, 0.1), (8, 8, 1001, 0.1),
                (8, 8, 2.5, 0.1), (8, 8, 30, 0.0), (8, 8, 30, float("nan")), (8, 8, 30, float("inf"))):
        with pytest.raises(ValueError):
            refine_params(*bad)
    lo, hi = refine_box(0.0, [1.0, 2.0], 2)
    assert lo.tolist() == [0.0, 0.0] and hi.tolist() == [1.0, 2.0] and lo.flags.c_contiguous
    for bad in ((1.0, 0.0), (0.0, float("inf")), (float("nan"), 1.0), ([0.0, 3.0], [1.0, 2.0])):
        with pytest.raises(ValueError):
            refine_box(*bad, 2)
    X, y, S = np.zeros((4, 2)), np.zeros(4), np.zeros((3, 2))
    for kw in (dict(lower=1.0, upper=0.0), dict(lower=0.0, upper=1.0, iters=-1), dict(lower=0.0, upper=1.0, step0=0.0),
               dict(lower=0.0, upper=1.0, acquisition="ucb"), dict(lower=0.0, upper=1.0, acquisition="ei")):
        with pytest.raises(ValueError):
            H.refine(X, y, [1.0, 1.0], S, **kw)
    with pytest.raises(ValueError):
        H.refine(X, y, [1.0, 1.0], np.zeros((4097, 2)), 0.0, 1.0)
    with pytest.raises(ValueError):
        H.refine(np.zeros((4, 17)), y, np.ones(17), np.zeros((3, 17)), 0.0, 1.0)
    for cls in (B.PointSelector, H.PointSelectorHost):
        assert callable(getattr(cls, "refine_next"))


@needs_hipcc
def test_the_refinement_kernels_need_no_scratch(tmp_path):
    """A fresh csrc/refine.hip compiles for gfx950 and none of the 16 instances of the two templated kernels spills: the hot
    kernel keeps its 2 + 2 d partial sums and the point in registers."""
    s = open(cb.assemble("refine", str(tmp_path))).read()
    sizes = {re.search(r"\.name:\s+(\S+)", b).group(1): int(re.search(r"\.private_segment_fixed_size:\s+(\d+)", b).group(1))
             for b in s.split("  - .agpr_count:")[1:]}
    for kernel in ("refine_grad_step_kernel", "refine_ks_kernel"):
        inst = {k: v for k, v in sizes.items() if kernel in k}
        assert len(inst) == 16, sorted(sizes)
        assert max(inst.values()) == 0, inst
    assert any("refine_finish_kernel" in k for k in sizes) and any("refine_init_kernel" in k for k in sizes)


@needs_hipcc
def test_no_barrier_of_the_refinement_kernels_is_reachable_with_an_lds_write_in_flight(capsys):
    assert "refine" in cb.UNITS
    rc = cb.main(["refine"])
    out = capsys.readouterr().out
    assert rc == 0, out
    assert "0 reachable" in out
