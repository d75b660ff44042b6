"""CPU-only checks of the Matern boundary: every gpbo_*_kern_f64 entry refuses a kernel id outside {0, 1, 2}, a Matern id with
d > GPBO_MAX_D and a Matern id with diag_add != 0 on the host before anything is launched, while legal ids get as far as the
next check; the Python layers refuse the unsupported combinations without a GPU; the Matern kernels compile for gfx950 without
scratch and are barrier-checked."""
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

NEW = ["gpbo_kxx_kern_f64", "gpbo_kstar_mu_kern_f64", "gpbo_factorise_kern_f64", "gpbo_posterior_acq_kern_f64",
       "gpbo_nlml_grad_kern_f64", "gpbo_nlml_hyper_kern_f64", "gpbo_select_next_host_kern_f64", "gpbo_nlml_grad_host_kern_f64",
       "gpbo_nlml_hyper_host_kern_f64"]
BAD_IDS = (-1, 3, 7, 1 << 20)


class _Args:
    """Arguments every check before the kernel id accepts: fake 256-byte aligned pointers (never dereferenced), real length
    scales (the host entries read them)."""

    def __init__(self):
        self.buf = (C.c_char * 1024)()
        self.p = C.c_void_p((C.addressof(self.buf) + 255) & ~255)
        self.ls = (C.c_double * 32)(*([0.5] * 32))
        self.lsp = C.cast(self.ls, C.c_void_p)

    def calls(self, lib):
        """name -> f(kernel, d, diag_add, wbytes); diag_add / wbytes are ignored by the entries that have none."""
        p, lsp = self.p, self.lsp
        return {
            "gpbo_kxx_kern_f64": lambda k, d, da, wb: lib.gpbo_kxx_kern_f64(p, 100, d, lsp, k, 1e-4, 1e-6, p, 128, None),
            "gpbo_kstar_mu_kern_f64": lambda k, d, da, wb: lib.gpbo_kstar_mu_kern_f64(p, 1000, p, 100, 128, d, lsp, k, p, da, 0, p,
                                                                                      1024, p, None),
            "gpbo_factorise_kern_f64": lambda k, d, da, wb: lib.gpbo_factorise_kern_f64(p, p, 100, d, lsp, k, 1e-4, 1e-6, 128, p, p, p,
                                                                                        p, p, wb, None),
            "gpbo_posterior_acq_kern_f64": lambda k, d, da, wb: lib.gpbo_posterior_acq_kern_f64(
                p, 1000, p, 100, 128, d, lsp, k, p, p, 1.0, 0, 4.0, 0.0, da, 0, 512, None, None, None, p, p, wb, None, None),
            "gpbo_nlml_grad_kern_f64": lambda k, d, da, wb: lib.gpbo_nlml_grad_kern_f64(p, p, p, p, 100, 128, d, lsp, k, p, p, p, wb,
                                                                                        None),
            "gpbo_nlml_hyper_kern_f64": lambda k, d, da, wb: lib.gpbo_nlml_hyper_kern_f64(p, p, p, p, 100, 128, d, lsp, k, 1e-2, 3, p,
                                                                                          p, None, p, wb, None),
            "gpbo_select_next_host_kern_f64": lambda k, d, da, wb: lib.gpbo_select_next_host_kern_f64(
                p, p, 100, d, lsp, k, 1e-4, 1e-6, p, 1000, 0, 4.0, 0.0, da, 0, None, None, None, None, p, p),
            "gpbo_nlml_grad_host_kern_f64": lambda k, d, da, wb: lib.gpbo_nlml_grad_host_kern_f64(p, p, 100, d, lsp, k, 1e-4, p),
            "gpbo_nlml_hyper_host_kern_f64": lambda k, d, da, wb: lib.gpbo_nlml_hyper_host_kern_f64(p, p, 100, d, lsp, k, 1e-2, 3, p),
        }


HAS_WORKSPACE = ("gpbo_factorise_kern_f64", "gpbo_posterior_acq_kern_f64", "gpbo_nlml_grad_kern_f64", "gpbo_nlml_hyper_kern_f64")
HAS_DIAG_ADD = ("gpbo_kstar_mu_kern_f64", "gpbo_posterior_acq_kern_f64", "gpbo_select_next_host_kern_f64")
ANY_D = ("gpbo_kxx_kern_f64", "gpbo_factorise_kern_f64", "gpbo_posterior_acq_kern_f64", "gpbo_select_next_host_kern_f64")


def test_header_constants_prototypes_and_names():
    repo = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    src = open(os.path.join(repo, "include", "gpbo.h")).read()
    defs = {k: int(v) for k, v in re.findall(r"#define\s+(GPBO_[A-Z0-9_]+)\s+\(?(-?\d+)\)?", src)}
    assert (defs["GPBO_KERNEL_SE"], defs["GPBO_KERNEL_MATERN32"], defs["GPBO_KERNEL_MATERN52"]) == (0, 1, 2)
    assert _lib.KERNEL_IDS == {"se": 0, "matern32": 1, "matern52": 2}
    assert defs["GPBO_VERSION"] == 151 and _lib.load().gpbo_version() == 151
    for name in NEW:
        assert name in _lib.SIGNATURES and name in src
        twin = name.replace("_kern_f64", "_f64")
        res, args = _lib.SIGNATURES[twin]
        # the twin with one int32 inserted right after ls_host (the first pointer that follows the int32 d)
        at = args.index(_lib._i32) + 2
        assert _lib.SIGNATURES[name] == (res, args[:at] + [_lib._i32] + args[at:]), name
    for bad in ("rbf", "matern", "", None, 1):
        with pytest.raises(ValueError):
            _lib.kernel_id(bad)


@pytest.mark.parametrize("name", NEW)
def test_kernel_id_refusals_come_before_any_hip_call(name):
    lib = _lib.load()
    a = _Args()
    call = a.calls(lib)[name]
    for k in BAD_IDS:                                   # a kernel id outside {0, 1, 2}
        assert call(k, 2, 0.0, 1 << 40) == -1, k
    for k in (1, 2):
        assert call(k, 17, 0.0, 1 << 40) == -1, k       # a Matern id with d > GPBO_MAX_D
        assert call(k, 1024, 0.0, 1 << 40) == -1, k
        if name in HAS_DIAG_ADD:
            assert call(k, 2, 1e-4, 1 << 40) == -1, k   # a Matern id with the N == M quirk
    if name in HAS_WORKSPACE:
        # every legal id passes the argument checks: the short workspace is what stops the call (still before any HIP call)
        for k in (0, 1, 2):
            for d in (1, 2, 16):
                assert call(k, d, 0.0, 8) == -3, (k, d)
        if name in ANY_D:
            assert call(0, 17, 0.0, 8) == -3            # the squared exponential keeps its any-d path
        if name in HAS_DIAG_ADD:
            assert call(0, 2, 1e-4, 8) == -3            # ... and its quirk


def test_all_null_arguments_are_refused_with_every_kernel_id():
    lib = _lib.load()
    for name in NEW:
        res, args = _lib.SIGNATURES[name]
        for k in (0, 1, 2):
            a = [None if t is C.c_void_p else (0.0 if t is C.c_double else 0) for t in args]
            a[args.index(_lib._i32) + 2] = k
            assert getattr(lib, name)(*a) == -1, (name, k)


def test_constructors_refuse_the_unsupported_combinations():
    from bayesian_optimisation_amd.host_binding import PointSelectorHost
    from bayesian_optimisation_amd.point_selector import PointSelector

    for kernel in ("matern32", "matern52"):
        for kw, word in ((dict(ard="grid"), "ard='grid'"), (dict(), "ard='grid'"),
                         (dict(ard="gradient", precision="fp32"), "precision"), (dict(ard="gradient", precision="i8"), "precision"),
                         (dict(ard="gradient", precision="i8c"), "precision"), (dict(ard="gradient", incremental=True), "incremental"),
                         (dict(ard="gradient", state_path="s.npz"), "state_path"),
                         (dict(ard="gradient", dense_outputs=False), "dense_outputs")):
            with pytest.raises(ValueError) as e:
                PointSelector(kernel=kernel, **kw)
            assert kernel in str(e.value) and word in str(e.value), str(e.value)   # which kernel, which option
        with pytest.raises(ValueError) as e:
            PointSelectorHost(kernel=kernel)
        assert kernel in str(e.value) and "ard='grid'" in str(e.value)
        for ard in ("gradient", "hyper"):
            assert PointSelector(kernel=kernel, ard=ard)._kernel == kernel
            ph = PointSelectorHost(kernel=kernel, ard=ard)
            for call, what in ((lambda: ph.select_batch(2), "select_batch"), (lambda: ph.select_thompson(2), "select_thompson"),
                               (lambda: ph.refine_next(), "refine_next"),
                               (lambda: ph.q_expected_improvement(), "q_expected_improvement")):
                with pytest.raises(ValueError) as e:
                    call()
                assert kernel in str(e.value) and what in str(e.value)
            ps = PointSelector(kernel=kernel, ard=ard)
            for call in (lambda: ps.select_batch(2), lambda: ps.select_thompson(2), lambda: ps.refine_next(),
                         lambda: ps.q_expected_improvement()):
                with pytest.raises(ValueError) as e:
                    call()
                assert kernel in str(e.value)
    for cls in (PointSelector, PointSelectorHost):
        for bad in ("rbf", "matern", None):
            with pytest.raises(ValueError):
                cls(kernel=bad)
        assert cls()._kernel == "se" and cls(kernel="se")._kernel == "se"


def test_host_binding_refuses_unknown_kernels_before_touching_the_library():
    from bayesian_optimisation_amd import host_binding as H

    X, y = np.zeros((4, 2)), np.zeros(4)
    for call in (lambda: H.nlml_and_grad(X, y, [1.0, 1.0], kernel="rbf"), lambda: H.nlml_hyper(X, y, [1.0, 1.0], 1e-2, kernel="rbf"),
                 lambda: H.select_next(X, y, [1.0, 1.0], np.zeros((5, 2)), kernel="rbf")):
        with pytest.raises(ValueError):
            call()


@needs_hipcc
@pytest.mark.parametrize("unit,kernels", [("kernel_build", ("kxx_kernel", "kstar_mu_kernel")),
                                          ("ard_grad", ("nlml_grad_kernel", "nlml_grad_matern_kernel"))])
def test_the_matern_kernels_compile_without_scratch_and_pass_the_barrier_check(tmp_path, capsys, unit, kernels):
    asm = open(cb.assemble(unit, str(tmp_path))).read()
    sizes = {re.search(r"\.name:\s+(\S+)", b).group(1): int(re.search(r"\.private_segment_fixed_size:\s+(\d+)", b).group(1))
             for b in asm.split("  - .agpr_count:")[1:]}
    for kernel in kernels:
        assert any(kernel in k for k in sizes), sorted(sizes)
    if unit == "ard_grad":   # 16 feature counts x 2 families beside the 16 squared-exponential kernels
        assert sum("nlml_grad_matern_kernel" in k for k in sizes) == 32
    else:                    # K(X,X): 16 x 3 families; K(X*,X) in fp64: 16 x 2 families x 2 store kinds more than before
        assert sum("kxx_kernel" in k for k in sizes) == 48
        assert sum("kstar_mu_kernel" in k and re.search(r"Lb[01]ELi[12]EE", k) is not None for k in sizes) == 64
    assert max(sizes.values()) == 0, {k: v for k, v in sizes.items() if v}
    assert unit in cb.UNITS
    rc = cb.main([unit])
    out = capsys.readouterr().out
    assert rc == 0 and "0 reachable" in out, out
