"""CPU-only checks of the max-value-entropy-search boundary (csrc/mes.hip): prototypes and constants of include/gpbo.h against
the binding, every refusal of the four entry points made on the host before anything is launched, the Python layers' refusals
without a GPU, and the compiled kernels: no scratch, every barrier with its LDS writes waited for."""
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
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("gpbo_mes_log_survival_f64", "gpbo_mes_acq_f64", "gpbo_mes_log_survival_host_f64", "gpbo_mes_acq_host_f64")
WORK = 1 << 20


def _fake_pointer():
    buf = (C.c_char * 1024)()
    return buf, C.c_void_p((C.addressof(buf) + 255) & ~255)   # 256-byte aligned like a device allocation; never dereferenced


def _values(*v):
    a = (C.c_double * 64)(*v)
    return a, C.cast(a, C.c_void_p)


def test_python_constants_and_signatures_match_the_header():
    src = open(os.path.join(REPO, "include", "gpbo.h")).read()
    defs = {k: int(v) for k, v in re.findall(r"#define\s+(GPBO_[A-Z_]+)\s+\(?(-?\d+)\)?", src)}
    assert defs["GPBO_MES_MAX_LEVELS"] == _lib.MES_MAX_LEVELS == 64
    assert defs["GPBO_MES_MAX_S"] == _lib.MES_MAX_S == 64
    assert defs["GPBO_MES_WORK_BYTES"] == _lib.MES_WORK_BYTES == WORK and WORK % 256 == 0
    assert WORK >= 8 * 1024 * 64 + 2 * 8 * 1024 + 256           # the partial sums, the arg-max records, the counter
    assert defs["GPBO_VERSION"] == 151 and _lib.load().gpbo_version() == 151
    i64, i32, p = C.c_int64, C.c_int32, _lib.Pointer
    want = {"gpbo_mes_log_survival_f64": [p, p, i64, p, i32, p, p, p, i64, p],
            "gpbo_mes_acq_f64": [p, p, i64, p, i32, i64, p, p, p, i64, p],
            "gpbo_mes_log_survival_host_f64": [p, p, i64, p, i32, p, p],
            "gpbo_mes_acq_host_f64": [p, p, i64, p, i32, p, p]}
    for name in NAMES:
        assert name in src
        assert _lib.SIGNATURES[name] == (C.c_int, want[name])
        assert getattr(_lib.load(), name).argtypes == want[name]
    assert not any(n.startswith("gpbo_mes") and n.endswith("_bytes") for n in _lib.SIGNATURES)   # the size is a constant


def test_log_survival_entry_refuses_on_the_host():
    lib = _lib.load()
    buf, p = _fake_pointer()
    zs, zp = _values(*np.linspace(-1.0, 1.0, 64))

    def call(mu=p, sigma=p, M=1000, z=zp, Q=63, out=p, nan=p, work=p, wbytes=WORK):
        return lib.gpbo_mes_log_survival_f64(mu, sigma, M, z, Q, out, nan, work, wbytes, None)

    for name in ("mu", "sigma", "z", "out", "nan", "work"):
        assert call(**{name: None}) == -1, name
    assert call(M=0) == -1 and call(M=-5) == -1 and call(M=(1 << 40) + 1) == -1
    assert call(Q=0) == -1 and call(Q=65) == -1 and call(Q=-1) == -1
    for bad in (float("nan"), float("inf"), float("-inf")):
        keep, bp = _values(0.0, 1.0, bad)
        assert call(z=bp, Q=3) == -1
        assert call(z=bp, Q=2, wbytes=WORK - 1) == -3         # the level beyond Q is not read
        del keep
    # the workspace: one byte short or not 256-byte aligned - after the arguments, before any HIP call
    assert call(wbytes=WORK - 1) == -3 and call(wbytes=0) == -3
    assert call(work=C.c_void_p(p.value + 8)) == -3
    assert call(M=1 << 40, Q=64, wbytes=WORK - 1) == -3 and call(M=1, Q=1, wbytes=WORK - 1) == -3
    del buf, zs


def test_acquisition_entry_refuses_on_the_host():
    lib = _lib.load()
    buf, p = _fake_pointer()
    ys, yp = _values(*np.linspace(-3.0, -1.0, 64))

    def call(mu=p, sigma=p, M=1000, y=yp, S=16, off=0, acq=None, res=p, work=p, wbytes=WORK):
        return lib.gpbo_mes_acq_f64(mu, sigma, M, y, S, off, acq, res, work, wbytes, None)

    for name in ("mu", "sigma", "y", "res", "work"):
        assert call(**{name: None}) == -1, name
    assert call(M=0) == -1 and call(M=(1 << 40) + 1) == -1
    assert call(S=0) == -1 and call(S=65) == -1
    for bad in (float("nan"), float("inf")):
        keep, bp = _values(-1.0, bad)
        assert call(y=bp, S=2) == -1
        del keep
    assert call(wbytes=WORK - 1) == -3
    assert call(work=C.c_void_p(p.value + 8)) == -3
    assert call(acq=p, S=64, off=1 << 40, wbytes=WORK - 1) == -3   # (the dense output is optional)
    del buf, ys


def test_host_entries_refuse_on_the_host():
    lib = _lib.load()
    buf, p = _fake_pointer()
    vs, vp = _values(*np.linspace(-1.0, 1.0, 64))
    keep, bp = _values(0.0, float("nan"))

    def surv(mu=p, sigma=p, M=10, z=vp, Q=63, out=p, nan=p):
        return lib.gpbo_mes_log_survival_host_f64(mu, sigma, M, z, Q, out, nan)

    def acq(mu=p, sigma=p, M=10, y=vp, S=16, out=None, res=p):
        return lib.gpbo_mes_acq_host_f64(mu, sigma, M, y, S, out, res)

    for name in ("mu", "sigma", "z", "out", "nan"):
        assert surv(**{name: None}) == -1, name
    for name in ("mu", "sigma", "y", "res"):
        assert acq(**{name: None}) == -1, name
    assert surv(M=0) == -1 and surv(M=(1 << 40) + 1) == -1 and surv(Q=0) == -1 and surv(Q=65) == -1 and surv(z=bp, Q=2) == -1
    assert acq(M=0) == -1 and acq(M=(1 << 40) + 1) == -1 and acq(S=0) == -1 and acq(S=65) == -1 and acq(y=bp, S=2) == -1
    del buf, vs, keep


class _NoLibrary:
    """Stands in for _lib.load() and the entry points: a refusal that reaches the library fails the test."""

    def __call__(self, *a, **k):
        raise AssertionError("the library was touched before the arguments were refused")


def test_python_layers_refuse_bad_arguments_before_the_library_is_touched(monkeypatch):
    from bayesian_optimisation_amd import PointSelector, PointSelectorHost
    from bayesian_optimisation_amd import host_binding as H
    from bayesian_optimisation_amd.model import SurrogateModel

    lib = _lib.load()   # (the selector classes bind it in their constructors)
    host = PointSelectorHost(ard="hyper")
    monkeypatch.setattr(_lib, "load", _NoLibrary())
    for fn in NAMES:
        monkeypatch.setattr(lib, fn, _NoLibrary(), raising=False)
    mu, sigma = np.zeros(10), np.ones(10)
    for z in ([], np.zeros(65), [0.0, np.nan], [np.inf]):
        with pytest.raises(ValueError):
            H.mes_log_survival(mu, sigma, z)
        with pytest.raises(ValueError):
            H.mes_acq(mu, sigma, z)
    with pytest.raises(ValueError):
        H.mes_log_survival(mu, sigma[:9], [0.0])
    with pytest.raises(ValueError):
        H.mes_acq(np.zeros(0), np.zeros(0), [0.0])
    # the selector classes: the options MES does not serve are named; bad parameters come before "call update_surrogate() first"
    with pytest.raises(ValueError, match="ard='marginal'"):
        PointSelector(ard="marginal").max_value_entropy_search()
    for precision in ("fp32", "i8", "i8c"):
        with pytest.raises(ValueError, match="precision"):
            PointSelector(precision=precision).max_value_entropy_search()
    with pytest.raises(ValueError, match="dense_outputs"):
        PointSelector(dense_outputs=False).max_value_entropy_search()
    for ps in (PointSelector(), PointSelector(ard="hyper", kernel="matern52"), host):
        for kw in (dict(n_samples=0), dict(n_samples=65), dict(n_samples=1.5), dict(seed=-1), dict(cap=float("nan")),
                   dict(cap="best"), dict(y_star="sobol"), dict(y_star=[0.0, 1.0]), dict(y_star=[np.nan] * 16)):
            with pytest.raises(ValueError):
                ps.max_value_entropy_search(**kw)
        with pytest.raises(RuntimeError, match="update_surrogate"):
            ps.max_value_entropy_search()
        assert ps.sampled_minima is None
    with pytest.raises(ValueError, match="kernel='se' only"):
        PointSelector(ard="hyper", kernel="matern52").max_value_entropy_search(y_star="thompson")
    with pytest.raises(ValueError, match="needs PointSelector"):   # the host class leaves the sample-path route to PointSelector
        host.max_value_entropy_search(y_star="thompson")
    # MES has no unit: the fitted model's map leaves its values alone (EI is scaled, LCB scaled and shifted)
    m = SurrogateModel("se", 0.01, 0.0, 5.0, 3.0, True)
    a = np.array([0.25, 1.5])
    assert m.acq_to_y("mes", a) is a and np.array_equal(m.acq_to_y("ei", a), 3.0 * a)
    assert m.best_to_y("mes", (0.25, 7, 0)) == (0.25, 7, 0)


def test_new_package_files_do_not_name_the_cpu_reference():
    word = "ora" + "cle"
    pkg = os.path.join(REPO, "bayesian_optimisation_amd")
    for f in ("mes.py", os.path.join("csrc", "mes.hip"), os.path.join("csrc", "mes_math.h")):
        assert word not in open(os.path.join(pkg, f)).read(), f


def _kernel_sizes(asm):
    return {re.search(r"\.name:\s+(\S+)", b).group(1): int(re.search(r"\.private_segment_fixed_size:\s+(\d+)", b).group(1))
            for b in asm.split("  - .agpr_count:")[1:]}


@needs_hipcc
def test_no_kernel_of_the_unit_needs_scratch(tmp_path):
    """A fresh csrc/mes.hip compiles for gfx950; the log-survival kernel (one instance, 64 levels) keeps one accumulator per
    level in registers: an array that the compiler could not keep there would show as scratch."""
    sizes = _kernel_sizes(open(cb.assemble("mes", str(tmp_path))).read())
    surv = {k: v for k, v in sizes.items() if "mes_log_survival_kernel" in k}
    assert len(surv) == 1, sorted(sizes)
    assert any("dense_acq_kernel" in k and "MesScore" in k for k in sizes) and any("mes_survival_finish_kernel" in k for k in sizes)
    assert max(sizes.values()) == 0, sizes


@needs_hipcc
def test_no_barrier_of_the_unit_is_reachable_with_an_lds_write_in_flight(capsys):
    assert "mes" in cb.UNITS
    rc = cb.main(["mes"])
    out = capsys.readouterr().out
    assert rc == 0, out
    assert "0 reachable" in out
    csrc = os.path.join(REPO, "bayesian_optimisation_amd", "csrc")   # the unit and the frame of its kernel (dense_acq.h)
    src = open(os.path.join(csrc, "mes.hip")).read() + open(os.path.join(csrc, "dense_acq.h")).read()
    code = re.sub(r"//[^\n]*", "", src)
    assert "__syncthreads" not in code and code.count("gpbo_syncthreads()") == 2   # every barrier is the waited-for one
