"""CPU-only checks of the constrained-acquisition boundary (csrc/constrained.hip): prototypes and constants of include/gpbo.h
against the binding, every refusal of the two entry points made on the host before anything is launched, the Python layers'
refusals without a GPU, and the compiled kernel: no scratch, no LDS beyond the arg-max slots, its barrier with the LDS writes
waited for."""
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
NAMES = ("gpbo_constrained_acq_f64", "gpbo_constrained_acq_host_f64")
WORK = 16640
NONE, EI, PI = 0, 1, 2


def _fake_pointer():
    buf = (C.c_char * 1024)()
    return buf, C.c_void_p((C.addressof(buf) + 255) & ~255)   # 256-byte aligned like a device allocation; never dereferenced


def _values(*v):
    a = (C.c_double * 8)(*v)
    return a, C.cast(a, C.c_void_p)


def test_python_constants_and_signatures_match_the_header():
    src = open(os.path.join(REPO, "include", "gpbo.h")).read()
    defs = {k: int(v) for k, v in re.findall(r"#define\s+(GPBO_[A-Z_]+)\s+\(?(-?\d+)\)?", src)}
    assert (defs["GPBO_CONS_BASE_NONE"], defs["GPBO_CONS_BASE_EI"], defs["GPBO_CONS_BASE_PI"]) == (NONE, EI, PI)
    assert (_lib.CONS_BASE_NONE, _lib.CONS_BASE_EI, _lib.CONS_BASE_PI) == (NONE, EI, PI)
    assert _lib.CONS_BASE_IDS == {"none": NONE, "ei": EI, "pi": PI}
    assert defs["GPBO_CONS_MAX_C"] == _lib.CONS_MAX_C == 8
    assert defs["GPBO_CONS_WORK_BYTES"] == _lib.CONS_WORK_BYTES == WORK and WORK % 256 == 0
    assert WORK >= 2 * 8 * 1024 + 256                            # the arg-max records of 1024 workgroups, the counter
    assert defs["GPBO_VERSION"] == 151 and _lib.load().gpbo_version() == 151
    i64, i32, f64, p = C.c_int64, C.c_int32, C.c_double, _lib.Pointer
    want = {"gpbo_constrained_acq_f64": [p, p, i64, i32, f64, f64, p, p, i64, i32, p, i64, p, p, p, p, i64, p],
            "gpbo_constrained_acq_host_f64": [p, p, i64, i32, f64, f64, p, p, i64, i32, p, p, p, p]}
    for name in NAMES:
        assert name in src
        assert _lib.SIGNATURES[name] == (C.c_int, want[name])
        assert getattr(_lib.load(), name).argtypes == want[name]
    assert not any(n.startswith("gpbo_constrained") and n.endswith("_bytes") for n in _lib.SIGNATURES)   # the size is a constant


def test_device_entry_refuses_on_the_host():
    lib = _lib.load()
    buf, p = _fake_pointer()
    us, up = _values(*np.linspace(-1.0, 1.0, 8))

    def call(mu=p, sigma=p, M=1000, base=EI, f_best=0.5, xi=0.0, cm=p, cs=p, ldc=1000, Cn=3, u=up, off=0, val=None, feas=None,
             res=p, work=p, wbytes=WORK):
        return lib.gpbo_constrained_acq_f64(mu, sigma, M, base, f_best, xi, cm, cs, ldc, Cn, u, off, val, feas, res, work, wbytes,
                                            None)

    assert lib.gpbo_constrained_acq_f64(*([None, None, 0, 0, 0.0, 0.0, None, None, 0, 0, None, 0] + [None] * 4 + [0, None])) == -1
    for name in ("mu", "sigma", "cm", "cs", "u", "res", "work"):
        assert call(**{name: None}) == -1, name
    assert call(M=0) == -1 and call(M=-5) == -1 and call(M=(1 << 40) + 1, ldc=1 << 41) == -1
    assert call(base=-1) == -1 and call(base=3) == -1
    assert call(Cn=-1) == -1 and call(Cn=9) == -1
    assert call(base=NONE, Cn=0) == -1                            # nothing to evaluate
    assert call(ldc=999) == -1 and call(ldc=0) == -1
    for bad in (float("nan"), float("inf"), float("-inf")):
        keep, bp = _values(0.0, 1.0, bad)
        assert call(u=bp, Cn=3) == -1
        assert call(u=bp, Cn=2, wbytes=WORK - 1) == -3            # the limit beyond C is not read
        for base in (EI, PI):
            assert call(base=base, f_best=bad) == -1 and call(base=base, xi=bad) == -1
        assert call(base=NONE, f_best=bad, xi=bad, wbytes=WORK - 1) == -3   # ... nor f_best / xi without a base
        del keep
    # what may be null: mu / sigma without a base, the constraints with C == 0, the dense outputs always
    assert call(base=NONE, mu=None, sigma=None, wbytes=WORK - 1) == -3
    assert call(Cn=0, cm=None, cs=None, u=None, wbytes=WORK - 1) == -3
    assert call(base=PI, Cn=0, cm=None, cs=None, u=None, wbytes=WORK - 1) == -3
    assert call(val=p, feas=p, Cn=8, off=(1 << 33) + 5, M=1 << 40, ldc=(1 << 40) + 37, wbytes=WORK - 1) == -3
    # the workspace: one byte short or not 256-byte aligned - after the arguments, before any HIP call
    assert call(wbytes=WORK - 1) == -3 and call(wbytes=0) == -3
    assert call(work=C.c_void_p(p.value + 8)) == -3
    assert lib.gpbo_version() == 151
    del buf, us


def test_host_entry_refuses_on_the_host():
    lib = _lib.load()
    buf, p = _fake_pointer()
    us, up = _values(*np.linspace(-1.0, 1.0, 8))
    keep, bp = _values(0.0, float("nan"))

    def call(mu=p, sigma=p, M=10, base=EI, f_best=0.5, xi=0.0, cm=p, cs=p, ldc=10, Cn=3, u=up, val=None, feas=None, res=p):
        return lib.gpbo_constrained_acq_host_f64(mu, sigma, M, base, f_best, xi, cm, cs, ldc, Cn, u, val, feas, res)

    assert lib.gpbo_constrained_acq_host_f64(*([None, None, 0, 0, 0.0, 0.0, None, None, 0, 0] + [None] * 4)) == -1
    for name in ("mu", "sigma", "cm", "cs", "u", "res"):
        assert call(**{name: None}) == -1, name
    assert call(M=0) == -1 and call(M=(1 << 40) + 1, ldc=1 << 41) == -1 and call(base=3) == -1 and call(Cn=9) == -1
    assert call(Cn=-1) == -1 and call(base=NONE, Cn=0) == -1 and call(ldc=9) == -1 and call(u=bp, Cn=2) == -1
    assert call(f_best=float("inf")) == -1 and call(base=PI, xi=float("nan")) == -1
    del buf, us, keep


class _NoLibrary:
    """Stands in for _lib.load() and the entry points: a refusal that reaches the library fails the test."""

    def __call__(self, *a, **k):
        raise AssertionError("the library was touched before the arguments were refused")


def test_python_layers_refuse_bad_arguments_before_the_library_is_touched(monkeypatch):
    import bayesian_optimisation_amd as pkg
    from bayesian_optimisation_amd import PointSelector, PointSelectorHost
    from bayesian_optimisation_amd import host_binding as H
    from bayesian_optimisation_amd.model import SurrogateModel

    assert "ConstrainedResult" in pkg.__all__ and pkg.ConstrainedResult.__dataclass_fields__.keys() >= {
        "best_val", "best_idx", "nan_count", "value", "log_feasibility", "base"}
    lib = _lib.load()   # (the selector classes bind it in their constructors)
    host, host_c = PointSelectorHost(ard="hyper"), PointSelectorHost()
    monkeypatch.setattr(_lib, "load", _NoLibrary())
    for fn in NAMES:
        monkeypatch.setattr(lib, fn, _NoLibrary(), raising=False)
    mu, sigma = np.zeros(10), np.ones(10)
    cm, cs = np.zeros((2, 10)), np.ones((2, 10))
    for kw in (dict(upper=[0.0]), dict(upper=[0.0, np.nan]), dict(upper=[0.0, np.inf]), dict(base="lcb"), dict(f_best=None),
               dict(f_best=np.nan), dict(xi=np.inf), dict(cons_mu=np.zeros((2, 9))), dict(cons_sigma=np.ones((2, 11))),
               dict(mu=np.zeros(9)), dict(base="none", upper=[], cons_mu=None, cons_sigma=None)):
        args = dict(mu=mu, sigma=sigma, cons_mu=cm, cons_sigma=cs, upper=[0.0, 1.0], base="ei", f_best=0.0, xi=0.0)
        args.update(kw)
        with pytest.raises(ValueError):
            H.constrained_acq(**args)
    with pytest.raises(ValueError):
        H.constrained_acq(mu, sigma, np.zeros((9, 10)), np.ones((9, 10)), np.zeros(9))   # more than 8 constraints
    # the selector classes: the options the constrained calls do not serve are named, for the object and for a constraint; bad
    # parameters come before "call update_surrogate() first"
    calls = (lambda ps, **kw: ps.probability_of_improvement(**kw),
             lambda ps, **kw: ps.constrained_expected_improvement([], [], **kw),
             lambda ps, **kw: ps.probability_of_feasibility([PointSelector()], [0.0], **kw))
    for call in calls:
        with pytest.raises(ValueError, match="ard='marginal'"):
            call(PointSelector(ard="marginal"))
        for precision in ("fp32", "i8", "i8c"):
            with pytest.raises(ValueError, match="precision"):
                call(PointSelector(precision=precision))
        with pytest.raises(ValueError, match="dense_outputs"):
            call(PointSelector(dense_outputs=False))
    for bad, what in ((PointSelector(ard="marginal"), "ard='marginal'"), (PointSelector(precision="i8"), "precision"),
                      (PointSelector(dense_outputs=False), "dense_outputs"), (host_c, "every constraint must be a PointSelector"),
                      (object(), "every constraint must be a PointSelector")):
        with pytest.raises(ValueError, match=what):
            PointSelector().constrained_expected_improvement([bad], [0.0])
    with pytest.raises(ValueError, match="every constraint must be a PointSelectorHost"):
        host.probability_of_feasibility([PointSelector()], [0.0])
    for ps, other in ((PointSelector(), PointSelector()), (PointSelector(ard="hyper", kernel="matern52"), PointSelector()),
                      (host, host_c)):
        for kw in (dict(upper=[]), dict(upper=[0.0, 1.0]), dict(upper=[np.nan]), dict(upper=[np.inf]), dict(xi=np.nan),
                   dict(xi="0"), dict(f_best="best"), dict(f_best="observed"), dict(f_best=np.inf), dict(f_best=None), dict(constraints=[other] * 9,
                                                                                                   upper=np.zeros(9))):
            args = dict(constraints=[other], upper=[0.0])
            args.update(kw)
            with pytest.raises(ValueError):
                ps.constrained_expected_improvement(**args)
        for kw in (dict(xi=np.inf), dict(f_best=np.nan), dict(f_best="feasible"), dict(f_best=[1.0])):
            with pytest.raises(ValueError):
                ps.probability_of_improvement(**kw)
        with pytest.raises(ValueError, match="at least one constraint"):
            ps.probability_of_feasibility([], [])
        for call in (lambda: ps.probability_of_improvement(), lambda: ps.probability_of_improvement(xi=0.1, f_best=2.0),
                     lambda: ps.constrained_expected_improvement([other], [0.0]),
                     lambda: ps.constrained_expected_improvement([], [], f_best=1.0),
                     lambda: ps.probability_of_feasibility([other], [0.0])):
            with pytest.raises(RuntimeError, match="update_surrogate"):
                call()
        assert ps.log_feasibility is None and ps.constrained_base is None and ps.constrained_incumbent is None
    # units: log cEI moves by log s under a fitted model, the logarithms of probabilities not at all
    m = SurrogateModel("se", 0.01, 0.0, 5.0, 3.0, True)
    a = np.array([-800.0, -0.25, -np.inf])
    assert np.array_equal(m.acq_to_y("log_cei", a), a + np.log(3.0)) and m.acq_to_y("log_cei", a)[2] == -np.inf
    assert m.acq_to_y("log_pi", a) is a and m.acq_to_y("log_pof", a) is a
    assert m.best_to_y("log_cei", (-2.0, 7, 0)) == (-2.0 + float(np.log(3.0)), 7, 0)
    assert m.best_to_y("log_pof", (-2.0, 7, 0)) == (-2.0, 7, 0) and SurrogateModel().acq_to_y("log_cei", a) is a


def test_new_package_files_do_not_name_the_cpu_reference():
    word = "ora" + "cle"
    pkg = os.path.join(REPO, "bayesian_optimisation_amd")
    for f in ("constrained.py", os.path.join("csrc", "constrained.hip"), os.path.join("csrc", "cons_math.h")):
        assert word not in open(os.path.join(pkg, f)).read(), f


def _kernel_metadata(asm, field):
    return {re.search(r"\.name:\s+(\S+)", b).group(1): int(re.search(r"\." + field + r":\s+(\d+)", b).group(1))
            for b in asm.split("  - .agpr_count:")[1:]}


@needs_hipcc
def test_the_kernel_needs_no_scratch_and_no_lds_beyond_the_argmax_slots(tmp_path):
    """A fresh csrc/constrained.hip compiles for gfx950 into ONE kernel: the constraint loop is a run-time loop over the
    kernel-argument record (a copy of the limits to private memory would show as scratch), and the only LDS is the four waves'
    arg-max records."""
    asm = open(cb.assemble("constrained", str(tmp_path))).read()
    scratch = _kernel_metadata(asm, "private_segment_fixed_size")
    assert len(scratch) == 1 and "dense_acq_kernel" in next(iter(scratch)) and "ConsScore" in next(iter(scratch)), sorted(scratch)
    assert max(scratch.values()) == 0, scratch
    assert max(_kernel_metadata(asm, "group_segment_fixed_size").values()) == 4 * 8 + 4 * 8


@needs_hipcc
def test_no_barrier_of_the_unit_is_reachable_with_an_lds_write_in_flight(capsys):
    assert "constrained" in cb.UNITS
    rc = cb.main(["constrained"])
    out = capsys.readouterr().out
    assert rc == 0, out
    assert "0 reachable" in out
    csrc = os.path.join(REPO, "bayesian_optimisation_amd", "csrc")   # the unit and the frame of its kernel (dense_acq.h)
    src = open(os.path.join(csrc, "constrained.hip")).read() + open(os.path.join(csrc, "dense_acq.h")).read()
    code = re.sub(r"//[^\n]*", "", src)
    assert "__syncthreads" not in code and code.count("gpbo_syncthreads()") == 1   # the barrier is the waited-for one
    assert "atomic" not in code                                                    # (the NaN counter's is gpbo_count_nan's)
