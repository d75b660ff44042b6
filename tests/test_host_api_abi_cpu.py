"""CPU-only checks of the host-pointer boundary (csrc/host_api.hip): gpbo_select_next_host_f64 and gpbo_select_qei_host_f64
refuse bad arguments with GPBO_ERR_ARG on the host, before a stream exists or a pointer is read on the device.  (What a
VALID call returns is not asserted here: that needs a GPU, tests/test_gpu_host_api.py.)"""
import ctypes as C

import numpy as np
import pytest

from bayesian_optimisation_amd import _lib

ERR_ARG, CHUNK_MAX = -1, 1 << 24   # GPBO_ERR_ARG, GPBO_CHUNK_MAX (include/gpbo.h)
GRANULE, MAX_D, MAX_D_ANY = _lib.CHUNK_GRANULE, _lib.MAX_D, _lib.MAX_D_ANY

# small real arrays behind every pointer (d up to GPBO_MAX_D_ANY + 1 columns, so that no refused call could read past one)
N, M, S = 4, 16, 4
X, Y, XS = np.zeros((N, MAX_D_ANY + 1)), np.zeros(N), np.zeros((M, MAX_D_ANY + 1))
LS, Z = np.full(MAX_D_ANY + 1, 0.5), np.zeros((S, 8))
LS_ZERO = LS.copy()
LS_ZERO[1] = 0.0
RES, INFO = np.zeros(4, dtype=np.int64), np.zeros(1, dtype=np.int32)


def _p(a):
    return a.ctypes.data_as(C.c_void_p)


def select_next(N=N, d=2, ls=LS, M=M, kind=0, chunk=0):
    return _lib.load().gpbo_select_next_host_f64(_p(X), _p(Y), N, d, _p(ls), 1e-4, 1e-6, _p(XS), M, kind, 4.0, 0.0, 0.0, chunk,
                                                 None, None, None, None, _p(RES), _p(INFO))


def select_qei(N=N, d=2, ls=LS, M=M, S=S, chunk=0):
    return _lib.load().gpbo_select_qei_host_f64(_p(X), _p(Y), N, d, _p(ls), 1e-4, 1e-6, _p(XS), M, 0.0, 0.0, _p(Z), S, chunk,
                                                None, _p(RES), _p(INFO))


BOTH = [dict(N=0), dict(ls=LS_ZERO), dict(chunk=GRANULE + 1), dict(chunk=500), dict(chunk=CHUNK_MAX + GRANULE)]
TABLE = ([(select_next, kw) for kw in BOTH + [dict(d=MAX_D_ANY + 1), dict(kind=7)]] +
         [(select_qei, kw) for kw in BOTH + [dict(d=MAX_D + 1), dict(M=12), dict(S=0)]])


def test_the_constants_the_table_uses_are_the_headers():
    import os
    import re

    repo = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    src = open(os.path.join(repo, "include", "gpbo.h")).read()
    for name, value in (("ERR_ARG", "(-1)"), ("CHUNK_MAX", "(1 << 24)"), ("CHUNK_GRANULE", str(GRANULE)), ("MAX_D", str(MAX_D)),
                        ("MAX_D_ANY", str(MAX_D_ANY))):
        assert re.search(rf"#define\s+GPBO_{name}\s+{re.escape(value)}\s", src), name


@pytest.mark.parametrize("entry,kw", TABLE, ids=[f"{f.__name__}-{'-'.join(kw)}-{i}" for i, (f, kw) in enumerate(TABLE)])
def test_host_entries_refuse_bad_arguments_on_the_host(entry, kw):
    RES[:], INFO[:] = 77, 77
    assert entry(**kw) == ERR_ARG
    assert np.all(RES == 77) and INFO[0] == 77   # a refused call leaves its outputs alone
