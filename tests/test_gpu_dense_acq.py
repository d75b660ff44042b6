"""The four acquisitions on the dense posterior (gpbo_acq_argmax_f64, gpbo_mes_acq_f64, gpbo_constrained_acq_f64,
gpbo_ehvi_acq_f64: instances of dense_acq_kernel, csrc/dense_acq.h) against the BITS recorded before they shared that frame:
tests/golden/dense_acq_bits.json, written by tests/golden/make_dense_acq_golden.py, which also owns the inputs (an integer hash
of the index: nothing stored), the cases and the runner.  No tolerance: the SHA-256 of every dense output, the bit pattern of
best_val, best_idx and nan_count are equal, and a second call gives what the first gave.

Sizes M = 1, 255, 256, 257, 262,145 (one lane; a masked tail; an exact workgroup; one candidate into a second workgroup; one
candidate into the second grid-stride trip of workgroup 0), each with NaNs planted at 0, 63, 64 and M - 1, zero sigmas, and the
best value twice (index 37 and M - 3), M = 1 also without them; idx_offset = 3 * 2^32 + 17; every case with and without its
dense outputs."""
import importlib.util
import json
import os

import pytest
import torch  # noqa: F401  (before the library initialises HIP)

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
_spec = importlib.util.spec_from_file_location("make_dense_acq_golden", os.path.join(HERE, "golden", "make_dense_acq_golden.py"))
G = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(G)

with open(G.FIXTURE) as _f:
    WANT = json.load(_f)
DENSE_OUTPUTS = {"acq": ["acq"], "mes": ["acq"], "cons": ["feas", "val"], "ehvi": ["val"]}
_RUNNERS = {}


def _runner(M, plant):
    if (M, plant) not in _RUNNERS:
        _RUNNERS[(M, plant)] = G.Runner(M, plant)
    return _RUNNERS[(M, plant)]


def test_the_fixture_holds_exactly_the_cases():
    ids = {G.case_id(e, p, M, plant, dense) for M, plant in G.size_variants() for e, p in G.cases() for dense in (True, False)}
    assert ids == set(WANT) and len(ids) == 6 * 11 * 2


@pytest.mark.parametrize("entry", ["acq", "mes", "cons", "ehvi"])
@pytest.mark.parametrize("M,plant", G.size_variants())
def test_bits_are_the_recorded_ones_and_repeat(M, plant, entry):
    run = _runner(M, plant)
    for e, par in G.cases():
        if e != entry:
            continue
        for dense in (True, False):
            cid = G.case_id(e, par, M, plant, dense)
            first, second = run.run(e, par, dense), run.run(e, par, dense)
            assert sorted(first["sha"]) == (DENSE_OUTPUTS[e] if dense else []), cid
            assert first == WANT[cid], cid
            assert second == first, cid
