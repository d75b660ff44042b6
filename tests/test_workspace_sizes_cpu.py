"""CPU-only: the size of every workspace is part of the ABI (callers allocate by the query and nothing else), so every
`*_workspace_bytes` / `*_bytes` query of include/gpbo.h returns what tests/golden/workspace_bytes.json recorded for it, over a
table of sizes that covers one and several chunks, ragged chunks, the limits of q, S, F and P, and the refused combinations
(negative values); and every entry point that takes a workspace refuses one that is a byte short with GPBO_ERR_WORKSPACE,
after its argument checks and before anything is launched (fake aligned pointers, never dereferenced).

`python tests/test_workspace_sizes_cpu.py` rewrites the table from the library in the tree: run it on the commit whose sizes
are to be kept, never to make this test pass."""
import ctypes as C
import itertools
import json
import os

import pytest

from bayesian_optimisation_amd import _lib

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "workspace_bytes.json")

NP = [128, 256, 384, 4096, 32768]
CHUNK = [512, 1024, 131072]
M = [1, 511, 512, 513, 131073]
Q = [1, 2, 16, _lib.BATCH_MAX_Q]
S = [1, 16, _lib.NEI_MAX_S]                 # = TS_MAX_PATHS = ENSEMBLE_MAX_S
F = [1, 1000, _lib.TS_MAX_FEATURES]
P = [1, 64, _lib.REFINE_MAX_P]
D = [1, 8, _lib.MAX_D]
G = [1, 64, 1100]
CAP = [1, 4096, 131073]
# (valid values, refused values) of each argument, in the order of the query's arguments
QUERIES = {
    "gpbo_factorise_workspace_bytes": [(NP, [])],
    "gpbo_append_workspace_bytes": [(NP, [0, -128])],
    "gpbo_loo_workspace_bytes": [(NP, [0, 100])],
    "gpbo_prepare_i8_bytes": [(NP, [0, 100, _lib.I8_MAX_N + 128])],
    "gpbo_fps_order_workspace_bytes": [([1, 100, 130, 4096, 32768], [0, -1])],
    "gpbo_acq_workspace_bytes": [],
    "gpbo_posterior_workspace_bytes": [(NP, [0, 100]), (CHUNK, [0, 500, (1 << 24) + 512]), (M, [0, -3])],
    "gpbo_qei_workspace_bytes": [(NP, [0, 100]), (CHUNK, [0, 500, (1 << 24) + 512]), (M, [0])],
    "gpbo_posterior_workspace_bytes_f32": [(NP, [0, 100, 384 + 64]), (CHUNK, [0, 1536 + 512, (1 << 24) + 1024]), (M, [0])],
    "gpbo_posterior_workspace_bytes_i8": [(NP, [0, 100, _lib.I8_MAX_N + 128]), (CHUNK, [0, 500]), (M, [0])],
    "gpbo_rescore_workspace_bytes": [(NP, [0, 100]), (CAP, [0, -1]), (CHUNK, [0, 500])],
    "gpbo_ensemble_workspace_bytes": [(NP, [0, 100]), (CHUNK, [0, 500]), (M, [0, (1 << 40) + 1])],
    "gpbo_posterior_nei_workspace_bytes": [(NP, [0, 100]), (CHUNK, [0, 500]), (M, [0]), (S, [0, _lib.NEI_MAX_S + 1])],
    "gpbo_nei_fantasies_workspace_bytes": [(NP, [0, 100, (1 << 20) + 128]), (S, [0, _lib.NEI_MAX_S + 1])],
    "gpbo_batch_workspace_bytes": [(NP, [0, 100]), (M + [64], [0]), (Q, [0, _lib.BATCH_MAX_Q + 1])],
    "gpbo_posterior_grad_workspace_bytes": [(NP, [0, 100]), (P, [0, _lib.REFINE_MAX_P + 1])],
    "gpbo_refine_workspace_bytes": [(NP, [0, 100]), (P, [0, _lib.REFINE_MAX_P + 1])],
    "gpbo_thompson_weights_workspace_bytes": [(NP, [0, 100]), (F, [0, _lib.TS_MAX_FEATURES + 1]), (S, [0, _lib.TS_MAX_PATHS + 1])],
    "gpbo_thompson_paths_workspace_bytes": [(NP, [0, 100]), (M, [0, (1 << 31) + 1]), (F, [0, _lib.TS_MAX_FEATURES + 1]),
                                            (S, [0, _lib.TS_MAX_PATHS + 1])],
    "gpbo_nlml_grid_batched_workspace_bytes": [([1, 65, 2048, 4097, 32768], [0, 32769]), (G, [0])],
    "gpbo_nlml_grad_workspace_bytes": [(NP, [0, 100]), (D, [0, _lib.MAX_D + 1])],
    "gpbo_nlml_hyper_workspace_bytes": [(NP, [0, 100]), (D, [0, _lib.MAX_D + 1])],
}


def table_arguments(name):
    """Every combination of the valid values, then each refused value in its place with the first valid value elsewhere (q > M
    of the batch query is among the combinations)."""
    spec = QUERIES[name]
    rows = [list(a) for a in itertools.product(*[ok for ok, _ in spec])]
    for i, (_, refused) in enumerate(spec):
        for bad in refused:
            rows.append([bad if j == i else ok[0] for j, (ok, _) in enumerate(spec)])
    return rows


def query_table(lib):
    return {name: [a + [int(getattr(lib, name)(*a))] for a in table_arguments(name)] for name in sorted(QUERIES)}


def test_every_size_query_of_the_binding_is_in_the_table():
    queries = {n for n, (res, _) in _lib.SIGNATURES.items() if res is C.c_int64 and "_bytes" in n}
    assert queries == set(QUERIES)


@pytest.mark.parametrize("name", sorted(QUERIES))
def test_workspace_sizes_are_the_recorded_ones(name):
    golden = json.load(open(GOLDEN))[name]
    lib = _lib.load()
    assert [g[:-1] for g in golden] == table_arguments(name)        # the table in the file is the table above
    assert any(g[-1] > 0 for g in golden)
    assert name in ("gpbo_factorise_workspace_bytes", "gpbo_acq_workspace_bytes") or any(g[-1] < 0 for g in golden)
    for *args, want in golden:
        assert int(getattr(lib, name)(*args)) == want, (name, args)


def _fake():
    buf = (C.c_char * 1024)()
    return buf, C.c_void_p((C.addressof(buf) + 255) & ~255)   # 256-byte aligned like a device allocation; never dereferenced


def test_a_workspace_one_byte_short_is_refused_by_the_entries_no_other_abi_test_covers():
    """(select_batch, posterior_grad, refine, the Thompson pair, the NEI pair, the ensemble, nlml_grad, nlml_hyper, loo and the
    batched grid have this check in their own *_abi_cpu.py files.)"""
    lib = _lib.load()
    buf, p = _fake()
    ls = (C.c_double * 16)(*([0.5] * 16))
    lsp = C.cast(ls, C.c_void_p)
    short, ok = -3, -1   # with the full size the next refusal of each call below is an argument's, or there is none before HIP
    N, Np, d, Mc = 100, 128, 2, 1000

    need = lib.gpbo_factorise_workspace_bytes(Np)
    assert lib.gpbo_factorise_f64(p, p, N, d, lsp, 1e-4, 1e-6, Np, p, p, p, p, p, need - 1, None) == short
    assert lib.gpbo_factorise_kern_f64(p, p, N, d, lsp, 2, 1e-4, 1e-6, Np, p, p, p, p, p, need - 1, None) == short
    need = lib.gpbo_append_workspace_bytes(Np)
    assert lib.gpbo_append_f64(p, p, 10, d, lsp, 1e-4, 1e-6, Np, p, p, None, p, p, p, p, need - 1, None) == short

    for chunk, M_ in ((512, Mc), (512, 512), (1024, 5000)):   # several chunks, one chunk (a single chunk buffer), ragged
        need = lib.gpbo_posterior_workspace_bytes(Np, chunk, M_)
        assert lib.gpbo_posterior_acq_f64(p, M_, p, N, Np, d, lsp, p, p, 1.0, 0, 4.0, 0.0, 0.0, 0, chunk, None, None, None, p, p,
                                          need - 1, None, None) == short
        assert lib.gpbo_posterior_acq_kern_f64(p, M_, p, N, Np, d, lsp, 1, p, p, 1.0, 0, 4.0, 0.0, 0.0, 0, chunk, None, None, None,
                                               p, p, need - 1, None, None) == short
        assert lib.gpbo_posterior_prefix_f64(p, M_, p, N, Np, d, lsp, p, p, 1.0, 0, 4.0, 0.0, 0, chunk, 128, None, None, None, p, p,
                                             need - 1, None, None) == short
        need = lib.gpbo_qei_workspace_bytes(Np, chunk, 8 * M_)
        assert lib.gpbo_posterior_qei_f64(p, 8 * M_, p, N, Np, d, lsp, p, p, 1.0, 0.0, 0.0, p, 16, 0, chunk, None, p, p, need - 1,
                                          None, None) == short
        need = lib.gpbo_posterior_workspace_bytes_i8(Np, chunk, M_)
        for fn in (lib.gpbo_posterior_acq_i8, lib.gpbo_posterior_acq_i8c):
            assert fn(p, M_, p, N, Np, d, lsp, p, p, 1.0, 0, 4.0, 0.0, 0, chunk, None, None, None, None, p, p, need - 1, None,
                      None) == short
    # (the int8 route refuses a length scale that is not positive AFTER the workspace check)
    bad = (C.c_double * 2)(0.5, 0.0)
    need = lib.gpbo_posterior_workspace_bytes_i8(Np, 512, Mc)
    i8 = lambda lsq, wb: lib.gpbo_posterior_acq_i8(p, Mc, p, N, Np, d, lsq, p, p, 1.0, 0, 4.0, 0.0, 0, 512, None, None, None, None,  # noqa: E731
                                                   p, p, wb, None, None)
    assert i8(C.cast(bad, C.c_void_p), need - 1) == short and i8(C.cast(bad, C.c_void_p), need) == ok

    need = lib.gpbo_posterior_workspace_bytes_f32(256, 1024, 3000)
    assert lib.gpbo_posterior_acq_f32(p, 3000, p, N, 256, d, lsp, p, p, 1.0, 0, 4.0, 0.0, 0.0, 0, 1024, None, None, None, None, p, p,
                                      need - 1, None, None) == short
    need = lib.gpbo_prepare_i8_bytes(Np)
    assert lib.gpbo_prepare_i8(p, Np, p, need - 1, None) == short

    stats = _lib.ScreenStats()
    need = lib.gpbo_rescore_workspace_bytes(Np, 4096, 512)
    assert lib.gpbo_rescore_f64(p, Mc, p, p, p, N, Np, d, lsp, p, p, 1.0, 0, 4.0, 0.0, 0, 1e-3, 64, 4096, 512, p, C.byref(stats), p,
                                need - 1, None) == short
    assert lib.gpbo_bound_select_f64(p, Mc, p, p, N, Np, d, lsp, p, p, 1.0, 0, 4.0, 0.0, 0, 64, 4096, 512, 0, p, C.byref(stats), p,
                                     need - 1, None) == short
    need = lib.gpbo_fps_order_workspace_bytes(N)
    assert lib.gpbo_fps_order_f64(p, p, N, d, lsp, 16, p, None, None, p, need - 1, None) == short
    need = lib.gpbo_acq_workspace_bytes()
    assert lib.gpbo_acq_argmax_f64(p, p, Mc, 0, 4.0, 0.0, 0, None, p, p, need - 1, None) == short
    need = lib.gpbo_nlml_grad_workspace_bytes(Np, d)
    assert lib.gpbo_nlml_grad_kern_f64(p, p, p, p, N, Np, d, lsp, 1, p, p, p, need - 1, None) == short
    need = lib.gpbo_nlml_hyper_workspace_bytes(Np, d)
    assert lib.gpbo_nlml_hyper_kern_f64(p, p, p, p, N, Np, d, lsp, 2, 1e-4, 3, p, p, p, p, need - 1, None) == short
    del buf


if __name__ == "__main__":
    with open(GOLDEN, "w") as f:
        json.dump(query_table(_lib.load()), f, separators=(",", ":"))
        f.write("\n")
