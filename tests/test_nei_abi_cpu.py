"""CPU-only checks of the noisy-expected-improvement boundary (csrc/nei.hip): the size contracts of gpbo_nei_fantasies_f64 /
gpbo_posterior_nei_kern_f64 / gpbo_nei_host_f64 and of the two workspace queries are refused on the host before anything is
launched, the Python layers refuse bad arguments without a GPU and before the library is touched, and no instance of the compiled
hot kernel needs scratch or has a barrier reachable with an LDS write in flight."""
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


def test_python_constants_and_signatures_match_the_header():
    repo = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    src = open(os.path.join(repo, "include", "gpbo.h")).read()
    defs = {k: int(v) for k, v in re.findall(r"#define\s+(GPBO_[A-Z_]+)\s+\(?(-?\d+)\)?", src)}
    assert defs["GPBO_NEI_MAX_S"] == _lib.NEI_MAX_S == 64
    assert defs["GPBO_VERSION"] == 151 and _lib.load().gpbo_version() == 151
    for name in ("gpbo_nei_fantasies_workspace_bytes", "gpbo_nei_fantasies_f64", "gpbo_posterior_nei_workspace_bytes",
                 "gpbo_posterior_nei_kern_f64", "gpbo_nei_host_f64"):
        assert name in _lib.SIGNATURES and name in src
        assert getattr(_lib.load(), name).argtypes == _lib.SIGNATURES[name][1]


def test_workspace_queries():
    lib = _lib.load()
    wf, wn = lib.gpbo_nei_fantasies_workspace_bytes, lib.gpbo_posterior_nei_workspace_bytes
    assert wf(128, 16) > 0 and wn(128, 512, 1000, 16) > 0
    assert wf(4096, 64) > 0 and wn(4096, 1 << 17, 1 << 21, 64) > 0
    for S in (0, 65, -1):
        assert wf(128, S) == -1 and wn(128, 512, 1000, S) == -1
    assert wf(100, 16) == -1 and wf(0, 16) == -1 and wn(100, 512, 1000, 16) == -1                  # Np granule
    assert wn(128, 500, 1000, 16) == -1 and wn(128, 0, 1000, 16) == -1 and wn(128, (1 << 24) + 512, 1000, 16) == -1   # chunk
    assert wn(128, 512, 0, 16) == -1 and wn(128, 512, -3, 16) == -1                                # M < 1
    prev = 0
    for S in range(1, 65):
        n = wn(256, 1024, 5000, S)
        assert n >= prev and n % 256 == 0 and wf(256, S) % 256 == 0
        prev = n
    # the scoring workspace holds the workspace of a ONE-chunk pass, the transposed weights and two dense vectors
    one_chunk = lib.gpbo_posterior_workspace_bytes(256, 1024, 1024)
    assert one_chunk + 8 * 256 * 64 + 2 * 8 * 5000 <= wn(256, 1024, 5000, 64) < lib.gpbo_posterior_workspace_bytes(256, 1024, 5000)


def test_scoring_entry_point_checks_its_size_contracts_on_the_host():
    lib = _lib.load()
    buf, p = _fake_pointer()
    ls = (C.c_double * 16)(*([0.5] * 16))
    lsp = C.cast(ls, C.c_void_p)
    need = lib.gpbo_posterior_nei_workspace_bytes(128, 512, 1000, 16)

    def call(M=1000, N=100, Np=128, d=2, lsp=lsp, kernel=0, U0=p, A=p, best=p, S=16, prior_var=1.000001, xi=0.0, chunk=512,
             mu=None, ldm=0, res=p, work=p, wbytes=need):
        return lib.gpbo_posterior_nei_kern_f64(p, M, p, N, Np, d, lsp, kernel, U0, A, best, S, prior_var, xi, 0, chunk, mu, ldm,
                                               None, None, res, work, wbytes, None)

    assert call(S=0) == -1 and call(S=65) == -1
    assert call(d=0) == -1 and call(d=17) == -1
    assert call(chunk=500) == -1 and call(chunk=0) == -1 and call(chunk=(1 << 24) + 512) == -1
    assert call(M=0) == -1 and call(N=0) == -1 and call(Np=100) == -1 and call(Np=256) == -1   # Np is gpbo_padded_n(N)
    assert call(kernel=3) == -1 and call(kernel=-1) == -1
    bad = (C.c_double * 2)(0.5, 0.0)
    assert call(lsp=C.cast(bad, C.c_void_p)) == -1
    assert call(prior_var=0.0) == -1 and call(prior_var=float("nan")) == -1 and call(prior_var=float("inf")) == -1
    assert call(xi=float("nan")) == -1 and call(xi=float("inf")) == -1
    assert call(mu=p, ldm=999) == -1                                # a dense output narrower than M
    assert call(U0=None) == -1 and call(A=None) == -1 and call(best=None) == -1 and call(res=None) == -1
    assert call(work=None) == -1 and call(lsp=None) == -1
    assert call(U0=C.c_void_p(p.value + 8)) == -1                   # the variance kernel's operand must be 16-byte aligned
    # a workspace one byte short, or not 256-byte aligned: after the arguments, before any HIP call
    assert call(wbytes=need - 1) == -3
    assert call(work=C.c_void_p(p.value + 8)) == -3
    assert call(kernel=2, wbytes=need - 1) == -3 and call(mu=p, ldm=1000, wbytes=need - 1) == -3
    del buf


def test_fantasies_entry_point_checks_its_size_contracts_on_the_host():
    lib = _lib.load()
    buf, p = _fake_pointer()
    need = lib.gpbo_nei_fantasies_workspace_bytes(128, 16)

    def call(K0d=p, U0=p, U=p, y=p, N=100, Np=128, Z=p, E=p, sd=0.3, S=16, A=p, F=p, best=p, work=p, wbytes=need):
        return lib.gpbo_nei_fantasies_f64(K0d, U0, U, y, N, Np, Z, E, sd, S, A, F, best, work, wbytes, None)

    assert call(S=0) == -1 and call(S=65) == -1
    assert call(Np=100) == -1 and call(N=129) == -1 and call(N=0) == -1
    assert call(sd=-0.1) == -1 and call(sd=float("nan")) == -1 and call(sd=float("inf")) == -1
    for name in ("K0d", "U0", "U", "y", "Z", "E", "A", "F", "best", "work"):
        assert call(**{name: None}) == -1
    for name in ("K0d", "U0", "U"):
        assert call(**{name: C.c_void_p(p.value + 8)}) == -1       # the GEMM's operands must be 16-byte aligned
    assert call(wbytes=need - 1) == -3
    assert call(work=C.c_void_p(p.value + 8)) == -3
    assert call(sd=0.0, wbytes=need - 1) == -3                      # rho = delta is legal
    del buf


def test_host_entry_point_checks_its_size_contracts_on_the_host():
    lib = _lib.load()
    buf, p = _fake_pointer()
    ls = (C.c_double * 16)(*([0.5] * 16))
    lsp = C.cast(ls, C.c_void_p)

    def call(M=1000, N=100, d=2, lsp=lsp, kernel=0, j1=0.09, j2=0.0, delta=1e-6, S=16, xi=0.0, chunk=0, res=p, info=p):
        return lib.gpbo_nei_host_f64(p, p, N, d, lsp, kernel, j1, j2, delta, p, M, p, p, S, xi, chunk, None, None, None, None,
                                     None, res, info)

    assert call(S=0) == -1 and call(S=65) == -1
    assert call(d=0) == -1 and call(d=17) == -1
    assert call(chunk=500) == -1
    assert call(M=0) == -1 and call(N=0) == -1 and call(kernel=3) == -1
    assert call(delta=0.0) == -1 and call(delta=-1e-6) == -1 and call(delta=0.1) == -1 and call(delta=float("nan")) == -1
    assert call(j1=float("inf")) == -1 and call(xi=float("nan")) == -1
    bad = (C.c_double * 2)(0.5, -1.0)
    assert call(lsp=C.cast(bad, C.c_void_p)) == -1
    assert call(res=None) == -1 and call(info=None) == -1
    del buf


class _NoLibrary:
    """Stands in for _lib.load(): a refusal that reaches the library fails the test."""

    def __call__(self, *a, **k):
        raise AssertionError("the library was touched before the arguments were refused")


def test_python_layers_refuse_bad_arguments_before_the_library_is_touched(monkeypatch):
    from bayesian_optimisation_amd import PointSelector, PointSelectorHost
    from bayesian_optimisation_amd import host_binding as H
    from bayesian_optimisation_amd import nei as NEI

    assert NEI.nei_params(16, 0) == (16, 0, 0.0, 1e-6)
    assert NEI.nei_params(np.int64(64), 3, 0.5, 1e-4, rho=1e-4) == (64, 3, 0.5, 1e-4)
    Z, E = NEI.nei_draws(5, 3, 7)
    rng = np.random.default_rng(7)
    assert Z.shape == E.shape == (3, 5) and np.array_equal(Z, rng.standard_normal((3, 5)))
    assert np.array_equal(E, rng.standard_normal((3, 5)))
    for bad in (dict(n_fantasies=0), dict(n_fantasies=65), dict(n_fantasies=2.0), dict(n_fantasies=True), dict(seed=-1),
                dict(seed=1.5), dict(xi=float("nan")), dict(xi=float("inf")), dict(delta=0.0), dict(delta=-1.0),
                dict(delta=float("nan")), dict(delta=0.1, rho=0.09)):
        kw = dict(n_fantasies=16, seed=0)
        kw.update(bad)
        with pytest.raises(ValueError):
            NEI.nei_params(**kw)
    with pytest.raises(ValueError):
        NEI.nei_best([0.0, 1.0], 3)
    with pytest.raises(ValueError):
        NEI.nei_best([0.0, np.nan, 1.0], 3)

    lib = _lib.load()   # (the selector classes bind it in their constructors)
    host = PointSelectorHost(ard="hyper")
    monkeypatch.setattr(_lib, "load", _NoLibrary())
    for fn in ("gpbo_nei_host_f64", "gpbo_nei_fantasies_f64", "gpbo_posterior_nei_kern_f64"):
        monkeypatch.setattr(lib, fn, _NoLibrary(), raising=False)
    X, y, Xs = np.zeros((4, 2)), np.zeros(4), np.zeros((10, 2))
    for kw in (dict(n_fantasies=0), dict(n_fantasies=65), dict(seed=-1), dict(delta=0.0), dict(delta=1.0), dict(xi=float("nan")),
               dict(best=[0.0]), dict(jitter1=1e-8, jitter2=0.0)):
        with pytest.raises(ValueError):
            H.select_nei(X, y, [1.0, 1.0], Xs, **kw)
    with pytest.raises(ValueError):
        H.select_nei(np.zeros((4, 17)), y, np.ones(17), np.zeros((10, 17)))                          # d = 17
    with pytest.raises(ValueError):
        H.select_nei(X, y, [1.0, 1.0], np.zeros((10, 3)))                                            # shapes
    with pytest.raises(ValueError, match="kernel"):
        H.select_nei(X, y, [1.0, 1.0], Xs, kernel="rbf")
    # the selector classes: the options NEI does not serve are named; bad parameters come before "call update_surrogate() first"
    with pytest.raises(ValueError, match="ard='marginal'"):
        PointSelector(ard="marginal").noisy_expected_improvement()
    for precision in ("fp32", "i8", "i8c"):
        with pytest.raises(ValueError, match="precision"):
            PointSelector(precision=precision).noisy_expected_improvement()
    with pytest.raises(ValueError, match="dense_outputs"):
        PointSelector(dense_outputs=False).noisy_expected_improvement()
    for ps in (PointSelector(), PointSelector(ard="hyper", kernel="matern52"), host):
        for kw in (dict(n_fantasies=0), dict(n_fantasies=65), dict(seed=-1), dict(delta=0.0), dict(xi=float("inf"))):
            with pytest.raises(ValueError):
                ps.noisy_expected_improvement(**kw)
        with pytest.raises(RuntimeError, match="update_surrogate"):
            ps.noisy_expected_improvement()


def _kernel_sizes(asm):
    return {re.search(r"\.name:\s+(\S+)", b).group(1): int(re.search(r"\.private_segment_fixed_size:\s+(\d+)", b).group(1))
            for b in asm.split("  - .agpr_count:")[1:]}


@needs_hipcc
def test_no_instance_of_the_nei_kernel_needs_scratch(tmp_path):
    """A fresh csrc/nei.hip compiles for gfx950 and no instance of the hot kernel (1 .. 4 column tiles of 16 fantasies) spills:
    4 x CT accumulator tiles and the operands of the unrolled k steps stay in registers; it runs on the fp64 matrix cores."""
    asm = open(cb.assemble("nei", str(tmp_path))).read()
    sizes = _kernel_sizes(asm)
    hot = {k: v for k, v in sizes.items() if "nei_kernel" in k}
    assert len(hot) == 4, sorted(sizes)
    for CT in range(1, 5):
        assert any(f"nei_kernelILi{CT}E" in k for k in hot), CT
    assert max(hot.values()) == 0, hot
    assert max(sizes.values()) == 0, sizes
    for other in ("nei_prep_kernel", "nei_pack_kernel", "nei_resid_kernel", "nei_sum_kernel", "nei_rowmin_kernel"):
        assert any(other in k for k in sizes)
    assert "v_mfma_f64_16x16x4" in asm


@needs_hipcc
def test_no_barrier_of_the_nei_kernels_is_reachable_with_an_lds_write_in_flight(capsys):
    assert "nei" in cb.UNITS
    rc = cb.main(["nei"])
    out = capsys.readouterr().out
    assert rc == 0, out
    assert "0 reachable" in out
