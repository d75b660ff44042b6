"""CPU-only checks of the boundary: libgpbo.so loads without a GPU and exports every symbol that
include/gpbo.h declares; the Python binding table matches the header; the product path refuses to
run without a GPU instead of falling back to anything."""
import ctypes
import os
import re

import numpy as np
import pytest

from bayesian_optimisation_amd import _lib

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _header_functions():
    src = open(os.path.join(REPO, "include", "gpbo.h")).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    return sorted(set(re.findall(r"\b(gpbo_[a-z0-9_]+)\s*\(", src)))


def test_library_is_built_and_loads_without_gpu():
    assert os.path.exists(_lib.LIB_PATH), "run bayesian_optimisation_amd/csrc/build.sh (or __graft_entry__.build())"
    lib = _lib.load()
    assert lib.gpbo_version() == 151
    assert lib.gpbo_padded_n(1) == 128 and lib.gpbo_padded_n(128) == 128 and lib.gpbo_padded_n(129) == 256
    assert b"workspace" in lib.gpbo_strerror(-3)


def test_every_header_symbol_is_exported_and_bound():
    names = _header_functions()
    assert len(names) >= 15
    raw = ctypes.CDLL(_lib.LIB_PATH)
    for n in names:
        assert hasattr(raw, n), f"{n} declared in include/gpbo.h but not exported by libgpbo.so"
        assert n in _lib.SIGNATURES, f"{n} has no ctypes prototype in _lib.SIGNATURES"
    assert sorted(_lib.SIGNATURES) == names


def test_argument_validation_needs_no_gpu():
    lib = _lib.load()
    # null pointers / bad sizes are rejected on the host before anything is launched
    assert lib.gpbo_kxx_f64(None, 4, 2, None, 1e-4, 1e-6, None, 128, None) == -1
    assert lib.gpbo_posterior_workspace_bytes(100, 512, 10) == -1      # Np not a multiple of 128
    assert lib.gpbo_posterior_workspace_bytes(128, 500, 10) == -1      # chunk not a multiple of 512
    assert lib.gpbo_posterior_workspace_bytes(128, 512, 1000) > 128 * 512 * 8
    assert lib.gpbo_factorise_workspace_bytes(256) == 8 * (2 * 256 * 256 + 256 * 64 + 256)
    assert lib.gpbo_nlml_grid_max_n() == 176 and lib.gpbo_nlml_grid_wave_max_n() == 64


def test_every_compute_entry_point_rejects_null_arguments():
    """All-NULL / all-zero arguments come back as GPBO_ERR_ARG from every compute call, before any HIP call."""
    import ctypes as C

    lib = _lib.load()
    skip = {"gpbo_version", "gpbo_nlml_grid_max_n", "gpbo_nlml_grid_wave_max_n", "gpbo_gemm_f64", "gpbo_gemm_tri_f64",  # gemm: M = 0 is a valid empty product
            "gpbo_profile_create", "gpbo_profile_read", "gpbo_profile_read_kstar", "gpbo_profile_read_qei", "gpbo_profile_reset",
            "gpbo_profile_destroy"}
    checked = 0
    for name, (res, args) in _lib.SIGNATURES.items():
        if res is not C.c_int or name in skip:
            continue
        a = [None if t is _lib.Pointer else (0.0 if t is C.c_double else 0) for t in args]
        assert getattr(lib, name)(*a) == -1, name
        checked += 1
    assert checked >= 61   # (the 70 functions that return a status, less the nine of them in `skip`)


def _header_prototypes():
    """name -> (return kind, [argument kinds]) of every prototype of include/gpbo.h; kinds: "ptr" (any `T *`), "str"
    (`const char *` as a return), "i64", "i32" (int32_t or int), "f64", "void"."""
    src = open(os.path.join(REPO, "include", "gpbo.h")).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    src = re.sub(r"//[^\n]*", "", src)
    src = re.sub(r"^\s*#.*$", "", src, flags=re.M)
    src = re.sub(r"typedef\s+struct\s+\w*\s*\{.*?\}\s*\w+\s*;", "", src, flags=re.S)
    src = src.replace('extern "C" {', "")
    scalar = {"int64_t": "i64", "int32_t": "i32", "int": "i32", "double": "f64", "void": "void"}

    def kind(decl, is_return=False):
        words = decl.replace("*", " * ").split()
        if "*" in words:
            return "str" if is_return and words[:3] == ["const", "char", "*"] else "ptr"
        words = [w for w in words if w != "const"]
        return scalar[words[0]]   # (an argument: the type, then its name)

    protos = {}
    for ret, name, args in re.findall(r"([\w\s\*]+?)\b(gpbo_[a-z0-9_]+)\s*\(([^()]*)\)\s*;", src):
        args = [a.strip() for a in args.split(",")]
        assert name not in protos, name
        protos[name] = (kind(ret, True), [] if args == ["void"] else [kind(a) for a in args])
    return protos


def _table_kind(t):
    if t is None:
        return "void"
    if t is ctypes.c_char_p:
        return "str"
    if issubclass(t, (ctypes.c_void_p, ctypes._Pointer)):
        return "ptr"
    return {ctypes.c_int64: "i64", ctypes.c_int32: "i32", ctypes.c_int: "i32", ctypes.c_double: "f64"}[t]


def _table_mismatches(table, protos):
    """Every way `table` (name -> (restype, argtypes)) departs from the header's prototypes, as strings."""
    bad = [f"{n}: only in the {'table' if n in table else 'header'}" for n in sorted(set(table) ^ set(protos))]
    for name in sorted(set(table) & set(protos)):
        res, args = table[name]
        ret, kinds = protos[name]
        if _table_kind(res) != ret:
            bad.append(f"{name}: returns {ret}, bound as {_table_kind(res)}")
        if len(args) != len(kinds):
            bad.append(f"{name}: {len(kinds)} arguments, {len(args)} bound")
        bad += [f"{name}: argument {i} is {k}, bound as {_table_kind(t)}"
                for i, (t, k) in enumerate(zip(args, kinds)) if _table_kind(t) != k]
    return bad


def test_every_prototype_matches_its_ctypes_signature():
    """Return type and every argument, in order and by width, of include/gpbo.h against _lib.SIGNATURES: an int32 bound
    where the header says int64_t would shift every later argument of the call without an error."""
    protos = _header_prototypes()
    assert sorted(protos) == _header_functions() and len(protos) >= 97   # every function of the header parsed
    assert _table_mismatches(_lib.SIGNATURES, protos) == []


def _seeded(edit):
    res, args = _lib.SIGNATURES["gpbo_posterior_acq_kern_f64"]   # (Xs, M, X, N, Np: int64, d: int32, ls_host, ...)
    args = list(args)
    edit(args)
    return dict(_lib.SIGNATURES, gpbo_posterior_acq_kern_f64=(res, args))


def _swap(i, j):
    def edit(args):
        args[i], args[j] = args[j], args[i]
    return edit


@pytest.mark.parametrize("edit,what", [(lambda args: args.pop(9), "24 bound"), (_swap(4, 5), "argument 4 is i64, bound as i32"),
                                       (_swap(0, 1), "argument 0 is ptr, bound as i64")],
                         ids=["dropped argument", "int32 for int64", "scalar for pointer"])
def test_the_signature_check_sees_a_seeded_mistake(edit, what):
    bad = _table_mismatches(_seeded(edit), _header_prototypes())
    assert bad and all(b.startswith("gpbo_posterior_acq_kern_f64: ") for b in bad) and any(what in b for b in bad), bad


def _address_seen_by_the_callee(obj):
    """What a C function receives for `obj` through an argument of type _lib.Pointer: memmove(dst, src, 0) returns dst."""
    memmove = ctypes.CDLL(None).memmove
    memmove.restype, memmove.argtypes = ctypes.c_void_p, [_lib.Pointer, _lib.Pointer, ctypes.c_size_t]
    return memmove(obj, ctypes.create_string_buffer(1), 0)


def test_pointer_arguments_take_arrays_and_tensors_as_they_are():
    import torch

    arr = (ctypes.c_int64 * 4)()
    a = np.zeros((4, 6))
    t = torch.zeros((4, 6), dtype=torch.float64)
    word = ctypes.c_int32(0)
    assert _lib.Pointer.from_param(None) is None   # (ctypes passes None as NULL)
    assert _address_seen_by_the_callee(ctypes.c_void_p(4096)) == 4096
    assert _address_seen_by_the_callee(4096) == 4096
    assert _address_seen_by_the_callee(arr) == ctypes.addressof(arr)
    assert _address_seen_by_the_callee(ctypes.byref(word)) == ctypes.addressof(word)
    assert _address_seen_by_the_callee(a) == a.ctypes.data and _address_seen_by_the_callee(a[1:, :]) == a.ctypes.data + 48
    assert _address_seen_by_the_callee(t) == t.data_ptr() and _address_seen_by_the_callee(t[2]) == t.data_ptr() + 96
    # a view that is not contiguous never reaches the library
    lib = _lib.load()
    for view in (a[:, ::2], a.T, t.t(), t[:, 1:]):
        with pytest.raises(ctypes.ArgumentError, match="contiguous"):
            lib.gpbo_kxx_f64(view, 4, 2, None, 1e-4, 1e-6, None, 128, None)
    with pytest.raises(ctypes.ArgumentError):
        lib.gpbo_kxx_f64(None, 4, 2, 1.5, 1e-4, 1e-6, None, 128, None)   # (a float is no pointer)


def test_checked_call_raises_with_the_function_name_and_the_status_text():
    lib = _lib.load()
    null = [None if t is _lib.Pointer else (0.0 if t is ctypes.c_double else 0)
            for t in _lib.SIGNATURES["gpbo_posterior_acq_kern_f64"][1]]
    with pytest.raises(_lib.GpboError) as by_check:
        _lib.check(lib.gpbo_posterior_acq_kern_f64(*null), "gpbo_posterior_acq_kern_f64")
    with pytest.raises(_lib.GpboError) as by_call:
        _lib.call(lib.gpbo_posterior_acq_kern_f64, *null)
    assert str(by_call.value) == str(by_check.value)
    assert str(by_call.value) == f"gpbo_posterior_acq_kern_f64: {lib.gpbo_strerror(-1).decode()} (status -1)"
    # another function and another status: a workspace of 8 bytes (refused before the pointers are touched)
    buf = (ctypes.c_char * 1024)()
    p = ctypes.c_void_p((ctypes.addressof(buf) + 255) & ~255)
    ls = (ctypes.c_double * 2)(0.5, 0.5)
    with pytest.raises(_lib.GpboError) as short:
        _lib.call(lib.gpbo_factorise_f64, p, p, 100, 2, ls, 1e-4, 1e-6, 128, p, p, p, p, p, 8, None)
    assert str(short.value) == f"gpbo_factorise_f64: {lib.gpbo_strerror(-3).decode()} (status -3)"
    # GPBO_OK returns (an empty product: nothing is launched)
    empty = [None if t is _lib.Pointer else (0.0 if t is ctypes.c_double else 0) for t in _lib.SIGNATURES["gpbo_gemm_f64"][1]]
    assert _lib.call(lib.gpbo_gemm_f64, *empty) is None


def test_size_contracts_are_checked_on_the_host():
    """Non-null pointers but sizes that break a documented contract: rejected without touching the pointers."""
    import ctypes as C

    lib = _lib.load()
    buf = (C.c_char * 1024)()
    p = C.c_void_p((C.addressof(buf) + 255) & ~255)  # 256-byte aligned like a device allocation; never dereferenced
    ls = (C.c_double * 16)(*([0.5] * 16))
    lsp = C.cast(ls, C.c_void_p)
    # factorise: Np must be gpbo_padded_n(N); workspace must be large enough
    assert lib.gpbo_factorise_f64(p, p, 100, 2, lsp, 1e-4, 1e-6, 256, p, p, p, p, p, 1 << 40, None) == -1
    assert lib.gpbo_factorise_f64(p, p, 100, 2, lsp, 1e-4, 1e-6, 128, p, p, p, p, p, 8, None) == -3
    # append: no room left in the padding; d beyond the compiled maximum; non-positive length scale
    assert lib.gpbo_append_f64(p, p, 128, 2, lsp, 1e-4, 1e-6, 128, p, p, None, p, p, p, p, 1 << 30, None) == -1
    assert lib.gpbo_append_f64(p, p, 10, 17, lsp, 1e-4, 1e-6, 128, p, p, None, p, p, p, p, 1 << 30, None) == -1
    bad = (C.c_double * 2)(0.5, 0.0)
    assert lib.gpbo_append_f64(p, p, 10, 2, C.cast(bad, C.c_void_p), 1e-4, 1e-6, 128, p, p, None, p, p, p, p, 1 << 30,
                               None) == -1
    assert lib.gpbo_append_f64(p, p, 10, 2, lsp, 1e-4, 1e-6, 128, p, p, None, p, p, p, p, 8, None) == -3
    assert lib.gpbo_append_workspace_bytes(128) == 8 * (3 * 128 + 8)
    # posterior: chunk granule, Np granule, unknown acquisition kind
    def post(Np, chunk, kind, wbytes=1 << 40):
        return lib.gpbo_posterior_acq_f64(p, 1000, p, 100, Np, 2, lsp, p, p, 1.0, kind, 4.0, 0.0, 0.0, 0, chunk,
                                          None, None, None, p, p, wbytes, None, None)
    assert post(100, 512, 0) == -1
    assert post(128, 500, 0) == -1
    assert post(128, 512, 7) == -1
    assert post(128, 1 << 25, 0) == -1   # chunk beyond GPBO_CHUNK_MAX
    assert post(128, 512, 0, wbytes=8) == -3
    # potrf / trtri: Np a multiple of 64
    assert lib.gpbo_potrf_f64(p, 100, p, p, None) == -1
    assert lib.gpbo_trtri_f64(p, p, 100, p, p, None) == -1
    # ARD grid: N beyond the in-LDS limit
    assert lib.gpbo_nlml_grid_f64(p, p, 177, 2, p, 4, 1e-4, p, None) == -1
    assert lib.gpbo_nlml_grid_wave_f64(p, p, 65, 2, p, 4, 1e-4, p, None) == -1 and lib.gpbo_nlml_grid_wave_f64(p, p, 8, 17, p, 4, 1e-4, p, None) == -1
    # fused factorisation: S is read by 16-byte LDS-DMA pieces - an 8-byte-offset view is refused, as are an odd or short ld
    p8 = C.c_void_p(p.value + 8)
    assert lib.gpbo_cholinv_f64(p8, 512, 256, p, None, None) == -1
    assert lib.gpbo_cholinv_f64(p, 511, 256, p, None, None) == -1
    assert lib.gpbo_cholinv_f64(p, 510, 256, p, None, None) == -1
    assert lib.gpbo_cholinv_f64(p, 2 * 32896, 32896, p, None, None) == -1   # beyond the plan's cap: factorise takes the chain


def test_batched_grid_workspace_contract_is_checked_on_the_host():
    """The one-launch ARD grid (csrc/ard.hip) at the BASELINE surrogate sizes: one byte short of the workspace query, or a
    workspace that is not 256-byte aligned, is GPBO_ERR_WORKSPACE in both likelihood modes; N beyond 32768 and G = 0 are
    GPBO_ERR_ARG.  The query is positive, never shrinks as G grows, and does not overflow at its largest sizes.  (The
    contract only: not the slot count or the cap behind it.)  Every call here is refused before anything is launched."""
    import ctypes as C

    lib = _lib.load()
    buf = (C.c_char * 1024)()
    p = C.c_void_p((C.addressof(buf) + 255) & ~255)   # never dereferenced
    ws = lib.gpbo_nlml_grid_batched_workspace_bytes
    entries = (lib.gpbo_nlml_grid_batched_f64, lib.gpbo_nlml_grid_batched_logdet_f64)
    for N in (2048, 4096, 8192):
        for G in (1, 64, 1100):
            need = ws(N, G)
            assert need > 0
            for fn in entries:
                assert fn(p, p, N, 2, p, G, 1e-4, p, p, need - 1, None) == -3, (N, G)
                for off in (8, 128):
                    assert fn(p, p, N, 2, p, G, 1e-4, p, C.c_void_p(p.value + off), need, None) == -3, (N, G, off)
    for fn in entries:
        assert fn(p, p, 32769, 2, p, 8, 1e-4, p, p, 1 << 62, None) == -1
        assert fn(p, p, 2048, 2, p, 0, 1e-4, p, p, 1 << 62, None) == -1
    assert ws(32769, 8) == -1 and ws(2048, 0) == -1
    for N in (1, 65, 2048, 2049, 4096, 4097, 8192, 32768):
        prev = 0
        for G in (1, 2, 31, 32, 127, 128, 508, 509, 512, 513, 1100, 1 << 20, 1 << 30):
            b = ws(N, G)
            assert b >= prev and b >= 8 * G, (N, G, b, prev)   # (G cells of length scales at least: no wrap-around)
            prev = b
    assert 8 << 30 <= ws(32768, 1 << 30) < 1 << 62


def test_library_path_override(monkeypatch):
    """GPBO_LIB=/path/to/variant.so makes _lib load that file: A/B tools never overwrite the installed library."""
    import importlib
    import subprocess
    import sys

    code = (f"import sys; sys.path.insert(0, {REPO!r}); import os; os.environ['GPBO_LIB'] = '/nonexistent/variant.so'\n"
            "from bayesian_optimisation_amd import _lib\n"
            "try:\n    _lib.load(); print('loaded')\nexcept _lib.GpboError as e:\n    print('refused', '/nonexistent/variant.so' in str(e))\n")
    out = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=120)
    assert out.stdout.strip() == "refused True", out.stdout + out.stderr
    for f in os.listdir(os.path.join(REPO, "tools")):
        if f.endswith(".sh"):
            txt = open(os.path.join(REPO, "tools", f)).read()
            assert "bayesian_optimisation_amd/libgpbo.so" not in txt.replace("cp bayesian_optimisation_amd/libgpbo.so ab_libs/", ""), \
                f"tools/{f} touches the installed library"


def test_product_path_fails_loudly_without_gpu():
    import torch

    if torch.cuda.is_available():
        pytest.skip("GPU present")
    from bayesian_optimisation_amd import DeviceGP, PointSelector

    with pytest.raises(_lib.GpboError):
        DeviceGP()
    ps = PointSelector()
    ps.measured_pts = np.zeros((2, 1))
    ps.measured_vals = np.zeros(2)
    ps.predicted_pts = np.zeros((5, 1))
    ps.feature_domain = [5]
    ps.length_scales = np.linspace(0.1, 1, 5)
    with pytest.raises(_lib.GpboError):
        ps.update_surrogate()


def test_product_package_does_not_import_the_oracle():
    pkg = os.path.join(REPO, "bayesian_optimisation_amd")
    for root, _, files in os.walk(pkg):
        for f in files:
            if f.endswith((".py", ".hip", ".h", ".sh")):
                txt = open(os.path.join(root, f)).read()
                assert "oracle" not in txt.replace("no CPU", ""), f"{f} mentions the oracle"


def test_python_constants_match_the_header():
    src = open(os.path.join(REPO, "include", "gpbo.h")).read()
    defs = {k: int(v) for k, v in re.findall(r"#define\s+(GPBO_[A-Z_]+)\s+\(?(-?\d+)\)?", src)}
    assert defs["GPBO_NPAD"] == _lib.NPAD and defs["GPBO_CHUNK_GRANULE"] == _lib.CHUNK_GRANULE
    assert defs["GPBO_MAX_D"] == _lib.MAX_D and defs["GPBO_ACQ_LCB"] == _lib.ACQ_LCB and defs["GPBO_ACQ_EI"] == _lib.ACQ_EI
    assert defs["GPBO_VERSION"] == _lib.load().gpbo_version()


def test_loader_refuses_a_second_hip_runtime():
    """Two HIP runtimes in one process do not share the device (round 1: torch.cuda.is_available() turned False after a
    host-pointer call through the other one).  If the system's libamdhip64 is already mapped when the package loads -
    and PyTorch's copy is what the loader binds to - loading must fail with a clear message, not at the first kernel."""
    import subprocess
    import sys

    sysrt = "/opt/rocm/lib/libamdhip64.so"
    if not os.path.exists(sysrt):
        pytest.skip("no system ROCm runtime in this image")
    code = (
        "import ctypes, sys\n"
        f"sys.path.insert(0, {REPO!r})\n"
        f"ctypes.CDLL({sysrt!r}, mode=ctypes.RTLD_GLOBAL)\n"
        "from bayesian_optimisation_amd import _lib\n"
        "try:\n"
        "    _lib.load()\n"
        "    print('loaded', len(_lib.mapped_hip_runtimes()))\n"
        "except _lib.GpboError as e:\n"
        "    print('refused' if 'two different HIP runtimes' in str(e) else 'other: ' + str(e))\n"
    )
    out = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stderr[-1500:]
    # either PyTorch is absent / shares the system runtime (one copy mapped: fine) or the clash is reported
    assert out.stdout.strip() in ("refused", "loaded 1"), out.stdout


def test_build_from_a_clean_tree(tmp_path):
    """The build recipe of __graft_entry__.build() (csrc/build.sh) on a tree that has neither objects nor a library:
    every translation unit compiles for gfx950 and the fresh library exports every symbol of include/gpbo.h."""
    import shutil
    import subprocess

    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    if not os.path.exists(hipcc):
        pytest.skip("no hipcc in this environment")
    src = os.path.join(REPO, "bayesian_optimisation_amd", "csrc")
    dst = tmp_path / "bayesian_optimisation_amd" / "csrc"
    dst.mkdir(parents=True)
    for f in os.listdir(src):
        if f.endswith((".hip", ".h", ".sh")):
            shutil.copy(os.path.join(src, f), dst / f)
    (tmp_path / "include").mkdir()
    shutil.copy(os.path.join(REPO, "include", "gpbo.h"), tmp_path / "include" / "gpbo.h")
    assert not (dst / "build").exists()
    subprocess.run(["bash", str(dst / "build.sh")], check=True, capture_output=True, timeout=900)
    lib = tmp_path / "bayesian_optimisation_amd" / "libgpbo.so"
    assert lib.exists()
    raw = ctypes.CDLL(str(lib))
    for n in _header_functions():
        assert hasattr(raw, n), n
    raw.gpbo_version.restype = ctypes.c_int
    assert raw.gpbo_version() == _lib.load().gpbo_version()
