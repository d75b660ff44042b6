"""ctypes binding of libgpbo.so (the C ABI declared in include/gpbo.h).

The library is built in-tree by `bayesian_optimisation_amd/csrc/build.sh` (or `__graft_entry__.build()`).
There is NO fallback: if the shared object is missing or a symbol is absent, loading raises.
"""
from __future__ import annotations

import ctypes as C
import os

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
# GPBO_LIB=/path/to/variant.so: A/B and timing-only builds (tools/ab*.sh, tools/build_variant.sh) are loaded from where
# they were built; the installed library is never overwritten by a tool.
LIB_PATH = os.environ.get("GPBO_LIB") or os.path.join(_HERE, "libgpbo.so")

GPBO_OK = 0
ACQ_LCB = 0
ACQ_EI = 1
NPAD = 128
CHUNK_GRANULE = 512
MAX_D = 16          # every route
MAX_D_ANY = 1024    # fp64 route (factorise, score): any d up to this, slow path beyond MAX_D
I8_MAX_N = 16384
BATCH_MAX_Q = 64
FANTASY_BELIEVER = 0
FANTASY_LIE = 1
REFINE_MAX_P = 4096
TS_MAX_PATHS = 64
TS_MAX_FEATURES = 16384
HYPER_MEAN = 1      # gpbo_nlml_hyper_f64: fit the constant mean
HYPER_SCALE = 2     # ... and the signal variance
HYPER_CELLS_MAX_N = 64   # gpbo_nlml_hyper_cells_f64: a cell's rows are the lanes of one wave
ENSEMBLE_MAX_S = 64      # gpbo_ensemble_acq_f64: models per call
NEI_MAX_S = 64           # gpbo_posterior_nei_kern_f64: fantasies per call
MES_MAX_LEVELS = 64      # gpbo_mes_log_survival_f64: levels per call
MES_MAX_S = 64           # gpbo_mes_acq_f64: sampled minima per call
MES_WORK_BYTES = 1 << 20   # the workspace of both: a constant
CONS_BASE_NONE, CONS_BASE_EI, CONS_BASE_PI = 0, 1, 2   # gpbo_constrained_acq_f64: the base term (GPBO_CONS_BASE_*)
CONS_BASE_IDS = {"none": CONS_BASE_NONE, "ei": CONS_BASE_EI, "pi": CONS_BASE_PI}
CONS_MAX_C = 8             # ... constraints per call
CONS_WORK_BYTES = 16640    # ... its workspace: a constant
EHVI_MAX_P = 128           # gpbo_ehvi_acq_f64: front points per call (GPBO_EHVI_MAX_P)
EHVI_WORK_BYTES = 16640    # ... its workspace: a constant
# covariance families of the gpbo_*_kern_f64 entry points (include/gpbo.h: GPBO_KERNEL_*)
KERNEL_IDS = {"se": 0, "matern32": 1, "matern52": 2}


def kernel_id(kernel: str) -> int:
    """GPBO_KERNEL_* of a family by name; ValueError for anything else."""
    try:
        return KERNEL_IDS[kernel]
    except (KeyError, TypeError):
        raise ValueError(f"kernel must be one of {sorted(KERNEL_IDS)}, got {kernel!r}") from None


_address = C.c_void_p.from_param   # an integer as a pointer argument (cheaper than a c_void_p object)
_NO_BYTES = C.c_char * 0


class Pointer(C.c_void_p):
    """A `T *` argument.  Arrays and tensors go in as they are: None (NULL), a C-contiguous numpy.ndarray, anything with
    data_ptr() / is_contiguous() (a torch tensor: this module does not import torch), and whatever c_void_p takes (a
    c_void_p, an integer, a ctypes array or pointer, byref(...)).  A view that is not contiguous is refused before the call
    (ctypes.ArgumentError): the library would read the rows of another matrix."""

    @classmethod
    def from_param(cls, obj):
        # (ordered by how often each kind arrives: this runs once per pointer argument of every call)
        if obj is None or type(obj) is C.c_void_p:
            return obj
        try:
            contiguous = obj.is_contiguous()
        except AttributeError:
            if isinstance(obj, np.ndarray):
                if not obj.flags.c_contiguous:
                    raise TypeError("an array passed to the library must be C-contiguous") from None
                try:
                    return _NO_BYTES.from_buffer(obj)   # (a ctypes array at its address: a fifth of the cost of obj.ctypes)
                except TypeError:
                    return C.c_void_p(obj.ctypes.data)  # a read-only array has no writable buffer to take
            return obj if isinstance(obj, C.c_void_p) else C.c_void_p.from_param(obj)
        if not contiguous:
            raise TypeError("a tensor passed to the library must be contiguous")
        return _address(obj.data_ptr())


_p = Pointer
_i64 = C.c_int64
_i32 = C.c_int32
_f64 = C.c_double

# name -> (restype, argtypes); mirrors include/gpbo.h one to one
SIGNATURES = {
    "gpbo_version": (C.c_int, []),
    "gpbo_strerror": (C.c_char_p, [C.c_int]),
    "gpbo_padded_n": (_i64, [_i64]),
    "gpbo_kxx_f64": (C.c_int, [_p, _i64, _i32, _p, _f64, _f64, _p, _i64, _p]),
    "gpbo_potrf_f64": (C.c_int, [_p, _i64, _p, _p, _p]),
    "gpbo_trtri_f64": (C.c_int, [_p, _p, _i64, _p, _p, _p]),
    "gpbo_cholinv_f64": (C.c_int, [_p, _i64, _i64, _p, _p, _p]),
    "gpbo_cholinv_plan": (C.c_int, [_i64, _p, _p, _p, _p, _p]),
    "gpbo_cholinv_tiles_f64": (C.c_int, [_p, _i64, _i64, _p, _i32, _p, _i64, _i32, _i32, _p]),
    "gpbo_alpha_f64": (C.c_int, [_p, _p, _i64, _i64, _p, _p, _p]),
    "gpbo_factorise_workspace_bytes": (_i64, [_i64]),
    "gpbo_factorise_f64": (C.c_int, [_p, _p, _i64, _i32, _p, _f64, _f64, _i64, _p, _p, _p, _p, _p, _i64, _p]),
    "gpbo_select_next_host_f64": (C.c_int, [_p, _p, _i64, _i32, _p, _f64, _f64, _p, _i64, _i32, _f64, _f64, _f64, _i64,
                                            _p, _p, _p, _p, _p, _p]),
    "gpbo_select_qei_host_f64": (C.c_int, [_p, _p, _i64, _i32, _p, _f64, _f64, _p, _i64, _f64, _f64, _p, _i32, _i64, _p,
                                           _p, _p]),
    "gpbo_nlml_grid_host_f64": (C.c_int, [_p, _p, _i64, _i32, _p, _i64, _f64, _p]),
    "gpbo_nlml_grid_logdet_host_f64": (C.c_int, [_p, _p, _i64, _i32, _p, _i64, _f64, _p]),
    "gpbo_append_workspace_bytes": (_i64, [_i64]),
    "gpbo_append_f64": (C.c_int, [_p, _p, _i64, _i32, _p, _f64, _f64, _i64, _p, _p, _p, _p, _p, _p, _p, _i64, _p]),
    "gpbo_scale_points_f64": (C.c_int, [_p, _i64, _i64, _i32, _p, _p, _p]),
    "gpbo_kstar_mu_f64": (C.c_int, [_p, _i64, _p, _i64, _i64, _i32, _p, _p, _f64, _i64, _p, _i64, _p, _p]),
    "gpbo_posterior_workspace_bytes": (_i64, [_i64, _i64, _i64]),
    "gpbo_posterior_acq_f64": (C.c_int, [_p, _i64, _p, _i64, _i64, _i32, _p, _p, _p, _f64, _i32, _f64, _f64, _f64,
                                         _i64, _i64, _p, _p, _p, _p, _p, _i64, _p, _p]),
    "gpbo_profile_create": (C.c_int, [_i32, C.POINTER(C.c_void_p)]),
    "gpbo_profile_reset": (None, [_p]),
    "gpbo_profile_read": (C.c_int, [_p, C.POINTER(_f64), C.POINTER(_i64), C.POINTER(_i64)]),
    "gpbo_profile_read_kstar": (C.c_int, [_p, C.POINTER(_f64), C.POINTER(_i64), C.POINTER(_i64)]),
    "gpbo_profile_read_qei": (C.c_int, [_p, C.POINTER(_f64), C.POINTER(_i64), C.POINTER(_i64)]),
    "gpbo_profile_destroy": (None, [_p]),
    "gpbo_qei_workspace_bytes": (_i64, [_i64, _i64, _i64]),
    "gpbo_posterior_qei_f64": (C.c_int, [_p, _i64, _p, _i64, _i64, _i32, _p, _p, _p, _f64, _f64, _f64, _p, _i32, _i64,
                                         _i64, _p, _p, _p, _i64, _p, _p]),
    "gpbo_padded_n_f32": (_i64, [_i64]),
    "gpbo_prepare_f32": (C.c_int, [_p, _p, _i64, _p, _p, _i64, _p]),
    "gpbo_posterior_workspace_bytes_f32": (_i64, [_i64, _i64, _i64]),
    "gpbo_posterior_acq_f32": (C.c_int, [_p, _i64, _p, _i64, _i64, _i32, _p, _p, _p, _f64, _i32, _f64, _f64, _f64,
                                         _i64, _i64, _p, _p, _p, _p, _p, _p, _i64, _p, _p]),
    "gpbo_prepare_i8_bytes": (_i64, [_i64]),
    "gpbo_prepare_i8": (C.c_int, [_p, _i64, _p, _i64, _p]),
    "gpbo_posterior_workspace_bytes_i8": (_i64, [_i64, _i64, _i64]),
    "gpbo_posterior_acq_i8": (C.c_int, [_p, _i64, _p, _i64, _i64, _i32, _p, _p, _p, _f64, _i32, _f64, _f64, _i64, _i64,
                                        _p, _p, _p, _p, _p, _p, _i64, _p, _p]),
    "gpbo_posterior_acq_i8c": (C.c_int, [_p, _i64, _p, _i64, _i64, _i32, _p, _p, _p, _f64, _i32, _f64, _f64, _i64, _i64,
                                         _p, _p, _p, _p, _p, _p, _i64, _p, _p]),
    "gpbo_posterior_prefix_f64": (C.c_int, [_p, _i64, _p, _i64, _i64, _i32, _p, _p, _p, _f64, _i32, _f64, _f64, _i64, _i64,
                                            _i64, _p, _p, _p, _p, _p, _i64, _p, _p]),
    "gpbo_bound_select_f64": (C.c_int, [_p, _i64, _p, _p, _i64, _i64, _i32, _p, _p, _p, _f64, _i32, _f64, _f64, _i64,
                                        _i64, _i64, _i64, _i64, _p, _p, _p, _i64, _p]),
    "gpbo_fps_order_workspace_bytes": (_i64, [_i64]),
    "gpbo_fps_order_f64": (C.c_int, [_p, _p, _i64, _i32, _p, _i64, _p, _p, _p, _p, _i64, _p]),
    "gpbo_fps_order_status": (C.c_int, [_p, _i64, _p, _p]),
    "gpbo_rescore_workspace_bytes": (_i64, [_i64, _i64, _i64]),
    "gpbo_rescore_f64": (C.c_int, [_p, _i64, _p, _p, _p, _i64, _i64, _i32, _p, _p, _p, _f64, _i32, _f64, _f64, _i64,
                                   _f64, _i64, _i64, _i64, _p, _p, _p, _i64, _p]),
    "gpbo_batch_workspace_bytes": (_i64, [_i64, _i64, _i32]),
    "gpbo_select_batch_f64": (C.c_int, [_p, _i64, _p, _i64, _i64, _i32, _p, _p, _p, _f64, _f64, _f64, _i32, _f64, _f64, _i32,
                                        _i32, _f64, _p, _p, _i64, _p, _p, _p, _p, _p, _i64, _p]),
    "gpbo_select_batch_host_f64": (C.c_int, [_p, _p, _i64, _i32, _p, _f64, _f64, _p, _i64, _i32, _f64, _f64, _i64, _i32, _i32,
                                             _f64, _p, _p, _p, _p, _p, _p]),
    "gpbo_posterior_grad_workspace_bytes": (_i64, [_i64, _i64]),
    "gpbo_posterior_grad_f64": (C.c_int, [_p, _i64, _p, _i64, _i64, _i32, _p, _p, _p, _f64, _i32, _f64, _f64, _p, _p, _p, _p, _p,
                                          _p, _p, _i64, _p]),
    "gpbo_refine_workspace_bytes": (_i64, [_i64, _i64]),
    "gpbo_refine_f64": (C.c_int, [_p, _i64, _p, _p, _p, _i64, _i64, _i32, _p, _p, _p, _f64, _i32, _f64, _f64, _i32, _f64, _p, _p,
                                  _p, _p, _p, _p, _i64, _p]),
    "gpbo_refine_host_f64": (C.c_int, [_p, _p, _i64, _i32, _p, _f64, _f64, _p, _i64, _p, _p, _i32, _f64, _f64, _i32, _f64, _p, _p,
                                       _p, _p, _p, _p]),
    "gpbo_thompson_weights_workspace_bytes": (_i64, [_i64, _i32, _i32]),
    "gpbo_thompson_weights_f64": (C.c_int, [_p, _p, _i64, _i64, _i32, _p, _p, _f64, _f64, _p, _p, _p, _p, _i32, _i32, _p, _p, _i64,
                                            _p]),
    "gpbo_thompson_paths_workspace_bytes": (_i64, [_i64, _i64, _i32, _i32]),
    "gpbo_thompson_paths_f64": (C.c_int, [_p, _i64, _p, _i64, _i64, _i32, _p, _p, _p, _p, _p, _i32, _i32, _i64, _p, _i64, _p, _p,
                                          _p, _p, _i64, _p]),
    "gpbo_thompson_host_f64": (C.c_int, [_p, _p, _i64, _i32, _p, _f64, _f64, _p, _i64, _p, _p, _p, _p, _i32, _i32, _p, _p, _p, _p,
                                         _p]),
    "gpbo_acq_workspace_bytes": (_i64, []),
    "gpbo_acq_argmax_f64": (C.c_int, [_p, _p, _i64, _i32, _f64, _f64, _i64, _p, _p, _p, _i64, _p]),
    "gpbo_nlml_grid_max_n": (C.c_int, []),
    "gpbo_nlml_grid_f64": (C.c_int, [_p, _p, _i64, _i32, _p, _i64, _f64, _p, _p]),
    "gpbo_nlml_grid_wave_max_n": (C.c_int, []),
    "gpbo_nlml_grid_wave_f64": (C.c_int, [_p, _p, _i64, _i32, _p, _i64, _f64, _p, _p]),
    "gpbo_nlml_grid_wave_logdet_f64": (C.c_int, [_p, _p, _i64, _i32, _p, _i64, _f64, _p, _p]),
    "gpbo_nlml_grid_batched_workspace_bytes": (_i64, [_i64, _i64]),
    "gpbo_nlml_grid_batched_f64": (C.c_int, [_p, _p, _i64, _i32, _p, _i64, _f64, _p, _p, _i64, _p]),
    "gpbo_nlml_grid_batched_logdet_f64": (C.c_int, [_p, _p, _i64, _i32, _p, _i64, _f64, _p, _p, _i64, _p]),
    "gpbo_nlml_cell_f64": (C.c_int, [_p, _p, _p, _i64, _i64, _p, _p, _p]),
    "gpbo_nlml_grad_workspace_bytes": (_i64, [_i64, _i32]),
    "gpbo_nlml_grad_f64": (C.c_int, [_p, _p, _p, _p, _i64, _i64, _i32, _p, _p, _p, _p, _i64, _p]),
    "gpbo_nlml_grad_host_f64": (C.c_int, [_p, _p, _i64, _i32, _p, _f64, _p]),
    "gpbo_nlml_hyper_workspace_bytes": (_i64, [_i64, _i32]),
    "gpbo_nlml_hyper_f64": (C.c_int, [_p, _p, _p, _p, _i64, _i64, _i32, _p, _f64, _i32, _p, _p, _p, _p, _i64, _p]),
    "gpbo_nlml_hyper_host_f64": (C.c_int, [_p, _p, _i64, _i32, _p, _f64, _i32, _p]),
    "gpbo_loo_workspace_bytes": (_i64, [_i64]),
    "gpbo_loo_f64": (C.c_int, [_p, _p, _p, _i64, _i64, _f64, _p, _p, _p, _p, _i64, _p]),
    # the Matern families: each is its twin above with `int32_t kernel` after ls_host
    "gpbo_kxx_kern_f64": (C.c_int, [_p, _i64, _i32, _p, _i32, _f64, _f64, _p, _i64, _p]),
    "gpbo_kstar_mu_kern_f64": (C.c_int, [_p, _i64, _p, _i64, _i64, _i32, _p, _i32, _p, _f64, _i64, _p, _i64, _p, _p]),
    "gpbo_factorise_kern_f64": (C.c_int, [_p, _p, _i64, _i32, _p, _i32, _f64, _f64, _i64, _p, _p, _p, _p, _p, _i64, _p]),
    "gpbo_posterior_acq_kern_f64": (C.c_int, [_p, _i64, _p, _i64, _i64, _i32, _p, _i32, _p, _p, _f64, _i32, _f64, _f64, _f64,
                                              _i64, _i64, _p, _p, _p, _p, _p, _i64, _p, _p]),
    "gpbo_nlml_grad_kern_f64": (C.c_int, [_p, _p, _p, _p, _i64, _i64, _i32, _p, _i32, _p, _p, _p, _i64, _p]),
    "gpbo_nlml_hyper_kern_f64": (C.c_int, [_p, _p, _p, _p, _i64, _i64, _i32, _p, _i32, _f64, _i32, _p, _p, _p, _p, _i64, _p]),
    "gpbo_select_next_host_kern_f64": (C.c_int, [_p, _p, _i64, _i32, _p, _i32, _f64, _f64, _p, _i64, _i32, _f64, _f64, _f64,
                                                 _i64, _p, _p, _p, _p, _p, _p]),
    "gpbo_nlml_grad_host_kern_f64": (C.c_int, [_p, _p, _i64, _i32, _p, _i32, _f64, _p]),
    "gpbo_nlml_hyper_host_kern_f64": (C.c_int, [_p, _p, _i64, _i32, _p, _i32, _f64, _i32, _p]),
    "gpbo_nlml_hyper_cells_f64": (C.c_int, [_p, _p, _i64, _i32, _p, _i64, _i32, _i32, _p, _p]),
    "gpbo_ensemble_workspace_bytes": (_i64, [_i64, _i64, _i64]),
    "gpbo_ensemble_acq_f64": (C.c_int, [_p, _i64, _p, _i64, _i64, _i32, _i32, _p, _i32, _p, _p, _p, _i32, _f64, _f64, _i64, _i64,
                                        _p, _p, _p, _p, _p, _i64, _p]),
    "gpbo_nei_fantasies_workspace_bytes": (_i64, [_i64, _i32]),
    "gpbo_nei_fantasies_f64": (C.c_int, [_p, _p, _p, _p, _i64, _i64, _p, _p, _f64, _i32, _p, _p, _p, _p, _i64, _p]),
    "gpbo_posterior_nei_workspace_bytes": (_i64, [_i64, _i64, _i64, _i32]),
    "gpbo_posterior_nei_kern_f64": (C.c_int, [_p, _i64, _p, _i64, _i64, _i32, _p, _i32, _p, _p, _p, _i32, _f64, _f64, _i64, _i64,
                                              _p, _i64, _p, _p, _p, _p, _i64, _p]),
    "gpbo_nei_host_f64": (C.c_int, [_p, _p, _i64, _i32, _p, _i32, _f64, _f64, _f64, _p, _i64, _p, _p, _i32, _f64, _i64, _p, _p,
                                    _p, _p, _p, _p, _p]),
    "gpbo_mes_log_survival_f64": (C.c_int, [_p, _p, _i64, _p, _i32, _p, _p, _p, _i64, _p]),
    "gpbo_mes_acq_f64": (C.c_int, [_p, _p, _i64, _p, _i32, _i64, _p, _p, _p, _i64, _p]),
    "gpbo_mes_log_survival_host_f64": (C.c_int, [_p, _p, _i64, _p, _i32, _p, _p]),
    "gpbo_mes_acq_host_f64": (C.c_int, [_p, _p, _i64, _p, _i32, _p, _p]),
    "gpbo_constrained_acq_f64": (C.c_int, [_p, _p, _i64, _i32, _f64, _f64, _p, _p, _i64, _i32, _p, _i64, _p, _p, _p, _p, _i64, _p]),
    "gpbo_constrained_acq_host_f64": (C.c_int, [_p, _p, _i64, _i32, _f64, _f64, _p, _p, _i64, _i32, _p, _p, _p, _p]),
    "gpbo_ehvi_acq_f64": (C.c_int, [_p, _p, _p, _p, _i64, _p, _i32, _f64, _f64, _i64, _p, _p, _p, _i64, _p]),
    "gpbo_ehvi_acq_host_f64": (C.c_int, [_p, _p, _p, _p, _i64, _p, _i32, _f64, _f64, _p, _p]),
    "gpbo_gemm_f64": (C.c_int, [_i32, _i64, _i64, _i64, _f64, _p, _i64, _i64, _p, _i64, _i64, _f64, _p, _i64, _i64,
                                _i32, _i32, _p]),
    "gpbo_gemm_tri_f64": (C.c_int, [_i32, _i64, _i64, _i64, _f64, _p, _i64, _i64, _p, _i64, _i64, _f64, _p, _i64, _i64,
                                    _i32, _i32, _i32, _i32, _p]),
}

_lib = None
hip_used_before_pytorch = False  # a host-pointer entry point initialised HIP while PyTorch was not imported


class ScreenStats(C.Structure):
    """gpbo_screen_stats (include/gpbo.h)."""
    _fields_ = [("survivors", _i64), ("rescored", _i64), ("rounds", _i32), ("fallback", _i32), ("tau", _f64),
                ("err_max", _f64)]


class GpboError(RuntimeError):
    pass


def _bind_to_pytorch_hip_runtime():
    """Two HIP runtimes in one process do not share the device: whichever initialises second sees no GPU.
    PyTorch-ROCm ships its own libamdhip64 (same SONAME as /opt/rocm's, which libgpbo.so would otherwise pull in).
    If PyTorch is installed but not imported yet (the NumPy-only host binding), load ITS runtime first, so that a
    later `import torch` in the same process finds the runtime it expects already in place.  Nothing is imported."""
    import importlib.util
    import sys

    if "torch" in sys.modules:
        return  # its runtime is loaded; libgpbo.so's NEEDED libamdhip64.so.7 resolves to it
    try:
        spec = importlib.util.find_spec("torch")
    except (ImportError, ValueError):
        spec = None
    if spec is None or not spec.origin:
        return
    libdir = os.path.join(os.path.dirname(spec.origin), "lib")
    # The whole ROCm stack PyTorch bundles, in dependency order, so that a later `import torch` finds every one of its
    # runtime libraries already in place and from ITS directory (tools/maps_probe.py shows what is mapped in each
    # load order; with only libamdhip64 preloaded the system ROCm's libhsa-amd-aqlprofile64 ended up inside PyTorch's
    # HSA runtime in the library-first order and in no other).
    for name in ("librocm-core.so", "libdrm.so", "libdrm_amdgpu.so", "libnuma.so", "libelf.so", "librocprofiler-register.so",
                 "libhsa-runtime64.so", "libamd_comgr.so", "libamdhip64.so", "libhiprtc.so", "libroctx64.so",
                 "libroctracer64.so"):
        rt = os.path.join(libdir, name)
        if os.path.exists(rt):
            try:
                C.CDLL(rt, mode=C.RTLD_GLOBAL)
            except OSError:
                pass  # fall back to whatever the dynamic linker resolves


def mapped_hip_runtimes():
    """Paths of every libamdhip64 mapped into this process (Linux: /proc/self/maps)."""
    try:
        with open("/proc/self/maps") as f:
            return sorted({line.split()[-1] for line in f if "libamdhip64" in line and line.split()[-1].startswith("/")})
    except OSError:
        return []


def note_hip_use():
    """Called by the NumPy-only binding right before a call that initialises HIP (see gp_device._torch)."""
    global hip_used_before_pytorch
    import sys

    if "torch" not in sys.modules:
        hip_used_before_pytorch = True


def load():
    """Load libgpbo.so and attach prototypes.  Raises if the library or any symbol is missing."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise GpboError(
            f"{LIB_PATH} not found: build it with bayesian_optimisation_amd/csrc/build.sh "
            "(there is no CPU fallback for the acquisition path)")
    _bind_to_pytorch_hip_runtime()
    lib = C.CDLL(LIB_PATH)
    rts = mapped_hip_runtimes()
    if len({os.path.realpath(p) for p in rts}) > 1:
        # two HIP runtimes in one process do not share the device: whichever initialises second sees no GPU (seen in
        # round 1 as torch.cuda.is_available() == False after a host-pointer call).  Fail here, loudly, not later.
        raise GpboError("two different HIP runtimes are mapped into this process: " + ", ".join(rts) + ". Load PyTorch (or "
                        "this package) before any other library that links libamdhip64, so that all of them share one.")
    for name, (res, args) in SIGNATURES.items():
        fn = getattr(lib, name)  # AttributeError if the symbol is missing
        fn.restype = res
        fn.argtypes = args
    _lib = lib
    return lib


def check(status: int, what: str):
    if status != GPBO_OK:
        msg = load().gpbo_strerror(status).decode()
        raise GpboError(f"{what}: {msg} (status {status})")


def call(fn, *args):
    """fn(*args) for a library function that returns a status; GpboError naming the function when it is not GPBO_OK."""
    status = fn(*args)
    if status != GPBO_OK:
        check(status, fn.__name__)

