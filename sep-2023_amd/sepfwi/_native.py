"""Loader / builder of libsepfwi.so, the HIP propagator behind the C ABI of include/sepfwi.h.

There is no CPU fallback: if the library cannot be loaded every operator call raises.
"""
from __future__ import annotations

import contextlib
import ctypes as C
import os
import subprocess

_PKG = os.path.dirname(os.path.abspath(__file__))
_ROOT = os.path.dirname(_PKG)                      # sep-2023_amd/
CSRC = os.path.join(_ROOT, "csrc")
LIB_PATH = os.path.join(_ROOT, "libsepfwi.so")
# The same sources built with -DSEPFWI_PROBES: sepfwi_set_option then also knows the tuning knobs (tile shapes, wave counts, launch
# structures) and the timing-only switches that the shipped library does not expose (include/sepfwi.h).  Used by scripts/ab_bench.py
# and by the tests that prove every selectable kernel structure bit-identical; never by the operators unless asked to (use_variant).
PROBES_LIB_PATH = os.path.join(_ROOT, "libsepfwi_probes.so")
# ... and with -DSEPFWI_PK_FAULT=<tile>: a fault-injection build whose persistent loop stalls on purpose (one tile stops publishing), for
# the one test that must see the loop's time-out path work (tests/test_gpu_parity.py::test_loop_failure_path_reports_and_recovers).
FAULT_LIB_PATH = os.path.join(_ROOT, "libsepfwi_fault.so")
VARIANTS = {"default": (LIB_PATH, []), "probes": (PROBES_LIB_PATH, ["-DSEPFWI_PROBES"]), "fault": (FAULT_LIB_PATH, ["-DSEPFWI_PK_FAULT=17"])}
PUBLIC_OPTIONS = ("bwd_fuse", "batch", "img_every", "quiet_skip", "obs_cache_mb", "probe")
SOURCES = ["kernels.hip", "schedule.cpp", "model_call.cpp", "param_maps.hip", "regularizer.hip", "smoother.hip", "conditioning.hip", "w2_misfit.hip", "robust_misfit.hip", "session.cpp", "session_run.cpp", "session_data.cpp", "session_persist.cpp", "session_batched.cpp", "obs_store.cpp", "host_checks.cpp", "persist_plan.cpp", "inject_plan.cpp", "das_gauge.hip", "das_gauge.cpp", "geophone.hip", "geophone.cpp", "pseudo_hessian.hip", "born.hip", "session_born.cpp", "exact_adjoint.hip", "session_exact.cpp", "config.cpp", "capi.cpp"]
HEADER = os.path.join(os.path.dirname(_ROOT), "include", "sepfwi.h")

_libs = {}
_active = os.environ.get("SEPFWI_LIB_VARIANT", "default")


class Stats(C.Structure):
    """mirror of struct sepfwi_stats (include/sepfwi.h)"""
    _fields_ = [("fwd_ms", C.c_double), ("bwd_ms", C.c_double), ("total_ms", C.c_double),
                ("cell_updates", C.c_double), ("fwd_steps", C.c_longlong), ("bwd_steps", C.c_longlong),
                ("launches", C.c_longlong), ("device_bytes", C.c_longlong), ("n_c", C.c_int),
                ("probe_kernel_us", C.c_double), ("probe_calls", C.c_longlong),
                ("obs_device_bytes", C.c_longlong), ("obs_host_bytes", C.c_longlong), ("obs_evictions", C.c_longlong), ("persist_steps", C.c_longlong), ("quiet_active", C.c_longlong), ("quiet_total", C.c_longlong)]


_I, _F, _P, _S = C.c_int, C.c_float, C.c_void_p, C.c_char_p
_SESSION = [_S, _I]                        # para_fname, gpu_id
_SHOTS = [_I, _I, _P, _S, _P]              # gpu_id, group_size, shot_ids, para_fname, hip_stream
_CUFD = [_P] * 9 + [_I, _I, _I, _P, _S]    # 5 outputs, 4 inputs, calc_id, gpu_id, group_size, shot_ids, para_fname
_PARAM = [_I] * 5 + [_P] * 13 + [_P]       # kind and sizes, 7 fields, 3 inputs, 3 outputs, hip_stream
_REG = [_I, _I, _F, _F] + [_P] * 7 + [_F, _P, _P, _P]
# Every function of include/sepfwi.h: name -> (restype, argtypes).  lib() declares them from here and tests/test_host_logic.py holds
# the table against the header's declarations, so a new entry point is one entry here (a line holds the functions that belong together).
API = {
    "sepfwi_last_error": (_S, []),
    "sepfwi_version": (_I, []), "sepfwi_device_count": (_I, []),
    "sepfwi_cufd": (_I, _CUFD), "sepfwi_cufd_stream": (_I, _CUFD + [_P, _I]),
    "sepfwi_release_all": (None, []), "sepfwi_invalidate_observed": (None, []),
    "sepfwi_cpml_profiles": (_I, [_P] * 6 + [_I, _I, _F, _F, _F]),
    "sepfwi_stf_taper": (_I, [_P, _I, _F, _F]), "sepfwi_shot_split": (_I, [_I, _I, _P]),
    "sepfwi_get_stats": (_I, _SESSION + [C.POINTER(Stats)]), "sepfwi_loop_status": (_I, _SESSION + [_S, _I]),
    "sepfwi_set_option": (_I, [_S, _I]), "sepfwi_get_option": (_I, [_S]),
    "sepfwi_debug_field": (_I, _SESSION + [_I, _I, _P]), "sepfwi_debug_live_bytes": (_I, [C.POINTER(C.c_longlong)] * 2),
    "sepfwi_set_observed": (_I, _SESSION + [_I, _P, _I, _I]), "sepfwi_set_observed_component": (_I, _SESSION + [_I, _I, _P, _I, _I]),
    "sepfwi_get_misfit_parts": (_I, _SESSION + [C.POINTER(C.c_double)]),
    "sepfwi_pseudo_hessian_arm": (_I, _SESSION + [_I]), "sepfwi_get_pseudo_hessian": (_I, _SESSION + [_P] * 3),
    "sepfwi_born": (_I, [_P] * 13 + _SHOTS), "sepfwi_born_src": (_I, [_P] * 13 + _SHOTS + [_P]),
    "sepfwi_adjoint_exact": (_I, [_P] * 14 + _SHOTS), "sepfwi_adjoint_exact_src": (_I, [_P] * 14 + _SHOTS + [_P, _P]),
    "sepfwi_condition": (_I, [_P, _I] + _SHOTS),
    "sepfwi_data_misfit": (_I, [_P] * 4 + _SHOTS),
    "sepfwi_data_gn": (_I, [_P] * 3 + _SHOTS), "sepfwi_data_gn_obs": (_I, [_P] * 4 + _SHOTS),
    "sepfwi_param_forward": (_I, [_I] * 5 + [_P] * 10 + [_P]),
    "sepfwi_param_backward": (_I, _PARAM), "sepfwi_param_jvp": (_I, _PARAM), "sepfwi_param_diag": (_I, _PARAM),
    "sepfwi_regularizer": (_I, _REG), "sepfwi_regularizer_hvp": (_I, _REG),
    "sepfwi_smooth_plan": (_I, [_I] * 4 + [_P] * 4 + [_P]), "sepfwi_smooth_apply": (_I, [_I] * 4 + [_P] * 4 + [_I, _P, _P, _P]),
}
EXPORTS = list(API)


def needs_build(variant: str = "default") -> bool:
    path = VARIANTS[variant][0]
    if not os.path.exists(path):
        return True
    t = os.path.getmtime(path)
    # every file of csrc/ is a translation unit of the library or one of its headers: the directory is the list
    return any(os.path.getmtime(f) > t for f in [os.path.join(CSRC, n) for n in os.listdir(CSRC)] + [HEADER])


def build(force: bool = False, verbose: bool = False, variant: str = "all") -> str:
    """hipcc --offload-arch=gfx950 ... (cross-compiles without a GPU; ~30 s per variant)."""
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    for name in (VARIANTS if variant == "all" else (variant,)):
        path, flags = VARIANTS[name]
        if not (force or needs_build(name)):
            continue
        # -ffp-contract=off: no fused multiply-adds chosen per kernel by the compiler, so every kernel structure (stream, batched,
        # unfused, persistent) gives bit-identical results; the kernels are memory-bound, it costs nothing
        extra = os.environ.get("SEPFWI_HIPCC_FLAGS", "").split()   # experiments only (e.g. -fgpu-flush-denormals-to-zero)
        cmd = [hipcc, "--offload-arch=gfx950", "-O3", "-std=c++17", "-ffp-contract=off", "-fPIC", "-shared", "-Wall"] + flags + extra + ["-o", path] + SOURCES + ["-ldl"]   # hipFFT is opened lazily (csrc/conditioning.hip)
        if verbose:
            print(" ".join(cmd))
        subprocess.check_call(cmd, cwd=CSRC)
    return LIB_PATH


@contextlib.contextmanager
def use_variant(name: str):
    """Route every operator call of the block to another build of the library (its own sessions and option block)."""
    global _active
    prev, _active = _active, name
    try:
        yield lib()
    finally:
        _active = prev


def lib():
    """The loaded library (ctypes.CDLL) with argument types declared."""
    if _active in _libs:
        return _libs[_active]
    path = VARIANTS[_active][0]
    # torch first: both link libamdhip64.so.7 and must share ONE HIP runtime in the process.
    import torch  # noqa: F401
    if not os.path.exists(path):
        raise RuntimeError(
            "%s is not built (%s missing). Run `python -c 'import __graft_entry__ as g; g.build()'`; "
            "there is no CPU fallback for the propagator." % (os.path.basename(path), path))
    L = C.CDLL(path)
    for name, (restype, argtypes) in API.items():
        f = getattr(L, name)
        f.restype, f.argtypes = restype, argtypes
    _libs[_active] = L
    return L


def ptr(t):
    """a tensor's data pointer as a C argument; None stays None (NULL)"""
    return None if t is None else C.c_void_p(t.data_ptr())


def path_arg(fname):
    """a parameter-file path as a C argument"""
    return str(fname).encode()


def ids_arg(ids):
    """a contiguous int32 numpy array of shot ids as a C argument (the array must outlive the call)"""
    return C.c_void_p(ids.ctypes.data)


def triple(ts):
    """up to three tensors as a C array of three pointers, padded with NULL"""
    ts = list(ts)
    return (C.c_void_p * 3)(*([t.data_ptr() for t in ts] + [None] * (3 - len(ts))))


def stream_arg(device):
    """torch's current stream on `device` as a C argument; None for the null stream"""
    import torch
    cs = torch.cuda.current_stream(device).cuda_stream
    return C.c_void_p(cs) if cs else None


class SepFwiError(RuntimeError):
    def __init__(self, code, msg):
        super().__init__("sepfwi error %d: %s" % (code, msg))
        self.code = code


def check(rc: int):
    if rc != 0:
        raise SepFwiError(rc, lib().sepfwi_last_error().decode(errors="replace"))
