"""ctypes binding of libsnowtri.so (the C ABI declared in include/snowtri.h).

This is the binding a SnowMocap maintainer would add: no torch types, plain
pointers and sizes.  There is NO CPU fallback: if the shared library is missing or no MI355X is
visible, calls raise -- the product path never routes through oracle/ or NumPy.
"""
from __future__ import annotations

import ctypes as ct
import os

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("SNOWTRI_LIB") or os.path.join(_HERE, "libsnowtri.so")   # override: A/B builds

OK, ERR_BAD_ARG, ERR_BAD_INDEX, ERR_HIP, ERR_SINGULAR, ERR_OVERFLOW, ERR_NO_DEVICE = range(7)
F32, F64 = 0, 1
HOST, DEVICE = 0, 1
PAIRWISE, DLT, DLT_ROBUST = 0, 1, 2
FLAG_SINGULAR, FLAG_OVERFLOW, FLAG_FASTPATH = 1, 2, 4
DESPIKE_MARK, DESPIKE_REPLACE = 0, 1                       # snowtri_despike_joint_track: mode
DESPIKE_KEPT, DESPIKE_SPIKE, DESPIKE_MISSING, DESPIKE_UNSUPPORTED = 0, 1, 2, 3   # ... and its codes
REPROJECT_RAW = 1              # snowtri_reproject / snowtri_reproject_cost: flags -- pixels on the raw (distorted) frame
REFINE_SCORE_WEIGHTS = 1       # snowtri_refine_joints: flags -- a view weighs its observation's score
REFINE_MISSING, REFINE_FEW_VIEWS, REFINE_KEPT, REFINE_MOVED = 0, 1, 2, 3   # ... and its codes
POSE_FIXED, POSE_FEW_OBS, POSE_KEPT, POSE_MOVED = 0, 1, 2, 3   # snowtri_refine_cameras: codes
INTR_FOCAL, INTR_CENTRE = 1, 2   # snowtri_refine_cameras_k: intr_flags
POSE_SWEEP_RECORDS = 1024 * 256   # ... and the records one sweep of k_pose_normal's grid covers (snowtri_pose_sweep_records)
SEED_FLAG_FULL = 1             # snowtri_seed_persons: flags -- the frame stopped at S seeds with a finite edge between free nodes left
CALL_NO_ZERO_FILL = 1         # snowtri_triangulate_condense_ex: the slots behind out_count[f] are left unwritten
TEST_LIB_PATH = os.path.join(_HERE, "libsnowtri_dbg.so")   # -DSNOWTRI_DEBUG_BOUNDS -DSNOWTRI_TEST_KNOBS (tests only: use_library)


class SnowtriError(RuntimeError):
    def __init__(self, status, where):
        self.status = status
        msg = _lib.snowtri_status_string(status).decode() if _lib is not None else str(status)
        detail = _lib.snowtri_last_error().decode() if (_lib is not None and status == ERR_HIP) else ""
        super().__init__(f"{where}: {msg}" + (f" [{detail}]" if detail else ""))


class Params(ct.Structure):
    """snowtri_params: thresholds of Human_Triangulation / _Condense (triangulation.py:50,95-100)."""
    _fields_ = [("keypoint_score_threshold", ct.c_double),
                ("average_score_threshold", ct.c_double),
                ("distance_threshold", ct.c_double),
                ("condense_distance_tol", ct.c_double),
                ("condense_person_num_tol", ct.c_double),
                ("condense_score_tol", ct.c_double),
                ("center_point_index", ct.c_int32),
                ("keypoint_num", ct.c_int32)]


def make_params(keypoint_score_threshold=0.5, average_score_threshold=0.0, distance_threshold=0.05,
                condense_distance_tol=0.1, condense_person_num_tol=0, condense_score_tol=0.0,
                center_point_index=18, keypoint_num=30, **_ignored):
    """Defaults are the reference's function-signature defaults (triangulation.py:50,95-100)."""
    return Params(float(keypoint_score_threshold), float(average_score_threshold),
                  float(distance_threshold), float(condense_distance_tol),
                  float(condense_person_num_tol), float(condense_score_tol),
                  int(center_point_index), int(keypoint_num))


_c_p = ct.c_void_p
_SIGNATURES = {
    # name: (restype, argtypes)  -- one entry per symbol declared in include/snowtri.h
    "snowtri_version": (ct.c_int, []),
    "snowtri_status_string": (ct.c_char_p, [ct.c_int]),
    "snowtri_last_error": (ct.c_char_p, []),
    "snowtri_device_count": (ct.c_int, []),
    "snowtri_build_info": (ct.c_char_p, []),
    "snowtri_ctx_overrides": (ct.c_char_p, [_c_p]),
    "snowtri_ctx_set_overlap": (ct.c_int, [_c_p, ct.c_int]),
    "snowtri_ctx_join": (ct.c_int, [_c_p, _c_p]),
    "snowtri_ctx_set_split": (ct.c_int, [_c_p, ct.c_int]),
    "snowtri_ctx_set_robust": (ct.c_int, [_c_p, ct.c_double, ct.c_int32]),
    "snowtri_triangulate_robust": (ct.c_int, [_c_p, ct.c_int64, ct.c_int32, _c_p, ct.c_int, _c_p, ct.POINTER(Params), ct.c_double,
                                              ct.c_int32, ct.c_int32, _c_p, _c_p, ct.c_int, _c_p, _c_p, _c_p, _c_p, ct.c_int, _c_p]),
    "snowtri_last_stream_counts": (ct.c_int, [_c_p, ct.POINTER(ct.c_int64 * 3)]),
    "snowtri_ctx_stream_probes": (ct.c_int, [_c_p, ct.POINTER(ct.c_int64 * 3)]),
    "snowtri_ctx_create": (ct.c_int, [ct.c_int32, _c_p, _c_p, _c_p, ct.c_int, ct.POINTER(_c_p)]),
    "snowtri_ctx_destroy": (ct.c_int, [_c_p]),
    "snowtri_ctx_num_cameras": (ct.c_int, [_c_p]),
    "snowtri_ctx_ray_matrices": (ct.c_int, [_c_p, _c_p]),
    "snowtri_ctx_synchronize": (ct.c_int, [_c_p]),
    "snowtri_fastmath_probe": (ct.c_int, [_c_p, ct.c_int64, _c_p, _c_p, _c_p, _c_p]),
    "snowtri_fastmath_probe_raw": (ct.c_int, [_c_p, ct.c_int64, _c_p, _c_p, _c_p]),
    "snowtri_calib_stream": (ct.c_int, [_c_p, _c_p, ct.c_int64, _c_p, ct.c_int64, _c_p]),
    "snowtri_rays_from_pixels": (ct.c_int, [_c_p, ct.c_int32, ct.c_int64, _c_p, _c_p]),
    "snowtri_skew_ray_batch": (ct.c_int, [_c_p, ct.c_int64, _c_p, _c_p, _c_p, _c_p, _c_p, _c_p,
                                          ct.POINTER(ct.c_int64)]),
    "snowtri_triangulate": (ct.c_int, [_c_p, ct.c_int64, ct.c_int32, ct.c_int32, _c_p, ct.c_int, _c_p,
                                       ct.POINTER(Params), _c_p, _c_p, _c_p, _c_p, ct.c_int, _c_p]),
    "snowtri_num_candidate_slots": (ct.c_int64, [ct.c_int32, ct.c_int32]),
    "snowtri_condense": (ct.c_int, [_c_p, ct.c_int64, ct.c_int32, ct.c_int32, _c_p, _c_p, _c_p,
                                    ct.POINTER(Params), ct.c_int32, _c_p, _c_p, _c_p, _c_p, _c_p,
                                    ct.c_int, _c_p]),
    "snowtri_candidates_token": (ct.c_int64, [_c_p]),
    "snowtri_condense_resident": (ct.c_int, [_c_p, ct.c_int64, ct.POINTER(Params), ct.c_int32, _c_p, _c_p, _c_p, _c_p, _c_p]),
    "snowtri_triangulate_condense": (ct.c_int, [_c_p, ct.c_int64, ct.c_int32, ct.c_int32, _c_p, ct.c_int,
                                                _c_p, ct.POINTER(Params), ct.c_int, ct.c_int32, _c_p,
                                                _c_p, ct.c_int, _c_p, _c_p, ct.c_int, _c_p]),
    "snowtri_triangulate_condense_ex": (ct.c_int, [_c_p, ct.c_int64, ct.c_int32, ct.c_int32, _c_p, ct.c_int,
                                                   _c_p, ct.POINTER(Params), ct.c_int, ct.c_int32, _c_p,
                                                   _c_p, ct.c_int, _c_p, _c_p, ct.c_int, _c_p, ct.c_uint32]),
    "snowtri_smooth_track": (ct.c_int, [_c_p, ct.c_int64, ct.c_int64, _c_p, ct.c_double, ct.c_double, ct.c_double,
                                        ct.c_double, _c_p, ct.c_int, _c_p]),
    "snowtri_smooth_joint_track": (ct.c_int, [_c_p, ct.c_int64, ct.c_int64, _c_p, ct.c_double, ct.c_double, ct.c_double,
                                              ct.c_double, _c_p, ct.c_int, _c_p]),
    "snowtri_smooth_coeffs": (ct.c_int, [ct.c_double, ct.c_double, ct.c_double, ct.c_double, _c_p]),
    "snowtri_smooth_shard_local": (ct.c_int, [_c_p, ct.c_int64, ct.c_int64, _c_p, ct.c_int, ct.c_double, ct.c_double,
                                              ct.c_double, ct.c_double, _c_p, _c_p, ct.c_int, _c_p]),
    "snowtri_smooth_shard_fix": (ct.c_int, [_c_p, ct.c_int64, ct.c_int64, ct.c_int, _c_p, ct.c_double, ct.c_double,
                                            ct.c_double, ct.c_double, _c_p, ct.c_int, _c_p]),
    "snowtri_smooth_shard_reduce": (ct.c_int, [_c_p, ct.c_int64, ct.c_int64, _c_p, ct.c_int, ct.c_double, ct.c_double, ct.c_double, ct.c_double, _c_p, _c_p]),
    "snowtri_smooth_shard_scan": (ct.c_int, [_c_p, ct.c_int64, ct.c_int64, _c_p, ct.c_int, _c_p, ct.c_double, ct.c_double, ct.c_double, ct.c_double, _c_p, _c_p]),
    "snowtri_blender_smooth_shard_reduce": (ct.c_int, [_c_p, ct.c_int64, ct.c_int64, _c_p, ct.c_int, _c_p, ct.c_double, _c_p, _c_p]),
    "snowtri_blender_smooth_shard_scan": (ct.c_int, [_c_p, ct.c_int64, ct.c_int64, _c_p, ct.c_int, _c_p, _c_p, ct.c_double, _c_p, _c_p]),
    "snowtri_smooth_shard_combine": (ct.c_int, [_c_p, ct.c_int32, ct.c_int32, ct.c_int64, _c_p, ct.c_double, ct.c_double,
                                                ct.c_double, ct.c_double, _c_p, ct.c_int, _c_p]),
    "snowtri_blender_points": (ct.c_int, [_c_p, ct.c_int64, ct.c_int32, _c_p, ct.c_int, _c_p, _c_p, ct.c_int, _c_p]),
    "snowtri_blender_smooth": (ct.c_int, [_c_p, ct.c_int64, ct.c_int64, _c_p, _c_p, _c_p, ct.c_double, _c_p,
                                          ct.c_int, _c_p]),
    "snowtri_blender_hold_shard_last": (ct.c_int, [_c_p, ct.c_int64, ct.c_int64, _c_p, _c_p, _c_p, _c_p]),
    "snowtri_blender_hold_shard_apply": (ct.c_int, [_c_p, ct.c_int32, ct.c_int32, ct.c_int64, ct.c_int64, _c_p, _c_p, _c_p, _c_p, _c_p]),
    "snowtri_blender_smooth_shard_local": (ct.c_int, [_c_p, ct.c_int64, ct.c_int64, _c_p, ct.c_int, _c_p, ct.c_double, _c_p, _c_p, _c_p]),
    "snowtri_blender_smooth_shard_combine": (ct.c_int, [_c_p, ct.c_int32, ct.c_int32, ct.c_int64, _c_p, _c_p, ct.c_double, _c_p, _c_p]),
    "snowtri_blender_smooth_shard_fix": (ct.c_int, [_c_p, ct.c_int64, ct.c_int64, ct.c_int, _c_p, _c_p, ct.c_double, _c_p, _c_p]),
    "snowtri_track_state_bytes": (ct.c_size_t, [ct.c_int32]),
    "snowtri_track_block_frames": (ct.c_int, []),
    "snowtri_track_persons": (ct.c_int, [_c_p, ct.c_int64, ct.c_int32, ct.c_int32, _c_p, ct.c_int, _c_p, ct.c_int32, ct.c_int32,
                                         ct.c_double, ct.c_int32, _c_p, _c_p, _c_p, _c_p, _c_p, ct.c_int, _c_p]),
    "snowtri_track_last_ms": (ct.c_int, [_c_p, ct.POINTER(ct.c_float * 2)]),
    "snowtri_track_gather": (ct.c_int, [_c_p, ct.c_int64, ct.c_int32, ct.c_int32, _c_p, ct.c_int, ct.c_int32, _c_p, _c_p,
                                        ct.c_int, _c_p]),
    "snowtri_fill_joint_track": (ct.c_int, [_c_p, ct.c_int64, ct.c_int64, _c_p, ct.c_int, ct.c_int32, _c_p, _c_p, ct.c_int, _c_p]),
    "snowtri_fill_block_frames": (ct.c_int, []),
    "snowtri_despike_joint_track": (ct.c_int, [_c_p, ct.c_int64, ct.c_int64, _c_p, ct.c_int, ct.c_int32, ct.c_double, ct.c_int32, _c_p, _c_p,
                                               ct.c_int, _c_p]),
    "snowtri_despike_block_frames": (ct.c_int, []),
    "snowtri_ctx_set_distortion": (ct.c_int, [_c_p, _c_p]),
    "snowtri_undistort_keypoints": (ct.c_int, [_c_p, ct.c_int64, ct.c_int32, ct.c_int32, _c_p, _c_p, ct.c_int,
                                               ct.c_int, _c_p]),
    "snowtri_reproject": (ct.c_int, [_c_p, ct.c_int64, ct.c_int32, ct.c_int32, _c_p, ct.c_int, ct.c_uint32, _c_p, ct.c_int, ct.c_int, _c_p]),
    "snowtri_reproject_cost": (ct.c_int, [_c_p, ct.c_int64, ct.c_int32, ct.c_int32, _c_p, ct.c_int, ct.c_int32, _c_p, ct.c_int, _c_p,
                                          ct.c_double, ct.c_uint32, _c_p, _c_p, ct.c_int, _c_p]),
    "snowtri_assign_detections": (ct.c_int, [_c_p, ct.c_int64, ct.c_int32, ct.c_int32, _c_p, _c_p, ct.c_double, ct.c_int32, _c_p, _c_p, _c_p,
                                             ct.c_int, _c_p]),
    "snowtri_refine_joints": (ct.c_int, [_c_p, ct.c_int64, ct.c_int32, ct.c_int32, _c_p, ct.c_int, ct.c_int32, _c_p, ct.c_int, _c_p, _c_p, _c_p,
                                         ct.c_double, ct.c_int32, ct.c_uint32, _c_p, _c_p, _c_p, ct.c_int, _c_p]),
    "snowtri_refine_joints_ex": (ct.c_int, [_c_p, ct.c_int64, ct.c_int32, ct.c_int32, _c_p, ct.c_int, ct.c_int32, _c_p, ct.c_int, _c_p, _c_p, _c_p,
                                            ct.c_double, ct.c_int32, ct.c_uint32, ct.c_double, _c_p, _c_p, _c_p, _c_p, ct.c_int, _c_p]),
    "snowtri_triangulate_matched": (ct.c_int, [_c_p, ct.c_int64, ct.c_int32, ct.c_int32, ct.c_int32, _c_p, ct.c_int, _c_p, _c_p, ct.c_double,
                                               ct.c_double, ct.c_int32, _c_p, _c_p, ct.c_int, _c_p, _c_p, ct.c_int, _c_p]),
    "snowtri_pair_cost": (ct.c_int, [_c_p, ct.c_int64, ct.c_int32, ct.c_int32, _c_p, ct.c_int, _c_p, _c_p, ct.c_double, _c_p, _c_p, ct.c_int, _c_p]),
    "snowtri_seed_persons": (ct.c_int, [_c_p, ct.c_int64, ct.c_int32, _c_p, _c_p, _c_p, _c_p, ct.c_double, ct.c_int32, ct.c_int32, ct.c_int32,
                                        _c_p, _c_p, _c_p, ct.c_int, _c_p]),
    "snowtri_pose_sweep_records": (ct.c_int, []),
    "snowtri_refine_cameras": (ct.c_int, [_c_p, ct.c_int64, ct.c_int32, ct.c_int32, _c_p, ct.c_int, ct.c_int32, _c_p, ct.c_int, _c_p, _c_p, _c_p,
                                          ct.c_double, ct.c_uint32, ct.c_int32, ct.c_int32, ct.c_uint32, _c_p, _c_p, _c_p, _c_p, _c_p, _c_p,
                                          ct.c_int, _c_p]),
    "snowtri_refine_cameras_ex": (ct.c_int, [_c_p, ct.c_int64, ct.c_int32, ct.c_int32, _c_p, ct.c_int, ct.c_int32, _c_p, ct.c_int, _c_p, _c_p, _c_p,
                                             ct.c_double, ct.c_uint32, ct.c_int32, ct.c_int32, ct.c_uint32, ct.c_double, _c_p, _c_p, _c_p, _c_p,
                                             _c_p, _c_p, _c_p, ct.c_int, _c_p]),
    "snowtri_refine_cameras_k": (ct.c_int, [_c_p, ct.c_int64, ct.c_int32, ct.c_int32, _c_p, ct.c_int, ct.c_int32, _c_p, ct.c_int, _c_p, _c_p, _c_p,
                                            ct.c_double, ct.c_uint32, ct.c_uint32, ct.c_uint32, ct.c_int32, ct.c_int32, ct.c_uint32, ct.c_double,
                                            _c_p, _c_p, _c_p, _c_p, _c_p, _c_p, _c_p, _c_p, ct.c_int, _c_p]),
    "snowtri_last_kernel_ms": (ct.c_int, [_c_p, ct.POINTER(ct.c_float * 2)]),
    "snowtri_set_timing": (ct.c_int, [_c_p, ct.c_int]),
    "snowtri_timing_collect": (ct.c_int, [_c_p, _c_p, ct.c_int32]),
    "snowtri_last_slow_frames": (ct.c_int64, [_c_p]),
    "snowtri_last_handover_persons": (ct.c_int64, [_c_p, _c_p]),
    "snowtri_last_kernel_names": (ct.c_char_p, [_c_p]),
    "snowtri_debug_faults": (ct.c_int64, [_c_p, ct.POINTER(ct.c_uint64)]),
    "snowtri_debug_selftest": (ct.c_int, [_c_p]),
}

_lib = None
_loaded = {}      # path -> bound CDLL handle (a process may hold the production library and the test build side by side)


def exported_symbols():
    return sorted(_SIGNATURES)


def _load(path):
    handle = _loaded.get(path)
    if handle is None:
        if not os.path.exists(path):
            raise ImportError(
                f"{path} is missing: build it with `python -c 'import __graft_entry__ as g; g.build()'` "
                "(hipcc --offload-arch=gfx950).  snowmocap_amd has no CPU fallback.")
        # One HIP runtime per process: PyTorch-ROCm bundles its own libamdhip64 (same SONAME as
        # /opt/rocm's).  Loading it FIRST makes the dynamic linker bind libsnowtri.so to that copy,
        # so torch streams / device pointers and our kernels share one runtime.  Loading ours first
        # would leave torch with a second runtime that sees no GPU.
        if os.environ.get("SNOWTRI_NO_TORCH", "0") != "1":
            try:
                import torch  # noqa: F401
            except Exception:
                pass
        handle = ct.CDLL(path)              # (RTLD_LOCAL: two builds of the library do not see each other's symbols)
        for name, (res, args) in _SIGNATURES.items():
            fn = getattr(handle, name)      # AttributeError if the ABI lost a symbol
            fn.restype = res
            fn.argtypes = args
        _loaded[path] = handle
    return handle


def lib():
    """Load libsnowtri.so (built by __graft_entry__.build() / `make -C snowmocap_amd/csrc`)."""
    global _lib
    if _lib is None:
        _lib = _load(LIB_PATH)
    return _lib


def use_library(path=None):
    """Bind the package to another build of the library -- the TEST build libsnowtri_dbg.so (device-side bounds checks + the
    route-forcing knobs, which the production library does not contain) -- or back to the production one (path=None).
    Returns the path that was bound before.  Contexts keep the library they were created with (Context.L), so objects made
    under one binding stay valid under the next; everything created afterwards uses the new one.  Tests only
    (tests/conftest.py::knob_lib)."""
    global _lib, LIB_PATH
    prev = LIB_PATH
    LIB_PATH = path or os.environ.get("SNOWTRI_LIB") or os.path.join(_HERE, "libsnowtri.so")
    _lib = _load(LIB_PATH)
    return prev


def build_info():
    """{"version": int, "arch": str, "variants": [build variants of the loaded binary]} (snowtri_build_info)."""
    raw = lib().snowtri_build_info().decode()
    d = dict(kv.split("=", 1) for kv in raw.split(";"))
    return {"version": int(d["version"]), "arch": d["arch"], "variants": [v for v in d.get("variants", "").split(",") if v]}


def check(status, where):
    if status != OK:
        raise SnowtriError(status, where)


def ptr(a):
    """void* for a C call: the data pointer of a NumPy array or of anything with data_ptr() (a torch tensor); an int is an address or
    a HIP stream handle (0: NULL); None and a c_void_p pass through."""
    if a is None or isinstance(a, ct.c_void_p):
        return a
    if isinstance(a, int):
        return ct.c_void_p(a) if a else None
    return ct.c_void_p(a.ctypes.data if isinstance(a, np.ndarray) else a.data_ptr())


def dtype_code(dt):
    dt = np.dtype(dt)
    if dt == np.float32:
        return F32
    if dt == np.float64:
        return F64
    raise TypeError(f"snowtri supports float32/float64 I/O, not {dt}")


def _float_code(dtype):
    """F32 / F64 of a NumPy or torch dtype (or its name)."""
    try:
        return dtype_code(dtype)
    except TypeError:
        return dtype_code(str(dtype).replace("torch.", ""))


def host_floats(a):
    """Anything array-like -> a contiguous NumPy array: float32 stays, every other dtype becomes float64 (no copy if it already is so)."""
    a = np.asarray(a)
    if a.dtype != np.float32:
        a = a.astype(np.float64, copy=False)
    return np.ascontiguousarray(a)


def free_mask(free, C):
    """Which cameras may move, as snowtri_refine_cameras' bit mask: None (all C), an int mask, a sequence of C booleans, or a
    sequence of camera indices."""
    if free is None:
        return (1 << C) - 1
    if isinstance(free, (int, np.integer)) and not isinstance(free, (bool, np.bool_)):
        mask = int(free)
    else:
        a = np.asarray(free)
        if a.dtype == bool:
            if a.shape != (C,):
                raise ValueError(f"free as booleans must have one entry per camera ({C})")
            idx = np.nonzero(a)[0]
        else:
            idx = a.astype(np.int64).reshape(-1)
            if len(idx) and (idx.min() < 0 or idx.max() >= C or (a != idx.reshape(a.shape)).any()):
                raise ValueError(f"free names a camera outside 0..{C - 1}")
        mask = 0
        for c in idx:
            mask |= 1 << int(c)
    if mask < 0 or mask >> C:
        raise ValueError(f"free has a bit at or above the number of cameras ({C})")
    return mask


class Space:
    """Where the arrays of one wrapper call live: on the host (NumPy arrays, staged by the library, synchronous) or on one CUDA device
    (torch tensors, used in place and asynchronously on `stream`, default torch's current stream of that device).  Made from the call's
    array arguments (None: ignored), which are all tensors or all not; `who` names the wrapper in the messages.  `device` is None on
    the host, else the torch device of the first tensor; every tensor checked later has to live there."""

    def __init__(self, who, *arrays, stream=None):
        tensors = [hasattr(a, "is_cuda") for a in arrays if a is not None]
        if any(tensors) and not all(tensors):
            raise ValueError(f"{who} takes host arrays or CUDA tensors, not a mixture")
        self.who, self.device, self.stream = who, None, None
        if any(tensors):
            import torch
            self.torch = torch
            self.device = next(a for a in arrays if a is not None).device
            if stream is None and self.device.type == "cuda":      # (a CPU tensor is refused by the check of its array)
                stream = torch.cuda.current_stream(self.device).cuda_stream
            self.stream = stream

    def _resident(self, a):
        return a.is_cuda and a.is_contiguous() and a.device == self.device

    def floats(self, a, what):
        """A float array in -> (the array, its F32 / F64 code): host_floats(a) on the host, a checked float32 / float64 tensor on the device."""
        if self.device is None:
            a = host_floats(a)
            return a, dtype_code(a.dtype)
        if a.dtype not in (self.torch.float32, self.torch.float64):
            raise TypeError(f"snowtri supports float32/float64 {what}, not {a.dtype}")
        if not self._resident(a):
            raise ValueError(f"a tensor given to {self.who} must be a contiguous CUDA tensor (NumPy arrays are staged from the host)")
        return a, F32 if a.dtype == self.torch.float32 else F64

    def ints(self, a, shape, what):
        """An int32 array of exactly `shape` in: converted on the host, checked on the device."""
        if self.device is None:
            a = np.ascontiguousarray(a, dtype=np.int32)
            ok = a.shape == tuple(shape)
        else:
            ok = a.dtype == self.torch.int32 and self._resident(a) and tuple(a.shape) == tuple(shape)
        if not ok:
            raise ValueError(f"{what} given to {self.who} must be {'int32' if self.device is None else 'a contiguous int32 CUDA tensor'} "
                             f"of shape {tuple(shape)} (got {a.dtype} {tuple(a.shape)})")
        return a

    def empty(self, shape, kind):
        """An uninitialised output: kind = "float32", "float64", "int32", "int64", "uint8", or "flags" (uint32 on the host, int32 in torch)."""
        if kind == "flags":
            kind = "uint32" if self.device is None else "int32"
        if self.device is None:
            return np.empty(shape, dtype=kind)
        return self.torch.empty(tuple(shape), dtype=getattr(self.torch, kind), device=self.device)

    def empty_like(self, a):
        return self.empty(a.shape, str(a.dtype).replace("torch.", ""))

    def tail(self):
        """The two arguments that end a HOST/DEVICE entry point: (memory space, stream)."""
        return (HOST, None) if self.device is None else (DEVICE, ptr(self.stream))


class Context:
    """Owner of a snowtri_ctx (rig constants + device scratch).  Not thread-safe."""

    def __init__(self, K=None, R=None, t=None, device=0):
        L = self.L = lib()                  # the library this context belongs to (use_library may rebind the package later)
        if L.snowtri_device_count() <= 0:
            raise SnowtriError(ERR_NO_DEVICE, "snowtri_ctx_create")
        if K is None:
            C = 0
            Kc = Rc = tc = None
        else:
            Kc = np.ascontiguousarray(K, dtype=np.float64).reshape(-1, 9)
            C = Kc.shape[0]
            Rc = np.ascontiguousarray(R, dtype=np.float64).reshape(C, 9)
            tc = np.ascontiguousarray(t, dtype=np.float64).reshape(C, 3)
        h = ct.c_void_p()
        rc = L.snowtri_ctx_create(C, ptr(Kc), ptr(Rc), ptr(tc), int(device), ct.byref(h))
        if rc == ERR_SINGULAR:
            raise np.linalg.LinAlgError("Singular matrix")     # np.linalg.inv(K), camera.py:242
        check(rc, "snowtri_ctx_create")
        self.handle = h
        self.C = C
        self.device = int(device)

    def close(self):
        if getattr(self, "handle", None):
            self.L.snowtri_ctx_destroy(self.handle)
            self.handle = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def synchronize(self):
        check(self.L.snowtri_ctx_synchronize(self.handle), "snowtri_ctx_synchronize")

    def ray_matrices(self):
        M = np.empty((self.C, 9))
        check(self.L.snowtri_ctx_ray_matrices(self.handle, ptr(M)), "snowtri_ctx_ray_matrices")
        return M.reshape(self.C, 3, 3)

    def set_distortion(self, D):
        """Row N4: per-camera lens coefficients D[C, 5] = (k1, k2, p1, p2, k3) (Camera.D)."""
        D2 = np.asarray(D, dtype=np.float64).reshape(self.C, -1)
        if D2.shape[1] > 5:
            if np.any(D2[:, 5:] != 0.0):
                raise ValueError("only the 5-coefficient lens model (k1, k2, p1, p2, k3) is supported")
            D2 = D2[:, :5]
        Dc = np.zeros((self.C, 5), dtype=np.float64)          # OpenCV's shorter forms (4 coefficients) mean k3 = 0
        Dc[:, :D2.shape[1]] = D2
        check(self.L.snowtri_ctx_set_distortion(self.handle, ptr(Dc)), "snowtri_ctx_set_distortion")

    def undistort_keypoints(self, kpts):
        """Raw-image keypoints kpts[F, C, Pmax, J, 3] -> the same array with (u, v) moved to the undistorted
        image (scores untouched); host arrays, float32 or float64.  A pixel's result depends on that pixel and its camera's
        lens only (not on the batch around it); a non-finite u or v gives a non-finite u and v."""
        a = host_floats(kpts)
        F, C, Pmax, J, three = a.shape
        assert C == self.C and three == 3
        out = np.empty_like(a)
        check(self.L.snowtri_undistort_keypoints(self.handle, F, Pmax, J, ptr(a), ptr(out), dtype_code(a.dtype), HOST,
                                                None), "snowtri_undistort_keypoints")
        return out

    # ---- reprojection (include/snowtri.h, "Reprojection") -----------------------------------------
    @staticmethod
    def _records_in(space, xyzs):
        """xyzs [F, P, kn, 4] in `space` -> (array, dtype code, F, P, kn)."""
        xyzs, code = space.floats(xyzs, "joints")
        if len(xyzs.shape) != 4 or xyzs.shape[-1] != 4:
            raise ValueError(f"xyzs must be [F, P, kn, 4] records (got shape {tuple(xyzs.shape)})")
        F, P, kn, _ = (int(v) for v in xyzs.shape)
        return xyzs, code, F, P, kn

    def _reproject_status(self, rc, where):
        if rc == ERR_BAD_ARG:
            raise ValueError(f"{where}: {self.L.snowtri_last_error().decode()}")
        check(rc, where)

    def reproject(self, xyzs, raw=False, dtype=None, stream=None):
        """Joint records xyzs [F, P, kn, 4] (float32 / float64; a host array, or a contiguous CUDA tensor used in place and
        asynchronously on `stream`, default torch's current one) -> pix [F, C, P, kn, 3] = (u, v, score) in every camera, the
        layout of kpts; (0, 0, 0) where the record is missing, the point is behind the camera or the pixel is not finite.
        raw: pixels on the raw frame (set_distortion first).  dtype: of pix, float32 or float64 (default: that of xyzs)."""
        space = Space("Context.reproject", xyzs, stream=stream)
        xyzs, code, F, P, kn = self._records_in(space, xyzs)
        pcode = code if dtype is None else _float_code(dtype)
        pix = space.empty((F, self.C, P, kn, 3), "float32" if pcode == F32 else "float64")
        rc = self.L.snowtri_reproject(self.handle, F, P, kn, ptr(xyzs), code, REPROJECT_RAW if raw else 0, ptr(pix), pcode, *space.tail())
        self._reproject_status(rc, "snowtri_reproject")
        return pix

    def reproject_cost(self, xyzs, kpts, n_persons=None, keypoint_score_threshold=0.0, raw=False, stream=None):
        """xyzs [F, P, kn, 4] against the detections kpts [F, C, Pmax, kn, 3] (n_persons [F, C] int32 or None) ->
        (cost_sum [F, C, P, Pmax] float64 px^2, cost_n int32): per 3D person and detection the summed squared pixel distance over the
        joints whose projection is valid and whose detection counts, and how many those are.  Host arrays, or contiguous CUDA tensors
        (all of them) used in place and asynchronously on `stream`.  raw: compared on the raw frame (set_distortion first)."""
        space = Space("Context.reproject_cost", xyzs, kpts, n_persons, stream=stream)
        xyzs, code, F, P, kn = self._records_in(space, xyzs)
        if len(kpts.shape) != 5 or tuple(kpts.shape[:2]) != (F, self.C) or tuple(kpts.shape[3:]) != (kn, 3):
            raise ValueError(f"kpts must be [F={F}, C={self.C}, Pmax, kn={kn}, 3] (got shape {tuple(kpts.shape)})")
        kpts, kcode = space.floats(kpts, "keypoints")
        Pmax = int(kpts.shape[2])
        if n_persons is not None:
            n_persons = space.ints(n_persons, (F, self.C), "n_persons")
        cs, cn = space.empty((F, self.C, P, Pmax), "float64"), space.empty((F, self.C, P, Pmax), "int32")
        rc = self.L.snowtri_reproject_cost(self.handle, F, P, kn, ptr(xyzs), code, Pmax, ptr(kpts), kcode, ptr(n_persons),
                                           float(keypoint_score_threshold), REPROJECT_RAW if raw else 0, ptr(cs), ptr(cn), *space.tail())
        self._reproject_status(rc, "snowtri_reproject_cost")
        return cs, cn

    def assign_detections(self, cost_sum, cost_n, gate_px, min_joints=8, with_person_of=False, with_total=False, stream=None):
        """The optimal one-to-one matching of detections to 3D persons per problem (include/snowtri.h, "Assignment"; k_assign):
        cost_sum [..., P, Pmax] float64 and cost_n int32 of the same shape, as reproject_cost returns them (P + Pmax <= 64) ->
        det_of [..., P] int32 (the detection of person p, -1: unmatched, which costs gate_px^2), then with_person_of: person_of
        [..., Pmax] int32 (the person that took detection q, -1: nobody), with_total: total [...] float64 (the summed mean cost of the
        matched pairs); one array, or a tuple in that order.  Host arrays, or contiguous CUDA tensors (both) used in place and
        asynchronously on `stream`.  Every output equals reproject.assign_detections_reference bit for bit."""
        space = Space("Context.assign_detections", cost_sum, cost_n, stream=stream)
        if int(min_joints) != min_joints or int(min_joints) < 1:
            raise ValueError("min_joints must be >= 1")
        if not float(gate_px) >= 0.0:
            raise ValueError("gate_px must be >= 0 and not NaN")
        if not float(gate_px) <= 1e150:
            raise ValueError("gate_px must not exceed 1e150 (staying unmatched costs gate_px^2, which must stay finite)")
        if space.device is None:
            cost_sum, cost_n = np.ascontiguousarray(cost_sum, dtype=np.float64), np.asarray(cost_n)
        elif cost_sum.dtype != space.torch.float64 or not space._resident(cost_sum):
            raise ValueError("cost_sum given to Context.assign_detections must be a contiguous float64 CUDA tensor")
        if len(cost_sum.shape) < 2 or tuple(cost_sum.shape) != tuple(cost_n.shape):
            raise ValueError("cost_sum and cost_n must both be [..., P, Pmax]")
        cost_n = space.ints(cost_n, cost_sum.shape, "cost_n")
        lead, P, Pmax = tuple(int(v) for v in cost_sum.shape[:-2]), int(cost_sum.shape[-2]), int(cost_sum.shape[-1])
        n = int(np.prod(lead, dtype=np.int64))
        det_of = space.empty(lead + (P,), "int32")
        person_of = space.empty(lead + (Pmax,), "int32") if with_person_of else None
        total = space.empty(lead, "float64") if with_total else None
        rc = self.L.snowtri_assign_detections(self.handle, n, P, Pmax, ptr(cost_sum), ptr(cost_n), float(gate_px), int(min_joints), ptr(det_of),
                                              ptr(person_of), ptr(total), *space.tail())
        self._reproject_status(rc, "snowtri_assign_detections")
        out = (det_of,) + ((person_of,) if with_person_of else ()) + ((total,) if with_total else ())
        return out if len(out) > 1 else det_of

    @staticmethod
    def _huber(huber_px):
        """huber_px -> None (the squared loss: None or 0) or delta > 0, checked: finite, >= 0 and at most 1e150."""
        if huber_px is None:
            return None
        d = float(huber_px)
        if not (d >= 0.0 and d <= 1e150):
            raise ValueError(f"huber_px must be finite, >= 0 and at most 1e150 (got {huber_px!r})")
        return d if d > 0.0 else None

    def _refine_in(self, space, xyzs, kpts, n_persons, det_of, views, iters):
        """The inputs refine_joints and refine_cameras share, checked in `space` ->
        (xyzs, its dtype code, F, P, kn, kpts, its dtype code, Pmax, n_persons, det_of, views)."""
        xyzs, code, F, P, kn = self._records_in(space, xyzs)
        if len(kpts.shape) != 5 or tuple(kpts.shape[:2]) != (F, self.C) or tuple(kpts.shape[3:]) != (kn, 3):
            raise ValueError(f"kpts must be [F={F}, C={self.C}, Pmax, kn={kn}, 3] (got shape {tuple(kpts.shape)})")
        kpts, kcode = space.floats(kpts, "keypoints")
        Pmax = int(kpts.shape[2])
        if int(iters) != iters:
            raise ValueError(f"iters must be an integer in 1..16 (got {iters})")
        if n_persons is not None:
            n_persons = space.ints(n_persons, (F, self.C), "n_persons")
        if det_of is not None:
            if space.device is not None and det_of.dtype == space.torch.int64:
                det_of = det_of.to(space.torch.int32).contiguous()
            det_of = space.ints(det_of, (F, self.C, P), "det_of")
        if views is not None:
            if space.device is None:
                views = np.ascontiguousarray(views)
                if views.dtype not in (np.uint32, np.int32) or views.shape != (F, P, kn):
                    raise ValueError(f"views given to {space.who} must be uint32 of shape {(F, P, kn)} (got {views.dtype} {views.shape})")
            else:
                views = space.ints(views, (F, P, kn), "views")
        return xyzs, code, F, P, kn, kpts, kcode, Pmax, n_persons, det_of, views

    def refine_joints(self, xyzs, kpts, det_of=None, n_persons=None, views=None, keypoint_score_threshold=0.0, iters=4,
                      score_weights=False, diagnostics=False, out=None, stream=None, huber_px=None):
        """Joint records xyzs [F, P, kn, 4] moved to a local minimum of their reprojection error against the detections kpts
        [F, C, Pmax, kn, 3] on the undistorted frame (include/snowtri.h, "Refinement"; at most `iters` Gauss-Newton steps, a record's
        cost never rises, scores untouched).  det_of [F, C, P]: the detection of camera c that shows person p (match_detections'
        int64 is handed on as int32; -1: none; None: detection p).  n_persons [F, C] int32 or None.  views [F, P, kn]: bit c = camera
        c may be used (the uint32 / torch int32 mask of DLT_ROBUST's diagnostics; None: every camera).  score_weights: a view weighs
        its observation's score instead of 1.  Host arrays, or contiguous CUDA tensors (all of them) used in place and
        asynchronously on `stream`.  out: xyzs itself refines in place (default: a new array).
        -> the refined records, or (records, cost [F, P, kn, 2] float64: E before and after, codes [F, P, kn] uint8: REFINE_*)
        with diagnostics=True.  huber_px (delta > 0 in pixels; None or 0: the squared loss, today's entry and today's results): the
        Huber loss of include/snowtri.h, "Refinement", ROBUST LOSS (snowtri_refine_joints_ex); with diagnostics=True a fourth result,
        outliers [F, P, kn] (uint32, int32 in torch): bit c = camera c is a view of the record and in the linear regime at the
        output point.  views & ~outliers is an inlier mask; fewer than two bits in it mark a record its inliers do not fix."""
        huber_px = self._huber(huber_px)
        space = Space("Context.refine_joints", xyzs, kpts, n_persons, det_of, views, stream=stream)
        xyzs, code, F, P, kn, kpts, kcode, Pmax, n_persons, det_of, views = self._refine_in(space, xyzs, kpts, n_persons, det_of, views, iters)
        if out is None:
            out = space.empty_like(xyzs)
        elif out is not xyzs:
            raise ValueError("out must be None (a new array) or xyzs itself (in place)")
        cost = space.empty((F, P, kn, 2), "float64") if diagnostics else None
        codes = space.empty((F, P, kn), "uint8") if diagnostics else None
        if huber_px is not None:
            outliers = space.empty((F, P, kn), "flags") if diagnostics else None
            rc = self.L.snowtri_refine_joints_ex(self.handle, F, P, kn, ptr(xyzs), code, Pmax, ptr(kpts), kcode, ptr(n_persons), ptr(det_of),
                                                 ptr(views), float(keypoint_score_threshold), int(iters),
                                                 REFINE_SCORE_WEIGHTS if score_weights else 0, huber_px, ptr(out), ptr(cost), ptr(codes),
                                                 ptr(outliers), *space.tail())
            self._reproject_status(rc, "snowtri_refine_joints_ex")
            return (out, cost, codes, outliers) if diagnostics else out
        rc = self.L.snowtri_refine_joints(self.handle, F, P, kn, ptr(xyzs), code, Pmax, ptr(kpts), kcode, ptr(n_persons), ptr(det_of), ptr(views),
                                          float(keypoint_score_threshold), int(iters), REFINE_SCORE_WEIGHTS if score_weights else 0, ptr(out),
                                          ptr(cost), ptr(codes), *space.tail())
        self._reproject_status(rc, "snowtri_refine_joints")
        return (out, cost, codes) if diagnostics else out

    def refine_cameras(self, xyzs, kpts, det_of=None, n_persons=None, views=None, keypoint_score_threshold=0.0, free=None, min_obs=64,
                       iters=8, score_weights=False, diagnostics=False, stream=None, huber_px=None, intrinsics=None, intrinsics_free=None):
        """The rig's poses moved to a local minimum of every free camera's reprojection error against the detections kpts
        [F, C, Pmax, kn, 3] on the undistorted frame, the joint records xyzs [F, P, kn, 4] held fixed (include/snowtri.h, "Camera pose
        refinement"; at most `iters` Gauss-Newton steps on six parameters per camera, a camera's cost never rises).  det_of, n_persons,
        views, keypoint_score_threshold, score_weights: as for refine_joints.  free: the cameras that may move -- None (all), a bit
        mask, or a sequence of camera indices / of C booleans; a camera with fewer than min_obs (>= 3) observations stays.  Host
        arrays, or contiguous CUDA tensors (all of them) used in place and asynchronously on `stream`; ONE call in flight per context.
        THE CONTEXT'S RIG IS NOT CHANGED: build a new Context from what is returned.
        -> (R [C, 3, 3], t [C, 3]) float64, or (R, t, report) with diagnostics=True: report = dict(cost [C, 2]: E before and after,
        n_obs [C] int64, codes [C] uint8: POSE_*, normal [C, 28]: E, g[6], H[21] at the input pose).  huber_px (delta > 0 in pixels;
        None or 0: the squared loss, today's entry and no new key): the Huber loss ("Camera pose refinement", ROBUST LOSS;
        snowtri_refine_cameras_ex), and the report gains n_outliers [C] int64: the observations in the linear regime at the output pose.
        intrinsics ("f": fx and fy, "c": cx and cy, "fc"; None, the default: the entries above, nothing changes): those intrinsics are
        parameters too ("Camera pose refinement", INTRINSICS; snowtri_refine_cameras_k) -> (K [C, 3, 3], R, t) or (K, R, t, report)
        with report["normal"] [C, 66] = E, g[10], H[55]; intrinsics_free: the cameras whose intrinsics may move, given like `free`
        (None: all) and independent of it.  The first such call on a context allocates that path's own workspace."""
        if intrinsics is not None:
            if not isinstance(intrinsics, str) or intrinsics not in ("f", "c", "fc"):
                raise ValueError(f'intrinsics must be None, "f", "c" or "fc" (got {intrinsics!r})')
            return self._refine_cameras_k(xyzs, kpts, det_of, n_persons, views, keypoint_score_threshold, free, min_obs, iters, score_weights,
                                          diagnostics, stream, huber_px, (INTR_FOCAL if "f" in intrinsics else 0) | (INTR_CENTRE if "c" in intrinsics else 0),
                                          intrinsics_free)
        huber_px = self._huber(huber_px)
        space = Space("Context.refine_cameras", xyzs, kpts, n_persons, det_of, views, stream=stream)
        xyzs, code, F, P, kn, kpts, kcode, Pmax, n_persons, det_of, views = self._refine_in(space, xyzs, kpts, n_persons, det_of, views, iters)
        if int(min_obs) != min_obs:
            raise ValueError(f"min_obs must be an integer >= 3 (got {min_obs})")
        mask = free_mask(free, self.C)
        R, t = space.empty((self.C, 3, 3), "float64"), space.empty((self.C, 3), "float64")
        rep = dict(cost=space.empty((self.C, 2), "float64"), n_obs=space.empty((self.C,), "int64"), codes=space.empty((self.C,), "uint8"),
                   normal=space.empty((self.C, 28), "float64")) if diagnostics else dict(cost=None, n_obs=None, codes=None, normal=None)
        if huber_px is not None:
            if diagnostics:
                rep["n_outliers"] = space.empty((self.C,), "int64")
            rc = self.L.snowtri_refine_cameras_ex(self.handle, F, P, kn, ptr(xyzs), code, Pmax, ptr(kpts), kcode, ptr(n_persons), ptr(det_of),
                                                  ptr(views), float(keypoint_score_threshold), mask, int(min_obs), int(iters),
                                                  REFINE_SCORE_WEIGHTS if score_weights else 0, huber_px, ptr(R), ptr(t), ptr(rep["cost"]),
                                                  ptr(rep["n_obs"]), ptr(rep["codes"]), ptr(rep["normal"]), ptr(rep.get("n_outliers")),
                                                  *space.tail())
            self._reproject_status(rc, "snowtri_refine_cameras_ex")
            return (R, t, rep) if diagnostics else (R, t)
        rc = self.L.snowtri_refine_cameras(self.handle, F, P, kn, ptr(xyzs), code, Pmax, ptr(kpts), kcode, ptr(n_persons), ptr(det_of), ptr(views),
                                           float(keypoint_score_threshold), mask, int(min_obs), int(iters),
                                           REFINE_SCORE_WEIGHTS if score_weights else 0, ptr(R), ptr(t), ptr(rep["cost"]), ptr(rep["n_obs"]),
                                           ptr(rep["codes"]), ptr(rep["normal"]), *space.tail())
        self._reproject_status(rc, "snowtri_refine_cameras")
        return (R, t, rep) if diagnostics else (R, t)

    def _refine_cameras_k(self, xyzs, kpts, det_of, n_persons, views, keypoint_score_threshold, free, min_obs, iters, score_weights, diagnostics,
                          stream, huber_px, intr_flags, intrinsics_free):
        """refine_cameras with intrinsics set: snowtri_refine_cameras_k."""
        huber_px = self._huber(huber_px)
        space = Space("Context.refine_cameras", xyzs, kpts, n_persons, det_of, views, stream=stream)
        xyzs, code, F, P, kn, kpts, kcode, Pmax, n_persons, det_of, views = self._refine_in(space, xyzs, kpts, n_persons, det_of, views, iters)
        if int(min_obs) != min_obs:
            raise ValueError(f"min_obs must be an integer >= 3 (got {min_obs})")
        mask, imask = free_mask(free, self.C), free_mask(intrinsics_free, self.C)
        K, R, t = space.empty((self.C, 3, 3), "float64"), space.empty((self.C, 3, 3), "float64"), space.empty((self.C, 3), "float64")
        rep = dict(cost=space.empty((self.C, 2), "float64"), n_obs=space.empty((self.C,), "int64"), codes=space.empty((self.C,), "uint8"),
                   normal=space.empty((self.C, 66), "float64")) if diagnostics else dict(cost=None, n_obs=None, codes=None, normal=None)
        if huber_px is not None and diagnostics:
            rep["n_outliers"] = space.empty((self.C,), "int64")
        rc = self.L.snowtri_refine_cameras_k(self.handle, F, P, kn, ptr(xyzs), code, Pmax, ptr(kpts), kcode, ptr(n_persons), ptr(det_of), ptr(views),
                                             float(keypoint_score_threshold), mask, imask, int(intr_flags), int(min_obs), int(iters),
                                             REFINE_SCORE_WEIGHTS if score_weights else 0, 0.0 if huber_px is None else huber_px, ptr(K), ptr(R),
                                             ptr(t), ptr(rep["cost"]), ptr(rep["n_obs"]), ptr(rep["codes"]), ptr(rep["normal"]),
                                             ptr(rep.get("n_outliers")), *space.tail())
        self._reproject_status(rc, "snowtri_refine_cameras_k")
        return (K, R, t, rep) if diagnostics else (K, R, t)

    def triangulate_matched(self, kpts, det_of=None, n_persons=None, keypoint_score_threshold=0.0, reproj_threshold_px=6.0, max_drops=1,
                            dtype=None, diagnostics=False, stream=None):
        """The robust N-view DLT of 3D person p over the detections det_of names (include/snowtri.h, "Matched triangulation";
        k_dlt_matched): kpts [F, C, Pmax, kn, 3] on the undistorted frame (float32 / float64), det_of [F, C, P] (match_detections'
        int64 is handed on as int32; -1: none; None: detection p, P = Pmax), n_persons [F, C] int32 or None; reproj_threshold_px and
        max_drops as for DLT_ROBUST.  Host arrays, or contiguous CUDA tensors (all of them) used in place and asynchronously on
        `stream`.  dtype: of the outputs, float32 or float64 (default: that of kpts).
        -> (xyzs [F, P, kn, 4], pscore [F, P]), or (xyzs, pscore, views [F, P, kn] uint32 / torch int32, resid [F, P, kn] px) with
        diagnostics=True.  A person's outputs equal DLT_ROBUST's on its gathered keypoints bit for bit."""
        space = Space("Context.triangulate_matched", kpts, n_persons, det_of, stream=stream)
        if len(kpts.shape) != 5 or int(kpts.shape[1]) != self.C or int(kpts.shape[4]) != 3:
            raise ValueError(f"kpts must be [F, C={self.C}, Pmax, kn, 3] (got shape {tuple(kpts.shape)})")
        kpts, kcode = space.floats(kpts, "keypoints")
        F, _, Pmax, kn, _ = (int(v) for v in kpts.shape)
        if n_persons is not None:
            n_persons = space.ints(n_persons, (F, self.C), "n_persons")
        P = Pmax
        if det_of is not None:
            if len(det_of.shape) != 3:
                raise ValueError(f"det_of must be [F={F}, C={self.C}, P] (got shape {tuple(det_of.shape)})")
            P = int(det_of.shape[2])
            if space.device is not None and det_of.dtype == space.torch.int64:
                det_of = det_of.to(space.torch.int32).contiguous()
            det_of = space.ints(det_of, (F, self.C, P), "det_of")
        ocode = kcode if dtype is None else _float_code(dtype)
        kind = "float32" if ocode == F32 else "float64"
        xyzs, pscore = space.empty((F, P, kn, 4), kind), space.empty((F, P), kind)
        views = space.empty((F, P, kn), "flags") if diagnostics else None
        resid = space.empty((F, P, kn), kind) if diagnostics else None
        rc = self.L.snowtri_triangulate_matched(self.handle, F, P, kn, Pmax, ptr(kpts), kcode, ptr(n_persons), ptr(det_of),
                                                float(keypoint_score_threshold), float(reproj_threshold_px), int(max_drops), ptr(xyzs),
                                                ptr(pscore), ocode, ptr(views), ptr(resid), *space.tail())
        self._reproject_status(rc, "snowtri_triangulate_matched")
        return (xyzs, pscore, views, resid) if diagnostics else (xyzs, pscore)

    def pair_cost(self, kpts, n_persons=None, claimed=None, keypoint_score_threshold=0.0, stream=None):
        """The squared line distance of every pair of detections of two cameras (include/snowtri.h, "Seeding"; k_pair_cost): kpts
        [F, C, Pmax, kn, 3] on the undistorted frame (float32 / float64), n_persons [F, C] int32 or None, claimed [F, C, Pmax] int32
        or None (>= 0: the detection is taken -- assign_detections' person_of; its int64 is handed on as int32) ->
        (pair_sum [F, NP, Pmax, Pmax] float64, world units squared, pair_n int32), NP = C (C - 1) / 2 camera pairs (a < b) in the
        reference's loop order.  Host arrays, or contiguous CUDA tensors (all of them) used in place and asynchronously on `stream`."""
        space = Space("Context.pair_cost", kpts, n_persons, claimed, stream=stream)
        if len(kpts.shape) != 5 or int(kpts.shape[1]) != self.C or int(kpts.shape[4]) != 3:
            raise ValueError(f"kpts must be [F, C={self.C}, Pmax, kn, 3] (got shape {tuple(kpts.shape)})")
        kpts, kcode = space.floats(kpts, "keypoints")
        F, _, Pmax, kn, _ = (int(v) for v in kpts.shape)
        n_persons, claimed = self._seed_lists(space, n_persons, claimed, F, Pmax)
        NP = self.C * (self.C - 1) // 2
        ps, pn = space.empty((F, NP, Pmax, Pmax), "float64"), space.empty((F, NP, Pmax, Pmax), "int32")
        rc = self.L.snowtri_pair_cost(self.handle, F, kn, Pmax, ptr(kpts), kcode, ptr(n_persons), ptr(claimed), float(keypoint_score_threshold),
                                      ptr(ps), ptr(pn), *space.tail())
        self._reproject_status(rc, "snowtri_pair_cost")
        return ps, pn

    def _seed_lists(self, space, n_persons, claimed, F, Pmax):
        """n_persons [F, C] and claimed [F, C, Pmax] of the seeding entries, checked in `space` (None stays None)."""
        if n_persons is not None:
            n_persons = space.ints(n_persons, (F, self.C), "n_persons")
        if claimed is not None:
            if space.device is not None and claimed.dtype == space.torch.int64:
                claimed = claimed.to(space.torch.int32).contiguous()
            claimed = space.ints(claimed, (F, self.C, Pmax), "claimed")
        return n_persons, claimed

    def seed_persons(self, pair_sum, pair_n, n_persons=None, claimed=None, S=None, gate=0.05, min_joints=8, min_views=3, with_flags=False,
                     stream=None):
        """A frame's free detections grouped into seeds (include/snowtri.h, "Seeding"; k_seed_group): pair_sum [F, NP, Pmax, Pmax]
        float64 and pair_n int32 as pair_cost returns them (C * Pmax <= 64), n_persons, claimed as for pair_cost, S seed slots
        (1..64; default min(64, C * Pmax // min_views)), gate an RMS line distance in world units ->
        (seed_det_of [F, C, S] int32 in the layout of det_of, n_seeds [F] int32), with_flags: also flags [F] (SEED_FLAG_FULL).
        Host arrays, or contiguous CUDA tensors (all of them).  Every output equals seed.seed_persons_reference bit for bit."""
        space = Space("Context.seed_persons", pair_sum, pair_n, n_persons, claimed, stream=stream)
        NP = self.C * (self.C - 1) // 2
        if len(pair_sum.shape) != 4 or int(pair_sum.shape[1]) != NP or int(pair_sum.shape[2]) != int(pair_sum.shape[3]) or \
                tuple(pair_sum.shape) != tuple(pair_n.shape):
            raise ValueError(f"pair_sum and pair_n must both be [F, NP={NP}, Pmax, Pmax] (got shapes {tuple(pair_sum.shape)}, {tuple(pair_n.shape)})")
        if space.device is None:
            pair_sum = np.ascontiguousarray(pair_sum, dtype=np.float64)
        elif pair_sum.dtype != space.torch.float64 or not space._resident(pair_sum):
            raise ValueError("pair_sum given to Context.seed_persons must be a contiguous float64 CUDA tensor")
        pair_n = space.ints(pair_n, pair_sum.shape, "pair_n")
        F, Pmax = int(pair_sum.shape[0]), int(pair_sum.shape[2])
        n_persons, claimed = self._seed_lists(space, n_persons, claimed, F, Pmax)
        if int(min_joints) != min_joints or int(min_views) != min_views:
            raise ValueError("min_joints and min_views must be integers")
        if S is None:
            S = max(1, min(64, self.C * Pmax // max(2, int(min_views))))
        if int(S) != S:
            raise ValueError("S must be an integer in 1..64")
        seed_det_of, n_seeds = space.empty((F, self.C, int(S)), "int32"), space.empty((F,), "int32")
        flags = space.empty((F,), "flags") if with_flags else None
        rc = self.L.snowtri_seed_persons(self.handle, F, Pmax, ptr(pair_sum), ptr(pair_n), ptr(n_persons), ptr(claimed), float(gate),
                                         int(min_joints), int(min_views), int(S), ptr(seed_det_of), ptr(n_seeds), ptr(flags), *space.tail())
        self._reproject_status(rc, "snowtri_seed_persons")
        return (seed_det_of, n_seeds, flags) if with_flags else (seed_det_of, n_seeds)

    def set_timing(self, enabled=True, attach=False):
        """attach: single-kernel calls carry the event pair on their dispatch (the kernel's own begin / end) instead of being bracketed."""
        check(self.L.snowtri_set_timing(self.handle, (2 if attach else 1) if enabled else 0), "snowtri_set_timing")

    def last_kernel_ms(self):
        arr = (ct.c_float * 2)()
        check(self.L.snowtri_last_kernel_ms(self.handle, ct.byref(arr)), "snowtri_last_kernel_ms")
        return float(arr[0]), float(arr[1])

    def timing_collect(self, cap=1024):
        """Durations (ms) of the fused calls recorded since the last collect (timing must be enabled)."""
        arr = (ct.c_float * cap)()
        n = self.L.snowtri_timing_collect(self.handle, arr, cap)
        if n < 0:
            raise SnowtriError(ERR_HIP, "snowtri_timing_collect")
        return [float(arr[i]) for i in range(n)]

    def overrides(self):
        """Test knobs (environment) this context was created under: "" when it runs the defaults."""
        return (self.L.snowtri_ctx_overrides(self.handle) or b"").decode()

    def set_overlap(self, n_streams):
        """Overlap mode: device calls of the fused entry rotate over n internal streams (1 = off); join() before reading results."""
        check(self.L.snowtri_ctx_set_overlap(self.handle, int(n_streams)), "snowtri_ctx_set_overlap")

    def set_split(self, segments):
        """Segments of one multi-person call (snowtri_ctx_set_split): 1 = the caller's stream only, >= 2 forced, 0 = the default policy."""
        check(self.L.snowtri_ctx_set_split(self.handle, int(segments)), "snowtri_ctx_set_split")

    def set_robust(self, reproj_threshold_px=6.0, max_drops=1):
        """Settings of method = DLT_ROBUST through the fused call (snowtri_ctx_set_robust): residual gate in pixels, views a joint may lose."""
        check(self.L.snowtri_ctx_set_robust(self.handle, float(reproj_threshold_px), int(max_drops)), "snowtri_ctx_set_robust")

    def join(self, stream=None):
        """`stream` (a HIP stream handle, default the null stream) waits for every overlapped call issued since the last join."""
        check(self.L.snowtri_ctx_join(self.handle, ptr(stream)), "snowtri_ctx_join")

    def last_stream_counts(self):
        """(frames past the association's first launch, frames with an exactly re-done candidate sum, frames left to
        k_frame_recompute) of the last multi-person call's last segment; (-1, -1, -1) if it did not take the streaming route."""
        arr = (ct.c_int64 * 3)()
        check(self.L.snowtri_last_stream_counts(self.handle, ct.byref(arr)), "snowtri_last_stream_counts")
        return int(arr[0]), int(arr[1]), int(arr[2])

    def stream_probes(self):
        """(probes run, internal streams discarded, verdict on the stream kept last: 1 = runs beside the others, 0 = no
        candidate did, -1 = no internal stream yet) -- see snowtri_ctx_stream_probes."""
        arr = (ct.c_int64 * 3)()
        check(self.L.snowtri_ctx_stream_probes(self.handle, ct.byref(arr)), "snowtri_ctx_stream_probes")
        return int(arr[0]), int(arr[1]), int(arr[2])

    def last_slow_frames(self):
        return int(self.L.snowtri_last_slow_frames(self.handle))

    def last_kernel_names(self):
        """Template names of the kernels the last fused call launched, in launch order."""
        return (self.L.snowtri_last_kernel_names(self.handle) or b"").decode()

    def debug_faults(self):
        """(violated device-side bounds checks since the last call, code << 32 | line of the first); (-1, 0) unless the
        library is the -DSNOWTRI_DEBUG_BOUNDS build (libsnowtri_dbg.so)."""
        first = ct.c_uint64(0)
        n = int(self.L.snowtri_debug_faults(self.handle, ct.byref(first)))
        return n, int(first.value)

    def last_handover_persons(self):
        """(persons fused as complete-graph clusters, persons fused from member lists) of the last multi-person call,
        (-1, -1) if it did not arm the hand-over."""
        other = ct.c_int64(-1)
        n = int(self.L.snowtri_last_handover_persons(self.handle, ct.byref(other)))
        return n, int(other.value)


_scratch_ctx = {}


def current_device():
    """The HIP device index the calling thread's work should land on: torch's current device when torch is loaded
    and sees a GPU (one process per GPU sets it with torch.cuda.set_device(local_rank)), else SNOWTRI_DEVICE or 0."""
    import sys
    t = sys.modules.get("torch")
    if t is not None:
        try:
            if t.cuda.is_available():
                return int(t.cuda.current_device())
        except Exception:
            pass
    return int(os.environ.get("SNOWTRI_DEVICE", "0"))


def scratch_context(device=None):
    """Rig-less context for entry points that need only device scratch (condense, skew rays, smoothing).
    One per device: a context's scratch and kernels live on the GPU it was created for."""
    dev = current_device() if device is None else int(device)
    key = (LIB_PATH, dev)                   # (a context belongs to the library that made it)
    ctx = _scratch_ctx.get(key)
    if ctx is None:
        ctx = _scratch_ctx[key] = Context(device=dev)
    return ctx
