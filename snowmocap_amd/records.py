"""Joint records: what the passes over a track xyzs[T][m][4] = (x, y, z, score) share (fill.py, despike.py; the kernels' side
of it is snowmocap_amd/csrc/snowtri_record.hpp).

A record is MISSING if its score == 0 (so -0.0 too) or any of its four values is not finite, else MEASURED: rule 1 of
"Gap filling" and of "Despiking" in include/snowtri.h.
"""
from __future__ import annotations

import ctypes as ct

import numpy as np

from . import _lib


def missing_records(xyzs):
    """[..., 4] records -> bool [...]: rule 1 (score == 0, or a value that is not finite)."""
    v = np.asarray(xyzs).astype(np.float64)
    return (v[..., 3] == 0) | ~np.isfinite(v).all(axis=-1)


def check_shape(shape):
    if len(shape) < 2 or shape[-1] != 4:
        raise ValueError(f"xyzs must be [T, ..., 4] records (got shape {tuple(shape)})")


def as_records(xyzs):
    """xyzs [T, ..., 4] (anything but float32 becomes float64; the axes between the first and the last are the lanes) ->
    (xyzs as that array, x [T, m, 4] contiguous, T, m).  For the NumPy references."""
    xyzs = np.asarray(xyzs)
    if xyzs.dtype != np.float32:
        xyzs = xyzs.astype(np.float64, copy=False)
    check_shape(xyzs.shape)
    T = xyzs.shape[0]
    m = int(np.prod(xyzs.shape[1:-1], dtype=np.int64))
    return xyzs, np.ascontiguousarray(xyzs).reshape(T, m, 4), T, m


def run_record_pass(ctx, xyzs, entry_name, extra_args, codes, stream, who):
    """The body of the GPU wrapper `who` (fill_joint_track, despike_joint_track; their docstrings say what xyzs, codes and stream may
    be): the C entry point `entry_name` on xyzs [T, ..., 4], `extra_args` being its ctypes arguments between xyz_dtype and out."""
    if ctx is None:
        ctx = _lib.scratch_context()
    if hasattr(xyzs, "is_cuda"):
        import torch
        if xyzs.dtype not in (torch.float32, torch.float64):
            raise TypeError(f"snowtri supports float32/float64 joints, not {xyzs.dtype}")
        check_shape(xyzs.shape)
        if not xyzs.is_cuda or not xyzs.is_contiguous():
            raise ValueError(f"a tensor given to {who} must be a contiguous CUDA tensor (NumPy arrays are staged from the host)")
        dtype = _lib.F32 if xyzs.dtype == torch.float32 else _lib.F64
        T, size = int(xyzs.shape[0]), xyzs.numel()
        out = torch.empty_like(xyzs)
        cd = torch.empty(xyzs.shape[:-1], dtype=torch.uint8, device=xyzs.device) if codes else None
        if stream is None:
            stream = torch.cuda.current_stream(xyzs.device).cuda_stream
        ptrs = (ct.c_void_p(xyzs.data_ptr()), ct.c_void_p(out.data_ptr()), ct.c_void_p(cd.data_ptr()) if codes else None)
        where = (_lib.DEVICE, ct.c_void_p(stream) if stream else None)
    else:
        xyzs = np.asarray(xyzs)
        if xyzs.dtype != np.float32:
            xyzs = xyzs.astype(np.float64, copy=False)
        xyzs = np.ascontiguousarray(xyzs)
        check_shape(xyzs.shape)
        dtype = _lib.dtype_code(xyzs.dtype)
        T, size = int(xyzs.shape[0]), xyzs.size
        out = np.empty_like(xyzs)
        cd = np.empty(xyzs.shape[:-1], dtype=np.uint8) if codes else None
        ptrs = (_lib.ptr(xyzs), _lib.ptr(out), _lib.ptr(cd))
        where = (_lib.HOST, None)
    m = int(size // (4 * T)) if T else 0
    rc = getattr(ctx.L, entry_name)(ctx.handle, T, m, ptrs[0], dtype, *extra_args, ptrs[1], ptrs[2], *where)
    if rc == _lib.ERR_BAD_ARG:
        raise ValueError(f"{entry_name}: {ctx.L.snowtri_last_error().decode()}")
    _lib.check(rc, entry_name)
    return out, cd
