"""Joint records: what the passes over a track xyzs[T][m][4] = (x, y, z, score) share (fill.py, despike.py; the kernels' side
of it is snowmocap_amd/csrc/snowtri_record.hpp).

A record is MISSING if its score == 0 (so -0.0 too) or any of its four values is not finite, else MEASURED: rule 1 of
"Gap filling" and of "Despiking" in include/snowtri.h.
"""
from __future__ import annotations

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
    (xyzs as that contiguous array, x = its view [T, m, 4], T, m).  For the NumPy references."""
    xyzs = _lib.host_floats(xyzs)
    check_shape(xyzs.shape)
    T = xyzs.shape[0]
    m = int(np.prod(xyzs.shape[1:-1], dtype=np.int64))
    return xyzs, xyzs.reshape(T, m, 4), T, m


def run_record_pass(ctx, xyzs, entry_name, extra_args, codes, stream, who):
    """The body of the GPU wrapper `who` (fill_joint_track, despike_joint_track; their docstrings say what xyzs, codes and stream may
    be): the C entry point `entry_name` on xyzs [T, ..., 4], `extra_args` being its ctypes arguments between xyz_dtype and out."""
    if ctx is None:
        ctx = _lib.scratch_context()
    space = _lib.Space(who, xyzs, stream=stream)
    xyzs, dtype = space.floats(xyzs, "joints")
    check_shape(xyzs.shape)
    T = int(xyzs.shape[0])
    m = int(np.prod(xyzs.shape[1:-1], dtype=np.int64)) if T else 0
    out = space.empty_like(xyzs)
    cd = space.empty(xyzs.shape[:-1], "uint8") if codes else None
    rc = getattr(ctx.L, entry_name)(ctx.handle, T, m, _lib.ptr(xyzs), dtype, *extra_args, _lib.ptr(out), _lib.ptr(cd), *space.tail())
    if rc == _lib.ERR_BAD_ARG:
        raise ValueError(f"{entry_name}: {ctx.L.snowtri_last_error().decode()}")
    _lib.check(rc, entry_name)
    return out, cd
