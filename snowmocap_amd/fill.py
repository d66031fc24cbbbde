"""Gap filling: short dropouts in a track of joint records bridged before the temporal filter sees them.

The condense step leaves a joint too few views saw as the record (0, 0, 0, 0), and a tracked person who is absent for a few
frames leaves whole skeletons of them; a filter takes either for a position at the origin.  The rule (include/snowtri.h,
"Gap filling") on xyzs[T][m][4] = (x, y, z, score), every lane on its own, all decisions and arithmetic in fp64:

  1. a record is MISSING if its score == 0 (so -0.0 too) or any of its four values is not finite, else MEASURED;
  2. a run of g <= max_gap missing records between the measured records A (frame a) and B (frame a + g + 1): record a + k
     becomes A + (k / (g + 1)) * (B - A) in all four components, every operation rounded separately, the result rounded
     once to the array's dtype -- code FILL_LERP;
  3. a run of at most max_gap missing records at the start (end) of the array becomes copies of the first (last) measured
     record -- code FILL_HOLD;
  4. everything else is copied bit for bit: FILL_MEASURED, or FILL_MISSING for a missing record no rule filled.

`fill_joint_track_reference` is that rule in NumPy (no GPU, no library): the oracle of the kernel, which must agree with it
bit for bit.  `fill_joint_track` runs the HIP kernel (snowtri_fill_joint_track).
"""
from __future__ import annotations

import ctypes as ct

import numpy as np

from . import _lib

FILL_MEASURED, FILL_LERP, FILL_HOLD, FILL_MISSING = 0, 1, 2, 3
MAX_GAP = 255                  # max_gap: 1 .. 255


def fill_block_frames():
    """Frames per tile of k_fill_gaps (snowtri_fill_block_frames): gaps around its multiples cross from one tile to the next."""
    return int(_lib.lib().snowtri_fill_block_frames())


def _check_max_gap(max_gap):
    if not (1 <= int(max_gap) <= MAX_GAP):
        raise ValueError(f"max_gap must lie in 1..{MAX_GAP} (got {max_gap})")
    return int(max_gap)


def _check_shape(shape):
    if len(shape) < 2 or shape[-1] != 4:
        raise ValueError(f"xyzs must be [T, ..., 4] records (got shape {tuple(shape)})")


def missing_records(xyzs):
    """[..., 4] records -> bool [...]: rule 1 (score == 0, or a value that is not finite)."""
    v = np.asarray(xyzs).astype(np.float64)
    return (v[..., 3] == 0) | ~np.isfinite(v).all(axis=-1)


def fill_joint_track_reference(xyzs, max_gap):
    """xyzs [T, ..., 4] (float32 / float64; the axes between the first and the last are the lanes) -> (out, codes): out of
    the same shape and dtype, codes uint8 of shape xyzs.shape[:-1].  Pure NumPy."""
    xyzs = np.asarray(xyzs)
    if xyzs.dtype != np.float32:
        xyzs = xyzs.astype(np.float64, copy=False)
    max_gap = _check_max_gap(max_gap)
    _check_shape(xyzs.shape)
    T = xyzs.shape[0]
    m = int(np.prod(xyzs.shape[1:-1], dtype=np.int64))
    x = np.ascontiguousarray(xyzs).reshape(T, m, 4)
    out = x.copy()
    codes = np.zeros((T, m), dtype=np.uint8)
    if T == 0 or m == 0:
        return out.reshape(xyzs.shape), codes.reshape(xyzs.shape[:-1])
    miss = missing_records(x)
    frame = np.arange(T, dtype=np.int64)[:, None]
    prev = np.maximum.accumulate(np.where(miss, -1, frame), axis=0)                   # last measured frame <= t, -1 = none
    nxt = np.minimum.accumulate(np.where(miss, T, frame)[::-1], axis=0)[::-1]         # next measured frame >= t, T = none
    g = nxt - prev - 1                                                                # length of the run a missing record is in
    lerp = miss & (prev >= 0) & (nxt < T) & (g <= max_gap)
    lead = miss & (prev < 0) & (nxt < T) & (nxt <= max_gap)
    trail = miss & (prev >= 0) & (nxt >= T) & (T - 1 - prev <= max_gap)
    codes[miss] = FILL_MISSING
    codes[lerp], codes[lead | trail] = FILL_LERP, FILL_HOLD
    lane = np.broadcast_to(np.arange(m)[None, :], (T, m))
    tt, ll = np.nonzero(lerp)
    if tt.size:
        A = x[prev[tt, ll], ll].astype(np.float64)
        B = x[nxt[tt, ll], ll].astype(np.float64)
        w = ((tt - prev[tt, ll]).astype(np.float64) / (g[tt, ll] + 1).astype(np.float64))[:, None]
        with np.errstate(all="ignore"):
            d = B - A
            p = w * d
            out[tt, ll] = (A + p).astype(x.dtype)                                     # separately rounded: NumPy fuses nothing
    out[lead] = x[nxt[lead], lane[lead]]
    out[trail] = x[prev[trail], lane[trail]]
    return out.reshape(xyzs.shape), codes.reshape(xyzs.shape[:-1])


def fill_joint_track(ctx, xyzs, max_gap, codes=True, stream=None):
    """The fill on the GPU.  ctx: a _lib.Context (None: the rig-less scratch context of the current device).  xyzs [T, ..., 4],
    float32 or float64: a CUDA(=HIP) tensor is used in place, asynchronously on `stream` (default: torch's current stream), and
    tensors come back; anything else is taken as a NumPy array, staged and synchronous.  Returns (out, codes) with codes
    uint8 of shape xyzs.shape[:-1], or None with codes=False (the kernel then does not write them)."""
    max_gap = _check_max_gap(max_gap)
    if ctx is None:
        ctx = _lib.scratch_context()
    L, h = ctx.L, ctx.handle
    if hasattr(xyzs, "is_cuda"):
        import torch
        if xyzs.dtype not in (torch.float32, torch.float64):
            raise TypeError(f"snowtri supports float32/float64 joints, not {xyzs.dtype}")
        _check_shape(xyzs.shape)
        if not xyzs.is_cuda or not xyzs.is_contiguous():
            raise ValueError("a tensor given to fill_joint_track must be a contiguous CUDA tensor (NumPy arrays are staged from the host)")
        code = _lib.F32 if xyzs.dtype == torch.float32 else _lib.F64
        T = int(xyzs.shape[0])
        m = int(xyzs.numel() // (4 * T)) if T else 0
        out = torch.empty_like(xyzs)
        fl = torch.empty(xyzs.shape[:-1], dtype=torch.uint8, device=xyzs.device) if codes else None
        if stream is None:
            stream = torch.cuda.current_stream(xyzs.device).cuda_stream
        args = (ct.c_void_p(xyzs.data_ptr()), code, max_gap, ct.c_void_p(out.data_ptr()),
                ct.c_void_p(fl.data_ptr()) if codes else None, _lib.DEVICE, ct.c_void_p(stream) if stream else None)
    else:
        xyzs = np.asarray(xyzs)
        if xyzs.dtype != np.float32:
            xyzs = xyzs.astype(np.float64, copy=False)
        xyzs = np.ascontiguousarray(xyzs)
        _check_shape(xyzs.shape)
        T = int(xyzs.shape[0])
        m = int(xyzs.size // (4 * T)) if T else 0
        out = np.empty_like(xyzs)
        fl = np.empty(xyzs.shape[:-1], dtype=np.uint8) if codes else None
        args = (_lib.ptr(xyzs), _lib.dtype_code(xyzs.dtype), max_gap, _lib.ptr(out), _lib.ptr(fl), _lib.HOST, None)
    rc = L.snowtri_fill_joint_track(h, T, m, *args)
    if rc == _lib.ERR_BAD_ARG:
        raise ValueError(f"snowtri_fill_joint_track: {L.snowtri_last_error().decode()}")
    _lib.check(rc, "snowtri_fill_joint_track")
    return out, fl
