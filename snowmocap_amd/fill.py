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

import numpy as np

from . import _lib
from .records import as_records, missing_records, run_record_pass  # noqa: F401  (missing_records: rule 1, importable from here)

FILL_MEASURED, FILL_LERP, FILL_HOLD, FILL_MISSING = 0, 1, 2, 3
MAX_GAP = 255                  # max_gap: 1 .. 255


def fill_block_frames():
    """Frames per tile of k_fill_gaps (snowtri_fill_block_frames): gaps around its multiples cross from one tile to the next."""
    return int(_lib.lib().snowtri_fill_block_frames())


def _check_max_gap(max_gap):
    if not (1 <= int(max_gap) <= MAX_GAP):
        raise ValueError(f"max_gap must lie in 1..{MAX_GAP} (got {max_gap})")
    return int(max_gap)


def fill_joint_track_reference(xyzs, max_gap):
    """xyzs [T, ..., 4] (float32 / float64; the axes between the first and the last are the lanes) -> (out, codes): out of
    the same shape and dtype, codes uint8 of shape xyzs.shape[:-1].  Pure NumPy."""
    max_gap = _check_max_gap(max_gap)
    xyzs, x, T, m = as_records(xyzs)
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
    return run_record_pass(ctx, xyzs, "snowtri_fill_joint_track", (_check_max_gap(max_gap),), codes, stream, "fill_joint_track")
