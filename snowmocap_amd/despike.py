"""Despiking: one- and two-frame jumps taken out of a track of joint records before gap filling.

A joint that was SEEN in the wrong place for a frame or two -- a flipped limb, a hand found on the neighbour -- is a measured
record: the gap filler leaves it alone and the second-order filter rings on it.  The rule (include/snowtri.h, "Despiking") on
xyzs[T][m][4] = (x, y, z, score), every lane on its own, all decisions in fp64:

  1. a record is MISSING if its score == 0 (so -0.0 too) or any of its four values is not finite, else MEASURED (records.py);
  2. the window of record (t, l): the n measured records of lane l at frames max(0, t - h) .. min(T - 1, t + h), itself included;
  3. per coordinate med = (v[(n - 1) // 2] + v[n // 2]) * 0.5 of the n values sorted ascending;
  4. d = value - med, d2 = (dx * dx + dy * dy) + dz * dz, every operation rounded separately;
  5. a measured record is a SPIKE iff n >= 3 and d2 > tol * tol (so not at equality, and not for a NaN d2);
  6. every spike is decided on the input: no iteration;
  7. DESPIKE_MARK writes a spike as four +0.0 (the gap filler's zero record), DESPIKE_REPLACE as (med + 0.0) rounded once to the
     array's dtype with the record's own score; everything else is copied bit for bit;
  8. codes: DESPIKE_KEPT, DESPIKE_SPIKE, DESPIKE_MISSING, DESPIKE_UNSUPPORTED (measured with n < 3: copied untested).

`despike_joint_track_reference` is that rule in NumPy (no GPU, no library): the oracle of the kernel, which must agree with it
bit for bit.  `despike_joint_track` runs the HIP kernel (snowtri_despike_joint_track).

The defaults half_window = 3, tol = 0.1 m come from a synthetic recipe (tests/despike_cases.py::recipe_track: two walkers at
0.03 m per frame, 5 mm of noise, 5 % dropouts, 2 % of the records moved by 0.15-0.6 m, a quarter of them for two frames), not from
footage.  half_window = 1 cannot see a run of two.  On a path faster than about tol / half_window per frame the median of a window
with holes sits off-centre and clean records next to dropouts are flagged (about 1 % at 0.08 m per frame).
"""
from __future__ import annotations

import numpy as np

from . import _lib
from ._lib import (DESPIKE_KEPT, DESPIKE_MARK, DESPIKE_MISSING, DESPIKE_REPLACE, DESPIKE_SPIKE, DESPIKE_UNSUPPORTED)  # noqa: F401
from .records import as_records, missing_records, run_record_pass

MAX_HALF_WINDOW = 4            # half_window: 1 .. 4


def despike_block_frames():
    """Frames per tile of k_despike (snowtri_despike_block_frames): windows around its multiples reach into the next tile."""
    return int(_lib.lib().snowtri_despike_block_frames())


def _check_args(half_window, tol, mode):
    if int(half_window) != half_window or not (1 <= int(half_window) <= MAX_HALF_WINDOW):
        raise ValueError(f"half_window must lie in 1..{MAX_HALF_WINDOW} (got {half_window})")
    tol = float(tol)
    if not tol >= 0.0:
        raise ValueError(f"tol must be >= 0 and not NaN (got {tol})")
    if mode not in (DESPIKE_MARK, DESPIKE_REPLACE):
        raise ValueError(f"mode must be DESPIKE_MARK or DESPIKE_REPLACE (got {mode})")
    return int(half_window), tol, int(mode)


def despike_args(despike):
    """TrackPipeline.run's `despike` argument -> None (off) or (tol, half_window), checked."""
    if despike is None:
        return None
    try:
        tol, half_window = despike
    except (TypeError, ValueError):
        raise ValueError(f"despike must be None (off) or (tol, half_window) (got {despike!r})") from None
    half_window, tol, _ = _check_args(half_window, tol, DESPIKE_MARK)
    return tol, half_window


def despike_joint_track_reference(xyzs, half_window, tol, mode=DESPIKE_MARK):
    """xyzs [T, ..., 4] (float32 / float64; the axes between the first and the last are the lanes) -> (out, codes): out of the same
    shape and dtype, codes uint8 of shape xyzs.shape[:-1].  Pure NumPy."""
    h, tol, mode = _check_args(half_window, tol, mode)
    xyzs, x, T, m = as_records(xyzs)
    out = x.copy()
    codes = np.zeros((T, m), dtype=np.uint8)
    if T == 0 or m == 0:
        return out.reshape(xyzs.shape), codes.reshape(xyzs.shape[:-1])
    v = x.astype(np.float64)
    miss = missing_records(x)
    pad = np.full((T + 2 * h, m, 3), np.inf)                                  # +inf: not measured, or outside the array
    pad[h:h + T] = np.where(miss[..., None], np.inf, v[..., :3])
    win = np.stack([pad[k:k + T] for k in range(2 * h + 1)], axis=0)          # [2h + 1, T, m, 3]: frames t - h .. t + h
    n = np.isfinite(win[..., 0]).sum(axis=0)                                  # [T, m]
    win = np.sort(win, axis=0)                                                # the n measured values first, ascending
    lo = np.maximum(n - 1, 0) // 2
    hi = n // 2
    a = np.take_along_axis(win, lo[None, :, :, None], axis=0)[0]
    b = np.take_along_axis(win, hi[None, :, :, None], axis=0)[0]
    with np.errstate(all="ignore"):
        s = a + b
        med = s * 0.5
        d = v[..., :3] - med
        sq = d * d                                                            # separately rounded: NumPy fuses nothing
        d2 = (sq[..., 0] + sq[..., 1]) + sq[..., 2]
        spike = ~miss & (n >= 3) & (d2 > tol * tol)
        rep = (med + 0.0).astype(x.dtype)
    codes[miss] = DESPIKE_MISSING
    codes[~miss & (n < 3)] = DESPIKE_UNSUPPORTED
    codes[spike] = DESPIKE_SPIKE
    if mode == DESPIKE_MARK:
        out[spike] = 0.0
    else:
        out[..., :3][spike] = rep[spike]
    return out.reshape(xyzs.shape), codes.reshape(xyzs.shape[:-1])


def despike_joint_track(ctx, xyzs, half_window=3, tol=0.1, mode=DESPIKE_MARK, codes=True, stream=None):
    """The pass on the GPU.  ctx: a _lib.Context (None: the rig-less scratch context of the current device).  xyzs [T, ..., 4],
    float32 or float64: a CUDA(=HIP) tensor is used in place, asynchronously on `stream` (default: torch's current stream), and
    tensors come back; anything else is taken as a NumPy array, staged and synchronous.  Returns (out, codes) with codes
    uint8 of shape xyzs.shape[:-1], or None with codes=False (the kernel then does not write them)."""
    return run_record_pass(ctx, xyzs, "snowtri_despike_joint_track", _check_args(half_window, tol, mode), codes, stream,
                           "despike_joint_track")
