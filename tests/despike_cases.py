"""Inputs shared by tests/test_despike_host.py and tests/test_gpu_despike.py: the synthetic recipe the defaults of the despike
pass come from, and small tracks with spikes aimed at the ends of the array, the tile edges of the kernel and runs of missing
records (built once per process, never modified)."""
import functools

import numpy as np

from snowmocap_amd import synth

EDGE_TOL = 5.0           # edge_track is built in units in which the exact-tie lane has integer coordinates
N_PATTERNS = 13


def _freeze(d):
    for v in d.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return d


def block_frames():
    """snowtri_despike_block_frames() where the library is there, else the value the kernel is built with today (the host tests
    need only SOME tile length to aim at)."""
    try:
        from snowmocap_amd.despike import despike_block_frames
        return despike_block_frames()
    except (ImportError, OSError, AttributeError):
        return 64


@functools.lru_cache(maxsize=None)
def recipe_track():
    """default_rng(7), synth.make_walkers with 600 frames, 2 persons, step = 0.03; 5 mm of Gaussian noise per coordinate, scores
    U(3.5, 8); 5 % of the records missing; 2 % of the records moved 0.15-0.6 m in a random direction (direction and amplitude drawn
    per record), a quarter of them followed by a second frame with the same offset.  x [T, m, 4] float64, truth [T, m, 3], moved
    and missing [T, m] bool."""
    rng = np.random.default_rng(7)
    T, P = 600, 2
    X, _ = synth.make_walkers(rng, T, P, step=0.03, J=133)
    x = np.concatenate([X + rng.normal(0, 0.005, X.shape), rng.uniform(3.5, 8, X.shape[:3] + (1,))], -1).reshape(T, P * 133, 4)
    m = x.shape[1]
    missing = rng.random((T, m)) < 0.05
    first = (rng.random((T, m)) < 0.02) & ~missing
    second = np.zeros_like(first)
    second[1:] = first[:-1] & (rng.random((T - 1, m)) < 0.25)
    second &= ~missing
    dirs = rng.normal(size=(T, m, 3))
    dirs /= np.linalg.norm(dirs, axis=-1, keepdims=True)
    off = dirs * rng.uniform(0.15, 0.6, (T, m, 1))
    off[1:][second[1:]] = off[:-1][second[1:]]          # the second frame of a run copies the offset of the first
    moved = first | second
    x[..., :3] += np.where(moved[..., None], off, 0)
    x[missing] = 0
    return _freeze(dict(x=x, truth=X.reshape(T, m, 3).copy(), moved=moved, missing=missing))


def _spike(x, t, l, k):
    """record (t, l) moved by more than 2 tol, in a direction and by an amount that depend on k"""
    if 0 <= t < x.shape[0]:
        x[t, l, :3] += np.array([(-1.0) ** k * (11.0 + 3 * (k % 5)), 7.0 * ((k % 3) - 1), 13.0 + (k % 4)])


def _run(x, t, l, r, k):
    for u in range(t, t + r):          # a run shares its offset
        _spike(x, u, l, k)


@functools.lru_cache(maxsize=None)
def edge_track(T, m, dtype, h, rot=0):
    """A smooth track (a quarter of a unit per frame against tol = EDGE_TOL = 5, a little deterministic jitter) with, on lane l,
    pattern (l + rot) % N_PATTERNS; r = 1 + (l // N_PATTERNS) % h is the lane's run length (single spikes and runs of 2..h), B the
    kernel's tile length:
       0  runs at frame 0 and ending at frame T - 1         1  runs at frame 1 and ending at frame T - 2
       2  a run starting at k B - 1 for every tile edge     3  ... at k B                 4  ... at k B + 1
       5  spikes inside runs of missing records that leave n = 2, 3 and 4 measured records in the window, and one next to a run
       6  missing records of every kind: NaN with a payload, +inf, -inf, score -0.0; spikes between them
       7  nothing measured (one record a NaN)               8  only two measured records
       9  the exact tie: integer coordinates, one record at (3, 4, 0) from its neighbours, d2 == tol^2
      10  its twin at (3, 4, 1)                             11  x alternates between +0.0 and -0.0: the median is a zero of either sign
      12  spikes every 2 h + 3 frames, runs of r
    Returns {"x": [T, m, 4] of dtype, "tol": EDGE_TOL}."""
    dtype = np.dtype(dtype)
    B = block_frames()
    rng = np.random.default_rng(1000003 * T + 1009 * m + 10 * h + rot)
    t = np.arange(T, dtype=np.float64)[:, None]
    l = np.arange(m, dtype=np.float64)[None, :]
    x = np.empty((T, m, 4))
    x[..., 0] = 0.25 * t + 3.0 * l
    x[..., 1] = 4.0 * np.sin(0.05 * t + l)
    x[..., 2] = 100.0 + 0.5 * l - 0.125 * t
    x[..., :3] += rng.uniform(-0.2, 0.2, (T, m, 3))
    x[..., 3] = 0.5 + 0.001 * ((7 * t + 3 * l) % 100)
    bits = np.zeros((T, m), dtype=bool)                   # records whose bits are set below, after the cast
    for lane in range(m):
        pat = (lane + rot) % N_PATTERNS
        r = 1 + (lane // N_PATTERNS) % h
        k = lane
        if pat == 0:
            _run(x, 0, lane, r, k)
            _run(x, T - r, lane, r, k + 1)
        elif pat == 1:
            _run(x, 1, lane, r, k)
            _run(x, T - 1 - r, lane, r, k + 1)
        elif pat in (2, 3, 4):
            for e in range(B, T + B, B):
                _run(x, e + (pat - 3), lane, r, k + e // B)
        elif pat == 5:
            c = h + 1
            for n in (2, 3, 4):                               # the window of frame c keeps n measured records, c among them
                if c + h >= T or n > 2 * h + 1:
                    break
                keep = [c] + [u for u in range(c - h, c + h + 1) if u != c][::2][:n - 1]
                for u in range(c - h, c + h + 1):
                    if u not in keep:
                        x[u, lane] = 0.0
                _spike(x, c, lane, k + n)
                c += 3 * h + 2
            if c + 3 < T:                                     # a spike directly behind a run of missing records
                x[c:c + 2, lane] = 0.0
                _spike(x, c + 2, lane, k)
        elif pat == 6:
            for j, u in enumerate(range(2, T, 5)):
                kind = j % 5
                if kind == 0:
                    x[u, lane, 1] = np.nan
                    bits[u, lane] = True
                elif kind == 1:
                    x[u, lane, 0] = np.inf
                elif kind == 2:
                    x[u, lane, 2] = -np.inf
                elif kind == 3:
                    x[u, lane, 3] = -0.0
                else:
                    _spike(x, u, lane, k + j)
        elif pat == 7:
            x[:, lane] = 0.0
            x[T // 2, lane] = (1.0, np.nan, 2.0, 0.5)
        elif pat == 8:
            keep = x[[0, min(T - 1, h)], lane].copy()
            x[:, lane] = 0.0
            x[[0, min(T - 1, h)], lane] = keep
        elif pat in (9, 10):
            x[:, lane, :3] = (10.0, 20.0, 30.0)
            x[min(T - 1, max(h, T // 2)), lane, :3] = (13.0, 24.0, 30.0 if pat == 9 else 31.0)
        elif pat == 11:
            x[:, lane, 0] = np.where(np.arange(T) % 2 == 0, 0.0, -0.0)
            for u in range(h + 1, T, 2 * h + 4):
                _spike(x, u, lane, k + u)
        else:
            for j, u in enumerate(range(h, T, 2 * h + 3)):
                _run(x, u, lane, min(r, T - u), k + j)
    x = x.astype(dtype)
    raw = x.view(np.uint32 if dtype == np.float32 else np.uint64)
    payload = np.uint32(0x7fc0beef) if dtype == np.float32 else np.uint64(0x7ff80000deadbeef)
    raw[..., 1][bits] = payload                               # a NaN with a payload, which has to survive the copy
    return _freeze(dict(x=x, tol=EDGE_TOL))
