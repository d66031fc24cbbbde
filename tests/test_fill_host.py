"""The gap-filling rule (include/snowtri.h, "Gap filling") in NumPy -- snowmocap_amd/fill.py::fill_joint_track_reference -- against
a deliberately naive per-lane loop and on hand-written tracks, and tracking.bridge_track_ids.  No GPU, no library."""
import numpy as np
import pytest

from snowmocap_amd.fill import (FILL_HOLD, FILL_LERP, FILL_MEASURED, FILL_MISSING, fill_joint_track_reference, missing_records)
from snowmocap_amd.tracking import bridge_track_ids


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint32 if a.dtype == np.float32 else np.uint64)


def naive_fill(xyzs, max_gap):
    """The rule read literally, one lane and one record at a time, in Python floats (IEEE fp64, no fused operations)."""
    T, m, _ = xyzs.shape
    out = xyzs.copy()
    codes = np.zeros((T, m), dtype=np.uint8)
    for l in range(m):
        rec = [[float(v) for v in xyzs[t, l]] for t in range(T)]
        miss = [r[3] == 0.0 or not all(np.isfinite(v) for v in r) for r in rec]
        measured = [t for t in range(T) if not miss[t]]
        for t in range(T):
            if miss[t]:
                codes[t, l] = FILL_MISSING
        for a, b in zip(measured[:-1], measured[1:]):
            g = b - a - 1
            if 1 <= g <= max_gap:
                for k in range(1, g + 1):
                    w = float(k) / float(g + 1)
                    for c in range(4):
                        d = rec[b][c] - rec[a][c]
                        p = w * d
                        out[a + k, l, c] = xyzs.dtype.type(rec[a][c] + p)
                    codes[a + k, l] = FILL_LERP
        if measured:
            b, a = measured[0], measured[-1]
            if 1 <= b <= max_gap:
                out[:b, l] = xyzs[b, l]
                codes[:b, l] = FILL_HOLD
            if 1 <= T - 1 - a <= max_gap:
                out[a + 1:, l] = xyzs[a, l]
                codes[a + 1:, l] = FILL_HOLD
    return out, codes


def random_track(rng, T, m, max_gap, dtype):
    """Measured records with non-zero scores; runs of 1 .. max_gap + 2 missing records of every kind the rule names."""
    x = rng.normal(0.0, 2.0, (T, m, 4))
    x[..., 3] = rng.uniform(0.1, 1.0, (T, m))
    x = x.astype(dtype)
    kinds = [(0.0, 0.0, 0.0, 0.0), (1.0, 2.0, 3.0, -0.0), (1.0, 2.0, 3.0, np.nan), (np.inf, 0.0, 0.0, 0.5), (0.0, np.nan, 0.0, 0.5),
             (0.0, 0.0, -np.inf, 0.5)]
    for l in range(m):
        t = int(rng.integers(0, max_gap + 3))
        while t < T:
            g = int(rng.integers(1, max_gap + 3))
            for u in range(t, min(T, t + g)):
                x[u, l] = kinds[int(rng.integers(len(kinds)))]
            t += g + int(rng.integers(1, 2 * max_gap + 4))
    return x


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
@pytest.mark.parametrize("T,m,max_gap", [(1, 3, 1), (2, 5, 1), (40, 17, 2), (97, 9, 8), (300, 4, 255)])
def test_reference_equals_the_naive_loop(dtype, T, m, max_gap):
    rng = np.random.default_rng(1000 * T + max_gap)
    x = random_track(rng, T, m, max_gap, dtype)
    got, codes = fill_joint_track_reference(x, max_gap)
    want, want_codes = naive_fill(x, max_gap)
    assert got.dtype == x.dtype and got.shape == x.shape and codes.dtype == np.uint8
    assert np.array_equal(codes, want_codes)
    assert np.array_equal(_bits(got), _bits(want))
    # measured records and unfilled missing ones are the input's bits
    keep = (codes == FILL_MEASURED) | (codes == FILL_MISSING)
    assert np.array_equal(_bits(got)[keep], _bits(x)[keep])
    assert np.array_equal(codes != FILL_MEASURED, missing_records(x))
    assert not missing_records(got[(codes == FILL_LERP) | (codes == FILL_HOLD)]).any()


def _lane(scores, dtype=np.float64):
    """One lane whose record t is (t, 10 t, -t, score): measured where score != 0."""
    T = len(scores)
    x = np.zeros((T, 1, 4), dtype=dtype)
    for t, s in enumerate(scores):
        x[t, 0] = (t, 10 * t, -t, s) if s else (0, 0, 0, 0)
    return x


def test_interior_gap_at_and_past_the_limit():
    g = 3
    x = _lane([1] + [0] * g + [1] + [0] * (g + 1) + [1])
    out, codes = fill_joint_track_reference(x, g)
    assert codes[:, 0].tolist() == [0] + [1] * g + [0] + [3] * (g + 1) + [0]
    assert np.array_equal(out[1:g + 1, 0, 0], [1.0, 2.0, 3.0])          # the missing frames' own coordinates come back
    assert np.array_equal(_bits(out[g + 2:2 * g + 3]), _bits(x[g + 2:2 * g + 3]))


def test_leading_and_trailing_runs_at_and_past_the_limit():
    g = 4
    x = _lane([0] * g + [1, 1] + [0] * g)
    out, codes = fill_joint_track_reference(x, g)
    assert codes[:, 0].tolist() == [2] * g + [0, 0] + [2] * g
    assert np.array_equal(out[:g, 0], np.repeat(x[g], g, axis=0)) and np.array_equal(out[g + 2:, 0], np.repeat(x[g + 1], g, axis=0))
    x = _lane([0] * (g + 1) + [1, 1] + [0] * (g + 1))
    out, codes = fill_joint_track_reference(x, g)
    assert codes[:, 0].tolist() == [3] * (g + 1) + [0, 0] + [3] * (g + 1)
    assert np.array_equal(_bits(out), _bits(x))


def test_all_missing_lane_and_single_frame():
    x = _lane([0] * 5)
    x[2, 0] = (1.0, np.nan, 2.0, 0.7)
    out, codes = fill_joint_track_reference(x, 8)
    assert (codes == FILL_MISSING).all() and np.array_equal(_bits(out), _bits(x))
    for s, c in ((1, FILL_MEASURED), (0, FILL_MISSING)):
        x = _lane([s])
        out, codes = fill_joint_track_reference(x, 8)
        assert codes.tolist() == [[c]] and np.array_equal(_bits(out), _bits(x))
    out, codes = fill_joint_track_reference(np.zeros((0, 6, 4), dtype=np.float32), 8)
    assert out.shape == (0, 6, 4) and codes.shape == (0, 6)


MISSING_KINDS = {"negative zero score": (1.0, 2.0, 3.0, -0.0), "NaN score": (1.0, 2.0, 3.0, np.nan), "infinite x": (np.inf, 2.0, 3.0, 0.9),
                 "NaN y": (1.0, np.nan, 3.0, 0.9), "negative infinite z": (1.0, 2.0, -np.inf, 0.9), "infinite score": (1.0, 2.0, 3.0, np.inf)}


@pytest.mark.parametrize("kind", sorted(MISSING_KINDS))
@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_what_counts_as_missing(kind, dtype):
    x = _lane([1, 1, 1], dtype)
    x[1, 0] = MISSING_KINDS[kind]
    assert missing_records(x)[:, 0].tolist() == [False, True, False]
    out, codes = fill_joint_track_reference(x, 1)
    assert codes[:, 0].tolist() == [0, 1, 0]
    assert np.array_equal(out[1, 0], np.asarray([1.0, 10.0, -1.0, 1.0], dtype=dtype))
    x = np.concatenate([x[1:2]] * 3)                     # nothing measured: the record survives with its payload
    out, codes = fill_joint_track_reference(x, 1)
    assert (codes == FILL_MISSING).all() and np.array_equal(_bits(out), _bits(x))


def test_interpolation_weights_are_the_fp64_expressions():
    rng = np.random.default_rng(7)
    A, B = rng.normal(0, 3, 4), rng.normal(0, 3, 4)
    A[3], B[3] = 0.3, 0.9
    x = np.zeros((4, 1, 4))
    x[0, 0], x[3, 0] = A, B
    out, codes = fill_joint_track_reference(x, 2)
    assert codes[:, 0].tolist() == [0, 1, 1, 0]
    for k in (1, 2):
        want = np.array([A[c] + (float(k) / 3.0) * (B[c] - A[c]) for c in range(4)])
        assert np.array_equal(_bits(out[k, 0]), _bits(want))
    out32, _ = fill_joint_track_reference(x.astype(np.float32), 2)       # float32 I/O: fp64 arithmetic on the converted values, one rounding
    A32, B32 = x[0, 0].astype(np.float32).astype(np.float64), x[3, 0].astype(np.float32).astype(np.float64)
    for k in (1, 2):
        want = np.array([A32[c] + (float(k) / 3.0) * (B32[c] - A32[c]) for c in range(4)]).astype(np.float32)
        assert np.array_equal(_bits(out32[k, 0]), _bits(want))


def test_shapes_and_argument_checks():
    x = np.random.default_rng(3).uniform(0.5, 1.0, (6, 2, 5, 4))
    x[2:4, 1, 3] = 0.0
    out, codes = fill_joint_track_reference(x, 2)
    assert out.shape == x.shape and codes.shape == (6, 2, 5)
    assert (codes[2:4, 1, 3] == FILL_LERP).all() and (np.delete(codes.reshape(6, 10), 8, axis=1) == 0).all()
    flat, fcodes = fill_joint_track_reference(x.reshape(6, 10, 4), 2)
    assert np.array_equal(flat.reshape(x.shape), out) and np.array_equal(fcodes.reshape(codes.shape), codes)
    for bad in (0, 256, -1):
        with pytest.raises(ValueError):
            fill_joint_track_reference(x, bad)


def test_bridge_track_ids():
    g = 3
    #            same id over a short run | different ids | a run of g + 1   | leading and trailing runs
    slot0 = [-1, -1, 5, -1, -1, -1, 5, 5, -1, 6, 6, -1, -1, -1, -1, 6, -1, -1]
    slot1 = [7, -1, 7, 7, 7, 7, 7, 7, 7, 7, 7, 7, 7, 7, 7, 7, 7, 7]        # a second slot, bridged on its own
    tid = np.array([slot0, slot1], dtype=np.int32).T
    got = bridge_track_ids(tid, g)
    assert got.dtype == np.int32 and got.shape == tid.shape
    assert got[:, 0].tolist() == [-1, -1, 5, 5, 5, 5, 5, 5, -1, 6, 6, -1, -1, -1, -1, 6, -1, -1]
    assert got[:, 1].tolist() == [7] * 18
    assert tid[3, 0] == -1                                                 # the input is not modified
    assert np.array_equal(bridge_track_ids(tid, g + 1)[11:15, 0], [6, 6, 6, 6])
    assert np.array_equal(bridge_track_ids(np.full((4, 2), -1, dtype=np.int32), 2), np.full((4, 2), -1))
