"""The despike rule (include/snowtri.h, "Despiking") in NumPy -- snowmocap_amd/despike.py::despike_joint_track_reference -- on the
synthetic recipe its defaults come from, against a deliberately naive per-record loop, and on hand-built lanes.  No GPU."""
import os
import re

import numpy as np
import pytest

import despike_cases as dc
from conftest import ROOT
from snowmocap_amd.despike import (DESPIKE_KEPT, DESPIKE_MARK, DESPIKE_MISSING, DESPIKE_REPLACE, DESPIKE_SPIKE, DESPIKE_UNSUPPORTED,
                                   despike_args, despike_joint_track_reference)
from snowmocap_amd.fill import FILL_MISSING, fill_joint_track_reference, missing_records


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint32 if a.dtype == np.float32 else np.uint64)


def naive_despike(xyzs, h, tol, mode):
    """The rule read literally, one record at a time, in Python floats (IEEE fp64, no fused operations)."""
    T, m, _ = xyzs.shape
    out = xyzs.copy()
    codes = np.zeros((T, m), dtype=np.uint8)
    tol2 = float(tol) * float(tol)
    for l in range(m):
        rec = [[float(v) for v in xyzs[t, l]] for t in range(T)]
        miss = [r[3] == 0.0 or not all(np.isfinite(v) for v in r) for r in rec]
        for t in range(T):
            if miss[t]:
                codes[t, l] = DESPIKE_MISSING
                continue
            win = [rec[u] for u in range(max(0, t - h), min(T - 1, t + h) + 1) if not miss[u]]
            n = len(win)
            if n < 3:
                codes[t, l] = DESPIKE_UNSUPPORTED
                continue
            med = []
            for c in range(3):
                v = sorted(r[c] for r in win)
                med.append((v[(n - 1) // 2] + v[n // 2]) * 0.5)
            d = [rec[t][c] - med[c] for c in range(3)]
            d2 = (d[0] * d[0] + d[1] * d[1]) + d[2] * d[2]
            if d2 > tol2:
                codes[t, l] = DESPIKE_SPIKE
                if mode == DESPIKE_MARK:
                    out[t, l] = 0.0
                else:
                    out[t, l, :3] = [xyzs.dtype.type(v + 0.0) for v in med]
    return out, codes


# ---------------------------------------------------------------------------------------------------------------- the recipe
def test_recipe_detection_and_false_positives():
    """Measured when the rule was chosen: 0.9976 and 0.00015."""
    r = dc.recipe_track()
    _, codes = despike_joint_track_reference(r["x"], 3, 0.1)
    spike = codes == DESPIKE_SPIKE
    detected = (spike & r["moved"]).sum() / r["moved"].sum()
    clean = ~r["moved"] & ~r["missing"]
    false_pos = (spike & clean).sum() / clean.sum()
    print(f"recipe: {int(r['moved'].sum())} moved records, detected {detected:.4f}, false positives {false_pos:.5f}")
    assert detected >= 0.99
    assert false_pos <= 0.001
    _, c1 = despike_joint_track_reference(r["x"], 1, 0.1)               # half_window = 1 cannot see runs of two
    assert ((c1 == DESPIKE_SPIKE) & r["moved"]).sum() / r["moved"].sum() < 0.7


def _rms_mm(filled, codes, truth):
    ok = codes != FILL_MISSING
    e = np.linalg.norm(filled[..., :3] - truth, axis=-1)[ok]
    return 1000.0 * float(np.sqrt((e * e).mean()))


def test_recipe_rms_after_the_fill():
    """Measured when the rule was chosen: 8.8 mm with the pass, 62.5 mm without (the noise alone: 8.7 mm)."""
    r = dc.recipe_track()
    marked, _ = despike_joint_track_reference(r["x"], 3, 0.1, DESPIKE_MARK)
    with_pass = _rms_mm(*fill_joint_track_reference(marked, 8), r["truth"])
    without = _rms_mm(*fill_joint_track_reference(r["x"], 8), r["truth"])
    print(f"recipe: RMS against the truth {with_pass:.2f} mm with despike + fill, {without:.2f} mm with the fill alone")
    assert with_pass < 10.0
    assert without > 50.0


# ---------------------------------------------------------------------------------------------------------------- the rule
@pytest.mark.parametrize("dtype", [np.float32, np.float64])
@pytest.mark.parametrize("T,m,h", [(1, 13, 1), (2, 13, 2), (3, 26, 1), (7, 13, 3), (40, 39, 2), (70, 52, 4), (131, 26, 3)])
@pytest.mark.parametrize("mode", [DESPIKE_MARK, DESPIKE_REPLACE])
def test_reference_equals_the_naive_loop(dtype, T, m, h, mode):
    e = dc.edge_track(T, m, dtype, h)
    got, codes = despike_joint_track_reference(e["x"], h, e["tol"], mode)
    want, want_codes = naive_despike(e["x"], h, e["tol"], mode)
    assert got.dtype == e["x"].dtype and got.shape == e["x"].shape and codes.dtype == np.uint8 and codes.shape == (T, m)
    assert np.array_equal(codes, want_codes)
    assert np.array_equal(_bits(got), _bits(want))


def test_edge_track_holds_what_its_docstring_says():
    B, h = dc.block_frames(), 3
    T = 2 * B + h
    e = dc.edge_track(T, 2 * dc.N_PATTERNS, np.float64, h)
    x = e["x"]
    _, c = despike_joint_track_reference(x, h, e["tol"])
    P = dc.N_PATTERNS
    assert c[0, 0] == DESPIKE_SPIKE and c[T - 1, 0] == DESPIKE_SPIKE and c[1, 0] == DESPIKE_KEPT          # single spikes at the ends
    assert (c[0:2, P] == DESPIKE_SPIKE).all() and (c[T - 2:, P] == DESPIKE_SPIKE).all()                    # runs of two at the ends
    assert c[1, 1] == DESPIKE_SPIKE and c[T - 2, 1] == DESPIKE_SPIKE
    for pat, off in ((2, -1), (3, 0), (4, 1)):
        assert c[B + off, pat] == DESPIKE_SPIKE and c[2 * B + off, pat] == DESPIKE_SPIKE, pat
        assert (c[B + off:B + off + 2, P + pat] == DESPIKE_SPIKE).all()
    assert c[h + 1, 5] == DESPIKE_UNSUPPORTED and c[4 * h + 3, 5] == DESPIKE_SPIKE and c[7 * h + 5, 5] == DESPIKE_SPIKE   # n = 2, 3, 4
    assert (c[2::5, 6][[0, 1, 2, 3]] == DESPIKE_MISSING).all() and c[22, 6] == DESPIKE_SPIKE
    assert np.isnan(x[2, 6, 1]) and _bits(x)[2, 6, 1] == 0x7ff80000deadbeef and np.signbit(x[17, 6, 3]) and x[17, 6, 3] == 0
    assert (c[:, 7] == DESPIKE_MISSING).all()
    assert sorted(np.unique(c[:, 8]).tolist()) == [DESPIKE_MISSING, DESPIKE_UNSUPPORTED] and (c[:, 8] == DESPIKE_UNSUPPORTED).sum() == 2
    assert (c[:, 9] == DESPIKE_KEPT).all() and (c[:, 10] == DESPIKE_SPIKE).sum() == 1
    rep, _ = despike_joint_track_reference(x, h, e["tol"], DESPIKE_REPLACE)
    at = np.nonzero(c[:, 11] == DESPIKE_SPIKE)[0]
    assert at.size >= 2 and (rep[at, 11, 0] == 0).all() and not np.signbit(rep[at, 11, 0]).any()            # a zero median is +0.0
    assert set(np.unique(c).tolist()) == {0, 1, 2, 3}


def test_the_exact_tie_is_kept():
    e = dc.edge_track(40, dc.N_PATTERNS, np.float64, 3)
    x = e["x"]
    t = int(np.nonzero(x[:, 9, 0] == 13.0)[0][0])
    assert e["tol"] == 5.0 and x[t, 9, :3].tolist() == [13.0, 24.0, 30.0] and x[t, 10, :3].tolist() == [13.0, 24.0, 31.0]
    _, c = despike_joint_track_reference(x, 3, 5.0)
    assert c[t, 9] == DESPIKE_KEPT and c[t, 10] == DESPIKE_SPIKE                    # d2 == tol^2 is not a spike, d2 = 26 is
    _, c = despike_joint_track_reference(x, 3, np.nextafter(5.0, 0.0))
    assert c[t, 9] == DESPIKE_SPIKE and c[t, 10] == DESPIKE_SPIKE


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_an_infinite_tolerance_flags_nothing(dtype):
    x = dc.edge_track(70, 2 * dc.N_PATTERNS, dtype, 2)["x"]
    for mode in (DESPIKE_MARK, DESPIKE_REPLACE):
        out, c = despike_joint_track_reference(x, 2, np.inf, mode)
        assert not (c == DESPIKE_SPIKE).any() and np.array_equal(_bits(out), _bits(x))
    huge = x.copy()                                                    # d2 overflows: +inf > +inf is false, and a NaN d2 is no spike
    huge[:, 0, :3] = np.finfo(dtype).max
    huge[5, 0, :3] = -np.finfo(dtype).max
    out, c = despike_joint_track_reference(huge, 2, np.inf)
    assert not (c == DESPIKE_SPIKE).any() and np.array_equal(_bits(out), _bits(huge))


@pytest.mark.parametrize("h", [1, 2, 3, 4])
def test_codes_partition_the_records(h):
    e = dc.edge_track(131, 3 * dc.N_PATTERNS, np.float64, h)
    x = e["x"]
    out, c = despike_joint_track_reference(x, h, e["tol"])
    miss = missing_records(x)
    T = x.shape[0]
    n = np.zeros(miss.shape, dtype=np.int64)
    for t in range(T):
        n[t] = (~miss[max(0, t - h):t + h + 1]).sum(axis=0)
    assert np.array_equal(c == DESPIKE_MISSING, miss)
    assert np.array_equal(c == DESPIKE_UNSUPPORTED, ~miss & (n < 3))
    assert np.array_equal((c == DESPIKE_KEPT) | (c == DESPIKE_SPIKE), ~miss & (n >= 3))
    keep = c != DESPIKE_SPIKE
    assert np.array_equal(_bits(out)[keep], _bits(x)[keep])             # everything but a spike: the input's bits, payloads included
    assert (_bits(out)[c == DESPIKE_SPIKE] == 0).all()                  # MARK: four +0.0


def test_lanes_are_independent():
    e = dc.edge_track(70, 3 * dc.N_PATTERNS, np.float32, 3)
    x = e["x"]
    out, c = despike_joint_track_reference(x, 3, e["tol"], DESPIKE_REPLACE)
    perm = np.random.default_rng(3).permutation(x.shape[1])
    po, pc = despike_joint_track_reference(x[:, perm], 3, e["tol"], DESPIKE_REPLACE)
    assert np.array_equal(_bits(po), _bits(out[:, perm])) and np.array_equal(pc, c[:, perm])
    some = [0, 5, 9, 17, 30]
    so, sc = despike_joint_track_reference(x[:, some], 3, e["tol"], DESPIKE_REPLACE)
    assert np.array_equal(_bits(so), _bits(out[:, some])) and np.array_equal(sc, c[:, some])


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_replace_differs_from_mark_only_on_spikes(dtype):
    e = dc.edge_track(131, 2 * dc.N_PATTERNS, dtype, 3)
    x = e["x"]
    mo, mc = despike_joint_track_reference(x, 3, e["tol"], DESPIKE_MARK)
    ro, rc = despike_joint_track_reference(x, 3, e["tol"], DESPIKE_REPLACE)
    assert np.array_equal(mc, rc) and (mc == DESPIKE_SPIKE).sum() > 20
    differ = (_bits(mo) != _bits(ro)).any(axis=-1)
    assert not (differ & (mc != DESPIKE_SPIKE)).any()
    s = mc == DESPIKE_SPIKE
    assert np.array_equal(_bits(ro)[s][:, 3], _bits(x)[s][:, 3])        # the record's own score bits
    assert not missing_records(ro[s]).any() and missing_records(mo[s]).all()
    assert (np.linalg.norm(ro[s][:, :3].astype(np.float64) - x[s][:, :3].astype(np.float64), axis=1) > e["tol"]).all()


def test_shapes_and_argument_checks():
    x = dc.recipe_track()["x"][:50, :20].reshape(50, 4, 5, 4)
    out, c = despike_joint_track_reference(x, 3, 0.1)
    assert out.shape == x.shape and c.shape == (50, 4, 5)
    flat, fc = despike_joint_track_reference(x.reshape(50, 20, 4), 3, 0.1)
    assert np.array_equal(flat.reshape(x.shape), out) and np.array_equal(fc.reshape(c.shape), c)
    out, c = despike_joint_track_reference(np.zeros((0, 6, 4), dtype=np.float32), 3, 0.1)
    assert out.shape == (0, 6, 4) and c.shape == (0, 6)
    for kw in (dict(half_window=0), dict(half_window=5), dict(half_window=1.5), dict(tol=-1e-9), dict(tol=np.nan), dict(mode=2), dict(mode=-1)):
        args = dict(half_window=3, tol=0.1, mode=DESPIKE_MARK)
        args.update(kw)
        with pytest.raises(ValueError):
            despike_joint_track_reference(x, **args)
    with pytest.raises(ValueError):
        despike_joint_track_reference(np.zeros((5, 3)), 3, 0.1)


def test_track_pipeline_checks_its_despike_argument():
    """What TrackPipeline.run does with `despike` before it touches the device."""
    assert despike_args(None) is None
    assert despike_args((0.1, 3)) == (0.1, 3) and despike_args([0.25, 1]) == (0.25, 1) and despike_args((np.inf, 4)) == (np.inf, 4)
    for bad in ((0.1,), (0.1, 3, 1), 0.1, "ab", (0.1, 0), (0.1, 5), (-0.1, 3), (np.nan, 3), (0.1, 2.5)):
        with pytest.raises(ValueError):
            despike_args(bad)
    import inspect
    from snowmocap_amd.pipeline import ShardedTrackPipeline, TrackPipeline
    assert inspect.signature(TrackPipeline.run).parameters["despike"].default is None
    assert "despike" not in inspect.signature(ShardedTrackPipeline.run).parameters and "despike" in ShardedTrackPipeline.__doc__


# ---------------------------------------------------------------------------------------------------------------- the networks
def _networks():
    """{W: [(i, j), ...]} read from the kernel's source: the compare-exchange sequences of despike_sort<W>"""
    src = open(os.path.join(ROOT, "snowmocap_amd", "csrc", "snowtri_despike.hpp")).read()
    nets = {}
    for W, body in re.findall(r"despike_sort<(\d)>\(double \(&v\)\[\d\]\) \{(.*?)\n\}", src, flags=re.S):
        nets[int(W)] = [(int(i), int(j)) for i, j in re.findall(r"CX\((\d), (\d)\)", body)]
    return nets


def test_the_kernels_networks_sort():
    """Zero-one principle: a network that sorts every 0/1 input sorts every input."""
    nets = _networks()
    assert sorted(nets) == [3, 5, 7, 9] and [len(nets[W]) for W in (3, 5, 7, 9)] == [3, 9, 16, 25]
    for W, net in nets.items():
        v = ((np.arange(1 << W)[:, None] >> np.arange(W)[None, :]) & 1).astype(np.int8)
        for i, j in net:
            assert 0 <= i < j < W
            lo, hi = np.minimum(v[:, i], v[:, j]), np.maximum(v[:, i], v[:, j])
            v[:, i], v[:, j] = lo, hi
        assert (np.diff(v, axis=1) >= 0).all(), W
