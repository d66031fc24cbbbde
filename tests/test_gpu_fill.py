"""Gap filling on the GPU (snowtri_fill_joint_track, snowmocap_amd/csrc/snowtri_fill.hpp) against its NumPy restatement
snowmocap_amd.fill.fill_joint_track_reference: records EQUAL bit for bit, codes equal, around the kernel's tile edges; the
argument checks of the entry point; and TrackPipeline.run(fill_gaps=...) with fixed slots and with tracked persons."""
import ctypes as ct

import numpy as np
import pytest

from test_fill_host import MISSING_KINDS, _bits, random_track

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def api():
    import snowmocap_amd as sm
    from snowmocap_amd import _lib
    assert _lib.lib().snowtri_device_count() > 0, "these tests need the HIP device"
    return sm


def _gpu(x, max_gap, codes=True, device=True, stream=None):
    """fill_joint_track on a NumPy array: through device tensors (asynchronous, then synchronised) or staged from the host."""
    import torch
    from snowmocap_amd.fill import fill_joint_track
    if not device:
        return fill_joint_track(None, x, max_gap, codes=codes)
    out, fl = fill_joint_track(None, torch.from_numpy(x).cuda(), max_gap, codes=codes, stream=stream)
    torch.cuda.synchronize()
    return out.cpu().numpy(), (fl.cpu().numpy() if fl is not None else None)


def _measured(rng, T, dtype):
    r = rng.normal(0.0, 2.0, (T, 4))
    r[:, 3] = rng.uniform(0.1, 1.0, T)
    return r.astype(dtype)


N_PATTERNS = 8


def edge_track(rng, T, m, max_gap, dtype, B, rot=0):
    """random_track (runs of 1 .. max_gap + 2 missing records), and on top of it lanes with ONE forced run each, placed
    against the edge between the first two tiles (frame B); pattern of lane l = (l + rot) % 8; a pattern that does not fit
    into T frames leaves the lane as it was:
      0  run ending at frame B - 1          1  run starting at frame B          2  run over frames B - 1 .. B
      3  run of max_gap records whose measured neighbours lie in different tiles        4  the same with max_gap + 1
      5  nothing measured                   6  a leading and a trailing run     7  (random)"""
    x = random_track(rng, T, m, max_gap, dtype)
    g = min(max_gap, 3)
    s = max(1, B - (max_gap + 1) // 2)
    runs = {0: [(B - g, g)], 1: [(B, g)], 2: [(B - 1, 2)], 3: [(s, max_gap)], 4: [(s, max_gap + 1)], 5: [(0, T)],
            6: [(0, min(max_gap, 2)), (T - min(max_gap, 2), min(max_gap, 2))]}
    for l in range(m):
        pat = (l + rot) % N_PATTERNS
        if pat not in runs:
            continue
        if pat == 5:
            x[:, l] = 0
            x[T // 2, l] = (1.0, np.nan, 2.0, 0.5)
            continue
        if pat == 6:
            fits = T >= 2 * runs[6][0][1] + 1
        else:
            lo, n = runs[pat][0]
            fits = lo >= 1 and lo + n <= T - 1 and (pat not in (3, 4) or lo + n >= B)
        if not fits:
            continue
        x[:, l] = _measured(rng, T, dtype)
        for lo, n in runs[pat]:
            x[lo:lo + n, l] = 0
    return x


def _t_values(B, max_gap):
    return [1, 2, 3, B - 1, B, B + 1, 2 * B + 3, 2 * B + 3 + max_gap + 2]      # the last: room for runs of max_gap + 2 at max_gap = 255


# ---------------------------------------------------------------------------------------------------------------- 1
@pytest.mark.parametrize("dtype", [np.float32, np.float64])
@pytest.mark.parametrize("m,max_gap", [(1, 8), (63, 1), (64, 2), (65, 255), (133, 8), (532, 2), (133, 255)])
def test_equals_the_reference_bit_for_bit(api, dtype, m, max_gap):
    from snowmocap_amd.fill import fill_block_frames, fill_joint_track_reference
    B = fill_block_frames()
    assert B >= 4
    seen = set()
    for T in _t_values(B, max_gap):
        for rot in (range(N_PATTERNS) if m < N_PATTERNS else (0,)):          # a single lane takes every pattern in turn
            rng = np.random.default_rng(100000 * max_gap + 1000 * m + 10 * T + rot)
            x = edge_track(rng, T, m, max_gap, dtype, B, rot)
            ref, ref_codes = fill_joint_track_reference(x, max_gap)
            got, codes = _gpu(x, max_gap)
            assert got.dtype == x.dtype and got.shape == x.shape and codes.dtype == np.uint8 and codes.shape == (T, m)
            bad = np.argwhere(codes != ref_codes)
            assert bad.size == 0, f"T={T} rot={rot}: codes differ first at (frame, lane) {bad[0]}: {codes[tuple(bad[0])]} != {ref_codes[tuple(bad[0])]}"
            bad = np.argwhere(_bits(got) != _bits(ref))
            assert bad.size == 0, f"T={T} rot={rot}: records differ first at (frame, lane, component) {bad[0]}"
            seen |= set(np.unique(ref_codes).tolist())
            if T >= 2 * B + 3 and m >= N_PATTERNS:
                assert set(np.unique(ref_codes).tolist()) == {0, 1, 2, 3}, (T, np.unique(ref_codes))
    assert seen == {0, 1, 2, 3}, seen                                        # the case tested every kind of record


def test_forced_runs_sit_where_the_docstring_says(api):
    """The premise of the test above: with max_gap = 8 the runs against the tile edge are filled or left as intended."""
    from snowmocap_amd.fill import fill_block_frames, fill_joint_track_reference
    B, g = fill_block_frames(), 8
    x = edge_track(np.random.default_rng(5), 2 * B + 3, 8, g, np.float64, B)
    _, c = fill_joint_track_reference(x, g)
    s = B - (g + 1) // 2
    assert (c[B - 3:B, 0] == 1).all() and c[B - 4, 0] == 0 and c[B, 0] == 0
    assert (c[B:B + 3, 1] == 1).all() and c[B - 1, 1] == 0
    assert (c[B - 1:B + 1, 2] == 1).all()
    assert (c[s:s + g, 3] == 1).all() and c[s - 1, 3] == 0 and c[s + g, 3] == 0 and s - 1 < B <= s + g
    assert (c[s:s + g + 1, 4] == 3).all() and c[s - 1, 4] == 0 and c[s + g + 1, 4] == 0
    assert (c[:, 5] == 3).all()
    assert (c[:2, 6] == 2).all() and (c[-2:, 6] == 2).all() and (c[2:-2, 6] == 0).all()


# ---------------------------------------------------------------------------------------------------------------- 2
@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_missing_record_predicates_and_payloads(api, dtype):
    kinds = sorted(MISSING_KINDS)
    m = len(kinds)
    rng = np.random.default_rng(17)
    x = np.stack([_measured(rng, 5, dtype) for _ in range(m)], axis=1)          # [5, m, 4]
    for l, k in enumerate(kinds):
        x[2, l] = MISSING_KINDS[k]
    got, codes = _gpu(x, 1)
    assert (codes[2] == 1).all() and (np.delete(codes, 2, axis=0) == 0).all(), codes      # every kind counts as missing, and is bridged
    want = (x[1].astype(np.float64) + 0.5 * (x[3].astype(np.float64) - x[1].astype(np.float64))).astype(dtype)
    assert np.array_equal(_bits(got[2]), _bits(want))
    # the same kinds in runs of two with max_gap = 1: left alone, byte for byte, and a NaN keeps its payload
    x[3] = x[2]
    raw = _bits(x)
    payload = np.uint32(0x7fc0beef) if dtype == np.float32 else np.uint64(0x7ff80000deadbeef)
    raw[2, 0, 1] = payload
    assert np.isnan(x[2, 0, 1])
    got, codes = _gpu(x, 1)
    assert (codes[2:4] == 3).all() and (codes[:2] == 0).all() and (codes[4] == 0).all()
    assert np.array_equal(_bits(got), _bits(x))
    assert np.argwhere(_bits(got) == payload).tolist() == [[2, 0, 1]]


# ---------------------------------------------------------------------------------------------------------------- 3
@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_properties(api, dtype):
    import torch
    from snowmocap_amd.fill import fill_block_frames, fill_joint_track
    B = fill_block_frames()
    T, m, g = 2 * B + 3, 133, 8
    rng = np.random.default_rng(23)
    x = edge_track(rng, T, m, g, dtype, B)
    got, codes = _gpu(x, g)
    again, codes2 = _gpu(x, g)
    assert np.array_equal(_bits(got), _bits(again)) and np.array_equal(codes, codes2)            # two runs are identical
    no_codes, none = _gpu(x, g, codes=False)
    assert none is None and np.array_equal(_bits(no_codes), _bits(got))                         # fill = NULL: the same out
    perm = rng.permutation(m)
    pg, pc = _gpu(np.ascontiguousarray(x[:, perm]), g)
    assert np.array_equal(_bits(pg), _bits(got[:, perm])) and np.array_equal(pc, codes[:, perm])  # lanes are independent
    hg, hc = _gpu(x, g, device=False)
    assert isinstance(hg, np.ndarray) and np.array_equal(_bits(hg), _bits(got)) and np.array_equal(hc, codes)   # SNOWTRI_HOST
    hg, hc = _gpu(x, g, device=False, codes=False)
    assert hc is None and np.array_equal(_bits(hg), _bits(got))
    side = torch.cuda.Stream()
    xd = torch.from_numpy(x).cuda()
    torch.cuda.synchronize()
    with torch.cuda.stream(side):
        sg, sc = fill_joint_track(None, xd, g)                                                   # torch's current stream: `side`
    eg, ec = fill_joint_track(None, xd, g, stream=side.cuda_stream)                              # ... and given explicitly
    side.synchronize()
    assert side.cuda_stream != 0
    for a, b in ((sg, sc), (eg, ec)):
        assert np.array_equal(_bits(a.cpu().numpy()), _bits(got)) and np.array_equal(b.cpu().numpy(), codes)
    shaped, scodes = _gpu(x[:, :132].reshape(T, 4, 33, 4).copy(), g)                             # [T, P, kn, 4]
    assert shaped.shape == (T, 4, 33, 4) and scodes.shape == (T, 4, 33)
    assert np.array_equal(_bits(shaped).reshape(T, 132, 4), _bits(got[:, :132]))


# ---------------------------------------------------------------------------------------------------------------- 4
def test_bad_arguments_are_refused_on_the_host(api):
    import torch
    from snowmocap_amd import _lib
    from snowmocap_amd.fill import fill_joint_track
    ctx = _lib.scratch_context()
    L, h = ctx.L, ctx.handle
    T, m = 5, 7
    x = np.random.default_rng(1).uniform(0.5, 1.0, (T, m, 4))
    out, fl = np.full((T, m, 4), 9.0), np.full((T, m), 9, dtype=np.uint8)

    def call(T=T, m=m, xp=_lib.ptr(x), dtype=_lib.F64, g=2, op=_lib.ptr(out), memspace=_lib.HOST):
        rc = L.snowtri_fill_joint_track(h, T, m, xp, dtype, g, op, _lib.ptr(fl), memspace, None)
        return rc, L.snowtri_last_error().decode()

    assert call()[0] == _lib.OK and (fl == 0).all() and np.array_equal(out, x)
    x0 = x.copy()
    for kw, word in ((dict(g=0), "max_gap"), (dict(g=256), "max_gap"), (dict(g=-3), "max_gap"), (dict(dtype=2), "dtype"), (dict(dtype=-1), "dtype"),
                     (dict(memspace=2), "memspace"), (dict(T=-1), "T < 0"), (dict(m=-1), "m < 0"), (dict(xp=None), "null"), (dict(op=None), "null"),
                     (dict(op=_lib.ptr(x)), "overlap"), (dict(op=ct.c_void_p(x.ctypes.data + 32)), "overlap"),
                     (dict(op=ct.c_void_p(x.ctypes.data - 32)), "overlap"), (dict(T=1 << 40, m=1 << 30), "2^58"),
                     (dict(T=1 << 45, m=64), "2^31 - 1")):
        out[:], fl[:] = 9.0, 9
        rc, msg = call(**kw)
        assert rc == _lib.ERR_BAD_ARG and msg.startswith("snowtri_fill_joint_track") and word in msg, (kw, rc, msg)
        assert (out == 9.0).all() and (fl == 9).all() and np.array_equal(x, x0), kw
    out[:], fl[:] = 9.0, 9
    assert call(T=0)[0] == _lib.OK and (out == 9.0).all() and (fl == 9).all()                      # T == 0 touches nothing
    assert L.snowtri_fill_joint_track(None, T, m, _lib.ptr(x), _lib.F64, 2, _lib.ptr(out), None, _lib.HOST, None) == _lib.ERR_BAD_ARG
    # device pointers: aligned to 16 bytes, distinct
    buf = torch.zeros(2 * T * m * 4 + 8, dtype=torch.float64, device="cuda")
    buf[:] = 9.0
    base = buf.data_ptr()
    assert base % 16 == 0
    nbytes = T * m * 32

    def dev_call(x_off, o_off):
        rc = L.snowtri_fill_joint_track(h, T, m, ct.c_void_p(base + x_off), _lib.F64, 2, ct.c_void_p(base + o_off), None, _lib.DEVICE, None)
        return rc, L.snowtri_last_error().decode()

    for x_off, o_off, word in ((8, nbytes + 16, "aligned"), (0, nbytes + 8, "aligned"), (0, 0, "overlap"), (0, nbytes - 16, "overlap"),
                               (nbytes - 16, 0, "overlap")):
        rc, msg = dev_call(x_off, o_off)
        assert rc == _lib.ERR_BAD_ARG and word in msg, (x_off, o_off, rc, msg)
    assert dev_call(0, nbytes)[0] == _lib.OK                                                      # back to back is not an overlap
    torch.cuda.synchronize()
    after = buf.cpu().numpy()
    assert (after[:T * m * 4] == 9.0).all() and (after[T * m * 4:2 * T * m * 4] == 9.0).all() and (after[2 * T * m * 4:] == 9.0).all()
    # the Python layer turns them into exceptions
    for bad in (0, 256):
        with pytest.raises(ValueError):
            fill_joint_track(None, x, bad)
    with pytest.raises(TypeError):
        fill_joint_track(None, torch.zeros((3, 2, 4), dtype=torch.float16, device="cuda"), 2)


# ---------------------------------------------------------------------------------------------------------------- 5
def test_bounds_checks_stay_silent_in_the_test_build(api):
    import os
    from snowmocap_amd import _lib
    from snowmocap_amd.fill import fill_block_frames, fill_joint_track_reference
    assert os.path.exists(_lib.TEST_LIB_PATH), "build the test library: make -C snowmocap_amd/csrc debug"
    prev = _lib.use_library(_lib.TEST_LIB_PATH)
    try:
        assert "SNOWTRI_DEBUG_BOUNDS" in _lib.build_info()["variants"]
        ctx = _lib.scratch_context()
        assert ctx.debug_faults()[0] == 0
        B = fill_block_frames()
        for dtype, T, m, g in ((np.float32, 2 * B + 3, 133, 8), (np.float64, B + 1, 65, 2), (np.float64, 4 * B + 9, 70, 255), (np.float32, 1, 1, 1)):
            x = edge_track(np.random.default_rng(T), T, m, g, dtype, B)
            ref, ref_codes = fill_joint_track_reference(x, g)
            got, codes = _gpu(x, g)
            assert np.array_equal(_bits(got), _bits(ref)) and np.array_equal(codes, ref_codes)
        n, first = ctx.debug_faults()
        assert n == 0, f"device-side bounds check failed {n} times; first: code {first >> 32} at line {first & 0xffffffff}"
    finally:
        _lib.use_library(prev)
    assert not _lib.LIB_PATH.endswith("_dbg.so")


# ---------------------------------------------------------------------------------------------------------------- 6
def _same_bytes(a, b):
    a, b = a.cpu().numpy(), b.cpu().numpy()
    return a.dtype == b.dtype and a.shape == b.shape and np.array_equal(np.ascontiguousarray(a).view(np.uint8), np.ascontiguousarray(b).view(np.uint8))


def test_pipeline_with_fixed_slots(api):
    """4 cameras, 1 person, 64 frames; joint 40 is seen by no camera in frames 20-23, joint 77 in frames 0-2."""
    import torch
    from snowmocap_amd import _lib, synth
    from snowmocap_amd.blender import CONTROL_POINT_NAMES
    from snowmocap_amd.fill import fill_joint_track_reference
    wl = synth.config_workload(2, F=64)
    K, R, t = wl["rig"]
    kpts = wl["kpts"].copy()
    low = 0.5 * wl["params"]["keypoint_score_threshold"]
    kpts[20:24, :, 0, 40, 2] = low
    kpts[0:3, :, 0, 77, 2] = low
    smo = {n: [2.0, 0.75, 0.0] for n in CONTROL_POINT_NAMES}
    pipe = api.TrackPipeline(K, R, t, wl["params"], smo, n_persons_out=1)
    plain = pipe.run(kpts, wl["n_persons"])
    off = pipe.run(kpts, wl["n_persons"], fill_gaps=0)
    on = pipe.run(kpts, wl["n_persons"], fill_gaps=8)
    torch.cuda.synchronize()
    assert list(off) == list(plain) and all(_same_bytes(off[k], plain[k]) for k in plain)        # 0: today's dict, key for key, bit for bit
    assert set(on) == set(plain) | {"xyzs_filled", "fill"} and (plain["tracked"] == 1).all()
    assert _same_bytes(on["xyzs"], plain["xyzs"])                                                # xyzs stays the unfilled triangulation
    x = on["xyzs"].cpu().numpy()
    assert (x[20:24, 0, 40] == 0).all() and (x[0:3, 0, 77] == 0).all() and x[19, 0, 40, 3] != 0 and x[3, 0, 77, 3] != 0
    ref, ref_codes = fill_joint_track_reference(x, 8)
    assert (ref_codes[20:24, 0, 40] == 1).all() and (ref_codes[0:3, 0, 77] == 2).all()
    assert on["fill"].dtype == torch.uint8 and np.array_equal(on["fill"].cpu().numpy(), ref_codes)
    assert np.array_equal(_bits(on["xyzs_filled"].cpu().numpy()), _bits(ref))
    # the filters consume the filled records: the same kernel on the same input
    th = wl["params"]
    sm = torch.empty_like(on["xyzs_filled"])
    ctx = pipe.bt.ctx
    _lib.check(ctx.L.snowtri_smooth_joint_track(ctx.handle, 64, 133, ct.c_void_p(on["xyzs_filled"].data_ptr()), float(th["smooth_f"]), float(th["smooth_z"]),
                                                float(th["smooth_r"]), float(th["smooth_delta_time"]), ct.c_void_p(sm.data_ptr()), _lib.DEVICE,
                                                ct.c_void_p(torch.cuda.current_stream().cuda_stream)), "snowtri_smooth_joint_track")
    torch.cuda.synchronize()
    assert _same_bytes(on["smoothed"], sm)
    assert not _same_bytes(on["smoothed"], plain["smoothed"])
    with pytest.raises(ValueError):
        pipe.run(kpts, wl["n_persons"], fill_gaps=256)
    pipe.close()


# ---------------------------------------------------------------------------------------------------------------- 7
def test_pipeline_with_tracked_persons(api):
    """The walker scene of tests/test_gpu_tracking.py (ring rig of 8 cameras, 4 walkers, 96 frames; person 2 invisible in frames
    30-33, person 1 gone from frame 60), with and without the fill, against the same detections without the dropouts."""
    from test_gpu_tracking import WALK, walker_scene
    from snowmocap_amd.blender import CONTROL_POINT_NAMES
    from snowmocap_amd.fill import fill_joint_track_reference
    drop, full = walker_scene(dropouts=True), walker_scene(dropouts=False)
    K, R, t = drop["rig"]
    cpi = int(drop["params"]["center_point_index"])
    smo = {n: [2.0, 0.75, 0.0] for n in CONTROL_POINT_NAMES}
    pipe = api.TrackPipeline(K, R, t, drop["params"], smo, n_persons_out=4)
    r0 = {k: v.cpu().numpy() for k, v in pipe.run(drop["kpts"], drop["n_persons"], ragged="track").items()}
    r8 = {k: v.cpu().numpy() for k, v in pipe.run(drop["kpts"], drop["n_persons"], ragged="track", fill_gaps=8).items()}
    rf = {k: v.cpu().numpy() for k, v in pipe.run(full["kpts"], full["n_persons"], ragged="track").items()}
    pipe.close()

    def slot_of_person(r, p):
        d = np.linalg.norm(r["xyzs"][0, :, cpi, :3] - drop["X"][0, p, cpi][None, :], axis=1)
        assert d.min() < 0.05
        return int(d.argmin())

    assert set(r8) == set(r0) | {"xyzs_filled", "fill", "bridged"}
    s2, s2f = slot_of_person(r8, 2), slot_of_person(rf, 2)
    assert slot_of_person(r0, 2) == s2 and not r0["present"][30:34, s2].any() and r0["present"][:30, s2].all() and r0["present"][34:, s2].all()
    # bridged: present through the dropout under one unchanged id, and marked exactly there
    assert r8["present"][:, s2].all() and (r8["track_id"][:, s2] == r8["track_id"][0, s2]).all() and r8["track_id"][0, s2] >= 0
    want_bridged = np.zeros((WALK["F"], 4), dtype=bool)
    want_bridged[30:34, s2] = True
    assert r8["bridged"].dtype == np.bool_ and np.array_equal(r8["bridged"], want_bridged)
    assert np.array_equal(r8["present"], r8["track_id"] >= 0) and np.array_equal(r8["tracked"], r8["present"].sum(axis=1))
    assert np.array_equal(_bits(r8["xyzs"]), _bits(r0["xyzs"])) and (r8["xyzs"][30:34, s2] == 0).all()      # xyzs stays unfilled
    # the records of the track are the reference applied to its gathered sequence
    idx = np.nonzero(r8["track_id"][:, s2] == r8["track_id"][0, s2])[0]
    ref, ref_codes = fill_joint_track_reference(r8["xyzs"][idx, s2], 8)
    assert (ref_codes[30:34] == 1).all() and np.array_equal(idx, np.arange(WALK["F"]))
    assert np.array_equal(_bits(r8["xyzs_filled"][idx, s2]), _bits(ref)) and np.array_equal(r8["fill"][idx, s2], ref_codes)
    # after the dropout the filtered centre joint is closer to the run that never lost the person
    e8 = np.linalg.norm(r8["smoothed"][34:41, s2, cpi, :3] - rf["smoothed"][34:41, s2f, cpi, :3], axis=1)
    e0 = np.linalg.norm(r0["smoothed"][34:41, s2, cpi, :3] - rf["smoothed"][34:41, s2f, cpi, :3], axis=1)
    print("centre joint of person 2 against the run without the dropout, frames 34-40 (m): filled", e8, "unfilled", e0)
    # Closer in the worst frame AND over the seven frames together.  Not frame by frame: the unfilled filter stood still for four
    # frames and catches up under-damped (z = 0.75), so its error passes through zero on the way to its overshoot, and in that
    # one frame nothing can be strictly closer.  The frame right after the dropout, where it is furthest behind, is checked alone.
    assert e8.max() < e0.max() and e8.sum() < e0.sum() and e8[0] < e0[0]
    # person 1 leaves for good at frame 60: a trailing run of 36 frames is not bridged and nothing is held across it
    s1 = slot_of_person(r8, 1)
    assert r8["present"][:60, s1].all() and not r8["present"][60:, s1].any() and not r8["bridged"][:, s1].any()
    assert (r8["smoothed"][60:, s1] == 0).all() and (r8["xyzs_filled"][60:, s1] == 0).all() and (r8["fill"][60:, s1] == 3).all()
    assert (r8["fill"][:60, s1, cpi] == 0).all()


# ---------------------------------------------------------------------------------------------------------------- 8
def test_pipeline_with_varying_counts_by_list_index(api):
    """ragged="reference" with person counts that vary (the walker scene in person order: 4 persons, 3 in frames 30-33, 3 from
    frame 60): slot i is filled on the gathered frames that carry it.  Joint 40 of everybody is below the keypoint threshold in
    frames 10-12."""
    from test_gpu_tracking import WALK, walker_scene
    from snowmocap_amd.blender import CONTROL_POINT_NAMES
    from snowmocap_amd.fill import fill_joint_track_reference
    sc = walker_scene(dropouts=True, permute=False)
    K, R, t = sc["rig"]
    kpts = sc["kpts"].copy()
    kpts[10:13, :, :, 40, 2] = np.where(kpts[10:13, :, :, 40, 2] > 0, 0.5 * sc["params"]["keypoint_score_threshold"], 0.0)
    smo = {n: [2.0, 0.75, 0.0] for n in CONTROL_POINT_NAMES}
    pipe = api.TrackPipeline(K, R, t, sc["params"], smo, n_persons_out=4)
    r0 = {k: v.cpu().numpy() for k, v in pipe.run(kpts, sc["n_persons"]).items()}
    r8 = {k: v.cpu().numpy() for k, v in pipe.run(kpts, sc["n_persons"], fill_gaps=8).items()}
    pipe.close()
    assert set(r8) == set(r0) | {"xyzs_filled", "fill"} and np.array_equal(_bits(r8["xyzs"]), _bits(r0["xyzs"]))
    trk = r8["tracked"]
    assert np.array_equal(trk, r0["tracked"]) and trk[0] == 4 and (trk[30:34] == 3).all() and (trk[60:] == 3).all()
    for i in range(4):
        idx = np.nonzero(trk > i)[0]
        ref, ref_codes = fill_joint_track_reference(r8["xyzs"][idx, i], 8)
        assert np.array_equal(_bits(r8["xyzs_filled"][idx, i]), _bits(ref)) and np.array_equal(r8["fill"][idx, i], ref_codes), i
        assert (r8["fill"][10:13, i, 40] == 1).all() and (r8["xyzs"][10:13, i, 40] == 0).all()
        rest = np.nonzero(trk <= i)[0]                       # frames that do not carry the slot: the records as they are
        assert np.array_equal(_bits(r8["xyzs_filled"][rest, i]), _bits(r8["xyzs"][rest, i])) and (r8["smoothed"][rest, i] == 0).all()
    assert not np.array_equal(r8["smoothed"][:, :, 40], r0["smoothed"][:, :, 40])
    assert WALK["F"] == trk.shape[0]
