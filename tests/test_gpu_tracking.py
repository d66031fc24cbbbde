"""Cross-frame person tracking on the GPU (snowtri_track_persons / snowtri_track_gather, snowmocap_amd/csrc/snowtri_track.hpp)
against its NumPy restatement snowmocap_amd.tracking.track_persons_reference: every integer output must be EQUAL, on the
GPU's own triangulated persons (a walker scene whose per-camera lists come in random order) and on synthetic person
lists that keep all 16 x 16 (slot, person) pairs busy around the chain kernel's staging-block sizes."""
import ctypes as ct

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

WALK = dict(F=96, P=4, step=0.03, seed=11, pout=8, S=6, gate=0.3)


@pytest.fixture(scope="module")
def api():
    import snowmocap_amd as sm
    from snowmocap_amd import _lib
    assert _lib.lib().snowtri_device_count() > 0, "these tests need the HIP device"
    return sm


def walker_scene(dropouts=True, permute=True):
    """ring_rig(8), 4 walkers on a 1.5 m circle, 0.03 m per frame, pixel sigma 1.0, 96 frames; thresholds of BASELINE configs[2]
    plus condense_person_num_tol = 10 (no ghost clusters: count[f] = visible persons).  With `dropouts` person 2 is invisible
    in frames 30-33 and person 1 is gone from frame 60."""
    from snowmocap_amd import synth
    rng = np.random.default_rng(WALK["seed"])
    K, R, t = synth.ring_rig(8)
    X, _ = synth.make_walkers(rng, WALK["F"], WALK["P"], WALK["step"])
    vis = np.ones((WALK["F"], WALK["P"]), dtype=bool)
    if dropouts:
        vis[30:34, 2] = False
        vis[60:, 1] = False
    kpts, npers = synth.make_keypoints_visible(rng, K, R, t, X, vis, pixel_sigma=1.0, permute_persons=permute)
    prm = dict(synth.default_thresholds(), average_score_threshold=1.0, condense_distance_tol=0.3, condense_person_num_tol=10)
    return dict(rig=(K, R, t), X=X, vis=vis, kpts=kpts, n_persons=npers, params=prm)


@pytest.fixture(scope="module")
def walkers(api):
    """The walker scene triangulated on the GPU, float32 and float64 outputs (device tensors + host copies)."""
    import torch
    from snowmocap_amd.batch import BatchTriangulator
    sc = walker_scene()
    K, R, t = sc["rig"]
    keys = ("keypoint_score_threshold", "average_score_threshold", "distance_threshold", "condense_distance_tol",
            "condense_person_num_tol", "condense_score_tol", "center_point_index", "keypoint_num")
    kp, npers = torch.from_numpy(sc["kpts"]).cuda(), torch.from_numpy(sc["n_persons"]).cuda()
    for dt in (np.float32, np.float64):
        bt = BatchTriangulator(K, R, t, {k: sc["params"][k] for k in keys}, pout_max=WALK["pout"], out_dtype=dt)
        out = bt.run_torch(kp, npers)
        torch.cuda.synchronize()
        sc[np.dtype(dt).name] = dict(xyzs=out["xyzs"], count=out["count"], xyzs_h=out["xyzs"].cpu().numpy(), count_h=out["count"].cpu().numpy())
        bt.close()
    return sc


def _host(out):
    return {k: v.cpu().numpy() for k, v in out.items()}


def _assert_same(got, ref, what=""):
    for k, name in enumerate(("slot_of", "person_of", "track_id", "flags")):
        g = got[name].astype(np.int64)
        assert g.shape == ref[k].shape and np.array_equal(g, ref[k].astype(np.int64)), \
            f"{what}{name}: first difference at frame {int(np.argwhere(g != ref[k])[0][0]) if g.shape == ref[k].shape else -1}"


def _assert_state(blob, st, S):
    from snowmocap_amd import tracking
    got = tracking.state_from_blob(blob, S)
    live = st["live"]
    assert got["next_id"] == st["next_id"] and np.array_equal(got["live"], live)
    for key in ("pos", "missed", "id"):               # the content of a free slot is unspecified
        assert np.array_equal(got[key][live], st[key][live]), key


# ---------------------------------------------------------------------------------------------------------------- 1
@pytest.mark.parametrize("dtype", ["float32", "float64"])
@pytest.mark.parametrize("max_missed,n_ids", [(8, 4), (2, 5)])
def test_walker_scene_keeps_one_identity_per_person(api, walkers, dtype, max_missed, n_ids):
    from snowmocap_amd.tracking import PersonTracker, track_persons_reference
    w = walkers[dtype]
    xyzs, count = w["xyzs_h"], w["count_h"]
    assert np.array_equal(count, walkers["vis"].sum(axis=1))             # no ghosts, nobody lost: count = visible persons
    trk = PersonTracker(None, S=WALK["S"], center_point_index=0, gate=WALK["gate"], max_missed=max_missed)
    got = _host(trk.run_torch(w["xyzs"], w["count"], gather=False))
    ref = track_persons_reference(xyzs, count, WALK["S"], 0, WALK["gate"], max_missed)
    _assert_same(got, ref)
    _assert_state(trk.state_blob(), ref[4], WALK["S"])
    # the premise: the condensed list order differs from frame 0's in most frames
    true_c = walkers["X"][:, :, 0, :]                                    # the centre joint is joint 0
    who = np.full((WALK["F"], WALK["pout"]), -1)
    for f in range(WALK["F"]):
        for p in range(int(count[f])):
            d = np.linalg.norm(true_c[f] - xyzs[f, p, 0, :3].astype(np.float64), axis=1)
            assert d.min() < 0.05
            who[f, p] = int(np.argmin(d))
    n_other_order = sum(1 for f in range(WALK["F"]) if not np.array_equal(who[f, :int(count[f])], who[0, :int(count[f])]))
    print(f"list order differs from frame 0 in {n_other_order} of {WALK['F']} frames")
    assert n_other_order > WALK["F"] // 2
    # every track id is exactly one true person
    owner = {}
    for f in range(WALK["F"]):
        for s in range(WALK["S"]):
            if got["track_id"][f, s] >= 0:
                owner.setdefault(int(got["track_id"][f, s]), set()).add(int(who[f, got["person_of"][f, s]]))
    assert all(len(v) == 1 for v in owner.values()), owner
    assert len(owner) == n_ids and sorted(owner) == list(range(n_ids))
    assert not got["flags"].any()
    if max_missed == 8:
        assert sorted(next(iter(v)) for v in owner.values()) == [0, 1, 2, 3]       # person 2 is the same track after its dropout
    else:
        slots2 = {int(np.argwhere(got["track_id"] == i)[0][1]) for i, v in owner.items() if v == {2}}
        assert len(slots2) == 1 and sum(1 for v in owner.values() if v == {2}) == 2          # a new id, in the re-used slot
    trk.close()


# ---------------------------------------------------------------------------------------------------------------- 2
def synthetic_lists(kn, F, dtype, integer=False, seed=3):
    """Person lists that keep a 16 x 16 tracker busy: 20 entities, ~18 visible per frame (so count[f] is often ABOVE Pout_max
    = 16 and births overflow), listed in random order, drifting (jitter 0.04 m on a 1 m lattice) or -- `integer` -- redrawn on a
    small integer grid every frame, which makes ties and d2 == gate^2 (gate 5: (3, 4, 0), (5, 0, 0)) the rule.  A few centres
    carry score 0 or a non-finite coordinate."""
    rng = np.random.default_rng(seed)
    P, E = 16, 20
    cpi = kn // 2
    xyzs = rng.normal(50.0, 1.0, size=(F, P, kn, 4)).astype(dtype)       # the other joints: never read
    count = np.zeros(F, dtype=np.int32)
    base = np.stack(np.meshgrid(np.arange(5), np.arange(4), [0.0], indexing="ij"), axis=-1).reshape(E, 3).astype(np.float64)
    pos = base.copy()
    for f in range(F):
        if integer:
            pos = 5.0 * rng.integers(0, 3, size=(E, 3)) + rng.choice([0.0, 3.0, 4.0], size=(E, 3))
        else:
            pos = pos + rng.normal(0.0, 0.04, size=pos.shape)
        seen = rng.permutation(np.nonzero(rng.random(E) < 0.9)[0])
        count[f] = len(seen) if f % 5 else min(len(seen), int(rng.integers(0, 17)))
        for p, e in enumerate(seen[:min(P, int(count[f]))]):
            xyzs[f, p, cpi, :3] = pos[e]
            xyzs[f, p, cpi, 3] = rng.uniform(0.5, 9.0)
            r = rng.random()
            if r < 0.01:
                xyzs[f, p, cpi, 3] = 0.0
            elif r < 0.02:
                xyzs[f, p, cpi, int(rng.integers(0, 3))] = [np.nan, np.inf, -np.inf][int(rng.integers(0, 3))]
    return xyzs, count, cpi


def _frames_with_all_pairs(xyzs, count, cpi, gate, mm):
    from snowmocap_amd.tracking import track_persons_reference
    st, n = None, 0
    for f in range(len(count)):
        c = xyzs[f, :min(16, int(count[f])), cpi].astype(np.float64)
        n_valid = int(((c[:, 3] != 0) & np.isfinite(c[:, :3]).all(axis=1)).sum())
        n += int(st is not None and int(st["live"].sum()) == 16 and n_valid == 16)
        st = track_persons_reference(xyzs[f:f + 1], count[f:f + 1], 16, cpi, gate, mm, state=st)[4]
    return n


def _block_sizes():
    from snowmocap_amd import tracking
    B = tracking.chain_block_frames()
    return B, [1, 2, B - 1, B, B + 1, 2 * B + 3]


def _run_synthetic(kn, check_busy=True):
    import torch
    from snowmocap_amd.tracking import PersonTracker, track_persons_reference
    B, sizes = _block_sizes()
    for integer, gate, mm in ((False, 0.3, 2), (True, 5.0, 1)):
        for dtype in (np.float32, np.float64):
            xyzs, count, cpi = synthetic_lists(kn, max(sizes), dtype, integer=integer)
            xd, cd = torch.from_numpy(xyzs).cuda(), torch.from_numpy(count).cuda()
            for F in sizes:
                trk = PersonTracker(None, S=16, center_point_index=cpi, gate=gate, max_missed=mm)
                got = _host(trk.run_torch(xd[:F].contiguous(), cd[:F].contiguous(), gather=False))
                ref = track_persons_reference(xyzs[:F], count[:F], 16, cpi, gate, mm)
                _assert_same(got, ref, f"kn={kn} F={F} {np.dtype(dtype).name} integer={integer}: ")
                _assert_state(trk.state_blob(), ref[4], 16)
            if check_busy:                                   # the data do what they are meant to (whole range, reference)
                assert (ref[3] & 1).any() and (count > 16).any() and len(np.unique(ref[2][ref[2] >= 0])) > 20      # overflow, deaths, births
                if not integer:                                # 16 live slots x 16 valid persons = all 256 pairs, in a third of the frames
                    assert _frames_with_all_pairs(xyzs, count, cpi, gate, mm) > len(count) // 3


@pytest.mark.parametrize("kn", [1, 30, 133])
def test_synthetic_lists_around_the_staging_block(api, kn):
    _run_synthetic(kn)


def test_integer_grid_has_ties_and_exact_gate_hits():
    """(the premise of the integer data set, on the reference alone: equal smallest distances and d2 == gate^2 both occur)"""
    from snowmocap_amd.tracking import state_from_blob, track_persons_reference      # noqa: F401
    xyzs, count, cpi = synthetic_lists(1, 40, np.float64, integer=True)
    ties = hits = 0
    st = None
    for f in range(40):
        prev = st
        out = track_persons_reference(xyzs[f:f + 1], count[f:f + 1], 16, cpi, 5.0, 1, state=st)
        st = out[4]
        if prev is None or not prev["live"].any():
            continue
        c = xyzs[f, :min(16, int(count[f])), cpi]
        ok = (c[:, 3] != 0) & np.isfinite(c[:, :3]).all(axis=1)
        d = c[ok][None, :, :3] - prev["pos"][prev["live"]][:, None, :]
        d2 = (d ** 2).sum(axis=-1)
        if not d2.size:
            continue
        hits += int((d2 == 25.0).sum())
        ties += int((d2 == d2.min()).sum() > 1)
    assert ties > 5 and hits > 20, (ties, hits)


# ---------------------------------------------------------------------------------------------------------------- 3
def test_state_carries_identities_across_calls(api, walkers):
    from snowmocap_amd.tracking import PersonTracker
    B, _ = _block_sizes()
    w = walkers["float32"]
    F = WALK["F"]
    a, b = 32, 2 * B                                       # a: inside person 2's dropout (frames 30-33); b: a staging-block edge
    assert 30 < a < 34 and a < b < F and b % B == 0
    kw = dict(S=WALK["S"], center_point_index=0, gate=WALK["gate"], max_missed=8)
    one = PersonTracker(None, **kw)
    whole = _host(one.run_torch(w["xyzs"], w["count"]))
    three = PersonTracker(None, **kw)
    parts = [_host(three.run_torch(w["xyzs"][lo:hi].contiguous(), w["count"][lo:hi].contiguous())) for lo, hi in ((0, a), (a, b), (b, F))]
    for key in whole:
        assert np.array_equal(np.concatenate([p[key] for p in parts]).view(np.uint8), whole[key].view(np.uint8)), key
    assert np.array_equal(one.state_blob(), three.state_blob())
    # an empty block leaves the state alone
    before = three.state_blob()
    empty = three.run_torch(w["xyzs"][:0].contiguous(), w["count"][:0].contiguous())
    assert empty["track_id"].shape == (0, WALK["S"]) and np.array_equal(three.state_blob(), before)
    # state = NULL: the same results from a fresh start, nothing saved
    fresh = PersonTracker(None, **kw)
    got = _host(fresh.run_torch(w["xyzs"], w["count"], carry=False))
    for key in whole:
        assert np.array_equal(got[key].view(np.uint8), whole[key].view(np.uint8)), key
    assert not fresh.state_blob().any()
    # reset() starts the identities over
    three.reset()
    again = _host(three.run_torch(w["xyzs"][b:].contiguous(), w["count"][b:].contiguous(), gather=False))
    assert sorted(np.unique(again["track_id"][again["track_id"] >= 0]).tolist()) == [0, 1, 2]
    assert len(np.unique(parts[2]["track_id"][parts[2]["track_id"] >= 0])) == 3


# ---------------------------------------------------------------------------------------------------------------- 4
@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_gather_copies_records_bit_for_bit(api, dtype):
    import torch
    from snowmocap_amd.tracking import PersonTracker, gather_reference
    F, P, S, kn = 37, 5, 7, 19
    rng = np.random.default_rng(4)
    xyzs = rng.normal(size=(F, P, kn, 4)).astype(dtype)
    bits = xyzs.view(np.uint32 if dtype == np.float32 else np.uint64)
    nan_at = rng.random(bits.shape) < 0.05                  # NaNs with payloads, quiet and signalling patterns
    payload = rng.integers(1, 1 << 20, size=bits.shape).astype(bits.dtype)
    bits[nan_at] = (np.array(0x7f800000 if dtype == np.float32 else 0x7ff0000000000000, dtype=bits.dtype) | payload)[nan_at]
    assert np.isnan(xyzs).any()
    person_of = rng.integers(-1, P, size=(F, S)).astype(np.int32)
    trk = PersonTracker(None, S=S, center_point_index=0, gate=1.0, max_missed=0)
    L, h = trk.ctx.L, trk.ctx.handle
    from snowmocap_amd import _lib
    xd, pd = torch.from_numpy(xyzs).cuda(), torch.from_numpy(person_of).cuda()
    out = torch.full((F, S, kn, 4), 7.0, dtype=xd.dtype, device="cuda")
    st = torch.cuda.current_stream().cuda_stream
    rc = L.snowtri_track_gather(h, F, P, kn, ct.c_void_p(xd.data_ptr()), _lib.dtype_code(dtype), S, ct.c_void_p(pd.data_ptr()),
                                ct.c_void_p(out.data_ptr()), _lib.DEVICE, ct.c_void_p(st))
    assert rc == _lib.OK
    torch.cuda.synchronize()
    want = gather_reference(xyzs, person_of)
    got = out.cpu().numpy()
    assert np.array_equal(got.view(bits.dtype), want.view(bits.dtype))
    assert not got[person_of < 0].view(bits.dtype).any() and (person_of < 0).any()
    host = np.full((F, S, kn, 4), 7.0, dtype=dtype)
    rc = L.snowtri_track_gather(h, F, P, kn, _lib.ptr(xyzs), _lib.dtype_code(dtype), S, _lib.ptr(person_of), _lib.ptr(host), _lib.HOST, None)
    assert rc == _lib.OK and np.array_equal(host.view(bits.dtype), want.view(bits.dtype))


# ---------------------------------------------------------------------------------------------------------------- 5
@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_host_calls_equal_device_calls(api, dtype):
    import torch
    from snowmocap_amd.tracking import PersonTracker
    B, _ = _block_sizes()
    xyzs, count, cpi = synthetic_lists(30, B + 9, dtype)
    kw = dict(S=16, center_point_index=cpi, gate=0.3, max_missed=2)
    dev, hst = PersonTracker(None, **kw), PersonTracker(None, **kw)
    for lo, hi in ((0, 11), (11, B + 9)):                   # two calls each: the state takes both routes too
        d = _host(dev.run_torch(torch.from_numpy(xyzs[lo:hi]).cuda(), torch.from_numpy(count[lo:hi]).cuda()))
        h = hst.run_host(xyzs[lo:hi], count[lo:hi])
        for key in d:
            assert np.array_equal(d[key].view(np.uint8), h[key].view(np.uint8)), key
        assert np.array_equal(dev.state_blob(), hst.state_blob())
    # a tracker moves its state between the two kinds of call
    mixed = PersonTracker(None, **kw)
    mixed.run_host(xyzs[:11], count[:11], gather=False)
    m = _host(mixed.run_torch(torch.from_numpy(xyzs[11:]).cuda(), torch.from_numpy(count[11:]).cuda(), gather=False))
    assert np.array_equal(m["track_id"], d["track_id"])


# ---------------------------------------------------------------------------------------------------------------- 6
def test_bad_arguments_report_their_status(api):
    from snowmocap_amd import _lib
    from snowmocap_amd.tracking import PersonTracker
    ctx = _lib.scratch_context()
    L, h = ctx.L, ctx.handle
    F, P, kn, S = 3, 4, 5, 4
    xyzs = np.zeros((F, 16, kn, 4), dtype=np.float32)
    count = np.zeros(F, dtype=np.int32)
    so, po, ti = np.full((F, 16), 9, dtype=np.int32), np.full((F, 16), 9, dtype=np.int32), np.full((F, 16), 9, dtype=np.int32)

    def call(F=F, P=P, kn=kn, S=S, cpi=0, gate=1.0, mm=0, dtype=_lib.F32, memspace=_lib.HOST):
        rc = L.snowtri_track_persons(h, F, P, kn, _lib.ptr(xyzs), dtype, _lib.ptr(count), S, cpi, gate, mm, None, _lib.ptr(so), _lib.ptr(po),
                                     _lib.ptr(ti), None, memspace, None)
        return rc, L.snowtri_last_error().decode()

    assert call()[0] == _lib.OK
    for kw in (dict(S=0), dict(S=17), dict(P=0), dict(P=17), dict(gate=-0.5), dict(gate=float("nan")), dict(gate=float("inf")), dict(mm=-1),
               dict(dtype=2), dict(memspace=2), dict(F=-1)):
        so[:] = 9
        rc, msg = call(**kw)
        assert rc == _lib.ERR_BAD_ARG and msg.startswith("snowtri_track_persons"), (kw, rc, msg)
        assert (so == 9).all()
    for cpi in (-1, kn, kn + 100):
        rc, msg = call(cpi=cpi)
        assert rc == _lib.ERR_BAD_INDEX and "center_point_index" in msg, (cpi, rc, msg)
    so[:] = 9
    assert call(F=0)[0] == _lib.OK and (so == 9).all()       # F == 0 touches nothing
    assert L.snowtri_track_persons(None, F, P, kn, _lib.ptr(xyzs), 0, _lib.ptr(count), S, 0, 1.0, 0, None, _lib.ptr(so), _lib.ptr(po), _lib.ptr(ti),
                                   None, _lib.HOST, None) == _lib.ERR_BAD_ARG
    assert L.snowtri_track_persons(h, F, P, kn, None, 0, _lib.ptr(count), S, 0, 1.0, 0, None, _lib.ptr(so), _lib.ptr(po), _lib.ptr(ti),
                                   None, _lib.HOST, None) == _lib.ERR_BAD_ARG
    for kw in (dict(S=0), dict(S=17), dict(P=17), dict(kn=0), dict(dtype=5)):
        a = dict(P=P, kn=kn, S=S, dtype=_lib.F32)
        a.update(kw)
        rc = L.snowtri_track_gather(h, F, a["P"], a["kn"], _lib.ptr(xyzs), a["dtype"], a["S"], _lib.ptr(po), _lib.ptr(xyzs), _lib.HOST, None)
        assert rc == _lib.ERR_BAD_ARG and L.snowtri_last_error().decode().startswith("snowtri_track_gather"), kw
    # the Python layer turns them into exceptions
    with pytest.raises(ValueError):
        PersonTracker(None, S=17)
    with pytest.raises(ValueError):
        PersonTracker(None, S=4, gate=-1.0).run_host(xyzs[:, :4], count)
    with pytest.raises(IndexError):
        PersonTracker(None, S=4, center_point_index=kn).run_host(xyzs[:, :4], count)
    assert L.snowtri_version() == 100


# ---------------------------------------------------------------------------------------------------------------- 7
def test_bounds_checks_stay_silent_in_the_test_build(api):
    import os
    from snowmocap_amd import _lib
    assert os.path.exists(_lib.TEST_LIB_PATH), "build the test library: make -C snowmocap_amd/csrc debug"
    prev = _lib.use_library(_lib.TEST_LIB_PATH)
    try:
        assert "SNOWTRI_DEBUG_BOUNDS" in _lib.build_info()["variants"]
        ctx = _lib.scratch_context()
        assert ctx.debug_faults()[0] == 0
        for kn in (1, 30, 133):
            _run_synthetic(kn, check_busy=False)
        # ... and the gather
        import torch
        from snowmocap_amd.tracking import PersonTracker
        xyzs, count, cpi = synthetic_lists(30, 40, np.float64)
        trk = PersonTracker(None, S=16, center_point_index=cpi, gate=0.3, max_missed=2)
        assert trk.ctx is ctx
        out = trk.run_torch(torch.from_numpy(xyzs).cuda(), torch.from_numpy(count).cuda())
        assert bool((out["xyzs_tracked"][..., 3] != 0).any())
        n, first = ctx.debug_faults()
        assert n == 0, f"device-side bounds check failed {n} times; first: code {first >> 32} at line {first & 0xffffffff}"
    finally:
        _lib.use_library(prev)
    assert not _lib.LIB_PATH.endswith("_dbg.so")


# ---------------------------------------------------------------------------------------------------------------- 8
def test_tracked_pipeline_equals_the_ordered_pipeline(api):
    """The walker scene without dropouts, twice: per-camera lists in random order -> TrackPipeline.run(ragged="track"); the
    same detections (noise drawn per frame, camera and true person before the lists are ordered) in person order ->
    ragged="refuse", the reference's index matching, which is right for them.  Slot by slot (through frame 0) the filtered
    tracks agree within the project's fp64 parity bound of 1e-8 m (only the fusion's summation order differs);
    ragged="reference" on the permuted lists does not: it filters whoever sits at a list index."""
    from snowmocap_amd import synth
    from snowmocap_amd.blender import CONTROL_POINT_NAMES
    perm, ordered = walker_scene(dropouts=False, permute=True), walker_scene(dropouts=False, permute=False)
    K, R, t = perm["rig"]
    # the same detections: every (frame, camera) list of one is a permutation of the other's
    assert np.array_equal(np.sort(perm["kpts"][..., 0, 0], axis=2), np.sort(ordered["kpts"][..., 0, 0], axis=2))
    assert not np.array_equal(perm["kpts"], ordered["kpts"])
    smo = {n: [2.0, 0.75, 0.0] for n in CONTROL_POINT_NAMES}
    pipe = api.TrackPipeline(K, R, t, perm["params"], smo, n_persons_out=4)
    trk = {k: v.cpu().numpy() for k, v in pipe.run(perm["kpts"], perm["n_persons"], ragged="track").items()}
    ref = {k: v.cpu().numpy() for k, v in pipe.run(ordered["kpts"], ordered["n_persons"], ragged="refuse").items()}
    idx = {k: v.cpu().numpy() for k, v in pipe.run(perm["kpts"], perm["n_persons"], ragged="reference").items()}
    pipe.close()
    assert trk["present"].all() and (trk["track_id"] == np.arange(4)[None, :]).all() and (trk["tracked"] == 4).all()
    # frame 0: which slot of the ordered run is slot s of the tracked run
    d0 = np.linalg.norm(trk["xyzs"][0, :, None, 0, :3] - ref["xyzs"][0, None, :, 0, :3], axis=-1)
    to_ref = d0.argmin(axis=1)
    assert sorted(to_ref.tolist()) == [0, 1, 2, 3] and d0.min(axis=1).max() < 1e-8
    worst = {}
    for key in ("xyzs", "smoothed", "points_smoothed"):
        worst[key] = float(np.abs(trk[key][..., :3] - ref[key][:, to_ref][..., :3]).max())
    print("tracked vs ordered pipeline, max |difference| in metres:", worst)
    assert worst["smoothed"] <= 1e-8 and worst["points_smoothed"] <= 1e-8 and worst["xyzs"] <= 1e-8
    assert np.array_equal(trk["valid"], ref["valid"][:, to_ref])
    # by list index the permuted lists give other tracks (a slot mixes persons)
    d0 = np.linalg.norm(idx["xyzs"][0, :, None, 0, :3] - ref["xyzs"][0, None, :, 0, :3], axis=-1)
    by_index = float(np.abs(idx["smoothed"][..., :3] - ref["smoothed"][:, d0.argmin(axis=1)][..., :3]).max())
    print("index-matched pipeline on the permuted lists differs by", by_index, "m")
    assert by_index > 0.1
    # the JSON form lists the present slots
    res = api.TrackPipeline.to_blender_result(trk["points_smoothed"], trk["valid"], present=trk["present"])
    assert len(res) == WALK["F"] and all(len(fr["armature"]) == 4 for fr in res)
