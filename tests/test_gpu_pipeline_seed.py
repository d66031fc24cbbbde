"""TrackPipeline.run(seed=...) on the GPU, on the detections of the recipe "crossing" (tests/assign_cases.py: 60 frames, 4 cameras,
3 walkers of 133 joints, lists permuted, 1 px of noise).

THE HOOK.  The pipeline is handed a first pass of TWO persons: the test wraps the triangulator's run_torch (a test-side wrapper of the
bound method; no code path of the package is touched) so that the first pass's records are the walkers A and B -- the truth + N(0, 1
cm) per joint, score 1 -- in slots 0 and 1, zeros behind them, count 2.  The third walker, C, is then a person the first pass
missed: nobody claims its detections, and run(retriangulate=12.0, one_to_one=True, seed=0.03) has to put it into slot count = 2.

Accuracy bar of a seeded record: 1 px of noise is 1 / 690 rad, 5 .. 8 mm across a ray at the 3.6 .. 5.5 m between C's path and the
cameras; four views leave about that much per joint in 3D (RMS over a person, 7.5 mm for the matched triangulation on this recipe:
README).  The bar is 2 cm RMS over the seeded person's joints per frame and 6 cm for a single joint (six sigma of the worst view).
"""
import functools

import numpy as np
import pytest

import assign_cases as ac
import pipeline_cases as plc
from snowmocap_amd import _lib, synth
from snowmocap_amd import seed as sd
from snowmocap_amd.reproject import assign_detections_reference, reprojection_cost_reference

pytestmark = pytest.mark.gpu

P_OUT = 4
RTR = 12.0
GATE = 0.03


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view({1: np.uint8, 4: np.uint32, 8: np.uint64}[a.dtype.itemsize])


@functools.lru_cache(maxsize=None)
def scene():
    cs = ac.crossing()
    rng = np.random.default_rng(20262)
    first = np.zeros((ac.CROSS_F, P_OUT, 133, 4))
    first[:, :2, :, :3] = cs["X"][:, :2] + rng.normal(0.0, 0.01, cs["X"][:, :2].shape)
    first[:, :2, :, 3] = 1.0
    prm = dict(synth.default_thresholds(), keypoint_score_threshold=ac.CROSS_THRESHOLD, keypoint_num=133)
    first.setflags(write=False)
    return dict(cs=cs, first=first, params=prm)


@pytest.fixture(scope="module")
def pipe():
    import torch
    from snowmocap_amd import TrackPipeline
    assert _lib.lib().snowtri_device_count() > 0, "these tests need the HIP device"
    sc = scene()
    cs = sc["cs"]
    p = TrackPipeline(cs["K"], cs["R"], cs["t"], sc["params"], plc.SMOOTH_PROFILE, n_persons_out=P_OUT)
    p.first_pass = p.bt.run_torch                              # the library's own first pass, for the test of seed=None

    def two_persons(kpts, n_persons=None, **kw):
        tri = dict(p.first_pass(kpts, n_persons, **kw))
        tri["xyzs"] = torch.from_numpy(np.array(sc["first"])).to(tri["xyzs"].device).to(tri["xyzs"].dtype)
        tri["count"] = torch.full_like(tri["count"], 2)
        tri["flags"] = torch.zeros_like(tri["flags"])
        return tri

    p.two_persons = two_persons
    yield p
    p.bt.run_torch = p.first_pass
    p.close()


def _run(pipe, hooked=True, **kw):
    import torch
    cs = scene()["cs"]
    pipe.bt.run_torch = pipe.two_persons if hooked else pipe.first_pass
    try:
        res = pipe.run(np.array(cs["kpts"]), np.array(cs["n_persons"]), **kw)
        torch.cuda.synchronize()
    finally:
        pipe.bt.run_torch = pipe.first_pass
    return {k: v.cpu().numpy() for k, v in res.items()}


def test_the_missed_person_appears_in_slot_count(pipe):
    sc = scene()
    cs = sc["cs"]
    F = ac.CROSS_F
    base = _run(pipe, retriangulate=RTR, one_to_one=True)
    res = _run(pipe, retriangulate=RTR, one_to_one=True, seed=GATE)
    assert set(res) == set(base) | {"seeded", "seed_det_of"}
    assert (base["count"] == 2).all() and (res["count"] == 3).all() and np.array_equal(res["flags"], base["flags"])
    seeded = res["seeded"]
    assert seeded.dtype == np.bool_ and seeded.shape == (F, P_OUT) and seeded[:, 2].all() and not seeded[:, [0, 1, 3]].any()
    det = res["seed_det_of"]
    assert det.dtype == np.int32 and det.shape == (F, 4, P_OUT) and (det[:, :, [0, 1, 3]] == -1).all()
    assert np.array_equal(det[:, :, 2], cs["det_true"][:, :, 2])                               # the detections generated for walker C
    # a slot that is not seeded keeps its bits -- in every key that is indexed by slot before the trackers and filters
    for k in ("xyzs", "retri_views", "retri_resid"):
        assert np.array_equal(_bits(res[k][:, [0, 1, 3]]), _bits(base[k][:, [0, 1, 3]])), k
    assert not base["xyzs"][:, 2:].any() and not res["xyzs"][:, 3].any()
    # the seeded records against the truth
    err = np.linalg.norm(res["xyzs"][:, 2, :, :3] - cs["X"][:, 2], axis=-1)                    # [F, J]
    rms = np.sqrt((err ** 2).mean(axis=1))
    print(f"    seeded person: RMS per frame {rms.min() * 1e3:.2f} .. {rms.max() * 1e3:.2f} mm, worst joint {err.max() * 1e3:.1f} mm")
    assert (res["xyzs"][:, 2, :, 3] != 0).all() and rms.max() < 0.02 and err.max() < 0.06
    views = res["retri_views"][:, 2].view(np.uint32)
    assert (views != 0).all() and (views <= 0xF).all() and (res["retri_resid"][:, 2] > 0).all()
    # ... and against the chain by the NumPy rules on the same first pass: the same seeds, the same records to rounding
    cost = reprojection_cost_reference(cs["K"], cs["R"], cs["t"], sc["first"], cs["kpts"], cs["n_persons"], ac.CROSS_THRESHOLD)
    person_of = assign_detections_reference(cost[0], cost[1], RTR)[1]
    sl = slice(27, 33)
    ref = sd.triangulate_seeded_reference(cs["K"], cs["R"], cs["t"], cs["kpts"][sl], cs["n_persons"][sl], person_of[sl], P_OUT, GATE, 3, 8,
                                          ac.CROSS_THRESHOLD, 6.0, 1)
    assert (ref["n_seeds"] == 1).all() and np.array_equal(ref["seed_det_of"][:, :, 0], det[sl, :, 2])
    assert np.abs(ref["xyzs"][:, 0] - res["xyzs"][sl, 2]).max() < 1e-9
    # downstream takes the raised count: slot 2 is tracked and filtered
    assert (res["tracked"] == 3).all() and (base["tracked"] == 2).all()
    assert res["smoothed"][:, 2, :, :3].any() and not base["smoothed"][:, 2].any()


def test_refine_sees_the_seeds_detections(pipe):
    base = _run(pipe, retriangulate=RTR, one_to_one=True, seed=GATE)
    res = _run(pipe, retriangulate=RTR, one_to_one=True, seed=GATE, refine=4)
    assert set(res) == set(base) | {"refine_cost", "refine_codes"}
    cost = res["refine_cost"][:, 2]                                                             # [F, J, 2]
    assert (res["refine_codes"][:, 2] >= _lib.REFINE_KEPT).all() and (cost[..., 1] <= cost[..., 0]).all() and (cost[..., 0] > 0).all()
    assert not np.array_equal(res["xyzs"][:, 2], base["xyzs"][:, 2])
    assert np.array_equal(res["seeded"], base["seeded"]) and np.array_equal(res["seed_det_of"], base["seed_det_of"])


def test_seed_none_is_todays_run_bit_for_bit(pipe):
    for hooked in (True, False):
        a = _run(pipe, hooked, retriangulate=RTR, one_to_one=True)
        b = _run(pipe, hooked, retriangulate=RTR, one_to_one=True, seed=None)
        assert set(a) == set(b) and "seeded" not in a
        for k in a:
            assert a[k].dtype == b[k].dtype and np.array_equal(_bits(a[k]), _bits(b[k])), (hooked, k)
    plain, off = _run(pipe, False), _run(pipe, False, seed=None)
    assert set(plain) == set(off)
    for k in plain:
        assert np.array_equal(_bits(plain[k]), _bits(off[k])), k


def test_seed_needs_the_one_to_one_retriangulation(pipe):
    cs = scene()["cs"]
    kp, npers = np.array(cs["kpts"]), np.array(cs["n_persons"])

    def never(*a, **k):
        raise AssertionError("refused before any work")

    pipe.bt.run_torch = never
    try:
        for kw in (dict(seed=GATE), dict(seed=GATE, retriangulate=RTR), dict(seed=GATE, one_to_one=True, refine=4),
                   dict(seed=GATE, one_to_one=True, reproject=6.0)):
            with pytest.raises(ValueError, match="seed= needs retriangulate= together with one_to_one=True"):
                pipe.run(kp, npers, **kw)
        for bad in (-1.0, (GATE, 1), (GATE, 3, 0), True):
            with pytest.raises(ValueError, match="seed"):
                pipe.run(kp, npers, retriangulate=RTR, one_to_one=True, seed=bad)
    finally:
        pipe.bt.run_torch = pipe.first_pass
