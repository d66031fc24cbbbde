"""TrackPipeline.run(retriangulate=...) and pose.refine_rig(retriangulate=True) on the GPU against the NumPy rules chained
(reprojection_cost_reference -> match_detections / assign_detections_reference -> matched.triangulate_matched_reference ->
matched.merge_records -> refine_joints_reference).

The scene: 24 frames, synth.ring_rig(4), 2 walkers, per-camera lists permuted, pixel sigma 1, and camera 1 shows joints 20-29 of
everybody 30 px off in frames 5-8 (views the leave-one-out loop drops).  Its detections carry 133 joints, not 17: the pipeline's
control-point stage refuses a keypoint_num below 130 (snowtri_blender_points), so 133 is the smallest scene TrackPipeline.run takes.
The bars are those of tests/test_gpu_matched.py (masks equal where the rule's margin is >= 1e-6, xyz within 1e-9 m on float64
records, scores at rtol 1e-6, resid within 1e-6 px + 1e-6 relative; refine: costs at rtol 1e-9, points within 1e-6 m) and, for
refine_rig, those of tests/test_gpu_pose.py::test_refine_rig_against_the_rule_driven_alternation."""
import functools

import numpy as np
import pytest

import pipeline_cases as plc
import pose_cases as pc
from snowmocap_amd import _lib, matched, pose, synth
from snowmocap_amd.refine import refine_joints_reference
from snowmocap_amd.reproject import assign_detections_reference, match_detections, reprojection_cost_reference
from test_gpu_pose import BAR_NOISY
from test_gpu_robust import MARGIN

pytestmark = pytest.mark.gpu

F, P, J = 24, 2, 133
GATES = (12.0, 1.45, 0.5)         # everybody matched (the 30 px views too: 8.3 px RMS over a person); about sqrt(2) px, the noise's RMS: some views are; nobody is


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view({1: np.uint8, 4: np.uint32, 8: np.uint64}[a.dtype.itemsize])


@functools.lru_cache(maxsize=None)
def scene():
    K, R, t = synth.ring_rig(4)
    rng = np.random.default_rng(20261)
    X, _ = synth.make_walkers(rng, F, P, 0.03, J=J)
    kpts, npers = synth.make_keypoints_visible(rng, K, R, t, X, pixel_sigma=1.0, permute_persons=True)
    kpts[5:9, 1, :, 20:30, 0] += 30.0
    prm = dict(synth.default_thresholds(), average_score_threshold=1.0, condense_distance_tol=0.3, condense_person_num_tol=4)
    for a in (K, R, t, X, kpts, npers):
        a.setflags(write=False)
    return dict(K=K, R=R, t=t, X=X, kpts=kpts, n_persons=npers, params=prm, thr=float(prm["keypoint_score_threshold"]))


@pytest.fixture(scope="module")
def pipe():
    from snowmocap_amd import TrackPipeline
    assert _lib.lib().snowtri_device_count() > 0, "these tests need the HIP device"
    sc = scene()
    p = TrackPipeline(sc["K"], sc["R"], sc["t"], sc["params"], plc.SMOOTH_PROFILE, n_persons_out=P)
    yield p
    p.close()


def _run(pipe, **kw):
    import torch
    sc = scene()
    res = pipe.run(np.array(sc["kpts"]), np.array(sc["n_persons"]), **kw)
    torch.cuda.synchronize()
    return {k: v.cpu().numpy() for k, v in res.items()}


_PLAIN = {}


def plain(pipe):
    """run() without options, once per module"""
    if "res" not in _PLAIN:
        _PLAIN["res"] = _run(pipe)
    return _PLAIN["res"]


@functools.lru_cache(maxsize=None)
def rule(gate, one_to_one, first_key):
    """The second pass by the rules on the first pass's records (first_key: their bytes, so the cache is per input)
    -> dict(det_of, ref: triangulate_matched_reference's answer)"""
    sc = scene()
    first = np.frombuffer(first_key, dtype=np.float64).reshape(F, P, J, 4)
    cs, cn = reprojection_cost_reference(sc["K"], sc["R"], sc["t"], first, sc["kpts"], sc["n_persons"], sc["thr"])
    det_of = assign_detections_reference(cs, cn, gate)[0] if one_to_one else match_detections(cs, cn, gate)[0]
    ref = matched.triangulate_matched_reference(sc["K"], sc["R"], sc["t"], sc["kpts"], det_of, sc["n_persons"], sc["thr"], 6.0, 1)
    return dict(det_of=det_of, ref=ref)


def _check_second_pass(res, first, gate, one_to_one=False):
    """res["xyzs"] (not refined), retri_views and retri_resid against the rule; -> (rule, the joints where the masks agree)"""
    sc = scene()
    rl = rule(gate, one_to_one, np.ascontiguousarray(first).tobytes())
    ref = rl["ref"]
    assert res["retri_views"].dtype == np.int32 and res["retri_views"].shape == (F, P, J) and res["retri_resid"].dtype == np.float64
    views = res["retri_views"].view(np.uint32)
    sure, same = ref["margin"] >= MARGIN, views == ref["views"]
    print(f"    gate {gate} px: records replaced {(views != 0).mean():.4f}, unsure {(~sure).sum()}, mask mismatches {(~same).sum()}, "
          f"drops histogram {np.bincount(ref['drops'].ravel()).tolist()}")
    assert same[sure].all()
    if not same.all():
        alt = matched.alternative_views(sc["K"], sc["R"], sc["t"], sc["kpts"], rl["det_of"], sc["n_persons"], sc["thr"], 6.0, 1, ref, below=MARGIN)
        assert (views[~same] == alt[~same]).all()
    kept = views == 0
    assert np.array_equal(kept, ref["views"] == 0)
    x = res["xyzs"]
    assert x.dtype == np.float64 and np.array_equal(_bits(x[kept]), _bits(first[kept]))          # a kept record: the first pass's bits
    assert not res["retri_resid"][kept].any()
    made = same & ~kept
    if made.any():
        err = np.abs(x[..., :3] - ref["xyzs"][..., :3])[made]
        dr = np.abs(res["retri_resid"] - ref["resid"])[made]
        print(f"    max |xyz - rule| = {err.max():.3e} m (bar 1e-9), max resid error = {dr.max():.3e} px")
        assert err.max() < 1e-9
        np.testing.assert_allclose(x[..., 3][made], ref["xyzs"][..., 3][made], rtol=1e-6)
        assert (dr <= 1e-6 + 1e-6 * np.abs(ref["resid"][made])).all()
    return rl, same


def test_off_is_the_default_run_bit_for_bit(pipe):
    a, b = plain(pipe), _run(pipe, retriangulate=None)
    assert set(a) == set(b) and "retri_views" not in a
    for k in a:
        assert a[k].dtype == b[k].dtype and np.array_equal(_bits(a[k]), _bits(b[k])), k
    assert (a["count"] == P).all()


@pytest.mark.parametrize("gate", GATES)
def test_records_are_the_rule_where_made_and_the_first_pass_elsewhere(pipe, gate):
    base = plain(pipe)
    res = _run(pipe, retriangulate=gate)
    assert set(res) == set(base) | {"retri_views", "retri_resid"}
    for k in ("count", "flags", "tracked"):
        assert np.array_equal(res[k], base[k]), k
    _check_second_pass(res, base["xyzs"], gate)
    views = res["retri_views"]
    if gate == GATES[0]:
        nviews = sum((views >> c) & 1 for c in range(4))
        assert (views != 0).all() and (nviews[5:9, :, 20:30] == 3).all()                  # the 30 px views were dropped
        sc = scene()
        e0, e1 = (float(np.sqrt(((r[..., :3] - sc["X"]) ** 2).sum(-1).mean())) for r in (base["xyzs"], res["xyzs"]))
        print(f"    RMS error against the truth: first pass {e0 * 1e3:.2f} mm, second pass {e1 * 1e3:.2f} mm")
    if gate == GATES[-1]:
        assert not views.any()
        for k in base:                                                                      # nothing replaced: the default run
            assert np.array_equal(_bits(res[k]), _bits(base[k])), k
    # the later stages received those records: N1 of res["xyzs"] (every slot is carried in every frame)
    sc = dict(params=scene()["params"])
    for i in range(P):
        want = plc._n1(sc, res["xyzs"][:, i])
        assert np.abs(res["smoothed"][:, i, :, :3] - want[..., :3]).max() <= plc.N1_ATOL
        assert np.array_equal(_bits(res["smoothed"][:, i, :, 3]), _bits(res["xyzs"][:, i, :, 3]))
    if gate == GATES[0]:
        assert not np.array_equal(res["smoothed"], base["smoothed"])


def test_one_to_one_alone_and_with_refine(pipe):
    """retriangulate= with one_to_one=True (legal without reproject= or refine=), then with refine= as well: the refinement is
    refine_joints_reference on the merged records with THIS det_of and the mask (all ones on a kept record)."""
    sc, base = scene(), plain(pipe)
    gate = GATES[1]
    alone = _run(pipe, retriangulate=(gate, 6.0, 1), one_to_one=True)
    rl, same = _check_second_pass(alone, base["xyzs"], gate, one_to_one=True)
    res = _run(pipe, retriangulate=gate, refine=4, one_to_one=True)
    assert set(res) == set(base) | {"retri_views", "retri_resid", "refine_cost", "refine_codes"}
    for k in ("retri_views", "retri_resid"):
        assert np.array_equal(_bits(res[k]), _bits(alone[k])), k
    merged, mask = matched.merge_records(base["xyzs"], alone["xyzs"], alone["retri_views"])
    assert np.array_equal(_bits(merged), _bits(alone["xyzs"])) and (mask[alone["retri_views"] == 0] == 0xFFFFFFFF).all()
    out, cost, codes = refine_joints_reference(sc["K"], sc["R"], sc["t"], merged, sc["kpts"], rl["det_of"], sc["n_persons"], mask, sc["thr"],
                                               iters=4)
    print(f"    codes equal {(res['refine_codes'] == codes).mean():.4f}, max |xyz - rule| = {np.abs(res['xyzs'] - out).max():.3e} m")
    assert (res["refine_codes"] == codes).mean() > 0.999
    assert np.allclose(res["refine_cost"], cost, rtol=1e-9, atol=0) and np.abs(res["xyzs"] - out).max() < 1e-6
    assert np.array_equal(_bits(res["xyzs"][..., 3]), _bits(merged[..., 3]))                   # scores untouched
    with pytest.raises(ValueError, match="one_to_one"):
        pipe.run(np.array(sc["kpts"]), np.array(sc["n_persons"]), one_to_one=True)
    with pytest.raises(ValueError, match="gate"):
        pipe.run(np.array(sc["kpts"]), np.array(sc["n_persons"]), one_to_one=True, retriangulate=np.inf)


def test_refine_rig_retriangulate_against_the_rule_driven_alternation():
    """pose.refine_rig(retriangulate=True) on the GPU (k_dlt_matched between the matching and refine_joints) against the same
    alternation by the NumPy rules, both with pose_cases.dlt_points as the first triangulation, on the two-person recipe."""
    rp = pc.recipe(P=2)
    bad = rp["bad"]
    args = (rp["K"], rp["Rd"], rp["td"], rp["kpts"])
    kw = dict(free=[bad], rounds=1, triangulate=pc.dlt_points, params=dict(keypoint_score_threshold=0.5), retriangulate=True)
    R, t, hist = pose.refine_rig(*args, **kw)
    Rr, tr, hr = pose.refine_rig(*args, reference=True, **kw)
    eR, et = pc.pose_error(R, t, Rr, tr, [bad])
    print(f"    |R - R_rule| = {eR:.2e}, |t - t_rule| / rig scale = {et:.2e}; view RMS {[round(float(h['view_rms'][bad]), 3) for h in hist]} px")
    assert eR <= BAR_NOISY[0] and et <= BAR_NOISY[1], (eR, et)
    for h, g in zip(hist, hr):
        assert np.allclose(h["view_rms"], g["view_rms"], rtol=0, atol=1e-6)
        if "codes" in h:
            assert np.array_equal(h["codes"], g["codes"]) and np.array_equal(h["n_obs"], g["n_obs"])
    keep = [c for c in range(8) if c != bad]
    assert np.array_equal(_bits(R[keep]), _bits(np.ascontiguousarray(rp["Rd"][keep])))
