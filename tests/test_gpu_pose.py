"""k_pose_normal / k_pose_step behind snowtri_refine_cameras (include/snowtri.h, "Camera pose refinement"), Context.refine_cameras /
pose.refine_cameras, CameraGroup.refine_poses and pose.refine_rig.  Inputs: tests/pose_cases.py -- the kernel against the NumPy rule on
the same inputs.

  * n_obs equal, exactly; codes equal -- FIXED / FEW_OBS everywhere, KEPT / MOVED wherever the rule's first step lowers E by more than
    1 % (at an exact start the two are decided by rounding);
  * exact detections: the poses within 4 x FLOOR_EXACT of the truth, on the shape, rigs and placements the floor was measured on;
    noisy detections: within 4 x FLOOR_NOISY of the 50-digit minimiser;
  * `normal` within 4 x NORMAL_UNITS eps * sum |term| of the rule's; cost[., 1] <= cost[., 0], and E recomputed by the rule at the
    output pose agrees with cost[., 1] to the same bound, on every case (the kernel forms E's terms in the rule's own operations);
  * R_out^T R_out - I below 64 eps; two runs give the same bits; a camera that may not move keeps its bits;
  * float32 records and keypoints at the six placements; torch DEVICE and NumPy HOST give the same bits; one record more than a sweep
    of the grid; the bad-arguments program; the debug build; refine_rig against the rule-driven alternation.
"""
import os
import subprocess

import numpy as np
import pytest

import pose_cases as pc
import refine_cases as rc
from snowmocap_amd import _lib, pose, synth

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EPS = pc.EPS
FIXED, FEW, KEPT, MOVED = pose.POSE_FIXED, pose.POSE_FEW_OBS, pose.POSE_KEPT, pose.POSE_MOVED
BAR_EXACT = tuple(pc.MARGIN * f for f in pc.FLOOR_EXACT)
BAR_NOISY = tuple(pc.MARGIN * f for f in pc.FLOOR_NOISY)
BAR_NORMAL = pc.MARGIN * pc.NORMAL_UNITS * EPS


@pytest.fixture(scope="module")
def api():
    import snowmocap_amd as sm
    assert _lib.lib().snowtri_device_count() > 0, "these tests need the HIP device"
    return sm


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view({8: np.uint64, 4: np.uint32, 1: np.uint8}[a.dtype.itemsize])


def _same_bits(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and np.array_equal(_bits(a), _bits(b))


def _run(cs, **over):
    ctx = _lib.Context(cs["K"], cs["Rd"], cs["td"])
    try:
        return ctx.refine_cameras(cs["xyzs"], cs["kpts"], diagnostics=True, **dict(cs["kw"], **over))
    finally:
        ctx.close()


def _magnitudes(cs, S, R, t, c, score_weights=False):
    """sum |term| [28] of camera c's E, g, H at the pose (R[c], t[c]) and the rule's sums there."""
    X, ou, ov, w = pc.camera_observations(cs, S, c, score_weights)
    terms, _ = pose.normal_terms(cs["K"][c], R[c], t[c], X, ou, ov, w)
    return np.abs(terms).sum(axis=0), pose._ordered_sum(terms)


def _check_against_the_rule(cs, got, ref, score_weights=False):
    """Everything that holds on every case: counts, codes, normal, costs, rotations, the cameras that stay."""
    R, t, rep = got
    Rr, tr, rr, S = ref
    C = cs["K"].shape[0]
    assert R.shape == (C, 3, 3) and t.shape == (C, 3) and R.dtype == t.dtype == np.float64
    assert rep["n_obs"].dtype == np.int64 and np.array_equal(rep["n_obs"], rr["n_obs"])
    still = (rr["codes"] == FIXED) | (rr["codes"] == FEW)
    assert np.array_equal(rep["codes"][still], rr["codes"][still]) and (rep["codes"][~still] >= KEPT).all()
    first = pose.refine_cameras_reference(cs["K"], cs["Rd"], cs["td"], cs["xyzs"], cs["kpts"], score_weights=score_weights,
                                          **dict(cs["kw"], iters=1))[2]["cost"]
    clear = ~still & (first[:, 1] < 0.99 * first[:, 0])
    assert np.array_equal(rep["codes"][clear], rr["codes"][clear]) and (rep["codes"][clear] == MOVED).all()
    assert np.isfinite(rep["cost"]).all() and (rep["cost"][:, 1] <= rep["cost"][:, 0]).all() and not rep["cost"][still].any()
    worst = 0.0
    for c in range(C):
        if rep["n_obs"][c]:
            mag, _ = _magnitudes(cs, S, cs["Rd"], cs["td"], c, score_weights)
            err = np.abs(rep["normal"][c] - rr["normal"][c]) / np.where(mag > 0, mag, 1.0)
            worst = max(worst, float(err.max()))
        else:
            assert not rep["normal"][c].any()
        if rep["codes"][c] != MOVED:
            assert _same_bits(R[c], cs["Rd"][c]) and _same_bits(t[c], cs["td"][c])
        if not still[c]:
            assert rep["cost"][c, 0] == rep["normal"][c, 0]
            assert np.abs(R[c].T @ R[c] - np.eye(3)).max() < 64 * EPS
            if rep["codes"][c] == MOVED:
                assert rep["cost"][c, 1] < rep["cost"][c, 0]
            # E at the output pose, recomputed by the rule: the terms are the rule's own plain operations at the same pose bits, only
            # the order of the sum differs, and sum |term| of E is E -- at exact detections too, where E is nothing but rounding
            mag, E = _magnitudes(cs, S, R, t, c, score_weights)
            assert abs(E[0] - rep["cost"][c, 1]) <= BAR_NORMAL * mag[0], (c, E[0], rep["cost"][c, 1])
    assert worst <= BAR_NORMAL, worst / EPS
    return worst / EPS


# ------------------------------------------------------------------------------------------------ the rule, shape by shape
@pytest.mark.parametrize("rig_name", pc.RIGS)
def test_counts_codes_normal_and_costs_against_the_rule(api, rig_name):
    worst = 0.0
    seen = np.zeros(4, dtype=np.int64)
    for shape in pc.SHAPES:
        for sigma in (0.0, 1.0):
            cs = pc.case(rig_name, shape, sigma, True)
            got = _run(cs)
            worst = max(worst, _check_against_the_rule(cs, got, pc.reference(rig_name, shape, sigma, True)))
            seen += np.bincount(got[2]["codes"], minlength=4)
            again = _run(cs)                                  # two runs, two contexts: the same bits
            assert _same_bits(got[0], again[0]) and _same_bits(got[1], again[1])
            assert all(_same_bits(got[2][k], again[2][k]) for k in ("cost", "n_obs", "codes", "normal"))
    cs = pc.case(rig_name, (6, 2, 17), 1.0, True)
    got = _run(cs, score_weights=True)
    _check_against_the_rule(cs, got, pc.reference(rig_name, (6, 2, 17), 1.0, True, score_weights=True), True)
    print(f"    {rig_name}: max |normal - rule| = {worst:.1f} eps * sum |term| (bar {pc.MARGIN * pc.NORMAL_UNITS:.0f}); codes seen {seen}")
    assert (seen[[FIXED, FEW, MOVED]] > 0).all()


# ------------------------------------------------------------------------------------------------ accuracy
@pytest.mark.parametrize("rig_name", pc.RIGS)
def test_exact_detections_return_to_the_true_pose(api, rig_name):
    wR = wt = 0.0
    for placement in pc.PLACEMENTS:
        cs = pc.case(rig_name, pc.EXACT_SHAPE, 0.0, True, placement=placement)
        R, t, rep = got = _run(cs)
        _check_against_the_rule(cs, got, pc.reference(rig_name, pc.EXACT_SHAPE, 0.0, True, placement=placement))
        assert (rep["codes"][list(cs["free"])] == MOVED).all()
        eR, et = pc.pose_error(R, t, cs["R"], cs["t"], cs["free"])
        wR, wt = max(wR, eR), max(wt, et)
        assert eR <= BAR_EXACT[0] and et <= BAR_EXACT[1], (placement, eR, et)
    print(f"    {rig_name}: max |R - R_true| = {wR:.2e} (bar {BAR_EXACT[0]:.2e}), |t - t_true| / rig scale = {wt:.2e} (bar {BAR_EXACT[1]:.2e})")


@pytest.mark.parametrize("rig_name", pc.RIGS)
def test_noisy_detections_against_the_exact_minimiser(api, rig_name):
    wR = wt = 0.0
    for sigma in (1.0, 2.0):
        cs = pc.case(rig_name, pc.MINIMISER_SHAPE, sigma, True)
        mn = pc.minimiser(rig_name, sigma)
        R, t, rep = got = _run(cs)
        _check_against_the_rule(cs, got, pc.reference(rig_name, pc.MINIMISER_SHAPE, sigma, True))
        cams = list(mn["cams"])
        assert (rep["codes"][cams] == MOVED).all()
        eR, et = pc.pose_error(R, t, mn["R"], mn["t"], cams)
        wR, wt = max(wR, eR), max(wt, et)
        assert eR <= BAR_NOISY[0] and et <= BAR_NOISY[1], (sigma, eR, et)
    print(f"    {rig_name}: max |R - R*| = {wR:.2e} (bar {BAR_NOISY[0]:.2e}), |t - t*| / rig scale = {wt:.2e} (bar {BAR_NOISY[1]:.2e})")


@pytest.mark.parametrize("placement", pc.PLACEMENTS)
def test_float32_records_and_keypoints(api, placement):
    """float32 in, the same float32 values given to the rule: everything of _check_against_the_rule, and the two end at the same
    pose within the noisy bar -- both are strict-decrease iterations on one cost, whose floor grows with sqrt(E), and E here (the
    rounding of the inputs to float32: hundredths of a pixel) lies below that of the sigma = 1 cases the floor was measured on."""
    for rig_name in ("floor", "ring5"):
        for sigma in (0.0, 1.0):
            cs = pc.case(rig_name, pc.EXACT_SHAPE, sigma, True, "float32", "float32", placement)
            assert cs["xyzs"].dtype == np.float32 and cs["kpts"].dtype == np.float32
            R, t, rep = got = _run(cs)
            ref = pc.reference(rig_name, pc.EXACT_SHAPE, sigma, True, "float32", "float32", placement)
            _check_against_the_rule(cs, got, ref)
            moved = [c for c in cs["free"] if rep["codes"][c] == MOVED]
            eR, et = pc.pose_error(R, t, ref[0], ref[1], moved)
            print(f"    {rig_name} {placement} sigma {sigma}: |R - R_rule| = {eR:.2e}, |t - t_rule| / rig scale = {et:.2e}")
            assert moved == list(cs["free"]) and eR <= BAR_NOISY[0] and et <= BAR_NOISY[1], (eR, et)


# ------------------------------------------------------------------------------------------------ spaces, sizes, the library around it
def test_torch_device_and_numpy_host_give_the_same_bits(api):
    import torch
    dev = torch.device("cuda", 0)
    for rig_name, shape, dt in (("floor", (6, 2, 17), "float64"), ("ring16", (2, 3, 21), "float32")):
        cs = pc.case(rig_name, shape, 1.0, True, dt, dt)
        host = _run(cs)
        ctx = _lib.Context(cs["K"], cs["Rd"], cs["td"])
        kw = dict(cs["kw"], det_of=torch.from_numpy(np.array(cs["det_of"])).to(dev), n_persons=torch.from_numpy(np.array(cs["n_persons"])).to(dev),
                  views=torch.from_numpy(np.array(cs["views"]).view(np.int32)).to(dev))
        x, kp = torch.from_numpy(np.array(cs["xyzs"])).to(dev), torch.from_numpy(np.array(cs["kpts"])).to(dev)
        for _ in range(2):                                    # the second call reuses the context's workspace
            R, t, rep = ctx.refine_cameras(x, kp, diagnostics=True, **kw)
            assert R.is_cuda and rep["n_obs"].dtype == torch.int64
            assert _same_bits(R.cpu().numpy(), host[0]) and _same_bits(t.cpu().numpy(), host[1])
            assert all(_same_bits(rep[k].cpu().numpy(), host[2][k]) for k in ("cost", "n_obs", "codes", "normal"))
        R2, t2 = pose.refine_cameras(ctx, x, kp, **kw)        # without diagnostics: the optional outputs are NULL
        assert _same_bits(R2.cpu().numpy(), host[0]) and _same_bits(t2.cpu().numpy(), host[1])
        ctx.close()


def test_one_record_more_than_a_sweep_of_the_grid(api):
    """F = POSE_SWEEP_RECORDS + 1 frames of one joint in three cameras (19 MB of keypoints): some lanes walk two records, and a
    camera's sum is made of 1024 partials.  Exact detections, a few of them spoiled."""
    assert _lib.lib().snowtri_pose_sweep_records() == _lib.POSE_SWEEP_RECORDS == 262144
    F = _lib.POSE_SWEEP_RECORDS + 1
    K, R, t, _, _ = __import__("undistort_cases").rig("ring3")
    rng = np.random.default_rng(rc._seed("pose-sweep"))
    X = synth.make_people(rng, F, 1, J=1)
    kp = np.concatenate([np.moveaxis(synth.project(K, R, t, X)[0], 0, 1), np.ones((F, 3, 1, 1, 1))], axis=-1)
    kp[::1001, 1, 0, 0, 0] = np.nan
    kp[5::977, :, 0, 0, 2] = 0.25
    x4 = np.concatenate([X, np.ones((F, 1, 1, 1))], axis=-1)
    x4[7::4099] = 0.0
    Rd, td = pc.drift("ring3", "home", R, t, [1])
    cs = dict(K=K, R=R, t=t, Rd=Rd, td=td, free=(1,), xyzs=x4, kpts=kp, det_of=None, n_persons=None, views=None, thr=0.5,
              kw=dict(keypoint_score_threshold=0.5, free=[1], min_obs=pc.MIN_OBS, iters=pc.ITERS))
    ref = pose.refine_cameras_reference(K, Rd, td, x4, kp, return_sets=True, **cs["kw"])
    got = _run(cs)
    units = _check_against_the_rule(cs, got, ref)
    spoiled = np.zeros(F, dtype=bool)
    spoiled[::1001] = spoiled[5::977] = spoiled[7::4099] = True
    assert ref[3][1, -1] and ref[2]["n_obs"][1] == F - spoiled.sum()                          # the last record counts
    eR, et = pc.pose_error(got[0], got[1], R, t, [1])
    print(f"    {F} records: |normal - rule| = {units:.1f} eps * sum |term|, |R - R_true| = {eR:.2e}, |t - t_true| / rig scale = {et:.2e}")
    assert got[2]["codes"].tolist() == [FIXED, MOVED, FIXED] and eR <= BAR_EXACT[0] and et <= BAR_EXACT[1]


def test_wrappers_refusals_the_empty_batch_and_the_camera_group(api, tmp_path):
    cs = pc.case("floor", (6, 2, 17), 1.0, True)
    ctx = _lib.Context(cs["K"], cs["Rd"], cs["td"])
    x, kp, kw = cs["xyzs"], cs["kpts"], cs["kw"]
    for bad in (dict(iters=0), dict(iters=17), dict(iters=2.5), dict(min_obs=2), dict(min_obs=6.5), dict(free=[4]), dict(free=1 << 4),
                dict(keypoint_score_threshold=float("nan"))):
        with pytest.raises(ValueError):
            ctx.refine_cameras(x, kp, **dict(kw, **bad))
    with pytest.raises(ValueError):
        ctx.refine_cameras(x[..., :3], kp, **kw)
    with pytest.raises(ValueError):
        ctx.refine_cameras(x, kp[:, :3], **kw)
    R, t, rep = ctx.refine_cameras(np.zeros((0, 2, 17, 4)), np.zeros((0, 4, 3, 17, 3)), free=[1, 3], min_obs=3, iters=2, diagnostics=True)
    assert _same_bits(R, np.ascontiguousarray(cs["Rd"])) and _same_bits(t, np.ascontiguousarray(cs["td"]))
    assert rep["codes"].tolist() == [FIXED, FEW, FIXED, FEW] and not rep["cost"].any() and not rep["n_obs"].any() and not rep["normal"].any()
    want = ctx.refine_cameras(x, kp, **kw)
    ctx.close()
    # CameraGroup.refine_poses: a NEW group with the refined poses, the original untouched
    group = api.CameraGroup(cap_ids=list(range(4)), resolutions=[(1280, 720)] * 4)
    for c, cam in enumerate(group.cameras):
        cam.K, cam.R, cam.t = np.array(cs["K"][c]), np.array(cs["Rd"][c]), np.array(cs["td"][c]).reshape(3, 1)
    new, rep = group.refine_poses(x, kp, diagnostics=True, **kw)
    assert new is not group and new.camera_num == 4 and rep["codes"].tolist() == [FIXED, MOVED, FIXED, MOVED]
    Kn, Rn, tn = new.rig_arrays()
    assert _same_bits(Rn, want[0]) and _same_bits(tn, want[1]) and _same_bits(Kn, np.ascontiguousarray(cs["K"]))
    assert new.cameras[1].t.shape == (3, 1) and _same_bits(group.rig_arrays()[1], np.ascontiguousarray(cs["Rd"]))


def test_entry_rejects_bad_arguments_on_a_real_context(api, tmp_path):
    """tests/abi_badargs_pose.c against libsnowtri.so on the GPU: every refusal that comes before a launch, the empty batch, a good call."""
    lib_dir = os.path.join(ROOT, "snowmocap_amd")
    exe = str(tmp_path / "abi_badargs_pose")
    subprocess.check_call(["gcc", "-std=c99", "-O1", "-I", os.path.join(ROOT, "include"), os.path.join(ROOT, "tests", "abi_badargs_pose.c"),
                           "-o", exe, "-L", lib_dir, "-lsnowtri", "-Wl,-rpath," + lib_dir])
    out = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0 and "0 failure(s)" in out.stdout, out.stdout[-3000:] + out.stderr[-2000:]


DBG_CODE = r'''
import sys, numpy as np
sys.path.insert(0, %(root)r)
sys.path.insert(0, %(tests)r)
import pose_cases as pc
from snowmocap_amd import _lib
assert _lib.LIB_PATH.endswith("libsnowtri_dbg.so") and "SNOWTRI_DEBUG_BOUNDS" in _lib.build_info()["variants"]
for rig_name, shape, dt in (("floor", (6, 2, 17), "float64"), ("ring8", (1, 1, 65), "float32"), ("ring16", (2, 3, 21), "float64"), ("ring3", (1, 1, 257), "float64")):
    cs = pc.case(rig_name, shape, 1.0, True, dt, dt)
    ctx = _lib.Context(cs["K"], cs["Rd"], cs["td"])
    R, t, rep = ctx.refine_cameras(cs["xyzs"], cs["kpts"], diagnostics=True, **cs["kw"])
    ref = pc.reference(rig_name, shape, 1.0, True, dt, dt)
    assert np.array_equal(rep["n_obs"], ref[2]["n_obs"]) and np.array_equal(rep["codes"], ref[2]["codes"])
    n, first = ctx.debug_faults()
    assert n == 0, "device-side bounds check failed %%d times; first: code %%d at line %%d" %% (n, first >> 32, first & 0xffffffff)
    ctx.close()
print("pose debug-bounds ok")
'''


def test_debug_build_counts_no_fault():
    dbg = os.path.join(ROOT, "snowmocap_amd", "libsnowtri_dbg.so")
    assert os.path.exists(dbg), f"{dbg} is missing: `make -C snowmocap_amd/csrc debug`"
    import sys
    env = dict(os.environ, SNOWTRI_LIB=dbg)
    code = DBG_CODE % {"root": ROOT, "tests": os.path.join(ROOT, "tests")}
    p = subprocess.run([sys.executable, "-c", code], env=env, capture_output=True, text=True, timeout=300)
    assert p.returncode == 0 and "pose debug-bounds ok" in p.stdout, (p.stdout[-2000:] + p.stderr[-3000:])


# ------------------------------------------------------------------------------------------------ the alternation
def test_refine_rig_against_the_rule_driven_alternation(api):
    """pose.refine_rig on the GPU (reprojection_cost, refine_joints and refine_cameras by their kernels) against the same alternation
    by the NumPy rules, both with pose_cases.dlt_points as the triangulation, after one round and after two: within the noisy bar."""
    rp = pc.recipe()
    bad = rp["bad"]
    args = (rp["K"], rp["Rd"], rp["td"], rp["kpts"])
    kw = dict(free=[bad], triangulate=pc.dlt_points, params=dict(keypoint_score_threshold=0.5))
    for rounds in (1, 2):
        R, t, hist = pose.refine_rig(*args, rounds=rounds, **kw)
        Rr, tr, hr = pose.refine_rig(*args, rounds=rounds, reference=True, **kw)
        eR, et = pc.pose_error(R, t, Rr, tr, [bad])
        print(f"    after round {rounds}: |R - R_rule| = {eR:.2e}, |t - t_rule| / rig scale = {et:.2e}; view RMS {hist[-1]['view_rms'][bad]:.3f} px")
        assert eR <= BAR_NOISY[0] and et <= BAR_NOISY[1], (rounds, eR, et)
        for h, g in zip(hist, hr):
            assert np.allclose(h["view_rms"], g["view_rms"], rtol=0, atol=1e-6)
            if "codes" in h:
                assert np.array_equal(h["codes"], g["codes"]) and np.array_equal(h["n_obs"], g["n_obs"])
        keep = [c for c in range(8) if c != bad]
        assert _same_bits(R[keep], np.ascontiguousarray(rp["Rd"][keep])) and _same_bits(t[keep], np.ascontiguousarray(rp["td"][keep]))


def test_refine_rig_with_the_library_triangulation_repairs_the_nudged_camera(api):
    """The whole alternation from the library's public pieces (BatchTriangulator with the DLT, reprojection_cost + match_detections,
    refine_joints, refine_cameras, a new context per round) on the recipe with ONE person (no association between the cameras, which
    a nudged camera upsets: pose.refine_rig's docstring): what tests/test_pose_host.py asserts of the rule-driven alternation."""
    rp = pc.recipe(P=1)
    bad = rp["bad"]
    R, t, hist = pose.refine_rig(rp["K"], rp["Rd"], rp["td"], rp["kpts"], free=[bad], rounds=2, method=_lib.DLT)
    rms = np.stack([h["view_rms"] for h in hist])
    others = np.delete(rms, bad, axis=1)
    print("    bad camera's view RMS per round:", np.round(rms[:, bad], 3), "others' median:", np.round(np.median(others, axis=1), 3),
          "overflow frames:", [h["overflow_frames"] for h in hist])
    assert all(isinstance(h["overflow_frames"], int) and 0 <= h["overflow_frames"] <= 40 for h in hist)
    assert rms[1, bad] < 0.5 * rms[0, bad] and rms[2, bad] <= 1.5 * np.median(others[2])
    assert np.abs(R[bad] - rp["R"][bad]).max() < np.abs(rp["Rd"][bad] - rp["R"][bad]).max()
