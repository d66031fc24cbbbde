"""Camera pose refinement on the host (no GPU): the NumPy rule (snowmocap_amd/pose.py::refine_cameras_reference) against the
consequences of the rule of include/snowtri.h ("Camera pose refinement"), against exact arithmetic, and the C entry refusing bad
arguments under AddressSanitizer.

  (a) the rule's analytic Jacobian against central differences of its own projection;
  (b) exact detections, a drifted rig: the rule returns to the true pose -- FLOOR_EXACT of tests/pose_cases.py, measured here over
      the six rigs and six placements;
  (c) sigma 1 and 2 px: its distance to the 50-digit minimiser over the same six parameters and the same S_c -- FLOOR_NOISY;
  (d) its E, g and H at the input pose and at the pose it ends at against 50-digit sums, in units of eps * sum |term| -- NORMAL_UNITS;
  (e) codes: FIXED and FEW_OBS poses are bit copies, the cost never rises, S_c is the per-view part of refine_joints' view set;
  (f) argument checking, and tests/abi_badargs_pose.c against the `make asan` library;
  (g) refine_rig, driven by the NumPy rules, on the recipe of the README.
"""
import os

import numpy as np
import pytest

import pose_cases as pc
import refine_cases as rc
from conftest import ROOT
from snowmocap_amd import pose
from snowmocap_amd.refine import refine_joints_reference

FIXED, FEW, KEPT, MOVED = pose.POSE_FIXED, pose.POSE_FEW_OBS, pose.POSE_KEPT, pose.POSE_MOVED


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint8)


def _holds(measured, committed):
    """A committed floor still describes what is measured: neither has left the other by more than a factor of two."""
    return committed / 2 <= measured <= 2 * committed


# ------------------------------------------------------------------------------------------------ (a) the Jacobian
@pytest.mark.parametrize("rig_name", pc.RIGS)
def test_jacobian_against_central_differences(rig_name):
    cs = pc.case(rig_name, pc.EXACT_SHAPE, 0.0, False)
    X = cs["xyzs"][..., :3].reshape(-1, 3)
    worst = 0.0
    for c in range(cs["K"].shape[0]):
        Kc, Rc, tc = cs["K"][c], cs["Rd"][c], cs["td"][c]
        du, dv = pose.pose_jacobian(Kc, Rc, tc, X)
        for k in range(6):
            h = 1e-6
            d = np.zeros(6)
            d[k] = h
            up = pose.project_camera(Kc, *pose.apply_delta(Rc, tc, d), X)
            um = pose.project_camera(Kc, *pose.apply_delta(Rc, tc, -d), X)
            # central differences: truncation h^2 |f'''| / 6 and rounding eps |u| / h, both far below 1e-6 of the derivative
            worst = max(worst, float(np.abs((up[3] - um[3]) / (2 * h) - du[:, k]).max() / np.abs(du[:, k]).max()),
                        float(np.abs((up[4] - um[4]) / (2 * h) - dv[:, k]).max() / max(np.abs(dv[:, k]).max(), np.abs(du[:, k]).max())))
    print(f"    {rig_name}: analytic Jacobian vs central differences, relative: {worst:.2e}")
    assert worst < 1e-6


def test_exp_is_a_rotation_and_the_identity_at_zero():
    assert np.array_equal(pose.rodrigues(np.zeros(3)), np.eye(3))
    rng = np.random.default_rng(5)
    for th in (1e-300, 1e-12, 1e-6, 0.01, 1.0, 3.0):
        ax = rng.normal(size=3)
        E = pose.rodrigues(ax / np.linalg.norm(ax) * th)
        assert np.abs(E.T @ E - np.eye(3)).max() < 8 * pc.EPS and abs(np.linalg.det(E) - 1) < 8 * pc.EPS
        assert abs(np.arccos(np.clip((np.trace(E) - 1) / 2, -1, 1)) - th) < 1e-7 * max(th, 1e-9) + 3e-8


# ------------------------------------------------------------------------------------------------ (b) exact detections
def test_exact_detections_return_to_the_true_pose():
    wR = wt = 0.0
    where = None
    for rig_name in pc.RIGS:
        for placement in pc.PLACEMENTS:
            cs = pc.case(rig_name, pc.EXACT_SHAPE, 0.0, True, placement=placement)
            R, t, rep, _ = pc.reference(rig_name, pc.EXACT_SHAPE, 0.0, True, placement=placement)
            moved = [c for c in cs["free"] if rep["codes"][c] == MOVED]
            assert moved == [c for c in cs["free"] if rep["n_obs"][c] >= pc.MIN_OBS] and len(moved) == len(cs["free"])
            eR, et = pc.pose_error(R, t, cs["R"], cs["t"], moved)
            if et > wt:
                where = (rig_name, placement)
            wR, wt = max(wR, eR), max(wt, et)
            assert rep["cost"][moved, 1].max() < 1e-12                                        # px^2: nothing but rounding is left
    print(f"    exact detections: max |R - R_true| = {wR:.3e}, max |t - t_true| / rig scale = {wt:.3e} at {where}")
    assert _holds(wR, pc.FLOOR_EXACT[0]) and _holds(wt, pc.FLOOR_EXACT[1]), (wR, wt)


# ------------------------------------------------------------------------------------------------ (c) the exact minimiser
def test_reference_against_the_exact_minimiser():
    wR = wt = 0.0
    for rig_name in pc.RIGS:
        for sigma in (1.0, 2.0):
            cs = pc.case(rig_name, pc.MINIMISER_SHAPE, sigma, True)
            mn = pc.minimiser(rig_name, sigma)
            R, t, rep, _ = pc.reference(rig_name, pc.MINIMISER_SHAPE, sigma, True)
            cams = list(mn["cams"])
            assert cams and (rep["codes"][cams] == MOVED).all()
            eR, et = pc.pose_error(R, t, mn["R"], mn["t"], cams)
            wR, wt = max(wR, eR), max(wt, et)
            # the minimiser's cost is the smallest there is; the rule's end cost agrees with it to the rounding of its pixels
            # (b = 2.5e-12 px each, tests/test_reproject_host.py): |dE| <= 2 sqrt(2) b sqrt(n E), as in tests/test_refine_host.py
            e1, em, n = rep["cost"][cams, 1], mn["E"][cams], rep["n_obs"][cams]
            tol = 2 * np.sqrt(2) * 2.5e-12 * np.sqrt(n * em) + 64 * pc.EPS * em
            assert (np.abs(e1 - em) <= tol).all(), (e1 - em, tol)
            print(f"    {rig_name} sigma {sigma}: |R - R*| = {eR:.3e}, |t - t*| / rig scale = {et:.3e}")
    print(f"    noisy detections: max |R - R*| = {wR:.3e}, max |t - t*| / rig scale = {wt:.3e}")
    assert _holds(wR, pc.FLOOR_NOISY[0]) and _holds(wt, pc.FLOOR_NOISY[1]), (wR, wt)


# ------------------------------------------------------------------------------------------------ (d) the normal equations
def test_normal_equations_against_50_digit_sums():
    worst = 0.0
    for rig_name in pc.RIGS:
        cs = pc.case(rig_name, pc.MINIMISER_SHAPE, 1.0, True)
        Ro, to, rep, S = pc.reference(rig_name, pc.MINIMISER_SHAPE, 1.0, True)
        for c in range(min(cs["K"].shape[0], 5)):              # fixed cameras too: `normal` is reported for every camera
            X, ou, ov, w = pc.camera_observations(cs, S, c)
            val, mag = pc.exact_normal(cs["K"][c], cs["Rd"][c], cs["td"][c], X, ou, ov, w)
            assert rep["n_obs"][c] == len(X) > 0 and (mag > 0).all()
            worst = max(worst, float((np.abs(rep["normal"][c] - val) / (pc.EPS * mag)).max()))
            if rep["codes"][c] == MOVED:                       # ... and the sums at the pose the rule ends at (cost[., 1] is its E)
                val, mag = pc.exact_normal(cs["K"][c], Ro[c], to[c], X, ou, ov, w)
                end = pose.evaluate_camera(cs["K"][c], Ro[c], to[c], X, ou, ov, w)[0]
                assert end[0] == rep["cost"][c, 1]
                worst = max(worst, float((np.abs(end - val) / (pc.EPS * mag)).max()))
    print(f"    the reference's E, g, H against 50-digit sums: {worst:.3e} eps * sum |term|")
    assert _holds(worst, pc.NORMAL_UNITS), worst


# ------------------------------------------------------------------------------------------------ (e) codes and consequences
@pytest.mark.parametrize("rig_name", pc.RIGS)
def test_codes_bit_copies_and_the_cost_never_rises(rig_name):
    seen = np.zeros(4, dtype=np.int64)
    for shape in pc.SHAPES:
        for sigma in (0.0, 1.0):
            for rec_dtype in ("float64", "float32"):
                if rec_dtype == "float32" and shape[2] > 65:
                    continue
                cs = pc.case(rig_name, shape, sigma, True, rec_dtype)
                R, t, rep, S = pc.reference(rig_name, shape, sigma, True, rec_dtype)
                C = cs["K"].shape[0]
                codes, cost = rep["codes"], rep["cost"]
                assert np.array_equal(rep["n_obs"], S.sum(axis=1)) and np.isfinite(cost).all() and (cost[:, 1] <= cost[:, 0]).all()
                for c in range(C):
                    if c not in cs["free"]:
                        assert codes[c] == FIXED
                    elif rep["n_obs"][c] < pc.MIN_OBS:
                        assert codes[c] == FEW
                    else:
                        assert codes[c] in (KEPT, MOVED)
                    if codes[c] != MOVED:
                        assert np.array_equal(_bits(R[c]), _bits(cs["Rd"][c])) and np.array_equal(_bits(t[c]), _bits(cs["td"][c]))
                        assert cost[c, 0] == cost[c, 1] and (codes[c] == KEPT or cost[c, 0] == 0.0)
                    else:
                        assert cost[c, 1] < cost[c, 0] and np.abs(R[c].T @ R[c] - np.eye(3)).max() < 64 * pc.EPS
                    assert rep["normal"][c, 0] == cost[c, 0] or codes[c] in (FIXED, FEW)
                seen += np.bincount(codes, minlength=4)
                # S_c is the per-view part of refine_joints' view set: wherever that rule keeps a record, its mask is S's column
                used = refine_joints_reference(cs["K"], cs["Rd"], cs["td"], cs["xyzs"], cs["kpts"], det_of=cs["det_of"],
                                               n_persons=cs["n_persons"], views=cs["views"], keypoint_score_threshold=cs["thr"],
                                               iters=1, return_views=True)[3].reshape(-1)
                mask = np.zeros(S.shape[1], dtype=np.uint32)
                for c in range(C):
                    mask |= S[c].astype(np.uint32) << np.uint32(c)
                kept = used != 0
                assert np.array_equal(mask[kept], used[kept]) and (S[:, ~kept].sum(axis=0) < 2).all()
    assert (seen[[FIXED, FEW, MOVED]] > 0).all(), seen


def test_iters_one_is_the_first_step_and_weights_count():
    cs = pc.case("floor", (6, 2, 17), 1.0, True)
    kw = dict(cs["kw"])
    full = pose.refine_cameras_reference(cs["K"], cs["Rd"], cs["td"], cs["xyzs"], cs["kpts"], **kw)
    kw["iters"] = 1
    one = pose.refine_cameras_reference(cs["K"], cs["Rd"], cs["td"], cs["xyzs"], cs["kpts"], **kw)
    assert (one[2]["steps"] <= 1).all() and (one[2]["cost"][:, 1] >= full[2]["cost"][:, 1]).all()
    assert np.array_equal(one[2]["normal"], full[2]["normal"]) and np.array_equal(one[2]["cost"][:, 0], full[2]["cost"][:, 0])
    kw = dict(cs["kw"], score_weights=True)
    wtd = pose.refine_cameras_reference(cs["K"], cs["Rd"], cs["td"], cs["xyzs"], cs["kpts"], **kw)
    assert np.array_equal(wtd[2]["n_obs"], full[2]["n_obs"]) and not np.array_equal(wtd[0], full[0])
    # free as a mask, as booleans and as indices is the same thing; None frees every camera
    C = cs["K"].shape[0]
    assert pose.free_mask([1, 3], C) == pose.free_mask(0b1010, C) == pose.free_mask([False, True, False, True], C) == 10
    assert pose.free_mask(None, C) == 15 and pose.free_mask([], C) == 0


def test_the_empty_batch_copies_every_pose():
    cs = pc.case("ring5", (1, 1, 8), 0.0, False)
    x, kp = np.zeros((0, 1, 8, 4)), np.zeros((0, 5, 1, 8, 3))
    R, t, rep = pose.refine_cameras_reference(cs["K"], cs["Rd"], cs["td"], x, kp, free=[1, 3], min_obs=3, iters=2)
    assert np.array_equal(_bits(R), _bits(cs["Rd"])) and np.array_equal(_bits(t), _bits(cs["td"]))
    assert rep["codes"].tolist() == [FIXED, FEW, FIXED, FEW, FIXED] and not rep["cost"].any() and not rep["n_obs"].any()
    assert not rep["normal"].any()


# ------------------------------------------------------------------------------------------------ (f) arguments
def test_argument_checking():
    cs = pc.case("floor", (3, 1, 17), 1.0, False)
    K, R, t, x, kp = cs["K"], cs["Rd"], cs["td"], cs["xyzs"], cs["kpts"]
    for bad in (dict(iters=0), dict(iters=17), dict(iters=2.5), dict(min_obs=2), dict(min_obs=3.5), dict(free=[4]), dict(free=16),
                dict(free=[True, False]), dict(keypoint_score_threshold=float("nan"))):
        with pytest.raises(ValueError):
            pose.refine_cameras_reference(K, R, t, x, kp, **bad)
    with pytest.raises(ValueError):
        pose.refine_cameras_reference(K, R, t, x[..., :3], kp)
    with pytest.raises(ValueError):
        pose.refine_cameras_reference(K, R, t, x, kp[:, :3])
    with pytest.raises(ValueError):
        pose.refine_cameras_reference(K, R, t, np.concatenate([x, x], axis=1), kp)            # P = 2 > Pmax = 1 without det_of
    Kbad = np.array(K, copy=True)
    Kbad[0, 1, 0] = 1e-3
    with pytest.raises(ValueError):
        pose.refine_cameras_reference(Kbad, R, t, x, kp)
    tri = lambda *a: None
    for bad in (dict(free=None), dict(free=[0, 1, 2, 3]), dict(free=[1], rounds=0), dict(free=[1], reference=True, triangulate=None)):
        with pytest.raises(ValueError):
            pose.refine_rig(K, R, t, kp, **dict(dict(triangulate=tri, reference=True), **bad))
    import inspect
    import snowmocap_amd
    import snowmocap_amd.pipeline as pl
    from snowmocap_amd import _lib
    from snowmocap_amd.camera import CameraGroup
    assert snowmocap_amd.refine_cameras is pose.refine_cameras and snowmocap_amd.refine_rig is pose.refine_rig
    assert {"refine_cameras", "refine_cameras_reference", "refine_rig"} <= set(snowmocap_amd.__all__)
    assert {"snowtri_refine_cameras", "snowtri_pose_sweep_records"} <= set(_lib.exported_symbols())
    assert (_lib.POSE_FIXED, _lib.POSE_FEW_OBS, _lib.POSE_KEPT, _lib.POSE_MOVED) == (0, 1, 2, 3) and _lib.POSE_SWEEP_RECORDS == 262144
    assert callable(CameraGroup.refine_poses) and callable(_lib.Context.refine_cameras)
    assert "pose" not in inspect.signature(pl.TrackPipeline.run).parameters                  # calibration happens before a recording
    hdr = open(os.path.join(ROOT, "include", "snowtri.h")).read()
    for word in ("Camera pose refinement", "SNOWTRI_POSE_FIXED", "SNOWTRI_POSE_FEW_OBS", "SNOWTRI_POSE_KEPT", "SNOWTRI_POSE_MOVED",
                 "to rounding, not bit for", "ONE CALL MAY BE IN FLIGHT PER", "allocated by the FIRST call"):
        assert word in hdr, word


def test_pose_entry_rejects_bad_arguments_under_asan(tmp_path):
    """`make asan` + tests/abi_badargs_pose.c, built and run exactly as tests/test_refine_host.py does for
    tests/abi_badargs_refine.c: a stand-alone C program on the CPU (no device visible), nothing preloaded."""
    import glob
    import shutil
    import subprocess
    csrc = os.path.join(ROOT, "snowmocap_amd", "csrc")
    so = os.path.join(csrc, "build", "libsnowtri_asan.so")
    clang = "/opt/rocm/lib/llvm/bin/clang"
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    if not (os.path.exists(hipcc) or shutil.which("hipcc")) or not os.path.exists(clang):
        pytest.skip("no ROCm toolchain (hipcc + its clang) on this machine: the ASan build of the C ABI cannot be made")
    sources = glob.glob(os.path.join(csrc, "*.hip")) + glob.glob(os.path.join(csrc, "*.hpp")) + [os.path.join(ROOT, "include", "snowtri.h")]
    if not os.path.exists(so) or os.path.getmtime(so) < max(os.path.getmtime(f) for f in sources):   # (the target always rebuilds: ~1 min)
        subprocess.check_call(["make", "-C", csrc, "-s", "asan"])
    exe = str(tmp_path / "abi_badargs_pose")
    subprocess.check_call([clang, "-std=c99", "-fsanitize=address", "-g", "-I", os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "tests", "abi_badargs_pose.c"), "-o", exe, so, "-Wl,-rpath," + os.path.dirname(so)])
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=0:abort_on_error=0", HIP_VISIBLE_DEVICES="", ROCR_VISIBLE_DEVICES="")
    p = subprocess.run([exe], env=env, capture_output=True, text=True, timeout=120)
    assert p.returncode == 0 and "0 failure(s)" in p.stdout, p.stdout[-3000:] + p.stderr[-3000:]
    assert "AddressSanitizer" not in p.stderr, p.stderr[-3000:]


# ------------------------------------------------------------------------------------------------ (g) the alternation
def test_refine_rig_repairs_the_nudged_camera():
    """The recipe of the README (pose_cases.recipe: 8 cameras, 40 x 2 x 17 joints, 1 px, camera 3 off by 0.5 degrees / 2 cm and the
    only free one), every step by its NumPy rule.  Measured here, per round (before round 1 | after round 1 | after round 2):
      the bad camera's view RMS   3.898 | 1.552 | 1.317 px   (the other cameras: 1.347 .. 1.624 | 1.275 .. 1.342 | 1.268 .. 1.337 px)
      its |R - R_true|            7.46e-3 | 1.29e-3 | 9.85e-4
      its |t - t_true|            20.0 | 13.6 | 8.9 mm
    Asserted: the view RMS after round 1 is below half the RMS before, and after round 2 within 1.5 x the median of the others."""
    rp = pc.recipe()
    bad = rp["bad"]
    R, t, hist = pose.refine_rig(rp["K"], rp["Rd"], rp["td"], rp["kpts"], free=[bad], rounds=2, triangulate=pc.dlt_points, reference=True,
                                 params=dict(keypoint_score_threshold=0.5))
    assert len(hist) == 3 and R.shape == (8, 3, 3) and t.shape == (8, 3) and all(h["overflow_frames"] == 0 for h in hist)
    rms = np.stack([h["view_rms"] for h in hist])
    others = np.delete(rms, bad, axis=1)
    print("    bad camera's view RMS per round:", np.round(rms[:, bad], 3), "others:", np.round(others.min(axis=1), 3), "..",
          np.round(others.max(axis=1), 3))
    # (the pose error per round: one more alternation per prefix)
    errs = [(np.abs(rp["Rd"][bad] - rp["R"][bad]).max(), np.linalg.norm(rp["td"][bad] - rp["t"][bad]))]
    R1, t1, _ = pose.refine_rig(rp["K"], rp["Rd"], rp["td"], rp["kpts"], free=[bad], rounds=1, triangulate=pc.dlt_points, reference=True,
                                params=dict(keypoint_score_threshold=0.5))
    errs += [(np.abs(R1[bad] - rp["R"][bad]).max(), np.linalg.norm(t1[bad] - rp["t"][bad])),
             (np.abs(R[bad] - rp["R"][bad]).max(), np.linalg.norm(t[bad] - rp["t"][bad]))]
    print("    bad camera's |R - R_true|, |t - t_true| (m) per round:", [(f"{a:.2e}", f"{b:.2e}") for a, b in errs])
    assert rms[1, bad] < 0.5 * rms[0, bad]
    assert rms[2, bad] <= 1.5 * np.median(others[2])
    for h in hist[:2]:
        assert h["codes"][bad] == MOVED and (np.delete(h["codes"], bad) == FIXED).all() and h["cost"][bad, 1] < h["cost"][bad, 0]
    keep = [c for c in range(8) if c != bad]
    assert np.array_equal(_bits(R[keep]), _bits(rp["Rd"][keep])) and np.array_equal(_bits(t[keep]), _bits(rp["td"][keep]))
