"""The Huber loss of "Refinement" and "Camera pose refinement" (include/snowtri.h, ROBUST LOSS) on the CPU: the NumPy rules
refine_joints_reference / refine_cameras_reference with huber_px, and what every layer does with the keyword before any GPU work.
Inputs: tests/huber_cases.py.  No GPU.

  (a) refusals of delta at every Python layer;
  (b) huber_px = None, 0 and 1e6 give the squared rule's outputs bit for bit;
  (c) the cost never rises; `outliers` and `n_outliers` are consistent with a recomputation at the output;
  (d) the accuracy floors huber_cases.JOINT_FLOOR and POSE_FLOOR are measured and asserted;
  (e) hand-made records: all views in the linear regime at X0, two views of which one is an outlier, a NaN pixel, a score below the
      threshold, a point behind a camera;
  (f) the public surface, and tests/abi_badargs_huber.c against the `make asan` library.
"""
import inspect
import os

import numpy as np
import pytest

import huber_cases as hc
import pose_cases as pc
import refine_cases as rc
from conftest import ROOT
from snowmocap_amd import pose
from snowmocap_amd import refine as rf

MISSING, FEW, KEPT, MOVED = rf.REFINE_MISSING, rf.REFINE_FEW_VIEWS, rf.REFINE_KEPT, rf.REFINE_MOVED
BAD_DELTAS = (-1.0, -0.0 - 1e-300, float("nan"), float("inf"), -float("inf"), 1.0000001e150)


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint8)


def _holds(measured, committed):
    """A committed floor still describes what is measured: neither has left the other by more than a factor of two."""
    return 0.5 * committed <= measured <= 2.0 * committed


def _joint_rule(cs, start="dlt", **kw):
    return rf.refine_joints_reference(cs["K"], cs["R"], cs["t"], cs[start], cs["kpts"], return_views=True, **rc.refine_kwargs(cs), **kw)


# ------------------------------------------------------------------------------------------------ (a) refusals
def test_every_layer_refuses_a_bad_delta():
    from snowmocap_amd import _lib
    cs = hc.joint_case("ring5", (2, 3, 21))
    ps = hc.pose_case("ring5", (2, 3, 21))
    rp_ = pc.recipe()
    for bad in BAD_DELTAS:
        with pytest.raises(ValueError, match="huber_px"):
            rf.check_huber(bad)
        with pytest.raises(ValueError, match="huber_px"):
            _lib.Context._huber(bad)
        with pytest.raises(ValueError, match="huber_px"):
            rf.refine_args((4, 6.0, False, bad))
        with pytest.raises(ValueError, match="huber_px"):
            _joint_rule(cs, huber_px=bad)
        with pytest.raises(ValueError, match="huber_px"):
            pose.refine_cameras_reference(ps["K"], ps["Rd"], ps["td"], ps["xyzs"], ps["kpts"], huber_px=bad, **ps["kw"])
        with pytest.raises(ValueError, match="huber_px"):
            pose.refine_rig(rp_["K"], rp_["Rd"], rp_["td"], rp_["kpts"], free=[rp_["bad"]], triangulate=pc.dlt_points, reference=True,
                            huber_px=bad)
    for ok, want in ((None, None), (0, None), (0.0, None), (-0.0, None), (3, 3.0), (1e150, 1e150), (5e-324, 5e-324)):
        assert rf.check_huber(ok) == want and _lib.Context._huber(ok) == want
    assert rf.refine_args((4, 6.0, False, 3)) == (4, 6.0, False, 3.0)
    assert rf.refine_args((4, 6.0, False, None)) == rf.refine_args((4, 6.0, False, 0)) == rf.refine_args((4, 6.0, False)) == (4, 6.0, False)
    assert rf.refine_args(4) == (4, 6.0, False) and rf.refine_args(None) is None
    for bad in ((4, 6.0), (4, 6.0, False, 3.0, 1), (0, 6.0, False, 3.0), (4, -1.0, False, 3.0)):
        with pytest.raises(ValueError):
            rf.refine_args(bad)


# ------------------------------------------------------------------------------------------------ (b) the squared rule's bits
@pytest.mark.parametrize("rec_dtype", ["float64", "float32"])
@pytest.mark.parametrize("rig_name", rc.RIGS)
def test_none_0_and_1e6_are_the_squared_rule_bit_for_bit_joints(rig_name, rec_dtype):
    moved = 0
    for shape in rc.SHAPES:
        cs = hc.joint_case(rig_name, shape, rec_dtype)
        for start in rc.STARTS:
            for sw in (False, True):
                base = _joint_rule(cs, start, score_weights=sw)
                assert len(base) == 4
                for d in (None, 0, 0.0):
                    same = _joint_rule(cs, start, score_weights=sw, huber_px=d)
                    assert len(same) == 4 and all(np.array_equal(_bits(a), _bits(b)) for a, b in zip(same, base)), (shape, start, d)
                big = _joint_rule(cs, start, score_weights=sw, huber_px=hc.BIG_DELTA)
                assert len(big) == 5 and big[4].dtype == np.uint32 and not big[4].any()
                assert all(np.array_equal(_bits(a), _bits(b)) for a, b in zip(big, base)), (shape, start)
                moved += int((base[2] == MOVED).sum())
    assert moved > 1000


@pytest.mark.parametrize("rig_name", rc.RIGS)
def test_none_0_and_1e6_are_the_squared_rule_bit_for_bit_cameras(rig_name):
    moved = 0
    for shape in pc.SHAPES:
        cs = hc.pose_case(rig_name, shape)
        args = (cs["K"], cs["Rd"], cs["td"], cs["xyzs"], cs["kpts"])
        base = pose.refine_cameras_reference(*args, **cs["kw"])
        for d in (None, 0, hc.BIG_DELTA):
            R, t, rep = pose.refine_cameras_reference(*args, huber_px=d, **cs["kw"])
            assert np.array_equal(_bits(R), _bits(base[0])) and np.array_equal(_bits(t), _bits(base[1])), (shape, d)
            assert ("n_outliers" in rep) == (d == hc.BIG_DELTA) and set(rep) - {"n_outliers"} == set(base[2])
            for key in base[2]:
                assert np.array_equal(_bits(rep[key]), _bits(base[2][key])), (shape, d, key)
            if d:
                assert rep["n_outliers"].dtype == np.int64 and not rep["n_outliers"].any()
        moved += int((base[2]["codes"] == pose.POSE_MOVED).sum())
    assert moved > 0


# ------------------------------------------------------------------------------------------------ (c) costs and outliers
@pytest.mark.parametrize("rec_dtype", ["float64", "float32"])
@pytest.mark.parametrize("rig_name", rc.RIGS)
def test_cost_never_rises_and_outliers_are_the_regimes_at_the_output(rig_name, rec_dtype):
    """With float64 records `outliers` and cost[., 1] are rule_at's at the rule's own output, bit for bit; with float32 records the
    output is rounded after the regimes were taken, so only cost[., 0] is compared.  Copied records: the input's bits, no outliers,
    the squared rule's codes -- the view set and the at-least-two-views clause do not know the loss."""
    flagged = refined = 0
    for shape in rc.SHAPES:
        cs = hc.joint_case(rig_name, shape, rec_dtype)
        sq = _joint_rule(cs)
        for delta in hc.DELTAS:
            for start in rc.STARTS:
                out, cost, codes, used, outl = hc.joint_reference(rig_name, shape, start, delta, rec_dtype)
                x = cs[start]
                copied = codes < KEPT
                assert (cost[..., 1] <= cost[..., 0]).all() and (cost[copied] == 0).all() and not outl[copied].any()
                assert out.dtype == x.dtype and np.array_equal(_bits(out[copied]), _bits(x[copied]))
                if start == "dlt":
                    assert np.array_equal(codes < KEPT, sq[2] < KEPT) and np.array_equal(codes[copied], sq[2][copied]) and np.array_equal(used, sq[3])
                assert not (outl & ~used).any() and (hc.popcount(used)[~copied] >= 2).all()
                e_in, _, _ = hc.rule_at(cs, start, x, used, delta)
                assert np.array_equal(_bits(e_in[~copied]), _bits(cost[..., 0][~copied]))
                if rec_dtype == "float64":
                    e_out, lin, _ = hc.rule_at(cs, start, out, used, delta)
                    assert np.array_equal(_bits(e_out[~copied]), _bits(cost[..., 1][~copied])) and np.array_equal(lin[~copied], outl[~copied])
                refined += int((~copied).sum())
                flagged += int((outl != 0).sum())
    assert refined > 1000 and flagged > 100


@pytest.mark.parametrize("rig_name", rc.RIGS)
def test_camera_cost_never_rises_and_n_outliers_is_the_count_at_the_output(rig_name):
    seen = 0
    for shape in pc.SHAPES:
        cs = hc.pose_case(rig_name, shape)
        for delta in hc.DELTAS:
            R, t, rep, S = hc.pose_reference(rig_name, shape, delta)
            sq = pose.refine_cameras_reference(cs["K"], cs["Rd"], cs["td"], cs["xyzs"], cs["kpts"], **cs["kw"])[2]
            still = rep["codes"] < pose.POSE_KEPT
            assert np.array_equal(rep["n_obs"], sq["n_obs"]) and np.array_equal(still, sq["codes"] < pose.POSE_KEPT)
            assert (rep["cost"][:, 1] <= rep["cost"][:, 0]).all() and not rep["n_outliers"][still].any() and not rep["cost"][still].any()
            assert np.array_equal(_bits(R[still]), _bits(cs["Rd"][still])) and np.array_equal(_bits(t[still]), _bits(cs["td"][still]))
            for c in np.nonzero(~still)[0]:
                X, ou, ov, w = hc.camera_observations(cs, S, c)
                assert rep["n_outliers"][c] == int(pose.linear_regime(cs["K"][c], R[c], t[c], X, ou, ov, delta).sum())
                assert pose.evaluate_camera(cs["K"][c], R[c], t[c], X, ou, ov, w, delta)[0][0] == rep["cost"][c, 1]
                seen += int(rep["n_outliers"][c])
    assert seen > 0


# ------------------------------------------------------------------------------------------------ (d) the floors
def test_reference_against_the_exact_huber_minimiser():
    """Measured here (CPU, the NumPy rule, iters = 16, start "dlt", shape (2, 3, 21)), |reference - 50-digit minimiser| / rig scale
    over the covered records, and the covered share of the refined ones:
      ring5   delta 3: 6.7e-10, 89 %    delta 6: 1.3e-9,  89 %
      ring8   delta 3: 8.8e-10, 93 %    delta 6: 2.8e-7,  95 %
      ring16  delta 3: 5.6e-10, 99 %    delta 6: 5.7e-10, 99 %"""
    worst = 0.0
    for rig_name in hc.ACCURACY_RIGS:
        scale = rc.rig_scale(rc.rig(rig_name)[2])
        for delta in hc.DELTAS:
            mn = hc.joint_minimiser(rig_name, delta)
            out = hc.joint_reference(rig_name, hc.ACCURACY_SHAPE, "dlt", delta, iters=hc.ACCURACY_ITERS)[0]
            share = mn["covered"].sum() / mn["refined"].sum()
            d = float((np.linalg.norm(out[..., :3] - mn["X"], axis=-1)[mn["covered"]] / scale).max())
            print(f"    {rig_name} delta {delta}: {d:.3e} of the rig scale over {int(mn['covered'].sum())} covered records ({share:.0%} of the refined)")
            assert share >= hc.MIN_COVERED, (rig_name, delta, share)
            worst = max(worst, d)
    assert _holds(worst, hc.JOINT_FLOOR), (worst, hc.JOINT_FLOOR)


def test_camera_reference_against_the_exact_huber_minimiser():
    wR = wt = 0.0
    for rig_name in hc.POSE_MINIMISER_RIGS:
        for delta in hc.DELTAS:
            mn = hc.pose_minimiser(rig_name, delta)
            R, t, rep, _ = hc.pose_reference(rig_name, hc.POSE_MINIMISER_SHAPE, delta)
            cams = list(mn["cams"])
            assert cams and (rep["codes"][cams] == pose.POSE_MOVED).all()
            eR, et = pc.pose_error(R, t, mn["R"], mn["t"], cams)
            print(f"    {rig_name} delta {delta}: |R - R_min| = {eR:.3e}, |t - t_min| / rig scale = {et:.3e}, steps {rep['steps'][cams].tolist()}")
            wR, wt = max(wR, eR), max(wt, et)
    assert _holds(wR, hc.POSE_FLOOR[0]) and _holds(wt, hc.POSE_FLOOR[1]), (wR, wt, hc.POSE_FLOOR)


def test_normal_equations_of_the_loss_against_50_digit_sums():
    worst = 0.0
    for rig_name in hc.POSE_MINIMISER_RIGS:
        cs = hc.pose_case(rig_name, hc.POSE_MINIMISER_SHAPE)
        for delta in hc.DELTAS:
            _, _, rep, S = hc.pose_reference(rig_name, hc.POSE_MINIMISER_SHAPE, delta)
            for c in range(min(cs["K"].shape[0], 5)):
                X, ou, ov, w = hc.camera_observations(cs, S, c)
                val, mag = hc.exact_huber_normal(cs["K"][c], cs["Rd"][c], cs["td"][c], X, ou, ov, w, delta)
                worst = max(worst, float((np.abs(rep["normal"][c] - val) / (pc.EPS * mag)).max()))
    print(f"    the rule's E, g, H of the loss within {worst:.1f} eps * sum |term| of the 50-digit sums")
    assert worst <= pc.NORMAL_UNITS, worst


# ------------------------------------------------------------------------------------------------ (e) hand-made records
@pytest.mark.parametrize("delta", hc.DELTAS)
def test_a_record_whose_views_are_all_linear_at_the_start(delta):
    """Every observation of joint 0 is 40 px off in its own direction: all of its views are in the linear regime at X0, kappa < 1 for
    all of them, H stays positive definite (IRLS weights), the record is refined like any other and its cost does not rise."""
    cs = hc.all_linear_case()
    out, cost, codes, used, outl = _joint_rule(cs, huber_px=delta)
    C = cs["K"].shape[0]
    _, lin0, _ = hc.rule_at(cs, "dlt", cs["dlt"], used, delta)
    assert used[0, 0, 0] == (1 << C) - 1 and lin0[0, 0, 0] == (1 << C) - 1
    assert (codes == MOVED).all() and (cost[..., 1] < cost[..., 0]).all()
    assert not outl[0, 0, 1:].any() and hc.popcount(outl[0, 0, 0]) >= C - 1        # no point fits C views thrown 40 px apart
    assert np.abs(out[0, 0, 1:, :3] - cs["X"][0, 0, 1:]).max() < 0.01


@pytest.mark.parametrize("delta", hc.DELTAS)
def test_two_views_of_which_one_is_an_outlier(delta):
    """|V| = 2 is counted whatever the regimes are: the record is refined (not FEW_VIEWS), its cost does not rise, and afterwards
    popcount(V & ~outliers) says whether the inliers fix its point -- with two views a point exists that fits both to a pixel, so the
    loss cannot tell which of the two is wrong."""
    cs = hc.two_views_case()
    out, cost, codes, used, outl = rf.refine_joints_reference(cs["K"], cs["R"], cs["t"], cs["dlt"], cs["kpts"], views=cs["views"],
                                                              keypoint_score_threshold=cs["thr"], return_views=True, huber_px=delta, iters=16)
    assert used[0, 0, 0] == 3 and codes[0, 0, 0] >= KEPT and cost[0, 0, 0, 1] <= cost[0, 0, 0, 0]
    assert (codes[0, 0, 1:] == MOVED).all() and not outl[0, 0, 1:].any()
    e_out, lin, _ = hc.rule_at(cs, "dlt", out, used, delta)
    assert lin[0, 0, 0] == outl[0, 0, 0] and e_out[0, 0, 0] == cost[0, 0, 0, 1]


@pytest.mark.parametrize("delta", hc.DELTAS)
def test_nan_pixels_low_scores_and_a_point_behind_a_camera(delta):
    """The view set does not know the loss: a NaN pixel and a score below the threshold leave the set, a point behind camera 0 loses
    that view (refine_cases.behind_case), and with every view gone but one the record is FEW_VIEWS and copied bit for bit."""
    cs = rc.behind_case("ring5")
    C = cs["K"].shape[0]
    kp = np.array(cs["kpts"], copy=True)
    kp[0, 1, 0, 1, 0] = np.nan                   # joint 1: camera 1 has a NaN u
    kp[0, 2, 0, 2, 2] = 0.25                     # joint 2: camera 2 scores below the threshold
    kp[0, 1:, 0, 3, 1] = np.nan                  # joint 3: only camera 0 is left
    kp[0, 3, 0, 2, 0] += 90.0                    # ... and an outlier among joint 2's views
    args = (cs["K"], cs["R"], cs["t"], cs["dlt"], kp)
    out, cost, codes, used, outl = rf.refine_joints_reference(*args, keypoint_score_threshold=cs["thr"], return_views=True, huber_px=delta)
    sq = rf.refine_joints_reference(*args, keypoint_score_threshold=cs["thr"], return_views=True)
    full = (1 << C) - 1
    assert used[0, 0].tolist() == [full & ~1, full & ~2, full & ~4, 0] and np.array_equal(used, sq[3])
    assert codes[0, 0].tolist() == [MOVED, MOVED, MOVED, FEW] and np.array_equal(codes < KEPT, sq[2] < KEPT)
    assert np.array_equal(_bits(out[0, 0, 3]), _bits(cs["dlt"][0, 0, 3])) and not cost[0, 0, 3].any() and outl[0, 0, 3] == 0
    assert outl[0, 0, 2] == 8 and (cost[..., 1] <= cost[..., 0]).all()
    assert np.linalg.norm(out[0, 0, 2, :3] - cs["X"][0, 0, 2]) < np.linalg.norm(sq[0][0, 0, 2, :3] - cs["X"][0, 0, 2])


def test_the_loss_brings_the_poses_closer_to_the_truth():
    """What the issue's prototype measured, on pose_cases.case shapes with the outliers: the squared loss leaves the free cameras
    1e-2 .. 6e-2 from the truth, the Huber loss several times closer, and iters = 8 and 16 give the same pose."""
    for rig_name in ("floor", "ring8"):
        cs = hc.pose_case(rig_name, (6, 2, 17))
        args = (cs["K"], cs["Rd"], cs["td"], cs["xyzs"], cs["kpts"])
        free = [c for c in cs["free"]]
        sq = pose.refine_cameras_reference(*args, **cs["kw"])
        e_sq = pc.pose_error(sq[0], sq[1], cs["R"], cs["t"], free)
        for delta in hc.DELTAS:
            hb = pose.refine_cameras_reference(*args, huber_px=delta, **cs["kw"])
            hb16 = pose.refine_cameras_reference(*args, huber_px=delta, **{**cs["kw"], "iters": 16})
            e_hb = pc.pose_error(hb[0], hb[1], cs["R"], cs["t"], free)
            print(f"    {rig_name} delta {delta}: squared {e_sq[0]:.2e} {e_sq[1]:.2e}, huber {e_hb[0]:.2e} {e_hb[1]:.2e}, steps {hb[2]['steps'][free].tolist()}")
            assert e_hb[0] < 0.5 * e_sq[0] and e_hb[1] < 0.5 * e_sq[1]
            assert np.array_equal(_bits(hb[0]), _bits(hb16[0])) and np.array_equal(_bits(hb[1]), _bits(hb16[1]))


# ------------------------------------------------------------------------------------------------ (f) the surface
def test_public_surface():
    import snowmocap_amd.pipeline as pl
    from snowmocap_amd import _lib
    from snowmocap_amd.camera import CameraGroup
    assert {"snowtri_refine_joints_ex", "snowtri_refine_cameras_ex"} <= set(_lib.exported_symbols())
    for fn in (_lib.Context.refine_joints, _lib.Context.refine_cameras, rf.refine_joints, rf.refine_joints_reference, pose.refine_cameras,
               pose.refine_cameras_reference, pose.refine_rig):
        assert inspect.signature(fn).parameters["huber_px"].default is None, fn
    assert "huber_px" in CameraGroup.refine_poses.__doc__ and "huber_px" in pl.TrackPipeline.run.__doc__
    hdr = open(os.path.join(ROOT, "include", "snowtri.h")).read()
    for word in ("ROBUST LOSS", "snowtri_refine_joints_ex", "snowtri_refine_cameras_ex", "huber_px", "n_outliers", "popcount(V & ~outliers) < 2",
                 "1e150", "Cauchy"):
        assert word in hdr, word
    assert "a robust loss (pass the `views` mask" not in hdr and "Huber / IRLS: outliers are the business" not in hdr


def test_entries_reject_bad_arguments_without_a_gpu(tmp_path):
    """`make asan` + tests/abi_badargs_huber.c, built and run exactly as tests/test_refine_host.py does for
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
    exe = str(tmp_path / "abi_badargs_huber")
    subprocess.check_call([clang, "-std=c99", "-fsanitize=address", "-g", "-I", os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "tests", "abi_badargs_huber.c"), "-o", exe, so, "-Wl,-rpath," + os.path.dirname(so)])
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=0:abort_on_error=0", HIP_VISIBLE_DEVICES="", ROCR_VISIBLE_DEVICES="")
    p = subprocess.run([exe], env=env, capture_output=True, text=True, timeout=120)
    assert p.returncode == 0 and "0 failure(s)" in p.stdout, p.stdout[-3000:] + p.stderr[-3000:]
    assert "AddressSanitizer" not in p.stderr, p.stderr[-3000:]
