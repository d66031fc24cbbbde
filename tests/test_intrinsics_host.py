"""Camera refinement with intrinsics on the host (no GPU): the NumPy rule (snowmocap_amd/pose.py::refine_cameras_reference with
intrinsics=...) against the consequences of the rule of include/snowtri.h ("Camera pose refinement", INTRINSICS), against exact
arithmetic, and the C entry refusing bad arguments under AddressSanitizer.

  (a) intrinsics=None is today's function, bit for bit; no camera in intrinsics_free is today's poses, bit for bit;
  (b) the four new Jacobian columns against central differences of the rule's own projection;
  (c) exact detections, a drifted rig with a drifted K: the rule returns to the true K, R, t -- FLOOR_EXACT_K of
      tests/intrinsics_cases.py, measured here over the six rigs and six placements;
  (d) sigma = 1 px: its distance to the 50-digit minimiser over the same ten parameters and the same S_c -- FLOOR_NOISY_K;
  (e) its E, g[10] and H[55] at the input and where it ends against 50-digit sums, in units of eps * sum |term| -- NORMAL_UNITS_K;
  (f) the parameter sets: codes, the parameters outside a camera's free set keep their bits, the cost never rises;
  (g) argument checking, and tests/abi_badargs_intrinsics.c against the `make asan` library;
  (h) refine_rig(intrinsics="fc"), driven by the NumPy rules, on a camera whose K is wrong and whose pose is right.
"""
import os

import numpy as np
import pytest

import intrinsics_cases as ic
import pose_cases as pc
from conftest import ROOT
from snowmocap_amd import pose

FIXED, FEW, KEPT, MOVED = pose.POSE_FIXED, pose.POSE_FEW_OBS, pose.POSE_KEPT, pose.POSE_MOVED


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint8)


def _same(a, b):
    a, b = np.asarray(a), np.asarray(b)
    return a.dtype == b.dtype and a.shape == b.shape and np.array_equal(_bits(a), _bits(b))


def _holds(measured, committed):
    """A committed floor still describes what is measured: neither has left the other by more than a factor of two."""
    return committed / 2 <= measured <= 2 * committed


# ------------------------------------------------------------------------------------------------ (a) off is off
@pytest.mark.parametrize("huber_px", [None, 3.0])
def test_intrinsics_none_is_todays_function_bit_for_bit(huber_px):
    for rig_name, shape in (("floor", (6, 2, 17)), ("ring5", (2, 3, 21))):
        cs = ic.case(rig_name, shape, 1.0, True)
        kw = dict(cs["kw"], huber_px=huber_px)
        del kw["intrinsics"], kw["intrinsics_free"]
        args = (cs["Kd"], cs["Rd"], cs["td"], cs["xyzs"], cs["kpts"])
        want = pose.refine_cameras_reference(*args, **kw)
        got = pose.refine_cameras_reference(*args, intrinsics=None, intrinsics_free=[1], **kw)
        assert len(got) == len(want) == 3 and _same(got[0], want[0]) and _same(got[1], want[1])
        assert got[2].keys() == want[2].keys() and all(_same(got[2][k], want[2][k]) for k in want[2])
        assert got[2]["normal"].shape == (cs["K"].shape[0], 28)
        # no camera in intrinsics_free: the ten-parameter rule takes today's steps on today's numbers
        K, R, t, rep = pose.refine_cameras_reference(*args, intrinsics="fc", intrinsics_free=[], **kw)
        assert _same(K, np.asarray(cs["Kd"])) and _same(R, want[0]) and _same(t, want[1])
        assert all(_same(rep[k], want[2][k]) for k in want[2] if k != "normal") and rep["normal"].shape == (cs["K"].shape[0], 66)
        assert _same(rep["normal"][:, :7], want[2]["normal"][:, :7]) and _same(rep["normal"][:, 11:32], want[2]["normal"][:, 7:])


# ------------------------------------------------------------------------------------------------ (b) the Jacobian
def test_intrinsic_columns_against_central_differences():
    cs = ic.case("floor", ic.EXACT_SHAPE, 0.0, False)
    X = cs["xyzs"][..., :3].reshape(-1, 3)
    worst = 0.0
    for c in range(cs["K"].shape[0]):
        Kc, Rc, tc = np.array(cs["Kd"][c]), cs["Rd"][c], cs["td"][c]
        ou = ov = np.zeros(len(X))
        terms, _ = pose.normal_terms_k(Kc, Rc, tc, X, ou, ov, np.ones(len(X)))
        _, _, _, u, v, _ = pose.project_camera(Kc, Rc, tc, X)
        # with a zero observation g[a] = du_a u + dv_a v per record: the columns are read back from it through two shifted copies
        for k, h in ((6, 1e-3), (7, 1e-3), (8, 1e-3), (9, 1e-3)):
            d = np.zeros(10)
            d[k] = h
            up = pose.project_camera(pose.apply_delta_k(Kc, Rc, tc, d, [k - k % 2, k - k % 2 + 1])[0], Rc, tc, X)
            um = pose.project_camera(pose.apply_delta_k(Kc, Rc, tc, -d, [k - k % 2, k - k % 2 + 1])[0], Rc, tc, X)
            du, dv = (up[3] - um[3]) / (2 * h), (up[4] - um[4]) / (2 * h)      # u and v are linear in the four: exact up to rounding
            worst = max(worst, float(np.abs(terms[:, 1 + k] - (du * u + dv * v)).max() / np.abs(terms[:, 1 + k]).max()))
    print(f"    the intrinsic columns of g vs central differences, relative: {worst:.2e}")
    assert worst < 1e-9


# ------------------------------------------------------------------------------------------------ (c) exact detections
def test_exact_detections_return_to_the_true_camera():
    worst, steps = [0.0] * 4, 0
    for rig_name in ic.RIGS:
        for placement in ic.PLACEMENTS:
            cs = ic.case(rig_name, ic.EXACT_SHAPE, 0.0, True, placement=placement)
            K, R, t, rep, _ = ic.reference(rig_name, ic.EXACT_SHAPE, 0.0, True, placement=placement)
            moved = [c for c in cs["free"] if rep["codes"][c] == MOVED]
            assert moved == list(cs["free"])
            worst = [max(a, b) for a, b in zip(worst, ic.camera_error(K, R, t, cs["K"], cs["R"], cs["t"], moved))]
            steps = max(steps, int(rep["steps"].max()))
            assert rep["cost"][moved, 1].max() < 1e-12                                        # px^2: nothing but rounding is left
            held = [c for c in range(cs["K"].shape[0]) if c not in cs["free"]]
            assert _same(K[held], np.asarray(cs["Kd"])[held]) and _same(R[held], np.asarray(cs["Rd"])[held]) and (rep["codes"][held] == FIXED).all()
    print(f"    exact detections: focal {worst[0]:.3e}, centre {worst[1]:.3e} px, |R - R_true| {worst[2]:.3e}, |t - t_true| / rig scale {worst[3]:.3e}; "
          f"at most {steps} steps")
    assert all(_holds(w, f) for w, f in zip(worst, ic.FLOOR_EXACT_K)), worst


# ------------------------------------------------------------------------------------------------ (d) the exact minimiser
def test_reference_against_the_exact_minimiser():
    worst = [0.0] * 4
    for rig_name in ic.RIGS:
        K, R, t, rep, _ = ic.reference(rig_name, ic.NOISY_SHAPE, ic.NOISY_SIGMA, True)
        mn = ic.minimiser(rig_name)
        cams = list(mn["cams"])
        assert cams and (rep["codes"][cams] == MOVED).all()
        err = ic.camera_error(K, R, t, mn["K"], mn["R"], mn["t"], cams)
        worst = [max(a, b) for a, b in zip(worst, err)]
        # the minimiser's cost is the smallest there is; the rule's end cost agrees with it to the rounding of its pixels
        # (b = 2.5e-12 px each, tests/test_reproject_host.py): |dE| <= 2 sqrt(2) b sqrt(n E), as in tests/test_pose_host.py
        e1, em, n = rep["cost"][cams, 1], mn["E"][cams], rep["n_obs"][cams]
        tol = 2 * np.sqrt(2) * 2.5e-12 * np.sqrt(n * em) + 64 * ic.EPS * em
        assert (np.abs(e1 - em) <= tol).all(), (e1 - em, tol)
        print(f"    {rig_name}: focal {err[0]:.3e}, centre {err[1]:.3e} px, |R - R*| {err[2]:.3e}, |t - t*| / rig scale {err[3]:.3e}")
    print(f"    noisy detections: focal {worst[0]:.3e}, centre {worst[1]:.3e} px, |R - R*| {worst[2]:.3e}, |t - t*| / rig scale {worst[3]:.3e}")
    assert all(_holds(w, f) for w, f in zip(worst, ic.FLOOR_NOISY_K)), worst


# ------------------------------------------------------------------------------------------------ (e) the normal equations
def test_normal_equations_against_50_digit_sums():
    worst = 0.0
    for rig_name in ic.RIGS:
        cs = ic.case(rig_name, ic.NOISY_SHAPE, ic.NOISY_SIGMA, True)
        Ko, Ro, to, rep, S = ic.reference(rig_name, ic.NOISY_SHAPE, ic.NOISY_SIGMA, True)
        for c in (ic.minimiser(rig_name)["cams"][0], 0):       # a fixed camera too: `normal` is reported for every camera
            X, ou, ov, w = ic.camera_observations(cs, S, c)
            val, mag = ic.exact_normal(cs["Kd"][c], cs["Rd"][c], cs["td"][c], X, ou, ov, w)
            nz = mag > 0                                       # fx.fy, fx.cy, fy.cx, cx.cy have no term at all (an axis-aligned
            zeros = [11 + pose.H_INDEX_K.index(ab) for ab in ((7, 6), (8, 7), (9, 6), (9, 8))]   # camera without skew has more)
            assert rep["n_obs"][c] == len(X) > 0 and not nz[zeros].any() and not rep["normal"][c][~nz].any()
            assert rep["normal"][c, 11 + pose.H_INDEX_K.index((9, 9))] == rep["normal"][c, 11 + pose.H_INDEX_K.index((8, 8))] == len(X)
            worst = max(worst, float((np.abs(rep["normal"][c] - val)[nz] / (ic.EPS * mag[nz])).max()))
            if rep["codes"][c] == MOVED:                       # ... and the sums where the rule ends (cost[., 1] is its E)
                val, mag = ic.exact_normal(Ko[c], Ro[c], to[c], X, ou, ov, w)
                end = pose.evaluate_camera_k(Ko[c], Ro[c], to[c], X, ou, ov, w)[0]
                assert end[0] == rep["cost"][c, 1]
                worst = max(worst, float((np.abs(end - val)[nz] / (ic.EPS * mag[nz])).max()))
    print(f"    the rule's E, g[10], H[55] against 50-digit sums: {worst:.3e} eps * sum |term|")
    assert _holds(worst, ic.NORMAL_UNITS_K), worst


# ------------------------------------------------------------------------------------------------ (f) the parameter sets
@pytest.mark.parametrize("intrinsics", ["f", "c", "fc"])
def test_parameter_sets_codes_and_bit_copies(intrinsics):
    cs = ic.case("ring8", (6, 2, 17), 1.0, True)
    C = cs["K"].shape[0]
    Kd, Rd, td = (np.ascontiguousarray(cs[k]) for k in ("Kd", "Rd", "td"))
    for free, ifree in (("odd", "odd"), ("none", "odd"), ("odd", "all"), ("all", "none")):
        K, R, t, rep, _ = ic.reference("ring8", (6, 2, 17), 1.0, True, intrinsics=intrinsics, free=free, intrinsics_free=ifree)
        pick = lambda which: {"odd": set(cs["free"]), "none": set(), "all": set(range(C))}[which]
        assert np.isfinite(rep["cost"]).all() and (rep["cost"][:, 1] <= rep["cost"][:, 0]).all() and rep["normal"].shape == (C, 66)
        for c in range(C):
            n = len(pose.free_set(c in pick(free), pose.intrinsics_flags(intrinsics) if c in pick(ifree) else 0))
            assert rep["codes"][c] == (FIXED if n == 0 else FEW if rep["n_obs"][c] < ic.MIN_OBS else rep["codes"][c]) and (n == 0 or rep["codes"][c] != FIXED)
            if c not in pick(free) or rep["codes"][c] != MOVED:
                assert _same(R[c], Rd[c]) and _same(t[c], td[c])
            if c not in pick(ifree) or rep["codes"][c] != MOVED:
                assert _same(K[c], Kd[c])
            if "f" not in intrinsics:
                assert K[c, 0, 0] == Kd[c, 0, 0] and K[c, 1, 1] == Kd[c, 1, 1]
            if "c" not in intrinsics:
                assert K[c, 0, 2] == Kd[c, 0, 2] and K[c, 1, 2] == Kd[c, 1, 2]
            assert _same(K[c, [0, 1, 2, 2, 2], [1, 0, 0, 1, 2]], Kd[c, [0, 1, 2, 2, 2], [1, 0, 0, 1, 2]])   # the skew and the last row
            if rep["codes"][c] == MOVED:
                assert rep["cost"][c, 1] < rep["cost"][c, 0] and K[c, 0, 0] > 0 and K[c, 1, 1] > 0
        assert (rep["codes"] == MOVED).any()


# ------------------------------------------------------------------------------------------------ (g) arguments
def test_argument_checking_and_the_public_names():
    cs = ic.case("floor", (3, 1, 17), 1.0, False)
    K, R, t, x, kp = cs["Kd"], cs["Rd"], cs["td"], cs["xyzs"], cs["kpts"]
    for bad in (dict(intrinsics="x"), dict(intrinsics="cf"), dict(intrinsics=3), dict(intrinsics="fc", intrinsics_free=[4]),
                dict(intrinsics="f", intrinsics_free=16), dict(intrinsics="c", iters=17), dict(intrinsics="c", min_obs=2)):
        with pytest.raises(ValueError):
            pose.refine_cameras_reference(K, R, t, x, kp, **bad)
    with pytest.raises(ValueError):
        pose.refine_rig(K, R, t, kp, free=[1], intrinsics="k", triangulate=lambda *a: None, reference=True)
    out = pose.refine_cameras_reference(K, R, t, np.zeros((0, 1, 17, 4)), np.zeros((0, 4, 1, 17, 3)), free=[1], intrinsics="fc", intrinsics_free=[2], min_obs=3)
    assert len(out) == 4 and _same(out[0], np.asarray(K)) and _same(out[1], np.asarray(R)) and out[3]["codes"].tolist() == [FIXED, FEW, FEW, FIXED]
    import inspect
    import snowmocap_amd.pipeline as pl
    from snowmocap_amd import _lib
    from snowmocap_amd.camera import CameraGroup
    assert "snowtri_refine_cameras_k" in set(_lib.exported_symbols()) and (_lib.INTR_FOCAL, _lib.INTR_CENTRE) == (1, 2)
    assert len(pose.H_INDEX) == 21 and len(pose.H_INDEX_K) == 55 and pose.H_INDEX_K[:21] == pose.H_INDEX
    for fn in (pose.refine_cameras_reference, pose.refine_cameras, pose.refine_rig, _lib.Context.refine_cameras):
        p = inspect.signature(fn).parameters
        assert p["intrinsics"].default is None and p["intrinsics_free"].default is None
    assert "intrinsics" in CameraGroup.refine_poses.__doc__
    assert "intrinsics" not in inspect.signature(pl.TrackPipeline.run).parameters              # calibration happens before a recording
    hdr = open(os.path.join(ROOT, "include", "snowtri.h")).read()
    for word in ("INTRINSICS (snowtri_refine_cameras_k)", "SNOWTRI_INTR_FOCAL", "SNOWTRI_INTR_CENTRE", "normal [C][66]", "ITS OWN WORKSPACE",
                 "Ten parameters need thousands of observations", "undistorted again from the raw frame"):
        assert word in hdr, word


def test_intrinsics_entry_rejects_bad_arguments_under_asan(tmp_path):
    """`make asan` + tests/abi_badargs_intrinsics.c, built and run exactly as tests/test_pose_host.py does for
    tests/abi_badargs_pose.c: a stand-alone C program on the CPU (no device visible), nothing preloaded."""
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
    exe = str(tmp_path / "abi_badargs_intrinsics")
    subprocess.check_call([clang, "-std=c99", "-fsanitize=address", "-g", "-I", os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "tests", "abi_badargs_intrinsics.c"), "-o", exe, so, "-Wl,-rpath," + os.path.dirname(so)])
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=0:abort_on_error=0", HIP_VISIBLE_DEVICES="", ROCR_VISIBLE_DEVICES="")
    p = subprocess.run([exe], env=env, capture_output=True, text=True, timeout=120)
    assert p.returncode == 0 and "0 failure(s)" in p.stdout, p.stdout[-3000:] + p.stderr[-3000:]
    assert "AddressSanitizer" not in p.stderr, p.stderr[-3000:]


# ------------------------------------------------------------------------------------------------ (h) the alternation
def wrong_K_recipe(F=40):
    """pose_cases.recipe with camera 3's POSE TRUE and its K wrong: fx, fy 2 % high, the centre off by (8, -5) px."""
    rp = pc.recipe(F=F)
    Kd = np.array(rp["K"], copy=True)
    Kd[rp["bad"], 0, 0] *= 1.02
    Kd[rp["bad"], 1, 1] *= 1.02
    Kd[rp["bad"], 0, 2] += 8.0
    Kd[rp["bad"], 1, 2] -= 5.0
    return rp, Kd


def test_refine_rig_repairs_a_wrong_K_where_pose_only_moves_the_camera():
    """Camera 3's pose is true and its K is wrong; three rounds, every step by its NumPy rule, a plain DLT as the triangulation.
    Measured here, 40 frames (1 360 observations of the camera), view RMS before 8.42 px, after rounds 1 | 2 | 3:
      pose only:                    2.553 | 1.497 | 1.364 px, the focal error stays 2.0e-2, the CORRECT camera is moved by 86.5 mm;
      fx, fy, cx, cy, pose held:    2.531 | 1.450 | 1.312 px, focal 8.7e-4, centre 0.18 px, the pose keeps its bits.
    Asserted: pose-only moves the camera by more than 3 cm and leaves K alone; the intrinsics with the pose held bring the focal
    error below 2e-3 and the centre within 1 px, and the RMS at least as low as pose-only's."""
    rp, Kd = wrong_K_recipe()
    bad = rp["bad"]
    kw = dict(rounds=3, triangulate=pc.dlt_points, reference=True, params=dict(keypoint_score_threshold=0.5))
    R, t, hist = pose.refine_rig(Kd, rp["R"], rp["t"], rp["kpts"], free=[bad], **kw)
    K2, R2, t2, hist2 = pose.refine_rig(Kd, rp["R"], rp["t"], rp["kpts"], free=[], intrinsics="fc", intrinsics_free=[bad], **kw)
    moved = float(np.linalg.norm(t[bad] - rp["t"][bad]))
    ef, ec = ic.camera_error(K2, R2, t2, rp["K"], rp["R"], rp["t"], [bad])[:2]
    print(f"    pose only: view RMS {[round(float(h['view_rms'][bad]), 3) for h in hist]}, camera moved by {1e3 * moved:.1f} mm")
    print(f"    intrinsics, pose held: view RMS {[round(float(h['view_rms'][bad]), 3) for h in hist2]}, focal {ef:.2e}, centre {ec:.2f} px")
    assert len(hist2) == 4 and K2.shape == (8, 3, 3) and moved > 0.03
    assert _same(R2, np.ascontiguousarray(rp["R"])) and _same(t2, np.ascontiguousarray(rp["t"]))
    keep = [c for c in range(8) if c != bad]
    assert _same(K2[keep], np.ascontiguousarray(Kd[keep])) and ef < 2e-3 and ec < 1.0
    assert hist2[-1]["view_rms"][bad] <= hist[-1]["view_rms"][bad] + 1e-9 and hist2[0]["view_rms"][bad] > 5.0
    assert all(h["codes"][bad] == MOVED and (np.delete(h["codes"], bad) == FIXED).all() for h in hist2[:3])
