"""Reprojection on the host (no GPU): the NumPy rule against a 50-digit projection, the matching and residual code on hand-made
matrices, and the two C entries refusing bad arguments under AddressSanitizer.

  * `reproject_reference` (snowmocap_amd/reproject.py: the rule of include/snowtri.h in plain fp64 operations) against
    tests/reproject_cases.py::exact on the five rigs at the six placements, 48 points per camera, float64 and float32 records:
    within a quarter of the bars the kernel is held to (tests/test_gpu_reproject.py derives them): 2.5e-12 px undistorted, 5e-12 px
    raw, wherever a point lies in the accuracy domain of the camera (pc2 > 0, |d| / pc2 <= 1.8).  Measured: 4.5e-13 and 1.4e-12 px
    (6.8e-13 px raw over the points of a camera's own pool).
  * `match_detections`, `view_residuals`: ties, min_joints, the gate, shared, rows without a candidate -- NumPy and torch (CPU
    tensors: the same code that runs on CUDA tensors) give the same answers.
  * tests/abi_badargs_reproject.c against the `make asan` library.
"""
import os

import numpy as np
import pytest

import reproject_cases as rc
from conftest import ROOT
from snowmocap_amd import reproject as rp


# ------------------------------------------------------------------------------------------------ the rule against 50 digits
@pytest.mark.parametrize("placement", rc.PLACEMENTS)
@pytest.mark.parametrize("rig_name", rc.RIGS)
def test_reference_projection_against_the_50_digit_value(rig_name, placement):
    worst = {"uv": 0.0, "raw": 0.0}
    for placement in (placement,):
        for dtype_name in ("float64", "float32"):
            ex = rc.exact(rig_name, placement, dtype_name)
            K, R, t, D = rc.rig(rig_name, placement)
            N = ex["X"].shape[0]
            own = ex["in_domain"][ex["owner"], np.arange(N)]
            assert own.all(), "a point must lie in the domain of the camera it was made for"
            assert ex["ratio"][ex["owner"], np.arange(N)].max() <= 1.6
            xyzs = np.concatenate([ex["X"], np.full((N, 1), 2.5)], axis=1).astype(dtype_name).reshape(1, 1, N, 4)
            for key, raw, bar in (("uv", False, rc.BAR_F64 / 4), ("raw", True, rc.BAR_F64_RAW / 4)):
                got = rp.reproject_reference(K, R, t, xyzs, D=D, raw=raw)[0, :, 0]             # [C, N, 3]
                front = ex["depth"] > 0
                assert np.array_equal(got[..., 2] != 0, front), (placement, dtype_name, key)   # (no pixel of these points overflows)
                assert (got[..., 2][front] == 2.5).all() and (got[~front] == 0).all()
                err = np.abs(got[..., :2] - ex[key])[ex["in_domain"]]
                worst[key] = max(worst[key], float(err.max()))
                assert err.max() <= bar, (placement, dtype_name, key, float(err.max()))
    print(f"    {rig_name} {placement}: max |reproject_reference - 50-digit value|: {worst['uv']:.2e} px undistorted, "
          f"{worst['raw']:.2e} px raw")


def test_reference_marks_invalid_records_and_points_behind_the_camera():
    cs = rc.case("ring5", (3, 1, 17))
    x = np.array(cs["xyzs"], copy=True)
    x[0, 0, 0, 3] = 0.0
    x[0, 0, 1, 3] = -0.0
    x[0, 0, 2, 1] = np.nan
    x[0, 0, 3, 0] = np.inf
    x[0, 0, 4, 3] = np.nan
    pix = rp.reproject_reference(cs["K"], cs["R"], cs["t"], x)
    assert (pix[0, :, 0, :5] == 0).all() and not np.isnan(pix).any()
    clean = rp.reproject_reference(cs["K"], cs["R"], cs["t"], cs["xyzs"])
    assert np.array_equal(pix[0, :, 0, 5:], clean[0, :, 0, 5:]) and np.array_equal(pix[1:], clean[1:])
    assert (clean[cs["depth"] <= 0] == 0).all() and (clean[cs["depth"] > 0][:, 2] != 0).all()
    for c in range(5):                                                                       # half a metre and 3 m behind camera c
        x = np.array(cs["xyzs"], copy=True)
        x[1, 0, 7, :3] = cs["t"][c] - 0.5 * cs["R"][c][:, 2] + 0.1 * cs["R"][c][:, 0]
        x[2, 0, 9, :3] = cs["t"][c] - 3.0 * cs["R"][c][:, 2] - 0.2 * cs["R"][c][:, 1]
        pix = rp.reproject_reference(cs["K"], cs["R"], cs["t"], x)
        assert (pix[1, c, 0, 7] == 0).all() and (pix[2, c, 0, 9] == 0).all()
        keep = np.ones(pix.shape[:-1], dtype=bool)
        keep[1, :, 0, 7] = keep[2, :, 0, 9] = False
        assert np.array_equal(pix[keep], clean[keep])
    with pytest.raises(ValueError):
        rp.reproject_reference(cs["K"], cs["R"], cs["t"], cs["xyzs"], raw=True)               # no D
    Kbad = np.array(cs["K"], copy=True)
    Kbad[1, 1, 0] = 1e-3
    with pytest.raises(ValueError):
        rp.reproject_reference(Kbad, cs["R"], cs["t"], cs["xyzs"])


def test_reference_cost_of_a_person_against_its_own_projection_is_zero():
    cs = rc.cost_case((4, 3, 3, 133, 6))
    K, R, t, D = cs["K"], cs["R"], cs["t"], cs["D"]
    for raw in (False, True):
        pix = rp.reproject_reference(K, R, t, cs["xyzs"], D=D, raw=raw)
        s, n = rp.reprojection_cost_reference(K, R, t, cs["xyzs"], pix, None, 0.25, D=D, raw=raw)   # (the gate drops the (0, 0, 0) pixels)
        valid = (pix[..., 2] != 0).sum(axis=-1)                                              # [F, C, P]
        for p in range(3):
            assert (s[:, :, p, p] == 0).all() and np.array_equal(n[:, :, p, p], valid[:, :, p])
        # against another person: only the joints both have, hundreds of pixels apart
        both = ((pix[:, :, 0, :, 2] != 0) & (pix[:, :, 1, :, 2] != 0)).sum(axis=-1)
        assert np.array_equal(n[:, :, 0, 1], both) and (s[:, :, 0, 1] > 100.0 * both).all()
    # the order of the sum is joint order: one explicit loop over one item
    s, n = rp.reprojection_cost_reference(K, R, t, cs["xyzs"], cs["kpts"], None, cs["thr"])
    pix = rp.reproject_reference(K, R, t, cs["xyzs"])
    acc, cnt = 0.0, 0
    for j in range(133):
        d = cs["kpts"][2, 1, 0, j]
        if pix[2, 1, 1, j, 2] != 0 and not d[2] < cs["thr"] and np.isfinite(d[0]) and np.isfinite(d[1]):
            du, dv = pix[2, 1, 1, j, 0] - d[0], pix[2, 1, 1, j, 1] - d[1]
            acc += du * du + dv * dv
            cnt += 1
    assert cnt == n[2, 1, 1, 0] and acc == s[2, 1, 1, 0] and 0 < cnt < 133


# ------------------------------------------------------------------------------------------------ matching on hand-made matrices
def _both(fn, *arrays, **kw):
    """fn on NumPy arrays and on torch CPU tensors -> the NumPy results, after asserting that the two agree."""
    import torch
    a = fn(*arrays, **kw)
    b = fn(*[torch.from_numpy(np.ascontiguousarray(x)) for x in arrays], **kw)
    for x, y in zip(a, b):
        assert np.array_equal(np.asarray(x), y.numpy(), equal_nan=True), (x, y)
    return a


def test_match_detections_on_hand_made_costs():
    n = np.full((1, 1, 5, 4), 10, dtype=np.int32)
    s = np.array([[[[50.0, 20.0, 20.0, 90.0],          # a tie between q = 1 and 2: the lower one
                    [400.0, 370.0, 380.0, 390.0],      # the best mean is 37 px^2 > 6^2: nobody
                    [360.0, 500.0, 500.0, 500.0],      # exactly on the gate (mean 36): taken
                    [10.0, 5.0, 700.0, 700.0],         # q = 1 is the best but has too few joints (below): q = 0
                    [90.0, 10.0, 800.0, 900.0]]]])     # chooses q = 1 as person 0 does: shared
    n[0, 0, 3, 1] = 7
    det, shared = _both(rp.match_detections, s, n, gate_px=6.0)
    assert det.tolist() == [[[1, -1, 0, 0, 1]]]
    assert shared.tolist() == [[[True, False, True, True, True]]]
    det, shared = _both(rp.match_detections, s, n, gate_px=6.0, min_joints=7)                 # now person 3 may take q = 1
    assert det.tolist() == [[[1, -1, 0, 1, 1]]] and shared.tolist() == [[[True, False, False, True, True]]]
    det, _ = _both(rp.match_detections, s, n, gate_px=7.0)                                   # 37 <= 49
    assert det[0, 0, 1] == 1
    # rows without a candidate: every cost_n below min_joints, cost_n == 0 with cost_sum == 0, no detection at all
    n0 = np.zeros((2, 3, 2, 2), dtype=np.int32)
    det, shared = _both(rp.match_detections, np.zeros((2, 3, 2, 2)), n0, gate_px=6.0)
    assert (det == -1).all() and not shared.any()
    det, shared = _both(rp.match_detections, np.zeros((2, 3, 2, 0)), np.zeros((2, 3, 2, 0), dtype=np.int32), gate_px=6.0)
    assert det.shape == (2, 3, 2) and (det == -1).all() and not shared.any()
    # -1 is not a detection two persons share; an infinite or NaN sum never wins
    s2 = np.array([[[[np.inf, np.nan], [np.nan, 1.0]]]])
    det, shared = _both(rp.match_detections, s2, np.full((1, 1, 2, 2), 9, dtype=np.int32), gate_px=6.0)
    assert det.tolist() == [[[-1, 1]]] and not shared.any()
    for bad in (dict(gate_px=float("nan")), dict(gate_px=-1.0), dict(gate_px=6.0, min_joints=0)):
        with pytest.raises(ValueError):
            rp.match_detections(s, n, **bad)


def test_view_residuals_on_hand_made_pixels():
    pix = np.zeros((1, 2, 2, 3, 3))
    pix[0, :, :, :, 2] = 1.0
    pix[0, 0, 0, :, :2] = [[10.0, 10.0], [20.0, 20.0], [30.0, 30.0]]
    pix[0, 0, 1, :, :2] = [[100.0, 50.0], [0.0, 0.0], [7.0, 7.0]]
    pix[0, 0, 1, 1] = 0.0                                                   # an invalid projection
    kp = np.zeros((1, 2, 2, 3, 3))
    kp[..., 2] = 5.0
    kp[0, 0, 1, :, :2] = [[13.0, 14.0], [20.0, 20.0], [30.0, 42.0]]         # person 0 in camera 0 is detection 1: 5, 0, 12 px
    kp[0, 0, 0, :, :2] = [[100.0, 51.0], [1.0, 1.0], [np.nan, 7.0]]         # person 1 is detection 0: 1 px, (invalid), (NaN pixel)
    kp[0, 0, 1, 1, 2] = 0.4                                                 # below the threshold: person 0 loses its 0-px joint
    det_of = np.array([[[1, 0], [-1, 0]]])
    resid, rms, n = _both(rp.view_residuals, pix, kp, det_of, keypoint_score_threshold=0.5)
    assert np.array_equal(resid[0, 0, 0], [5.0, np.nan, 12.0], equal_nan=True)
    assert np.array_equal(resid[0, 0, 1], [1.0, np.nan, np.nan], equal_nan=True)
    assert np.isnan(resid[0, 1, 0]).all() and n.tolist() == [[[2, 1], [0, 3]]]
    assert rms[0, 0, 0] == np.sqrt((25.0 + 144.0) / 2) and rms[0, 0, 1] == 1.0 and np.isnan(rms[0, 1, 0]) and rms[0, 1, 1] == 0.0


# ------------------------------------------------------------------------------------------------ bad arguments under ASan
def test_reproject_entries_reject_bad_arguments_under_asan(tmp_path):
    """`make asan` + tests/abi_badargs_reproject.c, built and run exactly as tests/test_abi_and_host.py does for tests/abi_badargs.c: a
    stand-alone C program on the CPU (no device visible), nothing preloaded."""
    import shutil
    import subprocess
    csrc = os.path.join(ROOT, "snowmocap_amd", "csrc")
    so = os.path.join(csrc, "build", "libsnowtri_asan.so")
    clang = "/opt/rocm/lib/llvm/bin/clang"
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    if not (os.path.exists(hipcc) or shutil.which("hipcc")) or not os.path.exists(clang):
        pytest.skip("no ROCm toolchain (hipcc + its clang) on this machine: the ASan build of the C ABI cannot be made")
    import glob
    sources = glob.glob(os.path.join(csrc, "*.hip")) + glob.glob(os.path.join(csrc, "*.hpp")) + [os.path.join(ROOT, "include", "snowtri.h")]
    if not os.path.exists(so) or os.path.getmtime(so) < max(os.path.getmtime(f) for f in sources):   # (the target always rebuilds: ~1 min)
        subprocess.check_call(["make", "-C", csrc, "-s", "asan"])
    exe = str(tmp_path / "abi_badargs_reproject")
    subprocess.check_call([clang, "-std=c99", "-fsanitize=address", "-g", "-I", os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "tests", "abi_badargs_reproject.c"), "-o", exe, so, "-Wl,-rpath," + os.path.dirname(so)])
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=0:abort_on_error=0", HIP_VISIBLE_DEVICES="", ROCR_VISIBLE_DEVICES="")
    p = subprocess.run([exe], env=env, capture_output=True, text=True, timeout=120)
    assert p.returncode == 0 and "0 failure(s)" in p.stdout, p.stdout[-3000:] + p.stderr[-3000:]
    assert "AddressSanitizer" not in p.stderr, p.stderr[-3000:]
