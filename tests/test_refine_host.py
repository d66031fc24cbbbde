"""Refinement on the host (no GPU): the NumPy rule (snowmocap_amd/refine.py::refine_joints_reference) against the consequences of
the rule of include/snowtri.h ("Refinement"), against an exact minimiser, and the C entry refusing bad arguments under
AddressSanitizer.

  (a) cost_out <= cost_in for every record and every copied record is bit-identical: six rigs, six shapes, sigma 0 / 1 / 2, both
      starts, float64 and float32 records, everything tests/refine_cases.py sprinkles in;
  (b) with sigma >= 1 every refined record is MOVED;
  (c) from the pairwise start and from the DLT start the rule reaches the same point (6 steps): within the kernel's bar;
  (d) its distance to the 50-digit minimiser: the rule's floor, REFERENCE_FLOOR of tests/refine_cases.py (measured here: 1.83e-9 of
      the rig scale at worst, 5.9e-9 m on the floor rig at sigma = 2 px);
  (e) the statistical claim on the 10 640-joint recipe: the refined RMS error against the truth is below the start's for both
      starts, and with a per-view sigma the score-weighted refinement is below the unit-weight one;
  (f) argument checking, and tests/abi_badargs_refine.c against the `make asan` library.
"""
import os

import numpy as np
import pytest

import refine_cases as rc
from conftest import ROOT
from snowmocap_amd import refine as rf
from snowmocap_amd.records import missing_records

MISSING, FEW, KEPT, MOVED = rf.REFINE_MISSING, rf.REFINE_FEW_VIEWS, rf.REFINE_KEPT, rf.REFINE_MOVED


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint8)


# ------------------------------------------------------------------------------------------------ (a), (b): the rule's consequences
@pytest.mark.parametrize("rec_dtype", ["float64", "float32"])
@pytest.mark.parametrize("rig_name", rc.RIGS)
def test_cost_never_rises_and_copied_records_keep_their_bits(rig_name, rec_dtype):
    seen = np.zeros(4, dtype=np.int64)
    for shape in rc.SHAPES:
        for sigma in rc.SIGMAS:
            cs = rc.case(rig_name, shape, sigma, True, rec_dtype)
            rc.assert_domain(cs)
            for start in rc.STARTS:
                out, cost, codes, used = rc.reference(rig_name, shape, sigma, start, True, rec_dtype)
                x = cs[start]
                assert out.dtype == x.dtype and out.shape == x.shape
                assert (cost[..., 1] <= cost[..., 0]).all() and np.isfinite(cost).all()
                copied = codes < KEPT
                assert np.array_equal(codes == MISSING, missing_records(x))
                assert np.array_equal(_bits(out)[copied], _bits(x)[copied]) and (cost[copied] == 0).all() and (used[copied] == 0).all()
                assert np.array_equal(_bits(out[..., 3]), _bits(x[..., 3]))                   # scores untouched, everywhere
                kept = codes == KEPT
                assert np.array_equal(_bits(out)[kept], _bits(x)[kept]) and (cost[kept, 0] == cost[kept, 1]).all()
                moved = codes == MOVED
                assert (cost[moved, 1] < cost[moved, 0]).all()
                pop = sum(((used >> c) & 1).astype(int) for c in range(32))
                assert (pop[~copied] >= 2).all()
                if sigma >= 1.0:
                    assert not kept.any(), (rig_name, shape, sigma, start, int(kept.sum()))   # (b)
                if cs["one_view"] is not None:
                    flat = codes.reshape(-1)
                    assert flat[cs["one_view"]] == FEW and flat[cs["two_views"]] >= KEPT and pop.reshape(-1)[cs["two_views"]] == 2
                seen += np.bincount(codes.reshape(-1), minlength=4)
    assert (seen[[MISSING, FEW, MOVED]] > 0).all(), seen


def test_sigma_zero_is_decided_by_rounding_and_still_never_worse():
    out, cost, codes, _ = rc.reference("floor", (5, 2, 133), 0.0, "dlt", False)
    assert set(np.unique(codes)) <= {KEPT, MOVED} and (cost[..., 1] <= cost[..., 0]).all()
    assert cost[..., 1].max() < 1e-15                                                          # px^2: the detections are exact


# ------------------------------------------------------------------------------------------------ (c) the two starts meet
@pytest.mark.parametrize("rig_name", rc.RIGS)
def test_both_starts_reach_the_same_point(rig_name):
    worst = 0.0
    for sigma in (1.0, 2.0):
        for shape in ((2, 3, 21), rc.MINIMISER_SHAPE):
            cs = rc.case(rig_name, shape, sigma)
            a = rc.reference(rig_name, shape, sigma, "pair", iters=6)
            b = rc.reference(rig_name, shape, sigma, "dlt", iters=6)
            assert np.array_equal(a[2], b[2]) and np.array_equal(a[3], b[3])                   # codes and view sets
            ref = a[2] >= KEPT
            d = np.linalg.norm(a[0][..., :3] - b[0][..., :3], axis=-1)[ref].max() / rc.rig_scale(cs["t"])
            worst = max(worst, float(d))
    print(f"    {rig_name}: max |refined(pair) - refined(dlt)| = {worst:.2e} of the rig scale (6 steps)")
    assert worst <= rc.BAR


# ------------------------------------------------------------------------------------------------ (d) the exact minimiser
FLOOR_RIG = "floor"             # the rig whose worst record is REFERENCE_FLOOR


@pytest.mark.parametrize("rig_name", rc.RIGS)
def test_reference_against_the_exact_minimiser(rig_name):
    w = 0.0
    for sigma in (1.0, 2.0):
        for kp_dtype in ("float64", "float32"):
            mn = rc.minimiser(rig_name, sigma, kp_dtype)
            cs = rc.case(rig_name, rc.MINIMISER_SHAPE, sigma, True, "float64", kp_dtype)
            assert mn["refined"].sum() >= 30
            for start in rc.STARTS:
                out, cost, codes, _ = rc.reference(rig_name, rc.MINIMISER_SHAPE, sigma, start, True, "float64", kp_dtype, "home",
                                                   rc.ACCURACY_ITERS)
                assert np.array_equal(codes >= KEPT, mn["refined"])
                d = np.linalg.norm(out[..., :3] - mn["X"], axis=-1)[mn["refined"]]
                w = max(w, float(d.max()) / rc.rig_scale(cs["t"]))
                # the minimiser's cost is the smallest there is, and the rule's end cost agrees with it to the rounding of the
                # rule's pixels: b = 2.5e-12 px each (what tests/test_reproject_host.py holds the NumPy projection to), so the
                # residual vector of a view moves by sqrt(2) b and E by at most 2 sqrt(2) b sum |r_c| <= 2 sqrt(2) b sqrt(C E)
                e1, em = cost[..., 1][mn["refined"]], mn["E"][mn["refined"]]
                tol = 2 * np.sqrt(2) * 2.5e-12 * np.sqrt(cs["K"].shape[0] * em) + 64 * np.finfo(float).eps * em
                assert (np.abs(e1 - em) <= tol).all() and (e1 >= em - tol).all()
    print(f"    {rig_name}: max |reference - exact minimiser| = {w:.2e} of the rig scale")
    # REFERENCE_FLOOR is the worst over the rigs, measured on FLOOR_RIG: no rig may have left it by more than a factor of two,
    # and that rig must still show it
    assert w <= 2 * rc.REFERENCE_FLOOR and (rig_name != FLOOR_RIG or w >= rc.REFERENCE_FLOOR / 2), w
    assert rc.BAR == 4 * rc.REFERENCE_FLOOR


# ------------------------------------------------------------------------------------------------ (e) the statistical claim
def _rms(x, X):
    return float(np.sqrt(((x[..., :3] - X) ** 2).sum(axis=-1).mean()))


@pytest.mark.parametrize("C", [4, 8])
def test_refined_joints_are_closer_to_the_truth(C):
    cs = rc.recipe(C)
    assert cs["X"].shape[:3] == (40, 2, 133)
    got = {}
    for start in rc.STARTS:
        out, cost, codes = rf.refine_joints_reference(cs["K"], cs["R"], cs["t"], cs[start], cs["kpts"])
        assert (codes == MOVED).all() and (cost[..., 1] < cost[..., 0]).all()
        got[start] = (_rms(cs[start], cs["X"]), _rms(out, cs["X"]))
        assert got[start][1] < got[start][0], got
    print(f"    {C} cameras, sigma 1 px: RMS error pair {got['pair'][0] * 1e3:.2f} -> {got['pair'][1] * 1e3:.2f} mm, "
          f"dlt {got['dlt'][0] * 1e3:.2f} -> {got['dlt'][1] * 1e3:.2f} mm")
    cs = rc.recipe(C, per_view_sigma=True)
    unit = rf.refine_joints_reference(cs["K"], cs["R"], cs["t"], cs["dlt"], cs["kpts"])[0]
    wtd = rf.refine_joints_reference(cs["K"], cs["R"], cs["t"], cs["dlt"], cs["kpts"], score_weights=True)[0]
    e0, e1, e2 = _rms(cs["dlt"], cs["X"]), _rms(unit, cs["X"]), _rms(wtd, cs["X"])
    print(f"    {C} cameras, per-view sigma: dlt {e0 * 1e3:.2f} mm, unit weights {e1 * 1e3:.2f} mm, weights 1 / sigma^2 {e2 * 1e3:.2f} mm")
    assert e2 < e1 < e0


# ------------------------------------------------------------------------------------------------ the rule by hand
def test_cost_and_view_set_by_hand():
    cs = rc.case("ring5", (2, 3, 21), 1.0)
    out, cost, codes, used = rc.reference("ring5", (2, 3, 21), 1.0, "dlt")
    K, R, t = cs["K"], cs["R"], cs["t"]
    for f, p, j in ((0, 0, 5), (1, 2, 20), (0, 1, 2)):
        for which, rec in ((0, cs["dlt"]), (1, out)):
            acc, mask = 0.0, 0
            X = rec[f, p, j, :3]
            for c in range(5):
                q = cs["det_of"][f, c, p]
                if not (0 <= q < cs["n_persons"][f, c]):
                    continue
                u, v, s = cs["kpts"][f, c, q, j]
                if not (np.isfinite(u) and np.isfinite(v)) or s < cs["thr"] or not (int(cs["views"][f, p, j]) >> c) & 1:
                    continue
                d = X - t[c]                                                               # the rule's operations, in its order
                pc = [(R[c, 0, i] * d[0] + R[c, 1, i] * d[1]) + R[c, 2, i] * d[2] for i in range(3)]
                x, y = pc[0] / pc[2], pc[1] / pc[2]
                du, dv = (K[c, 0, 0] * x + K[c, 0, 1] * y + K[c, 0, 2]) - u, (K[c, 1, 1] * y + K[c, 1, 2]) - v
                acc = acc + (du * du + dv * dv)
                mask |= 1 << c
            if codes[f, p, j] >= KEPT:
                assert mask == used[f, p, j] and acc == cost[f, p, j, which]
            else:
                assert bin(mask).count("1") < 2 or codes[f, p, j] == MISSING


@pytest.mark.parametrize("rig_name", ["floor", "ring8", "ring16"])
def test_a_point_behind_a_camera_loses_that_view(rig_name):
    cs = rc.behind_case(rig_name)
    C = cs["K"].shape[0]
    out, cost, codes, used = rf.refine_joints_reference(cs["K"], cs["R"], cs["t"], cs["dlt"], cs["kpts"], keypoint_score_threshold=cs["thr"],
                                                        return_views=True)
    full = (1 << C) - 1
    assert used[0, 0].tolist() == [full & ~1, full, full, full] and (codes >= KEPT).all() and (cost[..., 1] <= cost[..., 0]).all()


def test_det_of_none_pairs_person_p_with_detection_p_and_weights_count():
    cs = rc.case("floor", (3, 1, 17), 1.0, False)
    a = rf.refine_joints_reference(cs["K"], cs["R"], cs["t"], cs["dlt"], cs["kpts"])
    det = np.zeros((3, 4, 1), dtype=np.int64)
    b = rf.refine_joints_reference(cs["K"], cs["R"], cs["t"], cs["dlt"], cs["kpts"], det_of=det, n_persons=np.ones((3, 4), dtype=np.int32))
    for x, y in zip(a, b):
        assert np.array_equal(x, y)
    w = rf.refine_joints_reference(cs["K"], cs["R"], cs["t"], cs["dlt"], cs["kpts"], score_weights=True)
    assert (w[2] == MOVED).all() and not np.array_equal(w[0], a[0])
    one = rf.refine_joints_reference(cs["K"], cs["R"], cs["t"], cs["dlt"], cs["kpts"], iters=1)
    assert (one[1][..., 1] >= a[1][..., 1]).all() and (one[1][..., 1] <= one[1][..., 0]).all()


# ------------------------------------------------------------------------------------------------ (f) arguments
def test_argument_checking():
    cs = rc.case("floor", (3, 1, 17), 1.0, False)
    K, R, t, x, kp = cs["K"], cs["R"], cs["t"], cs["dlt"], cs["kpts"]
    for bad in (dict(iters=0), dict(iters=17), dict(iters=2.5), dict(keypoint_score_threshold=float("nan"))):
        with pytest.raises(ValueError):
            rf.refine_joints_reference(K, R, t, x, kp, **bad)
    with pytest.raises(ValueError):
        rf.refine_joints_reference(K, R, t, x[..., :3], kp)
    with pytest.raises(ValueError):
        rf.refine_joints_reference(K, R, t, x, kp[:, :3])
    with pytest.raises(ValueError):
        rf.refine_joints_reference(K, R, t, np.concatenate([x, x], axis=1), kp)               # P = 2 > Pmax = 1 without det_of
    Kbad = np.array(K, copy=True)
    Kbad[0, 1, 0] = 1e-3
    with pytest.raises(ValueError):
        rf.refine_joints_reference(Kbad, R, t, x, kp)
    assert rf.refine_args(None) is None and rf.refine_args(4) == (4, 6.0, False) and rf.refine_args((2, 3.5, True)) == (2, 3.5, True)
    for bad in (0, 17, (4, 6.0), (4, -1.0, False), (4, float("nan"), False), 1.5):
        with pytest.raises(ValueError):
            rf.refine_args(bad)
    import snowmocap_amd
    import snowmocap_amd.pipeline as pl
    import inspect
    assert snowmocap_amd.refine_joints is rf.refine_joints and "refine_joints_reference" in snowmocap_amd.__all__
    assert inspect.signature(pl.TrackPipeline.run).parameters["refine"].default is None
    assert "snowtri_refine_joints" in snowmocap_amd._lib.exported_symbols()


def test_refine_entry_rejects_bad_arguments_under_asan(tmp_path):
    """`make asan` + tests/abi_badargs_refine.c, built and run exactly as tests/test_reproject_host.py does for
    tests/abi_badargs_reproject.c: a stand-alone C program on the CPU (no device visible), nothing preloaded."""
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
    exe = str(tmp_path / "abi_badargs_refine")
    subprocess.check_call([clang, "-std=c99", "-fsanitize=address", "-g", "-I", os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "tests", "abi_badargs_refine.c"), "-o", exe, so, "-Wl,-rpath," + os.path.dirname(so)])
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=0:abort_on_error=0", HIP_VISIBLE_DEVICES="", ROCR_VISIBLE_DEVICES="")
    p = subprocess.run([exe], env=env, capture_output=True, text=True, timeout=120)
    assert p.returncode == 0 and "0 failure(s)" in p.stdout, p.stdout[-3000:] + p.stderr[-3000:]
    assert "AddressSanitizer" not in p.stderr, p.stderr[-3000:]
