"""k_pose_normal_k / k_pose_step_k behind snowtri_refine_cameras_k (include/snowtri.h, "Camera pose refinement", INTRINSICS), and the
keyword `intrinsics` of Context.refine_cameras / pose.refine_cameras, CameraGroup.refine_poses and pose.refine_rig.  Inputs:
tests/intrinsics_cases.py -- the kernels against the NumPy rule on the same inputs.

  * with intr_flags == 0 or intr_mask == 0 the entry is snowtri_refine_cameras_ex bit for bit on every output (HOST and DEVICE, both
    losses), of `normal` the 28 values the old entry has;
  * n_obs and codes equal the rule's; cost[., 0] and `normal` within MARGIN x NORMAL_UNITS_K eps * sum |term| of the rule's;
    cost[., 1] <= cost[., 0], and E recomputed by the rule at the returned K, R, t agrees with cost[., 1] to the same bound: every
    shape of pose_cases.SHAPES, rigs of 3, 4, 5, 8 and 16 cameras, one record more than a sweep of the grid;
  * exact detections: K, R, t within 4 x FLOOR_EXACT_K of the truth on six rigs x six placements; noisy detections: within
    4 x FLOOR_NOISY_K of the 50-digit minimiser;
  * every combination of "f", "c", "fc" with the pose free or fixed; a parameter outside a camera's free set keeps its bits;
  * float32, the Huber loss with n_outliers, two runs, torch DEVICE against NumPy HOST, the empty batch, the wrappers, the camera
    group, refine_rig against the rule-driven alternation, the bad-arguments program, the debug build.
"""
import os
import subprocess

import numpy as np
import pytest

import intrinsics_cases as ic
import pose_cases as pc
import refine_cases as rc
from snowmocap_amd import _lib, pose, synth

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EPS = ic.EPS
FIXED, FEW, KEPT, MOVED = pose.POSE_FIXED, pose.POSE_FEW_OBS, pose.POSE_KEPT, pose.POSE_MOVED
BAR_EXACT = tuple(ic.MARGIN * f for f in ic.FLOOR_EXACT_K)
BAR_NOISY = tuple(ic.MARGIN * f for f in ic.FLOOR_NOISY_K)
BAR_NORMAL = ic.MARGIN * ic.NORMAL_UNITS_K * EPS
REPORT = ("cost", "n_obs", "codes", "normal")


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
    ctx = _lib.Context(cs["Kd"], cs["Rd"], cs["td"])
    try:
        return ctx.refine_cameras(cs["xyzs"], cs["kpts"], diagnostics=True, **dict(cs["kw"], **over))
    finally:
        ctx.close()


def _within(err, bar):
    return all(e <= b for e, b in zip(err, bar))


def _magnitudes(cs, S, K, R, t, c, score_weights=False, huber_px=None):
    """sum |term| [66] of camera c's E, g, H at (K[c], R[c], t[c]) and the rule's sums there."""
    X, ou, ov, w = ic.camera_observations(cs, S, c, score_weights)
    terms, _ = pose.normal_terms_k(np.asarray(K)[c], R[c], t[c], X, ou, ov, w, huber_px)
    return np.abs(terms).sum(axis=0), pose._ordered_sum(terms)


def _check_against_the_rule(cs, got, ref, score_weights=False, huber_px=None, **over):
    """Everything that holds on every case: counts, codes, normal, costs, rotations, the parameters that stay."""
    K, R, t, rep = got
    Kr, Rr, tr, rr, S = ref
    C = cs["K"].shape[0]
    assert K.shape == R.shape == (C, 3, 3) and t.shape == (C, 3) and K.dtype == R.dtype == t.dtype == np.float64
    assert rep["normal"].shape == (C, 66) and rep["n_obs"].dtype == np.int64 and np.array_equal(rep["n_obs"], rr["n_obs"])
    still = (rr["codes"] == FIXED) | (rr["codes"] == FEW)
    assert np.array_equal(rep["codes"][still], rr["codes"][still]) and (rep["codes"][~still] >= KEPT).all()
    # KEPT or MOVED is the rule's wherever its first step lowers E by more than 1 % (at an exact start rounding decides)
    first = pose.refine_cameras_reference(cs["Kd"], cs["Rd"], cs["td"], cs["xyzs"], cs["kpts"], score_weights=score_weights, huber_px=huber_px,
                                          **dict(cs["kw"], **dict(over, iters=1)))[3]["cost"]
    clear = ~still & (first[:, 1] < 0.99 * first[:, 0])
    assert np.array_equal(rep["codes"][clear], rr["codes"][clear]) and (rep["codes"][clear] == MOVED).all()
    assert np.isfinite(rep["cost"]).all() and (rep["cost"][:, 1] <= rep["cost"][:, 0]).all() and not rep["cost"][still].any()
    Kd, Rd, td = (np.ascontiguousarray(cs[k]) for k in ("Kd", "Rd", "td"))
    worst = 0.0
    for c in range(C):
        if rep["n_obs"][c]:
            mag, _ = _magnitudes(cs, S, Kd, Rd, td, c, score_weights, huber_px)
            err = np.abs(rep["normal"][c] - rr["normal"][c]) / np.where(mag > 0, mag, 1.0)
            assert not rep["normal"][c][mag == 0].any()        # the structural zeros are zeros
            worst = max(worst, float(err.max()))
        else:
            assert not rep["normal"][c].any()
        if rep["codes"][c] != MOVED:
            assert _same_bits(K[c], Kd[c]) and _same_bits(R[c], Rd[c]) and _same_bits(t[c], td[c])
        assert _same_bits(K[c, [0, 1, 2, 2, 2], [1, 0, 0, 1, 2]], Kd[c, [0, 1, 2, 2, 2], [1, 0, 0, 1, 2]])       # the skew and the last row
        if not still[c]:
            assert rep["cost"][c, 0] == rep["normal"][c, 0]
            assert np.abs(R[c].T @ R[c] - np.eye(3)).max() < 64 * EPS and K[c, 0, 0] > 0 and K[c, 1, 1] > 0
            if rep["codes"][c] == MOVED:
                assert rep["cost"][c, 1] < rep["cost"][c, 0]
            # E at the returned parameters, recomputed by the rule: the terms are the rule's own plain operations at the same bits,
            # only the order of the sum differs, and sum |term| of E is E (under the loss too: rho >= 0)
            mag, E = _magnitudes(cs, S, K, R, t, c, score_weights, huber_px)
            assert abs(E[0] - rep["cost"][c, 1]) <= BAR_NORMAL * mag[0], (c, E[0], rep["cost"][c, 1])
    assert worst <= BAR_NORMAL, worst / EPS
    return worst / EPS


# ------------------------------------------------------------------------------------------------ off is the old entry
@pytest.mark.parametrize("space", ["host", "device"])
def test_no_intrinsics_free_is_the_old_entry_bit_for_bit(api, space):
    import torch
    dev = torch.device("cuda", 0)
    put = (lambda a: torch.from_numpy(np.array(a.view(np.int32) if a.dtype == np.uint32 else a)).to(dev)) if space == "device" else (lambda a: a)
    get = (lambda a: a.cpu().numpy()) if space == "device" else (lambda a: a)
    for rig_name, shape in (("ring5", (2, 3, 21)), ("floor", (6, 2, 17))):
        cs = ic.case(rig_name, shape, 1.0, True)
        ctx = _lib.Context(cs["Kd"], cs["Rd"], cs["td"])
        x, kp = put(cs["xyzs"]), put(cs["kpts"])
        shared = dict(det_of=put(cs["det_of"]), n_persons=put(cs["n_persons"]), views=put(cs["views"]), keypoint_score_threshold=cs["thr"],
                      free=list(cs["free"]), min_obs=ic.MIN_OBS, iters=ic.ITERS)
        for huber_px in (None, 3.0):
            R0, t0, rep0 = ctx.refine_cameras(x, kp, diagnostics=True, huber_px=huber_px, **shared)
            assert (get(rep0["codes"]) == MOVED).any()
            for intr_flags, intr_free in ((0, None), (3, []), (1, 0), (0, [])):
                K, R, t, rep = ctx._refine_cameras_k(x, kp, shared["det_of"], shared["n_persons"], shared["views"], cs["thr"], shared["free"],
                                                     ic.MIN_OBS, ic.ITERS, False, True, None, huber_px, intr_flags, intr_free)
                assert _same_bits(get(K), np.ascontiguousarray(cs["Kd"])) and _same_bits(get(R), get(R0)) and _same_bits(get(t), get(t0))
                assert all(_same_bits(get(rep[k]), get(rep0[k])) for k in rep0 if k != "normal") and rep.keys() == rep0.keys()
                n, n0 = get(rep["normal"]), get(rep0["normal"])
                assert _same_bits(n[:, :7], n0[:, :7]) and _same_bits(n[:, 11:32], n0[:, 7:]) and n[:, 32:].any()
        ctx.close()


# ------------------------------------------------------------------------------------------------ the rule, shape by shape
@pytest.mark.parametrize("rig_name", ic.RIGS)
def test_counts_codes_normal_and_costs_against_the_rule(api, rig_name):
    worst = 0.0
    seen = np.zeros(4, dtype=np.int64)
    for shape in ic.SHAPES:
        for sigma in (0.0, 1.0):
            cs = ic.case(rig_name, shape, sigma, True)
            got = _run(cs)
            worst = max(worst, _check_against_the_rule(cs, got, ic.reference(rig_name, shape, sigma, True)))
            seen += np.bincount(got[3]["codes"], minlength=4)
            again = _run(cs)                                  # two runs, two contexts: the same bits
            assert all(_same_bits(got[k], again[k]) for k in range(3)) and all(_same_bits(got[3][k], again[3][k]) for k in REPORT)
    cs = ic.case(rig_name, (6, 2, 17), 1.0, True)
    got = _run(cs, score_weights=True)
    _check_against_the_rule(cs, got, ic.reference(rig_name, (6, 2, 17), 1.0, True, score_weights=True), True)
    print(f"    {rig_name} ({cs['K'].shape[0]} cameras): max |normal - rule| = {worst:.1f} eps * sum |term| (bar {ic.MARGIN * ic.NORMAL_UNITS_K:.0f}); codes seen {seen}")
    assert (seen[[FIXED, FEW, MOVED]] > 0).all()


def test_the_rigs_have_3_5_8_and_16_cameras():
    assert {3, 5, 8, 16} <= {pc.case(r, (1, 1, 8), 0.0, True)["K"].shape[0] for r in ic.RIGS}


def test_one_record_more_than_a_sweep_of_the_grid(api):
    """F = POSE_SWEEP_RECORDS + 1 frames of one joint in three cameras: some lanes walk two records, and a camera's sum is made of
    1024 partials of 72 doubles.  Exact detections, a few of them spoiled; camera 1 drifted in pose and in K."""
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
    Kd = ic.drift_K("ring3", "home", K, [1])
    cs = dict(K=K, R=R, t=t, Kd=Kd, Rd=Rd, td=td, free=(1,), xyzs=x4, kpts=kp, det_of=None, n_persons=None, views=None, thr=0.5,
              kw=dict(keypoint_score_threshold=0.5, free=[1], min_obs=ic.MIN_OBS, iters=ic.ITERS, intrinsics="fc", intrinsics_free=[1]))
    ref = pose.refine_cameras_reference(Kd, Rd, td, x4, kp, return_sets=True, **cs["kw"])
    got = _run(cs)
    units = _check_against_the_rule(cs, got, ref, intrinsics_free=[1])
    spoiled = np.zeros(F, dtype=bool)
    spoiled[::1001] = spoiled[5::977] = spoiled[7::4099] = True
    assert ref[4][1, -1] and ref[3]["n_obs"][1] == F - spoiled.sum()                          # the last record counts
    err = ic.camera_error(*got[:3], K, R, t, [1])
    print(f"    {F} records: |normal - rule| = {units:.1f} eps * sum |term|; focal {err[0]:.2e}, centre {err[1]:.2e} px, |R - R_true| {err[2]:.2e}, |t - t_true| {err[3]:.2e}")
    assert got[3]["codes"].tolist() == [FIXED, MOVED, FIXED] and _within(err, BAR_EXACT)


# ------------------------------------------------------------------------------------------------ accuracy
@pytest.mark.parametrize("rig_name", ic.RIGS)
def test_exact_detections_return_to_the_true_camera(api, rig_name):
    worst = [0.0] * 4
    for placement in ic.PLACEMENTS:
        cs = ic.case(rig_name, ic.EXACT_SHAPE, 0.0, True, placement=placement)
        K, R, t, rep = got = _run(cs)
        _check_against_the_rule(cs, got, ic.reference(rig_name, ic.EXACT_SHAPE, 0.0, True, placement=placement))
        assert (rep["codes"][list(cs["free"])] == MOVED).all()
        err = ic.camera_error(K, R, t, cs["K"], cs["R"], cs["t"], cs["free"])
        worst = [max(a, b) for a, b in zip(worst, err)]
        assert _within(err, BAR_EXACT), (placement, err, BAR_EXACT)
    print(f"    {rig_name}: focal {worst[0]:.2e}, centre {worst[1]:.2e} px, |R - R_true| {worst[2]:.2e}, |t - t_true| / rig scale {worst[3]:.2e} (bars {BAR_EXACT})")


@pytest.mark.parametrize("rig_name", ic.RIGS)
def test_noisy_detections_against_the_exact_minimiser(api, rig_name):
    cs = ic.case(rig_name, ic.NOISY_SHAPE, ic.NOISY_SIGMA, True)
    mn = ic.minimiser(rig_name)
    K, R, t, rep = got = _run(cs)
    _check_against_the_rule(cs, got, ic.reference(rig_name, ic.NOISY_SHAPE, ic.NOISY_SIGMA, True))
    cams = list(mn["cams"])
    assert (rep["codes"][cams] == MOVED).all()
    err = ic.camera_error(K, R, t, mn["K"], mn["R"], mn["t"], cams)
    print(f"    {rig_name}: focal {err[0]:.2e}, centre {err[1]:.2e} px, |R - R*| {err[2]:.2e}, |t - t*| / rig scale {err[3]:.2e} (bars {BAR_NOISY})")
    assert _within(err, BAR_NOISY), (err, BAR_NOISY)


# ------------------------------------------------------------------------------------------------ the parameter sets
@pytest.mark.parametrize("intrinsics", ["f", "c", "fc"])
@pytest.mark.parametrize("free", ["odd", "none"])
def test_parameter_sets_against_the_rule(api, intrinsics, free):
    """"f", "c" and "fc" with the pose free or fixed, and with every camera's or only the odd cameras' intrinsics free: everything of
    _check_against_the_rule, the returned parameters within the noisy bar of the rule's (both are strict-decrease iterations on one
    cost from one start), and the parameters outside a camera's free set bit for bit."""
    rig_name, shape = "ring8", (6, 2, 17)
    cs = ic.case(rig_name, shape, 1.0, True)
    Kd, Rd, td = (np.ascontiguousarray(cs[k]) for k in ("Kd", "Rd", "td"))
    C = Kd.shape[0]
    for ifree in ("odd", "all"):
        pick = lambda which: {"odd": list(cs["free"]), "none": [], "all": None}[which]
        over = dict(intrinsics=intrinsics, free=pick(free), intrinsics_free=pick(ifree))
        ref = ic.reference(rig_name, shape, 1.0, True, intrinsics=intrinsics, free=free, intrinsics_free=ifree)
        K, R, t, rep = got = _run(cs, **over)
        _check_against_the_rule(cs, got, ref, **over)
        moved = [c for c in range(C) if rep["codes"][c] == MOVED]
        err = ic.camera_error(K, R, t, ref[0], ref[1], ref[2], moved)
        print(f"    {intrinsics} pose {free} intrinsics {ifree}: moved {moved}; vs the rule: focal {err[0]:.2e}, centre {err[1]:.2e} px, R {err[2]:.2e}, t {err[3]:.2e}")
        assert moved and _within(err, BAR_NOISY), err
        for c in range(C):
            if free == "none" or c not in cs["free"]:
                assert _same_bits(R[c], Rd[c]) and _same_bits(t[c], td[c])                    # the pose is held: its bits
            if ifree == "odd" and c not in cs["free"]:
                assert _same_bits(K[c], Kd[c])                                                # outside intr_mask: K's bits
            if "f" not in intrinsics:
                assert K[c, 0, 0] == Kd[c, 0, 0] and K[c, 1, 1] == Kd[c, 1, 1]
            if "c" not in intrinsics:
                assert K[c, 0, 2] == Kd[c, 0, 2] and K[c, 1, 2] == Kd[c, 1, 2]
            want = FIXED if (free == "none" or c not in cs["free"]) and (ifree == "odd" and c not in cs["free"]) else None
            assert want is None or rep["codes"][c] == want


# ------------------------------------------------------------------------------------------------ dtypes, the loss, spaces
@pytest.mark.parametrize("placement", ["home", "mm-site"])
def test_float32_records_and_keypoints(api, placement):
    """float32 in, the same float32 values given to the rule: everything of _check_against_the_rule, and the two end at the same
    parameters within the noisy bar (E here, the rounding of the inputs to float32, lies below that of the sigma = 1 cases)."""
    assert placement in ic.PLACEMENTS
    for rig_name in ("floor", "ring5"):
        for sigma in (0.0, 1.0):
            cs = ic.case(rig_name, ic.EXACT_SHAPE, sigma, True, "float32", "float32", placement)
            assert cs["xyzs"].dtype == np.float32 and cs["kpts"].dtype == np.float32
            K, R, t, rep = got = _run(cs)
            ref = ic.reference(rig_name, ic.EXACT_SHAPE, sigma, True, "float32", "float32", placement)
            _check_against_the_rule(cs, got, ref)
            moved = [c for c in cs["free"] if rep["codes"][c] == MOVED]
            err = ic.camera_error(K, R, t, ref[0], ref[1], ref[2], moved)
            print(f"    {rig_name} {placement} sigma {sigma}: vs the rule: focal {err[0]:.2e}, centre {err[1]:.2e} px, R {err[2]:.2e}, t {err[3]:.2e}")
            assert moved == list(cs["free"]) and _within(err, BAR_NOISY), err


def test_huber_at_three_pixels_with_n_outliers(api):
    """10 % of the free cameras' detections moved by 20 .. 150 px, delta = 3 px: the rule's checks under the loss, n_outliers exact."""
    for rig_name in ("floor", "ring8"):
        base = ic.case(rig_name, (6, 2, 17), 1.0, True)
        rng = np.random.default_rng(rc._seed("intr-huber", rig_name))
        kp = np.array(base["kpts"], copy=True)
        hit = rng.random(kp.shape[:-1]) < 0.10
        ang, far = rng.uniform(0, 2 * np.pi, hit.sum()), rng.uniform(20.0, 150.0, hit.sum())
        kp[hit, 0] += far * np.cos(ang)
        kp[hit, 1] += far * np.sin(ang)
        cs = dict(base, kpts=kp)
        ref = pose.refine_cameras_reference(cs["Kd"], cs["Rd"], cs["td"], cs["xyzs"], kp, return_sets=True, huber_px=3.0, **cs["kw"])
        K, R, t, rep = got = _run(cs, huber_px=3.0)
        _check_against_the_rule(cs, got, ref, huber_px=3.0)
        assert rep["n_outliers"].dtype == np.int64 and np.array_equal(rep["n_outliers"], ref[3]["n_outliers"]) and rep["n_outliers"].sum() > 0
        moved = [c for c in cs["free"] if rep["codes"][c] == MOVED]
        err = ic.camera_error(K, R, t, ref[0], ref[1], ref[2], moved)
        print(f"    {rig_name}: n_outliers {rep['n_outliers'].tolist()}; vs the rule: focal {err[0]:.2e}, centre {err[1]:.2e} px, R {err[2]:.2e}, t {err[3]:.2e}")
        assert moved == list(cs["free"])


def test_torch_device_and_numpy_host_give_the_same_bits(api):
    import torch
    dev = torch.device("cuda", 0)
    for rig_name, shape, dt in (("floor", (6, 2, 17), "float64"), ("ring16", (2, 3, 21), "float32")):
        cs = ic.case(rig_name, shape, 1.0, True, dt, dt)
        host = _run(cs)
        ctx = _lib.Context(cs["Kd"], cs["Rd"], cs["td"])
        kw = dict(cs["kw"], det_of=torch.from_numpy(np.array(cs["det_of"])).to(dev), n_persons=torch.from_numpy(np.array(cs["n_persons"])).to(dev),
                  views=torch.from_numpy(np.array(cs["views"]).view(np.int32)).to(dev))
        x, kp = torch.from_numpy(np.array(cs["xyzs"])).to(dev), torch.from_numpy(np.array(cs["kpts"])).to(dev)
        for _ in range(2):                                    # the second call reuses the context's intrinsics workspace
            K, R, t, rep = ctx.refine_cameras(x, kp, diagnostics=True, **kw)
            assert K.is_cuda and rep["n_obs"].dtype == torch.int64 and tuple(rep["normal"].shape) == (cs["K"].shape[0], 66)
            assert all(_same_bits(a.cpu().numpy(), b) for a, b in zip((K, R, t), host[:3]))
            assert all(_same_bits(rep[k].cpu().numpy(), host[3][k]) for k in REPORT)
        # the pose-only entry on the same context afterwards: its own workspace, its own bits
        R1, t1 = ctx.refine_cameras(x, kp, **{k: v for k, v in kw.items() if k != "intrinsics"})
        K2, R2, t2 = pose.refine_cameras(ctx, x, kp, **kw)    # without diagnostics: the optional outputs are NULL
        assert all(_same_bits(a.cpu().numpy(), b) for a, b in zip((K2, R2, t2), host[:3])) and not _same_bits(R1.cpu().numpy(), host[1])
        ctx.close()


def test_wrappers_refusals_the_empty_batch_and_the_camera_group(api):
    cs = ic.case("floor", (6, 2, 17), 1.0, True)
    ctx = _lib.Context(cs["Kd"], cs["Rd"], cs["td"])
    x, kp, kw = cs["xyzs"], cs["kpts"], cs["kw"]
    for bad in (dict(intrinsics="x"), dict(intrinsics="cf"), dict(intrinsics=1), dict(intrinsics_free=[4]), dict(intrinsics_free=1 << 4),
                dict(iters=17), dict(min_obs=2), dict(free=[4])):
        with pytest.raises(ValueError):
            ctx.refine_cameras(x, kp, **dict(kw, **bad))
    K, R, t, rep = ctx.refine_cameras(np.zeros((0, 2, 17, 4)), np.zeros((0, 4, 3, 17, 3)), free=[1], intrinsics="f", intrinsics_free=[1, 2], min_obs=3,
                                      iters=2, diagnostics=True)
    assert _same_bits(K, np.ascontiguousarray(cs["Kd"])) and _same_bits(R, np.ascontiguousarray(cs["Rd"])) and _same_bits(t, np.ascontiguousarray(cs["td"]))
    assert rep["codes"].tolist() == [FIXED, FEW, FEW, FIXED] and not rep["cost"].any() and not rep["n_obs"].any() and not rep["normal"].any()
    want = ctx.refine_cameras(x, kp, **kw)
    assert len(want) == 3
    ctx.close()
    # CameraGroup.refine_poses: a NEW group with the refined K, R, t, the original untouched
    group = api.CameraGroup(cap_ids=list(range(4)), resolutions=[(1280, 720)] * 4)
    for c, cam in enumerate(group.cameras):
        cam.K, cam.R, cam.t = np.array(cs["Kd"][c]), np.array(cs["Rd"][c]), np.array(cs["td"][c]).reshape(3, 1)
    new, rep = group.refine_poses(x, kp, diagnostics=True, **kw)
    assert new is not group and new.camera_num == 4 and rep["codes"].tolist() == [FIXED, MOVED, FIXED, MOVED]
    Kn, Rn, tn = new.rig_arrays()
    assert _same_bits(Kn, want[0]) and _same_bits(Rn, want[1]) and _same_bits(tn, want[2]) and not _same_bits(Kn, np.ascontiguousarray(cs["Kd"]))
    assert _same_bits(group.rig_arrays()[0], np.ascontiguousarray(cs["Kd"])) and _same_bits(group.rig_arrays()[1], np.ascontiguousarray(cs["Rd"]))


def test_entry_rejects_bad_arguments_on_a_real_context(api, tmp_path):
    """tests/abi_badargs_intrinsics.c against libsnowtri.so on the GPU: the new refusals, the empty batch, the old entry byte for
    byte with no intrinsics free, good calls."""
    lib_dir = os.path.join(ROOT, "snowmocap_amd")
    exe = str(tmp_path / "abi_badargs_intrinsics")
    subprocess.check_call(["gcc", "-std=c99", "-O1", "-I", os.path.join(ROOT, "include"), os.path.join(ROOT, "tests", "abi_badargs_intrinsics.c"),
                           "-o", exe, "-L", lib_dir, "-lsnowtri", "-Wl,-rpath," + lib_dir])
    out = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0 and "0 failure(s)" in out.stdout, out.stdout[-3000:] + out.stderr[-2000:]


DBG_CODE = r'''
import sys, numpy as np
sys.path.insert(0, %(root)r)
sys.path.insert(0, %(tests)r)
import intrinsics_cases as ic
from snowmocap_amd import _lib
assert _lib.LIB_PATH.endswith("libsnowtri_dbg.so") and "SNOWTRI_DEBUG_BOUNDS" in _lib.build_info()["variants"]
for rig_name, shape, dt, huber in (("floor", (6, 2, 17), "float64", None), ("ring8", (1, 1, 65), "float32", 3.0), ("ring16", (2, 3, 21), "float64", None),
                                   ("ring3", (1, 1, 257), "float64", 3.0), ("ring5", (2, 3, 21), "float64", None)):
    cs = ic.case(rig_name, shape, 1.0, True, dt, dt)
    ctx = _lib.Context(cs["Kd"], cs["Rd"], cs["td"])
    K, R, t, rep = ctx.refine_cameras(cs["xyzs"], cs["kpts"], diagnostics=True, huber_px=huber, **cs["kw"])
    ref = ic.reference(rig_name, shape, 1.0, True, dt, dt, huber_px=huber)
    assert np.array_equal(rep["n_obs"], ref[3]["n_obs"]) and np.array_equal(rep["codes"], ref[3]["codes"])
    n, first = ctx.debug_faults()
    assert n == 0, "device-side bounds check failed %%d times; first: code %%d at line %%d" %% (n, first >> 32, first & 0xffffffff)
    ctx.close()
print("intrinsics debug-bounds ok")
'''


def test_debug_build_counts_no_fault():
    dbg = os.path.join(ROOT, "snowmocap_amd", "libsnowtri_dbg.so")
    assert os.path.exists(dbg), f"{dbg} is missing: `make -C snowmocap_amd/csrc debug`"
    import sys
    env = dict(os.environ, SNOWTRI_LIB=dbg)
    code = DBG_CODE % {"root": ROOT, "tests": os.path.join(ROOT, "tests")}
    p = subprocess.run([sys.executable, "-c", code], env=env, capture_output=True, text=True, timeout=300)
    assert p.returncode == 0 and "intrinsics debug-bounds ok" in p.stdout, (p.stdout[-2000:] + p.stderr[-3000:])


# ------------------------------------------------------------------------------------------------ the alternation
def test_refine_rig_against_the_rule_driven_alternation(api):
    """pose.refine_rig(intrinsics="fc") on the GPU against the same alternation by the NumPy rules, both with pose_cases.dlt_points as
    the triangulation, after one round and after two, on the recipe with camera 3 nudged AND its K wrong (fx, fy 2 % high, the centre
    off by (8, -5) px): K, R, t within the noisy bar; the other cameras keep every bit."""
    rp = pc.recipe()
    bad = rp["bad"]
    Kd = np.array(rp["K"], copy=True)
    Kd[bad, 0, 0] *= 1.02
    Kd[bad, 1, 1] *= 1.02
    Kd[bad, 0, 2] += 8.0
    Kd[bad, 1, 2] -= 5.0
    args = (Kd, rp["Rd"], rp["td"], rp["kpts"])
    kw = dict(free=[bad], intrinsics="fc", intrinsics_free=[bad], triangulate=pc.dlt_points, params=dict(keypoint_score_threshold=0.5))
    for rounds in (1, 2):
        K, R, t, hist = pose.refine_rig(*args, rounds=rounds, **kw)
        Kr, Rr, tr, hr = pose.refine_rig(*args, rounds=rounds, reference=True, **kw)
        err = ic.camera_error(K, R, t, Kr, Rr, tr, [bad])
        print(f"    after round {rounds}: vs the rule: focal {err[0]:.2e}, centre {err[1]:.2e} px, R {err[2]:.2e}, t {err[3]:.2e}; "
              f"view RMS {hist[-1]['view_rms'][bad]:.3f} px; focal error {abs(K[bad, 0, 0] / rp['K'][bad, 0, 0] - 1):.2e}")
        assert _within(err, BAR_NOISY), (rounds, err)
        for h, g in zip(hist, hr):
            assert np.allclose(h["view_rms"], g["view_rms"], rtol=0, atol=1e-6)
            if "codes" in h:
                assert np.array_equal(h["codes"], g["codes"]) and np.array_equal(h["n_obs"], g["n_obs"])
        keep = [c for c in range(8) if c != bad]
        assert _same_bits(K[keep], np.ascontiguousarray(Kd[keep])) and _same_bits(R[keep], np.ascontiguousarray(rp["Rd"][keep]))
        assert _same_bits(t[keep], np.ascontiguousarray(rp["td"][keep]))
