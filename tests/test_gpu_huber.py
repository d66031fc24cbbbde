"""The Huber loss on the GPU: k_refine<.., HUBER> behind snowtri_refine_joints_ex, k_pose_normal<.., HUBER> / k_pose_step behind
snowtri_refine_cameras_ex, the huber_px keyword of Context.refine_joints / refine_cameras, refine.refine_joints,
pose.refine_cameras, CameraGroup.refine_poses, TrackPipeline.run(refine=(iters, gate_px, score_weights, huber_px)) and
pose.refine_rig(huber_px=...).  Inputs: tests/huber_cases.py; the rule: include/snowtri.h, ROBUST LOSS.

  1. the squared path: huber_px = 0 and 1e6 give every output of both _ex entries bit for bit as the entries without the loss;
  2. joint costs: cost[., 0] is the NumPy rule's E at the input and, with float64 records, cost[., 1] the rule's E at the kernel's own
     output point, bit for bit; no cost rises; MISSING / FEW_VIEWS are the rule's;
  3. `outliers` is the rule's classification at the kernel's output point (float32 records: views within the rounding margin of
     delta excused);
  4. accuracy against the 50-digit IRLS minimiser on the covered records;
  5. a record's bits do not depend on how the batch is cut;
  6. cameras: n_obs, `normal`, the poses against the 50-digit minimiser, two runs, n_outliers, FIXED / FEW_OBS cameras;
  7. the pipeline and refine_rig.
Both memory spaces (NumPy HOST, torch DEVICE), both record and keypoint dtypes, out_xyzs == xyzs.
"""
import ctypes as ct
import os
import subprocess

import numpy as np
import pytest

import huber_cases as hc
import pose_cases as pc
import refine_cases as rc
from snowmocap_amd import _lib, pose
from snowmocap_amd import refine as rf

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EPS = np.finfo(np.float64).eps
MISSING, FEW, KEPT, MOVED = rf.REFINE_MISSING, rf.REFINE_FEW_VIEWS, rf.REFINE_KEPT, rf.REFINE_MOVED
CODE = {"float32": _lib.F32, "float64": _lib.F64}


@pytest.fixture(scope="module")
def api():
    import snowmocap_amd as sm
    assert _lib.lib().snowtri_device_count() > 0, "these tests need the HIP device"
    return sm


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view({8: np.uint64, 4: np.uint32, 1: np.uint8}[a.dtype.itemsize])


def _same_bits(a, b):
    a, b = np.asarray(a), np.asarray(b)
    return a.dtype.itemsize == b.dtype.itemsize and a.shape == b.shape and np.array_equal(_bits(a), _bits(b))


def _host(a):
    return a.cpu().numpy() if hasattr(a, "cpu") else np.asarray(a)


def _dev(a):
    import torch
    if a is None:
        return None
    a = np.array(a, copy=True, order="C")                      # (the cases are read-only)
    return torch.from_numpy(a.view(np.int32) if a.dtype == np.uint32 else a).to("cuda:0")


def _joint_inputs(cs, start, space):
    """-> (xyzs, kpts, kwargs) of Context.refine_joints as host arrays or CUDA tensors (new copies: the case is read-only)."""
    kw = rc.refine_kwargs(cs)
    x, k = np.array(cs[start], copy=True), np.array(cs["kpts"], copy=True)
    if space == "torch":
        return _dev(x), _dev(k), dict(det_of=_dev(kw["det_of"]), n_persons=_dev(kw["n_persons"]), views=_dev(kw["views"]),
                                      keypoint_score_threshold=cs["thr"])
    return x, k, kw


def _joints(ctx, cs, start, space="numpy", in_place=False, **opts):
    x, k, kw = _joint_inputs(cs, start, space)
    res = ctx.refine_joints(x, k, diagnostics=True, out=x if in_place else None, **kw, **opts)
    if space == "torch":
        import torch
        torch.cuda.synchronize()
    res = tuple(_host(a) for a in res)
    return res[:3] + tuple(a.view(np.uint32) for a in res[3:])


def _p(a):
    return None if a is None else np.ascontiguousarray(a).ctypes.data_as(ct.c_void_p)


def _joints_ex_host(ctx, cs, start, huber_px, iters=4):
    """snowtri_refine_joints_ex itself on host arrays (Context.refine_joints takes the entry without the loss for huber_px = 0)."""
    kw = rc.refine_kwargs(cs)
    x, k = np.ascontiguousarray(cs[start]), np.ascontiguousarray(cs["kpts"])
    F, P, kn, _ = x.shape
    det = None if kw["det_of"] is None else np.ascontiguousarray(kw["det_of"], dtype=np.int32)
    npers = None if kw["n_persons"] is None else np.ascontiguousarray(kw["n_persons"], dtype=np.int32)
    views = None if kw["views"] is None else np.ascontiguousarray(kw["views"], dtype=np.uint32)
    out, cost, codes = np.empty_like(x), np.empty((F, P, kn, 2)), np.empty((F, P, kn), dtype=np.uint8)
    outl = np.full((F, P, kn), 0xdeadbeef, dtype=np.uint32)
    rcode = ctx.L.snowtri_refine_joints_ex(ctx.handle, F, P, kn, _p(x), CODE[str(x.dtype)], k.shape[2], _p(k), CODE[str(k.dtype)], _p(npers),
                                           _p(det), _p(views), float(cs["thr"]), iters, 0, float(huber_px), _p(out), _p(cost), _p(codes),
                                           _p(outl), _lib.HOST, None)
    assert rcode == _lib.OK, _lib.lib().snowtri_last_error()
    return out, cost, codes, outl


def _camera_inputs(cs, space):
    kw = dict(cs["kw"])
    x, k = np.array(cs["xyzs"], copy=True), np.array(cs["kpts"], copy=True)
    if space == "torch":
        kw.update(det_of=_dev(kw["det_of"]), n_persons=_dev(kw["n_persons"]), views=_dev(kw["views"]))
        return _dev(x), _dev(k), kw
    return x, k, kw


def _cameras(ctx, cs, space="numpy", **opts):
    x, k, kw = _camera_inputs(cs, space)
    R, t, rep = ctx.refine_cameras(x, k, diagnostics=True, **kw, **opts)
    if space == "torch":
        import torch
        torch.cuda.synchronize()
    return _host(R), _host(t), {key: _host(v) for key, v in rep.items()}


def _cameras_ex_host(ctx, cs, huber_px):
    kw = cs["kw"]
    x, k = np.ascontiguousarray(cs["xyzs"]), np.ascontiguousarray(cs["kpts"])
    F, P, kn, _ = x.shape
    C = cs["K"].shape[0]
    det = None if kw["det_of"] is None else np.ascontiguousarray(kw["det_of"], dtype=np.int32)
    npers = None if kw["n_persons"] is None else np.ascontiguousarray(kw["n_persons"], dtype=np.int32)
    views = None if kw["views"] is None else np.ascontiguousarray(kw["views"], dtype=np.uint32)
    R, t = np.empty((C, 3, 3)), np.empty((C, 3))
    rep = dict(cost=np.empty((C, 2)), n_obs=np.empty(C, dtype=np.int64), codes=np.empty(C, dtype=np.uint8), normal=np.empty((C, 28)),
               n_outliers=np.full(C, -7, dtype=np.int64))
    rcode = ctx.L.snowtri_refine_cameras_ex(ctx.handle, F, P, kn, _p(x), CODE[str(x.dtype)], k.shape[2], _p(k), CODE[str(k.dtype)], _p(npers),
                                            _p(det), _p(views), float(cs["thr"]), _lib.free_mask(kw["free"], C), kw["min_obs"], kw["iters"], 0,
                                            float(huber_px), _p(R), _p(t), _p(rep["cost"]), _p(rep["n_obs"]), _p(rep["codes"]),
                                            _p(rep["normal"]), _p(rep["n_outliers"]), _lib.HOST, None)
    assert rcode == _lib.OK, _lib.lib().snowtri_last_error()
    return R, t, rep


# ------------------------------------------------------------------------------------------------ 1. the squared path
@pytest.mark.parametrize("rec_dtype", ["float64", "float32"])
@pytest.mark.parametrize("rig_name", hc.KERNEL_RIGS)
def test_huber_0_and_1e6_are_the_squared_loss_bit_for_bit_joints(api, rig_name, rec_dtype):
    K, R, t = rc.rig(rig_name)
    ctx = _lib.Context(K, R, t)
    n = 0
    for shape in rc.SHAPES:
        for kp_dtype in ("float64", "float32") if shape == (2, 3, 21) else ("float64",):
            cs = hc.joint_case(rig_name, shape, rec_dtype, kp_dtype)
            for start in rc.STARTS:
                base = _joints(ctx, cs, start)
                assert len(base) == 3
                runs = [_joints_ex_host(ctx, cs, start, 0.0), _joints_ex_host(ctx, cs, start, hc.BIG_DELTA),
                        _joints(ctx, cs, start, huber_px=hc.BIG_DELTA), _joints(ctx, cs, start, "torch", huber_px=hc.BIG_DELTA),
                        _joints(ctx, cs, start, "torch", in_place=True, huber_px=hc.BIG_DELTA),
                        _joints(ctx, cs, start, in_place=True, huber_px=hc.BIG_DELTA)]
                for run in runs:
                    assert len(run) == 4 and (run[3] == 0).all(), (shape, start)
                    for k in range(3):
                        assert _same_bits(run[k], base[k]), (shape, kp_dtype, start, k)
                for same in (_joints(ctx, cs, start, huber_px=None), _joints(ctx, cs, start, huber_px=0), _joints(ctx, cs, start, "torch", huber_px=0.0)):
                    assert len(same) == 3 and all(_same_bits(same[k], base[k]) for k in range(3))
                n += int((base[2] == MOVED).sum())
    ctx.close()
    assert n > 1000


@pytest.mark.parametrize("dtype", ["float64", "float32"])
@pytest.mark.parametrize("rig_name", hc.KERNEL_RIGS)
def test_huber_0_and_1e6_are_the_squared_loss_bit_for_bit_cameras(api, rig_name, dtype):
    moved = 0
    for shape in pc.SHAPES:
        cs = hc.pose_case(rig_name, shape, dtype, dtype)
        ctx = _lib.Context(cs["K"], cs["Rd"], cs["td"])
        base = _cameras(ctx, cs)
        assert "n_outliers" not in base[2]
        for run in (_cameras_ex_host(ctx, cs, 0.0), _cameras_ex_host(ctx, cs, hc.BIG_DELTA), _cameras(ctx, cs, huber_px=hc.BIG_DELTA),
                    _cameras(ctx, cs, "torch", huber_px=hc.BIG_DELTA)):
            assert _same_bits(run[0], base[0]) and _same_bits(run[1], base[1]), shape
            for key in ("cost", "n_obs", "codes", "normal"):
                assert _same_bits(run[2][key], base[2][key]), (shape, key)
            assert (run[2]["n_outliers"] == 0).all()
        for same in (_cameras(ctx, cs, huber_px=None), _cameras(ctx, cs, "torch", huber_px=0)):
            assert "n_outliers" not in same[2] and _same_bits(same[0], base[0]) and _same_bits(same[1], base[1])
        moved += int((base[2]["codes"] == pose.POSE_MOVED).sum())
        ctx.close()
    assert moved > 0


# ------------------------------------------------------------------------------------------------ 2., 3. costs and outliers
@pytest.mark.parametrize("rec_dtype", ["float64", "float32"])
@pytest.mark.parametrize("rig_name", hc.KERNEL_RIGS)
def test_joint_costs_and_outliers_are_the_rules(api, rig_name, rec_dtype):
    """cost[., 0]: the NumPy rule's E at the input, bit for bit.  float64 records: cost[., 1] is the rule's E at the kernel's own output
    point and `outliers` the rule's regimes there, bit for bit.  float32 records: the output is rounded after the kernel classified
    its views, so a view whose residual lies within huber_cases.pixel_margin of delta at the rounded point is excused.  No cost rises;
    MISSING / FEW_VIEWS and their records' bits are the rule's; copied records have no outliers."""
    K, R, t = rc.rig(rig_name)
    ctx = _lib.Context(K, R, t)
    refined = flagged = excused = 0
    for shape in rc.SHAPES:
        for kp_dtype in ("float64", "float32") if shape == (2, 3, 21) else ("float64",):
            cs = hc.joint_case(rig_name, shape, rec_dtype, kp_dtype)
            for delta in hc.DELTAS:
                for start, space, in_place in (("dlt", "numpy", False), ("pair", "torch", False), ("dlt", "torch", True), ("pair", "numpy", True)):
                    out, cost, codes, outl = _joints(ctx, cs, start, space, in_place, huber_px=delta)
                    r_out, r_cost, r_codes, used, r_outl = hc.joint_reference(rig_name, shape, start, delta, rec_dtype, kp_dtype)
                    what = (shape, kp_dtype, delta, start, space)
                    x = cs[start]
                    copied = r_codes < KEPT
                    assert np.array_equal(codes < KEPT, copied) and np.array_equal(codes[copied], r_codes[copied]), what
                    assert out.dtype == x.dtype and np.array_equal(_bits(out)[copied], _bits(x)[copied]), what
                    assert np.array_equal(_bits(out[..., 3]), _bits(x[..., 3])) and (cost[copied] == 0).all() and (outl[copied] == 0).all()
                    assert np.array_equal(_bits(out)[codes == KEPT], _bits(x)[codes == KEPT]), what
                    assert (cost[..., 1] <= cost[..., 0]).all(), what
                    assert (outl & ~used == 0).all(), what
                    ref = ~copied
                    assert _same_bits(cost[..., 0][ref], r_cost[..., 0][ref]), what
                    e_out, lin, s = hc.rule_at(cs, start, out, used, delta)
                    if rec_dtype == "float64":
                        diff = _bits(cost[..., 1][ref]) != _bits(e_out[ref])
                        assert not diff.any(), (what, int(diff.sum()), float(np.abs(cost[..., 1][ref] - e_out[ref]).max()))
                        assert np.array_equal(outl[ref], lin[ref]), what
                    else:
                        margin = hc.pixel_margin(cs, out)
                        near = np.zeros_like(outl)
                        for c in range(K.shape[0]):
                            close = np.abs(np.sqrt(s[c]) - delta) <= margin
                            near |= close.astype(np.uint32) << np.uint32(c)
                        wrong = (outl ^ lin) & ~near
                        assert (wrong[ref] == 0).all(), what
                        excused += int(hc.popcount((outl ^ lin) & near)[ref].sum())
                    refined += int(ref.sum())
                    flagged += int((outl[ref] != 0).sum())
    ctx.close()
    print(f"    {rig_name} {rec_dtype}: {refined} refined records, {flagged} with an outlier at the output, {excused} views excused")
    assert refined > 1000 and flagged > 100


# ------------------------------------------------------------------------------------------------ 4. accuracy of joints
@pytest.mark.parametrize("rig_name", hc.ACCURACY_RIGS)
def test_refined_joints_against_the_exact_huber_minimiser(api, rig_name):
    """float64 records, iters = 16, shape (2, 3, 21): every covered record (huber_cases.joint_minimiser: the 50-digit IRLS minimiser
    settled and leaves at least 3 views in the quadratic regime) within huber_cases.JOINT_BAR = 4 x the floor the NumPy rule shows
    on the CPU; the covered records are at least 80 % of the refined ones."""
    K, R, t = rc.rig(rig_name)
    scale = rc.rig_scale(t)
    ctx = _lib.Context(K, R, t)
    cs = hc.joint_case(rig_name, hc.ACCURACY_SHAPE)
    for delta in hc.DELTAS:
        mn = hc.joint_minimiser(rig_name, delta)
        share = mn["covered"].sum() / mn["refined"].sum()
        assert share >= hc.MIN_COVERED, (delta, share)
        for space in ("numpy", "torch"):
            out, cost, codes, outl = _joints(ctx, cs, "dlt", space, iters=hc.ACCURACY_ITERS, huber_px=delta)
            assert np.array_equal(codes >= KEPT, mn["refined"])
            d = np.linalg.norm(out[..., :3] - mn["X"], axis=-1)[mn["covered"]] / scale
            print(f"    {rig_name} delta {delta} {space}: {int(mn['covered'].sum())} of {int(mn['refined'].sum())} covered ({share:.0%}); "
                  f"max |k_refine - minimiser| = {d.max():.2e} of the rig scale; bar {hc.JOINT_BAR:.2e}")
            assert d.max() <= hc.JOINT_BAR, (delta, space, float(d.max()))
    ctx.close()


# ------------------------------------------------------------------------------------------------ 5. independence
@pytest.mark.parametrize("rig_name", ["floor", "ring8", "ring3"])
def test_bits_do_not_depend_on_how_the_batch_is_cut(api, rig_name):
    cs = hc.joint_case(rig_name, rc.CUT_SHAPE)
    K, R, t = rc.rig(rig_name)
    ctx = _lib.Context(K, R, t)
    kw = rc.refine_kwargs(cs)
    for delta in hc.DELTAS:
        whole = _joints(ctx, cs, "dlt", huber_px=delta)
        assert (whole[2] == MOVED).sum() > 3000 and (whole[3] != 0).sum() > 300
        for cut in rc.CUTS:
            parts = [ctx.refine_joints(cs["dlt"][s], cs["kpts"][s], det_of=kw["det_of"][s], n_persons=kw["n_persons"][s], views=kw["views"][s],
                                       keypoint_score_threshold=cs["thr"], diagnostics=True, huber_px=delta) for s in (slice(0, cut), slice(cut, None))]
            for k in range(4):
                assert _same_bits(np.concatenate([parts[0][k], parts[1][k]]), whole[k]), (delta, cut, k)
        dev = _joints(ctx, cs, "dlt", "torch", huber_px=delta)
        for k in range(4):
            assert _same_bits(dev[k], whole[k]), (delta, k)
    ctx.close()


# ------------------------------------------------------------------------------------------------ 6. cameras
@pytest.mark.parametrize("dtype", ["float64", "float32"])
@pytest.mark.parametrize("rig_name", hc.KERNEL_RIGS)
def test_cameras_counts_bits_and_outliers(api, rig_name, dtype):
    """n_obs is the rule's exactly; two runs and the two memory spaces give the same bits; the cost does not rise; a FIXED or FEW_OBS
    camera keeps its pose bit for bit and reports no outliers; n_outliers is the rule's count at the kernel's own output pose (no
    observation of these cases lies within 1e-9, relative, of delta there: asserted first); `normal` agrees with the NumPy rule's
    E, g, H of the loss within pose_cases' bound."""
    moved = 0
    for shape in pc.SHAPES:
        cs = hc.pose_case(rig_name, shape, dtype, dtype)
        C = cs["K"].shape[0]
        ctx = _lib.Context(cs["K"], cs["Rd"], cs["td"])
        for delta in hc.DELTAS:
            R, t, rep = _cameras(ctx, cs, huber_px=delta)
            again = _cameras(ctx, cs, huber_px=delta)
            dev = _cameras(ctx, cs, "torch", huber_px=delta)
            for other in (again, dev):
                assert _same_bits(other[0], R) and _same_bits(other[1], t)
                for key in rep:
                    assert _same_bits(other[2][key], rep[key]), (shape, delta, key)
            Rr, tr, rrep, S = hc.pose_reference(rig_name, shape, delta, dtype, dtype)
            assert np.array_equal(rep["n_obs"], rrep["n_obs"]) and rep["n_outliers"].dtype == np.int64, (shape, delta)
            still = rrep["codes"] < pose.POSE_KEPT
            assert np.array_equal(rep["codes"] < pose.POSE_KEPT, still) and np.array_equal(rep["codes"][still], rrep["codes"][still])
            assert _same_bits(R[still], np.ascontiguousarray(cs["Rd"][still])) and _same_bits(t[still], np.ascontiguousarray(cs["td"][still]))
            assert (rep["n_outliers"][still] == 0).all() and (rep["cost"][still] == 0).all()
            assert (rep["cost"][:, 1] <= rep["cost"][:, 0]).all()
            X, _, obs = rf.observation_sets(cs["K"], cs["Rd"], cs["td"], cs["xyzs"], cs["kpts"], cs["det_of"], cs["n_persons"], cs["views"], cs["thr"])
            for c in range(C):
                Xc, ou, ov, w = X[S[c]], obs[c, S[c], 0], obs[c, S[c], 1], obs[c, S[c], 2]
                ref_n, _ = pose.evaluate_camera(cs["K"][c], cs["Rd"][c], cs["td"][c], Xc, ou, ov, w, delta)
                mag = np.abs(pose.normal_terms(cs["K"][c], cs["Rd"][c], cs["td"][c], Xc, ou, ov, w, delta)[0]).sum(axis=0)
                assert (np.abs(rep["normal"][c] - ref_n) <= 2 * pc.MARGIN * pc.NORMAL_UNITS * EPS * mag).all(), (shape, delta, c)
                if still[c]:
                    continue
                _, _, _, u, v, _ = rf.project_camera(cs["K"][c], R[c], t[c], Xc)
                r = np.sqrt((u - ou) ** 2 + (v - ov) ** 2)
                assert (np.abs(r - delta) > hc.NEAR_DELTA * delta).all(), (shape, delta, c)
                assert rep["n_outliers"][c] == int(pose.linear_regime(cs["K"][c], R[c], t[c], Xc, ou, ov, delta).sum()), (shape, delta, c)
                assert 0 < rep["n_outliers"][c] < rep["n_obs"][c] or rep["n_obs"][c] < 20
                e_here, _ = pose.evaluate_camera(cs["K"][c], R[c], t[c], Xc, ou, ov, w, delta)
                assert abs(rep["cost"][c, 1] - e_here[0]) <= pc.MARGIN * pc.NORMAL_UNITS * EPS * e_here[0], (shape, delta, c)
            moved += int((rep["codes"] == pose.POSE_MOVED).sum())
        ctx.close()
    assert moved > 0


@pytest.mark.parametrize("rig_name", hc.POSE_MINIMISER_RIGS)
def test_cameras_against_50_digit_sums_and_the_exact_huber_minimiser(api, rig_name):
    """`normal` at the input pose against a 50-digit evaluation of the loss' E, g, H, within MARGIN x NORMAL_UNITS eps * sum |term|
    (pose_cases' convention); the poses within MARGIN x huber_cases.POSE_FLOOR of the 50-digit minimiser of the loss."""
    shape = hc.POSE_MINIMISER_SHAPE
    cs = hc.pose_case(rig_name, shape)
    ctx = _lib.Context(cs["K"], cs["Rd"], cs["td"])
    for delta in hc.DELTAS:
        R, t, rep = _cameras(ctx, cs, huber_px=delta)
        S = hc.pose_reference(rig_name, shape, delta)[3]
        worst = 0.0
        for c in range(min(cs["K"].shape[0], 5)):
            X, ou, ov, w = hc.camera_observations(cs, S, c)
            val, mag = hc.exact_huber_normal(cs["K"][c], cs["Rd"][c], cs["td"][c], X, ou, ov, w, delta)
            assert rep["n_obs"][c] == len(X) > 0 and (mag > 0).all()
            worst = max(worst, float((np.abs(rep["normal"][c] - val) / (EPS * mag)).max()))
        assert worst <= pc.MARGIN * pc.NORMAL_UNITS, (delta, worst)
        mn = hc.pose_minimiser(rig_name, delta)
        cams = list(mn["cams"])
        assert cams and (rep["codes"][cams] == pose.POSE_MOVED).all()
        eR, et = pc.pose_error(R, t, mn["R"], mn["t"], cams)
        print(f"    {rig_name} delta {delta}: normal within {worst:.1f} eps sum |term|; |R - R_min| = {eR:.2e}, |t - t_min| / rig scale = {et:.2e}")
        assert eR <= pc.MARGIN * hc.POSE_FLOOR[0] and et <= pc.MARGIN * hc.POSE_FLOOR[1], (delta, eR, et)
    ctx.close()


def test_camera_group_takes_the_keyword(api):
    from snowmocap_amd.camera import CameraGroup
    cs = hc.pose_case("floor", (6, 2, 17))
    ctx = _lib.Context(cs["K"], cs["Rd"], cs["td"])
    R, t, rep = _cameras(ctx, cs, huber_px=3.0)
    R2, t2, rep2 = pose.refine_cameras(ctx, cs["xyzs"], cs["kpts"], diagnostics=True, huber_px=3.0, **cs["kw"])
    assert _same_bits(R2, R) and _same_bits(t2, t) and np.array_equal(rep2["n_outliers"], rep["n_outliers"])
    ctx.close()
    group = CameraGroup(cap_ids=list(range(4)), resolutions=[(1280, 720)] * 4)
    for c, cam in enumerate(group.cameras):
        cam.K, cam.R, cam.t = np.array(cs["K"][c]), np.array(cs["Rd"][c]), np.array(cs["td"][c]).reshape(3, 1)
    new, grep = group.refine_poses(cs["xyzs"], cs["kpts"], diagnostics=True, huber_px=3.0, **cs["kw"])
    _, Rn, tn = new.rig_arrays()
    assert np.array_equal(grep["n_outliers"], rep["n_outliers"]) and _same_bits(Rn, R) and _same_bits(tn, t)
    plain, prep = group.refine_poses(cs["xyzs"], cs["kpts"], diagnostics=True, **cs["kw"])
    assert "n_outliers" not in prep and not _same_bits(plain.rig_arrays()[1], Rn)


# ------------------------------------------------------------------------------------------------ 7. the pipeline and the rig
def test_pipeline_adds_refine_outliers_and_nothing_else_changes(api):
    import torch
    import pipeline_cases as plc
    from snowmocap_amd import reproject as rp
    sc = plc.scene("fixed", False)
    K, R, t = sc["rig"]
    pipe = api.TrackPipeline(K, R, t, sc["params"], plc.SMOOTH_PROFILE, n_persons_out=sc["slots"])
    assert sc["kpts"].shape[0] == 72
    squared = pipe.run(sc["kpts"], sc["n_persons"], refine=(4, 6.0, False))
    for off in ((4, 6.0, False, None), (4, 6.0, False, 0), (4, 6.0, False, 0.0)):
        same = pipe.run(sc["kpts"], sc["n_persons"], refine=off)
        assert list(same) == list(squared)
        for k in squared:
            assert _same_bits(_host(same[k]), _host(squared[k])), k
    res = pipe.run(sc["kpts"], sc["n_persons"], refine=(4, 6.0, False, 3.0))
    assert list(res) == list(squared) + ["refine_outliers"]
    plain = pipe.run(sc["kpts"], sc["n_persons"])
    ctx = pipe.bt.ctx
    kp = torch.from_numpy(np.ascontiguousarray(sc["und"][:, :, :, :pipe.kn])).to("cuda:0")
    npers = torch.from_numpy(np.ascontiguousarray(sc["n_persons"])).to("cuda:0")
    thr = float(sc["params"]["keypoint_score_threshold"])
    s, n = ctx.reproject_cost(plain["xyzs"], kp, n_persons=npers, keypoint_score_threshold=thr)
    det_of, _ = rp.match_detections(s, n, 6.0)
    want, cost, codes, outl = rf.refine_joints(ctx, plain["xyzs"], kp, det_of=det_of, n_persons=npers, keypoint_score_threshold=thr, iters=4,
                                               diagnostics=True, huber_px=3.0)
    assert _same_bits(_host(res["xyzs"]), _host(want)) and _same_bits(_host(res["refine_cost"]), _host(cost))
    assert _same_bits(_host(res["refine_codes"]), _host(codes)) and _same_bits(_host(res["refine_outliers"]), _host(outl))
    assert not _same_bits(_host(res["xyzs"]), _host(squared["xyzs"])) and not _same_bits(_host(res["smoothed"]), _host(squared["smoothed"]))
    for k in ("count", "flags", "tracked", "refine_codes"):      # what the loss does not change on this scene
        assert _same_bits(_host(res[k]), _host(squared[k])), k
    o = _host(res["refine_outliers"]).view(np.uint32)
    assert res["refine_outliers"].shape == res["refine_codes"].shape and (o[_host(codes) < KEPT] == 0).all()
    for bad in ((4, 6.0, False, -1.0), (4, 6.0, False, float("nan")), (4, 6.0, False, 2e150), (4, 6.0, False, 3.0, 1)):
        with pytest.raises(ValueError):
            pipe.run(sc["kpts"], sc["n_persons"], refine=bad)
    pipe.close()


def test_refine_rig_with_the_loss_against_the_rule_driven_alternation(api):
    """pose.refine_rig(huber_px=3) on the GPU against the same alternation by the NumPy rules, as tests/test_gpu_pose.py compares the
    two without the loss: the poses within 4 x pose_cases.FLOOR_NOISY, the view RMS to 1e-6 px, codes and n_obs equal.  The recipe's
    detections carry the outliers, so the matching gate is 40 px (a person's RMS over its views is 25 px with them; at the default
    12 px nobody is matched and the camera has too few observations to move)."""
    rp_ = pc.recipe()
    bad = rp_["bad"]
    kp, _ = hc._moved(rp_["kpts"], rc._seed("huber-rig"))
    args = (rp_["K"], rp_["Rd"], rp_["td"], kp)
    kw = dict(free=[bad], triangulate=pc.dlt_points, params=dict(keypoint_score_threshold=0.5), huber_px=3.0, gate_px=40.0)
    bar = tuple(pc.MARGIN * f for f in pc.FLOOR_NOISY)
    for rounds in (1, 2):
        R, t, hist = pose.refine_rig(*args, rounds=rounds, **kw)
        Rr, tr, hr = pose.refine_rig(*args, rounds=rounds, reference=True, **kw)
        eR, et = pc.pose_error(R, t, Rr, tr, [bad])
        print(f"    after round {rounds}: |R - R_rule| = {eR:.2e}, |t - t_rule| / rig scale = {et:.2e}; view RMS {hist[-1]['view_rms'][bad]:.3f} px")
        assert eR <= bar[0] and et <= bar[1], (rounds, eR, et)
        assert all(h["codes"][bad] == pose.POSE_MOVED and h["n_obs"][bad] > 1000 for h in hist[:-1])
        for h, g in zip(hist, hr):
            assert np.allclose(h["view_rms"], g["view_rms"], rtol=0, atol=1e-6)
            if "codes" in h:
                assert np.array_equal(h["codes"], g["codes"]) and np.array_equal(h["n_obs"], g["n_obs"])
        keep = [c for c in range(8) if c != bad]
        assert _same_bits(R[keep], np.ascontiguousarray(rp_["Rd"][keep])) and _same_bits(t[keep], np.ascontiguousarray(rp_["td"][keep]))
    # what the loss is for: the squared loss on the same detections leaves the nudged camera further from the truth than it started
    Rs, ts, _ = pose.refine_rig(*args, rounds=2, **{**kw, "huber_px": None})
    e0, eh, es = (pc.pose_error(a, b, rp_["R"], rp_["t"], [bad]) for a, b in ((rp_["Rd"], rp_["td"]), (R, t), (Rs, ts)))
    print(f"    pose error (|R - R_true|, |t - t_true| / scale): drifted {e0[0]:.2e} {e0[1]:.2e}, huber {eh[0]:.2e} {eh[1]:.2e}, squared {es[0]:.2e} {es[1]:.2e}")
    assert eh[0] < 0.5 * e0[0] and eh[0] < 0.5 * es[0] and eh[1] < 0.5 * es[1]
    with pytest.raises(ValueError):
        pose.refine_rig(*args, rounds=1, **{**kw, "huber_px": -3.0})


# ------------------------------------------------------------------------------------------------ refusals, bad arguments, debug build
def test_wrapper_refusals(api):
    cs = hc.joint_case("ring5", (2, 3, 21))
    ctx = _lib.Context(cs["K"], cs["R"], cs["t"])
    kw = rc.refine_kwargs(cs)
    ps = hc.pose_case("ring5", (2, 3, 21))
    for bad in (-1.0, float("nan"), float("inf"), -float("inf"), 1.1e150):
        with pytest.raises(ValueError, match="huber_px"):
            ctx.refine_joints(cs["dlt"], cs["kpts"], huber_px=bad, **kw)
        with pytest.raises(ValueError, match="huber_px"):
            rf.refine_joints(ctx, cs["dlt"], cs["kpts"], huber_px=bad, **kw)
        with pytest.raises(ValueError, match="huber_px"):
            ctx.refine_cameras(ps["xyzs"], ps["kpts"], huber_px=bad, **ps["kw"])
        with pytest.raises(ValueError, match="huber_px"):
            pose.refine_cameras(ctx, ps["xyzs"], ps["kpts"], huber_px=bad, **ps["kw"])
    for space in (_lib.HOST, _lib.DEVICE):
        assert ctx.L.snowtri_refine_joints_ex(ctx.handle, 0, 3, 21, None, _lib.F64, 4, None, _lib.F32, None, None, None, 0.5, 4, 0, 3.0, None,
                                              None, None, None, space, None) == _lib.OK
        assert ctx.L.snowtri_refine_joints_ex(ctx.handle, 0, 3, 21, None, _lib.F64, 4, None, _lib.F32, None, None, None, 0.5, 4, 0,
                                              float("nan"), None, None, None, None, space, None) == _lib.ERR_BAD_ARG
    out, cost, codes, outl = ctx.refine_joints(cs["dlt"][:0], cs["kpts"][:0], diagnostics=True, huber_px=3.0)
    assert out.shape == (0, 3, 21, 4) and outl.shape == (0, 3, 21) and outl.dtype == np.uint32
    assert isinstance(ctx.refine_joints(cs["dlt"], cs["kpts"], huber_px=3.0, **kw), np.ndarray)       # no diagnostics: the records alone
    ctx.close()


def test_entries_reject_bad_arguments_on_a_real_context(api, tmp_path):
    """tests/abi_badargs_huber.c against libsnowtri.so on the GPU."""
    lib_dir = os.path.join(ROOT, "snowmocap_amd")
    exe = str(tmp_path / "abi_badargs_huber")
    subprocess.check_call(["gcc", "-std=c99", "-O1", "-I", os.path.join(ROOT, "include"), os.path.join(ROOT, "tests", "abi_badargs_huber.c"),
                           "-o", exe, "-L", lib_dir, "-lsnowtri", "-Wl,-rpath," + lib_dir])
    out = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0 and "0 failure(s)" in out.stdout, out.stdout[-3000:] + out.stderr[-2000:]


DBG_CODE = r'''
import sys, numpy as np
sys.path.insert(0, %(root)r)
sys.path.insert(0, %(tests)r)
import huber_cases as hc, refine_cases as rc
from snowmocap_amd import _lib
assert _lib.LIB_PATH.endswith("libsnowtri_dbg.so") and "SNOWTRI_DEBUG_BOUNDS" in _lib.build_info()["variants"]
for rig_name, shape, dt in (("floor", (5, 2, 133), "float64"), ("ring8", (1, 1, 65), "float32"), ("ring16", (2, 3, 21), "float64"), ("ring3", (1, 1, 1), "float64")):
    cs = hc.joint_case(rig_name, shape, dt)
    ctx = _lib.Context(cs["K"], cs["R"], cs["t"])
    out, cost, codes, outl = ctx.refine_joints(cs["dlt"], cs["kpts"], diagnostics=True, huber_px=3.0, **rc.refine_kwargs(cs))
    ref = hc.joint_reference(rig_name, shape, "dlt", 3.0, dt)
    assert np.array_equal(codes < 2, ref[2] < 2) and (cost[..., 1] <= cost[..., 0]).all()
    n, first = ctx.debug_faults()
    assert n == 0, "device-side bounds check failed %%d times; first: code %%d at line %%d" %% (n, first >> 32, first & 0xffffffff)
    ctx.close()
for rig_name, shape, dt in (("floor", (6, 2, 17), "float64"), ("ring8", (1, 1, 65), "float32"), ("ring16", (2, 3, 21), "float64"), ("ring3", (1, 1, 257), "float64")):
    cs = hc.pose_case(rig_name, shape, dt, dt)
    ctx = _lib.Context(cs["K"], cs["Rd"], cs["td"])
    R, t, rep = ctx.refine_cameras(cs["xyzs"], cs["kpts"], diagnostics=True, huber_px=3.0, **cs["kw"])
    ref = hc.pose_reference(rig_name, shape, 3.0, dt, dt)
    assert np.array_equal(rep["n_obs"], ref[2]["n_obs"]) and (rep["n_outliers"] <= rep["n_obs"]).all()
    n, first = ctx.debug_faults()
    assert n == 0, "device-side bounds check failed %%d times; first: code %%d at line %%d" %% (n, first >> 32, first & 0xffffffff)
    ctx.close()
print("huber debug-bounds ok")
'''


def test_debug_build_counts_no_fault():
    dbg = os.path.join(ROOT, "snowmocap_amd", "libsnowtri_dbg.so")
    assert os.path.exists(dbg), f"{dbg} is missing: `make -C snowmocap_amd/csrc debug`"
    import sys
    env = dict(os.environ, SNOWTRI_LIB=dbg)
    code = DBG_CODE % {"root": ROOT, "tests": os.path.join(ROOT, "tests")}
    p = subprocess.run([sys.executable, "-c", code], env=env, capture_output=True, text=True, timeout=300)
    assert p.returncode == 0 and "huber debug-bounds ok" in p.stdout, p.stdout[-2000:] + p.stderr[-3000:]
