"""k_refine behind snowtri_refine_joints (include/snowtri.h, "Refinement"), Context.refine_joints / refine.refine_joints and
TrackPipeline.run(refine=...).  Inputs: tests/refine_cases.py.

  * accuracy: the kernel's float64 output against the 50-digit minimiser of the same records, every refined record, within
    refine_cases.BAR (4 x the floor the NumPy rule shows on the CPU) of the rig scale; float32 records: plus half a float32 ulp of the
    coordinate.  At the six placements the refined points, mapped back, agree with the home placement's within the same bar.
  * never worse: cost_out <= cost_in on every record, recomputed in plain NumPy from the kernel's input and output (64 eps of
    relative slack on that recomputation), including a batch with synth.add_outliers; the kernel's own cost array agrees with the
    recomputation to 128 eps of the sum -- at sigma = 0 too, where the costs are squares of pixel roundings: the kernel forms E in
    the rule's own plain operations.
  * classes against the NumPy rule: MISSING / FEW_VIEWS equal everywhere and those records bit-identical to the input; KEPT / MOVED
    equal where sigma >= 1 (at sigma = 0 acceptance is decided by rounding).
  * a record's bits are its own: cuts of a 40-frame batch, the reversed batch, in place against out of place, HOST against DEVICE,
    NumPy against torch.
  * fixed point, the routes (PAIRWISE, DLT, DLT_ROBUST with its views, the multi-person route with match_detections' det_of), the
    pipeline, the bad-arguments program, the debug build.
"""
import os
import subprocess

import numpy as np
import pytest

import dlt_frames_cases as fc
import refine_cases as rc
import reproject_cases
import undistort_cases as uc
from snowmocap_amd import _lib, synth
from snowmocap_amd import refine as rf
from snowmocap_amd import reproject as rp
from snowmocap_amd.records import missing_records

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EPS = np.finfo(np.float64).eps
MISSING, FEW, KEPT, MOVED = rf.REFINE_MISSING, rf.REFINE_FEW_VIEWS, rf.REFINE_KEPT, rf.REFINE_MOVED


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


def _run(ctx, cs, start, iters=4, **kw):
    return ctx.refine_joints(cs[start], cs["kpts"], iters=iters, diagnostics=True, **rc.refine_kwargs(cs), **kw)


def _cost_numpy(cs, rec, used):
    """E of the records `rec` over the view sets `used` in plain NumPy, the views summed in camera order [F, P, kn]."""
    K, R, t = cs["K"], cs["R"], cs["t"]
    F, P, kn = used.shape
    kp = np.asarray(cs["kpts"]).astype(np.float64)
    x = np.asarray(rec).astype(np.float64)
    u, v, _, _ = rp._project(K, R, t, None, False, np.where(np.isfinite(x), x, 0.0))
    E = np.zeros((F, P, kn))
    for c in range(K.shape[0]):
        q = np.broadcast_to(np.arange(P), (F, P)) if cs["det_of"] is None else np.maximum(cs["det_of"][:, c], 0)
        obs = np.take_along_axis(kp[:, c], q[:, :, None, None], axis=1)                          # [F, P, kn, 3]
        du, dv = u[:, c] - obs[..., 0], v[:, c] - obs[..., 1]
        E = E + np.where(((used >> np.uint32(c)) & 1).astype(bool), du * du + dv * dv, 0.0)
    return E


# ------------------------------------------------------------------------------------------------ accuracy
@pytest.mark.parametrize("rig_name", rc.RIGS)
def test_refined_joints_against_the_exact_minimiser(api, rig_name):
    K, R, t = rc.rig(rig_name)
    scale = rc.rig_scale(t)
    ctx = _lib.Context(K, R, t)
    worst = 0.0
    for sigma in (1.0, 2.0):
        for kp_dtype in ("float64", "float32"):
            mn = rc.minimiser(rig_name, sigma, kp_dtype)
            cs = rc.case(rig_name, rc.MINIMISER_SHAPE, sigma, True, "float64", kp_dtype)
            rc.assert_domain(cs)
            for start in rc.STARTS:
                out, cost, codes = _run(ctx, cs, start, rc.ACCURACY_ITERS)
                assert np.array_equal(codes >= KEPT, mn["refined"])
                d = np.linalg.norm(out[..., :3] - mn["X"], axis=-1)[mn["refined"]] / scale
                worst = max(worst, float(d.max()))
                assert d.max() <= rc.BAR, (sigma, kp_dtype, start, float(d.max()))
    # float32 records: the minimiser of the view sets fixed at the rounded start; the output is rounded once more
    mn = rc.minimiser(rig_name, 1.0, "float64", "float32")
    cs = rc.case(rig_name, rc.MINIMISER_SHAPE, 1.0, True, "float32", "float64")
    out, _, codes = _run(ctx, cs, "dlt", rc.ACCURACY_ITERS)
    assert out.dtype == np.float32 and np.array_equal(codes >= KEPT, mn["refined"])
    err = np.abs(out[..., :3].astype(np.float64) - mn["X"])[mn["refined"]]
    assert (err <= rc.BAR * scale + 0.5 * uc.f32_ulp(mn["X"][mn["refined"]])).all()
    ctx.close()
    print(f"    {rig_name}: max |k_refine - exact minimiser| = {worst:.2e} of the rig scale ({worst * scale:.2e} m); bar {rc.BAR:.2e}")


@pytest.mark.parametrize("rig_name", rc.RIGS)
def test_refined_joints_do_not_depend_on_where_the_world_stands(api, rig_name):
    home = None
    scale = rc.rig_scale(rc.rig(rig_name)[2])
    mn = rc.minimiser(rig_name, 1.0)
    for placement in rc.PLACEMENTS:
        cs = rc.case(rig_name, rc.MINIMISER_SHAPE, 1.0, True, "float64", "float64", placement)
        ctx = _lib.Context(cs["K"], cs["R"], cs["t"])
        out, cost, codes = _run(ctx, cs, "dlt", rc.ACCURACY_ITERS)
        ctx.close()
        back = fc.home(out[..., :3], placement)
        if home is None:
            home = (back, codes)
        assert np.array_equal(codes, home[1]), placement
        ref = codes >= KEPT
        d = np.linalg.norm(back - home[0], axis=-1)[ref].max() / scale
        dm = np.linalg.norm(back - mn["X"], axis=-1)[ref].max() / scale
        assert d <= rc.BAR and dm <= rc.BAR, (placement, float(d), float(dm))


# ------------------------------------------------------------------------------------------------ never worse, classes, costs
def _check_against_the_rule(ctx, cs, ref, start, sigma, figures):
    out, cost, codes = _run(ctx, cs, start)
    r_out, r_cost, r_codes, used = ref
    x = cs[start]
    copied = r_codes < KEPT
    assert np.array_equal(codes < KEPT, copied) and np.array_equal(codes[copied], r_codes[copied])
    assert out.dtype == x.dtype and np.array_equal(_bits(out)[copied], _bits(x)[copied])
    assert np.array_equal(_bits(out[..., 3]), _bits(x[..., 3])) and (cost[copied] == 0).all()
    assert np.array_equal(_bits(out)[codes == KEPT], _bits(x)[codes == KEPT])
    if sigma >= 1.0:
        assert np.array_equal(codes, r_codes)
    assert (cost[..., 1] <= cost[..., 0]).all()                                                   # in the kernel's own arithmetic
    ref_ = ~copied
    if x.dtype == np.float64 and ref_.any():                                                      # (a float32 output is rounded after its cost was taken)
        e_in, e_out = _cost_numpy(cs, x, used)[ref_], _cost_numpy(cs, out, used)[ref_]
        if sigma >= 1.0:
            figures["worse"] = max(figures["worse"], float(((e_out - e_in) / e_in).max()))
            for k, e in ((0, e_in), (1, e_out)):
                figures["cost"] = max(figures["cost"], float((np.abs(cost[..., k][ref_] - e) / e).max()))
        return e_in, e_out, cost[ref_]
    return None


@pytest.mark.parametrize("rec_dtype", ["float64", "float32"])
@pytest.mark.parametrize("rig_name", rc.RIGS)
def test_classes_and_costs_against_the_rule(api, rig_name, rec_dtype):
    """Classes against the NumPy rule on every shape, sigma, start; the kernel's own cost never rises; recomputed in plain NumPy from
    the kernel's input and output, cost_out <= cost_in (1 + 64 eps) on every record, sigma = 0 included, and the kernel's cost array
    agrees with that recomputation to 128 eps of the sum.  (The kernel forms E in the rule's own plain operations, so the two agree
    bit for bit wherever the view sets do; the slack is what the comparison was asked with.)"""
    K, R, t = rc.rig(rig_name)
    ctx = _lib.Context(K, R, t)
    fig = dict(worse=-1.0, cost=0.0)
    for shape in rc.SHAPES:
        for sigma in rc.SIGMAS if rec_dtype == "float64" else (1.0,):
            for kp_dtype in ("float64", "float32") if shape == (2, 3, 21) else ("float64",):
                cs = rc.case(rig_name, shape, sigma, True, rec_dtype, kp_dtype)
                for start in rc.STARTS:
                    ref = rc.reference(rig_name, shape, sigma, start, True, rec_dtype, kp_dtype)
                    got = _check_against_the_rule(ctx, cs, ref, start, sigma, fig)
                    if got is not None:
                        e_in, e_out, cost = got
                        assert (e_out <= e_in * (1.0 + 64 * EPS)).all(), (shape, sigma, start)
                        assert (np.abs(cost[:, 0] - e_in) <= 128 * EPS * e_in).all(), (shape, sigma, start)
                        assert (np.abs(cost[:, 1] - e_out) <= 128 * EPS * e_out).all(), (shape, sigma, start)
    ctx.close()
    print(f"    {rig_name} {rec_dtype}: max (E_out - E_in) / E_in recomputed = {fig['worse']:.2e}; max |cost - recomputed| / cost = "
          f"{fig['cost'] / EPS:.1f} eps")


def test_never_worse_recomputed_at_sigma_zero_with_64_eps(api):
    """cost_out <= cost_in (1 + 64 eps), both recomputed in plain NumPy, on the sigma = 0 cases (exact detections) of every rig: the
    costs are squares of pixel roundings there (1e-26 px^2), so this holds only because the kernel compares the very E the
    recomputation forms.  (With E taken from project_record's fused multiply-adds 1 243 of 18 146 records rose: EXPERIMENTS.md,
    round 19.)"""
    over = total = 0
    worst = 0.0
    for rig_name in rc.RIGS:
        K, R, t = rc.rig(rig_name)
        ctx = _lib.Context(K, R, t)
        for shape in rc.SHAPES:
            cs = rc.case(rig_name, shape, 0.0)
            for start in rc.STARTS:
                out, cost, codes = _run(ctx, cs, start)
                assert (cost[..., 1] <= cost[..., 0]).all()
                used = rc.reference(rig_name, shape, 0.0, start)[3]
                ref_ = codes >= KEPT
                e_in, e_out = _cost_numpy(cs, cs[start], used)[ref_], _cost_numpy(cs, out, used)[ref_]
                bad = ~(e_out <= e_in * (1.0 + 64 * EPS))
                over, total = over + int(bad.sum()), total + bad.size
                worst = max(worst, float(e_out[bad].max()) if bad.any() else 0.0)
        ctx.close()
    print(f"    sigma 0: {over} of {total} recomputed costs rose by more than 64 eps; the largest of them {worst:.2e} px^2")
    assert over == 0, f"{over} of {total} recomputed costs rose by more than 64 eps (the largest of them is {worst:.2e} px^2)"


@pytest.mark.parametrize("rig_name", ["floor", "ring8", "ring16"])
def test_cost_array_agrees_with_a_numpy_recomputation_to_128_eps(api, rig_name):
    """The kernel's cost array against E recomputed in plain NumPy from its input and output, held to 128 eps of the sum on every
    refined record of the (5, 2, 133) cases at sigma = 1 and 2.
    (With E taken from project_record's fused multiply-adds the two differed by 1 500 .. 154 000 eps: pixels a few 1e-13 px apart,
    and u(X) - u of a 1 px residual at u ~ 640 cancels three digits.  EXPERIMENTS.md, round 19.)"""
    K, R, t = rc.rig(rig_name)
    ctx = _lib.Context(K, R, t)
    worst = 0.0
    over = total = 0
    for sigma in (1.0, 2.0):
        cs = rc.case(rig_name, (5, 2, 133), sigma)
        out, cost, codes = _run(ctx, cs, "dlt")
        used = rc.reference(rig_name, (5, 2, 133), sigma, "dlt")[3]
        ref_ = codes >= KEPT
        for k, rec in ((0, cs["dlt"]), (1, out)):
            e = _cost_numpy(cs, rec, used)[ref_]
            rel = np.abs(cost[..., k][ref_] - e) / e
            worst, over, total = max(worst, float(rel.max())), over + int((rel > 128 * EPS).sum()), total + rel.size
    ctx.close()
    print(f"    {rig_name}: max |cost - recomputed| / cost = {worst / EPS:.0f} eps; {over} of {total} over 128 eps")
    assert over == 0, f"{over} of {total} costs differ from the NumPy recomputation by more than 128 eps (worst {worst / EPS:.0f} eps)"


def test_never_worse_with_outliers(api):
    K, R, t = synth.load_rig_json()
    rng = np.random.default_rng(rc._seed("outliers"))
    X = synth.make_people(rng, 8, 1)
    kp, _ = synth.make_keypoints(rng, K, R, t, X, pixel_sigma=1.0, dtype=np.float64)
    kp, cam = synth.add_outliers(rng, kp, fraction=0.1)
    assert (cam >= 0).sum() > 50
    N = 8 * 133
    pair, dlt = rc._starts(K, R, t, np.moveaxis(kp, 1, 0).reshape(4, N, 3), np.ones((4, N), dtype=bool), X.reshape(N, 3))
    cs = dict(K=K, R=R, t=t, kpts=kp, det_of=None, n_persons=None, views=None, thr=0.0)
    ctx = _lib.Context(K, R, t)
    for start in (pair, dlt):
        x = np.concatenate([start.reshape(8, 1, 133, 3), np.ones((8, 1, 133, 1))], axis=-1)
        out, cost, codes = ctx.refine_joints(x, kp, diagnostics=True)
        used = np.full((8, 1, 133), 15, dtype=np.uint32)
        e_in, e_out = _cost_numpy(cs, x, used), _cost_numpy(cs, out, used)
        print(f"    outliers: {int((codes == MOVED).sum())} of {codes.size} moved, summed cost {e_in.sum():.1f} -> {e_out.sum():.1f} px^2, "
              f"max (E_out - E_in) / E_in = {float(((e_out - e_in) / e_in).max()):.2e}")
        assert (codes >= KEPT).all() and (cost[..., 1] <= cost[..., 0]).all()
        assert (e_out <= e_in * (1.0 + 64 * EPS)).all()
        assert (np.abs(cost[..., 0] - e_in) <= 128 * EPS * e_in).all() and (np.abs(cost[..., 1] - e_out) <= 128 * EPS * e_out).all()
    ctx.close()


@pytest.mark.parametrize("rig_name", ["floor", "ring8", "ring16"])
def test_a_point_behind_a_camera_loses_that_view(api, rig_name):
    cs = rc.behind_case(rig_name)
    ctx = _lib.Context(cs["K"], cs["R"], cs["t"])
    out, cost, codes = ctx.refine_joints(cs["dlt"], cs["kpts"], keypoint_score_threshold=cs["thr"], diagnostics=True)
    ctx.close()
    r_out, r_cost, r_codes = rf.refine_joints_reference(cs["K"], cs["R"], cs["t"], cs["dlt"], cs["kpts"], keypoint_score_threshold=cs["thr"])
    assert np.array_equal(codes, r_codes) and (codes == MOVED).all()
    assert np.allclose(cost, r_cost, rtol=1e-9, atol=0) and np.abs(out - r_out).max() < 1e-6


# ------------------------------------------------------------------------------------------------ a record's bits are its own
def test_bits_do_not_depend_on_the_batch_around_a_record(api):
    import torch
    rig_name = "floor"
    cs = rc.case(rig_name, rc.CUT_SHAPE, 1.0)
    K, R, t = rc.rig(rig_name)
    ctx = _lib.Context(K, R, t)
    whole = _run(ctx, cs, "dlt")
    assert (whole[2] == MOVED).sum() > 4000
    kw = rc.refine_kwargs(cs)
    for cut in rc.CUTS:
        parts = [ctx.refine_joints(cs["dlt"][s], cs["kpts"][s], det_of=kw["det_of"][s], n_persons=kw["n_persons"][s], views=kw["views"][s],
                                   keypoint_score_threshold=cs["thr"], diagnostics=True) for s in (slice(0, cut), slice(cut, None))]
        for k in range(3):
            assert _same_bits(np.concatenate([parts[0][k], parts[1][k]]), whole[k]), (cut, k)
    # the records in reverse order (frames and joints; one person), det_of / views permuted alike
    rev = ctx.refine_joints(cs["dlt"][::-1, :, ::-1].copy(), cs["kpts"][::-1, :, :, ::-1].copy(), det_of=kw["det_of"][::-1].copy(),
                            n_persons=kw["n_persons"][::-1].copy(), views=kw["views"][::-1, :, ::-1].copy(), keypoint_score_threshold=cs["thr"],
                            diagnostics=True)
    for k in range(3):
        assert _same_bits(np.ascontiguousarray(rev[k][::-1, :, ::-1]), whole[k]), k
    # in place, on the host and on the device; HOST against DEVICE, NumPy against torch
    x = np.array(cs["dlt"], copy=True)
    same = ctx.refine_joints(x, cs["kpts"], out=x, **kw)
    assert same is x and _same_bits(x, whole[0])
    dev = lambda a, dt=None: None if a is None else torch.from_numpy(np.ascontiguousarray(a if dt is None else a.astype(dt))).to("cuda:0")
    xd, kd = dev(cs["dlt"]), dev(cs["kpts"])
    args = dict(det_of=dev(kw["det_of"]), n_persons=dev(kw["n_persons"]), views=dev(kw["views"].view(np.int32)), keypoint_score_threshold=cs["thr"])
    assert args["det_of"].dtype == torch.int64
    got = ctx.refine_joints(xd, kd, diagnostics=True, **args)
    torch.cuda.synchronize()
    assert _same_bits(xd.cpu().numpy(), cs["dlt"]), "the input buffer was written"
    for k in range(3):
        assert _same_bits(got[k].cpu().numpy(), whole[k]), k
    inplace = ctx.refine_joints(xd, kd, out=xd, **args)
    torch.cuda.synchronize()
    assert inplace is xd and _same_bits(xd.cpu().numpy(), whole[0])
    assert _same_bits(rf.refine_joints(ctx, cs["dlt"], cs["kpts"], **kw), whole[0])
    ctx.close()


@pytest.mark.parametrize("rig_name", ["floor", "ring5", "ring16"])
def test_refining_again_is_a_fixed_point(api, rig_name):
    K, R, t = rc.rig(rig_name)
    ctx = _lib.Context(K, R, t)
    for sigma in (1.0, 2.0):
        cs = rc.case(rig_name, (2, 3, 21), sigma)
        kw = rc.refine_kwargs(cs)
        once = ctx.refine_joints(cs["pair"], cs["kpts"], iters=rc.ACCURACY_ITERS, **kw)
        twice, cost, codes = ctx.refine_joints(once, cs["kpts"], iters=rc.ACCURACY_ITERS, diagnostics=True, **kw)
        assert (codes >= KEPT).sum() > 100
        d = np.linalg.norm(twice[..., :3] - once[..., :3], axis=-1)[codes >= KEPT].max() / rc.rig_scale(t)
        assert d <= rc.BAR and (cost[..., 1] <= cost[..., 0]).all(), float(d)
    ctx.close()


# ------------------------------------------------------------------------------------------------ the routes
def _summed_cost(ctx, xyzs, kp, npers, thr, det_of=None):
    s, n = ctx.reproject_cost(xyzs, kp, n_persons=npers, keypoint_score_threshold=thr)
    if det_of is None:
        return float(s[..., 0, 0].sum()) if s.shape[2:] == (1, 1) else None
    pick = np.take_along_axis(s, np.maximum(det_of, 0)[..., None], axis=-1)[..., 0]
    return float(np.where(det_of >= 0, pick, 0.0).sum())


@pytest.mark.parametrize("method", ["PAIRWISE", "DLT", "DLT_ROBUST"])
def test_single_person_routes_lower_their_cost(api, method):
    wl = synth.config_workload(2, F=16, dtype=np.float64)
    K, R, t = wl["rig"]
    kp = wl["kpts"]
    robust = method == "DLT_ROBUST"
    if robust:
        kp, _ = synth.add_outliers(np.random.default_rng(5), kp, fraction=0.1)
    bt = api.BatchTriangulator(K, R, t, wl["params"], pout_max=1, out_dtype=np.float64, method=getattr(_lib, method), diagnostics=robust)
    tri = bt.run_host(kp, wl["n_persons"])
    kn, thr = bt.params.keypoint_num, wl["params"]["keypoint_score_threshold"]
    views = tri["views"].reshape(16, 1, kn) if robust else None
    if robust:
        assert (tri["views"] != 15).any()
    kpn = np.ascontiguousarray(kp[:, :, :, :kn])
    out, cost, codes = bt.ctx.refine_joints(tri["xyzs"], kpn, n_persons=wl["n_persons"], views=views, keypoint_score_threshold=thr, diagnostics=True)
    assert (codes == MOVED).sum() > 0.9 * codes.size and (cost[..., 1] <= cost[..., 0]).all()
    before, after = cost[..., 0].sum(), cost[..., 1].sum()
    print(f"    {method}: summed cost {before:.1f} -> {after:.1f} px^2 over {int((codes >= KEPT).sum())} joints")
    assert after < before
    if not robust:                                             # the same figure from snowtri_reproject_cost (its joints: all views that count)
        a, b = _summed_cost(bt.ctx, tri["xyzs"], kpn, wl["n_persons"], thr), _summed_cost(bt.ctx, out, kpn, wl["n_persons"], thr)
        assert b < a and abs(a - before) <= 1e-9 * a and abs(b - after) <= 1e-9 * b
    bt.close()


def test_multi_person_route_lowers_its_cost(api):
    wl = synth.config_workload(3, F=6, dtype=np.float64)       # 8 cameras x 4 persons, every list permuted
    K, R, t = wl["rig"]
    bt = api.BatchTriangulator(K, R, t, wl["params"], pout_max=8, out_dtype=np.float64)
    tri = bt.run_host(wl["kpts"], wl["n_persons"])
    assert (tri["count"] >= 4).all()                           # (the association may list a ghost or two beside the four persons)
    kn, thr = bt.params.keypoint_num, wl["params"]["keypoint_score_threshold"]
    kpn = np.ascontiguousarray(wl["kpts"][:, :, :, :kn])
    s, n = bt.ctx.reproject_cost(tri["xyzs"], kpn, n_persons=wl["n_persons"], keypoint_score_threshold=thr)
    det_of, _ = rp.match_detections(s, n, 6.0)
    assert det_of.dtype == np.int64 and ((det_of >= 0).sum(axis=1) >= 2).sum() >= 4 * 6
    out, cost, codes = bt.ctx.refine_joints(tri["xyzs"], kpn, det_of=det_of, n_persons=wl["n_persons"], keypoint_score_threshold=thr, diagnostics=True)
    before, after = _summed_cost(bt.ctx, tri["xyzs"], kpn, wl["n_persons"], thr, det_of), _summed_cost(bt.ctx, out, kpn, wl["n_persons"], thr, det_of)
    refined = codes >= KEPT
    print(f"    8 x 4: summed cost {before:.1f} -> {after:.1f} px^2; {int((codes == MOVED).sum())} of {int(refined.sum())} refined joints moved")
    assert after < before and (cost[..., 1] <= cost[..., 0]).all() and cost[..., 1].sum() < cost[..., 0].sum()
    assert refined.sum() >= 4 * 6 * kn * 0.9 and (codes == MOVED).sum() > 0.9 * refined.sum()
    assert (codes[missing_records(tri["xyzs"])] == MISSING).all()
    bt.close()


# ------------------------------------------------------------------------------------------------ the pipeline
def test_pipeline_refines_before_everything_downstream(api):
    from snowmocap_amd.blender import CONTROL_POINT_NAMES
    mc = reproject_cases.match_case(4, 3, 24)
    thr = synth.default_thresholds()
    thr.update(keypoint_score_threshold=0.5, average_score_threshold=1.0, condense_distance_tol=0.3)
    smo = {n: [2.0, 0.75, 0.0] for n in CONTROL_POINT_NAMES}
    pipe = api.TrackPipeline(mc["K"], mc["R"], mc["t"], thr, smo, n_persons_out=3)
    plain = pipe.run(mc["kpts"], mc["n_persons"])
    none = pipe.run(mc["kpts"], mc["n_persons"], refine=None)
    res = pipe.run(mc["kpts"], mc["n_persons"], refine=4)
    res2 = pipe.run(mc["kpts"], mc["n_persons"], refine=(4, 6.0, False))
    today = ["xyzs", "smoothed", "points", "valid", "points_smoothed", "count", "flags", "tracked"]
    assert list(plain) == today and list(none) == today and list(res) == today + ["refine_cost", "refine_codes"]
    for k in today:
        assert _same_bits(none[k].cpu().numpy(), plain[k].cpu().numpy()), k
    for k in res:
        assert _same_bits(res[k].cpu().numpy(), res2[k].cpu().numpy()), k
    # by hand, from the unrefined run's records
    import torch
    ctx = pipe.bt.ctx
    kp = torch.from_numpy(np.ascontiguousarray(mc["kpts"][:, :, :, :pipe.kn])).to("cuda:0")
    npers = torch.from_numpy(np.ascontiguousarray(mc["n_persons"])).to("cuda:0")
    s, n = ctx.reproject_cost(plain["xyzs"], kp, n_persons=npers, keypoint_score_threshold=0.5)
    det_of, _ = rp.match_detections(s, n, 6.0)
    want, cost, codes = rf.refine_joints(ctx, plain["xyzs"], kp, det_of=det_of, n_persons=npers, keypoint_score_threshold=0.5, iters=4, diagnostics=True)
    assert _same_bits(res["xyzs"].cpu().numpy(), want.cpu().numpy()) and _same_bits(res["refine_cost"].cpu().numpy(), cost.cpu().numpy())
    assert _same_bits(res["refine_codes"].cpu().numpy(), codes.cpu().numpy()) and (codes.cpu().numpy() == MOVED).mean() > 0.95
    assert not _same_bits(res["xyzs"].cpu().numpy(), plain["xyzs"].cpu().numpy())
    assert not _same_bits(res["smoothed"].cpu().numpy(), plain["smoothed"].cpu().numpy())           # downstream sees the refined records
    for k in ("count", "flags", "tracked"):
        assert _same_bits(res[k].cpu().numpy(), plain[k].cpu().numpy()), k
    with pytest.raises(ValueError):
        pipe.run(mc["kpts"], mc["n_persons"], refine=0)
    pipe.close()


def test_pipeline_built_with_a_lens_refines_on_the_undistorted_copy(api):
    from oracle import undistort as ou
    from snowmocap_amd.blender import CONTROL_POINT_NAMES
    K, R, t, D, _ = uc.rig("floor")
    rng = np.random.default_rng(3)
    X = synth.make_people(rng, 24, 1) * [0.5, 0.5, 1.0]
    kp, npers = synth.make_keypoints(rng, K, R, t, X, pixel_sigma=1.0, dtype=np.float64)
    und = np.array(kp, copy=True)
    for c in range(K.shape[0]):
        kp[:, c, ..., :2] = ou.distort_pixels(K[c], D[c], kp[:, c, ..., :2])
    smo = {n: [2.0, 0.75, 0.0] for n in CONTROL_POINT_NAMES}
    pipe = api.TrackPipeline(K, R, t, synth.default_thresholds(), smo, n_persons_out=1, D=D)
    plain = pipe.run(kp, npers)
    res = pipe.run(kp, npers, refine=4)
    kn = pipe.kn
    cost = res["refine_cost"].cpu().numpy()
    assert (res["refine_codes"].cpu().numpy() == MOVED).all() and (cost[..., 1] < cost[..., 0]).all()
    # the cost was taken against the undistorted pixels: about 2 sigma^2 per view that counts, not the tens of px of the lens
    assert cost[..., 1].mean() < 8.0 * 2.0
    want = rf.refine_joints_reference(K, R, t, plain["xyzs"].cpu().numpy(), und[:, :, :, :kn], det_of=np.zeros((24, 4, 1), dtype=np.int64),
                                      n_persons=npers, keypoint_score_threshold=pipe.th["keypoint_score_threshold"])[0]
    assert np.abs(res["xyzs"].cpu().numpy() - want).max() < 1e-6
    pipe.close()


# ------------------------------------------------------------------------------------------------ buffers, bad arguments, debug build
def test_wrapper_refusals_and_empty_batches(api):
    import torch
    cs = rc.case("ring5", (2, 3, 21), 1.0)
    ctx = _lib.Context(cs["K"], cs["R"], cs["t"])
    kw = rc.refine_kwargs(cs)
    for space in (_lib.HOST, _lib.DEVICE):
        assert ctx.L.snowtri_refine_joints(ctx.handle, 0, 3, 21, None, _lib.F64, 4, None, _lib.F32, None, None, None, 0.5, 4, 0, None, None, None,
                                           space, None) == _lib.OK
    out, cost, codes = ctx.refine_joints(cs["dlt"][:0], cs["kpts"][:0], diagnostics=True)
    assert out.shape == (0, 3, 21, 4) and cost.shape == (0, 3, 21, 2) and codes.shape == (0, 3, 21)
    for bad in (dict(iters=0), dict(iters=17), dict(keypoint_score_threshold=float("nan"))):
        with pytest.raises(ValueError):
            ctx.refine_joints(cs["dlt"], cs["kpts"], **{**kw, **bad})
    with pytest.raises(ValueError, match="det_of"):
        ctx.refine_joints(np.concatenate([cs["dlt"], cs["dlt"]], axis=1), cs["kpts"])                 # P = 6 > Pmax = 4
    with pytest.raises(ValueError):
        ctx.refine_joints(cs["dlt"], cs["kpts"][:, :3], **kw)
    with pytest.raises(ValueError):
        ctx.refine_joints(cs["dlt"], cs["kpts"], **{**kw, "views": kw["views"][:, :2]})
    with pytest.raises(ValueError):
        ctx.refine_joints(cs["dlt"], cs["kpts"], out=np.empty_like(cs["dlt"]), **kw)
    with pytest.raises(ValueError):
        ctx.refine_joints(torch.from_numpy(np.array(cs["dlt"])).to("cuda:0"), cs["kpts"], **kw)       # a mixture
    wide = _lib.Context(*synth.ring_rig(33))
    with pytest.raises(ValueError, match="32"):
        wide.refine_joints(np.ones((1, 1, 1, 4)), np.ones((1, 33, 1, 1, 3)))
    wide.close()
    ctx.close()


def test_entry_rejects_bad_arguments_on_a_real_context(api, tmp_path):
    """tests/abi_badargs_refine.c against libsnowtri.so on the GPU: every refusal that comes before a launch, and one good call."""
    lib_dir = os.path.join(ROOT, "snowmocap_amd")
    exe = str(tmp_path / "abi_badargs_refine")
    subprocess.check_call(["gcc", "-std=c99", "-O1", "-I", os.path.join(ROOT, "include"), os.path.join(ROOT, "tests", "abi_badargs_refine.c"),
                           "-o", exe, "-L", lib_dir, "-lsnowtri", "-Wl,-rpath," + lib_dir])
    out = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0 and "0 failure(s)" in out.stdout, out.stdout[-3000:] + out.stderr[-2000:]


DBG_CODE = r'''
import sys, numpy as np
sys.path.insert(0, %(root)r)
sys.path.insert(0, %(tests)r)
import refine_cases as rc
from snowmocap_amd import _lib
assert _lib.LIB_PATH.endswith("libsnowtri_dbg.so") and "SNOWTRI_DEBUG_BOUNDS" in _lib.build_info()["variants"]
for rig_name, shape, dt in (("floor", (5, 2, 133), "float64"), ("ring8", (1, 1, 65), "float32"), ("ring16", (2, 3, 21), "float64"), ("ring3", (1, 1, 1), "float64")):
    cs = rc.case(rig_name, shape, 1.0, True, dt)
    ctx = _lib.Context(cs["K"], cs["R"], cs["t"])
    out, cost, codes = ctx.refine_joints(cs["dlt"], cs["kpts"], diagnostics=True, **rc.refine_kwargs(cs))
    ref = rc.reference(rig_name, shape, 1.0, "dlt", True, dt)
    assert np.array_equal(codes, ref[2]) and (cost[..., 1] <= cost[..., 0]).all()
    n, first = ctx.debug_faults()
    assert n == 0, "device-side bounds check failed %%d times; first: code %%d at line %%d" %% (n, first >> 32, first & 0xffffffff)
    ctx.close()
print("refine debug-bounds ok")
'''


def test_debug_build_counts_no_fault():
    dbg = os.path.join(ROOT, "snowmocap_amd", "libsnowtri_dbg.so")
    assert os.path.exists(dbg), f"{dbg} is missing: `make -C snowmocap_amd/csrc debug`"
    import sys
    env = dict(os.environ, SNOWTRI_LIB=dbg)
    code = DBG_CODE % {"root": ROOT, "tests": os.path.join(ROOT, "tests")}
    p = subprocess.run([sys.executable, "-c", code], env=env, capture_output=True, text=True, timeout=300)
    assert p.returncode == 0 and "refine debug-bounds ok" in p.stdout, (p.stdout[-2000:] + p.stderr[-3000:])
