"""k_reproject and k_reproject_cost behind snowtri_reproject / snowtri_reproject_cost (include/snowtri.h, "Reprojection"), and what
is built on them: reproject.match_detections / view_residuals, CameraGroup.reproject, TrackPipeline.run(reproject=...).
Inputs: tests/reproject_cases.py (the rigs of tests/undistort_cases.py at the six placements of tests/dlt_frames_cases.py).

The pixel bars are derived, not measured (eps = 2^-53):
  * d = X - t rounds once per coordinate; pc_i = sum_k R_ki d_k is two fused multiply-adds on a product, so |delta pc_i| <= 3 eps |d|
    (R's columns are unit vectors).  x = pc0 * (1 / pc2) adds 1.5 eps |x|.  With z = pc2:
        |delta x| <= 3 eps (|d| / z) (1 + |x|) + 1.5 eps |x| <= (3 * 1.8 * 2.5 + 2.3) eps ~ 16 eps        at |d| / z <= 1.8, |x| <= 1.5,
    about 18 eps with the second-order terms and y's share through the skew.  Times fx <= 760 px: 1.5e-12 px.
  * u = fx x + s y + cx is three roundings of sums below 1400 px: 3 * 1400 * eps = 4.7e-13 px.  Together 2e-12 px.
  * The lens (RAW) evaluates a degree-7 polynomial in (x, y) at |x| <= 1.5 in ~12 operations, ~10 eps of x_d, and passes delta x on
    through a Jacobian of norm <= 1.6 on these lenses: it adds about 1.5e-12 px.
  * The bars are 4 times that: 1e-11 px undistorted (4 * 2e-12 = 8e-12), 2e-11 px raw (4 * 3.5e-12 = 1.4e-11).
They hold where the derivation does (reproject_cases.IN_DOMAIN: pc2 > 0, |d| / pc2 <= 1.8), which is every point in the camera it
was made for and every joint of the cost and matching workloads in every camera.  float32 pixels: half a float32 ulp of the
expected value + 1e-9 px (the convention of tests/test_gpu_undistort.py).  float32 records are held to the exact projection of
the rounded values.

The cost bar.  Both sides add, over the same n joints, terms r_j^2 = du^2 + dv^2 whose du and dv differ between kernel and
reference by at most the pixel bar b each: the residual vector moves by at most delta = sqrt(2) b, so |r_j'| <= r_j + delta and
    |r_j'^2 - r_j^2| <= 2 r_j delta + delta^2,        |sum' - sum| <= 2 delta sum_j r_j + n delta^2.
The two sums are formed in different orders (joint order against four per lane and a butterfly) from terms rounded ~2 eps each:
n <= 256 positive terms, so both are within (n + 2) eps of the exact sum in the worst case and ~sqrt(n) eps typically; 256 * 2^-53
of the reference sum covers it.  cost_n is compared exactly: no projection of these workloads is within a millimetre of a camera
plane, and the score gate sees the same values on both sides.
"""
import os
import subprocess

import numpy as np
import pytest

import reproject_cases as rc
import undistort_cases as uc
from snowmocap_amd import _lib, synth
from snowmocap_amd import reproject as rp

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EPS = 2.0 ** -53


@pytest.fixture(scope="module")
def api():
    import snowmocap_amd as sm
    assert _lib.lib().snowtri_device_count() > 0, "these tests need the HIP device"
    return sm


def _context(K, R, t, D=None):
    ctx = _lib.Context(K, R, t)
    if D is not None:
        ctx.set_distortion(D)
    return ctx


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view({8: np.uint64, 4: np.uint32, 1: np.uint8}[a.dtype.itemsize])


def _same_bits(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and np.array_equal(_bits(a), _bits(b))


# ------------------------------------------------------------------------------------------------ 1. accuracy
@pytest.mark.parametrize("placement", rc.PLACEMENTS)
@pytest.mark.parametrize("rig_name", rc.RIGS)
def test_pixels_against_the_50_digit_projection(api, rig_name, placement):
    failed = []
    worst = {}
    K, R, t, D = rc.rig(rig_name, placement)
    ctx = _context(K, R, t, D)
    for shape in rc.shapes_of(rig_name):
        for x_dtype in ("float64", "float32"):
            cs = rc.case(rig_name, shape, placement, x_dtype)
            front = cs["depth"] > 0
            for raw, key, bar in ((False, "uv", rc.BAR_F64), (True, "raw", rc.BAR_F64_RAW)):
                for p_dtype in (np.float64, np.float32):
                    got = ctx.reproject(cs["xyzs"], raw=raw, dtype=p_dtype)
                    tag = f"{shape} xyzs {x_dtype} pix {np.dtype(p_dtype).name} {'raw' if raw else 'undistorted'}"
                    assert got.dtype == p_dtype and got.shape == cs["uv"].shape[:-1] + (3,), tag
                    score = np.where(front, np.broadcast_to(cs["xyzs"][:, None, :, :, 3].astype(p_dtype), front.shape), p_dtype(0))
                    if not _same_bits(got[..., 2], score.astype(p_dtype)):
                        failed.append(f"{tag}: scores are not the input's value (0 behind the camera)")
                    if (got[~front] != 0).any():
                        failed.append(f"{tag}: a point behind the camera did not give (0, 0, 0)")
                    m = cs["in_domain"]
                    err = np.abs(got[..., :2].astype(np.float64) - cs[key])[m]
                    tol = np.full(err.shape, bar) if p_dtype == np.float64 else (0.5 * uc.f32_ulp(cs[key]) + rc.F32_EXTRA)[m]
                    fig = err if p_dtype == np.float64 else err / uc.f32_ulp(cs[key])[m]
                    k = (key, np.dtype(p_dtype).name)
                    worst[k] = max(worst.get(k, 0.0), float(fig.max()))
                    if not (err <= tol).all():
                        failed.append(f"{tag}: {int((~(err <= tol)).sum())} of {err.size} over the bar, worst {float((err / tol).max()):.2f} x")
    ctx.close()
    print(f"    {rig_name} {placement}: max |k_reproject - exact|: float64 {worst['uv', 'float64']:.2e} px undistorted (bar {rc.BAR_F64:.0e}), "
          f"{worst['raw', 'float64']:.2e} px raw (bar {rc.BAR_F64_RAW:.0e}); float32 pixels {worst['uv', 'float32']:.4f} / "
          f"{worst['raw', 'float32']:.4f} float32 ulps (bar 0.5 + 1e-9 px)")
    assert not failed, f"{rig_name} {placement}: " + " | ".join(failed)


# ------------------------------------------------------------------------------------------------ 2. invalid records
@pytest.mark.parametrize("x_dtype", ["float64", "float32"])
@pytest.mark.parametrize("what", ["score 0", "score -0.0", "nan coordinate", "inf coordinate", "behind"])
def test_an_invalid_record_gives_zeros_and_changes_no_other_pixel(api, what, x_dtype):
    cs = rc.case("floor", (5, 2, 133), "home", x_dtype)
    K, R, t, D = cs["K"], cs["R"], cs["t"], cs["D"]
    x = np.array(cs["xyzs"], copy=True)
    flat = x.reshape(-1, 4)
    hit = np.zeros(flat.shape[0], dtype=bool)
    hit[11::37] = True
    cam = 2
    if what == "score 0":
        flat[hit, 3] = 0.0
    elif what == "score -0.0":
        flat[hit, 3] = -0.0
    elif what == "nan coordinate":
        flat[hit, np.arange(hit.sum()) % 3] = np.nan
    elif what == "inf coordinate":
        flat[hit, np.arange(hit.sum()) % 3] = np.where(np.arange(hit.sum()) % 2, np.inf, -np.inf)
    else:   # 0.5 .. 4 m behind camera `cam`, up to a metre off its axis
        rng = np.random.default_rng(5)
        n = int(hit.sum())
        flat[hit, :3] = t[cam] - R[cam][:, 2] * rng.uniform(0.5, 4.0, (n, 1)) + R[cam][:, 0] * rng.uniform(-1, 1, (n, 1)) + R[cam][:, 1] * rng.uniform(-1, 1, (n, 1))
    hit = hit.reshape(x.shape[:-1])                                                         # [F, P, kn]
    ctx = _context(K, R, t, D)
    for raw in (False, True):
        clean = ctx.reproject(cs["xyzs"], raw=raw)
        got = ctx.reproject(x, raw=raw)
        again = ctx.reproject(cs["xyzs"], raw=raw)
        assert _same_bits(again, clean)
        for c in range(K.shape[0]):
            if what != "behind" or c == cam:
                assert (_bits(got[:, c][hit]) == 0).all(), f"{what}, camera {c}: not exactly (0, 0, 0)"     # (+0.0, not -0.0)
            differ = (_bits(got[:, c]) != _bits(clean[:, c])).any(axis=-1) & ~hit
            assert not differ.any(), f"{what}, camera {c}: {int(differ.sum())} other pixels changed"
    ctx.close()


# ------------------------------------------------------------------------------------------------ 3. cuts
def _cut_case():
    cs = rc.case("floor", rc.CUT_SHAPE)
    pix = rp.reproject_reference(cs["K"], cs["R"], cs["t"], cs["xyzs"])
    rng = np.random.default_rng(17)
    kp = np.stack([pix, pix[:, :, :, ::-1]], axis=2)[:, :, :, 0] + 0.0                       # [F, C, 2, kn, 3]: the person, and it reversed
    kp[..., :2] += rng.normal(0.0, 1.5, kp[..., :2].shape)
    kp[..., 2] = rng.uniform(0.0, 5.0, kp.shape[:-1])
    return cs, kp, rng.integers(0, 3, kp.shape[:2]).astype(np.int32)


@pytest.mark.parametrize("raw", [False, True])
def test_bits_do_not_depend_on_how_the_frames_are_cut(api, raw):
    cs, kp, npers = _cut_case()
    ctx = _context(cs["K"], cs["R"], cs["t"], cs["D"])
    x = cs["xyzs"]
    edges = (0,) + rc.CUTS + (x.shape[0],)
    full = ctx.reproject(x, raw=raw)
    parts = np.concatenate([ctx.reproject(x[a:b], raw=raw) for a, b in zip(edges[:-1], edges[1:])], axis=0)
    differ = (_bits(full) != _bits(parts)).any(axis=-1)
    assert not differ.any(), f"k_reproject: {int(differ.sum())} pixels depend on the cut"
    for kpts, n_persons in ((kp, None), (kp.astype(np.float32), npers)):
        cost = lambda a, b: ctx.reproject_cost(x[a:b], kpts[a:b], None if n_persons is None else n_persons[a:b], 0.5, raw=raw)    # noqa: E731
        fs, fn = cost(0, x.shape[0])
        cut = [cost(a, b) for a, b in zip(edges[:-1], edges[1:])]
        ps, pn = np.concatenate([c[0] for c in cut], axis=0), np.concatenate([c[1] for c in cut], axis=0)
        assert np.array_equal(fn, pn) and (fn > 100).any() and (n_persons is None or (fn == 0).any())
        differ = _bits(fs) != _bits(ps)
        assert not differ.any(), f"k_reproject_cost: {int(differ.sum())} sums depend on the cut"
    ctx.close()


# ------------------------------------------------------------------------------------------------ 4. round trips
@pytest.mark.parametrize("rig_name", rc.RIGS)
def test_raw_projection_undistorted_again_is_the_plain_projection(api, rig_name):
    cs = rc.case(rig_name, (5, 2, 133))
    ctx = _context(cs["K"], cs["R"], cs["t"], cs["D"])
    plain = ctx.reproject(cs["xyzs"])
    back = ctx.undistort_keypoints(ctx.reproject(cs["xyzs"], raw=True))
    ctx.close()
    (u0, u1), (v0, v1) = uc.BOX                                                             # where the lenses are known to invert
    inside = cs["in_domain"] & (cs["uv"][..., 0] >= u0) & (cs["uv"][..., 0] <= u1) & (cs["uv"][..., 1] >= v0) & (cs["uv"][..., 1] <= v1)
    assert all(inside[:, c].mean() > 0.1 for c in range(inside.shape[1]))
    err = np.abs(back[..., :2] - plain[..., :2])[inside]
    print(f"    {rig_name}: max |undistort(reproject(RAW)) - reproject()| = {err.max():.2e} px over {int(inside.sum())} pixels")
    assert err.max() <= 1e-11 + 2e-11
    assert _same_bits(back[..., 2], plain[..., 2])


@pytest.mark.parametrize("method", ["PAIRWISE", "DLT"])
def test_projected_joints_triangulate_back_to_themselves(api, method):
    rec = uc.recording("floor", 40)
    X = rec["X"]                                                                             # [F, 1, 133, 3]
    xyzs = np.concatenate([X, np.full(X.shape[:-1] + (1,), 5.0)], axis=-1)
    ctx = _context(rec["K"], rec["R"], rec["t"])
    pix = ctx.reproject(xyzs)
    ctx.close()
    assert (pix[..., 2] == 5.0).all()
    bt = api.BatchTriangulator(rec["K"], rec["R"], rec["t"], synth.default_thresholds(), pout_max=1, out_dtype=np.float64, method=getattr(_lib, method))
    try:
        out = bt.run_host(pix, np.ones(pix.shape[:2], dtype=np.int32))
    finally:
        bt.close()
    err = np.abs(out["xyzs"][:, 0, :, :3] - X[:, 0]).max()
    print(f"    {method}: max |triangulate(reproject(X)) - X| = {err:.2e} m")
    assert out["status"] == _lib.OK and (out["count"] == 1).all() and err < 1e-7


# ------------------------------------------------------------------------------------------------ 5. the cost
def _sum_of_residuals(pix, kpts, n_persons, thr):
    """sum_j r_j [F, C, P, Pmax] over the joints that count, from the reference pixels."""
    kp = kpts.astype(np.float64)
    with np.errstate(all="ignore"):
        counts = ~(kp[..., 2] < thr) & np.isfinite(kp[..., 0]) & np.isfinite(kp[..., 1])
        if n_persons is not None:
            counts &= (np.arange(kp.shape[2])[None, None, :] < n_persons[:, :, None])[..., None]
        m = (pix[:, :, :, None, :, 2] != 0) & counts[:, :, None]
        r = np.hypot(pix[:, :, :, None, :, 0] - kp[:, :, None, :, :, 0], pix[:, :, :, None, :, 1] - kp[:, :, None, :, :, 1])
    return np.where(m, r, 0.0).sum(axis=-1)


@pytest.mark.parametrize("with_n_persons", [False, True])
@pytest.mark.parametrize("kp_dtype", ["float64", "float32"])
@pytest.mark.parametrize("shape", rc.COST_SHAPES)
def test_cost_against_the_reference(api, shape, kp_dtype, with_n_persons):
    cs = rc.cost_case(shape, kp_dtype, with_n_persons or shape == (3, 2, 5, 17, 5))
    K, R, t, D, x, kp, npers, thr = (cs[k] for k in ("K", "R", "t", "D", "xyzs", "kpts", "n_persons", "thr"))
    ratio = rc.domain_ratio(K, R, t, x)
    assert np.nanmax(ratio) <= rc.DOMAIN and np.nanmin(ratio) > 0, "the workload must lie in the accuracy domain of every camera"
    ctx = _context(K, R, t, D)
    for raw, bar in ((False, rc.BAR_F64), (True, rc.BAR_F64_RAW)):
        ref_s, ref_n = rp.reprojection_cost_reference(K, R, t, x, kp, npers, thr, D=D, raw=raw)
        got_s, got_n = ctx.reproject_cost(x, kp, npers, thr, raw=raw)
        assert got_s.dtype == np.float64 and got_n.dtype == np.int32 and got_s.shape == got_n.shape == ref_s.shape
        assert np.array_equal(got_n, ref_n), f"cost_n differs in {int((got_n != ref_n).sum())} of {ref_n.size} items"
        assert (got_s[ref_n == 0] == 0).all() and not np.isnan(got_s).any()
        delta = np.sqrt(2.0) * bar
        sum_r = _sum_of_residuals(rp.reproject_reference(K, R, t, x, D=D, raw=raw), kp, npers, thr)
        tol = 2.0 * delta * sum_r + ref_n * delta * delta + 256.0 * EPS * ref_s
        err = np.abs(got_s - ref_s)
        worst = float((err / np.maximum(tol, 1e-300)).max())
        print(f"    {shape} {kp_dtype} {'raw' if raw else 'undistorted'}: cost_n in 0..{int(ref_n.max())}, max |cost_sum - ref| / bound = {worst:.3f}, "
              f"max relative {float((err / np.maximum(ref_s, 1e-300)).max()):.1e}")
        assert (err <= tol).all(), f"{int((err > tol).sum())} of {err.size} sums over the bound (worst {worst:.2f} x)"
        if ref_n.size > 8:
            assert (ref_n > 0).any() and ((ref_n < shape[3]) & (ref_n > 0)).any()
    if npers is not None:                                                                    # nothing behind n_persons counts
        beyond = np.arange(shape[2])[None, None, :] >= npers[:, :, None]
        assert (got_n[np.broadcast_to(beyond[:, :, None, :], got_n.shape)] == 0).all()
    ctx.close()


@pytest.mark.parametrize("shape", [(3, 1, 1, 1, 1), (4, 3, 3, 133, 6), (8, 4, 4, 133, 4), (4, 2, 2, 64, 3)])
def test_cost_of_a_person_against_its_own_projection_is_exactly_zero(api, shape):
    """Both kernels project with one function: k_reproject's float64 pixels, used as detections, cost the person that made them 0."""
    cs = rc.cost_case(shape)
    ctx = _context(cs["K"], cs["R"], cs["t"], cs["D"])
    for raw in (False, True):
        pix = ctx.reproject(cs["xyzs"], raw=raw)
        s, n = ctx.reproject_cost(cs["xyzs"], pix, None, 0.25, raw=raw)                      # (the gate drops the (0, 0, 0) pixels)
        valid = (pix[..., 2] != 0).sum(axis=-1)                                              # [F, C, P]
        for p in range(shape[1]):
            assert (_bits(s[:, :, p, p]) == 0).all(), f"person {p}: up to {s[:, :, p, p].max():.3e} px^2 against its own pixels"
            assert np.array_equal(n[:, :, p, p], valid[:, :, p])
        assert valid.max() > 0.9 * shape[3] and (shape[3] < 100 or valid.min() < shape[3])       # (3 % of the records are missing)
        if shape[1] > 1:
            assert (s[:, :, 0, 1] > 100.0 * n[:, :, 0, 1]).all() and (n[:, :, 0, 1] > 0).all()
    ctx.close()


# ------------------------------------------------------------------------------------------------ 6. matching
@pytest.mark.parametrize("C,P", rc.MATCH_RIGS)
def test_matching_finds_the_known_permutation(api, C, P):
    import torch
    mc = rc.match_case(C, P)
    K, R, t = mc["K"], mc["R"], mc["t"]
    thr, gate = rc.MATCH_THRESHOLD, rc.MATCH_GATE
    ref_s, ref_n = rp.reprojection_cost_reference(K, R, t, mc["xyzs"], mc["kpts"], mc["n_persons"], thr)
    # the margin first, on the reference: the right detection is far inside the gate, every wrong one far outside
    mean = ref_s / np.maximum(ref_n, 1)
    right = np.take_along_axis(mean, mc["det_true"][..., None], axis=-1)[..., 0]
    wrong = np.where(np.arange(P)[None, None, None, :] == mc["det_true"][..., None], np.inf, mean)
    print(f"    {C} x {P}: own-person mean <= {right.max():.2f} px^2, wrong-person mean >= {wrong.min():.0f} px^2 (gate {gate * gate:.0f}); "
          f"joints per pair {int(ref_n.min())}..{int(ref_n.max())}")
    assert right.max() < gate * gate / 4 and wrong.min() > 1000.0 and ref_n.min() >= 100
    ref_det, ref_shared = rp.match_detections(ref_s, ref_n, gate)
    assert np.array_equal(ref_det, mc["det_true"]) and not ref_shared.any()
    ctx = _context(K, R, t)
    got_s, got_n = ctx.reproject_cost(mc["xyzs"], mc["kpts"], mc["n_persons"], thr)          # host arrays
    dev = torch.device("cuda", 0)
    on = lambda a: torch.from_numpy(np.array(a, copy=True)).to(dev)                           # noqa: E731
    dev_s, dev_n = ctx.reproject_cost(on(mc["xyzs"]), on(mc["kpts"]), on(mc["n_persons"]), thr)   # device tensors, in place
    det_t, shared_t = rp.match_detections(dev_s, dev_n, gate)
    assert det_t.is_cuda and shared_t.is_cuda
    torch.cuda.synchronize()
    ctx.close()
    assert _same_bits(dev_s.cpu().numpy(), got_s) and np.array_equal(dev_n.cpu().numpy(), got_n)
    det, shared = rp.match_detections(got_s, got_n, gate)
    for d, s in ((det, shared), (det_t.cpu().numpy(), shared_t.cpu().numpy())):
        assert np.array_equal(d, ref_det) and np.array_equal(d, mc["det_true"]) and not s.any()


# ------------------------------------------------------------------------------------------------ 7. pipeline, camera group
def _pipeline_inputs():
    from snowmocap_amd.blender import CONTROL_POINT_NAMES
    mc = rc.match_case(4, 3)
    thr = synth.default_thresholds()
    thr.update(keypoint_score_threshold=rc.MATCH_THRESHOLD, average_score_threshold=1.0, condense_distance_tol=0.3)
    return mc, thr, {n: [2.0, 0.75, 0.0] for n in CONTROL_POINT_NAMES}


def test_pipeline_reports_which_detection_is_whose(api):
    mc, thr, smo = _pipeline_inputs()
    pipe = api.TrackPipeline(mc["K"], mc["R"], mc["t"], thr, smo, n_persons_out=3)
    plain = pipe.run(mc["kpts"], mc["n_persons"])
    none = pipe.run(mc["kpts"], mc["n_persons"], reproject=None)
    res = pipe.run(mc["kpts"], mc["n_persons"], reproject=rc.MATCH_GATE)
    pipe.close()
    today = ["xyzs", "smoothed", "points", "valid", "points_smoothed", "count", "flags", "tracked"]
    assert list(plain) == today and list(none) == today
    assert list(res) == today + ["det_of", "shared", "view_rms", "view_n"]
    for k in today:
        assert _same_bits(res[k].cpu().numpy(), plain[k].cpu().numpy()) and _same_bits(none[k].cpu().numpy(), plain[k].cpu().numpy()), k
    out = {k: v.cpu().numpy() for k, v in res.items()}
    F, C, P = mc["det_true"].shape
    assert (out["count"] == P).all() and out["det_of"].shape == (F, C, P) and out["view_rms"].shape == (F, C, P)
    # xyzs lists the persons in the order the association found them: who is who, by the mean joint
    centre = out["xyzs"][..., :3].mean(axis=2)                                               # [F, P, 3]
    who = np.linalg.norm(centre[:, :, None] - mc["X"].mean(axis=2)[:, None], axis=-1).argmin(axis=-1)       # [F, slot] -> true person
    assert all(sorted(w) == list(range(P)) for w in who.tolist())
    want = np.take_along_axis(mc["det_true"], np.broadcast_to(who[:, None, :], (F, C, P)), axis=-1)
    assert np.array_equal(out["det_of"], want) and not out["shared"].any()
    print(f"    view_rms {np.nanmin(out['view_rms']):.2f} .. {np.nanmax(out['view_rms']):.2f} px over {int(out['view_n'].min())}.."
          f"{int(out['view_n'].max())} joints per view")
    assert np.isfinite(out["view_rms"]).all() and out["view_rms"].max() < 2.0 and out["view_n"].min() >= 100


def test_pipeline_built_with_a_lens_compares_on_the_raw_frame(api):
    from oracle import undistort as ou
    mc, thr, smo = _pipeline_inputs()
    K, R, t, D, _ = uc.rig("floor")
    X = mc["X"][:, :1] * [0.5, 0.5, 1.0]                                                    # one person around the middle of the floor rig
    rng = np.random.default_rng(3)
    kp, npers = synth.make_keypoints(rng, K, R, t, X, pixel_sigma=1.0, dtype=np.float64)
    for c in range(K.shape[0]):
        kp[:, c, ..., :2] = ou.distort_pixels(K[c], D[c], kp[:, c, ..., :2])
    thr = synth.default_thresholds()
    pipe = api.TrackPipeline(K, R, t, thr, smo, n_persons_out=1, D=D)
    res = {k: v.cpu().numpy() for k, v in pipe.run(kp, npers, reproject=rc.MATCH_GATE).items()}
    pipe.close()
    assert (res["count"] == 1).all() and (res["det_of"] == 0).all() and res["view_rms"].max() < 2.0     # (an undistorted comparison would be tens of px off)
    print(f"    raw-frame view_rms {res['view_rms'].min():.2f} .. {res['view_rms'].max():.2f} px")


def test_camera_group_reprojects_like_the_context(api):
    from snowmocap_amd.camera import CameraGroup
    group = CameraGroup(camera_group_info_path=synth.FLOOR_RIG_PATH)
    K, R, t = group.rig_arrays()
    D = synth.load_rig_distortion()
    rng = np.random.default_rng(9)
    xyzs = np.concatenate([synth.make_people(rng, 3, 2), rng.uniform(1.0, 8.0, (3, 2, 133, 1))], axis=-1)
    for raw in (False, True):
        got = group.reproject(xyzs, raw=raw)
        want = rp.reproject_reference(K, R, t, xyzs, D=D, raw=raw)
        assert got.shape == (3, K.shape[0], 2, 133, 3) and (got[..., 2] != 0).all()
        assert np.abs(got - want).max() <= (rc.BAR_F64_RAW if raw else rc.BAR_F64) * 1.25
        assert _same_bits(group.reproject(xyzs[1], raw=raw), got[1])                         # one frame [P, kn, 4]
    assert group.reproject(xyzs[:0]).shape == (0, K.shape[0], 2, 133, 3)


# ------------------------------------------------------------------------------------------------ buffers, bad arguments, debug build
def test_device_buffers_and_empty_batches(api):
    import torch
    cs = rc.case("ring5", (5, 2, 133))
    ctx = _context(cs["K"], cs["R"], cs["t"], cs["D"])
    C = cs["K"].shape[0]
    host = ctx.reproject(cs["xyzs"], raw=True, dtype=np.float32)
    src = torch.from_numpy(np.array(cs["xyzs"], copy=True)).to("cuda:0")
    pix = ctx.reproject(src, raw=True, dtype=torch.float32)
    torch.cuda.synchronize()
    assert _same_bits(src.cpu().numpy(), cs["xyzs"]), "the input buffer was written"
    assert _same_bits(pix.cpu().numpy(), host)
    for space in (_lib.HOST, _lib.DEVICE):
        assert ctx.L.snowtri_reproject(ctx.handle, 0, 2, 133, None, _lib.F64, 0, None, _lib.F64, space, None) == _lib.OK
        assert ctx.L.snowtri_reproject_cost(ctx.handle, 0, 2, 133, None, _lib.F64, 3, None, _lib.F32, None, 0.5, 0, None, None, space, None) == _lib.OK
    assert ctx.reproject(cs["xyzs"][:0]).shape == (0, C, 2, 133, 3)
    s, n = ctx.reproject_cost(cs["xyzs"][:0], np.zeros((0, C, 3, 133, 3), dtype=np.float32))
    assert s.shape == n.shape == (0, C, 2, 3)
    with pytest.raises(ValueError, match="256"):
        ctx.reproject_cost(np.ones((1, 1, 257, 4)), np.ones((1, C, 1, 257, 3)))
    with pytest.raises(ValueError):
        ctx.reproject(src[:, :, ::2])                                                        # not contiguous
    plain = _lib.Context(cs["K"], cs["R"], cs["t"])
    with pytest.raises(ValueError, match="snowtri_ctx_set_distortion"):
        plain.reproject(cs["xyzs"], raw=True)
    plain.close()
    ctx.close()


def test_entries_reject_bad_arguments_on_a_real_context(api, tmp_path):
    """tests/abi_badargs_reproject.c against libsnowtri.so on the GPU: every refusal that comes before a launch, and one good call each."""
    lib_dir = os.path.join(ROOT, "snowmocap_amd")
    exe = str(tmp_path / "abi_badargs_reproject")
    subprocess.check_call(["gcc", "-std=c99", "-O1", "-I", os.path.join(ROOT, "include"), os.path.join(ROOT, "tests", "abi_badargs_reproject.c"),
                           "-o", exe, "-L", lib_dir, "-lsnowtri", "-Wl,-rpath," + lib_dir])
    out = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0 and "0 failure(s)" in out.stdout, out.stdout[-3000:] + out.stderr[-2000:]


DBG_CODE = r'''
import sys, numpy as np
sys.path.insert(0, %(root)r)
sys.path.insert(0, %(tests)r)
import reproject_cases as rc
from snowmocap_amd import _lib
from snowmocap_amd import reproject as rp
assert _lib.LIB_PATH.endswith("libsnowtri_dbg.so") and "SNOWTRI_DEBUG_BOUNDS" in _lib.build_info()["variants"]
for shape, x_dtype in (((5, 2, 133), "float64"), ((1, 1, 1), "float32")):
    cs = rc.case("ring5", shape, "home", x_dtype)
    ctx = _lib.Context(cs["K"], cs["R"], cs["t"])
    ctx.set_distortion(cs["D"])
    for raw in (False, True):
        got = ctx.reproject(cs["xyzs"], raw=raw, dtype=np.float64)
        err = np.abs(got[..., :2] - cs["raw" if raw else "uv"])[cs["in_domain"]]
        assert err.max() <= (rc.BAR_F64_RAW if raw else rc.BAR_F64), (shape, raw, err.max())
    n, first = ctx.debug_faults()
    assert n == 0, "device-side bounds check failed %%d times; first: code %%d at line %%d" %% (n, first >> 32, first & 0xffffffff)
    ctx.close()
for shape in ((4, 3, 2, 65, 3), (3, 2, 5, 17, 5)):
    cs = rc.cost_case(shape, "float32", True)
    ctx = _lib.Context(cs["K"], cs["R"], cs["t"])
    s, n = ctx.reproject_cost(cs["xyzs"], cs["kpts"], cs["n_persons"], cs["thr"])
    ref_s, ref_n = rp.reprojection_cost_reference(cs["K"], cs["R"], cs["t"], cs["xyzs"], cs["kpts"], cs["n_persons"], cs["thr"])
    assert np.array_equal(n, ref_n) and np.allclose(s, ref_s, rtol=1e-12, atol=1e-9)
    k, first = ctx.debug_faults()
    assert k == 0, "device-side bounds check failed %%d times; first: code %%d at line %%d" %% (k, first >> 32, first & 0xffffffff)
    ctx.close()
print("reproject debug-bounds ok")
'''


def test_debug_build_counts_no_fault():
    dbg = os.path.join(ROOT, "snowmocap_amd", "libsnowtri_dbg.so")
    assert os.path.exists(dbg), f"{dbg} is missing: `make -C snowmocap_amd/csrc debug`"
    import sys
    env = dict(os.environ, SNOWTRI_LIB=dbg)
    code = DBG_CODE % {"root": ROOT, "tests": os.path.join(ROOT, "tests")}
    p = subprocess.run([sys.executable, "-c", code], env=env, capture_output=True, text=True, timeout=300)
    assert p.returncode == 0 and "reproject debug-bounds ok" in p.stdout, (p.stdout[-2000:] + p.stderr[-3000:])
