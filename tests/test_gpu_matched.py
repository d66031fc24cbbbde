"""snowtri_triangulate_matched on the GPU (k_dlt_matched): bit for bit against k_dlt_robust on each person's host-gathered keypoints,
against the NumPy rule (snowmocap_amd/matched.py) on the bars of tests/test_gpu_robust.py, independence of a person's bits from the
batch around it, the det_of / n_persons edges, untouched memory, the device-resident chain on the recipe "crossing", the C entry's
refusals and the debug build's device bounds checks."""
import os
import subprocess
import sys

import numpy as np
import pytest

import matched_cases as mc
import robust_cases as rc
from conftest import ROOT
from snowmocap_amd import _lib, matched, synth
from test_gpu_robust import MARGIN, XYZ_F32

pytestmark = pytest.mark.gpu

OUT_KEYS = ("xyzs", "pscore", "views", "resid")


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view({4: np.uint32, 8: np.uint64}[a.dtype.itemsize])


def _params(kn):
    return _lib.make_params(**dict(synth.default_thresholds(), keypoint_score_threshold=mc.KTHR, keypoint_num=kn, center_point_index=0))


def _robust(ctx, kp1, listed, tau, md, odt):
    """snowtri_triangulate_robust on one person's gathered keypoints [F, C, 1, kn, 3] -> xyzs [F, kn, 4], pscore [F], views, resid"""
    F, C, _, kn, _ = kp1.shape
    xyzs, ps = np.empty((F, 1, kn, 4), odt), np.empty((F, 1), odt)
    cnt, views, resid = np.empty(F, np.int32), np.empty((F, kn), np.uint32), np.empty((F, kn), odt)
    rcode = ctx.L.snowtri_triangulate_robust(ctx.handle, F, kn, _lib.ptr(kp1), _lib.dtype_code(kp1.dtype), _lib.ptr(listed), _params(kn), tau, md, 1,
                                             _lib.ptr(xyzs), _lib.ptr(ps), _lib.dtype_code(odt), _lib.ptr(cnt), None, _lib.ptr(views), _lib.ptr(resid),
                                             _lib.HOST, None)
    assert rcode == _lib.OK and ctx.last_kernel_names().startswith("k_dlt_robust<%d," % C)
    return dict(xyzs=xyzs[:, 0], pscore=ps[:, 0], views=views, resid=resid)


def _matched(ctx, kpts, det_of, n_persons, tau, md, odt, device=False, thr=mc.KTHR):
    if device:
        import torch
        dev = lambda a: None if a is None else torch.from_numpy(np.ascontiguousarray(a)).cuda()   # noqa: E731
        out = ctx.triangulate_matched(dev(kpts), dev(det_of), dev(n_persons), thr, tau, md, dtype=odt, diagnostics=True)
        torch.cuda.synchronize()
        out = [o.cpu().numpy() for o in out]
        out[2] = out[2].view(np.uint32)
    else:
        out = ctx.triangulate_matched(kpts, det_of, n_persons, thr, tau, md, dtype=odt, diagnostics=True)
    assert ctx.last_kernel_names().startswith("k_dlt_matched<%d," % kpts.shape[1]), ctx.last_kernel_names()      # it is k_dlt_matched that ran
    return dict(zip(OUT_KEYS, out))


def _assert_person_equals(got, p, one, what):
    for k in OUT_KEYS:
        assert np.array_equal(_bits(got[k][:, p]), _bits(one[k])), (k, p) + tuple(what)


def _shape_case(name, P, Pmax, kn, F, dtype):
    """-> (K, R, t, kpts, det_of, n_persons); P > Pmax: the persons behind Pmax name the detections of the first ones again"""
    b = mc.woven(name, min(P, Pmax), Pmax, F, kn, dtype)
    det = b["det_of"] if P <= Pmax else np.ascontiguousarray(np.concatenate([b["det_of"], b["det_of"][..., :P - Pmax]], axis=-1))
    return b["K"], b["R"], b["t"], b["kpts"], det, b["n_persons"]


# (P, Pmax, kn, F); the last: tiles of three frames and a last tile of one (a tile is a frame until F * P exceeds twice the CUs)
SHAPES = [(1, 1, 133, 1), (2, 3, 17, 17), (3, 2, 1, 40), (4, 4, 133, 40), (2, 2, 3, 1501)]


@pytest.mark.parametrize("P,Pmax,kn,F", SHAPES, ids=[f"P{p}-Pmax{q}-kn{k}-F{f}" for p, q, k, f in SHAPES])
@pytest.mark.parametrize("name", ["ring2", "ring3", "ring4", "ring5", "ring8"])
def test_bit_for_bit_against_k_dlt_robust(name, P, Pmax, kn, F):
    for dtype in ("float32", "float64"):
        K, R, t, kpts, det_of, n_persons = _shape_case(name, P, Pmax, kn, F, dtype)
        ctx = _lib.Context(K, R, t)
        variants = [(det_of, n_persons)] + ([(None, None)] if P == Pmax == 1 else [])
        for tau, md in rc.SETTINGS:
            for det, npers in variants:
                ones = []
                for p in range(P):
                    kp1, listed = matched.gather_person(kpts, det, npers, p)
                    ones.append(_robust(ctx, kp1, listed, tau, md, np.dtype(dtype)))
                for device in (False, True):
                    got = _matched(ctx, kpts, det, npers, tau, md, np.dtype(dtype), device)
                    for p in range(P):
                        _assert_person_equals(got, p, ones[p], (dtype, tau, md, device))
        ctx.close()


# (P, Pmax, kn, F): tiles of 3 frames x 2 persons x 133 joints (798 items, 12.5 waves) with a last tile of one frame, and tiles of
# 4 frames x 3 persons x 17 joints (204 items, 3.2 waves) with a last tile of three: the stash and the first record of a tile are
# indexed across frames AND waves
TILE_SHAPES = [(2, 2, 133, 1501), (3, 2, 17, 2051)]


@pytest.mark.parametrize("P,Pmax,kn,F", TILE_SHAPES, ids=[f"P{p}-Pmax{q}-kn{k}-F{f}" for p, q, k, f in TILE_SHAPES])
@pytest.mark.parametrize("name", ["ring3", "ring8"])
def test_bit_for_bit_on_tiles_of_several_frames_and_waves(name, P, Pmax, kn, F):
    for dtype, device in (("float32", False), ("float64", True)):
        K, R, t, kpts, det_of, n_persons = _shape_case(name, P, Pmax, kn, F, dtype)
        ctx = _lib.Context(K, R, t)
        for tau, md in ((6.0, 6), (2.5, 2)):
            got = _matched(ctx, kpts, det_of, n_persons, tau, md, np.dtype(dtype), device)
            for p in range(P):
                kp1, listed = matched.gather_person(kpts, det_of, n_persons, p)
                _assert_person_equals(got, p, _robust(ctx, kp1, listed, tau, md, np.dtype(dtype)), (dtype, tau, md, device))
        ctx.close()


def _compare_with_rule(key, tau, md, got, thr=mc.KTHR):
    """the bars of tests/test_gpu_robust.py::_compare"""
    b, det_of, _ = mc.case(key)
    ref = mc.reference(key, tau, md)
    f64 = got["xyzs"].dtype == np.float64
    views = got["views"].astype(np.uint32)
    sure = ref["margin"] >= MARGIN
    same = views == ref["views"]
    print(f"{key} tau={tau} max_drops={md} {got['xyzs'].dtype}: joints {views.size}, unsure {(~sure).sum()}, mask mismatches {(~same).sum()}, "
          f"drops histogram {np.bincount(ref['drops'].ravel()).tolist()}")
    assert same[sure].all(), f"{(~same & sure).sum()} masks differ where the reference's margin is >= {MARGIN}"
    if not same.all():
        alt = matched.alternative_views(b["K"], b["R"], b["t"], b["kpts"], det_of, b["n_persons"], thr, tau, md, ref, below=MARGIN)
        assert (views[~same] == alt[~same]).all(), "a mask that is neither the reference's nor its alternative"
    zero = ref["views"] == 0
    assert ((views == 0) == zero).all()
    assert not got["xyzs"][zero].any() and not got["resid"][zero].any()
    x, want = got["xyzs"].astype(np.float64), ref["xyzs"]
    err = np.abs(x[..., :3] - want[..., :3])[same]
    tol = 1e-9 if f64 else XYZ_F32
    dr = np.abs(got["resid"].astype(np.float64) - ref["resid"])[same]
    print(f"    max |xyz - rule| = {err.max():.3e} m (bar {tol:.0e}), max resid error = {dr.max():.3e} px")
    assert err.max() < tol, err.max()
    np.testing.assert_allclose(x[..., 3][same], want[..., 3][same], rtol=1e-6)
    if same.all():
        np.testing.assert_allclose(got["pscore"], ref["pscore"], rtol=1e-6)
    ra, rr = (1e-6, 1e-6) if f64 else (1e-5, 1e-6)
    assert (dr <= ra + rr * np.abs(ref["resid"][same])).all(), dr.max()
    return ref


RULE_CASES = [(("woven", "ring4", 2, 3, 17, 17, "float32"), 6.0, 6), (("woven", "ring4", 2, 3, 17, 17, "float32"), 2.5, 2),
              (("woven", "ring8", 2, 3, 17, 17, "float32"), 6.0, 1), (("woven", "ring2", 2, 3, 17, 17, "float32"), 6.0, 6), (("divergence",), 6.0, 6)]


@pytest.mark.parametrize("key,tau,md", RULE_CASES, ids=[f"{'-'.join(str(v) for v in k)}-tau{tau}-d{md}" for k, tau, md in RULE_CASES])
def test_parity_with_the_numpy_rule(key, tau, md):
    b, det_of, _ = mc.case(key)
    ctx = _lib.Context(b["K"], b["R"], b["t"])
    for odt in (np.float64, np.float32):
        ref = _compare_with_rule(key, tau, md, _matched(ctx, b["kpts"], det_of, b["n_persons"], tau, md, np.dtype(odt)))
    if key[0] == "divergence":                                   # persons that share a wave need 0, 1 and 2 drops side by side
        hist = [np.bincount(ref["drops"][:, p].ravel(), minlength=3) for p in range(3)]
        assert hist[0][1] == 1 and hist[1][0] == 0 and hist[2][0] == 133 and hist[2][2] > 50
    ctx.close()


def test_a_persons_bits_do_not_depend_on_the_batch_around_it():
    """F, P, Pmax, the slot and the neighbours: test_bit_for_bit_against_k_dlt_robust (every person equals the single-person kernel on
    its own observations in every shape).  Here: a 17 + 23 cut into calls, a person alone against the same person among others, a
    permuted list, another slot."""
    b = mc.woven("ring5", 3, 4, 40, 17)
    ctx = _lib.Context(b["K"], b["R"], b["t"])
    base = _matched(ctx, b["kpts"], b["det_of"], b["n_persons"], 6.0, 6, np.dtype(np.float32))
    parts = [_matched(ctx, np.ascontiguousarray(b["kpts"][lo:hi]), np.ascontiguousarray(b["det_of"][lo:hi]), np.ascontiguousarray(b["n_persons"][lo:hi]),
                      6.0, 6, np.dtype(np.float32), device=dev) for (lo, hi), dev in (((0, 17), False), ((17, 40), True))]
    for k in OUT_KEYS:
        assert np.array_equal(_bits(np.concatenate([p[k] for p in parts])), _bits(base[k])), k
    alone = _matched(ctx, b["kpts"], np.ascontiguousarray(b["det_of"][..., 1:2]), b["n_persons"], 6.0, 6, np.dtype(np.float32))
    swapped = _matched(ctx, b["kpts"], np.ascontiguousarray(b["det_of"][..., ::-1]), b["n_persons"], 6.0, 6, np.dtype(np.float32))
    perm = np.array([3, 1, 0, 2])
    inv = np.argsort(perm)
    det = np.where(b["det_of"] >= 0, inv[np.maximum(b["det_of"], 0)], -1).astype(np.int32)
    permuted = _matched(ctx, np.ascontiguousarray(b["kpts"][:, :, perm]), det, b["n_persons"], 6.0, 6, np.dtype(np.float32))
    for k in OUT_KEYS:
        assert np.array_equal(_bits(alone[k][:, 0]), _bits(base[k][:, 1])), k
        assert np.array_equal(_bits(swapped[k][:, ::-1]), _bits(base[k])), k
        assert np.array_equal(_bits(permuted[k]), _bits(base[k])), k
    ctx.close()


def test_edges_and_untouched_memory():
    import torch
    b = mc.woven("ring4", 2, 3, 17, 17)
    ctx = _lib.Context(b["K"], b["R"], b["t"])
    L, dt = ctx.L, np.dtype(np.float32)
    # det_of = -1, q >= n_persons, n_persons > Pmax, det_of None: the rule's gather, run by the single-person kernel
    det = b["det_of"].copy()
    det[:, 2, 0] = -1
    det[:, 1:, 1] = np.where(np.arange(17)[:, None] % 2 == 0, -1, det[:, 1:, 1])                 # person 1: one view in every other frame
    npers = b["n_persons"].copy()
    npers[:, 0] = np.where(np.arange(17) % 3 == 0, 1000, np.arange(17) % 3)                       # above Pmax, 1, 2
    for d, n in ((det, b["n_persons"]), (b["det_of"], npers), (None, npers), (None, None)):
        got = _matched(ctx, b["kpts"], d, n, 6.0, 6, dt, device=d is None)
        for p in range(got["xyzs"].shape[1]):
            kp1, listed = matched.gather_person(b["kpts"], d, n, p)
            _assert_person_equals(got, p, _robust(ctx, kp1, listed, 6.0, 6, dt), ("edges", p))
    z = _matched(ctx, b["kpts"], det, b["n_persons"], 6.0, 6, dt)
    assert not z["xyzs"][::2, 1].any() and not z["views"][::2, 1].any() and not z["resid"][::2, 1].any() and not z["pscore"][::2, 1].any()
    assert z["views"][1::2, 1].any()
    # NULL diagnostics and a NULL pscore write nothing; nothing is written behind an array's end (sentinels)
    F, C, Pmax, kn, _ = b["kpts"].shape
    P, n = 2, 17 * 2 * 17
    kp, dd, nn = (torch.from_numpy(np.ascontiguousarray(a)).cuda() for a in (b["kpts"], b["det_of"], b["n_persons"]))
    xyzs = torch.full((n * 4 + 64,), 7.0, dtype=torch.float32, device="cuda")
    ps = torch.full((F * P + 64,), 7.0, dtype=torch.float32, device="cuda")
    views = torch.full((n + 64,), 7, dtype=torch.int32, device="cuda")
    resid = torch.full((n + 64,), 7.0, dtype=torch.float32, device="cuda")

    def call(F_, ps_, views_, resid_):
        return L.snowtri_triangulate_matched(ctx.handle, F_, P, kn, Pmax, _lib.ptr(kp), _lib.F32, _lib.ptr(nn), _lib.ptr(dd), mc.KTHR, 6.0, 6, _lib.ptr(xyzs),
                                             _lib.ptr(ps_), _lib.F32, _lib.ptr(views_), _lib.ptr(resid_), _lib.DEVICE, None)
    assert call(F, None, None, None) == _lib.OK
    torch.cuda.synchronize()
    full = _matched(ctx, b["kpts"], b["det_of"], b["n_persons"], 6.0, 6, dt)
    assert np.array_equal(_bits(xyzs[:n * 4].cpu().numpy()), _bits(full["xyzs"].ravel()))
    assert (xyzs[n * 4:] == 7.0).all() and (ps == 7.0).all() and (views == 7).all() and (resid == 7.0).all()
    assert call(F, ps, views, resid) == _lib.OK
    torch.cuda.synchronize()
    assert np.array_equal(_bits(ps[:F * P].cpu().numpy()), _bits(full["pscore"].ravel())) and (ps[F * P:] == 7.0).all()
    assert np.array_equal(views[:n].cpu().numpy().view(np.uint32), full["views"].ravel()) and (views[n:] == 7).all()
    assert np.array_equal(_bits(resid[:n].cpu().numpy()), _bits(full["resid"].ravel())) and (resid[n:] == 7.0).all()
    # the same on the host path: without diagnostics the staging skips the two arrays, and xyzs and pscore are the full call's
    for odt in (np.float32, np.float64):
        want = _matched(ctx, b["kpts"], b["det_of"], b["n_persons"], 6.0, 6, np.dtype(odt))
        lean = ctx.triangulate_matched(b["kpts"], b["det_of"], b["n_persons"], mc.KTHR, 6.0, 6, dtype=odt, diagnostics=False)
        assert len(lean) == 2 and np.array_equal(_bits(lean[0]), _bits(want["xyzs"])) and np.array_equal(_bits(lean[1]), _bits(want["pscore"]))
    hx = np.full((F, P, kn, 4), 7.0, np.float32)                                    # ... and a NULL pscore beside them
    assert L.snowtri_triangulate_matched(ctx.handle, F, P, kn, Pmax, _lib.ptr(np.ascontiguousarray(b["kpts"])), _lib.F32,
                                         _lib.ptr(np.ascontiguousarray(b["n_persons"])), _lib.ptr(np.ascontiguousarray(b["det_of"])), mc.KTHR, 6.0, 6,
                                         _lib.ptr(hx), None, _lib.F32, None, None, _lib.HOST, None) == _lib.OK
    assert np.array_equal(_bits(hx), _bits(full["xyzs"]))
    # F == 0 is OK and looks at no pointer
    assert L.snowtri_triangulate_matched(ctx.handle, 0, P, kn, Pmax, None, _lib.F32, None, None, mc.KTHR, 6.0, 6, None, None, _lib.F32, None, None,
                                         _lib.DEVICE, None) == _lib.OK
    empty = ctx.triangulate_matched(np.zeros((0, 4, 3, 17, 3), np.float32), np.zeros((0, 4, 2), np.int32))
    assert empty[0].shape == (0, 2, 17, 4) and empty[1].shape == (0, 2)
    with pytest.raises(ValueError, match="max_drops"):
        ctx.triangulate_matched(b["kpts"], b["det_of"], max_drops=7)
    # with timing on, kernel_ms[0] is the kernel's time
    ctx.set_timing(True)
    _matched(ctx, b["kpts"], b["det_of"], b["n_persons"], 6.0, 6, dt)
    ms = ctx.last_kernel_ms()
    assert ms[0] > 0.0 and 0.0 <= ms[1] < 1.0                  # (no second phase: an empty event pair)
    ctx.close()


def test_the_chain_device_resident_on_crossing():
    """reproject_cost -> assign_detections -> triangulate_matched -> refine_joints(views=...) on CUDA tensors.  The triangulation equals
    the NumPy rule fed the same det_of on the bars above; the refinement equals refine_joints_reference fed the same records, det_of
    and views on the bar tests/test_gpu_refine.py holds k_refine to against its rule (costs at rtol 1e-9, points within 1e-6 m); the
    RMS error against the truth is below the 9 mm of the host test."""
    import torch
    import assign_cases as ac
    from snowmocap_amd.refine import refine_joints_reference
    cs = mc.crossing()
    ctx = _lib.Context(cs["K"], cs["R"], cs["t"])
    kp, x0, nn = (torch.from_numpy(np.ascontiguousarray(a)).cuda() for a in (cs["kpts"], cs["xyzs"], cs["n_persons"]))
    cost_sum, cost_n = ctx.reproject_cost(x0, kp, n_persons=nn, keypoint_score_threshold=ac.CROSS_THRESHOLD)
    det_of = ctx.assign_detections(cost_sum, cost_n, ac.CROSS_GATE)
    xyzs, pscore, views, resid = ctx.triangulate_matched(kp, det_of, nn, ac.CROSS_THRESHOLD, 6.0, 1, diagnostics=True)
    assert ctx.last_kernel_names() == "k_dlt_matched<4,double,double>"
    refined, cost, codes = ctx.refine_joints(xyzs, kp, det_of=det_of, n_persons=nn, views=views, keypoint_score_threshold=ac.CROSS_THRESHOLD,
                                             diagnostics=True)
    torch.cuda.synchronize()
    det_np = det_of.cpu().numpy()
    assert np.array_equal(det_np, mc.crossing_det_of("assign"))                       # (k_assign equals its rule bit for bit)
    got = dict(xyzs=xyzs.cpu().numpy(), pscore=pscore.cpu().numpy(), views=views.cpu().numpy().view(np.uint32), resid=resid.cpu().numpy())
    _compare_with_rule(("crossing", "assign"), 6.0, 1, got, thr=ac.CROSS_THRESHOLD)
    rms = mc.rms_error(got["xyzs"], cs["X"])
    r_out, r_cost, r_codes = refine_joints_reference(cs["K"], cs["R"], cs["t"], got["xyzs"], cs["kpts"], det_np, cs["n_persons"], got["views"],
                                                     ac.CROSS_THRESHOLD)
    out = refined.cpu().numpy()
    rms_refined = mc.rms_error(out, cs["X"])
    print(f"crossing: handed-in {mc.rms_error(cs['xyzs'], cs['X']) * 1e3:.2f} mm, re-triangulated {rms * 1e3:.2f} mm, refined {rms_refined * 1e3:.2f} mm, "
          f">= 3 views {(sum((got['views'] >> c) & 1 for c in range(4)) >= 3).mean():.4f}")
    assert rms < 0.009 and rms_refined < 0.009
    assert (codes.cpu().numpy() == r_codes).mean() > 0.999
    assert np.allclose(cost.cpu().numpy(), r_cost, rtol=1e-9, atol=0) and np.abs(out - r_out).max() < 1e-6
    ctx.close()


def test_entry_rejects_bad_arguments_on_a_real_context(tmp_path):
    """tests/abi_badargs_matched.c against libsnowtri.so on the GPU: refusals before any launch, then one good call."""
    lib_dir = os.path.join(ROOT, "snowmocap_amd")
    exe = str(tmp_path / "abi_badargs_matched")
    subprocess.check_call(["gcc", "-std=c99", "-O1", "-I", os.path.join(ROOT, "include"), os.path.join(ROOT, "tests", "abi_badargs_matched.c"),
                           "-o", exe, "-L", lib_dir, "-lsnowtri", "-lm", "-Wl,-rpath," + lib_dir])
    out = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0 and "0 failure(s)" in out.stdout, out.stdout[-3000:] + out.stderr[-2000:]


DBG_CODE = r'''
import sys, numpy as np
sys.path.insert(0, %(root)r)
sys.path.insert(0, %(tests)r)
import matched_cases as mc
from snowmocap_amd import _lib
assert _lib.LIB_PATH.endswith("libsnowtri_dbg.so") and "SNOWTRI_DEBUG_BOUNDS" in _lib.build_info()["variants"]
ran = 0
for name in ("ring2", "ring3", "ring4", "ring5", "ring8"):
    for P, Pmax, kn, F in ((1, 1, 133, 1), (2, 3, 17, 17), (3, 2, 1, 40), (4, 4, 133, 40), (2, 2, 3, 1501), (2, 2, 133, 1501), (3, 2, 17, 2051)):
        if (kn, F) in ((133, 1501), (17, 2051)) and name not in ("ring3", "ring8"):
            continue
        b = mc.woven(name, min(P, Pmax), Pmax, F, kn)
        det_of = b["det_of"] if P <= Pmax else np.ascontiguousarray(np.concatenate([b["det_of"], b["det_of"][..., :P - Pmax]], axis=-1))
        ctx = _lib.Context(b["K"], b["R"], b["t"])
        for dt in (np.float32, np.float64):
            out = ctx.triangulate_matched(b["kpts"], det_of, b["n_persons"], mc.KTHR, 6.0, 6, dtype=dt, diagnostics=True)
            n, first = ctx.debug_faults()
            assert n == 0, "device-side bounds check failed %%d times; first: code %%d at line %%d" %% (n, first >> 32, first & 0xffffffff)
            assert ctx.last_kernel_names().startswith("k_dlt_matched<")
            ran += 1
        ctx.close()
print("matched debug-bounds ok:", ran, "calls")
'''


def test_debug_bounds_on_the_bit_for_bit_batches():
    dbg = os.path.join(ROOT, "snowmocap_amd", "libsnowtri_dbg.so")
    assert os.path.exists(dbg), f"{dbg} is missing: `make -C snowmocap_amd/csrc debug`"
    env = dict(os.environ, SNOWTRI_LIB=dbg)
    p = subprocess.run([sys.executable, "-c", DBG_CODE % {"root": ROOT, "tests": os.path.join(ROOT, "tests")}], env=env, capture_output=True,
                       text=True, timeout=300)
    assert p.returncode == 0 and "matched debug-bounds ok" in p.stdout, (p.stdout[-2000:] + p.stderr[-3000:])
