"""method = DLT_ROBUST on the GPU (k_dlt_robust) against the rule in NumPy (snowmocap_amd/robust.py).

The kernel finds the DLT point by other arithmetic than the reference's SVD, so a comparison of the rule whose two sides agree to
rounding may come out the other way.  The reference reports the relative margin of its closest decision per joint: masks and drop
counts must be EQUAL wherever that margin is >= 1e-6, and elsewhere the mask must be the reference's or the one the rule gives with
that decision taken the other way (tests/test_robust_host.py caps the share of such joints at 0.5 % on every input used here).
Where the masks agree: xyz within 1e-9 m (float64 outputs) / XYZ_F32 (float32), scores at rtol 1e-6, resid within 1e-6 px + 1e-6
relative (float64: 1e-9 m at ~200 px/m is 2e-7 px) / 1e-5 px + 1e-6 relative (float32)."""
import ctypes as ct
import os
import subprocess
import sys

import numpy as np
import pytest

import robust_cases as rc
from conftest import ROOT
from snowmocap_amd import _lib, synth
from snowmocap_amd.batch import BatchTriangulator
from snowmocap_amd.robust import alternative_views

pytestmark = pytest.mark.gpu

XYZ_F32 = 2e-6      # tests/test_gpu_parity.py: float32 rounding of ~5 m coordinates
MARGIN = 1e-6


def _prm(kn, **kw):
    return dict(synth.default_thresholds(), keypoint_score_threshold=rc.KTHR, keypoint_num=kn, center_point_index=0, **kw)


def _batch(key):
    return rc.parity_batch(*key[1:]) if key[0] == "parity" else rc.divergence_batch(key[1])


def _run(key, kn, tau, md, out_dtype, diagnostics=True, pout=1, host=True, **kw):
    b = _batch(key)
    bt = BatchTriangulator(b["K"], b["R"], b["t"], _prm(kn), pout_max=pout, out_dtype=out_dtype, method=_lib.DLT_ROBUST,
                           reproj_threshold_px=tau, max_drops=md, diagnostics=diagnostics, **kw)
    try:
        if host:
            out = bt.run_host(b["kpts"], b["n_persons"])
            assert out["status"] == _lib.OK
        else:
            import torch
            kp = torch.from_numpy(np.ascontiguousarray(b["kpts"])).cuda()
            npers = torch.from_numpy(b["n_persons"].copy()).cuda() if b["n_persons"] is not None else None
            o = bt.run_torch(kp, npers)
            torch.cuda.synchronize()
            out = {k: v.cpu().numpy() for k, v in o.items()}
        names = bt.ctx.last_kernel_names()
    finally:
        bt.close()
    assert names.startswith("k_dlt_robust<%d," % b["K"].shape[0]), names
    return out


def _compare(key, kn, tau, md, out, what=""):
    """out: a result with diagnostics -- against the reference as the module docstring states."""
    b = _batch(key)
    ref = rc.reference(key, kn, tau, md)
    f64 = out["xyzs"].dtype == np.float64
    views = out["views"].astype(np.uint32)
    drops_ref = ref["drops"]
    sure = ref["margin"] >= MARGIN
    pc = lambda a: sum(((a >> np.uint32(c)) & 1).astype(np.int32) for c in range(8))
    kthr_pass = ~(b["kpts"][:, :, 0, :kn, 2].astype(np.float64) < rc.KTHR)
    if b["n_persons"] is not None:
        kthr_pass = kthr_pass & (b["n_persons"] > 0)[:, :, None]
    start = np.zeros(views.shape, np.uint32)
    for c in range(kthr_pass.shape[1]):
        start |= kthr_pass[:, c].astype(np.uint32) << np.uint32(c)
    drops = np.where(views != 0, pc(start) - pc(views), 0)
    same = views == ref["views"]
    print(f"{what}{key} kn={kn} tau={tau} max_drops={md} {out['xyzs'].dtype}: joints {views.size}, unsure {(~sure).sum()}, "
          f"mask mismatches {(~same).sum()}, drops histogram {np.bincount(drops_ref.ravel()).tolist()}")
    assert same[sure].all(), f"{(~same & sure).sum()} masks differ where the reference's margin is >= {MARGIN}"
    assert (drops[sure] == drops_ref[sure]).all()
    if not same.all():
        alt = alternative_views(b["K"], b["R"], b["t"], b["kpts"], b["n_persons"], rc.KTHR, kn, tau, md, ref, below=MARGIN)
        assert (views[~same] == alt[~same]).all(), "a mask that is neither the reference's nor its alternative"
    assert (out["count"] == 1).all() and (out["flags"] == _lib.FLAG_FASTPATH).all()
    # zero records and views = 0 exactly where the reference has them
    zero = ref["views"] == 0
    assert ((views == 0) == zero).all()
    assert not out["xyzs"][:, 0][zero].any() and not out["resid"][zero].any()
    got, want = out["xyzs"][:, 0].astype(np.float64), ref["xyzs"][:, 0]
    err = np.abs(got[..., :3] - want[..., :3])[same]
    tol = 1e-9 if f64 else XYZ_F32
    print(f"    max |xyz - reference| = {err.max():.3e} m (bar {tol:.0e}), max resid error = "
          f"{np.abs(out['resid'].astype(np.float64) - ref['resid'])[same].max():.3e} px")
    assert err.max() < tol, err.max()
    np.testing.assert_allclose(got[..., 3][same], want[..., 3][same], rtol=1e-6)
    if same.all():
        np.testing.assert_allclose(out["pscore"][:, 0], ref["pscore"][:, 0], rtol=1e-6)
    ra, rr = (1e-6, 1e-6) if f64 else (1e-5, 1e-6)
    dr = np.abs(out["resid"].astype(np.float64) - ref["resid"])[same]
    assert (dr <= ra + rr * np.abs(ref["resid"][same])).all(), dr.max()
    # slots behind the person are zero-filled
    assert not out["xyzs"][:, 1:].any() and not out["pscore"][:, 1:].any()


PARITY = [c for c in rc.gpu_cases() if c[0][0] == "parity"]


@pytest.mark.parametrize("key,kn,tau,md", PARITY, ids=[f"{k[1]}-F{k[2]}-J{k[3]}-{k[4]}-kn{kn}-tau{tau}-d{md}" for k, kn, tau, md in PARITY])
def test_parity_with_the_reference_rule(key, kn, tau, md):
    for out_dtype in (np.float64, np.float32):
        _compare(key, kn, tau, md, _run(key, kn, tau, md, out_dtype, pout=2 if key[2] == 3 else 1))


@pytest.mark.parametrize("kind", ["one", "all", "mixed"])
def test_divergence_shapes(kind):
    """One lane of one wave enters the leave-one-out round; every lane does; lanes of a wave need 0, 1 and 2 drops side by side."""
    key = ("divergence", kind)
    ref = rc.reference(key, 133, 6.0, 6)
    hist = np.bincount(ref["drops"].ravel(), minlength=3)
    if kind == "one":
        assert hist[1] == 1 and hist[2:].sum() == 0 and ref["drops"][1, 77] == 1
    elif kind == "all":
        assert hist[0] == 0
    else:
        # (joints with two shifted views: most take the two drops, the rest one or three)
        assert (ref["drops"][0, :9] == np.arange(9) % 3).all() and hist[0] == 133 and hist[1] >= 133 and hist[2] > 50
    for out_dtype in (np.float64, np.float32):
        _compare(key, 133, 6.0, 6, _run(key, 133, 6.0, 6, out_dtype))


def test_route_equivalences_bit_for_bit():
    key = ("parity", "ring5", 40, 133, "float32")
    b = _batch(key)
    base = _run(key, 133, 6.0, 6, np.float32)
    tor = _run(key, 133, 6.0, 6, np.float32, host=False)
    for k in ("xyzs", "pscore", "count", "views", "resid"):
        assert np.array_equal(base[k].view(np.uint32), tor[k].view(np.uint32)), k       # run_torch == run_host
    assert np.array_equal(base["flags"], tor["flags"].view(np.uint32))
    # diagnostics off: the fused call after set_robust -- the same joints
    fused = _run(key, 133, 6.0, 6, np.float32, diagnostics=False)
    assert set(fused) == {"xyzs", "pscore", "count", "flags", "status"}
    for k in ("xyzs", "pscore", "count", "flags"):
        assert np.array_equal(base[k].view(np.uint32), fused[k].view(np.uint32)), k
    # one 40-frame call == calls of 17 + 23 frames
    bt = BatchTriangulator(b["K"], b["R"], b["t"], _prm(133), out_dtype=np.float32, method=_lib.DLT_ROBUST, reproj_threshold_px=6.0,
                           max_drops=6, diagnostics=True)
    parts = [bt.run_host(b["kpts"][lo:hi], b["n_persons"][lo:hi]) for lo, hi in ((0, 17), (17, 40))]
    for k in ("xyzs", "pscore", "count", "flags", "views", "resid"):
        assert np.array_equal(np.concatenate([p[k] for p in parts]).view(np.uint32), base[k].view(np.uint32)), k
    # the fused call with set_robust == snowtri_triangulate_robust with null diagnostics (both straight through the C ABI)
    L, prm = bt.ctx.L, _lib.make_params(**_prm(133))
    kp, npers = np.ascontiguousarray(b["kpts"]), np.ascontiguousarray(b["n_persons"])
    res = []
    for direct in (False, True):
        xyzs, ps = np.full((40, 1, 133, 4), 7.0, np.float32), np.full((40, 1), 7.0, np.float32)
        cnt, fl = np.zeros(40, np.int32), np.zeros(40, np.uint32)
        if direct:
            rcode = L.snowtri_triangulate_robust(bt.ctx.handle, 40, 133, _lib.ptr(kp), _lib.F32, _lib.ptr(npers), prm, 2.5, 2, 1, _lib.ptr(xyzs),
                                                 _lib.ptr(ps), _lib.F32, _lib.ptr(cnt), _lib.ptr(fl), None, None, _lib.HOST, None)
        else:
            bt.ctx.set_robust(2.5, 2)
            rcode = L.snowtri_triangulate_condense(bt.ctx.handle, 40, 1, 133, _lib.ptr(kp), _lib.F32, _lib.ptr(npers), prm, _lib.DLT_ROBUST, 1,
                                                   _lib.ptr(xyzs), _lib.ptr(ps), _lib.F32, _lib.ptr(cnt), _lib.ptr(fl), _lib.HOST, None)
        assert rcode == _lib.OK and bt.ctx.last_kernel_names() == "k_dlt_robust<5,float,float>"
        res.append((xyzs, ps, cnt, fl))
    for a, c in zip(*res):
        assert np.array_equal(a.view(np.uint32), c.view(np.uint32))
    assert not np.array_equal(res[0][0], base["xyzs"])          # (2.5 px, 2 drops is another answer than 6 px, 6 drops)
    # F == 0 is OK and touches nothing
    assert L.snowtri_triangulate_robust(bt.ctx.handle, 0, 133, None, _lib.F32, None, prm, 6.0, 1, 1, None, None, _lib.F32, None, None, None,
                                        None, _lib.HOST, None) == _lib.OK
    bt.close()
    # zero_fill=False leaves slot 0 identical (device call, three slots)
    import torch
    kpt, npt = torch.from_numpy(kp).cuda(), torch.from_numpy(npers).cuda()
    outs = []
    for zf in (True, False):
        bz = BatchTriangulator(b["K"], b["R"], b["t"], _prm(133), pout_max=3, out_dtype=np.float32, method=_lib.DLT_ROBUST,
                               reproj_threshold_px=6.0, max_drops=6, zero_fill=zf)
        o = bz.alloc_outputs(40)
        o["xyzs"].fill_(5.0)
        o["pscore"].fill_(5.0)
        bz.run_torch(kpt, npt, out=o)
        torch.cuda.synchronize()
        outs.append({k: v.cpu().numpy() for k, v in o.items()})
        bz.close()
    assert np.array_equal(outs[0]["xyzs"][:, 0].view(np.uint32), outs[1]["xyzs"][:, 0].view(np.uint32))
    assert np.array_equal(outs[0]["xyzs"][:, 0].view(np.uint32), base["xyzs"][:, 0].view(np.uint32))
    assert np.array_equal(outs[0]["pscore"][:, 0], outs[1]["pscore"][:, 0]) and np.array_equal(outs[0]["count"], outs[1]["count"])
    assert not outs[0]["xyzs"][:, 1:].any() and not outs[0]["pscore"][:, 1:].any()
    assert (outs[1]["xyzs"][:, 1:] == 5.0).all()                # untouched, as the flag allows


@pytest.mark.parametrize("name", ["ring3", "floor", "ring8"])
def test_no_drop_settings_agree_with_method_dlt(name):
    """(6, 0) and (inf, 1) are method = DLT: within 2e-9 m of it on the same batch (float64), each within 1e-9 m of the same SVD."""
    key = ("parity", name, 40, 133, "float32")
    b = _batch(key)
    bt = BatchTriangulator(b["K"], b["R"], b["t"], _prm(133), out_dtype=np.float64, method=_lib.DLT)
    dlt = bt.run_host(b["kpts"], b["n_persons"])
    bt.close()
    ref = rc.reference(key, 133, 6.0, 0)
    assert np.abs(dlt["xyzs"][..., :3] - ref["xyzs"][..., :3]).max() < 1e-9
    for tau, md in ((6.0, 0), (float("inf"), 1)):
        out = _run(key, 133, tau, md, np.float64)
        d = np.abs(out["xyzs"][..., :3] - dlt["xyzs"][..., :3]).max()
        e = np.abs(out["xyzs"][..., :3] - ref["xyzs"][..., :3]).max()
        print(f"{name} ({tau}, {md}): max |robust - DLT| = {d:.3e} m, max |robust - SVD| = {e:.3e} m")
        assert d < 2e-9 and e < 1e-9
        np.testing.assert_allclose(out["xyzs"][..., 3], dlt["xyzs"][..., 3], rtol=1e-6)
        np.testing.assert_allclose(out["pscore"], dlt["pscore"], rtol=1e-6)
        assert np.array_equal(out["count"], dlt["count"]) and np.array_equal(out["flags"], dlt["flags"])
        assert np.array_equal(out["views"], ref["views"])


def test_validation():
    L = _lib.lib()
    K, R, t = rc.rig("ring4")
    rng = np.random.default_rng(1)
    X = synth.make_people(rng, 2, 2, J=17)
    kp2, np2 = synth.make_keypoints(rng, K, R, t, X)           # two detections per camera
    prm = _prm(17)
    bt = BatchTriangulator(K, R, t, prm, method=_lib.DLT_ROBUST)
    with pytest.raises(_lib.SnowtriError) as ei:
        bt.run_host(kp2, np2)
    assert ei.value.status == _lib.ERR_BAD_ARG and "Pmax == 1" in L.snowtri_last_error().decode()
    h, P = bt.ctx.handle, _lib.make_params(**prm)
    for tau, md in ((-1.0, 1), (float("nan"), 1), (6.0, 7), (6.0, -1)):
        assert L.snowtri_ctx_set_robust(h, tau, md) == _lib.ERR_BAD_ARG, (tau, md)
    assert L.snowtri_ctx_set_robust(h, float("inf"), 6) == _lib.OK and L.snowtri_ctx_set_robust(h, 0.0, 0) == _lib.OK
    kp1 = np.ascontiguousarray(kp2[:, :, :1])
    xyzs, ps, cnt = np.zeros((2, 1, 17, 4), np.float32), np.zeros((2, 1), np.float32), np.zeros(2, np.int32)

    def direct(tau, md, ctx=h, J=17, kp=kp1):
        return L.snowtri_triangulate_robust(ctx, 2, J, _lib.ptr(kp), _lib.F32, None, P, tau, md, 1, _lib.ptr(xyzs), _lib.ptr(ps), _lib.F32,
                                            _lib.ptr(cnt), None, None, None, _lib.HOST, None)
    assert direct(6.0, 1) == _lib.OK
    assert direct(6.0, 7) == _lib.ERR_BAD_ARG and "max_drops" in L.snowtri_last_error().decode()
    assert direct(-0.5, 1) == _lib.ERR_BAD_ARG and direct(float("nan"), 1) == _lib.ERR_BAD_ARG
    # method = 3 stays a bad argument
    assert L.snowtri_triangulate_condense(h, 2, 1, 17, _lib.ptr(kp1), _lib.F32, None, P, 3, 1, _lib.ptr(xyzs), _lib.ptr(ps), _lib.F32,
                                          _lib.ptr(cnt), None, _lib.HOST, None) == _lib.ERR_BAD_ARG
    bt.close()
    # nine cameras
    K9, R9, t9 = synth.ring_rig(9)
    c9 = _lib.Context(K9, R9, t9)
    kp9 = np.zeros((2, 9, 1, 17, 3), np.float32)
    assert direct(6.0, 1, ctx=c9.handle, kp=kp9) == _lib.ERR_BAD_ARG and "2 to 8 cameras" in L.snowtri_last_error().decode()
    c9.close()
    # misaligned device outputs
    import torch
    bt = BatchTriangulator(K, R, t, prm, method=_lib.DLT_ROBUST, diagnostics=True)
    kpt = torch.from_numpy(kp1).cuda()
    o = bt.alloc_outputs(2)
    raw = torch.empty(2 * 17 * 16 + 64, dtype=torch.uint8, device="cuda")

    def dev(xyz_ptr, views_ptr, resid_ptr):
        return L.snowtri_triangulate_robust(bt.ctx.handle, 2, 17, ct.c_void_p(kpt.data_ptr()), _lib.F32, None, P, 6.0, 1, 1, ct.c_void_p(xyz_ptr),
                                            ct.c_void_p(o["pscore"].data_ptr()), _lib.F32, ct.c_void_p(o["count"].data_ptr()),
                                            ct.c_void_p(o["flags"].data_ptr()), ct.c_void_p(views_ptr), ct.c_void_p(resid_ptr), _lib.DEVICE, None)
    good = (o["xyzs"].data_ptr(), o["views"].data_ptr(), o["resid"].data_ptr())
    assert dev(*good) == _lib.OK
    assert dev(raw.data_ptr() + 8, good[1], good[2]) == _lib.ERR_BAD_ARG          # joint records: 16 bytes
    assert dev(good[0], raw.data_ptr() + 2, good[2]) == _lib.ERR_BAD_ARG          # views: 4 bytes
    assert dev(good[0], good[1], raw.data_ptr() + 2) == _lib.ERR_BAD_ARG          # resid: its element
    torch.cuda.synchronize()
    bt.close()


DBG_CODE = r'''
import sys, numpy as np
sys.path.insert(0, %(root)r)
sys.path.insert(0, %(tests)r)
import robust_cases as rc
from snowmocap_amd import synth, _lib
from snowmocap_amd.batch import BatchTriangulator
assert _lib.LIB_PATH.endswith("libsnowtri_dbg.so") and "SNOWTRI_DEBUG_BOUNDS" in _lib.build_info()["variants"]
ran = 0
for name in ("floor", "ring8"):
    b = rc.parity_batch(name)
    for kn, pout, out_dtype, diag in ((133, 1, np.float32, True), (30, 3, np.float64, True), (133, 1, np.float32, False)):
        prm = dict(synth.default_thresholds(), keypoint_score_threshold=rc.KTHR, keypoint_num=kn, center_point_index=0)
        bt = BatchTriangulator(b["K"], b["R"], b["t"], prm, pout_max=pout, out_dtype=out_dtype, method=_lib.DLT_ROBUST,
                               reproj_threshold_px=6.0, max_drops=6, diagnostics=diag)
        out = bt.run_host(b["kpts"], b["n_persons"])
        n, first = bt.ctx.debug_faults()
        assert n == 0, "device-side bounds check failed %%d times; first: code %%d at line %%d" %% (n, first >> 32, first & 0xffffffff)
        assert bt.ctx.last_kernel_names().startswith("k_dlt_robust<")
        if diag:
            ref = rc.reference(("parity", name, 40, 133, "float32"), kn, 6.0, 6)
            assert np.array_equal(out["views"], ref["views"])
        bt.close()
        ran += 1
print("robust debug-bounds ok:", ran, "calls")
'''


def test_debug_bounds_on_the_parity_batches():
    dbg = os.path.join(ROOT, "snowmocap_amd", "libsnowtri_dbg.so")
    assert os.path.exists(dbg), f"{dbg} is missing: `make -C snowmocap_amd/csrc debug`"
    env = dict(os.environ, SNOWTRI_LIB=dbg)
    p = subprocess.run([sys.executable, "-c", DBG_CODE % {"root": ROOT, "tests": os.path.join(ROOT, "tests")}], env=env, capture_output=True,
                       text=True, timeout=300)
    assert p.returncode == 0 and "robust debug-bounds ok" in p.stdout, (p.stdout[-2000:] + p.stderr[-3000:])


def test_track_pipeline_runs_the_robust_method():
    """TrackPipeline(method=DLT_ROBUST) on a 30-frame single-person recording (the context's default settings): its triangulated
    joints are BatchTriangulator's."""
    from snowmocap_amd.pipeline import TrackPipeline
    K, R, t = rc.rig("floor")
    rng = np.random.default_rng(31)
    X, _ = synth.make_walkers(rng, 30, 1, step=0.03)
    kp, npers = synth.make_keypoints(rng, K, R, t, X, pixel_sigma=1.0, score_range=(3.5, 8.0))
    kp, cam = synth.add_outliers(rng, kp)
    thr = dict(synth.default_thresholds(), keypoint_score_threshold=rc.KTHR)
    profile = {n: [2.0, 0.75, 0.0] for n in __import__("snowmocap_amd.blender", fromlist=["CONTROL_POINT_NAMES"]).CONTROL_POINT_NAMES}
    pipe = TrackPipeline(K, R, t, thr, profile, n_persons_out=1, method=_lib.DLT_ROBUST)
    res = pipe.run(kp, npers)
    bt = BatchTriangulator(K, R, t, thr, pout_max=1, out_dtype=np.float64, method=_lib.DLT_ROBUST, diagnostics=True)
    want = bt.run_host(kp, npers)
    bt.close()
    got = res["xyzs"]
    got = got.cpu().numpy() if hasattr(got, "cpu") else np.asarray(got)
    assert np.array_equal(got.reshape(want["xyzs"].shape), want["xyzs"])
    hit = (cam >= 0)[:, :want["views"].shape[1]]
    assert (want["views"][hit] != 0xf).mean() > 0.9 and (want["views"][~hit] == 0xf).mean() > 0.99
