"""Row N4, k_undistort behind snowtri_undistort_keypoints / BatchTriangulator(D=...), held to the exact inverse of the lens model
(oracle/undistort_exact.py, 50 digits) on the lenses, rigs and shapes of tests/undistort_cases.py: five lenses incl. two barrel
ones, a different lens and a skew of 0.5-4 px per camera, C = 3, 4, 5, 8, per_cam below / equal to / above a wave and a block.

  * parity.  float64: within 1e-11 px of the exact inverse of the raw pixel.  Derived, not measured: evaluating the forward model
    costs ~10 eps at |x| <= 1.2 (normalised), Newton's fixed point sits that residual divided by the Jacobian's smallest eigenvalue
    (>= 0.31, test_undistort_host.py) away, times fx ~ 700 px = 2.5e-12 px; plus one output rounding of a 1300 px coordinate,
    2.3e-13; the bar is 4 times the sum.  float32: the exact inverse of the float32-rounded input, to half a float32 ulp of the
    expected value + 1e-9 px (the fp64 error above, with room; no conditioning enters).  Scores are the input's bits.
  * camera index: every observation lands on the inverse under ITS camera's lens and > 1 px from the inverse under any other's.
  * a pixel's bits depend on its own input only: frames 17..39 alone = the same frames of the 40-frame call; a NaN or a far-off
    pixel in each 64 changes no other observation; BatchTriangulator(D=...) gives the same bits for 40 frames and for 17 + 23.
  * non-finite pixels come out non-finite in u and v, score untouched; input buffers are left alone; F = 0 is OK; the debug build
    counts no device-side bounds fault.
"""
import os
import subprocess
import sys

import numpy as np
import pytest

import undistort_cases as uc
from snowmocap_amd import _lib, synth

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BAR_F64 = 1e-11             # px: 4 x (10 eps / 0.31 x 700 + 2.3e-13), see the module docstring
F32_EXTRA = 1e-9            # px, on top of half a float32 ulp of the expected value


@pytest.fixture(scope="module")
def api():
    import snowmocap_amd as sm
    assert _lib.lib().snowtri_device_count() > 0, "these tests need the HIP device"
    return sm


def _context(cs):
    ctx = _lib.Context(cs["K"], cs["R"], cs["t"])
    ctx.set_distortion(cs["D"])
    return ctx


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint64 if a.dtype == np.float64 else np.uint32)


def _same_bits(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and np.array_equal(_bits(a), _bits(b))


# ------------------------------------------------------------------------------------------------ parity
@pytest.mark.parametrize("rig_name", list(uc.RIGS))
def test_parity_with_the_exact_inverse(api, rig_name):
    failed = []
    worst = {"float64": {}, "float32": {}}
    ctx = None
    for shape in uc.shapes_of(rig_name):
        for dtype_name in ("float64", "float32"):
            cs = uc.case(rig_name, shape, dtype_name)
            ctx = ctx or _context(cs)
            got = ctx.undistort_keypoints(cs["kpts"])
            assert got.dtype == cs["kpts"].dtype and got.shape == cs["kpts"].shape
            if not np.array_equal(_bits(got[..., 2]), _bits(cs["kpts"][..., 2])):
                failed.append(f"{shape} {dtype_name}: scores are not the input's bits")
            err = np.abs(got[..., :2].astype(np.float64) - cs["want"])
            tol = np.full(err.shape, BAR_F64) if dtype_name == "float64" else 0.5 * uc.f32_ulp(cs["want"]) + F32_EXTRA
            for c, lens in enumerate(cs["lenses"]):
                fig = err[:, c] if dtype_name == "float64" else err[:, c] / uc.f32_ulp(cs["want"][:, c])     # (float32: in ulps of the expected value)
                worst[dtype_name][lens] = max(worst[dtype_name].get(lens, 0.0), float(np.nanmax(fig)))
            bad = ~(err <= tol)
            if bad.any():
                k = np.unravel_index(int(np.argmax(np.where(np.isfinite(err), err / tol, np.inf))), err.shape)
                failed.append(f"{shape} {dtype_name}: {int(bad.sum())} of {err.size} over the bar, worst at {k}: {err[k]:.3e} px against {tol[k]:.3e}")
    ctx.close()
    print(f"    {rig_name}: max |k_undistort - exact inverse| per lens, float64 (px): " + ", ".join(f"{k} {v:.2e}" for k, v in worst["float64"].items()))
    print(f"    {rig_name}: float32 route, max error in float32 ulps of the expected value (bar: 0.5 + 1e-9 px): "
          + ", ".join(f"{k} {v:.4f}" for k, v in worst["float32"].items()))
    assert not failed, f"{rig_name}: " + " | ".join(failed)


# ------------------------------------------------------------------------------------------------ camera index
@pytest.mark.parametrize("rig_name", uc.DISTINCT_LENS_RIGS)
def test_every_observation_gets_its_own_cameras_lens(api, rig_name):
    from oracle import undistort as ou
    ctx = None
    for shape in ((1, 3, 21), (5, 2, 133)):
        cs = uc.case(rig_name, shape)
        K, D, want = cs["K"], cs["D"], cs["want"]
        C = K.shape[0]
        raw = cs["kpts"][..., :2]
        # where another camera's lens (on this camera's K: a D stored under the wrong index), or another camera's whole row
        # (K and D: a wrong index in the kernel), would put each observation.  A Newton that leaves the lens's domain counts as far.
        alts = []
        for c in range(C):
            for o in range(C):
                if o != c:
                    for Kc in (K[c], K[o]):
                        a = np.full(want.shape, np.nan)
                        with np.errstate(all="ignore"):
                            a[:, c] = ou.undistort_pixels(Kc, D[o], raw[:, c])
                        alts.append((c, a))
        # on the reference first: the pixels where every other lens is > 2 px off
        sure = np.ones(want.shape[:-1], dtype=bool)
        for c, a in alts:
            sure[:, c] &= ~(np.linalg.norm(a[:, c] - want[:, c], axis=-1) <= 2.0)
        assert all(sure[:, c].mean() > 0.25 for c in range(C)), [float(sure[:, c].mean()) for c in range(C)]
        ctx = ctx or _context(cs)
        got = ctx.undistort_keypoints(cs["kpts"])[..., :2]
        own = np.linalg.norm(got - want, axis=-1)
        assert own.max() <= 2 * BAR_F64, (shape, own.max())
        for c, a in alts:
            other = np.linalg.norm(got[:, c] - a[:, c], axis=-1)
            assert not (other[sure[:, c]] <= 1.0).any(), (shape, c)
        print(f"    {rig_name} {shape}: {int(sure.sum())} of {sure.size} observations tell the cameras apart by > 2 px; all on their own lens")
    ctx.close()


# ------------------------------------------------------------------------------------------------ bits independent of the wave
@pytest.mark.parametrize("rig_name", ["floor", "ring3", "ring5"])
def test_frames_alone_equal_the_same_frames_of_the_full_call(api, rig_name):
    """17 frames shift every later observation by 17 x C x 133 lanes: 20, 63 and 41 mod 64 on 4, 3 and 5 cameras."""
    cs = uc.case(rig_name, uc.WAVE_SHAPE)
    ctx = _context(cs)
    full = ctx.undistort_keypoints(cs["kpts"])
    tail = ctx.undistort_keypoints(cs["kpts"][17:])
    head = ctx.undistort_keypoints(cs["kpts"][:17])
    ctx.close()
    assert np.abs(full[..., :2] - cs["want"]).max() <= BAR_F64
    differ = (_bits(full[17:]) != _bits(tail)).any(axis=-1)
    print(f"    {rig_name}: {int(differ.sum())} of {differ.size} observations of frames 17..39 change bits when run alone"
          + (f", by up to {np.abs(full[17:] - tail).max():.2e} px" if differ.any() else ""))
    assert not differ.any(), f"{int(differ.sum())} of {differ.size} observations depend on their wave-mates"
    assert _same_bits(full[:17], head)


@pytest.mark.parametrize("what", ["nan", "far"])
def test_a_bad_pixel_changes_no_other_observation(api, what):
    cs = uc.case(uc.WAVE_RIG, uc.WAVE_SHAPE)
    ctx = _context(cs)
    clean = ctx.undistort_keypoints(cs["kpts"])
    kp, hit = uc.poison(cs["kpts"], np.nan if what == "nan" else 1e9)
    got = ctx.undistort_keypoints(kp)
    again = ctx.undistort_keypoints(cs["kpts"])                       # nothing faulted: the context still answers
    ctx.close()
    assert _same_bits(again, clean)
    assert hit.sum() == -(-(hit.size - 37) // 64)
    differ = (_bits(got) != _bits(clean)).any(axis=-1) & ~hit
    print(f"    {what}: {int(differ.sum())} of {int((~hit).sum())} other observations change bits")
    assert not differ.any(), f"{int(differ.sum())} observations changed because a wave-mate was {what}"
    assert np.array_equal(_bits(got[..., 2]), _bits(kp[..., 2]))
    if what == "nan":
        assert not np.isfinite(got[hit][:, :2]).any()


@pytest.mark.parametrize("in_dtype", ["float64", "float32"])
@pytest.mark.parametrize("method", ["PAIRWISE", "DLT", "DLT_ROBUST"])
def test_batch_triangulator_is_bit_identical_however_the_frames_are_cut(api, method, in_dtype):
    rec = uc.recording(uc.WAVE_RIG, 40, in_dtype)
    bt = api.BatchTriangulator(rec["K"], rec["R"], rec["t"], synth.default_thresholds(), pout_max=1, out_dtype=np.float64,
                               method=getattr(_lib, method), D=rec["D"])
    try:
        full = bt.run_host(rec["kpts"], rec["n_persons"])
        parts = [bt.run_host(rec["kpts"][a:b], rec["n_persons"][a:b]) for a, b in ((0, 17), (17, 40))]
    finally:
        bt.close()
    assert full["status"] == _lib.OK and all(p["status"] == _lib.OK for p in parts)
    assert (full["count"] == 1).all() and np.abs(full["xyzs"][:, 0, :, :3] - rec["X"][:, 0]).max() < (1e-7 if in_dtype == "float64" else 1e-3)
    for key in ("xyzs", "pscore", "count", "flags"):
        cut = np.concatenate([p[key] for p in parts], axis=0)
        differ = int((np.ascontiguousarray(cut).view(np.uint8) != np.ascontiguousarray(full[key]).view(np.uint8)).sum())
        assert cut.dtype == full[key].dtype and differ == 0, f"{method} {in_dtype} {key}: {differ} bytes differ between 40 frames and 17 + 23"


# ------------------------------------------------------------------------------------------------ non-finite input
@pytest.mark.parametrize("dtype_name", ["float64", "float32"])
def test_non_finite_pixels_come_out_non_finite(api, dtype_name):
    cs = uc.case("ring5", (3, 1, 17), dtype_name)
    kp = np.array(cs["kpts"], copy=True)
    flat = kp.reshape(-1, 3)
    K = cs["K"]
    bad = {3: (np.nan, None), 40: (None, np.nan), 77: (np.inf, None), 110: (None, -np.inf), 150: (np.nan, np.inf), 201: (-np.inf, np.inf),
           230: (np.inf, float(K[3, 1, 2]))}                          # (lane 230 is camera 3: v on the principal point, y = 0)
    assert flat.shape[0] == 255 and (230 // 17) % 5 == 3
    for i, (u, v) in bad.items():
        if u is not None:
            flat[i, 0] = u
        if v is not None:
            flat[i, 1] = v
    ctx = _context(cs)
    clean = ctx.undistort_keypoints(cs["kpts"])
    got = ctx.undistort_keypoints(kp)
    again = ctx.undistort_keypoints(cs["kpts"])
    ctx.close()
    g = got.reshape(-1, 3)
    for i in bad:
        assert not np.isfinite(g[i, 0]) and not np.isfinite(g[i, 1]), (i, flat[i], g[i])
    assert np.array_equal(_bits(g[:, 2]), _bits(flat[:, 2]))
    rest = np.setdiff1d(np.arange(255), list(bad))
    assert np.array_equal(_bits(g[rest]), _bits(clean.reshape(-1, 3)[rest])) and _same_bits(again, clean)


# ------------------------------------------------------------------------------------------------ buffers
def test_device_buffers_are_left_alone(api):
    import torch
    L = _lib.lib()
    for dtype_name, code in (("float64", _lib.F64), ("float32", _lib.F32)):
        cs = uc.case("ring5", (5, 2, 133), dtype_name)
        F, C, P, J, _ = cs["kpts"].shape
        ctx = _context(cs)
        host = ctx.undistort_keypoints(cs["kpts"])
        src = torch.from_numpy(np.array(cs["kpts"], copy=True)).to("cuda:0")
        dst = torch.full_like(src, -7.0)
        st = torch.cuda.current_stream().cuda_stream
        _lib.check(L.snowtri_undistort_keypoints(ctx.handle, F, P, J, src.data_ptr(), dst.data_ptr(), code, _lib.DEVICE, st), "undistort")
        torch.cuda.synchronize()
        assert _same_bits(src.cpu().numpy(), cs["kpts"]), "the input buffer was written"
        assert _same_bits(dst.cpu().numpy(), host)
        _lib.check(L.snowtri_undistort_keypoints(ctx.handle, F, P, J, src.data_ptr(), src.data_ptr(), code, _lib.DEVICE, st), "undistort")
        torch.cuda.synchronize()
        assert _same_bits(src.cpu().numpy(), host), "in place differs from out of place"
        # F = 0: nothing to do, with or without buffers
        for space in (_lib.HOST, _lib.DEVICE):
            assert L.snowtri_undistort_keypoints(ctx.handle, 0, P, J, None, None, code, space, None) == _lib.OK
        assert ctx.undistort_keypoints(cs["kpts"][:0]).shape == (0, C, P, J, 3)
        assert L.snowtri_undistort_keypoints(ctx.handle, F, P, J, None, None, code, _lib.DEVICE, None) == _lib.ERR_BAD_ARG
        ctx.close()


@pytest.mark.parametrize("in_dtype", ["float64", "float32"])
def test_run_torch_leaves_the_callers_keypoints_alone(api, in_dtype):
    import torch
    rec = uc.recording(uc.WAVE_RIG, 40, in_dtype)
    bt = api.BatchTriangulator(rec["K"], rec["R"], rec["t"], synth.default_thresholds(), pout_max=1, out_dtype=np.float64, D=rec["D"])
    try:
        want = bt.run_host(rec["kpts"], rec["n_persons"])
        kp = torch.from_numpy(np.array(rec["kpts"], copy=True)).to("cuda:0")
        npers = torch.from_numpy(np.array(rec["n_persons"], copy=True)).to("cuda:0")
        out = bt.run_torch(kp, npers)
        out2 = bt.run_torch(kp, npers)                                # a second call sees the same raw pixels
        torch.cuda.synchronize()
        assert _same_bits(kp.cpu().numpy(), rec["kpts"]), "run_torch wrote the caller's keypoints"
        assert np.array_equal(npers.cpu().numpy(), rec["n_persons"])
        for o in (out, out2):
            assert _same_bits(o["xyzs"].cpu().numpy(), want["xyzs"]) and np.array_equal(o["count"].cpu().numpy(), want["count"])
    finally:
        bt.close()


# ------------------------------------------------------------------------------------------------ debug build
DBG_CODE = r'''
import sys, numpy as np
sys.path.insert(0, %(root)r)
sys.path.insert(0, %(tests)r)
import undistort_cases as uc
from snowmocap_amd import synth, _lib
from snowmocap_amd.batch import BatchTriangulator
assert _lib.LIB_PATH.endswith("libsnowtri_dbg.so") and "SNOWTRI_DEBUG_BOUNDS" in _lib.build_info()["variants"]
for dtype_name in ("float64", "float32"):
    cs = uc.case("ring5", (5, 2, 133), dtype_name)
    ctx = _lib.Context(cs["K"], cs["R"], cs["t"])
    ctx.set_distortion(cs["D"])
    got = ctx.undistort_keypoints(cs["kpts"])
    n, first = ctx.debug_faults()
    assert n == 0, "device-side bounds check failed %%d times; first: code %%d at line %%d" %% (n, first >> 32, first & 0xffffffff)
    err = np.abs(got[..., :2].astype(np.float64) - cs["want"])
    tol = %(bar)r if dtype_name == "float64" else 0.5 * uc.f32_ulp(cs["want"]) + %(extra)r
    assert (err <= tol).all(), (dtype_name, err.max())
    ctx.close()
rec = uc.recording(uc.WAVE_RIG, 40, "float64")
bt = BatchTriangulator(rec["K"], rec["R"], rec["t"], synth.default_thresholds(), pout_max=1, out_dtype=np.float64, D=rec["D"])
out = bt.run_host(rec["kpts"], rec["n_persons"])
n, first = bt.ctx.debug_faults()
assert n == 0, "device-side bounds check failed %%d times; first: code %%d at line %%d" %% (n, first >> 32, first & 0xffffffff)
assert (out["count"] == 1).all() and np.abs(out["xyzs"][:, 0, :, :3] - rec["X"][:, 0]).max() < 1e-7
bt.close()
print("undistort debug-bounds ok")
'''


def test_debug_build_counts_no_fault():
    dbg = os.path.join(ROOT, "snowmocap_amd", "libsnowtri_dbg.so")
    assert os.path.exists(dbg), f"{dbg} is missing: `make -C snowmocap_amd/csrc debug`"
    env = dict(os.environ, SNOWTRI_LIB=dbg)
    code = DBG_CODE % {"root": ROOT, "tests": os.path.join(ROOT, "tests"), "bar": BAR_F64, "extra": F32_EXTRA}
    p = subprocess.run([sys.executable, "-c", code], env=env, capture_output=True, text=True, timeout=300)
    assert p.returncode == 0 and "undistort debug-bounds ok" in p.stdout, (p.stdout[-2000:] + p.stderr[-3000:])
