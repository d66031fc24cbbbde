"""Despiking on the GPU (snowtri_despike_joint_track, snowmocap_amd/csrc/snowtri_despike.hpp) against its NumPy restatement
snowmocap_amd.despike.despike_joint_track_reference: records EQUAL bit for bit, codes equal, around the ends of the array, the
kernel's tile edges and runs of missing records; the routes into the entry point and its argument checks; the debug-bounds build
in a child process; and TrackPipeline.run(despike=...)."""
import ctypes as ct
import os
import subprocess
import sys

import numpy as np
import pytest

import despike_cases as dc
from conftest import ROOT

pytestmark = pytest.mark.gpu

MARK, REPLACE = 0, 1
T_KINDS = ("1", "2", "3", "2h", "2h+1", "B-1", "B", "B+1", "4B-1", "4B", "4B+1", "4B+h")
LANES = (1, 63, 64, 65, 130)


def frames(kind, B, h):
    return {"1": 1, "2": 2, "3": 3, "2h": 2 * h, "2h+1": 2 * h + 1, "B-1": B - 1, "B": B, "B+1": B + 1, "4B-1": 4 * B - 1, "4B": 4 * B,
            "4B+1": 4 * B + 1, "4B+h": 4 * B + h}[kind]


def _cases():
    """60 of the 12 x 5 x 4 x 2 x 2 combinations: every (T, h) pair, and every m with every T, h, dtype and mode."""
    out = []
    for ti, kind in enumerate(T_KINDS):
        for h in (1, 2, 3, 4):
            i = 4 * ti + (h - 1)
            out.append((kind, LANES[(ti + h) % 5], h, ("float32", "float64")[(i // 2 + ti) % 2], (MARK, REPLACE)[(i + ti // 2) % 2]))
    for ti, kind in enumerate(T_KINDS):                                  # twelve more: the m each T has not met yet, large T first
        h = 1 + (ti + 2) % 4
        out.append((kind, LANES[(ti + 3) % 5], h, ("float64", "float32")[ti % 2], (REPLACE, MARK)[(ti // 2) % 2]))
    return out


CASES = _cases()


def test_the_cases_cover_the_grid():
    assert len(CASES) == 60 and len(set(CASES)) == 60
    assert {(k, h) for k, _, h, _, _ in CASES} == {(k, h) for k in T_KINDS for h in (1, 2, 3, 4)}
    assert {(m, h) for _, m, h, _, _ in CASES} == {(m, h) for m in LANES for h in (1, 2, 3, 4)}
    assert {(m, d, o) for _, m, _, d, o in CASES} == {(m, d, o) for m in LANES for d in ("float32", "float64") for o in (MARK, REPLACE)}
    assert {(h, d, o) for _, _, h, d, o in CASES} == {(h, d, o) for h in (1, 2, 3, 4) for d in ("float32", "float64") for o in (MARK, REPLACE)}
    for m in LANES:
        assert len({k for k, mm, _, _, _ in CASES if mm == m}) >= 8, m


@pytest.fixture(scope="module")
def api():
    import snowmocap_amd as sm
    from snowmocap_amd import _lib
    assert _lib.lib().snowtri_device_count() > 0, "these tests need the HIP device"
    return sm


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint32 if a.dtype == np.float32 else np.uint64)


def _gpu(x, h, tol, mode, codes=True, device=True, stream=None):
    """despike_joint_track on a NumPy array: through device tensors (asynchronous, then synchronised) or staged from the host."""
    import torch
    from snowmocap_amd.despike import despike_joint_track
    if not device:
        return despike_joint_track(None, x, h, tol, mode, codes=codes)
    out, cd = despike_joint_track(None, torch.from_numpy(np.array(x)).cuda(), h, tol, mode, codes=codes, stream=stream)
    torch.cuda.synchronize()
    return out.cpu().numpy(), (cd.cpu().numpy() if cd is not None else None)


def _assert_equal(got, codes, ref, ref_codes, what):
    assert got.dtype == ref.dtype and got.shape == ref.shape and codes.dtype == np.uint8 and codes.shape == ref_codes.shape
    bad = np.argwhere(codes != ref_codes)
    assert bad.size == 0, f"{what}: codes differ first at (frame, lane) {bad[0]}: {codes[tuple(bad[0])]} != {ref_codes[tuple(bad[0])]}"
    bad = np.argwhere(_bits(got) != _bits(ref))
    assert bad.size == 0, f"{what}: records differ first at (frame, lane, component) {bad[0]}"


# ---------------------------------------------------------------------------------------------------------------- 1
@pytest.mark.parametrize("kind,m,h,dtype,mode", CASES)
def test_equals_the_reference_bit_for_bit(api, kind, m, h, dtype, mode):
    from snowmocap_amd.despike import despike_block_frames, despike_joint_track_reference
    B = despike_block_frames()
    assert B >= 2 * 4 + 1 and B == dc.block_frames()
    T = frames(kind, B, h)
    for rot in (range(dc.N_PATTERNS) if m < dc.N_PATTERNS else (0,)):          # a single lane takes every pattern in turn
        e = dc.edge_track(T, m, dtype, h, rot)
        ref, ref_codes = despike_joint_track_reference(e["x"], h, e["tol"], mode)
        got, codes = _gpu(e["x"], h, e["tol"], mode)
        _assert_equal(got, codes, ref, ref_codes, f"T={T} rot={rot}")
        if T >= 4 * B - 1 and m >= dc.N_PATTERNS:
            assert set(np.unique(ref_codes).tolist()) == {0, 1, 2, 3}


@pytest.mark.parametrize("dtype", ["float32", "float64"])
def test_equals_the_reference_on_the_recipe(api, dtype):
    from snowmocap_amd.despike import despike_joint_track_reference
    x = dc.recipe_track()["x"].astype(dtype)
    for mode in (MARK, REPLACE):
        ref, ref_codes = despike_joint_track_reference(x, 3, 0.1, mode)
        got, codes = _gpu(x, 3, 0.1, mode)
        _assert_equal(got, codes, ref, ref_codes, f"recipe mode={mode}")
    assert (ref_codes == 1).sum() > 3000


@pytest.mark.parametrize("dtype", ["float32", "float64"])
def test_ties_and_infinite_tolerance(api, dtype):
    from snowmocap_amd.despike import despike_joint_track_reference
    x = dc.edge_track(131, 2 * dc.N_PATTERNS, dtype, 3)["x"]
    t = int(np.nonzero(x[:, 9, 0] == 13.0)[0][0])
    got, codes = _gpu(x, 3, 5.0, MARK)
    assert codes[t, 9] == 0 and codes[t, 10] == 1                                     # d2 == tol^2 is not a spike
    for tol in (np.nextafter(5.0, 0.0), 0.0, np.inf):
        ref, ref_codes = despike_joint_track_reference(x, 3, tol, REPLACE)
        got, codes = _gpu(x, 3, tol, REPLACE)
        _assert_equal(got, codes, ref, ref_codes, f"tol={tol}")
    assert not (codes == 1).any() and np.array_equal(_bits(got), _bits(x))            # tol = inf: the input, bit for bit
    got, codes = _gpu(x, 3, np.nextafter(5.0, 0.0), MARK)
    assert codes[t, 9] == 1


# ---------------------------------------------------------------------------------------------------------------- 2
@pytest.mark.parametrize("dtype", ["float32", "float64"])
def test_routes(api, dtype):
    import torch
    from snowmocap_amd.despike import despike_block_frames, despike_joint_track, despike_joint_track_reference
    B = despike_block_frames()
    h, T, m = 3, 2 * B + 3, 133
    e = dc.edge_track(T, m, dtype, h)
    x, tol = e["x"], e["tol"]
    for mode in (MARK, REPLACE):
        ref, ref_codes = despike_joint_track_reference(x, h, tol, mode)                          # one call over T frames: no state to split
        got, codes = _gpu(x, h, tol, mode)
        _assert_equal(got, codes, ref, ref_codes, "device")
        again, codes2 = _gpu(x, h, tol, mode)
        assert np.array_equal(_bits(got), _bits(again)) and np.array_equal(codes, codes2)        # two runs are identical
        no_codes, none = _gpu(x, h, tol, mode, codes=False)
        assert none is None and np.array_equal(_bits(no_codes), _bits(got))                      # codes = NULL: the same out
        hg, hc = _gpu(x, h, tol, mode, device=False)
        assert isinstance(hg, np.ndarray) and np.array_equal(_bits(hg), _bits(got)) and np.array_equal(hc, codes)   # SNOWTRI_HOST
        hg, hc = _gpu(x, h, tol, mode, device=False, codes=False)
        assert hc is None and np.array_equal(_bits(hg), _bits(got))
    side = torch.cuda.Stream()
    xd = torch.from_numpy(np.array(x)).cuda()
    torch.cuda.synchronize()
    with torch.cuda.stream(side):
        sg, sc = despike_joint_track(None, xd, h, tol, REPLACE)                                  # torch's current stream: `side`
    eg, ec = despike_joint_track(None, xd, h, tol, REPLACE, stream=side.cuda_stream)             # ... and given explicitly
    side.synchronize()
    assert side.cuda_stream != 0
    for a, b in ((sg, sc), (eg, ec)):
        assert np.array_equal(_bits(a.cpu().numpy()), _bits(got)) and np.array_equal(b.cpu().numpy(), codes)
    shaped, scodes = _gpu(x[:, :132].reshape(T, 4, 33, 4).copy(), h, tol, REPLACE)               # [T, P, kn, 4]
    assert shaped.shape == (T, 4, 33, 4) and scodes.shape == (T, 4, 33)
    assert np.array_equal(_bits(shaped).reshape(T, 132, 4), _bits(got[:, :132]))


# ---------------------------------------------------------------------------------------------------------------- 3
def test_bad_arguments_are_refused_on_the_host(api):
    import torch
    from snowmocap_amd import _lib
    from snowmocap_amd.despike import despike_joint_track
    ctx = _lib.scratch_context()
    L, hd = ctx.L, ctx.handle
    T, m = 5, 7
    x = np.random.default_rng(1).uniform(0.5, 1.0, (T, m, 4))
    out, cd = np.full((T, m, 4), 9.0), np.full((T, m), 9, dtype=np.uint8)

    def call(T=T, m=m, xp=_lib.ptr(x), dtype=_lib.F64, h=2, tol=0.1, mode=MARK, op=_lib.ptr(out), memspace=_lib.HOST):
        rc = L.snowtri_despike_joint_track(hd, T, m, xp, dtype, h, tol, mode, op, _lib.ptr(cd), memspace, None)
        return rc, L.snowtri_last_error().decode()

    assert call(tol=np.inf)[0] == _lib.OK and (cd == 0).all() and np.array_equal(out, x)          # +infinity is allowed
    x0 = x.copy()
    for kw, word in ((dict(h=0), "half_window"), (dict(h=5), "half_window"), (dict(h=-1), "half_window"), (dict(tol=-1e-300), "tol"),
                     (dict(tol=np.nan), "tol"), (dict(tol=-np.inf), "tol"), (dict(mode=2), "mode"), (dict(mode=-1), "mode"),
                     (dict(dtype=2), "dtype"), (dict(dtype=-1), "dtype"), (dict(memspace=2), "memspace"), (dict(T=-1), "T < 0"),
                     (dict(m=-1), "m < 0"), (dict(xp=None), "null"), (dict(op=None), "null"), (dict(op=_lib.ptr(x)), "overlap"),
                     (dict(op=ct.c_void_p(x.ctypes.data + 32)), "overlap"), (dict(op=ct.c_void_p(x.ctypes.data - 32)), "overlap"),
                     (dict(T=1 << 40, m=1 << 30), "2^58"), (dict(T=1 << 45, m=64), "2^31 - 1")):
        out[:], cd[:] = 9.0, 9
        rc, msg = call(**kw)
        assert rc == _lib.ERR_BAD_ARG and msg.startswith("snowtri_despike_joint_track") and word in msg, (kw, rc, msg)
        assert (out == 9.0).all() and (cd == 9).all() and np.array_equal(x, x0), kw
    out[:], cd[:] = 9.0, 9
    assert call(T=0)[0] == _lib.OK and call(m=0)[0] == _lib.OK and (out == 9.0).all() and (cd == 9).all()   # T == 0 touches nothing
    assert L.snowtri_despike_joint_track(None, T, m, _lib.ptr(x), _lib.F64, 2, 0.1, MARK, _lib.ptr(out), None, _lib.HOST, None) == _lib.ERR_BAD_ARG
    # device pointers: aligned to 16 bytes, distinct
    buf = torch.zeros(2 * T * m * 4 + 8, dtype=torch.float64, device="cuda")
    buf[:] = 9.0
    base = buf.data_ptr()
    assert base % 16 == 0
    nbytes = T * m * 32

    def dev_call(x_off, o_off, T=T):
        rc = L.snowtri_despike_joint_track(hd, T, m, ct.c_void_p(base + x_off), _lib.F64, 2, 0.1, MARK, ct.c_void_p(base + o_off), None,
                                           _lib.DEVICE, None)
        return rc, L.snowtri_last_error().decode()

    for x_off, o_off, word in ((8, nbytes + 16, "aligned"), (0, nbytes + 8, "aligned"), (0, 0, "overlap"), (0, nbytes - 16, "overlap"),
                               (nbytes - 16, 0, "overlap")):
        rc, msg = dev_call(x_off, o_off)
        assert rc == _lib.ERR_BAD_ARG and word in msg, (x_off, o_off, rc, msg)
    assert dev_call(0, 0, T=0)[0] == _lib.OK                                                      # T == 0: nothing is looked at
    torch.cuda.synchronize()
    assert (buf.cpu().numpy() == 9.0).all()                                                       # ... and nothing was written
    assert dev_call(0, nbytes)[0] == _lib.OK                                                      # back to back is not an overlap
    torch.cuda.synchronize()
    after = buf.cpu().numpy()
    assert (after[:2 * T * m * 4] == 9.0).all() and (after[2 * T * m * 4:] == 9.0).all()          # constant lanes: nothing is a spike
    # the Python layer turns them into exceptions
    for kw in (dict(half_window=0), dict(half_window=5), dict(tol=-1.0), dict(tol=np.nan), dict(mode=2)):
        with pytest.raises(ValueError):
            despike_joint_track(None, x, **kw)
    with pytest.raises(TypeError):
        despike_joint_track(None, torch.zeros((3, 2, 4), dtype=torch.float16, device="cuda"))
    with pytest.raises(ValueError):
        despike_joint_track(None, torch.zeros((3, 2, 8), dtype=torch.float32, device="cuda")[..., ::2])


# ---------------------------------------------------------------------------------------------------------------- 4
DBG_CODE = r'''
import sys, numpy as np
sys.path.insert(0, %(root)r)
sys.path.insert(0, %(tests)r)
import despike_cases as dc
from snowmocap_amd import _lib
from snowmocap_amd.despike import despike_block_frames, despike_joint_track, despike_joint_track_reference
assert _lib.LIB_PATH.endswith("libsnowtri_dbg.so") and "SNOWTRI_DEBUG_BOUNDS" in _lib.build_info()["variants"]
ctx = _lib.scratch_context()
assert ctx.debug_faults()[0] == 0
B = despike_block_frames()
ran = 0
for dtype, T, m, h, mode in (("float32", 1, 1, 1, 0), ("float64", 2, 65, 4, 1), ("float32", B - 1, 64, 2, 1), ("float64", B + 1, 65, 3, 0),
                             ("float32", 4 * B + 4, 130, 4, 0), ("float64", 4 * B + 1, 63, 1, 1), ("float64", 2 * B + 3, 133, 2, 0),
                             ("float32", 4 * B - 1, 70, 3, 1)):
    e = dc.edge_track(T, m, dtype, h)
    ref, ref_codes = despike_joint_track_reference(e["x"], h, e["tol"], mode)
    got, codes = despike_joint_track(ctx, e["x"], h, e["tol"], mode)
    n, first = ctx.debug_faults()
    assert n == 0, "device-side bounds check failed %%d times; first: code %%d at line %%d" %% (n, first >> 32, first & 0xffffffff)
    assert np.array_equal(got.view(np.uint8), ref.view(np.uint8)) and np.array_equal(codes, ref_codes), (dtype, T, m, h, mode)
    ran += 1
print("despike debug-bounds ok:", ran, "calls")
'''


def test_debug_bounds_on_the_edge_tracks():
    dbg = os.path.join(ROOT, "snowmocap_amd", "libsnowtri_dbg.so")
    assert os.path.exists(dbg), f"{dbg} is missing: `make -C snowmocap_amd/csrc debug`"
    env = dict(os.environ, SNOWTRI_LIB=dbg)
    p = subprocess.run([sys.executable, "-c", DBG_CODE % {"root": ROOT, "tests": os.path.join(ROOT, "tests")}], env=env, capture_output=True,
                       text=True, timeout=300)
    assert p.returncode == 0 and "despike debug-bounds ok" in p.stdout, (p.stdout[-2000:] + p.stderr[-3000:])


# ---------------------------------------------------------------------------------------------------------------- 5
SPOTS = ((30, 0, 40), (30, 0, 77), (31, 0, 77), (45, 1, 100), (1, 1, 5), (58, 0, 9))      # (frame, person, joint); joint 77: a run of two


def spike_scene():
    """ring_rig(8), 2 walkers, 60 frames, pixel sigma 1.0, every camera lists both persons (the pairwise multi-person route).  With
    eight views the pairwise method outvotes one wrong detection, so each joint of SPOTS is seen by two cameras only (the scores of
    the other six are below the keypoint threshold) and the detection of one of the two is shifted along the epipolar line of the
    other, to where a point 0.3 m further down that camera's ray projects: the two rays still meet, 0.3 m from the joint."""
    from snowmocap_amd import synth
    rng = np.random.default_rng(19)
    F, P, A, B = 60, 2, 0, 2
    K, R, t = synth.ring_rig(8)
    X, _ = synth.make_walkers(rng, F, P, 0.03)
    kpts, npers = synth.make_keypoints_visible(rng, K, R, t, X, None, pixel_sigma=1.0, permute_persons=False)
    prm = dict(synth.default_thresholds(), average_score_threshold=1.0, condense_distance_tol=0.3, condense_person_num_tol=10)
    for f, p, j in SPOTS:
        ray = X[f, p, j] - t[A]
        uv, _ = synth.project(K, R, t, X[f, p, j] + 0.3 * ray / np.linalg.norm(ray))
        others = ~np.isin(np.arange(8), (A, B))
        kpts[f, others, p, j, 2] = 0.5 * prm["keypoint_score_threshold"]
        kpts[f, B, p, j, :2] = uv[B]
    return dict(rig=(K, R, t), X=X, kpts=kpts, n_persons=npers, params=prm)


def _same_bytes(a, b):
    a, b = a.cpu().numpy(), b.cpu().numpy()
    return a.dtype == b.dtype and a.shape == b.shape and np.array_equal(np.ascontiguousarray(a).view(np.uint8), np.ascontiguousarray(b).view(np.uint8))


def test_pipeline_takes_out_a_wrong_joint(api):
    from snowmocap_amd.blender import CONTROL_POINT_NAMES
    from snowmocap_amd.despike import despike_joint_track_reference
    from snowmocap_amd.fill import fill_joint_track_reference
    sc = spike_scene()
    K, R, t = sc["rig"]
    X = sc["X"]
    cpi = int(sc["params"]["center_point_index"])
    smo = {n: [2.0, 0.75, 0.0] for n in CONTROL_POINT_NAMES}
    pipe = api.TrackPipeline(K, R, t, sc["params"], smo, n_persons_out=2)
    run = lambda **kw: pipe.run(sc["kpts"], sc["n_persons"], ragged="track", **kw)     # noqa: E731
    plain, none8 = run(fill_gaps=8), run(fill_gaps=8, despike=None)
    assert list(none8) == list(plain) and all(_same_bytes(none8[k], plain[k]) for k in plain)     # None: today's dict, bit for bit
    plain0, none0 = run(), run(despike=None)
    assert list(none0) == list(plain0) and all(_same_bytes(none0[k], plain0[k]) for k in plain0)
    on = {k: v.cpu().numpy() for k, v in run(fill_gaps=8, despike=(0.1, 3)).items()}
    rep = {k: v.cpu().numpy() for k, v in run(despike=(0.1, 3)).items()}
    off = {k: v.cpu().numpy() for k, v in plain.items()}
    pipe.close()
    assert set(on) == set(off) | {"spike_codes", "xyzs_despiked"} and set(rep) == set(plain0) | {"spike_codes", "xyzs_despiked"}
    assert np.array_equal(_bits(on["xyzs"]), _bits(off["xyzs"])) and (on["present"]).all()          # xyzs stays the triangulation
    slot = [int(np.linalg.norm(on["xyzs"][0, :, cpi, :3] - X[0, p, cpi][None, :], axis=1).argmin()) for p in range(2)]
    assert sorted(slot) == [0, 1]
    assert on["spike_codes"].dtype == np.uint8 and on["spike_codes"].shape == on["xyzs"].shape[:3]
    for f, p, j in SPOTS:
        s = slot[p]
        assert on["spike_codes"][f, s, j] == 1, (f, p, j)                                           # coded SPIKE
        assert (on["xyzs_despiked"][f, s, j] == 0).all() and on["fill"][f, s, j] == 1               # marked, then interpolated
        with_pass = np.linalg.norm(on["xyzs_filled"][f, s, j, :3] - X[f, p, j])
        without = np.linalg.norm(off["xyzs_filled"][f, s, j, :3] - X[f, p, j])
        print(f"frame {f} person {p} joint {j}: filled track {with_pass:.4f} m from the truth with despike, {without:.4f} m without")
        assert with_pass < 0.03 and without > 0.10
    assert (on["spike_codes"] == 1).mean() < 0.01
    # the pass ran on the arrays the fill is given, immediately before it: the references chained on the gathered sequence of a slot
    for s in range(2):
        d, c = despike_joint_track_reference(on["xyzs"][:, s], 3, 0.1, MARK)
        assert np.array_equal(c, on["spike_codes"][:, s]) and np.array_equal(_bits(d), _bits(on["xyzs_despiked"][:, s]))
        fl, fc = fill_joint_track_reference(d, 8)
        assert np.array_equal(fc, on["fill"][:, s]) and np.array_equal(_bits(fl), _bits(on["xyzs_filled"][:, s]))
    assert not np.array_equal(on["smoothed"], off["smoothed"])
    # fill_gaps = 0: REPLACE -- the same verdicts, and no zero record where the input had none
    assert np.array_equal(rep["spike_codes"], on["spike_codes"])
    assert np.array_equal(rep["xyzs_despiked"][..., 3] == 0, rep["xyzs"][..., 3] == 0)
    for f, p, j in SPOTS:
        s = slot[p]
        assert np.array_equal(_bits(rep["xyzs_despiked"][f, s, j, 3:]), _bits(rep["xyzs"][f, s, j, 3:]))
        assert np.linalg.norm(rep["xyzs_despiked"][f, s, j, :3] - X[f, p, j]) < 0.1 < np.linalg.norm(rep["xyzs"][f, s, j, :3] - X[f, p, j])
    for s in range(2):
        d, c = despike_joint_track_reference(rep["xyzs"][:, s], 3, 0.1, REPLACE)
        assert np.array_equal(_bits(d), _bits(rep["xyzs_despiked"][:, s]))


def test_pipeline_with_fixed_slots(api):
    """The whole-array branch (every slot in every frame): the floor rig's 4 cameras, one walker, 64 frames; the detections of
    joint 40 in frames 20-21 are moved in ALL cameras to where a point 0.245 m from the joint projects."""
    import torch
    from snowmocap_amd import synth
    from snowmocap_amd.blender import CONTROL_POINT_NAMES
    from snowmocap_amd.despike import despike_joint_track_reference
    from snowmocap_amd.fill import fill_joint_track_reference
    rng = np.random.default_rng(23)
    K, R, t = synth.load_rig_json()
    X, _ = synth.make_walkers(rng, 64, 1, step=0.03)
    kpts, npers = synth.make_keypoints(rng, K, R, t, X, pixel_sigma=1.0, score_range=(3.5, 8.0))
    for f in (20, 21):
        uv, _ = synth.project(K, R, t, X[f, 0, 40] + np.array([0.2, -0.1, 0.1]))
        kpts[f, :, 0, 40, :2] = uv
    thr = synth.default_thresholds()
    smo = {n: [2.0, 0.75, 0.0] for n in CONTROL_POINT_NAMES}
    pipe = api.TrackPipeline(K, R, t, thr, smo, n_persons_out=1)
    plain = pipe.run(kpts, npers, fill_gaps=8)
    same = pipe.run(kpts, npers, fill_gaps=8, despike=None)
    on = pipe.run(kpts, npers, fill_gaps=8, despike=(0.1, 3))
    rep = pipe.run(kpts, npers, despike=(0.1, 3))
    torch.cuda.synchronize()
    assert list(same) == list(plain) and all(_same_bytes(same[k], plain[k]) for k in plain)
    assert set(on) == set(plain) | {"spike_codes", "xyzs_despiked"} and (on["tracked"] == 1).all()
    x = on["xyzs"].cpu().numpy()
    assert np.linalg.norm(x[20:22, 0, 40, :3] - X[20:22, 0, 40], axis=1).min() > 0.2
    d, c = despike_joint_track_reference(x, 3, 0.1, MARK)
    assert (c[20:22, 0, 40] == 1).all() and np.array_equal(on["spike_codes"].cpu().numpy(), c)
    assert np.array_equal(_bits(on["xyzs_despiked"].cpu().numpy()), _bits(d))
    fl, fc = fill_joint_track_reference(d, 8)
    assert np.array_equal(on["fill"].cpu().numpy(), fc) and np.array_equal(_bits(on["xyzs_filled"].cpu().numpy()), _bits(fl))
    assert np.linalg.norm(fl[20:22, 0, 40, :3] - X[20:22, 0, 40], axis=1).max() < 0.03
    d, c = despike_joint_track_reference(x, 3, 0.1, REPLACE)
    assert np.array_equal(_bits(rep["xyzs_despiked"].cpu().numpy()), _bits(d)) and "fill" not in rep
    for bad in ((0.1, 5), 0.1, (-1.0, 3)):
        with pytest.raises(ValueError):
            pipe.run(kpts, npers, despike=bad)
    pipe.close()
