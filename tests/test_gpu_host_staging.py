"""SNOWTRI_HOST against SNOWTRI_DEVICE for the entry points that stage host arrays through the context's device scratch
(snowmocap_amd/csrc/snowtri.hip: ctx->in, ctx->out).  A host call uploads its arrays, runs the kernels of the device call on the
staged copies, and downloads the outputs, so every output has to come back bit for bit as the device call leaves it: with an
optional array absent, across a regrowth of the scratch (it starts at 1 MiB and is freed and reallocated beyond that), and for
an array that is both read and written; and, for the per-frame and fused calls, on each of the routes the staging helper chooses by
the call's byte totals (section 5).  No tolerance anywhere: both sides are the same kernels on the same values.

Every output buffer starts as 0xA5 bytes on both routes, so a byte neither route writes compares equal and a byte only one of them
writes does not.  Only the production library is loaded.
"""
import ctypes as ct

import numpy as np
import pytest

import undistort_cases as uc
from snowmocap_amd import _lib

pytestmark = pytest.mark.gpu

FZRD = (1.7, 0.6, -0.4, 1.0 / 30.0)            # f, z, r, dt of the uniform filters
KN = 20                                        # joints per person outside the blender entries
KN_BLENDER = 130                               # snowtri_blender_points reads joint 129
POINTS = 24                                    # blender points per person


class Host:
    code = _lib.HOST

    @staticmethod
    def put(a):
        return None if a is None else np.array(a, copy=True, order="C")

    @staticmethod
    def out(shape, dtype):
        return np.full(int(np.prod(shape)) * np.dtype(dtype).itemsize, 0xA5, dtype=np.uint8).view(dtype).reshape(shape)

    @staticmethod
    def ptr(a):
        return _lib.ptr(a)

    @staticmethod
    def get(a):
        return a


class Device:
    code = _lib.DEVICE

    @staticmethod
    def put(a):
        import torch
        return None if a is None else torch.from_numpy(np.array(a, copy=True, order="C")).cuda()

    @staticmethod
    def out(shape, dtype):
        import torch
        return torch.from_numpy(Host.out(shape, dtype)).cuda()

    @staticmethod
    def ptr(a):
        return None if a is None else ct.c_void_p(a.data_ptr())

    @staticmethod
    def get(a):
        import torch
        torch.cuda.synchronize()
        return a.cpu().numpy()


def _same(got, want, what):
    assert len(got) == len(want), what
    for i, (g, w) in enumerate(zip(got, want)):
        assert (g is None) == (w is None), f"{what}: output {i}"
        if g is None:
            continue
        assert g.dtype == w.dtype and g.shape == w.shape, f"{what}: output {i}"
        gb, wb = np.ascontiguousarray(g).view(np.uint8), np.ascontiguousarray(w).view(np.uint8)
        assert np.array_equal(gb, wb), f"{what}: output {i} differs in {int((gb != wb).sum())} of {gb.size} bytes"


def _ok(rc, where):
    assert rc == _lib.OK, f"{where}: status {rc} [{_lib.lib().snowtri_last_error().decode()}]"


# ------------------------------------------------------------------------------------------------ the calls
# Each takes the context, the route (Host or Device), NumPy inputs, and returns its outputs as NumPy arrays (None: not asked for).
def smooth_track(ctx, M, x, joint=False):
    T = x.shape[0]
    n = x[0].size // (4 if joint else 1)
    dx, dy = M.put(x), M.out(x.shape, np.float64)
    fn = ctx.L.snowtri_smooth_joint_track if joint else ctx.L.snowtri_smooth_track
    _ok(fn(ctx.handle, T, n, M.ptr(dx), *FZRD, M.ptr(dy), M.code, None), "smooth track")
    return (M.get(dy),)


def shard_local(ctx, M, x, first, end_state=True):
    T, n = x.shape
    dx, dy = M.put(x), M.out(x.shape, np.float64)
    de = M.out((2 * n,), np.float64) if end_state else None
    _ok(ctx.L.snowtri_smooth_shard_local(ctx.handle, T, n, M.ptr(dx), first, *FZRD, M.ptr(dy), M.ptr(de), M.code, None),
        "snowtri_smooth_shard_local")
    return M.get(dy), (M.get(de) if end_state else None)


def shard_fix(ctx, M, y, start, first):
    T, n = y.shape
    dy, ds = M.put(y), M.put(start)
    _ok(ctx.L.snowtri_smooth_shard_fix(ctx.handle, T, n, first, M.ptr(ds), *FZRD, M.ptr(dy), M.code, None), "snowtri_smooth_shard_fix")
    return (M.get(dy),)


def shard_combine(ctx, M, gathered, rank):
    world, n = gathered.shape[0], (gathered.shape[1] - 1) // 4
    dg, ds = M.put(gathered), M.out((2 * n,), np.float64)
    _ok(ctx.L.snowtri_smooth_shard_combine(ctx.handle, world, rank, n, M.ptr(dg), *FZRD, M.ptr(ds), M.code, None),
        "snowtri_smooth_shard_combine")
    return (M.get(ds),)


def undistort(ctx, M, kpts):
    F, C, Pmax, J, _ = kpts.shape
    di, do = M.put(kpts), M.out(kpts.shape, kpts.dtype)
    _ok(ctx.L.snowtri_undistort_keypoints(ctx.handle, F, Pmax, J, M.ptr(di), M.ptr(do), _lib.dtype_code(kpts.dtype), M.code, None),
        "snowtri_undistort_keypoints")
    return (M.get(do),)


def blender_points(ctx, M, xyzs):
    n, kn = xyzs.shape[0], xyzs.shape[1]
    dx, dp, dv = M.put(xyzs), M.out((n, POINTS, 4), np.float64), M.out((n, POINTS), np.uint8)
    _ok(ctx.L.snowtri_blender_points(ctx.handle, n, kn, M.ptr(dx), _lib.dtype_code(xyzs.dtype), M.ptr(dp), M.ptr(dv), M.code, None),
        "snowtri_blender_points")
    return M.get(dp), M.get(dv)


def blender_smooth(ctx, M, points, valid, fzr):
    T, persons = points.shape[:2]
    dp, dv, do = M.put(points), M.put(valid), M.out(points.shape, np.float64)
    _ok(ctx.L.snowtri_blender_smooth(ctx.handle, T, persons, M.ptr(dp), M.ptr(dv), _lib.ptr(fzr), FZRD[3], M.ptr(do), M.code, None),
        "snowtri_blender_smooth")
    return (M.get(do),)


def track_persons(ctx, M, xyzs, count, S, state, flags=True):
    F, P, kn = xyzs.shape[:3]
    dx, dc, dst = M.put(xyzs), M.put(count), M.put(state)
    so, po, ti = M.out((F, P), np.int32), M.out((F, S), np.int32), M.out((F, S), np.int32)
    fl = M.out((F,), np.uint32) if flags else None
    _ok(ctx.L.snowtri_track_persons(ctx.handle, F, P, kn, M.ptr(dx), _lib.dtype_code(xyzs.dtype), M.ptr(dc), S, 3, 0.35, 2, M.ptr(dst),
                                    M.ptr(so), M.ptr(po), M.ptr(ti), M.ptr(fl), M.code, None), "snowtri_track_persons")
    return M.get(so), M.get(po), M.get(ti), (M.get(fl) if flags else None), (M.get(dst) if state is not None else None)


def track_gather(ctx, M, xyzs, person_of):
    F, P, kn = xyzs.shape[:3]
    S = person_of.shape[1]
    dx, dpo, do = M.put(xyzs), M.put(person_of), M.out((F, S, kn, 4), xyzs.dtype)
    _ok(ctx.L.snowtri_track_gather(ctx.handle, F, P, kn, M.ptr(dx), _lib.dtype_code(xyzs.dtype), S, M.ptr(dpo), M.ptr(do), M.code, None),
        "snowtri_track_gather")
    return (M.get(do),)


def record_pass(ctx, M, which, xyzs, codes=True):
    T, m = xyzs.shape[0], xyzs.shape[1] * xyzs.shape[2]
    dx, do = M.put(xyzs), M.out(xyzs.shape, xyzs.dtype)
    dc = M.out((T, m), np.uint8) if codes else None
    code = _lib.dtype_code(xyzs.dtype)
    if which == "fill":
        rc = ctx.L.snowtri_fill_joint_track(ctx.handle, T, m, M.ptr(dx), code, 5, M.ptr(do), M.ptr(dc), M.code, None)
    else:
        rc = ctx.L.snowtri_despike_joint_track(ctx.handle, T, m, M.ptr(dx), code, 2, 0.05, _lib.DESPIKE_REPLACE, M.ptr(do), M.ptr(dc), M.code, None)
    _ok(rc, which)
    return M.get(do), (M.get(dc) if codes else None)


def reproject(ctx, M, xyzs, pix_dtype, raw):
    F, P, kn = xyzs.shape[:3]
    dx, dp = M.put(xyzs), M.out((F, ctx.C, P, kn, 3), pix_dtype)
    _ok(ctx.L.snowtri_reproject(ctx.handle, F, P, kn, M.ptr(dx), _lib.dtype_code(xyzs.dtype), _lib.REPROJECT_RAW if raw else 0, M.ptr(dp),
                                _lib.dtype_code(pix_dtype), M.code, None), "snowtri_reproject")
    return (M.get(dp),)


def reproject_cost(ctx, M, xyzs, kpts, n_persons):
    F, P, kn = xyzs.shape[:3]
    Pmax = kpts.shape[2]
    dx, dk, dn = M.put(xyzs), M.put(kpts), M.put(n_persons)
    cs, cn = M.out((F, ctx.C, P, Pmax), np.float64), M.out((F, ctx.C, P, Pmax), np.int32)
    _ok(ctx.L.snowtri_reproject_cost(ctx.handle, F, P, kn, M.ptr(dx), _lib.dtype_code(xyzs.dtype), Pmax, M.ptr(dk), _lib.dtype_code(kpts.dtype),
                                     M.ptr(dn), 0.3, 0, M.ptr(cs), M.ptr(cn), M.code, None), "snowtri_reproject_cost")
    return M.get(cs), M.get(cn)


# ------------------------------------------------------------------------------------------------ inputs
@pytest.fixture(scope="module")
def rig():
    assert _lib.lib().snowtri_device_count() > 0, "these tests need the HIP device"
    assert _lib.build_info()["variants"] == [], "the production library only"
    K, R, t, D, _ = uc.rig("floor")
    return K, R, t, D


@pytest.fixture
def ctx(rig):
    K, R, t, D = rig
    c = _lib.Context(K, R, t)                  # fresh: its staging scratch has never been sized
    c.set_distortion(D)
    yield c
    c.close()


def _records(seed, shape, dtype=np.float64):
    """Joint records [..., 4] around the origin of the rig; some missing (score 0, the all-zero record, a NaN with a payload)."""
    rng = np.random.default_rng(seed)
    x = rng.uniform(-1.0, 1.0, size=shape + (4,))
    x[..., 2] = rng.uniform(0.2, 1.8, size=shape)
    x[..., 3] = rng.uniform(0.35, 1.0, size=shape)
    flat = x.reshape(-1, 4)
    flat[5::17, 3] = 0.0
    flat[7::29] = 0.0
    x = x.astype(dtype)
    nan = x.reshape(-1, 4)[11::31, 1].view({4: np.uint32, 8: np.uint64}[x.dtype.itemsize])
    nan[:] = {4: 0x7FC01234, 8: 0x7FF8000000001234}[x.dtype.itemsize]
    return x


def _track(seed, T, n):
    rng = np.random.default_rng(seed)
    return np.cumsum(rng.normal(0.0, 0.02, size=(T, n)), axis=0)


def _keypoints(seed, F, C, Pmax, J, dtype):
    rng = np.random.default_rng(seed)
    k = np.empty((F, C, Pmax, J, 3))
    k[..., 0] = rng.uniform(uc.BOX[0][0], uc.BOX[0][1], size=k.shape[:-1])
    k[..., 1] = rng.uniform(uc.BOX[1][0], uc.BOX[1][1], size=k.shape[:-1])
    k[..., 2] = rng.uniform(0.0, 1.0, size=k.shape[:-1])
    return k.astype(dtype)


def _people(seed, F, P, kn, dtype):
    """[F, P, kn, 4] persons that drift slowly, so that the tracker matches, loses and re-creates them, and their count [F]."""
    rng = np.random.default_rng(seed)
    base = rng.uniform(-1.0, 1.0, size=(1, P, 1, 3)) + np.cumsum(rng.normal(0.0, 0.03, size=(F, P, 1, 3)), axis=0)
    x = np.empty((F, P, kn, 4))
    x[..., :3] = base + rng.normal(0.0, 0.1, size=(F, P, kn, 3))
    x[..., 3] = rng.uniform(0.4, 1.0, size=(F, P, kn))
    x[9:12, 1, 3] = 0.0                        # a centre joint that drops out for three frames
    count = rng.integers(1, P + 1, size=F).astype(np.int32)
    return x.astype(dtype), count


def _fzr():
    rng = np.random.default_rng(5)
    fzr = np.empty((POINTS, 3))
    fzr[:, 0] = rng.uniform(0.8, 3.0, POINTS)
    fzr[:, 1] = rng.uniform(0.3, 1.0, POINTS)
    fzr[:, 2] = rng.uniform(-1.0, 1.0, POINTS)
    return np.ascontiguousarray(fzr)


def _gathered(seed, world, n):
    rng = np.random.default_rng(seed)
    g = rng.normal(0.0, 1.0, size=(world, 4 * n + 1))
    g[:, -1] = [37.0, 0.0, 41.0, 40.0][:world]   # shard lengths; the second shard is empty
    return g


# ------------------------------------------------------------------------------------------------ 1. HOST equals DEVICE
def test_smoothing_entries_host_equals_device(ctx):
    x = _track(1, 41, 3 * KN * 4)
    for joint in (False, True):
        xs = x.reshape(41, 3 * KN, 4) if joint else x
        _same(smooth_track(ctx, Host, xs, joint), smooth_track(ctx, Device, xs, joint), f"smooth track, joint records {joint}")
    for first in (1, 0):
        _same(shard_local(ctx, Host, x, first), shard_local(ctx, Device, x, first), f"snowtri_smooth_shard_local first={first}")
    g = _gathered(2, 4, x.shape[1])
    for rank in (0, 2, 3):
        _same(shard_combine(ctx, Host, g, rank), shard_combine(ctx, Device, g, rank), f"snowtri_smooth_shard_combine rank {rank}")


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
def test_undistort_host_equals_device(ctx, dtype):
    k = _keypoints(3, 40, ctx.C, 3, KN, dtype)
    _same(undistort(ctx, Host, k), undistort(ctx, Device, k), "snowtri_undistort_keypoints")


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
def test_blender_entries_host_equals_device(ctx, dtype):
    T, persons = 40, 3
    xyzs = _records(4, (T * persons, KN_BLENDER), dtype)
    host = blender_points(ctx, Host, xyzs)
    _same(host, blender_points(ctx, Device, xyzs), "snowtri_blender_points")
    points, valid = host[0].reshape(T, persons, POINTS, 4), host[1].reshape(T, persons, POINTS)
    assert 0 < valid.sum() < valid.size, "the hold needs both kinds of point"
    _same(blender_smooth(ctx, Host, points, valid, _fzr()), blender_smooth(ctx, Device, points, valid, _fzr()), "snowtri_blender_smooth")


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
def test_tracking_entries_host_equals_device(ctx, dtype):
    F, P, S = 40, 3, 3
    xyzs, count = _people(6, F, P, KN, dtype)
    state = np.zeros(int(ctx.L.snowtri_track_state_bytes(S)), dtype=np.uint8)
    host = track_persons(ctx, Host, xyzs, count, S, state)
    _same(host, track_persons(ctx, Device, xyzs, count, S, state), "snowtri_track_persons")
    assert (host[1] >= 0).any() and host[4].any(), "somebody is tracked and the state has moved"
    # the next block of frames continues from the state the first one left
    _same(track_persons(ctx, Host, xyzs[::-1], count[::-1], S, host[4]), track_persons(ctx, Device, xyzs[::-1], count[::-1], S, host[4]),
          "snowtri_track_persons from a saved state")
    _same(track_gather(ctx, Host, xyzs, host[1]), track_gather(ctx, Device, xyzs, host[1]), "snowtri_track_gather")


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
@pytest.mark.parametrize("which", ["fill", "despike"])
def test_record_passes_host_equal_device(ctx, which, dtype):
    xyzs = _records(7, (41, 3, KN), dtype)
    _same(record_pass(ctx, Host, which, xyzs), record_pass(ctx, Device, which, xyzs), which)


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
def test_reprojection_entries_host_equal_device(ctx, dtype):
    F, P, Pmax = 40, 3, 3
    xyzs = _records(8, (F, P, KN), dtype)
    for pix_dtype in (np.float64, np.float32):
        for raw in (False, True):
            _same(reproject(ctx, Host, xyzs, pix_dtype, raw), reproject(ctx, Device, xyzs, pix_dtype, raw), f"snowtri_reproject raw={raw}")
    n_persons = np.random.default_rng(9).integers(0, Pmax + 1, size=(F, ctx.C)).astype(np.int32)
    for kdt in (np.float64, np.float32):
        kpts = _keypoints(10, F, ctx.C, Pmax, KN, kdt)
        _same(reproject_cost(ctx, Host, xyzs, kpts, n_persons), reproject_cost(ctx, Device, xyzs, kpts, n_persons), "snowtri_reproject_cost")


# ------------------------------------------------------------------------------------------------ 2. optional arrays
def test_an_absent_optional_array_changes_no_other_output(ctx):
    xyzs = _records(11, (41, 3, KN))
    for which in ("fill", "despike"):
        full = record_pass(ctx, Host, which, xyzs)
        _same(record_pass(ctx, Host, which, xyzs, codes=False), (full[0], None), f"{which} without its codes")

    F, P, S = 40, 3, 3
    people, count = _people(12, F, P, KN, np.float64)
    state = np.zeros(int(ctx.L.snowtri_track_state_bytes(S)), dtype=np.uint8)
    full = track_persons(ctx, Host, people, count, S, state)
    _same(track_persons(ctx, Host, people, count, S, state, flags=False), full[:3] + (None, full[4]), "snowtri_track_persons without flags")
    # no state is a fresh start that is not saved: the all-zero state's outputs
    _same(track_persons(ctx, Host, people, count, S, None), full[:4] + (None,), "snowtri_track_persons without state")
    _same(track_persons(ctx, Host, people, count, S, None, flags=False), full[:3] + (None, None), "snowtri_track_persons without flags and state")

    Pmax = 3
    kpts = _keypoints(13, F, ctx.C, Pmax, KN, np.float64)
    everyone = np.full((F, ctx.C), Pmax, dtype=np.int32)   # what an absent n_persons stands for
    _same(reproject_cost(ctx, Host, xyzs[:F], kpts, None), reproject_cost(ctx, Host, xyzs[:F], kpts, everyone), "snowtri_reproject_cost without n_persons")
    _same(reproject_cost(ctx, Host, xyzs[:F], kpts, None), reproject_cost(ctx, Device, xyzs[:F], kpts, None), "snowtri_reproject_cost without n_persons")

    x = _track(14, 41, 3 * KN * 4)
    full = shard_local(ctx, Host, x, 0)
    _same(shard_local(ctx, Host, x, 0, end_state=False), (full[0], None), "snowtri_smooth_shard_local without end_state")


# ------------------------------------------------------------------------------------------------ 3. regrowth of the scratch
def test_staging_survives_a_regrowth_of_the_scratch_one_array_each_way(ctx):
    small, large = _track(15, 40, 240), _track(16, 640, 256)
    assert small.nbytes < (1 << 20) < large.nbytes          # 75 KiB, then 1.25 MiB in ctx->in and in ctx->out
    want = {id(a): smooth_track(ctx, Device, a) for a in (small, large)}   # (device calls leave the staging scratch alone)
    for step, a in enumerate((small, large, small)):
        _same(smooth_track(ctx, Host, a), want[id(a)], f"snowtri_smooth_track, call {step + 1} of small / large / small")


def test_staging_survives_a_regrowth_of_the_scratch_several_arrays(ctx):
    def inputs(seed, F, C, P, kn):
        return (_records(seed, (F, P, kn)), _keypoints(seed + 1, F, C, P, kn, np.float64),
                np.random.default_rng(seed + 2).integers(0, P + 1, size=(F, C)).astype(np.int32))
    small, large = inputs(17, 8, ctx.C, 2, KN), inputs(20, 64, ctx.C, 4, 64)
    assert small[1].nbytes < (1 << 20) < large[1].nbytes    # kpts alone: 1.5 MiB; the costs are 48 KiB, so only ctx->in regrows here
    want = {id(a): reproject_cost(ctx, Device, *a) for a in (small, large)}
    for step, a in enumerate((small, large, small)):
        _same(reproject_cost(ctx, Host, *a), want[id(a)], f"snowtri_reproject_cost, call {step + 1} of small / large / small")


# ------------------------------------------------------------------------------------------------ 4. an array read and written
def test_shard_fix_reads_and_writes_y_through_the_staging(ctx):
    x = _track(23, 41, 3 * KN * 4)
    start = np.random.default_rng(24).normal(0.0, 0.5, size=2 * x.shape[1])
    for first in (0, 1):
        y_host, _ = shard_local(ctx, Host, x, first)
        y_dev, _ = shard_local(ctx, Device, x, first)
        _same((y_host,), (y_dev,), "snowtri_smooth_shard_local")
        fixed = shard_fix(ctx, Host, y_host, start, first)
        _same(fixed, shard_fix(ctx, Device, y_dev, start, first), f"snowtri_smooth_shard_fix first={first}")
        assert not np.array_equal(fixed[0], y_host), "the fix has changed y"


# ------------------------------------------------------------------------------------------------ 5. the per-frame and fused calls
# snowtri_triangulate, snowtri_condense, snowtri_condense_resident and the fused call choose how a host call's arrays travel from
# its byte totals (snowtri.hip): one copy per array above kPinnedMaxBytes in either direction ("direct"), one page-locked block each
# way up to that ("page-locked"), and -- snowtri_triangulate and snowtri_condense_resident only -- kernels that read and write mapped
# page-locked memory while inputs plus outputs stay within kZeroCopyMaxBytes ("mapped").  Each case states the totals it computes
# and the route it means to reach; the library's own totals differ by the padding between arrays, tens of bytes.  (The one-launch
# kernel of the mapped snowtri_triangulate is not the device call's pair of kernels, but takes a slot's mean in their order: same bits.)
PINNED_MAX = 4 << 20                           # kPinnedMaxBytes
MAPPED_MAX = 256 << 10                         # kZeroCopyMaxBytes
JF = 16                                        # joints = keypoint_num of the per-frame cases


def _route(in_bytes, out_bytes, mapped):
    if max(in_bytes, out_bytes) > PINNED_MAX:
        return "direct"
    return "mapped" if mapped and in_bytes + out_bytes <= MAPPED_MAX else "page-locked"


def _twin_rig(C):
    """The first C cameras of a ring of three whose camera 1 is camera 0 moved sideways: the same K and R, another centre, so that equal
    pixels in the two are parallel rays bit for bit (a singular pair as snowtri_triangulate counts them)."""
    from snowmocap_amd import synth
    K, R, t = (a.copy() for a in synth.ring_rig(3))
    K[1], R[1] = K[0], R[0]
    t[1] = t[0] + R[0] @ np.array([0.4, 0.1, 0.0])
    return K[:C], R[:C], t[:C]


def _frames(seed, C, F, Pmax, J):
    """float32 keypoints [F, C, Pmax, J, 3] and n_persons [F, C]; every fifth frame the last camera has a person fewer than Pmax."""
    from snowmocap_amd import synth
    rng = np.random.default_rng(seed)
    kpts, n_persons = synth.make_keypoints(rng, *_twin_rig(C), synth.make_people(rng, F, Pmax, J=J), pixel_sigma=0.8)
    n_persons[2::5, C - 1] = Pmax - 1
    return kpts, n_persons


def _with_parallel_rays(kpts):
    """One joint of the second frame (the only one of a single frame) at the same pixel in cameras 0 and 1."""
    bad = kpts.copy()
    f, j = min(1, bad.shape[0] - 1), bad.shape[3] // 2
    bad[f, 0, 0, j, :2] = bad[f, 1, 0, j, :2]
    return bad


def _params(**over):
    from snowmocap_amd import synth
    return _lib.make_params(**dict(synth.default_thresholds(), keypoint_num=JF, center_point_index=0, **over))


APART = dict(condense_distance_tol=1e-9)       # no two candidates merge: three candidates of a frame are two persons (the last never seeds)


class frame_ctx:
    def __init__(self, C):
        self.C = C

    def __enter__(self):
        assert _lib.lib().snowtri_device_count() > 0, "these tests need the HIP device"
        assert _lib.build_info()["variants"] == [], "the production library only"
        self.ctx = _lib.Context(*_twin_rig(self.C))
        return self.ctx

    def __exit__(self, *exc):
        self.ctx.close()


def triangulate(ctx, M, kpts, n_persons, prm, status=_lib.OK):
    F, C, Pmax, J, _ = kpts.shape
    Kc = int(ctx.L.snowtri_num_candidate_slots(C, Pmax))
    # the host call defines the slots nobody fills as zeros; the device call leaves them alone, so it starts from zeros
    fresh = M.out if M is Host else (lambda shape, dtype: M.put(np.zeros(shape, dtype)))
    dk, dn = M.put(kpts), M.put(n_persons)
    o = fresh((F, Kc, J, 3), np.float64), fresh((F, Kc, J), np.float64), fresh((F, Kc), np.float64), fresh((F, Kc), np.uint8)
    rc = ctx.L.snowtri_triangulate(ctx.handle, F, Pmax, J, M.ptr(dk), _lib.dtype_code(kpts.dtype), M.ptr(dn), prm,
                                   *(M.ptr(a) for a in o), M.code, None)
    assert rc == status, f"snowtri_triangulate: status {rc}, not {status} [{_lib.lib().snowtri_last_error().decode()}]"
    return tuple(M.get(a) for a in o)


def _condensed(M, F, Pout, flags):
    return (M.out((F, Pout, JF, 3), np.float64), M.out((F, Pout, JF), np.float64), M.out((F, Pout), np.float64), M.out((F,), np.int32),
            M.out((F,), np.uint32) if flags else None)


def condense(ctx, M, cand, prm, Pout, keep=True, flags=True, status=_lib.OK):
    xyz, ks, _, kept = cand
    F, N, J = ks.shape
    dx, dk, dkeep = M.put(xyz), M.put(ks), M.put(kept if keep else None)
    o = _condensed(M, F, Pout, flags)
    rc = ctx.L.snowtri_condense(ctx.handle, F, N, J, M.ptr(dx), M.ptr(dk), M.ptr(dkeep), prm, Pout, *(M.ptr(a) for a in o), M.code, None)
    assert rc == status, f"snowtri_condense: status {rc}, not {status}"
    return tuple(None if a is None else M.get(a) for a in o)


def condense_resident(ctx, F, prm, Pout, flags=True, status=_lib.OK):
    o = _condensed(Host, F, Pout, flags)
    token = int(ctx.L.snowtri_candidates_token(ctx.handle))
    assert token != 0, "the host call has left its candidates on the device"
    rc = ctx.L.snowtri_condense_resident(ctx.handle, token, prm, Pout, *(Host.ptr(a) for a in o))
    assert rc == status, f"snowtri_condense_resident: status {rc}, not {status}"
    return o


def fused(ctx, M, kpts, n_persons, prm, Pout, out_dtype, pscore=True, flags=True, robust=False, diagnostics=False):
    """-> status, snowtri_last_slow_frames, (xyzs, pscore, count, flags, views, resid)"""
    F, C, Pmax, J, _ = kpts.shape
    dk, dn = M.put(kpts), M.put(n_persons)
    o = (M.out((F, Pout, JF, 4), out_dtype), M.out((F, Pout), out_dtype) if pscore else None, M.out((F,), np.int32),
         M.out((F,), np.uint32) if flags else None,
         M.out((F, JF), np.uint32) if diagnostics else None, M.out((F, JF), out_dtype) if diagnostics else None)
    p = [M.ptr(a) for a in o]
    codes = _lib.dtype_code(kpts.dtype), _lib.dtype_code(out_dtype)
    if robust:
        rc = ctx.L.snowtri_triangulate_robust(ctx.handle, F, J, M.ptr(dk), codes[0], M.ptr(dn), prm, 6.0, 1, Pout, p[0], p[1], codes[1], p[2], p[3],
                                              p[4], p[5], M.code, None)
    else:
        assert not diagnostics
        rc = ctx.L.snowtri_triangulate_condense(ctx.handle, F, Pmax, J, M.ptr(dk), codes[0], M.ptr(dn), prm, _lib.PAIRWISE, Pout, p[0], p[1], codes[1],
                                                p[2], p[3], M.code, None)
    return rc, ctx.last_slow_frames(), tuple(None if a is None else M.get(a) for a in o)


def _status_of(flags):
    any_ = int(np.bitwise_or.reduce(flags))
    return _lib.ERR_SINGULAR if any_ & _lib.FLAG_SINGULAR else _lib.ERR_OVERFLOW if any_ & _lib.FLAG_OVERFLOW else _lib.OK


def _triangulate_bytes(C, Pmax, J, F):
    Kc = C * (C - 1) // 2 * Pmax * Pmax
    return F * (C * Pmax * J * 3 * 4 + C * 4), F * Kc * (J * 4 * 8 + 8 + 1) + 8      # keypoints + n_persons | xyz, kscore, pscore, keep + the counter


def _resident_bytes(F, Pout):
    return F * (Pout * JF * 4 * 8 + Pout * 8 + 4)                                  # xyz, kscore | pscore | count


TRIANGULATE_CASES = [
    # C, Pmax, J, F: (input bytes, candidate bytes) -> route
    (3, 1, JF, 32, "mapped"),                  # 18 816 + 50 024 = 67 KiB: the one-launch kernel
    (3, 1, JF, 200, "page-locked"),            # 117 600 + 312 608 = 420 KiB
    (3, 1, JF, 2800, "direct"),                # 1 646 400 | 4 376 408: the candidates are above 4 MiB
    (2, 1, 4097, 1, "mapped"),                 # 98 336 + 131 121 = 224 KiB; J > 4096: k_triangulate + k_cand_mean, both mirrored
    (2, 2, 1, 1025, "mapped"),                 # 57 400 + 168 108 = 220 KiB; F * Kc = 4100 > 4096: the same two launches
]


@pytest.mark.parametrize("C,Pmax,J,F,route", TRIANGULATE_CASES)
def test_triangulate_host_equals_device_on_every_route(C, Pmax, J, F, route):
    assert _route(*_triangulate_bytes(C, Pmax, J, F), mapped=True) == route
    kpts, n_persons = _frames(30 + F, C, F, Pmax, J)
    prm = _params()
    with frame_ctx(C) as ctx:
        want = triangulate(ctx, Device, kpts, n_persons, prm)
        assert want[3].any() and (F == 1 or not want[3].all()), "kept candidates, and slots no pair of persons fills"
        _same(triangulate(ctx, Host, kpts, n_persons, prm), want, f"snowtri_triangulate, {route}")
        # a pair of parallel rays: counted on every route, and the counter is back at zero for the next call
        bad = _with_parallel_rays(kpts)
        want_bad = triangulate(ctx, Device, bad, n_persons, prm)
        _same(triangulate(ctx, Host, bad, n_persons, prm, status=_lib.ERR_SINGULAR), want_bad, f"snowtri_triangulate with parallel rays, {route}")
        _same(triangulate(ctx, Host, kpts, n_persons, prm), want, f"snowtri_triangulate after the singular call, {route}")


@pytest.mark.parametrize("F,route", [(32, "mapped"), (200, "page-locked"), (2800, "direct")])
def test_condense_resident_equals_condense_on_device_pointers(F, route):
    Pout = 3
    assert _route(0, _resident_bytes(F, Pout), mapped=True) == route     # 50 048 | 312 800 | 4 379 200 bytes of outputs
    kpts, n_persons = _frames(30 + F, 3, F, 1, JF)
    with frame_ctx(3) as ctx:
        cand = triangulate(ctx, Device, kpts, n_persons, _params())
        for prm, pout, status in ((_params(), Pout, _lib.OK), (_params(**APART), 1, _lib.ERR_OVERFLOW)):
            want = condense(ctx, Device, cand, prm, pout)
            assert want[3].max() >= 1 and (want[3].max() > pout) == (status == _lib.ERR_OVERFLOW)
            assert np.array_equal(want[4], np.where(want[3] > pout, _lib.FLAG_OVERFLOW, 0))
            for flags in (True, False):
                triangulate(ctx, Host, kpts, n_persons, prm)
                got = condense_resident(ctx, F, prm, pout, flags=flags, status=status)
                _same(got, want[:4] + ((want[4],) if flags else (None,)), f"snowtri_condense_resident, {route}, Pout_max {pout}, flags {flags}")


@pytest.mark.parametrize("F,route", [(64, "page-locked"), (2800, "direct")])
def test_condense_host_equals_device_on_both_routes(F, route):
    Pout = 3
    assert _route(F * 3 * (JF * 4 * 8 + 1), _resident_bytes(F, Pout) + 4 * F, mapped=False) == route   # inputs: 98 496 | 4 309 200 bytes
    kpts, n_persons = _frames(40 + F, 3, F, 1, JF)
    with frame_ctx(3) as ctx:
        cand = triangulate(ctx, Device, kpts, n_persons, _params())
        for keep in (True, False):
            for flags in (True, False):
                _same(condense(ctx, Host, cand, _params(), Pout, keep, flags), condense(ctx, Device, cand, _params(), Pout, keep, flags),
                      f"snowtri_condense, {route}, cand_keep {keep}, out_flags {flags}")
        want = condense(ctx, Device, cand, _params(**APART), 1)
        assert (want[4] == _lib.FLAG_OVERFLOW).any()
        _same(condense(ctx, Host, cand, _params(**APART), 1, status=_lib.ERR_OVERFLOW), want, f"snowtri_condense, {route}, overflow")


@pytest.mark.parametrize("out_dtype", [np.float32, np.float64])
@pytest.mark.parametrize("F,route", [(64, "page-locked"), (8000, "direct")])
@pytest.mark.parametrize("robust", [False, True])
def test_fused_calls_host_equal_device_on_both_routes(robust, F, route, out_dtype):
    Pout = 2
    osz = np.dtype(out_dtype).itemsize
    out_bytes = F * (Pout * JF * 4 * osz + Pout * osz + 8 + (JF * (4 + osz) if robust else 0))
    assert _route(_triangulate_bytes(3, 1, JF, F)[0], out_bytes, mapped=False) == route      # inputs: 37 632 | 4 704 000 bytes
    kpts, n_persons = _frames(50 + F, 3, F, 1, JF)
    with frame_ctx(3) as ctx:
        options = [dict(), dict(pscore=False), dict(flags=False)] + ([dict(diagnostics=True), dict(diagnostics=True, flags=False)] if robust else [])
        _, _, full = fused(ctx, Device, kpts, n_persons, _params(), Pout, out_dtype, robust=robust, diagnostics=robust)
        assert full[2].max() >= 1
        for opt in options:
            rc, slow, got = fused(ctx, Host, kpts, n_persons, _params(), Pout, out_dtype, robust=robust, **opt)
            want = tuple(w if g is not None else None for g, w in zip(got, full))
            _same(got, want, f"fused call, robust {robust}, {route}, {opt}")
            assert rc == _status_of(full[3]), f"{opt}: status {rc}"
            assert slow == int(((full[3] & _lib.FLAG_FASTPATH) == 0).sum()), f"{opt}: snowtri_last_slow_frames"
        if not robust:                         # (one detection per camera is one person at the most on the robust route)
            _, _, over = fused(ctx, Device, kpts, n_persons, _params(**APART), 1, out_dtype)
            assert (over[3] & _lib.FLAG_OVERFLOW).any() and not (over[3] & _lib.FLAG_SINGULAR).any()
            for opt in (dict(), dict(flags=False)):
                rc, slow, got = fused(ctx, Host, kpts, n_persons, _params(**APART), 1, out_dtype, **opt)
                _same(got, tuple(w if g is not None else None for g, w in zip(got, over)), f"fused call, overflow, {route}, {opt}")
                assert rc == _lib.ERR_OVERFLOW and slow == int(((over[3] & _lib.FLAG_FASTPATH) == 0).sum())


def test_per_frame_staging_survives_a_regrowth_of_every_buffer():
    """Large, small, large on one context: the device scratch and the page-locked buffers are all sized before a base pointer is taken."""
    prm = _params()
    with frame_ctx(3) as ctx:
        cases = {F: _frames(60 + F, 3, F, 1, JF) for F in (2800, 32)}
        want = {F: triangulate(ctx, Device, *a, prm) for F, a in cases.items()}
        condensed = {F: condense(ctx, Device, want[F], prm, 3) for F in cases}
        big, small = _frames(70, 3, 8000, 1, JF), _frames(71, 3, 64, 1, JF)
        fused_want = {id(a): fused(ctx, Device, *a, prm, 2, np.float64)[2] for a in (big, small)}
        for step, (F, a) in enumerate(((2800, big), (32, small), (2800, big))):
            _same(triangulate(ctx, Host, *cases[F], prm), want[F], f"snowtri_triangulate, call {step + 1} of large / small / large")
            _same(condense_resident(ctx, F, prm, 3), condensed[F], f"snowtri_condense_resident, call {step + 1}")
            _same(condense(ctx, Host, want[F], prm, 3), condensed[F], f"snowtri_condense, call {step + 1}")
            _same(fused(ctx, Host, *a, prm, 2, np.float64)[2], fused_want[id(a)], f"fused call, call {step + 1}")
