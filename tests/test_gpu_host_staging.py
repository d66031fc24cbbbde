"""SNOWTRI_HOST against SNOWTRI_DEVICE for the entry points that stage host arrays through the context's device scratch
(snowmocap_amd/csrc/snowtri.hip: ctx->in, ctx->out).  A host call uploads its arrays, runs the kernels of the device call on the
staged copies, and downloads the outputs, so every output has to come back bit for bit as the device call leaves it: with an
optional array absent, across a regrowth of the scratch (it starts at 1 MiB and is freed and reallocated beyond that), and for
an array that is both read and written.  No tolerance anywhere: both sides are the same kernels on the same values.

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
