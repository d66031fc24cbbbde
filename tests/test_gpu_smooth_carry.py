"""Rows N1 / N2 on the GPU at filters where the state a 256-frame workgroup hands to the next matters (tests/smooth_cases.py):
240 fps captures of the reference's profiles, slow, overdamped and undamped filters, at which P = A^256 runs from 2e-6 to 3 --
at the 30 fps profiles of the older smoothing tests it is 1e-20 ... 1e-77 and nothing there can see the four p** coefficients, the
M <- M P of the look-back, the P S_in of the published state, the exponent of the combine or k_smooth_carry past its first chunk.
Every entry is held to the reference rule evaluated in longdouble, within 16 x the committed fp64 sequential oracle's own error
on the same input (smooth_cases.tol).  Each test prints `carry: ...` lines with the figures it asserts on (pytest -s)."""
import ctypes as ct

import numpy as np
import pytest

import smooth_cases as sc

pytestmark = pytest.mark.gpu

NCASES = len(sc.CARRY_CASES)


def _report(what, err, tol, oerr):
    print(f"carry: {what}: err {err:.3e} oracle {oerr:.3e} ratio {err / oerr if oerr else float('nan'):.2f} tol {tol:.3e}")


@pytest.mark.parametrize("n", sc.TRACK_N)
@pytest.mark.parametrize("T", sc.TRACK_T)
@pytest.mark.parametrize("ci", range(NCASES))
def test_smooth_track_carries_the_state_across_workgroups(ci, T, n):
    import snowmocap_amd as api
    f, z, r, dt = sc.CARRY_CASES[ci]
    x, ry, _, tol, oerr = sc.track_case(ci, T, n)
    got = api.smooth_track(x, f=f, z=z, r=r, delta_time=dt)
    err = sc.distance(got, ry)
    _report(f"smooth_track case {ci} T {T} n {n}", err, tol, oerr)
    assert err <= tol, (sc.CARRY_CASES[ci], T, n, err, tol)
    assert np.array_equal(got[0].view(np.int64), x[0].view(np.int64))                        # frame 0 passes through


@pytest.mark.parametrize("T,m", sc.JOINT_SHAPES)
@pytest.mark.parametrize("ci", (0, 5))
def test_joint_track_carries_the_state_and_copies_the_scores(ci, T, m):
    """The SKIP4 instantiation: three lanes of a record filtered, the score lane copied bit for bit -- inf, NaN and 0 included."""
    from snowmocap_amd import _lib
    from oracle import oracle as orc
    case = sc.CARRY_CASES[ci]
    rng = np.random.default_rng([ci, T, m])
    x = np.cumsum(rng.normal(0, 0.01, size=(T, m, 4)), axis=0) + rng.uniform(-3, 3, size=(1, m, 4))
    x[..., 3] = rng.uniform(0, 9, size=(T, m))
    x[3, 0, 3] = np.inf
    x[4, 1, 3] = np.nan
    x[5, :, 3] = 0.0
    x[T - 1, m - 1, 3] = np.inf
    x[300, :, 3] = np.nan                                                                   # (a whole row, in the second workgroup)
    y = np.empty_like(x)
    ctx = _lib.scratch_context()
    _lib.check(ctx.L.snowtri_smooth_joint_track(ctx.handle, T, m, _lib.ptr(x), *case, _lib.ptr(y), _lib.HOST, None), "snowtri_smooth_joint_track")
    xyz = np.ascontiguousarray(x[..., :3]).reshape(T, 3 * m)
    ry, _ = sc.reference(xyz, case)
    want = orc.second_order_track(xyz, *case)
    tol, oerr = sc.tol(case, ry, want), sc.oracle_error(ry, want)
    err = sc.distance(y[..., :3].reshape(T, 3 * m), ry)
    _report(f"joint_track case {ci} T {T} m {m}", err, tol, oerr)
    assert err <= tol, (case, T, m, err, tol)
    assert np.array_equal(y[..., 3].view(np.int64), x[..., 3].view(np.int64))


@pytest.mark.parametrize("dt", (1 / 30, 1 / 240))
@pytest.mark.parametrize("T", (514, 1030))
@pytest.mark.parametrize("P", (1, 2))
def test_blender_smoothing_with_a_slow_to_fast_table_and_the_hold(P, T, dt):
    """TableCoef and HoldInput: 24 control points from 0.05 Hz to 2.25 Hz -- the table index decides how much carry a lane sees --
    with runs of invalid points from frame 0 on, across a wave, across a workgroup, one longer than a workgroup on a slow point,
    and a point that is never valid."""
    from snowmocap_amd import blender as bl
    pts, val, fzr, ref, tol, oerr = sc.blender_case(P, T, dt)
    prof = {nm: list(fzr[i]) for i, nm in enumerate(bl.CONTROL_POINT_NAMES)}
    got = bl.blender_smooth_track(pts, val, prof, dt)
    assert np.array_equal(np.isnan(got), np.isnan(ref.astype(np.float64)))
    err = sc.distance(got, ref)
    _report(f"blender_smooth P {P} T {T} fps {round(1 / dt)}", err, tol, oerr)
    assert err <= tol, (P, T, dt, err, tol)


def _blocks(x, bounds, dev):
    import torch
    return [torch.from_numpy(x[bounds[q]:bounds[q + 1]].copy()).to(dev) for q in range(len(bounds) - 1)]


def _check_starts(s, q, start_dev, label):
    """The entering state of rank q: the high-precision state, and the host twin, y and yd each within their tolerance."""
    from snowmocap_amd.sharded import combine_carries, smooth_coeffs
    A, cx, cxd = smooth_coeffs(*s["case"])
    host = combine_carries(s["payloads_gpu"], q, A, cxd)
    for j, (nm, tl) in enumerate((("y", s["tol_y"]), ("yd", s["tol_yd"]))):
        d_ref = sc.distance(start_dev[:, j], s["start"][q][:, j])
        d_host = float(np.abs(start_dev[:, j] - host[:, j]).max())
        print(f"carry: {label} rank {q} start {nm}: to reference {d_ref:.3e}, to combine_carries {d_host:.3e}, tol {tl:.3e}")
        assert d_ref <= tl and d_host <= tl, (s["case"], q, nm, d_ref, d_host, tl)


@pytest.mark.parametrize("n", (5, 130))
@pytest.mark.parametrize("ci", sc.SHARD_CASES)
def test_two_pass_shard_protocol_with_the_device_combine(ci, n):
    """snowtri_smooth_shard_reduce / _combine (k_smooth_combine, on the device) / _scan on blocks of (1, 256, 0, 300, 33, 700) frames:
    every rank's entering state against the high-precision state and against combine_carries, the assembled track against the
    reference.  The 300- and 700-frame blocks chain two and three workgroups with a live P; A^m reaches m = 700."""
    import torch
    from snowmocap_amd import _lib
    s = dict(sc.shard_case(ci, n))
    case, x, bounds, first = s["case"], s["x"], s["bounds"], s["first"]
    sizes, world = sc.SHARD_SIZES, len(sc.SHARD_SIZES)
    ctx = _lib.scratch_context()
    L = ctx.L
    dev = torch.device("cuda", 0)
    blocks = _blocks(x, bounds, dev)
    gathered = torch.zeros((world, 4 * n + 1), dtype=torch.float64, device=dev)
    for q, xb in enumerate(blocks):
        if sizes[q]:
            _lib.check(L.snowtri_smooth_shard_reduce(ctx.handle, sizes[q], n, _lib.ptr(xb), 1 if q == first else 0, *case,
                                                     ct.c_void_p(gathered[q].data_ptr()), None), "reduce")
            gathered[q, 2 * n:3 * n] = xb[0]
            gathered[q, 3 * n:4 * n] = xb[-1]
        gathered[q, 4 * n] = sizes[q]
    torch.cuda.synchronize(dev)
    gh = gathered.cpu().numpy()
    s["payloads_gpu"] = [(gh[q, :2 * n].reshape(n, 2), gh[q, 2 * n:3 * n], gh[q, 3 * n:4 * n], sizes[q]) for q in range(world)]
    got = np.zeros_like(x)
    for q, xb in enumerate(blocks):
        if not sizes[q]:
            continue
        start = torch.full((n, 2), float("nan"), dtype=torch.float64, device=dev)
        _lib.check(L.snowtri_smooth_shard_combine(ctx.handle, world, q, n, _lib.ptr(gathered), *case, _lib.ptr(start), _lib.DEVICE, None), "combine")
        yb = torch.empty_like(xb)
        _lib.check(L.snowtri_smooth_shard_scan(ctx.handle, sizes[q], n, _lib.ptr(xb), 1 if q == first else 0, _lib.ptr(start), *case,
                                               _lib.ptr(yb), None), "scan")
        torch.cuda.synchronize(dev)
        _check_starts(s, q, start.cpu().numpy(), f"two-pass case {ci} n {n}")
        got[bounds[q]:bounds[q + 1]] = yb.cpu().numpy()
    err = sc.distance(got, s["ref"][0])
    _report(f"two-pass case {ci} n {n}", err, s["tol_y"], s["oracle_err"])
    assert err <= s["tol_y"], (case, n, err, s["tol_y"])


@pytest.mark.parametrize("n", (5, 130))
@pytest.mark.parametrize("ci", sc.SHARD_CASES)
def test_five_pass_shard_protocol_with_a_live_chunk_power(ci, n):
    """snowtri_smooth_shard_local / _combine / _fix on the same blocks: the 700-frame block runs k_smooth_carry over three chunks
    and k_smooth_shard_end behind them, both through P."""
    from snowmocap_amd import _lib
    s = dict(sc.shard_case(ci, n))
    case, x, bounds, first = s["case"], s["x"], s["bounds"], s["first"]
    sizes, world = sc.SHARD_SIZES, len(sc.SHARD_SIZES)
    ctx = _lib.scratch_context()
    L = ctx.L
    shards = [np.ascontiguousarray(x[bounds[q]:bounds[q + 1]]) for q in range(world)]
    gathered = np.zeros((world, 4 * n + 1))
    ys = []
    for q, sh in enumerate(shards):
        y = np.empty_like(sh)
        E = np.zeros((n, 2))
        if sizes[q]:
            _lib.check(L.snowtri_smooth_shard_local(ctx.handle, sizes[q], n, _lib.ptr(sh), 1 if q == first else 0, *case, _lib.ptr(y), _lib.ptr(E),
                                                    _lib.HOST, None), "local")
            gathered[q, :2 * n] = E.reshape(-1)
            gathered[q, 2 * n:3 * n] = sh[0]
            gathered[q, 3 * n:4 * n] = sh[-1]
        gathered[q, 4 * n] = sizes[q]
        ys.append(y)
    s["payloads_gpu"] = [(gathered[q, :2 * n].reshape(n, 2), gathered[q, 2 * n:3 * n], gathered[q, 3 * n:4 * n], sizes[q]) for q in range(world)]
    for q, sh in enumerate(shards):
        if not sizes[q]:
            continue
        start = np.full((n, 2), np.nan)
        _lib.check(L.snowtri_smooth_shard_combine(ctx.handle, world, q, n, _lib.ptr(gathered), *case, _lib.ptr(start), _lib.HOST, None), "combine")
        _check_starts(s, q, start, f"five-pass case {ci} n {n}")
        _lib.check(L.snowtri_smooth_shard_fix(ctx.handle, sizes[q], n, 1 if q == first else 0, _lib.ptr(start), *case, _lib.ptr(ys[q]), _lib.HOST, None), "fix")
    err = sc.distance(np.concatenate(ys), s["ref"][0])
    _report(f"five-pass case {ci} n {n}", err, s["tol_y"], s["oracle_err"])
    assert err <= s["tol_y"], (case, n, err, s["tol_y"])


def test_blender_table_shard_protocol():
    """snowtri_blender_smooth_shard_reduce / _combine (k_smooth_combine<TableCoef>) / _scan on blocks of (300, 0, 520) frames of one
    person's control points, valid everywhere (the held track is the track), the slow-to-fast table."""
    import torch
    from snowmocap_amd import _lib
    from oracle import blender as ob
    sizes, dt, P = sc.BLENDER_SHARD_SIZES, 1 / 30, 1
    T, n, world = sum(sizes), 96, len(sizes)
    fzr = np.ascontiguousarray(sc.blender_table())
    rng = np.random.default_rng(sizes)
    pts = np.cumsum(rng.normal(0, 0.01, size=(T, P, 24, 4)), axis=0) + rng.uniform(-2, 2, size=(1, P, 24, 4))
    val = np.ones((T, P, 24), np.uint8)
    ref = sc.blender_reference(pts, val, fzr, dt)
    want = ob.smooth_track(pts, val, fzr, dt)
    tol, oerr = sc.tol(None, ref, want), sc.oracle_error(ref, want)
    bounds = np.cumsum((0,) + tuple(sizes))
    ctx = _lib.scratch_context()
    L = ctx.L
    dev = torch.device("cuda", 0)
    blocks = _blocks(pts.reshape(T, n), bounds, dev)
    gathered = torch.zeros((world, 4 * n + 1), dtype=torch.float64, device=dev)
    for q, xb in enumerate(blocks):
        if sizes[q]:
            _lib.check(L.snowtri_blender_smooth_shard_reduce(ctx.handle, sizes[q], P, _lib.ptr(xb), 1 if q == 0 else 0, _lib.ptr(fzr), dt,
                                                             ct.c_void_p(gathered[q].data_ptr()), None), "reduce")
            gathered[q, 2 * n:3 * n] = xb[0]
            gathered[q, 3 * n:4 * n] = xb[-1]
        gathered[q, 4 * n] = sizes[q]
    got = np.zeros((T, n))
    for q, xb in enumerate(blocks):
        if not sizes[q]:
            continue
        start = torch.full((n, 2), float("nan"), dtype=torch.float64, device=dev)
        _lib.check(L.snowtri_blender_smooth_shard_combine(ctx.handle, world, q, P, _lib.ptr(gathered), _lib.ptr(fzr), dt, _lib.ptr(start), None), "combine")
        yb = torch.empty_like(xb)
        _lib.check(L.snowtri_blender_smooth_shard_scan(ctx.handle, sizes[q], P, _lib.ptr(xb), 1 if q == 0 else 0, _lib.ptr(start), _lib.ptr(fzr), dt,
                                                       _lib.ptr(yb), None), "scan")
        torch.cuda.synchronize(dev)
        got[bounds[q]:bounds[q + 1]] = yb.cpu().numpy()
    err = sc.distance(got.reshape(pts.shape), ref)
    _report("blender shard (300, 0, 520)", err, tol, oerr)
    assert err <= tol, (err, tol)


@pytest.mark.parametrize("ci", sc.REPRO_CASES)
def test_runs_repeat_to_the_rounding_bound_where_P_is_alive(ci):
    """The look-back folds aggregates or an inclusive state, whichever a predecessor has published when it is read: the two
    orders agree in exact arithmetic only.  Where P underflows they agree to the bit (the 2.5 Hz tests assert that); here, with
    max|P| of 1 and 3 and nine workgroups down each of three columns, every run is within tol of the reference, hence any two
    within 2 tol of one another.  Bit equality is NOT asserted."""
    import torch
    from snowmocap_amd import _lib
    case = sc.CARRY_CASES[ci]
    T, n = sc.REPRO_SHAPE
    x, ry, _, tol, oerr = sc.track_case(ci, T, n)
    ctx = _lib.scratch_context()
    dev = torch.device("cuda", 0)
    xd = torch.from_numpy(x.copy()).to(dev)
    runs = []
    for rep in range(3):
        yd = torch.empty_like(xd)
        _lib.check(ctx.L.snowtri_smooth_track(ctx.handle, T, n, _lib.ptr(xd), *case, _lib.ptr(yd), _lib.DEVICE, None), "snowtri_smooth_track")
        torch.cuda.synchronize(dev)
        runs.append(yd.cpu().numpy())
        err = sc.distance(runs[-1], ry)
        _report(f"repeat case {ci} run {rep}", err, tol, oerr)
        assert err <= tol, (case, rep, err, tol)
    for a in range(3):
        for b in range(a + 1, 3):
            spread = float(np.abs(runs[a] - runs[b]).max())
            print(f"carry: repeat case {ci} runs {a},{b}: spread {spread:.3e} ({'bit-equal' if np.array_equal(runs[a], runs[b]) else 'not bit-equal'})")
            assert spread <= 2 * tol, (case, a, b, spread, tol)
