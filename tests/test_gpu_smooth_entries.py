"""The smoothing entries of the C ABI as ONE host layer under two families (snowtri.hip, "the smoothing entry layer"): what the
numeric tests of test_gpu_smooth_carry.py / test_gpu_scan.py do not see.

  - A per-bone table whose 24 rows are one filter IS the uniform filter: the snowtri_blender_smooth_shard_* passes and the
    snowtri_smooth_shard_* passes, both forms of the protocol, give the same bits -- end states, entering states, tracks.  At this
    filter (2.5 Hz at 30 fps) A^256 underflows, where include/snowtri.h promises repeatable bits for the one-pass scan; the
    five-pass form has a fixed order at any filter.
  - The context's table cache (ctx->blender_key), which the whole-track call and the shard passes share: a changed table or a
    changed dt is uploaded, an unchanged one gives the bits of a fresh context.
(The refusals of the same entries are in tests/abi_badargs.c.)"""
import numpy as np
import pytest

import smooth_cases as sc

pytestmark = pytest.mark.gpu

FZR_ROW, DT = (2.5, 0.75, 0.0), 1 / 30
SIZES = (1, 0, 300, 33)        # a one-frame first block, an empty rank, two chunks / two workgroups, a short tail


def _bits(a):
    return np.ascontiguousarray(a).view(np.int64)


def _shard_run(family, P, x):
    """Both forms of the sharded protocol on device blocks of SIZES frames of x [T, P * 96].  family "uniform": the
    snowtri_smooth_shard_* entries on n = P * 96 lanes; "bone": snowtri_blender_smooth_shard_* on P persons with the one-filter
    table.  -> {name: [per non-empty rank: array]} for the five-pass form's end states, entering states and tracks ("local_end",
    "local_start", "local_y") and the two-pass form's ("scan_end", "scan_start", "scan_y")."""
    import torch
    from snowmocap_amd import _lib
    n, world = P * 96, len(SIZES)
    ctx = _lib.scratch_context()
    L, h = ctx.L, ctx.handle
    fzr = np.ascontiguousarray(np.tile(FZR_ROW, (24, 1)))
    if family == "uniform":
        pre, lanes, coef, ms = "snowtri_smooth_shard", n, (*FZR_ROW, DT), (_lib.DEVICE,)
    else:
        pre, lanes, coef, ms = "snowtri_blender_smooth_shard", P, (_lib.ptr(fzr), DT), ()

    def call(name, *args):
        _lib.check(getattr(L, pre + name)(h, *args), pre + name)

    dev = torch.device("cuda", 0)
    bounds = np.cumsum((0,) + SIZES)
    blocks = [torch.from_numpy(x[bounds[q]:bounds[q + 1]].copy()).to(dev) for q in range(world)]
    out = {}
    for form in ("local", "scan"):
        gathered = torch.zeros((world, 4 * n + 1), dtype=torch.float64, device=dev)
        ys = [torch.full_like(b, float("nan")) for b in blocks]
        for q, xb in enumerate(blocks):
            gathered[q, 4 * n] = SIZES[q]
            if not SIZES[q]:
                continue
            first, end = 1 if q == 0 else 0, _lib.ptr(gathered[q])
            if form == "local":
                call("_local", SIZES[q], lanes, _lib.ptr(xb), first, *coef, _lib.ptr(ys[q]), end, *ms, None)
            else:
                call("_reduce", SIZES[q], lanes, _lib.ptr(xb), first, *coef, end, None)
            gathered[q, 2 * n:3 * n] = xb[0]
            gathered[q, 3 * n:4 * n] = xb[-1]
        starts = []
        for q, xb in enumerate(blocks):
            if not SIZES[q]:
                continue
            first = 1 if q == 0 else 0
            start = torch.full((n, 2), float("nan"), dtype=torch.float64, device=dev)
            call("_combine", world, q, lanes, _lib.ptr(gathered), *coef, _lib.ptr(start), *ms, None)
            if form == "local":
                call("_fix", SIZES[q], lanes, first, _lib.ptr(start), *coef, _lib.ptr(ys[q]), *ms, None)
            else:
                call("_scan", SIZES[q], lanes, _lib.ptr(xb), first, _lib.ptr(start), *coef, _lib.ptr(ys[q]), None)
            starts.append(start)
        torch.cuda.synchronize(dev)
        live = [q for q in range(world) if SIZES[q]]
        out[form + "_end"] = [gathered[q, :2 * n].cpu().numpy() for q in live]
        out[form + "_start"] = [s.cpu().numpy() for s in starts]
        out[form + "_y"] = [ys[q].cpu().numpy() for q in live]
    return out


@pytest.mark.parametrize("P", (1, 2))
def test_one_filter_table_gives_the_bits_of_the_uniform_entries(P):
    """n = 96 and 192 lanes: two and three 64-lane columns."""
    x = sc.walk(0, sum(SIZES), P * 96)
    uni, bone = _shard_run("uniform", P, x), _shard_run("bone", P, x)
    for name in uni:
        for q, (a, b) in enumerate(zip(uni[name], bone[name])):
            assert not np.isnan(a).any() and a.shape == b.shape, (name, q)
            same = np.array_equal(_bits(a), _bits(b))
            print(f"entries: P {P} {name} block {q}: max |uniform - bone| {float(np.abs(a - b).max(initial=0.0)):.3e}"
                  f" ({'bit-equal' if same else 'NOT bit-equal'})")
            assert same, (P, name, q)


def test_table_cache_follows_the_table_and_dt():
    """One context: A, B, (a shard pass with B), A, A at dt = 1/60.  The cache must be refilled at every change and must not be
    where an unchanged table's bits come to depend on what ran before."""
    import torch
    from snowmocap_amd import _lib
    T, P = 300, 1
    pts, val = sc.blender_track(P, T, DT)
    A = np.ascontiguousarray(np.tile(FZR_ROW, (24, 1)))
    B = np.ascontiguousarray(np.tile((1.5, 0.6, -0.5), (24, 1)))

    def smooth(ctx, fzr, dt):
        out = np.empty_like(pts)
        _lib.check(ctx.L.snowtri_blender_smooth(ctx.handle, T, P, _lib.ptr(pts), _lib.ptr(val), _lib.ptr(fzr), dt, _lib.ptr(out),
                                                _lib.HOST, None), "snowtri_blender_smooth")
        return _bits(out)

    def fresh(fzr, dt):
        ctx = _lib.Context()
        try:
            return smooth(ctx, fzr, dt)
        finally:
            ctx.close()

    dev = torch.device("cuda", 0)
    held = torch.from_numpy(np.nan_to_num(pts).reshape(T, P * 96)).to(dev)
    end = torch.empty(2 * P * 96, dtype=torch.float64, device=dev)
    ctx = _lib.Context()
    try:
        a1 = smooth(ctx, A, DT)
        b = smooth(ctx, B, DT)
        _lib.check(ctx.L.snowtri_blender_smooth_shard_reduce(ctx.handle, T, P, _lib.ptr(held), 1, _lib.ptr(B), DT, _lib.ptr(end), None),
                   "snowtri_blender_smooth_shard_reduce")
        torch.cuda.synchronize(dev)
        a2 = smooth(ctx, A, DT)
        a60 = smooth(ctx, A, 1 / 60)
    finally:
        ctx.close()
    assert np.array_equal(a1, a2)
    assert np.array_equal(a1, fresh(A, DT)) and np.array_equal(b, fresh(B, DT)) and np.array_equal(a60, fresh(A, 1 / 60))
    assert not np.array_equal(a1, b) and not np.array_equal(a1, a60) and not np.array_equal(b, a60)
