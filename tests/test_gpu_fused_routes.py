"""Every kernel route of the fused call (snowtri_triangulate_condense[_ex], snowtri_triangulate_robust), through the C ABI:

1. the FULL string snowtri_last_kernel_names returns for the route (the other tests check prefixes; scripts and profiles/ read
   the whole string), with the outputs compared as the route's own tests compare them: the pairwise routes as
   tests/test_gpu_single_rigs.py (oracle.triangulate_condense_batch; float32 outputs <= 2e-6 m + one float32 ulp, scores 3e-7
   relative; float64 <= 1e-8 m, 1e-9), DLT as tests/test_gpu_parity.py (oracle/dlt.py; 1e-9 m / 2e-6 m, scores 1e-6 relative),
   the robust DLT as tests/test_gpu_robust.py (the masks where the rule's margin is >= 1e-6, joints where the masks agree);
   the per-frame flags and the call's status against the rule on every route (_check_flags);
2. the timing plumbing of every launcher: snowtri_set_timing(ctx, 1) brackets a call with an event pair, (ctx, 2) lets the
   single-kernel launchers carry the ring's pair on their dispatch -- which launchers do, what snowtri_timing_collect and
   snowtri_last_kernel_ms return in either mode, and that the outputs do not depend on it.

The batches and the strings: tests/fused_route_cases.py.  (The lean kernel's multi-segment launch -- more than 12 x 4 x 512 x 6
frames per CU, ~37 million -- is out of a test's reach.)
"""
import ctypes as ct

import numpy as np
import pytest

import fused_route_cases as frc
from test_gpu_single_rigs import _compare as compare_pairwise

pytestmark = pytest.mark.gpu
XYZ_F32 = 2e-6      # tests/test_gpu_parity.py: float32 rounding of ~5 m coordinates


@pytest.fixture(scope="module")
def api():
    import snowmocap_amd as sm
    from snowmocap_amd import _lib
    assert _lib.lib().snowtri_device_count() > 0, "these tests need the HIP device"
    return sm


def _compare_dlt(out, want, wps, f64):
    assert (out["count"] == 1).all()
    err = np.abs(out["xyzs"][..., :3] - want[..., :3]).max()
    assert err < (1e-9 if f64 else XYZ_F32), err
    np.testing.assert_allclose(out["xyzs"][..., 3], want[..., 3], rtol=1e-6)
    np.testing.assert_allclose(out["pscore"], wps, rtol=1e-6)


def _compare_dlt_multi(out, want, wps, wcnt, f64):
    np.testing.assert_array_equal(out["count"], wcnt)
    # (float32 outputs: + one float32 ulp of the value -- a ghost cluster of two nearly parallel rays lies kilometres away)
    tol = 1e-9 * (1.0 + np.abs(want[..., :3])) if f64 else XYZ_F32 + 1.2e-7 * np.abs(want[..., :3])
    assert (np.abs(out["xyzs"][..., :3] - want[..., :3]) <= tol).all()
    np.testing.assert_allclose(out["xyzs"][..., 3], want[..., 3], rtol=1e-6)
    np.testing.assert_allclose(out["pscore"], wps, rtol=1e-6)


def _compare_robust(out, ref, f64):
    sure = ref["margin"] >= 1e-6
    same = out["views"].astype(np.uint32) == ref["views"]
    assert same[sure].all(), f"{(~same & sure).sum()} masks differ where the reference's margin is >= 1e-6"
    from snowmocap_amd import _lib
    assert (out["count"] == 1).all() and (out["flags"] == _lib.FLAG_FASTPATH).all()
    got, want = out["xyzs"][:, 0].astype(np.float64), ref["xyzs"][:, 0]
    err = np.abs(got[..., :3] - want[..., :3])[same]
    assert err.max() < (1e-9 if f64 else XYZ_F32), err.max()
    np.testing.assert_allclose(got[..., 3][same], want[..., 3][same], rtol=1e-6)
    if same.all():
        np.testing.assert_allclose(out["pscore"][:, 0], ref["pscore"][:, 0], rtol=1e-6)


def _check_flags(r, out, singular, overflow):
    """The per-frame flags of a route: SNOWTRI_FLAG_SINGULAR and _OVERFLOW where the rule has them (singular: the oracle's frame
    status, tests/test_gpu_single_rigs.py; overflow: more persons than slots, tests/test_gpu_handover.py) and nowhere else;
    SNOWTRI_FLAG_FASTPATH as the route's kernels set it (fused_route_cases._route), and no other bit."""
    from snowmocap_amd import _lib
    fl = out["flags"]
    fast = (fl & _lib.FLAG_FASTPATH) != 0
    print(f"    flags: fast path {int(fast.sum())} of {len(fl)}, not on {np.nonzero(~fast)[0][:12].tolist()}; singular "
          f"{np.nonzero(fl & _lib.FLAG_SINGULAR)[0].tolist()}; overflow {int(((fl & _lib.FLAG_OVERFLOW) != 0).sum())}")
    assert not (fl & ~np.uint32(_lib.FLAG_SINGULAR | _lib.FLAG_OVERFLOW | _lib.FLAG_FASTPATH)).any()
    np.testing.assert_array_equal((fl & _lib.FLAG_SINGULAR) != 0, singular)
    np.testing.assert_array_equal((fl & _lib.FLAG_OVERFLOW) != 0, overflow)
    if r["fast"] == "all":
        assert fast.all()
    elif r["fast"] == "none":
        assert not fast.any()
    else:       # (opposite cameras of a ring see nearly parallel rays: a few clean frames take the fall-back, tests/test_gpu_single_rigs.py)
        assert not fast[frc.NOBODY] and fast.mean() > 0.9
    assert out["status"] == (_lib.ERR_SINGULAR if singular.any() else _lib.ERR_OVERFLOW if overflow.any() else _lib.OK)


@pytest.mark.parametrize("route", [r["id"] for r in frc.ROUTES])
def test_route_names_in_full_and_outputs_against_the_rule(api, route, knobs):
    r = frc.BY_ID[route]
    K, R, t, kp, npers, prm = frc.batch(route)
    bt = frc.triangulator(api, route, knobs, diagnostics=r["rule"] == "robust")
    out = bt.run_host(kp, npers)
    names = bt.ctx.last_kernel_names()
    bt.close()
    knobs.clear()
    print(f"{route}: {names}")
    assert names == r["names"]
    f64 = r["out"] == "float64"
    ref = frc.reference(route, r["pout"])
    none = np.zeros(frc.F, dtype=bool)
    if r["rule"] == "pairwise":
        singular = ref["status"] != 0      # (the reference raises on such a frame: nothing to compare there but the flag)
        assert np.array_equal(np.nonzero(singular)[0], r["singular"])
        ok = ~singular
        compare_pairwise({k: out[k][ok] for k in ("xyzs", "pscore", "count")}, {k: ref[k][ok] for k in ("xyz", "kscore", "pscore", "count")},
                         int(ok.sum()), np.dtype(r["out"]), r["kn"], route)
        _check_flags(r, out, singular, ~singular & (ref["count"] > r["pout"]))
    elif r["rule"] == "dlt":
        _compare_dlt(out, ref[0], ref[1], f64)
        _check_flags(r, out, none, none)
    elif r["rule"] == "dlt_multi":
        _compare_dlt_multi(out, ref[0], ref[1], ref[2], f64)
        _check_flags(r, out, none, ref[2] > r["pout"])
    else:
        _compare_robust(out, ref, f64)
        _check_flags(r, out, none, none)


@pytest.mark.parametrize("route,attaches", frc.TIMED)
def test_timing_plumbing_of_every_launcher(api, route, attaches, knobs):
    """Six device calls in each mode of snowtri_set_timing: six durations in (0, 50) ms from snowtri_timing_collect (the bound
    of tests/test_gpu_lean.py); snowtri_last_kernel_ms has a pair of its own after a bracketed call, and after an attached one
    only where the launcher does not attach (k_fused_single, the streaming route, k_frame_general); the same bits in both modes."""
    import torch
    from snowmocap_amd import _lib
    K, R, t, kp, npers, prm = frc.batch(route)
    bt = frc.triangulator(api, route, knobs)
    dev = torch.device("cuda", 0)
    d_kp, d_np = torch.from_numpy(kp.copy()).to(dev), torch.from_numpy(npers.copy()).to(dev)
    outs = {}
    for mode in (1, 2):
        out = bt.alloc_outputs(frc.F, dev)
        bt.run_torch(d_kp, d_np, out=out)
        bt.ctx.set_timing(True, attach=mode == 2)
        for _ in range(6):
            bt.run_torch(d_kp, d_np, out=out)
        arr = (ct.c_float * 2)()
        rc = bt.ctx.L.snowtri_last_kernel_ms(bt.ctx.handle, ct.byref(arr))
        ms = bt.ctx.timing_collect()
        bt.ctx.set_timing(False)
        torch.cuda.synchronize(dev)
        print(f"{route} mode {mode}: {bt.ctx.last_kernel_names()[:40]} last_kernel_ms -> {rc}, ring {['%.4f' % m for m in ms]}")
        assert len(ms) == 6 and all(0.0 < m < 50.0 for m in ms), (mode, ms)
        assert rc == (_lib.ERR_BAD_ARG if mode == 2 and attaches else _lib.OK), (mode, rc)
        outs[mode] = {k: v.cpu().numpy() for k, v in out.items()}
    assert bt.ctx.last_kernel_names() == frc.BY_ID[route]["names"]
    bt.close()
    knobs.clear()
    for k in outs[1]:
        assert np.array_equal(outs[1][k].view(np.uint8), outs[2][k].view(np.uint8)), k
