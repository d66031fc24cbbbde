"""The one-to-one assignment on the GPU: k_assign (snowmocap_amd/csrc/snowtri_assign.hpp) through snowtri_assign_detections,
Context.assign_detections and reproject.assign_detections, against the NumPy rule reproject.assign_detections_reference BIT FOR BIT
-- det_of, person_of and the bits of total.  Inputs: tests/assign_cases.py.

  - every (P, Pmax) on both sides of the sub-wave widths 8 | 16 | 32 | 64, problem counts that are no multiple of the problems per
    wave or per workgroup, three cost families, from NumPy (HOST) and from torch (DEVICE), with and without the optional outputs;
  - costs that k_reproject_cost itself wrote, on the recipe with crossing persons;
  - a problem's bits do not depend on the call it is in (order, cuts) nor on the problems packed into its wave (trip counts diverge);
  - TrackPipeline.run(one_to_one=True) and refine_rig(one_to_one=True); the bad-arguments program on a real context.
"""
import os
import subprocess

import numpy as np
import pytest

import assign_cases as ac
from conftest import ROOT
from snowmocap_amd import _lib
from snowmocap_amd import reproject as rp

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ctx():
    assert _lib.lib().snowtri_device_count() > 0, "these tests need the HIP device"
    return _lib.scratch_context()


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view({8: np.uint64, 4: np.uint32, 1: np.uint8}[a.dtype.itemsize])


def _same(got, want):
    """the kernel's array (int32 or float64) against the rule's (int64 or float64): the same integers, the same bits"""
    got, want = np.asarray(got), np.asarray(want)
    if want.dtype == np.float64:
        return got.dtype == np.float64 and got.shape == want.shape and np.array_equal(_bits(got), _bits(want))
    return got.shape == want.shape and np.array_equal(got.astype(np.int64), want)


def _host(ctx, cs, cn, gate_px=ac.GATE_PX, min_joints=ac.MIN_JOINTS):
    return ctx.assign_detections(np.ascontiguousarray(cs), np.ascontiguousarray(cn), gate_px, min_joints, with_person_of=True, with_total=True)


# ------------------------------------------------------------------------------------------------ the kernel against the rule
@pytest.mark.parametrize("size", ac.SIZES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_kernel_equals_the_rule_bit_for_bit(ctx, size):
    import torch
    P, Pmax = size
    nmax = max(ac.COUNTS)
    for name in ac.FAMILIES:
        cs, cn = ac.family(name, P, Pmax, nmax)
        want = ac.reference(name, P, Pmax, nmax)
        for n in ac.COUNTS:
            got = _host(ctx, cs[:n], cn[:n])
            for g, w, what in zip(got, want, ("det_of", "person_of", "total")):
                assert _same(g, w[:n]), (name, size, n, what)
            only = ctx.assign_detections(np.ascontiguousarray(cs[:n]), np.ascontiguousarray(cn[:n]), ac.GATE_PX, ac.MIN_JOINTS)
            assert only.dtype == np.int32 and _same(only, want[0][:n]), (name, size, n)
            tcs, tcn = torch.from_numpy(np.array(cs[:n])).to("cuda:0"), torch.from_numpy(np.array(cn[:n])).to("cuda:0")
            dev = ctx.assign_detections(tcs, tcn, ac.GATE_PX, ac.MIN_JOINTS, with_person_of=True, with_total=True)
            for g, w, what in zip(dev, want, ("det_of", "person_of", "total")):
                assert g.is_cuda and _same(g.cpu().numpy(), w[:n]), (name, size, n, what, "device")
            d2, t2 = ctx.assign_detections(tcs, tcn, ac.GATE_PX, ac.MIN_JOINTS, with_total=True)
            assert _same(d2.cpu().numpy(), want[0][:n]) and _same(t2.cpu().numpy(), want[2][:n])
        det64 = rp.assign_detections(ctx, cs, cn, ac.GATE_PX, ac.MIN_JOINTS)
        assert det64.dtype == np.int64 and np.array_equal(det64, want[0])


def test_costs_written_by_the_cost_kernel(ctx):
    """float64 costs made by k_reproject_cost on the rig with crossing persons -> the rule on those very costs"""
    import torch
    cs = ac.crossing()
    rig = _lib.Context(cs["K"], cs["R"], cs["t"])
    s, n = rig.reproject_cost(cs["xyzs"], cs["kpts"], n_persons=cs["n_persons"], keypoint_score_threshold=ac.CROSS_THRESHOLD)
    want = rp.assign_detections_reference(s, n, ac.CROSS_GATE)
    got = rig.assign_detections(s, n, ac.CROSS_GATE, with_person_of=True, with_total=True)
    for g, w in zip(got, want):
        assert _same(g, w)
    assert (want[0] >= 0).mean() > 0.9 and (want[0] == cs["det_true"]).mean() > 0.9
    ts, tn = rig.reproject_cost(torch.from_numpy(np.array(cs["xyzs"])).to("cuda:0"), torch.from_numpy(np.array(cs["kpts"])).to("cuda:0"),
                                n_persons=torch.from_numpy(np.array(cs["n_persons"])).to("cuda:0"), keypoint_score_threshold=ac.CROSS_THRESHOLD)
    det = rp.assign_detections(rig, ts, tn, ac.CROSS_GATE)
    assert det.dtype == torch.int64 and np.array_equal(det.cpu().numpy(), rp.assign_detections_reference(ts.cpu().numpy(), tn.cpu().numpy(), ac.CROSS_GATE)[0])
    # an exact 0 under gate_px = 0: a person against its own float64 projection
    pix = rig.reproject(cs["xyzs"][:2], dtype=np.float64)
    own = np.ascontiguousarray(pix)
    s0, n0 = rig.reproject_cost(cs["xyzs"][:2], own, keypoint_score_threshold=ac.CROSS_THRESHOLD)
    d0 = rig.assign_detections(s0, n0, 0.0)
    assert np.array_equal(d0, np.broadcast_to(np.arange(3), d0.shape)) and _same(d0, rp.assign_detections_reference(s0, n0, 0.0)[0])
    rig.close()


# ------------------------------------------------------------------------------------------------ independence
@pytest.mark.parametrize("size", [(4, 4), (3, 5), (8, 9), (16, 16), (16, 17), (1, 63)], ids=lambda s: f"{s[0]}x{s[1]}")
def test_bits_do_not_depend_on_the_call(ctx, size):
    P, Pmax = size
    n = 65
    for name in ac.FAMILIES:
        cs, cn = ac.family(name, P, Pmax, max(ac.COUNTS))
        cs, cn = cs[:n], cn[:n]
        whole = _host(ctx, cs, cn)
        back = _host(ctx, cs[::-1], cn[::-1])
        parts = [_host(ctx, cs[a:b], cn[a:b]) for a, b in ((0, 1), (1, 4), (4, n))]
        for k in range(3):
            assert np.array_equal(_bits(back[k][::-1]), _bits(whole[k])), (name, size, k, "reversed")
            assert np.array_equal(_bits(np.concatenate([p[k] for p in parts], axis=0)), _bits(whole[k])), (name, size, k, "cut")


@pytest.mark.parametrize("size", [(4, 4), (2, 3), (8, 8), (5, 11), (16, 16), (12, 17)], ids=lambda s: f"{s[0]}x{s[1]}")
def test_a_hard_problem_among_easy_ones_in_its_wave(ctx, size):
    """W < 64: 64 / W problems share a wave and run their own trip counts.  One hard problem (every row contested, augmenting paths
    through the whole tree) among easy ones (one step per row) returns its own bits wherever it sits -- every slot of the first wave,
    a slot of a later wave of the workgroup, and the last, partly filled wave."""
    P, Pmax = size
    per = 64 // ac.width(P, Pmax)
    assert per > 1
    easy, hard = ac.easy_problem(P, Pmax), ac.hard_problem(P, Pmax)
    want_hard = [a[0, 0] for a in rp.assign_detections_reference(hard[0][None, None], hard[1][None, None], ac.GATE_PX, ac.MIN_JOINTS)]
    want_easy = [a[0, 0] for a in rp.assign_detections_reference(easy[0][None, None], easy[1][None, None], ac.GATE_PX, ac.MIN_JOINTS)]
    assert (want_hard[0] >= 0).sum() == min(P, Pmax) and want_hard[0][P - 1] == 0       # the last row pushed every other one along
    n = 5 * per + 1
    for at in list(range(per)) + [per + 1, 3 * per - 1, n - 1]:
        cs = np.repeat(easy[0][None, None], n, axis=0)
        cn = np.repeat(easy[1][None, None], n, axis=0)
        cs[at, 0], cn[at, 0] = hard
        got = _host(ctx, cs, cn)
        for k in range(3):
            assert _same(got[k][at, 0], want_hard[k]), (size, at, k)
            others = np.delete(got[k][:, 0], at, axis=0)
            assert all(_same(o, want_easy[k]) for o in others), (size, at, k)


# ------------------------------------------------------------------------------------------------ the callers
def _pipeline(scene):
    from snowmocap_amd import TrackPipeline
    import pipeline_cases as plc
    K, R, t = scene["rig"]
    return TrackPipeline(K, R, t, scene["params"], plc.SMOOTH_PROFILE, n_persons_out=scene["slots"])


def test_pipeline_without_collisions_is_the_default_run(ctx):
    import pipeline_cases as plc
    sc = plc.scene("fixed", False)
    pipe = _pipeline(sc)
    base = pipe.run(sc["kpts"], sc["n_persons"], reproject=6.0, refine=4)
    one = pipe.run(sc["kpts"], sc["n_persons"], reproject=6.0, refine=4, one_to_one=True)
    assert not base["shared"].any().item() and (base["det_of"] >= 0).float().mean().item() > 0.5
    assert [k for k in one if k != "person_of"] == list(base) and "person_of" in one
    for k in base:
        a, b = base[k].cpu().numpy(), one[k].cpu().numpy()
        assert a.dtype == b.dtype and a.shape == b.shape and np.array_equal(_bits(a), _bits(b)), k
    det, per = one["det_of"].cpu().numpy(), one["person_of"].cpu().numpy()
    assert per.shape == det.shape[:2] + (sc["kpts"].shape[2],) and per.dtype == np.int64
    for p in range(det.shape[2]):
        m = det[..., p] >= 0
        assert (np.take_along_axis(per, np.maximum(det[..., p:p + 1], 0), axis=2)[..., 0][m] == p).all()
    with pytest.raises(ValueError, match="one_to_one"):
        pipe.run(sc["kpts"], sc["n_persons"], one_to_one=True)
    for kw in (dict(reproject=float("inf")), dict(refine=(4, float("inf"), False)), dict(reproject=6.0, refine=(4, 1e200, False))):
        with pytest.raises(ValueError, match="1e150"):                                        # "no gate" is match_detections' alone
            pipe.run(sc["kpts"], sc["n_persons"], one_to_one=True, **kw)
    assert "det_of" in pipe.run(sc["kpts"], sc["n_persons"], reproject=float("inf"))
    again = pipe.run(sc["kpts"], sc["n_persons"], reproject=6.0, refine=4)                    # the switch does not stick
    assert "person_of" not in again
    pipe.close()


def test_pipeline_with_planted_collisions(ctx):
    """Camera 0 lists only two of its three detections in every other frame and the gate is opened wide: the person it no longer
    lists is still triangulated from the other cameras, and in camera 0 it fits a detection that belongs to somebody else.
    match_detections hands that detection to both; the assignment gives every detection to one person."""
    import pipeline_cases as plc
    import reproject_cases
    from snowmocap_amd import TrackPipeline, synth
    mc = reproject_cases.match_case(4, 3, 8)
    thr = synth.default_thresholds()
    thr.update(keypoint_score_threshold=0.5, average_score_threshold=1.0, condense_distance_tol=0.3)
    npers = np.array(mc["n_persons"], copy=True)
    npers[::2, 0] = 2
    pipe = TrackPipeline(mc["K"], mc["R"], mc["t"], thr, plc.SMOOTH_PROFILE, n_persons_out=3)
    kw = dict(reproject=1000.0, refine=(4, 1000.0, False))
    kpts = np.array(mc["kpts"])
    base = pipe.run(kpts, npers, **kw)
    one = pipe.run(kpts, npers, one_to_one=True, **kw)
    assert (base["count"] == 3).all().item() and base["shared"][::2, 0].any(dim=-1).all().item()   # the plant is there
    det = one["det_of"].cpu().numpy()
    srt = np.sort(det, axis=-1)
    assert not ((srt[..., 1:] == srt[..., :-1]) & (srt[..., 1:] >= 0)).any()                   # no detection twice within an (f, c)
    assert not one["shared"].any().item()
    assert ((det[::2, 0] >= 0).sum(axis=-1) == 2).all() and (det[1::2] >= 0).all()
    cost = one["refine_cost"].cpu().numpy()
    assert (cost[..., 1] <= cost[..., 0]).all()
    pipe.close()


def test_refine_rig_one_to_one_on_a_single_person_recording(ctx):
    import pose_cases as pc
    from snowmocap_amd import pose
    rcp = pc.recipe(P=1)
    args = (rcp["K"], rcp["Rd"], rcp["td"], rcp["kpts"])
    a = pose.refine_rig(*args, free=[rcp["bad"]], rounds=1, method=_lib.DLT)
    b = pose.refine_rig(*args, free=[rcp["bad"]], rounds=1, method=_lib.DLT, one_to_one=True)
    assert np.array_equal(_bits(a[0]), _bits(b[0])) and np.array_equal(_bits(a[1]), _bits(b[1]))
    assert np.array_equal(_bits(a[2][-1]["view_rms"]), _bits(b[2][-1]["view_rms"]))


# ------------------------------------------------------------------------------------------------ buffers, bad arguments, debug build
def test_wrapper_refusals_and_empty_batches(ctx):
    import torch
    cs, cn = ac.family("floats", 3, 5, 7)
    for space in (_lib.HOST, _lib.DEVICE):
        assert ctx.L.snowtri_assign_detections(ctx.handle, 0, 3, 5, None, None, 6.0, 8, None, None, None, space, None) == _lib.OK
    d, p, t = ctx.assign_detections(cs[:0], cn[:0], 6.0, with_person_of=True, with_total=True)
    assert d.shape == (0, 1, 3) and p.shape == (0, 1, 5) and t.shape == (0, 1)
    flat = ctx.assign_detections(np.ascontiguousarray(cs[:, 0]), np.ascontiguousarray(cn[:, 0]), ac.GATE_PX, ac.MIN_JOINTS)    # [n, P, Pmax]
    assert _same(flat, ac.reference("floats", 3, 5, 7)[0][:, 0])
    for bad, word in ((dict(gate_px=-1.0), "gate_px"), (dict(gate_px=float("nan")), "gate_px"), (dict(min_joints=0), "min_joints"),
                      (dict(gate_px=float("inf")), "1e150"), (dict(gate_px=1e200), "1e150")):
        kw = dict(gate_px=6.0, min_joints=8)
        kw.update(bad)
        with pytest.raises(ValueError, match=word):
            ctx.assign_detections(cs, cn, **kw)
    for space in (_lib.HOST, _lib.DEVICE):                                                    # ... and by the entry itself
        assert ctx.L.snowtri_assign_detections(ctx.handle, 7, 3, 5, _lib.ptr(np.array(cs)), _lib.ptr(np.array(cn)), float("inf"), 8,
                                               _lib.ptr(np.zeros((7, 3), dtype=np.int32)), None, None, space, None) == _lib.ERR_BAD_ARG
        assert b"1e150" in ctx.L.snowtri_last_error()
    # up to the widest gate it takes the kernel equals the rule, P > Pmax and inadmissible pairs included
    for gate in (1e6, 1e150):
        for P, Pmax in ((4, 2), (2, 2), (3, 5), (9, 7)):
            wc, wn = ac.family("inadmissible", P, Pmax, 65)
            got = ctx.assign_detections(np.array(wc), np.array(wn), gate, ac.MIN_JOINTS, with_person_of=True, with_total=True)
            for g, w in zip(got, rp.assign_detections_reference(wc, wn, gate, ac.MIN_JOINTS)):
                assert _same(g, w), (gate, P, Pmax)
    with pytest.raises(ValueError, match="64"):
        ctx.assign_detections(np.zeros((1, 40, 25)), np.ones((1, 40, 25), dtype=np.int32), 6.0)
    with pytest.raises(ValueError):
        ctx.assign_detections(cs, cn[..., :4], 6.0)
    with pytest.raises(ValueError):
        ctx.assign_detections(torch.from_numpy(np.array(cs)).to("cuda:0"), cn, 6.0)            # a mixture
    with pytest.raises(ValueError):
        ctx.assign_detections(torch.from_numpy(np.array(cs)).to("cuda:0").to(torch.float32), torch.from_numpy(np.array(cn)).to("cuda:0"), 6.0)


def test_kernel_time_goes_through_last_kernel_ms():
    own = _lib.Context()
    cs, cn = ac.family("floats", 4, 4, 257)
    own.set_timing(True)
    got = own.assign_detections(np.array(cs), np.array(cn), ac.GATE_PX, ac.MIN_JOINTS)
    ms = own.last_kernel_ms()
    assert 0.0 < ms[0] < 50.0 and 0.0 <= ms[1] < 1.0 and _same(got, ac.reference("floats", 4, 4, 257)[0])
    own.set_timing(False)
    own.close()


def test_entry_rejects_bad_arguments_on_a_real_context(ctx, tmp_path):
    """tests/abi_badargs_assign.c against libsnowtri.so on the GPU: refusals before any launch, then one good call."""
    lib_dir = os.path.join(ROOT, "snowmocap_amd")
    exe = str(tmp_path / "abi_badargs_assign")
    subprocess.check_call(["gcc", "-std=c99", "-O1", "-I", os.path.join(ROOT, "include"), os.path.join(ROOT, "tests", "abi_badargs_assign.c"),
                           "-o", exe, "-L", lib_dir, "-lsnowtri", "-Wl,-rpath," + lib_dir])
    out = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0 and "0 failure(s)" in out.stdout, out.stdout[-3000:] + out.stderr[-2000:]


DBG_CODE = r'''
import sys, numpy as np
sys.path.insert(0, %(root)r)
sys.path.insert(0, %(tests)r)
import assign_cases as ac
from snowmocap_amd import _lib
assert _lib.LIB_PATH.endswith("libsnowtri_dbg.so") and "SNOWTRI_DEBUG_BOUNDS" in _lib.build_info()["variants"]
ctx = _lib.scratch_context()
for P, Pmax in ((4, 4), (8, 9), (16, 17), (32, 32), (1, 63)):
    cs, cn = ac.family("inadmissible", P, Pmax, 7)
    got = ctx.assign_detections(np.ascontiguousarray(cs), np.ascontiguousarray(cn), ac.GATE_PX, ac.MIN_JOINTS)
    assert np.array_equal(got, ac.reference("inadmissible", P, Pmax, 7)[0])
    n, first = ctx.debug_faults()
    assert n == 0, "device-side bounds check failed %%d times; first: code %%d at line %%d" %% (n, first >> 32, first & 0xffffffff)
print("assign debug-bounds ok")
'''


def test_debug_build_counts_no_fault():
    dbg = os.path.join(ROOT, "snowmocap_amd", "libsnowtri_dbg.so")
    assert os.path.exists(dbg), f"{dbg} is missing: `make -C snowmocap_amd/csrc debug`"
    import sys
    env = dict(os.environ, SNOWTRI_LIB=dbg)
    code = DBG_CODE % {"root": ROOT, "tests": os.path.join(ROOT, "tests")}
    out = subprocess.run([sys.executable, "-c", code], env=env, capture_output=True, text=True, timeout=300)
    assert out.returncode == 0 and "assign debug-bounds ok" in out.stdout, out.stdout[-2000:] + out.stderr[-3000:]
