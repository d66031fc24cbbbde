"""Seeding on the GPU: k_pair_cost and k_seed_group (snowmocap_amd/csrc/snowtri_seed.hpp) through snowtri_pair_cost,
snowtri_seed_persons, Context.pair_cost / seed_persons and seed.triangulate_seeded.  Inputs: tests/seed_cases.py.

  - k_pair_cost against the 50-digit evaluation of its rule within MARGIN x FLOOR (tests/seed_cases.py: the floor is the NumPy
    rule's own error, the margin covers fused multiply-adds and another order of summation), pair_n exactly: 2, 3, 4 and 8 cameras,
    Pmax 1 .. 8, joint counts on both sides of every wave boundary up to 256, 1, 3 and 37 frames, both keypoint types, HOST and
    DEVICE, with ragged and empty lists, claimed detections, low scores and NaN pixels;
  - a pair's bits do not depend on its surroundings: alone, in a batch, cut into two calls, Pmax padded by unused slots;
  - k_seed_group against seed_persons_reference on the SAME arrays, every output bit for bit: the arrays k_pair_cost wrote,
    synthetic weight families, node counts on both sides of 8, 16, 32 and at 64, S in {1, 2, C * Pmax}, reordered and cut;
  - triangulate_seeded: its records are triangulate_matched on its own seed_det_of bit for bit, and the recipes' conditions hold on
    the device path; the bad-arguments program on real contexts; both kernels under the device-side bounds checks.
"""
import functools
import os
import subprocess
import sys

import numpy as np
import pytest

import assign_cases as ac
import pose_cases as pc
import seed_cases as sc
from conftest import ROOT
from snowmocap_amd import _lib, synth
from snowmocap_amd import seed as sd

pytestmark = pytest.mark.gpu

_CTX = {}


def _rig_ctx(C):
    """a context of C cameras (seed_persons needs the context for C alone)"""
    assert _lib.lib().snowtri_device_count() > 0, "these tests need the HIP device"
    if C not in _CTX:
        _CTX[C] = _lib.Context(*synth.ring_rig(C))
    return _CTX[C]


def _batch_ctx(b):
    return _lib.Context(b["K"], b["R"], b["t"])


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view({8: np.uint64, 4: np.uint32, 1: np.uint8}[a.dtype.itemsize])


def _dev(a):
    import torch
    return None if a is None else torch.from_numpy(np.array(a)).to("cuda:0")


@functools.lru_cache(maxsize=None)
def _exact(shape, dt):
    b = sc.batch(*shape, kp_dtype=dt)
    return sc.exact_pair_cost(b["K"], b["R"], b["t"], b["kpts"], b["n_persons"], b["claimed"], b["thr"])


# ------------------------------------------------------------------------------------------------ k_pair_cost against 50 digits
@pytest.mark.parametrize("shape", sc.EXACT_SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_pair_cost_against_the_exact_rule(shape):
    C, Pmax, kn, F = shape
    worst = 0.0
    for dt in ("float32", "float64"):
        b = sc.batch(*shape, kp_dtype=dt)
        root, n, _ = _exact(shape, dt)
        ctx = _batch_ctx(b)
        host = ctx.pair_cost(b["kpts"], b["n_persons"], b["claimed"], b["thr"])
        dev = ctx.pair_cost(_dev(b["kpts"]), _dev(b["n_persons"]), _dev(b["claimed"]), b["thr"])
        assert dev[0].is_cuda and dev[1].is_cuda
        dev = tuple(a.cpu().numpy() for a in dev)
        ctx.close()
        for ps, pn in (host, dev):
            assert ps.dtype == np.float64 and pn.dtype == np.int32 and ps.shape == pn.shape == (F, C * (C - 1) // 2, Pmax, Pmax)
            assert np.array_equal(pn, n), (shape, dt)
            assert (ps[pn == 0] == 0).all() and np.isfinite(ps).all()
            err = float(np.abs(sc.root_mean(ps, pn) - root).max()) / b["s"]
            worst = max(worst, err)
            print(f"    {shape} {dt}: max |root - exact| / s = {err:.3e} (bar {sc.MARGIN * sc.FLOOR:.3e}), pairs with joints {(n > 0).sum()} of {n.size}")
        assert np.array_equal(_bits(host[0]), _bits(dev[0]))                                   # HOST and DEVICE: the same kernel, the same bits
        assert (n > 0).any() or kn == 1                                                         # (one joint of one pair may be sprinkled away)
    assert worst <= sc.MARGIN * sc.FLOOR, (shape, worst)


def test_unlisted_inputs_none_means_everything_free():
    b = sc.batch(4, 2, 17, 3, kp_dtype="float64", sprinkled=False)
    ctx = _batch_ctx(b)
    a = ctx.pair_cost(b["kpts"], None, None, b["thr"])
    c = ctx.pair_cost(b["kpts"], b["n_persons"], b["claimed"], b["thr"])
    want = sd.pair_cost_reference(b["K"], b["R"], b["t"], b["kpts"], None, None, b["thr"], M=ctx.ray_matrices())
    ctx.close()
    assert np.array_equal(_bits(a[0]), _bits(c[0])) and np.array_equal(a[1], c[1]) and np.array_equal(a[1], want[1])
    assert np.allclose(a[0], want[0], rtol=1e-12, atol=0) and (a[1] == 17).all()


# ------------------------------------------------------------------------------------------------ independence
@pytest.mark.parametrize("shape", sc.BATCH_SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_a_pairs_bits_do_not_depend_on_its_surroundings(shape):
    C, Pmax, kn, F = shape
    b = sc.batch(*shape)
    ctx = _batch_ctx(b)
    kp, npers, cl = np.array(b["kpts"]), np.array(b["n_persons"]), np.array(b["claimed"])
    whole = ctx.pair_cost(kp, npers, cl, b["thr"])
    for f in (0, 1, F - 1):                                                                     # a frame alone
        one = ctx.pair_cost(kp[f:f + 1], npers[f:f + 1], cl[f:f + 1], b["thr"])
        assert np.array_equal(_bits(one[0][0]), _bits(whole[0][f])) and np.array_equal(one[1][0], whole[1][f]), (shape, f)
    cut = 1 if F < 5 else 5                                                                     # cut into two calls
    parts = [ctx.pair_cost(np.ascontiguousarray(kp[a:z]), npers[a:z], cl[a:z], b["thr"]) for a, z in ((0, cut), (cut, F))]
    for k in range(2):
        assert np.array_equal(_bits(np.concatenate([p[k] for p in parts])), _bits(whole[k])), (shape, k, "cut")
    back = ctx.pair_cost(np.ascontiguousarray(kp[::-1]), np.ascontiguousarray(npers[::-1]), np.ascontiguousarray(cl[::-1]), b["thr"])
    assert np.array_equal(_bits(back[0][::-1]), _bits(whole[0])) and np.array_equal(back[1][::-1], whole[1])
    pad = 3                                                                                     # Pmax padded by unused slots (another tile, another wave count)
    kp2 = np.full((F, C, Pmax + pad, kn, 3), np.nan, dtype=kp.dtype)
    kp2[:, :, :Pmax] = kp
    cl2 = np.full((F, C, Pmax + pad), 5, dtype=np.int32)
    cl2[:, :, :Pmax] = cl
    wide = ctx.pair_cost(kp2, npers, cl2, b["thr"])
    ctx.close()
    assert np.array_equal(_bits(wide[0][:, :, :Pmax, :Pmax]), _bits(whole[0])) and np.array_equal(wide[1][:, :, :Pmax, :Pmax], whole[1])
    outside = np.ones((Pmax + pad, Pmax + pad), dtype=bool)
    outside[:Pmax, :Pmax] = False
    assert not wide[0][:, :, outside].any() and not wide[1][:, :, outside].any()


# ------------------------------------------------------------------------------------------------ k_seed_group against the rule
def _group_both(ctx, cs, cn, npers, cl, S, gate, min_views, device=False):
    want = sd.seed_persons_reference(cs, cn, npers, cl, S, gate, sc.MIN_JOINTS, min_views)
    if device:
        got = ctx.seed_persons(_dev(cs), _dev(cn), _dev(npers), _dev(cl), S=S, gate=gate, min_joints=sc.MIN_JOINTS, min_views=min_views, with_flags=True)
        got = tuple(a.cpu().numpy() for a in got)
    else:
        got = ctx.seed_persons(np.ascontiguousarray(cs), np.ascontiguousarray(cn), npers, cl, S=S, gate=gate, min_joints=sc.MIN_JOINTS,
                               min_views=min_views, with_flags=True)
    return got, want


def _assert_same(got, want, what):
    for g, w, name in zip(got, want, ("seed_det_of", "n_seeds", "flags")):
        assert g.shape == w.shape and g.dtype.itemsize == 4 and np.array_equal(_bits(g), _bits(w)), (what, name)


@pytest.mark.parametrize("size", sc.GROUP_SIZES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_seed_group_equals_the_rule_bit_for_bit(size):
    C, Pmax = size
    ctx = _rig_ctx(C)
    n = 12
    seeds = 0
    for name in sc.FAMILIES:
        cs, cn, npers, cl = sc.family(name, C, Pmax, n)
        for S in sc.slots(C, Pmax):
            for min_views in sorted({2, min(3, C)}):
                got, want = _group_both(ctx, cs, cn, npers, cl, S, sc.GATE, min_views, device=(S == 2))
                _assert_same(got, want, (size, name, S, min_views))
                seeds += int(want[1].sum())
                if name in ("floats", "ties") and S == 1 and C * Pmax >= 9:
                    assert (want[2] == sd.FLAG_FULL).any()
    assert seeds > 0
    # None for the lists: everything free
    cs, cn, _, _ = sc.family("floats", C, Pmax, n)
    got, want = _group_both(ctx, cs, cn, None, None, None, sc.GATE, 2)
    _assert_same(got, want, (size, "none"))


@pytest.mark.parametrize("size", [(4, 2), (3, 5), (8, 8)], ids=lambda s: f"{s[0]}x{s[1]}")
def test_a_frames_seeds_do_not_depend_on_the_call(size):
    C, Pmax = size
    ctx = _rig_ctx(C)
    n = 37
    for name in ("floats", "ties"):
        cs, cn, npers, cl = (np.array(a) for a in sc.family(name, C, Pmax, n))
        kw = dict(S=3, gate=sc.GATE, min_joints=sc.MIN_JOINTS, min_views=2, with_flags=True)
        whole = ctx.seed_persons(cs, cn, npers, cl, **kw)
        back = ctx.seed_persons(*(np.ascontiguousarray(a[::-1]) for a in (cs, cn, npers, cl)), **kw)
        parts = [ctx.seed_persons(*(np.ascontiguousarray(a[lo:hi]) for a in (cs, cn, npers, cl)), **kw) for lo, hi in ((0, 1), (1, 6), (6, n))]
        for k in range(3):
            assert np.array_equal(back[k][::-1], whole[k]), (size, name, k, "reversed")
            assert np.array_equal(np.concatenate([p[k] for p in parts]), whole[k]), (size, name, k, "cut")


@pytest.mark.parametrize("shape", [(4, 3, 133, 37), (8, 8, 65, 3), (3, 2, 63, 37)], ids=lambda s: "x".join(map(str, s)))
def test_seed_group_on_the_arrays_the_cost_kernel_wrote(shape):
    C, Pmax, kn, F = shape
    b = sc.batch(*shape)
    ctx = _batch_ctx(b)
    ps, pn = ctx.pair_cost(b["kpts"], b["n_persons"], b["claimed"], b["thr"])
    total = 0
    for gate, min_views in ((0.03, 3), (0.01, 2), (0.2, 2)):
        for S in (1, Pmax):
            got, want = _group_both(ctx, ps, pn, b["n_persons"], b["claimed"], S, gate, min_views)
            _assert_same(got, want, (shape, gate, min_views, S))
            total += int(want[1].sum())
    ctx.close()
    assert total > 0


# ------------------------------------------------------------------------------------------------ the chain
def test_triangulate_seeded_is_matched_triangulation_on_its_own_seeds():
    """crossing(), every detection free, on the device: the conditions of the host test hold, and the records are
    triangulate_matched on the seed_det_of the chain returned, bit for bit"""
    import torch
    cs = ac.crossing()
    ctx = _lib.Context(cs["K"], cs["R"], cs["t"])
    kp, npers = _dev(cs["kpts"]), _dev(cs["n_persons"])
    for gate in (0.02, 0.03, 0.05):
        out = sd.triangulate_seeded(ctx, kp, npers, None, S=4, gate=gate, keypoint_score_threshold=ac.CROSS_THRESHOLD, diagnostics=True)
        assert all(torch.is_tensor(v) and v.is_cuda for v in out.values())
        det, ns = out["seed_det_of"].cpu().numpy(), out["n_seeds"].cpu().numpy()
        assert (ns == 3).all() and not out["flags"].cpu().numpy().any()
        for f in range(ac.CROSS_F):
            assert {tuple(det[f, :, s]) for s in range(3)} == {tuple(cs["det_true"][f, :, p]) for p in range(3)}, (gate, f)
        again = ctx.triangulate_matched(kp, det_of=out["seed_det_of"], n_persons=npers, keypoint_score_threshold=ac.CROSS_THRESHOLD, diagnostics=True)
        for a, g in zip(again, (out["xyzs"], out["pscore"], out["views"], out["resid"])):
            assert np.array_equal(_bits(a.cpu().numpy()), _bits(g.cpu().numpy()))
        x = out["xyzs"].cpu().numpy()
        assert not x[:, 3].any()                                                                # the slot behind n_seeds: zero records
        truth = np.stack([[cs["X"][f, int(np.nonzero(cs["det_true"][f, 0] == det[f, 0, s])[0][0])] for s in range(3)] for f in range(ac.CROSS_F)])
        rms = float(np.sqrt(((x[:, :3, :, :3] - truth) ** 2).sum(-1).mean()))
        print(f"    gate {gate}: RMS against the truth {rms * 1e3:.2f} mm")
        assert rms < 0.02
    # the host path returns the same seeds and records
    host = sd.triangulate_seeded(ctx, np.array(cs["kpts"]), np.array(cs["n_persons"]), None, S=4, gate=0.05, keypoint_score_threshold=ac.CROSS_THRESHOLD)
    assert np.array_equal(host["seed_det_of"], det) and np.array_equal(_bits(host["xyzs"]), _bits(x))
    ref = sd.triangulate_seeded_reference(cs["K"], cs["R"], cs["t"], cs["kpts"][:6], cs["n_persons"][:6], None, 4, 0.05, 3, 8, ac.CROSS_THRESHOLD)
    assert np.array_equal(ref["seed_det_of"], det[:6]) and np.abs(ref["xyzs"] - x[:6]).max() < 1e-9
    ctx.close()


def test_two_persons_on_the_nudged_rig_on_the_device():
    r = pc.recipe(P=2)
    ctx = _lib.Context(r["K"], r["Rd"], r["td"])
    kp = _dev(r["kpts"])
    out = sd.triangulate_seeded(ctx, kp, None, None, S=2, gate=0.05)
    det, ns = out["seed_det_of"].cpu().numpy(), out["n_seeds"].cpu().numpy()
    assert (ns == 2).all() and (det >= 0).all() and (det == det[:, :1]).all() and (np.sort(det[:, 0], axis=-1) == [0, 1]).all()
    out = sd.triangulate_seeded(ctx, kp, None, None, S=2, gate=0.02)
    det, ns = out["seed_det_of"].cpu().numpy(), out["n_seeds"].cpu().numpy()
    others = np.delete(det, r["bad"], axis=1)
    assert (ns == 2).all() and (det[:, r["bad"]] == -1).all() and (others >= 0).all() and (others == others[:, :1]).all()
    ctx.close()
    tri = sd.seeded_triangulator(2, 0.05)
    x = tri(r["K"], r["Rd"], r["td"], r["kpts"][:5], None)
    want = sd.seeded_triangulator(2, 0.05, reference=True)(r["K"], r["Rd"], r["td"], r["kpts"][:5], None)
    assert x.shape == (5, 2, 17, 4) and x.dtype == np.float64 and np.abs(x - want).max() < 1e-9


# ------------------------------------------------------------------------------------------------ the C entries, the debug build
def test_entries_reject_bad_arguments_on_real_contexts(tmp_path):
    """tests/abi_badargs_seed.c against libsnowtri.so on the GPU: refusals before any launch, then one good call of each entry."""
    lib_dir = os.path.join(ROOT, "snowmocap_amd")
    exe = str(tmp_path / "abi_badargs_seed")
    subprocess.check_call(["gcc", "-std=c99", "-O1", "-I", os.path.join(ROOT, "include"), os.path.join(ROOT, "tests", "abi_badargs_seed.c"),
                           "-o", exe, "-L", lib_dir, "-lsnowtri", "-lm", "-Wl,-rpath," + lib_dir])
    out = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0 and "0 failure(s)" in out.stdout, out.stdout[-3000:] + out.stderr[-2000:]


DBG_CODE = r'''
import sys, numpy as np
sys.path.insert(0, %(root)r)
sys.path.insert(0, %(tests)r)
import seed_cases as sc
from snowmocap_amd import _lib
assert _lib.LIB_PATH.endswith("libsnowtri_dbg.so") and "SNOWTRI_DEBUG_BOUNDS" in _lib.build_info()["variants"]
ran = 0
for shape in sc.EXACT_SHAPES + sc.BATCH_SHAPES:
    C, Pmax, kn, F = shape
    b = sc.batch(*shape)
    ctx = _lib.Context(b["K"], b["R"], b["t"])
    ps, pn = ctx.pair_cost(b["kpts"], b["n_persons"], b["claimed"], b["thr"])
    for S in (1, C * Pmax):
        ctx.seed_persons(ps, pn, b["n_persons"], b["claimed"], S=S, gate=0.05, min_views=2, with_flags=True)
    n, first = ctx.debug_faults()
    assert n == 0, "device-side bounds check failed %%d times; first: code %%d at line %%d" %% (n, first >> 32, first & 0xffffffff)
    ran += 1
    ctx.close()
print("seed debug-bounds ok:", ran, "batches")
'''


def test_debug_bounds_on_the_batches():
    dbg = os.path.join(ROOT, "snowmocap_amd", "libsnowtri_dbg.so")
    assert os.path.exists(dbg), f"{dbg} is missing: `make -C snowmocap_amd/csrc debug`"
    env = dict(os.environ, SNOWTRI_LIB=dbg)
    p = subprocess.run([sys.executable, "-c", DBG_CODE % {"root": ROOT, "tests": os.path.join(ROOT, "tests")}], env=env, capture_output=True,
                       text=True, timeout=300)
    assert p.returncode == 0 and "seed debug-bounds ok" in p.stdout, (p.stdout[-2000:] + p.stderr[-3000:])
