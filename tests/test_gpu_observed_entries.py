"""Every route through the host layer under the four entries that take joint records and per-camera detections (snowtri.hip:
with_float_pair, ObservedInputs): snowtri_reproject, snowtri_reproject_cost, snowtri_refine_joints, snowtri_refine_cameras, each with
the four pairs of (records dtype, second dtype), on HOST arrays and on DEVICE tensors, with det_of / n_persons / views given and
left out, on a 4-camera, a 5-camera and an 8-camera rig (k_refine<4>, k_refine<0>, k_refine<8>).

Every input value is rounded to float32 first and then held as float32 or as float64, so the eight runs of an entry are given the
same numbers.  The kernels convert every load to double and run with fp contract(off), so
  * the float64 and integer outputs (cost, codes, cost_sum, cost_n, R, t, the report) have the same bits in all eight runs;
  * the typed outputs of a float32 run (the refined records, pix) are the float64 run's output cast to float32, exactly.
F = 3, P = 2, Pmax = 3, kn = 5; detections are the projections + N(0, 1 px); one record is missing (score 0); no NaN.
"""
import functools
import itertools

import numpy as np
import pytest

import refine_cases as rc
from snowmocap_amd import _lib, pose, refine, synth

pytestmark = pytest.mark.gpu

F, P, PMAX, KN = 3, 2, 3, 5
THR = 0.5
RIGS = ("floor", "ring5", "ring8")                     # 4, 5 and 8 cameras
PAIRS = tuple(itertools.product(("float32", "float64"), repeat=2))
SPACES = ("host", "device")


@pytest.fixture(scope="module")
def api():
    import snowmocap_amd as sm
    assert _lib.lib().snowtri_device_count() > 0, "these tests need the HIP device"
    return sm


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view({8: np.uint64, 4: np.uint32, 1: np.uint8}[a.dtype.itemsize])


def _same_bits(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and np.array_equal(_bits(a), _bits(b))


@functools.lru_cache(maxsize=None)
def inputs(rig_name, given):
    """-> dict(K, R, t, xyzs [F, P, kn, 4], kpts [F, C, Pmax, kn, 3]: float64 arrays of float32 values, det_of / n_persons / views:
    arrays (given) or None); read-only.  With the lists given every camera's list is permuted, one det_of entry is -1, one n_persons
    cuts its list short and `views` takes a camera away from some records; without them detection p is person p."""
    K, R, t = rc.rig(rig_name)
    C = K.shape[0]
    rng = np.random.default_rng(rc._seed("observed", rig_name, given))
    X = synth.make_people(rng, F, P, J=KN)
    xyzs = np.concatenate([X, rng.uniform(0.5, 9.0, (F, P, KN, 1))], axis=-1)
    xyzs[1, 1, 2, 3] = 0.0                                                                   # a missing record
    uv = np.moveaxis(synth.project(K, R, t, X)[0], 0, 1) + rng.normal(0.0, 1.0, (F, C, P, KN, 2))
    sc = rng.uniform(0.6, 2.0, (F, C, P, KN))
    sc[rng.random(sc.shape) < 0.1] = 0.25                                                    # below the threshold
    kpts = np.empty((F, C, PMAX, KN, 3))
    kpts[..., :2], kpts[..., 2] = rng.uniform(0.0, 1280.0, (F, C, PMAX, KN, 2)), rng.uniform(0.6, 2.0, (F, C, PMAX, KN))
    det_of = n_persons = views = None
    if given:
        det_of = np.empty((F, C, P), dtype=np.int64)
        for f in range(F):
            for c in range(C):
                slots = rng.permutation(PMAX)[:P]                                            # person p stands in slot slots[p]
                kpts[f, c, slots, :, :2], kpts[f, c, slots, :, 2] = uv[f, c], sc[f, c]
                det_of[f, c] = slots
        det_of[0, 1, 0] = -1
        n_persons = np.full((F, C), PMAX, dtype=np.int32)
        n_persons[2, 0] = PMAX - 1
        views = np.full((F, P, KN), 0xffffffff, dtype=np.uint32)
        views[:, :, ::2] &= ~(np.uint32(1) << rng.integers(0, C, (F, P, (KN + 1) // 2)).astype(np.uint32))
    else:
        kpts[:, :, :P, :, :2], kpts[:, :, :P, :, 2] = uv, sc
    out = dict(K=K, R=R, t=t, xyzs=xyzs.astype(np.float32).astype(np.float64), kpts=kpts.astype(np.float32).astype(np.float64),
               det_of=det_of, n_persons=n_persons, views=views)
    for a in out.values():
        if isinstance(a, np.ndarray):
            a.setflags(write=False)
    return out


def _runs(rig_name, given, call):
    """call(ctx, xyzs, kpts, lists, second) -> a tuple of arrays, for the four dtype pairs in both spaces -> {(records dtype, second
    dtype, space): the tuple as NumPy arrays}.  kpts is held in the second dtype; lists = dict(det_of, n_persons, views) in the
    space's own kind."""
    import torch
    d = inputs(rig_name, given)
    ctx = _lib.Context(d["K"], d["R"], d["t"])
    got = {}
    try:
        for (xd, sd), space in itertools.product(PAIRS, SPACES):
            xyzs, kpts = d["xyzs"].astype(xd), d["kpts"].astype(sd)
            lists = dict(det_of=d["det_of"], n_persons=d["n_persons"], views=d["views"])
            if space == "device":
                dev = lambda a: None if a is None else torch.from_numpy(np.array(a)).to("cuda:0")
                xyzs, kpts = dev(xyzs), dev(kpts)
                lists = dict(det_of=dev(d["det_of"]), n_persons=dev(d["n_persons"]), views=dev(None if d["views"] is None else d["views"].view(np.int32)))
            res = call(ctx, xyzs, kpts, lists, sd)
            if space == "device":
                torch.cuda.synchronize()
                res = tuple(a.cpu().numpy() for a in res)
            got[(xd, sd, space)] = res
    finally:
        ctx.close()
    return got


def _assert_same_everywhere(got, names, typed=(), typed_by=0):
    """Output k of every run has the bits of the (float64, float64, host) run's -- cast to float32 first where k is in `typed` and the
    run's records (typed_by = 0) or its second dtype (typed_by = 1) are float32."""
    want = got[("float64", "float64", "host")]
    for key, res in got.items():
        assert len(res) == len(names)
        for k, name in enumerate(names):
            ref = want[k].astype(np.float32) if k in typed and key[typed_by] == "float32" else want[k]
            assert _same_bits(res[k], ref), (name,) + key


CASES = [(r, g) for r in RIGS for g in (True, False)]


@pytest.mark.parametrize("rig_name", RIGS)
def test_reproject_is_one_computation_for_every_dtype_pair_and_space(api, rig_name):
    """(records dtype, pix dtype): pix in float64 has the same bits from float32 and from float64 records, on the host and on the
    device; pix in float32 is that array cast.  (The entry takes no detections: the lists do not reach it.)"""
    def call(ctx, xyzs, kpts, lists, pix_dtype):
        return (ctx.reproject(xyzs, dtype=pix_dtype),)
    got = _runs(rig_name, False, call)
    pix = got[("float64", "float64", "host")][0]
    assert pix.shape == (F, rc.rig(rig_name)[0].shape[0], P, KN, 3) and pix.dtype == np.float64
    assert (pix[1, :, 1, 2] == 0).all() and (pix[0, :, 0, :, 2] > 0).all()                    # the missing record; valid projections
    _assert_same_everywhere(got, ("pix",), typed=(0,), typed_by=1)


@pytest.mark.parametrize("rig_name,given", CASES)
def test_reproject_cost_is_one_computation_for_every_dtype_pair_and_space(api, rig_name, given):
    def call(ctx, xyzs, kpts, lists, _):
        return ctx.reproject_cost(xyzs, kpts, n_persons=lists["n_persons"], keypoint_score_threshold=THR)
    got = _runs(rig_name, given, call)
    cost_sum, cost_n = got[("float64", "float64", "host")]
    assert cost_sum.dtype == np.float64 and cost_n.dtype == np.int32 and (cost_n > 0).sum() > cost_n.size // 2
    _assert_same_everywhere(got, ("cost_sum", "cost_n"))


@pytest.mark.parametrize("rig_name,given", CASES)
def test_refine_joints_is_one_computation_for_every_dtype_pair_and_space(api, rig_name, given):
    def call(ctx, xyzs, kpts, lists, _):
        return ctx.refine_joints(xyzs, kpts, keypoint_score_threshold=THR, iters=4, diagnostics=True, **lists)
    got = _runs(rig_name, given, call)
    out, cost, codes = got[("float64", "float64", "host")]
    assert codes[1, 1, 2] == refine.REFINE_MISSING and (codes == refine.REFINE_MISSING).sum() == 1
    assert (codes == refine.REFINE_MOVED).sum() >= codes.size // 2 and (cost[..., 1] <= cost[..., 0]).all()
    _assert_same_everywhere(got, ("records", "cost", "codes"), typed=(0,))


@pytest.mark.parametrize("rig_name,given", CASES)
def test_refine_cameras_is_one_computation_for_every_dtype_pair_and_space(api, rig_name, given):
    C = rc.rig(rig_name)[0].shape[0]

    def call(ctx, xyzs, kpts, lists, _):
        R, t, rep = ctx.refine_cameras(xyzs, kpts, keypoint_score_threshold=THR, free=list(range(1, C)), min_obs=3, iters=4,
                                       diagnostics=True, **lists)
        return R, t, rep["cost"], rep["n_obs"], rep["codes"], rep["normal"]
    got = _runs(rig_name, given, call)
    R, t, cost, n_obs, codes, normal = got[("float64", "float64", "host")]
    assert codes[0] == pose.POSE_FIXED and _same_bits(R[0], np.ascontiguousarray(rc.rig(rig_name)[1][0]))
    assert (codes[1:] == pose.POSE_MOVED).all() and (n_obs >= 3 * KN).all() and (cost[1:, 1] < cost[1:, 0]).all()
    _assert_same_everywhere(got, ("R", "t", "cost", "n_obs", "codes", "normal"))
