"""TrackPipeline.run with its options COMBINED, every stage held to its rule (tests/pipeline_cases.py: the scenes, the chained NumPy
rule, the stage-wise check and where each bound comes from; tests/test_pipeline_rules_host.py shows on the CPU that the scenes reach
the edges and that the check rejects seven planted mistakes).

One check_stages per case of pipeline_cases.CASES: refine -> track -> despike -> fill -> N1 -> control points -> N2 -> reproject as one
chain on the permuted walk (ragged="track": all four options, without the fill (REPLACE), without the despike, track_max_missed = 2),
the ordered walk by list index (ragged="reference": the slot-by-slot branch with despike, alone and with everything), two persons in
fixed slots (with and without the host check), the lens (raw pixels, D), keypoint_num = 130 < J, and the DLT methods.  Every figure
is printed per stage and the misses of a case are raised together.

Then, on the walk with everything on, the result is bit for bit the same from NumPy or CUDA-tensor inputs, after another recording
went through the same TrackPipeline, on a side stream, with reproject=None (every other key), and through the bounds-checked test
build of the library, which counts no fault.
"""
import os

import numpy as np
import pytest

import pipeline_cases as pc
from snowmocap_amd import _lib

pytestmark = pytest.mark.gpu

WALK_ALL = "walk-track-all"


@pytest.fixture(scope="module")
def api():
    import snowmocap_amd as sm
    assert _lib.lib().snowtri_device_count() > 0, "these tests need the HIP device"
    return sm


def _pipeline(api, sc, opts):
    K, R, t = sc["rig"]
    return api.TrackPipeline(K, R, t, sc["params"], pc.SMOOTH_PROFILE, n_persons_out=sc["slots"], D=sc["D"], method=opts["method"])


def _run(pipe, sc, opts, kpts=None, n_persons=None):
    import torch
    # (the scenes are shared and read-only: the pipeline gets its own copy)
    res = pipe.run(np.array(sc["kpts"]) if kpts is None else kpts, np.array(sc["n_persons"]) if n_persons is None else n_persons, check=opts["check"],
                   ragged=opts["ragged"], track_gate=pc.TRACK_GATE, track_max_missed=opts["track_max_missed"], fill_gaps=opts["fill_gaps"],
                   despike=opts["despike"], reproject=opts["reproject"], refine=opts["refine"])
    torch.cuda.synchronize()
    return {k: v.cpu().numpy() for k, v in res.items()}


@pytest.fixture(scope="module")
def results(api):
    """case id -> (result, result with refine=None), each computed once"""
    cache = {}

    def get(cid):
        if cid not in cache:
            sc, opts = pc.case(cid)
            pipe = _pipeline(api, sc, opts)
            try:
                cache[cid] = (_run(pipe, sc, opts), _run(pipe, sc, dict(opts, refine=None)))
            finally:
                pipe.close()
        return cache[cid]
    return get


def _assert_same_bits(got, want, what, skip=()):
    assert list(got) == [k for k in want if k not in skip], (what, list(got), list(want))
    for k in got:
        a, b = np.ascontiguousarray(got[k]), np.ascontiguousarray(want[k])
        assert a.dtype == b.dtype and a.shape == b.shape and np.array_equal(a.view(np.uint8), b.view(np.uint8)), f"{what}: {k} differs"


# ------------------------------------------------------------------------------------------------ every stage against its rule
@pytest.mark.parametrize("cid", list(pc.CASES))
def test_every_stage_against_its_rule(api, results, cid):
    sc, opts = pc.case(cid)
    res, plain = results(cid)
    st = pc.check_stages(res, plain, sc, opts, what=cid)
    assert len(st.worst) >= 8
    # the options did something: what the rules' own run shows (tests/test_pipeline_rules_host.py) happened on the GPU too
    if opts["despike"]:
        assert (res["spike_codes"] == pc.DESPIKE_SPIKE).sum() >= 2
    if opts["fill_gaps"]:
        assert set(np.unique(res["fill"]).tolist()) >= {pc.FILL_LERP, pc.FILL_HOLD, pc.FILL_MISSING}
    if opts["ragged"] == "track":
        tid = res["track_id"]
        assert max(len(np.unique(tid[:, i][tid[:, i] >= 0])) for i in range(sc["slots"])) >= 2


# ------------------------------------------------------------------------------------------------ one result, however it is asked for
def test_numpy_and_tensor_inputs_give_the_same_bits(api, results):
    import torch
    sc, opts = pc.case(WALK_ALL)
    want, _ = results(WALK_ALL)
    pipe = _pipeline(api, sc, opts)
    kp, npers = torch.from_numpy(np.array(sc["kpts"])).cuda(), torch.from_numpy(np.array(sc["n_persons"])).cuda()
    keep = kp.clone()
    got = _run(pipe, sc, opts, kp, npers)
    pipe.close()
    _assert_same_bits(got, want, "CUDA-tensor inputs")
    assert torch.equal(kp, keep), "the caller's keypoints were written"


def test_no_state_survives_a_call(api, results):
    """The same TrackPipeline: the walk, then 40 frames of two other persons, then the walk again."""
    sc, opts = pc.case(WALK_ALL)
    other = pc.scene("fixed", False)
    want, _ = results(WALK_ALL)
    pipe = _pipeline(api, sc, opts)
    first = _run(pipe, sc, opts)
    between = _run(pipe, sc, opts, np.array(other["kpts"][:40]), np.array(other["n_persons"][:40]))
    again = _run(pipe, sc, opts)
    pipe.close()
    assert between["xyzs"].shape[0] == 40 and (between["count"] == 2).all() and (between["tracked"] == 2).all()
    _assert_same_bits(first, want, "first run")
    _assert_same_bits(again, want, "the run after another recording")


def test_a_side_stream_gives_the_same_bits(api, results):
    import torch
    sc, opts = pc.case(WALK_ALL)
    want, _ = results(WALK_ALL)
    pipe = _pipeline(api, sc, opts)
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
        got = _run(pipe, sc, opts)
    pipe.close()
    _assert_same_bits(got, want, "side stream")


def test_reproject_none_changes_no_other_key(api, results):
    sc, opts = pc.case(WALK_ALL)
    want, _ = results(WALK_ALL)
    pipe = _pipeline(api, sc, opts)
    got = _run(pipe, sc, dict(opts, reproject=None))
    pipe.close()
    added = ("det_of", "shared", "view_rms", "view_n")
    assert all(k in want for k in added)
    _assert_same_bits(got, want, "reproject=None", skip=added)


def test_the_bounds_checked_build_gives_the_same_bits_and_counts_no_fault(api, results):
    sc, opts = pc.case(WALK_ALL)
    want, _ = results(WALK_ALL)
    assert os.path.exists(_lib.TEST_LIB_PATH), "build the test library: make -C snowmocap_amd/csrc debug"
    prev = _lib.use_library(_lib.TEST_LIB_PATH)
    try:
        assert "SNOWTRI_DEBUG_BOUNDS" in _lib.build_info()["variants"]
        pipe = _pipeline(api, sc, opts)
        ctx = pipe.bt.ctx
        assert ctx.debug_faults()[0] == 0
        got = _run(pipe, sc, opts)
        n, first = ctx.debug_faults()
        pipe.close()
        assert n == 0, f"device-side bounds check failed {n} times; first: code {first >> 32} at line {first & 0xffffffff}"
    finally:
        _lib.use_library(prev)
    assert not _lib.LIB_PATH.endswith("_dbg.so")
    _assert_same_bits(got, want, "bounds-checked build")
