"""k_fused_lean_coop<4, float, 133> holds the rig constants (ray matrices M, camera centres t, the first pair offsets) in
registers across its item loop; k_fused_lean and the other rigs read them from LDS item by item.  Same arithmetic either
way: a frame's bits must not depend on which kernel ran it, on the cut of the batch into launches, or on the run.

The product library decides the kernel by launch size (k_fused_lean_coop up to 32 frames per resident workgroup, 16 384
frames on an MI355X); the test build (conftest.Knobs) forces the wave-autonomous kernel with SNOWTRI_LEAN_COOP=0.
"""
import numpy as np
import pytest

from conftest import assert_scores_close, assert_xyz_close

pytestmark = pytest.mark.gpu

KEYS = ("xyzs", "pscore", "count", "flags")
COOP_MAX = 16384


@pytest.fixture(scope="module")
def api():
    import snowmocap_amd as sm
    from snowmocap_amd import _lib
    assert _lib.lib().snowtri_device_count() > 0, "these tests need the HIP device"
    return sm


def _run(api, K, R, t, prm, kp, npers):
    bt = api.BatchTriangulator(K, R, t, prm, pout_max=1, out_dtype=np.float32)
    out = bt.run_host(kp, npers)
    out["kernel"] = bt.ctx.last_kernel_names()
    bt.close()
    return out


def _same(a, b, msg):
    for key in KEYS:
        assert np.array_equal(a[key], b[key], equal_nan=True), f"{msg}: {key} differs"


def _run_cut(api, K, R, t, prm, kp, npers, step):
    """The batch in launches of `step` frames, outputs concatenated."""
    parts = [_run(api, K, R, t, prm, kp[s:s + step], npers[s:s + step]) for s in range(0, kp.shape[0], step)]
    return {key: np.concatenate([p[key] for p in parts]) for key in KEYS}


@pytest.mark.parametrize("F", [1, 31, 32, 33, 4000, 10000, 40000])
def test_four_cameras_resident_constants_same_bits_every_kernel(api, F, knobs):
    """4 cameras x 1 person (the bench's shape): two runs give the same bits; the other kernel gives the same bits
    (F <= 16 384: the wave-autonomous kernel forced; F = 40 000: k_fused_lean_coop on launches of 10 000 frames); frames
    that fall back are part of the batch; a sample agrees with the oracle."""
    from snowmocap_amd import synth
    from oracle import oracle as orc
    rng = np.random.default_rng(7100 + F)
    wl = synth.config_workload(2, F, seed=5)
    K, R, t = wl["rig"]
    prm = wl["params"]
    kp, npers = wl["kpts"].copy(), wl["n_persons"].copy()
    if F >= 2:
        kp[F - 1, 1, 0, :, :2] += 400.0                   # a frame the single-cluster check sends to the exact routine
    if F >= 33:
        kp[F // 2, 3, 0, 10, 0] = np.nan                  # an item that reports `bad` from the item loop
    a = _run(api, K, R, t, prm, kp, npers)
    b = _run(api, K, R, t, prm, kp, npers)
    _same(a, b, f"F={F}: second run")
    if F <= COOP_MAX:
        assert a["kernel"].startswith("k_fused_lean_coop<4,float,133>"), a["kernel"]
        knobs.set("SNOWTRI_LEAN_COOP", "0")
        c = _run(api, K, R, t, prm, kp, npers)
        knobs.clear("SNOWTRI_LEAN_COOP")
        assert c["kernel"].startswith("k_fused_lean<4,float,133>"), c["kernel"]
    else:
        assert a["kernel"].startswith("k_fused_lean<4,float,133>"), a["kernel"]
        c = _run_cut(api, K, R, t, prm, kp, npers, 10000)
    _same(a, c, f"F={F}: the other kernel")
    check = sorted(set(rng.choice(F, size=min(F, 16), replace=False).tolist()) | {0, F - 1, F // 2})
    ref = orc.triangulate_condense_batch(K, R, t, kp[check], npers[check], orc.make_params(**prm), 1)
    for i, f in enumerate(check):
        assert a["count"][f] == ref["count"][i], f"F={F} frame {f}: count"
        if ref["count"][i]:
            assert_scores_close(a["xyzs"][f, :1, :, 3], ref["kscore"][i, :1], rtol=3e-7, what=f"F={F} kscore frame {f}")
            assert_xyz_close(a["xyzs"][f, :1, :, :3], ref["xyz"][i, :1], 2e-6, score_ref=ref["kscore"][i, :1],
                             what=f"F={F} xyz frame {f}")


@pytest.mark.parametrize("C", [3, 5])
def test_three_and_five_cameras_coop_same_bits_as_autonomous_kernel(api, C, knobs):
    """The other rigs of the unrolled item (3 and 5 cameras, float32 outputs) keep reading the constants from LDS in both
    kernels, through the same lean_item: k_fused_lean_coop and the forced wave-autonomous kernel give the same bits."""
    from snowmocap_amd import synth
    rng = np.random.default_rng(7200 + C)
    K, R, t = synth.ring_rig(C)
    F = 2000
    X = synth.make_people(rng, F, 1)
    kp, npers = synth.make_keypoints(rng, K, R, t, X, pixel_sigma=1.0, score_range=(2.0, 8.0), dtype=np.float32)
    prm = dict(synth.default_thresholds(), condense_distance_tol=0.5)
    a = _run(api, K, R, t, prm, kp, npers)
    assert a["kernel"].startswith(f"k_fused_lean_coop<{C},float,133>"), a["kernel"]
    knobs.set("SNOWTRI_LEAN_COOP", "0")
    c = _run(api, K, R, t, prm, kp, npers)
    knobs.clear("SNOWTRI_LEAN_COOP")
    assert c["kernel"].startswith(f"k_fused_lean<{C},float,133>"), c["kernel"]
    _same(a, c, f"C={C}")
