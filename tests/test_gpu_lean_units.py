"""lean_item measures lengths in units of distance_threshold (the gate is n^2 > det, no product with the squared threshold;
snowtri_lean.hpp), and k_fused_lean_coop steps the byte offset of a lane's next fetch instead of reading it from a table in LDS.
What that could break, against the CPU oracle with the tolerances of tests/test_gpu_lean.py and test_gpu_lean_origin.py (counts
equal, scores <= 3e-7 relative, float32 joints <= 2e-6 m):

  * thresholds that are no power of two (default 0.05, 1e-3, 0.073, 0.5), on the floor rig and on the floor rig moved 47 m from
    the world origin, float32 keypoints (k_fused_lean_coop<4, float>: t' / lambda in registers) and float64 keypoints (t' / lambda
    from the kernel argument);
  * joints ON the gate: for a fifth of the joints one pair's distance is set to (1 +- 1e-6) x threshold by moving one pixel of
    float64 keypoints (Newton on the triple product, which is linear in the pixel); the float32 copy of the same keypoints lands
    where its pixels' spacing lets it, about 4e-7 m from there.  A flipped gate changes a joint's score by a whole pair's share,
    far outside the tolerance.  Joints with a pair within 1e-12 relative of the threshold (float64 model of the reference's
    formula) are left out of the comparison; they must be at most 0.1 % of the joints -- with these seeds there is none;
  * tiles of 1, 3, 19-20 and 32+ frames (F = 1, 3, 20, 33: the offset stream wraps from frame to frame inside the two fetches
    a wave has in flight, waves with and without a pass, the partial last pass), and one launch just above the cooperative
    limit (k_fused_lean), whose first frames are bit for bit what k_fused_lean_coop gives;
  * exact intersections and equal rays under a threshold that is no power of two: count and flags as the oracle's;
  * thresholds outside [2^-64, 2^64] m (zero, negative, denormal, huge, inf, NaN) leave the lean kernels for the route they
    took before there was a lean kernel, and match the oracle; the two ends of the range stay on the lean kernels.
"""
import numpy as np
import pytest

from conftest import assert_scores_close, assert_xyz_close
from test_gpu_lean_origin import FAR, J, XYZ_F32, _classes, _dyadic_fixture, _oracle, _run, api  # noqa: F401  (api: the fixture)

pytestmark = pytest.mark.gpu

THRESHOLDS = [0.05, 1e-3, 0.073, 0.5]
BAND = 1e-12            # |dist / threshold - 1| below this: the joint may fall on either side
COOP_FRAMES_PER_WG = 32  # kCoopMaxFrames
LEAN_WG_PER_CU = 2       # snowtri_ctx::lean_wg_per_cu


def _ray_matrices(K, R):
    return np.einsum("cij,cjk->cik", R, np.linalg.inv(K))


def _pair_list(C):
    return [(m, s) for m in range(C - 1) for s in range(m + 1, C)]


def _pair_distances(K, R, t, kp):
    """dist[F, pairs, J] of the skew rays of every camera pair, float64: |d . (h_m x h_s)| / |h_m x h_s|."""
    M = _ray_matrices(K, R)
    px = np.concatenate([kp[:, :, 0, :, :2].astype(np.float64), np.ones(kp.shape[:2] + (kp.shape[3], 1))], axis=-1)   # [F, C, J, 3]
    h = np.einsum("cik,fcjk->fcji", M, px)
    out = []
    for m, s in _pair_list(K.shape[0]):
        cr = np.cross(h[:, m], h[:, s])
        out.append(np.abs(cr @ (t[s] - t[m])) / np.sqrt((cr * cr).sum(-1)))
    return np.stack(out, axis=1)


def _seed_gate(rng, K, R, t, kp, dthr, share=0.2):
    """float64 keypoints, in place: for `share` of the joints the distance of one camera pair becomes (1 +- 1e-6) dthr, by moving
    one pixel coordinate of the pair's second camera.  Returns (frames, joints, pair indices, +1 / -1 side)."""
    assert kp.dtype == np.float64
    M = _ray_matrices(K, R)
    F, C = kp.shape[:2]
    key = np.unique(rng.integers(0, F * J, size=max(8, int(share * F * J))))
    f, j = key // J, key % J
    n = len(key)
    m = rng.integers(0, C - 1, size=n)
    s = rng.integers(m + 1, C)
    side = np.where(rng.random(n) < 0.5, 1.0, -1.0)
    target = (1.0 + side * 1e-6) * dthr
    d = t[s] - t[m]
    pm = np.concatenate([kp[f, m, 0, j, :2], np.ones((n, 1))], axis=1)
    hm = np.einsum("nik,nk->ni", M[m], pm)
    slope_u = (np.cross(hm, M[s][:, :, 0]) * d).sum(-1)     # d n / d u_s, d n / d v_s: n is linear in the pixel
    slope_v = (np.cross(hm, M[s][:, :, 1]) * d).sum(-1)
    use_v = np.abs(slope_v) >= np.abs(slope_u)
    slope = np.where(use_v, slope_v, slope_u)
    for _ in range(40):      # (fixed slope, the norm of the cross product moves with the pixel: linear convergence, slowest at 0.5 m)
        ps = np.concatenate([kp[f, s, 0, j, :2], np.ones((n, 1))], axis=1)
        cr = np.cross(hm, np.einsum("nik,nk->ni", M[s], ps))
        nn = (cr * d).sum(-1)
        step = (np.where(nn < 0, -1.0, 1.0) * target * np.sqrt((cr * cr).sum(-1)) - nn) / slope
        kp[f, s, 0, j, 1] += np.where(use_v, step, 0.0)
        kp[f, s, 0, j, 0] += np.where(use_v, 0.0, step)
    q = m * C - m * (m + 1) // 2 + (s - m - 1)       # index of (m, s) in _pair_list(C)
    return f, j, q, side


def _band(K, R, t, kp, dthr):
    """excluded[F, J]: a pair of the joint lies within BAND of the threshold (float64 model).  At most 0.1 % of the joints."""
    rel = np.abs(_pair_distances(K, R, t, kp) / dthr - 1.0)
    excluded = (rel < BAND).any(axis=1)
    assert excluded.mean() <= 1e-3, f"{excluded.sum()} of {excluded.size} joints within {BAND} of the threshold: another seed"
    return excluded


def _check(out, ref, frames, excluded, msg):
    """Counts, joint scores, joints and person scores of `frames` (indices into out / ref / excluded) against the oracle."""
    for f in frames:
        assert out["count"][f] == ref["count"][f], f"{msg} frame {f}: count {out['count'][f]} vs {ref['count'][f]}"
        if not ref["count"][f]:
            assert not out["xyzs"][f].any(), f"{msg} frame {f}: an empty frame must be zero-filled"
            continue
        keep = ~excluded[f]
        assert_scores_close(out["xyzs"][f, 0, keep, 3], ref["kscore"][f, 0, keep], rtol=3e-7, what=f"{msg} kscore frame {f}")
        assert_xyz_close(out["xyzs"][f, 0, keep, :3], ref["xyz"][f, 0, keep], XYZ_F32, score_ref=ref["kscore"][f, 0, keep],
                         what=f"{msg} xyz frame {f}")
        if keep.all():
            assert_scores_close(out["pscore"][f, :1], ref["pscore"][f, :1], rtol=3e-7, nterms=J, what=f"{msg} pscore frame {f}")


def _seeded_workload(F, far, dthr, seed, share=0.2):
    """Floor rig (moved by FAR with the scene if `far`), noisy float64 keypoints with gate seeds, thresholds with `dthr`."""
    from snowmocap_amd import synth
    rng = np.random.default_rng(seed)
    K, R, t = synth.load_rig_json()
    X = synth.make_people(rng, F, 1)
    if far:
        t, X = t + FAR, X + FAR
    kp, npers = synth.make_keypoints(rng, K, R, t, X, pixel_sigma=1.0, score_range=(2.0, 8.0), dtype=np.float64)
    seeds = _seed_gate(rng, K, R, t, kp, dthr, share)
    prm = dict(synth.default_thresholds(), distance_threshold=dthr)
    return K, R, t, kp, npers, prm, seeds


@pytest.mark.parametrize("far", [False, True], ids=["floor", "floor-moved"])
@pytest.mark.parametrize("F", [1, 3, 20, 33])
def test_thresholds_and_gate_against_oracle(api, F, far):
    """Every threshold, float64 keypoints (the seeds sit at (1 +- 1e-6) x threshold: checked in the model) and their float32 copy."""
    for dthr in THRESHOLDS:
        K, R, t, kp, npers, prm, (sf, sj, sq, side) = _seeded_workload(F, far, dthr, seed=int(1e6 * dthr) + 10 * F + far)
        dist = _pair_distances(K, R, t, kp)[sf, sq, sj]
        np.testing.assert_allclose(dist / dthr - 1.0, side * 1e-6, rtol=1e-4, atol=0, err_msg="the seeds are not on the gate")
        assert (side > 0).any() and (side < 0).any()
        for dtype, name in ((np.float64, "double"), (np.float32, "float")):
            kpd = kp.astype(dtype)
            msg = f"F={F} far={far} dthr={dthr} {name}"
            excluded = _band(K, R, t, kpd, dthr)
            ref = _oracle(K, R, t, kpd, npers, prm)
            out = _run(api, K, R, t, prm, kpd, npers)
            assert out["kernels"].startswith(f"k_fused_lean_coop<4,{name},133>"), (msg, out["kernels"])
            _check(out, ref, range(F), excluded, msg)


def test_launch_above_the_cooperative_limit(api):
    """One frame more than k_fused_lean_coop takes: k_fused_lean, float32 keypoints with gate seeds, threshold 0.073 on the moved
    rig.  Its first 513 frames are bit for bit what a 513-frame launch (the cooperative kernel) gives; a sample against the oracle."""
    import torch
    limit = torch.cuda.get_device_properties(0).multi_processor_count * LEAN_WG_PER_CU * COOP_FRAMES_PER_WG
    F = limit + 1
    K, R, t, kp, npers, prm, _ = _seeded_workload(F, True, 0.073, seed=4242, share=0.01)
    kp = kp.astype(np.float32)
    a = _run(api, K, R, t, prm, kp, npers)
    assert a["kernels"].startswith("k_fused_lean<4,float,133>"), a["kernels"]
    b = _run(api, K, R, t, prm, kp[:limit], npers[:limit])
    assert b["kernels"].startswith("k_fused_lean_coop<4,float,133>"), ("the limit is not what the context uses", b["kernels"])
    c = _run(api, K, R, t, prm, kp[:513], npers[:513])
    assert c["kernels"].startswith("k_fused_lean_coop<4,float,133>"), c["kernels"]
    for key in ("xyzs", "pscore", "count", "flags"):
        assert np.array_equal(a[key][:limit], b[key], equal_nan=True), f"{key} differs between the two kernels (tiles of 32)"
        assert np.array_equal(a[key][:513], c[key], equal_nan=True), f"{key} differs between the two kernels (tiles of 1-2)"
    rng = np.random.default_rng(1)
    check = sorted({0, 512, 513, limit - 1, limit} | set(int(x) for x in rng.choice(F, size=43, replace=False)))
    excluded = _band(K, R, t, kp[check], 0.073)
    ref = _oracle(K, R, t, kp[check], npers[check], prm)
    sub = {k: a[k][check] for k in ("xyzs", "pscore", "count")}
    _check(sub, ref, range(len(check)), excluded, "F=limit+1")


@pytest.mark.parametrize("C", [3, 5])
def test_three_and_five_cameras(api, C, knobs):
    """The instantiations that take t' / lambda from the kernel argument, both kernels: the same bits, and the oracle's results."""
    from snowmocap_amd import synth
    rng = np.random.default_rng(900 + C)
    F, dthr = 33, 0.073
    K, R, t = synth.ring_rig(C)
    t = t + FAR
    X = synth.make_people(rng, F, 1) + FAR
    kp, npers = synth.make_keypoints(rng, K, R, t, X, pixel_sigma=1.0, score_range=(2.0, 8.0), dtype=np.float64)
    _seed_gate(rng, K, R, t, kp, dthr)
    kp = kp.astype(np.float32)
    prm = dict(synth.default_thresholds(), distance_threshold=dthr)
    a = _run(api, K, R, t, prm, kp, npers)
    assert a["kernels"].startswith(f"k_fused_lean_coop<{C},float,133>"), a["kernels"]
    knobs.set("SNOWTRI_LEAN_COOP", "0")
    b = _run(api, K, R, t, prm, kp, npers)
    knobs.clear("SNOWTRI_LEAN_COOP")
    assert b["kernels"].startswith(f"k_fused_lean<{C},float,133>"), b["kernels"]
    for key in ("xyzs", "pscore", "count", "flags"):
        assert np.array_equal(a[key], b[key], equal_nan=True), f"C={C}: {key} differs between the two kernels"
    _check(a, _oracle(K, R, t, kp, npers, prm), range(F), _band(K, R, t, kp, dthr), f"C={C}")


@pytest.mark.parametrize("dthr", [0.75, 0.073, 3.0])
@pytest.mark.parametrize("kind", ["float32", "float64"])
def test_special_values_under_a_scaled_threshold(api, kind, dthr):
    """The dyadic fixture of test_gpu_lean_origin.py (exact intersections: n == 0 exactly, NaN pixels, NaN / negative / zero
    confidences; camera 0 off the origin) with thresholds other than 1: n / lambda is still exactly 0, the frames take the
    exact routine where they did, classes and counts are the oracle's."""
    K, R, t, kp, npers, prm = _dyadic_fixture(kind)
    prm = dict(prm, distance_threshold=dthr)
    ref = _oracle(K, R, t, kp, npers, prm, 32)
    out = _run(api, K, R, t, prm, kp, npers)
    assert out["kernels"].startswith("k_fused_lean_coop<4,"), out["kernels"]
    excluded = _band(K, R, t, kp, dthr)
    compared = blown = finite = 0
    for f in range(kp.shape[0]):
        if ref["status"][f] != 0:
            assert out["flags"][f] & 1, f
            continue
        assert out["count"][f] == ref["count"][f], f
        if not min(int(ref["count"][f]), 1):
            continue
        keep = ~excluded[f]
        g, o = out["xyzs"][f, 0, keep, 3].astype(np.float64), ref["kscore"][f, 0, keep]
        np.testing.assert_array_equal(_classes(g), _classes(o), err_msg=f"frame {f}")
        fin, zero = _classes(o) == 1, _classes(o) == 0
        np.testing.assert_allclose(g[fin], o[fin], rtol=1e-6, atol=1e-12, err_msg=f"frame {f}")
        gx, ox = out["xyzs"][f, 0, keep, :3], ref["xyz"][f, 0, keep]
        assert not gx[zero].any() and not ox[zero].any(), f
        np.testing.assert_allclose(gx[fin], ox[fin], rtol=1e-6, atol=2e-6, err_msg=f"frame {f}")
        blown += int((_classes(o) == 2).sum())
        finite += int(fin.sum())
        compared += 1
    assert compared >= 2 and blown > 0 and finite > 0, (compared, blown, finite)


def test_equal_rays_are_a_singular_pair(api):
    """Cameras 1 and 2 identical (det == 0 exactly, whatever the unit of length), threshold 0.073: the flag the oracle's status asks for."""
    from snowmocap_amd import synth
    rng = np.random.default_rng(812)
    F, C = 5, 4
    K, R, t = synth.ring_rig(C + 1)
    K, R, t = K[:C].copy(), R[:C].copy(), t[:C] + FAR
    K[2], R[2], t[2] = K[1], R[1], t[1]
    X = synth.make_people(rng, F, 1) + FAR
    kp, npers = synth.make_keypoints(rng, K, R, t, X, pixel_sigma=1.0)
    kp[:, 2] = kp[:, 1]
    prm = dict(synth.default_thresholds(), distance_threshold=0.073)
    ref = _oracle(K, R, t, kp, npers, prm, 4)
    out = _run(api, K, R, t, prm, kp, npers)
    assert out["kernels"].startswith("k_fused_lean_coop<4,float,133>"), out["kernels"]
    assert (ref["status"] != 0).any(), "the fixture holds no singular frame"
    for f in range(F):
        assert bool(out["flags"][f] & 1) == bool(ref["status"][f] != 0), (f, out["flags"][f], ref["status"][f])


@pytest.mark.parametrize("dthr,lean", [(2.0 ** -64, True), (2.0 ** 64, True), (2.0 ** -65, False), (2.0 ** 65, False), (0.0, False),
                                       (-1.0, False), (5e-324, False), (1e300, False), (float("inf"), False), (float("nan"), False)],
                         ids=lambda v: str(v))
def test_thresholds_outside_the_range_leave_the_lean_kernels(api, dthr, lean):
    """lean_units_ok: [2^-64, 2^64] m.  Inside, ends included, the lean kernel runs; outside the call takes k_fused_single as it
    would without a lean kernel.  Either way the oracle's results (a threshold of zero gates every pair, a huge one none)."""
    from snowmocap_amd import synth, _lib
    F = 20
    wl = synth.config_workload(2, F, seed=31)
    K, R, t = wl["rig"]
    t = t + FAR
    prm = dict(wl["params"], distance_threshold=dthr)
    out = _run(api, K, R, t, prm, wl["kpts"], wl["n_persons"])
    assert out["status"] == _lib.OK
    assert out["kernels"].startswith("k_fused_lean_coop<4,float,133>") == lean, out["kernels"]
    if not lean:
        assert out["kernels"].startswith("k_fused_single<4,0,float,float>"), out["kernels"]
    ref = _oracle(K, R, t, wl["kpts"], wl["n_persons"], prm)
    _check(out, ref, range(F), np.zeros((F, J), bool), f"dthr={dthr}")
