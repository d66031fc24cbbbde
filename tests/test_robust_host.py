"""method = DLT_ROBUST without a GPU: the rule itself (snowmocap_amd/robust.py, the NumPy definition the kernel is tested against) on
cases whose answer is known, its quality on the synthetic outlier recipe, the margin cap that keeps the GPU parity test honest, and
the new entry points of the C ABI."""
import ctypes as ct

import numpy as np
import pytest

import os

import robust_cases as rc
from conftest import ROOT
from snowmocap_amd import _lib, synth
from snowmocap_amd.robust import alternative_views, projection_matrices, triangulate_robust_reference
from oracle import dlt as odlt


def _exact_batch(name, F=2, J=6, seed=3, sigma=0.3, score=(4.0, 8.0)):
    K, R, t = rc.rig(name)
    rng = np.random.default_rng(seed)
    X = synth.make_people(rng, F, 1, J=J)
    kp, _ = synth.make_keypoints(rng, K, R, t, X, pixel_sigma=sigma, score_range=score, dtype=np.float64)
    return K, R, t, X, kp.copy()


def _ref(K, R, t, kp, npers=None, kthr=3.0, tau=6.0, max_drops=1):
    return triangulate_robust_reference(K, R, t, kp, npers, kthr, kp.shape[3], tau, max_drops)


def test_projection_matrices_are_the_dlt_definition():
    K, R, t = rc.rig("floor")
    assert np.array_equal(projection_matrices(K, R, t), odlt.projection_matrices(K, R, t))


@pytest.mark.parametrize("name", ["ring3", "floor", "ring8"])
def test_no_drop_allowed_is_the_dlt_oracle_exactly(name):
    b = rc.quality_batch(name)
    got = triangulate_robust_reference(b["K"], b["R"], b["t"], b["kpts"], None, rc.KTHR, 133, 6.0, 0)
    xyzs, pscore, count = odlt.dlt_batch(b["K"], b["R"], b["t"], b["kpts"], rc.KTHR, 133)
    assert np.array_equal(got["xyzs"], xyzs) and np.array_equal(got["pscore"], pscore) and np.array_equal(got["count"], count)
    assert (got["drops"] == 0).all() and (got["flags"] == _lib.FLAG_FASTPATH).all()
    # an infinite threshold drops nothing either
    inf = triangulate_robust_reference(b["K"], b["R"], b["t"], b["kpts"], None, rc.KTHR, 133, float("inf"), 3)
    assert np.array_equal(inf["xyzs"], xyzs) and (inf["drops"] == 0).all()


def test_two_views_drop_nothing_three_drop_to_two():
    K, R, t, X, kp = _exact_batch("ring2")
    kp[0, 1, 0, 2, 0] += 150.0
    r = _ref(K, R, t, kp, max_drops=6)
    assert (r["views"] == 3).all() and (r["drops"] == 0).all()
    assert r["resid"][0, 2] > 10.0                     # the error is there, and visible in the diagnostic
    K, R, t, X, kp = _exact_batch("ring3")
    kp[1, 2, 0, 4, 1] -= 150.0
    r = _ref(K, R, t, kp, max_drops=6)
    assert r["views"][1, 4] == 0b011 and r["drops"][1, 4] == 1
    assert np.linalg.norm(r["xyzs"][1, 0, 4, :3] - X[1, 0, 4]) < 0.02
    rest = np.ones((2, 6), bool)
    rest[1, 4] = False
    assert (r["views"][rest] == 0b111).all() and (r["drops"][rest] == 0).all()


def test_two_bad_cameras_of_eight_need_two_drops():
    K, R, t, X, kp = _exact_batch("ring8")
    kp[0, 1, 0, 3, 0] += 120.0
    kp[0, 6, 0, 3, 1] += 80.0
    one = _ref(K, R, t, kp, max_drops=1)
    two = _ref(K, R, t, kp, max_drops=2)
    six = _ref(K, R, t, kp, max_drops=6)
    assert one["drops"][0, 3] == 1 and bin(int(one["views"][0, 3])).count("1") == 7
    assert two["views"][0, 3] == 0xff & ~(1 << 1) & ~(1 << 6) and two["drops"][0, 3] == 2
    assert six["views"][0, 3] == two["views"][0, 3] and six["drops"][0, 3] == 2      # it stops when the residual is in
    assert np.linalg.norm(two["xyzs"][0, 0, 3, :3] - X[0, 0, 3]) < 0.01
    assert np.linalg.norm(one["xyzs"][0, 0, 3, :3] - X[0, 0, 3]) > np.linalg.norm(two["xyzs"][0, 0, 3, :3] - X[0, 0, 3])
    # resid is the RMS over the views that are left
    P = projection_matrices(K, R, t)
    Xh = np.append(two["xyzs"][0, 0, 3, :3], 1.0)
    r2 = []
    for c in (0, 2, 3, 4, 5, 7):
        p = P[c] @ Xh
        r2.append((p[0] / p[2] - kp[0, c, 0, 3, 0]) ** 2 + (p[1] / p[2] - kp[0, c, 0, 3, 1]) ** 2)
    assert two["resid"][0, 3] == pytest.approx(np.sqrt(np.mean(r2)), rel=1e-12)


def test_unlisted_and_score_gated_cameras_are_not_views():
    K, R, t, X, kp = _exact_batch("ring5")
    npers = np.ones((2, 5), np.int32)
    npers[1, 2] = 0
    kp[0, 4, 0, 1, 2] = 2.5                            # below kthr = 3
    kp[0, 0, 0, 5, 2] = np.nan                         # a NaN score is not below the threshold: the view counts (as in method = DLT)
    r = _ref(K, R, t, kp, npers)
    assert (r["views"][1] == 0b11011).all()
    assert r["views"][0, 1] == 0b01111 and r["views"][0, 5] == 0b11111 and np.isnan(r["xyzs"][0, 0, 5, 3])
    assert r["xyzs"][0, 0, 1, 3] == np.mean(kp[0, :4, 0, 1, 2])
    # fewer than two views: the zero record
    npers[1] = (0, 1, 0, 0, 0)
    r = _ref(K, R, t, kp, npers)
    assert (r["views"][1] == 0).all() and (r["xyzs"][1] == 0).all() and (r["resid"][1] == 0).all() and r["pscore"][1, 0] == 0.0
    assert r["count"][1] == 1
    # a gated camera is never a candidate: an outlier in it changes nothing
    kp2 = kp.copy()
    kp2[0, 4, 0, 1, 0] += 500.0
    r2 = _ref(K, R, t, kp2, npers)
    assert np.array_equal(r2["xyzs"][0, 0, 1], r["xyzs"][0, 0, 1]) and r2["views"][0, 1] == r["views"][0, 1]


def test_a_tie_goes_to_the_lower_camera(monkeypatch):
    """Two identical observations: leaving out either twin is the SAME subset problem (the same rows in the same order), so the two
    candidates tie exactly and the lower camera goes.  Then the selection on prescribed residuals (the solve replaced by a table):
    ties, a NaN candidate, nothing but NaN candidates."""
    from snowmocap_amd import robust
    K, R, t = (a.copy() for a in rc.rig("ring4"))
    K[3], R[3], t[3] = K[2], R[2], t[2]                # cameras 2 and 3 are one camera
    rng = np.random.default_rng(9)
    X = synth.make_people(rng, 1, 1, J=8)
    kp, _ = synth.make_keypoints(rng, K, R, t, X, pixel_sigma=0.5, score_range=(4.0, 8.0), dtype=np.float64)
    kp = kp.copy()
    kp[0, 3, 0, :, :2] = kp[0, 2, 0, :, :2]
    P = robust.projection_matrices(K, R, t)
    uv = np.ascontiguousarray(np.moveaxis(kp[:, :, 0, :, :2], 1, 2)).reshape(8, 4, 2)
    m2 = robust._solve(P, uv, np.full(8, 0b1011, np.uint32))[2]
    m3 = robust._solve(P, uv, np.full(8, 0b0111, np.uint32))[2]
    assert np.array_equal(m2, m3)                      # the tie is exact

    table = {}

    def fake_solve(P, uv, masks):
        n, C = uv.shape[:2]
        return np.zeros((n, 3)), np.zeros((n, C)), np.array([table[int(m)] for m in masks], dtype=np.float64)

    monkeypatch.setattr(robust, "_solve", fake_solve)
    nan = float("nan")

    def run(max_drops=1):
        return robust.triangulate_robust_reference(K, R, t, kp[:, :, :, :1], None, 3.0, 1, 6.0, max_drops)

    table.update({0b1111: 100.0, 0b1110: 50.0, 0b1101: 20.0, 0b1011: 20.0, 0b0111: 30.0})
    r = run()
    assert r["views"][0, 0] == 0b1101 and r["drops"][0, 0] == 1 and r["margin"][0, 0] == 0.0 and r["decision"][0, 0] == 1
    alt = robust.alternative_views(K, R, t, kp[:, :, :, :1], None, 3.0, 1, 6.0, 1, r)
    assert alt[0, 0] == 0b1011                         # the same decision taken the other way: the runner-up goes
    table.update({0b1110: nan, 0b1101: 70.0, 0b1011: 60.0, 0b0111: 60.0})
    r = run()
    assert r["views"][0, 0] == 0b1011                  # a NaN never wins against a number, and 60 == 60 goes to camera 2
    table.update({0b1110: nan, 0b1101: nan, 0b1011: nan, 0b0111: nan})
    r = run(max_drops=2)
    assert r["views"][0, 0] == 0b1110 and r["drops"][0, 0] == 1      # nothing but NaN: the lowest camera; a NaN m(S) ends the loop
    table.update({0b1111: 30.0})                       # below tau^2 = 36: nothing to do, and the margin says how close it was
    r = run()
    assert r["views"][0, 0] == 0b1111 and r["drops"][0, 0] == 0 and r["margin"][0, 0] == pytest.approx(6.0 / 36.0)


@pytest.mark.parametrize("name", ["ring4", "floor", "ring5", "ring8"])
def test_quality_on_the_outlier_recipe(name):
    b = rc.quality_batch(name)
    K, kp, cam, X = b["K"], b["kpts"], b["cam"], b["X"]
    C = K.shape[0]
    r = triangulate_robust_reference(b["K"], b["R"], b["t"], kp, None, rc.KTHR, 133, 6.0, C)
    passes = ~(kp[:, :, 0, :, 2].astype(np.float64) < rc.KTHR)             # [F, C, J]
    active = passes.sum(axis=1)
    full = np.zeros((12, 133), np.uint32)
    for c in range(C):
        full |= passes[:, c].astype(np.uint32) << np.uint32(c)
    shifted_counts = np.take_along_axis(passes, np.maximum(cam, 0)[:, None, :], axis=1)[:, 0] & (cam >= 0)
    sel = shifted_counts & (active >= 4)
    assert sel.sum() >= 50
    gone = ((r["views"] >> np.maximum(cam, 0).astype(np.uint32)) & 1) == 0
    err = np.linalg.norm(r["xyzs"][:, 0, :, :3] - X[:, 0], axis=-1)
    print(f"{name}: {sel.sum()} joints with a shifted view among >= 4, removed in {gone[sel].mean():.3f}, p95 {np.percentile(err[sel], 95):.4f} m, "
          f"max {err[sel].max():.4f} m, smallest margin {r['margin'].min():.3g}")
    assert gone[sel].mean() >= 0.95
    assert np.percentile(err[sel], 95) < 0.03
    clean = (cam < 0) & (active >= 2)
    assert clean.sum() > 1000 and (r["views"][clean] == full[clean]).all()


def test_margin_cap_on_every_gpu_input():
    """The GPU test demands equal masks only where the reference's margin is >= 1e-6: the share of joints it sets aside must stay
    small on every input it uses, or it would hide mask mismatches."""
    worst = 0.0
    for key, kn, tau, md in rc.gpu_cases():
        ref = rc.reference(key, kn, tau, md)
        share = float((ref["margin"] < 1e-6).mean())
        worst = max(worst, share)
        assert share <= 0.005, (key, kn, tau, md, share)
    print(f"largest share of joints with margin < 1e-6 over {len(rc.gpu_cases())} inputs: {worst:.4f}")


def test_diagnostics_refuse_what_their_entry_point_cannot_do():
    from snowmocap_amd.batch import BatchTriangulator
    K, R, t = rc.rig("ring4")
    for kw in (dict(zero_fill=False), dict(streams=2)):
        with pytest.raises(ValueError):               # (raised before a context is made: no GPU needed)
            BatchTriangulator(K, R, t, synth.default_thresholds(), method=_lib.DLT_ROBUST, diagnostics=True, **kw)


def test_new_entry_points_exist_and_reject_a_null_context():
    L = _lib.lib()
    handle = ct.CDLL(_lib.LIB_PATH)
    assert hasattr(handle, "snowtri_triangulate_robust") and hasattr(handle, "snowtri_ctx_set_robust")
    assert _lib.DLT_ROBUST == 2
    assert L.snowtri_ctx_set_robust(None, 6.0, 1) == _lib.ERR_BAD_ARG
    prm = _lib.make_params(keypoint_num=4, center_point_index=0)
    buf = np.zeros(64)
    cnt = np.zeros(4, np.int32)
    rc_ = L.snowtri_triangulate_robust(None, 1, 4, _lib.ptr(buf), _lib.F64, None, prm, 6.0, 1, 1, _lib.ptr(buf), None, _lib.F64,
                                       _lib.ptr(cnt), None, None, None, _lib.HOST, None)
    assert rc_ == _lib.ERR_BAD_ARG
    hdr = open(os.path.join(ROOT, "include", "snowtri.h")).read()
    assert "SNOWTRI_DLT_ROBUST = 2" in hdr and "synthetic" in hdr.lower()
