"""Every route of method = DLT and method = DLT_ROBUST wherever the rig stands in the world: the same rig and the SAME pixels at the
six placements of tests/dlt_frames_cases.py (metres / millimetres; at the origin, 47 m out, in site coordinates 1 km out), and a
rig with per-camera intrinsics (fx 600-3000, principal points off centre, a skew term) at home and at mm-moved.

The methods solve in the rig's own frame (include/snowtri.h, SNOWTRI_DLT; oracle/dlt.py), s = the rig scale of that definition
(4.5 u on the ring rigs).  At every placement:
  * float64 outputs within 2.5e-10 s of the oracle at that placement (+ 1e-9 of what |xyz - c| exceeds s by: a ghost cluster of two
    nearly parallel rays lies kilometres out) -- on the 4.5 m ring the suite's 1e-9 m, in rig units so that it means the same in mm;
    float32 outputs within XYZ_F32 s / 4.5 + one float32 ulp of the stored value; scores as test_dlt_wide_rigs (rtol 1e-6) and
    test_dlt_multi_person_against_oracle (rtol 1e-12, float64 in and out) have them; counts equal;
  * equivariance: xyz / u - D within twice that bound of the home output; masks, counts equal, robust resid within 2e-6 px;
  * joints within 0.05 u of the placed truth (a kernel that forgets to add the centre back fails loudly);
  * a joint nobody sees stays (0, 0, 0, 0), not the rig's centre;
  * k_dlt_coop<C> and k_fused_single<C,1> give identical bits.
Each test prints its figures per placement and fails at the end, naming every placement that missed.
"""
import numpy as np
import pytest

import dlt_frames_cases as fc
import robust_cases as rc
from snowmocap_amd import _lib, synth
from snowmocap_amd.robust import alternative_views

pytestmark = pytest.mark.gpu

XYZ_F32 = 2e-6              # tests/test_gpu_parity.py: float32 rounding of ~5 m coordinates, on the 4.5 m ring
XYZ_F64 = 2.5e-10           # x s
MARGIN = 1e-6               # tests/test_gpu_robust.py
NOISE = 0.5


@pytest.fixture(scope="module")
def api():
    import snowmocap_amd as sm
    assert _lib.lib().snowtri_device_count() > 0, "these tests need the HIP device"
    return sm


def K_count(rig_name):
    return fc.rig(rig_name)[0].shape[0]


def _placements(rig_name):
    return fc.MIXED_PLACEMENTS if rig_name.startswith("mixed") else tuple(fc.PLACEMENTS)


def _run(api, K, R, t, prm, kp, npers, out_dtype, pout=1, method=_lib.DLT, **kw):
    bt = api.BatchTriangulator(K, R, t, prm, pout_max=pout, out_dtype=out_dtype, method=method, **kw)
    try:
        out = bt.run_host(kp, npers)
        out["kernels"] = bt.ctx.last_kernel_names()
    finally:
        bt.close()
    assert out["status"] == _lib.OK
    return out


def _tolerance(want_xyz, t, out_dtype, factor=1.0):
    """The bound of the module docstring around `want_xyz` (world coordinates of the placement), elementwise."""
    from oracle import dlt as odlt
    c, s = odlt.rig_frame(t)
    if np.dtype(out_dtype) == np.float64:
        beyond = np.maximum(0.0, np.linalg.norm(want_xyz - c, axis=-1) - s)[..., None]
        return factor * (XYZ_F64 * s + 1e-9 * beyond) + 0.0 * want_xyz
    return factor * (XYZ_F32 * s / 4.5 + 2.0 ** -23 * np.abs(want_xyz))


class Report:
    """Figures per placement, printed as they come; the failures are raised together at the end."""

    def __init__(self, what):
        self.what, self.failed = what, []

    def check(self, ok, placement, msg):
        if not ok:
            self.failed.append(f"{placement}: {msg}")

    def bound(self, placement, label, err, tol, u):
        """err, tol: arrays of one shape.  Prints the largest error (in metres too) and records a miss."""
        err, tol = np.asarray(err, float), np.asarray(tol, float)
        if err.size == 0:
            return
        bad = ~(err <= tol)
        k = int(np.argmax(np.where(np.isfinite(err), err / tol, np.inf)))
        print(f"    {self.what} [{placement}] {label}: max |err| = {np.nanmax(err):.3e} ({np.nanmax(err) / u:.3e} m), worst err / bound = "
              f"{err.ravel()[k] / tol.ravel()[k]:.3g}, {int(bad.sum())} of {err.size} over")
        self.check(not bad.any(), placement, f"{label}: {int(bad.sum())} of {err.size} over the bound, worst err / bound = {err.ravel()[k] / tol.ravel()[k]:.3g}, "
                                             f"max |err| = {np.nanmax(err):.3e} ({np.nanmax(err) / u:.3e} m)")

    def finish(self):
        assert not self.failed, f"{self.what}: " + " | ".join(self.failed)


def _check_dlt(rep, placement, out, want, wps, wcnt, t, Xp_live, home_out, score_rtol, dead=()):
    """out: a result of method = DLT at `placement`; want / wps / wcnt: the oracle there; home_out: the result at home (same dtype)."""
    u, D = fc.PLACEMENTS[placement]
    dt = out["xyzs"].dtype
    rep.check(np.array_equal(out["count"], wcnt), placement, f"counts {out['count'].tolist()} vs the oracle's {wcnt.tolist()}")
    if not np.array_equal(out["count"], wcnt):
        return
    got = out["xyzs"].astype(np.float64)
    rep.bound(placement, f"{dt.name} xyz vs oracle", np.abs(got[..., :3] - want[..., :3]), _tolerance(want[..., :3], t, dt), u)
    rep.check(np.allclose(got[..., 3], want[..., 3], rtol=score_rtol, atol=0.0), placement, "joint scores")
    rep.check(np.allclose(out["pscore"].astype(np.float64), wps, rtol=score_rtol, atol=0.0), placement, "person scores")
    # equivariance: brought home, the placement's joints are the home joints
    hx = home_out["xyzs"].astype(np.float64)[..., :3]
    seen = want[..., 3] != 0
    rep.check(np.array_equal(home_out["count"], out["count"]), placement, "count differs from home")
    if placement != "home" and hx.shape == got[..., :3].shape:
        tol_home = _tolerance(want[..., :3], t, dt, factor=2.0) / u          # (twice the bound at the placement, in metres)
        rep.bound(placement, f"{dt.name} xyz / u - D vs home", np.abs(fc.home(got[..., :3], placement) - hx)[seen], tol_home[seen], 1.0)
        rep.check(np.array_equal(got[..., 3], home_out["xyzs"].astype(np.float64)[..., 3]), placement, "joint scores differ from home")
    # untouched slots: a joint nobody sees, and the slots behind count
    rep.check(not got[~seen].any(), placement, "a joint without a score is not (0, 0, 0, 0)")
    for f, p, j in dead:
        rep.check(want[f, p, j, 3] == 0.0 and not got[f, p, j].any(), placement, f"dead joint {(f, p, j)} = {got[f, p, j]}")
    # geometric sanity: the persons are where the placed truth is
    if Xp_live is not None:
        far = np.abs(got[:, 0, :, :3] - Xp_live)[seen[:, 0]]
        rep.check(far.max() < 0.05 * u, placement, f"joints {far.max() / u:.3g} m from the placed truth")


# ------------------------------------------------------------------------------------------------ one detection per camera
def _single_batch(rig_name, F, J, in_dtype, seed):
    K, R, t = fc.rig(rig_name)
    rng = np.random.default_rng(seed)
    # (0.6 m off the line between two opposite cameras: two views still fix the depth to centimetres)
    X = synth.make_people(rng, F, 1, J=J, centres=np.array([[0.3, 0.9, 0.0]]))
    kp, npers = synth.make_keypoints(rng, K, R, t, X, pixel_sigma=NOISE, score_range=(2.0, 8.0), dtype=in_dtype)
    kp, npers = kp.copy(), npers.copy()
    dead = [(0, 0, 1), (F - 1, 0, J - 1)]
    for f, _, j in dead:
        kp[f, :, 0, j, 2] = 0.5                      # a joint nobody sees
    kp[1, 1:, 0, 3, 2] = 0.5                         # a joint one camera sees
    dead.append((1, 0, 3))
    if K.shape[0] > 2:
        npers[F // 2, 1] = 0                         # a camera that lists nobody
    return K, R, t, X, kp, npers, dead


SINGLE = [("coop", "ring4", 133, 133, 5, np.float32, None), ("coop", "ring8", 133, 133, 5, np.float32, None),
          ("coop", "mixed4", 133, 133, 5, np.float32, None),
          ("fused", "ring2", 20, 17, 4, np.float64, None), ("fused", "ring3", 20, 17, 4, np.float64, None),
          ("fused", "ring5", 20, 17, 4, np.float64, None), ("fused", "mixed5", 20, 17, 4, np.float64, None),
          ("fused", "ring4", 133, 133, 5, np.float64, {"SNOWTRI_LEAN_MODE": "0"})]


@pytest.mark.parametrize("route,rig_name,J,kn,F,in_dtype,env", SINGLE, ids=[f"{c[0]}-{c[1]}-J{c[2]}-kn{c[3]}" for c in SINGLE])
def test_single_detection_routes(api, knobs, route, rig_name, J, kn, F, in_dtype, env):
    """k_dlt_coop<C> (the Wholebody shape) and k_fused_single<C,1> (keypoint_num < J; SNOWTRI_LEAN_MODE=0) at every placement."""
    from oracle import dlt as odlt
    K, R, t, X, kp, npers, dead = _single_batch(rig_name, F, J, in_dtype, seed=500 + 7 * K_count(rig_name) + J)
    C = K.shape[0]
    prm0 = dict(synth.default_thresholds(), keypoint_num=kn, center_point_index=0)
    rep = Report(f"{route} {rig_name}")
    home_out = {}
    for placement in _placements(rig_name):
        tp, Xp, u, D = fc.place(t, X, placement)
        prm = fc.place_params(prm0, placement)
        want, wps, wcnt = odlt.dlt_batch(K, R, tp, kp * (npers[:, :, None, None, None] > 0), prm["keypoint_score_threshold"], kn)
        for out_dtype in (np.float64, np.float32):
            for name, value in (env or {}).items():
                knobs.set(name, value)
            out = _run(api, K, R, tp, prm, kp, npers, out_dtype)
            knobs.clear()
            prefix = f"k_dlt_coop<{C}," if route == "coop" else f"k_fused_single<{C},1,"
            assert out["kernels"].startswith(prefix), out["kernels"]
            home_out.setdefault(np.dtype(out_dtype).name, out)
            _check_dlt(rep, placement, out, want, wps, wcnt, tp, Xp[:, 0, :kn], home_out[np.dtype(out_dtype).name], 1e-6,
                       dead=[d for d in dead if d[2] < kn])
    rep.finish()


@pytest.mark.parametrize("rig_name", ["ring4", "ring8", "mixed4"])
def test_coop_and_fused_single_give_identical_bits(api, knobs, rig_name):
    """The item is one function: k_dlt_coop<C> and k_fused_single<C,1> (SNOWTRI_LEAN_MODE=0) agree bit for bit at every placement."""
    K, R, t, X, kp, npers, dead = _single_batch(rig_name, 5, 133, np.float32, seed=500 + 7 * K_count(rig_name) + 133)
    C = K.shape[0]
    prm0 = dict(synth.default_thresholds(), keypoint_num=133, center_point_index=0)
    rep = Report(f"bits {rig_name}")
    for placement in _placements(rig_name):
        tp, _, u, D = fc.place(t, None, placement)
        prm = fc.place_params(prm0, placement)
        for out_dtype in (np.float64, np.float32):
            a = _run(api, K, R, tp, prm, kp, npers, out_dtype)
            knobs.set("SNOWTRI_LEAN_MODE", "0")
            b = _run(api, K, R, tp, prm, kp, npers, out_dtype)
            knobs.clear()
            assert a["kernels"].startswith(f"k_dlt_coop<{C},") and b["kernels"].startswith(f"k_fused_single<{C},1,"), (a["kernels"], b["kernels"])
            for key in ("xyzs", "count"):            # (the frames' mean scores are summed in each kernel's own order)
                rep.check(np.array_equal(a[key].view(np.uint8), b[key].view(np.uint8)), placement, f"{np.dtype(out_dtype).name} {key} differs")
    rep.finish()


# ------------------------------------------------------------------------------------------------ several detections per camera
def _multi_batch(rig_name, P, F, J, in_dtype, seed, ragged=True):
    K, R, t = fc.rig(rig_name)
    C = K.shape[0]
    rng = np.random.default_rng(seed)
    X = synth.make_people(rng, F, P, J=J)            # (persons 1.5 m apart: synth.person_centres)
    kp, npers = synth.make_keypoints(rng, K, R, t, X, pixel_sigma=NOISE, score_range=(3.5, 8.0), permute_persons=True, dtype=in_dtype)
    kp, npers = kp.copy(), npers.copy()
    if ragged:
        npers[1, 0] = P - 1                          # a ragged list -> member-list clusters
        npers[2, C - 1] = 0                          # a camera that lists nobody
    kp[0, :, :, 5, 2] = 1.0                          # a joint nobody sees
    return K, R, t, X, kp, npers


MULTI = [("cluster", "ring6", 3, 4, 12, None, 0.0), ("cluster", "mixed6", 3, 4, 12, None, 0.0), ("cluster0", "ring12", 2, 3, 12, None, 0.0),
         ("recompute", "ring6", 3, 4, 12, {"SNOWTRI_HANDOVER_MODE": "0"}, 0.0), ("recompute", "ring6", 3, 4, 12, None, 4.0),
         ("recompute", "mixed6", 3, 4, 12, {"SNOWTRI_HANDOVER_MODE": "0"}, 0.0)]


@pytest.mark.parametrize("route,rig_name,P,F,J,env,score_tol", MULTI,
                         ids=[f"{c[0]}-{c[1]}-{'knob' if c[5] else 'default'}-stol{c[6]}" for c in MULTI])
def test_multi_person_routes(api, knobs, route, rig_name, P, F, J, env, score_tol):
    """k_cluster_dlt<C> / <0> behind the streaming association and k_frame_recompute<1> (SNOWTRI_HANDOVER_MODE=0; an active
    condense_score_tol) at every placement: counts equal the oracle's, the persons are the oracle's."""
    from oracle import dlt as odlt, oracle as orc
    K, R, t, X, kp, npers = _multi_batch(rig_name, P, F, J, np.float64, seed=900 + K_count(rig_name))
    C = K.shape[0]
    prm0 = dict(synth.default_thresholds(), average_score_threshold=1.0, condense_distance_tol=0.3, condense_score_tol=score_tol,
                keypoint_num=J, center_point_index=0)
    pout = 2 * P + 2
    rep = Report(f"{route} {rig_name} stol={score_tol}")
    home_out = {}
    for placement in _placements(rig_name):
        tp, Xp, u, D = fc.place(t, X, placement)
        prm = fc.place_params(prm0, placement)
        want, wps, wcnt = odlt.dlt_multi_batch(K, R, tp, kp, npers, orc.make_params(**prm), pout)
        assert wcnt.min() >= 1 and wcnt.max() <= pout, wcnt
        for out_dtype in (np.float64, np.float32):
            for name, value in (env or {}).items():
                knobs.set(name, value)
            out = _run(api, K, R, tp, prm, kp, npers, out_dtype, pout=pout)
            knobs.clear()
            if route == "recompute":
                assert "k_cluster_dlt" not in out["kernels"] and out["kernels"].startswith("k_frame_recompute<1,"), out["kernels"]
            else:
                assert f"k_cluster_dlt<{C if route == 'cluster' else 0}," in out["kernels"], out["kernels"]
            home_out.setdefault(np.dtype(out_dtype).name, out)
            _check_dlt(rep, placement, out, want, wps, wcnt, tp, None, home_out[np.dtype(out_dtype).name],
                       1e-12 if out_dtype == np.float64 else 1e-6)
            # every true person has an output person within 0.05 u (frames whose lists are complete)
            got = out["xyzs"].astype(np.float64)
            for f in range(F):
                if (npers[f] < P).any() or score_tol:
                    continue
                for p in range(P):
                    d = np.linalg.norm(got[f, :wcnt[f], :, :3] - Xp[f, p][None], axis=-1)
                    vis = got[f, :wcnt[f], :, 3] > 0
                    rep.check(np.where(vis, d, 0).max(axis=1).min() < 0.05 * u, placement, f"frame {f}: nobody near true person {p}")
    rep.finish()


# ------------------------------------------------------------------------------------------------ method = DLT_ROBUST
def _robust_prm(placement):
    return fc.place_params(dict(synth.default_thresholds(), keypoint_score_threshold=rc.KTHR, keypoint_num=133, center_point_index=0), placement)


@pytest.mark.parametrize("max_drops", [1, 6])
@pytest.mark.parametrize("rig_name", list(rc.FRAMES_RIGS))
def test_robust_route(api, rig_name, max_drops):
    """k_dlt_robust<C> on the outlier recipe (tests/robust_cases.py::frames_batch) at every placement, by the margin rule of
    tests/test_gpu_robust.py: masks equal where the reference's margin is >= 1e-6, the reference's or its alternative elsewhere."""
    rep = Report(f"robust {rig_name} max_drops={max_drops}")
    home_out = {}
    for placement in rc.frames_placements(rig_name):
        key = ("frames", rig_name, placement)
        b = rc.frames_batch(rig_name, placement)
        ref = rc.reference(key, 133, 6.0, max_drops)
        u, D = fc.PLACEMENTS[placement]
        C = b["K"].shape[0]
        for out_dtype in (np.float64, np.float32):
            out = _run(api, b["K"], b["R"], b["t"], _robust_prm(placement), b["kpts"], b["n_persons"], out_dtype, method=_lib.DLT_ROBUST,
                       reproj_threshold_px=6.0, max_drops=max_drops, diagnostics=True)
            assert out["kernels"].startswith(f"k_dlt_robust<{C},"), out["kernels"]
            dn = np.dtype(out_dtype).name
            home_out.setdefault(dn, out)
            views = out["views"].astype(np.uint32)
            sure = ref["margin"] >= MARGIN
            same = views == ref["views"]
            rep.check(same[sure].all(), placement, f"{dn}: {(~same & sure).sum()} masks differ where the reference's margin is >= {MARGIN}")
            if not same.all():
                alt = alternative_views(b["K"], b["R"], b["t"], b["kpts"], b["n_persons"], rc.KTHR, 133, 6.0, max_drops, ref, below=MARGIN)
                rep.check((views[~same] == alt[~same]).all(), placement, f"{dn}: a mask that is neither the reference's nor its alternative")
            rep.check((out["count"] == 1).all() and (out["flags"] == _lib.FLAG_FASTPATH).all(), placement, f"{dn}: count / flags")
            zero = ref["views"] == 0
            assert zero.any()
            rep.check(((views == 0) == zero).all() and not out["xyzs"][:, 0][zero].any() and not out["resid"][zero].any(), placement,
                      f"{dn}: zero records")
            got, want = out["xyzs"][:, 0].astype(np.float64), ref["xyzs"][:, 0]
            rep.bound(placement, f"{dn} xyz vs reference", np.abs(got[..., :3] - want[..., :3])[same],
                      _tolerance(want[..., :3], b["t"], out_dtype)[same], u)
            rep.check(np.allclose(got[..., 3][same], want[..., 3][same], rtol=1e-6, atol=0.0), placement, f"{dn}: joint scores")
            ra, rr = (1e-6, 1e-6) if out_dtype == np.float64 else (1e-5, 1e-6)
            dr = np.abs(out["resid"].astype(np.float64) - ref["resid"])
            rep.bound(placement, f"{dn} resid vs reference (px)", dr[same], (ra + rr * np.abs(ref["resid"]))[same], 1.0)
            # the clean joints are where the placed truth is
            clean = (b["cam"] < 0) & ~zero
            far = np.abs(got[..., :3] - b["X"][:, 0])[clean]
            rep.check(far.max() < 0.05 * u, placement, f"{dn}: joints {far.max() / u:.3g} m from the placed truth")
            # equivariance
            h = home_out[dn]
            rep.check(np.array_equal(h["views"], out["views"]) and np.array_equal(h["count"], out["count"]), placement, f"{dn}: masks differ from home")
            if placement != "home":
                hx = h["xyzs"][:, 0].astype(np.float64)[..., :3]
                tol_home = _tolerance(want[..., :3], b["t"], out_dtype, factor=2.0) / u
                rep.bound(placement, f"{dn} xyz / u - D vs home", np.abs(fc.home(got[..., :3], placement) - hx)[~zero], tol_home[~zero], 1.0)
                if out_dtype == np.float64:
                    rep.bound(placement, "resid vs home (px)", np.abs(out["resid"] - h["resid"]), np.full(dr.shape, 2e-6), 1.0)
    rep.finish()
