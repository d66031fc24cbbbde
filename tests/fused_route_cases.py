"""The route table of the fused call (tests/test_gpu_fused_routes.py): one small batch per kernel route of
snowtri_triangulate_condense / snowtri_triangulate_robust on the synthetic rigs of snowmocap_amd/synth.py, with the string
snowtri_last_kernel_names returns for it.  70 frames: tiles come out uneven.

A route: C cameras, P detections per camera, J joints, keypoint_num kn, method, output type, output slots, the thresholds that
differ from the batch's own, the knobs that force it (the test build of the library) and the rule it is compared with:
"pairwise" (oracle.triangulate_condense_batch), "dlt" (oracle/dlt.py dlt_batch), "dlt_multi" (dlt_multi_batch) or "robust"
(snowmocap_amd.robust.triangulate_robust_reference).
"""
import functools

import numpy as np

from snowmocap_amd import _lib, synth

F = 70
STREAM_4X2 = ("k_candidate_sums<float,256> + k_candidate_sums_exact<float> + k_associate<float> + k_cluster_fuse<4,float> + "
              "k_cluster_members<float> + k_frame_recompute<0,float,float> (frames left behind)")
# the multi-person thresholds of tests/test_gpu_handover.py
MULTI = dict(keypoint_score_threshold=3.0, average_score_threshold=0.3, distance_threshold=0.05, condense_distance_tol=0.3,
             condense_person_num_tol=2, condense_score_tol=0.0, center_point_index=0)
ROBUST_TAU, ROBUST_DROPS = 6.0, 1
NOBODY, GATED = 3, 20      # single-person pairwise batches: the frame in which camera 1 lists nobody (it breaks the fast kernels'
                           # speculation), the frame whose confidences are all gated (it does not: every joint is empty)


def _route(id, names, C=4, P=1, J=133, kn=None, method=_lib.PAIRWISE, out="float32", pout=1, prm=None, knobs=None, rule="pairwise",
           fast="none", singular=()):
    """fast: which frames carry SNOWTRI_FLAG_FASTPATH -- "kernel": a speculating kernel (not frame NOBODY, nearly all others),
    "all": every frame (the DLT kernels have no other path), "none" (the multi-person kernels never set it).
    singular: frames that get a pair of equal rays (cameras 0 and 1 made twins: the same K and R, another centre)."""
    return dict(id=id, names=names, C=C, P=P, J=J, kn=J if kn is None else kn, method=method, out=out, pout=pout, prm=prm or {},
                knobs=knobs or {}, rule=rule, fast=fast, singular=tuple(singular))


ROUTES = [
    _route("lean_coop", "k_fused_lean_coop<4,float,133>", fast="kernel"),
    _route("lean_coop_f64", "k_fused_lean_coop<5,float,133,double>", C=5, out="float64", fast="kernel"),
    _route("lean", "k_fused_lean<4,float,133>", knobs={"SNOWTRI_LEAN_COOP": "0"}, fast="kernel"),
    _route("single_f64", "k_fused_single<4,0,float,double>", out="float64", fast="kernel"),
    _route("single_j17", "k_fused_single<4,0,float,float>", J=17, fast="kernel"),
    _route("dlt_coop", "k_dlt_coop<4,float,133,float>", method=_lib.DLT, rule="dlt", fast="all"),
    _route("dlt_single_kn", "k_fused_single<5,1,float,float>", C=5, kn=100, method=_lib.DLT, rule="dlt", fast="all"),
    _route("dlt_robust", "k_dlt_robust<4,float,float>", method=_lib.DLT_ROBUST, rule="robust", fast="all"),
    _route("stream_4x2", STREAM_4X2, P=2, pout=3),
    # keypoint_num < J with an active mean-score filter: the second candidate pass (the names do not show it)
    _route("stream_4x2_kn", STREAM_4X2, P=2, kn=30, pout=3, prm=dict(center_point_index=18, condense_score_tol="median")),
    _route("sumless_5", "k_singular_scan<float> + k_associate<float> + k_cluster_fuse<5,float> + k_cluster_members<float> + "
           "k_person_scores<float> + k_frame_recompute<0,float,float> (frames left behind)", C=5, J=17, singular=(7, 31)),
    _route("stream_dlt_4x2", "k_candidate_sums<float,256> + k_candidate_sums_exact<float> + k_associate<float> + k_cluster_dlt<4,float,float> + "
           "k_person_scores<float> + k_frame_recompute<1,float,float> (frames left behind)", P=2, pout=6, method=_lib.DLT, rule="dlt_multi",
           prm=dict(synth.default_thresholds(), average_score_threshold=1.0, condense_distance_tol=0.3)),
    _route("stream_wide_12x2", "k_candidate_sums<float,256> + k_candidate_sums_exact<float> + k_associate<float> + k_cluster_fuse_wide<float> + "
           "k_cluster_members<float> + k_frame_recompute<0,float,float> (frames left behind)", C=12, P=2, pout=1),      # one slot for two persons: SNOWTRI_FLAG_OVERFLOW
    # a negative distance_threshold keeps the call off the streaming route; float64 outputs keep it off the hand-over as well
    _route("recompute", "k_frame_recompute<0,float,double>", P=2, pout=3, out="float64", prm=dict(distance_threshold=-0.05)),
    _route("handover", "k_frame_recompute<0,float,float> + k_cluster_fuse<4,float> + k_cluster_members<float>", P=2, pout=1,
           knobs={"SNOWTRI_HANDOVER_MODE": "2"}),
    _route("general", "k_frame_general<float,float>", P=2, pout=1, knobs={"SNOWTRI_GENERAL_MODE": "1"}),
]
BY_ID = {r["id"]: r for r in ROUTES}
# one route of every launcher, and whether the launcher attaches the timing ring's event pair to its dispatch
TIMED = [("lean_coop", True), ("dlt_coop", True), ("dlt_robust", True), ("single_f64", False), ("stream_4x2", False), ("general", False)]


@functools.lru_cache(maxsize=None)
def batch(route_id):
    """(K, R, t, kpts [F, C, P, J, 3] float32, n_persons [F, C], thresholds) of a route: read-only, made once."""
    r = BY_ID[route_id]
    C, P, J = r["C"], r["P"], r["J"]
    rng = np.random.default_rng(4000 + 100 * C + 10 * P + J % 7)
    K, R, t = synth.ring_rig(C)
    if r["singular"]:                    # camera 1 is camera 0 moved sideways: equal pixels in the two are parallel rays
        K[1], R[1] = K[0], R[0]
        t[1] = t[0] + R[0] @ np.array([0.4, 0.1, 0.0])
    X = synth.make_people(rng, F, P, J=J)
    if P == 1:
        kp, npers = synth.make_keypoints(rng, K, R, t, X, pixel_sigma=1.0, score_range=(2.0, 8.0))
        prm = dict(synth.default_thresholds(), condense_distance_tol=0.5)
        if r["rule"] == "pairwise":
            npers[NOBODY, 1] = 0
            kp[GATED, :, 0, :, 2] = 0.0
            for f in r["singular"]:
                kp[f, 0, 0, 5, :2] = kp[f, 1, 0, 5, :2]
        elif r["rule"] == "dlt":
            npers[3, 1] = 0
        else:                            # the outlier recipe of the robust method: one camera shifted on a tenth of the joints
            kp, _ = synth.add_outliers(rng, kp, fraction=0.1)
    else:
        kp, npers = synth.make_keypoints(rng, K, R, t, X, pixel_sigma=0.7, score_range=(2.5, 9.0), permute_persons=True)
        prm = dict(MULTI)
        npers[1, 0] = P - 1              # a ragged person list: clusters that are no complete graph
    prm.update(keypoint_num=r["kn"], center_point_index=0)
    prm.update(r["prm"])
    if prm["condense_score_tol"] == "median":      # in the middle of the persons' mean scores: persons dropped, slots move up
        from oracle import oracle as orc
        ref0 = orc.triangulate_condense_batch(K, R, t, kp, npers, orc.make_params(**dict(prm, condense_score_tol=0.0)), 8)
        prm["condense_score_tol"] = float(np.median(ref0["pscore"][ref0["pscore"] > 0]))
    for a in (K, R, t, kp, npers):
        a.setflags(write=False)
    return K, R, t, kp, npers, prm


@functools.lru_cache(maxsize=None)
def reference(route_id, pout):
    """What the route's rule gives for its batch."""
    r = BY_ID[route_id]
    K, R, t, kp, npers, prm = batch(route_id)
    if r["rule"] == "pairwise":
        from oracle import oracle as orc
        return orc.triangulate_condense_batch(K, R, t, kp, npers, orc.make_params(**prm), max(pout, 4))
    if r["rule"] == "dlt":
        from oracle import dlt
        return dlt.dlt_batch(K, R, t, kp * (npers[:, :, None, None, None] > 0), prm["keypoint_score_threshold"], prm["keypoint_num"])
    if r["rule"] == "dlt_multi":
        from oracle import dlt, oracle as orc
        return dlt.dlt_multi_batch(K, R, t, kp, npers, orc.make_params(**prm), pout)
    from snowmocap_amd.robust import triangulate_robust_reference
    return triangulate_robust_reference(K, R, t, kp, npers, prm["keypoint_score_threshold"], prm["keypoint_num"], ROBUST_TAU, ROBUST_DROPS)


def triangulator(api, route_id, knobs=None, out=None, pout=None, **kw):
    """A BatchTriangulator on the route's rig (its knobs set through the `knobs` fixture first; clear them after closing it)."""
    r = BY_ID[route_id]
    for k, v in r["knobs"].items():
        knobs.set(k, v)
    K, R, t, _, _, prm = batch(route_id)
    return api.BatchTriangulator(K, R, t, prm, pout_max=pout or r["pout"], out_dtype=np.dtype(out or r["out"]), method=r["method"],
                                 reproj_threshold_px=ROBUST_TAU, max_drops=ROBUST_DROPS, **kw)
