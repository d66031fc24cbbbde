"""Matched triangulation: the robust N-view DLT of 3D person p over the detections that det_of names -- THE RULE in NumPy.

The matching chain (reprojection_cost, match_detections / assign_detections) ends in det_of[f, c, p], the detection of camera c that
belongs to 3D person p.  `triangulate_matched_reference` triangulates from that answer: it gathers person p's observation in every
camera and calls robust.triangulate_robust_reference on them, so the rule is DLT_ROBUST's on other observations and nothing else
(include/snowtri.h, "Matched triangulation", states it for the C ABI).  It is what the HIP kernel (k_dlt_matched,
csrc/snowtri_matched.hpp) is tested against; it is not on the product path and it is slow (an SVD per solve).
`triangulate_matched` runs the kernel.

Camera c LISTS person p in frame f iff q = det_of[f, c, p] satisfies 0 <= q < n_persons[f, c] (det_of None: q = p, which requires
P <= Pmax; n_persons None: Pmax everywhere; an n_persons above Pmax counts as Pmax) -- the first condition of refine_joints.  A
camera that does not list the person has the observation (0, 0, 0) and is in no view set.  Two persons may name the same detection
and then get the same record: one-to-one is the matcher's business.

Left out on purpose: ShardedTrackPipeline, more than 8 cameras, matching against the previous frame's persons (tracking by
reprojection).  (Seeding new persons from person_of's unclaimed detections: snowmocap_amd/seed.py.)
"""
from __future__ import annotations

import numpy as np

from .robust import triangulate_robust_reference

MAX_CAMERAS = 8


def gather_person(kpts, det_of, n_persons, p):
    """Person p's observations: kpts [F, C, Pmax, kn, 3], det_of [F, C, P] or None, n_persons [F, C] or None ->
    (kp [F, C, 1, kn, 3] of kpts' dtype, (0, 0, 0) where the camera does not list the person; listed [F, C] int32, 1 / 0)."""
    kpts = np.asarray(kpts)
    F, C, Pmax, kn, _ = kpts.shape
    if det_of is None:
        if p >= Pmax:
            raise ValueError("det_of=None pairs person p with detection p: P must not exceed Pmax")
        q = np.full((F, C), p, dtype=np.int64)
    else:
        q = np.asarray(det_of).astype(np.int64)[:, :, p]
    nq = np.full((F, C), Pmax, dtype=np.int64) if n_persons is None else np.minimum(np.asarray(n_persons).astype(np.int64).reshape(F, C), Pmax)
    listed = (q >= 0) & (q < nq)
    kp = np.take_along_axis(kpts, np.where(listed, q, 0)[:, :, None, None, None], axis=2)
    kp = np.where(listed[:, :, None, None, None], kp, np.zeros((), dtype=kpts.dtype))
    return np.ascontiguousarray(kp), listed.astype(np.int32)


def _check(kpts, det_of):
    kpts = np.asarray(kpts)
    if kpts.ndim != 5 or kpts.shape[-1] != 3 or kpts.shape[2] < 1:
        raise ValueError(f"kpts must be [F, C, Pmax >= 1, kn, 3] (got shape {kpts.shape})")
    F, C, Pmax, kn, _ = kpts.shape
    if det_of is None:
        P = Pmax
    else:
        det_of = np.asarray(det_of)
        if det_of.ndim != 3 or det_of.shape[:2] != (F, C) or det_of.shape[2] < 1:
            raise ValueError(f"det_of must be [F={F}, C={C}, P >= 1] (got shape {det_of.shape})")
        P = det_of.shape[2]
    return kpts, det_of, F, C, Pmax, kn, P


def triangulate_matched_reference(K, R, t, kpts, det_of=None, n_persons=None, keypoint_score_threshold=0.0, reproj_threshold_px=6.0,
                                  max_drops=1, _flip=None):
    """kpts [F, C, Pmax, kn, 3] on the undistorted frame (float32 or float64), det_of [F, C, P] or None (P = Pmax), n_persons [F, C]
    or None -> dict(xyzs [F, P, kn, 4] fp64, pscore [F, P], views [F, P, kn] uint32, resid [F, P, kn] fp64 px, drops [F, P, kn]
    int32, margin [F, P, kn] fp64, decision [F, P, kn] int32): per person what triangulate_robust_reference returns on its gathered
    observations.  _flip ([F, P, kn] int32, internal): alternative_views."""
    kpts, det_of, F, C, Pmax, kn, P = _check(kpts, det_of)
    out = dict(xyzs=np.zeros((F, P, kn, 4)), pscore=np.zeros((F, P)), views=np.zeros((F, P, kn), dtype=np.uint32), resid=np.zeros((F, P, kn)),
               drops=np.zeros((F, P, kn), dtype=np.int32), margin=np.full((F, P, kn), np.inf), decision=np.full((F, P, kn), -1, dtype=np.int32))
    for p in range(P):
        kp, listed = gather_person(kpts, det_of, n_persons, p)
        one = triangulate_robust_reference(K, R, t, kp, listed, keypoint_score_threshold, kn, reproj_threshold_px, max_drops,
                                           _flip=None if _flip is None else np.asarray(_flip)[:, p])
        out["xyzs"][:, p], out["pscore"][:, p] = one["xyzs"][:, 0], one["pscore"][:, 0]
        for k in ("views", "resid", "drops", "margin", "decision"):
            out[k][:, p] = one[k]
    return out


def alternative_views(K, R, t, kpts, det_of, n_persons, keypoint_score_threshold, reproj_threshold_px, max_drops, ref, below=1e-6):
    """views [F, P, kn] the rule gives when every joint whose margin is under `below` takes its closest decision the other way (equal
    to ref["views"] everywhere else), as robust.alternative_views does.  `ref`: triangulate_matched_reference on the same arguments."""
    close = ref["margin"] < below
    if not close.any():
        return ref["views"].copy()
    alt = triangulate_matched_reference(K, R, t, kpts, det_of, n_persons, keypoint_score_threshold, reproj_threshold_px, max_drops,
                                        _flip=np.where(close, ref["decision"], -1))
    return np.where(close, alt["views"], ref["views"]).astype(np.uint32)


def triangulate_matched(ctx, kpts, det_of=None, n_persons=None, keypoint_score_threshold=0.0, reproj_threshold_px=6.0, max_drops=1,
                        dtype=None, diagnostics=False, stream=None):
    """k_dlt_matched through the context of the rig (_lib.Context): Context.triangulate_matched.  -> (xyzs, pscore), or
    (xyzs, pscore, views, resid) with diagnostics=True."""
    return ctx.triangulate_matched(kpts, det_of=det_of, n_persons=n_persons, keypoint_score_threshold=keypoint_score_threshold,
                                   reproj_threshold_px=reproj_threshold_px, max_drops=max_drops, dtype=dtype, diagnostics=diagnostics,
                                   stream=stream)


def retriangulate_args(retriangulate):
    """The retriangulate= option of TrackPipeline.run: None (off) or gate_px or (gate_px[, reproj_threshold_px = 6.0[, max_drops = 1]])
    -> None or (gate_px, reproj_threshold_px, max_drops)."""
    if retriangulate is None:
        return None
    v = tuple(retriangulate) if isinstance(retriangulate, (tuple, list)) else (retriangulate,)
    if not 1 <= len(v) <= 3 or isinstance(v[0], bool):
        raise ValueError(f"retriangulate must be None, gate_px or (gate_px, reproj_threshold_px, max_drops) (got {retriangulate!r})")
    v = v + (6.0, 1)[len(v) - 1:]
    gate_px, tau = float(v[0]), float(v[1])
    if not gate_px > 0 or int(v[2]) != v[2]:
        raise ValueError(f"retriangulate: gate_px must be positive and max_drops an integer (got {retriangulate!r})")
    return gate_px, tau, int(v[2])


def merge_records(first, again, views, n_cameras=None):
    """The keep-the-old-record merge of a second triangulation pass (NumPy): a joint record of `again` made from at least 2 views
    (views != 0) replaces that of `first`, every other record keeps the bits of `first`, so the second pass never loses a joint
    -> (records, the views mask to hand to refine_joints / refine_cameras: all ones where the record was kept)."""
    views = np.asarray(views).astype(np.uint32)
    made = views != 0
    return np.where(made[..., None], again, first), np.where(made, views, np.uint32(0xFFFFFFFF)).astype(np.uint32)


__all__ = ["triangulate_matched", "triangulate_matched_reference", "alternative_views", "gather_person", "retriangulate_args", "merge_records"]
