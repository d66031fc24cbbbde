"""Reprojection: 3D joint records back into every camera's image, per-view match costs, and what is decided on them.

The rule is stated in include/snowtri.h ("Reprojection"); `reproject_reference` and `reprojection_cost_reference` are that rule in
NumPy, plain operations in its order (no fused multiply-add, the cost summed in joint order), and what the kernels k_reproject /
k_reproject_cost (snowmocap_amd/csrc/snowtri_reproject.hpp) are tested against.  `reproject` and `reprojection_cost` run the
kernels.  `match_detections` and `view_residuals` are the few lines of tensor code on top: which detection of camera c belongs to
3D person p, and how far each of its joints lies from the projection.  They take NumPy arrays, or torch tensors on their own
device without a host round trip.  `assign_detections` is match_detections' one-to-one counterpart: the optimal gated assignment per
(frame, camera), run by the kernel k_assign (snowmocap_amd/csrc/snowtri_assign.hpp), which equals `assign_detections_reference` bit for bit.
"""
from __future__ import annotations

import numpy as np

from . import _lib
from .records import missing_records


def _rig(K, R, t, D):
    K = np.asarray(K, dtype=np.float64).reshape(-1, 3, 3)
    C = K.shape[0]
    R = np.asarray(R, dtype=np.float64).reshape(C, 3, 3)
    t = np.asarray(t, dtype=np.float64).reshape(C, 3)
    if (K[:, 1, 0] != 0).any() or (K[:, 2, 0] != 0).any() or (K[:, 2, 1] != 0).any() or (K[:, 2, 2] != 1).any() \
            or (K[:, 0, 0] == 0).any() or (K[:, 1, 1] == 0).any():
        raise ValueError("K must be [[fx, s, cx], [0, fy, cy], [0, 0, 1]] for every camera")
    if D is not None:
        D = np.asarray(D, dtype=np.float64).reshape(C, -1)[:, :5]
    return K, R, t, D, C


def _project(K, R, t, D, raw, xyzs):
    """-> u, v [F, C, P, kn] float64 and valid [F, C, P, kn] (rules 1-4), the record's score [F, P, kn]."""
    K, R, t, D, C = _rig(K, R, t, D)
    if raw and D is None:
        raise ValueError("raw=True needs the lens coefficients D")
    x4 = np.asarray(xyzs)
    if x4.ndim != 4 or x4.shape[-1] != 4:
        raise ValueError(f"xyzs must be [F, P, kn, 4] records (got shape {x4.shape})")
    x4 = x4.astype(np.float64)
    F, P, kn, _ = x4.shape
    u, v = np.empty((F, C, P, kn)), np.empty((F, C, P, kn))
    valid = np.empty((F, C, P, kn), dtype=bool)
    measured = ~missing_records(x4)
    with np.errstate(all="ignore"):
        for c in range(C):
            d0, d1, d2 = x4[..., 0] - t[c, 0], x4[..., 1] - t[c, 1], x4[..., 2] - t[c, 2]
            pc0 = (R[c, 0, 0] * d0 + R[c, 1, 0] * d1) + R[c, 2, 0] * d2          # R^T d
            pc1 = (R[c, 0, 1] * d0 + R[c, 1, 1] * d1) + R[c, 2, 1] * d2
            pc2 = (R[c, 0, 2] * d0 + R[c, 1, 2] * d1) + R[c, 2, 2] * d2
            x, y = pc0 / pc2, pc1 / pc2
            if raw:
                k1, k2, p1, p2, k3 = D[c]
                r2 = x * x + y * y
                rho = 1 + r2 * (k1 + r2 * (k2 + r2 * k3))
                x, y = (x * rho + 2 * p1 * x * y + p2 * (r2 + 2 * x * x), y * rho + p1 * (r2 + 2 * y * y) + 2 * p2 * x * y)
            u[:, c] = K[c, 0, 0] * x + K[c, 0, 1] * y + K[c, 0, 2]
            v[:, c] = K[c, 1, 1] * y + K[c, 1, 2]
            valid[:, c] = measured & (pc2 > 0) & np.isfinite(u[:, c]) & np.isfinite(v[:, c])
    return u, v, valid, x4[..., 3]


def reproject_reference(K, R, t, xyzs, D=None, raw=False, dtype=np.float64):
    """The rule in NumPy: xyzs [F, P, kn, 4] -> pix [F, C, P, kn, 3] of `dtype`, (u, v, score) where the projection is valid and
    (0, 0, 0) elsewhere.  raw: through the lens D [C, 5] onto the raw frame."""
    u, v, valid, score = _project(K, R, t, D, raw, xyzs)
    pix = np.zeros(u.shape + (3,), dtype=np.float64)
    pix[..., 0] = np.where(valid, u, 0.0)
    pix[..., 1] = np.where(valid, v, 0.0)
    pix[..., 2] = np.where(valid, np.broadcast_to(score[:, None], u.shape), 0.0)
    return pix.astype(dtype)


def reprojection_cost_reference(K, R, t, xyzs, kpts, n_persons=None, keypoint_score_threshold=0.0, D=None, raw=False):
    """The rule in NumPy: xyzs [F, P, kn, 4] against kpts [F, C, Pmax, kn, 3] -> cost_sum [F, C, P, Pmax] float64 (px^2, summed in
    joint order), cost_n int32."""
    u, v, valid, _ = _project(K, R, t, D, raw, xyzs)
    kp = np.asarray(kpts).astype(np.float64)
    F, C, P, kn = u.shape
    if kp.ndim != 5 or kp.shape[:2] != (F, C) or kp.shape[3:] != (kn, 3):
        raise ValueError(f"kpts must be [F={F}, C={C}, Pmax, kn={kn}, 3] (got shape {kp.shape})")
    Pmax = kp.shape[2]
    thr = float(keypoint_score_threshold)
    if thr != thr:
        raise ValueError("keypoint_score_threshold is NaN")
    with np.errstate(all="ignore"):
        counts = ~(kp[..., 2] < thr) & np.isfinite(kp[..., 0]) & np.isfinite(kp[..., 1])            # [F, C, Pmax, kn]
        if n_persons is not None:
            counts &= (np.arange(Pmax)[None, None, :] < np.asarray(n_persons).reshape(F, C, 1))[..., None]
        cost_sum = np.zeros((F, C, P, Pmax))
        cost_n = np.zeros((F, C, P, Pmax), dtype=np.int32)
        for j in range(kn):
            du = u[:, :, :, None, j] - kp[:, :, None, :, j, 0]
            dv = v[:, :, :, None, j] - kp[:, :, None, :, j, 1]
            m = valid[:, :, :, None, j] & counts[:, :, None, :, j]
            cost_sum += np.where(m, du * du + dv * dv, 0.0)
            cost_n += m
    return cost_sum, cost_n


def reproject(ctx, xyzs, raw=False, dtype=None, stream=None):
    """k_reproject through the context of the rig (_lib.Context; raw=True after ctx.set_distortion): Context.reproject."""
    return ctx.reproject(xyzs, raw=raw, dtype=dtype, stream=stream)


def reprojection_cost(ctx, xyzs, kpts, n_persons=None, keypoint_score_threshold=0.0, raw=False, stream=None):
    """k_reproject_cost through the context of the rig: Context.reproject_cost."""
    return ctx.reproject_cost(xyzs, kpts, n_persons=n_persons, keypoint_score_threshold=keypoint_score_threshold, raw=raw, stream=stream)


def _is_tensor(a):
    return hasattr(a, "is_cuda")


def match_detections(cost_sum, cost_n, gate_px, min_joints=8):
    """cost_sum, cost_n [F, C, P, Pmax] -> det_of [F, C, P] (int64: the detection of camera c that belongs to 3D person p, or -1) and
    shared [F, C, P] (bool).  Among the detections q with cost_n >= min_joints the one with the lowest mean cost_sum / cost_n, ties to
    the lowest q; it is taken if that mean is <= gate_px^2 (so gate_px is an RMS pixel distance over the joints compared).
    The match is DELIBERATELY NOT ONE-TO-ONE: every person chooses on its own, nothing is taken away from a detection another person
    chose.  Two 3D persons that project onto one detection (one of them a ghost, or one hidden behind the other in that view) both
    report it, and `shared` marks the persons of one (f, c) that chose the same detection, for the caller to resolve with what it knows."""
    min_joints = int(min_joints)
    if min_joints < 1:
        raise ValueError("min_joints must be >= 1")
    if not float(gate_px) >= 0.0:
        raise ValueError("gate_px must be >= 0 and not NaN")
    gate2 = float(gate_px) * float(gate_px)
    if tuple(cost_sum.shape) != tuple(cost_n.shape) or len(cost_sum.shape) != 4:
        raise ValueError("cost_sum and cost_n must both be [F, C, P, Pmax]")
    Pmax = int(cost_sum.shape[-1])
    if _is_tensor(cost_sum):
        import torch
        inf = torch.full((), float("inf"), dtype=torch.float64, device=cost_sum.device)
        mean = cost_sum.to(torch.float64) / cost_n.clamp(min=1).to(torch.float64)
        mean = torch.where((cost_n >= min_joints) & ~torch.isnan(mean), mean, inf)
        q = torch.arange(Pmax, device=cost_sum.device)
        if Pmax:
            best = mean.min(dim=-1).values
            first = torch.where(mean == best[..., None], q, Pmax).min(dim=-1).values         # the lowest q among the ties
        else:
            best, first = inf.expand(cost_sum.shape[:-1]), torch.zeros(cost_sum.shape[:-1], dtype=torch.int64, device=cost_sum.device)
        det_of = torch.where(torch.isfinite(best) & (best <= gate2), first, -1)
        same = (det_of[..., :, None] == det_of[..., None, :]) & (det_of[..., :, None] >= 0)
        return det_of, same.sum(dim=-1) > 1
    cs, cn = np.asarray(cost_sum, dtype=np.float64), np.asarray(cost_n)
    with np.errstate(all="ignore"):
        mean = cs / np.maximum(cn, 1)
    mean = np.where((cn >= min_joints) & ~np.isnan(mean), mean, np.inf)
    if Pmax:
        best = mean.min(axis=-1)
        first = np.where(mean == best[..., None], np.arange(Pmax), Pmax).min(axis=-1)
    else:
        best, first = np.full(cs.shape[:-1], np.inf), np.zeros(cs.shape[:-1], dtype=np.int64)
    det_of = np.where(np.isfinite(best) & (best <= gate2), first, -1).astype(np.int64)
    same = (det_of[..., :, None] == det_of[..., None, :]) & (det_of[..., :, None] >= 0)
    return det_of, same.sum(axis=-1) > 1


def assign_gate(gate_px):
    """The gate of the one-to-one assignment, checked -> float.  match_detections reads an infinite gate as "no gate"; here staying
    unmatched COSTS gate_px^2, and the rule needs that cost, and the duals summed from it, finite: a gate_px above 1e150 is refused."""
    if not float(gate_px) >= 0.0:
        raise ValueError("gate_px must be >= 0 and not NaN")
    if not float(gate_px) <= 1e150:
        raise ValueError("gate_px must not exceed 1e150 (staying unmatched costs gate_px^2, which must stay finite; match_detections takes an infinite gate)")
    return float(gate_px)


def _assign_args(cost_sum, cost_n, gate_px, min_joints):
    """The checks assign_detections and its reference share, in match_detections' words -> (gate_px, min_joints)."""
    if int(min_joints) != min_joints or int(min_joints) < 1:
        raise ValueError("min_joints must be >= 1")
    assign_gate(gate_px)
    if tuple(cost_sum.shape) != tuple(cost_n.shape) or len(cost_sum.shape) != 4:
        raise ValueError("cost_sum and cost_n must both be [F, C, P, Pmax]")
    if int(cost_sum.shape[2]) < 1 or int(cost_sum.shape[3]) < 1 or int(cost_sum.shape[2]) + int(cost_sum.shape[3]) > 64:
        raise ValueError("assign_detections needs P >= 1, Pmax >= 1 and P + Pmax <= 64")
    return float(gate_px), int(min_joints)


def _assign_one(a, P, Pmax):
    """Rule 3 on one augmented matrix a [P, Pmax + P] -> the row of every column (-1: none).  The column scan of a step is written
    on whole NumPy rows: the same IEEE operation per column as the scalar loop, and argmin returns the FIRST least element, which is
    what the strict `minv[j] < delta` of a scan in increasing j keeps."""
    m = Pmax + P
    inf = np.inf
    u, v = np.zeros(P), np.zeros(m)
    row_of = np.full(m, -1, dtype=np.int64)
    for i in range(P):
        minv = np.full(m, inf)
        way = np.full(m, -1, dtype=np.int64)
        used = np.zeros(m, dtype=bool)
        j0, i0 = -1, i                                     # -1: the virtual column that holds row i
        while True:
            if j0 >= 0:
                used[j0] = True
            cur = (a[i0] - u[i0]) - v
            low = ~used & (cur < minv)
            minv[low] = cur[low]
            way[low] = j0
            j1 = int(np.argmin(np.where(used, inf, minv)))
            delta = minv[j1]
            if used[j1] or not delta < inf:                # (no finite column outside the tree: unreachable with a finite gate2 --
                j0 = -1                                    # row i's own dummy is one; the row is then left unmatched, as in k_assign)
                break
            rows = row_of[used]                            # the tree's rows: those of the used columns, and row i
            u[rows] = u[rows] + delta
            u[i] = u[i] + delta
            v[used] = v[used] - delta
            minv[~used] = minv[~used] - delta
            j0 = j1
            if row_of[j0] < 0:
                break
            i0 = int(row_of[j0])
        while j0 >= 0:
            j1 = int(way[j0])
            row_of[j0] = row_of[j1] if j1 >= 0 else i
            j0 = j1
    return row_of


def assign_detections_reference(cost_sum, cost_n, gate_px, min_joints=8):
    """The rule of include/snowtri.h ("Assignment") in NumPy: cost_sum, cost_n [F, C, P, Pmax] (reprojection_cost's) ->
    det_of [F, C, P] int64 (the detection of person p, or -1), person_of [F, C, Pmax] int64 (the person that took detection q, or
    -1) and total [F, C] float64.  Per (f, c): mean = cost_sum / cost_n, admissible iff cost_n >= min_joints, not NaN and
    -inf < mean <= gate_px^2 (match_detections' per-pair condition), +inf otherwise; one dummy column per person at gate_px^2 (staying
    unmatched); then the shortest-augmenting-path method with rows inserted in order, cur = (a[i0][j] - u[i0]) - v[j], both
    comparisons strict (ties to the lowest column).  The result is a minimum-sum ONE-TO-ONE matching, and the one k_assign returns
    bit for bit; total adds the matched means in increasing p."""
    gate_px, min_joints = _assign_args(cost_sum, cost_n, gate_px, min_joints)
    gate2 = gate_px * gate_px
    cs, cn = np.asarray(cost_sum, dtype=np.float64), np.asarray(cost_n)
    F, C, P, Pmax = cs.shape
    with np.errstate(all="ignore"):
        mean = cs / cn.astype(np.float64)
        ok = (cn >= min_joints) & ~np.isnan(mean) & (mean <= gate2) & (mean > -np.inf)
    mean = np.where(ok, mean, np.inf)
    det_of = np.full((F, C, P), -1, dtype=np.int64)
    person_of = np.full((F, C, Pmax), -1, dtype=np.int64)
    total = np.zeros((F, C))
    a = np.full((P, Pmax + P), np.inf)
    a[np.arange(P), Pmax + np.arange(P)] = gate2
    for f in range(F):
        for c in range(C):
            a[:, :Pmax] = mean[f, c]
            row_of = _assign_one(a, P, Pmax)
            acc = 0.0
            for q in range(Pmax):
                if row_of[q] >= 0:
                    det_of[f, c, row_of[q]] = q
                    person_of[f, c, q] = row_of[q]
            for p in range(P):
                if det_of[f, c, p] >= 0:
                    acc = acc + mean[f, c, p, det_of[f, c, p]]
            total[f, c] = acc
    return det_of, person_of, total


def assign_detections(ctx, cost_sum, cost_n, gate_px, min_joints=8, with_person_of=False, with_total=False, stream=None):
    """k_assign through a context (Context.assign_detections; any context, the rig is not used): cost_sum, cost_n [F, C, P, Pmax] ->
    det_of [F, C, P] in match_detections' dtype (int64), so it drops into view_residuals, refine_joints and refine_cameras unchanged
    -- but ONE-TO-ONE: no two persons of an (f, c) hold the same detection, and a person is left at -1 when its only detections
    inside the gate went to persons they fit better.  with_person_of: also person_of [F, C, Pmax] int64 (-1: a detection nobody
    claimed), with_total: also total [F, C] float64; a tuple in that order.  NumPy arrays, or CUDA tensors without a host round trip."""
    _assign_args(cost_sum, cost_n, gate_px, min_joints)
    if _is_tensor(cost_sum):
        import torch
        cost_sum, cost_n, wide = cost_sum.to(torch.float64).contiguous(), cost_n.to(torch.int32).contiguous(), lambda a: a.to(torch.int64)
    else:
        wide = lambda a: a.astype(np.int64)    # noqa: E731
    out = ctx.assign_detections(cost_sum, cost_n, gate_px, min_joints, with_person_of=with_person_of, with_total=with_total, stream=stream)
    if not (with_person_of or with_total):
        return wide(out)
    return tuple(wide(a) if i < 1 + bool(with_person_of) else a for i, a in enumerate(out))


def view_residuals(pix, kpts, det_of, keypoint_score_threshold):
    """pix [F, C, P, kn, 3] (reproject's output), kpts [F, C, Pmax, kn, 3], det_of [F, C, P] (match_detections) ->
    resid [F, C, P, kn] float64: the pixel distance between the projection of joint (p, j) and joint j of the detection person p was
    matched to in camera c -- NaN where the projection is invalid (its score is 0), the detection's joint does not count (score below
    the threshold, or a pixel that is not finite) or det_of < 0;
    view_rms [F, C, P]: the root mean square of a view's residuals (NaN when it has none); view_n [F, C, P]: how many it has."""
    thr = float(keypoint_score_threshold)
    if _is_tensor(pix):
        import torch
        pmax = int(kpts.shape[2])
        has = (det_of >= 0) if pmax else torch.zeros_like(det_of, dtype=torch.bool)
        if pmax:
            idx = det_of.clamp(min=0)[..., None, None].expand(*det_of.shape, kpts.shape[3], 3)
            det = torch.gather(kpts, 2, idx).to(torch.float64)
        else:
            det = torch.zeros(pix.shape, dtype=torch.float64, device=pix.device)
        p64 = pix.to(torch.float64)
        du, dv = p64[..., 0] - det[..., 0], p64[..., 1] - det[..., 1]
        ok = has[..., None] & (p64[..., 2] != 0) & ~(det[..., 2] < thr) & torch.isfinite(det[..., 0]) & torch.isfinite(det[..., 1])
        nan = torch.full((), float("nan"), dtype=torch.float64, device=pix.device)
        r2 = du * du + dv * dv
        resid = torch.where(ok, torch.sqrt(r2), nan)
        n = ok.sum(dim=-1)
        rms = torch.where(n > 0, torch.sqrt(torch.where(ok, r2, 0.0).sum(dim=-1) / n.clamp(min=1)), nan)
        return resid, rms, n
    p64, kp, det_of = np.asarray(pix).astype(np.float64), np.asarray(kpts).astype(np.float64), np.asarray(det_of)
    pmax = kp.shape[2]
    has = (det_of >= 0) & (pmax > 0)
    if pmax:
        det = np.take_along_axis(kp, np.maximum(det_of, 0)[..., None, None], axis=2)
    else:
        det = np.zeros(p64.shape)
    with np.errstate(all="ignore"):
        du, dv = p64[..., 0] - det[..., 0], p64[..., 1] - det[..., 1]
        ok = has[..., None] & (p64[..., 2] != 0) & ~(det[..., 2] < thr) & np.isfinite(det[..., 0]) & np.isfinite(det[..., 1])
        r2 = du * du + dv * dv
        resid = np.where(ok, np.sqrt(r2), np.nan)
        n = ok.sum(axis=-1)
        rms = np.where(n > 0, np.sqrt(np.where(ok, r2, 0.0).sum(axis=-1) / np.maximum(n, 1)), np.nan)
    return resid, rms, n


__all__ = ["reproject_reference", "reprojection_cost_reference", "reproject", "reprojection_cost", "match_detections", "view_residuals",
           "assign_detections", "assign_detections_reference"]
_ = _lib   # (the wrappers go through _lib.Context)
