"""Refinement: joint records of any route moved to a local minimum of their weighted reprojection error, in pixels.

Every route through the library ends in a closed-form 3D joint -- the score-weighted mean of two-ray midpoints (PAIRWISE), the
minimiser of an algebraic error (DLT, DLT_ROBUST, the per-cluster DLT).  None of them minimises the distance between the joint's
projections and the detections, which is the quantity the detector's noise lives in and the one `reprojection_cost` /
`view_residuals` report.  A few Gauss-Newton steps from the closed-form point, on a 3 x 3 system per joint, find the
maximum-likelihood point under pixel noise.

The rule is stated in include/snowtri.h ("Refinement").  `refine_joints_reference` is that rule in NumPy: plain operations in its
order (no fused multiply-add, a view's terms summed in camera order), no GPU, no library; it is what the host tests check and what
the kernel k_refine (snowmocap_amd/csrc/snowtri_refine.hpp) is compared with: classes and costs, and the distance of both to a
50-digit minimiser (tests/refine_cases.py).  `refine_joints` runs the kernel.

The keypoints are on the UNDISTORTED frame (undistort first: Context.undistort_keypoints is an exact inverse).  Not offered: more
than 32 cameras, ShardedTrackPipeline.

THE HUBER LOSS (huber_px = delta in pixels; None or 0: the squared loss, today's bits).  Per view s = ru^2 + rv^2; s <= delta^2:
rho = s, kappa = 1; otherwise r = sqrt(s), rho = (2 delta) r - delta^2, kappa = delta / r; E = sum w rho, H = sum (w kappa) J^T J,
g = sum (w kappa) J^T r (`huber_terms`; IRLS weights, no second-order term).  Everything else is the rule as it was.  With the loss
on, `outliers` [F, P, kn] says which views are in the linear regime at the output point; V & ~outliers is an inlier mask in the
format of `views`, which the pairwise route otherwise has no producer of.  IRLS CONVERGES LINEARLY: a record whose minimiser leaves
fewer than two views in the quadratic regime (0.8 % of the refined records with 5 cameras, 4 .. 5 % with 4, 15 .. 17 % with 3 on the
test cases) is not fixed by its inliers -- after 16 steps the rule is up to 7e-2 of the rig scale from where 200 steps of 50-digit
IRLS end, a fifth of them unsettled even then -- and popcount(V & ~outliers) < 2 marks it: keep its closed-form point.  With
exactly two quadratic views convergence is sometimes slow (up to 1.7e-5); with three or more the rule is within 6e-10 .. 3e-7 of the
rig scale of a 50-digit minimiser at iters = 16 (tests/huber_cases.py).  Not offered: other losses (Cauchy, Tukey), an automatic delta, the Triggs second-order correction, damping.

What it buys, on synthetic recipes (synth.ring_rig / the floor rig, two persons on the 1.5 m circle, 10 640 joints; not footage):
with 1 px of noise in 4 cameras the RMS error against the truth goes from 7.08 mm (pairwise) / 6.95 mm (DLT) to 6.48 mm, with 8
cameras from 5.37 / 5.29 to 4.87 mm; with a per-view sigma and score_weights = 1 / sigma^2 from 12.7 mm (DLT) over 11.8 mm (unit
weights) to 9.4 mm.  On a single person standing at the rig's centre the gain is below 1 %: the geometry is symmetric.
"""
from __future__ import annotations

import numpy as np

from . import _lib
from ._lib import REFINE_FEW_VIEWS, REFINE_KEPT, REFINE_MISSING, REFINE_MOVED  # noqa: F401
from .records import missing_records
from .reproject import _rig

MAX_ITERS = 16
MAX_CAMERAS = 32
MAX_HUBER_PX = 1e150


def _check_iters(iters):
    if int(iters) != iters or not (1 <= int(iters) <= MAX_ITERS):
        raise ValueError(f"iters must lie in 1..{MAX_ITERS} (got {iters})")
    return int(iters)


def check_huber(huber_px):
    """The `huber_px` argument of every layer -> None (the squared loss: None or 0) or delta > 0 in pixels, checked: finite, >= 0 and
    at most MAX_HUBER_PX (delta * delta must stay finite)."""
    if huber_px is None:
        return None
    d = float(huber_px)
    if not (d >= 0.0 and d <= MAX_HUBER_PX):
        raise ValueError(f"huber_px must be finite, >= 0 and at most 1e150 (got {huber_px!r})")
    return d if d > 0.0 else None


def huber_terms(s, delta):
    """The loss of ROBUST LOSS on s = ru * ru + rv * rv: -> rho, kappa, linear (all of s' shape), every operation rounded on its
    own: s <= delta * delta: rho = s, kappa = 1; otherwise r = sqrt(s), rho = (2 delta) r - delta * delta, kappa = delta / r."""
    delta = float(delta)
    two_d, dd = 2.0 * delta, delta * delta
    s = np.asarray(s, dtype=np.float64)
    with np.errstate(all="ignore"):
        linear = ~(s <= dd)
        r = np.sqrt(s)
        rho = np.where(linear, two_d * r - dd, s)
        kappa = np.where(linear, delta / r, 1.0)
    return rho, kappa, linear


def refine_args(refine):
    """TrackPipeline.run's `refine` argument -> None (off), (iters, gate_px, score_weights) or, with a Huber loss,
    (iters, gate_px, score_weights, huber_px), checked.  A fourth entry of None or 0 is the squared loss: the triple."""
    if refine is None:
        return None
    huber_px = None
    if isinstance(refine, (tuple, list)):
        if len(refine) == 4:
            iters, gate_px, score_weights, huber_px = refine
        elif len(refine) == 3:
            iters, gate_px, score_weights = refine
        else:
            raise ValueError(f"refine must be None (off), iters, (iters, gate_px, score_weights) or (iters, gate_px, score_weights, huber_px) (got {refine!r})")
    else:
        iters, gate_px, score_weights = refine, 6.0, False
    if not float(gate_px) >= 0.0:
        raise ValueError("refine: gate_px must be >= 0 and not NaN")
    huber_px = check_huber(huber_px)
    head = (_check_iters(iters), float(gate_px), bool(score_weights))
    return head if huber_px is None else head + (huber_px,)


def project_camera(Kc, Rc, tc, X):
    """Rules 1 and 3 of "Reprojection" for one camera: X [n, 3] -> x, y, pc2, u, v, ok [n] (ok: pc2 > 0 and a finite pixel)."""
    d0, d1, d2 = X[:, 0] - tc[0], X[:, 1] - tc[1], X[:, 2] - tc[2]
    pc0 = (Rc[0, 0] * d0 + Rc[1, 0] * d1) + Rc[2, 0] * d2
    pc1 = (Rc[0, 1] * d0 + Rc[1, 1] * d1) + Rc[2, 1] * d2
    pc2 = (Rc[0, 2] * d0 + Rc[1, 2] * d1) + Rc[2, 2] * d2
    x, y = pc0 / pc2, pc1 / pc2
    u = (Kc[0, 0] * x + Kc[0, 1] * y) + Kc[0, 2]
    v = Kc[1, 1] * y + Kc[1, 2]
    return x, y, pc2, u, v, (pc2 > 0) & np.isfinite(u) & np.isfinite(v)


def observation_sets(K, R, t, xyzs, kpts, det_of=None, n_persons=None, views=None, keypoint_score_threshold=0.0, score_weights=False):
    """Rule 1 of "Refinement" without its at-least-two-views clause, which is rule 1 of "Camera pose refinement": which observation of
    which camera is a view of which record.  xyzs [F, P, kn, 4], kpts [F, C, Pmax, kn, 3], det_of [F, C, P] or None, n_persons [F, C]
    or None, views [F, P, kn] (bit c: camera c may be used) or None ->
    X [N, 3] (the records' points, (0, 0, 0) for a missing one), S [C, N] bool, obs [C, N, 3] = (u_obs, v_obs, w)."""
    K, R, t, _, C = _rig(K, R, t, None)
    if C > MAX_CAMERAS:
        raise ValueError(f"more than {MAX_CAMERAS} cameras")
    thr = float(keypoint_score_threshold)
    if thr != thr:
        raise ValueError("keypoint_score_threshold is NaN")
    xin = _lib.host_floats(xyzs)
    if xin.ndim != 4 or xin.shape[-1] != 4:
        raise ValueError(f"xyzs must be [F, P, kn, 4] records (got shape {xin.shape})")
    F, P, kn, _ = xin.shape
    kp = np.asarray(kpts).astype(np.float64)
    if kp.ndim != 5 or kp.shape[:2] != (F, C) or kp.shape[3:] != (kn, 3) or kp.shape[2] < 1:
        raise ValueError(f"kpts must be [F={F}, C={C}, Pmax >= 1, kn={kn}, 3] (got shape {kp.shape})")
    Pmax = kp.shape[2]
    if det_of is None:
        if P > Pmax:
            raise ValueError("det_of=None pairs person p with detection p: P must not exceed Pmax")
        q = np.broadcast_to(np.arange(P, dtype=np.int64), (F, C, P))
    else:
        q = np.asarray(det_of).astype(np.int64).reshape(F, C, P)
    nq = np.full((F, C), Pmax, dtype=np.int64) if n_persons is None else np.asarray(n_persons).astype(np.int64).reshape(F, C)
    N = F * P * kn
    x4 = xin.astype(np.float64)
    measured = ~missing_records(x4).reshape(N)
    listed = (q >= 0) & (q < nq[..., None]) & (q < Pmax)                                               # [F, C, P]
    obs = np.take_along_axis(kp, np.where(listed, q, 0)[..., None, None], axis=2) if N else np.zeros((F, C, P, kn, 3))
    obs = np.moveaxis(obs, 1, 0).reshape(C, N, 3).copy()                                               # [C, N, (u, v, s)]
    listed = np.moveaxis(np.broadcast_to(listed[..., None], (F, C, P, kn)), 1, 0).reshape(C, N)
    allowed = np.full(N, 0xffffffff, dtype=np.uint32) if views is None else np.asarray(views).astype(np.uint32).reshape(N)
    X = np.where(measured[:, None], x4.reshape(N, 4)[:, :3], 0.0)
    S = np.zeros((C, N), dtype=bool)
    with np.errstate(all="ignore"):
        for c in range(C):
            ok = project_camera(K[c], R[c], t[c], X)[5]
            bit = ((allowed >> np.uint32(c)) & 1).astype(bool)
            S[c] = measured & listed[c] & np.isfinite(obs[c, :, 0]) & np.isfinite(obs[c, :, 1]) & ~(obs[c, :, 2] < thr) & bit & ok
    if not score_weights:
        obs[..., 2] = 1.0
    return X, S, obs


def refine_joints_reference(K, R, t, xyzs, kpts, det_of=None, n_persons=None, views=None, keypoint_score_threshold=0.0, iters=4,
                            score_weights=False, return_views=False, huber_px=None):
    """The rule in NumPy: xyzs [F, P, kn, 4] (float32 / float64), kpts [F, C, Pmax, kn, 3], det_of [F, C, P] or None, n_persons
    [F, C] or None, views [F, P, kn] (bit c: camera c may be used) or None ->
    (out: xyzs' shape and dtype, cost [F, P, kn, 2] float64, codes [F, P, kn] uint8); with return_views also the view set V of
    every record as a mask [F, P, kn] uint32 (0 for a copied record).  huber_px (delta > 0; None or 0: the squared loss, and
    nothing below): the Huber loss of ROBUST LOSS, and one more result at the very end, outliers [F, P, kn] uint32 (bit c:
    camera c is a view of the record and in the linear regime at the output point; 0 for a copied record)."""
    K, R, t, _, C = _rig(K, R, t, None)
    iters = _check_iters(iters)
    delta = check_huber(huber_px)
    X, V, obs = observation_sets(K, R, t, xyzs, kpts, det_of, n_persons, views, keypoint_score_threshold, score_weights)
    xin = _lib.host_floats(xyzs)
    F, P, kn, _ = xin.shape
    N = F * P * kn
    measured = ~missing_records(xin).reshape(N)

    def project(X):
        """X [n, 3] -> x, y, pc2, u, v, ok [C, n] (rules 1, 3 and the geometric half of rule 4 of "Reprojection")."""
        out = [project_camera(K[c], R[c], t[c], X) for c in range(C)]
        return [np.stack(a) for a in zip(*out)] if out else [np.zeros((0, X.shape[0]))] * 6

    def evaluate(X, V, ou, ov, w):
        """-> E [n], H [n, 6] (00, 10, 11, 20, 21, 22), g [n, 3], every view of V valid [n], the views of V in the linear regime
        [C, n] (all False under the squared loss); the views summed in camera order."""
        n = X.shape[0]
        x, y, pc2, u, v, ok = project(X)
        E, H, g = np.zeros(n), np.zeros((n, 6)), np.zeros((n, 3))
        valid = np.ones(n, dtype=bool)
        lin = np.zeros((C, n), dtype=bool)
        for c in range(C):
            ru, rv = u[c] - ou[c], v[c] - ov[c]
            wc = w[c]
            dx = [(R[c, k, 0] - x[c] * R[c, k, 2]) / pc2[c] for k in range(3)]
            dy = [(R[c, k, 1] - y[c] * R[c, k, 2]) / pc2[c] for k in range(3)]
            du = [K[c, 0, 0] * dx[k] + K[c, 0, 1] * dy[k] for k in range(3)]
            dv = [K[c, 1, 1] * dy[k] for k in range(3)]
            in_ = V[c]
            if delta is None:
                E = E + np.where(in_, w[c] * (ru * ru + rv * rv), 0.0)
            else:
                rho, kappa, linear = huber_terms(ru * ru + rv * rv, delta)
                E = E + np.where(in_, w[c] * rho, 0.0)
                wc = w[c] * kappa                      # the IRLS weight: H and g only
                lin[c] = in_ & linear
            for m, (a, b) in enumerate(((0, 0), (1, 0), (1, 1), (2, 0), (2, 1), (2, 2))):
                H[:, m] = H[:, m] + np.where(in_, wc * (du[a] * du[b] + dv[a] * dv[b]), 0.0)
            for k in range(3):
                g[:, k] = g[:, k] + np.where(in_, wc * (du[k] * ru + dv[k] * rv), 0.0)
            valid &= ok[c] | ~in_
        return E, H, g, valid, lin

    def solve(H, g):
        """H d = -g by LDL^T -> d [n, 3], every pivot finite and > 0 [n]."""
        p0 = H[:, 0]
        l10, l20 = H[:, 1] / p0, H[:, 3] / p0
        p1 = H[:, 2] - l10 * H[:, 1]
        m21 = H[:, 4] - l20 * H[:, 1]
        l21 = m21 / p1
        p2 = (H[:, 5] - l20 * H[:, 3]) - l21 * m21
        y0 = -g[:, 0]
        y1 = -g[:, 1] - l10 * y0
        y2 = (-g[:, 2] - l20 * y0) - l21 * y1
        s2 = y2 / p2
        s1 = y1 / p1 - l21 * s2
        s0 = (y0 / p0 - l10 * s1) - l20 * s2
        pd = (p0 > 0) & np.isfinite(p0) & (p1 > 0) & np.isfinite(p1) & (p2 > 0) & np.isfinite(p2)
        return np.stack([s0, s1, s2], axis=1), pd

    with np.errstate(all="ignore"):
        few = V.sum(axis=0) < 2
        V &= ~few[None, :]
        ou, ov, w = np.where(V, obs[..., 0], 0.0), np.where(V, obs[..., 1], 0.0), np.where(V, obs[..., 2], 0.0)
        E, H, g, _, lin = evaluate(X, V, ou, ov, w)
        E0 = E.copy()
        active = measured & ~few
        moved = np.zeros(N, dtype=bool)
        for _ in range(iters):
            idx = np.nonzero(active)[0]
            if not len(idx):
                break
            d, pd = solve(H[idx], g[idx])
            Xt = X[idx] + d
            Et, Ht, gt, valid, lint = evaluate(Xt, V[:, idx], ou[:, idx], ov[:, idx], w[:, idx])
            accept = pd & valid & (Et < E[idx])
            a = idx[accept]
            X[a], E[a], H[a], g[a] = Xt[accept], Et[accept], Ht[accept], gt[accept]
            lin[:, a] = lint[:, accept]
            moved[a] = True
            active[:] = False
            active[a] = True
    out = xin.copy().reshape(N, 4)
    out[moved, :3] = X[moved].astype(xin.dtype)
    copied = ~measured | few
    cost = np.stack([np.where(copied, 0.0, E0), np.where(copied, 0.0, E)], axis=1)
    codes = np.where(~measured, REFINE_MISSING, np.where(few, REFINE_FEW_VIEWS, np.where(moved, REFINE_MOVED, REFINE_KEPT))).astype(np.uint8)
    res = (out.reshape(xin.shape), cost.reshape(F, P, kn, 2), codes.reshape(F, P, kn))
    if return_views:
        mask = np.zeros(N, dtype=np.uint32)
        for c in range(C):
            mask |= V[c].astype(np.uint32) << np.uint32(c)
        res += (mask.reshape(F, P, kn),)
    if delta is not None:
        outl = np.zeros(N, dtype=np.uint32)
        for c in range(C):
            outl |= (lin[c] & ~copied).astype(np.uint32) << np.uint32(c)
        res += (outl.reshape(F, P, kn),)
    return res


def refine_joints(ctx, xyzs, kpts, det_of=None, n_persons=None, views=None, keypoint_score_threshold=0.0, iters=4, score_weights=False,
                  diagnostics=False, stream=None, huber_px=None):
    """k_refine through the context of the rig (_lib.Context): Context.refine_joints.  -> the refined records, or
    (records, cost, codes) with diagnostics=True; with a Huber loss (huber_px > 0) and diagnostics=True, (records, cost, codes,
    outliers)."""
    return ctx.refine_joints(xyzs, kpts, det_of=det_of, n_persons=n_persons, views=views, keypoint_score_threshold=keypoint_score_threshold,
                             iters=iters, score_weights=score_weights, diagnostics=diagnostics, stream=stream, huber_px=huber_px)


__all__ = ["refine_joints", "refine_joints_reference", "refine_args", "check_huber", "huber_terms", "REFINE_MISSING", "REFINE_FEW_VIEWS", "REFINE_KEPT", "REFINE_MOVED"]
