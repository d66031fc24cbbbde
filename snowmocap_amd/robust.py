"""Outlier-robust N-view triangulation: THE RULE of `method = DLT_ROBUST`, in NumPy.

`triangulate_robust_reference` is the definition the HIP kernel (k_dlt_robust, csrc/snowtri_robust.hpp) is tested against -- the
role tracking.track_persons_reference plays for the tracker.  It is not on the product path (BatchTriangulator runs the kernel)
and it is slow: an SVD per solve.

The rule (include/snowtri.h, snowtri_triangulate_robust, states it for the C ABI).  One detection per camera.  Per frame f and
joint j < keypoint_num, inputs converted to fp64, tau = reproj_threshold_px.  As in method = DLT the solve happens in the rig's own
frame: c = the mean of the camera centres (summed in camera order), s = max |t_c - c| over cameras and axes (1 if that is 0),
P[c] = K_c [R_c^T | -R_c^T (t_c - c) / s], and x below is the point in that frame (pixels do not depend on the frame):

1. S = {c : (n_persons is None or n_persons[f][c] > 0) and not (s_c < keypoint_score_threshold)}.  |S| < 2: the record is
   (0, 0, 0, 0), views = 0, resid = 0.
2. solve(S): x = the DLT solution over the views of S as method = DLT defines it (rows u P[c][2] - P[c][0], v P[c][2] - P[c][1];
   np.linalg.svd, last right singular vector, dehomogenised), X = c + s x; r_c^2 = (p0 / p2 - u_c)^2 + (p1 / p2 - v_c)^2 with
   p = P[c] (x, 1); m(S) = max_c r_c^2 (np.max: NaN if any is).
3. d = 0; while |S| >= 3 and d < max_drops and m(S) > tau^2: m_c = m(S \\ {c}) for every c in S in increasing c; drop c* = argmin:
   the lowest c starts as the best, a later candidate replaces it only if its m_c is strictly smaller, or if the best so far is NaN
   and m_c is not (ties go to the lowest c, a NaN never wins against a number); d += 1.
4. Joint = X(S), joint score = mean of s_c over S, views = bit mask of S, resid = sqrt(mean_{c in S} r_c^2) in pixels; person score =
   mean of the keypoint_num joint scores; count = 1; flags = FLAG_FASTPATH (what method = DLT writes).

With max_drops = 0 the rule is method = DLT.

DECISION MARGIN.  The kernel finds the same X by other arithmetic (A^T A, inverse iteration), so a comparison whose two sides agree
to rounding can come out the other way there.  The reference therefore reports, per joint, the smallest RELATIVE gap over the
decisions it took -- |m(S) - tau^2| / tau^2 at every loop test that reached the comparison, (second smallest m_c - smallest m_c) /
second smallest m_c at every drop -- and the index of that decision; `alternative_views` re-runs the joints below a margin with
that one decision taken the other way.  A test then demands equal masks wherever the margin is comfortable, and one of the two
masks elsewhere.
"""
from __future__ import annotations

import numpy as np

FLAG_FASTPATH = 4


def projection_matrices(K, R, t):
    """P[c] = K_c [R_c^T | -R_c^T t_c] (R camera->world, t the camera centre), [C, 3, 4] fp64."""
    K = np.asarray(K, dtype=np.float64)
    R = np.asarray(R, dtype=np.float64)
    C = K.shape[0]
    t = np.asarray(t, dtype=np.float64).reshape(C, 3)
    P = np.zeros((C, 3, 4))
    for c in range(C):
        Rt = R[c].T
        P[c] = K[c] @ np.concatenate([Rt, -(Rt @ t[c].reshape(3, 1))], axis=1)
    return P


def rig_frame(t):
    """-> (c, s): centre and scale of the frame the DLT is solved in (the rule above; oracle/dlt.py::rig_frame is the same)."""
    t = np.asarray(t, dtype=np.float64).reshape(-1, 3)
    c = np.zeros(3)
    for tc in t:                                    # summed in camera order
        c = c + tc
    c = c / t.shape[0]
    s = float(np.max(np.abs(t - c))) if t.size else 0.0
    return c, (s if s > 0.0 else 1.0)


def rig_projection_matrices(K, R, t):
    """-> (P [C, 3, 4], c, s) with P[c] = K_c [R_c^T | -R_c^T (t_c - c) / s]."""
    t = np.asarray(t, dtype=np.float64).reshape(-1, 3)
    c, s = rig_frame(t)
    return projection_matrices(K, R, (t - c) / s), c, s


def _solve(P, uv, masks):
    """P of rig_projection_matrices; uv [n, C, 2] fp64, masks [n] (every one with >= 2 bits) -> x [n, 3] in the rig's frame,
    r2 [n, C] (0 outside the mask), m [n]."""
    n, C = uv.shape[:2]
    X = np.zeros((n, 3))
    r2 = np.zeros((n, C))
    m = np.zeros(n)
    for mv in np.unique(masks):
        idx = np.nonzero(masks == mv)[0]
        cams = [c for c in range(C) if (int(mv) >> c) & 1]
        A = np.empty((len(idx), 2 * len(cams), 4))
        for k, c in enumerate(cams):
            A[:, 2 * k] = uv[idx, c, 0:1] * P[c, 2] - P[c, 0]
            A[:, 2 * k + 1] = uv[idx, c, 1:2] * P[c, 2] - P[c, 1]
        Xh = np.linalg.svd(A)[2][:, -1]
        with np.errstate(all="ignore"):
            Xg = Xh[:, :3] / Xh[:, 3:4]
            X[idx] = Xg
            rr = np.empty((len(idx), len(cams)))
            for k, c in enumerate(cams):
                p = Xg @ P[c, :, :3].T + P[c, :, 3]
                rr[:, k] = (p[:, 0] / p[:, 2] - uv[idx, c, 0]) ** 2 + (p[:, 1] / p[:, 2] - uv[idx, c, 1]) ** 2
                r2[idx, c] = rr[:, k]
            m[idx] = np.max(rr, axis=1)
    return X, r2, m


def _popcount(a):
    a = a.astype(np.uint32)
    return sum(((a >> c) & 1).astype(np.int32) for c in range(32))


def triangulate_robust_reference(K, R, t, kpts, n_persons, keypoint_score_threshold, keypoint_num, reproj_threshold_px, max_drops,
                                 _flip=None):
    """kpts [F, C, 1, J, 3] (float32 or float64), n_persons [F, C] or None ->
    dict(xyzs [F, 1, kn, 4] fp64, pscore [F, 1], count [F] int32, flags [F] uint32, views [F, kn] uint32, resid [F, kn] fp64,
         drops [F, kn] int32, margin [F, kn] fp64 (inf where no comparison was taken), decision [F, kn] int32 (-1 none)).
    _flip ([F, kn] int32, internal): the joint's decision of that index is taken the other way (alternative_views)."""
    kpts = np.asarray(kpts)
    F, C, Pm, J, _ = kpts.shape
    assert Pm == 1, "the robust rule is defined for one detection per camera"
    kn = int(keypoint_num)
    P, ctr, scl = rig_projection_matrices(K, R, t)
    tau = float(reproj_threshold_px)
    tau2 = tau * tau
    max_drops = int(max_drops)
    k64 = kpts[:, :, 0, :kn, :].astype(np.float64)                    # [F, C, kn, 3]
    N = F * kn
    uv = np.ascontiguousarray(np.moveaxis(k64[..., :2], 1, 2)).reshape(N, C, 2)
    sc = np.ascontiguousarray(np.moveaxis(k64[..., 2], 1, 2)).reshape(N, C)
    use = ~(sc < keypoint_score_threshold)
    if n_persons is not None:
        listed = np.asarray(n_persons).reshape(F, C) > 0
        use &= np.repeat(listed, kn, axis=0)
    S = np.zeros(N, dtype=np.uint32)
    for c in range(C):
        S |= (use[:, c].astype(np.uint32) << np.uint32(c))
    cnt = _popcount(S)
    ok = cnt >= 2
    X = np.zeros((N, 3))
    r2 = np.zeros((N, C))
    m = np.zeros(N)
    io = np.nonzero(ok)[0]
    if len(io):
        X[io], r2[io], m[io] = _solve(P, uv[io], S[io])
    d = np.zeros(N, dtype=np.int32)
    margin = np.full(N, np.inf)
    decision = np.full(N, -1, dtype=np.int32)
    ndec = np.zeros(N, dtype=np.int32)
    flip = np.full(N, -1, dtype=np.int32) if _flip is None else np.asarray(_flip, dtype=np.int32).reshape(N)

    def note(idx, rel):
        """decision `ndec` of the joints idx has the relative gap rel; -> which of them take it the other way"""
        lower = rel < margin[idx]
        margin[idx[lower]] = rel[lower]
        decision[idx[lower]] = ndec[idx[lower]]
        flipped = ndec[idx] == flip[idx]
        ndec[idx] += 1
        return flipped

    def loop_test(idx):
        """joints idx with |S| >= 3 and d < max_drops: m(S) > tau^2 ?"""
        with np.errstate(all="ignore"):
            cond = m[idx] > tau2
            rel = np.abs(m[idx] - tau2) / tau2
        rel = np.where(np.isfinite(rel), rel, np.inf)                 # (tau = 0 or inf, a NaN m: not a decision rounding can move)
        return cond ^ note(idx, rel)

    need = np.zeros(N, dtype=bool)
    el = np.nonzero(ok & (cnt >= 3) & (d < max_drops))[0]
    if len(el):
        need[el] = loop_test(el)
    while need.any():
        idx = np.nonzero(need)[0]
        n = len(idx)
        mc = np.full((n, C), np.nan)
        has = np.zeros((n, C), dtype=bool)
        Xc = np.zeros((n, C, 3))
        r2c = np.zeros((n, C, C))
        for c in range(C):
            sel = np.nonzero((S[idx] >> np.uint32(c)) & 1)[0]
            if not len(sel):
                continue
            has[sel, c] = True
            Xc[sel, c], r2c[sel, c], mc[sel, c] = _solve(P, uv[idx[sel]], S[idx[sel]] & ~np.uint32(1 << c))
        best = np.full(n, -1, dtype=np.int64)
        bm = np.zeros(n)
        for c in range(C):
            with np.errstate(all="ignore"):
                win = has[:, c] & ((best < 0) | (mc[:, c] < bm) | (np.isnan(bm) & ~np.isnan(mc[:, c])))
            best[win] = c
            bm[win] = mc[win, c]
        # the runner-up (what the drop would have been had the best been a little worse), and the gap to it
        rest = np.where(has, mc, np.nan)
        rest[np.arange(n), best] = np.nan
        second = np.full(n, -1, dtype=np.int64)
        sm = np.full(n, np.inf)
        for c in range(C):
            with np.errstate(all="ignore"):
                win = ~np.isnan(rest[:, c]) & ((second < 0) | (rest[:, c] < sm))
            second[win] = c
            sm[win] = rest[win, c]
        with np.errstate(all="ignore"):
            rel = (sm - bm) / sm
        rel = np.where((second >= 0) & np.isfinite(rel), rel, np.inf)
        flipped = note(idx, rel) & (second >= 0)
        pick = np.where(flipped, second, best)
        ar = np.arange(n)
        S[idx] &= ~(np.uint32(1) << pick.astype(np.uint32))
        X[idx] = Xc[ar, pick]
        r2[idx] = r2c[ar, pick]
        m[idx] = mc[ar, pick]
        cnt[idx] -= 1
        d[idx] += 1
        need[:] = False
        el = idx[(cnt[idx] >= 3) & (d[idx] < max_drops)]
        if len(el):
            need[el] = loop_test(el)

    out = np.zeros((F, 1, kn, 4))
    resid = np.zeros(N)
    flat = out.reshape(N, 4)
    for i in io:
        cams = [c for c in range(C) if (int(S[i]) >> c) & 1]
        flat[i, :3] = ctr + scl * X[i]
        flat[i, 3] = np.mean([sc[i, c] for c in cams])
        with np.errstate(all="ignore"):
            resid[i] = np.sqrt(np.mean([r2[i, c] for c in cams]))
    views = np.where(ok, S, np.uint32(0)).astype(np.uint32)
    pscore = out[:, :, :, 3].mean(axis=2) if kn else np.full((F, 1), np.nan)
    return dict(xyzs=out, pscore=pscore, count=np.ones(F, dtype=np.int32), flags=np.full(F, FLAG_FASTPATH, dtype=np.uint32),
                views=views.reshape(F, kn), resid=resid.reshape(F, kn), drops=d.reshape(F, kn), margin=margin.reshape(F, kn),
                decision=decision.reshape(F, kn))


def alternative_views(K, R, t, kpts, n_persons, keypoint_score_threshold, keypoint_num, reproj_threshold_px, max_drops, ref, below=1e-6):
    """views [F, kn] the rule gives when every joint whose margin is under `below` takes its closest decision the other way
    (equal to ref["views"] everywhere else).  `ref` is the result of triangulate_robust_reference on the same arguments."""
    close = ref["margin"] < below
    if not close.any():
        return ref["views"].copy()
    alt = triangulate_robust_reference(K, R, t, kpts, n_persons, keypoint_score_threshold, keypoint_num, reproj_threshold_px, max_drops,
                                       _flip=np.where(close, ref["decision"], -1))
    return np.where(close, alt["views"], ref["views"]).astype(np.uint32)
