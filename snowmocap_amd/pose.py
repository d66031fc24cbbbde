"""Camera pose refinement: the rig's extrinsics repaired from the joints the rig itself tracked.

K, R, t come from a calibration file and are trusted for a whole recording.  A rig does not hold still: a tripod is nudged, a mount
sags, and one camera ends up half a degree off.  `view_residuals` shows it -- the nudged camera's RMS stands out -- and this module
repairs it: the reprojection cost of `refine_joints`, minimised over the other block of unknowns, each camera's six pose parameters,
with the joints held fixed.  Alternated with triangulation (`refine_rig`) that is block-coordinate bundle adjustment of the
extrinsics.

The rule is stated in include/snowtri.h ("Camera pose refinement").  `refine_cameras_reference` is that rule in NumPy: plain
operations in its order (no fused multiply-add), a camera's observations summed in record order, no GPU, no library; it is what the
host tests check and what the kernels k_pose_normal / k_pose_step (snowmocap_amd/csrc/snowtri_pose.hpp) are compared with.
`refine_cameras` runs the kernels.

What it buys, on a synthetic recipe (tests/pose_cases.py::recipe: synth.ring_rig(8), two persons on the 1.5 m circle, 40 frames x 17
joints, 1 px of noise, camera 3 off by 0.5 degrees and 2 cm and the only free one; not footage), `refine_rig` driven by the NumPy
rules with a plain DLT as the triangulation: that camera's view RMS goes from 3.90 px (the others: 1.35 .. 1.62 px) to 1.55 px after
one round and 1.32 px after two (the others: 1.27 .. 1.34), its rotation error from 7.5e-3 over 1.3e-3 to 9.9e-4, its position error
from 20.0 over 13.6 to 8.9 mm.

THE GAUGE.  Joints and cameras together are determined only up to a rigid motion and a scale of the whole scene, so `refine_rig`
requires at least one camera to stay.  With only ONE camera held (a user who does not know which one moved) the bad camera's RMS
still falls in the first round, but the scale is then held by nothing but the noise and the rig creeps slowly round after round:
hold every camera that is trusted, and do not run more rounds than the RMS needs.

THE HUBER LOSS (huber_px; None or 0: the squared loss, today's bits): the loss of refine.py per observation, E_c = sum w rho, H and g
with the IRLS weights w kappa; the report gains n_outliers [C], the observations in the linear regime at the output pose.  A `views`
mask from DLT_ROBUST is no substitute here: its leave-one-out gate removes exactly the nudged camera's views, the observations the
pose step needs; the loss keeps them and down-weights the far ones.  On pose_cases.case with 10 % of the detections moved by
20-150 px the squared loss leaves the free cameras 2e-2 .. 4e-2 from the truth, delta = 3 px 1e-3 .. 3e-3 (tests/test_huber_host.py).

INTRINSICS (intrinsics="f", "c" or "fc"; None, the default: nothing changes anywhere).  A chessboard K a percent or two off, or a lens
refocused after calibration, is as common as a nudged tripod, and pose-only refinement HIDES it: on the recipe with camera 3's pose
true, its fx, fy 2 % high and its centre off by (8, -5) px, freeing only its pose brings its view RMS from 8.4 px to the noise by moving
a correct camera by centimetres, and view_rms then reports a healthy rig (EXPERIMENTS.md has the table).  The keyword adds fx, fy ("f")
and / or cx, cy ("c") to a camera's parameters (include/snowtri.h, INTRINSICS; snowtri_refine_cameras_k, k_pose_normal_k /
k_pose_step_k): ten parameters omega, tau, fx, fy, cx, cy, the free ones solved for together, K returned beside R and t.
intrinsics_free names the cameras whose intrinsics may move (None: all) and is independent of `free`: a camera that holds the gauge
may still have its K refined.  THE LIMITS: ten parameters need thousands of observations -- the principal point and the rotation are
strongly correlated (a shift of the centre and a small pan move the pixels almost alike), and with some 150 noisy observations per
camera all ten end as far from the truth as they started; free fewer, hold the pose, or record longer.  Pose-only refinement of a camera
whose K is wrong lowers its RMS by moving it.  With a lens (D != 0) the detections were undistorted with the OLD K and must be
undistorted again from the raw frame once K has moved; refine_rig does not do that.

Not offered: lens coefficients, the skew, a focal length shared between cameras, other losses (Cauchy, Tukey), an automatic delta,
damping, points and cameras adjusted in one system, ShardedTrackPipeline, more than 32 cameras.
"""
from __future__ import annotations

import numpy as np

from . import _lib
from ._lib import POSE_FEW_OBS, POSE_FIXED, POSE_KEPT, POSE_MOVED, free_mask  # noqa: F401
from .records import missing_records  # noqa: F401
from .refine import _check_iters, check_huber, huber_terms, observation_sets, project_camera  # noqa: F401  (rule 1, the projection and the loss are stated there, once)
from .reproject import _rig

H_INDEX = [(a, b) for a in range(6) for b in range(a + 1)]      # normal[7 + k] = H[a][b]: the lower triangle row by row
H_INDEX_K = [(a, b) for a in range(10) for b in range(a + 1)]   # with intrinsics: normal[11 + k] = H[a][b] over omega, tau, fx, fy, cx, cy
INTR_FOCAL, INTR_CENTRE = 1, 2                                   # SNOWTRI_INTR_FOCAL, SNOWTRI_INTR_CENTRE


def _check_min_obs(min_obs):
    if int(min_obs) != min_obs or int(min_obs) < 3:
        raise ValueError(f"min_obs must be an integer >= 3 (got {min_obs})")
    return int(min_obs)


def _ordered_sum(a):
    """The sum over axis 0 in index order (np.sum adds pairwise)."""
    return np.cumsum(a, axis=0)[-1] if a.shape[0] else np.zeros(a.shape[1:])


def rodrigues(omega):
    """Exp(omega) [3, 3] by the rule's formula: a = sin(th) / th, b = 2 sin^2(th / 2) / th^2, a = 1 and b = 1/2 at th = 0."""
    o0, o1, o2 = (float(v) for v in omega)
    th2 = (o0 * o0 + o1 * o1) + o2 * o2
    th = np.sqrt(th2)
    a, b = 1.0, 0.5
    if th > 0.0:
        sh = np.sin(0.5 * th)
        a = np.sin(th) / th
        b = (2.0 * (sh * sh)) / th2
    W = np.array([[0.0, -o2, o1], [o2, 0.0, -o0], [-o1, o0, 0.0]])
    E = np.empty((3, 3))
    for i in range(3):
        for j in range(3):
            w2 = (W[i, 0] * W[0, j] + W[i, 1] * W[1, j]) + W[i, 2] * W[2, j]
            E[i, j] = ((1.0 if i == j else 0.0) + a * W[i, j]) + b * w2
    return E


def apply_delta(Rc, tc, delta):
    """Rule 2: (Exp(omega) R_c, t_c + tau), every product-sum in plain operations."""
    E = rodrigues(delta[:3])
    Rn = np.empty((3, 3))
    for i in range(3):
        for j in range(3):
            Rn[i, j] = (E[i, 0] * Rc[0, j] + E[i, 1] * Rc[1, j]) + E[i, 2] * Rc[2, j]
    return Rn, np.array([tc[0] + delta[3], tc[1] + delta[4], tc[2] + delta[5]])


def pose_jacobian(Kc, Rc, tc, X):
    """Rule 3's analytic Jacobian at delta = 0: X [n, 3] -> du [n, 6], dv [n, 6] (columns: omega, tau)."""
    x, y, pc2, _, _, _ = project_camera(Kc, Rc, tc, X)
    d = [X[:, 0] - tc[0], X[:, 1] - tc[1], X[:, 2] - tc[2]]
    du, dv = np.empty((X.shape[0], 6)), np.empty((X.shape[0], 6))
    for k in range(6):
        if k < 3:                                   # column k of R^T [d]x = R^T (d x e_k)
            m, n = (k + 1) % 3, (k + 2) % 3
            a = [Rc[m, i] * d[n] - Rc[n, i] * d[m] for i in range(3)]
        else:                                       # column k - 3 of -R^T
            a = [-Rc[k - 3, i] * np.ones_like(x) for i in range(3)]
        dx, dy = (a[0] - x * a[2]) / pc2, (a[1] - y * a[2]) / pc2
        du[:, k] = Kc[0, 0] * dx + Kc[0, 1] * dy
        dv[:, k] = Kc[1, 1] * dy
    return du, dv


def linear_regime(Kc, Rc, tc, X, ou, ov, delta):
    """Which of one camera's observations are in the linear regime of the Huber loss delta at the pose (Rc, tc) -> [n] bool."""
    _, _, _, u, v, _ = project_camera(Kc, Rc, tc, X)
    ru, rv = u - ou, v - ov
    return huber_terms(ru * ru + rv * rv, delta)[2]


def normal_terms(Kc, Rc, tc, X, ou, ov, w, delta=None):
    """One camera's observations X [n, 3], (ou, ov, w) [n] at the pose (Rc, tc) -> terms [n, 28]: every observation's share of
    E, g[6], H[21] (the lower triangle row by row), and valid [n].  delta: None (the squared loss) or the Huber loss' delta > 0:
    E sums w rho, g and H carry the IRLS weight w kappa."""
    _, _, _, u, v, ok = project_camera(Kc, Rc, tc, X)
    du, dv = pose_jacobian(Kc, Rc, tc, X)
    ru, rv = u - ou, v - ov
    terms = np.empty((X.shape[0], 28))
    if delta is None:
        terms[:, 0] = w * (ru * ru + rv * rv)
    else:
        rho, kappa, _ = huber_terms(ru * ru + rv * rv, delta)
        terms[:, 0] = w * rho
        w = w * kappa
    for a in range(6):
        terms[:, 1 + a] = w * (du[:, a] * ru + dv[:, a] * rv)
    for k, (a, b) in enumerate(H_INDEX):
        terms[:, 7 + k] = w * (du[:, a] * du[:, b] + dv[:, a] * dv[:, b])
    return terms, ok


def evaluate_camera(Kc, Rc, tc, X, ou, ov, w, delta=None):
    """-> normal [28] = E, g[6], H[21], the terms summed in record order, and whether every observation is valid at that pose."""
    terms, ok = normal_terms(Kc, Rc, tc, X, ou, ov, w, delta)
    return _ordered_sum(terms), bool(ok.all())


def solve_normal(normal):
    """H delta = -g by a 6 x 6 LDL^T in plain operations -> delta [6], every pivot finite and > 0."""
    H = np.zeros((6, 6))
    for k, (a, b) in enumerate(H_INDEX):
        H[a, b] = normal[7 + k]
    g = normal[1:7]
    L, piv, y, delta = np.zeros((6, 6)), np.zeros(6), np.zeros(6), np.zeros(6)
    pd = True
    with np.errstate(all="ignore"):
        for a in range(6):
            for b in range(a + 1):
                s = H[a, b]
                for k in range(b):
                    s = s - L[a, k] * (L[b, k] * piv[k])
                if b < a:
                    L[a, b] = s / piv[b]
                else:
                    piv[a] = s
            pd = pd and bool(piv[a] > 0.0) and bool(np.isfinite(piv[a]))
        for a in range(6):
            s = -g[a]
            for k in range(a):
                s = s - L[a, k] * y[k]
            y[a] = s
        for a in range(5, -1, -1):
            s = y[a] / piv[a]
            for k in range(a + 1, 6):
                s = s - L[k, a] * delta[k]
            delta[a] = s
    return delta, pd


def intrinsics_flags(intrinsics):
    """intrinsics: None, "f", "c" or "fc" -> snowtri_refine_cameras_k's intr_flags (0 for None)."""
    if intrinsics is None:
        return 0
    if not isinstance(intrinsics, str) or intrinsics not in ("f", "c", "fc"):
        raise ValueError(f'intrinsics must be None, "f", "c" or "fc" (got {intrinsics!r})')
    return (INTR_FOCAL if "f" in intrinsics else 0) | (INTR_CENTRE if "c" in intrinsics else 0)


def free_set(pose_free, flags):
    """The free parameters of a camera, in the rule's order: the pose if pose_free, fx fy with INTR_FOCAL, cx cy with INTR_CENTRE."""
    return (list(range(6)) if pose_free else []) + ([6, 7] if flags & INTR_FOCAL else []) + ([8, 9] if flags & INTR_CENTRE else [])


def normal_terms_k(Kc, Rc, tc, X, ou, ov, w, delta=None):
    """normal_terms over ten parameters (INTRINSICS) -> terms [n, 66]: every observation's share of E, g[10], H[55], and valid [n]."""
    x, y, _, u, v, ok = project_camera(Kc, Rc, tc, X)
    du6, dv6 = pose_jacobian(Kc, Rc, tc, X)
    one, zero = np.ones_like(x), np.zeros_like(x)
    du = np.concatenate([du6, np.stack([x, zero, one, zero], axis=1)], axis=1)
    dv = np.concatenate([dv6, np.stack([zero, y, zero, one], axis=1)], axis=1)
    ru, rv = u - ou, v - ov
    terms = np.empty((X.shape[0], 66))
    if delta is None:
        terms[:, 0] = w * (ru * ru + rv * rv)
    else:
        rho, kappa, _ = huber_terms(ru * ru + rv * rv, delta)
        terms[:, 0] = w * rho
        w = w * kappa
    for a in range(10):
        terms[:, 1 + a] = w * (du[:, a] * ru + dv[:, a] * rv)
    for k, (a, b) in enumerate(H_INDEX_K):
        terms[:, 11 + k] = w * (du[:, a] * du[:, b] + dv[:, a] * dv[:, b])
    return terms, ok


def evaluate_camera_k(Kc, Rc, tc, X, ou, ov, w, delta=None):
    """-> normal [66] = E, g[10], H[55], the terms summed in record order, and whether every observation is valid there."""
    terms, ok = normal_terms_k(Kc, Rc, tc, X, ou, ov, w, delta)
    return _ordered_sum(terms), bool(ok.all())


def solve_normal_k(normal, idx):
    """H delta = -g over the rows and columns idx (the free set, in order) of normal [66], by solve_normal's LDL^T at size
    n = len(idx) in plain operations -> delta [10] (0 outside idx), every pivot finite and > 0."""
    n = len(idx)
    H = np.zeros((10, 10))
    for k, (a, b) in enumerate(H_INDEX_K):
        H[a, b] = normal[11 + k]
    g = normal[1:11]
    L, piv, y, d = np.zeros((n, n)), np.zeros(n), np.zeros(n), np.zeros(n)
    pd = True
    with np.errstate(all="ignore"):
        for a in range(n):
            for b in range(a + 1):
                s = H[idx[a], idx[b]]
                for k in range(b):
                    s = s - L[a, k] * (L[b, k] * piv[k])
                if b < a:
                    L[a, b] = s / piv[b]
                else:
                    piv[a] = s
            pd = pd and bool(piv[a] > 0.0) and bool(np.isfinite(piv[a]))
        for a in range(n):
            s = -g[idx[a]]
            for k in range(a):
                s = s - L[a, k] * y[k]
            y[a] = s
        for a in range(n - 1, -1, -1):
            s = y[a] / piv[a]
            for k in range(a + 1, n):
                s = s - L[k, a] * d[k]
            d[a] = s
    delta = np.zeros(10)
    for a in range(n):
        delta[idx[a]] = d[a]
    return delta, pd


def apply_delta_k(Kc, Rc, tc, delta, idx):
    """The trial of INTRINSICS: (K, Exp(omega) R, t + tau) with fx + d6, fy + d7, cx + d8, cy + d9; a parameter outside idx keeps its
    bits."""
    Kn, Rn, tn = np.array(Kc, copy=True), Rc, tc
    if 0 in idx:
        Rn, tn = apply_delta(Rc, tc, delta[:6])
    if 6 in idx:
        Kn[0, 0], Kn[1, 1] = Kc[0, 0] + delta[6], Kc[1, 1] + delta[7]
    if 8 in idx:
        Kn[0, 2], Kn[1, 2] = Kc[0, 2] + delta[8], Kc[1, 2] + delta[9]
    return Kn, Rn, tn


def _refine_cameras_reference_k(K, R, t, xyzs, kpts, det_of, n_persons, views, keypoint_score_threshold, free, min_obs, iters, score_weights,
                                return_sets, huber_px, flags, intrinsics_free):
    """refine_cameras_reference with intrinsics set: the rule of INTRINSICS."""
    K, R, t, _, C = _rig(K, R, t, None)
    iters = _check_iters(iters)
    hub = check_huber(huber_px)
    min_obs = _check_min_obs(min_obs)
    mask, imask = free_mask(free, C), free_mask(intrinsics_free, C)
    X, S, obs = observation_sets(K, R, t, xyzs, kpts, det_of, n_persons, views, keypoint_score_threshold, score_weights)
    K_out, R_out, t_out = np.array(K, dtype=np.float64, copy=True), np.array(R, copy=True), np.array(t, copy=True)
    cost, n_obs = np.zeros((C, 2)), np.zeros(C, dtype=np.int64)
    codes, normal, steps = np.zeros(C, dtype=np.uint8), np.zeros((C, 66)), np.zeros(C, dtype=np.int64)
    n_outliers = np.zeros(C, dtype=np.int64)
    with np.errstate(all="ignore"):
        for c in range(C):
            Xc, ou, ov, w = X[S[c]], obs[c, S[c], 0], obs[c, S[c], 1], obs[c, S[c], 2]
            n_obs[c] = len(Xc)
            Kc, Rc, tc = K_out[c].copy(), R[c], t[c]
            cur, _ = evaluate_camera_k(Kc, Rc, tc, Xc, ou, ov, w, hub)
            normal[c] = cur
            idx = free_set((mask >> c) & 1, flags if (imask >> c) & 1 else 0)
            if not idx:
                codes[c] = POSE_FIXED
                continue
            if n_obs[c] < min_obs:
                codes[c] = POSE_FEW_OBS
                continue
            codes[c] = POSE_KEPT
            cost[c, 0] = cur[0]
            for _ in range(iters):
                delta, pd = solve_normal_k(cur, idx)
                if not pd:
                    break
                Kt, Rt, tt = apply_delta_k(Kc, Rc, tc, delta, idx)
                nxt, valid = evaluate_camera_k(Kt, Rt, tt, Xc, ou, ov, w, hub)
                focal_ok = Kt[0, 0] > 0.0 and np.isfinite(Kt[0, 0]) and Kt[1, 1] > 0.0 and np.isfinite(Kt[1, 1])
                if not (valid and focal_ok and nxt[0] < cur[0]):
                    break
                Kc, Rc, tc, cur = Kt, Rt, tt, nxt
                codes[c] = POSE_MOVED
                steps[c] += 1
            cost[c, 1] = cur[0]
            K_out[c], R_out[c], t_out[c] = Kc, Rc, tc
            if hub is not None:
                n_outliers[c] = int(linear_regime(Kc, Rc, tc, Xc, ou, ov, hub).sum())
    report = dict(cost=cost, n_obs=n_obs, codes=codes, normal=normal, steps=steps)
    if hub is not None:
        report["n_outliers"] = n_outliers
    return (K_out, R_out, t_out, report, S) if return_sets else (K_out, R_out, t_out, report)


def refine_cameras_reference(K, R, t, xyzs, kpts, det_of=None, n_persons=None, views=None, keypoint_score_threshold=0.0, free=None,
                             min_obs=64, iters=8, score_weights=False, return_sets=False, huber_px=None, intrinsics=None,
                             intrinsics_free=None):
    """The rule in NumPy: xyzs [F, P, kn, 4], kpts [F, C, Pmax, kn, 3], det_of [F, C, P] or None, n_persons [F, C] or None, views
    [F, P, kn] or None; free: None (all), a bit mask, C booleans or camera indices ->
    (R [C, 3, 3], t [C, 3], report) with report = dict(cost [C, 2], n_obs [C] int64, codes [C] uint8, normal [C, 28], steps [C]: the
    steps accepted); with return_sets also S [C, N] bool, the observation sets.  huber_px (delta > 0; None or 0: the squared loss,
    and no new key): the Huber loss of ROBUST LOSS, and report["n_outliers"] [C] int64, the observations of S_c in the linear
    regime at the output pose (0 for FIXED and FEW_OBS cameras).  intrinsics ("f": fx and fy, "c": cx and cy, "fc"; None, the
    default: everything above, unchanged): the rule of INTRINSICS -> (K [C, 3, 3], R, t, report[, S]) with report["normal"] [C, 66] =
    E, g[10], H[55] (H_INDEX_K) at the input; intrinsics_free: the cameras whose intrinsics may move -- None (all), a bit mask, C
    booleans or camera indices -- independent of `free`."""
    flags = intrinsics_flags(intrinsics)
    if flags:
        return _refine_cameras_reference_k(K, R, t, xyzs, kpts, det_of, n_persons, views, keypoint_score_threshold, free, min_obs, iters,
                                           score_weights, return_sets, huber_px, flags, intrinsics_free)
    K, R, t, _, C = _rig(K, R, t, None)
    iters = _check_iters(iters)
    hub = check_huber(huber_px)
    min_obs = _check_min_obs(min_obs)
    mask = free_mask(free, C)
    X, S, obs = observation_sets(K, R, t, xyzs, kpts, det_of, n_persons, views, keypoint_score_threshold, score_weights)
    R_out, t_out = np.array(R, copy=True), np.array(t, copy=True)
    cost, n_obs = np.zeros((C, 2)), np.zeros(C, dtype=np.int64)
    codes, normal, steps = np.zeros(C, dtype=np.uint8), np.zeros((C, 28)), np.zeros(C, dtype=np.int64)
    n_outliers = np.zeros(C, dtype=np.int64)
    with np.errstate(all="ignore"):
        for c in range(C):
            Xc, ou, ov, w = X[S[c]], obs[c, S[c], 0], obs[c, S[c], 1], obs[c, S[c], 2]
            n_obs[c] = len(Xc)
            cur, _ = evaluate_camera(K[c], R[c], t[c], Xc, ou, ov, w, hub)
            normal[c] = cur
            if not (mask >> c) & 1:
                codes[c] = POSE_FIXED
                continue
            if n_obs[c] < min_obs:
                codes[c] = POSE_FEW_OBS
                continue
            codes[c] = POSE_KEPT
            Rc, tc = R[c], t[c]
            cost[c, 0] = cur[0]
            for _ in range(iters):
                delta, pd = solve_normal(cur)
                if not pd:
                    break
                Rt, tt = apply_delta(Rc, tc, delta)
                nxt, valid = evaluate_camera(K[c], Rt, tt, Xc, ou, ov, w, hub)
                if not (valid and nxt[0] < cur[0]):
                    break
                Rc, tc, cur = Rt, tt, nxt
                codes[c] = POSE_MOVED
                steps[c] += 1
            cost[c, 1] = cur[0]
            R_out[c], t_out[c] = Rc, tc
            if hub is not None:
                n_outliers[c] = int(linear_regime(K[c], Rc, tc, Xc, ou, ov, hub).sum())
    report = dict(cost=cost, n_obs=n_obs, codes=codes, normal=normal, steps=steps)
    if hub is not None:
        report["n_outliers"] = n_outliers
    return (R_out, t_out, report, S) if return_sets else (R_out, t_out, report)


def refine_cameras(ctx, xyzs, kpts, det_of=None, n_persons=None, views=None, keypoint_score_threshold=0.0, free=None, min_obs=64, iters=8,
                   score_weights=False, diagnostics=False, stream=None, huber_px=None, intrinsics=None, intrinsics_free=None):
    """k_pose_normal / k_pose_step through the context of the rig (_lib.Context): Context.refine_cameras.  -> (R, t), or
    (R, t, report) with diagnostics=True; the context's own rig is not changed.  huber_px > 0: the Huber loss, and the report gains
    n_outliers [C].  intrinsics ("f", "c", "fc"; None: nothing changes): k_pose_normal_k / k_pose_step_k, -> (K, R, t) or
    (K, R, t, report) with report["normal"] [C, 66]; intrinsics_free: the cameras whose intrinsics may move (None: all)."""
    kw = dict(det_of=det_of, n_persons=n_persons, views=views, keypoint_score_threshold=keypoint_score_threshold, free=free, min_obs=min_obs,
              iters=iters, score_weights=score_weights, diagnostics=diagnostics, stream=stream, huber_px=huber_px)
    if intrinsics is not None:
        kw.update(intrinsics=intrinsics, intrinsics_free=intrinsics_free)
    return ctx.refine_cameras(xyzs, kpts, **kw)


# ------------------------------------------------------------------------------------------------ the alternation
class _LibrarySteps:
    """The four steps of one round of refine_rig on the GPU, from the library's public pieces (host arrays in and out)."""

    def __init__(self, method, params, P):
        self.method, self.params, self.P = method, params, P

    def triangulate(self, K, R, t, kpts, n_persons):
        from .batch import BatchTriangulator
        bt = BatchTriangulator(K, R, t, self.params, pout_max=self.P, out_dtype=np.float64, method=self.method)
        try:
            res = bt.run_host(kpts, n_persons)
        finally:
            bt.close()
        if res["status"] != _lib.ERR_OVERFLOW:            # (a frame with more clusters than `persons` keeps `persons` of them: a nudged
            _lib.check(res["status"], "refine_rig: triangulation")   # camera splits a person in two until it is repaired)
        self.overflow_frames = int(((res["flags"] & _lib.FLAG_OVERFLOW) != 0).sum())   # ... and the round's history says how many
        return res["xyzs"]

    def open(self, K, R, t):
        self.K, self.ctx = K, _lib.Context(K, R, t)

    def close(self):
        self.ctx.close()

    def cost(self, xyzs, kpts, n_persons, thr):
        return self.ctx.reproject_cost(xyzs, kpts, n_persons=n_persons, keypoint_score_threshold=thr)

    def assign(self, cost_sum, cost_n, gate_px, min_joints):
        from .reproject import assign_detections
        return assign_detections(self.ctx, cost_sum, cost_n, gate_px, min_joints)

    def pixels(self, xyzs):
        return self.ctx.reproject(xyzs, dtype=np.float64)

    def matched(self, kpts, det_of, n_persons, thr):
        return self.ctx.triangulate_matched(kpts, det_of=det_of, n_persons=n_persons, keypoint_score_threshold=thr, dtype=np.float64,
                                            diagnostics=True)

    def joints(self, xyzs, kpts, **kw):
        return self.ctx.refine_joints(xyzs, kpts, **kw)

    def cameras(self, xyzs, kpts, **kw):
        out = self.ctx.refine_cameras(xyzs, kpts, diagnostics=True, **kw)
        return out if len(out) == 4 else (self.K,) + tuple(out)


class _ReferenceSteps:
    """The same steps by the NumPy rules (no GPU); the triangulation is the caller's."""

    def __init__(self, triangulate):
        self.triangulate = triangulate

    def open(self, K, R, t):
        self.rig = (K, R, t)

    def close(self):
        pass

    def cost(self, xyzs, kpts, n_persons, thr):
        from .reproject import reprojection_cost_reference
        return reprojection_cost_reference(*self.rig, xyzs, kpts, n_persons=n_persons, keypoint_score_threshold=thr)

    def assign(self, cost_sum, cost_n, gate_px, min_joints):
        from .reproject import assign_detections_reference
        return assign_detections_reference(cost_sum, cost_n, gate_px, min_joints)[0]

    def pixels(self, xyzs):
        from .reproject import reproject_reference
        return reproject_reference(*self.rig, xyzs)

    def matched(self, kpts, det_of, n_persons, thr):
        from .matched import triangulate_matched_reference
        ref = triangulate_matched_reference(*self.rig, kpts, det_of, n_persons, thr)
        return ref["xyzs"], ref["pscore"], ref["views"], ref["resid"]

    def joints(self, xyzs, kpts, **kw):
        from .refine import refine_joints_reference
        return refine_joints_reference(*self.rig, xyzs, kpts, **kw)[0]

    def cameras(self, xyzs, kpts, **kw):
        out = refine_cameras_reference(*self.rig, xyzs, kpts, **kw)
        return out if len(out) == 4 else (self.rig[0],) + tuple(out)


def refine_rig(K, R, t, kpts, n_persons=None, free=None, rounds=2, method=_lib.DLT, params=None, persons=None, gate_px=12.0,
               min_joints=8, joint_iters=4, camera_iters=8, min_obs=64, score_weights=False, triangulate=None, reference=False,
               one_to_one=False, retriangulate=False, huber_px=None, intrinsics=None, intrinsics_free=None):
    """Block-coordinate bundle adjustment of the extrinsics: `rounds` times triangulate on the current rig, match the detections to the
    3D persons (reprojection_cost + match_detections, gate_px), refine the joints (refine_joints, joint_iters), refine the free cameras
    (refine_cameras, camera_iters, min_obs), and build a new context from the result.  Host arrays: kpts [F, C, Pmax, kn, 3] on the
    UNDISTORTED frame, n_persons [F, C] or None.

    free (REQUIRED): the cameras that may move, as a bit mask, C booleans or camera indices.  It must leave at least one camera out --
    the gauge: joints and cameras together are determined only up to a rigid motion and a scale.  Hold every camera that is trusted:
    with only one held, the bad camera's RMS still falls in the first round, but the rig then creeps slowly round after round.
    params: the triangulation's thresholds (default: the function-signature defaults with keypoint_num = kn and the centre joint
    min(18, kn - 1)); persons: the 3D persons per frame (default Pmax).  CALIBRATE ON A SINGLE-PERSON RECORDING (Pmax = 1: every
    camera's detection is the same person and the DLT takes every view).  With several persons per frame the triangulation first
    has to associate detections across cameras with the very rig that is wrong: a camera half a degree off misses a joint 5 m away
    by 4 cm, its ray pairs fall outside distance_threshold or form a second cluster, and on the two-person recipe the alternation
    did not repair it (EXPERIMENTS.md).  triangulate(K, R, t, kpts, n_persons) -> xyzs [F, P, kn, 4]
    replaces the BatchTriangulator; reference=True runs every other step by its NumPy rule (no GPU; needs `triangulate`).
    one_to_one=True: the matching step is the optimal one-to-one assignment (reproject.assign_detections, k_assign; with reference=True
    its NumPy rule assign_detections_reference) instead of match_detections, with the same gate_px and min_joints; gate_px must
    then not exceed 1e150, since staying unmatched costs gate_px^2 (ValueError before any work).
    retriangulate=True: each round triangulates every person again from the round's det_of before refine_joints
    (matched.triangulate_matched, k_dlt_matched, with the robust defaults 6.0 px and 1 drop; with reference=True its NumPy rule
    triangulate_matched_reference), so a person is fused from every view the matcher gave it, not only from those the first
    triangulation associated.  A joint the second pass made from at least 2 views replaces the first pass's record, every other
    record is kept (matched.merge_records), and the views mask -- all ones on a kept record -- is passed on to refine_joints and
    refine_cameras.  It does NOT repair the two-person recipe above (measured: the same view RMS per round with and without, the
    first triangulation has already split the persons: EXPERIMENTS.md round 28).  False (the default): nothing changes.
    huber_px (delta > 0 in pixels; None or 0, the default: the squared loss, nothing changes): the Huber loss of ROBUST LOSS in both
    the joint step and the camera step of every round, in the library steps and the reference=True steps alike; finite, >= 0 and at
    most 1e150 (ValueError before any work).
    intrinsics ("f": fx and fy, "c": cx and cy, "fc"; None, the default: nothing changes) and intrinsics_free (the cameras whose
    intrinsics may move; None: all; independent of `free`, so the gauge camera's K may be refined): the camera step also solves for
    those intrinsics (INTRINSICS above and in include/snowtri.h) and K is carried from round to round, in the library steps and the
    reference=True steps alike; the result is then (K [C, 3, 3], R, t, history).  The detections stay the ones handed in: with a
    lens they were undistorted with the old K and should be undistorted again from the raw frame once K has moved.

    -> (R [C, 3, 3], t [C, 3], history): history[r] = dict(overflow_frames: the frames in which the library's triangulation found
    more clusters than `persons` and dropped some (0 with the caller's `triangulate`), view_rms [C]: each camera's RMS pixel residual over its matched views
    BEFORE round r's pose step, cost [C, 2], n_obs [C], codes [C]: that step's report), and a last entry with the view_rms of the
    returned rig alone."""
    from .reproject import match_detections, view_residuals
    K, R, t, _, C = _rig(K, R, t, None)
    if free is None:
        raise ValueError("refine_rig: free is required (the cameras that may move)")
    mask = free_mask(free, C)
    if mask == (1 << C) - 1:
        raise ValueError("refine_rig: free must leave at least one camera out (the gauge: a rigid motion and a scale of the whole scene)")
    if int(rounds) != rounds or int(rounds) < 1:
        raise ValueError("refine_rig: rounds must be an integer >= 1")
    kpts = _lib.host_floats(kpts)
    if kpts.ndim != 5 or kpts.shape[1] != C or kpts.shape[-1] != 3:
        raise ValueError(f"kpts must be [F, C={C}, Pmax, kn, 3] (got shape {kpts.shape})")
    F, _, Pmax, kn, _ = kpts.shape
    P = Pmax if persons is None else int(persons)
    if n_persons is not None:
        n_persons = np.ascontiguousarray(n_persons, dtype=np.int32).reshape(F, C)
    if params is None:
        params = dict(keypoint_num=kn, center_point_index=min(18, kn - 1))
    thr = float(params.get("keypoint_score_threshold", 0.5)) if isinstance(params, dict) else float(params.keypoint_score_threshold)
    if one_to_one:
        from .reproject import assign_gate
        assign_gate(gate_px)
    huber_px = check_huber(huber_px)
    intr = intrinsics_flags(intrinsics)
    imask = free_mask(intrinsics_free, C) if intr else 0
    if reference and triangulate is None:
        raise ValueError("refine_rig: reference=True needs `triangulate` (the library's triangulation runs on the GPU)")
    steps = _ReferenceSteps(triangulate) if reference else _LibrarySteps(method, params, P)
    if triangulate is not None:
        steps.triangulate = triangulate
    K, R, t = np.array(K, dtype=np.float64, copy=True), np.array(R, copy=True), np.array(t, copy=True)
    history = []

    def measure(xyzs):
        cs, cn = steps.cost(xyzs, kpts, n_persons, thr)
        if one_to_one:
            det_of = np.asarray(steps.assign(np.asarray(cs), np.asarray(cn), gate_px, min_joints))
        else:
            det_of, _ = match_detections(np.asarray(cs), np.asarray(cn), gate_px, min_joints)
        resid = view_residuals(steps.pixels(xyzs), kpts, det_of, thr)[0]                   # [F, C, P, kn], NaN where nothing counts
        r2 = np.moveaxis(np.asarray(resid) ** 2, 1, 0).reshape(C, -1)
        with np.errstate(all="ignore"):
            rms = np.sqrt(np.nansum(r2, axis=1) / np.maximum((~np.isnan(r2)).sum(axis=1), 1))
        return det_of, np.where((~np.isnan(r2)).any(axis=1), rms, np.nan)

    for r in range(int(rounds) + 1):
        steps.overflow_frames = 0
        xyzs = np.ascontiguousarray(steps.triangulate(K, R, t, kpts, n_persons), dtype=np.float64)
        steps.open(K, R, t)
        try:
            det_of, view_rms = measure(xyzs)
            if r == int(rounds):
                history.append(dict(overflow_frames=steps.overflow_frames, view_rms=view_rms))
                break
            kw = dict(det_of=det_of, n_persons=n_persons, keypoint_score_threshold=thr, score_weights=score_weights)
            if huber_px is not None:
                kw["huber_px"] = huber_px
            if retriangulate:
                from .matched import merge_records
                again, _, views, _ = steps.matched(kpts, det_of, n_persons, thr)
                xyzs, kw["views"] = merge_records(xyzs, np.asarray(again, dtype=np.float64), views)
                xyzs = np.ascontiguousarray(xyzs)
            xyzs = steps.joints(xyzs, kpts, iters=joint_iters, **kw)
            if intr:
                kw.update(intrinsics=intrinsics, intrinsics_free=imask)
            Kn, R, t, rep = steps.cameras(xyzs, kpts, free=mask, min_obs=min_obs, iters=camera_iters, **kw)
            K, R, t = np.array(Kn, dtype=np.float64), np.array(R, dtype=np.float64), np.array(t, dtype=np.float64)
            history.append(dict(overflow_frames=steps.overflow_frames, view_rms=view_rms, cost=np.array(rep["cost"]), n_obs=np.array(rep["n_obs"]), codes=np.array(rep["codes"])))
        finally:
            steps.close()
    return (K, R, t, history) if intr else (R, t, history)


__all__ = ["refine_cameras", "refine_cameras_reference", "refine_rig", "POSE_FIXED", "POSE_FEW_OBS", "POSE_KEPT", "POSE_MOVED"]
