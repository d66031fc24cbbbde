"""Inputs shared by tests/test_pose_host.py and tests/test_gpu_pose.py (k_pose_normal / k_pose_step, snowmocap_amd/pose.py): drifted
rigs over the cases of tests/refine_cases.py, the exact minimiser of a camera's reprojection cost over its six pose parameters in
50-digit arithmetic, 50-digit normal equations, and the recipe of the README's figures.  No GPU code; everything is seeded.

A CASE is refine_cases.case as it is -- rig, placement, persons of synth.make_people on the 1.5 m circle, detections = exact
projections + N(0, sigma), and with `sprinkle` everything a recording sprinkles in (missing records, low scores, NaN pixels, permuted
lists, det_of = -1, short n_persons, a views mask) -- with two changes: the joint records handed over are the TRUTH (the joints are
held fixed here; a record refine_cases marks missing stays missing), and the rig the library is given has DRIFTED: every free camera
is rotated by 0.3 .. 1 degree about a seeded random axis and moved by 1 .. 3 cm (in the placement's unit).  The free cameras are the
odd ones, so every rig also has cameras that must keep their bits.

THE ACCURACY BARS, in the manner of refine_cases.REFERENCE_FLOOR.  The rule accepts a step only while E decreases strictly in fp64, so
it stops resolving a step d once d^T H d < eps E.  With exact detections E itself is rounding and the reference returns to the true
pose to FLOOR_EXACT = (largest |R - R_true| entry, |t - t_true| / rig scale); with noise it reaches the 50-digit minimiser over the
same six parameters and the same S_c to FLOOR_NOISY.  Both are measured by tests/test_pose_host.py on the CPU, which fails if a
committed constant has moved by more than a factor of two; the kernel is held to 4 x the floor, k_refine's margin: one step earlier
or later at the floor is worth about the floor.  NORMAL_UNITS is the error of the reference's E, g and H against 50-digit sums, at the
(drifted) input pose and at the pose it ends at, in units of eps * sum |term|.
"""
import functools

import numpy as np

import dlt_frames_cases as fc
import refine_cases as rc
from snowmocap_amd import pose, synth

RIGS = rc.RIGS
PLACEMENTS = rc.PLACEMENTS
SHAPES = [(1, 1, 8), (1, 1, 64), (1, 1, 65), (2, 3, 21), (6, 2, 17), (1, 1, 255), (1, 1, 256), (1, 1, 257)]      # (F, P, kn)
EXACT_SHAPE = (6, 2, 17)
MINIMISER_SHAPE = rc.MINIMISER_SHAPE                      # (3, 1, 17)
MIN_OBS = 6
ITERS = 8
DIGITS = 50
EPS = float(np.finfo(np.float64).eps)

# measured by tests/test_pose_host.py (CPU, the NumPy rule, float64 records and keypoints, iters = 8, min_obs = 6):
#   test_exact_detections_return_to_the_true_pose, EXACT_SHAPE with the sprinkles, six rigs x six placements: the largest
#     |R - R_true| entry 2.476e-14, the largest |t - t_true| / rig scale 3.614e-14 (both on the floor rig at "mm-site");
#   test_reference_against_the_exact_minimiser, MINIMISER_SHAPE with the sprinkles, six rigs at home, sigma 1 and 2: 3.821e-9 and
#     3.943e-9 (ring8 at sigma 1; the other rigs 5e-13 .. 2e-9: a camera with some 35 observations of one person);
#   test_normal_equations_against_50_digit_sums, the same cases at sigma 1, at the drifted input pose (71.1) and at the pose the rule
#     ends at (128.5): 128.5 eps * sum |term| (a residual of a pixel or a few is the difference of two pixels of several hundred).
# Each test measures its figure again and fails if it has left the constant by more than a factor of two either way.
FLOOR_EXACT = (2.476e-14, 3.614e-14)
FLOOR_NOISY = (3.821e-9, 3.943e-9)
NORMAL_UNITS = 128.5
MARGIN = 4.0


def free_cameras(C):
    return [c for c in range(C) if c % 2 == 1]


def drift(rig_name, placement, R, t, free, angle=(0.3, 1.0), shift=(0.01, 0.03)):
    """-> (R', t') with every camera of `free` rotated by angle[0] .. angle[1] degrees about a random axis and moved by
    shift[0] .. shift[1] metres (times the placement's unit) in a random direction; seeded by (rig, placement)."""
    rng = np.random.default_rng(rc._seed("drift", rig_name, placement))
    unit = fc.PLACEMENTS[placement][0]
    Rd, td = np.array(R, copy=True), np.array(t, copy=True)
    for c in free:
        axis, way = rng.normal(size=3), rng.normal(size=3)
        axis, way = axis / np.linalg.norm(axis), way / np.linalg.norm(way)
        Rd[c] = pose.rodrigues(axis * np.deg2rad(rng.uniform(*angle))) @ R[c]
        td[c] = t[c] + way * (unit * rng.uniform(*shift))
    return Rd, td


@functools.lru_cache(maxsize=None)
def case(rig_name, shape, sigma=0.0, sprinkle=True, rec_dtype="float64", kp_dtype="float64", placement="home"):
    """-> dict(K, R, t: the TRUE rig (placed), Rd, td: the drifted one, free: the cameras that drifted, xyzs [F,P,kn,4] of rec_dtype:
    the true joints, kpts, det_of, n_persons, views, thr as refine_cases.case gives them, kw: the keyword arguments of the entry);
    read-only."""
    cs = rc.case(rig_name, shape, sigma, sprinkle, rec_dtype, kp_dtype, placement)
    C = cs["K"].shape[0]
    free = free_cameras(C)
    Rd, td = drift(rig_name, placement, cs["R"], cs["t"], free)
    start = np.asarray(cs["dlt"]).astype(np.float64)
    gone = pose.missing_records(start)
    rec = np.concatenate([cs["X"], start[..., 3:4]], axis=-1)
    rec[gone] = start[gone]                                   # a missing record stays what it was: zeros, a NaN x, a score of -0.0
    out = dict(K=cs["K"], R=cs["R"], t=cs["t"], Rd=Rd, td=td, free=tuple(free), xyzs=rec.astype(rec_dtype), kpts=cs["kpts"],
               det_of=cs["det_of"], n_persons=cs["n_persons"], views=cs["views"], thr=cs["thr"])
    out["kw"] = dict(det_of=cs["det_of"], n_persons=cs["n_persons"], views=cs["views"], keypoint_score_threshold=cs["thr"],
                     free=list(free), min_obs=MIN_OBS, iters=ITERS)
    for a in out.values():
        if isinstance(a, np.ndarray):
            a.setflags(write=False)
    return out


@functools.lru_cache(maxsize=None)
def reference(rig_name, shape, sigma=0.0, sprinkle=True, rec_dtype="float64", kp_dtype="float64", placement="home", score_weights=False):
    """refine_cameras_reference on a case's drifted rig -> (R, t, report, S); computed once."""
    cs = case(rig_name, shape, sigma, sprinkle, rec_dtype, kp_dtype, placement)
    return pose.refine_cameras_reference(cs["K"], cs["Rd"], cs["td"], cs["xyzs"], cs["kpts"], score_weights=score_weights,
                                         return_sets=True, **cs["kw"])


def pose_error(R, t, R_true, t_true, cams):
    """-> (largest |R - R_true| entry, largest |t - t_true| / rig scale) over the cameras `cams`."""
    cams = list(cams)
    if not cams:
        return 0.0, 0.0
    return (float(np.abs(np.asarray(R)[cams] - R_true[cams]).max()),
            float(np.abs(np.asarray(t)[cams] - t_true[cams]).max()) / rc.rig_scale(t_true))


def camera_observations(cs, S, c, score_weights=False):
    """The observations of camera c as the rule sees them -> X [n, 3], ou, ov, w [n] (record order)."""
    X, S2, obs = pose.observation_sets(cs["K"], cs["Rd"], cs["td"], cs["xyzs"], cs["kpts"], cs["det_of"], cs["n_persons"], cs["views"],
                                       cs["thr"], score_weights)
    assert np.array_equal(S, S2)
    return X[S[c]], obs[c, S[c], 0], obs[c, S[c], 1], obs[c, S[c], 2]


# ------------------------------------------------------------------------------------------------ 50-digit arithmetic
def _mp_terms(mp, Kc, R, t, X, ou, ov, w):
    """-> E, g [6], H [6][6] and the sums of |term| of each, at the pose (R: 3 x 3 list of mpf, t: list of mpf)."""
    m = lambda a: mp.mpf(float(a))
    fx, sk, cx, fy, cy = m(Kc[0, 0]), m(Kc[0, 1]), m(Kc[0, 2]), m(Kc[1, 1]), m(Kc[1, 2])
    E, aE = mp.mpf(0), mp.mpf(0)
    g, ag = [mp.mpf(0)] * 6, [mp.mpf(0)] * 6
    H, aH = [[mp.mpf(0)] * 6 for _ in range(6)], [[mp.mpf(0)] * 6 for _ in range(6)]
    for n in range(X.shape[0]):
        d = [m(X[n, i]) - t[i] for i in range(3)]
        pc = [R[0][i] * d[0] + R[1][i] * d[1] + R[2][i] * d[2] for i in range(3)]
        x, y = pc[0] / pc[2], pc[1] / pc[2]
        ru, rv, wn = fx * x + sk * y + cx - m(ou[n]), fy * y + cy - m(ov[n]), m(w[n])
        du, dv = [], []
        for k in range(6):
            if k < 3:
                a_, b_ = (k + 1) % 3, (k + 2) % 3
                col = [R[a_][i] * d[b_] - R[b_][i] * d[a_] for i in range(3)]
            else:
                col = [-R[k - 3][i] for i in range(3)]
            dx, dy = (col[0] - x * col[2]) / pc[2], (col[1] - y * col[2]) / pc[2]
            du.append(fx * dx + sk * dy)
            dv.append(fy * dy)
        e = wn * (ru * ru + rv * rv)
        E, aE = E + e, aE + abs(e)
        for a in range(6):
            ga = wn * (du[a] * ru + dv[a] * rv)
            g[a], ag[a] = g[a] + ga, ag[a] + abs(ga)
            for b in range(a + 1):
                h = wn * (du[a] * du[b] + dv[a] * dv[b])
                H[a][b], aH[a][b] = H[a][b] + h, aH[a][b] + abs(h)
                H[b][a] = H[a][b]
    return E, g, H, aE, ag, aH


def exact_normal(Kc, Rc, tc, X, ou, ov, w):
    """E, g, H of one camera at the fp64 pose (Rc, tc) in DIGITS-digit arithmetic -> (normal [28] rounded once to fp64, the sums of
    |term| [28])."""
    import mpmath as mp
    with mp.workdps(DIGITS):
        R = [[mp.mpf(float(Rc[i, j])) for j in range(3)] for i in range(3)]
        t = [mp.mpf(float(a)) for a in tc]
        E, g, H, aE, ag, aH = _mp_terms(mp, Kc, R, t, X, ou, ov, w)
        val = [E] + g + [H[a][b] for a, b in pose.H_INDEX]
        mag = [aE] + ag + [aH[a][b] for a, b in pose.H_INDEX]
        return np.array([float(v) for v in val]), np.array([float(v) for v in mag])


def exact_pose_minimum(Kc, R0, t0, X, ou, ov, w, tol="1e-30", max_steps=100):
    """Gauss-Newton on E(omega, tau) in DIGITS-digit arithmetic from the fp64 pose (R0, t0), the pose updated as the rule updates it
    (Exp(omega) R, t + tau), until |delta| < tol -> (R [3, 3], t [3] rounded once to fp64, E as float, steps)."""
    import mpmath as mp
    with mp.workdps(DIGITS):
        R = [[mp.mpf(float(R0[i, j])) for j in range(3)] for i in range(3)]
        t = [mp.mpf(float(a)) for a in t0]
        tol = mp.mpf(tol)
        for step in range(max_steps):
            E, g, H, _, _, _ = _mp_terms(mp, Kc, R, t, X, ou, ov, w)
            delta = mp.lu_solve(mp.matrix(H), -mp.matrix(g))
            om = [delta[0], delta[1], delta[2]]
            th = mp.sqrt(om[0] ** 2 + om[1] ** 2 + om[2] ** 2)
            a, b = (mp.sin(th) / th, 2 * mp.sin(th / 2) ** 2 / th ** 2) if th > 0 else (mp.mpf(1), mp.mpf(1) / 2)
            W = [[0, -om[2], om[1]], [om[2], 0, -om[0]], [-om[1], om[0], 0]]
            Ex = [[(1 if i == j else 0) + a * W[i][j] + b * sum(W[i][k] * W[k][j] for k in range(3)) for j in range(3)] for i in range(3)]
            R = [[sum(Ex[i][k] * R[k][j] for k in range(3)) for j in range(3)] for i in range(3)]
            t = [t[i] + delta[3 + i] for i in range(3)]
            if mp.sqrt(sum(delta[i] ** 2 for i in range(6))) < tol:
                break
        else:
            raise AssertionError("the exact Gauss-Newton iteration did not settle")
        E = _mp_terms(mp, Kc, R, t, X, ou, ov, w)[0]
        return np.array([[float(v) for v in row] for row in R]), np.array([float(v) for v in t]), float(E), step + 1


@functools.lru_cache(maxsize=None)
def minimiser(rig_name, sigma, kp_dtype="float64", rec_dtype="float64", placement="home", shape=MINIMISER_SHAPE):
    """The exact minimiser of every free camera of case(rig, shape, sigma, True, ...) that has at least MIN_OBS observations, over the
    rule's own S_c, started at the true pose -> dict(R [C,3,3], t [C,3] (the true pose where none was computed), cams: the cameras
    computed, E [C]); read-only."""
    cs = case(rig_name, shape, sigma, True, rec_dtype, kp_dtype, placement)
    _, _, rep, S = reference(rig_name, shape, sigma, True, rec_dtype, kp_dtype, placement)
    Rm, tm, Em, cams = np.array(cs["R"], copy=True), np.array(cs["t"], copy=True), np.zeros(cs["K"].shape[0]), []
    for c in cs["free"]:
        if rep["n_obs"][c] < MIN_OBS:
            continue
        X, ou, ov, w = camera_observations(cs, S, c)
        Rm[c], tm[c], Em[c], _ = exact_pose_minimum(cs["K"][c], cs["R"][c], cs["t"][c], X, ou, ov, w)
        cams.append(c)
    out = dict(R=Rm, t=tm, E=Em, cams=tuple(cams))
    for a in out.values():
        if isinstance(a, np.ndarray):
            a.setflags(write=False)
    return out


# ------------------------------------------------------------------------------------------------ the statistical recipe
def dlt_points(K, R, t, kpts, n_persons=None):
    """A plain homogeneous DLT of detection p of every camera -> records [F, Pmax, kn, 4] float64 (score 1): the triangulation step
    of the reference-driven refine_rig (the recipe's lists are not permuted: detection p is person p)."""
    from snowmocap_amd.robust import projection_matrices
    kp = np.asarray(kpts, dtype=np.float64)
    F, C, Pmax, kn, _ = kp.shape
    Pm = projection_matrices(K, R, t)
    A = np.empty((F, Pmax, kn, 2 * C, 4))
    for c in range(C):
        A[..., 2 * c, :] = kp[:, c, :, :, 0:1] * Pm[c, 2] - Pm[c, 0]
        A[..., 2 * c + 1, :] = kp[:, c, :, :, 1:2] * Pm[c, 2] - Pm[c, 1]
    Xh = np.linalg.svd(A)[2][..., -1, :]
    return np.concatenate([Xh[..., :3] / Xh[..., 3:4], np.ones((F, Pmax, kn, 1))], axis=-1)


@functools.lru_cache(maxsize=None)
def recipe(C=8, bad=3, F=40, P=2, kn=17, sigma=1.0, angle_deg=0.5, shift=0.02):
    """The recipe of the README's figures: synth.ring_rig(C), P persons on the 1.5 m circle, F x P x kn joints, exact projections +
    N(0, sigma) with score 1, camera `bad` off by angle_deg about a seeded axis and `shift` metres.
    -> dict(K, R, t: the truth, Rd, td: the calibration file that no longer holds, X, kpts [F,C,P,kn,3] float64, bad); read-only."""
    K, R, t = synth.ring_rig(C)
    rng = np.random.default_rng(rc._seed("pose-recipe", C, bad, F, P, kn, sigma))
    X = synth.make_people(rng, F, P, J=kn)
    uv = np.moveaxis(synth.project(K, R, t, X)[0], 0, 1) + sigma * rng.normal(0.0, 1.0, (F, C, P, kn, 2))
    kp = np.concatenate([uv, np.ones((F, C, P, kn, 1))], axis=-1)
    axis, way = rng.normal(size=3), rng.normal(size=3)
    Rd, td = np.array(R, copy=True), np.array(t, copy=True)
    Rd[bad] = pose.rodrigues(axis / np.linalg.norm(axis) * np.deg2rad(angle_deg)) @ R[bad]
    td[bad] = t[bad] + way / np.linalg.norm(way) * shift
    out = dict(K=K, R=R, t=t, Rd=Rd, td=td, X=X, kpts=kp, bad=bad)
    for a in out.values():
        if isinstance(a, np.ndarray):
            a.setflags(write=False)
    return out
