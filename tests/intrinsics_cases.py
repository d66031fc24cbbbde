"""Inputs shared by tests/test_intrinsics_host.py and tests/test_gpu_intrinsics.py (k_pose_normal_k / k_pose_step_k behind
snowtri_refine_cameras_k, snowmocap_amd/pose.py with intrinsics=...): the cases of tests/pose_cases.py with a calibration whose K has
drifted too, the exact minimiser of a camera's reprojection cost over its ten parameters in 50-digit arithmetic, and 50-digit normal
equations.  No GPU code; everything is seeded.

A CASE is pose_cases.case as it is -- the true joints, the drifted poses Rd, td of the odd cameras -- plus Kd: the K the library is
given, in which every free (odd) camera's fx and fy are off by 1 .. 3 % and its cx and cy by 2 .. 10 px, each with a random sign,
seeded by (rig, placement).  iters = 16 and min_obs = 6; the keyword is intrinsics="fc" unless a test says otherwise.

THE ACCURACY BARS, in the manner of pose_cases: the rule accepts a step only while E decreases strictly in fp64.  With exact
detections it returns to the true K, R, t to FLOOR_EXACT_K = (|fx, fy - true| / true, |cx, cy - true| px, largest |R - R_true| entry,
|t - t_true| / rig scale); with noise it reaches the 50-digit minimiser over the same ten parameters and the same S_c to FLOOR_NOISY_K
(the same four figures).  NORMAL_UNITS_K is the error of the rule's E, g[10] and H[55] against 50-digit sums, at the drifted input
and at the parameters it ends at, in units of eps * sum |term|.  All three are measured by tests/test_intrinsics_host.py on the CPU,
which fails if a committed constant has moved by more than a factor of two; the kernel is held to MARGIN = 4 x the floor.
"""
import functools

import numpy as np

import pose_cases as pc
import refine_cases as rc
from snowmocap_amd import pose

RIGS = pc.RIGS
PLACEMENTS = pc.PLACEMENTS
SHAPES = pc.SHAPES
EXACT_SHAPE = pc.EXACT_SHAPE                              # (6, 2, 17): some 150 observations per camera
NOISY_SHAPE = pc.EXACT_SHAPE                              # ten parameters want more than MINIMISER_SHAPE's 35 observations
NOISY_SIGMA = 1.0
MIN_OBS = 6
ITERS = 16
DIGITS = pc.DIGITS
EPS = pc.EPS
MARGIN = pc.MARGIN

# measured by tests/test_intrinsics_host.py (CPU, the NumPy rule with intrinsics="fc", float64 records and keypoints, iters = 16,
# min_obs = 6); the order is (focal, relative; centre, px; largest |R - R_true| entry; |t - t_true| / rig scale):
#   test_exact_detections_return_to_the_true_camera, EXACT_SHAPE with the sprinkles, six rigs x six placements, every free camera
#     (at most 9 steps): 1.155e-13, 1.056e-10 px, 1.307e-13, 1.011e-13;
#   test_reference_against_the_exact_minimiser, NOISY_SHAPE with the sprinkles, six rigs at home, sigma 1, the first two free cameras
#     of each rig (133 .. 176 observations): 8.601e-9, 1.001e-5 px, 1.157e-8, 5.949e-9, all four on ring5 (the other rigs
#     2e-11 .. 4e-9; the centre is the loosest parameter, as the limits of INTRINSICS say);
#   test_normal_equations_against_50_digit_sums, the same cases, the first of those cameras and camera 0 (fixed) of each rig, at the
#     drifted input and at the parameters the rule ends at: 57.8 eps * sum |term|.
# Each test measures its figure again and fails if it has left the constant by more than a factor of two either way.
FLOOR_EXACT_K = (1.155e-13, 1.056e-10, 1.307e-13, 1.011e-13)
FLOOR_NOISY_K = (8.601e-9, 1.001e-5, 1.157e-8, 5.949e-9)
NORMAL_UNITS_K = 57.8


def drift_K(rig_name, placement, K, free, focal=(0.01, 0.03), centre=(2.0, 10.0)):
    """-> K' with fx, fy of every camera of `free` off by focal[0] .. focal[1] (relative) and cx, cy by centre[0] .. centre[1] px,
    each with a random sign; seeded by (rig, placement)."""
    rng = np.random.default_rng(rc._seed("drift-K", rig_name, placement))
    Kd = np.array(K, dtype=np.float64, copy=True)
    for c in free:
        sf, sc = rng.choice([-1.0, 1.0], size=2), rng.choice([-1.0, 1.0], size=2)
        Kd[c, 0, 0] *= 1.0 + sf[0] * rng.uniform(*focal)
        Kd[c, 1, 1] *= 1.0 + sf[1] * rng.uniform(*focal)
        Kd[c, 0, 2] += sc[0] * rng.uniform(*centre)
        Kd[c, 1, 2] += sc[1] * rng.uniform(*centre)
    return Kd


@functools.lru_cache(maxsize=None)
def case(rig_name, shape, sigma=0.0, sprinkle=True, rec_dtype="float64", kp_dtype="float64", placement="home"):
    """pose_cases.case plus Kd (the drifted K) and kw with iters = ITERS, min_obs = MIN_OBS, intrinsics = "fc" and intrinsics_free =
    the free cameras; read-only."""
    cs = dict(pc.case(rig_name, shape, sigma, sprinkle, rec_dtype, kp_dtype, placement))
    cs["Kd"] = drift_K(rig_name, placement, cs["K"], cs["free"])
    cs["Kd"].setflags(write=False)
    cs["kw"] = dict(cs["kw"], min_obs=MIN_OBS, iters=ITERS, intrinsics="fc", intrinsics_free=list(cs["free"]))
    return cs


@functools.lru_cache(maxsize=None)
def reference(rig_name, shape, sigma=0.0, sprinkle=True, rec_dtype="float64", kp_dtype="float64", placement="home", score_weights=False,
              intrinsics="fc", free="odd", intrinsics_free="odd", huber_px=None):
    """refine_cameras_reference on a case's drifted rig -> (K, R, t, report, S); computed once.  free / intrinsics_free: "odd" (the
    case's free cameras), "none" or "all"."""
    cs = case(rig_name, shape, sigma, sprinkle, rec_dtype, kp_dtype, placement)
    pick = lambda which: {"odd": list(cs["free"]), "none": [], "all": None}[which]
    kw = dict(cs["kw"], intrinsics=intrinsics, free=pick(free), intrinsics_free=pick(intrinsics_free), huber_px=huber_px)
    return pose.refine_cameras_reference(cs["Kd"], cs["Rd"], cs["td"], cs["xyzs"], cs["kpts"], score_weights=score_weights, return_sets=True, **kw)


def camera_error(K, R, t, K_true, R_true, t_true, cams):
    """-> (largest |f - f_true| / f_true over fx, fy; largest |c - c_true| px over cx, cy; largest |R - R_true| entry; largest
    |t - t_true| / rig scale) over the cameras `cams`."""
    cams = list(cams)
    if not cams:
        return 0.0, 0.0, 0.0, 0.0
    K, Kt = np.asarray(K)[cams], np.asarray(K_true)[cams]
    ef = max(float(np.abs(K[:, 0, 0] / Kt[:, 0, 0] - 1.0).max()), float(np.abs(K[:, 1, 1] / Kt[:, 1, 1] - 1.0).max()))
    ec = max(float(np.abs(K[:, 0, 2] - Kt[:, 0, 2]).max()), float(np.abs(K[:, 1, 2] - Kt[:, 1, 2]).max()))
    return (ef, ec) + pc.pose_error(R, t, R_true, t_true, cams)


def camera_observations(cs, S, c, score_weights=False):
    """The observations of camera c as the rule sees them (S_c at the drifted pose and the drifted K) -> X [n, 3], ou, ov, w [n]."""
    X, S2, obs = pose.observation_sets(cs["Kd"], cs["Rd"], cs["td"], cs["xyzs"], cs["kpts"], cs["det_of"], cs["n_persons"], cs["views"],
                                       cs["thr"], score_weights)
    assert np.array_equal(S, S2)
    return X[S[c]], obs[c, S[c], 0], obs[c, S[c], 1], obs[c, S[c], 2]


# ------------------------------------------------------------------------------------------------ 50-digit arithmetic
def _mp_terms(mp, k5, R, t, X, ou, ov, w):
    """-> E, g [10], H [10][10] and the sums of |term| of each, at (k5 = fx, s, cx, fy, cy; R: 3 x 3 list; t: list), all mpf."""
    m = lambda a: mp.mpf(float(a))
    fx, sk, cx, fy, cy = k5
    zero, one = mp.mpf(0), mp.mpf(1)
    E, aE = zero, zero
    g, ag = [zero] * 10, [zero] * 10
    H, aH = [[zero] * 10 for _ in range(10)], [[zero] * 10 for _ in range(10)]
    for n in range(X.shape[0]):
        d = [m(X[n, i]) - t[i] for i in range(3)]
        pcam = [R[0][i] * d[0] + R[1][i] * d[1] + R[2][i] * d[2] for i in range(3)]
        x, y = pcam[0] / pcam[2], pcam[1] / pcam[2]
        ru, rv, wn = fx * x + sk * y + cx - m(ou[n]), fy * y + cy - m(ov[n]), m(w[n])
        du, dv = [], []
        for k in range(6):
            if k < 3:
                a_, b_ = (k + 1) % 3, (k + 2) % 3
                col = [R[a_][i] * d[b_] - R[b_][i] * d[a_] for i in range(3)]
            else:
                col = [-R[k - 3][i] for i in range(3)]
            dx, dy = (col[0] - x * col[2]) / pcam[2], (col[1] - y * col[2]) / pcam[2]
            du.append(fx * dx + sk * dy)
            dv.append(fy * dy)
        du += [x, zero, one, zero]
        dv += [zero, y, zero, one]
        e = wn * (ru * ru + rv * rv)
        E, aE = E + e, aE + abs(e)
        for a in range(10):
            ga = wn * (du[a] * ru + dv[a] * rv)
            g[a], ag[a] = g[a] + ga, ag[a] + abs(ga)
            for b in range(a + 1):
                h = wn * (du[a] * du[b] + dv[a] * dv[b])
                H[a][b], aH[a][b] = H[a][b] + h, aH[a][b] + abs(h)
                H[b][a] = H[a][b]
    return E, g, H, aE, ag, aH


def _mp_camera(mp, Kc, Rc, tc):
    k5 = [mp.mpf(float(Kc[0, 0])), mp.mpf(float(Kc[0, 1])), mp.mpf(float(Kc[0, 2])), mp.mpf(float(Kc[1, 1])), mp.mpf(float(Kc[1, 2]))]
    return k5, [[mp.mpf(float(Rc[i, j])) for j in range(3)] for i in range(3)], [mp.mpf(float(a)) for a in tc]


def exact_normal(Kc, Rc, tc, X, ou, ov, w):
    """E, g[10], H[55] of one camera at the fp64 parameters in DIGITS-digit arithmetic -> (normal [66] rounded once to fp64, the sums
    of |term| [66])."""
    import mpmath as mp
    with mp.workdps(DIGITS):
        k5, R, t = _mp_camera(mp, Kc, Rc, tc)
        E, g, H, aE, ag, aH = _mp_terms(mp, k5, R, t, X, ou, ov, w)
        val = [E] + g + [H[a][b] for a, b in pose.H_INDEX_K]
        mag = [aE] + ag + [aH[a][b] for a, b in pose.H_INDEX_K]
        return np.array([float(v) for v in val]), np.array([float(v) for v in mag])


def exact_camera_minimum(K0, R0, t0, X, ou, ov, w, tol="1e-30", max_steps=100):
    """Gauss-Newton on E(omega, tau, fx, fy, cx, cy) in DIGITS-digit arithmetic from the fp64 parameters (K0, R0, t0), updated as the
    rule updates them, until |delta| < tol (the pose in its own units, the focal lengths relative, the centre in px / 1000)
    -> (K [3, 3], R [3, 3], t [3] rounded once to fp64, E as float, steps)."""
    import mpmath as mp
    with mp.workdps(DIGITS):
        k5, R, t = _mp_camera(mp, K0, R0, t0)
        tol = mp.mpf(tol)
        for step in range(max_steps):
            E, g, H, _, _, _ = _mp_terms(mp, k5, R, t, X, ou, ov, w)
            delta = mp.lu_solve(mp.matrix(H), -mp.matrix(g))
            om = [delta[0], delta[1], delta[2]]
            th = mp.sqrt(om[0] ** 2 + om[1] ** 2 + om[2] ** 2)
            a, b = (mp.sin(th) / th, 2 * mp.sin(th / 2) ** 2 / th ** 2) if th > 0 else (mp.mpf(1), mp.mpf(1) / 2)
            W = [[0, -om[2], om[1]], [om[2], 0, -om[0]], [-om[1], om[0], 0]]
            Ex = [[(1 if i == j else 0) + a * W[i][j] + b * sum(W[i][k] * W[k][j] for k in range(3)) for j in range(3)] for i in range(3)]
            R = [[sum(Ex[i][k] * R[k][j] for k in range(3)) for j in range(3)] for i in range(3)]
            t = [t[i] + delta[3 + i] for i in range(3)]
            k5 = [k5[0] + delta[6], k5[1], k5[2] + delta[8], k5[3] + delta[7], k5[4] + delta[9]]
            size = [delta[i] for i in range(6)] + [delta[6] / k5[0], delta[7] / k5[3], delta[8] / 1000, delta[9] / 1000]
            if mp.sqrt(sum(v ** 2 for v in size)) < tol:
                break
        else:
            raise AssertionError("the exact Gauss-Newton iteration did not settle")
        E = _mp_terms(mp, k5, R, t, X, ou, ov, w)[0]
        Kn = np.array(K0, dtype=np.float64, copy=True)
        Kn[0, 0], Kn[0, 2], Kn[1, 1], Kn[1, 2] = float(k5[0]), float(k5[2]), float(k5[3]), float(k5[4])
        return Kn, np.array([[float(v) for v in row] for row in R]), np.array([float(v) for v in t]), float(E), step + 1


@functools.lru_cache(maxsize=None)
def minimiser(rig_name, sigma=NOISY_SIGMA, placement="home", shape=NOISY_SHAPE, max_cams=2):
    """The exact ten-parameter minimiser of the first max_cams free cameras of case(rig, shape, sigma, True) that the rule moved,
    over the rule's own S_c, started where the rule ended (the iteration converges quadratically: a few steps)
    -> dict(K, R, t (the rule's output where none was computed), cams: the cameras computed, E [C]); read-only."""
    cs = case(rig_name, shape, sigma, True, placement=placement)
    Kr, Rr, tr, rep, S = reference(rig_name, shape, sigma, True, placement=placement)
    Km, Rm, tm, Em, cams = np.array(Kr, copy=True), np.array(Rr, copy=True), np.array(tr, copy=True), np.zeros(cs["K"].shape[0]), []
    for c in cs["free"]:
        if rep["codes"][c] != pose.POSE_MOVED or len(cams) == max_cams:
            continue
        X, ou, ov, w = camera_observations(cs, S, c)
        Km[c], Rm[c], tm[c], Em[c], _ = exact_camera_minimum(Kr[c], Rr[c], tr[c], X, ou, ov, w)
        cams.append(c)
    out = dict(K=Km, R=Rm, t=tm, E=Em, cams=tuple(cams))
    for a in out.values():
        if isinstance(a, np.ndarray):
            a.setflags(write=False)
    return out
