"""Inputs shared by tests/test_huber_host.py and tests/test_gpu_huber.py (the Huber loss of include/snowtri.h, "Refinement" and
"Camera pose refinement", ROBUST LOSS: k_refine / k_pose_normal with HUBER, snowmocap_amd/refine.py and pose.py with huber_px).
No GPU code; everything is seeded.

A CASE is refine_cases.case / pose_cases.case at sigma 1 with the sprinkles, and a seeded 10 % of ALL detections (every camera, every
list slot, every joint) moved by 20 .. 150 px in a random direction.  Nothing else changes: the start records, det_of, n_persons, the
views mask, the drifted rig of a pose case.  DELTAS = (3, 6) px.

`rule_at` evaluates the rule's E and its regimes at GIVEN points over GIVEN view sets with the functions the NumPy rule itself is
made of (refine.project_camera, refine.huber_terms; the views added in camera order): it is what the kernel's cost at its own
output point and its `outliers` word are compared with, bit for bit.

EXACT MINIMISER (`exact_huber_minimum`, `exact_huber_pose_minimum`): IRLS on the Huber cost in 50-digit mpmath, over the rule's own
view / observation set, started at the NumPy rule's output, at most MAX_EXACT_STEPS steps, settled when a step is below 1e-30.

THE ACCURACY BARS follow refine_cases.REFERENCE_FLOOR / BAR and pose_cases.FLOOR_NOISY / MARGIN: the constants below are what
tests/test_huber_host.py measured for the NumPy rule on the CPU; that test measures them again and fails if one has moved by more
than a factor of two; the kernels are held to 4 x the floor.
"""
import functools

import numpy as np

import pose_cases as pc
import refine_cases as rc
from snowmocap_amd import pose
from snowmocap_amd import refine as rf

DELTAS = (3.0, 6.0)
BIG_DELTA = 1e6                     # no view of any case is in the linear regime: the squared loss' bits
OUTLIER_SHARE = 0.10
OUTLIER_PX = (20.0, 150.0)
KERNEL_RIGS = ("ring3", "ring16", "floor", "ring8")       # k_refine<0> (3 and 16 cameras), <4>, <8>
ACCURACY_RIGS = ("ring5", "ring8", "ring16")
ACCURACY_SHAPE = (2, 3, 21)
ACCURACY_ITERS = 16
MIN_QUADRATIC = 3                   # a record is covered by the accuracy test if its minimiser leaves this many views quadratic
MIN_COVERED = 0.80                  # ... and the covered records must be this share of the refined ones, on each rig
MAX_EXACT_STEPS = 200
DIGITS = 50
NEAR_DELTA = 1e-9                   # the pose tests' cases hold no observation this close (relative) to delta

# measured by tests/test_huber_host.py::test_reference_against_the_exact_huber_minimiser (CPU, the NumPy rule, float64 records and
# keypoints, iters = 16, ACCURACY_SHAPE, ring5 / ring8 / ring16, delta 3 and 6, start "dlt"): the largest |reference - 50-digit
# minimiser| / rig scale over the covered records.  The host test measures it again and fails if it has moved by more than a factor
# of two either way; the kernel is held to JOINT_BAR.
# Measured: 2.759e-7 (ring8 at delta 6: one record with exactly three quadratic views on which IRLS is still converging at step
# 16; the other five (rig, delta) pairs 5.6e-10 .. 1.3e-9), with 89 % (ring5), 93 .. 95 % (ring8) and 99 % (ring16) of the refined
# records covered.
JOINT_FLOOR = 2.759e-7
JOINT_BAR = 4.0 * JOINT_FLOOR


def _moved(kpts, seed):
    """kpts [F, C, Pmax, kn, 3] -> a copy with OUTLIER_SHARE of the detections moved by OUTLIER_PX in a random direction, and the
    mask of the moved ones [F, C, Pmax, kn]."""
    rng = np.random.default_rng(seed)
    kp = np.array(kpts, dtype=np.float64, copy=True)
    hit = rng.random(kp.shape[:-1]) < OUTLIER_SHARE
    ang = rng.uniform(0.0, 2.0 * np.pi, kp.shape[:-1])
    far = rng.uniform(*OUTLIER_PX, kp.shape[:-1])
    kp[..., 0] = np.where(hit, kp[..., 0] + far * np.cos(ang), kp[..., 0])
    kp[..., 1] = np.where(hit, kp[..., 1] + far * np.sin(ang), kp[..., 1])
    return kp.astype(np.asarray(kpts).dtype), hit


def _frozen(out):
    for a in out.values():
        if isinstance(a, np.ndarray):
            a.setflags(write=False)
    return out


@functools.lru_cache(maxsize=None)
def joint_case(rig_name, shape, rec_dtype="float64", kp_dtype="float64", sprinkle=True):
    """refine_cases.case(rig, shape, 1.0, sprinkle, ...) with the outliers; `moved` [F, C, Pmax, kn]: which detections; read-only."""
    cs = dict(rc.case(rig_name, shape, 1.0, sprinkle, rec_dtype, kp_dtype))
    cs["kpts"], cs["moved"] = _moved(cs["kpts"], rc._seed("huber-joints", rig_name, shape, sprinkle))
    return _frozen(cs)


@functools.lru_cache(maxsize=None)
def pose_case(rig_name, shape, rec_dtype="float64", kp_dtype="float64"):
    """pose_cases.case(rig, shape, 1.0, True, ...) with the outliers; read-only."""
    cs = dict(pc.case(rig_name, shape, 1.0, True, rec_dtype, kp_dtype))
    cs["kpts"], cs["moved"] = _moved(cs["kpts"], rc._seed("huber-pose", rig_name, shape))
    cs["kw"] = dict(cs["kw"])
    return _frozen(cs)


@functools.lru_cache(maxsize=None)
def joint_reference(rig_name, shape, start, delta, rec_dtype="float64", kp_dtype="float64", iters=4, score_weights=False):
    """refine_joints_reference with huber_px = delta on a joint case -> (out, cost, codes, views used, outliers) -- without the last
    for delta None or 0; read-only, computed once."""
    cs = joint_case(rig_name, shape, rec_dtype, kp_dtype)
    res = rf.refine_joints_reference(cs["K"], cs["R"], cs["t"], cs[start], cs["kpts"], iters=iters, score_weights=score_weights,
                                     return_views=True, huber_px=delta, **rc.refine_kwargs(cs))
    for a in res:
        a.setflags(write=False)
    return res


@functools.lru_cache(maxsize=None)
def pose_reference(rig_name, shape, delta, rec_dtype="float64", kp_dtype="float64", score_weights=False):
    """refine_cameras_reference with huber_px = delta on a pose case's drifted rig -> (R, t, report, S); computed once."""
    cs = pose_case(rig_name, shape, rec_dtype, kp_dtype)
    return pose.refine_cameras_reference(cs["K"], cs["Rd"], cs["td"], cs["xyzs"], cs["kpts"], score_weights=score_weights,
                                         return_sets=True, huber_px=delta, **cs["kw"])


def rule_at(cs, start, points, used, delta, score_weights=False):
    """The rule's E and regimes at the points `points` [F, P, kn, >= 3] over the view sets `used` [F, P, kn] uint32, with the
    observations and weights of the case's records cs[start] (the view set is the caller's: nothing is decided again here)
    -> E [F, P, kn], linear [F, P, kn] uint32 (bit c: camera c is in `used` and in the linear regime), s [C, F, P, kn] (the squared
    pixel residual of every camera, whatever `used` says).  Plain operations in the rule's order, the views added in camera order."""
    K, R, t = cs["K"], cs["R"], cs["t"]
    kw = rc.refine_kwargs(cs)
    _, _, obs = rf.observation_sets(K, R, t, cs[start], cs["kpts"], kw["det_of"], kw["n_persons"], kw["views"],
                                    kw["keypoint_score_threshold"], score_weights)
    F, P, kn = used.shape
    N = F * P * kn
    X = np.asarray(points).astype(np.float64).reshape(N, -1)[:, :3]
    X = np.where(np.isfinite(X), X, 0.0)
    V = np.asarray(used).astype(np.uint32).reshape(N)
    E, lin, s_all = np.zeros(N), np.zeros(N, dtype=np.uint32), np.zeros((K.shape[0], N))
    with np.errstate(all="ignore"):
        for c in range(K.shape[0]):
            in_ = ((V >> np.uint32(c)) & 1).astype(bool)
            _, _, _, u, v, _ = rf.project_camera(K[c], R[c], t[c], X)
            ou, ov, w = np.where(in_, obs[c, :, 0], 0.0), np.where(in_, obs[c, :, 1], 0.0), np.where(in_, obs[c, :, 2], 0.0)
            ru, rv = u - ou, v - ov
            s = ru * ru + rv * rv
            s_all[c] = s
            if delta is None:
                E = E + np.where(in_, w * s, 0.0)
            else:
                rho, _, linear = rf.huber_terms(s, delta)
                E = E + np.where(in_, w * rho, 0.0)
                lin |= (in_ & linear).astype(np.uint32) << np.uint32(c)
    return E.reshape(F, P, kn), lin.reshape(F, P, kn), s_all.reshape(-1, F, P, kn)


def pixel_margin(cs, points):
    """How far rounding a point to float32 can move its pixel in any camera of the case's rig, per record [F, P, kn], in px: half a
    float32 ulp of each coordinate (the rounding), times the sum over the coordinates of the largest |du / dX_k|, |dv / dX_k| over
    the cameras at that point, with a factor 2 for the second-order remainder and the Euclidean norm of (du, dv)."""
    K, R, t = cs["K"], cs["R"], cs["t"]
    X = np.asarray(points).astype(np.float64)[..., :3]
    X = np.where(np.isfinite(X), X, 0.0)
    shape = X.shape[:-1]
    Xf = X.reshape(-1, 3)
    half_ulp = 0.5 * np.spacing(np.abs(Xf).astype(np.float32)).astype(np.float64)           # [N, 3]
    worst = np.zeros(Xf.shape[0])
    with np.errstate(all="ignore"):
        for c in range(K.shape[0]):
            x, y, pc2, _, _, _ = rf.project_camera(K[c], R[c], t[c], Xf)
            move = np.zeros(Xf.shape[0])
            for k in range(3):
                dx, dy = (R[c, k, 0] - x * R[c, k, 2]) / pc2, (R[c, k, 1] - y * R[c, k, 2]) / pc2
                du, dv = K[c, 0, 0] * dx + K[c, 0, 1] * dy, K[c, 1, 1] * dy
                move = move + np.hypot(du, dv) * half_ulp[:, k]
            worst = np.maximum(worst, np.where(np.isfinite(move), move, 0.0))
    return (2.0 * worst).reshape(shape)


def popcount(a):
    a = np.asarray(a).astype(np.uint32)
    return sum(((a >> np.uint32(c)) & 1).astype(np.int64) for c in range(32))


# ------------------------------------------------------------------------------------------------ hand-made records
def all_linear_case(rig_name="ring5", far=40.0):
    """One frame, four joints, every camera holds a usable observation, and EVERY observation of joint 0 is moved by `far` px (each
    camera in its own direction), so all of its views are in the linear regime at X0 for delta 3 and 6.  -> dict like rc.case."""
    cs = dict(rc.behind_case(rig_name))
    K, R, t = cs["K"], cs["R"], cs["t"]
    C = K.shape[0]
    rng = np.random.default_rng(rc._seed("huber-all-linear", rig_name))
    from snowmocap_amd import synth
    X = synth.make_people(rng, 1, 1, J=4)
    uv, _ = synth.project(K, R, t, X)
    kp = np.concatenate([np.moveaxis(uv, 0, 1) + rng.normal(0.0, 1.0, (1, C, 1, 4, 2)), np.ones((1, C, 1, 4, 1))], axis=-1)
    ang = rng.uniform(0.0, 2.0 * np.pi, C)
    kp[0, :, 0, 0, 0] += far * np.cos(ang)
    kp[0, :, 0, 0, 1] += far * np.sin(ang)
    cs.update(X=X, kpts=kp, dlt=np.concatenate([X + 0.004, np.ones((1, 1, 4, 1))], axis=-1))
    cs.pop("behind")
    return cs


def two_views_case(rig_name="ring5", far=60.0):
    """One frame, four joints, and a views mask that leaves joint 0 cameras 0 and 1 only, camera 1's observation moved by `far` px:
    two views of which one is an outlier.  -> dict like rc.case (views given)."""
    cs = all_linear_case(rig_name, far=0.0)
    kp = np.array(cs["kpts"], copy=True)
    kp[0, 1, 0, 0, 0] += far
    views = np.full((1, 1, 4), 0xffffffff, dtype=np.uint32)
    views[0, 0, 0] = 0b11
    cs.update(kpts=kp, views=views)
    return cs


# ------------------------------------------------------------------------------------------------ 50-digit arithmetic: joints
def exact_huber_minimum(K, R, t, obs, X0, delta, tol="1e-30", max_steps=MAX_EXACT_STEPS):
    """IRLS on E(X) = sum_c w_c rho(|proj_c(X) - (u_c, v_c)|^2) in DIGITS-digit arithmetic from the fp64 values of K, R, t and the
    observations obs = [(c, u, v, w), ...], started at X0: H = sum w kappa J^T J, g = sum w kappa J^T r, X += -H^-1 g, until |step| <
    tol or max_steps -> (X [3] rounded once to fp64, E as float, steps, settled, the number of views in the quadratic regime at X)."""
    import mpmath as mp
    with mp.workdps(DIGITS):
        m = lambda a: mp.mpf(float(a))
        d_, dd = m(delta), m(delta) * m(delta)
        cams = []
        for c, u, v, w in obs:
            cams.append(([[m(R[c][k, i]) for k in range(3)] for i in range(3)], [m(a) for a in t[c]],
                         m(K[c][0, 0]), m(K[c][0, 1]), m(K[c][0, 2]), m(K[c][1, 1]), m(K[c][1, 2]), m(u), m(v), m(w)))
        X = [m(a) for a in X0]
        tol = mp.mpf(tol)

        def sums(X, steer=True):
            H, g, E, quad = mp.zeros(3, 3), mp.zeros(3, 1), mp.mpf(0), 0
            for Rt, tc, fx, s, cx, fy, cy, u, v, w in cams:
                d = [X[i] - tc[i] for i in range(3)]
                pc_ = [Rt[i][0] * d[0] + Rt[i][1] * d[1] + Rt[i][2] * d[2] for i in range(3)]
                x, y = pc_[0] / pc_[2], pc_[1] / pc_[2]
                ru, rv = fx * x + s * y + cx - u, fy * y + cy - v
                ss = ru * ru + rv * rv
                if ss <= dd:
                    rho, kap, quad = ss, mp.mpf(1), quad + 1
                else:
                    r = mp.sqrt(ss)
                    rho, kap = 2 * d_ * r - dd, d_ / r
                E += w * rho
                if not steer:
                    continue
                dx = [(Rt[0][k] - x * Rt[2][k]) / pc_[2] for k in range(3)]
                dy = [(Rt[1][k] - y * Rt[2][k]) / pc_[2] for k in range(3)]
                du = [fx * dx[k] + s * dy[k] for k in range(3)]
                dv = [fy * dy[k] for k in range(3)]
                wk = w * kap
                for a in range(3):
                    g[a] += wk * (du[a] * ru + dv[a] * rv)
                    for b in range(3):
                        H[a, b] += wk * (du[a] * du[b] + dv[a] * dv[b])
            return E, g, H, quad

        settled = False
        for step in range(max_steps):
            _, g, H, _ = sums(X)
            dlt = mp.lu_solve(H, -g)
            X = [X[i] + dlt[i] for i in range(3)]
            if mp.sqrt(dlt[0] ** 2 + dlt[1] ** 2 + dlt[2] ** 2) < tol:
                settled = True
                break
        E, _, _, quad = sums(X, steer=False)
        return np.array([float(a) for a in X]), float(E), step + 1, settled, quad


@functools.lru_cache(maxsize=None)
def joint_minimiser(rig_name, delta, shape=ACCURACY_SHAPE, start="dlt"):
    """The 50-digit minimiser of every record of joint_case(rig, shape) that the rule refines, over the rule's own view set, started
    at the NumPy rule's output (iters = ACCURACY_ITERS) -> dict(X [F,P,kn,3] (NaN where none was computed), refined [F,P,kn] bool,
    covered [F,P,kn] bool: the minimiser settled and leaves at least MIN_QUADRATIC views in the quadratic regime); read-only.
    A record with fewer than MIN_QUADRATIC quadratic views at the rule's own output is not covered and its minimiser is not run (it
    is the record on which IRLS needs hundreds of steps): that only narrows `covered`, whose share the tests assert."""
    cs = joint_case(rig_name, shape)
    out, _, codes, used, outl = joint_reference(rig_name, shape, start, delta, iters=ACCURACY_ITERS)
    F, P, kn = shape
    kp = np.asarray(cs["kpts"]).astype(np.float64)
    Xm = np.full((F, P, kn, 3), np.nan)
    refined = codes >= 2
    covered = np.zeros((F, P, kn), dtype=bool)
    enough = popcount(used & ~outl) >= MIN_QUADRATIC
    for f, p, j in zip(*np.nonzero(refined & enough)):
        obs = []
        for c in range(cs["K"].shape[0]):
            if (int(used[f, p, j]) >> c) & 1:
                q = int(cs["det_of"][f, c, p])
                obs.append((c, kp[f, c, q, j, 0], kp[f, c, q, j, 1], 1.0))
        Xm[f, p, j], _, _, settled, quad = exact_huber_minimum(cs["K"], cs["R"], cs["t"], obs, out[f, p, j, :3], delta)
        covered[f, p, j] = settled and quad >= MIN_QUADRATIC
    return _frozen(dict(X=Xm, refined=refined, covered=covered))


# ------------------------------------------------------------------------------------------------ 50-digit arithmetic: cameras
def _mp_huber_terms(mp, Kc, R, t, X, ou, ov, w, delta):
    """pose_cases._mp_terms with the loss: -> E, g [6], H [6][6] and the sums of |term| of each, at the pose (R, t) of mpf."""
    m = lambda a: mp.mpf(float(a))
    fx, sk, cx, fy, cy = m(Kc[0, 0]), m(Kc[0, 1]), m(Kc[0, 2]), m(Kc[1, 1]), m(Kc[1, 2])
    d_, dd = m(delta), m(delta) * m(delta)
    E, aE = mp.mpf(0), mp.mpf(0)
    g, ag = [mp.mpf(0)] * 6, [mp.mpf(0)] * 6
    H, aH = [[mp.mpf(0)] * 6 for _ in range(6)], [[mp.mpf(0)] * 6 for _ in range(6)]
    for n in range(X.shape[0]):
        d = [m(X[n, i]) - t[i] for i in range(3)]
        pc_ = [R[0][i] * d[0] + R[1][i] * d[1] + R[2][i] * d[2] for i in range(3)]
        x, y = pc_[0] / pc_[2], pc_[1] / pc_[2]
        ru, rv, wn = fx * x + sk * y + cx - m(ou[n]), fy * y + cy - m(ov[n]), m(w[n])
        ss = ru * ru + rv * rv
        if ss <= dd:
            rho, kap = ss, mp.mpf(1)
        else:
            r = mp.sqrt(ss)
            rho, kap = 2 * d_ * r - dd, d_ / r
        du, dv = [], []
        for k in range(6):
            if k < 3:
                a_, b_ = (k + 1) % 3, (k + 2) % 3
                col = [R[a_][i] * d[b_] - R[b_][i] * d[a_] for i in range(3)]
            else:
                col = [-R[k - 3][i] for i in range(3)]
            dx, dy = (col[0] - x * col[2]) / pc_[2], (col[1] - y * col[2]) / pc_[2]
            du.append(fx * dx + sk * dy)
            dv.append(fy * dy)
        e = wn * rho
        E, aE = E + e, aE + abs(e)
        wk = wn * kap
        for a in range(6):
            ga = wk * (du[a] * ru + dv[a] * rv)
            g[a], ag[a] = g[a] + ga, ag[a] + abs(ga)
            for b in range(a + 1):
                h = wk * (du[a] * du[b] + dv[a] * dv[b])
                H[a][b], aH[a][b] = H[a][b] + h, aH[a][b] + abs(h)
                H[b][a] = H[a][b]
    return E, g, H, aE, ag, aH


def exact_huber_normal(Kc, Rc, tc, X, ou, ov, w, delta):
    """E, g, H of the loss for one camera at the fp64 pose (Rc, tc) in DIGITS-digit arithmetic -> (normal [28] rounded once to fp64,
    the sums of |term| [28]): pose_cases.exact_normal with the loss."""
    import mpmath as mp
    with mp.workdps(DIGITS):
        R = [[mp.mpf(float(Rc[i, j])) for j in range(3)] for i in range(3)]
        t = [mp.mpf(float(a)) for a in tc]
        E, g, H, aE, ag, aH = _mp_huber_terms(mp, Kc, R, t, X, ou, ov, w, delta)
        val = [E] + g + [H[a][b] for a, b in pose.H_INDEX]
        mag = [aE] + ag + [aH[a][b] for a, b in pose.H_INDEX]
        return np.array([float(v) for v in val]), np.array([float(v) for v in mag])


def exact_huber_pose_minimum(Kc, R0, t0, X, ou, ov, w, delta, tol="1e-30", max_steps=MAX_EXACT_STEPS):
    """IRLS on the loss' E(omega, tau) in DIGITS-digit arithmetic from the fp64 pose (R0, t0), the pose updated as the rule updates it,
    until |delta| < tol -> (R [3, 3], t [3] rounded once to fp64, E as float, steps): pose_cases.exact_pose_minimum with the loss."""
    import mpmath as mp
    with mp.workdps(DIGITS):
        R = [[mp.mpf(float(R0[i, j])) for j in range(3)] for i in range(3)]
        t = [mp.mpf(float(a)) for a in t0]
        tol = mp.mpf(tol)
        for step in range(max_steps):
            E, g, H, _, _, _ = _mp_huber_terms(mp, Kc, R, t, X, ou, ov, w, delta)
            dl = mp.lu_solve(mp.matrix(H), -mp.matrix(g))
            om = [dl[0], dl[1], dl[2]]
            th = mp.sqrt(om[0] ** 2 + om[1] ** 2 + om[2] ** 2)
            a, b = (mp.sin(th) / th, 2 * mp.sin(th / 2) ** 2 / th ** 2) if th > 0 else (mp.mpf(1), mp.mpf(1) / 2)
            W = [[0, -om[2], om[1]], [om[2], 0, -om[0]], [-om[1], om[0], 0]]
            Ex = [[(1 if i == j else 0) + a * W[i][j] + b * sum(W[i][k] * W[k][j] for k in range(3)) for j in range(3)] for i in range(3)]
            R = [[sum(Ex[i][k] * R[k][j] for k in range(3)) for j in range(3)] for i in range(3)]
            t = [t[i] + dl[3 + i] for i in range(3)]
            if mp.sqrt(sum(dl[i] ** 2 for i in range(6))) < tol:
                break
        else:
            raise AssertionError("the exact IRLS iteration did not settle")
        E = _mp_huber_terms(mp, Kc, R, t, X, ou, ov, w, delta)[0]
        return np.array([[float(v) for v in row] for row in R]), np.array([float(v) for v in t]), float(E), step + 1


POSE_MINIMISER_RIGS = KERNEL_RIGS
POSE_MINIMISER_SHAPE = pc.MINIMISER_SHAPE


def camera_observations(cs, S, c):
    """The observations of camera c of a pose case as the rule sees them -> X [n, 3], ou, ov, w [n] (record order)."""
    X, S2, obs = pose.observation_sets(cs["K"], cs["Rd"], cs["td"], cs["xyzs"], cs["kpts"], cs["det_of"], cs["n_persons"], cs["views"], cs["thr"])
    assert np.array_equal(S, S2)
    return X[S[c]], obs[c, S[c], 0], obs[c, S[c], 1], obs[c, S[c], 2]


@functools.lru_cache(maxsize=None)
def pose_minimiser(rig_name, delta, shape=POSE_MINIMISER_SHAPE):
    """The 50-digit minimiser of the loss for every free camera of pose_case(rig, shape) with at least MIN_OBS observations, over the
    rule's own S_c, started at the NumPy rule's output -> dict(R [C,3,3], t [C,3], cams: the cameras computed); read-only."""
    cs = pose_case(rig_name, shape)
    Rr, tr, rep, S = pose_reference(rig_name, shape, delta)
    Rm, tm, cams = np.array(Rr, copy=True), np.array(tr, copy=True), []
    for c in cs["free"]:
        if rep["n_obs"][c] < pc.MIN_OBS:
            continue
        X, ou, ov, w = camera_observations(cs, S, c)
        Rm[c], tm[c], _, _ = exact_huber_pose_minimum(cs["K"][c], Rr[c], tr[c], X, ou, ov, w, delta)
        cams.append(c)
    return _frozen(dict(R=Rm, t=tm, cams=tuple(cams)))


# measured by tests/test_huber_host.py::test_camera_reference_against_the_exact_huber_minimiser (CPU, the NumPy rule, float64,
# iters = 8, min_obs = 6, POSE_MINIMISER_SHAPE with the sprinkles and the outliers, POSE_MINIMISER_RIGS, delta 3 and 6): the largest
# (|R - R_min| entry, |t - t_min| / rig scale) over the free cameras.  The host test measures it again and fails if it has moved by
# more than a factor of two; the kernels are held to pose_cases.MARGIN x this.
# Measured: (4.519e-9, 5.162e-9), both on ring16 at delta 6 (ring8 3.8e-9 / 3.7e-9, floor 1.7e-9 / 2.3e-9, ring3 3.4e-10 / 4.2e-10):
# the size of pose_cases.FLOOR_NOISY, 4 .. 8 accepted steps.
POSE_FLOOR = (4.519e-9, 5.162e-9)
