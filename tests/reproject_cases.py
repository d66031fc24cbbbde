"""Inputs shared by tests/test_reproject_host.py and tests/test_gpu_reproject.py (k_reproject, k_reproject_cost): world points with
their projections in 50-digit arithmetic, the launch shapes, the cost workloads and the permuted recordings of the matching tests.
No GPU code; everything is seeded.

Rigs are those of tests/undistort_cases.py (`uc.rig`: a skewed K and a lens of its own per camera, fx <= 760).  Each camera c of a rig
owns 48 WORLD POINTS: the first 48 true pixels of `uc.pool(rig, c)` (box [-50, 1330] x [-50, 770]) back-projected to depths of
1.5 .. 6 m, so every camera has points all over its own image.  A placement of tests/dlt_frames_cases.py moves rig and points
together (t' = u (t + D), X' = u (X + D)): six positions / units of the world, the same pixels.  `exact(...)` projects every point
of a rig's pool into EVERY camera with mpmath, formed from the fp64 values of K, R, t', D, X' (of the float32 roundings of X' for
float32 records): the undistorted pixel, the raw pixel (the lens is oracle.undistort_exact._distort), and pc2 and |d| / pc2 of the
point in that camera.  A case draws its [F, P, kn] records from the pool, so every lane of every shape has an exact answer.

The accuracy bars hold where the tests' derivation holds, IN_DOMAIN: pc2 > 0 and |d| / pc2 <= 1.8 in the camera at hand.  A point
always is in the domain of the camera it was made for (|d| / pc2 <= 1.6 at the corners of the box); a camera that sees the point at a
grazing angle divides by a small pc2, and the error of x = pc0 / pc2 grows with |d| / pc2 without bound.
"""
import functools
import zlib

import numpy as np

import dlt_frames_cases as fc
import undistort_cases as uc
from snowmocap_amd import synth

RIGS = tuple(uc.RIGS)                            # ring3, ring5, ring8, floor, floor-s0
PLACEMENTS = tuple(fc.PLACEMENTS)
PER_CAM = 48
DEPTHS = (1.5, 6.0)
DOMAIN = 1.8                                     # |d| / pc2
SHAPES = [(1, 1, 1), (3, 1, 17), (1, 3, 21), (2, 1, 64), (5, 2, 133)]      # (F, P, kn)
BLOCK_SHAPE = (1, 1, 256)                        # on a 4-camera rig: one block per camera
CUT_SHAPE = (40, 1, 133)
CUTS = (1, 7, 39)
DIGITS = 50

# what the tests hold the float64 pixels to (px); the arithmetic is in the docstring of tests/test_gpu_reproject.py
BAR_F64 = 1e-11
BAR_F64_RAW = 2e-11
F32_EXTRA = 1e-9


def shapes_of(rig_name):
    return SHAPES + ([BLOCK_SHAPE] if uc.RIGS[rig_name][0] == 4 else [])


def _seed(*parts):
    return zlib.crc32(repr(parts).encode())


@functools.lru_cache(maxsize=None)
def rig(rig_name, placement="home"):
    """-> K, R, t' (placed), D; read-only."""
    K, R, t, D, _ = uc.rig(rig_name)
    tp, _, _, _ = fc.place(t, None, placement)
    out = (K.copy(), R.copy(), np.ascontiguousarray(tp), D.copy())
    for a in out:
        a.setflags(write=False)
    return out


@functools.lru_cache(maxsize=None)
def points(rig_name, placement="home", dtype_name="float64"):
    """-> X' [C * PER_CAM, 3] float64 values representable in `dtype_name`, owner [C * PER_CAM] (the camera a point was made for)."""
    K, R, t, _, _ = uc.rig(rig_name)
    C = K.shape[0]
    X, owner = [], []
    for c in range(C):
        rng = np.random.default_rng(_seed("points", rig_name, c))
        px = uc.pool(rig_name, c)["true"][:PER_CAM]
        depth = rng.uniform(*DEPTHS, PER_CAM)
        ray = np.linalg.solve(K[c], np.concatenate([px, np.ones((PER_CAM, 1))], axis=1).T).T        # z = 1
        X.append(t[c] + (ray * depth[:, None]) @ R[c].T)
        owner += [c] * PER_CAM
    _, Xp, _, _ = fc.place(t, np.concatenate(X), placement)
    Xp = Xp.astype(dtype_name).astype(np.float64)
    Xp.setflags(write=False)
    return Xp, np.array(owner)


def _camera_mp(K, R, t, D):
    import mpmath as mp
    m = lambda a: mp.mpf(float(a))
    return ([[m(R[k, i]) for k in range(3)] for i in range(3)], [m(v) for v in t], [m(K[0, 0]), m(K[0, 1]), m(K[0, 2]), m(K[1, 1]), m(K[1, 2])],
            None if D is None else [m(k) for k in np.asarray(D).reshape(-1)[:5]])


def project_exact_mp(K, R, t, D, X, cam=None):
    """One point into one camera in DIGITS-digit arithmetic, formed from the fp64 values: -> (u, v, u_raw, v_raw, pc2, |d| / pc2) as mpf
    (the raw pixel is None without D).  cam: _camera_mp(K, R, t, D), when many points go into one camera."""
    import mpmath as mp
    from oracle import undistort_exact as ue
    with mp.workdps(DIGITS):
        Rt, tm, (fx, s, cx, fy, cy), Dm = cam or _camera_mp(K, R, t, D)
        d = [mp.mpf(float(X[i])) - tm[i] for i in range(3)]
        pc = [Rt[i][0] * d[0] + Rt[i][1] * d[1] + Rt[i][2] * d[2] for i in range(3)]                 # R^T d
        x, y = pc[0] / pc[2], pc[1] / pc[2]
        u, v = fx * x + s * y + cx, fy * y + cy
        ur = vr = None
        if Dm is not None:
            xd, yd, _, _, _ = ue._distort(x, y, Dm)
            ur, vr = fx * xd + s * yd + cx, fy * yd + cy
        return u, v, ur, vr, pc[2], mp.sqrt(d[0] * d[0] + d[1] * d[1] + d[2] * d[2]) / abs(pc[2])


@functools.lru_cache(maxsize=None)
def exact(rig_name, placement="home", dtype_name="float64"):
    """Every point of the pool in every camera -> dict(X [N,3], owner [N], uv [C,N,2], raw [C,N,2] (exact values rounded once to fp64),
    depth [C,N] (pc2 in world units), ratio [C,N] (|d| / pc2), in_domain [C,N]); read-only."""
    import mpmath as mp
    K, R, t, D = rig(rig_name, placement)
    X, owner = points(rig_name, placement, dtype_name)
    C, N = K.shape[0], X.shape[0]
    uv, raw = np.empty((C, N, 2)), np.empty((C, N, 2))
    depth, ratio = np.empty((C, N)), np.empty((C, N))
    with mp.workdps(DIGITS):
        for c in range(C):
            cam = _camera_mp(K[c], R[c], t[c], D[c])
            for i in range(N):
                u, v, ur, vr, z, q = project_exact_mp(None, None, None, None, X[i], cam)
                uv[c, i], raw[c, i], depth[c, i], ratio[c, i] = (float(u), float(v)), (float(ur), float(vr)), float(z), float(q)
    out = dict(X=X, owner=owner, uv=uv, raw=raw, depth=depth, ratio=ratio, in_domain=(depth > 0) & (ratio <= DOMAIN))
    for a in out.values():
        a.setflags(write=False)
    return out


@functools.lru_cache(maxsize=None)
def case(rig_name, shape, placement="home", dtype_name="float64"):
    """-> dict(K, R, t, D, xyzs [F,P,kn,4] of `dtype_name` (scores in (0.1, 9)), uv / raw [F,C,P,kn,2] exact pixels, in_domain
    [F,C,P,kn], depth [F,C,P,kn]); read-only."""
    F, P, kn = shape
    K, R, t, D = rig(rig_name, placement)
    ex = exact(rig_name, placement, dtype_name)
    rng = np.random.default_rng(_seed("case", rig_name, shape))
    idx = rng.integers(0, ex["X"].shape[0], (F, P, kn))
    xyzs = np.empty((F, P, kn, 4))
    xyzs[..., :3] = ex["X"][idx]
    xyzs[..., 3] = rng.uniform(0.1, 9.0, (F, P, kn))
    xyzs = xyzs.astype(dtype_name)
    assert np.array_equal(xyzs[..., :3].astype(np.float64), ex["X"][idx])
    gather = lambda a: np.ascontiguousarray(np.moveaxis(a[:, idx], 0, 1))                             # [C, F, P, kn, ...] -> [F, C, ...]
    out = dict(K=K, R=R, t=t, D=D, xyzs=xyzs, uv=gather(ex["uv"]), raw=gather(ex["raw"]), in_domain=gather(ex["in_domain"]),
               depth=gather(ex["depth"]))
    for a in out.values():
        a.setflags(write=False)
    return out


# ------------------------------------------------------------------------------------------------ cost workloads
COST_SHAPES = [(3, 1, 1, 1, 1), (4, 1, 1, 133, 5), (4, 3, 3, 133, 6), (8, 4, 4, 133, 4), (3, 2, 5, 17, 5), (4, 3, 2, 65, 3),
               (4, 2, 2, 64, 3)]                                                                       # (C, P, Pmax, kn, F)
COST_RIG = {3: "ring3", 4: "floor", 8: "ring8"}
COST_THRESHOLD = 0.5


@functools.lru_cache(maxsize=None)
def cost_case(shape, kp_dtype="float64", with_n_persons=False):
    """P persons standing around the middle of the scene (synth.make_people on the 1.5 m circle: every joint inside the accuracy domain
    of every camera, which the tests assert), a few records missing; Pmax detections per camera: the exact raw-frame / undistorted
    projection of person q % P plus N(0, 2 px) -- detection q against person p != q % P is a real mismatch of hundreds of pixels --
    a tenth of them scored below the threshold, one in 40 with a NaN u or v.  The detections are made for `raw` = False and True alike
    (they are noise around the undistorted pixel; the raw comparison just sees other residuals).
    -> dict(K, R, t, D, xyzs [F,P,kn,4] float64, kpts [F,C,Pmax,kn,3] of kp_dtype, n_persons [F,C] int32 or None, thr); read-only."""
    C, P, Pmax, kn, F = shape
    K, R, t, D, _ = uc.rig(COST_RIG[C])
    rng = np.random.default_rng(_seed("cost", shape))
    X = synth.make_people(rng, F, P, J=kn)
    xyzs = np.concatenate([X, rng.uniform(0.5, 9.0, (F, P, kn, 1))], axis=-1)
    if F * P * kn > 8:
        gone = rng.random((F, P, kn)) < 0.03
        xyzs[gone] = 0.0
    uv, _ = synth.project(K, R, t, X)                                                                 # [C, F, P, kn, 2]
    uv = np.moveaxis(uv, 0, 1)
    kp = np.empty((F, C, Pmax, kn, 3))
    for q in range(Pmax):
        kp[:, :, q, :, :2] = uv[:, :, q % P] + rng.normal(0.0, 2.0, (F, C, kn, 2))
    kp[..., 2] = np.where(rng.random((F, C, Pmax, kn)) < 0.1, rng.uniform(0.0, 0.499, (F, C, Pmax, kn)), rng.uniform(0.5, 8.0, (F, C, Pmax, kn)))
    if kp[..., 0].size > 8:
        bad = rng.random((F, C, Pmax, kn)) < 0.025
        which = rng.integers(0, 2, (F, C, Pmax, kn))
        kp[..., 0] = np.where(bad & (which == 0), np.nan, kp[..., 0])
        kp[..., 1] = np.where(bad & (which == 1), np.nan, kp[..., 1])
    npers = rng.integers(0, Pmax + 1, (F, C)).astype(np.int32) if with_n_persons else None
    out = dict(K=K, R=R, t=t, D=D, xyzs=xyzs, kpts=kp.astype(kp_dtype), n_persons=npers, thr=COST_THRESHOLD)
    for a in out.values():
        if isinstance(a, np.ndarray):
            a.setflags(write=False)
    return out


def domain_ratio(K, R, t, xyzs):
    """|d| / pc2 [F, C, P, kn] of the measured records (NaN for the others) in plain fp64: which projections the bars cover."""
    x = np.asarray(xyzs, dtype=np.float64)
    out = np.empty((x.shape[0], K.shape[0]) + x.shape[1:3])
    with np.errstate(all="ignore"):
        for c in range(K.shape[0]):
            d = x[..., :3] - t[c]
            z = d @ R[c][:, 2]
            out[:, c] = np.where((x[..., 3] != 0) & np.isfinite(x).all(axis=-1), np.linalg.norm(d, axis=-1) / z, np.nan)
    return out


# ------------------------------------------------------------------------------------------------ matching recordings
MATCH_RIGS = [(4, 3), (8, 4), (3, 2)]            # cameras x persons
MATCH_F = 4
MATCH_GATE = 6.0
MATCH_THRESHOLD = 0.5


@functools.lru_cache(maxsize=None)
def match_case(C, P, F=MATCH_F):
    """synth.ring_rig(C), P persons on the 1.5 m circle; detections = synth.project + N(0, 1 px), scores U(0, 8), each (f, c) list in
    the order perm[f, c] (detection q of camera c is person perm[f, c, q]).
    -> dict(K, R, t, X [F,P,133,3], xyzs [F,P,133,4] (score 1), kpts [F,C,P,133,3] float64, n_persons, perm [F,C,P], det_true [F,C,P]
    (the detection that shows person p)); read-only."""
    K, R, t = synth.ring_rig(C)
    rng = np.random.default_rng(_seed("match", C, P, F))
    X = synth.make_people(rng, F, P)
    J = X.shape[2]
    uv, _ = synth.project(K, R, t, X)
    uv = np.moveaxis(uv, 0, 1) + rng.normal(0.0, 1.0, (F, C, P, J, 2))
    rec = np.concatenate([uv, rng.uniform(0.0, 8.0, (F, C, P, J, 1))], axis=-1)
    perm = np.empty((F, C, P), dtype=np.int64)
    kp = np.empty_like(rec)
    for f in range(F):
        for c in range(C):
            perm[f, c] = rng.permutation(P)
            kp[f, c] = rec[f, c, perm[f, c]]
    det_true = np.argsort(perm, axis=-1)
    xyzs = np.concatenate([X, np.ones(X.shape[:-1] + (1,))], axis=-1)
    out = dict(K=K, R=R, t=t, X=X, xyzs=xyzs, kpts=kp, n_persons=np.full((F, C), P, dtype=np.int32), perm=perm, det_true=det_true)
    for a in out.values():
        a.setflags(write=False)
    return out
