"""Inputs shared by tests/test_refine_host.py and tests/test_gpu_refine.py (k_refine, snowmocap_amd/refine.py): rigs, persons,
noisy detections with everything a recording sprinkles in, the two closed-form start points, and the exact minimiser of the
reprojection cost in 50-digit arithmetic.  No GPU code; everything is seeded.

Rigs: the five of tests/undistort_cases.py (3, 4, 5, 8 cameras, skewed K; their lenses are not used: refinement works on the
undistorted frame) and synth.ring_rig(16) for the kernel's generic-C path.  Persons: synth.make_people on the 1.5 m circle, so every
joint lies within |d| / pc2 <= 1.8 of every camera (`assert_domain`): no record has to be left out of any comparison.  Detections:
exact projections + N(0, sigma).  A placement of tests/dlt_frames_cases.py moves rig, truth and start points together; the pixels
stay.

SPRINKLED IN (`sprinkle=True`; the lists then have Pmax = P + 1 slots): 3 % missing records (zero records, one with a NaN x, one
with the score -0.0), 10 % of the observations scored below the threshold, one in 40 with a NaN u or v, every camera's list permuted
with the true det_of, 5 % of the det_of rows -1, an n_persons that cuts one list in ten short by one, a `views` mask that removes one
camera on 10 % of the joints, and -- where the shape has at least 8 records -- record 1 with exactly ONE view left and record 2 with
exactly TWO (by the `views` mask, over observations repaired to be usable).  `behind_case` is the point behind one camera.

START POINTS, NumPy, computed at home from the observations that count: `pair` = the mean of the two-ray midpoints over the pairs of
usable views weighted by the product of their scores, `dlt` = the homogeneous least-squares point.  A record with fewer than two
usable views starts 1 cm from the truth.

EXACT MINIMISER (`exact_minimum`): per record Gauss-Newton on the rule's cost with the rule's view set and weights, in 50-digit
mpmath, started at the truth and run until the step is below 1e-30 (home metres); computed for MINIMISER_SHAPE on every rig at sigma 1
and 2 and cached per process.

THE ACCURACY BAR.  The rule accepts a step only while E decreases strictly in fp64, so it stops resolving a step d once
d^T H d < eps E, i.e. |d| ~ sqrt(eps E / lambda_min(H)): with E of a few px^2 and lambda_min(H) of 1e4 .. 1e5 px^2 / m^2 that is
1e-10 .. 1e-9 m.  REFERENCE_FLOOR is the largest distance of refine_joints_reference (iters = ACCURACY_ITERS, both starts, float64
records, both keypoint dtypes, all six rigs, sigma 1 and 2) to the exact minimiser that tests/test_refine_host.py measured on the
CPU, in units of the rig scale (the largest camera offset from the mean centre: what the DLT tests use); the test asserts that the
constant still covers what it measures.  The kernel is held to BAR = 4 x REFERENCE_FLOOR: its fma and summation order can end the
iteration one step earlier or later than the reference, and one step at the floor is worth about the floor.
"""
import functools
import zlib

import numpy as np

import dlt_frames_cases as fc
import undistort_cases as uc
from snowmocap_amd import synth
from snowmocap_amd.refine import refine_joints_reference

RIGS = tuple(uc.RIGS) + ("ring16",)              # ring3, ring5, ring8, floor, floor-s0, ring16
PLACEMENTS = tuple(fc.PLACEMENTS)
SHAPES = [(1, 1, 1), (1, 1, 64), (1, 1, 65), (3, 1, 17), (2, 3, 21), (5, 2, 133)]      # (F, P, kn)
CUT_SHAPE = (40, 1, 133)
CUTS = (1, 7, 39)
MINIMISER_SHAPE = (3, 1, 17)
SIGMAS = (0.0, 1.0, 2.0)
STARTS = ("pair", "dlt")
THRESHOLD = 0.5
DOMAIN = 1.8
DIGITS = 50
ACCURACY_ITERS = 8

# measured by tests/test_refine_host.py::test_reference_against_the_exact_minimiser (CPU, the NumPy rule): the largest
# |reference - exact minimiser| / rig scale over the six rigs, sigma 1 and 2, both starts, float64 and float32 keypoints was
# 1.829e-9 (the floor rig at sigma = 2 px: 5.9e-9 m at a rig scale of 3.22 m; the worst of the other rigs 3.2e-10 .. 9.4e-10).
# REFERENCE_FLOOR is that figure; the host test measures it again and fails if it has moved by more than a factor of two either
# way.  BAR = 4 x REFERENCE_FLOOR is what the kernel is held to (the derivation is in the docstring).
REFERENCE_FLOOR = 1.829e-9
BAR = 4.0 * REFERENCE_FLOOR


def _seed(*parts):
    return zlib.crc32(repr(parts).encode())


@functools.lru_cache(maxsize=None)
def rig(rig_name, placement="home"):
    """-> K, R, t' (placed); read-only."""
    if rig_name == "ring16":
        K, R, t = synth.ring_rig(16)
    else:
        K, R, t, _, _ = uc.rig(rig_name)
    tp, _, _, _ = fc.place(t, None, placement)
    out = (np.array(K, copy=True), np.array(R, copy=True), np.ascontiguousarray(tp))
    for a in out:
        a.setflags(write=False)
    return out


def rig_scale(t):
    """The largest camera offset from the mean centre (any axis): the unit of the accuracy bar."""
    t = np.asarray(t, dtype=np.float64)
    return float(np.max(np.abs(t - t.mean(axis=0))))


def domain_ratio(K, R, t, X):
    """|d| / pc2 [C, ...] of the points X [..., 3] in plain fp64."""
    out = np.empty((K.shape[0],) + X.shape[:-1])
    for c in range(K.shape[0]):
        d = X - t[c]
        out[c] = np.linalg.norm(d, axis=-1) / (d @ R[c][:, 2])
    return out


def assert_domain(cs):
    q = domain_ratio(cs["K"], cs["R"], cs["t"], cs["X"])
    assert (q > 0).all() and q.max() <= DOMAIN, float(q.max())


def _starts(K, R, t, obs, use, X):
    """obs [C, N, 3], use [C, N], truth X [N, 3] -> (pair [N, 3], dlt [N, 3]) at home."""
    C, N = use.shape
    rays = np.empty((C, N, 3))
    Pm = np.empty((C, 3, 4))
    for c in range(C):
        px = np.stack([obs[c, :, 0], obs[c, :, 1], np.ones(N)], axis=1)
        px = np.where(use[c][:, None], px, 1.0)
        rays[c] = np.linalg.solve(K[c], px.T).T @ R[c].T
        Pm[c] = K[c] @ np.concatenate([R[c].T, -(R[c].T @ t[c].reshape(3, 1))], axis=1)
    acc, wsum = np.zeros((N, 3)), np.zeros(N)
    for a in range(C):
        for b in range(a + 1, C):
            both = use[a] & use[b]
            da, db, w0 = rays[a], rays[b], t[a] - t[b]
            aa, bb, ab = (da * da).sum(1), (db * db).sum(1), (da * db).sum(1)
            d_, e_ = da @ w0, db @ w0
            den = aa * bb - ab * ab
            with np.errstate(all="ignore"):
                sa, sb = (ab * e_ - bb * d_) / den, (aa * e_ - ab * d_) / den
            mid = 0.5 * ((t[a] + sa[:, None] * da) + (t[b] + sb[:, None] * db))
            w = np.where(both & (den > 1e-12), obs[a, :, 2] * obs[b, :, 2], 0.0)
            acc += np.where(w[:, None] > 0, w[:, None] * mid, 0.0)
            wsum += w
    enough = use.sum(axis=0) >= 2
    fallback = X + 0.01
    with np.errstate(all="ignore"):
        pair = np.where((enough & (wsum > 0))[:, None], acc / wsum[:, None], fallback)
    A = np.zeros((N, 2 * C, 4))
    for c in range(C):
        m = use[c][:, None]
        A[:, 2 * c] = np.where(m, np.where(use[c], obs[c, :, 0], 0.0)[:, None] * Pm[c, 2] - Pm[c, 0], 0.0)
        A[:, 2 * c + 1] = np.where(m, np.where(use[c], obs[c, :, 1], 0.0)[:, None] * Pm[c, 2] - Pm[c, 1], 0.0)
    Xh = np.linalg.svd(A)[2][:, -1]
    with np.errstate(all="ignore"):
        dlt = np.where(enough[:, None], Xh[:, :3] / Xh[:, 3:4], fallback)
    return pair, dlt


@functools.lru_cache(maxsize=None)
def case(rig_name, shape, sigma=1.0, sprinkle=True, rec_dtype="float64", kp_dtype="float64", placement="home"):
    """-> dict(K, R, t (placed), X [F,P,kn,3] the truth (placed), pair / dlt [F,P,kn,4] start records of rec_dtype (placed), kpts
    [F,C,Pmax,kn,3] of kp_dtype, det_of [F,C,P] int64 / n_persons [F,C] int32 / views [F,P,kn] uint32 (None without the sprinkles),
    thr, one_view / two_views: flat record indices or None); read-only.  The random draws depend on (rig, shape, sigma, sprinkle) only."""
    F, P, kn = shape
    K, R, t0 = rig(rig_name)
    C = K.shape[0]
    rng = np.random.default_rng(_seed("refine", rig_name, shape, sigma, sprinkle))
    X = synth.make_people(rng, F, P, J=kn)
    N = F * P * kn
    uv = np.moveaxis(synth.project(K, R, t0, X)[0], 0, 1) + sigma * rng.normal(0.0, 1.0, (F, C, P, kn, 2))       # [F, C, P, kn, 2]
    sc = rng.uniform(0.5, 8.0, (F, C, P, kn))
    score = rng.uniform(0.5, 9.0, (F, P, kn))
    Pmax = P + 1 if sprinkle else P
    kp = np.zeros((F, C, Pmax, kn, 3))
    det_of = n_persons = views = one_view = two_views = None
    gone = np.zeros((F, P, kn), dtype=bool)
    if not sprinkle:
        kp[..., :2], kp[..., 2] = uv, sc
        use = np.ones((C, N), dtype=bool)
    else:
        low = rng.random((F, C, P, kn)) < 0.10
        sc = np.where(low, rng.uniform(0.0, 0.499, sc.shape), sc)
        bad = rng.random((F, C, P, kn)) < 0.025
        which = rng.integers(0, 2, (F, C, P, kn))
        finite_uv = uv.copy()
        uv[..., 0] = np.where(bad & (which == 0), np.nan, uv[..., 0])
        uv[..., 1] = np.where(bad & (which == 1), np.nan, uv[..., 1])
        det_of = np.empty((F, C, P), dtype=np.int64)
        n_persons = np.full((F, C), P, dtype=np.int32)
        views = np.full((F, P, kn), 0xffffffff, dtype=np.uint32)
        drop = rng.random((F, P, kn)) < 0.10
        views[drop] &= ~(np.uint32(1) << rng.integers(0, C, int(drop.sum())).astype(np.uint32))
        if N >= 8:                                           # records 1 and 2: exactly one and exactly two views, on usable observations
            one_view, two_views = 1, 2
            for flat, cams in ((1, (0,)), (2, (0, 1))):
                f, p, j = np.unravel_index(flat, (F, P, kn))
                views[f, p, j] = sum(1 << c for c in cams)
                for c in cams:
                    sc[f, c, p, j] = 1.0
                    uv[f, c, p, j] = finite_uv[f, c, p, j]
        keep_listed = np.zeros((F, C, P), dtype=bool)        # (f, c, p) of the repaired observations stay matched
        if N >= 8:
            for flat, cams in ((1, (0,)), (2, (0, 1))):
                f, p, j = np.unravel_index(flat, (F, P, kn))
                keep_listed[f, list(cams), p] = True
        for f in range(F):
            for c in range(C):
                perm = rng.permutation(P)                     # slot q of the list shows person perm[q]
                kp[f, c, :P, :, :2], kp[f, c, :P, :, 2] = uv[f, c, perm], sc[f, c, perm]
                kp[f, c, P, :, :2], kp[f, c, P, :, 2] = rng.uniform(0.0, 1280.0, (kn, 2)), rng.uniform(0.5, 8.0, kn)   # a junk detection
                det_of[f, c] = np.argsort(perm)
                if rng.random() < 0.10 and not keep_listed[f, c].any():
                    n_persons[f, c] = P - 1                   # whoever stands in the last slot is no longer listed
        det_of = np.where((rng.random((F, C, P)) < 0.05) & ~keep_listed, -1, det_of)
        if N >= 8:
            gone = rng.random((F, P, kn)) < 0.03
            gone.reshape(-1)[[1, 2]] = False
        listed = (det_of >= 0) & (det_of < n_persons[..., None])
        bit = ((views[:, None] >> np.arange(C, dtype=np.uint32)[None, :, None, None]) & 1).astype(bool)
        use = listed[..., None] & np.isfinite(uv).all(axis=-1) & ~(sc < THRESHOLD) & bit
        use = np.moveaxis(use, 1, 0).reshape(C, N)
    obs = np.moveaxis(np.concatenate([uv, sc[..., None]], axis=-1), 1, 0).reshape(C, N, 3)
    pair, dlt = _starts(K, R, t0, obs, use, X.reshape(N, 3))
    t, Xp, _, _ = fc.place(t0, X, placement)
    out = dict(K=K, R=R, t=np.ascontiguousarray(t), X=Xp, kpts=kp.astype(kp_dtype), det_of=det_of, n_persons=n_persons, views=views,
               thr=THRESHOLD, one_view=one_view, two_views=two_views)
    for name, start in (("pair", pair), ("dlt", dlt)):
        rec = np.concatenate([fc.place(t0, start, placement)[1].reshape(F, P, kn, 3), score[..., None]], axis=-1)
        rec[gone] = 0.0
        if sprinkle and N >= 8:
            g = np.nonzero(gone.reshape(-1))[0]
            if len(g) >= 2:                                   # two other ways of being missing: a NaN coordinate, a score of -0.0
                rec.reshape(N, 4)[g[0]] = [np.nan, 1.0, 1.0, 2.0]
                rec.reshape(N, 4)[g[1]] = [0.5, 0.25, 1.0, -0.0]
        out[name] = rec.astype(rec_dtype)
    for a in out.values():
        if isinstance(a, np.ndarray):
            a.setflags(write=False)
    return out


def refine_kwargs(cs):
    return dict(det_of=cs["det_of"], n_persons=cs["n_persons"], views=cs["views"], keypoint_score_threshold=cs["thr"])


@functools.lru_cache(maxsize=None)
def reference(rig_name, shape, sigma, start, sprinkle=True, rec_dtype="float64", kp_dtype="float64", placement="home", iters=4,
              score_weights=False):
    """refine_joints_reference on a case -> (out, cost, codes, views used [F,P,kn] uint32); read-only, computed once."""
    cs = case(rig_name, shape, sigma, sprinkle, rec_dtype, kp_dtype, placement)
    res = refine_joints_reference(cs["K"], cs["R"], cs["t"], cs[start], cs["kpts"], iters=iters, score_weights=score_weights,
                                  return_views=True, **refine_kwargs(cs))
    for a in res:
        a.setflags(write=False)
    return res


def behind_case(rig_name):
    """Four records of one frame whose joint 0 lies a decimetre BEHIND camera 0 (in front of the others); every camera holds a
    usable observation of every joint.  -> dict like case() (no det_of / n_persons / views), `behind`: the camera."""
    K, R, t = rig(rig_name)
    C = K.shape[0]
    rng = np.random.default_rng(_seed("behind", rig_name))
    X = synth.make_people(rng, 1, 1, J=4)
    X[0, 0, 0] = t[0] - 0.1 * R[0][:, 2] + 0.05 * R[0][:, 0]
    uv, depth = synth.project(K, R, t, X)
    assert depth[0, 0, 0, 0] < 0 and (depth[1:, 0, 0, 0] > 0).all() and (depth[:, 0, 0, 1:] > 0).all()
    kp = np.concatenate([np.moveaxis(uv, 0, 1) + rng.normal(0.0, 1.0, (1, C, 1, 4, 2)), np.ones((1, C, 1, 4, 1))], axis=-1)
    rec = np.concatenate([X + 0.004, np.ones((1, 1, 4, 1))], axis=-1)
    return dict(K=K, R=R, t=t, X=X, kpts=kp, dlt=rec, det_of=None, n_persons=None, views=None, thr=THRESHOLD, behind=0)


# ------------------------------------------------------------------------------------------------ the exact minimiser
def exact_minimum(K, R, t, obs, X0, tol="1e-30", max_steps=200):
    """Gauss-Newton on E(X) = sum_c w_c |proj_c(X) - (u_c, v_c)|^2 in DIGITS-digit arithmetic from the fp64 values of K, R, t and the
    observations obs = [(c, u, v, w), ...], started at X0, until |step| < tol -> (X [3] rounded once to fp64, E as float, steps)."""
    import mpmath as mp
    with mp.workdps(DIGITS):
        m = lambda a: mp.mpf(float(a))
        cams = []
        for c, u, v, w in obs:
            cams.append(([[m(R[c][k, i]) for k in range(3)] for i in range(3)], [m(a) for a in t[c]],
                         m(K[c][0, 0]), m(K[c][0, 1]), m(K[c][0, 2]), m(K[c][1, 1]), m(K[c][1, 2]), m(u), m(v), m(w)))
        X = [m(a) for a in X0]
        tol = mp.mpf(tol)
        for step in range(max_steps):
            H = mp.zeros(3, 3)
            g = mp.zeros(3, 1)
            E = mp.mpf(0)
            for Rt, tc, fx, s, cx, fy, cy, u, v, w in cams:
                d = [X[i] - tc[i] for i in range(3)]
                pc = [Rt[i][0] * d[0] + Rt[i][1] * d[1] + Rt[i][2] * d[2] for i in range(3)]
                x, y = pc[0] / pc[2], pc[1] / pc[2]
                ru, rv = fx * x + s * y + cx - u, fy * y + cy - v
                dx = [(Rt[0][k] - x * Rt[2][k]) / pc[2] for k in range(3)]
                dy = [(Rt[1][k] - y * Rt[2][k]) / pc[2] for k in range(3)]
                du = [fx * dx[k] + s * dy[k] for k in range(3)]
                dv = [fy * dy[k] for k in range(3)]
                E += w * (ru * ru + rv * rv)
                for a in range(3):
                    g[a] += w * (du[a] * ru + dv[a] * rv)
                    for b in range(3):
                        H[a, b] += w * (du[a] * du[b] + dv[a] * dv[b])
            dlt = mp.lu_solve(H, -g)
            X = [X[i] + dlt[i] for i in range(3)]
            if mp.sqrt(dlt[0] ** 2 + dlt[1] ** 2 + dlt[2] ** 2) < tol:
                break
        else:
            raise AssertionError("the exact Gauss-Newton iteration did not settle")
        return np.array([float(a) for a in X]), float(E), step + 1


@functools.lru_cache(maxsize=None)
def minimiser(rig_name, sigma, kp_dtype="float64", rec_dtype="float64", placement="home", shape=MINIMISER_SHAPE):
    """The exact minimiser of every record of case(rig, shape, sigma, sprinkle=True, ...) that the rule refines (its view set and
    weights are the rule's: the view set does not depend on the start on these cases, which the host test asserts)
    -> dict(X [F,P,kn,3] (NaN where the record is copied), E [F,P,kn], refined [F,P,kn] bool); read-only."""
    cs = case(rig_name, shape, sigma, True, rec_dtype, kp_dtype, placement)
    _, _, codes, used = reference(rig_name, shape, sigma, "dlt", True, rec_dtype, kp_dtype, placement)
    F, P, kn = shape
    kp = np.asarray(cs["kpts"]).astype(np.float64)
    Xm, Em = np.full((F, P, kn, 3), np.nan), np.full((F, P, kn), np.nan)
    refined = codes >= 2
    for f, p, j in zip(*np.nonzero(refined)):
        obs = []
        for c in range(cs["K"].shape[0]):
            if (int(used[f, p, j]) >> c) & 1:
                q = int(cs["det_of"][f, c, p])
                obs.append((c, kp[f, c, q, j, 0], kp[f, c, q, j, 1], 1.0))
        Xm[f, p, j], Em[f, p, j], _ = exact_minimum(cs["K"], cs["R"], cs["t"], obs, cs["X"][f, p, j])
    out = dict(X=Xm, E=Em, refined=refined)
    for a in out.values():
        a.setflags(write=False)
    return out


# ------------------------------------------------------------------------------------------------ the statistical recipe
@functools.lru_cache(maxsize=None)
def recipe(C, per_view_sigma=False, F=40, P=2, kn=133):
    """The recipe of the README's figures: the floor rig (C = 4) or synth.ring_rig(8), two persons on the 1.5 m circle, 10 640 joints,
    exact projections + N(0, sigma): sigma = 1 px, or per observation sigma = U(0.3, 3) px with the score 1 / sigma^2.
    -> dict(K, R, t, X, kpts float64, pair, dlt [F,P,kn,4], thr = 0)."""
    K, R, t = synth.load_rig_json() if C == 4 else synth.ring_rig(C)
    rng = np.random.default_rng(_seed("recipe", C, per_view_sigma))
    X = synth.make_people(rng, F, P, J=kn)
    uv = np.moveaxis(synth.project(K, R, t, X)[0], 0, 1)
    sig = rng.uniform(0.3, 3.0, (F, C, P, kn)) if per_view_sigma else np.ones((F, C, P, kn))
    uv = uv + sig[..., None] * rng.normal(0.0, 1.0, uv.shape)
    kp = np.concatenate([uv, (1.0 / sig ** 2)[..., None]], axis=-1)
    N = F * P * kn
    obs = np.moveaxis(kp, 1, 0).reshape(C, N, 3)
    pair, dlt = _starts(K, R, t, obs, np.ones((C, N), dtype=bool), X.reshape(N, 3))
    rec = lambda s: np.concatenate([s.reshape(F, P, kn, 3), np.ones((F, P, kn, 1))], axis=-1)
    return dict(K=K, R=R, t=t, X=X, kpts=kp, pair=rec(pair), dlt=rec(dlt), thr=0.0)
