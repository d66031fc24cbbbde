"""Cases for the one-to-one assignment (include/snowtri.h, "Assignment"; reproject.assign_detections_reference, k_assign).

  - three families of cost arrays (cost_sum, cost_n [n, 1, P, Pmax]): random floats, tie-laden integers, 30 % inadmissible pairs;
  - an exhaustive minimum over all partial one-to-one matchings, a scalar transcription of rule 3 (plain Python loops, one column at
    a time) and the augmented matrix scipy's linear_sum_assignment takes;
  - the packing problems: an easy one (one step per row) and a hard one (every row contested, long augmenting paths);
  - the synthetic recipe "crossing": three walkers of one build, two of them passing shoulder to shoulder along the optical axis of
    camera 0, so that their images cross there; and its measurement for match_detections against assign_detections.
Everything cached is read-only.
"""
import functools
import itertools
import zlib

import numpy as np

from snowmocap_amd import synth

GATE_PX = 6.0
GATE2 = 36.0
MIN_JOINTS = 8
FAMILIES = ("floats", "ties", "inadmissible")
SIZES = [(1, 1), (1, 5), (5, 1), (4, 4), (3, 5), (4, 5), (8, 8), (8, 9), (16, 16), (16, 17), (32, 32), (1, 63), (63, 1)]     # (P, Pmax)
COUNTS = (1, 7, 65, 257)
TIE_VALUES = (0.0, 12.0, 24.0, 36.0, 48.0)


def width(P, Pmax):
    """the sub-wave width k_assign is compiled for"""
    return next(w for w in (8, 16, 32, 64) if w >= P + Pmax)


def _seed(*parts):
    return zlib.crc32(repr(parts).encode())


@functools.lru_cache(maxsize=None)
def family(name, P, Pmax, n):
    """-> (cost_sum [n, 1, P, Pmax] float64, cost_n int32), for GATE_PX and MIN_JOINTS.
    floats: means U(0, 1.5 gate2) as sums over 8..40 joints.  ties: means from TIE_VALUES over 8 joints (sums and quotients exact).
    inadmissible: floats with 30 % of the pairs spoilt -- too few joints, a NaN sum, an infinite sum, no joint at all."""
    rng = np.random.default_rng(_seed(name, P, Pmax, n))
    shape = (n, 1, P, Pmax)
    if name == "ties":
        cn = np.full(shape, 8, dtype=np.int32)
        cs = rng.choice(TIE_VALUES, size=shape) * 8.0
    else:
        cn = rng.integers(MIN_JOINTS, 41, size=shape).astype(np.int32)
        cs = rng.uniform(0.0, 1.5 * GATE2, size=shape) * cn
        if name == "inadmissible":
            kind = rng.integers(0, 4, size=shape)
            bad = rng.random(shape) < 0.3
            cn = np.where(bad & (kind == 0), rng.integers(1, MIN_JOINTS, size=shape), cn).astype(np.int32)
            cs = np.where(bad & (kind == 1), np.nan, cs)
            cs = np.where(bad & (kind == 2), np.inf, cs)
            cn = np.where(bad & (kind == 3), 0, cn).astype(np.int32)
            cs = np.where(bad & (kind == 3), 0.0, cs)
    cs.setflags(write=False)
    cn.setflags(write=False)
    return cs, cn


@functools.lru_cache(maxsize=None)
def reference(name, P, Pmax, n):
    """assign_detections_reference on family(...) -> (det_of [n, 1, P], person_of [n, 1, Pmax], total [n, 1]); computed once."""
    from snowmocap_amd.reproject import assign_detections_reference
    out = assign_detections_reference(*family(name, P, Pmax, n), GATE_PX, MIN_JOINTS)
    for a in out:
        a.setflags(write=False)
    return out


def means(cost_sum, cost_n, gate2, min_joints):
    """rule 1 -> mean [.., P, Pmax], +inf where the pair is inadmissible"""
    with np.errstate(all="ignore"):
        m = np.asarray(cost_sum, dtype=np.float64) / np.asarray(cost_n).astype(np.float64)
        ok = (np.asarray(cost_n) >= min_joints) & ~np.isnan(m) & (m <= gate2) & (m > -np.inf)
    return np.where(ok, m, np.inf)


def augmented(mean, gate2):
    """rule 2 -> a [P, Pmax + P]"""
    P, Pmax = mean.shape
    a = np.full((P, Pmax + P), np.inf)
    a[:, :Pmax] = mean
    a[np.arange(P), Pmax + np.arange(P)] = gate2
    return a


def brute_force(mean, gate2):
    """The least total + gate2 * (unmatched persons) over ALL partial one-to-one matchings on admissible pairs (P, Pmax <= 5)."""
    P, Pmax = mean.shape
    best = np.inf
    for choice in itertools.product(range(-1, Pmax), repeat=P):
        taken = [q for q in choice if q >= 0]
        if len(taken) != len(set(taken)):
            continue
        cost = 0.0
        for p, q in enumerate(choice):
            cost += gate2 if q < 0 else mean[p, q]
        best = min(best, cost)
    return best


def scalar_rule(a, Pmax):
    """Rule 3 one column at a time, plain Python floats -> det_of [P] (a: the augmented matrix)."""
    P, m = a.shape
    inf = float("inf")
    u, v, row_of = [0.0] * P, [0.0] * m, [-1] * m
    for i in range(P):
        minv, way, used = [inf] * m, [-1] * m, [False] * m
        j0, i0 = -1, i
        while True:
            if j0 >= 0:
                used[j0] = True
            delta, j1 = inf, -1
            for j in range(m):
                if not used[j]:
                    cur = (float(a[i0, j]) - u[i0]) - v[j]
                    if cur < minv[j]:
                        minv[j], way[j] = cur, j0
                    if minv[j] < delta:
                        delta, j1 = minv[j], j
            u[i] += delta
            for j in range(m):
                if used[j]:
                    u[row_of[j]] += delta
                    v[j] -= delta
                else:
                    minv[j] -= delta
            j0 = j1
            if row_of[j0] < 0:
                break
            i0 = row_of[j0]
        while j0 >= 0:
            j1 = way[j0]
            row_of[j0] = row_of[j1] if j1 >= 0 else i
            j0 = j1
    det = [-1] * P
    for q in range(Pmax):
        if row_of[q] >= 0:
            det[row_of[q]] = q
    return np.array(det, dtype=np.int64)


# ------------------------------------------------------------------------------------------------ packing
def easy_problem(P, Pmax):
    """identity-like: person p fits detection p at 1 and every other at 30 -- each row ends its search in one step"""
    mean = np.full((P, Pmax), 30.0)
    mean[np.arange(min(P, Pmax)), np.arange(min(P, Pmax))] = 1.0
    return mean * 8.0, np.full((P, Pmax), 8, dtype=np.int32)


def hard_problem(P, Pmax):
    """mean[p][q] = (p + 1)(q + 1) / 2^k < gate2: every row likes column 0 best and the dearest rows come LAST, so each insertion
    takes column 0 and pushes every row before it one column along -- augmenting paths through the whole tree.  Exact in fp64."""
    scale = 1.0
    while P * Pmax * scale > 32.0:
        scale *= 0.5
    mean = (np.arange(P) + 1.0)[:, None] * (np.arange(Pmax) + 1.0)[None, :] * scale
    return mean * 8.0, np.full((P, Pmax), 8, dtype=np.int32)


# ------------------------------------------------------------------------------------------------ the recipe "crossing"
CROSS_F = 60
CROSS_GATE = 30.0           # px: wide enough for the recipe's whole-body shift (0.05 m is 8 px at 4.5 m, per axis)
CROSS_THRESHOLD = 0.5
CROSS_SIGMA_3D = 0.01       # m: the error of each joint of the 3D records handed to the matcher ...
CROSS_SHIFT_3D = 0.05       # ... and of the whole body of a person in a frame (what a wrong association or a nudged camera does)
CROSS_SIGMA_PX = 1.0


@functools.lru_cache(maxsize=None)
def crossing(C=4, F=CROSS_F):
    """The rig of reproject_cases.match_case(C, 3), synth.ring_rig(C) (camera 0 on the +x axis looking at the origin).  Three persons of ONE build (the same joint offsets):
    A walks along y = +0.2 from x = -0.3 to +0.3, B along y = -0.2 from x = +0.3 to -0.3 -- they pass shoulder to shoulder at the
    origin, and their images cross in the cameras on the y axis, one 0.4 m behind the other -- and C crosses the scene along
    x = -0.9 from y = -1.5 to +1.5, through both their images in the cameras on the x axis.  Detections: projections +
    N(0, CROSS_SIGMA_PX), scores U(3.5, 8), the list of every (f, c) permuted.  The 3D records the matcher is given: truth + a shift
    of the whole body N(0, CROSS_SHIFT_3D) per person and frame + N(0, CROSS_SIGMA_3D) per joint, score 1.
    -> dict(K, R, t, X [F, 3, J, 3], xyzs [F, 3, J, 4], kpts [F, C, 3, J, 3] float64, n_persons [F, C], det_true [F, C, 3])."""
    import reproject_cases
    mc = reproject_cases.match_case(C, 3)                   # its rig: synth.ring_rig(C)
    K, R, t = mc["K"], mc["R"], mc["t"]
    rng = np.random.default_rng(_seed("crossing", C, F))
    J = 133
    body = (rng.random((J, 3)) - np.array([0.5, 0.5, 0.0])) * np.array([0.5, 0.35, 1.8])
    s = np.linspace(-1.0, 1.0, F)
    centres = np.zeros((F, 3, 3))
    centres[:, 0, 0], centres[:, 0, 1] = 0.3 * s, 0.2
    centres[:, 1, 0], centres[:, 1, 1] = -0.3 * s, -0.2
    centres[:, 2, 0], centres[:, 2, 1] = -0.9, 1.5 * s
    X = centres[:, :, None, :] + body[None, None, :, :]
    uv, _ = synth.project(K, R, t, X)
    uv = np.moveaxis(uv, 0, 1) + rng.normal(0.0, CROSS_SIGMA_PX, (F, C, 3, J, 2))
    rec = np.concatenate([uv, rng.uniform(3.5, 8.0, (F, C, 3, J, 1))], axis=-1)
    perm = np.empty((F, C, 3), dtype=np.int64)
    kp = np.empty_like(rec)
    for f in range(F):
        for c in range(C):
            perm[f, c] = rng.permutation(3)
            kp[f, c] = rec[f, c, perm[f, c]]
    noisy = X + rng.normal(0.0, CROSS_SHIFT_3D, (F, 3, 1, 3)) + rng.normal(0.0, CROSS_SIGMA_3D, X.shape)
    xyzs = np.concatenate([noisy, np.ones(X.shape[:-1] + (1,))], axis=-1)
    out = dict(K=K, R=R, t=t, X=X, xyzs=xyzs, kpts=kp, n_persons=np.full((F, C), 3, dtype=np.int32), det_true=np.argsort(perm, axis=-1))
    for a in out.values():
        a.setflags(write=False)
    return out


def what_it_buys(cs, det_of, refine):
    """-> (share of (f, c, p) that are shared, share matched to the detection generated for them, RMS error in metres of
    refine(det_of) -> records against the truth)"""
    det_of = np.asarray(det_of)
    same = (det_of[..., :, None] == det_of[..., None, :]) & (det_of[..., :, None] >= 0)
    out = np.asarray(refine(det_of))
    rms = float(np.sqrt(((out[..., :3] - cs["X"]) ** 2).sum(axis=-1).mean()))
    return float((same.sum(axis=-1) > 1).mean()), float((det_of == cs["det_true"]).mean()), rms
