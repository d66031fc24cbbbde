"""Seeding: 3D persons from the detections nobody claimed -- THE RULE in NumPy, and the wrappers of the two kernels.

The matching chain (reprojection_cost, assign_detections, triangulate_matched, refine_joints) improves the persons the first
triangulation found.  assign_detections' person_of[f, c, q] == -1 marks a detection no person took: a candidate for a person the
triangulation missed.  Two steps turn them into persons (include/snowtri.h, "Seeding", states both for the C ABI):

  pair_cost      per camera pair (a < b, the reference's loop order), detection q of a and r of b: the squared distance between the
                 two LINES of every joint that counts, summed -> pair_sum, pair_n [F, NP, Pmax, Pmax]   (k_pair_cost)
  seed_persons   per frame the free detections are nodes, the mean pair costs inside the gate are edges; the cheapest edge starts
                 a set, the set grows by the node whose largest edge to it is smallest while it stays a CLIQUE over different
                 cameras, and a set of at least min_views members is a seed -> seed_det_of [F, C, S], n_seeds [F]   (k_seed_group)

seed_det_of has the layout and meaning of det_of, so triangulate_matched takes it unchanged: `triangulate_seeded` is the chain.
With claimed=None every detection is free and the chain is an association of its own, in ray space: `seeded_triangulator` hands it
to pose.refine_rig as its triangulation step.

`pair_cost_reference` and `seed_persons_reference` are what the kernels are tested against; they are not on the product path.

Left out on purpose: more than 8 cameras, C * Pmax > 64, seeding across time (a seed knows nothing of the frame before it),
ShardedTrackPipeline.
"""
from __future__ import annotations

import numpy as np

MAX_CAMERAS = 8
MAX_JOINTS = 256
MAX_NODES = 64
MAX_GATE = 1e150
FLAG_FULL = 1


def camera_pairs(C):
    """The camera pairs (a < b) in the reference's loop order -> [NP, 2]."""
    return np.array([(a, b) for a in range(C - 1) for b in range(a + 1, C)], dtype=np.int64).reshape(-1, 2)


def cameras_of_pairs(NP):
    """C with C (C - 1) / 2 == NP."""
    C = int(round((1 + (1 + 8 * int(NP)) ** 0.5) / 2))
    if C < 2 or C * (C - 1) // 2 != int(NP):
        raise ValueError(f"pair_sum has {NP} camera pairs, which is C (C - 1) / 2 for no C >= 2")
    return C


def free_nodes(F, C, Pmax, n_persons, claimed):
    """Rule 1 -> free [F, C, Pmax] bool: q < n_persons[f, c] and claimed[f, c, q] < 0 (None: Pmax everywhere, nothing claimed)."""
    q = np.arange(Pmax)
    free = np.ones((F, C, Pmax), dtype=bool) if n_persons is None else q[None, None, :] < np.asarray(n_persons).reshape(F, C)[:, :, None]
    if claimed is not None:
        claimed = np.asarray(claimed)
        if claimed.shape != (F, C, Pmax):
            raise ValueError(f"claimed must be [F={F}, C={C}, Pmax={Pmax}] (got shape {claimed.shape})")
        free = free & (claimed < 0)
    return free


def _check_kpts(kpts, C=None):
    kpts = np.asarray(kpts)
    if kpts.ndim != 5 or kpts.shape[-1] != 3 or kpts.shape[2] < 1 or kpts.shape[3] < 1:
        raise ValueError(f"kpts must be [F, C, Pmax >= 1, kn >= 1, 3] (got shape {kpts.shape})")
    if C is not None and kpts.shape[1] != C:
        raise ValueError(f"kpts must be [F, C={C}, Pmax, kn, 3] (got shape {kpts.shape})")
    if not 2 <= kpts.shape[1] <= MAX_CAMERAS:
        raise ValueError("the pair cost takes 2 to 8 cameras")
    if kpts.shape[3] > MAX_JOINTS:
        raise ValueError("kn must not exceed 256 joints")
    return kpts


def pair_cost_reference(K, R, t, kpts, n_persons=None, claimed=None, keypoint_score_threshold=0.0, M=None):
    """Rules 1-5 of the pair cost in NumPy, fp64: kpts [F, C, Pmax, kn, 3] (float32 or float64), n_persons [F, C] or None, claimed
    [F, C, Pmax] or None -> (pair_sum [F, NP, Pmax, Pmax] float64, pair_n int32).  M [C, 3, 3]: the ray matrices to use instead of
    R K^-1 (Context.ray_matrices)."""
    thr = float(keypoint_score_threshold)
    if thr != thr:
        raise ValueError("keypoint_score_threshold is NaN")
    K, R, t = np.asarray(K, dtype=np.float64), np.asarray(R, dtype=np.float64), np.asarray(t, dtype=np.float64)
    C = R.shape[0]
    kpts = _check_kpts(kpts, C)
    F, _, Pmax, kn, _ = kpts.shape
    if M is None:
        M = np.stack([R[c] @ np.linalg.inv(K[c]) for c in range(C)])
    kp = kpts.astype(np.float64)
    free = free_nodes(F, C, Pmax, n_persons, claimed)
    with np.errstate(all="ignore"):
        u, v = kp[..., 0], kp[..., 1]
        h = M[None, :, None, None, :, 0] * u[..., None] + M[None, :, None, None, :, 1] * v[..., None] + M[None, :, None, None, :, 2]
        ok = ~(kp[..., 2] < thr) & np.isfinite(u) & np.isfinite(v) & free[..., None]              # [F, C, Pmax, kn]
        pairs = camera_pairs(C)
        pair_sum = np.zeros((F, len(pairs), Pmax, Pmax))
        pair_n = np.zeros((F, len(pairs), Pmax, Pmax), dtype=np.int32)
        for k, (a, b) in enumerate(pairs):
            ha, hb = h[:, a, :, None], h[:, b, None, :]                                           # [F, Pmax, 1, kn, 3], [F, 1, Pmax, kn, 3]
            n = np.cross(ha, hb)
            nn = (n * n).sum(axis=-1)
            w = (n * (t[b] - t[a])).sum(axis=-1)
            d2 = w * w / nn
            counts = ok[:, a, :, None] & ok[:, b, None, :] & (nn > 0) & np.isfinite(d2)
            pair_n[:, k] = counts.sum(axis=-1)
            pair_sum[:, k] = np.where(counts, d2, 0.0).sum(axis=-1)
    return pair_sum, pair_n


def seed_args(gate, min_joints, min_views, S, C, Pmax):
    """The checks seed_persons and its reference share, in the words of the C entry -> (gate, min_joints, min_views, S)."""
    if int(min_joints) != min_joints or int(min_joints) < 1:
        raise ValueError("min_joints must be >= 1")
    if not float(gate) >= 0.0:
        raise ValueError("gate must be >= 0 and not NaN")
    if not float(gate) <= MAX_GATE:
        raise ValueError("gate must not exceed 1e150 (the means are compared with gate * gate, which must stay finite)")
    if C * Pmax > MAX_NODES:
        raise ValueError("C * Pmax must not exceed 64 (the nodes of a frame are the lanes of one wave)")
    if int(min_views) != min_views or not 2 <= int(min_views) <= C:
        raise ValueError(f"min_views must lie in 2..C (C = {C})")
    if S is None:
        S = max(1, min(64, C * Pmax // int(min_views)))
    if int(S) != S or not 1 <= int(S) <= 64:
        raise ValueError("S must lie in 1..64")
    return float(gate), int(min_joints), int(min_views), int(S)


def edge_weights(pair_sum, pair_n, gate2, min_joints, C, Pmax):
    """Rule 2 of one frame: pair_sum, pair_n [NP, Pmax, Pmax] -> W [N, N] float64, symmetric, +inf where there is no admissible edge."""
    N = C * Pmax
    W = np.full((N, N), np.inf)
    with np.errstate(all="ignore"):
        mean = np.asarray(pair_sum, dtype=np.float64) / np.asarray(pair_n).astype(np.float64)
        ok = (np.asarray(pair_n) >= min_joints) & ~np.isnan(mean) & (mean <= gate2)
    mean = np.where(ok, mean, np.inf)
    for k, (a, b) in enumerate(camera_pairs(C)):
        W[a * Pmax:(a + 1) * Pmax, b * Pmax:(b + 1) * Pmax] = mean[k]
        W[b * Pmax:(b + 1) * Pmax, a * Pmax:(a + 1) * Pmax] = mean[k].T
    return W


def _seed_frame(W, free, C, Pmax, min_views, S):
    """Rules 3-7 on one frame's weights (W is changed: rejected edges become +inf) -> (det [C, S], n_seeds, full)."""
    N = C * Pmax
    inf = np.inf
    free = free.copy()
    det = np.full((C, S), -1, dtype=np.int32)
    ns, full = 0, False
    upper = np.triu(np.ones((N, N), dtype=bool), 1)
    while True:
        both = free[:, None] & free[None, :] & upper
        cand = np.where(both, W, inf)
        flat = int(np.argmin(cand))                               # the FIRST least element of the row-major scan: the lowest (x, y)
        x, y = divmod(flat, N)
        if not cand[x, y] < inf:
            break
        if ns >= S:
            full = True
            break
        members, cams = [x, y], {x // Pmax, y // Pmax}
        while True:
            best, bz = inf, -1
            for z in range(N):
                if not free[z] or z in members or z // Pmax in cams:
                    continue
                worst = max(W[z, m] for m in members)             # +inf as soon as one edge is missing
                if worst < best:                                   # strict: ties to the lowest node
                    best, bz = worst, z
            if bz < 0:
                break
            members.append(bz)
            cams.add(bz // Pmax)
        if len(members) < min_views:
            W[x, y] = W[y, x] = inf
            continue
        for m in members:
            det[m // Pmax, ns] = m % Pmax
            free[m] = False
        ns += 1
    return det, ns, full


def seed_persons_reference(pair_sum, pair_n, n_persons=None, claimed=None, S=None, gate=0.05, min_joints=8, min_views=3):
    """The grouping rule of include/snowtri.h ("Seeding") in NumPy: pair_sum, pair_n [F, NP, Pmax, Pmax], n_persons [F, C] or None,
    claimed [F, C, Pmax] or None -> (seed_det_of [F, C, S] int32, n_seeds [F] int32, flags [F] uint32).  After the one division of
    rule 2 there are only comparisons: k_seed_group returns the same bits."""
    pair_sum, pair_n = np.asarray(pair_sum), np.asarray(pair_n)
    if pair_sum.ndim != 4 or pair_sum.shape != pair_n.shape or pair_sum.shape[2] != pair_sum.shape[3] or pair_sum.shape[2] < 1:
        raise ValueError("pair_sum and pair_n must both be [F, NP, Pmax, Pmax]")
    F, NP, Pmax, _ = pair_sum.shape
    C = cameras_of_pairs(NP)
    gate, min_joints, min_views, S = seed_args(gate, min_joints, min_views, S, C, Pmax)
    gate2 = gate * gate
    free = free_nodes(F, C, Pmax, n_persons, claimed).reshape(F, C * Pmax)
    seed_det_of = np.full((F, C, S), -1, dtype=np.int32)
    n_seeds = np.zeros(F, dtype=np.int32)
    flags = np.zeros(F, dtype=np.uint32)
    for f in range(F):
        W = edge_weights(pair_sum[f], pair_n[f], gate2, min_joints, C, Pmax)
        seed_det_of[f], n_seeds[f], full = _seed_frame(W, free[f], C, Pmax, min_views, S)
        flags[f] = FLAG_FULL if full else 0
    return seed_det_of, n_seeds, flags


def pair_cost(ctx, kpts, n_persons=None, claimed=None, keypoint_score_threshold=0.0, stream=None):
    """k_pair_cost through the context of the rig (_lib.Context): Context.pair_cost."""
    return ctx.pair_cost(kpts, n_persons=n_persons, claimed=claimed, keypoint_score_threshold=keypoint_score_threshold, stream=stream)


def seed_persons(ctx, pair_sum, pair_n, n_persons=None, claimed=None, S=None, gate=0.05, min_joints=8, min_views=3, with_flags=False,
                 stream=None):
    """k_seed_group through a context of the rig's camera count: Context.seed_persons.  The arguments are checked before the library
    is asked, in the words of seed_persons_reference."""
    if len(pair_sum.shape) != 4 or tuple(pair_sum.shape) != tuple(pair_n.shape) or int(pair_sum.shape[2]) != int(pair_sum.shape[3]):
        raise ValueError("pair_sum and pair_n must both be [F, NP, Pmax, Pmax]")
    C = cameras_of_pairs(int(pair_sum.shape[1]))
    gate, min_joints, min_views, S = seed_args(gate, min_joints, min_views, S, C, int(pair_sum.shape[2]))
    return ctx.seed_persons(pair_sum, pair_n, n_persons=n_persons, claimed=claimed, S=S, gate=gate, min_joints=min_joints, min_views=min_views,
                            with_flags=with_flags, stream=stream)


def triangulate_seeded(ctx, kpts, n_persons=None, claimed=None, S=None, gate=0.05, min_views=3, min_joints=8, keypoint_score_threshold=0.0,
                       reproj_threshold_px=6.0, max_drops=1, diagnostics=False, dtype=None, stream=None):
    """pair_cost -> seed_persons -> triangulate_matched(det_of=seed_det_of) through the context of the rig, device-resident when the
    arrays are CUDA tensors: kpts [F, C, Pmax, kn, 3] on the undistorted frame, n_persons [F, C] or None, claimed [F, C, Pmax] or None
    (assign_detections' person_of; None: every detection is free) ->
    dict(xyzs [F, S, kn, 4], pscore [F, S], n_seeds [F], seed_det_of [F, C, S], flags [F]; diagnostics=True: views, resid [F, S, kn]).
    A slot at or behind n_seeds[f] holds zero records: its det_of is -1 in every camera."""
    C, Pmax = int(kpts.shape[1]), int(kpts.shape[2])
    gate, min_joints, min_views, S = seed_args(gate, min_joints, min_views, S, C, Pmax)
    thr = float(keypoint_score_threshold)
    ps, pn = ctx.pair_cost(kpts, n_persons=n_persons, claimed=claimed, keypoint_score_threshold=thr, stream=stream)
    det, ns, flags = ctx.seed_persons(ps, pn, n_persons=n_persons, claimed=claimed, S=S, gate=gate, min_joints=min_joints, min_views=min_views,
                                      with_flags=True, stream=stream)
    tri = ctx.triangulate_matched(kpts, det_of=det, n_persons=n_persons, keypoint_score_threshold=thr, reproj_threshold_px=reproj_threshold_px,
                                  max_drops=max_drops, dtype=dtype, diagnostics=diagnostics, stream=stream)
    out = dict(xyzs=tri[0], pscore=tri[1], n_seeds=ns, seed_det_of=det, flags=flags)
    if diagnostics:
        out["views"], out["resid"] = tri[2], tri[3]
    return out


def triangulate_seeded_reference(K, R, t, kpts, n_persons=None, claimed=None, S=None, gate=0.05, min_views=3, min_joints=8,
                                 keypoint_score_threshold=0.0, reproj_threshold_px=6.0, max_drops=1):
    """The same chain by the NumPy rules (pair_cost_reference, seed_persons_reference, matched.triangulate_matched_reference) ->
    dict(xyzs, pscore, n_seeds, seed_det_of, flags, views, resid)."""
    from .matched import triangulate_matched_reference
    kpts = _check_kpts(kpts)
    thr = float(keypoint_score_threshold)
    ps, pn = pair_cost_reference(K, R, t, kpts, n_persons, claimed, thr)
    det, ns, flags = seed_persons_reference(ps, pn, n_persons, claimed, S, gate, min_joints, min_views)
    tri = triangulate_matched_reference(K, R, t, kpts, det, n_persons, thr, reproj_threshold_px, max_drops)
    return dict(xyzs=tri["xyzs"], pscore=tri["pscore"], n_seeds=ns, seed_det_of=det, flags=flags, views=tri["views"], resid=tri["resid"])


def seeded_triangulator(P, gate=0.05, min_views=3, min_joints=8, keypoint_score_threshold=0.0, reproj_threshold_px=6.0, max_drops=1,
                        reference=False, device=0):
    """-> triangulate(K, R, t, kpts, n_persons) -> xyzs [F, P, kn, 4] float64, the triangulation step pose.refine_rig accepts: every
    detection free, P seed slots, the library path on a context of the rig it is handed (reference=True: the NumPy rules, no GPU)."""
    kw = dict(S=int(P), gate=gate, min_views=min_views, min_joints=min_joints, keypoint_score_threshold=keypoint_score_threshold,
              reproj_threshold_px=reproj_threshold_px, max_drops=max_drops)

    def triangulate(K, R, t, kpts, n_persons=None):
        if reference:
            return triangulate_seeded_reference(K, R, t, kpts, n_persons, **kw)["xyzs"]
        from . import _lib
        ctx = _lib.Context(K, R, t, device=device)
        try:
            return np.asarray(triangulate_seeded(ctx, _lib.host_floats(kpts), n_persons, dtype=np.float64, **kw)["xyzs"], dtype=np.float64)
        finally:
            ctx.close()

    return triangulate


def seed_option(seed):
    """The seed= option of TrackPipeline.run: None (off) or gate or (gate[, min_views = 3[, min_joints = 8]]) ->
    None or (gate, min_views, min_joints)."""
    if seed is None:
        return None
    v = tuple(seed) if isinstance(seed, (tuple, list)) else (seed,)
    if not 1 <= len(v) <= 3 or isinstance(v[0], bool):
        raise ValueError(f"seed must be None, gate or (gate, min_views, min_joints) (got {seed!r})")
    v = v + (3, 8)[len(v) - 1:]
    if not float(v[0]) >= 0.0 or not float(v[0]) <= MAX_GATE or int(v[1]) != v[1] or int(v[2]) != v[2] or int(v[1]) < 2 or int(v[2]) < 1:
        raise ValueError(f"seed: gate must lie in 0..1e150, min_views must be an integer >= 2 and min_joints one >= 1 (got {seed!r})")
    return float(v[0]), int(v[1]), int(v[2])


__all__ = ["pair_cost", "pair_cost_reference", "seed_persons", "seed_persons_reference", "triangulate_seeded", "triangulate_seeded_reference",
           "seeded_triangulator", "seed_option", "camera_pairs", "edge_weights", "free_nodes"]
