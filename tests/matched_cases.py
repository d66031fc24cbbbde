"""Inputs shared by tests/test_matched_host.py and tests/test_gpu_matched.py: single-person batches of the robust method's tests
woven into multi-person detections lists, and the NumPy rule's answers on them (computed once per process, never modified)."""
import functools

import numpy as np

import robust_cases as rc
from assign_cases import crossing  # noqa: F401  (the recipe of the issue: 60 frames, 4 cameras, 3 persons, 133 joints)
from snowmocap_amd.matched import triangulate_matched_reference

KTHR = rc.KTHR


def _freeze(d):
    for v in d.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return d


def _weave(singles, Pmax, seed):
    """singles: P batches with kpts [F, C, 1, J, 3] and n_persons [F, C] or None on ONE rig -> person p sits at a seeded permuted
    position of every (f, c) list of length Pmax >= P; the other positions hold a decoy detection; a camera that lists nobody for
    person p (its batch's n_persons == 0) names a position at or behind n_persons, or -1."""
    P = len(singles)
    F, C, _, J, _ = singles[0]["kpts"].shape
    assert Pmax >= P
    rng = np.random.default_rng(seed)
    dtype = singles[0]["kpts"].dtype
    kpts = np.empty((F, C, Pmax, J, 3), dtype=dtype)
    kpts[..., 0] = rng.uniform(100.0, 1100.0, (F, C, Pmax, J))           # decoys: pixels anywhere, scores above the gate
    kpts[..., 1] = rng.uniform(100.0, 600.0, (F, C, Pmax, J))
    kpts[..., 2] = rng.uniform(3.5, 8.0, (F, C, Pmax, J))
    det_of = np.empty((F, C, P), dtype=np.int32)
    for f in range(F):
        for c in range(C):
            pos = rng.permutation(Pmax)[:P]
            det_of[f, c] = pos
            for p in range(P):
                kpts[f, c, pos[p]] = singles[p]["kpts"][f, c, 0]
    n_persons = np.full((F, C), Pmax, dtype=np.int32)
    for p in range(P):
        if singles[p]["n_persons"] is not None:
            det_of[..., p] = np.where(singles[p]["n_persons"] > 0, det_of[..., p], -1)
    return kpts, det_of, n_persons


@functools.lru_cache(maxsize=None)
def woven(name, P, Pmax, F=40, J=133, dtype="float32", fraction=0.1):
    """P batches robust_cases.parity_batch(name, seed=11 + p) woven -> dict(K, R, t, kpts, det_of, n_persons, singles)."""
    singles = [rc.parity_batch(name, F, J, dtype, fraction, 11 + p) for p in range(P)]
    kpts, det_of, n_persons = _weave(singles, Pmax, 1000 + 10 * P + Pmax)
    b = singles[0]
    return _freeze(dict(K=b["K"], R=b["R"], t=b["t"], kpts=kpts, det_of=det_of, n_persons=n_persons)) | dict(singles=tuple(singles))


@functools.lru_cache(maxsize=None)
def woven_divergence():
    """robust_cases.divergence_batch 'one', 'all' and 'mixed' as three persons of one 8-camera scene (Pmax = 4): persons that share
    a wave need 0, 1 and 2 drops side by side."""
    singles = [rc.divergence_batch(k) for k in ("one", "all", "mixed")]
    kpts, det_of, n_persons = _weave(singles, 4, 77)
    b = singles[0]
    return _freeze(dict(K=b["K"], R=b["R"], t=b["t"], kpts=kpts, det_of=det_of, n_persons=n_persons)) | dict(singles=tuple(singles))


def single_listed(single):
    """the n_persons a single-person batch hands to the robust rule, as int32 [F, C]"""
    F, C = single["kpts"].shape[:2]
    return np.ones((F, C), dtype=np.int32) if single["n_persons"] is None else (np.asarray(single["n_persons"]) > 0).astype(np.int32)


@functools.lru_cache(maxsize=None)
def reference(key, tau, max_drops):
    """key: ("woven", name, P, Pmax, F, J, dtype), ("divergence",) or ("crossing", which det_of) -> the NumPy rule's answer."""
    b, det_of, thr = case(key)
    return _freeze(triangulate_matched_reference(b["K"], b["R"], b["t"], b["kpts"], det_of, b["n_persons"], thr, tau, max_drops))


def case(key):
    """-> (batch, det_of, keypoint_score_threshold)"""
    if key[0] == "woven":
        b = woven(*key[1:])
        return b, b["det_of"], KTHR
    if key[0] == "divergence":
        b = woven_divergence()
        return b, b["det_of"], KTHR
    b = crossing()
    return b, crossing_det_of(key[1]), 0.5


@functools.lru_cache(maxsize=None)
def crossing_det_of(which):
    """det_true, or the det_of of assign_detections_reference on the handed-in records (gate and threshold of assign_cases)."""
    import assign_cases as ac
    from snowmocap_amd.reproject import assign_detections_reference, reprojection_cost_reference
    cs = crossing()
    if which == "true":
        return cs["det_true"]
    cost_sum, cost_n = reprojection_cost_reference(cs["K"], cs["R"], cs["t"], cs["xyzs"], cs["kpts"], n_persons=cs["n_persons"],
                                                   keypoint_score_threshold=ac.CROSS_THRESHOLD)
    det = np.ascontiguousarray(assign_detections_reference(cost_sum, cost_n, ac.CROSS_GATE)[0])
    det.setflags(write=False)
    return det


def rms_error(xyzs, X):
    return float(np.sqrt(((np.asarray(xyzs)[..., :3] - X) ** 2).sum(axis=-1).mean()))
