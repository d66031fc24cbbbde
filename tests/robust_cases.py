"""Inputs shared by tests/test_robust_host.py and tests/test_gpu_robust.py: the outlier recipe on the rigs of the robust
method's tests, and the reference rule's answers on them (computed once per process, never modified)."""
import functools

import numpy as np

from snowmocap_amd import synth
from snowmocap_amd.robust import triangulate_robust_reference

KTHR = 3.0
SETTINGS = ((6.0, 1), (6.0, 6), (2.5, 2), (float("inf"), 1), (6.0, 0))     # (reproj_threshold_px, max_drops)
RIGS = ("ring2", "ring3", "ring4", "floor", "ring5", "ring8")


@functools.lru_cache(maxsize=None)
def rig(name):
    return synth.load_rig_json() if name == "floor" else synth.ring_rig(int(name[4:]))


def _freeze(d):
    for v in d.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return d


@functools.lru_cache(maxsize=None)
def quality_batch(name):
    """The recipe of the issue: default_rng(5), 12 frames, 1 px of noise, scores U(2, 8), one camera shifted on 10 % of the joints."""
    K, R, t = rig(name)
    rng = np.random.default_rng(5)
    X = synth.make_people(rng, 12, 1)
    kp, _ = synth.make_keypoints(rng, K, R, t, X, pixel_sigma=1.0, score_range=(2.0, 8.0))
    kpo, cam = synth.add_outliers(rng, kp)
    return _freeze(dict(K=K, R=R, t=t, X=X, kpts=kpo, cam=cam))


@functools.lru_cache(maxsize=None)
def parity_batch(name, F=40, J=133, dtype="float32", fraction=0.1, seed=11):
    """The parity input: the outlier recipe, scores U(2, 8) against kthr = 3, and one camera that lists nobody in some frames."""
    K, R, t = rig(name)
    C = K.shape[0]
    rng = np.random.default_rng(seed + C)
    X = synth.make_people(rng, F, 1, J=J)
    kp, npers = synth.make_keypoints(rng, K, R, t, X, pixel_sigma=1.0, score_range=(2.0, 8.0), dtype=np.dtype(dtype))
    kpo, cam = synth.add_outliers(rng, kp, fraction=fraction)
    npers = npers.copy()
    npers[::3, (C - 1) // 2] = 0
    return _freeze(dict(K=K, R=R, t=t, X=X, kpts=kpo, cam=cam, n_persons=npers))


@functools.lru_cache(maxsize=None)
def divergence_batch(kind):
    """8 cameras, 3 frames of 133 joints (seven waves).  'one': exactly one joint of one frame has an outlier; 'all': every joint
    has one; 'mixed': neighbouring joints carry 0, 1 and 2 shifted cameras in turn (lanes of one wave need 0, 1 and 2 drops)."""
    K, R, t = rig("ring8")
    rng = np.random.default_rng(23)
    F, J = 3, 133
    X = synth.make_people(rng, F, 1)
    kp, npers = synth.make_keypoints(rng, K, R, t, X, pixel_sigma=1.0, score_range=(3.5, 8.0))
    kp = kp.copy()
    if kind == "one":
        kp[1, 5, 0, 77, 0] += 90.0
    elif kind == "all":
        kp, _ = synth.add_outliers(rng, kp, fraction=1.1)
    else:
        for f in range(F):
            for j in range(J):
                n = (f + j) % 3
                cams = rng.choice(8, size=n, replace=False)
                for k, c in enumerate(cams):
                    kp[f, c, 0, j, 0] += 60.0 + 25.0 * k
                    kp[f, c, 0, j, 1] -= 45.0
    return _freeze(dict(K=K, R=R, t=t, X=X, kpts=kp, n_persons=None))


FRAMES_RIGS = ("ring3", "ring8", "mixed8")      # (dlt_frames_cases.rig names; the rig with per-camera intrinsics at two placements)


def frames_placements(name):
    import dlt_frames_cases as fc
    return fc.MIXED_PLACEMENTS if name.startswith("mixed") else tuple(fc.PLACEMENTS)


@functools.lru_cache(maxsize=None)
def frames_batch(name, placement):
    """tests/test_gpu_dlt_frames.py: 3 frames of 133 joints, 0.5 px of noise, the outlier recipe, one camera that lists nobody in
    frame 1, two joints without two views -- generated ONCE at home (the same pixels at every placement); K, R and the rig and scene moved to `placement`."""
    import dlt_frames_cases as fc
    K, R, t = fc.rig(name)
    C = K.shape[0]
    rng = np.random.default_rng(41 + C)
    X = synth.make_people(rng, 3, 1)
    kp, npers = synth.make_keypoints(rng, K, R, t, X, pixel_sigma=0.5, score_range=(2.0, 8.0))
    kpo, cam = synth.add_outliers(rng, kp)
    npers = npers.copy()
    npers[1, (C - 1) // 2] = 0
    kpo[0, :, 0, 7, 2] = 0.5                          # a joint nobody sees, a joint one camera sees: the zero record
    kpo[2, 1:, 0, 9, 2] = 0.5
    tp, Xp, _, _ = fc.place(t, X, placement)
    return _freeze(dict(K=K, R=R, t=tp, X=Xp, kpts=kpo, cam=cam, n_persons=npers))


def batch(batch_key):
    if batch_key[0] == "parity":
        return parity_batch(*batch_key[1:])
    if batch_key[0] == "frames":
        return frames_batch(*batch_key[1:])
    return divergence_batch(batch_key[1])


@functools.lru_cache(maxsize=None)
def reference(batch_key, kn, tau, max_drops):
    """batch_key: ("parity", name, F, J, dtype), ("divergence", kind) or ("frames", name, placement)."""
    b = batch(batch_key)
    return _freeze(triangulate_robust_reference(b["K"], b["R"], b["t"], b["kpts"], b["n_persons"], KTHR, kn, tau, max_drops))


# every (batch, keypoint_num, settings) the GPU file compares with the reference -- the margin-cap test walks the same list
def gpu_cases():
    cases = []
    for name in RIGS:
        for tau, md in SETTINGS:
            cases.append((("parity", name, 40, 133, "float32"), 133, tau, md))
    for name in RIGS:
        for F in (1, 3):
            cases.append((("parity", name, F, 133, "float32"), 133, 6.0, 6))
        cases.append((("parity", name, 40, 133, "float64"), 133, 6.0, 6))
        for tau, md in ((6.0, 1), (2.5, 2)):
            cases.append((("parity", name, 40, 133, "float32"), 30, tau, md))
            cases.append((("parity", name, 40, 17, "float32"), 17, tau, md))
    for kind in ("one", "all", "mixed"):
        cases.append((("divergence", kind), 133, 6.0, 6))
    cases += frames_cases()
    return cases


# what tests/test_gpu_dlt_frames.py compares with the reference: every placement of every rig, tau 6, one and six drops
def frames_cases():
    return [(("frames", name, placement), 133, 6.0, md) for name in FRAMES_RIGS for placement in frames_placements(name) for md in (1, 6)]
