"""Inputs, exact results and the comparison routine shared by tests/test_skew_exact_host.py and tests/test_gpu_skew_exact.py: the
default (skew-ray) method on general rigs, held to oracle/skew_exact.py (the rule in 50-digit arithmetic).

Rigs       ring<C> / mixed<C> (tests/dlt_frames_cases.py), the floor rig, and rolled<C>: every camera rolled about its axis by its
           own angle (-180 .. 180 degrees), its own K with a skew term, heights 1.2-3.5 m and distances 2.5-7 m from the subject.
Placements the six of dlt_frames_cases.PLACEMENTS through place / place_params (mixed: MIXED_PLACEMENTS): the same pixels everywhere;
           condense_score_tol scales by 1 / u as average_score_threshold does (place_params below).
Scenes     single(): one detection per camera, J = 133 or less, 0.7 px noise, confidences on both sides of the keypoint gate, a
           joint nobody scores, a joint one camera alone scores, a camera that lists nobody;
           multi(): P boxed people, lists permuted per camera, a ragged list, an empty list, a person one camera missed (its
           confidences zero), a joint nobody scores; thresholds "tight" (average_score_threshold and condense_score_tol inside the
           spread of the exact means: true candidates and persons on both sides), "clean" (every true candidate kept, every wrong
           pairing dropped: complete clusters), "band" (thresholds 1e-7 from a decision of the exact rule) and "ghosts" (every candidate kept, a
           condense_distance_tol at which some wrong pairings join a person's cluster and others form their own, Pout_max below the
           person count).
Thresholds distance_threshold sits near the median exact pair distance of the scene (measured once with the exact rule, then
           written here as a round number); none is derived from a kernel's output.
"""
import functools

import numpy as np

import dlt_frames_cases as fc
from snowmocap_amd import synth

KTHR = 3.0                 # (a float32 value: the gate is the same comparison in either keypoint type)
NOISE = 0.7
XYZ_F32 = 2e-6             # x s / 4.5 (+ one float32 ulp of the value)
XYZ_F64 = 2.5e-10          # x s
MARGIN_MIN = 1e-9          # the well-posedness condition: no decision of the exact rule closer to its threshold than this


# ------------------------------------------------------------------------------------------------------------------------ rigs
def rolled_rig(C, seed=4242, with_rolls=False):
    """C cameras around the subject at their own distance (2.5-7 m) and height (1.2-3.5 m), each rolled about its optical axis by its
    own angle, the angles spread over -180 .. 180 degrees, each with its own K (fx 500-1500, fy 3 % off, skew, off-centre
    principal point).  (tests/test_lean_item_algebra.py::_random_rig with the roll made explicit.)"""
    rng = np.random.default_rng(seed + C)
    K, R, t = np.zeros((C, 3, 3)), np.zeros((C, 3, 3)), np.zeros((C, 3))
    rolls = np.deg2rad(rng.permutation(np.linspace(-180.0, 180.0, C, endpoint=False) + 180.0 / C))
    dist = rng.permutation(np.linspace(2.5, 7.0, C))
    hgt = rng.permutation(np.linspace(1.2, 3.5, C))
    for c in range(C):
        ang = 2.0 * np.pi * (c + rng.uniform(-0.2, 0.2)) / C
        t[c] = [dist[c] * np.cos(ang), dist[c] * np.sin(ang), hgt[c]]
        z = np.array([0.0, 0.0, 1.0]) + rng.uniform(-0.2, 0.2, 3) - t[c]
        z /= np.linalg.norm(z)
        x = np.cross(z, [0.0, 0.0, 1.0])
        x /= np.linalg.norm(x)
        y = np.cross(z, x)
        cr, sr = np.cos(rolls[c]), np.sin(rolls[c])
        R[c] = np.stack([cr * x + sr * y, -sr * x + cr * y, z], axis=1)
        fx = rng.uniform(500.0, 1500.0)
        K[c] = [[fx, rng.uniform(0.5, 2.0) * (-1) ** c, 640.0 + rng.uniform(-120, 120)], [0.0, 1.03 * fx, 360.0 + rng.uniform(-80, 80)],
                [0.0, 0.0, 1.0]]
    return (K, R, t, rolls) if with_rolls else (K, R, t)


def rig(name):
    """-> K, R, t of "ring<C>", "mixed<C>", "rolled<C>" or "floor", the camera centres moved onto a grid of 2^-20 m (under a micrometre):
    t + D and u (t + D) of dlt_frames_cases.place are then EXACT in float64 at all six placements, so every placement holds the
    same rig to the last bit and the exact rule is equivariant to its working precision, not to an ulp of a kilometre."""
    if name == "floor":
        K, R, t = synth.load_rig_json()
    elif name.startswith("rolled"):
        K, R, t = rolled_rig(int(name[6:]))
    else:
        K, R, t = fc.rig(name)
    return K, R, np.round(t * 2.0 ** 20) / 2.0 ** 20


def place_params(prm, placement):
    """dlt_frames_cases.place_params, and condense_score_tol / u: under this method a person's mean score is a mean of
    confidence / (1000 x a distance in world units) like a candidate's (under DLT it is a mean confidence and does not scale)."""
    out = fc.place_params(prm, placement)
    out["condense_score_tol"] = out["condense_score_tol"] / fc.PLACEMENTS[placement][0]
    return out


def placements(rig_name):
    return fc.MIXED_PLACEMENTS if rig_name.startswith("mixed") else tuple(fc.PLACEMENTS)


def subtract_scale(t):
    """L of the score bound: the largest magnitude the rule subtracts at a placement, max |t_c| + the rig diameter."""
    t = np.asarray(t, float).reshape(-1, 3)
    return float(np.linalg.norm(t, axis=1).max() + max(np.linalg.norm(a - b) for a in t for b in t))


# ---------------------------------------------------------------------------------------------------------------------- scenes
def single(rig_name, F, J, in_dtype, seed):
    K, R, t = rig(rig_name)
    C = K.shape[0]
    rng = np.random.default_rng(seed)
    X = synth.make_people(rng, F, 1, J=J, centres=np.array([[0.3, 0.9, 0.0]]))
    kp, npers = synth.make_keypoints(rng, K, R, t, X, pixel_sigma=NOISE, score_range=(2.0, 8.0), dtype=in_dtype)
    kp, npers = kp.copy(), npers.copy()
    kp[0, :, 0, 1, 2] = 0.5                          # a joint nobody scores
    kp[F - 1, 1:, 0, 3, 2] = 0.5                     # a joint one camera alone scores
    if C > 2:
        npers[F - 1, 1] = 0                          # a camera that lists nobody
        kp[F - 1, 1] = 0
    return dict(K=K, R=R, t=t, X=X, kpts=kp, n_persons=npers, dead=[(0, 0, 1), (F - 1, 0, 3)])


def multi(rig_name, P, F, J, in_dtype, seed):
    K, R, t = rig(rig_name)
    C = K.shape[0]
    rng = np.random.default_rng(seed)
    X = synth.make_people(rng, F, P, J=J)
    kp, npers = synth.make_keypoints(rng, K, R, t, X, pixel_sigma=NOISE, score_range=(2.5, 8.0), permute_persons=True, dtype=in_dtype)
    kp, npers = kp.copy(), npers.copy()
    kp[0, :, :, 5, 2] = 1.0                          # a joint nobody scores
    npers[1, 0] = P - 1                              # a ragged list
    kp[1, 0, P - 1:] = 0
    if F > 2:
        npers[2, C - 1] = 0                          # an empty list
        kp[2, C - 1] = 0
    kp[F - 1, 1, 0, :, 2] = 0.0                      # a person one camera missed: listed, every confidence zero
    return dict(K=K, R=R, t=t, X=X, kpts=kp, n_persons=npers, dead=[])


# ----------------------------------------------------------------------------------------------------------------------- cases
# name -> (kind, rig, P, F, J, keypoint dtype, seed, thresholds, Pout_max)
def _prm(J, **kw):
    out = dict(keypoint_score_threshold=KTHR, average_score_threshold=0.0, distance_threshold=0.004, condense_distance_tol=0.3,
               condense_person_num_tol=0, condense_score_tol=0.0, center_point_index=0, keypoint_num=J)
    out.update(kw)
    return out


TIGHT = dict(average_score_threshold=1.0, distance_threshold=0.006, condense_person_num_tol=2, condense_distance_tol=0.25)
CLEAN = dict(average_score_threshold=0.1, distance_threshold=0.006, condense_person_num_tol=2, condense_distance_tol=0.25)
# "band": the thresholds of "tight" moved next to a decision of the EXACT rule (figures of oracle/skew_exact.py on m-rolled3-tight at
# home): average_score_threshold 1e-7 below the smallest kept candidate mean (1.04176025224...: still kept), condense_score_tol 1e-7
# above a kept person's mean (2.03937935764...: now dropped).  Well posed for the rule (margin 1e-7 >= 1e-9), inside the 1e-6 band
# in which the streaming association does not trust its fast sums: the frame goes to k_candidate_sums_exact / k_frame_recompute.
BAND = dict(average_score_threshold=1.0417601480640406, condense_score_tol=2.039379561582069, distance_threshold=0.006,
            condense_person_num_tol=2, condense_distance_tol=0.25)
GHOSTS = dict(average_score_threshold=0.0, distance_threshold=0.006, condense_score_tol=0.02, condense_person_num_tol=0, condense_distance_tol=0.6)

CASES = {
    # one detection per camera, the Wholebody skeleton: the lean kernels (float32 outputs; float64 from five cameras on),
    # k_fused_single<C,0> (three and four cameras with float64 outputs), the general kernels (two cameras)
    "s-ring4": ("single", "ring4", 1, 3, 133, np.float32, 11, _prm(133), 1),
    "s-rolled4": ("single", "rolled4", 1, 3, 133, np.float32, 12, _prm(133), 1),
    "s-mixed4": ("single", "mixed4", 1, 2, 133, np.float32, 13, _prm(133), 1),
    "s-floor": ("single", "floor", 1, 2, 133, np.float64, 14, _prm(133), 1),
    "s-ring2": ("single", "ring2", 1, 2, 133, np.float32, 15, _prm(133), 1),
    "s-rolled3": ("single", "rolled3", 1, 2, 133, np.float32, 16, _prm(133), 1),
    "s-rolled5": ("single", "rolled5", 1, 2, 133, np.float64, 17, _prm(133), 1),
    "s-ring6": ("single", "ring6", 1, 2, 133, np.float32, 18, _prm(133), 1),
    "s-rolled8": ("single", "rolled8", 1, 2, 133, np.float32, 19, _prm(133), 1),
    # one detection per camera on shapes the lean kernels do not take: the route without a candidate pass
    "s-rolled6-J20": ("single", "rolled6", 1, 3, 20, np.float32, 20, _prm(17, condense_distance_tol=0.2), 2),
    "s-ring12-J8": ("single", "ring12", 1, 2, 8, np.float64, 21, _prm(8, condense_distance_tol=0.2), 2),
    # several detections per camera
    "m-rolled2-ghosts": ("multi", "rolled2", 2, 3, 12, np.float32, 30, _prm(12, **GHOSTS), 2),
    "m-rolled3-tight": ("multi", "rolled3", 3, 4, 12, np.float32, 31, _prm(12, condense_score_tol=2.0, **TIGHT), 4),
    "m-rolled3-band": ("multi", "rolled3", 3, 4, 12, np.float32, 31, _prm(12, **BAND), 4),
    "m-rolled3-ghosts": ("multi", "rolled3", 3, 4, 12, np.float32, 31, _prm(12, **GHOSTS), 2),
    "m-ring4-tight": ("multi", "ring4", 2, 4, 16, np.float64, 32, _prm(16, condense_score_tol=2.2, **TIGHT), 3),
    "m-mixed4-ghosts": ("multi", "mixed4", 2, 3, 12, np.float32, 33, _prm(12, **GHOSTS), 2),
    "m-rolled8-tight": ("multi", "rolled8", 2, 3, 10, np.float32, 34, _prm(10, condense_score_tol=4.0, **TIGHT), 3),
    "m-rolled8-clean": ("multi", "rolled8", 2, 3, 10, np.float32, 34, _prm(10, **CLEAN), 3),
    "m-rolled8-ghosts": ("multi", "rolled8", 2, 3, 10, np.float32, 34, _prm(10, **GHOSTS), 2),
    "m-ring12-tight": ("multi", "ring12", 2, 2, 8, np.float32, 35, _prm(8, condense_score_tol=4.0, **TIGHT), 3),
    "m-ring12-clean": ("multi", "ring12", 2, 2, 8, np.float32, 35, _prm(8, **CLEAN), 3),
    "m-rolled16-ghosts": ("multi", "rolled16", 2, 2, 6, np.float64, 36, _prm(6, **GHOSTS), 2),
}


@functools.lru_cache(maxsize=None)
def scene(name):
    kind, rig_name, P, F, J, dt, seed, prm, pout = CASES[name]
    sc = single(rig_name, F, J, dt, seed) if kind == "single" else multi(rig_name, P, F, J, dt, seed)
    sc.update(prm=prm, pout=pout, rig_name=rig_name, kind=kind, name=name)
    return sc


@functools.lru_cache(maxsize=None)
def _prepared(scene_key):
    from oracle import skew_exact as sx
    sc = scene(scene_key)
    return sx.prepare(sc["K"], sc["R"], sc["kpts"], sc["n_persons"])


def _scene_key(name):
    """Cases that share a scene (the same rig, people and seed, other thresholds) share its prepared rays."""
    kind, rig_name, P, F, J, dt, seed, prm, pout = CASES[name]
    for other, spec in CASES.items():
        if spec[:7] == CASES[name][:7]:
            return other
    return name


@functools.lru_cache(maxsize=None)
def exact(name, placement):
    """The exact rule of case `name` at `placement` (computed once per process)."""
    from oracle import skew_exact as sx
    sc = scene(name)
    tp = fc.place(sc["t"], None, placement)[0]
    return sx.evaluate(_prepared(_scene_key(name)), tp, place_params(sc["prm"], placement), sc["pout"])


@functools.lru_cache(maxsize=None)
def exact_with_slots(name, placement, pout):
    """`exact` with another Pout_max (the per-frame entries return every person)."""
    from oracle import skew_exact as sx
    sc = scene(name)
    tp = fc.place(sc["t"], None, placement)[0]
    return sx.evaluate(_prepared(_scene_key(name)), tp, place_params(sc["prm"], placement), pout)


def placed(name, placement):
    """-> (t', X', thresholds, u) of the case at the placement."""
    sc = scene(name)
    tp, Xp, u, D = fc.place(sc["t"], sc["X"], placement)
    return tp, Xp, place_params(sc["prm"], placement), u


# ------------------------------------------------------------------------------------------------------------------ comparison
def xyz_bound(want_xyz, t, out_dtype, factor=1.0):
    """The bound around `want_xyz` (world coordinates of the placement), elementwise: float64 outputs 2.5e-10 s + 1e-9 of what
    |xyz - c| exceeds s by, (c, s) the rig frame of oracle/dlt.py; float32 outputs 2e-6 s / 4.5 + one float32 ulp of the value."""
    from oracle import dlt as odlt
    c, s = odlt.rig_frame(t)
    if np.dtype(out_dtype) == np.float64:
        beyond = np.maximum(0.0, np.linalg.norm(want_xyz - c, axis=-1) - s)[..., None]
        return factor * (XYZ_F64 * s + 1e-9 * beyond) + 0.0 * want_xyz
    return factor * (XYZ_F32 * s / 4.5 + 2.0 ** -23 * np.abs(want_xyz))


def _scores(got, want, rtol, dist_err, nterms, what):
    from conftest import assert_scores_close
    try:
        with np.errstate(divide="ignore", invalid="ignore"):
            assert_scores_close(got, want, rtol=rtol, what=what, dist_err=dist_err, nterms=nterms)
    except AssertionError as e:
        return str(e)
    return None


def compare(got, want, t, out_dtype, u=1.0, Xtrue=None, dead=(), xyz_factor=1.0):
    """got: dict(xyz [F, pout, kn, 3], kscore [F, pout, kn], pscore [F, pout], count [F], status [F]) of a kernel route or of the
    fp64 oracle; want: an oracle/skew_exact.py::evaluate result at the same placement (rig centres t, u units per metre).
    -> (failures: list of (quantity, message), figures: dict quantity -> worst error / bound).  Frames with an exactly singular
    pair are compared on status only."""
    fails, fig = [], {}
    f32 = np.dtype(out_dtype) == np.float32
    F, pout, kn = want["xyz"].shape[:3]
    gst = np.asarray(got["status"]).reshape(F) != 0
    if not np.array_equal(gst, want["status"] != 0):
        fails.append(("status", f"singular frames {np.nonzero(gst)[0].tolist()} vs the rule's {np.nonzero(want['status'])[0].tolist()}"))
        return fails, fig
    ok = want["status"] == 0
    if not np.array_equal(np.asarray(got["count"])[ok], want["count"][ok]):
        fails.append(("count", f"{np.asarray(got['count'])[ok].tolist()} vs the rule's {want['count'][ok].tolist()}"))
        return fails, fig
    L = subtract_scale(t)
    gx, gk, gp = (np.asarray(got[k], dtype=np.float64) for k in ("xyz", "kscore", "pscore"))
    worst_x = worst_far = 0.0
    n_truth = 0
    for f in np.nonzero(ok)[0]:
        m = min(int(want["count"][f]), pout)
        if gx[f, m:].any() or gk[f, m:].any() or gp[f, m:].any():
            fails.append(("zero fill", f"frame {f}: slots behind the count are not zero"))
        if not m:
            continue
        wx, wk, wp = want["xyz"][f, :m], want["kscore"][f, :m], want["pscore"][f, :m]
        seen = wk != 0
        if gx[f, :m][~seen].any() or gk[f, :m][~seen].any():
            fails.append(("dead joint", f"frame {f}: a joint without a score is not (0, 0, 0, 0): {gx[f, :m][~seen][:2]}"))
        err, tol = np.abs(gx[f, :m] - wx)[seen], xyz_bound(wx, t, out_dtype, xyz_factor)[seen]
        if err.size:
            worst_x = max(worst_x, float(np.max(err / tol)))
            if not (err <= tol).all():
                fails.append(("xyz", f"frame {f}: max |err| = {err.max():.3e} ({err.max() / u:.3e} m), worst err / bound = {np.max(err / tol):.3g}"))
        nmem = max(len(mm) for mm in want["members"][f][:m])
        msg = _scores(gk[f, :m], wk, 3e-7 if f32 else 1e-9, 1e-14 * L, nmem, f"kscore frame {f}")
        if msg:
            fails.append(("kscore", msg))
        msg = _scores(gp[f, :m], wp, 3e-7 if f32 else 1e-9, 1e-14 * L, nmem * max(kn, 1), f"pscore frame {f}")
        if msg:
            fails.append(("pscore", msg))
        if Xtrue is not None:                                # geometric sanity: where the rule's joint lies within 0.04 u of a true person's
            for p in range(m):                               # (wrong pairings and grazing pairs do not), the joint lies within 0.05 u of it
                dw = np.linalg.norm(wx[p][None] - Xtrue[f][:, :kn], axis=-1)             # [P, kn]
                dg = np.linalg.norm(gx[f, p][None] - Xtrue[f][:, :kn], axis=-1)
                near = seen[p][None] & (dw < 0.04 * u)
                n_truth += int(near.sum())
                if near.any():
                    worst_far = max(worst_far, float(dg[near].max()) / u)
                    if not (dg[near] < 0.05 * u).all():
                        fails.append(("truth", f"frame {f} person {p}: a joint {dg[near].max() / u:.3g} m from the placed truth"))
    for f, p, j in dead:
        if want["status"][f] == 0 and want["count"][f] > p and (want["kscore"][f, p, j] != 0 or gx[f, p, j].any() or gk[f, p, j] != 0):
            fails.append(("dead joint", f"{(f, p, j)}: rule score {want['kscore'][f, p, j]}, got {gx[f, p, j]}, {gk[f, p, j]}"))
    fig["xyz"] = worst_x
    fig["truth_m"] = worst_far
    fig["truth_joints"] = n_truth
    return fails, fig


def as_result(out, kn=None):
    """A BatchTriangulator.run_host result -> the dict `compare` takes (status per frame from the singular flag)."""
    from snowmocap_amd import _lib
    x = out["xyzs"]
    return dict(xyz=x[..., :3], kscore=x[..., 3], pscore=out["pscore"], count=out["count"],
                status=((out["flags"] & _lib.FLAG_SINGULAR) != 0).astype(np.int32))


def oracle_result(K, R, t, kpts, n_persons, prm, pout):
    """The fp64 C oracle in the dict `compare` takes."""
    from oracle import oracle as orc
    ref = orc.triangulate_condense_batch(K, R, t, kpts, n_persons, orc.make_params(**prm), pout)
    return dict(xyz=ref["xyz"], kscore=ref["kscore"], pscore=ref["pscore"], count=ref["count"], status=(ref["status"] == 1).astype(np.int32))
