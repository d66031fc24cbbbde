"""Inputs shared by tests/test_undistort_host.py and tests/test_gpu_undistort.py (row N4, k_undistort): lenses, rigs, raw pixels with
their exact inverses (oracle/undistort_exact.py), the launch shapes, and the wave-uniform exit rule the kernel used to have, in NumPy.
No GPU code; everything is seeded.

A case is (rig, (F, P, J), dtype).  Each camera of a rig owns a POOL of true undistorted pixels, uniform in [-50, 1330] x [-50, 770];
`forward_exact` rounded to float64 gives the raw pixels, and what the kernel is held to is the exact inverse of THAT raw pixel (of
its float32 rounding for float32 keypoints), not the true pixel.  A case draws its [F, C, P, J] observations from its cameras' pools
(seeded), so every lane of every shape has an exact answer while the suite computes POOL inverses per camera and dtype once
(functools.lru_cache; ~0.7 ms each).
"""
import functools
import zlib

import numpy as np

from snowmocap_amd import synth

BOX = ((-50.0, 1330.0), (-50.0, 770.0))
POOL = 144                                       # pixels per camera

LENSES = {                                       # (k1, k2, p1, p2, k3)
    "shipped": tuple(float(v) for v in synth.load_rig_distortion()[0]),
    "barrel": (-0.30, 0.10, 0.001, -0.0008, -0.015),
    "strong-barrel": (-0.38, 0.18, 0.0, 0.0, -0.045),
    "pincushion": (0.25, 0.05, -0.002, 0.001, 0.0),
    "tangential": (0.02, 0.0, 0.02, -0.015, 0.0),
}
LENS_NAMES = tuple(LENSES)

# rig -> (cameras, skewed, first lens).  Camera c carries lens (first + c) % 5: within the first five cameras the lens identifies c.
RIGS = {"ring3": (3, True, 0), "ring5": (5, True, 0), "ring8": (8, True, 0), "floor": (4, True, 0), "floor-s0": (4, False, 3)}
# (floor-s0 keeps the shipped intrinsics, whose principal points sit up to 50 px off centre: r2 reaches 1.45 in a corner, where the
# strong barrel's radial eigenvalue 1 + 3 k1 r2 + 5 k2 r2^2 + 7 k3 r2^3 has dropped to 0.28 -- so that rig starts at the pincushion lens)
DISTINCT_LENS_RIGS = ("ring3", "ring5", "floor", "floor-s0")

SHAPES = [(1, 1, 1),                             # n_obs = C: every lane another camera
          (3, 1, 17),
          (1, 3, 21),                            # per_cam = 63, below a wave
          (2, 1, 64),                            # per_cam = a wave
          (5, 2, 133),                           # per_cam = 266: a wave spans two cameras, the last block is partial
          (40, 1, 133)]                          # the recording of the wave tests
BLOCK_SHAPE = (1, 1, 256)                        # on a 4-camera rig: per_cam = a block, n_obs = 4 blocks
WAVE_SHAPE = (40, 1, 133)
WAVE_RIG = "floor"                               # camera 0 carries the shipped lens


def shapes_of(rig_name):
    return SHAPES + ([BLOCK_SHAPE] if RIGS[rig_name][0] == 4 else [])


def rig(name):
    """-> K [C,3,3], R, t, D [C,5], lens name per camera."""
    C, skewed, first = RIGS[name]
    K, R, t = synth.load_rig_json() if name.startswith("floor") else synth.ring_rig(C)
    K = K.copy()
    for c in range(C):
        if skewed:                               # own focal lengths, centre and skew per camera (0.5 ... 4 px)
            fx = 676.0 + 9.0 * c
            K[c] = [[fx, 0.5 + 3.5 * c / (C - 1), 603.0 + 13.0 * c], [0.0, 1.012 * fx - 3.0 * c, 378.0 - 6.0 * c], [0.0, 0.0, 1.0]]
        else:
            assert K[c, 0, 1] == 0.0             # the shipped intrinsics: s = 0 everywhere
    names = [LENS_NAMES[(first + c) % len(LENS_NAMES)] for c in range(C)]
    return K, R, t, np.array([LENSES[n] for n in names]), names


def _seed(*parts):
    return zlib.crc32(repr(parts).encode())


@functools.lru_cache(maxsize=None)
def pool(rig_name, cam, dtype_name="float64"):
    """-> dict(true [POOL,2], raw [POOL,2] (float64 values, representable in `dtype_name`), inv [POOL,2] exact inverse of raw,
    roundtrip [POOL]: |forward_exact(exact_inverse(raw)) - raw| in 50-digit arithmetic, px)."""
    import mpmath as mp
    from oracle import undistort_exact as ue
    K, _, _, D, _ = rig(rig_name)
    if dtype_name == "float32":
        raw = pool(rig_name, cam)["raw"].astype(np.float32).astype(np.float64)
        true = pool(rig_name, cam)["true"]
    else:
        rng = np.random.default_rng(_seed("pool", rig_name, cam))
        true = np.stack([rng.uniform(*BOX[0], POOL), rng.uniform(*BOX[1], POOL)], axis=-1)
        raw = ue.forward_exact(K[cam], D[cam], true)
    inv, back = np.empty_like(raw), np.empty(raw.shape[0])
    for i, (u, v) in enumerate(raw):
        iu, iv = ue.exact_inverse_mp(K[cam], D[cam], float(u), float(v))
        fu, fv = ue.forward_exact_mp(K[cam], D[cam], iu, iv)               # (of the unrounded inverse)
        inv[i] = float(iu), float(iv)
        with mp.workdps(ue.DIGITS):
            back[i] = float(max(abs(fu - mp.mpf(float(u))), abs(fv - mp.mpf(float(v)))))
    out = dict(true=true, raw=raw, inv=inv, roundtrip=back)
    for a in out.values():
        a.setflags(write=False)
    return out


@functools.lru_cache(maxsize=None)
def case(rig_name, shape, dtype_name="float64"):
    """-> dict(K, R, t, D, kpts [F,C,P,J,3] of `dtype_name` (raw pixels, scores in (0, 9)), want [F,C,P,J,2] float64 exact inverses,
    true [F,C,P,J,2]).  Read-only: shared between tests."""
    F, P, J = shape
    K, R, t, D, names = rig(rig_name)
    C = K.shape[0]
    rng = np.random.default_rng(_seed("case", rig_name, shape))
    idx = rng.integers(0, POOL, (F, C, P, J))
    kp = np.empty((F, C, P, J, 3))
    want, true = np.empty((F, C, P, J, 2)), np.empty((F, C, P, J, 2))
    for c in range(C):
        p = pool(rig_name, c, dtype_name)
        kp[:, c, ..., :2], want[:, c], true[:, c] = p["raw"][idx[:, c]], p["inv"][idx[:, c]], p["true"][idx[:, c]]
    kp[..., 2] = rng.uniform(0.0, 9.0, (F, C, P, J))
    raw64 = kp[..., :2].copy()
    kp = kp.astype(dtype_name)
    assert np.array_equal(kp[..., :2].astype(np.float64), raw64)          # the pool's raw pixels are representable in the case's dtype
    out = dict(K=K, R=R, t=t, D=D, lenses=names, kpts=kp, want=want, true=true)
    for a in (K, R, t, D, kp, want, true):
        a.setflags(write=False)
    return out


@functools.lru_cache(maxsize=None)
def recording(rig_name=WAVE_RIG, F=40, dtype_name="float64"):
    """A person seen by every camera of `rig_name` for F frames, detected on the RAW frames: the undistorted projections of
    synth.make_keypoints (no pixel noise) pushed through each camera's lens (oracle/undistort.py::distort_pixels, which
    test_undistort_host.py holds to forward_exact).  The joints of a frame spread over ~300 px, so the lanes of a wave need
    different step counts.  -> dict(K, R, t, D, kpts [F,C,1,133,3], n_persons [F,C], X [F,1,133,3]); read-only."""
    from oracle import undistort as ou
    K, R, t, D, _ = rig(rig_name)
    rng = np.random.default_rng(_seed("recording", rig_name, F))
    X = synth.make_people(rng, F, 1)
    kp, npers = synth.make_keypoints(rng, K, R, t, X, pixel_sigma=0.0, dtype=np.float64)
    kp = kp.copy()
    for c in range(K.shape[0]):
        kp[:, c, ..., :2] = ou.distort_pixels(K[c], D[c], kp[:, c, ..., :2])
    kp = kp.astype(dtype_name)
    for a in (K, R, t, D, kp, npers, X):
        a.setflags(write=False)
    return dict(K=K, R=R, t=t, D=D, kpts=kp, n_persons=npers, X=X)


def f32_ulp(x):
    """Spacing of float32 at |x| (float64 arithmetic; the binade of x itself, so a bound of half of it never widens at a power of two)."""
    ax = np.maximum(np.abs(np.asarray(x, dtype=np.float64)), 2.0 ** -126)
    return 2.0 ** (np.floor(np.log2(ax)) - 23)


def poison(kpts, value, every=64, at=37):
    """A copy of kpts with (u, v) of one observation in each `every` (flat order, lane `at` of each group) set to `value`.
    -> (copy, mask [F,C,P,J] of the observations touched)."""
    out = np.array(kpts, copy=True)
    flat = out.reshape(-1, 3)
    hit = np.zeros(flat.shape[0], dtype=bool)
    hit[at % every::every] = True
    flat[hit, :2] = value
    return out, hit.reshape(kpts.shape[:-1])


def emulate_wave_uniform(K, D, raw, first_wave=64, wave=64, iters=8, tol=1e-8):
    """The exit rule k_undistort had before a lane's bits were made its own: the Newton loop of a wave runs until EVERY lane's step
    is below `tol` (or `iters`), and every lane keeps applying its step until then.  raw [N, 2] float64, lanes in order; the first
    wave holds `first_wave` lanes, the following ones `wave` -- two values of first_wave align the same observations to their waves
    in two ways.  Plain NumPy (no fma, `/` for the reciprocal): it shows what the RULE permits, not the kernel's bits."""
    K = np.asarray(K, dtype=np.float64)
    fx, s, cx, fy, cy = K[0, 0], K[0, 1], K[0, 2], K[1, 1], K[1, 2]
    k1, k2, p1, p2, k3 = [float(v) for v in np.asarray(D, dtype=np.float64).reshape(-1)[:5]]
    raw = np.asarray(raw, dtype=np.float64).reshape(-1, 2)
    out = np.empty_like(raw)
    lo = 0
    with np.errstate(invalid="ignore", over="ignore", divide="ignore"):
        while lo < raw.shape[0]:
            hi = min(raw.shape[0], lo + (first_wave if lo == 0 else wave))
            yd = (raw[lo:hi, 1] - cy) / fy
            xd = (raw[lo:hi, 0] - cx - s * yd) / fx
            x, y = xd.copy(), yd.copy()
            for _ in range(iters):
                r2 = x * x + y * y
                rho = 1 + r2 * (k1 + r2 * (k2 + r2 * k3))
                drho = k1 + r2 * (2 * k2 + r2 * 3 * k3)
                f1 = x * rho + 2 * p1 * x * y + p2 * (r2 + 2 * x * x) - xd
                f2 = y * rho + p1 * (r2 + 2 * y * y) + 2 * p2 * x * y - yd
                a = rho + 2 * x * x * drho + 2 * p1 * y + 6 * p2 * x
                b = 2 * x * y * drho + 2 * p1 * x + 2 * p2 * y
                d = rho + 2 * y * y * drho + 6 * p1 * y + 2 * p2 * x
                det = a * d - b * b
                dx, dy = (d * f1 - b * f2) / det, (a * f2 - b * f1) / det
                x, y = x - dx, y - dy
                if np.all(np.maximum(np.abs(dx), np.abs(dy)) < tol):       # (NaN compares false: its wave runs to the bound)
                    break
            out[lo:hi, 0], out[lo:hi, 1] = fx * x + s * y + cx, fy * y + cy
            lo = hi
    return out
