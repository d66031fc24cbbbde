"""Inputs shared by tests/test_dlt_frames_host.py and tests/test_gpu_dlt_frames.py: the same rig and the same pixels placed at six
positions / units of the world.  A placement (u, D) moves a rig and its scene together: t' = u (t + D), X' = u (X + D) -- u world
units per metre, D the offset in metres -- so every camera sees the SAME pixels.  Thresholds in world units scale by u; the
association's candidate score is confidence / (1000 x a distance in world units), so average_score_threshold scales by 1 / u:
with both, every placement poses the association the same questions."""
import numpy as np

from snowmocap_amd import synth

FAR = np.array([40.0, -25.0, 3.0])              # (FAR of tests/test_gpu_lean_origin.py)
SITE = np.array([800.0, -600.0, 30.0])          # site coordinates
PLACEMENTS = {"home": (1.0, np.zeros(3)), "moved": (1.0, FAR), "site": (1.0, SITE),
              "mm": (1000.0, np.zeros(3)), "mm-moved": (1000.0, FAR), "mm-site": (1000.0, SITE)}
MIXED_PLACEMENTS = ("home", "mm-moved")         # where the rig with per-camera intrinsics runs
WORLD_UNIT_THRESHOLDS = ("distance_threshold", "condense_distance_tol")


def place(t, X, name):
    """-> (t', X', u, D) of the placement `name` (X may be None)."""
    u, D = PLACEMENTS[name]
    return u * (np.asarray(t, float) + D), (None if X is None else u * (np.asarray(X, float) + D)), u, D


def place_params(prm, name):
    u = PLACEMENTS[name][0]
    out = dict(prm)
    for k in WORLD_UNIT_THRESHOLDS:
        if k in out:
            out[k] = out[k] * u
    if "average_score_threshold" in out:
        out["average_score_threshold"] = out["average_score_threshold"] / u
    return out


def home(xyz, name):
    """World coordinates of a placement -> metres at home: xyz / u - D."""
    u, D = PLACEMENTS[name]
    return np.asarray(xyz, float) / u - D


def mixed_rig(C):
    """ring_rig(C) with per-camera intrinsics: fx from 600 to 3000 (fy 1 % off), principal points off centre, a small skew."""
    K, R, t = synth.ring_rig(C)
    for c in range(C):
        fx = 600.0 + 2400.0 * c / max(1, C - 1)
        K[c] = [[fx, 0.4 + 0.3 * c, 640.0 + 37.0 * c - 90.0], [0.0, 1.01 * fx, 360.0 - 23.0 * c + 50.0], [0.0, 0.0, 1.0]]
    return K, R, t


def rig(name):
    """"ring<C>" or "mixed<C>"."""
    return mixed_rig(int(name[5:])) if name.startswith("mixed") else synth.ring_rig(int(name[4:]))


def rig_scale(t):
    """s of the DLT definition (oracle/dlt.py::rig_frame) -- the unit the bounds are stated in."""
    from oracle import dlt as odlt
    return odlt.rig_frame(t)[1]
