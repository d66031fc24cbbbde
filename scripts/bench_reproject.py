#!/usr/bin/env python3
"""GPU box: the reprojection kernels (snowtri_reproject, k_reproject; snowtri_reproject_cost, k_reproject_cost) on a device-resident
batch of the shape of configs[2] -- 10 000 frames x 8 cameras x 4 persons x 133 joints (synth.config_workload_device(3, ...): the
ring rig, per-view lists permuted, N(0, 1 px)) -- beside k_undistort on the SAME-shaped keypoint array [F][C][P][kn][3] in the same
process: it writes the same bytes per observation as k_reproject, reads more, and iterates a Newton loop, so its time is the
yardstick k_reproject is expected to stay under.

  - HIP events around single launches queued back to back, median of --calls launches per round after a warm-up, all kernels
    measured in alternating rounds;
  - float32 and float64 pixels / keypoints (records float64), undistorted and RAW;
  - GB/s against the algorithmic bytes: k_reproject one read of xyzs + one write of pix; k_undistort one read + one write of kpts;
    k_reproject_cost one read of xyzs, kpts and n_persons + one write of cost_sum and cost_n -- and beside its time the time ONE
    read of its inputs would take at the rate k_reproject measured;
  - the pixels are compared with the NumPy rule on the first 4 frames, the costs too.

    python scripts/bench_reproject.py [--frames=N] [--calls=N] [--rounds=N]
Prints one JSON line; the figures go into EXPERIMENTS.md.
"""
import ctypes as ct
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch

from snowmocap_amd import _lib, synth
from snowmocap_amd import reproject as rp


def arg(name, default):
    return ([int(a.split("=")[1]) for a in sys.argv if a.startswith(f"--{name}=")] or [default])[0]


F, CALLS, ROUNDS = arg("frames", 10000), arg("calls", 10), arg("rounds", 3)
THR = 3.0


def event_ms(fn, calls):
    """durations of `calls` single launches, each between its own event pair, queued back to back"""
    pairs = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(calls)]
    for a, b in pairs:
        a.record()
        fn()
        b.record()
    torch.cuda.synchronize()
    return [a.elapsed_time(b) for a, b in pairs]


def main():
    dev = torch.device("cuda", 0)
    wl = synth.config_workload_device(3, F, 11, dev, dtype=torch.float64)
    K, R, t = wl["rig"]
    C, P, kn = K.shape[0], int(wl["kpts"].shape[2]), int(wl["kpts"].shape[3])
    D = np.tile(np.array([[-0.30, 0.10, 0.001, -0.0008, -0.015]]), (C, 1))                  # a barrel lens on every camera
    ctx = _lib.Context(K, R, t)
    ctx.set_distortion(D)
    L, h = ctx.L, ctx.handle
    g = torch.Generator(device=dev)
    g.manual_seed(12)
    centres = torch.from_numpy(synth.person_centres(P)).to(dev)
    box = torch.tensor([0.6, 0.6, 1.8], dtype=torch.float64, device=dev)
    off = torch.tensor([0.5, 0.5, 0.0], dtype=torch.float64, device=dev)
    xyzs = torch.empty((F, P, kn, 4), dtype=torch.float64, device=dev)
    xyzs[..., :3] = (torch.rand((F, P, kn, 3), generator=g, dtype=torch.float64, device=dev) - off) * box + centres[None, :, None, :]
    xyzs[..., 3] = 3.5 + 4.5 * torch.rand((F, P, kn), generator=g, dtype=torch.float64, device=dev)
    xyzs[torch.rand((F, P, kn), generator=g, device=dev) < 0.03] = 0.0                      # 3 % missing records
    kp = {"float64": wl["kpts"], "float32": wl["kpts"].to(torch.float32)}
    npers = wl["n_persons"]
    tdt = {"float64": torch.float64, "float32": torch.float32}
    code = {"float64": _lib.F64, "float32": _lib.F32}
    pix = {k: torch.empty((F, C, P, kn, 3), dtype=v, device=dev) for k, v in tdt.items()}
    und = {k: torch.empty_like(v) for k, v in kp.items()}
    cs = torch.empty((F, C, P, P), dtype=torch.float64, device=dev)
    cn = torch.empty((F, C, P, P), dtype=torch.int32, device=dev)
    st = ct.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
    p = lambda a: ct.c_void_p(a.data_ptr())     # noqa: E731

    def reproject(dt, raw):
        _lib.check(L.snowtri_reproject(h, F, P, kn, p(xyzs), _lib.F64, _lib.REPROJECT_RAW if raw else 0, p(pix[dt]), code[dt], _lib.DEVICE, st),
                   "snowtri_reproject")

    def cost(dt, raw):
        _lib.check(L.snowtri_reproject_cost(h, F, P, kn, p(xyzs), _lib.F64, P, p(kp[dt]), code[dt], p(npers), THR,
                                            _lib.REPROJECT_RAW if raw else 0, p(cs), p(cn), _lib.DEVICE, st), "snowtri_reproject_cost")

    def undistort(dt):
        _lib.check(L.snowtri_undistort_keypoints(h, F, P, kn, p(kp[dt]), p(und[dt]), code[dt], _lib.DEVICE, st), "snowtri_undistort_keypoints")

    runs = {}
    for dt in ("float64", "float32"):
        runs[f"undistort_{dt}"] = lambda dt=dt: undistort(dt)
        for raw in (False, True):
            tag = "_raw" if raw else ""
            runs[f"reproject_{dt}{tag}"] = lambda dt=dt, raw=raw: reproject(dt, raw)
            runs[f"reproject_cost_{dt}{tag}"] = lambda dt=dt, raw=raw: cost(dt, raw)
    for fn in runs.values():
        for _ in range(2):
            fn()
    torch.cuda.synchronize()
    ms = {k: [] for k in runs}
    for _ in range(ROUNDS):                                  # alternating rounds: drift hits every kernel alike
        for k, fn in runs.items():
            ms[k] += event_ms(fn, CALLS)
    med = {k: float(np.median(v)) for k, v in ms.items()}

    # the result against the NumPy rule on the first frames
    nf = min(F, 4)
    x_h = xyzs[:nf].cpu().numpy()
    worst_px, costs_ok = 0.0, True
    for raw in (False, True):
        reproject("float64", raw)
        cost("float64", raw)
        torch.cuda.synchronize()
        ref = rp.reproject_reference(K, R, t, x_h, D=D, raw=raw)
        worst_px = max(worst_px, float(np.abs(pix["float64"][:nf].cpu().numpy() - ref).max()))
        ref_s, ref_n = rp.reprojection_cost_reference(K, R, t, x_h, kp["float64"][:nf].cpu().numpy(), npers[:nf].cpu().numpy(), THR, D=D, raw=raw)
        costs_ok = costs_ok and bool(np.array_equal(cn[:nf].cpu().numpy(), ref_n) and np.allclose(cs[:nf].cpu().numpy(), ref_s, rtol=1e-12, atol=1e-8))

    n_obs = F * C * P * kn
    x_bytes = 32 * F * P * kn

    def esz(k):
        return 8 if "float64" in k else 4

    def bytes_of(k):
        if k.startswith("undistort"):
            return 2 * 3 * esz(k) * n_obs
        if k.startswith("reproject_cost"):
            return x_bytes + 3 * esz(k) * n_obs + 4 * F * C + 12 * F * C * P * P
        return x_bytes + 3 * esz(k) * n_obs

    gbps = {k: bytes_of(k) / med[k] * 1e-6 for k in med}
    line = dict(what="reproject", frames=F, cameras=C, persons=P, joints=kn, observations=n_obs, calls_per_kernel=CALLS * ROUNDS,
                max_px_error_vs_numpy_rule_first_frames=worst_px, costs_equal_numpy_rule_first_frames=costs_ok,
                ms_median={k: round(v, 4) for k, v in med.items()}, ms_min={k: round(float(min(v)), 4) for k, v in ms.items()},
                GBps={k: round(v, 1) for k, v in gbps.items()},
                reproject_over_undistort={dt: round(med[f"reproject_{dt}"] / med[f"undistort_{dt}"], 3) for dt in ("float64", "float32")},
                reproject_raw_over_undistort={dt: round(med[f"reproject_{dt}_raw"] / med[f"undistort_{dt}"], 3) for dt in ("float64", "float32")},
                reproject_within_undistort=all(med[f"reproject_{dt}{tag}"] <= med[f"undistort_{dt}"] for dt in ("float64", "float32") for tag in ("", "_raw")),
                cost_input_read_ms_at_reproject_rate={dt: round((bytes_of(f"reproject_cost_{dt}") - 12 * F * C * P * P) / (gbps[f"reproject_{dt}"] * 1e6), 4)
                                                      for dt in ("float64", "float32")})
    print(json.dumps(line))
    if worst_px > 3e-11 or not costs_ok:
        sys.exit("the reprojection differs from the NumPy rule")


if __name__ == "__main__":
    main()
