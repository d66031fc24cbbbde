#!/usr/bin/env python3
"""GPU box: the despike pass (snowtri_despike_joint_track, k_despike) on a device-resident track of the shape of the next_rows
lines -- T = 100 000 frames, m = 4 x 133 lanes, 1.7 GB as float64 -- a smooth path with 5 mm of noise, 2 % of the records moved by
0.15-0.6 m and 5 % missing, beside k_fill_gaps (max_gap = 8) and snowtri_smooth_joint_track on the SAME float64 array in the same
process (all three passes read and write every record once: their times are the yardsticks).

  - HIP events around single launches queued back to back, median of --calls launches per round after a warm-up, all kernels
    measured in alternating rounds;
  - half_window = 1..4, float64 and float32 records, without and with the code array, tol = 0.1, MARK;
  - GB/s against the algorithmic bytes: (1 + 2 H / block_frames) reads and 1 write per record (+ 1 byte with codes);
  - the result is compared bit for bit with the NumPy reference on the first 8 lanes, for every half_window and both dtypes.

    python scripts/bench_despike.py [--frames=N] [--lanes=N] [--calls=N] [--rounds=N]
Prints one JSON line; the figures go into EXPERIMENTS.md.
"""
import ctypes as ct
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch

from snowmocap_amd import _lib
from snowmocap_amd.despike import despike_joint_track_reference


def arg(name, default):
    return ([int(a.split("=")[1]) for a in sys.argv if a.startswith(f"--{name}=")] or [default])[0]


T, M, CALLS, ROUNDS = arg("frames", 100000), arg("lanes", 4 * 133), arg("calls", 10), arg("rounds", 3)
TOL = 0.1


def event_ms(fn, calls):
    """durations of `calls` single launches, each between its own event pair, queued back to back"""
    pairs = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(calls)]
    for a, b in pairs:
        a.record()
        fn()
        b.record()
    torch.cuda.synchronize()
    return [a.elapsed_time(b) for a, b in pairs]


def make_track(dev, seed=5):
    """every lane on its own smooth path (a few centimetres per frame at most) + 5 mm of noise; 2 % of the records moved by
    0.15-0.6 m in a random direction; 5 % of the records missing (zero records)"""
    g = torch.Generator(device=dev)
    g.manual_seed(seed)
    f64 = torch.float64
    t = torch.arange(T, dtype=f64, device=dev)[:, None]
    lane = torch.arange(M, dtype=f64, device=dev)[None, :]
    x = torch.empty((T, M, 4), dtype=f64, device=dev)
    x[..., 0] = 1.5 * torch.cos(0.02 * t + lane)
    x[..., 1] = 1.5 * torch.sin(0.02 * t + lane)
    x[..., 2] = 1.0 + 0.3 * torch.sin(0.013 * t + 0.7 * lane)
    x[..., :3] += 0.005 * torch.randn((T, M, 3), generator=g, dtype=f64, device=dev)
    x[..., 3] = 3.5 + 4.5 * torch.rand((T, M), generator=g, dtype=f64, device=dev)
    moved = torch.rand((T, M), generator=g, device=dev) < 0.02
    d = torch.randn((T, M, 3), generator=g, dtype=f64, device=dev)
    d = d / d.norm(dim=-1, keepdim=True) * (0.15 + 0.45 * torch.rand((T, M, 1), generator=g, dtype=f64, device=dev))
    x[..., :3] += torch.where(moved[..., None], d, torch.zeros_like(d))
    missing = torch.rand((T, M), generator=g, device=dev) < 0.05
    x[missing] = 0.0
    return x, float((moved & ~missing).float().mean()), float(missing.float().mean())


def main():
    dev = torch.device("cuda", 0)
    ctx = _lib.scratch_context()
    L, h = ctx.L, ctx.handle
    x64, frac_moved, frac_missing = make_track(dev)
    x = {"float64": x64, "float32": x64.to(torch.float32)}
    out = {k: torch.empty_like(v) for k, v in x.items()}
    sm = torch.empty_like(x64)
    codes = torch.empty((T, M), dtype=torch.uint8, device=dev)
    st = ct.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
    p = lambda a: ct.c_void_p(a.data_ptr())     # noqa: E731
    code = {"float64": _lib.F64, "float32": _lib.F32}

    def despike(dt, hw, with_codes):
        _lib.check(L.snowtri_despike_joint_track(h, T, M, p(x[dt]), code[dt], hw, TOL, _lib.DESPIKE_MARK, p(out[dt]),
                                                 p(codes) if with_codes else None, _lib.DEVICE, st), "snowtri_despike_joint_track")

    def fill():
        _lib.check(L.snowtri_fill_joint_track(h, T, M, p(x64), _lib.F64, 8, p(out["float64"]), None, _lib.DEVICE, st), "snowtri_fill_joint_track")

    def smooth():
        _lib.check(L.snowtri_smooth_joint_track(h, T, M, p(x64), 2.5, 0.75, 0.0, 1.0 / 30.0, p(sm), _lib.DEVICE, st), "snowtri_smooth_joint_track")

    runs = {"fill_gap8": fill, "smooth_joint_track": smooth}
    for dt in ("float64", "float32"):
        for hw in (1, 2, 3, 4):
            runs[f"despike_{dt}_h{hw}"] = lambda dt=dt, hw=hw: despike(dt, hw, False)
            runs[f"despike_{dt}_h{hw}_codes"] = lambda dt=dt, hw=hw: despike(dt, hw, True)
    for fn in runs.values():
        for _ in range(2):
            fn()
    torch.cuda.synchronize()
    ms = {k: [] for k in runs}
    for _ in range(ROUNDS):                                  # alternating rounds: drift hits every kernel alike
        for k, fn in runs.items():
            ms[k] += event_ms(fn, CALLS)
    med = {k: float(np.median(v)) for k, v in ms.items()}
    # the result, bit for bit, on the first lanes
    n_check = min(M, 8)
    same, n_codes = True, None
    for dt in ("float64", "float32"):
        ref_in = x[dt][:, :n_check].contiguous().cpu().numpy()
        for hw in (1, 2, 3, 4):
            despike(dt, hw, True)
            torch.cuda.synchronize()
            ref, ref_codes = despike_joint_track_reference(ref_in, hw, TOL, _lib.DESPIKE_MARK)
            got = out[dt][:, :n_check].contiguous().cpu().numpy()
            same = same and bool(np.array_equal(got.view(np.uint8), ref.view(np.uint8)) and np.array_equal(codes[:, :n_check].cpu().numpy(), ref_codes))
            if dt == "float64" and hw == 3:
                n_codes = torch.bincount(codes.view(-1).to(torch.int64), minlength=4).tolist()
    B = int(L.snowtri_despike_block_frames())

    def bytes_of(k):
        if not k.startswith("despike"):
            return 64 * T * M
        rec = 32 if "float64" in k else 16
        hw = int(k.split("_h")[1][0])
        return T * M * (rec * (2.0 + 2.0 * hw / B) + (1 if k.endswith("codes") else 0))

    line = dict(what="despike", frames=T, lanes=M, tol=TOL, moved_fraction=frac_moved, missing_fraction=frac_missing,
                calls_per_kernel=CALLS * ROUNDS, block_frames=B, codes_count_float64_h3=n_codes, equals_reference_on_first_lanes=same,
                ms_median={k: round(v, 4) for k, v in med.items()}, ms_min={k: round(float(min(v)), 4) for k, v in ms.items()},
                GBps={k: round(bytes_of(k) / med[k] * 1e-6, 1) for k in med},
                over_fill={k: round(med[k] / med["fill_gap8"], 3) for k in med if k.startswith("despike")},
                h3_float64_over_smooth=round(med["despike_float64_h3"] / med["smooth_joint_track"], 3))
    print(json.dumps(line))
    if not same:
        sys.exit("the despike pass differs from the NumPy reference")


if __name__ == "__main__":
    main()
