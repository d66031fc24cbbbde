#!/usr/bin/env python3
"""GPU box: the gap filler (snowtri_fill_joint_track, k_fill_gaps) on a device-resident fp64 track of the shape of the next_rows
lines -- T = 100 000 frames, m = 4 x 133 lanes, 1.7 GB -- with 5 % of the records missing in runs of 1-8 frames, beside
snowtri_smooth_joint_track on the SAME array in the same process (both passes move 64 bytes per record: its time is the yardstick).

  - HIP events around single launches queued back to back, median of --calls launches per round after a warm-up, the three
    kernels measured in alternating rounds;
  - max_gap = 8 without and with the code array, and max_gap = 255 on the same data (what the early-exit halo costs in the
    worst configured case);
  - GB/s against the algorithmic bytes: 64 per record (+ 1 with codes);
  - the result is compared bit for bit with the NumPy reference on the first 8 lanes.

    python scripts/bench_fill.py [--frames=N] [--lanes=N] [--calls=N] [--rounds=N]
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
from snowmocap_amd.fill import fill_joint_track_reference


def arg(name, default):
    return ([int(a.split("=")[1]) for a in sys.argv if a.startswith(f"--{name}=")] or [default])[0]


T, M, CALLS, ROUNDS = arg("frames", 100000), arg("lanes", 4 * 133), arg("calls", 20), arg("rounds", 3)


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
    """measured records everywhere, then runs of 1-8 missing ones (zero records) started with the probability that leaves ~5 % missing"""
    g = torch.Generator(device=dev)
    g.manual_seed(seed)
    x = torch.randn((T, M, 4), generator=g, dtype=torch.float64, device=dev)
    x[..., 3] = 0.1 + 0.9 * torch.rand((T, M), generator=g, dtype=torch.float64, device=dev)
    start = torch.rand((T, M), generator=g, device=dev) < 0.05 / 4.5
    length = torch.randint(1, 9, (T, M), generator=g, device=dev)
    length = torch.where(start, length, torch.zeros_like(length))
    missing = torch.zeros((T, M), dtype=torch.bool, device=dev)
    for j in range(8):
        missing[j:] |= length[:T - j] > j
    x[missing] = 0.0
    return x, float(missing.float().mean())


def main():
    dev = torch.device("cuda", 0)
    ctx = _lib.scratch_context()
    L, h = ctx.L, ctx.handle
    x, frac = make_track(dev)
    out, sm = torch.empty_like(x), torch.empty_like(x)
    codes = torch.empty((T, M), dtype=torch.uint8, device=dev)
    st = ct.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
    xp, op, sp, cp = (ct.c_void_p(a.data_ptr()) for a in (x, out, sm, codes))

    def fill(max_gap, with_codes):
        _lib.check(L.snowtri_fill_joint_track(h, T, M, xp, _lib.F64, max_gap, op, cp if with_codes else None, _lib.DEVICE, st),
                   "snowtri_fill_joint_track")

    def smooth():
        _lib.check(L.snowtri_smooth_joint_track(h, T, M, xp, 2.5, 0.75, 0.0, 1.0 / 30.0, sp, _lib.DEVICE, st), "snowtri_smooth_joint_track")

    runs = {"fill_gap8": lambda: fill(8, False), "fill_gap8_codes": lambda: fill(8, True), "fill_gap255": lambda: fill(255, False),
            "smooth_joint_track": smooth}
    for fn in runs.values():
        for _ in range(3):
            fn()
    torch.cuda.synchronize()
    ms = {k: [] for k in runs}
    for _ in range(ROUNDS):                                  # alternating rounds: drift hits every kernel alike
        for k, fn in runs.items():
            ms[k] += event_ms(fn, CALLS)
    med = {k: float(np.median(v)) for k, v in ms.items()}
    # the result, bit for bit, on the first lanes
    fill(8, True)
    torch.cuda.synchronize()
    n_check = min(M, 8)
    ref, ref_codes = fill_joint_track_reference(x[:, :n_check].cpu().numpy(), 8)
    same = bool(np.array_equal(out[:, :n_check].contiguous().cpu().numpy().view(np.uint64), ref.view(np.uint64))
                and np.array_equal(codes[:, :n_check].cpu().numpy(), ref_codes))
    n_codes = torch.bincount(codes.view(-1).to(torch.int64), minlength=4).tolist()
    rec_bytes = 64 * T * M
    line = dict(what="fill", frames=T, lanes=M, dtype="float64", missing_fraction=frac, calls_per_kernel=CALLS * ROUNDS,
                block_frames=int(L.snowtri_fill_block_frames()), codes_count=n_codes, equals_reference_on_first_lanes=same,
                ms_median=med, ms_min={k: float(min(v)) for k, v in ms.items()},
                GBps={k: (rec_bytes + (T * M if k == "fill_gap8_codes" else 0)) / med[k] * 1e-6 for k in med},
                fill_over_smooth=med["fill_gap8"] / med["smooth_joint_track"],
                fill_codes_over_smooth=med["fill_gap8_codes"] / med["smooth_joint_track"],
                fill_gap255_over_gap8=med["fill_gap255"] / med["fill_gap8"])
    print(json.dumps(line))
    if not same:
        sys.exit("the fill differs from the NumPy reference")


if __name__ == "__main__":
    main()
