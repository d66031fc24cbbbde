#!/usr/bin/env python
"""What the leave-one-out gate of method = DLT_ROBUST costs beside method = DLT (a record for EXPERIMENTS.md, not a gate).

Workload: 4 cameras x 1 person x 133 joints x 10 000 frames (the floor rig), float32 in and out, device-resident; every launch is
timed by a HIP event pair attached to its dispatch (snowtri_set_timing(ctx, 2): the kernel's own begin and end, as the roofline loop
of bench.py), launches queued back to back on one stream.  Three things in ONE process:
  (a) method = DLT                      k_dlt_coop
  (b) DLT_ROBUST on the clean batch     k_dlt_robust: one solve + C reprojections per joint, the round never entered
  (c) DLT_ROBUST, 10 % outlier joints   one camera shifted by 20-150 px on 10 % of the joints (synth.add_outliers)
Prints one JSON line.  Run it under a time limit of its own:  timeout -k 10 300 python scripts/bench_robust.py
"""
import argparse
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=10000)
    ap.add_argument("--launches", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--threshold-px", type=float, default=6.0)
    ap.add_argument("--max-drops", type=int, default=1)
    args = ap.parse_args()
    import torch
    from snowmocap_amd import _lib, synth
    from snowmocap_amd.batch import BatchTriangulator

    F = args.frames
    wl = synth.config_workload(2, F, seed=5)
    K, R, t = wl["rig"]
    clean = wl["kpts"]
    dirty, cam = synth.add_outliers(np.random.default_rng(6), clean, fraction=0.1)
    dev = torch.device("cuda", 0)
    d_clean, d_dirty = torch.from_numpy(clean).to(dev), torch.from_numpy(dirty).to(dev)

    def timed(method, kpts):
        bt = BatchTriangulator(K, R, t, wl["params"], pout_max=1, out_dtype=np.float32, method=method,
                               reproj_threshold_px=args.threshold_px, max_drops=args.max_drops)
        out = bt.alloc_outputs(F, dev)
        for _ in range(args.warmup):
            bt.run_torch(kpts, None, out=out)
        torch.cuda.synchronize(dev)
        bt.ctx.set_timing(True, attach=True)
        ms = []
        left = args.launches
        while left > 0:                                   # (the ring holds 1024 pairs)
            n = min(left, 1000)
            for _ in range(n):
                bt.run_torch(kpts, None, out=out)
            ms += bt.ctx.timing_collect()
            left -= n
        bt.ctx.set_timing(False)
        torch.cuda.synchronize(dev)
        name = bt.ctx.last_kernel_names()
        bt.close()
        return {"kernel": name, "us_median": float(np.median(ms)) * 1e3, "us_mean": float(np.mean(ms)) * 1e3,
                "us_min": float(np.min(ms)) * 1e3, "launches": len(ms)}

    a = timed(_lib.DLT, d_clean)
    b = timed(_lib.DLT_ROBUST, d_clean)
    c = timed(_lib.DLT_ROBUST, d_dirty)
    a2 = timed(_lib.DLT, d_clean)                          # (a) again at the end: drift of the box over the run
    print(json.dumps({"workload": f"4x1x133x{F} float32, device-resident", "device": torch.cuda.get_device_name(0),
                      "threshold_px": args.threshold_px, "max_drops": args.max_drops, "outlier_joints": float((cam >= 0).mean()),
                      "a_dlt": a, "b_robust_clean": b, "c_robust_outliers": c, "a_dlt_again": a2,
                      "ratio_b_over_a": b["us_median"] / a["us_median"], "ratio_c_over_a": c["us_median"] / a["us_median"]}))


if __name__ == "__main__":
    main()
