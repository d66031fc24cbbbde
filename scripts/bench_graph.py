#!/usr/bin/env python
"""What a hipGraph buys a caller that replays the fused call instead of launching it (a record for EXPERIMENTS.md, not a gate).

Workload: BASELINE configs[1] -- 4 cameras x 1 person x 133 joints x 10 000 frames (the floor rig), float32 in and out,
device-resident, k_fused_lean_coop.  K = 20 steps on one side stream, three ways in ONE process:
  (a) eager          a loop of K BatchTriangulator.run_torch calls
  (b) one graph      the K calls captured into one graph, one replay
  (c) K replays      one call captured, K replays of that graph
Each way is timed by ONE HIP event pair around the whole loop (no synchronise, no event inside it), after warm-up loops, `rounds`
times; the three ways alternate inside a round, so that clock drift falls on all of them alike.  Reported: the median, minimum and
maximum over the rounds of (loop time / K), in microseconds per step, host launch cost included -- which is the point.
The multi-person streaming route (stream_4x2) is left out: a capture of it is not among the verified ones (include/snowtri.h,
GRAPH CAPTURE).  Every graph is captured on one stream and is a linear chain.
Prints one JSON line.  Run it under a time limit of its own:  timeout -k 10 300 python scripts/bench_graph.py
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
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=5)
    args = ap.parse_args()
    import torch
    from snowmocap_amd import synth
    from snowmocap_amd.batch import BatchTriangulator

    F, K_STEPS = args.frames, args.steps
    wl = synth.config_workload(2, F, seed=5)
    K, R, t = wl["rig"]
    dev = torch.device("cuda", 0)
    kp, npers = torch.from_numpy(wl["kpts"]).to(dev), torch.from_numpy(wl["n_persons"]).to(dev)
    bt = BatchTriangulator(K, R, t, wl["params"], pout_max=1, out_dtype=np.float32)
    out = bt.alloc_outputs(F, dev)
    side = torch.cuda.Stream(device=dev)
    torch.cuda.synchronize(dev)

    def eager():
        for _ in range(K_STEPS):
            bt.run_torch(kp, npers, out=out)

    with torch.cuda.stream(side):
        eager()                                            # the warm-up call(s) a capture needs
    torch.cuda.synchronize(dev)
    name = bt.ctx.last_kernel_names()
    g_all, g_one = torch.cuda.CUDAGraph(), torch.cuda.CUDAGraph()
    with torch.cuda.graph(g_all, stream=side):
        eager()
    with torch.cuda.graph(g_one, stream=side):
        bt.run_torch(kp, npers, out=out)
    torch.cuda.synchronize(dev)

    def replays():
        for _ in range(K_STEPS):
            g_one.replay()

    ways = {"eager": eager, "one_graph_of_k_calls": g_all.replay, "k_replays_of_one_call": replays}
    us = {k: [] for k in ways}
    with torch.cuda.stream(side):
        for rnd in range(args.warmup + args.rounds):
            for k, fn in ways.items():
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record(side)
                fn()
                e1.record(side)
                e1.synchronize()
                if rnd >= args.warmup:
                    us[k].append(e0.elapsed_time(e1) * 1e3 / K_STEPS)
    torch.cuda.synchronize(dev)
    res = {k: {"us_per_step_median": float(np.median(v)), "us_per_step_min": float(np.min(v)), "us_per_step_max": float(np.max(v))}
           for k, v in us.items()}
    del g_all, g_one
    torch.cuda.synchronize(dev)
    bt.close()
    print(json.dumps({"workload": f"4x1x133x{F} float32, device-resident", "kernel": name, "device": torch.cuda.get_device_name(0),
                      "steps": K_STEPS, "rounds": args.rounds, **res}))


if __name__ == "__main__":
    main()
