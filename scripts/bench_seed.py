#!/usr/bin/env python
"""What k_pair_cost and k_seed_group cost beside the default multi-person call on the same keypoints, and what the seeded association
buys on the recipes (a record for EXPERIMENTS.md, not a gate).

Workload: 10 000 frames x 133 joints on synth.ring_rig(C), 8 cameras x 4 detections and 4 cameras x 2, float32 keypoints,
device-resident; 1 px of noise, every camera's list permuted per frame, every detection free.  In ONE process, each launch between a
HIP event pair on one stream (snowtri_set_timing(ctx, 1)), (a), (b) and (c) in --repeats interleaved blocks of --launches launches
each (the ratio is that of the medians over all blocks; every block's is printed):
  (a) k_pair_cost      snowtri_pair_cost
  (b) the default call BatchTriangulator(method=PAIRWISE, pout_max=P).run_torch: the fused multi-person call, which visits the same
                       ray pairs (midpoints, scores, the greedy clustering, fusion)
  (c) k_seed_group     snowtri_seed_persons on (a)'s output, gate 0.05 m, min_views 3
Yardstick: (a) no longer than (b).  --recipes adds: refine_rig on pose_cases.recipe(P=2) with triangulate=seeded_triangulator(2, 0.05)
(view RMS of the nudged camera per round), and the RMS against the truth of triangulate_seeded on assign_cases.crossing().
Prints one JSON line per configuration.  Run it under a time limit of its own:  timeout -k 10 300 python scripts/bench_seed.py
"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def timings(args):
    import torch
    from snowmocap_amd import _lib, synth
    from snowmocap_amd.batch import BatchTriangulator

    F, J, thr = args.frames, 133, 3.0
    dev = torch.device("cuda", 0)
    for C, P in ((8, 4), (4, 2)):
        K, R, t = synth.ring_rig(C)
        rng = np.random.default_rng(300 + C)
        X = synth.make_people(rng, F, P, J=J)
        kp, npers = synth.make_keypoints(rng, K, R, t, X, pixel_sigma=1.0, score_range=(3.5, 8.0), permute_persons=True, dtype=np.float32)
        d_kp = torch.from_numpy(np.ascontiguousarray(kp)).to(dev)
        d_np = torch.from_numpy(np.ascontiguousarray(npers, dtype=np.int32)).to(dev)
        ctx = _lib.Context(K, R, t)
        prm = dict(synth.default_thresholds(), average_score_threshold=1.0, condense_distance_tol=0.3)    # (synth.config_workload(3): the README's 8 x 4)
        bt = BatchTriangulator(K, R, t, prm, pout_max=P, out_dtype=np.float32, method=_lib.PAIRWISE)
        out = bt.alloc_outputs(F, dev)
        for _ in range(args.warmup):
            ps, pn = ctx.pair_cost(d_kp, d_np, None, thr)
            ctx.seed_persons(ps, pn, d_np, None, S=P, gate=0.05)
            bt.run_torch(d_kp, d_np, out=out)
        torch.cuda.synchronize(dev)
        a, b, c, ratios = [], [], [], []
        for _ in range(args.repeats):                                                 # interleaved: the box drifts over a run
            ctx.set_timing(True)
            ai, ci = [], []
            for _ in range(args.launches):
                ps, pn = ctx.pair_cost(d_kp, d_np, None, thr)
                ai.append(ctx.last_kernel_ms()[0])
            for _ in range(args.launches):
                det, ns = ctx.seed_persons(ps, pn, d_np, None, S=P, gate=0.05)
                ci.append(ctx.last_kernel_ms()[0])
            ctx.set_timing(False)
            bt.ctx.set_timing(True)
            for _ in range(args.launches):
                bt.run_torch(d_kp, d_np, out=out)
            bi = bt.ctx.timing_collect()
            bt.ctx.set_timing(False)
            a, b, c = a + ai, b + bi, c + ci
            ratios.append(float(np.median(ai) / np.median(bi)))
        name_b = bt.ctx.last_kernel_names()
        found = float((ns == P).float().mean())
        bt.close()
        ctx.close()
        ratio = float(np.median(a) / np.median(b))
        print(json.dumps({"workload": f"{C}x{P}x{J}x{F} float32, device-resident", "device": torch.cuda.get_device_name(0),
                          "a_pair_cost": {"us_median": float(np.median(a)) * 1e3, "us_min": float(np.min(a)) * 1e3},
                          "b_default_call": {"kernels": name_b, "us_median": float(np.median(b)) * 1e3, "us_min": float(np.min(b)) * 1e3},
                          "c_seed_group": {"us_median": float(np.median(c)) * 1e3, "us_min": float(np.min(c)) * 1e3},
                          "frames_with_all_persons_seeded": found, "ratio_a_over_b": ratio, "ratio_per_repeat": [round(r, 4) for r in ratios],
                          "yardstick_a_within_b": "held" if ratio <= 1.0 else "missed"}), flush=True)
        del d_kp, out, ps, pn


def recipes():
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import assign_cases as ac
    import pose_cases as pc
    from snowmocap_amd import _lib, pose
    from snowmocap_amd import seed as sd
    r = pc.recipe(P=2)
    bad = r["bad"]
    rows = {}
    for name, tri in (("default", None), ("seeded", sd.seeded_triangulator(2, 0.05))):
        _, _, hist = pose.refine_rig(r["K"], r["Rd"], r["td"], r["kpts"], free=[bad], rounds=3, triangulate=tri)
        others = [c for c in range(r["K"].shape[0]) if c != bad]
        rows[name] = {"view_rms_px_of_the_nudged_camera": [round(float(h["view_rms"][bad]), 3) for h in hist],
                      "median_view_rms_px_of_the_others": [round(float(np.median(h["view_rms"][others])), 3) for h in hist],
                      "overflow_frames": [int(h["overflow_frames"]) for h in hist]}
    print(json.dumps({"recipe": "pose_cases.recipe(P=2), refine_rig rounds=3", **rows}), flush=True)
    cs = ac.crossing()
    ctx = _lib.Context(cs["K"], cs["R"], cs["t"])
    out = sd.triangulate_seeded(ctx, np.array(cs["kpts"]), np.array(cs["n_persons"]), None, S=3, gate=0.03, keypoint_score_threshold=ac.CROSS_THRESHOLD)
    ctx.close()
    det = out["seed_det_of"]
    truth = np.stack([[cs["X"][f, int(np.nonzero(cs["det_true"][f, 0] == det[f, 0, s])[0][0])] for s in range(3)] for f in range(ac.CROSS_F)])
    rms = float(np.sqrt(((out["xyzs"][..., :3] - truth) ** 2).sum(-1).mean()))
    print(json.dumps({"recipe": "assign_cases.crossing(), triangulate_seeded from no persons, gate 0.03", "frames_with_3_seeds": int((out["n_seeds"] == 3).sum()),
                      "rms_mm_against_the_truth": round(rms * 1e3, 3)}), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=10000)
    ap.add_argument("--launches", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--recipes", action="store_true")
    args = ap.parse_args()
    timings(args)
    if args.recipes:
        recipes()


if __name__ == "__main__":
    main()
