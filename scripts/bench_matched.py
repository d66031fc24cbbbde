#!/usr/bin/env python
"""What k_dlt_matched costs beside k_dlt_robust on the same observations (a record for EXPERIMENTS.md, not a gate).

Workload: 10 000 frames x 133 joints on synth.ring_rig(C), 4 cameras x 2 persons and 8 cameras x 4 persons, float64 and float32 in
and out, device-resident; 1 px of noise, one camera shifted on 10 % of the joints (synth.add_outliers), every camera's list permuted
per frame.  In ONE process, each launch between a HIP event pair on one stream (snowtri_set_timing(ctx, 1)), (a) and (b) in
--repeats interleaved blocks of --launches launches each (the ratio is that of the medians over all blocks; every block's is printed):
  (a) k_dlt_matched       snowtri_triangulate_matched through det_of (the inverse of the permutation)
  (b) k_dlt_robust        snowtri_triangulate_robust on the PRE-GATHERED F * P single-person frames [F * P, C, 1, 133, 3]
  (c) k_reproject_cost    the step that precedes the matching, on (a)'s records (torch events)
Yardstick: (a) no longer than 1.10 x (b) -- twice the 5 % box-to-box spread, for the det_of reads.  Prints one JSON line per
configuration.  Run it under a time limit of its own:  timeout -k 10 300 python scripts/bench_matched.py
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
    ap.add_argument("--launches", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--repeats", type=int, default=5)
    args = ap.parse_args()
    import torch
    from snowmocap_amd import _lib, synth
    from snowmocap_amd.batch import BatchTriangulator

    F, J, thr, tau, md = args.frames, 133, 3.0, 6.0, 1
    dev = torch.device("cuda", 0)
    for C, P in ((4, 2), (8, 4)):
        K, R, t = synth.ring_rig(C)
        rng = np.random.default_rng(100 + C)
        X = synth.make_people(rng, F, P, J=J)
        kp, npers = synth.make_keypoints(rng, K, R, t, X, pixel_sigma=1.0, score_range=(3.5, 8.0), dtype=np.float64)
        kp = np.concatenate([synth.add_outliers(rng, np.ascontiguousarray(kp[:, :, p:p + 1]), fraction=0.1)[0] for p in range(P)], axis=2)
        perm = np.argsort(rng.random((F, C, P)), axis=-1)                         # position i of a list holds person perm[i]
        listed = np.take_along_axis(kp, perm[..., None, None], axis=2)
        det_of = np.argsort(perm, axis=-1).astype(np.int32)
        singles = np.ascontiguousarray(np.moveaxis(kp, 2, 1).reshape(F * P, C, 1, J, 3))
        for dtype in (np.float64, np.float32):
            d_kp = torch.from_numpy(np.ascontiguousarray(listed.astype(dtype))).to(dev)
            d_det, d_np = torch.from_numpy(det_of).to(dev), torch.from_numpy(np.ascontiguousarray(npers, dtype=np.int32)).to(dev)
            d_single = torch.from_numpy(singles.astype(dtype)).to(dev)
            ctx = _lib.Context(K, R, t)
            prm = dict(synth.default_thresholds(), keypoint_score_threshold=thr, keypoint_num=J, center_point_index=0)
            bt = BatchTriangulator(K, R, t, prm, pout_max=1, out_dtype=dtype, method=_lib.DLT_ROBUST, reproj_threshold_px=tau, max_drops=md)
            out = bt.alloc_outputs(F * P, dev)
            for _ in range(args.warmup):
                ctx.triangulate_matched(d_kp, d_det, d_np, thr, tau, md, dtype=dtype)
                bt.run_torch(d_single, None, out=out)
            torch.cuda.synchronize(dev)
            a, b, ratios = [], [], []
            for _ in range(args.repeats):                                             # (a) and (b) interleaved: the box drifts over a run
                ctx.set_timing(True)
                ai = []
                for _ in range(args.launches):
                    xyzs, _ = ctx.triangulate_matched(d_kp, d_det, d_np, thr, tau, md, dtype=dtype)
                    ai.append(ctx.last_kernel_ms()[0])
                name_a = ctx.last_kernel_names()
                ctx.set_timing(False)
                bt.ctx.set_timing(True)
                for _ in range(args.launches):
                    bt.run_torch(d_single, None, out=out)
                bi = bt.ctx.timing_collect()
                bt.ctx.set_timing(False)
                a, b = a + ai, b + bi
                ratios.append(float(np.median(ai) / np.median(bi)))
            name_b = bt.ctx.last_kernel_names()
            same = bool(torch.equal(out["xyzs"].view(F, P, J, 4), xyzs))
            bt.close()
            c = []
            for i in range(args.warmup + args.launches):
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                ctx.reproject_cost(xyzs, d_kp, n_persons=d_np, keypoint_score_threshold=thr)
                e1.record()
                e1.synchronize()
                if i >= args.warmup:
                    c.append(e0.elapsed_time(e1))
            ctx.close()
            ratio = float(np.median(a) / np.median(b))
            print(json.dumps({"workload": f"{C}x{P}x{J}x{F} {np.dtype(dtype).name}, device-resident", "device": torch.cuda.get_device_name(0),
                              "a_matched": {"kernel": name_a, "us_median": float(np.median(a)) * 1e3, "us_min": float(np.min(a)) * 1e3},
                              "b_robust_pregathered": {"kernel": name_b, "us_median": float(np.median(b)) * 1e3, "us_min": float(np.min(b)) * 1e3},
                              "c_reproject_cost": {"us_median": float(np.median(c)) * 1e3, "us_min": float(np.min(c)) * 1e3},
                              "records_equal_bit_for_bit": same, "ratio_a_over_b": ratio, "ratio_per_repeat": [round(r, 4) for r in ratios],
                              "yardstick_1.10": "held" if ratio <= 1.10 else "missed"}))
            del d_kp, d_single, xyzs, out


if __name__ == "__main__":
    main()
