#!/usr/bin/env python
"""What the Huber loss of refine_joints / refine_cameras costs beside the squared loss, and what it buys (a record for
EXPERIMENTS.md, not a gate).

TIMINGS, device-resident, float64 records and keypoints, each call between a torch event pair on one stream, the variants in
--repeats interleaved blocks of --launches calls each (the ratios are those of the medians over all blocks; every block's is printed):
  k_refine at iters = 4 on 10 000 frames x 133 joints, 4 x 1 (the floor rig) and 8 x 1 (synth.ring_rig(8)): squared and huber_px = 3,
  on clean detections (1 px of noise) and with one camera shifted by 20-150 px on 10 % of the joints (synth.add_outliers);
  snowtri_refine_cameras at iters = 1 (two evaluations of k_pose_normal and two k_pose_step) at 4 x 1 and 8 x 4, likewise.
  --parent-lib PATH: a build of the parent commit's library; its squared-loss calls are timed in the same blocks, so that the
  squared-loss instantiations of this build can be held against it inside the spread of the parent's own repeats.
The loss adds one fp64 sqrt, one division and two selects per view and evaluation to three divisions and about sixty fma; the ratio
has no target.

WHAT IT BUYS (--buys), on recipes, not footage: 80 frames x 1 person x 133 joints, 1 px of noise, add_outliers on 10 % of the joints,
4 and 8 cameras: the RMS error against the truth of DLT, DLT + refine_joints, DLT + refine_joints(huber_px = 3) and
DLT_ROBUST + refine_joints(views = its mask).
Prints one JSON line per measurement.  Run it under a time limit of its own:  timeout -k 10 400 python scripts/bench_huber.py
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
    ap.add_argument("--launches", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--huber-px", type=float, default=3.0)
    ap.add_argument("--parent-lib", default=None)
    ap.add_argument("--buys", action="store_true")
    args = ap.parse_args()
    import torch
    from snowmocap_amd import _lib, synth

    dev = torch.device("cuda", 0)
    J, delta = 133, args.huber_px
    to_dev = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)

    def parent_context(K, R, t):
        """A context of the parent commit's build (it has no _ex entries: they are left out of the binding table while it loads)."""
        if not args.parent_lib:
            return None
        keep = dict(_lib._SIGNATURES)
        for name in ("snowtri_refine_joints_ex", "snowtri_refine_cameras_ex"):
            _lib._SIGNATURES.pop(name)
        try:
            prev = _lib.use_library(os.path.abspath(args.parent_lib))
            ctx = _lib.Context(K, R, t)
        finally:
            _lib._SIGNATURES.clear()
            _lib._SIGNATURES.update(keep)
        _lib.use_library(prev)
        return ctx

    def timed(fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        e1.synchronize()
        return e0.elapsed_time(e1)

    def blocks(variants):
        """variants: {name: callable} -> {name: all times [ms]}, {name: the median of each block}"""
        for fn in variants.values():
            for _ in range(args.warmup):
                fn()
        torch.cuda.synchronize(dev)
        ms, per = {k: [] for k in variants}, {k: [] for k in variants}
        for _ in range(args.repeats):
            for k, fn in variants.items():
                got = [timed(fn) for _ in range(args.launches)]
                ms[k] += got
                per[k].append(float(np.median(got)))
        return ms, per

    def report(what, workload, ms, per):
        med = {k: float(np.median(v)) * 1e3 for k, v in ms.items()}
        row = {"what": what, "workload": workload, "device": torch.cuda.get_device_name(0), "huber_px": delta,
               "us_median": {k: round(v, 1) for k, v in med.items()}, "us_min": {k: round(float(np.min(v)) * 1e3, 1) for k, v in ms.items()},
               "us_block_medians": {k: [round(x * 1e3, 1) for x in v] for k, v in per.items()}}
        for tag in ("clean", "outliers"):
            if f"huber_{tag}" in med:
                row[f"ratio_huber_over_squared_{tag}"] = round(med[f"huber_{tag}"] / med[f"squared_{tag}"], 4)
            if f"parent_squared_{tag}" in med:
                p = np.array(per[f"parent_squared_{tag}"])
                row[f"squared_minus_parent_{tag}_us"] = round(med[f"squared_{tag}"] - med[f"parent_squared_{tag}"], 1)
                row[f"parent_block_spread_{tag}_us"] = round(float(p.max() - p.min()) * 1e3, 1)
        print(json.dumps(row), flush=True)

    def workload(C, P, F):
        K, R, t = synth.load_rig_json() if C == 4 else synth.ring_rig(C)
        rng = np.random.default_rng(200 + C + P)
        X = synth.make_people(rng, F, P, J=J)
        kp, npers = synth.make_keypoints(rng, K, R, t, X, pixel_sigma=1.0, score_range=(3.5, 8.0), dtype=np.float64)
        dirty = np.concatenate([synth.add_outliers(rng, np.ascontiguousarray(kp[:, :, p:p + 1]), fraction=0.1)[0] for p in range(P)], axis=2)
        rec = np.concatenate([X + rng.normal(0.0, 0.005, X.shape), np.ones(X.shape[:-1] + (1,))], axis=-1)
        return (K, R, t), rec, kp[..., :J, :], dirty[..., :J, :], X

    if not args.buys:
        for C in (4, 8):
            rig, rec, clean, dirty, _ = workload(C, 1, args.frames)
            ctx, old = _lib.Context(*rig), parent_context(*rig)
            x, kc, kd = to_dev(rec), to_dev(clean), to_dev(dirty)
            out = torch.empty_like(x)
            variants = {}
            for tag, k in (("clean", kc), ("outliers", kd)):
                variants[f"squared_{tag}"] = lambda k=k: ctx.refine_joints(x, k, keypoint_score_threshold=3.0, iters=4)
                variants[f"huber_{tag}"] = lambda k=k: ctx.refine_joints(x, k, keypoint_score_threshold=3.0, iters=4, huber_px=delta)
                if old is not None:
                    variants[f"parent_squared_{tag}"] = lambda k=k: old.refine_joints(x, k, keypoint_score_threshold=3.0, iters=4)
            report("k_refine, iters = 4", f"{C}x1x{J}x{args.frames} float64, device-resident", *blocks(variants))
            if old is not None:
                same = torch.equal(ctx.refine_joints(x, kd, keypoint_score_threshold=3.0, iters=4), old.refine_joints(x, kd, keypoint_score_threshold=3.0, iters=4))
                print(json.dumps({"what": "squared-loss records of this build and of the parent build", "cameras": C, "equal_bit_for_bit": bool(same)}))
                old.close()
            ctx.close()
            del x, kc, kd, out
        for C, P in ((4, 1), (8, 4)):
            rig, rec, clean, dirty, _ = workload(C, P, args.frames)
            ctx, old = _lib.Context(*rig), parent_context(*rig)
            x, kc, kd = to_dev(rec), to_dev(clean), to_dev(dirty)
            kw = dict(keypoint_score_threshold=3.0, iters=1, free=[1])
            variants = {}
            for tag, k in (("clean", kc), ("outliers", kd)):
                variants[f"squared_{tag}"] = lambda k=k: ctx.refine_cameras(x, k, **kw)
                variants[f"huber_{tag}"] = lambda k=k: ctx.refine_cameras(x, k, huber_px=delta, **kw)
                if old is not None:
                    variants[f"parent_squared_{tag}"] = lambda k=k: old.refine_cameras(x, k, **kw)
            report("snowtri_refine_cameras, iters = 1 (2 x k_pose_normal + 2 x k_pose_step)", f"{C}x{P}x{J}x{args.frames} float64, device-resident",
                   *blocks(variants))
            if old is not None:
                old.close()
            ctx.close()
            del x, kc, kd
        return

    from snowmocap_amd.batch import BatchTriangulator
    for C in (4, 8):
        (K, R, t), _, clean, dirty, X = workload(C, 1, 80)
        prm = dict(synth.default_thresholds(), keypoint_score_threshold=3.0, keypoint_num=J, center_point_index=0)
        rms = lambda rec: float(np.sqrt((np.linalg.norm(np.asarray(rec)[..., :3] - X, axis=-1) ** 2).mean()) * 1e3)
        row = {"what": "RMS error against the truth [mm]", "workload": f"{C}x1x{J}x80, 1 px, 10 % outlier joints", "huber_px": delta}
        for tag, kp in (("clean", clean), ("outliers", dirty)):
            kp = np.ascontiguousarray(kp)
            bt = BatchTriangulator(K, R, t, prm, pout_max=1, out_dtype=np.float64, method=_lib.DLT)
            dlt = bt.run_host(kp, None)["xyzs"]
            bt.close()
            bt = BatchTriangulator(K, R, t, prm, pout_max=1, out_dtype=np.float64, method=_lib.DLT_ROBUST, diagnostics=True)
            rob = bt.run_host(kp, None)
            bt.close()
            ctx = _lib.Context(K, R, t)
            sq = ctx.refine_joints(dlt, kp, keypoint_score_threshold=3.0, iters=8)
            hb, _, _, outl = ctx.refine_joints(dlt, kp, keypoint_score_threshold=3.0, iters=8, huber_px=delta, diagnostics=True)
            masked = ctx.refine_joints(rob["xyzs"], kp, views=rob["views"].reshape(80, 1, J), keypoint_score_threshold=3.0, iters=8)
            ctx.close()
            row[tag] = {"dlt": round(rms(dlt), 3), "dlt_refine": round(rms(sq), 3), "dlt_refine_huber": round(rms(hb), 3),
                        "dlt_robust": round(rms(rob["xyzs"]), 3), "dlt_robust_refine_views": round(rms(masked), 3),
                        "records_with_an_outlier_view": round(float((outl != 0).mean()), 4)}
        print(json.dumps(row), flush=True)


if __name__ == "__main__":
    main()
