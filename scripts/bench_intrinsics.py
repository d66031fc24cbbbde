#!/usr/bin/env python3
"""GPU box: camera refinement with intrinsics (snowtri_refine_cameras_k: k_pose_normal_k + k_pose_step_k) beside the pose-only entry
(snowtri_refine_cameras: k_pose_normal + k_pose_step) on scripts/bench_pose.py's workload: a device-resident batch of 10 000 frames x
133 joints, float64, at 4 x 1 (the floor rig, one person) and 8 x 4 (synth.ring_rig(8), four persons), the joints exact, the
detections their projections + N(0, 1 px), every camera free, off by 0.5 degrees / 2 cm and with fx, fy 2 % high and the centre off
by (8, -5) px.

  - HIP events around single calls queued back to back, median of --calls calls per block, every kernel measured in --blocks
    interleaved blocks; per figure the median over all calls and the medians of the blocks (their spread is
    what a difference between two builds has to exceed);
  - ONE evaluation = call(iters = 2) - call(iters = 1), where every camera is still moving (no block is skipped); (1) the
    ten-parameter evaluation beside the pose-only one in the same run, and the ratio of their fp64 operation counts per
    observation (FLOPS_POSE, FLOPS_INTR below, tallied from pose_add_obs and pose_add_obs_k);
  - (2) with --parent-lib=PATH (a build of the parent commit, `make OUT=...` in a checkout of it) the pose-only call of that build in
    the same blocks: the pose-only kernels are untouched, so the two must agree within the block-to-block spread;
  - (3) a whole call at iters = 4, both entries;
  - the ten-parameter sums are compared with the NumPy rule on the first 4 frames.

    python scripts/bench_intrinsics.py [--frames=N] [--calls=N] [--blocks=N] [--parent-lib=PATH]
Prints one JSON line; the figures go into EXPERIMENTS.md.
"""
import ctypes as ct
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch

from snowmocap_amd import _lib, pose

import bench_pose as bp


def arg(name, default, kind=int):
    return ([kind(a.split("=", 1)[1]) for a in sys.argv if a.startswith(f"--{name}=")] or [default])[0]


F, CALLS, BLOCKS, PARENT = arg("frames", 10000), arg("calls", 10), arg("blocks", 5), arg("parent-lib", "", str)
bp.F = F
KN = bp.KN
SHAPES = bp.SHAPES
# fp64 VALU arithmetic per observation, fma, multiply and add each counted once, the four divisions (1 / pc2 of rule 1, x, y and
# 1 / pc2 of the evaluation) left out of both: rule 1's projection 17; the evaluation's projection, residual and E 31; the six pose
# columns 18 (three cross products) + 24 (dx, dy) + 18 (du, dv); w du, w dv 12; g 12; the 6 x 6 block of H 42 -> 174 in
# pose_add_obs' kernel.  pose_add_obs_k adds w x, w y 2; g 4; rows 6..9 against the pose columns 24; fx.fx, fy.fy 2; three plain
# adds (cx.fx, cy.fy, cx.cx) -> 209
FLOPS_POSE, FLOPS_INTR = 174, 209


def main():
    dev = torch.device("cuda", 0)
    st = ct.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
    p = lambda a: ct.c_void_p(a.data_ptr())     # noqa: E731
    parent = None
    if PARENT:
        _lib.lib()                                # (torch's HIP runtime first, as _lib arranges it)
        parent = ct.CDLL(PARENT)
        for name in ("snowtri_ctx_create", "snowtri_ctx_destroy", "snowtri_refine_cameras"):
            getattr(parent, name).restype, getattr(parent, name).argtypes = _lib._SIGNATURES[name]
    runs, check, keep = {}, {}, []
    for C, P in SHAPES:
        K, R, t, Rd, td, rec, kp = bp.workload(C, P, dev)
        Kd = np.array(K, dtype=np.float64, copy=True)
        Kd[:, 0, 0] *= 1.02
        Kd[:, 1, 1] *= 1.02
        Kd[:, 0, 2] += 8.0
        Kd[:, 1, 2] -= 5.0
        ctx = _lib.Context(Kd, Rd, td)
        tag = f"{C}x{P}"
        Ko = torch.empty((C, 3, 3), dtype=torch.float64, device=dev)
        Ro = torch.empty((C, 3, 3), dtype=torch.float64, device=dev)
        to = torch.empty((C, 3), dtype=torch.float64, device=dev)
        cost = torch.empty((C, 2), dtype=torch.float64, device=dev)
        codes = torch.empty((C,), dtype=torch.uint8, device=dev)
        mask = (1 << C) - 1

        def cameras(it, L=ctx.L, h=ctx.handle, rec=rec, kp=kp, Ro=Ro, to=to, cost=cost, codes=codes, P=P, mask=mask):
            _lib.check(L.snowtri_refine_cameras(h, F, P, KN, p(rec), _lib.F64, P, p(kp), _lib.F64, None, None, None, 0.5, mask, 64, it, 0,
                                                p(Ro), p(to), p(cost), None, p(codes), None, _lib.DEVICE, st), "snowtri_refine_cameras")

        def cameras_k(it, ctx=ctx, rec=rec, kp=kp, Ko=Ko, Ro=Ro, to=to, cost=cost, codes=codes, P=P, mask=mask):
            _lib.check(ctx.L.snowtri_refine_cameras_k(ctx.handle, F, P, KN, p(rec), _lib.F64, P, p(kp), _lib.F64, None, None, None, 0.5, mask, mask, 3,
                                                      64, it, 0, 0.0, p(Ko), p(Ro), p(to), p(cost), None, p(codes), None, None, _lib.DEVICE, st),
                       "snowtri_refine_cameras_k")
        for it in (1, 2, 4):
            runs[f"pose{it}_{tag}"] = lambda it=it, f=cameras: f(it)
            runs[f"intr{it}_{tag}"] = lambda it=it, f=cameras_k: f(it)
        if parent is not None:
            h = ct.c_void_p()
            Kc, Rc, tc = (np.ascontiguousarray(a, dtype=np.float64) for a in (Kd, Rd, td))
            _lib.check(parent.snowtri_ctx_create(C, _lib.ptr(Kc), _lib.ptr(Rc), _lib.ptr(tc), 0, ct.byref(h)), "parent snowtri_ctx_create")
            for it in (1, 2, 4):
                runs[f"parent{it}_{tag}"] = lambda it=it, f=cameras, h=h: f(it, L=parent, h=h)
            keep.append(h)
        check[tag] = (Kd, Rd, td, ctx, rec, kp, cost, codes, C, P)
        keep.append((ctx, rec, kp, Ko, Ro, to))
    for fn in runs.values():
        for _ in range(2):
            fn()
    torch.cuda.synchronize()
    ms = {k: [] for k in runs}
    # interleaved blocks: drift hits every kernel alike.  The pose-only calls of the two builds are neighbours and every other block
    # runs in reverse order, so each of them follows the other as often as it precedes it; the ten-parameter calls, which draw more
    # power, come last and follow each other.
    order = sorted((k for k in runs if not k.startswith("intr")), key=lambda k: (k.split("_")[1], int(k.split("_")[0][-1]), k)) + [k for k in runs if k.startswith("intr")]
    for b in range(BLOCKS):
        for k in (order[::-1] if b & 1 else order):
            ms[k].append(bp.event_ms(runs[k], CALLS))
    med = {k: float(np.median(np.concatenate(v))) for k, v in ms.items()}
    blocks = {k: [round(float(np.median(b)), 4) for b in v] for k, v in ms.items()}

    worst, all_moved = 0.0, True
    for tag, (Kd, Rd, td, ctx, rec, kp, cost, codes, C, P) in check.items():
        runs[f"intr2_{tag}"]()
        torch.cuda.synchronize()
        all_moved = all_moved and bool((codes == pose.POSE_MOVED).all()) and bool((cost[:, 1] < cost[:, 0]).all())
        rep = ctx.refine_cameras(rec[:4].contiguous(), kp[:4].contiguous(), keypoint_score_threshold=0.5, iters=1, diagnostics=True, intrinsics="fc")[3]
        ref = pose.refine_cameras_reference(Kd, Rd, td, rec[:4].cpu().numpy(), kp[:4].cpu().numpy(), keypoint_score_threshold=0.5, iters=1,
                                            intrinsics="fc")[3]
        assert np.array_equal(rep["n_obs"].cpu().numpy(), ref["n_obs"]) and int(ref["n_obs"][0]) == 4 * P * KN
        scale = np.abs(ref["normal"]).max(axis=0)
        worst = max(worst, float((np.abs(rep["normal"].cpu().numpy() - ref["normal"]) / np.where(scale > 0, scale, 1.0)).max()))

    tags = list(check)
    one = {w: {tag: med[f"{w}2_{tag}"] - med[f"{w}1_{tag}"] for tag in tags} for w in (("pose", "intr") + (("parent",) if parent else ()))}
    one_blocks = {w: {tag: [round(b2 - b1, 4) for b1, b2 in zip(blocks[f"{w}1_{tag}"], blocks[f"{w}2_{tag}"])] for tag in tags} for w in one}
    line = dict(what="intrinsics", build_variants=_lib.build_info()["variants"], frames=F, joints=KN, shapes=tags, calls_per_kernel=CALLS * BLOCKS,
                max_rel_normal_vs_numpy_rule_first_frames=worst, every_camera_moved_at_iters_2=all_moved,
                ms_median={k: round(v, 4) for k, v in med.items()}, ms_block_medians=blocks,
                ms_one_evaluation={w: {tag: round(v, 4) for tag, v in d.items()} for w, d in one.items()}, ms_one_evaluation_blocks=one_blocks,
                intr_over_pose_one_evaluation={tag: round(one["intr"][tag] / one["pose"][tag], 3) for tag in tags},
                intr_over_pose_flops_tally=round(FLOPS_INTR / FLOPS_POSE, 3),
                intr_over_pose_call_iters_4={tag: round(med[f"intr4_{tag}"] / med[f"pose4_{tag}"], 3) for tag in tags})
    if parent:
        line["pose_call_iters_4_over_parent"] = {tag: round(med[f"pose4_{tag}"] / med[f"parent4_{tag}"], 4) for tag in tags}
        line["pose_block_spread_iters_4"] = {tag: round(max(blocks[f"pose4_{tag}"]) / min(blocks[f"pose4_{tag}"]), 4) for tag in tags}
        line["parent_block_spread_iters_4"] = {tag: round(max(blocks[f"parent4_{tag}"]) / min(blocks[f"parent4_{tag}"]), 4) for tag in tags}
        for h in keep:
            if isinstance(h, ct.c_void_p):
                parent.snowtri_ctx_destroy(h)
    print(json.dumps(line))
    if worst > 1e-9 or not all_moved:
        sys.exit("the refinement with intrinsics differs from the NumPy rule")


if __name__ == "__main__":
    main()
