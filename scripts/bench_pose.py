#!/usr/bin/env python3
"""GPU box: camera pose refinement (snowtri_refine_cameras: k_pose_normal + k_pose_step) on a device-resident batch of 10 000 frames x
133 joints at 4 x 1 (the floor rig, one person) and 8 x 4 (synth.ring_rig(8), four persons on the 1.5 m circle), the joints exact,
the detections their projections + N(0, 1 px), every camera free and off by 0.5 degrees / 2 cm, beside k_reproject with float64
pixels on the SAME records in the same process: that kernel reads the same records and computes the same projections, and writes
every pixel where an evaluation writes almost nothing, so its time is the yardstick ONE evaluation is aimed at.

  - HIP events around single calls queued back to back, median of --calls calls per round after a warm-up, all kernels measured in
    alternating rounds;
  - a call at iters = n is n + 1 evaluations (2 (n + 1) launches): ONE evaluation = call(iters = 2) - call(iters = 1), where every
    camera is still moving (no block is skipped); the whole call at iters = 4 is reported beside it;
  - records and keypoints float64 and float32;
  - GB/s of an evaluation against its algorithmic bytes: per camera one read of its observations, and the records once;
  - the sums are compared with the NumPy rule on the first 4 frames.

    python scripts/bench_pose.py [--frames=N] [--calls=N] [--rounds=N]
Prints one JSON line; the figures go into EXPERIMENTS.md.  With SNOWTRI_LIB pointing at a development build
(`make OUT=ab/libsnowtri_pose_rec.so EXTRA="-DSNOWTRI_DEV_EXPERIMENTS -DSNOWTRI_POSE_PER_RECORD"`) the same script measures the kernel
shape that lost, k_pose_normal_rec; `build_variants` in the line says which build ran.
"""
import ctypes as ct
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch

from snowmocap_amd import _lib, pose, synth


def arg(name, default):
    return ([int(a.split("=")[1]) for a in sys.argv if a.startswith(f"--{name}=")] or [default])[0]


F, CALLS, ROUNDS = arg("frames", 10000), arg("calls", 10), arg("rounds", 3)
KN = 133
SHAPES = ((4, 1), (8, 4))                                   # (cameras, persons)


def event_ms(fn, calls):
    """durations of `calls` single calls, each between its own event pair, queued back to back"""
    pairs = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(calls)]
    for a, b in pairs:
        a.record()
        fn()
        b.record()
    torch.cuda.synchronize()
    return [a.elapsed_time(b) for a, b in pairs]


def workload(C, P, dev):
    """-> K, R, t (the truth), Rd, td (every camera off by 0.5 degrees / 2 cm), records [F, P, KN, 4] and kpts [F, C, P, KN, 3] float64
    CUDA tensors (score 1; the projections of the records + N(0, 1 px))."""
    K, R, t = synth.load_rig_json() if C == 4 else synth.ring_rig(C)
    g = torch.Generator(device=dev)
    g.manual_seed(40 + C)
    box = torch.tensor([0.6, 0.6, 1.8], dtype=torch.float64, device=dev)
    off = torch.tensor([0.5, 0.5, 0.0], dtype=torch.float64, device=dev)
    centres = torch.from_numpy(synth.person_centres(P)).to(dev)
    X = (torch.rand((F, P, KN, 3), generator=g, dtype=torch.float64, device=dev) - off) * box + centres[None, :, None, :]
    kp = torch.ones((F, C, P, KN, 3), dtype=torch.float64, device=dev)
    for c in range(C):
        pc = (X - torch.from_numpy(t[c]).to(dev)) @ torch.from_numpy(np.ascontiguousarray(R[c])).to(dev)       # R^T (X - t)
        pix = (pc / pc[..., 2:3]) @ torch.from_numpy(np.ascontiguousarray(K[c].T)).to(dev)
        kp[:, c, :, :, :2] = pix[..., :2] + torch.randn((F, P, KN, 2), generator=g, dtype=torch.float64, device=dev)
    rec = torch.cat([X, torch.ones((F, P, KN, 1), dtype=torch.float64, device=dev)], dim=-1).contiguous()
    rng = np.random.default_rng(40 + C)
    Rd, td = np.array(R, copy=True), np.array(t, copy=True)
    for c in range(C):
        axis, way = rng.normal(size=3), rng.normal(size=3)
        Rd[c] = pose.rodrigues(axis / np.linalg.norm(axis) * np.deg2rad(0.5)) @ R[c]
        td[c] = t[c] + way / np.linalg.norm(way) * 0.02
    return K, R, t, Rd, td, rec, kp


def main():
    dev = torch.device("cuda", 0)
    tdt = {"float64": torch.float64, "float32": torch.float32}
    runs, check, keep = {}, {}, []
    st = ct.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
    p = lambda a: ct.c_void_p(a.data_ptr())     # noqa: E731
    for C, P in SHAPES:
        K, R, t, Rd, td, rec64, kp64 = workload(C, P, dev)
        for dt in ("float64", "float32"):
            rec, kp = rec64.to(tdt[dt]).contiguous(), kp64.to(tdt[dt]).contiguous()
            ctx = _lib.Context(K, Rd, td)
            code = _lib.F64 if dt == "float64" else _lib.F32
            tag = f"{C}x{P}_{dt}"
            Ro = torch.empty((C, 3, 3), dtype=torch.float64, device=dev)
            to = torch.empty((C, 3), dtype=torch.float64, device=dev)
            cost = torch.empty((C, 2), dtype=torch.float64, device=dev)
            codes = torch.empty((C,), dtype=torch.uint8, device=dev)
            pix = torch.empty((F, C, P, KN, 3), dtype=torch.float64, device=dev)
            mask = (1 << C) - 1

            def cameras(it, ctx=ctx, rec=rec, kp=kp, code=code, Ro=Ro, to=to, cost=cost, codes=codes, P=P, mask=mask):   # (the C entry itself: no allocation between the events)
                _lib.check(ctx.L.snowtri_refine_cameras(ctx.handle, F, P, KN, p(rec), code, P, p(kp), code, None, None, None, 0.5, mask, 64, it, 0,
                                                        p(Ro), p(to), p(cost), None, p(codes), None, _lib.DEVICE, st), "snowtri_refine_cameras")

            def reproject(ctx=ctx, rec=rec, code=code, pix=pix, P=P):
                _lib.check(ctx.L.snowtri_reproject(ctx.handle, F, P, KN, p(rec), code, 0, p(pix), _lib.F64, _lib.DEVICE, st), "snowtri_reproject")
            for it in (1, 2, 4):
                runs[f"pose{it}_{tag}"] = lambda it=it, cameras=cameras: cameras(it)
            runs[f"reproject_{tag}"] = reproject
            check[tag] = (K, Rd, td, ctx, rec, kp, cost, codes, C, P)
            keep.append((ctx, rec, kp, Ro, to, pix))
    for fn in runs.values():
        for _ in range(2):
            fn()
    torch.cuda.synchronize()
    ms = {k: [] for k in runs}
    for _ in range(ROUNDS):                                  # alternating rounds: drift hits every kernel alike
        for k, fn in runs.items():
            ms[k] += event_ms(fn, CALLS)
    med = {k: float(np.median(v)) for k, v in ms.items()}

    # every camera moved at iters = 2 and lowered its cost (so no block was skipped in the evaluations timed); the sums against the
    # NumPy rule on the first frames
    worst, all_moved = 0.0, True
    for tag, (K, Rd, td, ctx, rec, kp, cost, codes, C, P) in check.items():
        runs[f"pose2_{tag}"]()
        torch.cuda.synchronize()
        all_moved = all_moved and bool((codes == pose.POSE_MOVED).all()) and bool((cost[:, 1] < cost[:, 0]).all())
        _, _, rep = ctx.refine_cameras(rec[:4].contiguous(), kp[:4].contiguous(), keypoint_score_threshold=0.5, iters=1, diagnostics=True)
        ref = pose.refine_cameras_reference(K, Rd, td, rec[:4].cpu().numpy(), kp[:4].cpu().numpy(), keypoint_score_threshold=0.5, iters=1)[2]
        assert np.array_equal(rep["n_obs"].cpu().numpy(), ref["n_obs"]) and int(ref["n_obs"][0]) == 4 * P * KN
        scale = np.abs(ref["normal"]).max(axis=0)
        worst = max(worst, float((np.abs(rep["normal"].cpu().numpy() - ref["normal"]) / scale).max()))

    def esz(k):
        return 8 if "float64" in k else 4

    def eval_bytes(k):
        C, P = (int(v) for v in k.split("_")[-2].split("x"))
        return F * P * KN * (3 * esz(k) * C + 4 * esz(k))

    tags = list(check)
    one = {tag: med[f"pose2_{tag}"] - med[f"pose1_{tag}"] for tag in tags}
    ratio = {tag: round(one[tag] / med[f"reproject_{tag}"], 3) for tag in tags}
    line = dict(what="pose", build_variants=_lib.build_info()["variants"], frames=F, joints=KN, shapes=[f"{C}x{P}" for C, P in SHAPES], calls_per_kernel=CALLS * ROUNDS,
                max_rel_normal_vs_numpy_rule_first_frames=worst, every_camera_moved_at_iters_2=all_moved,
                ms_median={k: round(v, 4) for k, v in med.items()}, ms_min={k: round(float(min(v)), 4) for k, v in ms.items()},
                ms_one_evaluation={tag: round(v, 4) for tag, v in one.items()},
                ms_one_evaluation_from_iters_4={tag: round((med[f"pose4_{tag}"] - med[f"pose2_{tag}"]) / 2.0, 4) for tag in tags},
                GBps_one_evaluation={tag: round(eval_bytes(f"x_{tag}") / one[tag] * 1e-6, 1) for tag in tags},
                one_evaluation_over_reproject=ratio, one_evaluation_within_reproject=all(v <= 1.0 for v in ratio.values()))
    print(json.dumps(line))
    if worst > 1e-9 or not all_moved:
        sys.exit("the pose refinement differs from the NumPy rule")


if __name__ == "__main__":
    main()
