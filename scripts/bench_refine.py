#!/usr/bin/env python3
"""GPU box: k_refine (snowtri_refine_joints) on a device-resident batch of 10 000 frames x 133 joints at 4 x 1 (the floor rig) and
8 x 1 (synth.ring_rig(8)), one person in the middle, exact projections + N(0, 1 px), beside k_dlt_robust with max_drops = 0 on the
SAME keypoints in the same process: that kernel reads the same observations and writes the same records, and does one 4 x 4 solve
plus C reprojections per joint, so its time is the yardstick k_refine at iters = 4 is aimed at.  The start of the refinement is that
kernel's output: the DLT point of the same batch.

  - HIP events around single launches queued back to back, median of --calls launches per round after a warm-up, all kernels
    measured in alternating rounds;
  - records and keypoints float64 and float32; iters = 1, 2, 4, 8 (how the time grows with iters tells VALU-bound from memory-bound:
    the bytes do not depend on iters);
  - GB/s against the algorithmic bytes: k_refine one read of xyzs and of the C observations of a record + one write of xyzs;
    k_dlt_robust one read of the observations + one write of the record, its view mask and its residual;
  - the result is compared with the NumPy rule on the first 2 frames.

    python scripts/bench_refine.py [--frames=N] [--calls=N] [--rounds=N]
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
from snowmocap_amd import refine as rf
from snowmocap_amd.batch import BatchTriangulator


def arg(name, default):
    return ([int(a.split("=")[1]) for a in sys.argv if a.startswith(f"--{name}=")] or [default])[0]


F, CALLS, ROUNDS = arg("frames", 10000), arg("calls", 10), arg("rounds", 3)
KN = 133
ITERS = (1, 2, 4, 8)


def event_ms(fn, calls):
    """durations of `calls` single launches, each between its own event pair, queued back to back"""
    pairs = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(calls)]
    for a, b in pairs:
        a.record()
        fn()
        b.record()
    torch.cuda.synchronize()
    return [a.elapsed_time(b) for a, b in pairs]


def workload(C, dev):
    """-> K, R, t, kpts [F, C, 1, KN, 3] float64 CUDA tensor (the projections of one person in a 0.6 x 0.6 x 1.8 m box + N(0, 1 px),
    scores U(3.5, 8))."""
    K, R, t = synth.load_rig_json() if C == 4 else synth.ring_rig(C)
    g = torch.Generator(device=dev)
    g.manual_seed(20 + C)
    box = torch.tensor([0.6, 0.6, 1.8], dtype=torch.float64, device=dev)
    off = torch.tensor([0.5, 0.5, 0.0], dtype=torch.float64, device=dev)
    X = (torch.rand((F, KN, 3), generator=g, dtype=torch.float64, device=dev) - off) * box
    kp = torch.empty((F, C, 1, KN, 3), dtype=torch.float64, device=dev)
    for c in range(C):
        pc = (X - torch.from_numpy(t[c]).to(dev)) @ torch.from_numpy(np.ascontiguousarray(R[c])).to(dev)       # R^T (X - t)
        pix = (pc / pc[..., 2:3]) @ torch.from_numpy(np.ascontiguousarray(K[c].T)).to(dev)
        kp[:, c, 0, :, :2] = pix[..., :2] + torch.randn((F, KN, 2), generator=g, dtype=torch.float64, device=dev)
    kp[..., 2] = 3.5 + 4.5 * torch.rand((F, C, 1, KN), generator=g, dtype=torch.float64, device=dev)
    return K, R, t, kp


def main():
    dev = torch.device("cuda", 0)
    params = synth.default_thresholds()
    params.update(keypoint_num=KN, center_point_index=18)
    tdt = {"float64": torch.float64, "float32": torch.float32}
    thr = float(params["keypoint_score_threshold"])
    runs, check = {}, {}
    keep = []
    st = ct.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
    p = lambda a: ct.c_void_p(a.data_ptr())     # noqa: E731
    for C in (4, 8):
        K, R, t, kp64 = workload(C, dev)
        for dt in ("float64", "float32"):
            kp = kp64.to(tdt[dt]).contiguous()
            bt = BatchTriangulator(K, R, t, params, pout_max=1, out_dtype=np.dtype(dt), method=_lib.DLT_ROBUST, diagnostics=True, max_drops=0)
            tri = bt.alloc_outputs(F, dev)
            bt.run_torch(kp, None, out=tri)
            torch.cuda.synchronize()
            assert bool((tri["count"] == 1).all())
            start = tri["xyzs"].clone()
            out = torch.empty_like(start)
            tag = f"{C}x1_{dt}"
            runs[f"dlt_robust0_{tag}"] = lambda bt=bt, kp=kp, tri=tri: bt.run_torch(kp, None, out=tri)
            code = _lib.F64 if dt == "float64" else _lib.F32

            def refine(it, bt=bt, start=start, kp=kp, out=out, code=code):      # (the C entry itself: no allocation between the events)
                _lib.check(bt.ctx.L.snowtri_refine_joints(bt.ctx.handle, F, 1, KN, p(start), code, 1, p(kp), code, None, None, None, thr, it, 0,
                                                          p(out), None, None, _lib.DEVICE, st), "snowtri_refine_joints")
            for it in ITERS:
                runs[f"refine{it}_{tag}"] = lambda it=it, refine=refine: refine(it)
            check[tag] = (K, R, t, bt, start, kp)
            keep.append((bt, tri, out))
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
    worst, moved, classes_ok = 0.0, {}, True
    for tag, (K, R, t, bt, start, kp) in check.items():
        got, cost, codes = bt.ctx.refine_joints(start, kp, keypoint_score_threshold=thr, iters=4, diagnostics=True)
        torch.cuda.synchronize()
        moved[tag] = round(float((codes == rf.REFINE_MOVED).double().mean()), 4)
        assert bool((cost[..., 1] <= cost[..., 0]).all())
        ref, _, rcodes = rf.refine_joints_reference(K, R, t, start[:2].cpu().numpy(), kp[:2].cpu().numpy(), keypoint_score_threshold=thr, iters=4)
        classes_ok = classes_ok and bool(np.array_equal(codes[:2].cpu().numpy(), rcodes))
        if tag.endswith("float64"):
            worst = max(worst, float(np.abs(got[:2].cpu().numpy() - ref).max()))

    def esz(k):
        return 8 if "float64" in k else 4

    def bytes_of(k):
        C = int(k.split("_")[-2][0])
        n = F * KN
        if k.startswith("dlt_robust0"):
            return n * (3 * esz(k) * C + 4 * esz(k) + 4 + esz(k))
        return n * (3 * esz(k) * C + 2 * 4 * esz(k))

    gbps = {k: bytes_of(k) / med[k] * 1e-6 for k in med}
    tags = list(check)
    ratio = {tag: round(med[f"refine4_{tag}"] / med[f"dlt_robust0_{tag}"], 3) for tag in tags}
    line = dict(what="refine", frames=F, joints=KN, records=F * KN, calls_per_kernel=CALLS * ROUNDS,
                max_m_vs_numpy_rule_first_frames=worst, classes_equal_numpy_rule_first_frames=classes_ok, moved_fraction=moved,
                ms_median={k: round(v, 4) for k, v in med.items()}, ms_min={k: round(float(min(v)), 4) for k, v in ms.items()},
                GBps={k: round(v, 1) for k, v in gbps.items()}, refine4_over_dlt_robust0=ratio,
                refine4_within_dlt_robust0=all(v <= 1.0 for v in ratio.values()),
                ms_per_extra_iter={tag: round((med[f"refine8_{tag}"] - med[f"refine4_{tag}"]) / 4.0, 4) for tag in tags},
                ms_at_zero_iters_extrapolated={tag: round(2.0 * med[f"refine1_{tag}"] - med[f"refine2_{tag}"], 4) for tag in tags})
    print(json.dumps(line))
    if worst > 1e-7 or not classes_ok:
        sys.exit("the refinement differs from the NumPy rule")


if __name__ == "__main__":
    main()
