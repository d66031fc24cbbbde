#!/usr/bin/env python3
"""GPU box: the one-to-one assignment (snowtri_assign_detections, k_assign) on device-resident costs that k_reproject_cost wrote, on
the synthetic multi-person recipe -- synth.ring_rig(8), P persons on the 1.5 m circle, 133 joints uniform in a 0.6 x 0.6 x 1.8 m box
around each centre, detections = exact projections + N(0, 1 px) with confidences U(3.5, 8) in a per-(frame, camera) permuted order,
the 3D records = the truth + N(0, 1 cm) -- for 10 000 frames x 8 cameras at P = Pmax = 4 and P = Pmax = 16 (80 000 problems each).

  - beside k_assign, in the same run on the same tensors: (a) k_reproject_cost, the stage that feeds it, and (b) the torch
    match_detections it replaces (one call = its dozen of tensor kernels);
  - HIP events around single calls queued back to back, median of --calls calls per round after a warm-up, the three measured in
    alternating rounds;
  - the yardstick at 4 x 4: k_assign takes no longer than k_reproject_cost; 16 x 16 and (b) are reported without a target;
  - det_of / person_of / total of the first frames are compared with the NumPy rule, bit for bit;
  - what it buys: tests/assign_cases.py::crossing through the kernels (k_reproject_cost, then match_detections or k_assign, then
    k_refine) -- the share of (f, c, p) that are shared, the share matched to the detection generated for them, the RMS error of the
    refined joints against the truth.  Figures of one synthetic recipe, not of footage.

    python scripts/bench_assign.py [--frames=N] [--calls=N] [--rounds=N]
Prints one JSON line; the figures go into EXPERIMENTS.md.
"""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np
import torch

from snowmocap_amd import _lib, synth
from snowmocap_amd import reproject as rp


def arg(name, default):
    return ([int(a.split("=")[1]) for a in sys.argv if a.startswith(f"--{name}=")] or [default])[0]


F, CALLS, ROUNDS = arg("frames", 10000), arg("calls", 10), arg("rounds", 3)
THR, GATE, J = 3.0, 12.0, 133


def event_ms(fn, calls):
    """durations of `calls` single calls, each between its own event pair, queued back to back"""
    pairs = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(calls)]
    for a, b in pairs:
        a.record()
        fn()
        b.record()
    torch.cuda.synchronize()
    return [a.elapsed_time(b) for a, b in pairs]


def recipe(P, dev, seed, chunk=1000):
    """-> (K, R, t), xyzs [F, P, J, 4] float64, kpts [F, 8, P, J, 3] float32, n_persons [F, 8] int32, all on the device"""
    K, R, t = synth.ring_rig(8)
    C = K.shape[0]
    g = torch.Generator(device=dev)
    g.manual_seed(seed)
    f64 = torch.float64
    Kt, Rt, tt = (torch.from_numpy(np.ascontiguousarray(a)).to(dev) for a in (K, R, t))
    centres = torch.from_numpy(synth.person_centres(P)).to(dev)
    box = torch.tensor([0.6, 0.6, 1.8], dtype=f64, device=dev)
    off = torch.tensor([0.5, 0.5, 0.0], dtype=f64, device=dev)
    xyzs = torch.empty((F, P, J, 4), dtype=f64, device=dev)
    kpts = torch.empty((F, C, P, J, 3), dtype=torch.float32, device=dev)
    for lo in range(0, F, chunk):
        n = min(chunk, F - lo)
        X = (torch.rand((n, P, J, 3), generator=g, dtype=f64, device=dev) - off) * box + centres[None, :, None, :]
        xyzs[lo:lo + n, ..., :3] = X + 0.01 * torch.randn((n, P, J, 3), generator=g, dtype=f64, device=dev)
        xyzs[lo:lo + n, ..., 3] = 1.0
        for c in range(C):
            pix = ((X - tt[c]) @ Rt[c]) @ Kt[c].T
            uv = pix[..., :2] / pix[..., 2:3] + torch.randn((n, P, J, 2), generator=g, dtype=f64, device=dev)
            rec = torch.cat([uv, 3.5 + 4.5 * torch.rand((n, P, J, 1), generator=g, dtype=f64, device=dev)], dim=-1)
            perm = torch.argsort(torch.rand((n, P), generator=g, device=dev), dim=1)
            kpts[lo:lo + n, c] = torch.gather(rec, 1, perm[:, :, None, None].expand(n, P, J, 3)).to(torch.float32)
    return (K, R, t), xyzs, kpts, torch.full((F, C), P, dtype=torch.int32, device=dev)


def measure(P, dev):
    (K, R, t), xyzs, kpts, npers = recipe(P, dev, 27 + P)
    ctx = _lib.Context(K, R, t)
    cs, cn = ctx.reproject_cost(xyzs, kpts, n_persons=npers, keypoint_score_threshold=THR)
    runs = {
        "reproject_cost": lambda: ctx.reproject_cost(xyzs, kpts, n_persons=npers, keypoint_score_threshold=THR),
        "match_detections_torch": lambda: rp.match_detections(cs, cn, GATE),
        "assign": lambda: ctx.assign_detections(cs, cn, GATE),
        "assign_all_outputs": lambda: ctx.assign_detections(cs, cn, GATE, with_person_of=True, with_total=True),
    }
    for fn in runs.values():
        for _ in range(2):
            fn()
    torch.cuda.synchronize()
    ms = {k: [] for k in runs}
    for _ in range(ROUNDS):                                  # alternating rounds: drift hits every kernel alike
        for k, fn in runs.items():
            ms[k] += event_ms(fn, CALLS)
    med = {k: float(np.median(v)) for k, v in ms.items()}
    nf = min(F, 16)
    got = ctx.assign_detections(cs[:nf].contiguous(), cn[:nf].contiguous(), GATE, with_person_of=True, with_total=True)
    want = rp.assign_detections_reference(cs[:nf].cpu().numpy(), cn[:nf].cpu().numpy(), GATE)
    equal = bool(np.array_equal(got[0].cpu().numpy(), want[0]) and np.array_equal(got[1].cpu().numpy(), want[1])
                 and np.array_equal(got[2].cpu().numpy().view(np.uint64), want[2].view(np.uint64)))
    old, shared = rp.match_detections(cs, cn, GATE)
    new = ctx.assign_detections(cs, cn, GATE)
    out = dict(P=P, Pmax=P, problems=F * 8, ms_median={k: round(v, 4) for k, v in med.items()},
               ms_min={k: round(float(min(v)), 4) for k, v in ms.items()}, equals_numpy_rule_first_frames=equal,
               shared_share_match_detections=float(shared.float().mean().item()),
               det_of_differs_share=float((old != new.to(torch.int64)).float().mean().item()),
               assign_over_reproject_cost=round(med["assign"] / med["reproject_cost"], 4),
               assign_over_match_detections_torch=round(med["assign"] / med["match_detections_torch"], 4),
               input_GBps=round(12 * F * 8 * P * P / med["assign"] * 1e-6, 1))
    ctx.close()
    return out


def what_it_buys(dev):
    import assign_cases as ac
    cs = ac.crossing()
    ctx = _lib.Context(cs["K"], cs["R"], cs["t"])
    x, kp, npers = (torch.from_numpy(np.array(cs[k])).to(dev) for k in ("xyzs", "kpts", "n_persons"))
    s, n = ctx.reproject_cost(x, kp, n_persons=npers, keypoint_score_threshold=ac.CROSS_THRESHOLD)

    def refine(det_of):
        det = torch.from_numpy(np.ascontiguousarray(det_of)).to(dev)
        return ctx.refine_joints(x, kp, det_of=det, n_persons=npers, keypoint_score_threshold=ac.CROSS_THRESHOLD).cpu().numpy()

    out = dict(recipe="tests/assign_cases.py::crossing", frames=int(x.shape[0]), cameras=int(kp.shape[1]), persons=3,
               start_rms_mm=round(1e3 * float(np.sqrt(((cs["xyzs"][..., :3] - cs["X"]) ** 2).sum(axis=-1).mean())), 3))
    for gate in (12.0, ac.CROSS_GATE):
        old = rp.match_detections(s, n, gate)[0].cpu().numpy()
        new = rp.assign_detections(ctx, s, n, gate).cpu().numpy()
        for name, det in (("match_detections", old), ("assign_detections", new)):
            shared, own, rms = ac.what_it_buys(cs, det, refine)
            out[f"gate{int(gate)}_{name}"] = dict(shared_share=round(shared, 5), matched_to_own_share=round(own, 5),
                                                   unmatched_share=round(float((det < 0).mean()), 5), refined_rms_mm=round(1e3 * rms, 3))
    ctx.close()
    return out


def main():
    dev = torch.device("cuda", 0)
    sizes = [measure(P, dev) for P in (4, 16)]
    held = sizes[0]["ms_median"]["assign"] <= sizes[0]["ms_median"]["reproject_cost"]
    line = dict(what="assign", frames=F, cameras=8, joints=J, gate_px=GATE, calls_per_kernel=CALLS * ROUNDS, sizes=sizes,
                yardstick_4x4_assign_within_reproject_cost=bool(held), what_it_buys=what_it_buys(dev))
    print(json.dumps(line))
    if not all(s["equals_numpy_rule_first_frames"] for s in sizes):
        sys.exit("k_assign differs from the NumPy rule")


if __name__ == "__main__":
    main()
