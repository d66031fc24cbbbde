#!/usr/bin/env python3
"""GPU box: the person tracker (snowtri_track_persons / snowtri_track_gather) on 10 000 frames of the 8 cameras x 4 persons
configuration (Pout_max 16, S 8, float32 outputs), HIP events after a warm-up:

  - k_track_centres and k_track_chain separately (snowtri_set_timing brackets them inside the call: snowtri_track_last_ms),
    k_track_gather between two events of its own;
  - the snowtri_triangulate_condense call the tracker serves, same shape, same process, for scale;
  - the gather's achieved bytes/s (read the present persons + person_of, write every slot) beside a copy_ of equal volume.

    python scripts/bench_tracking.py [--frames=N] [--calls=N] [--slots=S]
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
from snowmocap_amd.batch import BatchTriangulator
from snowmocap_amd.tracking import PersonTracker


def arg(name, default):
    return ([int(a.split("=")[1]) for a in sys.argv if a.startswith(f"--{name}=")] or [default])[0]


F, CALLS, S, POUT, GEN = arg("frames", 10000), arg("calls", 20), arg("slots", 8), 16, 500


def event_ms(fn, calls):
    """median and minimum of `calls` single launches, each between its own event pair, queued back to back"""
    pairs = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(calls)]
    for a, b in pairs:
        a.record()
        fn()
        b.record()
    torch.cuda.synchronize()
    ms = sorted(a.elapsed_time(b) for a, b in pairs)
    return ms[len(ms) // 2], ms[0]


def main():
    dev = torch.device("cuda", 0)
    wl = synth.config_workload(3, 1)                      # rig and thresholds of BASELINE configs[2] (ghost clusters included) ...
    K, R, t = wl["rig"]
    rng = np.random.default_rng(3)                          # ... on persons that WALK (0.03 m per frame), lists in random order
    X, _ = synth.make_walkers(rng, GEN, 4, 0.03)
    kpts, n_persons = synth.make_keypoints_visible(rng, K, R, t, X)
    kp = torch.from_numpy(kpts).to(dev).repeat(F // GEN, 1, 1, 1, 1).contiguous()
    npers = torch.from_numpy(n_persons).to(dev).repeat(F // GEN, 1).contiguous()
    frames = int(kp.shape[0])
    bt = BatchTriangulator(K, R, t, wl["params"], pout_max=POUT, out_dtype=np.float32)
    out = bt.alloc_outputs(frames, dev)
    for _ in range(3):
        bt.run_torch(kp, npers, out=out)
    torch.cuda.synchronize()
    tri_med, tri_min = event_ms(lambda: bt.run_torch(kp, npers, out=out), CALLS)
    xyzs, count = out["xyzs"], out["count"]
    kn = int(xyzs.shape[2])

    trk = PersonTracker(bt.ctx, S=S, center_point_index=bt.params.center_point_index, gate=0.3, max_missed=8)
    res = trk.run_torch(xyzs, count, gather=True, carry=False)                      # warm-up (scratch allocation)
    torch.cuda.synchronize()
    bt.ctx.set_timing(True)
    cen, chain = [], []
    ms2 = (ct.c_float * 2)()
    for _ in range(CALLS):
        trk.run_torch(xyzs, count, gather=False, carry=False)
        _lib.check(bt.ctx.L.snowtri_track_last_ms(bt.ctx.handle, ct.byref(ms2)), "snowtri_track_last_ms")
        cen.append(float(ms2[0]))
        chain.append(float(ms2[1]))
    bt.ctx.set_timing(False)
    person_of, tracked = res["person_of"], res["xyzs_tracked"]
    st = ct.c_void_p(torch.cuda.current_stream(dev).cuda_stream)

    def gather():
        _lib.check(bt.ctx.L.snowtri_track_gather(bt.ctx.handle, frames, POUT, kn, ct.c_void_p(xyzs.data_ptr()), _lib.F32, S,
                                                 ct.c_void_p(person_of.data_ptr()), ct.c_void_p(tracked.data_ptr()), _lib.DEVICE, st),
                   "snowtri_track_gather")

    for _ in range(3):
        gather()
    g_med, g_min = event_ms(gather, CALLS)
    n_present = int((person_of >= 0).sum())
    person_bytes = kn * 16
    g_bytes = n_present * person_bytes + person_of.numel() * 4 + frames * S * person_bytes
    src = torch.empty(g_bytes // 2, dtype=torch.uint8, device=dev)
    dst = torch.empty_like(src)
    for _ in range(3):
        dst.copy_(src)
    c_med, c_min = event_ms(lambda: dst.copy_(src), CALLS)
    ids = res["track_id"]
    line = dict(what="tracking", frames=frames, cams=8, persons=4, pout_max=POUT, slots=S, keypoint_num=kn, calls=CALLS,
                mean_count=float(count.float().mean()), track_ids=int(ids.max()) + 1, overflow_frames=int((res["flags"] & 1).sum()),
                k_track_centres_ms=float(np.median(cen)), k_track_chain_ms=float(np.median(chain)),
                k_track_chain_us_per_frame=1e3 * float(np.median(chain)) / frames, k_track_chain_ms_min=min(chain),
                k_track_gather_ms=g_med, k_track_gather_ms_min=g_min, gather_bytes=g_bytes, gather_GBps=g_bytes / g_med * 1e-6,
                copy_same_bytes_ms=c_med, copy_GBps=g_bytes / c_med * 1e-6,
                triangulate_condense_ms=tri_med, triangulate_condense_ms_min=tri_min,
                chain_over_triangulation=float(np.median(chain)) / tri_med, kernels=bt.ctx.last_kernel_names())
    print(json.dumps(line))


if __name__ == "__main__":
    main()
