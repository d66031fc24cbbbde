"""The capture protocol of tests/test_gpu_graph_capture.py and its cases: SNOWTRI_DEVICE entries whose header text says
"asynchronous on `stream`, no host read, no allocation, no internal stream" captured into a hipGraph on ONE stream, and the replays
compared with eager calls bit for bit (which entries, and which are left out and why: the module text of that file).

A Case says how to open what the calls need (a context, a BatchTriangulator), which static inputs and outputs a call takes, how to
issue the call on torch's current stream INTO the outputs it is handed, and three input sets A, B, C.  `run` holds every case to the
same nine steps (the numbers of the module text of tests/test_gpu_graph_capture.py).  The calls go through the C ABI with outputs the
case allocates (the Python wrappers of most entries allocate theirs per call: nothing a sentinel could be written to beforehand);
BatchTriangulator.run_torch(out=...) is the exception and is used as it is.
"""
import numpy as np

from snowmocap_amd import _lib

REPLAYS = ("A", "B", "C", "A")
SENTINEL_BYTE = 0x5a


# ---------------------------------------------------------------------------------------------------------------- tensors and bits
def tensors(arrays, dev):
    import torch
    def one(v):
        v = np.array(v, copy=True)
        return torch.from_numpy(v.view(np.int32) if v.dtype == np.uint32 else v).to(dev)      # (masks are int32 in torch)
    return {k: one(v) for k, v in arrays.items()}


def alloc(spec, dev):
    """spec: {name: (shape, torch dtype name)} -> sentinel-filled tensors."""
    import torch
    out = {k: torch.empty(tuple(shape), dtype=getattr(torch, dt), device=dev) for k, (shape, dt) in spec.items()}
    fill_sentinel(out)
    return out


def fill_sentinel(outs):
    """NaN in every float, 0x5a in every byte of an integer."""
    import torch
    for t in outs.values():
        if t.is_floating_point():
            t.fill_(float("nan"))
        else:
            t.view(torch.uint8).fill_(SENTINEL_BYTE)


def host(outs):
    return {k: v.cpu().numpy() for k, v in outs.items()}


def same_bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.dtype.itemsize == b.dtype.itemsize and np.array_equal(a.view(np.uint8), b.view(np.uint8))


def assert_same(got, want, what):
    assert list(got) == list(want), what
    for k in want:
        assert same_bits(got[k], want[k]), f"{what}: output {k} differs in {int((np.ascontiguousarray(got[k]).view(np.uint8) != np.ascontiguousarray(want[k]).view(np.uint8)).sum())} bytes"


def current_stream(dev):
    import torch
    return _lib.ptr(torch.cuda.current_stream(dev).cuda_stream)


def rolled(arrays, shift, keys=None):
    """The arrays rolled along their leading axis (those named by `keys`; default all)."""
    return {k: (np.roll(v, shift, axis=0) if keys is None or k in keys else np.array(v, copy=True)) for k, v in arrays.items()}


# ---------------------------------------------------------------------------------------------------------------- the protocol
class Case:
    """open() -> handle; context(handle) -> the _lib.Context whose stream_probes are read; outputs(handle) -> the spec of `alloc`;
    call(handle, ins, outs): the device call(s) on torch's current stream, raising unless every entry returns SNOWTRI_OK;
    close(handle).  sets: {"A" | "B" | "C": {input name: array}}.  moving(eager(A)): the outputs that must differ between eager(A),
    (B) and (C) (default: all).  warm(handle): checks after the warm-up call (kernel names).  before_capture(handle): settings changed
    between the warm-up call and the capture.  compare(got, want, what): how a replay is compared with the eager call (default:
    every output as bits)."""
    roll_keys = ()       # outputs for which eager(B) == eager(A) rolled by one frame (frames are independent)

    def context(self, h):
        return h

    def close(self, h):
        h.close()

    def moving(self, ref_a):
        """The outputs that must differ between eager(A), eager(B) and eager(C): those that are not the same in every frame of eager(A)
        (the count and the flags of a clean single-person batch are, and a roll cannot move them), unless a case knows better."""
        return [k for k, v in ref_a.items() if not same_bits(v, np.broadcast_to(v[:1], v.shape))]

    def warm(self, h):
        pass

    def before_capture(self, h):
        pass

    def compare(self, got, want, what):
        assert_same(got, want, what)


def eager(case, dev, name):
    """Step 7's reference: the call on a fresh context with fresh tensors holding input set `name`."""
    import torch
    h = case.open()
    try:
        case.before_capture(h)
        ins, outs = tensors(case.sets[name], dev), alloc(case.outputs(h), dev)
        side = torch.cuda.Stream(device=dev)
        torch.cuda.synchronize(dev)
        with torch.cuda.stream(side):
            case.call(h, ins, outs)
        torch.cuda.synchronize(dev)
        return host(outs)
    finally:
        torch.cuda.synchronize(dev)
        case.close(h)


def references(case, dev):
    """eager(A), eager(B), eager(C), checked to differ where the outputs depend on data (step 8) and -- `roll_keys` -- to be each
    other's rolls where frames are independent."""
    ref = {name: eager(case, dev, name) for name in ("A", "B", "C")}
    keys = case.moving(ref["A"])
    assert keys
    for a, b in (("A", "B"), ("A", "C"), ("B", "C")):
        for k in keys:
            assert not same_bits(ref[a][k], ref[b][k]), f"eager({a}) and eager({b}) agree in {k}: the input sets do not move it"
    for k in case.roll_keys:
        assert same_bits(ref["B"][k], np.roll(ref["A"][k], 1, axis=0)), f"eager(B) is not eager(A) rolled by one frame in {k}"
    return ref


def run(case, dev, ref=None):
    """Steps 1-9.  Returns the outputs of the four replays (host arrays)."""
    import torch
    ref = ref or references(case, dev)
    staged = {name: tensors(case.sets[name], dev) for name in ("A", "B", "C")}
    h = case.open()
    g = None
    try:
        ins = {k: v.clone() for k, v in staged["A"].items()}                        # 1. static tensors
        outs = alloc(case.outputs(h), dev)
        side = torch.cuda.Stream(device=dev)
        torch.cuda.synchronize(dev)
        with torch.cuda.stream(side):                                                # 2. the eager warm-up call
            case.call(h, ins, outs)
        torch.cuda.synchronize(dev)
        case.warm(h)
        case.before_capture(h)
        fill_sentinel(outs)                                                          # 3.
        torch.cuda.synchronize(dev)
        untouched = host(outs)
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g, stream=side):                                       # 4. (call raises unless SNOWTRI_OK)
            case.call(h, ins, outs)
        torch.cuda.synchronize(dev)
        assert_same(host(outs), untouched, "a capture executes nothing")            # 5.
        assert case.context(h).stream_probes() == (0, 0, -1)                         # 6. no internal stream: one linear chain
        got = []
        for i, name in enumerate(REPLAYS):                                           # 7.
            with torch.cuda.stream(side):
                for k, t in ins.items():
                    t.copy_(staged[name][k])
                g.replay()
            torch.cuda.synchronize(dev)
            got.append(host(outs))
            case.compare(got[-1], ref[name], f"replay {i + 1} (set {name}) against the eager call")
        return got
    finally:                                                                         # 9. graph, synchronise, context
        del g
        torch.cuda.synchronize(dev)
        case.close(h)


def _dev(ins):
    return next(iter(ins.values())).device


def _swap_cameras(a, axis=1):
    """cameras 0 and 1 of an [F, C, ...] array change places (in place): the one changed det_of / n_persons row of set C"""
    idx = [slice(None)] * a.ndim
    i0, i1 = list(idx), list(idx)
    i0[axis], i1[axis] = 0, 1
    tmp = a[tuple(i0)].copy()
    a[tuple(i0)] = a[tuple(i1)]
    a[tuple(i1)] = tmp


def abc(A, swap=()):
    """B: A rolled by one frame; C: A rolled by 17 with cameras 0 and 1 swapped in the arrays `swap` names."""
    A = {k: np.array(v, copy=True) for k, v in A.items()}
    C = rolled(A, 17)
    for k in swap:
        _swap_cameras(C[k])
    return {"A": A, "B": rolled(A, 1), "C": C}


# ---------------------------------------------------------------------------------------------------------------- a. the fused call
class Fused(Case):
    """One route of tests/fused_route_cases.py through BatchTriangulator.run_torch(out=static outputs).  frames: the 70-frame batch
    repeated to that length.  split: the snowtri_ctx_set_split value set between the warm-up call and the capture (multi-person
    routes are warmed up under set_split(1), as include/snowtri.h asks of a capturing caller).  kw: BatchTriangulator's."""

    def __init__(self, api, route, frames=None, split=None, pout=None, **kw):
        import fused_route_cases as frc
        self.api, self.frc, self.route, self.r, self.kw, self.split = api, frc, route, frc.BY_ID[route], kw, split
        assert not self.r["knobs"], "only the routes the production library reaches by shape"
        self.pout = pout or self.r["pout"]
        kp, npers = frc.batch(route)[3:5]
        if frames:
            kp, npers = np.resize(kp, (frames,) + kp.shape[1:]), np.resize(npers, (frames,) + npers.shape[1:])
        self.F = kp.shape[0]
        self.sets = abc(dict(kpts=kp, n_persons=npers), swap=("n_persons",))
        if self.r["P"] == 1:
            self.roll_keys = ("xyzs", "pscore", "count", "flags") + (("views", "resid") if kw.get("diagnostics") else ())

    def open(self):
        bt = self.frc.triangulator(self.api, self.route, pout=self.pout, **self.kw)
        if self.r["P"] > 1:
            bt.ctx.set_split(1)
        return bt

    def context(self, bt):
        return bt.ctx

    def before_capture(self, bt):
        if self.split is not None:
            bt.ctx.set_split(self.split)

    def outputs(self, bt):
        tdt, kn, F = self.r["out"], self.r["kn"], self.F
        spec = dict(xyzs=((F, self.pout, kn, 4), tdt), pscore=((F, self.pout), tdt), count=((F,), "int32"), flags=((F,), "int32"))
        if bt.diagnostics:
            spec.update(views=((F, kn), "int32"), resid=((F, kn), tdt))
        return spec

    def call(self, bt, ins, outs):
        bt.run_torch(ins["kpts"], ins["n_persons"], out=outs)

    def warm(self, bt):
        self.names = bt.ctx.last_kernel_names()


class FusedNoZeroFill(Fused):
    """lean_coop with zero_fill=False.  nobody=(): the batch of the route table as it is.  nobody=(5, 40): no camera lists anybody in
    those frames of set A (count[f] = 0 there, and where the rolls take them in B and C), so slot 0 of such a frame lies behind
    count[f].
    include/snowtri.h calls the slots behind count[f] UNSPECIFIED: the call spends no stores on padding them, and a kernel may still
    write there (k_fused_lean_coop stores every joint it solves speculatively before it knows the frame's count).  What a graph has to
    keep is therefore this: counts, flags and the slots below count[f] equal the eager call's as bits; and behind count[f] every value
    is either what the eager call wrote at that place into its sentinel-filled buffer, or -- where the eager call left its sentinel --
    what the graph's buffer held before the replay (the sentinel in the first replay, an earlier replay's record later).  A replay
    that cleared, or wrote, a place the eager call does not touch fails."""

    def __init__(self, api, nobody=()):
        super().__init__(api, "lean_coop", zero_fill=False)
        A = self.sets["A"]
        if len(nobody):
            A["n_persons"][list(nobody)] = 0
        self.nobody = tuple(nobody)
        self.sets = abc(A, swap=("n_persons",))
        self.roll_keys = ()
        self.held = None
        self.figures = []

    def compare(self, got, want, what):
        for k in ("count", "flags"):
            assert same_bits(got[k], want[k]), (what, k)
        pout = want["xyzs"].shape[1]
        used = np.arange(pout)[None, :] < np.minimum(want["count"], pout)[:, None]          # [F, pout]
        assert used.any() and ((~used).any() or not self.nobody)
        nan32 = np.array([np.nan], dtype=np.float32).view(np.uint32)[0]
        if not self.nobody:       # the table's batch: whatever lies behind count[f] still holds the sentinel, after every replay
            for k in ("xyzs", "pscore"):
                assert same_bits(got[k][used], want[k][used]), f"{what}: {k} below count[f]"
                assert (got[k][~used].reshape(-1).view(np.uint32) == nan32).all(), f"{what}: the sentinel behind count[f] in {k}"
            self.figures.append((what, int((~used).sum())))
            return
        if self.held is None:
            self.held = {k: want[k].copy() for k in ("xyzs", "pscore")}       # the eager call's buffer: the sentinel where it wrote nothing
        for k in ("xyzs", "pscore"):
            assert same_bits(got[k][used], want[k][used]), f"{what}: {k} below count[f]"
            g, w, h = (a[k][~used].reshape(-1).view(np.uint32) for a in (got, want, self.held))
            untouched = w == nan32                                             # places the eager call left as its buffer held them
            self.figures.append((what, k, int(g.size), int(untouched.sum()), int((g.view(np.float32) == 0).sum())))
            print(f"{what}: {k} behind count[f]: {g.size} values; the eager call leaves {int(untouched.sum())} untouched, writes "
                  f"{int((~untouched).sum())} ({int((w.view(np.float32)[~untouched] == 0).sum())} of them zeros)")
            assert np.array_equal(g[~untouched], w[~untouched]), f"{what}: {k} behind count[f]: a value the kernel writes differs from the eager call's"
            assert np.array_equal(g[untouched], h[untouched]), f"{what}: {k} behind count[f]: a place the eager call leaves alone was written"
            self.held[k] = got[k].copy()


def lean_launch_frames(num_cus):
    """The smallest F for which launch_fused_lean (snowtri.hip) leaves k_fused_lean_coop for k_fused_lean: the small launch takes
    F <= num_cus * lean_wg_per_cu (2) * kCoopMaxFrames (32)."""
    return num_cus * 2 * 32 + 1


# ---------------------------------------------------------------------------------------------------------------- b. the entries
class Entry(Case):
    """A case on a plain context: rig = (K, R, t) or None (the rig-less scratch context), D = lens coefficients or None."""
    rig, D = None, None

    def open(self):
        ctx = _lib.Context(*self.rig) if self.rig else _lib.Context()
        if self.D is not None:
            ctx.set_distortion(self.D)
        return ctx


def _ok(ctx, rc, where):
    if rc != _lib.OK:
        raise _lib.SnowtriError(rc, f"{where}: {ctx.L.snowtri_last_error().decode()}")


class Reproject(Entry):
    """snowtri_reproject, then snowtri_reproject_cost, on reproject_cases.cost_case((4, 2, 2, 5, 3)) with n_persons."""

    def __init__(self, raw):
        import reproject_cases as rc
        cs = rc.cost_case((4, 2, 2, 5, 3), "float64", True)
        self.rig, self.D, self.thr, self.flags = (cs["K"], cs["R"], cs["t"]), cs["D"], cs["thr"], _lib.REPROJECT_RAW if raw else 0
        self.sets = abc(dict(xyzs=cs["xyzs"], kpts=cs["kpts"], n_persons=cs["n_persons"]), swap=("n_persons",))
        self.F, self.C, self.Pmax = cs["kpts"].shape[:3]
        self.P, self.kn = cs["xyzs"].shape[1:3]

    def outputs(self, ctx):
        F, C, P, Pmax, kn = self.F, self.C, self.P, self.Pmax, self.kn
        return dict(pix=((F, C, P, kn, 3), "float64"), cost_sum=((F, C, P, Pmax), "float64"), cost_n=((F, C, P, Pmax), "int32"))

    def call(self, ctx, ins, outs):
        p, st, tail = _lib.ptr, current_stream(_dev(ins)), (_lib.DEVICE,)
        _ok(ctx, ctx.L.snowtri_reproject(ctx.handle, self.F, self.P, self.kn, p(ins["xyzs"]), _lib.F64, self.flags, p(outs["pix"]), _lib.F64,
                                         *tail, st), "snowtri_reproject")
        _ok(ctx, ctx.L.snowtri_reproject_cost(ctx.handle, self.F, self.P, self.kn, p(ins["xyzs"]), _lib.F64, self.Pmax, p(ins["kpts"]), _lib.F64,
                                              p(ins["n_persons"]), self.thr, self.flags, p(outs["cost_sum"]), p(outs["cost_n"]), *tail, st),
            "snowtri_reproject_cost")


class Assign(Entry):
    """snowtri_assign_detections on the cost arrays of assign_cases.crossing() (the NumPy rule's: the inputs of the entry)."""

    def __init__(self):
        import assign_cases as ac
        from snowmocap_amd.reproject import reprojection_cost_reference
        cs = ac.crossing()
        cost_sum, cost_n = reprojection_cost_reference(cs["K"], cs["R"], cs["t"], cs["xyzs"], cs["kpts"], n_persons=cs["n_persons"],
                                                       keypoint_score_threshold=ac.CROSS_THRESHOLD)
        self.gate, self.min_joints = ac.CROSS_GATE, ac.MIN_JOINTS
        self.sets = abc(dict(cost_sum=np.ascontiguousarray(cost_sum, dtype=np.float64), cost_n=np.ascontiguousarray(cost_n, dtype=np.int32)),
                        swap=("cost_sum", "cost_n"))
        self.F, self.C, self.P, self.Pmax = cost_sum.shape

    def outputs(self, ctx):
        F, C, P, Pmax = self.F, self.C, self.P, self.Pmax
        return dict(det_of=((F, C, P), "int32"), person_of=((F, C, Pmax), "int32"), total=((F, C), "float64"))

    def call(self, ctx, ins, outs):
        p = _lib.ptr
        _ok(ctx, ctx.L.snowtri_assign_detections(ctx.handle, self.F * self.C, self.P, self.Pmax, p(ins["cost_sum"]), p(ins["cost_n"]), self.gate,
                                                 self.min_joints, p(outs["det_of"]), p(outs["person_of"]), p(outs["total"]), _lib.DEVICE,
                                                 current_stream(_dev(ins))), "snowtri_assign_detections")


class Matched(Entry):
    """snowtri_triangulate_matched with its diagnostics on matched_cases.woven("ring4", 2, 3): two persons woven into lists of three."""
    TAU, DROPS = 6.0, 1

    def __init__(self):
        import matched_cases as mc
        b, det_of, self.thr = mc.case(("woven", "ring4", 2, 3, 40, 133, "float32"))
        self.rig = (b["K"], b["R"], b["t"])
        self.sets = abc(dict(kpts=b["kpts"], det_of=np.asarray(det_of, dtype=np.int32), n_persons=b["n_persons"]), swap=("det_of",))
        self.F, self.C, self.Pmax, self.kn = b["kpts"].shape[:4]
        self.P = det_of.shape[2]

    def outputs(self, ctx):
        F, P, kn = self.F, self.P, self.kn
        return dict(xyzs=((F, P, kn, 4), "float32"), pscore=((F, P), "float32"), views=((F, P, kn), "int32"), resid=((F, P, kn), "float32"))

    def call(self, ctx, ins, outs):
        p = _lib.ptr
        _ok(ctx, ctx.L.snowtri_triangulate_matched(ctx.handle, self.F, self.P, self.kn, self.Pmax, p(ins["kpts"]), _lib.F32, p(ins["n_persons"]),
                                                   p(ins["det_of"]), self.thr, self.TAU, self.DROPS, p(outs["xyzs"]), p(outs["pscore"]), _lib.F32,
                                                   p(outs["views"]), p(outs["resid"]), _lib.DEVICE, current_stream(_dev(ins))),
            "snowtri_triangulate_matched")


class Seed(Entry):
    """snowtri_pair_cost, then snowtri_seed_persons on its outputs, on seed_cases.batch(4, 3, 133, 37)."""
    MIN_VIEWS = 3

    def __init__(self):
        import seed_cases as sd
        b = sd.batch(4, 3, 133, 37)
        self.rig, self.thr, self.gate, self.min_joints = (b["K"], b["R"], b["t"]), b["thr"], sd.GATE, sd.MIN_JOINTS
        self.sets = abc(dict(kpts=b["kpts"], n_persons=b["n_persons"], claimed=b["claimed"]), swap=("n_persons",))
        self.F, self.C, self.Pmax, self.kn = b["kpts"].shape[:4]
        self.S = self.C * self.Pmax // self.MIN_VIEWS

    def outputs(self, ctx):
        F, C, Pm, NP = self.F, self.C, self.Pmax, self.C * (self.C - 1) // 2
        return dict(pair_sum=((F, NP, Pm, Pm), "float64"), pair_n=((F, NP, Pm, Pm), "int32"), seed_det_of=((F, C, self.S), "int32"),
                    n_seeds=((F,), "int32"), flags=((F,), "int32"))

    def call(self, ctx, ins, outs):
        p, st = _lib.ptr, current_stream(_dev(ins))
        _ok(ctx, ctx.L.snowtri_pair_cost(ctx.handle, self.F, self.kn, self.Pmax, p(ins["kpts"]), _lib.F32, p(ins["n_persons"]), p(ins["claimed"]),
                                         self.thr, p(outs["pair_sum"]), p(outs["pair_n"]), _lib.DEVICE, st), "snowtri_pair_cost")
        _ok(ctx, ctx.L.snowtri_seed_persons(ctx.handle, self.F, self.Pmax, p(outs["pair_sum"]), p(outs["pair_n"]), p(ins["n_persons"]),
                                            p(ins["claimed"]), self.gate, self.min_joints, self.MIN_VIEWS, self.S, p(outs["seed_det_of"]),
                                            p(outs["n_seeds"]), p(outs["flags"]), _lib.DEVICE, st), "snowtri_seed_persons")


class RefineJoints(Entry):
    """snowtri_refine_joints (huber_px None) or snowtri_refine_joints_ex (huber_px > 0) with diagnostics on refine_cases.case("floor",
    (5, 2, 133)) from its DLT start: det_of, n_persons and views all given."""
    ITERS = 4

    def __init__(self, huber_px=None):
        import refine_cases as rfc
        cs = rfc.case("floor", (5, 2, 133))
        self.rig, self.thr, self.huber = (cs["K"], cs["R"], cs["t"]), cs["thr"], huber_px
        self.sets = abc(dict(xyzs=cs["dlt"], kpts=cs["kpts"], det_of=cs["det_of"].astype(np.int32), n_persons=cs["n_persons"], views=cs["views"]),
                        swap=("det_of",))
        self.F, self.C, self.Pmax, self.kn = cs["kpts"].shape[:4]
        self.P = cs["dlt"].shape[1]

    def outputs(self, ctx):
        F, P, kn = self.F, self.P, self.kn
        spec = dict(out=((F, P, kn, 4), "float64"), cost=((F, P, kn, 2), "float64"), codes=((F, P, kn), "uint8"))
        if self.huber:
            spec["outliers"] = ((F, P, kn), "int32")
        return spec

    def call(self, ctx, ins, outs):
        p, st = _lib.ptr, current_stream(_dev(ins))
        head = (ctx.handle, self.F, self.P, self.kn, p(ins["xyzs"]), _lib.F64, self.Pmax, p(ins["kpts"]), _lib.F64, p(ins["n_persons"]),
                p(ins["det_of"]), p(ins["views"]), self.thr, self.ITERS, 0)
        if self.huber:
            _ok(ctx, ctx.L.snowtri_refine_joints_ex(*head, float(self.huber), p(outs["out"]), p(outs["cost"]), p(outs["codes"]), p(outs["outliers"]),
                                                    _lib.DEVICE, st), "snowtri_refine_joints_ex")
        else:
            _ok(ctx, ctx.L.snowtri_refine_joints(*head, p(outs["out"]), p(outs["cost"]), p(outs["codes"]), _lib.DEVICE, st), "snowtri_refine_joints")


class RefineCameras(Entry):
    """snowtri_refine_cameras with its report on pose_cases.recipe(): the drifted rig, the camera that drifted free to move, the
    records pose_cases.dlt_points gives.  The entry sums over frames, so B and C also take a camera's detections away in a few frames
    (n_persons rows): n_obs moves, and every sum with it."""

    def __init__(self):
        import pose_cases as pc
        rp = pc.recipe()
        self.rig, self.bad = (rp["K"], rp["Rd"], rp["td"]), rp["bad"]
        kp = rp["kpts"]
        self.F, self.C, self.P, self.kn = kp.shape[:4]
        A = dict(xyzs=pc.dlt_points(rp["K"], rp["Rd"], rp["td"], kp), kpts=kp, n_persons=np.full((self.F, self.C), self.P, dtype=np.int32))
        self.sets = abc(A)
        self.sets["B"]["n_persons"][0:3, self.bad] = 0
        self.sets["C"]["n_persons"][5:12, self.bad] = 1
        self.min_obs, self.iters = 64, pc.ITERS

    def outputs(self, ctx):
        C = self.C
        return dict(R=((C, 3, 3), "float64"), t=((C, 3), "float64"), cost=((C, 2), "float64"), n_obs=((C,), "int64"), codes=((C,), "uint8"),
                    normal=((C, 28), "float64"))

    def moving(self, ref_a):
        return ["R", "t", "cost", "n_obs", "normal"]

    def call(self, ctx, ins, outs):
        p = _lib.ptr
        _ok(ctx, ctx.L.snowtri_refine_cameras(ctx.handle, self.F, self.P, self.kn, p(ins["xyzs"]), _lib.F64, self.P, p(ins["kpts"]), _lib.F64,
                                              p(ins["n_persons"]), None, None, 0.5, 1 << self.bad, self.min_obs, self.iters, 0, p(outs["R"]),
                                              p(outs["t"]), p(outs["cost"]), p(outs["n_obs"]), p(outs["codes"]), p(outs["normal"]), _lib.DEVICE,
                                              current_stream(_dev(ins))), "snowtri_refine_cameras")


class RecordPass(Entry):
    """snowtri_fill_joint_track or snowtri_despike_joint_track with codes on a float32 track of block_frames + 3 frames x 70 lanes: two
    tiles in time, two lane columns."""
    LANES = 70

    def __init__(self, which):
        self.which = which
        if which == "fill":
            from snowmocap_amd.fill import fill_block_frames
            from test_fill_host import random_track
            self.T, self.args = fill_block_frames() + 3, (3,)
            x = random_track(np.random.default_rng(77), self.T, self.LANES, 3, np.float32)
        else:
            import despike_cases as dc
            from snowmocap_amd.despike import despike_block_frames
            self.T = despike_block_frames() + 3
            et = dc.edge_track(self.T, self.LANES, "float32", 3)
            x, self.args = et["x"], (3, float(et["tol"]), _lib.DESPIKE_MARK)
        self.sets = abc(dict(xyzs=x))

    def outputs(self, ctx):
        return dict(out=((self.T, self.LANES, 4), "float32"), codes=((self.T, self.LANES), "uint8"))

    def call(self, ctx, ins, outs):
        entry = ctx.L.snowtri_fill_joint_track if self.which == "fill" else ctx.L.snowtri_despike_joint_track
        _ok(ctx, entry(ctx.handle, self.T, self.LANES, _lib.ptr(ins["xyzs"]), _lib.F32, *self.args, _lib.ptr(outs["out"]), _lib.ptr(outs["codes"]),
                       _lib.DEVICE, current_stream(_dev(ins))), self.which)


# ---------------------------------------------------------------------------------------------------------------- d. a chain
class Chain(Case):
    """What a per-recording loop would put into one graph, each stage reading the static output of the stage before it: undistort +
    the fused dlt_robust call; reproject_cost + assign_detections; triangulate_matched + refine_joints; the tracker (a fresh start
    per call: state = NULL); despike + fill.  4 cameras, one person (a walker), 133 joints, chain_block_frames() + 8 frames.
    (snowtri_smooth_joint_track would end the chain, but no capture of the smoothing scan is verified: the module text of
    tests/test_gpu_graph_capture.py.  TrackPipeline.run itself reads counts on the host -- pipeline.py, `check` and the ragged
    tracks -- and cannot be captured: out of scope.)"""
    J, S, LENS = 133, 2, (0.02, 0.004, 0.001, -0.001, 0.0)

    def __init__(self, api):
        from snowmocap_amd import synth
        from snowmocap_amd.tracking import chain_block_frames
        self.api, self.F = api, chain_block_frames() + 8
        rng = np.random.default_rng(2024)
        self.K, self.R, self.t = synth.ring_rig(4)
        X, _ = synth.make_walkers(rng, self.F, 1, 0.01, J=self.J)
        kp, npers = synth.make_keypoints(rng, self.K, self.R, self.t, X, pixel_sigma=1.0, score_range=(2.0, 8.0))
        kp, _ = synth.add_outliers(rng, kp, fraction=0.1)
        kp[20:23, :, 0, :, 2] = 0.0                     # three frames nobody is seen in: a dropout for the tracker and the fill
        kp, npers = np.ascontiguousarray(kp, dtype=np.float32), npers.astype(np.int32)
        npers[3, 1] = 0
        self.prm = dict(synth.default_thresholds(), keypoint_num=self.J, center_point_index=0)
        self.thr = float(self.prm["keypoint_score_threshold"])
        self.sets = abc(dict(kpts=kp, n_persons=npers), swap=("n_persons",))

    def open(self):
        return self.api.BatchTriangulator(self.K, self.R, self.t, self.prm, pout_max=1, out_dtype=np.float64, method=_lib.DLT_ROBUST,
                                          D=np.tile(self.LENS, (4, 1)), reproj_threshold_px=6.0, max_drops=1)

    def context(self, bt):
        return bt.ctx

    def outputs(self, bt):
        F, C, J, S, f8 = self.F, 4, self.J, self.S, "float64"
        return dict(xyzs=((F, 1, J, 4), f8), pscore=((F, 1), f8), count=((F,), "int32"), flags=((F,), "int32"),
                    cost_sum=((F, C, 1, 1), f8), cost_n=((F, C, 1, 1), "int32"), det_of=((F, C, 1), "int32"),
                    xyzs_matched=((F, 1, J, 4), f8), pscore_matched=((F, 1), f8), views=((F, 1, J), "int32"), resid=((F, 1, J), f8),
                    xyzs_refined=((F, 1, J, 4), f8), refine_cost=((F, 1, J, 2), f8), refine_codes=((F, 1, J), "uint8"),
                    slot_of=((F, 1), "int32"), person_of=((F, S), "int32"), track_id=((F, S), "int32"), track_flags=((F,), "int32"),
                    xyzs_tracked=((F, S, J, 4), f8), despiked=((F, S * J, 4), f8), spike_codes=((F, S * J), "uint8"),
                    filled=((F, S * J, 4), f8), fill_codes=((F, S * J), "uint8"))

    def call(self, bt, ins, o):
        ctx, L, h, p, st, F, J, S, D = bt.ctx, bt.ctx.L, bt.ctx.handle, _lib.ptr, current_stream(_dev(ins)), self.F, self.J, self.S, _lib.DEVICE
        F64, F32 = _lib.F64, _lib.F32
        bt.run_torch(ins["kpts"], ins["n_persons"], out={k: o[k] for k in ("xyzs", "pscore", "count", "flags")})
        kp, npers = p(bt.last_undistorted_kpts), p(ins["n_persons"])
        _ok(ctx, L.snowtri_reproject_cost(h, F, 1, J, p(o["xyzs"]), F64, 1, kp, F32, npers, self.thr, 0, p(o["cost_sum"]), p(o["cost_n"]), D, st),
            "snowtri_reproject_cost")
        _ok(ctx, L.snowtri_assign_detections(h, F * 4, 1, 1, p(o["cost_sum"]), p(o["cost_n"]), 30.0, 8, p(o["det_of"]), None, None, D, st),
            "snowtri_assign_detections")
        _ok(ctx, L.snowtri_triangulate_matched(h, F, 1, J, 1, kp, F32, npers, p(o["det_of"]), self.thr, 6.0, 1, p(o["xyzs_matched"]),
                                               p(o["pscore_matched"]), F64, p(o["views"]), p(o["resid"]), D, st), "snowtri_triangulate_matched")
        _ok(ctx, L.snowtri_refine_joints(h, F, 1, J, p(o["xyzs_matched"]), F64, 1, kp, F32, npers, p(o["det_of"]), p(o["views"]), self.thr, 4, 0,
                                         p(o["xyzs_refined"]), p(o["refine_cost"]), p(o["refine_codes"]), D, st), "snowtri_refine_joints")
        _ok(ctx, L.snowtri_track_persons(h, F, 1, J, p(o["xyzs_refined"]), F64, p(o["count"]), S, 0, 0.3, 1, None, p(o["slot_of"]), p(o["person_of"]),
                                         p(o["track_id"]), p(o["track_flags"]), D, st), "snowtri_track_persons")
        _ok(ctx, L.snowtri_track_gather(h, F, 1, J, p(o["xyzs_refined"]), F64, S, p(o["person_of"]), p(o["xyzs_tracked"]), D, st), "snowtri_track_gather")
        _ok(ctx, L.snowtri_despike_joint_track(h, F, S * J, p(o["xyzs_tracked"]), F64, 3, 0.1, _lib.DESPIKE_MARK, p(o["despiked"]), p(o["spike_codes"]),
                                               D, st), "snowtri_despike_joint_track")
        _ok(ctx, L.snowtri_fill_joint_track(h, F, S * J, p(o["despiked"]), F64, 3, p(o["filled"]), p(o["fill_codes"]), D, st), "snowtri_fill_joint_track")
