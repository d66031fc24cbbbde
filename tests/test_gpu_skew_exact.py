"""Every route the dispatch can take for the default (skew-ray) method, against the EXACT rule (oracle/skew_exact.py, 50 digits) on
general rigs: ring, mixed (per-camera K with skew), rolled (every camera rolled by its own angle, its own K, heights and distances
2x apart) and the floor rig, at the six placements of tests/dlt_frames_cases.py -- the same pixels in metres / millimetres, at the
origin, 47 m out and 1 km out (tests/skew_cases.py).  The production route where it is the default, the others forced through the
`knobs` fixture; the route is read back from Context.last_kernel_names() in every run.

Per case, route, output type and placement:
  * counts, person order, the singular / overflow flags and the zero fill behind count equal the rule's;
  * xyz within 2.5e-10 s + 1e-9 (|xyz - c| - s)+ (float64) or 2e-6 s / 4.5 + one float32 ulp (float32), (c, s) = oracle.dlt.rig_frame(t);
    scores by conftest.assert_scores_close, rtol 1e-9 / 3e-7, dist_err = 1e-14 (max |t_c| + rig diameter);
  * a joint nobody scores stays (0, 0, 0, 0); joints lie within 0.05 u of the placed truth wherever the rule's do (0.04 u);
  * equivariance: xyz / u - D within twice the bound of the same route's home output;
  * k_fused_lean_coop / k_fused_lean, and the streaming route with / without its candidate pass, give identical joints bit for bit.
The per-frame entries (Human_Triangulation / Human_Triangulation_Condense; snowtri_triangulate / snowtri_condense on device buffers)
run one mixed and one rolled case against the same rule.
The bounds are the project's (tests/test_gpu_dlt_frames.py, tests/test_gpu_parity.py) in rig units; tests/test_skew_exact_host.py
shows the fp64 C oracle inside them at every placement (worst 0.8 % of the xyz bound, at site).  Figures are printed per placement;
a test fails at the end, naming every placement that missed.
"""
import numpy as np
import pytest

import dlt_frames_cases as fc
import skew_cases as sk
from snowmocap_amd import _lib

pytestmark = pytest.mark.gpu
TN = {np.dtype(np.float32): "float", np.dtype(np.float64): "double"}


@pytest.fixture(scope="module")
def api():
    import snowmocap_amd as sm
    assert _lib.lib().snowtri_device_count() > 0, "these tests need the HIP device"
    return sm


class Report:
    """(tests/test_gpu_dlt_frames.py::Report) figures per placement, printed as they come; the failures raised together at the end."""

    def __init__(self, what):
        self.what, self.failed, self.worst = what, [], {}

    def add(self, placement, label, fails, fig):
        self.worst[placement] = max(self.worst.get(placement, 0.0), fig.get("xyz", 0.0))
        print(f"    {self.what} [{placement}] {label}: worst xyz err / bound = {fig.get('xyz', 0.0):.3g}, {fig.get('truth_joints', 0)} joints within "
              f"{fig.get('truth_m', 0.0):.3g} m of the truth, {len(fails)} misses")
        self.failed += [f"{placement} {label} {q}: {msg}" for q, msg in fails]

    def check(self, ok, placement, msg):
        if not ok:
            self.failed.append(f"{placement}: {msg}")

    def finish(self):
        assert not self.failed, f"{self.what}: " + " | ".join(self.failed[:12]) + (f" ... ({len(self.failed)} in all)" if len(self.failed) > 12 else "")


def _run(api, knobs, sc, tp, prm, out_dtype, env):
    for k, v in (env or {}).items():                      # (a forced route: the test build of the library, conftest.Knobs)
        knobs.set(k, v)
    bt = api.BatchTriangulator(sc["K"], sc["R"], tp, prm, pout_max=sc["pout"], out_dtype=out_dtype)
    try:
        out = bt.run_host(sc["kpts"], sc["n_persons"])
        out["kernels"] = bt.ctx.last_kernel_names()
        out["handed"] = bt.ctx.last_handover_persons()
        out["stream_counts"] = bt.ctx.last_stream_counts()
    finally:
        bt.close()
        knobs.clear()
    return out


def _route_ok(names, expect, C, tin, tout):
    """expect: a tuple of (how, pattern) with how in "starts", "has", "lacks", "is"; {C} {tin} {tout} are filled in."""
    for how, pat in expect:
        pat = pat.format(C=C, tin=tin, tout=tout)
        ok = {"starts": names.startswith(pat), "has": pat in names, "lacks": pat not in names, "is": names == pat}[how]
        if not ok:
            return False
    return True


def _case_on_route(api, knobs, rep, name, label, env, expect, out_dtypes=(np.float64, np.float32)):
    """One case on one route at every placement and output type -> {(placement, dtype name): out}."""
    sc = sk.scene(name)
    C, tin = sc["K"].shape[0], TN[sc["kpts"].dtype]
    outs, home_out = {}, {}
    for placement in sk.placements(sc["rig_name"]):
        tp, Xp, prm, u = sk.placed(name, placement)
        want = sk.exact(name, placement)
        over = want["count"] > sc["pout"]
        for out_dtype in out_dtypes:
            dn = np.dtype(out_dtype).name
            out = _run(api, knobs, sc, tp, prm, out_dtype, env)
            assert _route_ok(out["kernels"], expect, C, tin, TN[np.dtype(out_dtype)]), (name, label, dn, out["kernels"], expect)
            outs[placement, dn] = out
            fails, fig = sk.compare(sk.as_result(out), want, tp, out_dtype, u, Xtrue=Xp, dead=sc["dead"])
            rep.add(placement, f"{label} {dn}", fails, fig)
            rep.check(np.array_equal((out["flags"] & _lib.FLAG_OVERFLOW) != 0, over), placement, f"{label} {dn}: overflow flags")
            rep.check(out["status"] == (_lib.ERR_OVERFLOW if over.any() else _lib.OK), placement, f"{label} {dn}: status {out['status']}")
            h = home_out.setdefault(dn, out)
            rep.check(np.array_equal(h["count"], out["count"]), placement, f"{label} {dn}: count differs from home")
            if placement != "home" and not fails and np.array_equal(h["count"], out["count"]):
                seen = want["kscore"] != 0
                gx, hx = out["xyzs"][..., :3].astype(np.float64), h["xyzs"][..., :3].astype(np.float64)
                err = np.abs(fc.home(gx, placement) - hx)[seen]
                tol = (sk.xyz_bound(want["xyz"], tp, out_dtype, 2.0) / u)[seen]
                if err.size:
                    print(f"    {rep.what} [{placement}] {label} {dn}: xyz / u - D vs home, worst err / (2 x bound) = {np.max(err / tol):.3g}")
                    rep.check((err <= tol).all(), placement, f"{label} {dn}: xyz / u - D vs home: worst err / (2 x bound) = {np.max(err / tol):.3g}")
    return outs


def _same_bits(rep, a, b, what, keys=("xyzs", "count")):
    for key in a:
        if key not in b:
            continue
        for k in keys:
            rep.check(np.array_equal(a[key][k].view(np.uint8), b[key][k].view(np.uint8)), key[0], f"{key[1]} {k}: {what} differ in bits")


# ----------------------------------------------------------------------------------------------------- one detection per camera
LEAN_COOP = (("starts", "k_fused_lean_coop<{C},{tin},133"),)
LEAN = (("starts", "k_fused_lean<{C},{tin},133"),)
SINGLE0 = (("starts", "k_fused_single<{C},0,"),)
SUMLESS = (("starts", "k_singular_scan<"), ("has", "k_associate<"), ("lacks", "k_candidate_sums"))
SUMS = (("starts", "k_candidate_sums<"), ("has", "k_associate<"))
GENERAL = (("starts", "k_frame_general<"),)
RECOMPUTE = (("is", "k_frame_recompute<0,{tin},{tout}>"),)
F32, F64 = (np.float32,), (np.float64,)


@pytest.mark.parametrize("name", ["s-ring4", "s-rolled4", "s-mixed4", "s-floor"])
def test_four_cameras(api, knobs, name):
    """The bench's shape: k_fused_lean_coop<4,float> (constants in registers) and k_fused_lean<4> with float32 outputs -- identical
    bits -- and k_fused_single<4,0> with float64 outputs."""
    rep = Report(name)
    a = _case_on_route(api, knobs, rep, name, "lean coop", None, LEAN_COOP, F32)
    b = _case_on_route(api, knobs, rep, name, "lean", {"SNOWTRI_LEAN_COOP": "0"}, LEAN, F32)
    _same_bits(rep, a, b, "k_fused_lean_coop and k_fused_lean")
    _case_on_route(api, knobs, rep, name, "fused single", None, SINGLE0, F64)
    rep.finish()


@pytest.mark.parametrize("name", ["s-rolled5", "s-ring6", "s-rolled8"])
def test_five_to_eight_cameras(api, knobs, name):
    """The rolled item of the lean kernels, float32 and float64 outputs, cooperative and plain: identical bits."""
    rep = Report(name)
    a = _case_on_route(api, knobs, rep, name, "lean coop", None, LEAN_COOP)
    b = _case_on_route(api, knobs, rep, name, "lean", {"SNOWTRI_LEAN_COOP": "0"}, LEAN)
    _same_bits(rep, a, b, "k_fused_lean_coop and k_fused_lean")
    rep.finish()


def test_three_cameras(api, knobs):
    """k_fused_lean_coop<3> (float32 outputs), k_fused_single<3,0> (float64 outputs, and float32 with SNOWTRI_LEAN_MODE=0)."""
    rep = Report("s-rolled3")
    _case_on_route(api, knobs, rep, "s-rolled3", "lean coop", None, LEAN_COOP, F32)
    _case_on_route(api, knobs, rep, "s-rolled3", "fused single", None, SINGLE0, F64)
    _case_on_route(api, knobs, rep, "s-rolled3", "fused single (lean off)", {"SNOWTRI_LEAN_MODE": "0"}, SINGLE0, F32)
    rep.finish()


def test_two_cameras(api, knobs):
    """Two cameras, one detection each: one candidate, which the reference's condense never emits (range(n - 1) is empty) -- count 0
    and untouched slots on the route the dispatch takes (no fast kernel below three cameras) and on both general kernels."""
    rep = Report("s-ring2")
    _case_on_route(api, knobs, rep, "s-ring2", "default", None, SUMLESS)
    _case_on_route(api, knobs, rep, "s-ring2", "general", {"SNOWTRI_GENERAL_MODE": "1"}, GENERAL)
    _case_on_route(api, knobs, rep, "s-ring2", "recompute", {"SNOWTRI_HANDOVER_MODE": "0"}, RECOMPUTE)
    rep.finish()


@pytest.mark.parametrize("name,fuse", [("s-rolled6-J20", "k_cluster_fuse<6,"), ("s-ring12-J8", "k_cluster_fuse_wide<")])
def test_route_without_a_candidate_pass(api, knobs, name, fuse):
    """k_singular_scan -> k_associate -> cluster kernels -> k_person_scores (keypoint_num < J, two slots; twelve cameras), and the same
    call with its candidate pass kept (SNOWTRI_SUMLESS_MODE=0): the same joints bit for bit."""
    rep = Report(name)
    a = _case_on_route(api, knobs, rep, name, "sumless", None, SUMLESS + (("has", fuse), ("has", "k_person_scores<")))
    b = _case_on_route(api, knobs, rep, name, "candidate pass", {"SNOWTRI_SUMLESS_MODE": "0"}, SUMS + (("has", fuse),))
    _same_bits(rep, a, b, "the route with and without its candidate pass")
    rep.finish()


@pytest.mark.parametrize("name", ["s-rolled4", "s-rolled5"])
def test_single_detection_on_the_general_kernels(api, knobs, name):
    """Both general modes on a one-detection batch: SNOWTRI_GENERAL_MODE=1 (k_frame_general, candidates spilled) and =2 (the
    recompute route; with one detection per camera the streaming association without a candidate pass)."""
    rep = Report(name)
    _case_on_route(api, knobs, rep, name, "general mode 1", {"SNOWTRI_GENERAL_MODE": "1"}, GENERAL)
    _case_on_route(api, knobs, rep, name, "general mode 2", {"SNOWTRI_GENERAL_MODE": "2"}, SUMLESS)
    _case_on_route(api, knobs, rep, name, "general mode 2, phase 3 inside", {"SNOWTRI_GENERAL_MODE": "2", "SNOWTRI_HANDOVER_MODE": "0"}, RECOMPUTE)
    rep.finish()


# ------------------------------------------------------------------------------------------------ several detections per camera
MULTI = [n for n in sk.CASES if n.startswith("m-")]
COMPLETE = ("m-rolled2-ghosts", "m-rolled3-tight", "m-ring4-tight", "m-rolled8-clean", "m-ring12-clean")      # (k_cluster_fuse<2..8>, _wide)
MEMBER_LISTS = ("m-rolled3-ghosts", "m-ring4-tight", "m-mixed4-ghosts", "m-rolled8-tight", "m-rolled8-ghosts", "m-ring12-tight", "m-rolled16-ghosts")


@pytest.mark.parametrize("name", MULTI)
def test_multi_person_routes(api, knobs, name):
    """The streaming association (k_candidate_sums -> k_associate -> k_cluster_fuse<C> / k_cluster_fuse_wide / k_cluster_members),
    k_frame_recompute with phase 3 inside (SNOWTRI_HANDOVER_MODE=0) and k_frame_general (SNOWTRI_GENERAL_MODE=1).  Which cluster
    kernel fused how many persons is read back (last_handover_persons); "band": a frame through k_candidate_sums_exact and
    a frame whose person filter is re-done (past the association's first launch, or left to k_frame_recompute: last_stream_counts)."""
    sc = sk.scene(name)
    C = sc["K"].shape[0]
    fuse = f"k_cluster_fuse<{C}," if C <= 8 else "k_cluster_fuse_wide<"
    rep = Report(name)
    outs = _case_on_route(api, knobs, rep, name, "streaming", None, SUMS + (("has", fuse), ("has", "k_cluster_members<")))
    _case_on_route(api, knobs, rep, name, "recompute", {"SNOWTRI_HANDOVER_MODE": "0"}, RECOMPUTE)
    _case_on_route(api, knobs, rep, name, "general", {"SNOWTRI_GENERAL_MODE": "1"}, GENERAL)
    want = sk.exact(name, "home")
    persons = int(np.minimum(want["count"], sc["pout"]).sum())
    for key, out in outs.items():
        n_complete, n_other = out["handed"]
        print(f"    {name} [{key[0]}] {key[1]}: {n_complete} persons through {fuse}..>, {n_other} through k_cluster_members, "
              f"stream counts (frames, exact candidate sums, left to k_frame_recompute) = {out['stream_counts']}")
        rep.check(n_complete + n_other == persons or out["stream_counts"][0] > 0 or out["stream_counts"][2] > 0, key[0],
                  f"{key[1]}: {out['handed']} persons handed over, {persons} output persons, stream counts {out['stream_counts']}")
    n_complete, n_other = outs["home", "float64"]["handed"]
    if name in COMPLETE:                                   # every candidate of a person kept: the complete-graph kernel has work
        rep.check(n_complete >= 1, "home", f"no cluster through {fuse}: {outs['home', 'float64']['handed']}")
    if name in MEMBER_LISTS:                               # a wrong pairing in a cluster, a dropped candidate: member lists
        rep.check(n_other >= 1, "home", f"no cluster through k_cluster_members: {outs['home', 'float64']['handed']}")
    if name.endswith("band"):                              # decisions 1e-7 from their thresholds are re-done exactly, at every placement
        for key, out in outs.items():
            rep.check(out["stream_counts"][1] >= 1 and (out["stream_counts"][0] >= 1 or out["stream_counts"][2] >= 1), key[0],
                      f"{key[1]}: no frame through k_candidate_sums_exact, or none past the association's first launch: {out['stream_counts']}")
    rep.finish()


# ------------------------------------------------------------------------------------------------------ the per-frame entries
PER_FRAME = ["m-mixed4-ghosts", "m-rolled3-ghosts"]
SLOTS = 8                                                  # (the per-frame entries return every person: more slots than any frame has)


def _camera_group(K, R, t):
    from snowmocap_amd.camera import CameraGroup
    C = K.shape[0]
    cg = CameraGroup(cap_ids=list(range(C)), resolutions=[(1280, 720)] * C)
    for c, cam in enumerate(cg.cameras):
        cam.K, cam.R, cam.t = K[c].copy(), R[c].copy(), t[c].reshape(3, 1).copy()
    return cg


@pytest.mark.parametrize("name", PER_FRAME)
def test_per_frame_python_entries(api, name):
    """Human_Triangulation -> Human_Triangulation_Condense frame by frame (k_triangulate_slots, the device-resident candidates,
    k_condense; these entries record no kernel names: the route is read off snowtri_triangulate's own size rule): the kept
    candidates are the rule's, every person is the rule's within the float64 bounds."""
    from snowmocap_amd import triangulation as tri
    sc = sk.scene(name)
    F, C, P, J, _ = sc["kpts"].shape
    rep = Report(name)
    for placement in sk.placements(sc["rig_name"]):
        tp, Xp, prm, u = sk.placed(name, placement)
        want = sk.exact_with_slots(name, placement, SLOTS)
        assert want["count"].max() <= SLOTS
        kn = prm["keypoint_num"]
        got = dict(xyz=np.zeros((F, SLOTS, kn, 3)), kscore=np.zeros((F, SLOTS, kn)), pscore=np.zeros((F, SLOTS)), count=np.zeros(F, np.int32),
                   status=np.zeros(F, np.int32))
        cg = _camera_group(sc["K"], sc["R"], tp)
        for f in range(F):
            cg.clear_2D_points()
            for c in range(C):
                for p in range(int(sc["n_persons"][f, c])):
                    cg.add_human_2D_points(sc["kpts"][f, c, p, :, :2], sc["kpts"][f, c, p, :, 2], c)
            res = tri.Human_Triangulation(cg, prm["keypoint_score_threshold"], prm["average_score_threshold"], prm["distance_threshold"])
            rep.check(len(res["hrnet_triangulate_points"]) == len(want["kept"][f]), placement, f"frame {f}: {len(res['hrnet_triangulate_points'])} "
                      f"candidates kept, the rule keeps {len(want['kept'][f])}")
            con = tri.Human_Triangulation_Condense(res, prm["condense_distance_tol"], prm["condense_person_num_tol"], prm["condense_score_tol"],
                                                   prm["center_point_index"], kn)
            n = len(con["hrnet_triangulate_points"])
            got["count"][f] = n
            for i in range(min(n, SLOTS)):
                got["xyz"][f, i] = con["hrnet_triangulate_points"][i]
                got["kscore"][f, i] = con["hrnet_triangulate_keypoint_scores"][i]
                got["pscore"][f, i] = con["hrnet_triangulate_person_scores"][i]
        fails, fig = sk.compare(got, want, tp, np.float64, u, Xtrue=Xp)
        rep.add(placement, "per-frame float64", fails, fig)
    rep.finish()


@pytest.mark.parametrize("name", PER_FRAME)
def test_materialised_entries_on_device_buffers(api, name):
    """snowtri_triangulate -> snowtri_condense over the whole batch in device memory (k_triangulate, k_cand_mean, k_condense with a
    keep mask: no host mirror, so not the one-launch slot kernel), against the rule."""
    import torch
    sc = sk.scene(name)
    F, C, P, J, _ = sc["kpts"].shape
    dev = torch.device("cuda", 0)
    rep = Report(name)
    for placement in sk.placements(sc["rig_name"]):
        tp, Xp, prm, u = sk.placed(name, placement)
        want = sk.exact_with_slots(name, placement, SLOTS)
        kn = prm["keypoint_num"]
        ctx = _lib.Context(sc["K"], sc["R"], tp)
        try:
            L = ctx.L
            Kc = int(L.snowtri_num_candidate_slots(C, P))
            kp = torch.from_numpy(sc["kpts"]).to(dev)
            npers = torch.from_numpy(sc["n_persons"].astype(np.int32)).to(dev)
            f64 = dict(dtype=torch.float64, device=dev)
            cxyz, cks, cps = torch.zeros((F, Kc, J, 3), **f64), torch.zeros((F, Kc, J), **f64), torch.zeros((F, Kc), **f64)
            keep = torch.zeros((F, Kc), dtype=torch.uint8, device=dev)
            oxyz, oks, ops = torch.zeros((F, SLOTS, kn, 3), **f64), torch.zeros((F, SLOTS, kn), **f64), torch.zeros((F, SLOTS), **f64)
            cnt = torch.zeros(F, dtype=torch.int32, device=dev)
            prm_c = _lib.make_params(**prm)
            torch.cuda.synchronize()
            rc = L.snowtri_triangulate(ctx.handle, F, P, J, _lib.ptr(kp.data_ptr()), _lib.dtype_code(sc["kpts"].dtype), _lib.ptr(npers.data_ptr()), prm_c,
                                       _lib.ptr(cxyz.data_ptr()), _lib.ptr(cks.data_ptr()), _lib.ptr(cps.data_ptr()), _lib.ptr(keep.data_ptr()),
                                       _lib.DEVICE, None)
            assert rc == _lib.OK, rc
            rc = L.snowtri_condense(ctx.handle, F, Kc, J, _lib.ptr(cxyz.data_ptr()), _lib.ptr(cks.data_ptr()), _lib.ptr(keep.data_ptr()), prm_c, SLOTS,
                                    _lib.ptr(oxyz.data_ptr()), _lib.ptr(oks.data_ptr()), _lib.ptr(ops.data_ptr()), _lib.ptr(cnt.data_ptr()), None,
                                    _lib.DEVICE, None)
            assert rc == _lib.OK, rc
            ctx.synchronize()
            torch.cuda.synchronize()
            rep.check(keep.sum(dim=1).cpu().tolist() == [len(k) for k in want["kept"]], placement, "kept candidates per frame")
            got = dict(xyz=oxyz.cpu().numpy(), kscore=oks.cpu().numpy(), pscore=ops.cpu().numpy(), count=cnt.cpu().numpy(), status=np.zeros(F, np.int32))
        finally:
            ctx.close()
        fails, fig = sk.compare(got, want, tp, np.float64, u, Xtrue=Xp)
        rep.add(placement, "materialised float64", fails, fig)
    rep.finish()
