"""Matched triangulation on the host (no GPU): the NumPy rule matched.triangulate_matched_reference (include/snowtri.h, "Matched
triangulation") against triangulate_robust_reference per person, its det_of / n_persons edges, what it buys on the recipe
"crossing", the share of near-tie decisions on the inputs the GPU file uses, the signatures of the Python entries, and the C entry
refusing bad arguments under AddressSanitizer (tests/abi_badargs_matched.c against the `make asan` library)."""
import inspect
import os

import numpy as np
import pytest

import matched_cases as mc
import robust_cases as rc
from conftest import ROOT
from snowmocap_amd import matched
from snowmocap_amd.robust import triangulate_robust_reference

KEYS = ("xyzs", "pscore", "views", "resid", "drops", "margin", "decision")


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint64) if a.dtype == np.float64 else a


def _rule(b, det_of, n_persons, tau=6.0, md=6):
    return matched.triangulate_matched_reference(b["K"], b["R"], b["t"], b["kpts"], det_of, n_persons, mc.KTHR, tau, md)


def _same(a, b, p, q=None):
    q = p if q is None else q
    for k in KEYS:
        assert np.array_equal(_bits(a[k][:, p]), _bits(b[k][:, q])), k


@pytest.mark.parametrize("name,P,Pmax", [("ring4", 2, 3), ("ring3", 3, 3), ("ring8", 1, 2)])
def test_rule_equals_the_robust_rule_per_person_bit_for_bit(name, P, Pmax):
    b = mc.woven(name, P, Pmax, 12, 17)
    for tau, md in ((6.0, 6), (2.5, 2)):
        got = _rule(b, b["det_of"], b["n_persons"], tau, md)
        for p, s in enumerate(b["singles"]):
            one = triangulate_robust_reference(s["K"], s["R"], s["t"], s["kpts"], s["n_persons"], mc.KTHR, 17, tau, md)
            for k in KEYS:
                want = one[k][:, 0] if k in ("xyzs", "pscore") else one[k]
                assert np.array_equal(_bits(got[k][:, p]), _bits(want)), (k, p)
        assert (got["drops"] > 0).any()                       # (the batches carry outliers: the loop ran)


def test_permuting_a_list_with_det_of_changes_no_bit():
    b = mc.woven("ring4", 2, 3, 12, 17)
    base = _rule(b, b["det_of"], b["n_persons"])
    perm = np.array([2, 0, 1])
    kp = b["kpts"].copy()
    kp[:, 1] = b["kpts"][:, 1][:, perm]                       # the new list of camera 1: position i holds the old detection perm[i]
    det = b["det_of"].copy()
    inv = np.argsort(perm)
    det[:, 1] = np.where(det[:, 1] >= 0, inv[np.maximum(det[:, 1], 0)], -1)
    got = _rule(dict(b, kpts=kp), det, b["n_persons"])
    for p in range(2):
        _same(got, base, p)


def test_det_of_and_n_persons_edges():
    b = mc.woven("ring4", 2, 3, 12, 17)
    base = _rule(b, b["det_of"], b["n_persons"])
    # det_of = -1 and q >= n_persons: the camera is outside every set of that person, the other person is untouched
    det = b["det_of"].copy()
    det[:, 2, 0] = -1
    a = _rule(b, det, b["n_persons"])
    npers = b["n_persons"].copy()
    npers[:, 2] = b["det_of"][:, 2, 0]                        # person 0's detection is the first one behind the count
    c = _rule(b, b["det_of"], npers)
    assert not (a["views"][:, 0] & 4).any() and (base["views"][:, 0] & 4).any()
    _same(a, base, 1)
    _same(c, a, 0)
    # every camera but one gone: fewer than two views is the zero record
    det = b["det_of"].copy()
    det[:, 1:, 0] = -1
    z = _rule(b, det, b["n_persons"])
    assert not z["xyzs"][:, 0].any() and not z["views"][:, 0].any() and not z["resid"][:, 0].any() and not z["pscore"][:, 0].any()
    # an n_persons above Pmax counts as Pmax; n_persons None means Pmax everywhere
    big = _rule(b, b["det_of"], np.full_like(b["n_persons"], 1000))
    none = _rule(b, b["det_of"], None)
    for p in range(2):
        _same(big, base, p)
        _same(none, base, p)
    # det_of = None equals det_of[..., p] = p (and P = Pmax: the decoy is a person too)
    ident = np.broadcast_to(np.arange(3, dtype=np.int32), (12, 4, 3))
    x, y = _rule(b, None, b["n_persons"]), _rule(b, ident, b["n_persons"])
    assert x["xyzs"].shape == (12, 3, 17, 4)
    for p in range(3):
        _same(x, y, p)
    with pytest.raises(ValueError, match="det_of"):
        matched.triangulate_matched_reference(b["K"], b["R"], b["t"], b["kpts"], b["det_of"][:, :3], None)
    # two persons naming one detection get the same record
    det = b["det_of"].copy()
    det[..., 1] = det[..., 0]
    two = _rule(b, det, b["n_persons"])
    _same(two, two, 0, 1)
    _same(two, base, 0)


def test_what_it_buys_on_crossing():
    """The handed-in records are 88.2 mm RMS from the truth; re-triangulated from all matched views the rule gives 7.48 mm with
    det_true and 7.57 mm with the det_of of assign_detections_reference: both below 9 mm."""
    cs = mc.crossing()
    handed = mc.rms_error(cs["xyzs"], cs["X"])
    print(f"handed-in records: {handed * 1e3:.2f} mm")
    assert handed > 0.05
    for which in ("true", "assign"):
        ref = mc.reference(("crossing", which), 6.0, 1)
        rms = mc.rms_error(ref["xyzs"], cs["X"])
        close = int((ref["margin"] < 1e-6).sum())
        print(f"det_of {which}: RMS {rms * 1e3:.2f} mm, margins under 1e-6: {close} of {ref['margin'].size}")
        assert rms < 0.009
        assert close <= 0.001 * ref["margin"].size


def test_near_ties_are_rare_on_the_gpu_inputs():
    """At most 0.1 % of a batch's joints may have margin < 1e-6 (the GPU file then demands equal masks there or the alternative)."""
    for name in ("ring2", "ring4", "ring8"):
        for tau, md in rc.SETTINGS:
            ref = mc.reference(("woven", name, 2, 3, 17, 17, "float32"), tau, md)
            assert (ref["margin"] < 1e-6).sum() <= 0.001 * ref["margin"].size, (name, tau, md)
    ref = mc.reference(("divergence",), 6.0, 6)
    assert (ref["margin"] < 1e-6).sum() <= 0.001 * ref["margin"].size
    # ... and the alternative of a batch without near ties is the batch's own masks
    b = mc.woven("ring4", 2, 3, 17, 17)
    ref = mc.reference(("woven", "ring4", 2, 3, 17, 17, "float32"), 6.0, 6)
    alt = matched.alternative_views(b["K"], b["R"], b["t"], b["kpts"], b["det_of"], b["n_persons"], mc.KTHR, 6.0, 6, ref)
    assert np.array_equal(alt, ref["views"])
    forced = matched.alternative_views(b["K"], b["R"], b["t"], b["kpts"], b["det_of"], b["n_persons"], mc.KTHR, 6.0, 6, ref, below=np.inf)
    assert forced.shape == ref["views"].shape and (forced != ref["views"]).any()


def test_signatures_exports_and_header():
    import snowmocap_amd
    from snowmocap_amd import _lib
    assert snowmocap_amd.triangulate_matched is matched.triangulate_matched and "triangulate_matched_reference" in snowmocap_amd.__all__
    assert "snowtri_triangulate_matched" in _lib.exported_symbols()
    sig = inspect.signature(_lib.Context.triangulate_matched).parameters
    assert [sig[k].default for k in ("det_of", "n_persons", "keypoint_score_threshold", "reproj_threshold_px", "max_drops", "dtype",
                                     "diagnostics", "stream")] == [None, None, 0.0, 6.0, 1, None, False, None]
    hdr = open(os.path.join(ROOT, "include", "snowtri.h")).read()
    assert "Matched triangulation" in hdr and "int snowtri_triangulate_matched(" in hdr
    from snowmocap_amd import pipeline, pose
    assert inspect.signature(pipeline.TrackPipeline.run).parameters["retriangulate"].default is None
    assert inspect.signature(pose.refine_rig).parameters["retriangulate"].default is False
    assert matched.retriangulate_args(None) is None and matched.retriangulate_args(8) == (8.0, 6.0, 1)
    assert matched.retriangulate_args((8.0, 4.0)) == (8.0, 4.0, 1) and matched.retriangulate_args([8, 4, 2]) == (8.0, 4.0, 2)
    for bad in ((), (1, 2, 3, 4), 0.0, True, (6.0, 6.0, 1.5)):
        with pytest.raises(ValueError, match="retriangulate"):
            matched.retriangulate_args(bad)


def test_merge_keeps_the_first_pass_where_the_second_made_no_record():
    first = np.arange(2 * 3 * 4, dtype=np.float64).reshape(1, 2, 3, 4)
    again = -np.ones_like(first)
    views = np.array([[[0, 5, 0], [3, 0, 9]]], dtype=np.uint32)
    out, mask = matched.merge_records(first, again, views)
    assert np.array_equal(_bits(out[views == 0]), _bits(first[views == 0])) and (out[views != 0] == -1).all()
    assert mask.dtype == np.uint32 and np.array_equal(mask, np.where(views == 0, 0xFFFFFFFF, views))


def test_refine_rig_retriangulate_by_the_rules_on_the_two_person_recipe():
    """refine_rig(reference=True, triangulate=pose_cases.dlt_points, retriangulate=True) on pose_cases.recipe(P=2): every figure of the
    history is finite, the held cameras keep their bits, and without the option the call is what it was (the option is off by default)."""
    import pose_cases as pc
    from snowmocap_amd import pose
    rp = pc.recipe(P=2)
    bad = rp["bad"]
    kw = dict(free=[bad], rounds=1, triangulate=pc.dlt_points, reference=True, params=dict(keypoint_score_threshold=0.5))
    R, t, hist = pose.refine_rig(rp["K"], rp["Rd"], rp["td"], rp["kpts"], retriangulate=True, **kw)
    assert len(hist) == 2 and np.isfinite(R).all() and np.isfinite(t).all()
    for h in hist:
        assert all(np.isfinite(np.asarray(v, dtype=np.float64)).all() for v in h.values()), h
    print("    bad camera's view RMS per round:", [round(float(h["view_rms"][bad]), 3) for h in hist])
    keep = [c for c in range(R.shape[0]) if c != bad]
    assert np.array_equal(_bits(R[keep]), _bits(np.ascontiguousarray(rp["Rd"][keep])))
    a = pose.refine_rig(rp["K"], rp["Rd"], rp["td"], rp["kpts"], **kw)
    b = pose.refine_rig(rp["K"], rp["Rd"], rp["td"], rp["kpts"], retriangulate=False, **kw)
    assert np.array_equal(_bits(a[0]), _bits(b[0])) and np.array_equal(_bits(a[1]), _bits(b[1]))


def test_matched_entry_rejects_bad_arguments_under_asan(tmp_path):
    """`make asan` + tests/abi_badargs_matched.c, built and run exactly as tests/test_assign_host.py does for
    tests/abi_badargs_assign.c: a stand-alone C program on the CPU (no device visible), nothing preloaded."""
    import glob
    import shutil
    import subprocess
    csrc = os.path.join(ROOT, "snowmocap_amd", "csrc")
    so = os.path.join(csrc, "build", "libsnowtri_asan.so")
    clang = "/opt/rocm/lib/llvm/bin/clang"
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    if not (os.path.exists(hipcc) or shutil.which("hipcc")) or not os.path.exists(clang):
        pytest.skip("no ROCm toolchain (hipcc + its clang) on this machine: the ASan build of the C ABI cannot be made")
    sources = glob.glob(os.path.join(csrc, "*.hip")) + glob.glob(os.path.join(csrc, "*.hpp")) + [os.path.join(ROOT, "include", "snowtri.h")]
    if not os.path.exists(so) or os.path.getmtime(so) < max(os.path.getmtime(f) for f in sources):   # (the target always rebuilds: ~1 min)
        subprocess.check_call(["make", "-C", csrc, "-s", "asan"])
    exe = str(tmp_path / "abi_badargs_matched")
    subprocess.check_call([clang, "-std=c99", "-fsanitize=address", "-g", "-I", os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "tests", "abi_badargs_matched.c"), "-o", exe, so, "-Wl,-rpath," + os.path.dirname(so)])
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=0:abort_on_error=0", HIP_VISIBLE_DEVICES="", ROCR_VISIBLE_DEVICES="")
    p = subprocess.run([exe], env=env, capture_output=True, text=True, timeout=120)
    assert p.returncode == 0 and "0 failure(s)" in p.stdout, p.stdout[-3000:] + p.stderr[-3000:]
    assert "AddressSanitizer" not in p.stderr, p.stderr[-3000:]
