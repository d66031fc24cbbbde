"""The one-to-one assignment on the host (no GPU): the NumPy rule reproject.assign_detections_reference (include/snowtri.h,
"Assignment") against an exhaustive minimum, against scipy, against match_detections where the two must agree, on the collision it
exists for and on the edges of admissibility; the arguments of the Python entries; and the C entry refusing bad arguments under
AddressSanitizer (tests/abi_badargs_assign.c against the `make asan` library).
"""
import inspect
import os
import re

import numpy as np
import pytest

import assign_cases as ac
from conftest import ROOT
from snowmocap_amd import reproject as rp

EPS = float(np.finfo(np.float64).eps)


def _rule(cs, cn, gate_px=ac.GATE_PX, min_joints=ac.MIN_JOINTS):
    """one problem [P, Pmax] -> (det_of [P], person_of [Pmax], total)"""
    d, p, t = rp.assign_detections_reference(np.asarray(cs)[None, None], np.asarray(cn)[None, None], gate_px, min_joints)
    return d[0, 0], p[0, 0], float(t[0, 0])


def _check_matching(det_of, person_of, total, mean):
    P, Pmax = mean.shape
    got = det_of[det_of >= 0]
    assert len(set(got.tolist())) == len(got) and (got < Pmax).all()                           # injective
    assert all(np.isfinite(mean[p, det_of[p]]) for p in range(P) if det_of[p] >= 0)            # every matched pair is admissible
    inverse = np.full(Pmax, -1, dtype=np.int64)
    for p in range(P):
        if det_of[p] >= 0:
            inverse[det_of[p]] = p
    assert np.array_equal(person_of, inverse)
    acc = 0.0
    for p in range(P):
        if det_of[p] >= 0:
            acc = acc + mean[p, det_of[p]]
    assert acc == total


# ------------------------------------------------------------------------------------------------ the exhaustive minimum
@pytest.mark.parametrize("P", [1, 2, 3, 4, 5])
def test_rule_attains_the_exhaustive_minimum(P):
    """Costs from {0, 12, 24, 36, 48} against gate2 = 36, over 8 joints: every sum is exact and ties are everywhere, so the rule's
    total + gate2 * (unmatched) must EQUAL the minimum over all partial one-to-one matchings."""
    for Pmax in range(1, 6):
        cs, cn = ac.family("ties", P, Pmax, 12)
        det_of, person_of, total = rp.assign_detections_reference(cs, cn, ac.GATE_PX, ac.MIN_JOINTS)
        mean = ac.means(cs, cn, ac.GATE2, ac.MIN_JOINTS)
        for i in range(cs.shape[0]):
            _check_matching(det_of[i, 0], person_of[i, 0], float(total[i, 0]), mean[i, 0])
            assert total[i, 0] + ac.GATE2 * int((det_of[i, 0] < 0).sum()) == ac.brute_force(mean[i, 0], ac.GATE2), (P, Pmax, i)
            assert np.array_equal(ac.scalar_rule(ac.augmented(mean[i, 0], ac.GATE2), Pmax), det_of[i, 0])


@pytest.mark.parametrize("name", ["floats", "inadmissible"])
def test_vector_and_scalar_forms_of_the_rule_agree(name):
    """the NumPy rule handles the columns of a step as one vector: the same matching as the scan one column at a time"""
    for P, Pmax in ((3, 5), (8, 9), (16, 16), (1, 63), (63, 1)):
        cs, cn = ac.family(name, P, Pmax, 4)
        det_of = rp.assign_detections_reference(cs, cn, ac.GATE_PX, ac.MIN_JOINTS)[0]
        mean = ac.means(cs, cn, ac.GATE2, ac.MIN_JOINTS)
        for i in range(4):
            assert np.array_equal(ac.scalar_rule(ac.augmented(mean[i, 0], ac.GATE2), Pmax), det_of[i, 0])


# ------------------------------------------------------------------------------------------------ scipy
SCIPY_SIZES = [(2, 3), (5, 5), (7, 4), (11, 11), (16, 17), (32, 32), (1, 63), (63, 1)]


@pytest.mark.parametrize("name", ac.FAMILIES)
def test_total_against_scipy(name):
    """scipy.optimize.linear_sum_assignment on the augmented matrix a [P, Pmax + P] gives the exact optimum up to the rounding of its
    own sum.  The rule's matching is optimal for the duals it carries, and those are rounded: a step of an insertion performs one
    rounding on each u, v and minv it touches, an insertion of row i has at most i + 1 steps but touches each of the Pmax + P
    columns' three numbers (v, minv, and the u of its row) about once per row inserted, so the objective collects about
    3 P (P + Pmax) roundings of values below 2 gate2, each at most eps / 2 * 2 gate2 = eps gate2.  The bar is that count times
    eps gate2 -- a few thousand eps of gate2 at 32 x 32 -- and it also covers the P roundings of either side's own sum."""
    from scipy.optimize import linear_sum_assignment
    worst = 0.0
    for P, Pmax in SCIPY_SIZES:
        n = 3 if P * Pmax >= 256 else 24
        cs, cn = ac.family(name, P, Pmax, n)
        det_of, _, total = rp.assign_detections_reference(cs, cn, ac.GATE_PX, ac.MIN_JOINTS)
        mean = ac.means(cs, cn, ac.GATE2, ac.MIN_JOINTS)
        bar = 3 * P * (P + Pmax) * EPS * ac.GATE2
        for i in range(n):
            a = ac.augmented(mean[i, 0], ac.GATE2)
            r, c = linear_sum_assignment(a)
            best = float(a[r, c].sum())
            got = float(total[i, 0]) + ac.GATE2 * int((det_of[i, 0] < 0).sum())
            worst = max(worst, abs(got - best) / ac.GATE2)
            assert abs(got - best) <= bar, (name, P, Pmax, i, got, best)
    print(f"    {name}: max |rule - scipy| = {worst:.2e} x gate2")


# ------------------------------------------------------------------------------------------------ the old matcher
def test_agrees_with_match_detections_where_nothing_is_shared():
    """Where match_detections reports no shared person and no row holds two equal means, the sum of the row minima (gate2 for a row
    without an admissible pair) is a lower bound that the assignment attains, and it is attained by that matching alone."""
    seen = 0
    for name in ac.FAMILIES:
        for P, Pmax in ((1, 5), (2, 6), (3, 5), (4, 5), (3, 12)):
            cs, cn = ac.family(name, P, Pmax, 40)
            old, shared = rp.match_detections(cs, cn, ac.GATE_PX, ac.MIN_JOINTS)
            new = rp.assign_detections_reference(cs, cn, ac.GATE_PX, ac.MIN_JOINTS)[0]
            mean = ac.means(cs, cn, ac.GATE2, ac.MIN_JOINTS)
            srt = np.sort(np.where(np.isfinite(mean), mean, np.arange(Pmax) + 1e9), axis=-1)
            distinct = Pmax == 1 or (srt[..., 1:] != srt[..., :-1]).all(axis=(-1, -2))
            use = ~shared.any(axis=-1) & distinct                          # (two inadmissible pairs are not two equal means)
            assert np.array_equal(new[use], old[use]) and new.dtype == old.dtype
            seen += int(use.sum())
    assert seen > 100


def test_the_collision():
    cn = np.full((2, 2), 10, dtype=np.int32)
    cs = np.array([[4.0, 20.0], [9.0, 16.0]]) * 10                       # both closest to detection 0; person 1 also fits detection 1
    old, shared = rp.match_detections(cs[None, None], cn[None, None], ac.GATE_PX)
    assert old[0, 0].tolist() == [0, 0] and shared.all()
    det_of, person_of, total = _rule(cs, cn)
    assert det_of.tolist() == [0, 1] and person_of.tolist() == [0, 1] and total == 20.0          # 4 + 16 < 20 + 9
    cs2 = np.array([[4.0, 6.0], [3.0, 30.0]]) * 10                       # ... and where the other permutation is the smaller sum
    det_of, person_of, total = _rule(cs2, cn)
    assert det_of.tolist() == [1, 0] and person_of.tolist() == [1, 0] and total == 9.0
    cs3 = np.array([[4.0, 50.0], [9.0, 40.0]]) * 10                      # detection 1 outside the gate: the worse-fitting person goes without
    det_of, person_of, total = _rule(cs3, cn)
    assert det_of.tolist() == [0, -1] and person_of.tolist() == [0, -1] and total == 4.0
    cs4 = np.array([[9.0, 50.0], [4.0, 40.0]]) * 10
    assert _rule(cs4, cn)[0].tolist() == [-1, 0]
    det, per, tot = rp.assign_detections_reference(np.stack([cs, cs3])[:, None], np.stack([cn, cn])[:, None], ac.GATE_PX)
    assert det.shape == (2, 1, 2) and det.dtype == np.int64 and per.shape == (2, 1, 2) and tot.shape == (2, 1) and tot.dtype == np.float64


def test_edges_of_admissibility():
    one = np.ones((1, 1))
    assert _rule(one * 7, np.full((1, 1), 7, dtype=np.int32))[0].tolist() == [-1]             # cost_n just below min_joints
    assert _rule(one * 8, np.full((1, 1), 8, dtype=np.int32))[0].tolist() == [0]              # ... and at it
    assert _rule(one * 36 * 8, np.full((1, 1), 8, dtype=np.int32)) [0].tolist() == [0]         # mean exactly gate2: admissible
    assert _rule(one * 36 * 8, np.full((1, 1), 8, dtype=np.int32))[2] == 36.0
    assert _rule(one * np.nextafter(36.0, 37.0) * 8, np.full((1, 1), 8, dtype=np.int32))[0].tolist() == [-1]
    cn = np.full((2, 3), 9, dtype=np.int32)
    cs = np.array([[np.nan, np.inf, 18.0], [9.0, np.nan, -np.inf]])
    det_of, person_of, total = _rule(cs, cn)
    assert det_of.tolist() == [2, 0] and person_of.tolist() == [1, -1, 0] and total == 3.0
    det_of, person_of, total = _rule(np.full((3, 2), np.nan), np.full((3, 2), 9, dtype=np.int32))   # nothing admissible
    assert det_of.tolist() == [-1, -1, -1] and person_of.tolist() == [-1, -1] and total == 0.0
    det_of, person_of, total = _rule(np.zeros((2, 2)), np.zeros((2, 2), dtype=np.int32))             # no joint counted (behind n_persons)
    assert det_of.tolist() == [-1, -1] and total == 0.0
    # gate_px = 0: only an exact 0 is admissible (a person against its own projection), and it ties with staying unmatched -- the
    # real column is the lower one and wins
    cs0 = np.array([[0.0, 1e-300], [0.0, 0.0]])
    det_of, person_of, total = _rule(cs0, np.full((2, 2), 8, dtype=np.int32), gate_px=0.0)
    assert det_of.tolist() == [0, 1] and total == 0.0
    assert _rule(cs0[:, ::-1], np.full((2, 2), 8, dtype=np.int32), gate_px=0.0)[0].tolist() == [1, 0]


def test_argument_errors():
    cs, cn = np.zeros((1, 1, 2, 2)), np.ones((1, 1, 2, 2), dtype=np.int32)

    class NoContext:
        def assign_detections(self, *a, **k):
            raise AssertionError("the arguments are checked before the library is asked")

    for fn in (rp.assign_detections_reference, lambda *a, **k: rp.assign_detections(NoContext(), *a, **k)):
        for args, word in (((cs, cn, 6.0, 0), "min_joints"), ((cs, cn, -1.0), "gate_px"), ((cs, cn, float("nan")), "gate_px"),
                           ((cs, cn, float("inf")), "gate_px must not exceed 1e150"), ((cs, cn, 1e200), "gate_px must not exceed 1e150"),
                           ((cs, cn, 1.0000001e150), "gate_px must not exceed 1e150"),
                           ((cs[0], cn[0], 6.0), "[F, C, P, Pmax]"), ((cs, cn[..., :1], 6.0), "[F, C, P, Pmax]"),
                           ((np.zeros((1, 1, 40, 25)), np.ones((1, 1, 40, 25), dtype=np.int32), 6.0), "P + Pmax <= 64"),
                           ((np.zeros((1, 1, 0, 2)), np.ones((1, 1, 0, 2), dtype=np.int32), 6.0), "P >= 1")):
            with pytest.raises(ValueError, match=re.escape(word)):
                fn(*args)
    for old, new in (("min_joints must be >= 1", (cs, cn, 6.0, 0)), ("gate_px must be >= 0 and not NaN", (cs, cn, -2.0))):
        with pytest.raises(ValueError) as a:
            rp.match_detections(*new)
        with pytest.raises(ValueError) as b:
            rp.assign_detections_reference(*new)
        assert str(a.value) == str(b.value) == old                                            # match_detections' wording
    import snowmocap_amd
    import snowmocap_amd.pipeline as pl
    import snowmocap_amd.pose as pose
    assert snowmocap_amd.assign_detections is rp.assign_detections and "assign_detections_reference" in snowmocap_amd.__all__
    assert "snowtri_assign_detections" in snowmocap_amd._lib.exported_symbols()
    assert inspect.signature(pl.TrackPipeline.run).parameters["one_to_one"].default is False
    assert inspect.signature(pose.refine_rig).parameters["one_to_one"].default is False
    sig = inspect.signature(snowmocap_amd._lib.Context.assign_detections).parameters
    assert [sig[k].default for k in ("min_joints", "with_person_of", "with_total", "stream")] == [8, False, False, None]


def test_a_gate_above_1e150_is_refused_by_the_callers_and_wide_gates_work():
    """Staying unmatched costs gate_px^2: match_detections reads an infinite gate as "no gate", the assignment refuses it -- in
    refine_rig before any work -- and up to the widest gate it takes (1e150) it matches as many persons as can be matched, one
    to one and on admissible pairs only, P > Pmax and inadmissible pairs included."""
    import pose_cases as pc
    from snowmocap_amd import pose
    cs = pc.recipe(C=4, bad=1, F=6, P=1, kn=17)

    def never(*a):
        raise AssertionError("refused before any work")

    for gate in (float("inf"), 1e200):
        with pytest.raises(ValueError, match=re.escape("gate_px must not exceed 1e150")):
            pose.refine_rig(cs["K"], cs["Rd"], cs["td"], cs["kpts"], free=[1], rounds=1, triangulate=never, reference=True, one_to_one=True,
                            gate_px=gate)
    assert rp.assign_gate(1e150) == 1e150 and rp.assign_gate(0) == 0.0
    from scipy.optimize import linear_sum_assignment
    for gate in (1e6, 1e150):
        for P, Pmax in ((4, 2), (2, 2), (3, 5), (4, 4)):
            c, n = ac.family("inadmissible", P, Pmax, 30)
            det_of, person_of, total = rp.assign_detections_reference(c, n, gate, ac.MIN_JOINTS)
            mean = ac.means(c, n, gate * gate, ac.MIN_JOINTS)
            for i in range(30):
                _check_matching(det_of[i, 0], person_of[i, 0], float(total[i, 0]), mean[i, 0])
                a = ac.augmented(mean[i, 0], gate * gate)
                r, q = linear_sum_assignment(a)
                assert int((det_of[i, 0] >= 0).sum()) == int((q < Pmax).sum())                 # as many persons matched as can be
                assert np.array_equal(ac.scalar_rule(a, Pmax), det_of[i, 0])


def test_refine_rig_reference_path_takes_the_numpy_rule():
    """refine_rig(reference=True, one_to_one=True) runs the NumPy rule; on a single-person recording it is the default's result"""
    import pose_cases as pc
    from snowmocap_amd import pose
    cs = pc.recipe(C=4, bad=1, F=6, P=1, kn=17)
    tri = lambda K, R, t, kp, npers: pc.dlt_points(K, R, t, kp, npers)     # noqa: E731
    kw = dict(free=[1], rounds=1, triangulate=tri, reference=True, min_obs=6)
    a = pose.refine_rig(cs["K"], cs["Rd"], cs["td"], cs["kpts"], **kw)
    b = pose.refine_rig(cs["K"], cs["Rd"], cs["td"], cs["kpts"], one_to_one=True, **kw)
    assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])


def test_assign_entry_rejects_bad_arguments_under_asan(tmp_path):
    """`make asan` + tests/abi_badargs_assign.c, built and run exactly as tests/test_refine_host.py does for
    tests/abi_badargs_refine.c: a stand-alone C program on the CPU (no device visible), nothing preloaded."""
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
    exe = str(tmp_path / "abi_badargs_assign")
    subprocess.check_call([clang, "-std=c99", "-fsanitize=address", "-g", "-I", os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "tests", "abi_badargs_assign.c"), "-o", exe, so, "-Wl,-rpath," + os.path.dirname(so)])
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=0:abort_on_error=0", HIP_VISIBLE_DEVICES="", ROCR_VISIBLE_DEVICES="")
    p = subprocess.run([exe], env=env, capture_output=True, text=True, timeout=120)
    assert p.returncode == 0 and "0 failure(s)" in p.stdout, p.stdout[-3000:] + p.stderr[-3000:]
    assert "AddressSanitizer" not in p.stderr, p.stderr[-3000:]
