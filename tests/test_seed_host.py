"""Seeding on the host (no GPU): the NumPy rules seed.pair_cost_reference and seed.seed_persons_reference (include/snowtri.h,
"Seeding") on the recipes the feature was proposed with, the pair cost against a 50-digit evaluation of its rule on general rigs at
six placements (the FLOOR of tests/seed_cases.py), the edges of both rules, the signatures of the Python entries, and the C entries
refusing bad arguments under AddressSanitizer (tests/abi_badargs_seed.c against the `make asan` library).
"""
import inspect
import os
import re

import numpy as np
import pytest

import assign_cases as ac
import pose_cases as pc
import seed_cases as sc
from conftest import ROOT
from snowmocap_amd import seed as sd


# ------------------------------------------------------------------------------------------------ the recipes
@pytest.mark.parametrize("gate", [0.02, 0.03, 0.05])
def test_crossing_from_no_persons_at_all(gate):
    """every detection free, threshold 0.5, min_views 3: exactly the three persons in 60 of 60 frames, each seed a column of det_true"""
    cs = ac.crossing()
    ps, pn = sd.pair_cost_reference(cs["K"], cs["R"], cs["t"], cs["kpts"], cs["n_persons"], None, ac.CROSS_THRESHOLD)
    det, ns, flags = sd.seed_persons_reference(ps, pn, cs["n_persons"], None, None, gate, 8, 3)
    assert det.shape == (ac.CROSS_F, 4, 4) and det.dtype == np.int32 and ns.dtype == np.int32 and flags.dtype == np.uint32
    assert (ns == 3).all() and not flags.any()
    for f in range(ac.CROSS_F):
        assert {tuple(det[f, :, s]) for s in range(3)} == {tuple(cs["det_true"][f, :, p]) for p in range(3)}, f
        assert (det[f, :, 3] == -1).all()


def test_two_persons_on_the_nudged_rig():
    """pose_cases.recipe(P=2) on the calibration that no longer holds (the reference's association overflows there in 40 of 40
    frames): gate 0.05 finds the 2 true persons on all 8 views in every frame; gate 0.02 finds them on 7, the nudged camera in
    neither."""
    r = pc.recipe(P=2)
    ps, pn = sd.pair_cost_reference(r["K"], r["Rd"], r["td"], r["kpts"], None, None, 0.0)
    det, ns, _ = sd.seed_persons_reference(ps, pn, None, None, 2, 0.05, 8, 3)
    assert (ns == 2).all() and (det >= 0).all()
    for f in range(det.shape[0]):                                # (the recipe's lists are not permuted: detection p is person p)
        assert all((det[f, :, s] == det[f, 0, s]).all() for s in range(2)) and {det[f, 0, 0], det[f, 0, 1]} == {0, 1}, f
    det, ns, _ = sd.seed_persons_reference(ps, pn, None, None, 2, 0.02, 8, 3)
    assert (ns == 2).all() and (det[:, r["bad"]] == -1).all()
    others = np.delete(det, r["bad"], axis=1)
    assert (others >= 0).all() and (others == others[:, :1]).all() and (np.sort(others[:, 0], axis=-1) == [0, 1]).all()


# ------------------------------------------------------------------------------------------------ 50 digits
def test_reference_against_the_exact_rule():
    """pair_cost_reference against rules 1-4 in 50 digits on the general rigs at their placements, both keypoint types: pair_n is
    exact, and the largest |sqrt(mean) - sqrt(mean_exact)| / s IS the floor the kernel's bar is made of -- the committed constant
    must be within a factor of two of what is measured here."""
    worst, where, n_pairs = 0.0, None, 0
    for case in sc.exact_cases():
        s = sc.exact_scene(*case)
        root, n, _ = sc.exact_values(*case)
        ps, pn = sd.pair_cost_reference(s["K"], s["R"], s["t"], s["kpts"], s["n_persons"], s["claimed"], s["thr"])
        assert np.array_equal(pn, n) and pn.dtype == np.int32, case
        assert (ps[pn == 0] == 0).all()
        err = float(np.abs(sc.root_mean(ps, pn) - root).max()) / s["s"]
        n_pairs += int((n > 0).sum())
        if err > worst:
            worst, where = err, case
    print(f"    floor: {worst:.3e} at {where}; {n_pairs} pairs with joints")
    assert n_pairs > 2000
    assert sc.FLOOR / 2 <= worst <= sc.FLOOR * 2, (worst, sc.FLOOR)


def test_the_exact_rule_is_the_same_at_every_placement():
    """(a check of the checker) the line distance depends on t_b - t_a alone, exact on the 2^-20 grid of skew_cases.rig: a placement
    scales every root by its unit and changes nothing else beyond the last digit"""
    home = sc.exact_values("rolled4", "home")
    for pl in ("site", "mm-site"):
        got, s = sc.exact_values("rolled4", pl), sc.exact_scene("rolled4", pl)
        assert np.array_equal(got[1], home[1])
        assert np.allclose(got[0], home[0] * s["u"], rtol=1e-15, atol=0)


# ------------------------------------------------------------------------------------------------ edges of the pair cost
def _two_cameras():
    K = np.tile(np.array([[700.0, 0.0, 640.0], [0.0, 700.0, 360.0], [0.0, 0.0, 1.0]]), (2, 1, 1))
    R = np.tile(np.eye(3), (2, 1, 1))
    t = np.array([[0.0, 0.0, 0.0], [1.0, 0.0, 0.0]])
    return K, R, t


def test_pair_cost_edges():
    K, R, t = _two_cameras()
    kn = 4
    kp = np.zeros((1, 2, 2, kn, 3))
    kp[..., 0], kp[..., 1], kp[..., 2] = 640.0, 360.0, 1.0                  # every ray is the optical axis: parallel
    ps, pn = sd.pair_cost_reference(K, R, t, kp)
    assert (pn == 0).all() and (ps == 0).all()                               # nn == 0 does not count
    kp[0, 0, :, :, 0] = 640.0 + 70.0 * np.arange(kn)                         # camera 0 looks right, camera 1 straight ahead, both in the plane y = 0
    kp[0, 1, 1, :, 1] = 360.0 + 7.0                                          # ... detection 1 of camera 1 looks down by 0.01
    ps, pn = sd.pair_cost_reference(K, R, t, kp)
    assert pn[0, 0, 0, 0] == kn - 1 and ps[0, 0, 0, 0] == 0.0                 # joint 0 is still parallel; coplanar lines meet
    assert pn[0, 0, 0, 1] == kn and ps[0, 0, 0, 1] > 0
    want = sc.exact_pair_cost(K, R, t, kp)
    assert np.array_equal(pn, want[1]) and np.allclose(ps, want[2], rtol=1e-13)
    bad = kp.copy()
    bad[0, 0, 0, 1, 0] = np.nan                                              # a NaN pixel does not count
    bad[0, 1, 1, 2, 1] = np.inf
    bad[0, 1, 1, 3, 2] = 0.2                                                 # ... nor a score under the threshold
    ps2, pn2 = sd.pair_cost_reference(K, R, t, bad, keypoint_score_threshold=0.5)
    assert pn2[0, 0, 0, 1] == kn - 3 and pn2[0, 0, 1, 1] == kn - 2 and np.isfinite(ps2).all()
    # a claimed member, or one behind n_persons, gives (0, 0) -- whatever its keypoints hold
    poison = kp.copy()
    poison[0, 0, 1] = np.nan
    poison[0, 1, 0] = np.inf
    claimed = np.array([[[-1, 3], [-1, -1]]])
    npers = np.array([[2, 2]])
    ps3, pn3 = sd.pair_cost_reference(K, R, t, poison, npers, claimed)
    assert (pn3[0, 0, 1, :] == 0).all() and (ps3[0, 0, 1, :] == 0).all() and pn3[0, 0, 0, 1] == kn and pn3[0, 0, 0, 0] == 0
    ps4, pn4 = sd.pair_cost_reference(K, R, t, poison, np.array([[1, 2]]), None)
    assert np.array_equal(pn4, pn3) and np.array_equal(ps4, ps3)
    ps5, pn5 = sd.pair_cost_reference(K, R, t, kp, np.zeros((1, 2), dtype=np.int32))
    assert (pn5 == 0).all() and (ps5 == 0).all()
    with pytest.raises(ValueError, match="NaN"):
        sd.pair_cost_reference(K, R, t, kp, keypoint_score_threshold=float("nan"))
    with pytest.raises(ValueError, match="256"):
        sd.pair_cost_reference(K, R, t, np.zeros((1, 2, 1, 257, 3)))
    with pytest.raises(ValueError, match="2 to 8 cameras"):
        sd.pair_cost_reference(np.tile(K[:1], (9, 1, 1)), np.tile(R[:1], (9, 1, 1)), np.zeros((9, 3)), np.zeros((1, 9, 1, 2, 3)))


# ------------------------------------------------------------------------------------------------ edges of the grouping
def _arrays(C, Pmax, edges, n=10):
    """(pair_sum, pair_n) [1, NP, Pmax, Pmax] with the given {(x, y): mean} (x < y nodes), every other pair far outside any gate"""
    pairs = {(int(a), int(b)): k for k, (a, b) in enumerate(sd.camera_pairs(C))}
    cs = np.full((1, len(pairs), Pmax, Pmax), 1e6 * n)
    cn = np.full(cs.shape, n, dtype=np.int32)
    for (x, y), m in edges.items():
        cs[0, pairs[x // Pmax, y // Pmax], x % Pmax, y % Pmax] = m * n
    return cs, cn


def _rule(C, Pmax, edges, S=None, gate=1.0, min_joints=8, min_views=3, n_persons=None, claimed=None, n=10):
    det, ns, fl = sd.seed_persons_reference(*_arrays(C, Pmax, edges, n), n_persons, claimed, S, gate, min_joints, min_views)
    return det[0], int(ns[0]), int(fl[0])


def test_a_rejected_pair_returns_its_members_to_the_pool():
    """C = 4, one detection each: the cheapest edge (0, 1) cannot grow (node 1 has no other edge), so min_views = 3 rejects it and
    node 0 is free again for the triangle (0, 2, 3) that follows"""
    edges = {(0, 1): 0.01, (0, 2): 0.2, (0, 3): 0.3, (2, 3): 0.25}
    det, ns, fl = _rule(4, 1, edges)
    assert ns == 1 and det[:, 0].tolist() == [0, -1, 0, 0] and fl == 0
    det, ns, fl = _rule(4, 1, edges, min_views=2)                            # ... and with min_views = 2 the pair is a seed, the rest another
    assert ns == 2 and det[:, 0].tolist() == [0, 0, -1, -1] and det[:, 1].tolist() == [-1, -1, 0, 0]


def test_ties_go_to_the_lowest_pair_and_the_lowest_node():
    edges = {(0, 2): 0.5, (1, 3): 0.5, (0, 3): 0.5, (1, 2): 0.5}             # C = 2, Pmax = 2: nodes 0, 1 | 2, 3, all equal
    det, ns, _ = _rule(2, 2, edges, min_views=2)
    assert ns == 2 and det[:, 0].tolist() == [0, 0] and det[:, 1].tolist() == [1, 1]      # (0, 2) first, then (1, 3)
    # growing: nodes 4 and 5 (camera 2) both complete the pair (0, 2) at the same largest edge -> node 4
    edges = {(0, 2): 0.1, (0, 4): 0.3, (2, 4): 0.2, (0, 5): 0.2, (2, 5): 0.3}
    det, ns, _ = _rule(3, 2, edges)
    assert ns == 1 and det[:, 0].tolist() == [0, 0, 0]
    edges[(2, 5)] = 0.29                                                      # ... and node 5 as soon as its largest edge is smaller
    det, ns, _ = _rule(3, 2, edges)
    assert ns == 1 and det[:, 0].tolist() == [0, 0, 1]


def test_a_chain_is_not_a_clique():
    """0 - 1 - 2 - 3 connected through single edges: no three nodes are mutually close, nothing is chained together"""
    edges = {(0, 1): 0.1, (1, 2): 0.1, (2, 3): 0.1}
    assert _rule(4, 1, edges)[1] == 0
    det, ns, _ = _rule(4, 1, edges, min_views=2)
    assert ns == 2 and det[:, 0].tolist() == [0, 0, -1, -1] and det[:, 1].tolist() == [-1, -1, 0, 0]


def test_full_flag_and_admissibility():
    tri = {(0, 2): 0.1, (0, 4): 0.1, (2, 4): 0.1, (1, 3): 0.2, (1, 5): 0.2, (3, 5): 0.2}      # two persons on three cameras
    det, ns, fl = _rule(3, 2, tri, S=1)
    assert ns == 1 and fl == sd.FLAG_FULL and det.shape == (3, 1) and det[:, 0].tolist() == [0, 0, 0]
    det, ns, fl = _rule(3, 2, tri, S=2)
    assert ns == 2 and fl == 0 and det[:, 1].tolist() == [1, 1, 1]                              # S reached, but nothing is left
    one = {(0, 2): 0.1, (0, 4): 0.1, (2, 4): 0.1}
    assert _rule(3, 2, one, S=1)[1:] == (1, 0)
    # admissibility: the mean exactly at gate2 passes, the next double does not; too few joints; a NaN sum
    assert _rule(3, 2, one, gate=np.sqrt(0.1) if np.sqrt(0.1) ** 2 >= 0.1 else np.nextafter(np.sqrt(0.1), 1))[1] == 1
    assert _rule(3, 2, one, gate=0.3)[1] == 0
    assert _rule(3, 2, one, n=7)[1] == 0 and _rule(3, 2, one, n=8)[1] == 1
    cs, cn = _arrays(3, 2, one)
    cs[0, 0, 0, 0] = np.nan
    assert sd.seed_persons_reference(cs, cn)[1][0] == 0
    # nobody listed: no seeds; a claimed node is out of the pool
    assert _rule(3, 2, tri, n_persons=np.zeros((1, 3), dtype=np.int32))[1] == 0
    det, ns, _ = _rule(3, 2, tri, claimed=np.array([[[0, -1], [-1, -1], [-1, -1]]]))
    assert ns == 1 and det[:, 0].tolist() == [1, 1, 1]
    det, ns, _ = _rule(3, 2, tri, n_persons=np.array([[2, 1, 2]], dtype=np.int32))
    assert ns == 1 and det[:, 0].tolist() == [0, 0, 0]


def test_permuting_the_lists_permutes_the_seeds_and_nothing_else():
    """Every camera's list permuted, claimed permuted alike: seed_det_of's values follow the permutation, n_seeds, flags and the
    order of the seeds stay -- on inputs without exact ties, and the recipe has none: two admissible weights of a frame closer than
    1e-9 (relative) occur in no frame of it."""
    cs = ac.crossing()
    F, C, Pmax = cs["kpts"].shape[:3]
    rng = np.random.default_rng(7)
    claimed = np.where(rng.random((F, C, Pmax)) < 0.1, 0, -1).astype(np.int32)
    ps, pn = sd.pair_cost_reference(cs["K"], cs["R"], cs["t"], cs["kpts"], cs["n_persons"], claimed, ac.CROSS_THRESHOLD)
    assert sc.near_tie_share(ps, pn, 0.03 ** 2, 8, C, Pmax) == 0.0
    base = sd.seed_persons_reference(ps, pn, cs["n_persons"], claimed, None, 0.03, 8, 3)
    perm = np.stack([[rng.permutation(Pmax) for _ in range(C)] for _ in range(F)])            # new position i holds old detection perm[i]
    kp2 = np.take_along_axis(cs["kpts"], perm[..., None, None], axis=2)
    cl2 = np.take_along_axis(claimed, perm, axis=2)
    ps2, pn2 = sd.pair_cost_reference(cs["K"], cs["R"], cs["t"], kp2, cs["n_persons"], cl2, ac.CROSS_THRESHOLD)
    got = sd.seed_persons_reference(ps2, pn2, cs["n_persons"], cl2, None, 0.03, 8, 3)
    back = np.where(got[0] >= 0, np.take_along_axis(perm, np.maximum(got[0], 0), axis=2), -1)
    assert np.array_equal(back, base[0]) and np.array_equal(got[1], base[1]) and np.array_equal(got[2], base[2])
    assert (base[1] >= 2).all() and (base[1] < 3).any()                                           # (claimed detections cost some seeds)


@pytest.mark.parametrize("name", sc.FAMILIES)
def test_families_behave_as_described(name):
    """the synthetic weight families of the GPU test do what their names say under the rule"""
    C, Pmax = 4, 3
    cs, cn, npers, claimed = sc.family(name, C, Pmax, 20)
    det, ns, fl = sd.seed_persons_reference(cs, cn, npers, claimed, None, sc.GATE, sc.MIN_JOINTS, 3)
    inverse = (det >= 0).sum(axis=1)                                                               # views per seed slot
    assert ((inverse == 0) | (inverse >= 3)).all()
    for f in range(20):                                                                           # no detection in two seeds
        for c in range(C):
            used = det[f, c][det[f, c] >= 0]
            assert len(set(used.tolist())) == len(used)
    if name == "inadmissible" or name == "chains":
        assert (ns == 0).all()
    if name == "clique":
        assert (ns == 1).all() and (det[:, :, 0] == 0).all()
    if name == "rejects":
        assert (ns == 1).all() and (det[:, :3, 0] == 0).all() and (det[:, 3, 0] == -1).all()
    if name in ("floats", "ties"):
        assert (ns > 0).any()


# ------------------------------------------------------------------------------------------------ the chain and the entries
def test_reference_chain_recovers_the_crossing_persons():
    """triangulate_seeded_reference from no persons at all on a few frames of the recipe: three persons, each within the matched
    triangulation's accuracy of one true person (1 px of noise at 4.5 m on 4 views: centimetres per joint, millimetres in the mean)"""
    cs = ac.crossing()
    sl = slice(28, 32)                                                                            # the frames in which A and B pass
    out = sd.triangulate_seeded_reference(cs["K"], cs["R"], cs["t"], cs["kpts"][sl, :, :, :24], cs["n_persons"][sl], None, 3, 0.03, 3, 8,
                                          ac.CROSS_THRESHOLD)
    assert (out["n_seeds"] == 3).all() and out["xyzs"].shape == (4, 3, 24, 4)
    for f in range(4):
        for s in range(3):
            p = int(np.nonzero((cs["det_true"][sl][f, 0] == out["seed_det_of"][f, 0, s]))[0][0])
            err = np.linalg.norm(out["xyzs"][f, s, :, :3] - cs["X"][sl][f, p, :24], axis=-1)
            assert err.max() < 0.05 and np.sqrt((err ** 2).mean()) < 0.02, (f, s, err.max())


def test_seeded_triangulator_drops_into_refine_rig():
    """refine_rig(reference=True) with the seeded association as its triangulation step, on a small two-person recording with one
    nudged camera: it runs, and the view RMS of the nudged camera falls"""
    from snowmocap_amd import pose
    r = pc.recipe(C=4, bad=1, F=10, P=2, kn=17)
    tri = sd.seeded_triangulator(2, 0.05, reference=True)
    first = tri(r["K"], r["Rd"], r["td"], r["kpts"], None)
    assert first.shape == (10, 2, 17, 4) and (first[..., 3] != 0).all()
    out = pose.refine_rig(r["K"], r["Rd"], r["td"], r["kpts"], free=[1], rounds=2, triangulate=tri, reference=True, min_obs=6, one_to_one=True)
    hist = out[2]
    assert hist[-1]["view_rms"][1] < hist[0]["view_rms"][1]


def test_signatures_defaults_exports_and_header():
    import snowmocap_amd
    from snowmocap_amd import _lib, pipeline
    for name in ("pair_cost", "pair_cost_reference", "seed_persons", "seed_persons_reference", "triangulate_seeded",
                 "triangulate_seeded_reference", "seeded_triangulator"):
        assert getattr(snowmocap_amd, name) is getattr(sd, name) and name in snowmocap_amd.__all__
    assert {"snowtri_pair_cost", "snowtri_seed_persons"} <= set(_lib.exported_symbols())
    sig = inspect.signature(sd.triangulate_seeded).parameters
    assert [sig[k].default for k in ("n_persons", "claimed", "gate", "min_views", "min_joints", "keypoint_score_threshold",
                                     "reproj_threshold_px", "max_drops", "diagnostics")] == [None, None, 0.05, 3, 8, 0.0, 6.0, 1, False]
    sig = inspect.signature(_lib.Context.seed_persons).parameters
    assert [sig[k].default for k in ("n_persons", "claimed", "S", "gate", "min_joints", "min_views", "with_flags", "stream")] == \
        [None, None, None, 0.05, 8, 3, False, None]
    sig = inspect.signature(_lib.Context.pair_cost).parameters
    assert [sig[k].default for k in ("n_persons", "claimed", "keypoint_score_threshold", "stream")] == [None, None, 0.0, None]
    assert inspect.signature(pipeline.TrackPipeline.run).parameters["seed"].default is None
    assert _lib.SEED_FLAG_FULL == sd.FLAG_FULL == 1
    header = open(os.path.join(ROOT, "include", "snowtri.h")).read()
    for word in ("Seeding:", "int snowtri_pair_cost(", "int snowtri_seed_persons(", "#define SNOWTRI_SEED_FLAG_FULL 1u", "BIT FOR BIT"):
        assert word in header, word
    assert "seeding new persons from the detections nobody" not in header
    readme = open(os.path.join(ROOT, "README.md")).read()
    assert "seeding new persons from `person_of`'s unclaimed detections" not in readme and "triangulate_seeded" in readme


def test_argument_errors():
    cs, cn = np.zeros((1, 6, 2, 2)), np.ones((1, 6, 2, 2), dtype=np.int32)

    class NoContext:
        def seed_persons(self, *a, **k):
            raise AssertionError("the arguments are checked before the library is asked")

    for fn in (sd.seed_persons_reference, lambda *a, **k: sd.seed_persons(NoContext(), *a, **k)):
        for kw, word in ((dict(min_joints=0), "min_joints must be >= 1"), (dict(gate=-1.0), "gate must be >= 0 and not NaN"),
                         (dict(gate=float("nan")), "gate must be >= 0 and not NaN"), (dict(gate=1e200), "gate must not exceed 1e150"),
                         (dict(gate=float("inf")), "gate must not exceed 1e150"), (dict(min_views=1), "min_views must lie in 2..C"),
                         (dict(min_views=5), "min_views must lie in 2..C"), (dict(S=0), "S must lie in 1..64"), (dict(S=65), "S must lie in 1..64")):
            with pytest.raises(ValueError, match=re.escape(word)):
                fn(cs, cn, **kw)
        with pytest.raises(ValueError, match=re.escape("C * Pmax must not exceed 64")):
            fn(np.zeros((1, 6, 17, 17)), np.ones((1, 6, 17, 17), dtype=np.int32))
        with pytest.raises(ValueError, match="camera pairs"):
            fn(np.zeros((1, 5, 2, 2)), np.ones((1, 5, 2, 2), dtype=np.int32))
        with pytest.raises(ValueError, match=re.escape("[F, NP, Pmax, Pmax]")):
            fn(cs, cn[..., :1])
    for bad in (True, (0.03, 1), (0.03, 3, 0), -0.1, (0.03, 3, 8, 1), float("nan")):
        with pytest.raises(ValueError, match="seed"):
            sd.seed_option(bad)
    assert sd.seed_option(None) is None and sd.seed_option(0.03) == (0.03, 3, 8) and sd.seed_option((0.02, 2)) == (0.02, 2, 8)


def test_seed_entries_reject_bad_arguments_under_asan(tmp_path):
    """`make asan` + tests/abi_badargs_seed.c, built and run exactly as tests/test_matched_host.py does for
    tests/abi_badargs_matched.c: a stand-alone C program on the CPU (no device visible), nothing preloaded."""
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
    exe = str(tmp_path / "abi_badargs_seed")
    subprocess.check_call([clang, "-std=c99", "-fsanitize=address", "-g", "-I", os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "tests", "abi_badargs_seed.c"), "-o", exe, so, "-Wl,-rpath," + os.path.dirname(so)])
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=0:abort_on_error=0", HIP_VISIBLE_DEVICES="", ROCR_VISIBLE_DEVICES="")
    p = subprocess.run([exe], env=env, capture_output=True, text=True, timeout=120)
    assert p.returncode == 0 and "0 failure(s)" in p.stdout, p.stdout[-3000:] + p.stderr[-3000:]
    assert "AddressSanitizer" not in p.stderr, p.stderr[-3000:]
