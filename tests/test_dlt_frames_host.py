"""The DLT definition (oracle/dlt.py: solved in the rig's own frame) against a 50-digit solve of the same definition
(oracle/dlt_exact.py), without a GPU, wherever the rig stands: the six placements of dlt_frames_cases on ring rigs of 2, 4 and 8
cameras and on a rig with per-camera intrinsics, the same pixels everywhere.

Bounds, with s the rig scale of the definition: the fp64 SVD oracles and the robust rule's reference within 1e-12 s of the exact
point (an fp64 SVD of the 2N x 4 matrix A in the rig frame is backward stable: errors of a few eps s times the conditioning
~1e2..1e3 of the smallest singular vector at 1 px of noise, 1e-13 s at the most), residuals within 1e-9 px, equal view masks.
"""
import functools

import mpmath as mp
import numpy as np
import pytest

import dlt_frames_cases as fc
from oracle import dlt as odlt
from oracle import dlt_exact as ex
from snowmocap_amd import synth
from snowmocap_amd.robust import triangulate_robust_reference

RIGS = ("ring2", "ring4", "ring8", "mixed5")
KTHR = 3.0
J = 6
CASES = [(r, p) for r in RIGS for p in fc.PLACEMENTS]


@functools.lru_cache(maxsize=None)
def pixels(rig_name):
    """One frame of J joints at home, 1 px of noise, float64; joint 1 loses camera 0 to the score gate, joint 2 has one view only."""
    K, R, t = fc.rig(rig_name)
    rng = np.random.default_rng(2024)
    X = synth.make_people(rng, 1, 1, J=J)
    kp, _ = synth.make_keypoints(rng, K, R, t, X, pixel_sigma=1.0, score_range=(3.5, 8.0), dtype=np.float64)
    kp = kp.copy()
    if K.shape[0] > 2:
        kp[0, 0, 0, 1, 2] = 1.0
    kp[0, 1:, 0, 2, 2] = 1.0
    kp.setflags(write=False)
    return K, R, t, X, kp


def _obs(kp, j, kthr=KTHR):
    return [(c, kp[0, c, 0, j, 0], kp[0, c, 0, j, 1]) for c in range(kp.shape[1]) if not kp[0, c, 0, j, 2] < kthr]


@functools.lru_cache(maxsize=None)
def exact_points(rig_name, placement):
    K, R, t, X, kp = pixels(rig_name)
    tp, _, _, _ = fc.place(t, None, placement)
    Ps, c, s = ex.projection_matrices_exact(K, R, tp)
    out = np.zeros((J, 3))
    for j in range(J):
        obs = _obs(kp, j)
        if len(obs) >= 2:
            out[j] = [float(x) for x in ex.dlt_point_exact(Ps, c, s, obs)]
    out.setflags(write=False)
    return out


@pytest.mark.parametrize("rig_name,placement", CASES)
def test_dlt_batch_and_point_against_the_exact_reference(rig_name, placement):
    K, R, t, X, kp = pixels(rig_name)
    tp, Xp, u, D = fc.place(t, X, placement)
    s = fc.rig_scale(tp)
    want = exact_points(rig_name, placement)
    got, pscore, count = odlt.dlt_batch(K, R, tp, kp, KTHR, J)
    err = np.abs(got[0, 0, :, :3] - want).max()
    print(f"{rig_name} {placement}: s = {s:.6g}, dlt_batch max |err| = {err:.3e} = {err / s:.2e} s")
    assert err <= 1e-12 * s
    assert not got[0, 0, 2].any() and not want[2].any()                   # one view: the zero record
    live = [j for j in range(J) if j != 2]
    assert np.abs(got[0, 0, live, :3] - Xp[0, 0, live]).max() < 0.05 * u  # (it is the placed scene)
    P, ctr, scl = odlt.rig_projection_matrices(K, R, tp)
    for j in live:
        obs = [(c, kp[0, c, 0, j, 0], kp[0, c, 0, j, 1], kp[0, c, 0, j, 2]) for c in range(K.shape[0])]
        xyz, score = odlt._dlt_point(P, obs, KTHR, ctr, scl)
        assert np.abs(xyz - want[j]).max() <= 1e-12 * s
        assert score == got[0, 0, j, 3]


@pytest.mark.parametrize("rig_name,placement", CASES)
def test_the_exact_point_does_not_depend_on_the_placement(rig_name, placement):
    """The definition is equivariant: the exact point of a placement, brought home, is the exact point at home (to the rounding of
    the placed camera centres: an ulp of u |t + D|, far below 1e-12 s here... in metres: 1e-13 m at the site placements)."""
    tp = fc.place(pixels(rig_name)[2], None, placement)[0]
    s_home = fc.rig_scale(pixels(rig_name)[2])
    back = fc.home(exact_points(rig_name, placement), placement)
    live = [j for j in range(J) if j != 2]
    ulp_t = np.spacing(np.abs(tp).max()) / fc.PLACEMENTS[placement][0]
    assert np.abs(back[live] - exact_points(rig_name, "home")[live]).max() <= 1e-12 * s_home + 8 * ulp_t


@functools.lru_cache(maxsize=None)
def _multi_batch():
    """3 cameras, 2 persons 1.5 m apart, permuted person order, 0.5 px of noise."""
    K, R, t = synth.ring_rig(3)
    rng = np.random.default_rng(77)
    X = synth.make_people(rng, 1, 2, J=4)
    kp, npers = synth.make_keypoints(rng, K, R, t, X, pixel_sigma=0.5, permute_persons=True, dtype=np.float64)
    return K, R, t, X, kp, npers


@pytest.mark.parametrize("placement", list(fc.PLACEMENTS))
def test_dlt_multi_batch_against_the_exact_reference(placement):
    """Two persons behind the reference's association: each output person is the exact DLT point of the (camera, person) rows that
    lie nearest to it in the image -- found from the placed truth, so the association is checked too."""
    from oracle import oracle as orc
    K, R, t, X, kp, npers = _multi_batch()
    tp, Xp, u, D = fc.place(t, X, placement)
    s = fc.rig_scale(tp)
    prm = dict(synth.default_thresholds(), average_score_threshold=1.0, condense_distance_tol=0.3, keypoint_num=4,
               center_point_index=1, keypoint_score_threshold=KTHR)
    prm = fc.place_params(prm, placement)
    out, pscore, count = odlt.dlt_multi_batch(K, R, tp, kp, npers, orc.make_params(**prm), 4)
    assert 2 <= count[0] <= 4                        # (the two persons, and what ghost clusters the association leaves)
    Ps, c, sc = ex.projection_matrices_exact(K, R, tp)
    uv_true, _ = synth.project(K, R, tp, Xp)                              # [C, F, P, J, 2]
    for who in range(2):
        dist = [np.linalg.norm(out[0, k, 1, :3] - Xp[0, who, 1]) for k in range(count[0])]
        slot = int(np.argmin(dist))
        assert dist[slot] < 0.05 * u
        for j in range(4):
            obs = []
            for cam in range(3):
                listed = int(np.argmin([np.linalg.norm(kp[0, cam, p, j, :2] - uv_true[cam, 0, who, j]) for p in range(2)]))
                obs.append((cam, kp[0, cam, listed, j, 0], kp[0, cam, listed, j, 1]))
            want = np.array([float(x) for x in ex.dlt_point_exact(Ps, c, sc, obs)])
            assert np.abs(out[0, slot, j, :3] - want).max() <= 1e-12 * s, (placement, slot, j)


@functools.lru_cache(maxsize=None)
def _robust_pixels(rig_name):
    K, R, t, X, kp = pixels(rig_name)
    kp = kp.copy()
    C = K.shape[0]
    kp[0, C - 1, 0, 0, 0] += 90.0                     # one camera wrong about joint 0
    kp[0, 0, 0, 4, 1] -= 60.0                         # two cameras wrong about joint 4
    kp[0, C // 2, 0, 4, 0] += 75.0
    kp.setflags(write=False)
    return kp


@pytest.mark.parametrize("max_drops", [1, 6])
@pytest.mark.parametrize("rig_name,placement", CASES)
def test_robust_reference_against_the_exact_rule(rig_name, placement, max_drops):
    K, R, t, X, _ = pixels(rig_name)
    kp = _robust_pixels(rig_name)
    tp, Xp, u, D = fc.place(t, X, placement)
    s = fc.rig_scale(tp)
    ref = triangulate_robust_reference(K, R, tp, kp, None, KTHR, J, 6.0, max_drops)
    Ps, c, sc = ex.projection_matrices_exact(K, R, tp)
    for j in range(J):
        obs = _obs(kp, j)
        if len(obs) < 2:
            assert ref["views"][0, j] == 0 and not ref["xyzs"][0, 0, j].any() and ref["resid"][0, j] == 0.0
            continue
        xyz, views, resid, margin = ex.robust_point_exact(Ps, c, sc, obs, 6.0, max_drops)
        assert margin > 1e-6, (j, margin)             # (no decision of the fixture is one that rounding could move)
        assert ref["views"][0, j] == views, (rig_name, placement, j, ref["views"][0, j], views)
        err = np.abs(ref["xyzs"][0, 0, j, :3] - np.array([float(x) for x in xyz])).max()
        assert err <= 1e-12 * s, (rig_name, placement, j, err)
        assert abs(ref["resid"][0, j] - float(resid)) <= 1e-9, (rig_name, placement, j)
    if K.shape[0] >= 4:
        assert bin(int(ref["views"][0, 0])).count("1") == len(_obs(kp, 0)) - 1         # the outlier went


def test_normal_equations_in_world_coordinates_miss_the_exact_answer():
    """Why the frame matters (a regression guard on the model behind the definition): A^T A formed in fp64 from the WORLD-frame
    matrices P = K [R^T | -R^T t] of a millimetre rig in site coordinates, solved by eigh (at least as accurate as the kernels'
    inverse iteration), misses the exact answer of that same world-frame problem by more than a millimetre; formed from the
    rig-frame matrices it is within 1e-12 s of the exact answer of the definition."""
    worst_world, worst_rig = 0.0, 0.0
    for rig_name in ("ring2", "ring4", "ring8"):
        K, R, t, X, kp = pixels(rig_name)
        tp, Xp, u, D = fc.place(t, X, "mm-site")
        s = fc.rig_scale(tp)
        Pw = odlt.projection_matrices(K, R, tp)
        Pr, ctr, scl = odlt.rig_projection_matrices(K, R, tp)
        Psw, cw, sw = ex.projection_matrices_exact(K, R, tp, frame="world")
        for j in (0, 3, 4, 5):
            obs = _obs(kp, j)

            def normal_equations(P):
                A = np.array([row for c, uu, vv in obs for row in (uu * P[c, 2] - P[c, 0], vv * P[c, 2] - P[c, 1])])
                e = np.linalg.eigh(A.T @ A)[1][:, 0]
                return e[:3] / e[3]
            exact_world = np.array([float(x) for x in ex.dlt_point_exact(Psw, cw, sw, obs)])
            worst_world = max(worst_world, np.abs(normal_equations(Pw) - exact_world).max() / u)
            worst_rig = max(worst_rig, np.abs(ctr + scl * normal_equations(Pr) - exact_points(rig_name, "mm-site")[j]).max() / s)
    print(f"A^T A in fp64, mm-site: world frame misses its exact answer by {worst_world:.3e} m, rig frame by {worst_rig:.3e} s")
    assert worst_world > 1e-3
    assert worst_rig <= 1e-12
