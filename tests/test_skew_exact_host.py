"""The default (skew-ray) method's exact rule (oracle/skew_exact.py, 50 digits) on the rigs, placements and scenes of
tests/skew_cases.py, without a GPU:

  * the scenes reach the edges the rule has -- both sides of every threshold, a wrong pairing that joins a person's cluster, one that
    forms its own, a dropped person, a truncated list, a joint nobody scores -- and are WELL POSED: no decision of the exact rule
    is closer than 1e-9 (relative) to its threshold at any placement, no frame holds an exactly singular pair;
  * the fp64 C oracle (oracle/snowtri_oracle.c: the reference's arithmetic) meets, against the exact rule, the very bounds the
    kernels are held to (skew_cases.compare), at every case and placement: the bounds are attainable by plain fp64 arithmetic;
  * equivariance of the rule itself: the exact persons of every placement, brought home, are the exact home persons to 1e-30;
  * teeth: skew_cases.compare rejects the oracle with each of six planted mistakes and names what failed.
"""
import mpmath as mp
import numpy as np
import pytest

import dlt_frames_cases as fc
import skew_cases as sk
from oracle import skew_exact as sx

ALL = list(sk.CASES)


def _each():
    for name in ALL:
        for placement in sk.placements(sk.scene(name)["rig_name"]):
            yield name, placement, sk.exact(name, placement)


def test_scenes_reach_the_edges_and_are_well_posed():
    seen = dict(dist_in=0, dist_out=0, cand_kept=0, cand_dropped=0, centre_in=0, centre_out=0, person_kept=0, person_dropped=0,
                ghost_merged=0, ghost_own=0, truncated=0, dead=0, gate_below=0, empty_list=0, ragged=0, no_person=0)
    smallest = (np.inf, None, None, None)
    frames = singular = 0
    for name, placement, r in _each():
        m, which = sx.smallest_margin(r)
        if m < smallest[0]:
            smallest = (m, which, name, placement)
        frames += len(r["count"])
        singular += int((r["status"] != 0).sum())
        if placement != "home":
            continue
        sc, prm = sk.scene(name), sk.scene(name)["prm"]
        C, P = sc["K"].shape[0], sc["kpts"].shape[2]
        d = np.array([float(x) for x in r["dists"]])
        seen["dist_in"] += int((d <= prm["distance_threshold"]).sum())
        seen["dist_out"] += int((d > prm["distance_threshold"]).sum())
        if prm["average_score_threshold"] > 0:
            cm = np.array([float(x) for x in r["cand_means"]])
            seen["cand_kept"] += int((cm >= prm["average_score_threshold"]).sum())
            seen["cand_dropped"] += int(((cm < prm["average_score_threshold"]) & (cm > 0)).sum())    # (a TRUE candidate dropped, not only ghosts at 0)
        cd = np.array([float(x) for x in r["centre_dists"]])
        seen["centre_in"] += int((cd <= prm["condense_distance_tol"]).sum())
        seen["centre_out"] += int((cd > prm["condense_distance_tol"]).sum())
        if prm["condense_score_tol"] > 0:
            pm = np.array([float(x) for x in r["person_means"]])
            seen["person_kept"] += int((pm >= prm["condense_score_tol"]).sum())
            seen["person_dropped"] += int(((pm < prm["condense_score_tol"]) & (pm > 0)).sum())
        for f in range(len(r["count"])):
            full = (sc["n_persons"][f] == P).all()
            # a cluster larger than the camera pairs holds a wrong pairing; more persons than people: a wrong pairing of its own
            seen["ghost_merged"] += sum(1 for mm in r["members"][f] if len(mm) > C * (C - 1) // 2)
            seen["ghost_own"] += int(full and r["count"][f] > P)
            seen["truncated"] += int(r["count"][f] > sc["pout"])
            seen["no_person"] += int(r["count"][f] == 0)
            k = min(int(r["count"][f]), sc["pout"])
            seen["dead"] += int((r["kscore"][f, :k] == 0).sum())
        live = sc["kpts"][..., 2][sc["kpts"][..., 2] != 0]
        seen["gate_below"] += int((live < sk.KTHR).sum())
        seen["empty_list"] += int((sc["n_persons"] == 0).sum())
        seen["ragged"] += int(((sc["n_persons"] > 0) & (sc["n_persons"] < P)).sum())
    print(f"\n    edges met at home: {seen}")
    print(f"    smallest decision margin over {frames} frames (all placements): {smallest[0]:.3e} ({smallest[1]}, {smallest[2]} at {smallest[3]}); "
          f"frames with an exactly singular pair: {singular}; frames left out of a comparison: 0")
    assert all(v > 0 for v in seen.values()), {k: v for k, v in seen.items() if not v}
    assert smallest[0] >= sk.MARGIN_MIN, smallest
    assert singular == 0
    # the "band" case sits where it says: inside the 1e-6 in which the streaming association re-does a decision exactly
    for placement in sk.placements("rolled3"):
        mg = sk.exact("m-rolled3-band", placement)["margins"]
        assert 5e-8 < float(min(mg["candidate_mean"])) < 2e-7 and 5e-8 < float(min(mg["person_mean"])) < 2e-7, (placement, min(mg["candidate_mean"]))


def test_fp64_oracle_meets_the_bounds_against_the_exact_rule():
    """The bounds of skew_cases.compare (float64 outputs) hold for the reference's own arithmetic in fp64 at every placement, site
    coordinates included: no bound had to be replaced by a measured one."""
    from oracle import oracle as orc
    missed = []
    worst = {}
    for name, placement, want in _each():
        sc = sk.scene(name)
        tp, Xp, prm, u = sk.placed(name, placement)
        got = sk.oracle_result(sc["K"], sc["R"], tp, sc["kpts"], sc["n_persons"], prm, sc["pout"])
        fails, fig = sk.compare(got, want, tp, np.float64, u, Xtrue=Xp, dead=sc["dead"])
        worst[placement] = max(worst.get(placement, 0.0), fig.get("xyz", 0.0))
        missed += [f"{name} [{placement}] {q}: {msg}" for q, msg in fails]
        if placement == "home":                               # membership: the kept candidates and every cluster's size
            for f in range(len(want["count"])):
                res = orc.human_triangulation_frame(sc["K"], sc["R"], tp, sc["kpts"][f], sc["n_persons"][f], orc.make_params(**prm))
                if res["enum_index"].tolist() != want["kept"][f]:
                    missed.append(f"{name} frame {f}: kept candidates {res['enum_index'].tolist()} vs the rule's {want['kept'][f]}")
                con = orc.condense_frame(res, orc.make_params(**prm))
                if [int(v) for v in con["member_count"]] != [len(m) for m in want["members"][f]]:
                    missed.append(f"{name} frame {f}: cluster sizes {con['member_count']} vs {[len(m) for m in want['members'][f]]}")
    print("\n    fp64 oracle against the exact rule, worst xyz error / bound per placement: " + ", ".join(f"{k} {v:.3g}" for k, v in worst.items()))
    assert not missed, " | ".join(missed[:8])


def test_exact_rule_is_equivariant():
    worst = 0.0
    for name in ALL:
        sc = sk.scene(name)
        h = sk.exact(name, "home")
        for placement in sk.placements(sc["rig_name"]):
            if placement == "home":
                continue
            r = sk.exact(name, placement)
            u, D = fc.PLACEMENTS[placement]
            assert np.array_equal(r["count"], h["count"]) and r["kept"] == h["kept"] and r["members"] == h["members"], (name, placement)
            with mp.workdps(sx.DIGITS):
                for f in range(len(h["count"])):
                    for pr, ph in zip(r["xyz_mp"][f], h["xyz_mp"][f]):
                        for xr, xh in zip(pr, ph):
                            if not any(xh):                   # a joint nobody scores stays (0, 0, 0): not moved with the rig
                                assert not any(xr), (name, placement, f)
                                continue
                            for a in range(3):
                                worst = max(worst, float(abs(xr[a] / mp.mpf(u) - mp.mpf(float(D[a])) - xh[a]) / max(abs(xh[a]), mp.mpf(1))))
            # the scores scale by 1 / u exactly
            assert np.allclose(r["pscore"] * u, h["pscore"], rtol=1e-14, atol=0.0), (name, placement)
    print(f"\n    exact persons brought home vs exact home persons: worst relative difference {worst:.3e}")
    assert worst <= 1e-30


def _oracle(sc, K, R, tp, prm):
    return sk.oracle_result(K, R, tp, sc["kpts"], sc["n_persons"], prm, sc["pout"])


def _mistake_skew(name):
    sc = sk.scene(name)
    K = sc["K"].copy()
    K[:, 0, 1] = 0.0
    return "home", _oracle(sc, K, sc["R"], sc["t"], sc["prm"])


def _mistake_principal_point(name):
    sc = sk.scene(name)
    K = sc["K"].copy()
    K[1, :2, 2] = K[2, :2, 2]
    return "home", _oracle(sc, K, sc["R"], sc["t"], sc["prm"])


def _mistake_roll(name):
    sc = sk.scene(name)
    _, _, _, rolls = sk.rolled_rig(sc["K"].shape[0], with_rolls=True)
    c, s = np.cos(-rolls[2]), np.sin(-rolls[2])
    R = sc["R"].copy()
    R[2] = R[2] @ np.array([[c, -s, 0.0], [s, c, 0.0], [0.0, 0.0, 1.0]])
    assert np.allclose(R[2][:, 2], sc["R"][2][:, 2])          # the same optical axis, the roll taken out
    return "home", _oracle(sc, sc["K"], R, sc["t"], sc["prm"])


def _mistake_t0(name):
    sc = sk.scene(name)
    tp, _, prm, _ = sk.placed(name, "moved")
    got = _oracle(sc, sc["K"], sc["R"], tp, prm)
    got["xyz"] = np.where((got["kscore"] != 0)[..., None], got["xyz"] - tp[0], got["xyz"])
    return "moved", got


def _mistake_units(name):
    sc = sk.scene(name)
    tp = sk.placed(name, "mm")[0]
    return "mm", _oracle(sc, sc["K"], sc["R"], tp, sc["prm"])    # (the thresholds of home, in metres, on a millimetre rig)


def _mistake_reverse(name):
    sc = sk.scene(name)
    r = sx.evaluate(sk._prepared(sk._scene_key(name)), sc["t"], sc["prm"], sc["pout"], reverse_condense=True)
    return "home", dict(xyz=r["xyz"], kscore=r["kscore"], pscore=r["pscore"], count=r["count"], status=r["status"])


MISTAKES = [("the skew term zeroed", _mistake_skew, "s-rolled4", {"xyz", "kscore", "count"}),
            ("camera 1's principal point taken from camera 2", _mistake_principal_point, "s-rolled4", {"xyz", "kscore", "count"}),
            ("camera 2's roll removed from R", _mistake_roll, "s-rolled4", {"xyz", "kscore", "count"}),
            ("t_0 not added back to the fused point", _mistake_t0, "s-rolled4", {"xyz"}),
            ("thresholds not scaled at mm", _mistake_units, "m-rolled3-tight", {"count", "kscore", "dead joint"}),
            ("the condense running in reverse order", _mistake_reverse, "m-rolled3-ghosts", {"xyz", "count", "kscore"})]


@pytest.mark.parametrize("what,make,name,expect", MISTAKES, ids=[m[0] for m in MISTAKES])
def test_comparison_rejects_a_planted_mistake(what, make, name, expect):
    """The routine the GPU tests use must reject each mistake and say which quantity failed; unplanted, the same case passes
    (test_fp64_oracle_meets_the_bounds_against_the_exact_rule)."""
    sc = sk.scene(name)
    placement, got = make(name)
    tp, Xp, prm, u = sk.placed(name, placement)
    fails, _ = sk.compare(got, sk.exact(name, placement), tp, np.float64, u, Xtrue=Xp, dead=sc["dead"])
    assert fails, f"{what}: not rejected"
    print(f"\n    {what}: rejected on {sorted({q for q, _ in fails})}; first: {fails[0][0]}: {fails[0][1][:140]}")
    assert expect & {q for q, _ in fails}, (what, fails[0])
