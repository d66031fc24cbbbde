"""The chained NumPy rule of TrackPipeline.run and its stage-wise check (tests/pipeline_cases.py), on the CPU alone:

  * the scenes reach the edges by the rules alone (conditions on the INPUTS: if one fails, the scene is changed, not the assertion):
    a slot carrying two ids, a bridged run, a person born after frame 0 and one gone for good, a two-frame spike, fill codes 1, 2
    and 3, a control point invalid at the start of a sequence and valid later, more than 90 % of the refined joints MOVED, frames
    with tracked < count[0] in the ordered walk -- each in the cases whose options can show it; and every det_of decision (the
    refinement's and the reprojection's) is separated from its runner-up and from the gate by more than a relative 1e-9, so the
    integer comparison on the GPU cannot hinge on rounding;
  * the NumPy projection is within reproject_cases.BAR_F64_RAW of the 50-digit pixel on the scenes' own joints: its half of the
    4e-11 px view_rms is held to;
  * check_stages accepts reference_run for every case of the GPU matrix;
  * check_stages rejects each planted mistake of pipeline_cases.PLANTS, naming the stage.
"""
import numpy as np
import pytest

import pipeline_cases as pc
import reproject_cases as rpc
from snowmocap_amd import _lib
from snowmocap_amd.reproject import _project

MEASURED, LERP, HOLD, MISSING = 0, 1, 2, 3
HAND_R_POLE = 13


def _runs(cid):
    sc, opts = pc.case(cid)
    return sc, opts, pc.reference_run(sc, opts), pc.reference_run(sc, dict(opts, refine=None))


@pytest.mark.parametrize("cid", list(pc.CASES))
def test_the_scene_reaches_the_edges_by_the_rules_alone(cid):
    sc, opts, res, plain = _runs(cid)
    P = sc["slots"]
    walk, track = sc["name"] in ("walk", "kn130"), opts["ragged"] == "track"
    seqs = pc.sequences(res, opts, P)
    assert seqs and all(len(idx) for _, idx in seqs)
    if walk:
        assert res["count"].tolist() == [3] * 20 + [2] * 4 + [3] * 12 + [2] * 14 + [3] * 22
    else:
        assert (res["count"] == P).all()
    if walk and track:
        tid = res["track_id"]
        ids = [np.unique(tid[:, i][tid[:, i] >= 0]) for i in range(P)]
        assert max(len(v) for v in ids) >= 2, "no slot carries two ids"
        first = {int(one): int(np.nonzero(tid == one)[0].min()) for v in ids for one in v}
        last = {int(one): int(np.nonzero(tid == one)[0].max()) for v in ids for one in v}
        assert max(first.values()) > 0 and min(last.values()) < pc.F - 1, "nobody is born after frame 0, or nobody leaves for good"
        if opts["fill_gaps"] and opts["track_max_missed"] >= 4:
            b = res["bridged"]
            assert b.any() and (b[20:24].sum(axis=1) == 1).all() and b.sum() == 4, "person 2's four frames are not bridged"
    if walk and not track:
        assert (res["tracked"] < res["count"][0]).any() and (res["tracked"] == np.minimum(res["count"], 3)).all()
    if opts["despike"]:
        codes = res["spike_codes"]
        a, b = pc.SPIKE_FRAMES
        there = [i for i, idx in seqs if a in idx and b in idx]
        assert there and all(codes[a, i, pc.SPIKE_JOINT] == codes[b, i, pc.SPIKE_JOINT] == pc.DESPIKE_SPIKE for i in there), "no two-frame spike"
    if opts["fill_gaps"]:
        assert set(np.unique(res["fill"]).tolist()) >= {LERP, HOLD, MISSING}
        for i, idx in seqs:
            if idx[0] == 0:
                assert (res["fill"][0:3, i, 77] == HOLD).all() and (res["fill"][0:16, i, 112] == MISSING).all()
    # the hold: hand_r_pole is invalid at the start of a sequence that begins at frame 0 (its joints 112 and 117 are missing there) and valid later
    held = 0
    for i, idx in seqs:
        v = res["valid"][idx, i, HAND_R_POLE]
        if idx[0] == 0:
            assert not v[0] and v[-1] and not v[:16].any(), (i, v.tolist())
            assert np.isnan(res["points"][idx[0], i, HAND_R_POLE, :3]).all() and not res["points_smoothed"][idx[1], i, HAND_R_POLE].any()
            held += 1
    assert held >= 1
    if opts["refine"] is not None:
        codes = res["refine_codes"]
        refined = codes >= _lib.REFINE_KEPT
        assert refined.sum() > 0.85 * (codes != _lib.REFINE_MISSING).sum() and (codes == pc.REFINE_MOVED).sum() > 0.9 * refined.sum()
        assert not np.array_equal(res["xyzs"], plain["xyzs"])


def _margins(cs, cn, gate):
    """the relative distance of every match decision from flipping: best mean against the runner-up and against the gate"""
    with np.errstate(all="ignore"):
        mean = np.where(cn >= 8, cs / np.maximum(cn, 1), np.inf)
    srt = np.sort(mean, axis=-1)
    best = srt[..., 0]
    has = np.isfinite(best)
    out = [np.abs(best[has] - gate * gate) / (gate * gate)]
    if mean.shape[-1] > 1:
        second = srt[..., 1]
        both = has & np.isfinite(second)
        out.append((second[both] - best[both]) / second[both])
    return np.concatenate(out)


@pytest.mark.parametrize("cid", [c for c, v in pc.CASES.items() if v[2].get("reproject") is not None])
def test_no_match_decision_hinges_on_rounding(cid):
    sc, opts, res, plain = _runs(cid)
    listed = plain["xyzs_listed"] if opts["ragged"] == "track" else plain["xyzs"]
    _, _, _, det_of, cs, cn = pc.refine_rule(sc, opts, listed)
    rp = pc.reproject_rule(sc, opts, res["xyzs"])
    m = np.concatenate([_margins(cs, cn, pc.refine_args(opts["refine"])[1]), _margins(rp["cost_sum"], rp["cost_n"], float(opts["reproject"]))])
    print(f"    {cid}: smallest relative margin of a det_of decision {m.min():.3e} over {m.size} decisions")
    assert m.size and m.min() > 1e-9
    # the listed persons are matched in at least two views (the refinement has something to work on; the one exception is frame 6 of
    # the DLT walk, where the oracle's greedy clustering merges observations of two persons into one), and nobody shares a detection
    there = np.arange(det_of.shape[2])[None, :] < res["count"][:, None]
    assert ((det_of >= 0).sum(axis=1) >= 2)[there].mean() > 0.99 and not res["shared"].any()


@pytest.mark.parametrize("cid", ["walk-track-all", "lens-all"])
def test_numpy_projection_against_the_50_digit_pixel(cid):
    """view_rms is held to 2 x BAR_F64_RAW = 4e-11 px: the kernel's distance from the exact raw pixel (tests/test_gpu_reproject.py) plus
    the NumPy rule's, measured here on the scene's own final joints.  An RMS moves by no more than its largest residual does."""
    sc, opts, res, _ = _runs(cid)
    K, R, t = sc["rig"]
    D, raw = sc["D"], sc["D"] is not None
    x = res["xyzs"]
    u, v, valid, _ = _project(K, R, t, D, raw, x)
    rng = np.random.default_rng(5)
    where = np.argwhere(valid)
    worst = 0.0
    for f, c, p, j in where[rng.choice(len(where), 120, replace=False)]:
        eu, ev, eur, evr, _, ratio = rpc.project_exact_mp(K[c], R[c], t[c], None if D is None else D[c], x[f, p, j, :3])
        assert float(ratio) <= rpc.DOMAIN
        worst = max(worst, abs(float((eur if raw else eu) - float(u[f, c, p, j]))), abs(float((evr if raw else ev) - float(v[f, c, p, j]))))
    print(f"    {cid}: NumPy projection within {worst:.3e} px of the exact pixel on 120 joints; its share of the {pc.VIEW_RMS_TOL:.1e} px bound "
          f"is {rpc.BAR_F64_RAW:.1e} px")
    assert worst <= rpc.BAR_F64_RAW


@pytest.mark.parametrize("cid", list(pc.CASES))
def test_the_check_accepts_the_rule(cid):
    sc, opts, res, plain = _runs(cid)
    st = pc.check_stages(res, plain, sc, opts, what=cid, verbose=False)
    assert len(st.worst) >= 8 and not st.failed


@pytest.mark.parametrize("plant", list(pc.PLANTS))
def test_the_check_rejects_a_planted_mistake(plant):
    cid, stages = pc.PLANTS[plant]
    sc, opts = pc.case(cid)
    good, plain = pc.reference_run(sc, opts), pc.reference_run(sc, dict(opts, refine=None))
    bad = pc.reference_run(sc, opts, plant=plant)
    assert set(bad) == set(good)
    with pytest.raises(pc.StageMiss) as info:
        pc.check_stages(bad, plain, sc, opts, what=plant, verbose=False)
    print(f"    {info.value}"[:400])
    assert info.value.stages[0] in stages, info.value.stages
    # ... and nothing upstream of the mistake was touched: the stages before it pass
    order = ["keys", "triangulation", "refine", "tracking", "despike", "fill", "smoothed", "points", "points_smoothed", "reproject"]
    assert all(order.index(s) >= min(order.index(x) for x in stages) for s in info.value.stages)


def test_a_difference_upstream_does_not_flip_a_verdict_downstream():
    """Every rule is fed the previous stage as found in the result: refined joints moved by 1e-9 m (inside the refine bound) carry
    through tracking, despiking, filling and the filters of a consistent chain, and the check still accepts it."""
    sc, opts = pc.case("walk-track-all")
    plain = pc.reference_run(sc, dict(opts, refine=None))
    K, R, t = sc["rig"]
    listed = np.array(pc.refine_rule(sc, opts, plain["xyzs_listed"])[0], copy=True)
    moved = ~pc.missing_records(listed)
    listed[..., 0][moved] += 1e-9
    res = dict(pc.reference_run(sc, opts))
    # the chain downstream of the shifted records, by the same rules
    trk = pc.tracking_rule(sc, opts, listed, res["count"])
    res.update(xyzs_listed=listed, xyzs=trk["xyzs"], slot_of=trk["slot_of"], track_id=trk["track_id"], present=trk["present"], tracked=trk["tracked"],
               bridged=trk["bridged"], track_flags=trk["track_flags"])
    seqs = pc.sequences(res, opts, sc["slots"])
    res["xyzs_despiked"], res["spike_codes"] = pc.despike_rule(res["xyzs"], seqs, opts)
    res["xyzs_filled"], res["fill"] = pc.fill_rule(res["xyzs_despiked"], res["xyzs"], seqs, opts)
    res["smoothed"] = pc.smoothed_rule(sc, res["xyzs_filled"], seqs)
    res["points"], res["valid"] = pc.points_rule(res["smoothed"], seqs)
    res["points_smoothed"] = pc.points_smoothed_rule(sc, res["points"], res["valid"], seqs)
    rp = pc.reproject_rule(sc, opts, res["xyzs"])
    res.update({k: rp[k] for k in ("det_of", "shared", "view_rms", "view_n")})
    pc.check_stages(res, plain, sc, opts, what="shifted by 1e-9 m", verbose=False)
    assert 1e-9 < (pc.REFINE_XYZ * pc.rfc.rig_scale(t))
