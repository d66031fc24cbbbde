"""The default (skew-ray) method in 50-digit arithmetic (mpmath): what oracle/snowtri_oracle.c and the kernels are held to.

TEST INFRASTRUCTURE ONLY (see oracle/snowtri_oracle.c header for the rules).

The rule (include/snowtri.h; the line references of oracle/snowtri_oracle.c), on the fp64 VALUES of K, R, t, the float32 or float64
pixels and confidences and the thresholds, every step below in 50 digits:
  rays      h = R inv(K) (u, v, 1), not normalised;
  pair      a = hm.hm, b = hm.hs, c = hs.hs, det = a c - b^2, d = ts - tm, e = hm.d, f = hs.d,
            S0 = (c e - b f) / det, S1 = (a f - b e) / det, Wm = hm S0 + tm, Ws = -hs S1 + ts, dist = |Wm - Ws|, W = (Wm + Ws) / 2;
            det == 0 exactly: the pair is singular, the frame is reported (status 1), not evaluated;
  score     ((sm + ss) / 2) / (1000 dist), 0 when sm < kthr or ss < kthr or dist > dthr.  The confidences are DATA: with float32
            keypoints the reference adds and halves them as float32 scalars, and so does the rule (one float32 rounding of the sum);
  candidate mean of the J joint scores; dropped iff mean < average_score_threshold; candidates in the reference's loop order
            (camera pairs mc < sc, persons of mc, persons of sc);
  condense  greedy in list order: seeds 0 .. n-2 not absorbed yet, a later candidate is absorbed iff its centre joint is NOT further
            than condense_distance_tol from the SEED's; clusters smaller than condense_person_num_tol dropped (members stay absorbed);
  fusion    per joint b < keypoint_num: sum of the members' scores; sum == 0 -> (0, 0, 0, 0); else xyz = sum_i (s_i / sum) W_i,
            score = sum / members; person mean over keypoint_num, dropped iff mean < condense_score_tol;
  output    the first Pout_max persons; count is the number of persons before the cut.

Besides the persons the rule returns the MARGIN of every decision it took -- |x - threshold| / threshold of dist (where both
confidences pass: elsewhere the score is 0 whatever dist is), candidate mean, centre distance, person mean (a threshold <= 0 decides
nothing about non-negative means: no margin) -- and per pair item the sine between the two rays and det.

The rays, a, b, c and det do not depend on t: `prepare` forms them once, `evaluate` places the rig.
"""
import mpmath as mp
import numpy as np

DIGITS = 50


def _f(v):
    return mp.mpf(float(v))


def _dot(x, y):
    return x[0] * y[0] + x[1] * y[1] + x[2] * y[2]


def prepare(K, R, kpts, n_persons):
    """Everything of the rule that does not depend on t or a threshold.  kpts [F, C, Pmax, J, 3] float32 / float64, n_persons [F, C]."""
    kpts = np.asarray(kpts)
    assert kpts.dtype in (np.float32, np.float64)
    F, C, Pmax, J, _ = kpts.shape
    K, R = np.asarray(K, np.float64), np.asarray(R, np.float64)
    n_persons = np.asarray(n_persons).reshape(F, C)
    is32 = kpts.dtype == np.float32
    frames = []
    with mp.workdps(DIGITS):
        M = []
        for c in range(C):
            Km = mp.matrix([[_f(v) for v in row] for row in K[c]])
            Rm = mp.matrix([[_f(v) for v in row] for row in R[c]])
            Mc = Rm * mp.inverse(Km)
            M.append([[Mc[i, j] for j in range(3)] for i in range(3)])
        for f in range(F):
            rays = {}
            for c in range(C):
                for p in range(int(n_persons[f, c])):
                    hs = []
                    for j in range(J):
                        u, v = _f(kpts[f, c, p, j, 0]), _f(kpts[f, c, p, j, 1])
                        hs.append(tuple(M[c][i][0] * u + M[c][i][1] * v + M[c][i][2] for i in range(3)))
                    rays[c, p] = hs
            cands = []
            for mc in range(C - 1):
                for sc in range(mc + 1, C):
                    for pm in range(int(n_persons[f, mc])):
                        for ps in range(int(n_persons[f, sc])):
                            items = []
                            for j in range(J):
                                hm, hs = rays[mc, pm][j], rays[sc, ps][j]
                                a, b, c_ = _dot(hm, hm), _dot(hm, hs), _dot(hs, hs)
                                det = a * c_ - b * b
                                sm, ss = kpts[f, mc, pm, j, 2], kpts[f, sc, ps, j, 2]
                                half = _f((sm + ss) / np.float32(2)) if is32 else (_f(sm) + _f(ss)) / 2
                                items.append((hm, hs, a, b, c_, det, (1 / det if det != 0 else None), float(sm), float(ss), half))
                            cands.append((mc, sc, pm, ps, items))
            frames.append(cands)
    return dict(frames=frames, F=F, C=C, J=J)


def item_stats(prep):
    """-> (sine [n], det [n]) over every pair item of every frame, as float64 (an exactly singular item: sine 0, det 0)."""
    sines, dets = [], []
    with mp.workdps(DIGITS):
        for cands in prep["frames"]:
            for _, _, _, _, items in cands:
                for hm, hs, a, b, c, det, inv, sm, ss, half in items:
                    dets.append(float(det))
                    sines.append(float(mp.sqrt(det / (a * c))) if a * c != 0 and det > 0 else 0.0)
    return np.array(sines), np.array(dets)


def _rel(x, thr):
    return abs(x - thr) / abs(thr)


def evaluate(prep, t, prm, pout, reverse_condense=False):
    """The rule for the rig placed at t [C, 3] with the thresholds prm (a dict with the names of snowtri_params).
    -> dict: xyz [F, pout, kn, 3], kscore [F, pout, kn], pscore [F, pout], count [F], status [F] (1: an exactly singular pair), as
    float64 (every value rounded once); xyz_mp [F][person][joint] -> 3 mpf; kept [F] lists of enumeration indices of the kept
    candidates; members [F] lists (per output person before the cut) of lists of kept-candidate positions;
    margins: dict name -> list of mpf; n_singular.  reverse_condense is a planted mistake for the tests, never the rule."""
    F, C, J = prep["F"], prep["C"], prep["J"]
    kn, ci = int(prm["keypoint_num"]), int(prm["center_point_index"])
    if ci < 0:
        ci += J
    assert 0 <= ci < J and 0 <= kn <= J
    out = dict(xyz=np.zeros((F, pout, kn, 3)), kscore=np.zeros((F, pout, kn)), pscore=np.zeros((F, pout)), count=np.zeros(F, np.int32),
               status=np.zeros(F, np.int32), xyz_mp=[], kept=[], members=[], n_singular=0,
               margins=dict(distance=[], candidate_mean=[], centre=[], person_mean=[]), dists=[], cand_means=[], person_means=[],
               centre_dists=[], dead_joints=0)
    mg = out["margins"]
    with mp.workdps(DIGITS):
        tt = [[_f(v) for v in row] for row in np.asarray(t, np.float64).reshape(C, 3)]
        kthr, athr, dthr = float(prm["keypoint_score_threshold"]), _f(prm["average_score_threshold"]), _f(prm["distance_threshold"])
        ctol, ntol, stol = _f(prm["condense_distance_tol"]), float(prm["condense_person_num_tol"]), _f(prm["condense_score_tol"])
        for f in range(F):
            cands = prep["frames"][f]
            out["xyz_mp"].append([])
            out["kept"].append([])
            out["members"].append([])
            sing = sum(1 for cd in cands for it in cd[4] if it[6] is None)
            if sing:
                out["n_singular"] += sing
                out["status"][f] = 1
                continue
            kept = []                                       # (enumeration index, W [J], score [J])
            for idx, (mc, sc, pm, ps, items) in enumerate(cands):
                tm, ts = tt[mc], tt[sc]
                d = (ts[0] - tm[0], ts[1] - tm[1], ts[2] - tm[2])
                Ws, scs = [], []
                for hm, hs, a, b, c, det, inv, sm, ss, half in items:
                    e, g = _dot(hm, d), _dot(hs, d)
                    S0, S1 = (c * e - b * g) * inv, (a * g - b * e) * inv
                    wm = (hm[0] * S0 + tm[0], hm[1] * S0 + tm[1], hm[2] * S0 + tm[2])
                    ws = (ts[0] - hs[0] * S1, ts[1] - hs[1] * S1, ts[2] - hs[2] * S1)
                    df = (wm[0] - ws[0], wm[1] - ws[1], wm[2] - ws[2])
                    dist = mp.sqrt(_dot(df, df))
                    Ws.append(((wm[0] + ws[0]) / 2, (wm[1] + ws[1]) / 2, (wm[2] + ws[2]) / 2))
                    live = not (sm < kthr or ss < kthr)
                    if live:
                        mg["distance"].append(_rel(dist, dthr))
                        out["dists"].append(dist)
                    scs.append(half / (dist * 1000) if live and not dist > dthr else mp.mpf(0))
                mean = mp.fsum(scs) / J
                out["cand_means"].append(mean)
                if athr > 0:
                    mg["candidate_mean"].append(_rel(mean, athr))
                if mean < athr:
                    continue
                kept.append((idx, Ws, scs))
            out["kept"][f] = [k[0] for k in kept]
            n = len(kept)
            persons = []
            absorbed = [False] * n
            order = list(range(n))
            if reverse_condense:
                order.reverse()
            for oi in range(n - 1):
                m0 = order[oi]
                if absorbed[m0]:
                    continue
                members = [m0]
                c0 = kept[m0][1][ci]
                for oj in range(oi + 1, n):
                    s0 = order[oj]
                    if absorbed[s0]:
                        continue
                    c1 = kept[s0][1][ci]
                    df = (c0[0] - c1[0], c0[1] - c1[1], c0[2] - c1[2])
                    dist = mp.sqrt(_dot(df, df))
                    mg["centre"].append(_rel(dist, ctol))
                    out["centre_dists"].append(dist)
                    if dist > ctol:
                        continue
                    absorbed[s0] = True
                    members.append(s0)
                if len(members) < ntol:
                    continue
                xyz, ks = [], []
                for b_ in range(kn):
                    sm_ = mp.fsum(kept[i][2][b_] for i in members)
                    if sm_ == 0:
                        xyz.append((mp.mpf(0), mp.mpf(0), mp.mpf(0)))
                        ks.append(mp.mpf(0))
                        out["dead_joints"] += 1
                        continue
                    xyz.append(tuple(mp.fsum(kept[i][2][b_] / sm_ * kept[i][1][b_][a_] for i in members) for a_ in range(3)))
                    ks.append(sm_ / len(members))
                mean = mp.fsum(ks) / kn if kn else mp.nan
                out["person_means"].append(mean)
                if stol > 0:
                    mg["person_mean"].append(_rel(mean, stol))
                if mean < stol:
                    continue
                persons.append((xyz, ks, mean, members))
            out["count"][f] = len(persons)
            out["members"][f] = [p[3] for p in persons]
            out["xyz_mp"][f] = [p[0] for p in persons]
            for i, (xyz, ks, mean, _) in enumerate(persons[:pout]):
                out["xyz"][f, i] = [[float(v) for v in x] for x in xyz]
                out["kscore"][f, i] = [float(v) for v in ks]
                out["pscore"][f, i] = float(mean)
    return out


def smallest_margin(res):
    """-> (margin as float, name) of the tightest decision of an `evaluate` result (inf, None if it took none)."""
    best, name = mp.inf, None
    for k, v in res["margins"].items():
        if v and min(v) < best:
            best, name = min(v), k
    return float(best), name
