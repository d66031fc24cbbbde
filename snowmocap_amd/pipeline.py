"""Additive whole-recording form of main.py:47-106: every stage after 2D detection on the GPU, device-resident.

    [undistort raw-frame keypoints (N4)] -> triangulate + condense (A1-A4, the hot path) -> temporal smoothing (N1)
    -> Blender control points (N2) -> per-bone smoothing (N2) -> the reference's JSON track

One call per recording instead of one Python iteration per frame.  The per-frame protocol of the reference
identifies persons by list index and lets the list length vary from frame to frame: its filter banks are those of
frame 0, later frames are zip-truncated against them (triangulation.py:169-171, blender.py:152-166).  `run` follows
that: n_persons_out is the number of SLOTS, frame f carries min(count[f], count[0]) persons (fixture G9).  PyTorch is
used for device memory and the stream only.
"""
from __future__ import annotations


import numpy as np

from . import _lib
from .batch import BatchTriangulator
from .blender import CONTROL_POINT_NAMES, _WIDTH
from .despike import DESPIKE_MARK, DESPIKE_MISSING, DESPIKE_REPLACE, DESPIKE_UNSUPPORTED, despike_args, despike_joint_track
from .fill import FILL_MISSING, MAX_GAP, fill_joint_track
from .refine import refine_args


class TrackPipeline:
    def __init__(self, K, R, t, thresholds, blender_smooth_profile, n_persons_out=1, D=None, device=0,
                 method=_lib.PAIRWISE):
        """thresholds: the dict of configs/snowmocap_default_config.json (8 triangulation keys + smooth_f, smooth_z,
        smooth_r, smooth_delta_time); blender_smooth_profile: {control point: [f, z, r]}."""
        self.th = dict(thresholds)
        self.P = int(n_persons_out)
        self.bt = BatchTriangulator(K, R, t, {k: self.th[k] for k in (
            "keypoint_score_threshold", "average_score_threshold", "distance_threshold", "condense_distance_tol",
            "condense_person_num_tol", "condense_score_tol", "center_point_index", "keypoint_num")},
            pout_max=self.P, out_dtype=np.float64, device=device, method=method, D=D)
        self.kn = self.bt.params.keypoint_num
        self.fzr = np.ascontiguousarray([blender_smooth_profile[n] for n in CONTROL_POINT_NAMES], dtype=np.float64)
        self.device = device

    def close(self):
        self.bt.close()

    def run(self, kpts, n_persons=None, check=True, ragged="reference", track_gate=0.3, track_max_missed=8, fill_gaps=0, despike=None,
            reproject=None, refine=None, one_to_one=False, retriangulate=None, seed=None):
        """kpts [F, C, Pmax, J, 3] (NumPy or CUDA tensor; raw-frame pixels if D was given) ->
        dict of CUDA tensors: xyzs [F, P, kn, 4] (triangulated), smoothed [F, P, kn, 4], points [F, P, 24, 4],
        valid [F, P, 24], points_smoothed [F, P, 24, 4], count [F], flags [F], tracked [F] (P = n_persons_out slots).

        Person counts that vary from frame to frame follow the reference (ragged="reference"): its filter banks are those of
        frame 0 and `zip` matches a frame's persons to them BY LIST INDEX (triangulation.py:169-171, blender.py:152-166), so
        frame f carries tracked[f] = min(count[f], count[0]) persons, the persons behind that are dropped, and a bank whose
        person is missing in a frame is not stepped in that frame (its time stands still).  Per slot i this is the plain
        filter over the frames with tracked > i: those are gathered, filtered by the same kernels and scattered back;
        slots at or behind tracked[f] hold zeros.  Frame 0 must fit the slots (count[0] <= n_persons_out).
        ragged="refuse": raise unless every frame resolves to exactly n_persons_out persons (round 4's behaviour).
        check=False skips the host read of counts and flags and treats every slot of every frame as tracked.
        ragged="track": persons are matched ACROSS FRAMES instead of by list index (tracking.PersonTracker on the n_persons_out
        slots: greedy nearest-centre matching within track_gate metres, a slot is given up after track_max_missed frames without
        its person).  Every array is then indexed by SLOT -- xyzs is the tracked gather of the triangulated persons (their list
        order is kept in xyzs_listed / slot_of) -- and each track id is filtered over the frames in which it occupies its slot,
        so a slot that is re-used by a new id starts fresh filters.  Adds present [F, P] (bool) and track_id [F, P]; tracked [F]
        counts the present slots (they need not be a prefix: pass present= to to_blender_result).  Reads track_id on the host.
        fill_gaps=g > 0: short dropouts are bridged before the filters see them (fill.fill_joint_track with max_gap = g: a joint
        the condense step left as the record (0, 0, 0, 0), or a record with a non-finite value, for at most g frames is
        interpolated between its measured neighbours instead of pulling its filter towards the origin).  The fill runs on the
        sequence the filters run on -- the whole [F, P * kn] array when every slot is carried in every frame, otherwise the
        gathered frames of the slot or track id -- and the filters consume the filled records.  Adds xyzs_filled [F, P, kn, 4]
        and fill [F, P, kn] (uint8, fill.FILL_*; outside every filtered sequence: the records of xyzs, FILL_MEASURED or
        FILL_MISSING); xyzs stays the unfilled triangulation.  With ragged="track" a track id that leaves its slot for at most
        g frames and returns to it is BRIDGED first (tracking.bridge_track_ids on the host copy of track_id): its frame set
        becomes that of the bridged id, the tracked gather holds zero records where the person was absent, so those are
        interpolated like any missing joint; track_id and present are then the bridged ones and bridged [F, P] (bool) marks
        the frames that were added.  0 (the default): nothing of this, the dict is today's.  Not addressed: a joint that is
        missing in the first frame of a sequence for more than g frames still seeds its filter with zeros.
        despike=(tol, half_window): one- and two-frame jumps are taken out first (despike.despike_joint_track: a measured record
        further than tol metres from the median of its lane's measured records at frames t - half_window .. t + half_window).  The
        pass runs on exactly the arrays the fill is given (or would be given), immediately before it -- with ragged="track" after
        the gather per track slot.  With fill_gaps > 0 a spike becomes the zero record (DESPIKE_MARK) and the fill bridges it; with
        fill_gaps == 0 it becomes the window median (DESPIKE_REPLACE), since without a filler a marked spike would reach the filter
        as a position at the origin.  Adds spike_codes [F, P, kn] (uint8, despike.DESPIKE_*) and xyzs_despiked [F, P, kn, 4], the
        records the fill (or the filters) consumed; outside every filtered sequence: the records of xyzs, DESPIKE_MISSING or
        DESPIKE_UNSUPPORTED.  None (the default): off, nothing changes and no extra key appears.
        reproject=gate_px: how the views agree with the result.  res["xyzs"] (whatever indexes it: list order, or slots with
        ragged="track") is projected back into every camera and compared with the keypoints the caller passed -- on the RAW frame
        when the pipeline was built with D, so no undistorted copy is made: reproject.match_detections on k_reproject_cost with
        this gate (an RMS pixel distance) and the pipeline's keypoint_score_threshold, reproject.view_residuals on k_reproject.
        Adds det_of [F, C, P] (the detection of camera c that belongs to person p of xyzs, -1: none), shared [F, C, P] (persons of one
        view that chose the same detection: the match is not one-to-one), view_rms [F, C, P] (px, NaN without a match) and view_n.
        None (the default): off, nothing changes and no key is added.
        refine=iters or (iters, gate_px, score_weights): the triangulated joints are moved to a local minimum of their reprojection
        error (refine.refine_joints: at most `iters` Gauss-Newton steps, a joint's cost never rises, scores untouched) right after
        triangulation, before tracking, despiking, filling and smoothing, so everything downstream -- xyzs included -- is made of
        the refined records.  Three steps on the UNDISTORTED keypoints: reprojection_cost of the triangulated persons against every
        detection, reproject.match_detections with gate_px (default 6.0, the default of the robust gate; score_weights default
        False) to find the detection of each camera that shows each person, refine_joints with that det_of and the pipeline's
        keypoint_score_threshold.  With D the triangulator's own undistorted copy of the keypoints is reused (no second k_undistort
        pass).  Adds refine_codes [F, P, kn] (uint8, refine.REFINE_*) and refine_cost [F, P, kn, 2] (px^2 before and after), both in
        the triangulation's list order.  None (the default): off, nothing changes and no key is added.
        refine=(iters, gate_px, score_weights, huber_px) with huber_px > 0: the refinement minimises the Huber loss of
        include/snowtri.h, "Refinement", ROBUST LOSS, instead of the squared error (delta = huber_px pixels: a view further off than
        that pulls with a constant force, not a growing one), and refine_outliers [F, P, kn] (int32 bit mask: camera c is a view of
        the record and beyond delta at the refined point) is added beside refine_codes, in the same order.  A huber_px of None or 0
        is the triple: no bit changes and no key is added.
        one_to_one=True: the matching step of reproject= and of refine= is reproject.assign_detections (k_assign: the optimal
        assignment per frame and camera with the same gate, at most one person per detection) instead of match_detections.  A person
        whose only detections inside the gate went to persons they fit better is then unmatched in that view (det_of -1) instead of
        sharing one; with reproject=, shared -- still computed from det_of by the same expression -- is all False and person_of
        [F, C, Pmax] is added (the person that took detection q, -1: a detection nobody claimed).  It needs reproject, refine
        or retriangulate (ValueError otherwise), and gates of at most 1e150 px: staying unmatched costs gate_px^2, so the infinite gate that
        match_detections reads as "no gate" is refused.  False (the default): nothing changes.
        retriangulate=gate_px or (gate_px, reproj_threshold_px, max_drops) (the last two default to 6.0 and 1): every person is
        triangulated again from ALL the views that show it, right after the first triangulation and before refine=.  Three steps on
        the UNDISTORTED keypoints: reprojection_cost of the first pass's persons, the matching step above with gate_px (one_to_one is
        honoured, and is legal with retriangulate= alone), matched.triangulate_matched (k_dlt_matched: DLT_ROBUST's rule on the
        detections det_of names).  A joint record the second pass made from at least 2 views replaces the first pass's; every other
        record keeps the first pass's bits, so no joint is lost; count and flags are the first pass's.  Adds retri_views [F, P, kn]
        (int32 bit mask of the cameras used, 0: the record was kept) and retri_resid [F, P, kn] (RMS px, 0 where kept), both in the
        triangulation's list order.  With refine= as well the refinement reuses this det_of (its own gate_px is then not used) and
        is given retri_views as its `views`, all ones where the record was kept.  None (the default): off, nothing changes and no
        key is added.
        seed=gate or (gate, min_views, min_joints) (the last two default to 3 and 8): persons the first pass MISSED are seeded from
        the detections nobody claimed, right after the retriangulation merge and before refine=.  It needs retriangulate= together
        with one_to_one=True (ValueError otherwise, before any work): that matching step is where person_of on the undistorted
        keypoints comes from.  seed.triangulate_seeded (k_pair_cost, k_seed_group, k_dlt_matched) runs with claimed = person_of,
        S = n_persons_out slots, gate an RMS line distance in world units, and the retriangulation's reproj_threshold_px and
        max_drops; seed i < min(n_seeds[f], n_persons_out - count[f]) is written to slot count[f] + i of xyzs -- a slot that holds
        zeros otherwise, so no measured record is lost -- and count[f] is raised by that number; flags stay the first pass's.
        Everything downstream (the ragged rules, tracking, despiking, filling, the filters) takes the raised count.  Adds seeded
        [F, P] (bool) and seed_det_of [F, C, P] (the detections of a seeded slot, -1 everywhere else); retri_views / retri_resid of a
        seeded slot are the seed triangulation's, and refine= sees the seed's det_of and views mask there.  A slot that is not seeded
        keeps its bits.  None (the default): off, nothing changes and no key is added."""
        from .matched import retriangulate_args
        from .seed import seed_option
        rtr = retriangulate_args(retriangulate)
        sdo = seed_option(seed)
        if sdo and not (rtr and one_to_one):
            raise ValueError("seed= needs retriangulate= together with one_to_one=True: their matching step says which detections nobody claimed")
        if one_to_one and reproject is None and refine is None and rtr is None:
            raise ValueError("one_to_one=True needs reproject=, refine= or retriangulate=: it chooses how their matching step pairs persons "
                             "and detections")
        one_to_one, rfn = bool(one_to_one), refine_args(refine)
        if one_to_one:                                     # before any work: the assignment needs a finite gate (<= 1e150)
            from .reproject import assign_gate
            for gate in ([reproject] if reproject is not None else []) + ([rfn[1]] if rfn else []) + ([rtr[0]] if rtr else []):
                assign_gate(gate)
        res = self._run(kpts, n_persons, check, ragged, track_gate, track_max_missed, fill_gaps, despike, rfn, one_to_one, rtr, sdo)
        if reproject is not None:
            self._add_reprojection(res, kpts, n_persons, float(reproject), one_to_one)
        return res

    def _match(self, cost_sum, cost_n, gate_px, one_to_one):
        """The matching step of run(reproject=..., refine=...) -> (det_of, shared, person_of or None)."""
        from .reproject import assign_detections, match_detections
        if not one_to_one:
            return match_detections(cost_sum, cost_n, gate_px) + (None,)
        det_of, person_of = assign_detections(self.bt.ctx, cost_sum, cost_n, gate_px, with_person_of=True)
        same = (det_of[..., :, None] == det_of[..., None, :]) & (det_of[..., :, None] >= 0)
        return det_of, same.sum(dim=-1) > 1, person_of

    def _add_reprojection(self, res, kpts, n_persons, gate_px, one_to_one=False):
        """run(reproject=gate_px): res["xyzs"] against the keypoints the caller passed (on the raw frame when the pipeline has D)."""
        import torch
        from .reproject import view_residuals
        dev = torch.device("cuda", self.device)
        if not torch.is_tensor(kpts):
            kpts = torch.from_numpy(np.ascontiguousarray(kpts)).to(dev)
        if n_persons is not None and not torch.is_tensor(n_persons):
            n_persons = torch.from_numpy(np.ascontiguousarray(n_persons, dtype=np.int32)).to(dev)
        if n_persons is not None:
            n_persons = n_persons.to(torch.int32).contiguous()
        kpts = kpts.contiguous()
        J = int(kpts.shape[3])
        if J != self.kn:                                  # the joints the triangulation kept are the first kn of a detection
            kpts = kpts[:, :, :, :self.kn].contiguous()
        xyzs = res["xyzs"].contiguous()
        ctx, raw, thr = self.bt.ctx, self.bt.undistort, float(self.th["keypoint_score_threshold"])
        cost_sum, cost_n = ctx.reproject_cost(xyzs, kpts, n_persons=n_persons, keypoint_score_threshold=thr, raw=raw)
        res["det_of"], res["shared"], person_of = self._match(cost_sum, cost_n, gate_px, one_to_one)
        if person_of is not None:
            res["person_of"] = person_of
        pix = ctx.reproject(xyzs, raw=raw, dtype=torch.float64)
        _, res["view_rms"], res["view_n"] = view_residuals(pix, kpts, res["det_of"], thr)

    def _undistorted(self):
        """The undistorted keypoints of the last triangulation, cut to the joints it kept (the first kn of a detection)."""
        ukpts = self.bt.last_undistorted_kpts
        if int(ukpts.shape[3]) != self.kn:
            ukpts = ukpts[:, :, :, :self.kn].contiguous()
        return ukpts

    def _retriangulate(self, xyzs, n_persons, rtr, one_to_one=False):
        """run(retriangulate=...): the first pass's records against the undistorted keypoints of the call that made them
        -> (merged records, retri_views, retri_resid, det_of, person_of: assign_detections' with one_to_one, else None)."""
        import torch
        gate_px, tau, max_drops = rtr
        ukpts = self._undistorted()
        ctx, thr = self.bt.ctx, float(self.th["keypoint_score_threshold"])
        xyzs = xyzs.contiguous()
        cost_sum, cost_n = ctx.reproject_cost(xyzs, ukpts, n_persons=n_persons, keypoint_score_threshold=thr)
        det_of, _, person_of = self._match(cost_sum, cost_n, gate_px, one_to_one)
        again, _, views, resid = ctx.triangulate_matched(ukpts, det_of=det_of, n_persons=n_persons, keypoint_score_threshold=thr,
                                                         reproj_threshold_px=tau, max_drops=max_drops, dtype=xyzs.dtype, diagnostics=True)
        return torch.where((views != 0)[..., None], again, xyzs), views, resid, det_of, person_of

    def _seed(self, xyzs, count, n_persons, person_of, rtr, sdo, retri_views, retri_resid, det_of):
        """run(seed=...): persons seeded from the detections person_of left unclaimed, written behind the first pass's persons
        -> (records, retri_views, retri_resid, det_of, the raised count, seeded [F, P], seed_det_of [F, C, P])."""
        import torch
        from .seed import triangulate_seeded
        gate, min_views, min_joints = sdo
        P, ctx, thr = self.P, self.bt.ctx, float(self.th["keypoint_score_threshold"])
        sd = triangulate_seeded(ctx, self._undistorted(), n_persons=n_persons, claimed=person_of, S=P, gate=gate, min_views=min_views,
                                min_joints=min_joints, keypoint_score_threshold=thr, reproj_threshold_px=rtr[1], max_drops=rtr[2],
                                diagnostics=True, dtype=xyzs.dtype)
        first = count.to(torch.int64).clamp(min=0, max=P)                                    # the slots the first pass holds
        taken = torch.minimum(sd["n_seeds"].to(torch.int64), P - first)
        i = torch.arange(P, device=xyzs.device)[None, :] - first[:, None]                    # slot -> seed index
        seeded = (i >= 0) & (i < taken[:, None])
        src = i.clamp(min=0, max=P - 1)
        per_joint = lambda a: torch.gather(a, 1, src[:, :, None].expand(-1, -1, a.shape[2]))   # noqa: E731
        seed_det = torch.gather(sd["seed_det_of"].to(det_of.dtype), 2, src[:, None, :].expand(-1, det_of.shape[1], -1))
        xyzs = torch.where(seeded[:, :, None, None], torch.gather(sd["xyzs"], 1, src[:, :, None, None].expand(-1, -1, *xyzs.shape[2:])), xyzs)
        retri_views = torch.where(seeded[:, :, None], per_joint(sd["views"]), retri_views)
        retri_resid = torch.where(seeded[:, :, None], per_joint(sd["resid"]), retri_resid)
        det_of = torch.where(seeded[:, None, :], seed_det, det_of)
        seed_det_of = torch.where(seeded[:, None, :], seed_det, -1).to(torch.int32)
        return xyzs.contiguous(), retri_views.contiguous(), retri_resid.contiguous(), det_of.contiguous(), \
            (count + taken.to(count.dtype)).contiguous(), seeded, seed_det_of

    def _refine(self, xyzs, n_persons, rfn, one_to_one=False, matched=None):
        """run(refine=...): the triangulated records against the undistorted keypoints of the call that made them
        -> (refined records, cost, codes), and with a Huber loss (a fourth entry in rfn) the outliers mask as well.  matched: (det_of, retri_views) of run(retriangulate=...), used instead of a matching step."""
        import torch
        iters, gate_px, score_weights = rfn[:3]
        huber_px = rfn[3] if len(rfn) > 3 else None
        ukpts = self._undistorted()
        ctx, thr = self.bt.ctx, float(self.th["keypoint_score_threshold"])
        xyzs = xyzs.contiguous()
        if matched is None:
            cost_sum, cost_n = ctx.reproject_cost(xyzs, ukpts, n_persons=n_persons, keypoint_score_threshold=thr)
            det_of, views = self._match(cost_sum, cost_n, gate_px, one_to_one)[0], None
        else:
            det_of, views = matched[0], torch.where(matched[1] != 0, matched[1], -1).contiguous()   # a kept record: every camera
        return ctx.refine_joints(xyzs, ukpts, det_of=det_of, n_persons=n_persons, views=views, keypoint_score_threshold=thr, iters=iters,
                                 score_weights=score_weights, diagnostics=True, huber_px=huber_px)

    def _run(self, kpts, n_persons, check, ragged, track_gate, track_max_missed, fill_gaps, despike, rfn=None, one_to_one=False, rtr=None,
             sdo=None):
        """run() without its reprojection keys."""
        dsp = despike_args(despike)
        import torch
        dev = torch.device("cuda", self.device)
        if not torch.is_tensor(kpts):
            kpts = torch.from_numpy(np.ascontiguousarray(kpts)).to(dev)
        if n_persons is not None and not torch.is_tensor(n_persons):
            n_persons = torch.from_numpy(np.ascontiguousarray(n_persons, dtype=np.int32)).to(dev)
        F = kpts.shape[0]
        L, h = self.bt.ctx.L, self.bt.ctx.handle
        st = _lib.ptr(torch.cuda.current_stream(dev).cuda_stream)
        tri = self.bt.run_torch(kpts, n_persons)
        xyzs, matched, count = tri["xyzs"], None, tri["count"]
        if rtr:
            xyzs, retri_views, retri_resid, det_of, person_of = self._retriangulate(xyzs, n_persons, rtr, one_to_one)
            if sdo:                                      # (the checks below read the raised count)
                xyzs, retri_views, retri_resid, det_of, count, seeded, seed_det_of = self._seed(xyzs, count, n_persons, person_of, rtr, sdo,
                                                                                                 retri_views, retri_resid, det_of)
            matched = (det_of, retri_views)
        tracked = None                                   # None: every slot of every frame
        if check:
            cnt = count.cpu().numpy()
            flg = tri["flags"].cpu().numpy()
            if (flg & _lib.FLAG_SINGULAR).any():    # the reference's np.linalg.inv raises (triangulation.py:26)
                raise np.linalg.LinAlgError(f"Singular matrix (frame {int(np.argmax((flg & _lib.FLAG_SINGULAR) != 0))})")
            if ragged != "track" and not (cnt == self.P).all():
                if ragged == "refuse":
                    bad = int(np.argmax(cnt != self.P))
                    raise ValueError(f"frame {bad} resolved to {int(cnt[bad])} persons, the track is built for {self.P}")
                if F and int(cnt[0]) > self.P:
                    raise ValueError(f"frame 0 resolved to {int(cnt[0])} persons, the track has {self.P} slots (n_persons_out)")
                tracked = np.minimum(cnt, int(cnt[0]) if F else 0).astype(np.int32)
        if rfn:
            xyzs, refine_cost, refine_codes, *refine_outliers = self._refine(xyzs, n_persons, rfn, one_to_one, matched)
        th = self.th
        fzrd =(float(th["smooth_f"]), float(th["smooth_z"]), float(th["smooth_r"]), float(th["smooth_delta_time"]))
        fill_gaps = int(fill_gaps)
        if fill_gaps < 0 or fill_gaps > MAX_GAP:
            raise ValueError(f"fill_gaps must be 0 (off) or a max_gap in 1..{MAX_GAP} (got {fill_gaps})")
        dsp_mode = DESPIKE_MARK if fill_gaps > 0 else DESPIKE_REPLACE
        pts = torch.empty((F, self.P, 24, 4), dtype=torch.float64, device=dev)
        val = torch.empty((F, self.P, 24), dtype=torch.uint8, device=dev)

        def blender_points(x, n, p_out, v_out):
            _lib.check(L.snowtri_blender_points(h, n, self.kn, _lib.ptr(x), _lib.F64, _lib.ptr(p_out),
                                                _lib.ptr(v_out), _lib.DEVICE, st), "snowtri_blender_points")

        def filter_rows(src, idx, i, sm, pts_s, filled=None, codes=None, desp=None, scodes=None):
            """slot i over the frames idx (the first of them seeds the filters): gather, [despike into desp / scodes,] [fill into
            filled / codes,] N1, N2 points, N2 filters, scatter"""
            T = int(idx.numel())
            xi = src[idx, i].contiguous()                                   # [T, kn, 4]
            if desp is not None:
                xi, di = despike_joint_track(self.bt.ctx, xi, dsp[1], dsp[0], dsp_mode)
                desp[idx, i] = xi
                scodes[idx, i] = di
            if filled is not None:
                xi, ci = fill_joint_track(self.bt.ctx, xi, fill_gaps)
                filled[idx, i] = xi
                codes[idx, i] = ci
            si = torch.empty_like(xi)
            _lib.check(L.snowtri_smooth_joint_track(h, T, self.kn, _lib.ptr(xi), *fzrd, _lib.ptr(si),
                                                    _lib.DEVICE, st), "snowtri_smooth_joint_track")
            pi = torch.empty((T, 1, 24, 4), dtype=torch.float64, device=dev)
            vi = torch.empty((T, 1, 24), dtype=torch.uint8, device=dev)
            blender_points(si, T, pi, vi)
            qi = torch.empty_like(pi)
            _lib.check(L.snowtri_blender_smooth(h, T, 1, _lib.ptr(pi), _lib.ptr(vi),
                                                _lib.ptr(self.fzr), fzrd[3], _lib.ptr(qi), _lib.DEVICE, st),
                       "snowtri_blender_smooth")
            sm[idx, i] = si
            pts[idx, i] = pi[:, 0]
            val[idx, i] = vi[:, 0]
            pts_s[idx, i] = qi[:, 0]

        def missing(x):
            """records.missing_records on a tensor"""
            return (x[..., 3] == 0) | ~torch.isfinite(x).all(dim=-1)

        def unfilled(x):
            """(xyzs_filled, fill) before any sequence has been filled: the records as they are, measured or missing"""
            return x.clone(), missing(x).to(torch.uint8) * FILL_MISSING

        def undespiked(x):
            """(xyzs_despiked, spike_codes) before any sequence has been despiked: the records as they are, missing or untested"""
            return x.clone(), torch.where(missing(x), DESPIKE_MISSING, DESPIKE_UNSUPPORTED).to(torch.uint8)

        if ragged == "track":
            from .tracking import PersonTracker, bridge_track_ids
            trk_out = PersonTracker(self.bt.ctx, S=self.P, center_point_index=self.bt.params.center_point_index, gate=track_gate,
                                    max_missed=track_max_missed).run_torch(xyzs, count, gather=True, carry=False)
            listed, xyzs = xyzs, trk_out["xyzs_tracked"]
            tid = trk_out["track_id"].cpu().numpy()                          # the host decides which frames a track covers
            if fill_gaps:
                tid = bridge_track_ids(tid, fill_gaps)
            filled, codes = unfilled(xyzs) if fill_gaps else (None, None)
            desp, scodes = undespiked(xyzs) if dsp else (None, None)
            sm = torch.zeros_like(xyzs)
            pts.zero_()
            val.zero_()
            pts_s = torch.zeros_like(pts)
            for i in range(self.P):
                for one in np.unique(tid[:, i][tid[:, i] >= 0]):
                    filter_rows(xyzs, torch.from_numpy(np.nonzero(tid[:, i] == one)[0]).to(dev), i, sm, pts_s, filled, codes, desp, scodes)
            present = trk_out["person_of"] >= 0
            res = dict(xyzs=xyzs, smoothed=sm, points=pts, valid=val, points_smoothed=pts_s, count=count, flags=tri["flags"],
                       tracked=present.sum(dim=1).to(torch.int32), present=present, track_id=trk_out["track_id"],
                       slot_of=trk_out["slot_of"], track_flags=trk_out["flags"], xyzs_listed=listed)
            if fill_gaps:
                res["track_id"] = torch.from_numpy(tid).to(dev)
                res["present"] = res["track_id"] >= 0
                res["bridged"] = res["present"] & ~present
                res["tracked"] = res["present"].sum(dim=1).to(torch.int32)
                res["xyzs_filled"], res["fill"] = filled, codes
            if dsp:
                res["xyzs_despiked"], res["spike_codes"] = desp, scodes
            if rfn:
                res["refine_cost"], res["refine_codes"] = refine_cost, refine_codes
                if refine_outliers:
                    res["refine_outliers"] = refine_outliers[0]
            if rtr:
                res["retri_views"], res["retri_resid"] = retri_views, retri_resid
            if sdo:
                res["seeded"], res["seed_det_of"] = seeded, seed_det_of
            return res
        if tracked is None:
            src = xyzs
            if dsp:
                desp, scodes = despike_joint_track(self.bt.ctx, src, dsp[1], dsp[0], dsp_mode)
                src = desp
            if fill_gaps:
                filled, codes = fill_joint_track(self.bt.ctx, src, fill_gaps)
                src = filled
            sm = torch.empty_like(xyzs)                    # only the points are filtered, the scores copied (triangulation.py:169-184)
            _lib.check(L.snowtri_smooth_joint_track(h, F, self.P * self.kn, _lib.ptr(src), *fzrd, _lib.ptr(sm),
                                                    _lib.DEVICE, st), "snowtri_smooth_joint_track")
            blender_points(sm, F * self.P, pts, val)
            pts_s = torch.empty_like(pts)
            _lib.check(L.snowtri_blender_smooth(h, F, self.P, _lib.ptr(pts), _lib.ptr(val),
                                                _lib.ptr(self.fzr), fzrd[3], _lib.ptr(pts_s), _lib.DEVICE, st),
                       "snowtri_blender_smooth")
            trk = torch.full((F,), self.P, dtype=torch.int32, device=dev)
        else:
            # slot by slot over the frames that carry it (frame 0 among them: it seeds the slot's filters)
            trk = torch.from_numpy(tracked).to(dev)
            filled, codes = unfilled(xyzs) if fill_gaps else (None, None)
            desp, scodes = undespiked(xyzs) if dsp else (None, None)
            sm = torch.zeros_like(xyzs)
            pts.zero_()
            val.zero_()
            pts_s = torch.zeros_like(pts)
            for i in range(int(tracked[0]) if F else 0):
                filter_rows(xyzs, torch.nonzero(trk > i).view(-1), i, sm, pts_s, filled, codes, desp, scodes)
        res = dict(xyzs=xyzs, smoothed=sm, points=pts, valid=val, points_smoothed=pts_s, count=count,
                   flags=tri["flags"], tracked=trk)
        if fill_gaps:
            res["xyzs_filled"], res["fill"] = filled, codes
        if dsp:
            res["xyzs_despiked"], res["spike_codes"] = desp, scodes
        if rfn:
            res["refine_cost"], res["refine_codes"] = refine_cost, refine_codes
            if refine_outliers:
                res["refine_outliers"] = refine_outliers[0]
        if rtr:
            res["retri_views"], res["retri_resid"] = retri_views, retri_resid
        if sdo:
            res["seeded"], res["seed_det_of"] = seeded, seed_det_of
        return res

    @staticmethod
    def to_blender_result(points_smoothed, valid, armature_profile=None, tracked=None, present=None):
        """Device (or NumPy) track -> the list the reference dumps with save_blender_result (blender.py:180-187):
        one {'armature': [per person {name: list}], 'score': [per person {name: 0/1}]} per frame.  tracked [F]: persons
        frame f carries (run()'s "tracked"; default: every slot).  present [F, P] (run(ragged="track")): the slots frame f
        carries, listed in slot order; it replaces `tracked`."""
        pts = points_smoothed.cpu().numpy() if hasattr(points_smoothed, "cpu") else np.asarray(points_smoothed)
        val = valid.cpu().numpy() if hasattr(valid, "cpu") else np.asarray(valid)
        if tracked is None:
            trk = np.full(pts.shape[0], pts.shape[1], dtype=np.int64)
        else:
            trk = (tracked.cpu().numpy() if hasattr(tracked, "cpu") else np.asarray(tracked)).astype(np.int64)
        live = np.arange(pts.shape[1])[None, :] < trk[:, None]
        if present is not None:
            live = (present.cpu().numpy() if hasattr(present, "cpu") else np.asarray(present)).astype(bool)
        if not val[..., 1][live].all():
            raise np.linalg.LinAlgError("SVD did not converge")     # the reference raises on a NaN pelvis matrix
        names = list(armature_profile.keys()) if armature_profile is not None else list(CONTROL_POINT_NAMES)
        slot = {n: i for i, n in enumerate(CONTROL_POINT_NAMES)}
        frames = []
        for f in range(pts.shape[0]):
            frames.append({
                "armature": [{n: pts[f, p, slot[n], :_WIDTH[n]].tolist() for n in names} for p in np.nonzero(live[f])[0]],
                "score": [{n: int(val[f, p, slot[n]]) for n in names} for p in np.nonzero(live[f])[0]]})
        return frames


class ShardedTrackPipeline:
    """TrackPipeline on a FRAME SHARD (one instance per rank, one process per GPU): the whole chain after 2D detection runs on
    the rank's contiguous frame block and only the final animation track is gathered (round-4 review, item 4b):

        A1-A4 on the block  ->  N1 with the carry exchange (4n + 1 doubles per rank, sharded.smooth_track_sharded)
        ->  N2 control points (per frame)  ->  N2 per-bone filters with the hold exchange + the carry exchange
        (sharded.blender_smooth_sharded)  ->  ONE all-gather of [F, P, 24, 4] float64 + valid [F, P, 24] + tracked [F]

    instead of gathering the [F, P, kn, 4] joint track first (at roofline speed that gather is ~8x the kernel):
    792 + 24 bytes per person and frame against 2 128 for 133 float32 joints.
    A person count that varies from frame to frame follows the reference, as TrackPipeline.run(ragged="reference") does on one
    GPU (round-5 review, item 4): the filter banks are those of frame 0 and `zip` matches a frame's persons to them by list
    index (triangulation.py:169-171, blender.py:152-166), so frame f carries tracked[f] = min(count[f], count[0]) persons.
    That needs ONE number of another rank -- count[0], handed round with the ranks' error bits (sharded.tracked_counts) --
    and per slot i the frames with tracked > i that a rank holds are a block of the slot's own frame sequence: the N1 carry
    exchange and the N2 hold + carry exchanges run on those blocks unchanged (an empty block is a rank none of whose frames
    carries the slot; the block with frame 0 starts the sequence).
    TrackPipeline.run's fill_gaps is NOT offered here: a gap that crosses a shard boundary needs the measured records on both
    sides of it, i.e. a halo exchange of up to max_gap frames per rank before the fill, which has not been built.  Its despike is
    left out for the same reason: the window of a record within half_window frames of a shard boundary holds records of the
    neighbouring rank.  Its reproject is not offered either: the caller holds only its own block of keypoints, and the per-view
    keys would have to be gathered beside the track; run TrackPipeline-style reprojection per rank with reproject.reprojection_cost
    on the block's xyzs if it is wanted.  Its refine is not offered for the same reason: refine.refine_joints on the block's xyzs and
    keypoints does per rank what TrackPipeline.run(refine=...) does, a joint's refinement needs nothing from another frame."""

    def __init__(self, K, R, t, thresholds, blender_smooth_profile, n_persons_out=1, device=0, group=None, method=_lib.PAIRWISE):
        self.pipe = TrackPipeline(K, R, t, thresholds, blender_smooth_profile, n_persons_out=n_persons_out, device=device, method=method)
        self.group = group
        self.device = device

    def close(self):
        self.pipe.close()

    def run(self, kpts_local, F_total, n_persons_local=None, gather=True, ragged="reference"):
        """kpts_local [T_r, C, Pmax, J, 3] CUDA tensor: the block shard_bounds(F_total, world, rank) gives this rank.  Returns
        points_smoothed / valid / tracked of the WHOLE track on every rank (gather=True) or of the block, plus the block's own
        stages.  ragged="refuse": every frame of every rank must resolve to exactly n_persons_out persons (round 4's contract)."""
        import torch
        import torch.distributed as dist
        from .sharded import (blender_smooth_sharded, gather_track_chunked, shard_bounds, smooth_track_sharded, tracked_counts)
        p = self.pipe
        dev = kpts_local.device
        rank, world = dist.get_rank(self.group), dist.get_world_size(self.group)
        lo, hi, per = shard_bounds(int(F_total), world, rank)
        T = int(kpts_local.shape[0])
        if T != hi - lo:
            raise ValueError(f"ShardedTrackPipeline: rank {rank} holds {T} frames, shard_bounds gives it [{lo}, {hi})")
        L, h = p.bt.ctx.L, p.bt.ctx.handle
        st = _lib.ptr(torch.cuda.current_stream(dev).cuda_stream)
        P, kn, th = p.P, p.kn, p.th
        if T:
            tri = p.bt.run_torch(kpts_local, n_persons_local)
        else:
            tri = p.bt.alloc_outputs(0, dev)
        # every rank learns count[0] and whether every block is usable BEFORE the exchanges below (nobody is left waiting in one)
        bits = torch.zeros((), dtype=torch.int32, device=dev)
        if T:
            bits = (((tri["flags"] & _lib.FLAG_SINGULAR) != 0).any().to(torch.int32) + 2 * (tri["count"] != P).any().to(torch.int32)).to(torch.int32)
        tracked, count0, bits = tracked_counts(tri["count"], int(F_total), P, group=self.group, flag_bits=bits)
        if bits & 1:
            raise np.linalg.LinAlgError("Singular matrix (a frame of some rank)")     # the reference's np.linalg.inv raises (triangulation.py:26)
        if (bits & 2) and ragged == "refuse":
            raise ValueError(f"a frame of some rank did not resolve to {P} persons (ragged=\"refuse\")")
        xyzs = tri["xyzs"]
        fkw = dict(f=th["smooth_f"], z=th["smooth_z"], r=th["smooth_r"], delta_time=th["smooth_delta_time"], group=self.group, ctx=p.bt.ctx)
        pts = torch.empty((T, P, 24, 4), dtype=torch.float64, device=dev)
        val = torch.empty((T, P, 24), dtype=torch.uint8, device=dev)

        def blender_points(x, n_, p_out, v_out):
            _lib.check(L.snowtri_blender_points(h, n_, kn, _lib.ptr(x), _lib.F64, _lib.ptr(p_out),
                                                _lib.ptr(v_out), _lib.DEVICE, st), "snowtri_blender_points")

        if not (bits & 2):
            # every frame of every rank carries all P slots: the whole block at once
            sm = smooth_track_sharded(xyzs.view(T, P * kn * 4) if T else xyzs.reshape(0, P * kn * 4), F_total=F_total, **fkw).view(T, P, kn, 4)
            if T:
                sm[..., 3] = xyzs[..., 3]                  # only the points are filtered (triangulation.py:169-184)
                blender_points(sm, T * P, pts, val)
            pts_s = blender_smooth_sharded(pts, val, p.fzr, th["smooth_delta_time"], group=self.group, ctx=p.bt.ctx, F_total=F_total)
        else:
            # slot by slot over the frames that carry it; every rank walks the SAME count0 slots (the exchanges are collectives)
            sm = torch.zeros_like(xyzs)
            pts.zero_()
            val.zero_()
            pts_s = torch.zeros_like(pts)
            holds0 = lo == 0 and hi > 0                    # frame 0 carries every tracked slot: its rank starts every slot's sequence
            for i in range(count0):
                idx = torch.nonzero(tracked > i).view(-1)
                Ti = int(idx.numel())
                xi = xyzs[idx, i].contiguous().view(Ti, kn * 4)
                si = smooth_track_sharded(xi, first=holds0 and Ti > 0, **fkw).view(Ti, kn, 4)
                pi = torch.empty((Ti, 1, 24, 4), dtype=torch.float64, device=dev)
                vi = torch.empty((Ti, 1, 24), dtype=torch.uint8, device=dev)
                if Ti:
                    si[..., 3] = xi.view(Ti, kn, 4)[..., 3]
                    blender_points(si, Ti, pi, vi)
                qi = blender_smooth_sharded(pi, vi, p.fzr, th["smooth_delta_time"], group=self.group, ctx=p.bt.ctx, first=holds0 and Ti > 0)
                if Ti:
                    sm[idx, i] = si
                    pts[idx, i] = pi[:, 0]
                    val[idx, i] = vi[:, 0]
                    pts_s[idx, i] = qi[:, 0]
        out = dict(xyzs_local=xyzs, smoothed_local=sm, points_local=pts, valid_local=val, points_smoothed_local=pts_s,
                   count_local=tri["count"], flags_local=tri["flags"], tracked_local=tracked, count0=count0)
        if gather:
            def copy_block(lo_, hi_, views):
                views["points_smoothed"][: hi_ - lo_] = pts_s[lo_:hi_]
                views["valid"][: hi_ - lo_] = val[lo_:hi_]
                views["tracked"][: hi_ - lo_] = tracked[lo_:hi_]
            g = gather_track_chunked(copy_block, T, int(F_total), {"points_smoothed": ((P, 24, 4), torch.float64), "valid": ((P, 24), torch.uint8),
                                                                   "tracked": ((), torch.int32)},
                                     chunks=1, group=self.group, device=dev)
            out["points_smoothed"], out["valid"], out["tracked"] = g["points_smoothed"], g["valid"], g["tracked"]
            out["gather_bytes"] = world * per * (P * 24 * 4 * 8 + P * 24 + 4) + world * 16
            out["gather_bytes_joint_track"] = world * per * (P * kn * 16 + P * 4 + 8)
        return out
