"""Cross-frame person tracking: stable identities for the persons snowtri_triangulate_condense resolves frame by frame.

The condense step lists a frame's persons in whatever order its clusters formed (in practice: camera 0's detection order), so
`xyzs[f][p]` and `xyzs[f + 1][p]` need not be the same human.  The tracker here assigns every person of every frame to one
of S SLOTS by greedy nearest-centre matching and gives every new appearance a fresh TRACK ID.  The rule (include/snowtri.h,
"Person tracking") per frame, on fp64 centres:

  1. a person p < count[f] is VALID when its centre joint has score != 0 and three finite coordinates;
  2. d2(s, p) = (dx*dx + dy*dy) + dz*dz, every product and sum rounded separately, for every slot live at the start of
     the frame and every valid person;
  3. greedy: repeatedly the smallest d2 <= gate*gate among unassigned (slot, person) pairs, ties to the lowest s, then the
     lowest p; the slot takes the person's centre, missed = 0;
  4. births: every valid person left over, in increasing p, takes the lowest slot that was NOT live at the start of the
     frame (and has not been taken in this step) under id = next_id++; none left: slot_of = -1 and TRACK_FLAG_OVERFLOW;
  5. ageing: a slot that was live and got nobody counts missed += 1 and is freed once missed > max_missed (re-usable
     from the next frame on).

`track_persons_reference` is that rule in NumPy (no GPU, no library): the oracle of the kernels, which must agree with it
bit for bit.  `PersonTracker` runs the HIP kernels (snowtri_track_persons / snowtri_track_gather) and keeps the state
between calls, so a recording can be processed in consecutive frame blocks.
"""
from __future__ import annotations

import numpy as np

from . import _lib

TRACK_FLAG_OVERFLOW = 1        # SNOWTRI_TRACK_FLAG_OVERFLOW: a valid person of this frame found no free slot
MAX_SLOTS = 16                 # S and Pout_max of the tracker: 1 .. 16 (S x Pout_max <= 256 pairs, four per lane of one wave)
_STATE_HEADER_BYTES, _STATE_SLOT_BYTES = 16, 40


def state_bytes(S):
    """Size of the opaque state blob for S slots (the library's snowtri_track_state_bytes gives the same number)."""
    return _STATE_HEADER_BYTES + _STATE_SLOT_BYTES * int(S)


def chain_block_frames():
    """Frames per staging block of k_track_chain (snowtri_track_block_frames): batches around its multiples are the sizes
    at which the kernel's double buffering changes path."""
    return int(_lib.lib().snowtri_track_block_frames())


def fresh_state(S):
    return dict(live=np.zeros(S, dtype=bool), pos=np.zeros((S, 3)), missed=np.zeros(S, dtype=np.int32),
                id=np.zeros(S, dtype=np.int32), next_id=0)


def state_to_blob(state):
    """Reference state -> the library's blob: int32 (next_id, 0, 0, 0) | pos [S][3] fp64 | int32 [S][4] (live, missed, id, 0)."""
    S = state["live"].shape[0]
    blob = np.zeros(state_bytes(S), dtype=np.uint8)
    blob[:4] = np.array([state["next_id"]], dtype=np.int32).view(np.uint8)
    blob[16:16 + 24 * S] = np.ascontiguousarray(state["pos"], dtype=np.float64).view(np.uint8).reshape(-1)
    meta = np.zeros((S, 4), dtype=np.int32)
    meta[:, 0], meta[:, 1], meta[:, 2] = state["live"], state["missed"], state["id"]
    blob[16 + 24 * S:] = meta.view(np.uint8).reshape(-1)
    return blob


def state_from_blob(blob, S):
    blob = np.ascontiguousarray(blob, dtype=np.uint8).reshape(-1)
    assert blob.shape[0] == state_bytes(S)
    meta = blob[16 + 24 * S:].view(np.int32).reshape(S, 4)
    return dict(live=meta[:, 0] != 0, pos=blob[16:16 + 24 * S].view(np.float64).reshape(S, 3).copy(), missed=meta[:, 1].copy(),
                id=meta[:, 2].copy(), next_id=int(blob[:4].view(np.int32)[0]))


def _check_args(P, kn, S, center_point_index, gate, max_missed):
    if not (1 <= S <= MAX_SLOTS) or not (1 <= P <= MAX_SLOTS):
        raise ValueError(f"S and Pout_max must lie in 1..{MAX_SLOTS} (got S={S}, Pout_max={P})")
    if not (np.isfinite(gate) and gate >= 0):
        raise ValueError(f"gate must be finite and >= 0 (got {gate})")
    if max_missed < 0:
        raise ValueError(f"max_missed must be >= 0 (got {max_missed})")
    if not (0 <= center_point_index < kn):
        raise IndexError(f"center_point_index {center_point_index} outside [0, {kn})")


def track_persons_reference(xyzs, count, S, center_point_index, gate, max_missed, state=None):
    """xyzs [F, Pout_max, keypoint_num, 4] (float32 / float64), count [F] as snowtri_triangulate_condense writes them ->
    (slot_of [F, Pout_max], person_of [F, S], track_id [F, S], flags [F], new state).  `state`: what an earlier call returned
    (None = fresh); it is not modified.  Pure NumPy."""
    xyzs = np.asarray(xyzs)
    F, P, kn = xyzs.shape[0], xyzs.shape[1], xyzs.shape[2]
    S = int(S)
    _check_args(P, kn, S, center_point_index, gate, max_missed)
    count = np.asarray(count).reshape(F)
    st = fresh_state(S) if state is None else {k: (v.copy() if isinstance(v, np.ndarray) else v) for k, v in state.items()}
    live, pos, missed, ids = st["live"], st["pos"], st["missed"], st["id"]
    next_id = int(st["next_id"])
    slot_of = np.full((F, P), -1, dtype=np.int32)
    person_of = np.full((F, S), -1, dtype=np.int32)
    track_id = np.full((F, S), -1, dtype=np.int32)
    flags = np.zeros(F, dtype=np.uint32)
    cen = xyzs[:, :, center_point_index, :].astype(np.float64)          # inputs are converted to fp64 first
    g2 = np.float64(gate) * np.float64(gate)
    ar_p = np.arange(P)
    with np.errstate(all="ignore"):
        for f in range(F):
            c = cen[f]
            valid = (ar_p < count[f]) & (c[:, 3] != 0) & np.isfinite(c[:, :3]).all(axis=1)
            live0 = live.copy()
            d = c[None, :, :3] - pos[:, None, :]                          # [S, P, 3]
            d2 = (d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1]) + d[..., 2] * d[..., 2]     # separately rounded: NumPy fuses nothing
            ok = live0[:, None] & valid[None, :] & (d2 <= g2)
            ss, pp = np.nonzero(ok)
            order = np.lexsort((pp, ss, d2[ss, pp]))                      # by d2, then s, then p: the greedy's pick order
            got_slot = np.zeros(S, dtype=bool)
            got_person = np.zeros(P, dtype=bool)
            for k in order:
                s, p = int(ss[k]), int(pp[k])
                if got_slot[s] or got_person[p]:
                    continue
                got_slot[s] = got_person[p] = True
                slot_of[f, p], person_of[f, s] = s, p
                pos[s] = c[p, :3]
                missed[s] = 0
            free = [s for s in range(S) if not live0[s]]                   # births never re-use a slot freed in this frame
            for p in range(P):
                if not valid[p] or got_person[p]:
                    continue
                if not free:
                    flags[f] |= TRACK_FLAG_OVERFLOW
                    continue
                s = free.pop(0)
                live[s], missed[s], ids[s] = True, 0, next_id
                next_id += 1
                pos[s] = c[p, :3]
                slot_of[f, p], person_of[f, s] = s, p
            for s in range(S):
                if person_of[f, s] >= 0:
                    track_id[f, s] = ids[s]
                elif live0[s]:
                    missed[s] += 1
                    if missed[s] > max_missed:
                        live[s] = False
    st["next_id"] = next_id
    return slot_of, person_of, track_id, flags, st


def gather_reference(xyzs, person_of):
    """xyzs_tracked[f][s] = xyzs[f][person_of[f][s]] (bit for bit), zeros where person_of is -1."""
    xyzs = np.asarray(xyzs)
    F, S = person_of.shape
    out = np.zeros((F, S) + xyzs.shape[2:], dtype=xyzs.dtype)
    ff, ss = np.nonzero(person_of >= 0)
    out[ff, ss] = xyzs[ff, person_of[ff, ss]]
    return out


def bridge_track_ids(track_id, max_gap):
    """track_id [F, S] as the tracker writes it (-1 = slot empty in this frame) -> a copy in which, per slot, a run of -1 of
    length <= max_gap between two frames that carry the SAME id takes that id: the person was lost for a moment and came back
    to the slot (which max_missed kept for them).  Runs between different ids, and leading or trailing runs, stay -1.  NumPy."""
    tid = np.array(track_id, dtype=np.int32, copy=True)
    assert tid.ndim == 2
    for s in range(tid.shape[1]):
        seen = np.nonzero(tid[:, s] >= 0)[0]
        for a, b in zip(seen[:-1], seen[1:]):
            if 1 <= b - a - 1 <= int(max_gap) and tid[a, s] == tid[b, s]:
                tid[a + 1:b, s] = tid[a, s]
    return tid


class PersonTracker:
    """The tracker on the GPU.  ctx_or_rig: a _lib.Context to share (e.g. BatchTriangulator.ctx), a (K, R, t) rig, or None
    for the rig-less scratch context of the current device.  The state lives where the last call's data lived (device
    memory for run_torch, a NumPy blob for run_host) and is moved if the two are mixed; reset() starts over."""

    def __init__(self, ctx_or_rig=None, S=MAX_SLOTS, center_point_index=18, gate=0.3, max_missed=0):
        if isinstance(ctx_or_rig, _lib.Context):
            self.ctx, self._own = ctx_or_rig, False
        elif ctx_or_rig is None:
            self.ctx, self._own = _lib.scratch_context(), False
        else:
            K, R, t = ctx_or_rig
            self.ctx, self._own = _lib.Context(K, R, t), True
        self.S, self.cpi, self.gate, self.max_missed = int(S), int(center_point_index), float(gate), int(max_missed)
        nbytes = int(self.ctx.L.snowtri_track_state_bytes(self.S))
        if nbytes <= 0:
            raise ValueError(f"S must lie in 1..{MAX_SLOTS} (got {S})")
        self.state_nbytes = nbytes
        self._state = None

    def reset(self):
        self._state = None

    def close(self):
        if self._own:
            self.ctx.close()
        self._state = None

    def state_blob(self):
        """Host copy of the state (uint8 [snowtri_track_state_bytes(S)]); all-zero before the first call."""
        if self._state is None:
            return np.zeros(self.state_nbytes, dtype=np.uint8)
        return self._state.copy() if isinstance(self._state, np.ndarray) else self._state.cpu().numpy()

    def _raise(self, rc, where):
        if rc == _lib.ERR_BAD_INDEX:
            raise IndexError(f"{where}: {self.ctx.L.snowtri_last_error().decode()}")
        if rc == _lib.ERR_BAD_ARG:
            raise ValueError(f"{where}: {self.ctx.L.snowtri_last_error().decode()}")
        _lib.check(rc, where)

    def _run(self, space, xyzs, count, gather, state_in):
        """One call in `space`.  state_in: None (state = NULL), or a function that gives the state blob in that space; it is asked only
        once the arguments have passed their checks, so a refused call leaves the state where it was."""
        xyzs, code = space.floats(xyzs, "joints")
        if len(xyzs.shape) != 4 or xyzs.shape[-1] != 4:
            raise ValueError(f"xyzs must be [F, Pout_max, kn, 4] records (got shape {tuple(xyzs.shape)})")
        F, P, kn, _ = (int(v) for v in xyzs.shape)
        count = space.ints(count, (F,), "count")
        state = state_in() if state_in else None
        L, h, S, tail = self.ctx.L, self.ctx.handle, self.S, space.tail()
        out = dict(slot_of=space.empty((F, P), "int32"), person_of=space.empty((F, S), "int32"), track_id=space.empty((F, S), "int32"),
                   flags=space.empty((F,), "flags"))
        rc = L.snowtri_track_persons(h, F, P, kn, _lib.ptr(xyzs), code, _lib.ptr(count), S, self.cpi, self.gate, self.max_missed,
                                     _lib.ptr(state), _lib.ptr(out["slot_of"]), _lib.ptr(out["person_of"]), _lib.ptr(out["track_id"]),
                                     _lib.ptr(out["flags"]), *tail)
        if rc:
            self._raise(rc, "snowtri_track_persons")
        if gather:
            out["xyzs_tracked"] = space.empty((F, S, kn, 4), "float32" if code == _lib.F32 else "float64")
            rc = L.snowtri_track_gather(h, F, P, kn, _lib.ptr(xyzs), code, S, _lib.ptr(out["person_of"]), _lib.ptr(out["xyzs_tracked"]), *tail)
            if rc:
                self._raise(rc, "snowtri_track_gather")
        return out

    def run_host(self, xyzs, count, gather=True, carry=True):
        """NumPy in / NumPy out (staged, synchronous).  carry=False: a fresh start that is not saved (state = NULL)."""
        def state():
            if self._state is None:
                self._state = np.zeros(self.state_nbytes, dtype=np.uint8)
            elif not isinstance(self._state, np.ndarray):
                self._state = self._state.cpu().numpy()
            return self._state
        return self._run(_lib.Space("PersonTracker.run_host"), xyzs, np.reshape(count, -1), gather, state if carry else None)

    def run_torch(self, xyzs, count, gather=True, carry=True, stream=None):
        """CUDA(=HIP) tensors in / out, asynchronous on `stream` (default: torch's current stream); no host read."""
        import torch
        space = _lib.Space("PersonTracker.run_torch", xyzs, count, stream=stream)
        if space.device is None:
            raise ValueError("PersonTracker.run_torch takes contiguous CUDA tensors (run_host takes NumPy arrays)")

        def state():
            if self._state is None:
                self._state = torch.zeros(self.state_nbytes, dtype=torch.uint8, device=space.device)
            elif isinstance(self._state, np.ndarray):
                self._state = torch.from_numpy(self._state).to(space.device)
            return self._state
        return self._run(space, xyzs, count.view(-1) if count.is_contiguous() else count, gather, state if carry else None)
