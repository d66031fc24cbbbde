"""The tracking rule (include/snowtri.h, "Person tracking") on hand-built tracks with INTEGER coordinates, where d2 is exact:
snowmocap_amd.tracking.track_persons_reference, the NumPy restatement the GPU kernels are compared with.  No GPU."""
import numpy as np
import pytest

from snowmocap_amd import _lib, tracking
from snowmocap_amd.tracking import TRACK_FLAG_OVERFLOW, track_persons_reference

KN, CPI = 3, 1


def scene(frames, P=4, dtype=np.float64):
    """frames: per frame a list of (x, y, z) or (x, y, z, score) centres in list order -> xyzs [F, P, KN, 4], count [F]."""
    F = len(frames)
    xyzs = np.zeros((F, P, KN, 4), dtype=dtype)
    count = np.zeros(F, dtype=np.int32)
    for f, people in enumerate(frames):
        count[f] = len(people)
        for p, c in enumerate(people):
            xyzs[f, p, :, :3] = 1000.0 + p                # the other joints are far away: only the centre joint may be read
            xyzs[f, p, :, 3] = 1.0
            xyzs[f, p, CPI, :3] = c[:3]
            xyzs[f, p, CPI, 3] = c[3] if len(c) > 3 else 2.0
    return xyzs, count


def run(frames, S=4, gate=2.0, max_missed=1, P=4, state=None):
    xyzs, count = scene(frames, P)
    return track_persons_reference(xyzs, count, S, CPI, gate, max_missed, state=state)


A, B = (0, 0, 0), (10, 0, 0)


def test_two_persons_swapping_list_order_keep_their_slots_and_ids():
    slot_of, person_of, track_id, flags, _ = run([[A, B], [B, A], [(1, 0, 0), (11, 0, 0)], [(11, 0, 0), (1, 0, 0)]])
    assert slot_of[:, :2].tolist() == [[0, 1], [1, 0], [0, 1], [1, 0]]
    assert person_of[:, :2].tolist() == [[0, 1], [1, 0], [0, 1], [1, 0]]
    assert (track_id[:, :2] == [0, 1]).all() and (track_id[:, 2:] == -1).all() and (person_of[:, 2:] == -1).all()
    assert (slot_of[:, 2:] == -1).all() and not flags.any()


@pytest.mark.parametrize("max_missed", [1, 3])
def test_dropout_of_max_missed_frames_keeps_id_and_slot_one_more_gets_a_new_id_in_the_reused_slot(max_missed):
    kept = [[A, B]] + [[A]] * max_missed + [[A, B]]
    _, person_of, track_id, _, st = run(kept, max_missed=max_missed)
    assert person_of[-1, :2].tolist() == [0, 1] and track_id[-1, :2].tolist() == [0, 1]
    assert (person_of[1:-1, 1] == -1).all() and (track_id[1:-1, 1] == -1).all()
    assert st["next_id"] == 2 and st["missed"][1] == 0
    lost = [[A, B]] + [[A]] * (max_missed + 1) + [[A, B]]
    slot_of, person_of, track_id, _, st = run(lost, max_missed=max_missed)
    assert slot_of[-1, :2].tolist() == [0, 1] and track_id[-1, :2].tolist() == [0, 2]       # slot 1 again, a new identity
    assert st["next_id"] == 3


def test_births_use_only_slots_free_at_the_start_of_the_frame():
    # slot 0 (A) dies in frame 1 (max_missed = 0); the newcomer of frame 1 must not take it in that frame, only later ones may
    C, D = (20, 0, 0), (30, 0, 0)
    slot_of, person_of, track_id, flags, _ = run([[A, B], [B, C], [B, C, D]], max_missed=0, S=3)
    assert person_of[1].tolist() == [-1, 0, 1] and track_id[1].tolist() == [-1, 1, 2]
    assert person_of[2].tolist() == [2, 0, 1] and track_id[2].tolist() == [3, 1, 2]
    assert slot_of[2, :3].tolist() == [1, 2, 0] and not flags.any()
    # with every other slot busy the newcomer of the frame in which a slot dies overflows, and is born one frame later
    slot_of, person_of, track_id, flags, _ = run([[A, B], [B, C], [B, C]], max_missed=0, S=2)
    assert slot_of[1, :2].tolist() == [1, -1] and flags.tolist() == [0, TRACK_FLAG_OVERFLOW, 0]
    assert person_of[2].tolist() == [1, 0] and track_id[2].tolist() == [2, 1]


def test_full_slots_set_the_overflow_flag():
    slot_of, person_of, track_id, flags, st = run([[A, B, (20, 0, 0)], [A, B, (20, 0, 0)]], S=2)
    assert slot_of[:, :3].tolist() == [[0, 1, -1]] * 2 and flags.tolist() == [TRACK_FLAG_OVERFLOW] * 2
    assert track_id.tolist() == [[0, 1]] * 2 and st["next_id"] == 2


def test_equal_distances_go_to_the_lowest_slot_then_the_lowest_person():
    # slots 0, 1 at x = 0, 4; one person at x = 2: d2 = 4 to both -> slot 0
    _, person_of, _, _, _ = run([[(0, 0, 0), (4, 0, 0)], [(2, 0, 0)]], gate=3.0)
    assert person_of[1, :2].tolist() == [0, -1]
    # slot 0 at x = 2; persons at x = 0 and 4: d2 = 4 from both -> person 0; person 1 is born in slot 1
    slot_of, person_of, track_id, _, _ = run([[(2, 0, 0)], [(0, 0, 0), (4, 0, 0)]], gate=3.0)
    assert slot_of[1, :2].tolist() == [0, 1] and track_id[1, :2].tolist() == [0, 1]
    # a 2 x 2 square of ties: slots at (0,0), (2,2); persons at (2,0), (0,2): all four d2 = 4 -> (s0, p0) then (s1, p1)
    _, person_of, _, _, _ = run([[(0, 0, 0), (2, 2, 0)], [(2, 0, 0), (0, 2, 0)]], gate=3.0)
    assert person_of[1, :2].tolist() == [0, 1]
    # the smaller distance wins over the lower index: slots at 0 and 5, persons at 4 (p0) and 1 (p1)
    _, person_of, _, _, _ = run([[(0, 0, 0), (5, 0, 0)], [(4, 0, 0), (1, 0, 0)]], gate=10.0)
    assert person_of[1, :2].tolist() == [1, 0]


def test_a_distance_equal_to_the_gate_matches_and_one_beyond_does_not():
    _, _, track_id, _, _ = run([[A], [(3, 4, 0)]], gate=5.0)              # d2 = 25 = gate^2
    assert track_id[1, :2].tolist() == [0, -1]
    _, _, track_id, _, _ = run([[A], [(3, 4, 1)]], gate=5.0)              # d2 = 26
    assert track_id[1, :2].tolist() == [-1, 1]
    _, _, track_id, _, _ = run([[A], [A]], gate=0.0)                      # a zero gate still matches an unmoved person
    assert track_id[1, :2].tolist() == [0, -1]


def test_centres_with_score_zero_or_a_nan_are_skipped():
    frames = [[A, B], [(0, 0, 0, 0.0), B], [(np.nan, 0, 0), B], [(0, np.inf, 0), B], [A, B]]
    slot_of, person_of, track_id, flags, _ = run(frames, max_missed=5)
    assert slot_of[1:4, 0].tolist() == [-1, -1, -1] and (slot_of[:, 1] == 1).all()
    assert person_of[:, 0].tolist() == [0, -1, -1, -1, 0] and track_id[:, 0].tolist() == [0, -1, -1, -1, 0]
    assert not flags.any()
    # a NaN score is a score != 0: the person counts
    _, _, track_id, _, _ = run([[(0, 0, 0, np.nan)]])
    assert track_id[0, 0] == 0


def test_frames_without_persons_age_the_slots():
    slot_of, person_of, track_id, flags, st = run([[A], [], [], [A]], max_missed=2)
    assert track_id[:, 0].tolist() == [0, -1, -1, 0] and (slot_of[1:3] == -1).all()
    _, _, track_id, _, st = run([[A], [], [], [], [A]], max_missed=2)
    assert track_id[:, 0].tolist() == [0, -1, -1, -1, 1]
    out = run([[], []])
    assert (out[0] == -1).all() and (out[1] == -1).all() and (out[2] == -1).all() and out[4]["next_id"] == 0
    # persons listed behind count[f] are not there
    xyzs, count = scene([[A, B]])
    count[0] = 1
    slot_of = track_persons_reference(xyzs, count, 4, CPI, 2.0, 1)[0]
    assert slot_of[0].tolist() == [0, -1, -1, -1]


def _random_scene(seed, F=40, P=5):
    rng = np.random.default_rng(seed)
    frames = []
    pos = rng.integers(-20, 20, size=(P, 3))
    for f in range(F):
        pos = pos + rng.integers(-1, 2, size=pos.shape)
        here = [tuple(int(v) for v in pos[p]) for p in rng.permutation(P) if rng.random() < 0.8]
        frames.append(here)
    return frames


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_chunked_calls_with_state_equal_one_whole_call(dtype):
    frames = _random_scene(5)
    xyzs, count = scene(frames, P=5, dtype=dtype)
    whole = track_persons_reference(xyzs, count, 6, CPI, 3.0, 2)
    assert len(np.unique(whole[2][whole[2] >= 0])) > 5          # tracks end and new ones begin in this scene
    st = None
    parts = []
    for lo, hi in ((0, 7), (7, 8), (8, 8), (8, 31), (31, 40)):
        out = track_persons_reference(xyzs[lo:hi], count[lo:hi], 6, CPI, 3.0, 2, state=st)
        st_before = st
        st = out[4]
        assert st is not st_before                                # the state handed in is not modified
        parts.append(out)
    for k in range(4):
        assert np.array_equal(np.concatenate([p_[k] for p_ in parts]), whole[k])
    for key in ("live", "pos", "missed", "id"):
        keep = whole[4]["live"] if key != "live" else slice(None)
        assert np.array_equal(st[key][keep], whole[4][key][keep])
    assert st["next_id"] == whole[4]["next_id"]
    # the state survives the library's blob format
    blob = tracking.state_to_blob(st)
    back = tracking.state_from_blob(blob, 6)
    assert blob.shape[0] == tracking.state_bytes(6) and back["next_id"] == st["next_id"]
    assert all(np.array_equal(back[k], st[k]) for k in ("live", "pos", "missed", "id"))
    assert not tracking.state_to_blob(tracking.fresh_state(6)).any()      # all-zero = fresh


def test_arguments_are_checked():
    xyzs, count = scene([[A]])
    for kw in (dict(S=0), dict(S=17), dict(gate=-1.0), dict(gate=np.nan), dict(gate=np.inf), dict(max_missed=-1)):
        args = dict(S=4, center_point_index=CPI, gate=1.0, max_missed=0)
        args.update(kw)
        with pytest.raises(ValueError):
            track_persons_reference(xyzs, count, **args)
    for cpi in (-1, KN):
        with pytest.raises(IndexError):
            track_persons_reference(xyzs, count, 4, cpi, 1.0, 0)
    with pytest.raises(ValueError):
        track_persons_reference(np.zeros((1, 17, KN, 4)), np.zeros(1, dtype=np.int32), 4, CPI, 1.0, 0)


def test_state_bytes_is_positive_and_monotone_in_the_slot_count():
    L = _lib.lib()
    sizes = [int(L.snowtri_track_state_bytes(S)) for S in range(1, 17)]
    assert sizes[0] > 0 and all(b > a for a, b in zip(sizes, sizes[1:]))
    assert sizes == [tracking.state_bytes(S) for S in range(1, 17)]
    assert L.snowtri_track_state_bytes(0) == 0 and L.snowtri_track_state_bytes(17) == 0
    assert 1 <= tracking.chain_block_frames() <= 1024


def test_gather_reference_copies_bits():
    xyzs, count = scene([[A, B], [B, A]])
    xyzs[1, 0, 2, 0] = np.nan
    person_of = np.array([[1, -1, 0], [-1, 0, -1]], dtype=np.int32)
    got = tracking.gather_reference(xyzs, person_of)
    assert np.array_equal(got[0, 0].view(np.uint64), xyzs[0, 1].view(np.uint64)) and not got[0, 1].any()
    assert np.array_equal(got[1, 1].view(np.uint64), xyzs[1, 0].view(np.uint64)) and not got[1, 0].any() and not got[1, 2].any()
