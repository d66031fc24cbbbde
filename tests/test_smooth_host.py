"""Rows N1 / N2 where the chunk-to-chunk carry matters, on the CPU (tests/smooth_cases.py): the high-precision reference against
mpmath, the teeth of the case list -- a NumPy twin of k_smooth_scan's association with P = A^256 transposed or zeroed, or R = A^32
transposed, must leave the tolerance by three decades at every CARRY_CASE and stay inside the old tests' 2e-10 at the filter those
use -- and sharded.combine_carries against the high-precision state."""
import numpy as np
import pytest

import smooth_cases as sc

T_TEETH = 1030


def test_the_carry_cases_carry():
    """max|A^256| of the cases against the old tests' filter: what makes a mutant of P visible at all."""
    blind = np.abs(sc.a_power(sc.a_matrix(sc.BLIND_CASE), sc.CHUNK)).max()
    assert blind < 1e-60
    for case in sc.CARRY_CASES:
        A = sc.a_matrix(case)
        assert np.abs(np.linalg.eigvals(A)).max() <= 1.0 + 1e-12, case            # stable: unstable filters overflow in the reference too
        assert np.abs(sc.a_power(A, sc.CHUNK)).max() > 1e-7, case                   # (1.8e-6 ... 3.1 against 1e-20 ... 1e-77 at the 30 fps profiles)
    assert abs(np.abs(np.linalg.eigvals(sc.a_matrix(sc.CARRY_CASES[6]))).max() - 1.0) < 1e-12      # undamped: nothing decays
    assert np.iscomplexobj(np.linalg.eigvals(sc.a_matrix(sc.CARRY_CASES[0])))
    assert np.isrealobj(np.linalg.eigvals(sc.a_matrix(sc.CARRY_CASES[3])))                          # overdamped: no rotation
    for dt in (1 / 30, 1 / 240):
        assert sc.blender_table_is_stable(sc.blender_table(), dt)
    f = sc.blender_table()[:, 0]
    assert np.all(np.diff(f) > 0) and f[0] == 0.05


@pytest.mark.parametrize("ci", range(len(sc.CARRY_CASES)))
def test_longdouble_reference_equals_mpmath(ci):
    """The vectorised longdouble form of the rule against 40 digits on the lanes {0, 63, 64, n - 1}: 2^-60 of the largest |y|.
    (Where np.longdouble has no 64-bit mantissa, `reference` is the mpmath form on every lane, rounded to the widest type there
    is: then this holds that rounding to half an fp64 ulp.)"""
    case = sc.CARRY_CASES[ci]
    x, ry, ryd, _, _ = sc.track_case(ci, T_TEETH, 130)
    lanes = sc.mp_lanes(130)
    assert lanes == [0, 63, 64, 129]
    my, myd = sc.reference_mp(x, case, lanes)
    assert sc.WIDE == (np.finfo(np.longdouble).nmant >= 63)
    bound = (2.0 ** -60 if sc.WIDE else 2.0 ** -53) * float(np.abs(ry).max())
    d = sc.mp_distance(ry[:, lanes], my)
    assert d <= bound, (case, d, bound)


def test_the_state_oracle_is_the_committed_oracle():
    """oracle_state -- the fp64 sequential rule that also returns yd, for the shard tests' bound on yd -- computes the y of
    oracle.second_order_track bit for bit."""
    from oracle import oracle as orc
    for ci in (0, 3, 6):
        x = sc.walk(ci, 600, 7)
        assert np.array_equal(sc.oracle_state(x, sc.CARRY_CASES[ci])[0], orc.second_order_track(x, *sc.CARRY_CASES[ci]))


@pytest.mark.parametrize("ci", range(len(sc.CARRY_CASES)))
def test_a_wrong_P_or_R_leaves_the_tolerance_by_three_decades(ci):
    case = sc.CARRY_CASES[ci]
    x, ry, _, tol, oerr = sc.track_case(ci, T_TEETH, 130)
    A = sc.a_matrix(case)
    Pm, Rm = sc.a_power(A, sc.CHUNK), sc.a_power(A, sc.WAVE)
    for depth in (0, 1, 3, "all"):
        d = sc.distance(sc.twin(x, case, depth=depth), ry)
        print(f"twin case {ci} depth {depth}: err {d:.3e} oracle {oerr:.3e} tol {tol:.3e}")
        assert d <= tol, (case, depth, d, tol)
    for name, kw in (("P transposed", dict(Pm=Pm.T)), ("P = 0", dict(Pm=np.zeros((2, 2)))), ("R transposed", dict(Rm=Rm.T))):
        for depth in (0, "all"):
            d = sc.distance(sc.twin(x, case, depth=depth, **kw), ry)
            print(f"twin case {ci} {name} depth {depth}: shift {d:.3e} = {d / tol:.1e} tol")
            assert d >= 1000 * tol, (case, name, depth, d, tol)


def test_the_old_filter_cannot_see_P():
    """At (2.5 Hz, 0.75, 0.5) and 30 fps the P mutants stay inside the 2e-10 of the older smoothing tests -- why those could not
    tell them from the kernel -- while R, which acts inside a chunk, is seen there too."""
    from oracle import oracle as orc
    case = sc.BLIND_CASE
    x = sc.walk(len(sc.CARRY_CASES), T_TEETH, 130)
    want = orc.second_order_track(x, *case)
    A = sc.a_matrix(case)
    Pm, Rm = sc.a_power(A, sc.CHUNK), sc.a_power(A, sc.WAVE)
    for kw in (dict(), dict(Pm=Pm.T), dict(Pm=np.zeros((2, 2)))):
        for depth in (0, "all"):
            assert np.abs(sc.twin(x, case, depth=depth, **kw) - want).max() < 2e-10
    assert np.abs(sc.twin(x, case, Rm=Rm.T) - want).max() > 2e-10


@pytest.mark.parametrize("ci", sc.SHARD_CASES)
def test_combine_carries_returns_the_state_entering_every_block(ci):
    """sharded.combine_carries on blocks of (1, 256, 0, 300, 33, 700) frames, the payload end states taken from the high-precision
    zero-state responses: for every non-empty rank the entering state is the reference (y, yd) behind the frame before the
    block, corrected for the xd = 0 its first frame is filtered with.  A^m with m up to 700 at filters where it does not vanish."""
    from snowmocap_amd.sharded import combine_carries, smooth_coeffs
    s = sc.shard_case(ci, 5)
    A, cx, cxd = smooth_coeffs(*s["case"])
    for q, size in enumerate(sc.SHARD_SIZES):
        if size == 0:
            continue
        got = combine_carries(s["payloads"], q, A, cxd)
        dy, dyd = sc.distance(got[:, 0], s["start"][q][:, 0]), sc.distance(got[:, 1], s["start"][q][:, 1])
        print(f"combine_carries case {ci} rank {q}: y {dy:.3e} / {s['tol_y']:.3e}, yd {dyd:.3e} / {s['tol_yd']:.3e}")
        assert dy <= s["tol_y"] and dyd <= s["tol_yd"], (s["case"], q, dy, s["tol_y"], dyd, s["tol_yd"])


def test_blender_reference_follows_the_oracle():
    """The per-point reference with the hold (frame 0 as given, zero seed, held input) against oracle/blender.py::smooth_track:
    the same NaN pattern, and values as close as two evaluations of one rule in fp64 and longdouble are."""
    pts, val, fzr, ref, tol, oerr = sc.blender_case(2, 514, 1 / 30)
    from oracle import blender as ob
    want = ob.smooth_track(pts, val, fzr, 1 / 30)
    r64 = ref.astype(np.float64)
    assert np.array_equal(np.isnan(r64), np.isnan(want))
    assert np.isnan(r64[0, 0, 23]).all() and np.isfinite(r64[1:, 0, 23]).all()        # never valid: zeros filtered from a zero seed
    assert np.array_equal(r64[1:, 0, 23], np.zeros_like(r64[1:, 0, 23]))
    assert 0 < oerr < 1e-11 and tol < 2e-10
