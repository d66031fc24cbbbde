// snowtri_fill.hpp -- short dropouts in a track of joint records bridged before smoothing (include/snowtri.h, "Gap filling").
//
// The condense step leaves a joint too few views saw as the record (0, 0, 0, 0), and a tracked person who is absent for a few
// frames leaves whole skeletons of them; the temporal filter would take either for a position at the origin.  k_fill_gaps
// rewrites xyzs[T][m][4] -> out[T][m][4]: a run of at most max_gap MISSING records between two MEASURED ones becomes their
// linear interpolation (code 1), a run that short at either end of the array becomes copies of its one measured neighbour
// (code 2), everything else is copied bit for bit (code 0 measured, code 3 missing and left alone).
//
// One thread per lane l < m, consecutive threads on consecutive lanes: a wave reads 64 adjacent 16- or 32-byte records of one
// frame with 16-byte loads.  A wave owns a TILE of 64 lanes x kRecBlockFrames frames (four tiles, consecutive in time, per
// workgroup) and writes exactly the records of its tile:
//   1. BACKWARDS from the frame before the tile for the nearest measured record A, at most max_gap frames or down to frame 0
//      (one record when the frame before the tile is measured);
//   2. FORWARD through the tile in trips of kFillAhead frames with a window of kFillAhead records: a slot is refilled with the
//      record kFillAhead frames on as soon as it has been read, so a trip's refills are in flight together and the wait at the
//      head of the next trip is for the window as a whole -- one memory latency per kFillAhead frames, not per frame.  The last
//      measured record and the length of the run of missing records behind it stay in registers.  A measured record closes
//      the run: its frames inside the tile are written then.  A run that outgrows max_gap is given up at once -- its frames are
//      copied from the input again (at most max_gap re-reads per run), later frames of it are copied as they come;
//   3. a run still open at the end of the tile is followed FORWARD, at most until it outgrows max_gap or the track ends.
// No LDS, no communication between workgroups, no atomics; the result does not depend on the tile length.  On tracks with few
// dropouts the halo is one extra record per lane and tile: 1 + 1 / kRecBlockFrames reads and 1 write per record from HBM
// (not counted: the re-reads of a run that was given up and the look into a neighbouring tile from a run at the edge, both
// of records some wave has just read).
//
// A neighbouring tile READS records of this tile through `in` while this one writes them through `out`: the two arrays must not
// overlap (the host refuses).  The interpolation is written with contraction off -- w = k / (g + 1), d = B - A, p = w d,
// v = A + p, each rounded once in fp64, v rounded once to the I/O type -- which are the bits
// snowmocap_amd/fill.py::fill_joint_track_reference computes.
#pragma once
#include <type_traits>
#include "snowtri_record.hpp"

namespace snowtri {

constexpr int kFillAhead = 4;          // records a thread has in flight inside its tile
constexpr int kFillMaxGap = 255;

enum : unsigned char { kFillMeasured = 0, kFillLerp = 1, kFillHold = 2, kFillMissing = 3 };

// record k of the g missing ones between A and B, k = 1 .. g
template <typename IO>
__device__ __forceinline__ Rec<IO> fill_lerp(const Rec<IO> &A, const Rec<IO> &B, int k, int g) {
#pragma clang fp contract(off)   // every operation rounded separately: the bits NumPy computes
    double a[4], b[4], v[4];
    rec_values(A, a);
    rec_values(B, b);
    const double w = (double)k / (double)(g + 1);
#pragma unroll
    for (int c = 0; c < 4; c++) {
        const double d = b[c] - a[c];
        const double p = w * d;
        v[c] = a[c] + p;
    }
    Rec<IO> r;
    rec_pack(v, r);
    return r;
}

template <typename IO>
struct FillTile {
    int64_t m, l, t0, t1;   // the lane, and the frames [t0, t1) this thread writes
    int max_gap;
    const uint4 *__restrict__ in;
    uint4 *__restrict__ out;
    unsigned char *__restrict__ fill;

    __device__ __forceinline__ int64_t rec(int64_t t) const { return t * m + l; }
    __device__ __forceinline__ void put_at(int64_t rec_index, const Rec<IO> &r, unsigned char code) const {
        rec_store<IO>(out, rec_index, r);
        if (fill) fill[rec_index] = code;
    }
    __device__ __forceinline__ void put(int64_t t, const Rec<IO> &r, unsigned char code) const {
        SNOWTRI_DEV_CHECK(t >= t0 && t < t1 && l >= 0 && l < m, 80);
        put_at(rec(t), r, code);
    }
    // The run of `run` missing records in front of frame `end` is decided: A (if has_a) is the measured record before it, B (if
    // has_b) the one at `end`.  Writes the frames of the run that lie in the tile.
    __device__ __forceinline__ void resolve(int64_t end, int run, bool has_a, const Rec<IO> &A, bool has_b, const Rec<IO> &B) const {
        const int64_t first = end - run;   // first frame of the run; A sits at first - 1
        const int64_t lo = first > t0 ? first : t0, hi = end < t1 ? end : t1;
        const bool fits = run <= max_gap;
        const Rec<IO> H = rec_select<IO>(has_a, A, B);
        for (int64_t t = lo; t < hi; t++) {
            if (fits && has_a && has_b)
                put(t, fill_lerp<IO>(A, B, (int)(t - first) + 1, run), kFillLerp);
            else if (fits && (has_a || has_b))
                put(t, H, kFillHold);
            else
                put(t, rec_load<IO>(in, rec(t)), kFillMissing);
        }
    }
};

template <typename IO>
__global__ __launch_bounds__(64 * kRecWaves) void k_fill_gaps(int64_t T, int64_t m, int max_gap, int64_t ncols, const uint4 *__restrict__ in,
                                                              uint4 *__restrict__ out, unsigned char *__restrict__ fill) {
    const RecTile own = rec_tile<false>(T, m, ncols);
    if (own.nothing) return;
    FillTile<IO> tile;
    tile.m = m, tile.l = own.l, tile.t0 = own.t0, tile.t1 = own.t1;
    tile.max_gap = max_gap, tile.in = in, tile.out = out, tile.fill = fill;
    const int64_t t0 = tile.t0, t1 = tile.t1;
    SNOWTRI_DEV_CHECK(max_gap >= 1 && max_gap <= kFillMaxGap && t0 >= 0 && t1 <= T, 81);

    // 1. the nearest measured record behind the tile.  None within max_gap frames: the run that enters the tile is as long as
    // the frames looked at, which is either the whole track so far (t0 <= max_gap) or already max_gap, one short of given up.
    Rec<IO> A = {};
    bool has_a = false;
    int run = 0;   // missing records directly in front of the current frame, saturating at max_gap + 1 (= given up)
    for (int64_t t = t0 - 1; t >= 0 && run < max_gap; t--) {
        A = rec_load<IO>(in, tile.rec(t));
        if (!rec_is_missing(A)) {
            has_a = true;
            break;
        }
        run++;
    }

    // 2. the tile, kFillAhead frames per trip: slot i of the window holds frame tc + i and is refilled with frame tc + i +
    // kFillAhead as soon as it has been read, so the loads of the next kFillAhead - 1 frames are outstanding while one is used.
    // The trip is unrolled (the window never moves between registers), and in the trips of the first loop every refill is
    // unconditional: a load behind a branch would leave the compiler no count of the loads in flight to wait on, and it
    // would wait for all of them.  The last one or two trips (refills past the tile's end are skipped, a clipped tile ends
    // inside a trip) run guarded.  r = record index of frame t, stepped by m.
    Rec<IO> q[kFillAhead] = {};
    int64_t r = tile.rec(t0);
    const int64_t ahead = (int64_t)kFillAhead * m;
#pragma unroll
    for (int i = 0; i < kFillAhead; i++)
        if (t0 + i < t1) q[i] = rec_load<IO>(in, r + i * m);
    auto trip = [&](const int64_t tc, auto guarded) {
#pragma unroll
        for (int i = 0; i < kFillAhead; i++) {
            const int64_t t = tc + i;
            if (decltype(guarded)::value && t >= t1) break;
            const Rec<IO> cur = q[i];
            if (!decltype(guarded)::value || t + kFillAhead < t1) {
                SNOWTRI_DEV_CHECK(r + ahead == tile.rec(t + kFillAhead) && t + kFillAhead < t1, 82);
                q[i] = rec_load<IO>(in, r + ahead);
            }
            SNOWTRI_DEV_CHECK(r == tile.rec(t) && t >= t0 && t < t1, 80);
            if (!rec_is_missing(cur)) {
                tile.put_at(r, cur, kFillMeasured);
                if (run > 0 && run <= max_gap) tile.resolve(t, run, has_a, A, true, cur);
                A = cur, has_a = true, run = 0;
            } else if (run > max_gap) {
                tile.put_at(r, cur, kFillMissing);
            } else if (++run > max_gap) {
                tile.resolve(t + 1, run, has_a, A, false, A);   // outgrown: given up, this frame included
            }
            r += m;
        }
    };
    int64_t tc = t0;
#pragma unroll 1
    for (; tc + 2 * kFillAhead <= t1; tc += kFillAhead) trip(tc, std::false_type{});
#pragma unroll 1
    for (; tc < t1; tc += kFillAhead) trip(tc, std::true_type{});

    // 3. a run that leaves the tile undecided
    if (run > 0 && run <= max_gap) {
        Rec<IO> B = {};
        bool has_b = false;
        int64_t t = t1;
        for (; t < T && run <= max_gap; t++) {
            B = rec_load<IO>(in, tile.rec(t));
            if (!rec_is_missing(B)) {
                has_b = true;
                break;
            }
            run++;
        }
        tile.resolve(t, run, has_a, A, has_b, B);
    }
}

}  // namespace snowtri
