// snowtri_despike.hpp -- one- and two-frame jumps taken out of a track of joint records before gap filling (include/snowtri.h,
// "Despiking").
//
// A joint that was SEEN in the wrong place for a frame or two (a flipped limb, a hand found on the neighbour) counts as measured:
// the gap filler leaves it alone and the second-order filter rings on it.  k_despike rewrites xyzs[T][m][4] -> out[T][m][4]: a
// measured record further than tol from the per-coordinate median of the measured records of its lane at frames t - H .. t + H
// (itself included, at least three of them) is a SPIKE and becomes the zero record (MARK: the gap filler takes over) or the
// median with its own score (REPLACE); everything else is copied bit for bit.  Every verdict is made on the input: no iteration.
//
// The geometry is k_fill_gaps': one thread per lane l < m, consecutive threads on consecutive lanes, so a wave reads 64 adjacent
// 16- or 32-byte records of one frame with 16-byte loads; a wave owns a TILE of 64 lanes x kRecBlockFrames frames (four
// tiles, consecutive in time, per workgroup), writes exactly the records of its tile and reads, besides them, the H frames
// before and the H frames after it (clipped to the array): 1 + 2 H / kRecBlockFrames reads and 1 write per record.
//
// Inside a tile two rings of W = 2 H + 1 slots stay in registers, slot of frame t = (t - t0) mod W in both:
//   win   the WINDOW: x, y, z of frames t - H .. t + H as fp64, +infinity where the record is missing or outside the array, and
//         one bit per slot for "measured" (n = popcount);
//   raw   the records of frames t .. t + 2 H as the bits they are stored as: the centre's, so that a copy is bit for bit, and
//         the loads on their way -- the slot of the centre is refilled with frame t + W as soon as the centre has been taken
//         out, and a record enters the window H steps after its load was issued: H records (2 H 16-byte loads with fp64 I/O) are
//         in flight per lane.
// The frame loop is unrolled by W (the idiom of trip() in snowtri_fill.hpp), so neither ring ever moves between registers and
// every slot index is a constant.  The median of a coordinate is a fixed compare-exchange network on the W values (3 / 9 / 16 /
// 25 exchanges of one v_min_f64 + one v_max_f64 for W = 3 / 5 / 7 / 9; operands are finite or +infinity, never NaN): the n
// measured values come out first, ascending, and the two middle ones for the lane's n are picked by selects.
// No LDS, no atomics, no communication between workgroups; the result does not depend on the tile length.
//
// EXPECTED BOUND: HBM.  With fp64 records the three networks, the picks and the test compile to ~185 VALU instructions per record
// at H = 3 (~80 v_min / v_max_f64, ~70 v_cndmask_b32; ~240 at H = 4, ~90 at H = 1) against 64 + 6 bytes moved.  The chip issues
// ~39 T non-packed fp64 lane-operations/s (78.6 Tflop/s counts an fma as two) and moves ~5 TB/s in a streaming kernel: 70 bytes take
// as long as ~550 operations, so every H should sit under the memory roof with fp64 records, and float32 records (half the bytes,
// 9 conversions more per step) should come near the VALU roof only at H = 4.  Measured (EXPERIMENTS.md round 14): the fp64 time
// does not move with H (0.727 ... 0.733 ms for H = 1 ... 4 on 100 000 x 532 records), float32 rises 11 % from H = 3 to H = 4.
//
// A neighbouring tile READS records of this tile through `in` while this one writes them through `out`: the two arrays must not
// overlap (the host refuses).  The decision arithmetic is written with contraction off -- med = (a + b) * 0.5, d = v - med,
// d2 = (dx dx + dy dy) + dz dz, each operation rounded once -- which are the bits
// snowmocap_amd/despike.py::despike_joint_track_reference computes.
#pragma once
#include <type_traits>
#include "snowtri_record.hpp"

namespace snowtri {

constexpr int kDespikeMaxHalf = 4;        // half_window: 1 .. 4

enum : unsigned char { kDespikeKept = 0, kDespikeSpike = 1, kDespikeMissing = 2, kDespikeUnsupported = 3 };
enum : int { kDespikeMark = 0, kDespikeReplace = 1 };

// One compare-exchange: two instructions.  (fmin / fmax would be these two behind a canonicalising v_max_f64 x, x of every operand
// the compiler cannot prove quiet -- every value of the window, at every step; the operands here are finite or +infinity.)
__device__ __forceinline__ void despike_cx(double &a, double &b) {
    double lo, hi;
    asm("v_min_f64 %0, %1, %2" : "=v"(lo) : "v"(a), "v"(b));
    asm("v_max_f64 %0, %1, %2" : "=v"(hi) : "v"(a), "v"(b));
    a = lo, b = hi;
}

// Sorting networks of minimal size (Knuth, TAOCP 3, 5.3.4; each is checked on all 2^W zero-one inputs by tests/test_despike_host.py,
// which reads the exchanges from this file).
template <int W>
__device__ __forceinline__ void despike_sort(double (&v)[W]);
// clang-format off
#define CX(i, j) despike_cx(v[i], v[j])
template <> __device__ __forceinline__ void despike_sort<3>(double (&v)[3]) {
    CX(0, 2); CX(0, 1); CX(1, 2);
}
template <> __device__ __forceinline__ void despike_sort<5>(double (&v)[5]) {
    CX(0, 3); CX(1, 4); CX(0, 2); CX(1, 3); CX(0, 1); CX(2, 4); CX(1, 2); CX(3, 4); CX(2, 3);
}
template <> __device__ __forceinline__ void despike_sort<7>(double (&v)[7]) {
    CX(0, 6); CX(2, 3); CX(4, 5); CX(0, 2); CX(1, 4); CX(3, 6); CX(0, 1); CX(2, 5); CX(3, 4); CX(1, 2); CX(4, 6); CX(2, 3); CX(4, 5);
    CX(1, 2); CX(3, 4); CX(5, 6);
}
template <> __device__ __forceinline__ void despike_sort<9>(double (&v)[9]) {
    CX(0, 3); CX(1, 7); CX(2, 5); CX(4, 8); CX(0, 7); CX(2, 4); CX(3, 8); CX(5, 6); CX(0, 2); CX(1, 3); CX(4, 5); CX(7, 8); CX(1, 4);
    CX(3, 6); CX(5, 7); CX(0, 1); CX(2, 4); CX(3, 5); CX(6, 8); CX(2, 3); CX(4, 5); CX(6, 7); CX(1, 2); CX(3, 4); CX(5, 6);
}
#undef CX
// clang-format on

// (v[(n - 1) / 2] + v[n / 2]) * 0.5 of the ascending values: the n measured ones come first, the +infinity of the missing slots
// last.  n = 0 (a missing centre: the result is not used) reads v[0].
template <int H>
__device__ __forceinline__ double despike_median(double (&v)[2 * H + 1], int n) {
#pragma clang fp contract(off)
    despike_sort<2 * H + 1>(v);
    const int lo = (n - 1) >> 1, hi = n >> 1;   // both <= H
    double a = v[0], b = v[0];
#pragma unroll
    for (int k = 1; k <= H; k++) {
        a = lo == k ? v[k] : a;
        b = hi == k ? v[k] : b;
    }
    const double s = a + b;
    return s * 0.5;
}

// The spike's replacement: (mx + 0.0, my + 0.0, mz + 0.0) rounded once to the I/O type (+ 0.0: a zero median is +0.0 whichever
// zero the network left in the middle), the record's own score bits.
__device__ __forceinline__ Rec<float> despike_replacement(const Rec<float> &cur, const double med[3]) {
    double v[4] = {med[0] + 0.0, med[1] + 0.0, med[2] + 0.0, 0.0};
    Rec<float> r;
    rec_pack(v, r);
    r.q[0].w = cur.q[0].w;
    return r;
}
__device__ __forceinline__ Rec<double> despike_replacement(const Rec<double> &cur, const double med[3]) {
    double v[4] = {med[0] + 0.0, med[1] + 0.0, med[2] + 0.0, 0.0};
    Rec<double> r;
    rec_pack(v, r);
    r.q[1].z = cur.q[1].z, r.q[1].w = cur.q[1].w;
    return r;
}

// The window ring: coordinates as fp64 (+infinity = not measured), one bit per slot for "measured".
template <int W>
struct DespikeWindow {
    double x[W], y[W], z[W];
    unsigned measured;

    template <typename IO>
    __device__ __forceinline__ void enter(int slot, const Rec<IO> &r) {
        double v[4];
        rec_values(r, v);
        const bool ok = !rec_is_missing(r);
        const double inf = __longlong_as_double(0x7ff0000000000000ll);
        x[slot] = ok ? v[0] : inf, y[slot] = ok ? v[1] : inf, z[slot] = ok ? v[2] : inf;
        measured = (measured & ~(1u << slot)) | ((ok ? 1u : 0u) << slot);
    }
};

template <typename IO, int H>
__global__ __launch_bounds__(64 * kRecWaves, 2) void k_despike(int64_t T, int64_t m, double tol2, int mode, int64_t ncols,
                                                               const uint4 *__restrict__ in, uint4 *__restrict__ out,
                                                               unsigned char *__restrict__ codes) {
    constexpr int W = 2 * H + 1;
    static_assert(H >= 1 && H <= kDespikeMaxHalf, "half_window");
    const RecTile own = rec_tile<true>(T, m, ncols);       // (one wave per y, taken as uniform: the frame loops below are uniform)
    if (own.nothing) return;
    const int64_t l = own.l, t0 = own.t0, t1 = own.t1;     // the tile: frames [t0, t1)
    const int64_t tend = t1 + H < T ? t1 + H : T;          // frames read: [max(0, t0 - H), tend)
    SNOWTRI_DEV_CHECK(l >= 0 && t0 >= 0 && t0 < t1 && t1 <= tend && tend <= T && (mode == kDespikeMark || mode == kDespikeReplace), 91);
    const Rec<IO> zero = {};   // score 0: missing

    // the halo behind the tile and the first W frames from t0 on, all loads issued before the first is looked at
    Rec<IO> halo[H], raw[W];
    int64_t r = t0 * m + l;        // record index of the centre frame, stepped by m
#pragma unroll
    for (int k = 0; k < H; k++) {
        const int64_t t = t0 - H + k;
        SNOWTRI_DEV_CHECK(t < 0 || (r - (int64_t)(H - k) * m == t * m + l && t < T), 93);
        halo[k] = t >= 0 ? rec_load<IO>(in, r - (int64_t)(H - k) * m) : zero;
    }
#pragma unroll
    for (int k = 0; k < W; k++) raw[k] = t0 + k < tend ? rec_load<IO>(in, r + (int64_t)k * m) : zero;
    DespikeWindow<W> win;
    win.measured = 0;
#pragma unroll
    for (int k = 0; k < H; k++) win.template enter<IO>(H + 1 + k, halo[k]);   // frame t0 - H + k: slot (k - H) mod W
#pragma unroll
    for (int k = 0; k < H; k++) win.template enter<IO>(k, raw[k]);

    const int64_t ahead = (int64_t)W * m;
    auto trip = [&](const int64_t tc, auto guarded) {
#pragma unroll
        for (int i = 0; i < W; i++) {
            const int64_t t = tc + i;
            if (decltype(guarded)::value && t >= t1) break;
            // the centre leaves the raw ring, frame t + W takes its slot; frame t + H enters the window
            const Rec<IO> cur = raw[i];
            if (!decltype(guarded)::value || t + W < tend) {
                SNOWTRI_DEV_CHECK(r + ahead == (t + W) * m + l && t + W < tend, 92);
                raw[i] = rec_load<IO>(in, r + ahead);
            } else {
                raw[i] = zero;
            }
            win.template enter<IO>((i + H) % W, raw[(i + H) % W]);

            const bool meas = (win.measured >> i) & 1u;
            const int n = __popc(win.measured);
            double med[3], d2;
            {
#pragma clang fp contract(off)   // every operation rounded separately: the bits NumPy computes
                double v[W];   // (the network sorts in place: a copy of the ring)
#pragma unroll
                for (int k = 0; k < W; k++) v[k] = win.x[k];
                med[0] = despike_median<H>(v, n);
#pragma unroll
                for (int k = 0; k < W; k++) v[k] = win.y[k];
                med[1] = despike_median<H>(v, n);
#pragma unroll
                for (int k = 0; k < W; k++) v[k] = win.z[k];
                med[2] = despike_median<H>(v, n);
                const double dx = win.x[i] - med[0], dy = win.y[i] - med[1], dz = win.z[i] - med[2];
                const double xx = dx * dx, yy = dy * dy, zz = dz * dz;
                const double s = xx + yy;
                d2 = s + zz;
            }
            const bool spike = meas && n >= 3 && d2 > tol2;   // (false for a NaN d2)
            const Rec<IO> rep = rec_select<IO>(mode == kDespikeReplace, despike_replacement(cur, med), zero);
            SNOWTRI_DEV_CHECK(r == t * m + l && t >= t0 && t < t1 && l < m, 90);
            rec_store<IO>(out, r, rec_select<IO>(spike, rep, cur));
            if (codes) codes[r] = !meas ? kDespikeMissing : spike ? kDespikeSpike : n >= 3 ? kDespikeKept : kDespikeUnsupported;
            r += m;
        }
    };
    // trips all of whose frames lie in the tile and all of whose refills lie inside [0, tend): tc + W <= t1 and tc + 2 W <= tend.
    // A COUNTED loop on a wave-uniform count: with the two comparisons as the loop condition, or a frame index the compiler cannot
    // prove uniform, the rings are copied register to register at the back edge and fp64 H = 4 spills at 256 VGPRs (177 this way).
    const int64_t room = (t1 - W < tend - 2 * W ? t1 - W : tend - 2 * W) - t0;
    const int full = room >= 0 ? (int)(room / W) + 1 : 0;
    int64_t tc = t0;
#pragma unroll 1
    for (int it = 0; it < full; it++, tc += W) trip(tc, std::false_type{});
#pragma unroll 1
    for (; tc < t1; tc += W) trip(tc, std::true_type{});
}

}  // namespace snowtri
