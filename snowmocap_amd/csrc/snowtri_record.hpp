// snowtri_record.hpp -- what the streaming passes over a track of joint records xyzs[T][m][4] share (k_fill_gaps in
// snowtri_fill.hpp, k_despike in snowtri_despike.hpp): the record as the bits it is stored as, the rule that makes a record
// MISSING (include/snowtri.h, "Gap filling" rule 1 and "Despiking" rule 1), and the tile a wave owns.
#pragma once
#include "snowtri_math.hpp"

namespace snowtri {

// The geometry of a record pass: one thread per lane l < m, consecutive threads on consecutive lanes, so a wave reads 64 adjacent
// 16- or 32-byte records of one frame with 16-byte loads.  A wave owns a TILE of 64 lanes x kRecBlockFrames frames and writes
// exactly the records of its tile; a workgroup is kRecWaves tiles, consecutive in time, of the same 64 lanes, on a one-dimensional
// grid of ncols = ceil(m / 64) columns.
constexpr int kRecBlockFrames = 64;   // frames per tile
constexpr int kRecWaves = 4;          // tiles (consecutive in time) per workgroup

// The tile of the calling thread: its lane l and the frames [t0, t1) it writes; `nothing`: the lane or the tile lies outside the
// track.  UniformWave takes the wave's index through readfirstlane, which tells the compiler that t0 and t1 are wave-uniform
// (there is one wave per threadIdx.y); k_despike says why it needs that, k_fill_gaps does without.
struct RecTile {
    int64_t l, t0, t1;
    bool nothing;
};
template <bool UniformWave>
__device__ __forceinline__ RecTile rec_tile(int64_t T, int64_t m, int64_t ncols) {
    const int64_t wg = blockIdx.x;
    const int64_t row = wg / ncols, col = wg - row * ncols;
    RecTile r;
    r.l = col * 64 + threadIdx.x;
    if constexpr (UniformWave)
        r.t0 = (row * kRecWaves + __builtin_amdgcn_readfirstlane((int)threadIdx.y)) * kRecBlockFrames;
    else
        r.t0 = (row * kRecWaves + threadIdx.y) * kRecBlockFrames;
    r.nothing = r.l >= m || r.t0 >= T;
    r.t1 = r.t0 + kRecBlockFrames < T ? r.t0 + kRecBlockFrames : T;
    return r;
}

// One record as the bits it is stored as: 16 bytes (float) or 32 bytes (double).
template <typename IO>
struct Rec {
    static constexpr int NQ = (int)sizeof(IO) / 4;   // 16-byte words per record
    uint4 q[NQ];
};

template <typename IO>
__device__ __forceinline__ Rec<IO> rec_load(const uint4 *__restrict__ base, int64_t rec) {
    Rec<IO> r;
#pragma unroll
    for (int i = 0; i < Rec<IO>::NQ; i++) r.q[i] = base[rec * Rec<IO>::NQ + i];
    return r;
}

template <typename IO>
__device__ __forceinline__ void rec_store(uint4 *__restrict__ base, int64_t rec, const Rec<IO> &r) {
#pragma unroll
    for (int i = 0; i < Rec<IO>::NQ; i++) base[rec * Rec<IO>::NQ + i] = r.q[i];
}

__device__ __forceinline__ void rec_values(const Rec<float> &r, double v[4]) {
    v[0] = (double)__uint_as_float(r.q[0].x), v[1] = (double)__uint_as_float(r.q[0].y);
    v[2] = (double)__uint_as_float(r.q[0].z), v[3] = (double)__uint_as_float(r.q[0].w);
}
__device__ __forceinline__ void rec_values(const Rec<double> &r, double v[4]) {
    v[0] = __hiloint2double((int)r.q[0].y, (int)r.q[0].x), v[1] = __hiloint2double((int)r.q[0].w, (int)r.q[0].z);
    v[2] = __hiloint2double((int)r.q[1].y, (int)r.q[1].x), v[3] = __hiloint2double((int)r.q[1].w, (int)r.q[1].z);
}
__device__ __forceinline__ void rec_pack(const double v[4], Rec<float> &r) {
    r.q[0] = make_uint4(__float_as_uint((float)v[0]), __float_as_uint((float)v[1]), __float_as_uint((float)v[2]), __float_as_uint((float)v[3]));
}
__device__ __forceinline__ void rec_pack(const double v[4], Rec<double> &r) {
    r.q[0] = make_uint4((unsigned)__double2loint(v[0]), (unsigned)__double2hiint(v[0]), (unsigned)__double2loint(v[1]), (unsigned)__double2hiint(v[1]));
    r.q[1] = make_uint4((unsigned)__double2loint(v[2]), (unsigned)__double2hiint(v[2]), (unsigned)__double2loint(v[3]), (unsigned)__double2hiint(v[3]));
}

// a ? x : y word by word (a conditional between two records as objects would send both through memory)
template <typename IO>
__device__ __forceinline__ Rec<IO> rec_select(bool a, const Rec<IO> &x, const Rec<IO> &y) {
    Rec<IO> r;
#pragma unroll
    for (int i = 0; i < Rec<IO>::NQ; i++)
        r.q[i] = make_uint4(a ? x.q[i].x : y.q[i].x, a ? x.q[i].y : y.q[i].y, a ? x.q[i].z : y.q[i].z, a ? x.q[i].w : y.q[i].w);
    return r;
}

// MISSING, for every record pass: score == 0 (so -0.0 too) or any of the four values not finite; otherwise MEASURED.  Decided on
// the values converted to fp64.
template <typename IO>
__device__ __forceinline__ bool rec_is_missing(const Rec<IO> &r) {
    double v[4];
    rec_values(r, v);
    return v[3] == 0.0 || !(isfinite(v[0]) && isfinite(v[1]) && isfinite(v[2]) && isfinite(v[3]));
}

}  // namespace snowtri
