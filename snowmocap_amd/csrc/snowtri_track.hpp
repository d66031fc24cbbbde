// snowtri_track.hpp -- cross-frame person tracking behind the outputs of the fused call (include/snowtri.h, "Person tracking").
//
// The condense step lists a frame's persons in the order its clusters formed; the tracker gives them stable SLOTS and
// TRACK IDS by greedy nearest-centre matching from frame to frame.  Three kernels:
//
//   k_track_centres  parallel over (frame, person): the ONE centre record of every person -> centres[F][P][4] fp64
//                    (x, y, z, valid) in context scratch.  valid = p < count[f], score != 0, three finite coordinates.
//   k_track_chain    the recurrence.  It is serial in frames by definition, so ONE wave (wave 0 of one workgroup) walks them;
//                    the S x P <= 256 (slot, person) pairs sit four per lane -- lane = 16 * (s / 4) + p, k = s % 4 -- and a
//                    greedy round is a wave-wide minimum of the fp64 bit pattern of d2 (non-negative, so it orders as an
//                    unsigned integer) followed by four ballots that pick the lowest (s, p) among the lanes that hold it.
//                    The walking wave never waits for HBM: the other three waves of the workgroup copy the next block of
//                    kTrackBlockFrames frames of centres into the idle half of a double-buffered LDS arena and write the
//                    finished block's slot_of / person_of / track_id / flags out, coalesced, while it walks; one barrier
//                    per block.  Slot positions live in LDS (wave-private), live / missed / id in lane s, next_id in
//                    every lane.  State is read from and written to the caller's blob by lanes 0..S-1 (vector accesses).
//   k_track_gather   bandwidth: xyzs_tracked[f][s] = person_of[f][s] >= 0 ? xyzs[f][person_of[f][s]] : 0 as 16-byte records
//                    per lane in the I/O dtype, copied as bits (NaN payloads survive).
//
// d2 = (dx*dx + dy*dy) + dz*dz with every product and sum rounded separately (contraction off): the NumPy restatement
// snowmocap_amd/tracking.py::track_persons_reference computes the same bits, and every integer output agrees with it.
#pragma once
#include "snowtri_math.hpp"

namespace snowtri {

constexpr int kTrackMax = 16;               // S and Pout_max: 1 .. 16
constexpr int kTrackBlockFrames = 32;       // frames per staging block of k_track_chain
constexpr int kTrackChainThreads = 256;     // wave 0 walks, waves 1..3 stage and write out
constexpr int kTrackStagers = kTrackChainThreads - 64;
constexpr unsigned int kTrackFlagOverflow = 1u;

// The state blob: int32 (next_id, 0, 0, 0) | pos [S][3] fp64 | int32 [S][4] (live, missed, id, 0).  All-zero = fresh.
constexpr size_t kTrackStateHeader = 16, kTrackStatePerSlot = 40;
inline size_t track_state_bytes(int S) { return kTrackStateHeader + kTrackStatePerSlot * (size_t)S; }

template <typename TIO>
__global__ __launch_bounds__(256) void k_track_centres(int64_t F, int P, int kn, int centre, const TIO *__restrict__ xyzs,
                                                       const int32_t *__restrict__ count, double *__restrict__ centres) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= F * P) return;
    const int64_t f = i / P;
    const int p = (int)(i - f * P);
    SNOWTRI_DEV_CHECK(f >= 0 && f < F && p >= 0 && p < P && centre >= 0 && centre < kn, 70);
    const size_t rec = (size_t)i * kn + centre;   // the centre record of person (f, p)
    double x, y, z, sc;
    if constexpr (sizeof(TIO) == 4) {
        const float4 v = reinterpret_cast<const float4 *>(xyzs)[rec];
        x = (double)v.x, y = (double)v.y, z = (double)v.z, sc = (double)v.w;
    } else {
        const double2 a = reinterpret_cast<const double2 *>(xyzs)[2 * rec], b = reinterpret_cast<const double2 *>(xyzs)[2 * rec + 1];
        x = a.x, y = a.y, z = b.x, sc = b.y;
    }
    const bool valid = p < count[f] && sc != 0.0 && isfinite(x) && isfinite(y) && isfinite(z);
    double2 *o = reinterpret_cast<double2 *>(centres) + 2 * (size_t)i;
    o[0] = valid ? make_double2(x, y) : make_double2(0.0, 0.0);
    o[1] = valid ? make_double2(z, 1.0) : make_double2(0.0, 0.0);
}

__device__ __forceinline__ double track_d2(double cx, double cy, double cz, double px, double py, double pz) {
#pragma clang fp contract(off)   // every product and sum rounded separately: the bits NumPy computes
    const double dx = cx - px, dy = cy - py, dz = cz - pz;
    const double xx = dx * dx, yy = dy * dy, zz = dz * dz;
    return (xx + yy) + zz;
}

// Minimum of a 64-bit key over the wave, the same value in every lane (and wave-uniform for the compiler).  Rows of 16 lanes
// by four DPP rotations (row_ror 8, 4, 2, 1: afterwards every lane holds its row's minimum), the four rows by v_readlane and
// scalar compares: no LDS crossbar on the chain's critical path (six dependent ds_bpermute pairs before).
__device__ __forceinline__ unsigned long long track_wave_min(unsigned long long v) {
    unsigned int lo = (unsigned int)v, hi = (unsigned int)(v >> 32);
#define SNOWTRI_TRACK_ROR_MIN(CTRL)                                                                          \
    {                                                                                                        \
        const unsigned int olo = (unsigned int)__builtin_amdgcn_update_dpp((int)lo, (int)lo, CTRL, 0xf, 0xf, false); \
        const unsigned int ohi = (unsigned int)__builtin_amdgcn_update_dpp((int)hi, (int)hi, CTRL, 0xf, 0xf, false); \
        const bool less = ohi < hi || (ohi == hi && olo < lo);                                               \
        lo = less ? olo : lo;                                                                                \
        hi = less ? ohi : hi;                                                                                \
    }
    SNOWTRI_TRACK_ROR_MIN(0x128)   // row_ror:8
    SNOWTRI_TRACK_ROR_MIN(0x124)   // row_ror:4
    SNOWTRI_TRACK_ROR_MIN(0x122)   // row_ror:2
    SNOWTRI_TRACK_ROR_MIN(0x121)   // row_ror:1
#undef SNOWTRI_TRACK_ROR_MIN
    unsigned long long m = ~0ull;
#pragma unroll
    for (int row = 0; row < 4; ++row) {
        const unsigned long long r = ((unsigned long long)(unsigned int)__builtin_amdgcn_readlane((int)hi, 16 * row) << 32) |
                                     (unsigned int)__builtin_amdgcn_readlane((int)lo, 16 * row);
        m = r < m ? r : m;
    }
    return m;
}

// position of the r-th set bit of m (r < popcount(m))
__device__ __forceinline__ int track_nth_bit(unsigned int m, int r) {
    for (int i = 0; i < r; ++i) m &= m - 1u;
    return __ffs((int)m) - 1;
}

// lanes of ONE wave exchange data through LDS: order the accesses for the compiler (the hardware runs a wave's LDS
// instructions in order)
__device__ __forceinline__ void track_wave_lds_sync() {
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

__global__ __launch_bounds__(kTrackChainThreads) void k_track_chain(int64_t F, int P, int S, double gate2, int max_missed,
                                                                   const double *__restrict__ centres, unsigned char *state,
                                                                   int32_t *__restrict__ slot_of, int32_t *__restrict__ person_of,
                                                                   int32_t *__restrict__ track_id, uint32_t *__restrict__ flags) {
    constexpr int B = kTrackBlockFrames, M = kTrackMax;
    __shared__ double2 s_cen[2][B * M * 2];   // [frame in block][p] -> (x, y), (z, valid); row stride P
    __shared__ int32_t s_slot[2][B * M];      // row stride P
    __shared__ int32_t s_person[2][B * M];    // row stride S
    __shared__ int32_t s_id[2][B * M];        // row stride S
    __shared__ uint32_t s_flags[2][B];
    __shared__ double s_pos[M * 3];           // slot positions: wave 0 only

    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int64_t nb = (F + B - 1) / B;

    // frames of block b
    auto block_frames = [&](int64_t b) { return (int)((F - b * B) < (int64_t)B ? (F - b * B) : (int64_t)B); };
    // waves 1..3: centres of block b -> arena half `buf`
    auto stage = [&](int64_t b, int buf) {
        const int n = block_frames(b) * P * 2;
        SNOWTRI_DEV_CHECK(b >= 0 && b < nb && n > 0 && n <= B * M * 2, 71);
        const double2 *src = reinterpret_cast<const double2 *>(centres) + (size_t)b * B * P * 2;
        for (int i = tid - 64; i < n; i += kTrackStagers) s_cen[buf][i] = src[i];
    };
    // waves 1..3: results of block b, held in output half `buf`, -> HBM
    auto write_out = [&](int64_t b, int buf) {
        const int nf = block_frames(b);
        const int64_t f0 = b * B;
        SNOWTRI_DEV_CHECK(b >= 0 && b < nb && nf > 0 && nf <= B && f0 + nf <= F, 72);
        for (int i = tid - 64; i < nf * P; i += kTrackStagers) slot_of[f0 * P + i] = s_slot[buf][i];
        for (int i = tid - 64; i < nf * S; i += kTrackStagers) {
            person_of[f0 * S + i] = s_person[buf][i];
            track_id[f0 * S + i] = s_id[buf][i];
        }
        if (flags)
            for (int i = tid - 64; i < nf; i += kTrackStagers) flags[f0 + i] = s_flags[buf][i];
    };

    // walking-wave state: lane s < S holds its slot's (live, missed, id); next_id in every lane
    int live = 0, missed = 0, id = 0, next_id = 0;
    const int p = lane & 15, sgrp = lane >> 4;   // this lane's person, and its four slots 4 * sgrp + k
    if (wave == 0) {
        if (lane < M * 3) s_pos[lane] = 0.0;
        if (state) {
            next_id = *reinterpret_cast<const int32_t *>(state);
            if (lane < S) {
                const double *sp = reinterpret_cast<const double *>(state + kTrackStateHeader) + 3 * lane;
                const int32_t *sm = reinterpret_cast<const int32_t *>(state + kTrackStateHeader + 24 * (size_t)S) + 4 * lane;
                s_pos[3 * lane + 0] = sp[0], s_pos[3 * lane + 1] = sp[1], s_pos[3 * lane + 2] = sp[2];
                live = sm[0] != 0, missed = sm[1], id = sm[2];
            }
        }
        track_wave_lds_sync();
    } else
        stage(0, 0);
    __syncthreads();

    for (int64_t b = 0; b < nb; ++b) {
        const int buf = (int)(b & 1);
        if (wave != 0) {
            if (b + 1 < nb) stage(b + 1, buf ^ 1);
            if (b > 0) write_out(b - 1, buf ^ 1);
        } else {
            const int nf = block_frames(b);
            for (int fi = 0; fi < nf; ++fi) {
                // 1. this lane's person and the masks everybody needs
                SNOWTRI_DEV_CHECK(fi >= 0 && fi < B && (fi * P + P) * 2 <= B * M * 2, 73);
                double cx = 0.0, cy = 0.0, cz = 0.0;
                bool pvalid = false;
                if (p < P) {
                    const double2 a = s_cen[buf][(fi * P + p) * 2], c = s_cen[buf][(fi * P + p) * 2 + 1];
                    cx = a.x, cy = a.y, cz = c.x, pvalid = c.y != 0.0;
                }
                const unsigned int live_mask = (unsigned int)__ballot(lane < S && live != 0) & 0xffffu;    // over s: live at the start
                const unsigned int valid_mask = (unsigned int)__ballot(lane < M && pvalid) & 0xffffu;      // over p
                // 2. distances of this lane's four pairs; ~0 = no candidate (d2 is finite and >= 0 where it counts)
                unsigned long long key[4];
#pragma unroll
                for (int k = 0; k < 4; ++k) {
                    const int s = 4 * sgrp + k;
                    key[k] = ~0ull;
                    if (pvalid && ((live_mask >> s) & 1u)) {
                        SNOWTRI_DEV_CHECK(s >= 0 && s < S, 74);
                        const double d2 = track_d2(cx, cy, cz, s_pos[3 * s], s_pos[3 * s + 1], s_pos[3 * s + 2]);
                        if (d2 <= gate2) key[k] = (unsigned long long)__double_as_longlong(d2);
                    }
                }
                // 3. greedy rounds
                unsigned int slot_taken = 0u, person_taken = 0u;
                int my_person = -1, my_slot = -1;   // lane s: person_of[s]; lane p: slot_of[p]
                for (int round = 0; round < M; ++round) {
                    unsigned long long lmin = ~0ull;
                    const bool pfree = !((person_taken >> p) & 1u);
#pragma unroll
                    for (int k = 0; k < 4; ++k) {
                        const bool avail = pfree && !((slot_taken >> (4 * sgrp + k)) & 1u);
                        lmin = (avail && key[k] < lmin) ? key[k] : lmin;
                    }
                    const unsigned long long wmin = track_wave_min(lmin);
                    if (wmin == ~0ull) break;
                    // ties: lowest s = 4 * sgrp + k, then lowest p -- the first set bit of (k-major, p-minor) words, sgrp by sgrp
                    unsigned long long m[4];
#pragma unroll
                    for (int k = 0; k < 4; ++k)
                        m[k] = __ballot(pfree && !((slot_taken >> (4 * sgrp + k)) & 1u) && key[k] == wmin);
                    int ws = -1, wp = -1;
#pragma unroll
                    for (int g = 3; g >= 0; --g) {
                        const unsigned long long w = ((m[0] >> (16 * g)) & 0xffffull) | (((m[1] >> (16 * g)) & 0xffffull) << 16) |
                                                     (((m[2] >> (16 * g)) & 0xffffull) << 32) | (((m[3] >> (16 * g)) & 0xffffull) << 48);
                        if (w) {
                            const int idx = __ffsll((long long)w) - 1;
                            ws = 4 * g + (idx >> 4), wp = idx & 15;
                        }
                    }
                    SNOWTRI_DEV_CHECK(ws >= 0 && ws < S && wp >= 0 && wp < P, 75);
                    slot_taken |= 1u << ws;
                    person_taken |= 1u << wp;
                    if (lane == ws) my_person = wp;
                    if (lane == wp) my_slot = ws;
                }
                // 4. births: the r-th unassigned valid person takes the r-th slot that was not live at the start
                const unsigned int born_p = valid_mask & ~person_taken;
                const unsigned int free_s = ~live_mask & ((1u << S) - 1u);
                const int n_born = min(__popc(born_p), __popc(free_s));
                if (lane < M && ((born_p >> lane) & 1u)) {
                    const int r = __popc(born_p & ((1u << lane) - 1u));
                    if (r < n_born) my_slot = track_nth_bit(free_s, r);
                }
                bool matched = my_person >= 0;
                if (lane < M && ((free_s >> lane) & 1u)) {
                    const int r = __popc(free_s & ((1u << lane) - 1u));
                    if (r < n_born) {
                        my_person = track_nth_bit(born_p, r);
                        live = 1, missed = 0, id = next_id + r;
                    }
                }
                next_id += n_born;
                // 5. ageing, positions, this frame's outputs
                if (lane < S) {
                    if (matched)
                        missed = 0;
                    else if ((live_mask >> lane) & 1u) {
                        missed += 1;
                        if (missed > max_missed) live = 0;
                    }
                    SNOWTRI_DEV_CHECK(my_person >= -1 && my_person < P && fi * S + lane < B * M, 76);
                    if (my_person >= 0) {
                        const double2 a = s_cen[buf][(fi * P + my_person) * 2], c = s_cen[buf][(fi * P + my_person) * 2 + 1];
                        s_pos[3 * lane] = a.x, s_pos[3 * lane + 1] = a.y, s_pos[3 * lane + 2] = c.x;
                    }
                    s_person[buf][fi * S + lane] = my_person;
                    s_id[buf][fi * S + lane] = my_person >= 0 ? id : -1;
                }
                if (lane < P) {
                    SNOWTRI_DEV_CHECK(my_slot >= -1 && my_slot < S && fi * P + lane < B * M, 77);
                    s_slot[buf][fi * P + lane] = my_slot;
                }
                if (lane == 0) s_flags[buf][fi] = __popc(born_p) > n_born ? kTrackFlagOverflow : 0u;
                track_wave_lds_sync();   // s_pos of this frame is read by every lane in the next
            }
        }
        __syncthreads();
    }
    if (wave != 0) {
        if (nb > 0) write_out(nb - 1, (int)((nb - 1) & 1));
    } else if (state) {
        if (lane == 0) {
            int32_t *hd = reinterpret_cast<int32_t *>(state);
            hd[0] = next_id, hd[1] = 0, hd[2] = 0, hd[3] = 0;
        }
        if (lane < S) {
            double *sp = reinterpret_cast<double *>(state + kTrackStateHeader) + 3 * lane;
            int32_t *sm = reinterpret_cast<int32_t *>(state + kTrackStateHeader + 24 * (size_t)S) + 4 * lane;
            sp[0] = s_pos[3 * lane], sp[1] = s_pos[3 * lane + 1], sp[2] = s_pos[3 * lane + 2];
            sm[0] = live, sm[1] = missed, sm[2] = id, sm[3] = 0;
        }
    }
}

// One 16-byte record per lane (float32: one joint; float64: half a joint), bits only.
__global__ __launch_bounds__(256) void k_track_gather(int64_t F, int P, int S, int rec_per_person, const uint4 *__restrict__ xyzs,
                                                      const int32_t *__restrict__ person_of, uint4 *__restrict__ out) {
    const int64_t total = F * S * (int64_t)rec_per_person;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (int64_t)gridDim.x * blockDim.x) {
        const int64_t fs = i / rec_per_person;   // f * S + s
        const int r = (int)(i - fs * rec_per_person);
        const int64_t f = fs / S;
        const int pp = person_of[fs];
        SNOWTRI_DEV_CHECK(f >= 0 && f < F && pp >= -1 && pp < P, 78);
        uint4 v = make_uint4(0u, 0u, 0u, 0u);
        if (pp >= 0 && pp < P) v = xyzs[(size_t)(f * P + pp) * rec_per_person + r];
        out[i] = v;
    }
}

}  // namespace snowtri
