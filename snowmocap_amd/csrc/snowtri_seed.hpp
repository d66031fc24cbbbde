// snowtri_seed.hpp -- seeding of 3D persons from the detections nobody claimed: the line distance of every pair of detections of two
// cameras (k_pair_cost), and the grouping of a frame's free detections into cliques of mutually close ones (k_seed_group).  No
// reference counterpart.
//
// The rule (include/snowtri.h, "Seeding"), all in fp64.  Per camera pair k = (a < b) in the reference's loop order, detection q of a
// and r of b, joint j:
//   1. h_c = M_c (u, v, 1), M_c = R_c K_c^-1 the ray matrix of the context
//   2. n = h_a x h_b, nn = n . n, w = (t_b - t_a) . n, d2 = w * w / nn     (the squared distance between the two lines)
//   3. the joint counts iff both detections count (q < n_persons, not score < threshold, finite u and v), nn > 0 and d2 is finite
//   4. pair_n = the number of counting joints, pair_sum = the sum of their d2, 0 when pair_n is 0
//   5. a pair with a claimed member or a member behind n_persons is (0, 0) and its keypoints are not read.
// The ray of a joint and the products of an item are written with explicit fma: no contraction is left to the compiler's choice.
//
// k_pair_cost: ONE WORKGROUP PER (frame, camera pair), min(4, Pmax) waves.  The rays of a detection are needed by (C - 1) Pmax items;
// here every ray of camera b is formed once per workgroup -- all threads fill an LDS tile [3][RT][kn] (x, y, z planes: consecutive
// lanes read consecutive doubles) with the rays of up to RT detections of b, a joint that does not count as the ray (NaN, NaN, NaN),
// which fails nn > 0 -- and every ray of camera a once per wave: wave w owns the detections q = w, w + waves, ... of a, lane l holds
// the rays of joints l, l + 64, l + 128, l + 192 in registers (kSeedMaxJoints = 256) and walks the r of the tile.  An item's sum is
// a lane's joints in increasing order, then a fixed xor butterfly: its order depends on kn alone, not on F, Pmax, RT or the item's
// place in the launch.  pair_n needs no butterfly: a ballot of the lanes that count and a population count.
//
// k_seed_group: ONE WAVE PER FRAME, a lane is a NODE x = c * Pmax + q (C * Pmax <= 64).  The weights W[x][y] live in LDS (N x N
// doubles, +inf where there is no admissible edge), formed by the one division of the rule; afterwards there are only comparisons.
// The free nodes are a 64-bit ballot that every lane holds; lane x scans its row for the least (W[x][y], y) over free y > x, and the
// least (weight, x, y) of the wave comes from an xor butterfly on the totally ordered tuple -- exact in any order, so the kernel's
// choice is the serial scan's.  Growing a clique: lane z keeps the LARGEST edge to the members so far (a running maximum: exact),
// +inf once any edge is missing or its camera is taken, and the butterfly picks the least (largest edge, z).
#pragma once
#include "snowtri_kernels.hpp"

namespace snowtri {

constexpr int kSeedMaxJoints = 256;     // snowtri_pair_cost: kn <= 4 joints per lane
constexpr int kSeedMaxCams = 8;         // snowtri_pair_cost: 2 to 8 cameras
constexpr int kSeedMaxWaves = 4;        // waves per workgroup of k_pair_cost, each with its own detections of camera a
constexpr int kSeedTileBytes = 32 * 1024;   // the LDS tile of camera b's rays (24 bytes per joint)
constexpr int kSeedMaxNodes = 64;       // snowtri_seed_persons: C * Pmax, the lanes of one wave
constexpr double kSeedMaxGate = 1e150;  // gate: gate * gate stays finite

__host__ __device__ inline int seed_tile_dets(int Pmax, int kn) {   // RT: detections of camera b per LDS tile
    const int fit = kSeedTileBytes / (24 * kn);
    return Pmax < fit ? Pmax : (fit < 1 ? 1 : fit);
}

__device__ __forceinline__ bool seed_finite(double a) { return fabs(a) < __builtin_huge_val(); }   // (false for NaN)

// -> whether the joint counts (rule 3, the detection's part); the ray in h
template <typename TK>
__device__ __forceinline__ bool seed_ray(const double *__restrict__ M, const Kp3<TK> d, double kthr, double &hx, double &hy, double &hz) {
    const double u = (double)d.u, v = (double)d.v;
    hx = fma(M[0], u, fma(M[1], v, M[2]));
    hy = fma(M[3], u, fma(M[4], v, M[5]));
    hz = fma(M[6], u, fma(M[7], v, M[8]));
    return !((double)d.s < kthr) && seed_finite(u) && seed_finite(v);
}

// kpts [F][C][Pmax][kn][3], n_persons [F][C] or null, claimed [F][C][Pmax] or null -> pair_sum / pair_n [F][NP][Pmax][Pmax];
// grid = F * NP, block = 64 * min(kSeedMaxWaves, Pmax), dynamic LDS = 24 * RT * kn bytes
template <typename TK>
__global__ __launch_bounds__(64 * kSeedMaxWaves) void k_pair_cost(int64_t n_wg, int C, int NP, int Pmax, int kn, int RT, double kthr, Rig rig,
                                                                   const TK *__restrict__ kpts, const int32_t *__restrict__ n_persons,
                                                                   const int32_t *__restrict__ claimed, double *__restrict__ pair_sum,
                                                                   int32_t *__restrict__ pair_n) {
    extern __shared__ double s_ray[];   // [3][RT][kn]
    constexpr int kPerLane = kSeedMaxJoints / 64;
    const int64_t wg = blockIdx.x;
    if (wg >= n_wg) return;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, waves = blockDim.x >> 6;
    const int64_t f = wg / NP;
    const int k = (int)(wg - f * NP);
    const int a = rig.pairs[2 * k], b = rig.pairs[2 * k + 1];
    SNOWTRI_DEV_CHECK(kn <= kSeedMaxJoints && RT >= 1 && RT <= Pmax && 24 * RT * kn <= kSeedTileBytes + 24 * kSeedMaxJoints && a >= 0 && a < b && b < C &&
                          NP == rig.npairs, 120);
    const int64_t fa = f * C + a, fb = f * C + b;
    const int na = n_persons ? min(n_persons[fa], Pmax) : Pmax, nb = n_persons ? min(n_persons[fb], Pmax) : Pmax;
    const Kp3<TK> *deta = reinterpret_cast<const Kp3<TK> *>(kpts) + fa * Pmax * (int64_t)kn;
    const Kp3<TK> *detb = reinterpret_cast<const Kp3<TK> *>(kpts) + fb * Pmax * (int64_t)kn;
    const int32_t *cla = claimed ? claimed + fa * Pmax : nullptr, *clb = claimed ? claimed + fb * Pmax : nullptr;
    double Ma[9], Mb[9];
#pragma unroll
    for (int i = 0; i < 9; i++) {
        Ma[i] = rig.M[9 * a + i];
        Mb[i] = rig.M[9 * b + i];
    }
    const double d0 = rig.pairc[6 * k], d1 = rig.pairc[6 * k + 1], d2c = rig.pairc[6 * k + 2];   // t_b - t_a
    const double nan = __builtin_nan("");
    double *sx = s_ray, *sy = s_ray + (size_t)RT * kn, *sz = s_ray + 2 * (size_t)RT * kn;
    double *osum = pair_sum + wg * Pmax * (int64_t)Pmax;
    int32_t *on = pair_n + wg * Pmax * (int64_t)Pmax;

    for (int r0 = 0; r0 < Pmax; r0 += RT) {
        const int rt = min(RT, Pmax - r0);
        __syncthreads();   // (the tile before this one has been read)
        for (int e = threadIdx.x; e < rt * kn; e += blockDim.x) {
            const int rl = e / kn, r = r0 + rl;
            const bool free_b = r < nb && !(clb && clb[r] >= 0);
            if (free_b) {   // (a detection that is not free is not read: its items are (0, 0) below)
                double hx, hy, hz;
                const bool ok = seed_ray(Mb, detb[(int64_t)r0 * kn + e], kthr, hx, hy, hz);
                sx[e] = ok ? hx : nan;
                sy[e] = ok ? hy : nan;
                sz[e] = ok ? hz : nan;
            }
        }
        __syncthreads();
        for (int q = wave; q < Pmax; q += waves) {   // wave-uniform
            const bool free_a = q < na && !(cla && cla[q] >= 0);
            double ax[kPerLane], ay[kPerLane], az[kPerLane];
#pragma unroll
            for (int i = 0; i < kPerLane; i++) {
                const int j = i * 64 + lane;
                ax[i] = ay[i] = az[i] = nan;
                if (free_a && j < kn) {
                    double hx, hy, hz;
                    if (seed_ray(Ma, deta[(int64_t)q * kn + j], kthr, hx, hy, hz)) {
                        ax[i] = hx;
                        ay[i] = hy;
                        az[i] = hz;
                    }
                }
            }
            for (int rl = 0; rl < rt; rl++) {
                const int r = r0 + rl;
                const bool both = free_a && r < nb && !(clb && clb[r] >= 0);   // wave-uniform
                double sum = 0.0;
                int n = 0;
                if (both) {
#pragma unroll
                    for (int i = 0; i < kPerLane; i++) {
                        const int j = i * 64 + lane;
                        bool counts = false;
                        double dd = 0.0;
                        if (j < kn) {
                            const double bx = sx[rl * kn + j], by = sy[rl * kn + j], bz = sz[rl * kn + j];
                            const double n0 = fma(ay[i], bz, -(az[i] * by));
                            const double n1 = fma(az[i], bx, -(ax[i] * bz));
                            const double n2 = fma(ax[i], by, -(ay[i] * bx));
                            const double nn = fma(n2, n2, fma(n1, n1, n0 * n0));
                            const double w = fma(d2c, n2, fma(d1, n1, d0 * n0));
                            dd = (w * w) / nn;
                            counts = nn > 0.0 && seed_finite(dd);
                        }
                        if (counts) sum += dd;
                        n += __builtin_popcountll(__ballot(counts));   // (uniform: every lane holds the wave's count)
                    }
#pragma unroll
                    for (int s = 32; s >= 1; s >>= 1) sum += __shfl_xor(sum, s, 64);   // the same pairs in the same order for every item
                }
                if (lane == 0) {
                    const int o = q * Pmax + r;
                    osum[o] = n ? sum : 0.0;
                    on[o] = n;
                }
            }
        }
    }
}

// The least (key, x, y) of the wave in every lane; a lane without a candidate passes key = +inf.
__device__ __forceinline__ void seed_wave_min(double &key, int &x, int &y) {
#pragma unroll
    for (int s = 32; s >= 1; s >>= 1) {
        const double ok = __shfl_xor(key, s, 64);
        const int ox = __shfl_xor(x, s, 64), oy = __shfl_xor(y, s, 64);
        if (ok < key || (ok == key && (ox < x || (ox == x && oy < y)))) {
            key = ok;
            x = ox;
            y = oy;
        }
    }
}

// pair_sum / pair_n [F][NP][Pmax][Pmax], n_persons [F][C] or null, claimed [F][C][Pmax] or null -> seed_det_of [F][C][S], n_seeds [F],
// flags [F] or null; grid = F, block = 64, dynamic LDS = 8 N N bytes (N = C * Pmax <= 64)
__global__ __launch_bounds__(64) void k_seed_group(int64_t F, int C, int Pmax, int S, double gate2, int min_joints, int min_views,
                                                    const int32_t *__restrict__ pairs, const double *__restrict__ pair_sum,
                                                    const int32_t *__restrict__ pair_n, const int32_t *__restrict__ n_persons,
                                                    const int32_t *__restrict__ claimed, int32_t *__restrict__ seed_det_of,
                                                    int32_t *__restrict__ n_seeds, uint32_t *__restrict__ flags) {
    extern __shared__ double s_w[];   // [N][N]
    const int64_t f = blockIdx.x;
    if (f >= F) return;
    const double inf = __builtin_huge_val();
    const int lane = threadIdx.x, N = C * Pmax, NP = C * (C - 1) / 2, PP = Pmax * Pmax;
    SNOWTRI_DEV_CHECK(N >= 2 && N <= kSeedMaxNodes && S >= 1 && S <= 64 && min_views >= 2 && min_views <= C && blockDim.x == 64, 121);
    for (int e = lane; e < N * N; e += 64) s_w[e] = inf;
    __syncthreads();
    const double *ps = pair_sum + f * NP * (int64_t)PP;
    const int32_t *pn = pair_n + f * NP * (int64_t)PP;
    for (int e = lane; e < NP * PP; e += 64) {
        const int k = e / PP, qr = e - k * PP, q = qr / Pmax, r = qr - q * Pmax;
        const int x = pairs[2 * k] * Pmax + q, y = pairs[2 * k + 1] * Pmax + r;
        const int32_t cn = pn[e];
        const double mean = ps[e] / (double)cn;   // the rule's one division
        const bool ok = cn >= min_joints && mean == mean && mean <= gate2;
        if (ok) {
            s_w[x * N + y] = mean;
            s_w[y * N + x] = mean;
        }
    }
    __syncthreads();
    const bool node = lane < N;
    const int myc = node ? lane / Pmax : 0, myq = node ? lane - myc * Pmax : 0;
    bool is_free = false;
    if (node) {
        const int nq = n_persons ? n_persons[f * C + myc] : Pmax;
        is_free = myq < nq && !(claimed && claimed[(f * C + myc) * (int64_t)Pmax + myq] >= 0);
    }
    unsigned long long freemask = __ballot(is_free);
    const double *row = s_w + (node ? lane : 0) * N;
    int my_seed = -1, ns = 0;
    bool full = false;
    for (;;) {   // (every turn removes an edge or at least two free nodes)
        // the least edge between two free nodes, ties to the lowest (x, y)
        double key = inf;
        int kx = 64, ky = 64;
        if (node && ((freemask >> lane) & 1ull)) {
            for (int y = lane + 1; y < N; y++) {
                const double w = row[y];
                if (((freemask >> y) & 1ull) && w < key) {   // strict: the lowest y of equal weights
                    key = w;
                    ky = y;
                }
            }
            if (key < inf) kx = lane;
        }
        seed_wave_min(key, kx, ky);
        if (!(key < inf)) break;
        if (ns >= S) {
            full = true;
            break;
        }
        const int x0 = kx, y0 = ky;
        unsigned long long members = (1ull << x0) | (1ull << y0), cams = (1ull << (x0 / Pmax)) | (1ull << (y0 / Pmax));
        int size = 2;
        double worst = inf;   // my largest edge to a member; +inf: no candidate
        if (node && ((freemask >> lane) & 1ull) && !((members >> lane) & 1ull)) {
            const double wa = row[x0], wb = row[y0];
            worst = wa > wb ? wa : wb;   // (+inf wins: a missing edge)
        }
        for (;;) {
            double zk = ((cams >> myc) & 1ull) || ((members >> lane) & 1ull) || !node ? inf : worst;
            int zx = zk < inf ? lane : 64, zy = 0;
            seed_wave_min(zk, zx, zy);
            if (!(zk < inf)) break;
            members |= 1ull << zx;
            cams |= 1ull << (zx / Pmax);
            size++;
            if (node && worst < inf) {
                const double wz = row[zx];
                worst = wz > worst ? wz : worst;
            }
        }
        if (size < min_views) {
            __syncthreads();   // (every lane has read its row)
            if (lane == 0) {
                s_w[x0 * N + y0] = inf;
                s_w[y0 * N + x0] = inf;
            }
            __syncthreads();
        } else {
            if ((members >> lane) & 1ull) my_seed = ns;
            freemask &= ~members;
            ns++;
        }
    }
    for (int s = 0; s < S; s++) {   // slots at or behind n_seeds hold -1
        const unsigned long long m = __ballot(my_seed == s);
        if (lane < C) {
            const unsigned long long sub = (m >> (lane * Pmax)) & (Pmax >= 64 ? ~0ull : ((1ull << Pmax) - 1ull));
            seed_det_of[(f * C + lane) * (int64_t)S + s] = sub ? (int32_t)__builtin_ctzll(sub) : -1;
        }
    }
    if (lane == 0) {
        n_seeds[f] = ns;
        if (flags) flags[f] = full ? 1u : 0u;
    }
}

}  // namespace snowtri
