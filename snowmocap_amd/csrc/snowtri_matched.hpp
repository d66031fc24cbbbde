// snowtri_matched.hpp -- k_dlt_matched: snowtri_triangulate_matched, the robust N-view DLT of 3D person p over the detections that
// det_of names (include/snowtri.h, "Matched triangulation", states the rule; snowmocap_amd/matched.py is the rule in NumPy).
//
// The rule is DLT_ROBUST's on other observations, and so is the kernel: one lane per (frame, person, joint), the lane's C
// observations in registers, robust_item of snowtri_robust.hpp -- k_dlt_robust's own item, the same functions under the same
// fp contract(off) -- on them.  Every select is per lane and the wave votes only decide how long a wave runs, so an item's bits do
// not depend on its wave-mates: a person's record equals k_dlt_robust's on that person's gathered keypoints bit for bit.
//
// Frame: a workgroup owns a tile of T frames.  The tile's det_of / n_persons entries are resolved ONCE into LDS as "detection index
// or -1" per (frame, person, camera); a lane loads its observations through that index (lanes of consecutive j are contiguous in
// memory, as in k_dlt_robust); a camera that does not list the person gives the observation (0, 0, 0) and is outside the start set.
// The joint scores go through an LDS stash, one barrier, then the person scores: the mean of the kn joint scores, summed in
// k_dlt_robust's order, which depends on kn alone.  The records of a tile are contiguous in every output, in item order.
#pragma once
#include "snowtri_robust.hpp"

namespace snowtri {

// [P[C][12] + the rig frame | stash [T][P][kn] fp64 | detection index [T][P][C]]
__host__ __device__ constexpr size_t matched_lds_bytes(int C, int T, int P, int kn) {
    return (((size_t)96 * C + 8 * kDltFrame + (size_t)8 * T * P * kn + (size_t)4 * T * P * C) + 15) & ~(size_t)15;
}

template <int C, typename TIn, typename TOut>
__global__ __launch_bounds__(kBlock, kRobustWaves) void k_dlt_matched(int64_t F, int P, int Pmax, int kn, int T, Rig rig,
                                                                     const TIn *__restrict__ kpts, const int32_t *__restrict__ n_persons,
                                                                     const int32_t *__restrict__ det_of, double kthr, double tau2, int max_drops,
                                                                     TOut *__restrict__ out4, TOut *__restrict__ out_ps,
                                                                     uint32_t *__restrict__ out_views, TOut *__restrict__ out_resid) {
#pragma clang fp contract(off)   // comparisons decide here: no result may depend on which inlined copy computed it (see dlt_item)
    static_assert(C >= 2 && C <= kRobustMaxCams, "k_dlt_matched: two to eight cameras");
    extern __shared__ __attribute__((aligned(16))) char smem[];
    double *Pl = reinterpret_cast<double *>(smem);                            // [C][12] rig frame -> pixel matrices, then the frame
    double *stash = Pl + 12 * C + kDltFrame;                                  // [T][P][kn] joint scores
    int32_t *didx = reinterpret_cast<int32_t *>(stash + (size_t)T * P * kn);  // [T][P][C] the detection of camera c that shows the person, or -1
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int64_t f0 = (int64_t)blockIdx.x * T;
    const int nf = (int)((F - f0) < T ? (F - f0) : T);
    SNOWTRI_DEV_CHECK(f0 >= 0 && f0 < F && nf >= 1 && nf <= T && P >= 1 && Pmax >= 1 && kn >= 1 && (det_of || P <= Pmax), 64);
    if (tid < 12 * C + kDltFrame) Pl[tid] = rig.P[tid];
    // camera c lists person p in frame f iff q = det_of[f][c][p] (NULL: p) satisfies 0 <= q < min(n_persons[f][c] (NULL: Pmax), Pmax)
    for (int e = tid; e < nf * P * C; e += kBlock) {
        const int fl = e / (P * C), r = e - fl * (P * C), p = r / C, c = r - p * C;
        const int64_t fc = (f0 + fl) * C + c;
        const int32_t q = det_of ? det_of[fc * P + p] : p;
        int32_t nq = n_persons ? n_persons[fc] : Pmax;
        nq = nq > Pmax ? Pmax : nq;
        SNOWTRI_DEV_CHECK(fl < nf && p < P && c < C && e < T * P * C, 65);
        didx[e] = (q >= 0 && q < nq) ? q : -1;
    }
    __syncthreads();

    const Kp3<TIn> *kp3 = reinterpret_cast<const Kp3<TIn> *>(kpts);
    const int nrows = nf * P, nitems = nrows * kn;
    const int64_t rec0 = f0 * P * (int64_t)kn;   // the tile's first record in every per-joint output
    // passes of 64 items per wave: the bound is wave-uniform (the wave votes of robust_item need every lane of the wave)
    for (int base = wave * 64; base < nitems; base += kBlock) {
        const int i = base + lane;
        const bool live = i < nitems;
        const int ic = live ? i : nitems - 1;   // lanes past the end read the tile's last item and store nothing
        const int row = ic / kn, j = ic - row * kn, fl = row / P;
        SNOWTRI_DEV_CHECK(row >= 0 && row < nrows && j >= 0 && j < kn && fl < nf && f0 + fl < F, 66);
        Kp3<TIn> obs[C];
        uint32_t listed = 0u;
        {
            const Kp3<TIn> *fp = kp3 + ((f0 + fl) * C) * (int64_t)Pmax * kn + j;
            const int32_t *dq = didx + row * C;
#pragma unroll
            for (int c = 0; c < C; c++) {
                const int32_t q = dq[c];
                const bool in = q >= 0;
                SNOWTRI_DEV_CHECK(q >= -1 && q < Pmax, 67);
                const Kp3<TIn> o = fp[((size_t)c * Pmax + (in ? q : 0)) * kn];
                obs[c] = Kp3<TIn>{in ? o.u : (TIn)0, in ? o.v : (TIn)0, in ? o.s : (TIn)0};
                listed |= in ? (1u << c) : 0u;
            }
        }
        uint32_t S = 0u;
#pragma unroll
        for (int c = 0; c < C; c++) S |= (!((double)obs[c].s < kthr) && ((listed >> c) & 1u)) ? (1u << c) : 0u;
        S = live ? S : 0u;
        int cnt = __popc(S);
        const bool ok = cnt >= 2;

        double x, y, z, sum;
        robust_item<C, TIn>(obs, Pl, tau2, max_drops, ok, S, cnt, x, y, z, sum);

        double ssum = 0.0;
#pragma unroll
        for (int c = 0; c < C; c++) ssum += ((S >> c) & 1u) ? (double)obs[c].s : 0.0;
        const double rc = dlt_recip((double)cnt);
        const double os = ok ? ssum * rc : 0.0;
        if (live) {
            Vec4T<TOut> *o = reinterpret_cast<Vec4T<TOut> *>(out4) + rec0 + i;
            // (x, y, z) is in the rig's frame, where the residuals were taken (P maps that frame to pixels): the world point is written
            *o = Vec4T<TOut>{(TOut)(ok ? dlt_to_world(x, Pl + 12 * C, 0) : 0.0), (TOut)(ok ? dlt_to_world(y, Pl + 12 * C, 1) : 0.0),
                             (TOut)(ok ? dlt_to_world(z, Pl + 12 * C, 2) : 0.0), (TOut)os};
            SNOWTRI_DEV_CHECK(i < T * P * kn, 68);
            stash[i] = os;
            if (out_views) out_views[rec0 + i] = ok ? S : 0u;
            if (out_resid) out_resid[rec0 + i] = (TOut)(ok ? sqrt(sum * rc) : 0.0);
        }
    }
    if (!out_ps) return;   // (uniform: nobody waits at the barrier below)
    __syncthreads();       // the tile's joint scores are in the stash
    // ---- per (frame, person): person score = mean of the kn joint scores.  Eight lanes per row, 32 rows per pass (k_dlt_robust's sum).
    constexpr int G = 8;
    const int sub = tid & (G - 1);
    for (int base = 0; base < nrows; base += kBlock / G) {
        const int w = base + tid / G;
        const bool live = w < nrows;
        double sum = 0.0;
        if (live) {
            const double *row = stash + w * kn;
            for (int b = sub; b < kn; b += G) sum += row[b];
        }
#pragma unroll
        for (int off = G / 2; off > 0; off >>= 1) sum += __shfl_xor(sum, off, 64);
        if (live && sub == 0) out_ps[f0 * P + w] = (TOut)(sum / (double)kn);
    }
}

}  // namespace snowtri
