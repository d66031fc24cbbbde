// snowtri_robust.hpp -- k_dlt_robust: method = SNOWTRI_DLT_ROBUST, the N-view DLT of one detection per camera with a
// leave-one-out gate on the reprojection residual (include/snowtri.h states the rule; snowmocap_amd/robust.py is the rule
// in NumPy and what the tests compare with).
//
// One lane per (frame, joint < keypoint_num).  A lane keeps its C observations in registers, solves the DLT over the views
// that pass the keypoint gate -- dlt_add_observation / dlt_solve / dlt_recip of snowtri_fused.hpp, unchanged -- and reprojects
// the point into those views: m = the largest squared pixel residual.  That is all a clean joint pays.  A wave enters the
// leave-one-out round only while one of its lanes still has m > tau^2, three or more views and a drop left (__any): the loop
// over the candidate camera is then wave-uniform, a candidate's subset is a bit mask (the rows of A^T A are re-accumulated
// from the registers with weights 0 / 1), and lanes that do not try the candidate run the solve with `live` = false.  Every
// select is per lane, so a settled lane keeps its answer whatever its wave-mates still do (the discipline of
// dlt_inverse_iteration); the wave votes inside dlt_solve only decide how long the wave goes on.  That item is robust_item below,
// which k_dlt_matched (snowtri_matched.hpp) calls on other observations.
//
// Frame: k_fused_single's -- a workgroup owns a tile of T frames, the joint scores go through an LDS stash, one barrier, then
// the frames' mean scores (person score), count = 1, flags = FASTPATH as the DLT kernels write them.  A tile is one
// workgroup (no persistent loop): nothing outlives a tile.  Results do not depend on T: an item never looks at its
// neighbours, and a frame's mean is summed in an order fixed by keypoint_num alone.
#pragma once
#include "snowtri_fused.hpp"

namespace snowtri {

constexpr int kRobustWaves = 2;       // waves per SIMD the kernel is compiled for (256 VGPRs: the observations stay beside dlt_solve)
constexpr int kRobustMaxCams = 8;
constexpr int kRobustMaxDrops = 6;    // at most C - 2 views can go
constexpr int kRobustMaxTile = 16;    // frames per workgroup

// [P[C][12] + the rig frame | stash [T][kn] fp64 | detection mask per frame]
__host__ __device__ constexpr size_t robust_lds_bytes(int C, int T, int kn) {
    return (((size_t)96 * C + 8 * kDltFrame + (size_t)8 * T * kn + (size_t)4 * T) + 15) & ~(size_t)15;
}

// The item both robust kernels run (k_dlt_robust here, k_dlt_matched in snowtri_matched.hpp): rules 2 and 3 on a lane's C observations.
// In: S = the start set (0 for a lane past the end), cnt = |S|, ok = cnt >= 2, Pl = P[C][12] in LDS.  Out: S and cnt of the final set,
// (x, y, z) = its point in the rig's frame, sum = the total of its squared pixel residuals.  The wave must enter with every lane.
template <int C, typename TIn>
__device__ __forceinline__ void robust_item(const Kp3<TIn> (&obs)[C], const double *Pl, double tau2, int max_drops, bool ok, uint32_t &S, int &cnt,
                                            double &x, double &y, double &z, double &sum) {
#pragma clang fp contract(off)   // comparisons decide here: no result may depend on which inlined copy computed it (see dlt_item)
    // solve(Tm): X = the DLT point of the views in Tm, m = max, sum = total of their squared pixel residuals (m is NaN if one is)
    auto solve = [&](uint32_t Tm, bool act, double &x, double &y, double &z, double &m, double &sum) {
#pragma clang fp contract(off)
        double A[4][4];
        asm volatile("" ::: "memory");   // (P is read from LDS where a camera's rows are formed: hoisted it is 12 C doubles)
#pragma unroll
        for (int c = 0; c < C; c++) {
            __builtin_amdgcn_sched_barrier(0);   // a camera's twelve LDS reads stay with its observation (register budget)
            const double w = ((Tm >> c) & 1u) ? 1.0 : 0.0;
            if (c == 0)
                dlt_add_observation<true, true>(A, Pl + 12 * c, (double)obs[c].u, (double)obs[c].v, w);
            else
                dlt_add_observation<true, false>(A, Pl + 12 * c, (double)obs[c].u, (double)obs[c].v, w);
        }
        double e[4];
        dlt_solve(A, act, e);
        const double r = dlt_recip(e[3]);
        x = e[0] * r;
        y = e[1] * r;
        z = e[2] * r;
        m = 0.0;
        sum = 0.0;
        bool isnan_ = false;
        asm volatile("" ::: "memory");
#pragma unroll
        for (int c = 0; c < C; c++) {
            __builtin_amdgcn_sched_barrier(0);
            const double *P = Pl + 12 * c;
            const double p0 = fma(P[0], x, fma(P[1], y, fma(P[2], z, P[3])));
            const double p1 = fma(P[4], x, fma(P[5], y, fma(P[6], z, P[7])));
            const double p2 = fma(P[8], x, fma(P[9], y, fma(P[10], z, P[11])));
            const double ip = dlt_recip(p2);
            const double du = p0 * ip - (double)obs[c].u, dv = p1 * ip - (double)obs[c].v;
            const double r2 = du * du + dv * dv;
            const bool in = (Tm >> c) & 1u;
            const double r2c = in ? r2 : 0.0;
            isnan_ = isnan_ || (in && r2 != r2);
            m = r2c > m ? r2c : m;
            sum += r2c;
        }
        m = isnan_ ? __builtin_nan("") : m;
    };

    double m;
    solve(S, ok, x, y, z, m, sum);
    int d = 0;
    bool need = ok && cnt >= 3 && d < max_drops && m > tau2;
    while (__any(need)) {
        // leave-one-out: the subset whose worst residual is smallest wins; ties go to the lowest camera, a NaN never beats a number
        double bx = x, by = y, bz = z, bm = m, bsum = sum;
        int bc = -1;
#pragma unroll 1
        for (int c = 0; c < C; c++) {
            const bool cand = need && ((S >> c) & 1u);
            if (!__any(cand)) continue;
            double cx, cy, cz, cm, csum;
            solve(cand ? (S & ~(1u << c)) : 0u, cand, cx, cy, cz, cm, csum);
            const bool win = cand && (bc < 0 || cm < bm || (bm != bm && cm == cm));
            bx = win ? cx : bx;
            by = win ? cy : by;
            bz = win ? cz : bz;
            bm = win ? cm : bm;
            bsum = win ? csum : bsum;
            bc = win ? c : bc;
        }
        SNOWTRI_DEV_CHECK(!need || (bc >= 0 && bc < C && ((S >> bc) & 1u)), 62);
        // a lane that is not in the round keeps what it has
        S = need ? (S & ~(1u << (bc & 7))) : S;
        x = need ? bx : x;
        y = need ? by : y;
        z = need ? bz : z;
        m = need ? bm : m;
        sum = need ? bsum : sum;
        cnt -= need ? 1 : 0;
        d += need ? 1 : 0;
        need = need && cnt >= 3 && d < max_drops && m > tau2;
    }
}

template <int C, typename TIn, typename TOut>
__global__ __launch_bounds__(kBlock, kRobustWaves) void k_dlt_robust(int64_t F, int J, int T, Rig rig, const TIn *__restrict__ kpts,
                                                                    const int32_t *__restrict__ n_persons, Params prm, double tau2,
                                                                    int max_drops, int Pout, TOut *__restrict__ out4,
                                                                    TOut *__restrict__ out_ps, int32_t *__restrict__ out_count,
                                                                    uint32_t *__restrict__ out_flags, uint32_t *__restrict__ out_views,
                                                                    TOut *__restrict__ out_resid) {
#pragma clang fp contract(off)   // comparisons decide here: no result may depend on which inlined copy computed it (see dlt_item)
    static_assert(C >= 2 && C <= kRobustMaxCams, "k_dlt_robust: two to eight cameras");
    extern __shared__ __attribute__((aligned(16))) char smem[];
    const int kn = prm.kn;
    double *Pl = reinterpret_cast<double *>(smem);                           // [C][12] rig frame -> pixel matrices, then the frame
    double *stash = Pl + 12 * C + kDltFrame;                                 // [T][kn] joint scores
    uint32_t *fmask = reinterpret_cast<uint32_t *>(stash + (size_t)T * kn);  // [T] bit c: camera c lists a detection
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int64_t f0 = (int64_t)blockIdx.x * T;
    const int nf = (int)((F - f0) < T ? (F - f0) : T);
    SNOWTRI_DEV_CHECK(f0 >= 0 && f0 < F && nf >= 1 && nf <= T && T <= kRobustMaxTile && kn >= 0 && kn <= J, 60);
    if (tid < 12 * C + kDltFrame) Pl[tid] = rig.P[tid];
    if (tid < nf) {
        uint32_t m = (1u << C) - 1u;
        if (n_persons) {
            m = 0u;
            for (int c = 0; c < C; c++) m |= n_persons[(f0 + tid) * C + c] > 0 ? (1u << c) : 0u;
        }
        fmask[tid] = m;
    }
    __syncthreads();

    const Kp3<TIn> *kp3 = reinterpret_cast<const Kp3<TIn> *>(kpts);
    const int nitems = nf * kn;
    // passes of 64 items per wave: the bound is wave-uniform (the wave votes below need every lane of the wave)
    for (int base = wave * 64; base < nitems; base += kBlock) {
        const int i = base + lane;
        const bool live = i < nitems;
        const int ic = live ? i : nitems - 1;   // lanes past the end read the tile's last item and store nothing
        const int fl = ic / kn, j = ic - fl * kn;
        SNOWTRI_DEV_CHECK(fl >= 0 && fl < nf && j >= 0 && j < kn && f0 + fl < F, 61);
        Kp3<TIn> obs[C];
        {
            const Kp3<TIn> *p = kp3 + ((f0 + fl) * C) * (int64_t)J + j;
#pragma unroll
            for (int c = 0; c < C; c++) obs[c] = p[(size_t)c * J];
        }
        uint32_t S = 0u;
        {
            const uint32_t npmask = fmask[fl];
#pragma unroll
            for (int c = 0; c < C; c++) S |= (!((double)obs[c].s < prm.kthr) && ((npmask >> c) & 1u)) ? (1u << c) : 0u;
        }
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
            const int64_t f = f0 + fl;
            Vec4T<TOut> *o = reinterpret_cast<Vec4T<TOut> *>(out4) + (f * Pout) * (int64_t)kn + j;
            // (x, y, z) is in the rig's frame, where the residuals were taken (P maps that frame to pixels): the world point is written
            *o = Vec4T<TOut>{(TOut)(ok ? dlt_to_world(x, Pl + 12 * C, 0) : 0.0), (TOut)(ok ? dlt_to_world(y, Pl + 12 * C, 1) : 0.0),
                             (TOut)(ok ? dlt_to_world(z, Pl + 12 * C, 2) : 0.0), (TOut)os};
            SNOWTRI_DEV_CHECK(fl * kn + j < T * kn, 63);
            stash[fl * kn + j] = os;
            if (out_views) out_views[f * kn + j] = ok ? S : 0u;
            if (out_resid) out_resid[f * kn + j] = (TOut)(ok ? sqrt(sum * rc) : 0.0);
        }
    }
    // unused person slots
    if (Pout > 1 && !prm.no_zero_fill) {
        Vec4T<TOut> *tile_out = reinterpret_cast<Vec4T<TOut> *>(out4) + f0 * Pout * (int64_t)kn;
        const int per = (Pout - 1) * kn;
        for (int64_t i = tid; i < (int64_t)nf * per; i += kBlock) {
            const int64_t w = i / per, r = i - w * per;
            tile_out[w * Pout * kn + kn + r] = Vec4T<TOut>{(TOut)0, (TOut)0, (TOut)0, (TOut)0};
        }
    }
    __syncthreads();   // the tile's joint scores are in the stash
    // ---- per frame: person score = mean of the keypoint_num joint scores, count = 1.  Eight lanes per frame, 32 frames per pass.
    {
        constexpr int G = 8;
        const int sub = tid & (G - 1);
        for (int base = 0; base < nf; base += kBlock / G) {
            const int w = base + tid / G;
            const bool live = w < nf;
            double sum = 0.0;
            if (live) {
                const double *row = stash + w * kn;
                for (int b = sub; b < kn; b += G) sum += row[b];
            }
#pragma unroll
            for (int off = G / 2; off > 0; off >>= 1) sum += __shfl_xor(sum, off, 64);
            if (live && sub == 0) {
                const int64_t f = f0 + w;
                out_count[f] = 1;
                if (out_ps) {
                    out_ps[f * Pout] = (TOut)(sum / (double)kn);
                    if (!prm.no_zero_fill)
                        for (int slot = 1; slot < Pout; slot++) out_ps[f * Pout + slot] = (TOut)0;
                }
                if (out_flags) out_flags[f] = kFlagFast;
            }
        }
    }
}

}  // namespace snowtri
