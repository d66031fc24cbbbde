// snowtri_pose_intr.hpp -- camera refinement with intrinsics: the pose kernels of snowtri_pose.hpp widened from six to ten
// parameters per camera, omega[3], tau[3], fx, fy, cx, cy (include/snowtri.h, "Camera pose refinement", INTRINSICS, states the rule;
// snowmocap_amd/pose.py::refine_cameras_reference(intrinsics=...) is the rule in NumPy).  Sibling kernels behind
// snowtri_refine_cameras_k: k_pose_normal / k_pose_step and their workspace are not touched, so the entries without intrinsics keep
// their instructions, registers and bits.  Shared with them: pose_record, refine_observation, refine_admits (the observation set is
// rule 1 at the INPUT pose and the INPUT K), pose_rotate, the trial table's layout (q[12..16] = fx, s, cx, fy, cy).
//
// k_pose_normal_k: k_pose_normal's grid, walk, butterfly, LDS fold and vector store, with a partial of kPoseKPartial = 72 doubles:
// E | g[10] | H[55] (the lower triangle of the 10 x 10 matrix row by row) | n | invalid | linear-regime count | padding.  The six
// pose columns of the Jacobian, E, and the 28 sums they make are pose_add_obs' operation for operation, so those sums have
// k_pose_normal's bits.  The four new columns are (x, 0), (0, y), (1, 0), (0, 1): their products are formed from w x, w y and w, the
// four entries of H that are structurally zero (fx.fy, fx.cy, fy.cx, cx.cy) are neither summed nor reduced -- the block stores 0.0 --
// and cy.cy is stored from cx.cx, both being sum w: a lane carries 61 sums and three counts.
//
// k_pose_step_k: one workgroup of 1024 lanes.  A camera's partials are added in k_pose_step's order -- 32 runs of consecutive
// blocks, each in block order, then the runs in order -- in three passes of 32 slots, so a sum's bits depend on (F, P, kn, C) alone
// and the pose sums stay k_pose_step's.  Then lane c takes camera c's decision: the free set (pose if in free_mask; focal and / or
// centre if in intr_mask), the LDL^T over exactly those rows and columns (one instantiation per free set, every index static), the
// accept test (every observation valid, fx and fy finite and > 0, E strictly lower), the next trial pose and intrinsics; behind the
// last evaluation the outputs, K_out among them.  Contraction is off in the whole kernel.
//
// Every result is written with ordinary vector stores; no floating-point atomics anywhere.
#pragma once
#include "snowtri_pose.hpp"

namespace snowtri {

constexpr int kPoseKParams = 10;
constexpr int kPoseKNormal = 66;         // E, g[10], H[55]
constexpr int kPoseKPartial = 72;        // ... n, invalid, linear-regime count (HUBER; else 0), padding
constexpr int kPoseKStateStride = 80;    // per camera: normal[66] at the current parameters, E at the input, n, code, linear-regime count
constexpr uint32_t kIntrFocal = 1u, kIntrCentre = 2u;   // SNOWTRI_INTR_FOCAL, SNOWTRI_INTR_CENTRE

__host__ __device__ constexpr int pose_k_h(int a, int b) { return 11 + a * (a + 1) / 2 + b; }   // H[a][b], b <= a, in a partial
// fx.fy, cx.fy, cy.fx, cy.cx: zero whatever the data is
__host__ __device__ constexpr bool pose_k_zero_slot(int k) {
    return k == pose_k_h(7, 6) || k == pose_k_h(8, 7) || k == pose_k_h(9, 6) || k == pose_k_h(9, 8);
}
constexpr int kPoseKDupSlot = pose_k_h(9, 9), kPoseKDupOf = pose_k_h(8, 8);   // cy.cy = cx.cx = sum w

// the intrinsics workspace, in doubles: trial [C][kProjStride] | cur [C][kProjStride] | state [C][kPoseKStateStride] |
// active [32] int32 (16 doubles) | K [C][9], the context's (uploaded when the workspace is made) | partials [kPoseGridCap][C][kPoseKPartial]
__host__ __device__ inline size_t pose_kws_trial(int C) { return 0; }
__host__ __device__ inline size_t pose_kws_cur(int C) { return (size_t)C * kProjStride; }
__host__ __device__ inline size_t pose_kws_state(int C) { return (size_t)2 * C * kProjStride; }
__host__ __device__ inline size_t pose_kws_active(int C) { return pose_kws_state(C) + (size_t)C * kPoseKStateStride; }
__host__ __device__ inline size_t pose_kws_K(int C) { return pose_kws_active(C) + 16; }
__host__ __device__ inline size_t pose_kws_partials(int C) { return pose_kws_K(C) + (((size_t)C * 9 + 1) & ~(size_t)1); }
__host__ __device__ inline size_t pose_kws_doubles(int C) { return pose_kws_partials(C) + (size_t)kPoseGridCap * C * kPoseKPartial; }

// pose_add_obs over ten parameters: acc is a partial's first 66 slots (the structurally zero ones and cy.cy are never touched).
// Everything up to and including the 6 x 6 block is pose_add_obs' own text.
template <bool HUBER>
__device__ __forceinline__ bool pose_add_obs_k(double (&acc)[kPoseKNormal], const double *__restrict__ q, double ou, double ov, double w, double X,
                                               double Y, double Z, const HuberConst &hc, bool &lin) {
#pragma clang fp contract(off)
    const double fx = q[12], sk = q[13], fy = q[15];
    const double d0 = X - q[9], d1 = Y - q[10], d2 = Z - q[11];
    const double pc0 = (q[0] * d0 + q[3] * d1) + q[6] * d2;
    const double pc1 = (q[1] * d0 + q[4] * d1) + q[7] * d2;
    const double pc2 = (q[2] * d0 + q[5] * d1) + q[8] * d2;
    const double x = pc0 / pc2, y = pc1 / pc2;
    const double u = (fx * x + sk * y) + q[14], v = fy * y + q[16];
    const bool valid = pc2 > 0.0 && finite_f64(u) && finite_f64(v);
    const double ru = u - ou, rv = v - ov;
    if constexpr (HUBER) {
        double rho, kappa;
        lin = huber_terms(hc, ru * ru + rv * rv, rho, kappa);
        acc[0] = acc[0] + w * rho;
        w = w * kappa;   // the IRLS weight
    } else {
        lin = false;
        acc[0] = acc[0] + w * (ru * ru + rv * rv);
    }
    // H and g only steer: fused multiply-adds from here on
    const double iz = 1.0 / pc2;
    double du[6], dv[6];
#pragma unroll
    for (int k = 0; k < 6; k++) {
        double a0, a1, a2;   // column k of dpc / ddelta
        if (k == 0) {
            a0 = fma(q[3], d2, -(q[6] * d1)); a1 = fma(q[4], d2, -(q[7] * d1)); a2 = fma(q[5], d2, -(q[8] * d1));
        } else if (k == 1) {
            a0 = fma(q[6], d0, -(q[0] * d2)); a1 = fma(q[7], d0, -(q[1] * d2)); a2 = fma(q[8], d0, -(q[2] * d2));
        } else if (k == 2) {
            a0 = fma(q[0], d1, -(q[3] * d0)); a1 = fma(q[1], d1, -(q[4] * d0)); a2 = fma(q[2], d1, -(q[5] * d0));
        } else {
            a0 = -q[3 * (k - 3)]; a1 = -q[3 * (k - 3) + 1]; a2 = -q[3 * (k - 3) + 2];
        }
        const double dx = fma(-x, a2, a0) * iz, dy = fma(-y, a2, a1) * iz;
        du[k] = fma(fx, dx, sk * dy);
        dv[k] = fy * dy;
    }
#pragma unroll
    for (int a = 0; a < 6; a++) {
        const double wu = w * du[a], wv = w * dv[a];
        acc[1 + a] = fma(wu, ru, fma(wv, rv, acc[1 + a]));
#pragma unroll
        for (int b = 0; b <= a; b++) acc[pose_k_h(a, b)] = fma(wu, du[b], fma(wv, dv[b], acc[pose_k_h(a, b)]));
    }
    // the intrinsics: (du, dv) / d(fx, fy, cx, cy) = (x, 0), (0, y), (1, 0), (0, 1)
    const double wx = w * x, wy = w * y;
    acc[7] = fma(wx, ru, acc[7]);
    acc[8] = fma(wy, rv, acc[8]);
    acc[9] = fma(w, ru, acc[9]);
    acc[10] = fma(w, rv, acc[10]);
#pragma unroll
    for (int b = 0; b < 6; b++) {
        acc[pose_k_h(6, b)] = fma(wx, du[b], acc[pose_k_h(6, b)]);
        acc[pose_k_h(7, b)] = fma(wy, dv[b], acc[pose_k_h(7, b)]);
        acc[pose_k_h(8, b)] = fma(w, du[b], acc[pose_k_h(8, b)]);
        acc[pose_k_h(9, b)] = fma(w, dv[b], acc[pose_k_h(9, b)]);
    }
    acc[pose_k_h(6, 6)] = fma(wx, x, acc[pose_k_h(6, 6)]);
    acc[pose_k_h(7, 7)] = fma(wy, y, acc[pose_k_h(7, 7)]);
    acc[pose_k_h(8, 6)] = acc[pose_k_h(8, 6)] + wx;
    acc[pose_k_h(9, 7)] = acc[pose_k_h(9, 7)] + wy;
    acc[pose_k_h(8, 8)] = acc[pose_k_h(8, 8)] + w;
    return valid;
}

// k_pose_normal's arguments -> partials [G][C][kPoseKPartial]
template <typename TX, typename TK, bool HUBER = false>
__global__ __launch_bounds__(kPoseBlock) void k_pose_normal_k(int64_t n_rec, int C, int P, int Pmax, int kn, double kthr, uint32_t flags,
                                                              const double *__restrict__ base, const double *__restrict__ trial,
                                                              const int32_t *__restrict__ active, const TX *__restrict__ xyzs,
                                                              const TK *__restrict__ kpts, const int32_t *__restrict__ n_persons,
                                                              const int32_t *__restrict__ det_of, const uint32_t *__restrict__ views,
                                                              double *__restrict__ partials, HuberConst hc) {
    const int c = blockIdx.y;
    SNOWTRI_DEV_CHECK(!HUBER || (hc.d > 0.0 && hc.dd > 0.0 && finite_f64(hc.dd)), 109);
    SNOWTRI_DEV_CHECK(c >= 0 && c < C && (int)gridDim.y == C && C <= kRefineMaxCams && (int)gridDim.x <= kPoseGridCap && Pmax >= 1 &&
                          (det_of || P <= Pmax), 108);
    if (active && !active[c]) return;   // (block-uniform: nobody waits at the barrier below)
    const double *__restrict__ q0 = base + (size_t)c * kProjStride;
    const double *__restrict__ q = trial + (size_t)c * kProjStride;
    const bool score_w = (flags & kRefineScoreWeights) != 0;
    double acc[kPoseKNormal];
#pragma unroll
    for (int k = 0; k < kPoseKNormal; k++) acc[k] = 0.0;
    double n_in = 0.0, n_bad = 0.0;
    [[maybe_unused]] double n_lin = 0.0;
    constexpr int kSums = HUBER ? kPoseKNormal + 3 : kPoseKNormal + 2;   // acc, n_in, n_bad and, with the loss, n_lin
    for (int64_t i = blockIdx.x * (int64_t)kPoseBlock + threadIdx.x; i < n_rec; i += (int64_t)gridDim.x * kPoseBlock) {
        int64_t f;
        int p, j;
        double X, Y, Z, ou, ov, os;
        const bool measured = pose_record(xyzs, i, n_rec, P, kn, f, p, j, X, Y, Z);
        const uint32_t allowed = views ? views[i] : 0xffffffffu;
        const bool listed = refine_observation(kpts, n_persons, det_of, f, c, C, P, Pmax, kn, p, j, ou, ov, os);
        if (refine_admits(q0, measured, listed, ou, ov, os, kthr, allowed, c, X, Y, Z)) {   // rule 1, at the input pose and the input K
            bool lin;
            const bool valid = pose_add_obs_k<HUBER>(acc, q, ou, ov, score_w ? os : 1.0, X, Y, Z, hc, lin);
            n_in += 1.0;
            n_bad += valid ? 0.0 : 1.0;
            if constexpr (HUBER) n_lin += lin ? 1.0 : 0.0;
        }
    }
    // the block's partial: a fixed butterfly over the wave, then the four waves in wave order
    __shared__ double lds[kPoseBlock / 64][kPoseKPartial];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
#pragma unroll
    for (int k = 0; k < kSums; k++) {
        if (pose_k_zero_slot(k) || k == kPoseKDupSlot) continue;   // (k is a constant once unrolled)
        double v = k < kPoseKNormal ? acc[k] : (k == kPoseKNormal ? n_in : k == kPoseKNormal + 1 ? n_bad : n_lin);
#pragma unroll
        for (int w = 32; w >= 1; w >>= 1) v += __shfl_xor(v, w, 64);
        if (lane == 0) lds[wave][k] = v;
    }
    __syncthreads();
    if (threadIdx.x < kPoseKPartial) {
        const int k = threadIdx.x, src = k == kPoseKDupSlot ? kPoseKDupOf : k;
        double v = 0.0;
        if (k < kSums && !pose_k_zero_slot(k)) v = ((lds[0][src] + lds[1][src]) + lds[2][src]) + lds[3][src];
        partials[((size_t)blockIdx.x * C + c) * kPoseKPartial + k] = v;
    }
}

// The free set m (bit 0: the pose, bit 1: fx and fy, bit 2: cx and cy): how many parameters, and the k-th of them
__host__ __device__ constexpr int pose_sub_count(int m) { return ((m & 1) ? 6 : 0) + ((m & 2) ? 2 : 0) + ((m & 4) ? 2 : 0); }
__host__ __device__ constexpr int pose_sub_index(int m, int k) {
    if (m & 1) {
        if (k < 6) return k;
        k -= 6;
    }
    if (m & 2) {
        if (k < 2) return 6 + k;
        k -= 2;
    }
    return 8 + k;
}

// pose_solve over the rows and columns of the free set M, in order: h is the lower triangle of the 10 x 10 matrix row by row.
// delta of a parameter outside the set is 0.  -> every pivot is finite and > 0.
template <int M>
__device__ __forceinline__ bool pose_solve_sub(const double *h, const double *g, double (&delta)[kPoseKParams]) {
#pragma clang fp contract(off)
    constexpr int n = pose_sub_count(M);
    double L[n][n], piv[n], y[n], d[n];
    bool pd = true;
#pragma unroll
    for (int a = 0; a < n; a++) {
#pragma unroll
        for (int b = 0; b <= a; b++) {
            const int ia = pose_sub_index(M, a), ib = pose_sub_index(M, b);
            double s = h[ia * (ia + 1) / 2 + ib];
#pragma unroll
            for (int k = 0; k < b; k++) s = s - L[a][k] * (L[b][k] * piv[k]);
            if (b < a) L[a][b] = s / piv[b];
            else piv[a] = s;
        }
        pd = pd && piv[a] > 0.0 && finite_f64(piv[a]);
    }
#pragma unroll
    for (int a = 0; a < n; a++) {
        double s = -g[pose_sub_index(M, a)];
#pragma unroll
        for (int k = 0; k < a; k++) s = s - L[a][k] * y[k];
        y[a] = s;
    }
#pragma unroll
    for (int a = n - 1; a >= 0; a--) {
        double s = y[a] / piv[a];
#pragma unroll
        for (int k = a + 1; k < n; k++) s = s - L[k][a] * d[k];
        d[a] = s;
    }
#pragma unroll
    for (int k = 0; k < kPoseKParams; k++) delta[k] = 0.0;
#pragma unroll
    for (int a = 0; a < n; a++) delta[pose_sub_index(M, a)] = d[a];
    return pd;
}

// Behind evaluation `eval` (0: at the input) of G blocks per camera: the sums, every camera's decision and next trial; with `last`
// the outputs.  ws: the intrinsics workspace (pose_kws_*), base: the input pose table.
__global__ __launch_bounds__(kPoseStepBlock) void k_pose_step_k(int C, int G, int eval, int last, uint32_t free_mask, uint32_t intr_mask,
                                                                uint32_t intr_flags, int min_obs, const double *__restrict__ base,
                                                                double *__restrict__ ws, double *__restrict__ K_out, double *__restrict__ R_out,
                                                                double *__restrict__ t_out, double *__restrict__ cost,
                                                                int64_t *__restrict__ n_obs, uint8_t *__restrict__ codes,
                                                                double *__restrict__ normal, int64_t *__restrict__ n_outliers) {
#pragma clang fp contract(off)
    __shared__ double seg_sum[kPoseSegments][32];
    __shared__ double tot[kRefineMaxCams][kPoseKPartial];
    double *trial = ws + pose_kws_trial(C), *cur = ws + pose_kws_cur(C), *state = ws + pose_kws_state(C);
    int32_t *active = reinterpret_cast<int32_t *>(ws + pose_kws_active(C));
    const double *Kin = ws + pose_kws_K(C), *partials = ws + pose_kws_partials(C);
    const int lane32 = threadIdx.x & 31, seg = threadIdx.x >> 5;
    const int Gs = (G + kPoseSegments - 1) / kPoseSegments;
    SNOWTRI_DEV_CHECK(C >= 1 && C <= kRefineMaxCams && G >= 0 && G <= kPoseGridCap && Gs <= kPoseSegments && (int)blockDim.x == kPoseSegments * 32, 110);
    for (int c = 0; c < C; c++) {
        const bool evaluated = eval == 0 || active[c] != 0;   // (block-uniform)
        if (!evaluated) continue;
        for (int pass = 0; pass < (kPoseKPartial + 31) / 32; pass++) {
            const int slot = pass * 32 + lane32;
            const bool has = slot < kPoseKPartial;
            double v[kPoseSegments];
#pragma unroll
            for (int k = 0; k < kPoseSegments; k++) {   // the loads first, all in flight; then the additions in block order
                const int b = seg * Gs + k;
                v[k] = (has && k < Gs && b < G) ? partials[((size_t)b * C + c) * kPoseKPartial + slot] : 0.0;
            }
            double s = 0.0;
#pragma unroll
            for (int k = 0; k < kPoseSegments; k++) s = s + v[k];
            seg_sum[seg][lane32] = s;
            __syncthreads();
            if (threadIdx.x < 32 && has) {
                double t_ = 0.0;
                for (int k = 0; k < kPoseSegments; k++) t_ = t_ + seg_sum[k][lane32];
                tot[c][slot] = t_;
            }
            __syncthreads();
        }
    }
    __syncthreads();   // active[] is read above by every lane and written below by lane c: every read comes first
    const int c = threadIdx.x;
    if (c >= C) return;
    const double *b_ = base + (size_t)c * kProjStride;
    double *tr = trial + (size_t)c * kProjStride, *cu = cur + (size_t)c * kProjStride, *st = state + (size_t)c * kPoseKStateStride;
    const double *sum = tot[c];
    const uint32_t intr = ((intr_mask >> c) & 1u) ? intr_flags : 0u;
    const int set = (int)((free_mask >> c) & 1u) | ((intr & kIntrFocal) ? 2 : 0) | ((intr & kIntrCentre) ? 4 : 0);   // the free set
    bool act;
    if (eval == 0) {
        for (int k = 0; k < kProjStride; k++) cu[k] = tr[k] = b_[k];
        for (int k = 0; k < kPoseKNormal; k++) st[k] = sum[k];
        if (normal)
            for (int k = 0; k < kPoseKNormal; k++) normal[(size_t)c * kPoseKNormal + k] = sum[k];
        const bool few = sum[kPoseKNormal] < (double)min_obs;
        st[66] = sum[0];
        st[67] = sum[kPoseKNormal];
        st[69] = sum[kPoseKNormal + 2];   // the observations in the linear regime at the parameters the state is of (0 under the squared loss)
        st[68] = set == 0 ? (double)kPoseFixed : few ? (double)kPoseFewObs : (double)kPoseKept;
        act = set != 0 && !few;
    } else if (active[c]) {
        const bool focal_ok = tr[12] > 0.0 && finite_f64(tr[12]) && tr[15] > 0.0 && finite_f64(tr[15]);
        const bool accept = sum[kPoseKNormal + 1] == 0.0 && focal_ok && sum[0] < st[0];
        if (accept) {
            for (int k = 0; k < 17; k++) cu[k] = tr[k];   // the pose and fx, s, cx, fy, cy (s is never changed)
            for (int k = 0; k < kPoseKNormal; k++) st[k] = sum[k];
            st[68] = (double)kPoseMoved;
            st[69] = sum[kPoseKNormal + 2];
        }
        act = accept;
    } else
        act = false;
    if (act && !last) {
        double delta[kPoseKParams];
        switch (set) {
            case 1: act = pose_solve_sub<1>(st + 11, st + 1, delta); break;
            case 2: act = pose_solve_sub<2>(st + 11, st + 1, delta); break;
            case 3: act = pose_solve_sub<3>(st + 11, st + 1, delta); break;
            case 4: act = pose_solve_sub<4>(st + 11, st + 1, delta); break;
            case 5: act = pose_solve_sub<5>(st + 11, st + 1, delta); break;
            case 6: act = pose_solve_sub<6>(st + 11, st + 1, delta); break;
            default: act = pose_solve_sub<7>(st + 11, st + 1, delta); break;
        }
        if (act) {
            if (set & 1) {
                double om[3] = {delta[0], delta[1], delta[2]}, Rn[9];
                pose_rotate(cu, om, Rn);
                for (int k = 0; k < 9; k++) tr[k] = Rn[k];
                for (int k = 0; k < 3; k++) tr[9 + k] = cu[9 + k] + delta[3 + k];
            }
            if (set & 2) {
                tr[12] = cu[12] + delta[6];
                tr[15] = cu[15] + delta[7];
            }
            if (set & 4) {
                tr[14] = cu[14] + delta[8];
                tr[16] = cu[16] + delta[9];
            }
        }
    }
    active[c] = (act && !last) ? 1 : 0;
    if (last) {
        const int code = (int)st[68];
        const bool still = code == kPoseFixed || code == kPoseFewObs;
        if (K_out) {
            for (int k = 0; k < 9; k++) K_out[(size_t)c * 9 + k] = Kin[(size_t)c * 9 + k];   // the skew and the last row: the context's bits
            if (code == kPoseMoved) {
                K_out[(size_t)c * 9] = cu[12];
                K_out[(size_t)c * 9 + 2] = cu[14];
                K_out[(size_t)c * 9 + 4] = cu[15];
                K_out[(size_t)c * 9 + 5] = cu[16];
            }
        }
        for (int k = 0; k < 9; k++) R_out[(size_t)c * 9 + k] = cu[k];
        for (int k = 0; k < 3; k++) t_out[(size_t)c * 3 + k] = cu[9 + k];
        if (cost) {
            cost[2 * c] = still ? 0.0 : st[66];
            cost[2 * c + 1] = still ? 0.0 : st[0];
        }
        if (n_obs) n_obs[c] = (int64_t)st[67];
        if (codes) codes[c] = (uint8_t)code;
        if (n_outliers) n_outliers[c] = still ? 0 : (int64_t)st[69];
    }
}

}  // namespace snowtri
