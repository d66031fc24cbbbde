// snowtri_pose.hpp -- camera pose refinement: each camera's six pose parameters moved to a local minimum of its weighted
// reprojection error with the joints held fixed (include/snowtri.h, "Camera pose refinement", states the rule;
// snowmocap_amd/pose.py is the rule in NumPy and what the tests compare with).  No reference counterpart.  The same cost as
// k_refine's (snowtri_refine.hpp), minimised over the other block of unknowns.
//
// k_pose_normal: ONE evaluation of every camera at a trial pose table, which has the layout of the context's proj table
// (kProjStride doubles per camera).  Grid (G, C), G = min(ceil(n_rec / 256), kPoseGridCap): blockIdx.y is the camera, so its
// constants -- the INPUT pose, which fixes the observation set, and the TRIAL pose, which the sums are formed at -- are
// wave-uniform scalar loads.  A lane walks the records i = (b + k G) 256 + tid.  Whether record i is an observation of the camera
// is decided by k_refine's own chain, shared with it (refine_observation + refine_admits of snowtri_refine.hpp: the per-view
// conditions, with refine_view = project_record operation for operation at the input pose), so n_obs is the rule's exactly.  The residual and E are formed in the rule's plain operations, the Jacobian, H
// and g with fused multiply-adds (they only steer).  A lane keeps E, g[6], H[21], the count and the count of observations that are
// invalid at the trial pose in registers; at the end a fixed xor butterfly over the wave, the four waves added in wave order
// through LDS, and one vector store of the block's 32-double partial.  A camera whose iteration has ended is skipped: the block
// reads its flag and returns.
//
// k_pose_step: one workgroup of 1024 lanes.  A camera's partials are added in a fixed two-level order -- segment s = the blocks
// [s Gs, (s + 1) Gs), Gs = ceil(G / 32), each in block order, then the 32 segments in order -- so a sum's bits depend on
// (F, P, kn, C) alone.  Then lane c takes camera c's decision: accept or reject the trial (rule 4), the 6 x 6 LDL^T solve,
// Exp(omega) R, the next trial pose and the camera's flag; behind the last evaluation it writes the outputs.  Contraction is off in
// the whole kernel: E(trial) < E and the pivots decide, and the solve is the NumPy rule's operation for operation.
//
// HUBER == true (include/snowtri.h, ROBUST LOSS; snowtri_refine_cameras_ex with huber_px > 0) is a second instantiation of
// k_pose_normal: the loss of snowtri_refine.hpp's huber_terms per observation -- w rho in E, the IRLS weight w kappa in H and g, kappa
// formed again in every evaluation -- and the count of the observations in the linear regime in slot 30 of the partial, which the
// squared-loss instantiation leaves 0 as before.  k_pose_step keeps that count with the state of the pose it belongs to and writes
// n_outliers behind the last evaluation.
//
// Every result is written with ordinary vector stores; no floating-point atomics anywhere.
#pragma once
#include "snowtri_refine.hpp"

namespace snowtri {

constexpr int kPoseBlock = 256;
constexpr int kPoseGridCap = 1024;       // blocks per camera: one sweep of the grid covers kPoseGridCap * 256 records
constexpr int kPosePartial = 32;         // doubles per partial: E, g[6], H[21], n, invalid, linear-regime count (HUBER; else 0), padding
constexpr int kPoseSegments = 32;        // k_pose_step adds a camera's partials in this many runs of consecutive blocks
constexpr int kPoseStepBlock = 1024;
constexpr int kPoseStateStride = 32;     // per camera: E, g[6], H[21] at the current pose, E at the input, n, code, linear-regime count
enum : uint8_t { kPoseFixed = 0, kPoseFewObs = 1, kPoseKept = 2, kPoseMoved = 3 };

// the context's workspace, in doubles: trial [C][kProjStride] | cur [C][kProjStride] | state [C][kPoseStateStride] |
// active [32] int32 (16 doubles) | partials [kPoseGridCap][C][kPosePartial]
__host__ __device__ inline size_t pose_ws_trial(int C) { return 0; }
__host__ __device__ inline size_t pose_ws_cur(int C) { return (size_t)C * kProjStride; }
__host__ __device__ inline size_t pose_ws_state(int C) { return (size_t)2 * C * kProjStride; }
__host__ __device__ inline size_t pose_ws_active(int C) { return pose_ws_state(C) + (size_t)C * kPoseStateStride; }
__host__ __device__ inline size_t pose_ws_partials(int C) { return pose_ws_active(C) + 16; }
__host__ __device__ inline size_t pose_ws_doubles(int C) { return pose_ws_partials(C) + (size_t)kPoseGridCap * C * kPosePartial; }

// One observation's terms at the trial pose q: E in the rule's plain operations, the 2 x 6 Jacobian at delta = 0
// (dpc / domega = R^T [d]x, dpc / dtau = -R^T), H (lower triangle, row by row) and g with fma.  -> valid at the trial pose.
// HUBER: w rho in E, w kappa in H and g; lin: the observation is in the linear regime.
template <bool HUBER>
__device__ __forceinline__ bool pose_add_obs(double (&acc)[28], const double *__restrict__ q, double ou, double ov, double w, double X, double Y,
                                             double Z, const HuberConst &hc, bool &lin) {
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
        for (int b = 0; b <= a; b++) acc[7 + a * (a + 1) / 2 + b] = fma(wu, du[b], fma(wv, dv[b], acc[7 + a * (a + 1) / 2 + b]));
    }
    return valid;
}

// Record i of [F][P][kn] taken apart (32-bit index arithmetic where it is enough) and read: -> measured; (X, Y, Z) is the record's
// point, (0, 0, 0) for a missing one: a record that is no observation computes on a finite point and nothing of it is kept.
template <typename TX>
__device__ __forceinline__ bool pose_record(const TX *__restrict__ xyzs, int64_t i, int64_t n_rec, int P, int kn, int64_t &f, int &p, int &j,
                                            double &X, double &Y, double &Z) {
    const int64_t per_frame = (int64_t)P * kn;
    int pj;
    if (n_rec <= 0x7fffffff) {
        const uint32_t fi = (uint32_t)i / (uint32_t)per_frame;
        f = fi;
        pj = (int)((uint32_t)i - fi * (uint32_t)per_frame);
    } else {
        f = i / per_frame;
        pj = (int)(i - f * per_frame);
    }
    p = pj / kn;
    j = pj - p * kn;
    SNOWTRI_DEV_CHECK(i >= 0 && i < n_rec && f >= 0 && p >= 0 && p < P && j >= 0 && j < kn, 103);
    const Rec4<TX> r = reinterpret_cast<const Rec4<TX> *>(xyzs)[i];
    const double rx = (double)r.x, ry = (double)r.y, rz = (double)r.z, rs = (double)r.s;
    const bool measured = rs != 0.0 && finite_f64(rx) && finite_f64(ry) && finite_f64(rz) && finite_f64(rs);
    X = measured ? rx : 0.0;
    Y = measured ? ry : 0.0;
    Z = measured ? rz : 0.0;
    return measured;
}

// xyzs [F][P][kn][4], kpts [F][C][Pmax][kn][3], n_persons [F][C] or null, det_of [F][C][P] or null, views [F][P][kn] or null;
// base: the input pose table (fixes the observation sets), trial: the table the sums are formed at, active [C] or null (null:
// every camera) -> partials [G][C][kPosePartial]; n_rec = F * P * kn, G = gridDim.x, C = gridDim.y.  HUBER: the loss hc
template <typename TX, typename TK, bool HUBER = false>
__global__ __launch_bounds__(kPoseBlock) void k_pose_normal(int64_t n_rec, int C, int P, int Pmax, int kn, double kthr, uint32_t flags,
                                                            const double *__restrict__ base, const double *__restrict__ trial,
                                                            const int32_t *__restrict__ active, const TX *__restrict__ xyzs,
                                                            const TK *__restrict__ kpts, const int32_t *__restrict__ n_persons,
                                                            const int32_t *__restrict__ det_of, const uint32_t *__restrict__ views,
                                                            double *__restrict__ partials, HuberConst hc) {
    const int c = blockIdx.y;
    SNOWTRI_DEV_CHECK(!HUBER || (hc.d > 0.0 && hc.dd > 0.0 && finite_f64(hc.dd)), 107);
    SNOWTRI_DEV_CHECK(c >= 0 && c < C && (int)gridDim.y == C && C <= kRefineMaxCams && (int)gridDim.x <= kPoseGridCap && Pmax >= 1 &&
                          (det_of || P <= Pmax), 102);
    if (active && !active[c]) return;   // (block-uniform: nobody waits at the barrier below)
    const double *__restrict__ q0 = base + (size_t)c * kProjStride;
    const double *__restrict__ q = trial + (size_t)c * kProjStride;
    const bool score_w = (flags & kRefineScoreWeights) != 0;
    double acc[28];
#pragma unroll
    for (int k = 0; k < 28; k++) acc[k] = 0.0;
    double n_in = 0.0, n_bad = 0.0;   // (counts as doubles: exact up to 2^53, and they travel with the sums)
    [[maybe_unused]] double n_lin = 0.0;
    constexpr int kSums = HUBER ? 31 : 30;   // what a block adds up: acc[28], n_in, n_bad and, with the loss, n_lin
    for (int64_t i = blockIdx.x * (int64_t)kPoseBlock + threadIdx.x; i < n_rec; i += (int64_t)gridDim.x * kPoseBlock) {
        int64_t f;
        int p, j;
        double X, Y, Z, ou, ov, os;
        const bool measured = pose_record(xyzs, i, n_rec, P, kn, f, p, j, X, Y, Z);
        const uint32_t allowed = views ? views[i] : 0xffffffffu;
        const bool listed = refine_observation(kpts, n_persons, det_of, f, c, C, P, Pmax, kn, p, j, ou, ov, os);
        if (refine_admits(q0, measured, listed, ou, ov, os, kthr, allowed, c, X, Y, Z)) {   // k_refine's own rule 1
            bool lin;
            const bool valid = pose_add_obs<HUBER>(acc, q, ou, ov, score_w ? os : 1.0, X, Y, Z, hc, lin);
            n_in += 1.0;
            n_bad += valid ? 0.0 : 1.0;
            if constexpr (HUBER) n_lin += lin ? 1.0 : 0.0;
        }
    }
    // the block's partial: a fixed butterfly over the wave, then the four waves in wave order
    __shared__ double lds[kPoseBlock / 64][kPosePartial];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
#pragma unroll
    for (int k = 0; k < kSums; k++) {
        double v = k < 28 ? acc[k] : (k == 28 ? n_in : k == 29 ? n_bad : n_lin);
#pragma unroll
        for (int w = 32; w >= 1; w >>= 1) v += __shfl_xor(v, w, 64);
        if (lane == 0) lds[wave][k] = v;
    }
    __syncthreads();
    if (threadIdx.x < kPosePartial) {
        const int k = threadIdx.x;
        double v = 0.0;
        if (k < kSums) v = ((lds[0][k] + lds[1][k]) + lds[2][k]) + lds[3][k];
        partials[((size_t)blockIdx.x * C + c) * kPosePartial + k] = v;
    }
}

#ifdef SNOWTRI_POSE_PER_RECORD
// THE SHAPE THAT LOST (EXPERIMENTS.md round 22; a -DSNOWTRI_DEV_EXPERIMENTS -DSNOWTRI_POSE_PER_RECORD build launches it in
// k_pose_normal's place, scripts/bench_pose.py measures either): a lane per record that loops over the cameras.  A record and its
// `views` word are read once instead of once per camera, and the camera constants are still scalar loads (the loop index is
// uniform); but a lane cannot keep 30 C sums, so every (sweep, camera) ends in a butterfly over the wave whose total lane 0 adds to
// the wave's LDS row of that camera.  Grid (G), the same partials [G][C][kPosePartial] for the same k_pose_step.
template <typename TX, typename TK>
__global__ __launch_bounds__(kPoseBlock) void k_pose_normal_rec(int64_t n_rec, int C, int P, int Pmax, int kn, double kthr, uint32_t flags,
                                                                const double *__restrict__ base, const double *__restrict__ trial,
                                                                const int32_t *__restrict__ active, const TX *__restrict__ xyzs,
                                                                const TK *__restrict__ kpts, const int32_t *__restrict__ n_persons,
                                                                const int32_t *__restrict__ det_of, const uint32_t *__restrict__ views,
                                                                double *__restrict__ partials) {
    SNOWTRI_DEV_CHECK(C >= 1 && C <= kRefineMaxCams && (int)gridDim.x <= kPoseGridCap && gridDim.y == 1 && Pmax >= 1 && (det_of || P <= Pmax), 105);
    __shared__ double lds[kPoseBlock / 64][kRefineMaxCams][kPosePartial];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    for (int k = threadIdx.x; k < C * kPosePartial; k += kPoseBlock)
#pragma unroll
        for (int w = 0; w < kPoseBlock / 64; w++) lds[w][k / kPosePartial][k % kPosePartial] = 0.0;
    __syncthreads();
    const bool score_w = (flags & kRefineScoreWeights) != 0;
    for (int64_t i0 = blockIdx.x * (int64_t)kPoseBlock; i0 < n_rec; i0 += (int64_t)gridDim.x * kPoseBlock) {   // (block-uniform trip count)
        const int64_t i1 = i0 + threadIdx.x;
        const bool live = i1 < n_rec;
        const int64_t i = live ? i1 : n_rec - 1;   // lanes past the end read the last record and add nothing
        int64_t f;
        int p, j;
        double X, Y, Z;
        const bool measured = pose_record(xyzs, i, n_rec, P, kn, f, p, j, X, Y, Z);
        const uint32_t allowed = views ? views[i] : 0xffffffffu;
#pragma unroll 1
        for (int c = 0; c < C; c++) {
            if (active && !active[c]) continue;   // (uniform)
            double ou, ov, os, term[28];
#pragma unroll
            for (int k = 0; k < 28; k++) term[k] = 0.0;
            double n_in = 0.0, n_bad = 0.0;
            const bool listed = refine_observation(kpts, n_persons, det_of, f, c, C, P, Pmax, kn, p, j, ou, ov, os);
            if (live && refine_admits(base + (size_t)c * kProjStride, measured, listed, ou, ov, os, kthr, allowed, c, X, Y, Z)) {
                bool lin_;
                const bool valid = pose_add_obs<false>(term, trial + (size_t)c * kProjStride, ou, ov, score_w ? os : 1.0, X, Y, Z, HuberConst{}, lin_);
                n_in = 1.0;
                n_bad = valid ? 0.0 : 1.0;
            }
#pragma unroll
            for (int k = 0; k < 30; k++) {
                double v = k < 28 ? term[k] : (k == 28 ? n_in : n_bad);
#pragma unroll
                for (int w = 32; w >= 1; w >>= 1) v += __shfl_xor(v, w, 64);
                if (lane == 0) lds[wave][c][k] += v;
            }
        }
    }
    __syncthreads();
    for (int k = threadIdx.x; k < C * kPosePartial; k += kPoseBlock) {
        const int c = k / kPosePartial, s = k % kPosePartial;
        partials[((size_t)blockIdx.x * C + c) * kPosePartial + s] = s < 30 ? ((lds[0][c][s] + lds[1][c][s]) + lds[2][c][s]) + lds[3][c][s] : 0.0;
    }
}
#endif

// H delta = -g by a 6 x 6 LDL^T in plain operations (the NumPy rule's, operation for operation); h: the lower triangle row by row.
// -> every pivot is finite and > 0 (delta is meaningful only then).
__device__ __forceinline__ bool pose_solve(const double *h, const double *g, double (&delta)[6]) {
#pragma clang fp contract(off)
    double L[6][6], piv[6], y[6];
    bool pd = true;
#pragma unroll
    for (int a = 0; a < 6; a++) {
#pragma unroll
        for (int b = 0; b <= a; b++) {
            double s = h[a * (a + 1) / 2 + b];
#pragma unroll
            for (int k = 0; k < b; k++) s = s - L[a][k] * (L[b][k] * piv[k]);
            if (b < a) L[a][b] = s / piv[b];
            else piv[a] = s;
        }
        pd = pd && piv[a] > 0.0 && finite_f64(piv[a]);
    }
#pragma unroll
    for (int a = 0; a < 6; a++) {
        double s = -g[a];
#pragma unroll
        for (int k = 0; k < a; k++) s = s - L[a][k] * y[k];
        y[a] = s;
    }
#pragma unroll
    for (int a = 5; a >= 0; a--) {
        double s = y[a] / piv[a];
#pragma unroll
        for (int k = a + 1; k < 6; k++) s = s - L[k][a] * delta[k];
        delta[a] = s;
    }
    return pd;
}

// R (row-major, camera -> world) <- Exp(omega) R by Rodrigues' formula: a = sin(th) / th, b = 2 sin^2(th / 2) / th^2.
__device__ __forceinline__ void pose_rotate(const double *R, const double *om, double *out) {
#pragma clang fp contract(off)
    const double th2 = (om[0] * om[0] + om[1] * om[1]) + om[2] * om[2];
    const double th = sqrt(th2);
    double a = 1.0, b = 0.5;
    if (th > 0.0) {
        const double sh = sin(0.5 * th);
        a = sin(th) / th;
        b = (2.0 * (sh * sh)) / th2;
    }
    const double W[3][3] = {{0.0, -om[2], om[1]}, {om[2], 0.0, -om[0]}, {-om[1], om[0], 0.0}};
    double E[3][3];
#pragma unroll
    for (int i = 0; i < 3; i++)
#pragma unroll
        for (int j = 0; j < 3; j++) {
            const double w2 = (W[i][0] * W[0][j] + W[i][1] * W[1][j]) + W[i][2] * W[2][j];
            E[i][j] = ((i == j ? 1.0 : 0.0) + a * W[i][j]) + b * w2;
        }
#pragma unroll
    for (int i = 0; i < 3; i++)
#pragma unroll
        for (int j = 0; j < 3; j++) out[3 * i + j] = (E[i][0] * R[j] + E[i][1] * R[3 + j]) + E[i][2] * R[6 + j];
}

// Behind evaluation `eval` (0: at the input pose) of G blocks per camera: the sums, every camera's decision and next trial pose;
// with `last` the outputs.  ws: the context's workspace (pose_ws_*), base: the input pose table.
__global__ __launch_bounds__(kPoseStepBlock) void k_pose_step(int C, int G, int eval, int last, uint32_t free_mask, int min_obs,
                                                              const double *__restrict__ base, double *__restrict__ ws,
                                                              double *__restrict__ R_out, double *__restrict__ t_out, double *__restrict__ cost,
                                                              int64_t *__restrict__ n_obs, uint8_t *__restrict__ codes,
                                                              double *__restrict__ normal, int64_t *__restrict__ n_outliers) {
#pragma clang fp contract(off)
    __shared__ double seg_sum[kPoseSegments][kPosePartial];
    __shared__ double tot[kRefineMaxCams][kPosePartial];
    double *trial = ws + pose_ws_trial(C), *cur = ws + pose_ws_cur(C), *state = ws + pose_ws_state(C);
    int32_t *active = reinterpret_cast<int32_t *>(ws + pose_ws_active(C));
    const double *partials = ws + pose_ws_partials(C);
    const int slot = threadIdx.x & (kPosePartial - 1), seg = threadIdx.x >> 5;
    const int Gs = (G + kPoseSegments - 1) / kPoseSegments;
    SNOWTRI_DEV_CHECK(C >= 1 && C <= kRefineMaxCams && G >= 0 && G <= kPoseGridCap && Gs <= kPoseSegments, 104);
    for (int c = 0; c < C; c++) {
        const bool evaluated = eval == 0 || active[c] != 0;   // (block-uniform)
        if (!evaluated) continue;
        double v[kPoseSegments];
#pragma unroll
        for (int k = 0; k < kPoseSegments; k++) {   // the loads first, all in flight; then the additions in block order
            const int b = seg * Gs + k;
            v[k] = (k < Gs && b < G) ? partials[((size_t)b * C + c) * kPosePartial + slot] : 0.0;
        }
        double s = 0.0;
#pragma unroll
        for (int k = 0; k < kPoseSegments; k++) s = s + v[k];
        seg_sum[seg][slot] = s;
        __syncthreads();
        if (threadIdx.x < kPosePartial) {
            double t_ = 0.0;
            for (int k = 0; k < kPoseSegments; k++) t_ = t_ + seg_sum[k][slot];
            tot[c][slot] = t_;
        }
        __syncthreads();
    }
    __syncthreads();   // active[] is read above by every lane and written below by lane c: every read comes first
    const int c = threadIdx.x;
    if (c >= C) return;
    const double *b_ = base + (size_t)c * kProjStride;
    double *tr = trial + (size_t)c * kProjStride, *cu = cur + (size_t)c * kProjStride, *st = state + (size_t)c * kPoseStateStride;
    const double *sum = tot[c];
    bool act;
    if (eval == 0) {
        for (int k = 0; k < kProjStride; k++) cu[k] = tr[k] = b_[k];
        for (int k = 0; k < 28; k++) st[k] = sum[k];
        if (normal)
            for (int k = 0; k < 28; k++) normal[(size_t)c * 28 + k] = sum[k];
        const bool is_free = (free_mask >> c) & 1u, few = sum[28] < (double)min_obs;
        st[28] = sum[0];
        st[29] = sum[28];
        st[31] = sum[30];   // the observations in the linear regime at the pose the state is of (0 under the squared loss)
        st[30] = !is_free ? (double)kPoseFixed : few ? (double)kPoseFewObs : (double)kPoseKept;
        act = is_free && !few;
    } else if (active[c]) {
        const bool accept = sum[29] == 0.0 && sum[0] < st[0];
        if (accept) {
            for (int k = 0; k < 12; k++) cu[k] = tr[k];
            for (int k = 0; k < 28; k++) st[k] = sum[k];
            st[30] = (double)kPoseMoved;
            st[31] = sum[30];
        }
        act = accept;
    } else
        act = false;
    if (act && !last) {
        double delta[6];
        act = pose_solve(st + 7, st + 1, delta);
        if (act) {
            double Rn[9];
            pose_rotate(cu, delta, Rn);
            for (int k = 0; k < 9; k++) tr[k] = Rn[k];
            for (int k = 0; k < 3; k++) tr[9 + k] = cu[9 + k] + delta[3 + k];
        }
    }
    active[c] = (act && !last) ? 1 : 0;
    if (last) {
        const int code = (int)st[30];
        const bool still = code == kPoseFixed || code == kPoseFewObs;
        for (int k = 0; k < 9; k++) R_out[(size_t)c * 9 + k] = cu[k];
        for (int k = 0; k < 3; k++) t_out[(size_t)c * 3 + k] = cu[9 + k];
        if (cost) {
            cost[2 * c] = still ? 0.0 : st[28];
            cost[2 * c + 1] = still ? 0.0 : st[0];
        }
        if (n_obs) n_obs[c] = (int64_t)st[29];
        if (codes) codes[c] = (uint8_t)code;
        if (n_outliers) n_outliers[c] = still ? 0 : (int64_t)st[31];
    }
}

}  // namespace snowtri
