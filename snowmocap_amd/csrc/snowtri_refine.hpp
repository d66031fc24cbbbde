// snowtri_refine.hpp -- k_refine: joint records of any route moved to a local minimum of their weighted reprojection error by a few
// Gauss-Newton steps on a 3 x 3 system per joint (include/snowtri.h, "Refinement", states the rule; snowmocap_amd/refine.py is the
// rule in NumPy and what the tests compare classes and costs with).  No reference counterpart.
//
// One lane per record (f, p, j).  The geometry is project_record's (snowtri_reproject.hpp): d = X - t_c first, so nothing depends
// on where the world's origin lies.  The view set is fixed with refine_view, which is project_record operation for operation (the
// same chain of fma, one 1 / pc2): a view is in the set exactly when snowtri_reproject calls its pixel valid.  The COST, which
// decides every step and is reported, is formed in the rule's own plain operations instead (refine_add_view): it equals the NumPy
// rule's E at the same point bit for bit, so "the cost never rises" holds in the arithmetic a caller recomputes it in, down to
// exact detections where E is nothing but rounding.  H and g, which only steer, use fma.  Contraction is off in the kernel and in
// refine_add_view: every product-sum is an explicit fma or separately rounded operations, whichever inlined copy computes it.
//
// The camera constants are the context's proj table (kProjStride doubles per camera), read with a wave-uniform index: scalar loads,
// no LDS, no barrier.  The observations:
//   CT = 4, 8 (the rig has exactly CT cameras): (u, v, w) of every camera stay in registers, all loops unrolled, no scratch;
//   CT = 0 (any other C <= 32): a loop over the cameras that reads the observation again from the cache at every evaluation.
// A camera outside the view set keeps its place in the loop with weight 0, a zeroed observation and 1 / pc2 replaced by 0, so its
// terms are exact zeros whatever its geometry is; a lane without a view set (missing, fewer than two views, past the end) works on
// the point (0, 0, 0) and stores the record it read.
//
// evaluate(X) -> E, H = sum w J^T J (six values), g = sum w J^T r, and whether every view of the set is valid at X.  The point a
// step is tried at is the point the next step starts from, so an accepted trial's H and g are kept: iters + 1 evaluations and one
// pass that fixes the view set.  The iteration is a wave loop, while (__any(active)); every select is per lane, so a settled lane
// keeps its bits whatever its wave-mates still do, and a record's output depends on its own record, its own observations and the
// rig only.
//
// HUBER == true (include/snowtri.h, ROBUST LOSS; snowtri_refine_joints_ex with huber_px > 0) is a second instantiation of the same
// kernel: per view s = ru ru + rv rv is compared with delta^2, a view beyond it adds (2 delta) sqrt(s) - delta^2 to E and weighs
// delta / sqrt(s) of w in H and g (IRLS; kappa is formed again in every evaluation, nothing is held per view), and the evaluation
// carries the mask of the views in the linear regime, which behind the last accepted step is the `outliers` word.  The sqrt is the
// correctly rounded one and E stays in the rule's plain operations.  HUBER == false compiles to the instructions it did before the
// switch existed (what the loss adds is under if constexpr).
#pragma once
#include "snowtri_reproject.hpp"

namespace snowtri {

constexpr int kRefineMaxCams = 32;    // a view set is a 32-bit mask (the mask snowtri_triangulate_robust writes)
constexpr int kRefineMaxIters = 16;
constexpr int kRefineBlock = 256;
constexpr uint32_t kRefineScoreWeights = 1u;   // SNOWTRI_REFINE_SCORE_WEIGHTS
enum : uint8_t { kRefineMissing = 0, kRefineFewViews = 1, kRefineKept = 2, kRefineMoved = 3 };

struct RefineEval {
    double E, h00, h10, h11, h20, h21, h22, g0, g1, g2;
    bool valid;   // every view of the set projects validly
};

// The loss' constants, formed once in fp64 on the host: delta, 2 delta, delta^2 (all 0 and unused under the squared loss).
struct HuberConst {
    double d, two_d, dd;
};

// ROBUST LOSS on one view's s = ru ru + rv rv, every operation rounded on its own: -> in the linear regime; rho and kappa.
__device__ __forceinline__ bool huber_terms(const HuberConst &hc, double s, double &rho, double &kappa) {
#pragma clang fp contract(off)
    const bool lin = !(s <= hc.dd);
    const double r = __dsqrt_rn(s);   // correctly rounded, as the NumPy rule's
    const double t = hc.two_d * r;
    rho = lin ? t - hc.dd : s;
    kappa = lin ? hc.d / r : 1.0;
    return lin;
}

// project_record's rules 1 and 3 on a measured record's point, kept open: -> pc2 > 0 and finite u, v.
__device__ __forceinline__ bool refine_view(const double *__restrict__ q, double X, double Y, double Z, double &x, double &y, double &iz,
                                            double &u, double &v) {
    const double d0 = X - q[9], d1 = Y - q[10], d2 = Z - q[11];
    const double pc0 = fma(q[6], d2, fma(q[3], d1, q[0] * d0));
    const double pc1 = fma(q[7], d2, fma(q[4], d1, q[1] * d0));
    const double pc2 = fma(q[8], d2, fma(q[5], d1, q[2] * d0));
    iz = 1.0 / pc2;
    x = pc0 * iz;
    y = pc1 * iz;
    u = fma(q[12], x, fma(q[13], y, q[14]));
    v = fma(q[15], y, q[16]);
    return pc2 > 0.0 && finite_f64(u) && finite_f64(v);
}

// Camera c's observation of record (f, p, j): -> listed (rule 1, first item), and (u, v, s) -- of detection 0 when not listed.
// kpts [F][C][Pmax][kn][3], n_persons [F][C] or null, det_of [F][C][P] or null.  Shared with snowtri_pose.hpp.
template <typename TK>
__device__ __forceinline__ bool refine_observation(const TK *__restrict__ kpts, const int32_t *__restrict__ n_persons,
                                                   const int32_t *__restrict__ det_of, int64_t f, int c, int C, int P, int Pmax, int kn, int p,
                                                   int j, double &ou, double &ov, double &os) {
    const int64_t fc = f * C + c;
    const int q = det_of ? det_of[fc * P + p] : p;
    const int nq = n_persons ? n_persons[fc] : Pmax;
    const bool listed = q >= 0 && q < nq && q < Pmax;   // (q < Pmax: an n_persons past the array is not followed)
    SNOWTRI_DEV_CHECK(c >= 0 && c < C && Pmax >= 1, 98);
    const Kp3<TK> o = reinterpret_cast<const Kp3<TK> *>(kpts)[(fc * Pmax + (listed ? q : 0)) * (int64_t)kn + j];
    ou = (double)o.u;
    ov = (double)o.v;
    os = (double)o.s;
    return listed;
}

// Rule 1 for one camera (q: its proj row): is the observation (ou, ov, os) of the measured point (X, Y, Z) a view of the record?
__device__ __forceinline__ bool refine_admits(const double *__restrict__ q, bool measured, bool listed, double ou, double ov, double os, double kthr,
                                              uint32_t allowed, int c, double X, double Y, double Z) {
    double x, y, iz, pu, pv;
    const bool front = refine_view(q, X, Y, Z, x, y, iz, pu, pv);
    return measured && listed && finite_f64(ou) && finite_f64(ov) && !(os < kthr) && ((allowed >> c) & 1u) && front;
}

// One view's terms of E, H and g at X: w ((u - ou)^2 + (v - ov)^2), w J^T J, w J^T r with the 2 x 3 Jacobian
// dx = (R^T row 0 - x R^T row 2) / pc2, dy likewise, du = fx dx + s dy, dv = fy dy.  in == false: exact zeros.
// HUBER: w rho in E, w kappa in H and g; -> the view is in the linear regime (false under the squared loss and for in == false,
// whose s is 0).
template <bool HUBER>
__device__ __forceinline__ bool refine_add_view(RefineEval &e, const double *__restrict__ q, bool in, double ou, double ov, double w, double X,
                                                double Y, double Z, const HuberConst &hc) {
#pragma clang fp contract(off)
    // THE COST IS THE RULE'S, OPERATION FOR OPERATION: E decides every step and is what the caller is told, so it is formed as
    // include/snowtri.h and refine_joints_reference write it -- every product, sum and quotient rounded on its own, in their order,
    // the views added in camera order -- and equals the NumPy rule's E at the same point bit for bit.  (The fma chain of
    // project_record gives pixels a few 1e-13 px away; in u(X) - u that is 1e-13 of E, and at exact detections all of it.)
    const double fx = q[12], sk = q[13], fy = q[15];
    const double d0 = X - q[9], d1 = Y - q[10], d2 = Z - q[11];
    const double pc0 = (q[0] * d0 + q[3] * d1) + q[6] * d2;
    const double pc1 = (q[1] * d0 + q[4] * d1) + q[7] * d2;
    const double pc2 = (q[2] * d0 + q[5] * d1) + q[8] * d2;
    double x = pc0 / pc2, y = pc1 / pc2;
    const double u = (fx * x + sk * y) + q[14], v = fy * y + q[16];
    e.valid = e.valid && ((pc2 > 0.0 && finite_f64(u) && finite_f64(v)) || !in);
    const double ru = in ? u - ou : 0.0, rv = in ? v - ov : 0.0;
    bool lin = false;
    if constexpr (HUBER) {
        double rho, kappa;
        lin = huber_terms(hc, ru * ru + rv * rv, rho, kappa);
        e.E = e.E + w * rho;
        w = w * kappa;   // the IRLS weight (w * 1.0 is w: the quadratic regime is the squared rule operation for operation)
    } else {
        e.E = e.E + w * (ru * ru + rv * rv);
    }
    // H and g only steer: fused multiply-adds from here on
    const double iz = in ? 1.0 / pc2 : 0.0;
    x = in ? x : 0.0;
    y = in ? y : 0.0;
    const double dx0 = fma(-x, q[2], q[0]) * iz, dx1 = fma(-x, q[5], q[3]) * iz, dx2 = fma(-x, q[8], q[6]) * iz;
    const double dy0 = fma(-y, q[2], q[1]) * iz, dy1 = fma(-y, q[5], q[4]) * iz, dy2 = fma(-y, q[8], q[7]) * iz;
    const double du0 = fma(fx, dx0, sk * dy0), du1 = fma(fx, dx1, sk * dy1), du2 = fma(fx, dx2, sk * dy2);
    const double dv0 = fy * dy0, dv1 = fy * dy1, dv2 = fy * dy2;
    const double wu0 = w * du0, wu1 = w * du1, wu2 = w * du2, wv0 = w * dv0, wv1 = w * dv1, wv2 = w * dv2;
    e.h00 = fma(wu0, du0, fma(wv0, dv0, e.h00));
    e.h10 = fma(wu1, du0, fma(wv1, dv0, e.h10));
    e.h11 = fma(wu1, du1, fma(wv1, dv1, e.h11));
    e.h20 = fma(wu2, du0, fma(wv2, dv0, e.h20));
    e.h21 = fma(wu2, du1, fma(wv2, dv1, e.h21));
    e.h22 = fma(wu2, du2, fma(wv2, dv2, e.h22));
    e.g0 = fma(wu0, ru, fma(wv0, rv, e.g0));
    e.g1 = fma(wu1, ru, fma(wv1, rv, e.g1));
    e.g2 = fma(wu2, ru, fma(wv2, rv, e.g2));
    return lin;
}

// H d = -g by LDL^T; -> every pivot is finite and > 0 (d is meaningful only then).
__device__ __forceinline__ bool refine_solve(const RefineEval &e, double &s0, double &s1, double &s2) {
    const double p0 = e.h00;
    const double i0 = 1.0 / p0;
    const double l10 = e.h10 * i0, l20 = e.h20 * i0;
    const double p1 = fma(-l10, e.h10, e.h11);
    const double i1 = 1.0 / p1;
    const double m21 = fma(-l20, e.h10, e.h21);
    const double l21 = m21 * i1;
    const double p2 = fma(-l21, m21, fma(-l20, e.h20, e.h22));
    const double i2 = 1.0 / p2;
    const double y0 = -e.g0;
    const double y1 = fma(-l10, y0, -e.g1);
    const double y2 = fma(-l21, y1, fma(-l20, y0, -e.g2));
    s2 = y2 * i2;
    s1 = fma(-l21, s2, y1 * i1);
    s0 = fma(-l20, s2, fma(-l10, s1, y0 * i0));
    return p0 > 0.0 && finite_f64(p0) && p1 > 0.0 && finite_f64(p1) && p2 > 0.0 && finite_f64(p2);
}

// xyzs / out [F][P][kn][4] (out may be xyzs itself), kpts [F][C][Pmax][kn][3], n_persons [F][C] or null, det_of [F][C][P] or null,
// views [F][P][kn] or null -> out, cost [F][P][kn][2] or null, codes [F][P][kn] or null; n_rec = F * P * kn.  HUBER: the loss hc
// and -> outliers [F][P][kn] or null (bit c: camera c is a view and in the linear regime at the output point; 0 for a copied record)
template <int CT, typename TX, typename TK, bool HUBER = false>
__global__ __launch_bounds__(kRefineBlock) void k_refine(int64_t n_rec, int C, int P, int Pmax, int kn, double kthr, int iters, uint32_t flags,
                                                         const double *__restrict__ proj, const TX *xyzs, const TK *__restrict__ kpts,
                                                         const int32_t *__restrict__ n_persons, const int32_t *__restrict__ det_of,
                                                         const uint32_t *__restrict__ views, TX *out, double *__restrict__ cost,
                                                         uint8_t *__restrict__ codes, HuberConst hc, uint32_t *__restrict__ outliers) {
#pragma clang fp contract(off)   // comparisons decide here (E(X + d) < E(X), the pivots): nothing is left to the place of inlining
    static_assert(CT == 0 || (CT >= 2 && CT <= 8), "k_refine: observations in registers for up to eight cameras");
    constexpr int kRegs = CT > 0 ? CT : 1;
    const int64_t i0 = blockIdx.x * (int64_t)kRefineBlock + threadIdx.x;
    const bool live = i0 < n_rec;
    const int64_t i = live ? i0 : n_rec - 1;   // lanes past the end read the last record and store nothing (the wave votes below)
    const int64_t per_frame = (int64_t)P * kn;
    const int64_t f = i / per_frame;
    const int pj = (int)(i - f * per_frame);
    const int p = pj / kn, j = pj - p * kn;
    const int nc = CT > 0 ? CT : C;
    SNOWTRI_DEV_CHECK(f >= 0 && p >= 0 && p < P && j >= 0 && j < kn && (CT == 0 || CT == C) && C <= kRefineMaxCams && (det_of || P <= Pmax), 97);
    SNOWTRI_DEV_CHECK(HUBER ? (hc.d > 0.0 && hc.dd > 0.0 && finite_f64(hc.dd)) : outliers == nullptr, 106);
    const Rec4<TX> r = reinterpret_cast<const Rec4<TX> *>(xyzs)[i];
    const double rx = (double)r.x, ry = (double)r.y, rz = (double)r.z, rs = (double)r.s;
    const bool measured = rs != 0.0 && finite_f64(rx) && finite_f64(ry) && finite_f64(rz) && finite_f64(rs);
    const uint32_t allowed = views ? views[i] : 0xffffffffu;
    const bool score_w = (flags & kRefineScoreWeights) != 0;
    // the point every evaluation of a lane without a view set works on: finite, so that nothing it computes is ever a trap
    double X = measured ? rx : 0.0, Y = measured ? ry : 0.0, Z = measured ? rz : 0.0;

    auto observation = [&](int c, double &ou, double &ov, double &os) -> bool {
        return refine_observation(kpts, n_persons, det_of, f, c, C, P, Pmax, kn, p, j, ou, ov, os);
    };

    // ---- rule 1: the view set, fixed once at X0
    uint32_t V = 0u;
    double ou[kRegs], ov[kRegs], ow[kRegs];
#pragma unroll
    for (int k = 0; k < kRegs; k++) ou[k] = ov[k] = ow[k] = 0.0;
    auto admit = [&](int c, double &u_, double &v_, double &w_) {
        double s_;
        const bool listed = observation(c, u_, v_, s_);
        const bool in = refine_admits(proj + (size_t)c * kProjStride, measured, listed, u_, v_, s_, kthr, allowed, c, X, Y, Z);
        V |= in ? (1u << c) : 0u;
        u_ = in ? u_ : 0.0;
        v_ = in ? v_ : 0.0;
        w_ = in ? (score_w ? s_ : 1.0) : 0.0;
    };
    if constexpr (CT > 0) {
#pragma unroll
        for (int c = 0; c < CT; c++) {
            asm volatile("" ::: "memory");   // (as in evaluate: a camera's constants are loaded where they are used)
            admit(c, ou[c], ov[c], ow[c]);
        }
    } else {
#pragma unroll 1
        for (int c = 0; c < nc; c++) {
            double u_, v_, w_;
            admit(c, u_, v_, w_);
        }
    }
    const bool few = __popc(V) < 2;
    V = few ? 0u : V;
    bool active = live && measured && !few;

    auto evaluate = [&](double ex, double ey, double ez, uint32_t &lin) -> RefineEval {
        RefineEval e = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, true};
        lin = 0u;
        if constexpr (CT > 0) {
#pragma unroll
            for (int c = 0; c < CT; c++) {
                // a camera's seventeen constants are loaded (scalar loads, from the cache) where its terms are formed: hoisted out
                // of the iteration they are 17 CT doubles held in, and spilled from, scalar registers
                asm volatile("" ::: "memory");
                const bool l_ = refine_add_view<HUBER>(e, proj + (size_t)c * kProjStride, (V >> c) & 1u, ou[c], ov[c], ow[c], ex, ey, ez, hc);
                if constexpr (HUBER) lin |= l_ ? (1u << c) : 0u;
            }
        } else {
#pragma unroll 1
            for (int c = 0; c < nc; c++) {
                double u_, v_, s_;
                observation(c, u_, v_, s_);
                const bool in = (V >> c) & 1u;
                const bool l_ = refine_add_view<HUBER>(e, proj + (size_t)c * kProjStride, in, in ? u_ : 0.0, in ? v_ : 0.0,
                                                       in ? (score_w ? s_ : 1.0) : 0.0, ex, ey, ez, hc);
                if constexpr (HUBER) lin |= l_ ? (1u << c) : 0u;
            }
        }
        return e;
    };

    // ---- rules 3 and 4
    uint32_t cur_lin, nxt_lin;   // the views in the linear regime at the current point and at the trial (HUBER only)
    RefineEval cur = evaluate(X, Y, Z, cur_lin);
    const double E0 = cur.E;
    bool moved = false;
    int it = 0;
    while (__any(active) && it < iters) {
        double s0, s1, s2;
        const bool pd = refine_solve(cur, s0, s1, s2);
        const double tx = X + s0, ty = Y + s1, tz = Z + s2;
        const bool tryit = active && pd;
        const RefineEval nxt = evaluate(tryit ? tx : X, tryit ? ty : Y, tryit ? tz : Z, nxt_lin);
        const bool accept = tryit && nxt.valid && nxt.E < cur.E;
        X = accept ? tx : X;
        Y = accept ? ty : Y;
        Z = accept ? tz : Z;
        cur.E = accept ? nxt.E : cur.E;
        cur.h00 = accept ? nxt.h00 : cur.h00;
        cur.h10 = accept ? nxt.h10 : cur.h10;
        cur.h11 = accept ? nxt.h11 : cur.h11;
        cur.h20 = accept ? nxt.h20 : cur.h20;
        cur.h21 = accept ? nxt.h21 : cur.h21;
        cur.h22 = accept ? nxt.h22 : cur.h22;
        cur.g0 = accept ? nxt.g0 : cur.g0;
        cur.g1 = accept ? nxt.g1 : cur.g1;
        cur.g2 = accept ? nxt.g2 : cur.g2;
        if constexpr (HUBER) cur_lin = accept ? nxt_lin : cur_lin;
        moved = moved || accept;
        active = accept;
        ++it;
    }

    if (!live) return;
    const bool copied = !measured || few;
    Rec4<TX> o = r;   // a copied or kept record: the bits that were read
    if (moved) {
        o.x = (TX)X;
        o.y = (TX)Y;
        o.z = (TX)Z;
    }
    reinterpret_cast<Rec4<TX> *>(out)[i] = o;
    if (cost) {
        cost[2 * i] = copied ? 0.0 : E0;
        cost[2 * i + 1] = copied ? 0.0 : cur.E;
    }
    if (codes) codes[i] = !measured ? kRefineMissing : few ? kRefineFewViews : moved ? kRefineMoved : kRefineKept;
    if constexpr (HUBER)
        if (outliers) outliers[i] = copied ? 0u : (cur_lin & V);   // (a plain vector store)
}

}  // namespace snowtri
