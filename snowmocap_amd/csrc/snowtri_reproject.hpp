// snowtri_reproject.hpp -- reprojection: 3D joint records back into every camera's image (k_reproject), and the per-view match
// cost of every 3D person against every detection of a camera (k_reproject_cost).  No reference counterpart.
//
// The rule (include/snowtri.h, "Reprojection"), per camera c and record (X, score), all in fp64:
//   1. d = X - t_c, pc = R_c^T d, x = pc0 / pc2, y = pc1 / pc2                         (R: camera -> world, t: the camera centre)
//   2. RAW only: (x, y) through the forward lens model of snowtri_undistort.hpp (x_d, y_d of its header)
//   3. u = fx x + s y + cx, v = fy y + cy
//   4. valid iff the record is measured (score != 0, four finite values), pc2 > 0 and u, v are finite; else the pixel is (0, 0, 0).
// Both kernels call ONE function for that, project_record, written with explicit fma so that no contraction is left to the
// compiler's choice at the place of inlining: the pixel k_reproject stores and the pixel k_reproject_cost compares are the same
// bits, which is why the cost of a person against its own float64 projection is an exact 0.
// x and y share one correctly rounded 1 / pc2 (a division and two products instead of two divisions: 1 eps instead of 0.5).
//
// k_reproject: one lane per OUTPUT observation (f, c, p, j), no loop; 16 / 32 bytes read (the record, shared by the C lanes that
// project it -- cache hits) and 12 / 24 written.  k_reproject_cost: one wave per (f, c, p); lane l projects joints l, l + 64,
// l + 128, l + 192 once (kCostMaxJoints = 256: they stay in registers), then walks the Pmax detections of the camera, each a
// coalesced read of kn keypoints, and reduces (sum, n) over the wave with a fixed xor butterfly -- the order of an item's sum
// depends on kn alone.  Nothing is written but cost_sum / cost_n.
#pragma once
#include "snowtri_kernels.hpp"

namespace snowtri {

constexpr int kProjStride = 24;       // doubles per camera: R[9] (row-major, camera -> world), t[3], fx s cx fy cy, k1 k2 p1 p2 k3 (pad)
constexpr int kCostMaxJoints = 256;   // snowtri_reproject_cost: kn <= 4 joints per lane
constexpr int kCostWaves = 4;         // (f, c, p) items per workgroup of k_reproject_cost

struct ProjCam {
    double R[9], t[3], fx, s, cx, fy, cy, k1, k2, p1, p2, k3;
};

__device__ __forceinline__ ProjCam load_proj_cam(const double *__restrict__ q) {
    ProjCam m;
#pragma unroll
    for (int i = 0; i < 9; i++) m.R[i] = q[i];
#pragma unroll
    for (int i = 0; i < 3; i++) m.t[i] = q[9 + i];
    m.fx = q[12]; m.s = q[13]; m.cx = q[14]; m.fy = q[15]; m.cy = q[16];
    m.k1 = q[17]; m.k2 = q[18]; m.p1 = q[19]; m.p2 = q[20]; m.k3 = q[21];
    return m;
}

__device__ __forceinline__ bool finite_f64(double a) { return fabs(a) < __builtin_huge_val(); }   // (false for NaN)

// -> valid (rule 4); u, v are meaningful only then.
__device__ __forceinline__ bool project_record(const ProjCam &m, bool raw, double X, double Y, double Z, double score, double &u, double &v) {
    const double d0 = X - m.t[0], d1 = Y - m.t[1], d2 = Z - m.t[2];
    const double pc0 = fma(m.R[6], d2, fma(m.R[3], d1, m.R[0] * d0));
    const double pc1 = fma(m.R[7], d2, fma(m.R[4], d1, m.R[1] * d0));
    const double pc2 = fma(m.R[8], d2, fma(m.R[5], d1, m.R[2] * d0));
    const double iz = 1.0 / pc2;
    double x = pc0 * iz, y = pc1 * iz;
    if (raw) {
        const double r2 = fma(x, x, y * y);
        const double rho = fma(r2, fma(r2, fma(r2, m.k3, m.k2), m.k1), 1.0);
        const double xy2 = 2.0 * x * y;
        const double xd = fma(x, rho, fma(m.p1, xy2, m.p2 * fma(2.0 * x, x, r2)));
        const double yd = fma(y, rho, fma(m.p2, xy2, m.p1 * fma(2.0 * y, y, r2)));
        x = xd;
        y = yd;
    }
    u = fma(m.fx, x, fma(m.s, y, m.cx));
    v = fma(m.fy, y, m.cy);
    const bool measured = score != 0.0 && finite_f64(X) && finite_f64(Y) && finite_f64(Z) && finite_f64(score);
    return measured && pc2 > 0.0 && finite_f64(u) && finite_f64(v);
}

template <typename T>
struct Rec4 {  // one joint record as stored in xyzs: (x, y, z, score)
    T x, y, z, s;
};

// xyzs [F][P][kn][4] -> pix [F][C][P][kn][3]; n_obs = F * C * P * kn, per_person = kn, per_cam = P * kn
template <typename TX, typename TP>
__global__ __launch_bounds__(256) void k_reproject(int64_t n_obs, int C, int P, int kn, int raw, const double *__restrict__ proj,
                                                    const TX *__restrict__ xyzs, TP *__restrict__ pix) {
    const int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x;
    if (i >= n_obs) return;
    const int64_t per_cam = (int64_t)P * kn;
    const int64_t fc = i / per_cam, pj = i - fc * per_cam;   // pj = p * kn + j
    const int64_t f = fc / C;
    const int c = (int)(fc - f * C);
    SNOWTRI_DEV_CHECK(c >= 0 && c < C && pj >= 0 && pj < per_cam && f * per_cam + pj < n_obs / C, 95);   // the record lies inside xyzs
    const ProjCam m = load_proj_cam(proj + (size_t)c * kProjStride);
    const Rec4<TX> r = reinterpret_cast<const Rec4<TX> *>(xyzs)[f * per_cam + pj];
    double u, v;
    const bool ok = project_record(m, raw != 0, (double)r.x, (double)r.y, (double)r.z, (double)r.s, u, v);
    Kp3<TP> o;
    o.u = ok ? (TP)u : (TP)0;
    o.v = ok ? (TP)v : (TP)0;
    o.s = ok ? (TP)r.s : (TP)0;
    reinterpret_cast<Kp3<TP> *>(pix)[i] = o;
}

// xyzs [F][P][kn][4], kpts [F][C][Pmax][kn][3], n_persons [F][C] or null -> cost_sum / cost_n [F][C][P][Pmax]; n_items = F * C * P
template <typename TX, typename TK>
__global__ __launch_bounds__(64 * kCostWaves) void k_reproject_cost(int64_t n_items, int C, int P, int Pmax, int kn, int raw, double kthr,
                                                                    const double *__restrict__ proj, const TX *__restrict__ xyzs,
                                                                    const TK *__restrict__ kpts, const int32_t *__restrict__ n_persons,
                                                                    double *__restrict__ cost_sum, int32_t *__restrict__ cost_n) {
    constexpr int kPerLane = kCostMaxJoints / 64;
    const int lane = threadIdx.x & 63;
    const int64_t item = blockIdx.x * (int64_t)kCostWaves + (threadIdx.x >> 6);   // wave-uniform
    if (item >= n_items) return;
    const int64_t fc = item / P;
    const int p = (int)(item - fc * P);
    const int64_t f = fc / C;
    const int c = (int)(fc - f * C);
    SNOWTRI_DEV_CHECK(kn <= kCostMaxJoints && c >= 0 && c < C && p >= 0 && p < P && f >= 0, 96);
    const ProjCam m = load_proj_cam(proj + (size_t)c * kProjStride);
    const Rec4<TX> *rec = reinterpret_cast<const Rec4<TX> *>(xyzs) + (f * P + p) * (int64_t)kn;
    double pu[kPerLane], pv[kPerLane];
    bool ok[kPerLane];
#pragma unroll
    for (int k = 0; k < kPerLane; k++) {
        const int j = k * 64 + lane;
        pu[k] = pv[k] = 0.0;
        ok[k] = false;
        if (j < kn) {
            const Rec4<TX> r = rec[j];
            ok[k] = project_record(m, raw != 0, (double)r.x, (double)r.y, (double)r.z, (double)r.s, pu[k], pv[k]);
        }
    }
    const int nq = n_persons ? n_persons[fc] : Pmax;   // detections q >= nq do not count
    const Kp3<TK> *det = reinterpret_cast<const Kp3<TK> *>(kpts) + fc * Pmax * (int64_t)kn;
    for (int q = 0; q < Pmax; q++) {
        double sum = 0.0;
        int n = 0;
        if (q < nq) {
#pragma unroll
            for (int k = 0; k < kPerLane; k++) {
                const int j = k * 64 + lane;
                if (j < kn && ok[k]) {
                    const Kp3<TK> d = det[(int64_t)q * kn + j];
                    const double du = pu[k] - (double)d.u, dv = pv[k] - (double)d.v;
                    const bool counts = !((double)d.s < kthr) && finite_f64((double)d.u) && finite_f64((double)d.v);
                    if (counts) {
                        sum += fma(dv, dv, du * du);
                        n++;
                    }
                }
            }
        }
#pragma unroll
        for (int w = 32; w >= 1; w >>= 1) {   // the same pairs in the same order for every item: lane 0 ends with the wave's total
            sum += __shfl_xor(sum, w, 64);
            n += __shfl_xor(n, w, 64);
        }
        if (lane == 0) {
            const int64_t o = item * Pmax + q;
            cost_sum[o] = n ? sum : 0.0;
            cost_n[o] = n;
        }
    }
}

}  // namespace snowtri
