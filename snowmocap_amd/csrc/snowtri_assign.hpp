// snowtri_assign.hpp -- one-to-one matching of a camera's detections to the 3D persons (k_assign): the optimal gated assignment per
// (frame, camera) on the costs k_reproject_cost wrote.  No reference counterpart.
//
// The rule (include/snowtri.h, "Assignment"), per problem of P persons (rows) and Pmax detections (columns), all in fp64:
//   1. mean[p][q] = cost_sum / cost_n (one correctly rounded division); the pair is admissible iff cost_n >= min_joints, the mean is
//      not NaN and -inf < mean <= gate2; every other pair costs +inf.
//   2. a[P][Pmax + P]: the means, then one private dummy column per person that costs gate2 (staying unmatched).
//   3. The shortest-augmenting-path method in its textbook form: rows inserted in order, duals u (rows), v (columns), minv, way; per
//      step cur = (a[i0][j] - u[i0]) - v[j] on every column outside the tree, minv[j] = cur where cur < minv[j], then delta = the
//      smallest minv outside the tree and its LOWEST column; u of the tree's rows += delta, v of its columns -= delta, every other
//      minv -= delta.  Additions, subtractions and comparisons only: nothing can contract into a fused multiply-add.
//   4. det_of, person_of, total = the means of the matched pairs added in increasing p.
//
// A LANE IS A COLUMN.  It holds v[j], minv[j], way[j], used[j], the row matched to column j and that row's u, all in registers; the
// row under insertion and its u are uniform over the problem's lanes.  delta and its column come from an xor butterfly over the
// lanes on the pair (minv, column) -- the minimum of a totally ordered pair is exact in any order, so the kernel's choice is the
// serial scan's.  What a step reads of another lane (the row of column j0 and its u; the chain of `way` during augmentation) comes
// through __shfl: no LDS round trip, no array with a dynamic index.  The butterfly is written with the generic __shfl_xor on the
// double and the int of the pair at every distance; which of them the compiler turns into DPP row operations (the distances below
// 16 stay inside a row of 16 lanes) and which into ds_bpermute_b32 was left to it and not inspected: at a few per cent of the kernel
// that feeds it (EXPERIMENTS.md, round 27) the choice was not worth hand-written cross-lane code.
// The problems of one call share P and Pmax, so W = the smallest of 8, 16, 32, 64 that holds the P + Pmax columns is a template
// parameter, a wave carries 64 / W problems side by side, and every cross-lane operation stays inside an aligned group of W lanes
// (xor distances below W, __shfl sources base + column).  The groups of a wave run their own trip counts: each loop turns while ANY
// group of the wave still has work, and a group that is done sits behind its own predicate with its registers untouched -- so a
// problem's bits depend on its own costs, gate2 and min_joints alone, not on its neighbours in the wave.
// The means are formed once per entry, in a coalesced pass over the wave's 64 / W consecutive problems, and kept in LDS (at most
// 16 W doubles per wave: P Pmax <= W^2 / 4): row i0 of a step is a dynamic row, lane j reads mean[i0][j], consecutive lanes
// consecutive words.
#pragma once
#include "snowtri_kernels.hpp"

namespace snowtri {

constexpr int kAssignWaves = 4;        // waves per workgroup of k_assign, each with its own problems
constexpr int kAssignMaxColumns = 64;  // P + Pmax: the columns of a problem are the lanes of (a part of) one wave
constexpr double kAssignMaxGate = 1e150;   // gate_px: gate2 <= 1e300 keeps the dummies' cost and the duals summed from it finite

template <int W>
__global__ __launch_bounds__(64 * kAssignWaves) void k_assign(int64_t n, int P, int Pmax, double gate2, int min_joints,
                                                              const double *__restrict__ cost_sum, const int32_t *__restrict__ cost_n,
                                                              int32_t *__restrict__ det_of, int32_t *__restrict__ person_of,
                                                              double *__restrict__ total) {
    static_assert(W == 8 || W == 16 || W == 32 || W == 64, "a sub-wave of 8, 16, 32 or 64 lanes");
    constexpr int kPer = 64 / W;                        // problems per wave
    constexpr int kMeanCap = kPer * (W / 2) * (W / 2);  // P + Pmax <= W: P * Pmax <= W^2 / 4
    __shared__ double s_mean[kAssignWaves][kMeanCap];
    __shared__ int s_det[kAssignWaves][64];
    const double inf = __builtin_huge_val();
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int j = lane & (W - 1), base = lane - j, sub = lane / W;      // my column, my group's first lane, my group
    const int64_t first = (blockIdx.x * (int64_t)kAssignWaves + wave) * kPer;   // the wave's first problem
    const int64_t prob = first + sub;
    const bool live = prob < n;
    const int PQ = P * Pmax, ncols = Pmax + P;
    SNOWTRI_DEV_CHECK(P >= 1 && Pmax >= 1 && ncols <= W && kPer * PQ <= kMeanCap, 97);
    double *sm = s_mean[wave];
    int *sd = s_det[wave];

    // the means of the wave's problems: consecutive in memory, read once, coalesced
    const int64_t left = n - first;
    const int n_ent = (left >= kPer ? kPer : left > 0 ? (int)left : 0) * PQ;
    for (int e = lane; e < n_ent; e += 64) {
        const int64_t g = first * PQ + e;
        const double cs = cost_sum[g];
        const int32_t cn = cost_n[g];
        const double mean = cs / (double)cn;
        const bool ok = cn >= min_joints && mean == mean && mean <= gate2 && mean > -inf;
        sm[e] = ok ? mean : inf;
    }
    sd[lane] = -1;   // (a row that ends without a column -- unreachable with a finite gate2 -- reads as unmatched, never as stale LDS)
    __syncthreads();
    const double *row0 = sm + sub * PQ;

    const bool col = live && j < ncols;
    double v = 0.0, uj = 0.0;   // v[j]; u of the row matched to column j
    int pj = -1;                // the row matched to column j
    for (int i = 0; i < P; i++) {
        double ui = 0.0, minv = inf;   // u of row i (uniform over the group)
        int way = -1, j0 = -1;         // -1: the virtual column that holds row i
        bool used = false;
        int i0 = i;
        double u0 = 0.0;
        bool run = live;
        while (__any(run)) {
            if (run && j == j0) used = true;
            double key = inf;
            int kcol = W;
            if (run && col && !used) {
                const double a = j < Pmax ? row0[i0 * Pmax + j] : (j - Pmax == i0 ? gate2 : inf);
                const double cur = (a - u0) - v;
                if (cur < minv) {
                    minv = cur;
                    way = j0;
                }
                key = minv;
                kcol = j;
            }
#pragma unroll
            for (int w = W / 2; w >= 1; w >>= 1) {   // the least (minv, column) of the group, in every lane of it
                const double ok = __shfl_xor(key, w, 64);
                const int oc = __shfl_xor(kcol, w, 64);
                if (ok < key || (ok == key && oc < kcol)) {
                    key = ok;
                    kcol = oc;
                }
            }
            if (run && !(key < inf)) {   // (no finite column outside the tree: unreachable, row i's own dummy at the finite gate2
                run = false;             // is one -- the entry refuses an infinite gate2; the row is then left unmatched)
                j0 = -1;
            }
            if (run) {
                const double delta = key;
                if (used) {
                    uj += delta;
                    v -= delta;
                } else {
                    minv -= delta;
                }
                ui += delta;
                j0 = kcol;
            }
            const int src = base + (j0 & (W - 1));
            const int p0 = __shfl(pj, src, 64);
            const double up0 = __shfl(uj, src, 64);
            if (run) {
                if (p0 < 0) {
                    run = false;   // a free column: the path ends at j0
                } else {
                    i0 = p0;
                    u0 = up0;
                }
            }
        }
        // augment: every column of the path takes the row of the column before it, the first takes row i
        bool aug = live && j0 >= 0;
        while (__any(aug)) {
            const int wj = __shfl(way, base + (j0 & (W - 1)), 64);
            const int src = base + (wj & (W - 1));
            int prow = __shfl(pj, src, 64);
            double pu = __shfl(uj, src, 64);
            if (aug) {
                if (wj < 0) {
                    prow = i;
                    pu = ui;
                }
                if (j == j0) {
                    pj = prow;
                    uj = pu;
                }
                j0 = wj;
                aug = wj >= 0;
            }
        }
    }

    if (col && pj >= 0) sd[base + pj] = j < Pmax ? j : -1;   // every row sits on exactly one column
    __syncthreads();
    const bool rowlane = live && j < P;
    const int d = rowlane ? sd[base + j] : -1;
    if (rowlane) det_of[prob * P + j] = d;
    if (person_of && live && j < Pmax) person_of[prob * Pmax + j] = pj;
    if (total) {
        const bool has = rowlane && d >= 0;
        const double m = has ? row0[j * Pmax + d] : 0.0;
        double t = 0.0;
        for (int p = 0; p < P; p++) {   // in increasing p, plain additions
            const double mp = __shfl(m, base + p, 64);
            const int hp = __shfl((int)has, base + p, 64);
            if (hp) t += mp;
        }
        if (live && j == 0) total[prob] = t;
    }
}

}  // namespace snowtri
