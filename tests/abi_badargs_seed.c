/* Drives snowtri_pair_cost and snowtri_seed_persons with invalid arguments: the C ABI must report, never crash or read through a bad
 * pointer.  Plain C99, its own main.
 *
 *   - without a GPU (tests/test_seed_host.py builds it against the AddressSanitizer build of the library, `make asan`): a null
 *     context, with good and with bad other arguments, and every refusal of snowtri_seed_persons that needs no context;
 *   - with a GPU (tests/test_gpu_seed.py runs it against libsnowtri.so): the same plus, on real contexts, every refusal that comes
 *     before a launch -- sizes, dtype codes, memory spaces, a NaN threshold, 1 and 9 cameras, kn past 256, the gate, min_joints,
 *     min_views, S, C * Pmax past 64, missing and misaligned pointers, a batch past the size limits -- the empty batch, and one
 *     good call of each entry.
 * Exit code = number of failed expectations; prints each failure.
 */
#include <math.h>
#include <stdint.h>
#include <stdio.h>
#include <string.h>

#include "snowtri.h"

static int failures = 0;
#define EXPECT(call, want)                                                                    \
    do {                                                                                      \
        long long got_ = (long long)(call);                                                   \
        if (got_ != (long long)(want)) {                                                      \
            printf("FAIL %s:%d  %s  -> %lld, expected %lld\n", __FILE__, __LINE__, #call, got_, (long long)(want)); \
            failures++;                                                                       \
        }                                                                                     \
    } while (0)
#define SAYS(word) EXPECT(snowtri_last_error() != NULL && strstr(snowtri_last_error(), word) != NULL, 1)

enum { F = 2, J = 9, PM = 2, C = 4, NP = 6, S = 3, NC = F * NP * PM * PM };

int main(void) {
    static double kp[F * C * PM * J * 3 + 3], ps[NC + 1];
    static int32_t pn[NC + 1], np[F * C + 1], cl[F * C * PM + 1], det[F * C * S + 1], ns[F + 1];
    static uint32_t fl[F + 1];
    volatile double zero = 0.0;
    const double nan = zero / zero;
    int i;
    for (i = 0; i < F * C; i++) np[i] = PM;
    for (i = 0; i < F * C * PM; i++) cl[i] = -1;

#define COST(ctx_, F_, J_, Pm_, k_, kdt_, np_, cl_, thr_, ps_, pn_, ms_) \
    snowtri_pair_cost(ctx_, F_, J_, Pm_, k_, kdt_, np_, cl_, thr_, ps_, pn_, ms_, NULL)
#define GOODC(ctx_) COST(ctx_, F, J, PM, kp, SNOWTRI_F64, np, cl, 0.5, ps, pn, SNOWTRI_HOST)
#define SEED(ctx_, F_, Pm_, ps_, pn_, np_, cl_, g_, mj_, mv_, S_, d_, ns_, fl_, ms_) \
    snowtri_seed_persons(ctx_, F_, Pm_, ps_, pn_, np_, cl_, g_, mj_, mv_, S_, d_, ns_, fl_, ms_, NULL)
#define GOODS(ctx_) SEED(ctx_, F, PM, ps, pn, np, cl, 0.05, 8, 3, S, det, ns, fl, SNOWTRI_HOST)
    /* ---- null context ---------------------------------------------------------------------------------------- */
    EXPECT(GOODC(NULL), SNOWTRI_ERR_BAD_ARG);
    SAYS("snowtri_pair_cost: null context");
    EXPECT(COST(NULL, 0, J, PM, NULL, SNOWTRI_F64, NULL, NULL, 0.5, NULL, NULL, SNOWTRI_HOST), SNOWTRI_ERR_BAD_ARG);
    EXPECT(COST(NULL, -1, 0, 0, NULL, 9, NULL, NULL, nan, NULL, NULL, 7), SNOWTRI_ERR_BAD_ARG);
    EXPECT(GOODS(NULL), SNOWTRI_ERR_BAD_ARG);
    SAYS("snowtri_seed_persons: null context");
    EXPECT(SEED(NULL, 0, PM, NULL, NULL, NULL, NULL, 0.05, 8, 3, S, NULL, NULL, NULL, SNOWTRI_HOST), SNOWTRI_ERR_BAD_ARG);
    /* the refusals of snowtri_seed_persons that name their argument with or without a context */
    EXPECT(SEED(NULL, F, PM, ps, pn, np, cl, 0.05, 8, 3, S, det, ns, fl, 5), SNOWTRI_ERR_BAD_ARG);
    SAYS("memspace");
    EXPECT(SEED(NULL, -1, PM, ps, pn, np, cl, 0.05, 8, 3, S, det, ns, fl, SNOWTRI_HOST), SNOWTRI_ERR_BAD_ARG);
    SAYS("F < 0");
    EXPECT(SEED(NULL, F, 0, ps, pn, np, cl, 0.05, 8, 3, S, det, ns, fl, SNOWTRI_HOST), SNOWTRI_ERR_BAD_ARG);
    SAYS("Pmax");
    EXPECT(SEED(NULL, F, PM, ps, pn, np, cl, 0.05, 8, 3, 0, det, ns, fl, SNOWTRI_HOST), SNOWTRI_ERR_BAD_ARG);
    EXPECT(SEED(NULL, F, PM, ps, pn, np, cl, 0.05, 8, 3, 65, det, ns, fl, SNOWTRI_HOST), SNOWTRI_ERR_BAD_ARG);
    SAYS("S must lie in 1..64");
    EXPECT(SEED(NULL, F, PM, ps, pn, np, cl, 0.05, 0, 3, S, det, ns, fl, SNOWTRI_HOST), SNOWTRI_ERR_BAD_ARG);
    SAYS("min_joints");
    EXPECT(SEED(NULL, F, PM, ps, pn, np, cl, -0.05, 8, 3, S, det, ns, fl, SNOWTRI_HOST), SNOWTRI_ERR_BAD_ARG);
    EXPECT(SEED(NULL, F, PM, ps, pn, np, cl, nan, 8, 3, S, det, ns, fl, SNOWTRI_HOST), SNOWTRI_ERR_BAD_ARG);
    SAYS("gate must be >= 0");
    EXPECT(SEED(NULL, F, PM, ps, pn, np, cl, 1.0000001e150, 8, 3, S, det, ns, fl, SNOWTRI_HOST), SNOWTRI_ERR_BAD_ARG);
    EXPECT(SEED(NULL, F, PM, ps, pn, np, cl, 1.0 / zero, 8, 3, S, det, ns, fl, SNOWTRI_HOST), SNOWTRI_ERR_BAD_ARG);
    SAYS("gate must not exceed 1e150");

    /* ---- real contexts (GPU box only) -------------------------------------------------------------------------- */
    if (snowtri_device_count() > 0) {
        snowtri_ctx *ctx = NULL, *one = NULL, *nine = NULL;
        static double K[9 * 9], R[9 * 9], t[9 * 3];
        int c, f, p, j;
        for (c = 0; c < 9; c++) {
            const double k[9] = {700, 0.5, 640, 0, 700, 360, 0, 0, 1}, r[9] = {1, 0, 0, 0, 1, 0, 0, 0, 1};
            memcpy(K + 9 * c, k, sizeof k);
            memcpy(R + 9 * c, r, sizeof r);
            t[3 * c] = 0.5 * c;
            t[3 * c + 1] = 0.1 * c + 0.03 * c * c;           /* (no two baselines parallel: no wrong pair of lines is coplanar) */
            t[3 * c + 2] = 0.02 * c;
        }
        /* detection q of every camera shows the points (1.0 q + 0.05 j, 0.3, 4): exact pixels */
        for (f = 0; f < F; f++)
            for (c = 0; c < C; c++)
                for (p = 0; p < PM; p++)
                    for (j = 0; j < J; j++) {
                        double *o = kp + 3 * (((f * C + c) * PM + p) * J + j);
                        const double pz = 4.0 - t[3 * c + 2], px = (1.0 * p + 0.05 * j - t[3 * c]) / pz, py = (0.3 - t[3 * c + 1]) / pz;
                        o[0] = 700 * px + 0.5 * py + 640;
                        o[1] = 700 * py + 360;
                        o[2] = 1.0;
                    }
        EXPECT(snowtri_ctx_create(4, K, R, t, 0, &ctx), SNOWTRI_OK);
        EXPECT(snowtri_ctx_create(1, K, R, t, 0, &one), SNOWTRI_OK);
        EXPECT(snowtri_ctx_create(9, K, R, t, 0, &nine), SNOWTRI_OK);
        memset(ps, 0, sizeof ps);
        memset(pn, 0, sizeof pn);
        memset(det, 0, sizeof det);
        memset(ns, 0, sizeof ns);
        memset(fl, 0, sizeof fl);
        /* snowtri_pair_cost */
        EXPECT(GOODC(one), SNOWTRI_ERR_BAD_ARG);
        SAYS("2 to 8 cameras");
        EXPECT(GOODC(nine), SNOWTRI_ERR_BAD_ARG);
        SAYS("2 to 8 cameras");
        EXPECT(COST(ctx, -1, J, PM, kp, SNOWTRI_F64, np, cl, 0.5, ps, pn, SNOWTRI_HOST), SNOWTRI_ERR_BAD_ARG);
        EXPECT(COST(ctx, F, 0, PM, kp, SNOWTRI_F64, np, cl, 0.5, ps, pn, SNOWTRI_HOST), SNOWTRI_ERR_BAD_ARG);
        SAYS("kn < 1");
        EXPECT(COST(ctx, F, J, 0, kp, SNOWTRI_F64, np, cl, 0.5, ps, pn, SNOWTRI_HOST), SNOWTRI_ERR_BAD_ARG);
        SAYS("Pmax");
        EXPECT(COST(ctx, F, 257, PM, kp, SNOWTRI_F64, np, cl, 0.5, ps, pn, SNOWTRI_HOST), SNOWTRI_ERR_BAD_ARG);
        SAYS("256 joints");
        EXPECT(COST(ctx, F, J, PM, kp, 7, np, cl, 0.5, ps, pn, SNOWTRI_HOST), SNOWTRI_ERR_BAD_ARG);
        SAYS("dtype");
        EXPECT(COST(ctx, F, J, PM, kp, SNOWTRI_F64, np, cl, 0.5, ps, pn, 5), SNOWTRI_ERR_BAD_ARG);
        SAYS("memspace");
        EXPECT(COST(ctx, F, J, PM, kp, SNOWTRI_F64, np, cl, nan, ps, pn, SNOWTRI_HOST), SNOWTRI_ERR_BAD_ARG);
        SAYS("keypoint_score_threshold");
        EXPECT(COST(ctx, 0, J, PM, NULL, SNOWTRI_F64, NULL, NULL, nan, NULL, NULL, SNOWTRI_HOST), SNOWTRI_ERR_BAD_ARG);   /* ... even on an empty batch */
        EXPECT(COST(ctx, F, J, PM, NULL, SNOWTRI_F64, np, cl, 0.5, ps, pn, SNOWTRI_HOST), SNOWTRI_ERR_BAD_ARG);
        EXPECT(COST(ctx, F, J, PM, kp, SNOWTRI_F64, np, cl, 0.5, NULL, pn, SNOWTRI_HOST), SNOWTRI_ERR_BAD_ARG);
        EXPECT(COST(ctx, F, J, PM, kp, SNOWTRI_F64, np, cl, 0.5, ps, NULL, SNOWTRI_HOST), SNOWTRI_ERR_BAD_ARG);
        SAYS("null array");
        EXPECT(COST(ctx, F, J, PM, (char *)kp + 4, SNOWTRI_F64, np, cl, 0.5, ps, pn, SNOWTRI_DEVICE), SNOWTRI_ERR_BAD_ARG);
        EXPECT(COST(ctx, F, J, PM, kp, SNOWTRI_F64, (int32_t *)((char *)np + 1), cl, 0.5, ps, pn, SNOWTRI_DEVICE), SNOWTRI_ERR_BAD_ARG);
        EXPECT(COST(ctx, F, J, PM, kp, SNOWTRI_F64, np, (int32_t *)((char *)cl + 2), 0.5, ps, pn, SNOWTRI_DEVICE), SNOWTRI_ERR_BAD_ARG);
        EXPECT(COST(ctx, F, J, PM, kp, SNOWTRI_F64, np, cl, 0.5, (double *)((char *)ps + 4), pn, SNOWTRI_DEVICE), SNOWTRI_ERR_BAD_ARG);
        EXPECT(COST(ctx, F, J, PM, kp, SNOWTRI_F64, np, cl, 0.5, ps, (int32_t *)((char *)pn + 2), SNOWTRI_DEVICE), SNOWTRI_ERR_BAD_ARG);
        SAYS("aligned");
        EXPECT(COST(ctx, ((int64_t)1 << 40), J, PM, kp, SNOWTRI_F64, np, cl, 0.5, ps, pn, SNOWTRI_HOST), SNOWTRI_ERR_BAD_ARG);
        SAYS("workgroups");
        EXPECT(COST(ctx, ((int64_t)1 << 28), J, 1 << 14, kp, SNOWTRI_F64, np, cl, 0.5, ps, pn, SNOWTRI_HOST), SNOWTRI_ERR_BAD_ARG);
        SAYS("2^48");
        EXPECT(COST(ctx, 0, J, PM, NULL, SNOWTRI_F64, NULL, NULL, 0.5, NULL, NULL, SNOWTRI_HOST), SNOWTRI_OK);           /* empty batch: no pointer is looked at */
        EXPECT(COST(ctx, 0, J, PM, NULL, SNOWTRI_F32, NULL, NULL, 0.5, NULL, NULL, SNOWTRI_DEVICE), SNOWTRI_OK);
        /* snowtri_seed_persons */
        EXPECT(GOODS(one), SNOWTRI_ERR_BAD_ARG);
        SAYS("at least 2 cameras");
        EXPECT(SEED(ctx, F, 17, ps, pn, np, cl, 0.05, 8, 3, S, det, ns, fl, SNOWTRI_HOST), SNOWTRI_ERR_BAD_ARG);       /* 4 x 17 nodes */
        SAYS("C * Pmax must not exceed 64");
        EXPECT(SEED(nine, F, 8, ps, pn, np, cl, 0.05, 8, 3, S, det, ns, fl, SNOWTRI_HOST), SNOWTRI_ERR_BAD_ARG);      /* 9 x 8 nodes */
        SAYS("C * Pmax must not exceed 64");
        EXPECT(SEED(ctx, F, PM, ps, pn, np, cl, 0.05, 8, 1, S, det, ns, fl, SNOWTRI_HOST), SNOWTRI_ERR_BAD_ARG);
        EXPECT(SEED(ctx, F, PM, ps, pn, np, cl, 0.05, 8, 5, S, det, ns, fl, SNOWTRI_HOST), SNOWTRI_ERR_BAD_ARG);
        SAYS("min_views must lie in 2..C");
        EXPECT(SEED(ctx, F, PM, ps, pn, np, cl, 0.05, 0, 3, S, det, ns, fl, SNOWTRI_HOST), SNOWTRI_ERR_BAD_ARG);
        SAYS("min_joints");
        EXPECT(SEED(ctx, F, PM, ps, pn, np, cl, nan, 8, 3, S, det, ns, fl, SNOWTRI_HOST), SNOWTRI_ERR_BAD_ARG);
        EXPECT(SEED(ctx, F, PM, ps, pn, np, cl, -1.0, 8, 3, S, det, ns, fl, SNOWTRI_HOST), SNOWTRI_ERR_BAD_ARG);
        SAYS("gate must be >= 0");
        EXPECT(SEED(ctx, F, PM, ps, pn, np, cl, 1e200, 8, 3, S, det, ns, fl, SNOWTRI_HOST), SNOWTRI_ERR_BAD_ARG);
        SAYS("1e150");
        EXPECT(SEED(ctx, F, PM, ps, pn, np, cl, 0.05, 8, 3, 65, det, ns, fl, SNOWTRI_HOST), SNOWTRI_ERR_BAD_ARG);
        SAYS("S must lie");
        EXPECT(SEED(ctx, 0, PM, NULL, NULL, NULL, NULL, 0.05, 8, 5, S, NULL, NULL, NULL, SNOWTRI_HOST), SNOWTRI_ERR_BAD_ARG);   /* ... even on an empty batch */
        EXPECT(SEED(ctx, F, PM, NULL, pn, np, cl, 0.05, 8, 3, S, det, ns, fl, SNOWTRI_HOST), SNOWTRI_ERR_BAD_ARG);
        EXPECT(SEED(ctx, F, PM, ps, NULL, np, cl, 0.05, 8, 3, S, det, ns, fl, SNOWTRI_HOST), SNOWTRI_ERR_BAD_ARG);
        EXPECT(SEED(ctx, F, PM, ps, pn, np, cl, 0.05, 8, 3, S, NULL, ns, fl, SNOWTRI_HOST), SNOWTRI_ERR_BAD_ARG);
        EXPECT(SEED(ctx, F, PM, ps, pn, np, cl, 0.05, 8, 3, S, det, NULL, fl, SNOWTRI_HOST), SNOWTRI_ERR_BAD_ARG);
        SAYS("null array");
        EXPECT(SEED(ctx, F, PM, (double *)((char *)ps + 4), pn, np, cl, 0.05, 8, 3, S, det, ns, fl, SNOWTRI_DEVICE), SNOWTRI_ERR_BAD_ARG);
        EXPECT(SEED(ctx, F, PM, ps, (int32_t *)((char *)pn + 2), np, cl, 0.05, 8, 3, S, det, ns, fl, SNOWTRI_DEVICE), SNOWTRI_ERR_BAD_ARG);
        EXPECT(SEED(ctx, F, PM, ps, pn, (int32_t *)((char *)np + 1), cl, 0.05, 8, 3, S, det, ns, fl, SNOWTRI_DEVICE), SNOWTRI_ERR_BAD_ARG);
        EXPECT(SEED(ctx, F, PM, ps, pn, np, (int32_t *)((char *)cl + 2), 0.05, 8, 3, S, det, ns, fl, SNOWTRI_DEVICE), SNOWTRI_ERR_BAD_ARG);
        EXPECT(SEED(ctx, F, PM, ps, pn, np, cl, 0.05, 8, 3, S, (int32_t *)((char *)det + 2), ns, fl, SNOWTRI_DEVICE), SNOWTRI_ERR_BAD_ARG);
        EXPECT(SEED(ctx, F, PM, ps, pn, np, cl, 0.05, 8, 3, S, det, (int32_t *)((char *)ns + 1), fl, SNOWTRI_DEVICE), SNOWTRI_ERR_BAD_ARG);
        EXPECT(SEED(ctx, F, PM, ps, pn, np, cl, 0.05, 8, 3, S, det, ns, (uint32_t *)((char *)fl + 2), SNOWTRI_DEVICE), SNOWTRI_ERR_BAD_ARG);
        SAYS("aligned");
        EXPECT(SEED(ctx, ((int64_t)1 << 31), PM, ps, pn, np, cl, 0.05, 8, 3, S, det, ns, fl, SNOWTRI_HOST), SNOWTRI_ERR_BAD_ARG);
        SAYS("2^31");
        EXPECT(SEED(ctx, 0, PM, NULL, NULL, NULL, NULL, 0.05, 8, 3, S, NULL, NULL, NULL, SNOWTRI_HOST), SNOWTRI_OK);    /* empty batch: no pointer is looked at */
        EXPECT(SEED(ctx, 0, PM, NULL, NULL, NULL, NULL, 0.05, 8, 3, S, NULL, NULL, NULL, SNOWTRI_DEVICE), SNOWTRI_OK);
        for (i = 0; i < NC; i++) failures += ps[i] != 0.0 || pn[i] != 0;                      /* nothing was written */
        for (i = 0; i < F * C * S; i++) failures += det[i] != 0;
        for (i = 0; i < F; i++) failures += ns[i] != 0 || fl[i] != 0u;
        /* one good call of each, so that the refusals above are refusals of their argument and not of everything: exact pixels give
         * line distances of rounding size between the detections of one person and of centimetres to a metre between those of two */
        EXPECT(GOODC(ctx), SNOWTRI_OK);
        for (f = 0; f < F; f++)
            for (c = 0; c < NP; c++)
                for (p = 0; p < PM; p++) {
                    i = ((f * NP + c) * PM + p) * PM + p;
                    EXPECT(pn[i], J);
                    EXPECT(ps[i] >= 0.0 && ps[i] < 1e-18, 1);
                }
        EXPECT(GOODS(ctx), SNOWTRI_OK);
        for (f = 0; f < F; f++) {
            EXPECT(ns[f], 2);
            EXPECT(fl[f], 0u);
            const int first = det[(f * C) * S];                    /* (which person's rounding is smaller decides the order) */
            EXPECT(first == 0 || first == 1, 1);
            for (c = 0; c < C; c++) {
                EXPECT(det[(f * C + c) * S + 0], first);
                EXPECT(det[(f * C + c) * S + 1], 1 - first);
                EXPECT(det[(f * C + c) * S + 2], -1);
            }
        }
        EXPECT(snowtri_ctx_destroy(ctx), SNOWTRI_OK);
        EXPECT(snowtri_ctx_destroy(one), SNOWTRI_OK);
        EXPECT(snowtri_ctx_destroy(nine), SNOWTRI_OK);
    }
    printf("abi_badargs_seed: %d failure(s)\n", failures);
    return failures;
}
