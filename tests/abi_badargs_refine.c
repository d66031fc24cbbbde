/* Drives snowtri_refine_joints with invalid arguments: the C ABI must report, never crash or read through a bad pointer.  Plain C99,
 * its own main (tests/abi_badargs_reproject.c covers the reprojection entries).
 *
 *   - without a GPU (tests/test_refine_host.py builds it against the AddressSanitizer build of the library, `make asan`): a null
 *     context, with good and with bad other arguments;
 *   - with a GPU (tests/test_gpu_refine.py runs it against libsnowtri.so): the same plus, on real contexts, every refusal that comes
 *     before a launch -- sizes, dtype codes, memory spaces, flag bits, iters, a K of the wrong form, a NaN threshold, more than 32
 *     cameras, P > Pmax without det_of, missing and misaligned pointers, an output that overlaps the input other than exactly, a
 *     batch past the size limit -- the empty batch, and one good call out of place and one in place.
 * Exit code = number of failed expectations; prints each failure.
 */
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

enum { F = 2, P = 2, J = 5, PM = 3, C = 4, N = F * P * J };

int main(void) {
    static double xyz[N * 4 + 4], out[N * 4 + 4], kp[F * C * PM * J * 3], cost[N * 2];
    static uint8_t codes[N];
    static int32_t np[F * C], det[F * C * P];
    static uint32_t views[N];
    const uint32_t SW = SNOWTRI_REFINE_SCORE_WEIGHTS;
    volatile double zero = 0.0;
    const double nan = zero / zero;
    int i;
    for (i = 0; i < N; i++) {
        xyz[4 * i] = 0.1 * (i % 7);
        xyz[4 * i + 1] = 0.3;
        xyz[4 * i + 2] = 4.0;
        xyz[4 * i + 3] = 1.0;
        views[i] = 0xfu;
    }
    for (i = 0; i < F * C; i++) np[i] = PM;
    for (i = 0; i < F * C * P; i++) det[i] = i % P;

#define REFINE(ctx_, F_, P_, J_, x_, xdt_, Pm_, k_, kdt_, np_, det_, vw_, thr_, it_, fl_, o_, c_, cd_, ms_) \
    snowtri_refine_joints(ctx_, F_, P_, J_, x_, xdt_, Pm_, k_, kdt_, np_, det_, vw_, thr_, it_, fl_, o_, c_, cd_, ms_, NULL)
#define GOOD(ctx_) REFINE(ctx_, F, P, J, xyz, SNOWTRI_F64, PM, kp, SNOWTRI_F64, np, det, views, 0.5, 4, 0u, out, cost, codes, SNOWTRI_HOST)
    /* ---- null context ---------------------------------------------------------------------------------------- */
    EXPECT(GOOD(NULL), SNOWTRI_ERR_BAD_ARG);
    EXPECT(REFINE(NULL, 0, P, J, NULL, SNOWTRI_F64, PM, NULL, SNOWTRI_F64, NULL, NULL, NULL, 0.5, 4, 0u, NULL, NULL, NULL, SNOWTRI_HOST), SNOWTRI_ERR_BAD_ARG);
    EXPECT(REFINE(NULL, -1, 0, 0, NULL, 9, 0, NULL, -1, NULL, NULL, NULL, nan, 0, 8u, NULL, NULL, NULL, 7), SNOWTRI_ERR_BAD_ARG);
    EXPECT(snowtri_last_error() != NULL && strstr(snowtri_last_error(), "snowtri_refine_joints") != NULL, 1);

    /* ---- real contexts (GPU box only) -------------------------------------------------------------------------- */
    if (snowtri_device_count() > 0) {
        snowtri_ctx *ctx = NULL, *none = NULL, *odd = NULL, *wide = NULL;
        static double K[33 * 9], R[33 * 9], t[33 * 3];
        double Kodd[9] = {700, 0, 640, 0.001, 700, 360, 0, 0, 1};
        int c, f, p, j;
        for (c = 0; c < 33; c++) {
            const double k[9] = {700, 0.5, 640, 0, 700, 360, 0, 0, 1}, r[9] = {1, 0, 0, 0, 1, 0, 0, 0, 1};
            memcpy(K + 9 * c, k, sizeof k);
            memcpy(R + 9 * c, r, sizeof r);
            t[3 * c] = 0.5 * c;
            t[3 * c + 1] = 0.1 * (c % 3);
            t[3 * c + 2] = 0.0;
        }
        /* detection q of camera c shows person q: the exact pixel of the record plus a pixel or two */
        for (f = 0; f < F; f++)
            for (c = 0; c < C; c++)
                for (p = 0; p < PM; p++)
                    for (j = 0; j < J; j++) {
                        const double *x = xyz + 4 * ((f * P + (p % P)) * J + j);
                        double *o = kp + 3 * (((f * C + c) * PM + p) * J + j);
                        const double px = (x[0] - t[3 * c]) / x[2], py = (x[1] - t[3 * c + 1]) / x[2];
                        o[0] = 700 * px + 0.5 * py + 640 + ((c + j) % 3 - 1) * 1.5;
                        o[1] = 700 * py + 360 + ((c + 2 * j) % 3 - 1) * 1.0;
                        o[2] = 1.0;
                    }
        EXPECT(snowtri_ctx_create(4, K, R, t, 0, &ctx), SNOWTRI_OK);
        EXPECT(snowtri_ctx_create(0, NULL, NULL, NULL, 0, &none), SNOWTRI_OK);
        EXPECT(snowtri_ctx_create(1, Kodd, R, t, 0, &odd), SNOWTRI_OK);
        EXPECT(snowtri_ctx_create(33, K, R, t, 0, &wide), SNOWTRI_OK);
        memset(out, 0, sizeof out);
        memset(cost, 0, sizeof cost);
        memset(codes, 0, sizeof codes);
        EXPECT(GOOD(none), SNOWTRI_ERR_BAD_ARG);                                              /* no cameras */
        EXPECT(GOOD(odd), SNOWTRI_ERR_BAD_ARG);                                               /* K is not the pinhole form */
        EXPECT(strstr(snowtri_last_error(), "[[fx, s, cx]") != NULL, 1);
        EXPECT(GOOD(wide), SNOWTRI_ERR_BAD_ARG);                                              /* 33 cameras */
        EXPECT(strstr(snowtri_last_error(), "32") != NULL, 1);
        EXPECT(REFINE(ctx, -1, P, J, xyz, SNOWTRI_F64, PM, kp, SNOWTRI_F64, np, det, views, 0.5, 4, 0u, out, cost, codes, SNOWTRI_HOST), SNOWTRI_ERR_BAD_ARG);
        EXPECT(REFINE(ctx, F, 0, J, xyz, SNOWTRI_F64, PM, kp, SNOWTRI_F64, np, det, views, 0.5, 4, 0u, out, cost, codes, SNOWTRI_HOST), SNOWTRI_ERR_BAD_ARG);
        EXPECT(REFINE(ctx, F, P, 0, xyz, SNOWTRI_F64, PM, kp, SNOWTRI_F64, np, det, views, 0.5, 4, 0u, out, cost, codes, SNOWTRI_HOST), SNOWTRI_ERR_BAD_ARG);
        EXPECT(REFINE(ctx, F, P, J, xyz, SNOWTRI_F64, 0, kp, SNOWTRI_F64, np, det, views, 0.5, 4, 0u, out, cost, codes, SNOWTRI_HOST), SNOWTRI_ERR_BAD_ARG);
        EXPECT(REFINE(ctx, F, P, J, xyz, 7, PM, kp, SNOWTRI_F64, np, det, views, 0.5, 4, 0u, out, cost, codes, SNOWTRI_HOST), SNOWTRI_ERR_BAD_ARG);
        EXPECT(REFINE(ctx, F, P, J, xyz, SNOWTRI_F64, PM, kp, 2, np, det, views, 0.5, 4, 0u, out, cost, codes, SNOWTRI_HOST), SNOWTRI_ERR_BAD_ARG);
        EXPECT(REFINE(ctx, F, P, J, xyz, SNOWTRI_F64, PM, kp, SNOWTRI_F64, np, det, views, 0.5, 4, 0u, out, cost, codes, 5), SNOWTRI_ERR_BAD_ARG);
        EXPECT(REFINE(ctx, F, P, J, xyz, SNOWTRI_F64, PM, kp, SNOWTRI_F64, np, det, views, 0.5, 4, 2u, out, cost, codes, SNOWTRI_HOST), SNOWTRI_ERR_BAD_ARG);   /* an unknown flag bit */
        EXPECT(strstr(snowtri_last_error(), "flag") != NULL, 1);
        EXPECT(REFINE(ctx, F, P, J, xyz, SNOWTRI_F64, PM, kp, SNOWTRI_F64, np, det, views, nan, 4, 0u, out, cost, codes, SNOWTRI_HOST), SNOWTRI_ERR_BAD_ARG);
        EXPECT(REFINE(ctx, F, P, J, xyz, SNOWTRI_F64, PM, kp, SNOWTRI_F64, np, det, views, 0.5, 0, 0u, out, cost, codes, SNOWTRI_HOST), SNOWTRI_ERR_BAD_ARG);
        EXPECT(REFINE(ctx, F, P, J, xyz, SNOWTRI_F64, PM, kp, SNOWTRI_F64, np, det, views, 0.5, 17, 0u, out, cost, codes, SNOWTRI_HOST), SNOWTRI_ERR_BAD_ARG);
        EXPECT(strstr(snowtri_last_error(), "iters") != NULL, 1);
        EXPECT(REFINE(ctx, 0, P, J, NULL, SNOWTRI_F64, PM, NULL, SNOWTRI_F64, NULL, NULL, NULL, 0.5, 17, 0u, NULL, NULL, NULL, SNOWTRI_HOST), SNOWTRI_ERR_BAD_ARG);   /* ... even on an empty batch */
        EXPECT(REFINE(ctx, F, 4, J, xyz, SNOWTRI_F64, PM, kp, SNOWTRI_F64, np, NULL, views, 0.5, 4, 0u, out, cost, codes, SNOWTRI_HOST), SNOWTRI_ERR_BAD_ARG);   /* P = 4 > Pmax = 3, no det_of */
        EXPECT(strstr(snowtri_last_error(), "det_of") != NULL, 1);
        EXPECT(REFINE(ctx, F, P, J, NULL, SNOWTRI_F64, PM, kp, SNOWTRI_F64, np, det, views, 0.5, 4, 0u, out, cost, codes, SNOWTRI_HOST), SNOWTRI_ERR_BAD_ARG);
        EXPECT(REFINE(ctx, F, P, J, xyz, SNOWTRI_F64, PM, NULL, SNOWTRI_F64, np, det, views, 0.5, 4, 0u, out, cost, codes, SNOWTRI_HOST), SNOWTRI_ERR_BAD_ARG);
        EXPECT(REFINE(ctx, F, P, J, xyz, SNOWTRI_F64, PM, kp, SNOWTRI_F64, np, det, views, 0.5, 4, 0u, NULL, cost, codes, SNOWTRI_HOST), SNOWTRI_ERR_BAD_ARG);
        EXPECT(REFINE(ctx, F, P, J, (char *)xyz + 4, SNOWTRI_F64, PM, kp, SNOWTRI_F64, np, det, views, 0.5, 4, 0u, out, cost, codes, SNOWTRI_DEVICE), SNOWTRI_ERR_BAD_ARG);
        EXPECT(REFINE(ctx, F, P, J, xyz, SNOWTRI_F64, PM, (char *)kp + 2, SNOWTRI_F32, np, det, views, 0.5, 4, 0u, out, cost, codes, SNOWTRI_DEVICE), SNOWTRI_ERR_BAD_ARG);
        EXPECT(REFINE(ctx, F, P, J, xyz, SNOWTRI_F64, PM, kp, SNOWTRI_F64, (int32_t *)((char *)np + 1), det, views, 0.5, 4, 0u, out, cost, codes, SNOWTRI_DEVICE), SNOWTRI_ERR_BAD_ARG);
        EXPECT(REFINE(ctx, F, P, J, xyz, SNOWTRI_F64, PM, kp, SNOWTRI_F64, np, (int32_t *)((char *)det + 2), views, 0.5, 4, 0u, out, cost, codes, SNOWTRI_DEVICE), SNOWTRI_ERR_BAD_ARG);
        EXPECT(REFINE(ctx, F, P, J, xyz, SNOWTRI_F64, PM, kp, SNOWTRI_F64, np, det, (uint32_t *)((char *)views + 2), 0.5, 4, 0u, out, cost, codes, SNOWTRI_DEVICE), SNOWTRI_ERR_BAD_ARG);
        EXPECT(REFINE(ctx, F, P, J, xyz, SNOWTRI_F64, PM, kp, SNOWTRI_F64, np, det, views, 0.5, 4, 0u, out, (double *)((char *)cost + 4), codes, SNOWTRI_DEVICE), SNOWTRI_ERR_BAD_ARG);
        EXPECT(strstr(snowtri_last_error(), "aligned") != NULL, 1);
        /* an output one record into the input, and one record before it */
        EXPECT(REFINE(ctx, F, P, J, xyz, SNOWTRI_F64, PM, kp, SNOWTRI_F64, np, det, views, 0.5, 4, 0u, xyz + 4, cost, codes, SNOWTRI_HOST), SNOWTRI_ERR_BAD_ARG);
        EXPECT(REFINE(ctx, F, P, J, xyz + 4, SNOWTRI_F64, PM, kp, SNOWTRI_F64, np, det, views, 0.5, 4, 0u, xyz, cost, codes, SNOWTRI_HOST), SNOWTRI_ERR_BAD_ARG);
        EXPECT(strstr(snowtri_last_error(), "overlap") != NULL, 1);
        EXPECT(REFINE(ctx, ((int64_t)1 << 40), 2000000000, 2000000000, xyz, SNOWTRI_F64, 2000000000, kp, SNOWTRI_F64, np, det, views, 0.5, 4, 0u, out, cost, codes, SNOWTRI_HOST), SNOWTRI_ERR_BAD_ARG);
        EXPECT(REFINE(ctx, ((int64_t)1 << 62), 1, 1, xyz, SNOWTRI_F64, 1, kp, SNOWTRI_F64, np, det, views, 0.5, 4, 0u, out, cost, codes, SNOWTRI_HOST), SNOWTRI_ERR_BAD_ARG);
        EXPECT(strstr(snowtri_last_error(), "records") != NULL, 1);
        EXPECT(REFINE(ctx, 0, P, J, NULL, SNOWTRI_F64, PM, NULL, SNOWTRI_F64, NULL, NULL, NULL, 0.5, 4, 0u, NULL, NULL, NULL, SNOWTRI_HOST), SNOWTRI_OK);      /* empty batch: no pointer is looked at */
        EXPECT(REFINE(ctx, 0, P, J, NULL, SNOWTRI_F32, PM, NULL, SNOWTRI_F32, NULL, NULL, NULL, 0.5, 1, SW, NULL, NULL, NULL, SNOWTRI_DEVICE), SNOWTRI_OK);
        for (i = 0; i < N * 4; i++) failures += out[i] != 0.0;                                /* nothing was written */
        for (i = 0; i < N; i++) failures += codes[i] != 0 || cost[2 * i] != 0.0 || cost[2 * i + 1] != 0.0;
        /* one good call, so that the refusals above are refusals of their argument and not of everything: every record has four
         * views, moves, ends with a lower cost and keeps its score; the same call in place gives the same bits */
        EXPECT(GOOD(ctx), SNOWTRI_OK);
        for (i = 0; i < N; i++) {
            EXPECT(codes[i], SNOWTRI_REFINE_MOVED);
            EXPECT(cost[2 * i + 1] < cost[2 * i] && cost[2 * i + 1] >= 0.0, 1);
            EXPECT(out[4 * i + 3] == xyz[4 * i + 3] && out[4 * i + 2] != xyz[4 * i + 2], 1);
        }
        EXPECT(REFINE(ctx, F, P, J, xyz, SNOWTRI_F64, PM, kp, SNOWTRI_F64, NULL, NULL, NULL, 0.5, 4, SW, xyz, NULL, NULL, SNOWTRI_HOST), SNOWTRI_OK);
        EXPECT(memcmp(xyz, out, sizeof(double) * 4 * N), 0);                                  /* (every score is 1: the weights change nothing) */
        EXPECT(snowtri_ctx_destroy(ctx), SNOWTRI_OK);
        EXPECT(snowtri_ctx_destroy(none), SNOWTRI_OK);
        EXPECT(snowtri_ctx_destroy(odd), SNOWTRI_OK);
        EXPECT(snowtri_ctx_destroy(wide), SNOWTRI_OK);
    }
    printf("abi_badargs_refine: %d failure(s)\n", failures);
    return failures;
}
