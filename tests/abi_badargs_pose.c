/* Drives snowtri_refine_cameras with invalid arguments: the C ABI must report, never crash or read through a bad pointer.  Plain C99,
 * its own main (tests/abi_badargs_refine.c covers snowtri_refine_joints).
 *
 *   - without a GPU (tests/test_pose_host.py builds it against the AddressSanitizer build of the library, `make asan`): a null
 *     context, with good and with bad other arguments;
 *   - with a GPU (tests/test_gpu_pose.py runs it against libsnowtri.so): the same plus, on real contexts, every refusal that comes
 *     before a launch -- sizes, dtype codes, memory spaces, flag bits, iters, min_obs, free_mask bits at or above C, a K of the wrong
 *     form, a NaN threshold, more than 32 cameras, P > Pmax without det_of, missing and misaligned pointers, a batch past the size
 *     limit -- the empty batch, which copies every pose and looks at no input pointer, and one good call.
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

enum { F = 3, P = 2, J = 5, PM = 3, C = 4, N = F * P * J };

int main(void) {
    static double xyz[N * 4 + 4], kp[F * C * PM * J * 3], Ro[C * 9 + 1], to[C * 3 + 1], cost[C * 2 + 1], normal[C * 28 + 1];
    static int64_t nobs[C + 1];
    static uint8_t codes[C];
    static int32_t np[F * C], det[F * C * P];
    static uint32_t views[N];
    const uint32_t SW = SNOWTRI_REFINE_SCORE_WEIGHTS;
    volatile double zero = 0.0;
    const double nan = zero / zero;
    int i;
    for (i = 0; i < N; i++) {
        xyz[4 * i] = 0.37 * (i % 7) - 1.0;
        xyz[4 * i + 1] = 0.29 * (i % 5) - 0.5;
        xyz[4 * i + 2] = 4.0 + 0.13 * (i % 3);
        xyz[4 * i + 3] = 1.0;
        views[i] = 0xfu;
    }
    for (i = 0; i < F * C; i++) np[i] = PM;
    for (i = 0; i < F * C * P; i++) det[i] = i % P;

#define POSE(ctx_, F_, P_, J_, x_, xdt_, Pm_, k_, kdt_, np_, det_, vw_, thr_, fm_, mo_, it_, fl_, R_, t_, c_, n_, cd_, nm_, ms_) \
    snowtri_refine_cameras(ctx_, F_, P_, J_, x_, xdt_, Pm_, k_, kdt_, np_, det_, vw_, thr_, fm_, mo_, it_, fl_, R_, t_, c_, n_, cd_, nm_, ms_, NULL)
#define GOOD(ctx_) POSE(ctx_, F, P, J, xyz, SNOWTRI_F64, PM, kp, SNOWTRI_F64, np, det, views, 0.5, 0xau, 6, 4, 0u, Ro, to, cost, nobs, codes, normal, SNOWTRI_HOST)
#define WITH(F_, P_, J_, x_, xdt_, Pm_, k_, kdt_, np_, det_, vw_, thr_, fm_, mo_, it_, fl_, R_, t_, c_, n_, nm_, ms_) \
    POSE(ctx, F_, P_, J_, x_, xdt_, Pm_, k_, kdt_, np_, det_, vw_, thr_, fm_, mo_, it_, fl_, R_, t_, c_, n_, codes, nm_, ms_)
    /* ---- null context ---------------------------------------------------------------------------------------- */
    EXPECT(GOOD(NULL), SNOWTRI_ERR_BAD_ARG);
    EXPECT(POSE(NULL, 0, P, J, NULL, SNOWTRI_F64, PM, NULL, SNOWTRI_F64, NULL, NULL, NULL, 0.5, 0u, 6, 4, 0u, Ro, to, NULL, NULL, NULL, NULL, SNOWTRI_HOST), SNOWTRI_ERR_BAD_ARG);
    EXPECT(POSE(NULL, -1, 0, 0, NULL, 9, 0, NULL, -1, NULL, NULL, NULL, nan, 0xffffffffu, 0, 0, 8u, NULL, NULL, NULL, NULL, NULL, NULL, 7), SNOWTRI_ERR_BAD_ARG);
    EXPECT(snowtri_last_error() != NULL && strstr(snowtri_last_error(), "snowtri_refine_cameras") != NULL, 1);
    EXPECT(snowtri_pose_sweep_records(), 1024 * 256);

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
        /* detection q of camera c shows person q: the exact pixel of the record as a camera 3 cm to the side would see it */
        for (f = 0; f < F; f++)
            for (c = 0; c < C; c++)
                for (p = 0; p < PM; p++)
                    for (j = 0; j < J; j++) {
                        const double *x = xyz + 4 * ((f * P + (p % P)) * J + j);
                        double *o = kp + 3 * (((f * C + c) * PM + p) * J + j);
                        const double px = (x[0] - t[3 * c] - 0.03) / x[2], py = (x[1] - t[3 * c + 1] + 0.02) / x[2];
                        o[0] = 700 * px + 0.5 * py + 640;
                        o[1] = 700 * py + 360;
                        o[2] = 1.0;
                    }
        EXPECT(snowtri_ctx_create(4, K, R, t, 0, &ctx), SNOWTRI_OK);
        EXPECT(snowtri_ctx_create(0, NULL, NULL, NULL, 0, &none), SNOWTRI_OK);
        EXPECT(snowtri_ctx_create(1, Kodd, R, t, 0, &odd), SNOWTRI_OK);
        EXPECT(snowtri_ctx_create(33, K, R, t, 0, &wide), SNOWTRI_OK);
        memset(Ro, 0, sizeof Ro);
        memset(to, 0, sizeof to);
        memset(cost, 0, sizeof cost);
        memset(codes, 9, sizeof codes);
        EXPECT(GOOD(none), SNOWTRI_ERR_BAD_ARG);                                              /* no cameras */
        EXPECT(POSE(odd, F, P, J, xyz, SNOWTRI_F64, PM, kp, SNOWTRI_F64, np, det, views, 0.5, 1u, 6, 4, 0u, Ro, to, cost, nobs, codes, normal, SNOWTRI_HOST), SNOWTRI_ERR_BAD_ARG);   /* K is not the pinhole form */
        EXPECT(strstr(snowtri_last_error(), "[[fx, s, cx]") != NULL, 1);
        EXPECT(GOOD(wide), SNOWTRI_ERR_BAD_ARG);                                              /* 33 cameras */
        EXPECT(strstr(snowtri_last_error(), "32") != NULL, 1);
        EXPECT(WITH(-1, P, J, xyz, SNOWTRI_F64, PM, kp, SNOWTRI_F64, np, det, views, 0.5, 0xau, 6, 4, 0u, Ro, to, cost, nobs, normal, SNOWTRI_HOST), SNOWTRI_ERR_BAD_ARG);
        EXPECT(WITH(F, 0, J, xyz, SNOWTRI_F64, PM, kp, SNOWTRI_F64, np, det, views, 0.5, 0xau, 6, 4, 0u, Ro, to, cost, nobs, normal, SNOWTRI_HOST), SNOWTRI_ERR_BAD_ARG);
        EXPECT(WITH(F, P, 0, xyz, SNOWTRI_F64, PM, kp, SNOWTRI_F64, np, det, views, 0.5, 0xau, 6, 4, 0u, Ro, to, cost, nobs, normal, SNOWTRI_HOST), SNOWTRI_ERR_BAD_ARG);
        EXPECT(WITH(F, P, J, xyz, SNOWTRI_F64, 0, kp, SNOWTRI_F64, np, det, views, 0.5, 0xau, 6, 4, 0u, Ro, to, cost, nobs, normal, SNOWTRI_HOST), SNOWTRI_ERR_BAD_ARG);
        EXPECT(WITH(F, P, J, xyz, 7, PM, kp, SNOWTRI_F64, np, det, views, 0.5, 0xau, 6, 4, 0u, Ro, to, cost, nobs, normal, SNOWTRI_HOST), SNOWTRI_ERR_BAD_ARG);
        EXPECT(WITH(F, P, J, xyz, SNOWTRI_F64, PM, kp, 2, np, det, views, 0.5, 0xau, 6, 4, 0u, Ro, to, cost, nobs, normal, SNOWTRI_HOST), SNOWTRI_ERR_BAD_ARG);
        EXPECT(WITH(F, P, J, xyz, SNOWTRI_F64, PM, kp, SNOWTRI_F64, np, det, views, 0.5, 0xau, 6, 4, 0u, Ro, to, cost, nobs, normal, 5), SNOWTRI_ERR_BAD_ARG);
        EXPECT(WITH(F, P, J, xyz, SNOWTRI_F64, PM, kp, SNOWTRI_F64, np, det, views, 0.5, 0xau, 6, 4, 2u, Ro, to, cost, nobs, normal, SNOWTRI_HOST), SNOWTRI_ERR_BAD_ARG);   /* an unknown flag bit */
        EXPECT(strstr(snowtri_last_error(), "flag") != NULL, 1);
        EXPECT(WITH(F, P, J, xyz, SNOWTRI_F64, PM, kp, SNOWTRI_F64, np, det, views, nan, 0xau, 6, 4, 0u, Ro, to, cost, nobs, normal, SNOWTRI_HOST), SNOWTRI_ERR_BAD_ARG);
        EXPECT(WITH(F, P, J, xyz, SNOWTRI_F64, PM, kp, SNOWTRI_F64, np, det, views, 0.5, 0xau, 6, 0, 0u, Ro, to, cost, nobs, normal, SNOWTRI_HOST), SNOWTRI_ERR_BAD_ARG);
        EXPECT(WITH(F, P, J, xyz, SNOWTRI_F64, PM, kp, SNOWTRI_F64, np, det, views, 0.5, 0xau, 6, 17, 0u, Ro, to, cost, nobs, normal, SNOWTRI_HOST), SNOWTRI_ERR_BAD_ARG);
        EXPECT(strstr(snowtri_last_error(), "iters") != NULL, 1);
        EXPECT(WITH(F, P, J, xyz, SNOWTRI_F64, PM, kp, SNOWTRI_F64, np, det, views, 0.5, 0xau, 2, 4, 0u, Ro, to, cost, nobs, normal, SNOWTRI_HOST), SNOWTRI_ERR_BAD_ARG);
        EXPECT(WITH(F, P, J, xyz, SNOWTRI_F64, PM, kp, SNOWTRI_F64, np, det, views, 0.5, 0xau, -5, 4, 0u, Ro, to, cost, nobs, normal, SNOWTRI_HOST), SNOWTRI_ERR_BAD_ARG);
        EXPECT(strstr(snowtri_last_error(), "min_obs") != NULL, 1);
        EXPECT(WITH(F, P, J, xyz, SNOWTRI_F64, PM, kp, SNOWTRI_F64, np, det, views, 0.5, 0x10u, 6, 4, 0u, Ro, to, cost, nobs, normal, SNOWTRI_HOST), SNOWTRI_ERR_BAD_ARG);   /* camera 4 of 4 */
        EXPECT(WITH(F, P, J, xyz, SNOWTRI_F64, PM, kp, SNOWTRI_F64, np, det, views, 0.5, 0x8000000au, 6, 4, 0u, Ro, to, cost, nobs, normal, SNOWTRI_HOST), SNOWTRI_ERR_BAD_ARG);
        EXPECT(strstr(snowtri_last_error(), "free_mask") != NULL, 1);
        EXPECT(WITH(0, P, J, NULL, SNOWTRI_F64, PM, NULL, SNOWTRI_F64, NULL, NULL, NULL, 0.5, 0xau, 6, 17, 0u, Ro, to, NULL, NULL, NULL, SNOWTRI_HOST), SNOWTRI_ERR_BAD_ARG);   /* ... even on an empty batch */
        EXPECT(WITH(F, 4, J, xyz, SNOWTRI_F64, PM, kp, SNOWTRI_F64, np, NULL, views, 0.5, 0xau, 6, 4, 0u, Ro, to, cost, nobs, normal, SNOWTRI_HOST), SNOWTRI_ERR_BAD_ARG);   /* P = 4 > Pmax = 3, no det_of */
        EXPECT(strstr(snowtri_last_error(), "det_of") != NULL, 1);
        EXPECT(WITH(F, P, J, NULL, SNOWTRI_F64, PM, kp, SNOWTRI_F64, np, det, views, 0.5, 0xau, 6, 4, 0u, Ro, to, cost, nobs, normal, SNOWTRI_HOST), SNOWTRI_ERR_BAD_ARG);
        EXPECT(WITH(F, P, J, xyz, SNOWTRI_F64, PM, NULL, SNOWTRI_F64, np, det, views, 0.5, 0xau, 6, 4, 0u, Ro, to, cost, nobs, normal, SNOWTRI_HOST), SNOWTRI_ERR_BAD_ARG);
        EXPECT(WITH(F, P, J, xyz, SNOWTRI_F64, PM, kp, SNOWTRI_F64, np, det, views, 0.5, 0xau, 6, 4, 0u, NULL, to, cost, nobs, normal, SNOWTRI_HOST), SNOWTRI_ERR_BAD_ARG);
        EXPECT(WITH(F, P, J, xyz, SNOWTRI_F64, PM, kp, SNOWTRI_F64, np, det, views, 0.5, 0xau, 6, 4, 0u, Ro, NULL, cost, nobs, normal, SNOWTRI_HOST), SNOWTRI_ERR_BAD_ARG);
        EXPECT(WITH(0, P, J, NULL, SNOWTRI_F64, PM, NULL, SNOWTRI_F64, NULL, NULL, NULL, 0.5, 0xau, 6, 4, 0u, NULL, to, NULL, NULL, NULL, SNOWTRI_HOST), SNOWTRI_ERR_BAD_ARG);   /* the empty batch writes the poses too */
        EXPECT(WITH(F, P, J, (char *)xyz + 4, SNOWTRI_F64, PM, kp, SNOWTRI_F64, np, det, views, 0.5, 0xau, 6, 4, 0u, Ro, to, cost, nobs, normal, SNOWTRI_DEVICE), SNOWTRI_ERR_BAD_ARG);
        EXPECT(WITH(F, P, J, xyz, SNOWTRI_F64, PM, (char *)kp + 2, SNOWTRI_F32, np, det, views, 0.5, 0xau, 6, 4, 0u, Ro, to, cost, nobs, normal, SNOWTRI_DEVICE), SNOWTRI_ERR_BAD_ARG);
        EXPECT(WITH(F, P, J, xyz, SNOWTRI_F64, PM, kp, SNOWTRI_F64, (int32_t *)((char *)np + 1), det, views, 0.5, 0xau, 6, 4, 0u, Ro, to, cost, nobs, normal, SNOWTRI_DEVICE), SNOWTRI_ERR_BAD_ARG);
        EXPECT(WITH(F, P, J, xyz, SNOWTRI_F64, PM, kp, SNOWTRI_F64, np, (int32_t *)((char *)det + 2), views, 0.5, 0xau, 6, 4, 0u, Ro, to, cost, nobs, normal, SNOWTRI_DEVICE), SNOWTRI_ERR_BAD_ARG);
        EXPECT(WITH(F, P, J, xyz, SNOWTRI_F64, PM, kp, SNOWTRI_F64, np, det, (uint32_t *)((char *)views + 2), 0.5, 0xau, 6, 4, 0u, Ro, to, cost, nobs, normal, SNOWTRI_DEVICE), SNOWTRI_ERR_BAD_ARG);
        EXPECT(WITH(F, P, J, xyz, SNOWTRI_F64, PM, kp, SNOWTRI_F64, np, det, views, 0.5, 0xau, 6, 4, 0u, (double *)((char *)Ro + 4), to, cost, nobs, normal, SNOWTRI_DEVICE), SNOWTRI_ERR_BAD_ARG);
        EXPECT(WITH(F, P, J, xyz, SNOWTRI_F64, PM, kp, SNOWTRI_F64, np, det, views, 0.5, 0xau, 6, 4, 0u, Ro, (double *)((char *)to + 4), cost, nobs, normal, SNOWTRI_DEVICE), SNOWTRI_ERR_BAD_ARG);
        EXPECT(WITH(F, P, J, xyz, SNOWTRI_F64, PM, kp, SNOWTRI_F64, np, det, views, 0.5, 0xau, 6, 4, 0u, Ro, to, (double *)((char *)cost + 4), nobs, normal, SNOWTRI_DEVICE), SNOWTRI_ERR_BAD_ARG);
        EXPECT(WITH(F, P, J, xyz, SNOWTRI_F64, PM, kp, SNOWTRI_F64, np, det, views, 0.5, 0xau, 6, 4, 0u, Ro, to, cost, (int64_t *)((char *)nobs + 4), normal, SNOWTRI_DEVICE), SNOWTRI_ERR_BAD_ARG);
        EXPECT(WITH(F, P, J, xyz, SNOWTRI_F64, PM, kp, SNOWTRI_F64, np, det, views, 0.5, 0xau, 6, 4, 0u, Ro, to, cost, nobs, (double *)((char *)normal + 4), SNOWTRI_DEVICE), SNOWTRI_ERR_BAD_ARG);
        EXPECT(strstr(snowtri_last_error(), "aligned") != NULL, 1);
        EXPECT(WITH(((int64_t)1 << 40), 2000000000, 2000000000, xyz, SNOWTRI_F64, 2000000000, kp, SNOWTRI_F64, np, det, views, 0.5, 0xau, 6, 4, 0u, Ro, to, cost, nobs, normal, SNOWTRI_HOST), SNOWTRI_ERR_BAD_ARG);
        EXPECT(WITH(((int64_t)1 << 62), 1, 1, xyz, SNOWTRI_F64, 1, kp, SNOWTRI_F64, np, det, views, 0.5, 0xau, 6, 4, 0u, Ro, to, cost, nobs, normal, SNOWTRI_HOST), SNOWTRI_ERR_BAD_ARG);
        EXPECT(strstr(snowtri_last_error(), "records") != NULL, 1);
        for (i = 0; i < C * 9; i++) failures += Ro[i] != 0.0;                                 /* nothing was written */
        for (i = 0; i < C; i++) failures += codes[i] != 9 || cost[2 * i] != 0.0 || to[3 * i] != 0.0;
        /* the empty batch: every pose is copied, free cameras have too few observations, no input pointer is looked at */
        EXPECT(WITH(0, P, J, NULL, SNOWTRI_F32, PM, NULL, SNOWTRI_F32, NULL, NULL, NULL, 0.5, 0xau, 3, 1, SW, Ro, to, cost, nobs, normal, SNOWTRI_HOST), SNOWTRI_OK);
        EXPECT(memcmp(Ro, R, sizeof(double) * 9 * C), 0);
        EXPECT(memcmp(to, t, sizeof(double) * 3 * C), 0);
        for (c = 0; c < C; c++) {
            EXPECT(codes[c], (c & 1) ? SNOWTRI_POSE_FEW_OBS : SNOWTRI_POSE_FIXED);
            EXPECT(nobs[c] == 0 && cost[2 * c] == 0.0 && cost[2 * c + 1] == 0.0 && normal[28 * c] == 0.0 && normal[28 * c + 27] == 0.0, 1);
        }
        EXPECT(WITH(0, P, J, NULL, SNOWTRI_F64, PM, NULL, SNOWTRI_F64, NULL, NULL, NULL, 0.5, 0u, 3, 16, 0u, Ro, to, NULL, NULL, NULL, SNOWTRI_HOST), SNOWTRI_OK);
        /* one good call, so that the refusals above are refusals of their argument and not of everything: cameras 1 and 3 see
         * every record, move and end with a lower cost; cameras 0 and 2 keep their bits and still report their normal equations */
        EXPECT(GOOD(ctx), SNOWTRI_OK);
        for (c = 0; c < C; c++) {
            EXPECT(nobs[c], N);
            EXPECT(normal[28 * c] > 0.0 && normal[28 * c + 7] > 0.0, 1);
            if (c & 1) {
                EXPECT(codes[c], SNOWTRI_POSE_MOVED);
                EXPECT(cost[2 * c + 1] < cost[2 * c] && cost[2 * c + 1] >= 0.0 && cost[2 * c] == normal[28 * c], 1);
                EXPECT(memcmp(to + 3 * c, t + 3 * c, sizeof(double) * 3) != 0, 1);
            } else {
                EXPECT(codes[c], SNOWTRI_POSE_FIXED);
                EXPECT(cost[2 * c] == 0.0 && cost[2 * c + 1] == 0.0, 1);
                EXPECT(memcmp(Ro + 9 * c, R + 9 * c, sizeof(double) * 9) == 0 && memcmp(to + 3 * c, t + 3 * c, sizeof(double) * 3) == 0, 1);
            }
        }
        EXPECT(POSE(ctx, F, P, J, xyz, SNOWTRI_F64, PM, kp, SNOWTRI_F64, NULL, NULL, NULL, 0.5, 0xfu, 3, 16, SW, Ro, to, NULL, NULL, NULL, NULL, SNOWTRI_HOST), SNOWTRI_OK);
        EXPECT(snowtri_ctx_destroy(ctx), SNOWTRI_OK);
        EXPECT(snowtri_ctx_destroy(none), SNOWTRI_OK);
        EXPECT(snowtri_ctx_destroy(odd), SNOWTRI_OK);
        EXPECT(snowtri_ctx_destroy(wide), SNOWTRI_OK);
    }
    printf("abi_badargs_pose: %d failure(s)\n", failures);
    return failures;
}
