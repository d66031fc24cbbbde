/* Drives snowtri_refine_cameras_k with invalid arguments: the C ABI must report, never crash or read through a bad pointer.  Plain
 * C99, its own main (tests/abi_badargs_pose.c covers snowtri_refine_cameras, whose refusals this entry shares).
 *
 *   - without a GPU (tests/test_intrinsics_host.py builds it against the AddressSanitizer build of the library, `make asan`): a
 *     null context, with good and with bad other arguments;
 *   - with a GPU (tests/test_gpu_intrinsics.py runs it against libsnowtri.so): the same plus, on a real context, the refusals this
 *     entry adds -- an unknown intr_flags bit, an intr_mask bit at or above C, intr_flags != 0 with a NULL K_out, a misaligned
 *     K_out -- a few it shares (iters, min_obs, free_mask, a NULL R_out), nothing written by any of them, the empty batch, which
 *     copies every camera, a call with intr_flags == 0 and one with intr_mask == 0 against snowtri_refine_cameras_ex byte for byte,
 *     and one good call with every intrinsic free.
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

enum { F = 6, P = 2, J = 7, PM = 3, C = 4, N = F * P * J };

int main(void) {
    static double xyz[N * 4 + 4], kp[F * C * PM * J * 3], Ko[C * 9 + 1], Ro[C * 9 + 1], to[C * 3 + 1], cost[C * 2 + 1], normal[C * 66 + 1];
    static double Re[C * 9], te[C * 3], coste[C * 2], normale[C * 28];
    static int64_t nobs[C + 1], nobse[C], nout[C + 1];
    static uint8_t codes[C], codese[C];
    static int32_t np[F * C], det[F * C * P];
    static uint32_t views[N];
    const uint32_t FC = SNOWTRI_INTR_FOCAL | SNOWTRI_INTR_CENTRE;
    volatile double zero = 0.0;
    const double nan = zero / zero;
    int i;
    for (i = 0; i < N; i++) {
        xyz[4 * i] = 0.37 * (i % 7) - 1.0 + 0.011 * (i % 11);
        xyz[4 * i + 1] = 0.29 * (i % 5) - 0.5 + 0.013 * (i % 13);
        xyz[4 * i + 2] = 4.0 + 0.23 * (i % 3) + 0.05 * (i % 17);
        xyz[4 * i + 3] = 1.0;
        views[i] = 0xfu;
    }
    for (i = 0; i < F * C; i++) np[i] = PM;
    for (i = 0; i < F * C * P; i++) det[i] = i % P;

#define CAMK(ctx_, F_, x_, k_, fm_, im_, if_, mo_, it_, fl_, hp_, K_, R_, t_, c_, n_, cd_, nm_, no_, ms_) \
    snowtri_refine_cameras_k(ctx_, F_, P, J, x_, SNOWTRI_F64, PM, k_, SNOWTRI_F64, np, det, views, 0.5, fm_, im_, if_, mo_, it_, fl_, hp_, K_, R_, t_, c_, n_, cd_, nm_, no_, ms_, NULL)
#define GOOD(ctx_) CAMK(ctx_, F, xyz, kp, 0xau, 0xfu, FC, 6, 8, 0u, 0.0, Ko, Ro, to, cost, nobs, codes, normal, nout, SNOWTRI_HOST)
    /* ---- null context ---------------------------------------------------------------------------------------- */
    EXPECT(GOOD(NULL), SNOWTRI_ERR_BAD_ARG);
    EXPECT(CAMK(NULL, 0, NULL, NULL, 0u, 0u, 0u, 6, 4, 0u, 0.0, NULL, Ro, to, NULL, NULL, NULL, NULL, NULL, SNOWTRI_HOST), SNOWTRI_ERR_BAD_ARG);
    EXPECT(CAMK(NULL, -1, NULL, NULL, 0xffffffffu, 0xffffffffu, 0xfcu, 0, 0, 8u, nan, NULL, NULL, NULL, NULL, NULL, NULL, NULL, NULL, 7), SNOWTRI_ERR_BAD_ARG);
    EXPECT(snowtri_last_error() != NULL && strstr(snowtri_last_error(), "snowtri_refine_cameras_k") != NULL, 1);

    /* ---- a real context (GPU box only) ------------------------------------------------------------------------- */
    if (snowtri_device_count() > 0) {
        snowtri_ctx *ctx = NULL;
        static double K[C * 9], R[C * 9], t[C * 3];
        int c, f, p, j;
        for (c = 0; c < C; c++) {
            const double k[9] = {700, 0.5, 640, 0, 705, 360, 0, 0, 1}, r[9] = {1, 0, 0, 0, 1, 0, 0, 0, 1};
            memcpy(K + 9 * c, k, sizeof k);
            memcpy(R + 9 * c, r, sizeof r);
            t[3 * c] = 0.5 * c;
            t[3 * c + 1] = 0.1 * (c % 3);
            t[3 * c + 2] = 0.0;
        }
        /* detection q of camera c shows person q: the exact pixel of the record as a camera 3 cm to the side, with a focal length
         * 2 % longer and a centre 6 px off, would see it */
        for (f = 0; f < F; f++)
            for (c = 0; c < C; c++)
                for (p = 0; p < PM; p++)
                    for (j = 0; j < J; j++) {
                        const double *x = xyz + 4 * ((f * P + (p % P)) * J + j);
                        double *o = kp + 3 * (((f * C + c) * PM + p) * J + j);
                        const double px = (x[0] - t[3 * c] - 0.03) / x[2], py = (x[1] - t[3 * c + 1] + 0.02) / x[2];
                        o[0] = 714 * px + 0.5 * py + 646;
                        o[1] = 719 * py + 355;
                        o[2] = 1.0;
                    }
        EXPECT(snowtri_ctx_create(4, K, R, t, 0, &ctx), SNOWTRI_OK);
        memset(Ko, 0, sizeof Ko);
        memset(Ro, 0, sizeof Ro);
        memset(to, 0, sizeof to);
        memset(cost, 0, sizeof cost);
        memset(codes, 9, sizeof codes);
        EXPECT(CAMK(ctx, F, xyz, kp, 0xau, 0xfu, 4u, 6, 8, 0u, 0.0, Ko, Ro, to, cost, nobs, codes, normal, nout, SNOWTRI_HOST), SNOWTRI_ERR_BAD_ARG);   /* an unknown intr_flags bit */
        EXPECT(strstr(snowtri_last_error(), "intr_flags") != NULL, 1);
        EXPECT(CAMK(ctx, F, xyz, kp, 0xau, 0xfu, 0x80000001u, 6, 8, 0u, 0.0, Ko, Ro, to, cost, nobs, codes, normal, nout, SNOWTRI_HOST), SNOWTRI_ERR_BAD_ARG);
        EXPECT(strstr(snowtri_last_error(), "intr_flags") != NULL, 1);
        EXPECT(CAMK(ctx, F, xyz, kp, 0xau, 0x10u, FC, 6, 8, 0u, 0.0, Ko, Ro, to, cost, nobs, codes, normal, nout, SNOWTRI_HOST), SNOWTRI_ERR_BAD_ARG);   /* camera 4 of 4 */
        EXPECT(strstr(snowtri_last_error(), "intr_mask") != NULL, 1);
        EXPECT(CAMK(ctx, F, xyz, kp, 0xau, 0x8000000au, 0u, 6, 8, 0u, 0.0, Ko, Ro, to, cost, nobs, codes, normal, nout, SNOWTRI_HOST), SNOWTRI_ERR_BAD_ARG);   /* ... whatever the flags */
        EXPECT(strstr(snowtri_last_error(), "intr_mask") != NULL, 1);
        EXPECT(CAMK(ctx, F, xyz, kp, 0xau, 0xfu, FC, 6, 8, 0u, 0.0, NULL, Ro, to, cost, nobs, codes, normal, nout, SNOWTRI_HOST), SNOWTRI_ERR_BAD_ARG);   /* K_out is required */
        EXPECT(strstr(snowtri_last_error(), "K_out") != NULL, 1);
        EXPECT(CAMK(ctx, 0, NULL, NULL, 0xau, 0u, SNOWTRI_INTR_FOCAL, 6, 8, 0u, 0.0, NULL, Ro, to, NULL, NULL, NULL, NULL, NULL, SNOWTRI_HOST), SNOWTRI_ERR_BAD_ARG);   /* ... on an empty batch and with no camera in the mask too */
        EXPECT(strstr(snowtri_last_error(), "K_out") != NULL, 1);
        EXPECT(CAMK(ctx, F, xyz, kp, 0xau, 0xfu, FC, 6, 8, 0u, 0.0, (double *)((char *)Ko + 4), Ro, to, cost, nobs, codes, normal, nout, SNOWTRI_DEVICE), SNOWTRI_ERR_BAD_ARG);
        EXPECT(strstr(snowtri_last_error(), "K_out") != NULL && strstr(snowtri_last_error(), "aligned") != NULL, 1);
        EXPECT(CAMK(ctx, F, xyz, kp, 0xau, 0xfu, FC, 6, 8, 0u, 0.0, Ko, Ro, to, cost, nobs, codes, (double *)((char *)normal + 4), nout, SNOWTRI_DEVICE), SNOWTRI_ERR_BAD_ARG);
        /* shared with snowtri_refine_cameras_ex */
        EXPECT(CAMK(ctx, F, xyz, kp, 0xau, 0xfu, FC, 6, 17, 0u, 0.0, Ko, Ro, to, cost, nobs, codes, normal, nout, SNOWTRI_HOST), SNOWTRI_ERR_BAD_ARG);
        EXPECT(strstr(snowtri_last_error(), "iters") != NULL, 1);
        EXPECT(CAMK(ctx, F, xyz, kp, 0xau, 0xfu, FC, 2, 8, 0u, 0.0, Ko, Ro, to, cost, nobs, codes, normal, nout, SNOWTRI_HOST), SNOWTRI_ERR_BAD_ARG);
        EXPECT(strstr(snowtri_last_error(), "min_obs") != NULL, 1);
        EXPECT(CAMK(ctx, F, xyz, kp, 0x10u, 0xfu, FC, 6, 8, 0u, 0.0, Ko, Ro, to, cost, nobs, codes, normal, nout, SNOWTRI_HOST), SNOWTRI_ERR_BAD_ARG);
        EXPECT(strstr(snowtri_last_error(), "free_mask") != NULL, 1);
        EXPECT(CAMK(ctx, F, xyz, kp, 0xau, 0xfu, FC, 6, 8, 2u, 0.0, Ko, Ro, to, cost, nobs, codes, normal, nout, SNOWTRI_HOST), SNOWTRI_ERR_BAD_ARG);
        EXPECT(CAMK(ctx, F, xyz, kp, 0xau, 0xfu, FC, 6, 8, 0u, -1.0, Ko, Ro, to, cost, nobs, codes, normal, nout, SNOWTRI_HOST), SNOWTRI_ERR_BAD_ARG);
        EXPECT(strstr(snowtri_last_error(), "huber_px") != NULL, 1);
        EXPECT(CAMK(ctx, F, xyz, kp, 0xau, 0xfu, FC, 6, 8, 0u, 0.0, Ko, NULL, to, cost, nobs, codes, normal, nout, SNOWTRI_HOST), SNOWTRI_ERR_BAD_ARG);
        EXPECT(CAMK(ctx, F, NULL, kp, 0xau, 0xfu, FC, 6, 8, 0u, 0.0, Ko, Ro, to, cost, nobs, codes, normal, nout, SNOWTRI_HOST), SNOWTRI_ERR_BAD_ARG);
        for (i = 0; i < C * 9; i++) failures += Ro[i] != 0.0 || Ko[i] != 0.0;                  /* nothing was written */
        for (i = 0; i < C; i++) failures += codes[i] != 9 || cost[2 * i] != 0.0 || to[3 * i] != 0.0;
        /* the empty batch: every camera is copied, free cameras have too few observations, no input pointer is looked at */
        EXPECT(CAMK(ctx, 0, NULL, NULL, 0x2u, 0x8u, FC, 3, 1, 0u, 0.0, Ko, Ro, to, cost, nobs, codes, normal, NULL, SNOWTRI_HOST), SNOWTRI_OK);
        EXPECT(memcmp(Ko, K, sizeof(double) * 9 * C), 0);
        EXPECT(memcmp(Ro, R, sizeof(double) * 9 * C), 0);
        EXPECT(memcmp(to, t, sizeof(double) * 3 * C), 0);
        for (c = 0; c < C; c++) {
            EXPECT(codes[c], (c == 1 || c == 3) ? SNOWTRI_POSE_FEW_OBS : SNOWTRI_POSE_FIXED);
            EXPECT(nobs[c] == 0 && cost[2 * c] == 0.0 && cost[2 * c + 1] == 0.0 && normal[66 * c] == 0.0 && normal[66 * c + 65] == 0.0, 1);
        }
        /* no intrinsics free: snowtri_refine_cameras_ex byte for byte, with and without the loss */
        for (i = 0; i < 4; i++) {
            const double hp = (i & 1) ? 3.0 : 0.0;
            static int64_t noute[C];
            EXPECT(snowtri_refine_cameras_ex(ctx, F, P, J, xyz, SNOWTRI_F64, PM, kp, SNOWTRI_F64, np, det, views, 0.5, 0xau, 6, 8, 0u, hp, Re, te, coste,
                                             nobse, codese, normale, noute, SNOWTRI_HOST, NULL), SNOWTRI_OK);
            EXPECT(CAMK(ctx, F, xyz, kp, 0xau, (i & 2) ? 0u : 0xfu, (i & 2) ? FC : 0u, 6, 8, 0u, hp, Ko, Ro, to, cost, nobs, codes, normal, nout, SNOWTRI_HOST), SNOWTRI_OK);
            EXPECT(memcmp(Ko, K, sizeof(double) * 9 * C), 0);
            EXPECT(memcmp(Ro, Re, sizeof Re) == 0 && memcmp(to, te, sizeof te) == 0 && memcmp(cost, coste, sizeof coste) == 0, 1);
            EXPECT(memcmp(nobs, nobse, sizeof nobse) == 0 && memcmp(codes, codese, sizeof codese) == 0 && memcmp(nout, noute, sizeof noute) == 0, 1);
            for (c = 0; c < C; c++) {
                EXPECT(memcmp(normal + 66 * c, normale + 28 * c, sizeof(double) * 7), 0);            /* E, g[6] */
                EXPECT(memcmp(normal + 66 * c + 11, normale + 28 * c + 7, sizeof(double) * 21), 0);  /* the 6 x 6 block of H */
            }
        }
        /* one good call, so that the refusals above are refusals of their argument and not of everything: cameras 1 and 3 move in
         * all ten parameters, cameras 0 and 2 only in their four intrinsics and keep the bits of their pose */
        EXPECT(GOOD(ctx), SNOWTRI_OK);
        for (c = 0; c < C; c++) {
            EXPECT(nobs[c], N);
            EXPECT(codes[c], SNOWTRI_POSE_MOVED);
            EXPECT(normal[66 * c] > 0.0 && normal[66 * c + 11] > 0.0 && normal[66 * c + 65] == (double)N && normal[66 * c + 64] == 0.0, 1);
            EXPECT(cost[2 * c + 1] < cost[2 * c] && cost[2 * c + 1] >= 0.0 && cost[2 * c] == normal[66 * c], 1);
            EXPECT(Ko[9 * c] != K[9 * c] && Ko[9 * c + 2] != K[9 * c + 2] && Ko[9 * c] > 0.0 && Ko[9 * c + 4] > 0.0, 1);
            EXPECT(Ko[9 * c + 1] == 0.5 && Ko[9 * c + 3] == 0.0 && Ko[9 * c + 6] == 0.0 && Ko[9 * c + 7] == 0.0 && Ko[9 * c + 8] == 1.0, 1);
            if (c & 1)
                EXPECT(memcmp(to + 3 * c, t + 3 * c, sizeof(double) * 3) != 0, 1);
            else
                EXPECT(memcmp(Ro + 9 * c, R + 9 * c, sizeof(double) * 9) == 0 && memcmp(to + 3 * c, t + 3 * c, sizeof(double) * 3) == 0, 1);
        }
        /* only the centre of camera 2: every other K, and the focal lengths of camera 2, keep their bits */
        EXPECT(CAMK(ctx, F, xyz, kp, 0x0u, 0x4u, SNOWTRI_INTR_CENTRE, 3, 16, SNOWTRI_REFINE_SCORE_WEIGHTS, 0.0, Ko, Ro, to, NULL, NULL, codes, NULL, NULL, SNOWTRI_HOST), SNOWTRI_OK);
        for (c = 0; c < C; c++) {
            EXPECT(codes[c], c == 2 ? SNOWTRI_POSE_MOVED : SNOWTRI_POSE_FIXED);
            if (c != 2) EXPECT(memcmp(Ko + 9 * c, K + 9 * c, sizeof(double) * 9), 0);
        }
        EXPECT(Ko[18] == K[18] && Ko[22] == K[22] && Ko[20] != K[20] && Ko[23] != K[23], 1);
        EXPECT(snowtri_ctx_destroy(ctx), SNOWTRI_OK);
    }
    printf("abi_badargs_intrinsics: %d failure(s)\n", failures);
    return failures;
}
