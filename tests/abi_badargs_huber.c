/* Drives snowtri_refine_joints_ex and snowtri_refine_cameras_ex with invalid arguments: the C ABI must report, never crash or read
 * through a bad pointer.  Plain C99, its own main (tests/abi_badargs_refine.c and tests/abi_badargs_pose.c cover the arguments the
 * two entries share with snowtri_refine_joints and snowtri_refine_cameras; this program covers what the _ex entries add).
 *
 *   - without a GPU (tests/test_huber_host.py builds it against the AddressSanitizer build of the library, `make asan`): a null
 *     context, with good and with bad other arguments;
 *   - with a GPU (tests/test_gpu_huber.py runs it against libsnowtri.so): the same plus, on a real context, a huber_px that is NaN,
 *     negative, infinite or above 1e150, misaligned new outputs, an `outliers` that overlaps xyzs or out_xyzs, NULL new outputs,
 *     F == 0, huber_px == 0 against the entries without the loss (the same bytes), and good calls with the loss.
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
    /* xyz and the outliers words share one block, so that an overlap can be asked for */
    static double block[N * 4 + N], kp[F * C * PM * J * 3], out[N * 4 + 1], out0[N * 4], cost[N * 2 + 1], cost0[N * 2];
    static double Ro[C * 9 + 1], to[C * 3 + 1], Ro0[C * 9], to0[C * 3], ccost[C * 2], ccost0[C * 2], normal[C * 28], normal0[C * 28];
    static int64_t nobs[C], nobs0[C], noutl[C + 1];
    static uint8_t codes[N], codes0[N], ccodes[C], ccodes0[C];
    static uint32_t outl[N + 1];
    static int32_t np[F * C], det[F * C * P];
    static uint32_t views[N];
    double *xyz = block;
    volatile double zero = 0.0;
    const double nan = zero / zero, inf = 1.0 / zero;
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

#define JOINTS(ctx_, F_, h_, x_, o_, c_, cd_, ol_, ms_) \
    snowtri_refine_joints_ex(ctx_, F_, P, J, x_, SNOWTRI_F64, PM, kp, SNOWTRI_F64, np, det, views, 0.5, 4, 0u, h_, o_, c_, cd_, ol_, ms_, NULL)
#define CAMS(ctx_, F_, h_, R_, t_, c_, n_, cd_, nm_, no_, ms_) \
    snowtri_refine_cameras_ex(ctx_, F_, P, J, xyz, SNOWTRI_F64, PM, kp, SNOWTRI_F64, np, det, views, 0.5, 0xau, 6, 4, 0u, h_, R_, t_, c_, n_, cd_, nm_, no_, ms_, NULL)
    /* ---- null context ---------------------------------------------------------------------------------------- */
    EXPECT(JOINTS(NULL, F, 3.0, xyz, out, cost, codes, outl, SNOWTRI_HOST), SNOWTRI_ERR_BAD_ARG);
    EXPECT(snowtri_last_error() != NULL && strstr(snowtri_last_error(), "snowtri_refine_joints_ex") != NULL, 1);
    EXPECT(JOINTS(NULL, -1, nan, NULL, NULL, NULL, NULL, NULL, 7), SNOWTRI_ERR_BAD_ARG);
    EXPECT(JOINTS(NULL, 0, 0.0, NULL, NULL, NULL, NULL, NULL, SNOWTRI_HOST), SNOWTRI_ERR_BAD_ARG);
    EXPECT(CAMS(NULL, F, 3.0, Ro, to, ccost, nobs, ccodes, normal, noutl, SNOWTRI_HOST), SNOWTRI_ERR_BAD_ARG);
    EXPECT(snowtri_last_error() != NULL && strstr(snowtri_last_error(), "snowtri_refine_cameras_ex") != NULL, 1);
    EXPECT(CAMS(NULL, -1, -inf, NULL, NULL, NULL, NULL, NULL, NULL, NULL, 7), SNOWTRI_ERR_BAD_ARG);

    /* ---- a real context (GPU box only) ------------------------------------------------------------------------- */
    if (snowtri_device_count() > 0) {
        snowtri_ctx *ctx = NULL;
        static double K[C * 9], R[C * 9], t[C * 3];
        int c, f, p, j, any;
        for (c = 0; c < C; c++) {
            const double k[9] = {700, 0.5, 640, 0, 700, 360, 0, 0, 1}, r[9] = {1, 0, 0, 0, 1, 0, 0, 0, 1};
            memcpy(K + 9 * c, k, sizeof k);
            memcpy(R + 9 * c, r, sizeof r);
            t[3 * c] = 0.5 * c;
            t[3 * c + 1] = 0.1 * (c % 3);
            t[3 * c + 2] = 0.0;
        }
        /* detection q of camera c shows person q: the pixel of the record as a camera 3 cm to the side would see it; camera 2's
         * detections of joint 0 are 80 px off: outliers of any delta used below */
        for (f = 0; f < F; f++)
            for (c = 0; c < C; c++)
                for (p = 0; p < PM; p++)
                    for (j = 0; j < J; j++) {
                        const double *x = xyz + 4 * ((f * P + (p % P)) * J + j);
                        double *o = kp + 3 * (((f * C + c) * PM + p) * J + j);
                        const double px = (x[0] - t[3 * c] - 0.03) / x[2], py = (x[1] - t[3 * c + 1] + 0.02) / x[2];
                        o[0] = 700 * px + 0.5 * py + 640 + ((c == 2 && j == 0) ? 80.0 : 0.0);
                        o[1] = 700 * py + 360;
                        o[2] = 1.0;
                    }
        EXPECT(snowtri_ctx_create(C, K, R, t, 0, &ctx), SNOWTRI_OK);
        memset(out, 0, sizeof out);
        memset(codes, 9, sizeof codes);
        memset(outl, 0xee, sizeof outl);
        memset(Ro, 0, sizeof Ro);
        memset(noutl, 0x77, sizeof noutl);
        /* huber_px */
        EXPECT(JOINTS(ctx, F, nan, xyz, out, cost, codes, outl, SNOWTRI_HOST), SNOWTRI_ERR_BAD_ARG);
        EXPECT(strstr(snowtri_last_error(), "huber_px") != NULL, 1);
        EXPECT(JOINTS(ctx, F, -1.0, xyz, out, cost, codes, outl, SNOWTRI_HOST), SNOWTRI_ERR_BAD_ARG);
        EXPECT(JOINTS(ctx, F, -inf, xyz, out, cost, codes, outl, SNOWTRI_HOST), SNOWTRI_ERR_BAD_ARG);
        EXPECT(JOINTS(ctx, F, inf, xyz, out, cost, codes, outl, SNOWTRI_HOST), SNOWTRI_ERR_BAD_ARG);
        EXPECT(JOINTS(ctx, F, 1.0000001e150, xyz, out, cost, codes, outl, SNOWTRI_HOST), SNOWTRI_ERR_BAD_ARG);
        EXPECT(strstr(snowtri_last_error(), "1e150") != NULL, 1);
        EXPECT(JOINTS(ctx, 0, nan, NULL, NULL, NULL, NULL, NULL, SNOWTRI_HOST), SNOWTRI_ERR_BAD_ARG);          /* ... even on an empty batch */
        EXPECT(CAMS(ctx, F, nan, Ro, to, ccost, nobs, ccodes, normal, noutl, SNOWTRI_HOST), SNOWTRI_ERR_BAD_ARG);
        EXPECT(strstr(snowtri_last_error(), "huber_px") != NULL, 1);
        EXPECT(CAMS(ctx, F, -0.5, Ro, to, ccost, nobs, ccodes, normal, noutl, SNOWTRI_HOST), SNOWTRI_ERR_BAD_ARG);
        EXPECT(CAMS(ctx, F, inf, Ro, to, ccost, nobs, ccodes, normal, noutl, SNOWTRI_HOST), SNOWTRI_ERR_BAD_ARG);
        EXPECT(CAMS(ctx, F, 2e150, Ro, to, ccost, nobs, ccodes, normal, noutl, SNOWTRI_HOST), SNOWTRI_ERR_BAD_ARG);
        EXPECT(CAMS(ctx, 0, nan, Ro, to, NULL, NULL, NULL, NULL, NULL, SNOWTRI_HOST), SNOWTRI_ERR_BAD_ARG);
        /* misaligned new outputs (SNOWTRI_DEVICE: the pointers are used as they are; refused before anything is launched) */
        EXPECT(JOINTS(ctx, F, 3.0, xyz, out, cost, codes, (uint32_t *)((char *)outl + 2), SNOWTRI_DEVICE), SNOWTRI_ERR_BAD_ARG);
        EXPECT(strstr(snowtri_last_error(), "aligned") != NULL, 1);
        EXPECT(CAMS(ctx, F, 3.0, Ro, to, ccost, nobs, ccodes, normal, (int64_t *)((char *)noutl + 4), SNOWTRI_DEVICE), SNOWTRI_ERR_BAD_ARG);
        EXPECT(strstr(snowtri_last_error(), "aligned") != NULL, 1);
        /* outliers overlapping the records it is computed from, or the records written */
        EXPECT(JOINTS(ctx, F, 3.0, xyz, out, cost, codes, (uint32_t *)(xyz + 4 * N) - 1, SNOWTRI_HOST), SNOWTRI_ERR_BAD_ARG);
        EXPECT(strstr(snowtri_last_error(), "outliers") != NULL, 1);
        EXPECT(JOINTS(ctx, F, 3.0, xyz, out, cost, codes, (uint32_t *)xyz, SNOWTRI_HOST), SNOWTRI_ERR_BAD_ARG);
        EXPECT(JOINTS(ctx, F, 3.0, xyz, out, cost, codes, (uint32_t *)(out + 2), SNOWTRI_HOST), SNOWTRI_ERR_BAD_ARG);
        EXPECT(JOINTS(ctx, F, 0.0, xyz, out, cost, codes, (uint32_t *)(out + 2), SNOWTRI_HOST), SNOWTRI_ERR_BAD_ARG);   /* whatever the loss */
        EXPECT(JOINTS(ctx, F, 3.0, xyz, xyz, cost, codes, (uint32_t *)(xyz + 8), SNOWTRI_HOST), SNOWTRI_ERR_BAD_ARG);
        for (i = 0; i < N * 4; i++) failures += out[i] != 0.0;                                /* nothing was written */
        for (i = 0; i < N; i++) failures += codes[i] != 9 || outl[i] != 0xeeeeeeeeu;
        for (i = 0; i < C * 9; i++) failures += Ro[i] != 0.0;
        /* ... and right behind xyz is no overlap */
        EXPECT(JOINTS(ctx, F, 3.0, xyz, out, cost, codes, (uint32_t *)(xyz + 4 * N), SNOWTRI_HOST), SNOWTRI_OK);
        /* F == 0: SNOWTRI_OK, no pointer is looked at */
        EXPECT(JOINTS(ctx, 0, 3.0, NULL, NULL, NULL, NULL, NULL, SNOWTRI_HOST), SNOWTRI_OK);
        EXPECT(CAMS(ctx, 0, 3.0, Ro, to, ccost, nobs, ccodes, normal, noutl, SNOWTRI_HOST), SNOWTRI_OK);
        EXPECT(memcmp(Ro, R, sizeof(double) * 9 * C), 0);
        for (c = 0; c < C; c++) EXPECT(noutl[c] == 0 && nobs[c] == 0, 1);
        EXPECT(noutl[C], 0x7777777777777777ll);
        /* huber_px == 0 is the squared loss: the bytes of the entries without the loss; outliers are zeros */
        EXPECT(snowtri_refine_joints(ctx, F, P, J, xyz, SNOWTRI_F64, PM, kp, SNOWTRI_F64, np, det, views, 0.5, 4, 0u, out0, cost0, codes0, SNOWTRI_HOST, NULL), SNOWTRI_OK);
        EXPECT(JOINTS(ctx, F, 0.0, xyz, out, cost, codes, outl, SNOWTRI_HOST), SNOWTRI_OK);
        EXPECT(memcmp(out, out0, sizeof out0) == 0 && memcmp(cost, cost0, sizeof cost0) == 0 && memcmp(codes, codes0, sizeof codes0) == 0, 1);
        for (i = 0; i < N; i++) failures += outl[i] != 0u;
        EXPECT(outl[N], 0xeeeeeeeeu);
        EXPECT(snowtri_refine_cameras(ctx, F, P, J, xyz, SNOWTRI_F64, PM, kp, SNOWTRI_F64, np, det, views, 0.5, 0xau, 6, 4, 0u, Ro0, to0, ccost0, nobs0, ccodes0, normal0, SNOWTRI_HOST, NULL), SNOWTRI_OK);
        EXPECT(CAMS(ctx, F, 0.0, Ro, to, ccost, nobs, ccodes, normal, noutl, SNOWTRI_HOST), SNOWTRI_OK);
        EXPECT(memcmp(Ro, Ro0, sizeof Ro0) == 0 && memcmp(to, to0, sizeof to0) == 0 && memcmp(ccost, ccost0, sizeof ccost0) == 0, 1);
        EXPECT(memcmp(nobs, nobs0, sizeof nobs0) == 0 && memcmp(ccodes, ccodes0, sizeof ccodes0) == 0 && memcmp(normal, normal0, sizeof normal0) == 0, 1);
        for (c = 0; c < C; c++) EXPECT(noutl[c], 0);
        /* good calls with the loss: joint 0 of every person has camera 2 as an outlier at the output, the other joints have none;
         * the cost does not rise; NULL new outputs are fine; in place is fine */
        EXPECT(JOINTS(ctx, F, 3.0, xyz, out, cost, codes, outl, SNOWTRI_HOST), SNOWTRI_OK);
        any = 0;
        for (i = 0; i < N; i++) {
            EXPECT(codes[i] >= SNOWTRI_REFINE_KEPT && cost[2 * i + 1] <= cost[2 * i], 1);
            EXPECT(outl[i] & ~0xfu, 0);
            if (i % J == 0) any += (outl[i] >> 2) & 1u;
        }
        EXPECT(any, F * P);
        EXPECT(outl[N], 0xeeeeeeeeu);
        EXPECT(JOINTS(ctx, F, 3.0, xyz, out, NULL, NULL, NULL, SNOWTRI_HOST), SNOWTRI_OK);
        EXPECT(CAMS(ctx, F, 3.0, Ro, to, ccost, nobs, ccodes, normal, noutl, SNOWTRI_HOST), SNOWTRI_OK);
        for (c = 0; c < C; c++) {
            EXPECT(nobs[c], N);
            EXPECT(noutl[c] >= 0 && noutl[c] <= N, 1);
            if (c & 1) EXPECT(ccost[2 * c + 1] <= ccost[2 * c], 1);
            else EXPECT(noutl[c] == 0 && ccodes[c] == SNOWTRI_POSE_FIXED, 1);
        }
        EXPECT(noutl[C], 0x7777777777777777ll);
        EXPECT(CAMS(ctx, F, 3.0, Ro, to, NULL, NULL, NULL, NULL, NULL, SNOWTRI_HOST), SNOWTRI_OK);
        EXPECT(JOINTS(ctx, F, 6.0, xyz, xyz, cost, codes, outl, SNOWTRI_HOST), SNOWTRI_OK);
        EXPECT(snowtri_ctx_destroy(ctx), SNOWTRI_OK);
    }
    printf("abi_badargs_huber: %d failure(s)\n", failures);
    return failures;
}
