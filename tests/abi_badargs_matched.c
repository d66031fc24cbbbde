/* Drives snowtri_triangulate_matched with invalid arguments: the C ABI must report, never crash or read through a bad pointer.
 * Plain C99, its own main.
 *
 *   - without a GPU (tests/test_matched_host.py builds it against the AddressSanitizer build of the library, `make asan`): a null
 *     context, with good and with bad other arguments;
 *   - with a GPU (tests/test_gpu_matched.py runs it against libsnowtri.so): the same plus, on real contexts, every refusal that comes
 *     before a launch -- sizes, dtype codes, memory spaces, a NaN threshold, the robust settings, 1 and 9 cameras, P > Pmax without
 *     det_of, missing and misaligned pointers, a batch past the size limits, P * kn past the LDS -- the empty batch, and one good call.
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

enum { F = 2, P = 2, J = 5, PM = 3, C = 4, N = F * P * J };

int main(void) {
    static double out[N * 4 + 4], kp[F * C * PM * J * 3 + 3], ps[F * P], resid[N + 1];
    static uint32_t views[N + 1];
    static int32_t np[F * C + 1], det[F * C * P + 1];
    volatile double zero = 0.0;
    const double nan = zero / zero;
    int i;
    for (i = 0; i < F * C; i++) np[i] = PM;
    for (i = 0; i < F * C * P; i++) det[i] = (i % P) + 1;      /* person p is detection p + 1 */

#define TRI(ctx_, F_, P_, J_, Pm_, k_, kdt_, np_, det_, thr_, tau_, md_, o_, ps_, odt_, vw_, rs_, ms_) \
    snowtri_triangulate_matched(ctx_, F_, P_, J_, Pm_, k_, kdt_, np_, det_, thr_, tau_, md_, o_, ps_, odt_, vw_, rs_, ms_, NULL)
#define GOOD(ctx_) TRI(ctx_, F, P, J, PM, kp, SNOWTRI_F64, np, det, 0.5, 6.0, 1, out, ps, SNOWTRI_F64, views, resid, SNOWTRI_HOST)
    /* ---- null context ---------------------------------------------------------------------------------------- */
    EXPECT(GOOD(NULL), SNOWTRI_ERR_BAD_ARG);
    EXPECT(TRI(NULL, 0, P, J, PM, NULL, SNOWTRI_F64, NULL, NULL, 0.5, 6.0, 1, NULL, NULL, SNOWTRI_F64, NULL, NULL, SNOWTRI_HOST), SNOWTRI_ERR_BAD_ARG);
    EXPECT(TRI(NULL, -1, 0, 0, 0, NULL, 9, NULL, NULL, nan, -1.0, 9, NULL, NULL, -1, NULL, NULL, 7), SNOWTRI_ERR_BAD_ARG);
    SAYS("snowtri_triangulate_matched");

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
            t[3 * c + 1] = 0.1 * (c % 3);
            t[3 * c + 2] = 0.0;
        }
        /* detection q of every camera shows the point (0.1 q + 0.05 j, 0.3, 4); person p is detection p + 1 */
        for (f = 0; f < F; f++)
            for (c = 0; c < C; c++)
                for (p = 0; p < PM; p++)
                    for (j = 0; j < J; j++) {
                        double *o = kp + 3 * (((f * C + c) * PM + p) * J + j);
                        const double px = (0.1 * p + 0.05 * j - t[3 * c]) / 4.0, py = (0.3 - t[3 * c + 1]) / 4.0;
                        o[0] = 700 * px + 0.5 * py + 640;
                        o[1] = 700 * py + 360;
                        o[2] = 1.0;
                    }
        EXPECT(snowtri_ctx_create(4, K, R, t, 0, &ctx), SNOWTRI_OK);
        EXPECT(snowtri_ctx_create(1, K, R, t, 0, &one), SNOWTRI_OK);
        EXPECT(snowtri_ctx_create(9, K, R, t, 0, &nine), SNOWTRI_OK);
        memset(out, 0, sizeof out);
        memset(ps, 0, sizeof ps);
        memset(views, 0, sizeof views);
        memset(resid, 0, sizeof resid);
        EXPECT(GOOD(one), SNOWTRI_ERR_BAD_ARG);
        SAYS("2 to 8 cameras");
        EXPECT(GOOD(nine), SNOWTRI_ERR_BAD_ARG);
        SAYS("2 to 8 cameras");
        EXPECT(TRI(ctx, -1, P, J, PM, kp, SNOWTRI_F64, np, det, 0.5, 6.0, 1, out, ps, SNOWTRI_F64, views, resid, SNOWTRI_HOST), SNOWTRI_ERR_BAD_ARG);
        EXPECT(TRI(ctx, F, 0, J, PM, kp, SNOWTRI_F64, np, det, 0.5, 6.0, 1, out, ps, SNOWTRI_F64, views, resid, SNOWTRI_HOST), SNOWTRI_ERR_BAD_ARG);
        EXPECT(TRI(ctx, F, P, 0, PM, kp, SNOWTRI_F64, np, det, 0.5, 6.0, 1, out, ps, SNOWTRI_F64, views, resid, SNOWTRI_HOST), SNOWTRI_ERR_BAD_ARG);
        EXPECT(TRI(ctx, F, P, J, 0, kp, SNOWTRI_F64, np, det, 0.5, 6.0, 1, out, ps, SNOWTRI_F64, views, resid, SNOWTRI_HOST), SNOWTRI_ERR_BAD_ARG);
        SAYS("Pmax");
        EXPECT(TRI(ctx, F, P, J, PM, kp, 7, np, det, 0.5, 6.0, 1, out, ps, SNOWTRI_F64, views, resid, SNOWTRI_HOST), SNOWTRI_ERR_BAD_ARG);
        EXPECT(TRI(ctx, F, P, J, PM, kp, SNOWTRI_F64, np, det, 0.5, 6.0, 1, out, ps, 2, views, resid, SNOWTRI_HOST), SNOWTRI_ERR_BAD_ARG);
        SAYS("dtype");
        EXPECT(TRI(ctx, F, P, J, PM, kp, SNOWTRI_F64, np, det, 0.5, 6.0, 1, out, ps, SNOWTRI_F64, views, resid, 5), SNOWTRI_ERR_BAD_ARG);
        SAYS("memspace");
        EXPECT(TRI(ctx, F, P, J, PM, kp, SNOWTRI_F64, np, det, nan, 6.0, 1, out, ps, SNOWTRI_F64, views, resid, SNOWTRI_HOST), SNOWTRI_ERR_BAD_ARG);
        SAYS("keypoint_score_threshold");
        EXPECT(TRI(ctx, F, P, J, PM, kp, SNOWTRI_F64, np, det, 0.5, -0.5, 1, out, ps, SNOWTRI_F64, views, resid, SNOWTRI_HOST), SNOWTRI_ERR_BAD_ARG);
        EXPECT(TRI(ctx, F, P, J, PM, kp, SNOWTRI_F64, np, det, 0.5, nan, 1, out, ps, SNOWTRI_F64, views, resid, SNOWTRI_HOST), SNOWTRI_ERR_BAD_ARG);
        SAYS("reproj_threshold_px");
        EXPECT(TRI(ctx, F, P, J, PM, kp, SNOWTRI_F64, np, det, 0.5, 6.0, -1, out, ps, SNOWTRI_F64, views, resid, SNOWTRI_HOST), SNOWTRI_ERR_BAD_ARG);
        EXPECT(TRI(ctx, F, P, J, PM, kp, SNOWTRI_F64, np, det, 0.5, 6.0, 7, out, ps, SNOWTRI_F64, views, resid, SNOWTRI_HOST), SNOWTRI_ERR_BAD_ARG);
        SAYS("max_drops");
        EXPECT(TRI(ctx, 0, P, J, PM, NULL, SNOWTRI_F64, NULL, NULL, 0.5, 6.0, 7, NULL, NULL, SNOWTRI_F64, NULL, NULL, SNOWTRI_HOST), SNOWTRI_ERR_BAD_ARG);   /* ... even on an empty batch */
        EXPECT(TRI(ctx, F, 4, J, PM, kp, SNOWTRI_F64, np, NULL, 0.5, 6.0, 1, out, ps, SNOWTRI_F64, views, resid, SNOWTRI_HOST), SNOWTRI_ERR_BAD_ARG);       /* P = 4 > Pmax = 3, no det_of */
        SAYS("det_of");
        EXPECT(TRI(ctx, F, P, J, PM, NULL, SNOWTRI_F64, np, det, 0.5, 6.0, 1, out, ps, SNOWTRI_F64, views, resid, SNOWTRI_HOST), SNOWTRI_ERR_BAD_ARG);
        SAYS("null array");
        EXPECT(TRI(ctx, F, P, J, PM, kp, SNOWTRI_F64, np, det, 0.5, 6.0, 1, NULL, ps, SNOWTRI_F64, views, resid, SNOWTRI_HOST), SNOWTRI_ERR_BAD_ARG);
        SAYS("out_xyzs");
        EXPECT(TRI(ctx, F, P, J, PM, (char *)kp + 4, SNOWTRI_F64, np, det, 0.5, 6.0, 1, out, ps, SNOWTRI_F64, views, resid, SNOWTRI_DEVICE), SNOWTRI_ERR_BAD_ARG);
        EXPECT(TRI(ctx, F, P, J, PM, kp, SNOWTRI_F64, (int32_t *)((char *)np + 1), det, 0.5, 6.0, 1, out, ps, SNOWTRI_F64, views, resid, SNOWTRI_DEVICE), SNOWTRI_ERR_BAD_ARG);
        EXPECT(TRI(ctx, F, P, J, PM, kp, SNOWTRI_F64, np, (int32_t *)((char *)det + 2), 0.5, 6.0, 1, out, ps, SNOWTRI_F64, views, resid, SNOWTRI_DEVICE), SNOWTRI_ERR_BAD_ARG);
        EXPECT(TRI(ctx, F, P, J, PM, kp, SNOWTRI_F64, np, det, 0.5, 6.0, 1, (char *)out + 8, ps, SNOWTRI_F64, views, resid, SNOWTRI_DEVICE), SNOWTRI_ERR_BAD_ARG);
        EXPECT(TRI(ctx, F, P, J, PM, kp, SNOWTRI_F64, np, det, 0.5, 6.0, 1, out, (char *)ps + 4, SNOWTRI_F64, views, resid, SNOWTRI_DEVICE), SNOWTRI_ERR_BAD_ARG);
        EXPECT(TRI(ctx, F, P, J, PM, kp, SNOWTRI_F64, np, det, 0.5, 6.0, 1, out, ps, SNOWTRI_F64, (uint32_t *)((char *)views + 2), resid, SNOWTRI_DEVICE), SNOWTRI_ERR_BAD_ARG);
        EXPECT(TRI(ctx, F, P, J, PM, kp, SNOWTRI_F64, np, det, 0.5, 6.0, 1, out, ps, SNOWTRI_F64, views, (char *)resid + 4, SNOWTRI_DEVICE), SNOWTRI_ERR_BAD_ARG);
        SAYS("aligned");
        EXPECT(TRI(ctx, ((int64_t)1 << 62), 1, 1, 1, kp, SNOWTRI_F64, np, det, 0.5, 6.0, 1, out, ps, SNOWTRI_F64, views, resid, SNOWTRI_HOST), SNOWTRI_ERR_BAD_ARG);
        SAYS("records");
        EXPECT(TRI(ctx, F, 200, 133, 200, kp, SNOWTRI_F64, np, det, 0.5, 6.0, 1, out, ps, SNOWTRI_F64, views, resid, SNOWTRI_HOST), SNOWTRI_ERR_BAD_ARG);   /* 26 600 scores per frame */
        SAYS("LDS");
        EXPECT(TRI(ctx, 0, P, J, PM, NULL, SNOWTRI_F64, NULL, NULL, 0.5, 6.0, 1, NULL, NULL, SNOWTRI_F64, NULL, NULL, SNOWTRI_HOST), SNOWTRI_OK);           /* empty batch: no pointer is looked at */
        EXPECT(TRI(ctx, 0, P, J, PM, NULL, SNOWTRI_F32, NULL, NULL, 0.5, 6.0, 1, NULL, NULL, SNOWTRI_F32, NULL, NULL, SNOWTRI_DEVICE), SNOWTRI_OK);
        for (i = 0; i < N * 4; i++) failures += out[i] != 0.0;                                /* nothing was written */
        for (i = 0; i < N; i++) failures += views[i] != 0u || resid[i] != 0.0;
        /* one good call, so that the refusals above are refusals of their argument and not of everything: exact pixels of four
         * cameras give the point back, every view kept, no residual to speak of */
        EXPECT(GOOD(ctx), SNOWTRI_OK);
        EXPECT(strncmp(snowtri_last_kernel_names(ctx), "k_dlt_matched<4,double,double>", 30), 0);
        for (f = 0; f < F; f++)
            for (p = 0; p < P; p++) {
                EXPECT(fabs(ps[f * P + p] - 1.0) < 1e-12, 1);
                for (j = 0; j < J; j++) {
                    const double *o = out + 4 * ((f * P + p) * J + j);
                    i = (f * P + p) * J + j;
                    EXPECT(fabs(o[0] - (0.1 * (p + 1) + 0.05 * j)) < 1e-9 && fabs(o[1] - 0.3) < 1e-9 && fabs(o[2] - 4.0) < 1e-9 && fabs(o[3] - 1.0) < 1e-12, 1);
                    EXPECT(views[i], 0xfu);
                    EXPECT(resid[i] >= 0.0 && resid[i] < 1e-6, 1);
                }
            }
        EXPECT(snowtri_ctx_destroy(ctx), SNOWTRI_OK);
        EXPECT(snowtri_ctx_destroy(one), SNOWTRI_OK);
        EXPECT(snowtri_ctx_destroy(nine), SNOWTRI_OK);
    }
    printf("abi_badargs_matched: %d failure(s)\n", failures);
    return failures;
}
