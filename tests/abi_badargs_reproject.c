/* Drives snowtri_reproject and snowtri_reproject_cost with invalid arguments: the C ABI must report, never crash or read through a
 * bad pointer.  Plain C99, its own main (tests/abi_badargs.c covers the entries that came before).
 *
 *   - without a GPU (tests/test_reproject_host.py builds it against the AddressSanitizer build of the library, `make asan`):
 *     a null context, with good and with bad other arguments;
 *   - with a GPU (tests/test_gpu_reproject.py runs it against libsnowtri.so): the same plus, on real contexts, every refusal that
 *     comes before a launch -- sizes, dtype codes, memory spaces, flag bits, RAW without a lens, a K of the wrong form, a NaN
 *     threshold, more than 256 joints, missing and misaligned pointers, batches past the size limits -- and the empty batch.
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

int main(void) {
    static double xyz[2 * 2 * 5 * 4], pix[2 * 4 * 2 * 5 * 3], kp[2 * 4 * 3 * 5 * 3], cs[2 * 4 * 2 * 3];
    static int32_t cn[2 * 4 * 2 * 3], np[2 * 4];
    const int F = 2, P = 2, J = 5, Pm = 3;
    const uint32_t RAW = SNOWTRI_REPROJECT_RAW;
    volatile double zero = 0.0;
    const double nan = zero / zero;
    int i;
    for (i = 0; i < 2 * 2 * 5; i++) {
        xyz[4 * i] = 0.1 * i;
        xyz[4 * i + 1] = 0.3;
        xyz[4 * i + 2] = 4.0;
        xyz[4 * i + 3] = 1.0;
    }
    for (i = 0; i < 8; i++) np[i] = 3;

    /* ---- null context ---------------------------------------------------------------------------------------- */
#define REPROJECT(ctx_, F_, P_, J_, x_, xdt_, fl_, p_, pdt_, ms_) snowtri_reproject(ctx_, F_, P_, J_, x_, xdt_, fl_, p_, pdt_, ms_, NULL)
#define COST(ctx_, F_, P_, J_, x_, xdt_, Pm_, k_, kdt_, np_, thr_, fl_, s_, n_, ms_) \
    snowtri_reproject_cost(ctx_, F_, P_, J_, x_, xdt_, Pm_, k_, kdt_, np_, thr_, fl_, s_, n_, ms_, NULL)
    EXPECT(REPROJECT(NULL, F, P, J, xyz, SNOWTRI_F64, 0u, pix, SNOWTRI_F64, SNOWTRI_HOST), SNOWTRI_ERR_BAD_ARG);
    EXPECT(REPROJECT(NULL, 0, P, J, NULL, SNOWTRI_F64, 0u, NULL, SNOWTRI_F64, SNOWTRI_HOST), SNOWTRI_ERR_BAD_ARG);
    EXPECT(REPROJECT(NULL, -1, 0, 0, NULL, 9, 8u, NULL, -1, 7), SNOWTRI_ERR_BAD_ARG);
    EXPECT(COST(NULL, F, P, J, xyz, SNOWTRI_F64, Pm, kp, SNOWTRI_F64, np, 0.5, 0u, cs, cn, SNOWTRI_HOST), SNOWTRI_ERR_BAD_ARG);
    EXPECT(COST(NULL, 0, P, J, NULL, SNOWTRI_F64, Pm, NULL, SNOWTRI_F64, NULL, 0.5, 0u, NULL, NULL, SNOWTRI_HOST), SNOWTRI_ERR_BAD_ARG);
    EXPECT(COST(NULL, -1, 0, 0, NULL, 9, 0, NULL, -1, NULL, nan, 8u, NULL, NULL, 7), SNOWTRI_ERR_BAD_ARG);
    EXPECT(snowtri_last_error() != NULL && strstr(snowtri_last_error(), "snowtri_reproject_cost") != NULL, 1);

    /* ---- real contexts (GPU box only) -------------------------------------------------------------------------- */
    if (snowtri_device_count() > 0) {
        snowtri_ctx *ctx = NULL, *none = NULL, *odd = NULL;
        double K[4 * 9], R[4 * 9], t[4 * 3], D[4 * 5], Kodd[9] = {700, 0, 640, 0.001, 700, 360, 0, 0, 1};
        int c;
        memset(D, 0, sizeof D);
        for (c = 0; c < 4; c++) {
            const double k[9] = {700, 0.5, 640, 0, 700, 360, 0, 0, 1}, r[9] = {1, 0, 0, 0, 1, 0, 0, 0, 1};
            memcpy(K + 9 * c, k, sizeof k);
            memcpy(R + 9 * c, r, sizeof r);
            t[3 * c] = 0.5 * c;
            t[3 * c + 1] = 0.0;
            t[3 * c + 2] = 0.0;
            D[5 * c] = -0.1;
        }
        EXPECT(snowtri_ctx_create(4, K, R, t, 0, &ctx), SNOWTRI_OK);
        EXPECT(snowtri_ctx_create(0, NULL, NULL, NULL, 0, &none), SNOWTRI_OK);
        EXPECT(snowtri_ctx_create(1, Kodd, R, t, 0, &odd), SNOWTRI_OK);
        /* a scratch-only context has no cameras to project into; a K with an entry below the diagonal is not the pinhole form */
        EXPECT(REPROJECT(none, F, P, J, xyz, SNOWTRI_F64, 0u, pix, SNOWTRI_F64, SNOWTRI_HOST), SNOWTRI_ERR_BAD_ARG);
        EXPECT(COST(none, F, P, J, xyz, SNOWTRI_F64, Pm, kp, SNOWTRI_F64, np, 0.5, 0u, cs, cn, SNOWTRI_HOST), SNOWTRI_ERR_BAD_ARG);
        EXPECT(REPROJECT(odd, F, P, J, xyz, SNOWTRI_F64, 0u, pix, SNOWTRI_F64, SNOWTRI_HOST), SNOWTRI_ERR_BAD_ARG);
        EXPECT(strstr(snowtri_last_error(), "[[fx, s, cx]") != NULL, 1);
        EXPECT(COST(odd, F, P, J, xyz, SNOWTRI_F64, Pm, kp, SNOWTRI_F64, NULL, 0.5, 0u, cs, cn, SNOWTRI_HOST), SNOWTRI_ERR_BAD_ARG);
        memset(pix, 0, sizeof pix);
        memset(cs, 0, sizeof cs);
        memset(cn, 0, sizeof cn);
        /* snowtri_reproject */
        EXPECT(REPROJECT(ctx, -1, P, J, xyz, SNOWTRI_F64, 0u, pix, SNOWTRI_F64, SNOWTRI_HOST), SNOWTRI_ERR_BAD_ARG);
        EXPECT(REPROJECT(ctx, F, 0, J, xyz, SNOWTRI_F64, 0u, pix, SNOWTRI_F64, SNOWTRI_HOST), SNOWTRI_ERR_BAD_ARG);
        EXPECT(REPROJECT(ctx, F, P, 0, xyz, SNOWTRI_F64, 0u, pix, SNOWTRI_F64, SNOWTRI_HOST), SNOWTRI_ERR_BAD_ARG);
        EXPECT(REPROJECT(ctx, F, P, J, xyz, 7, 0u, pix, SNOWTRI_F64, SNOWTRI_HOST), SNOWTRI_ERR_BAD_ARG);
        EXPECT(REPROJECT(ctx, F, P, J, xyz, SNOWTRI_F64, 0u, pix, -1, SNOWTRI_HOST), SNOWTRI_ERR_BAD_ARG);
        EXPECT(REPROJECT(ctx, F, P, J, xyz, SNOWTRI_F64, 0u, pix, SNOWTRI_F64, 5), SNOWTRI_ERR_BAD_ARG);
        EXPECT(REPROJECT(ctx, F, P, J, xyz, SNOWTRI_F64, 2u, pix, SNOWTRI_F64, SNOWTRI_HOST), SNOWTRI_ERR_BAD_ARG);        /* an unknown flag bit */
        EXPECT(REPROJECT(ctx, F, P, J, xyz, SNOWTRI_F64, RAW, pix, SNOWTRI_F64, SNOWTRI_HOST), SNOWTRI_ERR_BAD_ARG);       /* no D set */
        EXPECT(strstr(snowtri_last_error(), "snowtri_ctx_set_distortion") != NULL, 1);
        EXPECT(REPROJECT(ctx, 0, P, J, NULL, SNOWTRI_F64, RAW, NULL, SNOWTRI_F64, SNOWTRI_HOST), SNOWTRI_ERR_BAD_ARG);     /* ... even on an empty batch */
        EXPECT(REPROJECT(ctx, F, P, J, NULL, SNOWTRI_F64, 0u, pix, SNOWTRI_F64, SNOWTRI_HOST), SNOWTRI_ERR_BAD_ARG);
        EXPECT(REPROJECT(ctx, F, P, J, xyz, SNOWTRI_F64, 0u, NULL, SNOWTRI_F64, SNOWTRI_HOST), SNOWTRI_ERR_BAD_ARG);
        EXPECT(REPROJECT(ctx, F, P, J, (char *)xyz + 4, SNOWTRI_F64, 0u, pix, SNOWTRI_F64, SNOWTRI_DEVICE), SNOWTRI_ERR_BAD_ARG);
        EXPECT(REPROJECT(ctx, F, P, J, xyz, SNOWTRI_F64, 0u, (char *)pix + 2, SNOWTRI_F32, SNOWTRI_DEVICE), SNOWTRI_ERR_BAD_ARG);
        EXPECT(REPROJECT(ctx, ((int64_t)1 << 40), 2000000000, 2000000000, xyz, SNOWTRI_F64, 0u, pix, SNOWTRI_F64, SNOWTRI_HOST), SNOWTRI_ERR_BAD_ARG);
        EXPECT(REPROJECT(ctx, ((int64_t)1 << 62), 1, 1, xyz, SNOWTRI_F64, 0u, pix, SNOWTRI_F64, SNOWTRI_HOST), SNOWTRI_ERR_BAD_ARG);
        EXPECT(strstr(snowtri_last_error(), "observations") != NULL, 1);
        EXPECT(REPROJECT(ctx, 0, P, J, NULL, SNOWTRI_F64, 0u, NULL, SNOWTRI_F64, SNOWTRI_HOST), SNOWTRI_OK);               /* empty batch: no pointer is looked at */
        EXPECT(REPROJECT(ctx, 0, P, J, NULL, SNOWTRI_F32, 0u, NULL, SNOWTRI_F32, SNOWTRI_DEVICE), SNOWTRI_OK);
        /* snowtri_reproject_cost */
        EXPECT(COST(ctx, -1, P, J, xyz, SNOWTRI_F64, Pm, kp, SNOWTRI_F64, np, 0.5, 0u, cs, cn, SNOWTRI_HOST), SNOWTRI_ERR_BAD_ARG);
        EXPECT(COST(ctx, F, 0, J, xyz, SNOWTRI_F64, Pm, kp, SNOWTRI_F64, np, 0.5, 0u, cs, cn, SNOWTRI_HOST), SNOWTRI_ERR_BAD_ARG);
        EXPECT(COST(ctx, F, P, 0, xyz, SNOWTRI_F64, Pm, kp, SNOWTRI_F64, np, 0.5, 0u, cs, cn, SNOWTRI_HOST), SNOWTRI_ERR_BAD_ARG);
        EXPECT(COST(ctx, F, P, 257, xyz, SNOWTRI_F64, Pm, kp, SNOWTRI_F64, np, 0.5, 0u, cs, cn, SNOWTRI_HOST), SNOWTRI_ERR_BAD_ARG);
        EXPECT(strstr(snowtri_last_error(), "256") != NULL, 1);
        EXPECT(COST(ctx, F, P, J, xyz, SNOWTRI_F64, 0, kp, SNOWTRI_F64, np, 0.5, 0u, cs, cn, SNOWTRI_HOST), SNOWTRI_ERR_BAD_ARG);
        EXPECT(COST(ctx, F, P, J, xyz, 7, Pm, kp, SNOWTRI_F64, np, 0.5, 0u, cs, cn, SNOWTRI_HOST), SNOWTRI_ERR_BAD_ARG);
        EXPECT(COST(ctx, F, P, J, xyz, SNOWTRI_F64, Pm, kp, 2, np, 0.5, 0u, cs, cn, SNOWTRI_HOST), SNOWTRI_ERR_BAD_ARG);
        EXPECT(COST(ctx, F, P, J, xyz, SNOWTRI_F64, Pm, kp, SNOWTRI_F64, np, 0.5, 0u, cs, cn, -1), SNOWTRI_ERR_BAD_ARG);
        EXPECT(COST(ctx, F, P, J, xyz, SNOWTRI_F64, Pm, kp, SNOWTRI_F64, np, 0.5, 4u, cs, cn, SNOWTRI_HOST), SNOWTRI_ERR_BAD_ARG);
        EXPECT(COST(ctx, F, P, J, xyz, SNOWTRI_F64, Pm, kp, SNOWTRI_F64, np, 0.5, RAW, cs, cn, SNOWTRI_HOST), SNOWTRI_ERR_BAD_ARG);   /* no D set */
        EXPECT(COST(ctx, F, P, J, xyz, SNOWTRI_F64, Pm, kp, SNOWTRI_F64, np, nan, 0u, cs, cn, SNOWTRI_HOST), SNOWTRI_ERR_BAD_ARG);
        EXPECT(COST(ctx, F, P, J, NULL, SNOWTRI_F64, Pm, kp, SNOWTRI_F64, np, 0.5, 0u, cs, cn, SNOWTRI_HOST), SNOWTRI_ERR_BAD_ARG);
        EXPECT(COST(ctx, F, P, J, xyz, SNOWTRI_F64, Pm, NULL, SNOWTRI_F64, np, 0.5, 0u, cs, cn, SNOWTRI_HOST), SNOWTRI_ERR_BAD_ARG);
        EXPECT(COST(ctx, F, P, J, xyz, SNOWTRI_F64, Pm, kp, SNOWTRI_F64, np, 0.5, 0u, NULL, cn, SNOWTRI_HOST), SNOWTRI_ERR_BAD_ARG);
        EXPECT(COST(ctx, F, P, J, xyz, SNOWTRI_F64, Pm, kp, SNOWTRI_F64, np, 0.5, 0u, cs, NULL, SNOWTRI_HOST), SNOWTRI_ERR_BAD_ARG);
        EXPECT(COST(ctx, F, P, J, xyz, SNOWTRI_F64, Pm, kp, SNOWTRI_F64, np, 0.5, 0u, (double *)((char *)cs + 4), cn, SNOWTRI_DEVICE), SNOWTRI_ERR_BAD_ARG);
        EXPECT(COST(ctx, F, P, J, xyz, SNOWTRI_F64, Pm, kp, SNOWTRI_F64, np, 0.5, 0u, cs, (int32_t *)((char *)cn + 2), SNOWTRI_DEVICE), SNOWTRI_ERR_BAD_ARG);
        EXPECT(COST(ctx, F, P, J, xyz, SNOWTRI_F64, Pm, kp, SNOWTRI_F64, (int32_t *)((char *)np + 1), 0.5, 0u, cs, cn, SNOWTRI_DEVICE), SNOWTRI_ERR_BAD_ARG);
        EXPECT(COST(ctx, ((int64_t)1 << 40), 2000000000, J, xyz, SNOWTRI_F64, Pm, kp, SNOWTRI_F64, np, 0.5, 0u, cs, cn, SNOWTRI_HOST), SNOWTRI_ERR_BAD_ARG);
        EXPECT(COST(ctx, ((int64_t)1 << 30), 1, J, xyz, SNOWTRI_F64, 2000000000, kp, SNOWTRI_F64, np, 0.5, 0u, cs, cn, SNOWTRI_HOST), SNOWTRI_ERR_BAD_ARG);
        EXPECT(COST(ctx, 0, P, J, NULL, SNOWTRI_F64, Pm, NULL, SNOWTRI_F64, NULL, 0.5, 0u, NULL, NULL, SNOWTRI_HOST), SNOWTRI_OK);
        EXPECT(COST(ctx, 0, P, J, NULL, SNOWTRI_F32, Pm, NULL, SNOWTRI_F32, NULL, 0.5, 0u, NULL, NULL, SNOWTRI_DEVICE), SNOWTRI_OK);
        for (i = 0; i < (int)(sizeof pix / sizeof pix[0]); i++) failures += pix[i] != 0.0;    /* nothing was written */
        for (i = 0; i < (int)(sizeof cn / sizeof cn[0]); i++) failures += cn[i] != 0 || cs[i] != 0.0;
        /* with a lens the RAW calls go through, and so do the plain ones: one good call each, so that the refusals above are
         * refusals of their argument and not of everything */
        EXPECT(snowtri_ctx_set_distortion(ctx, D), SNOWTRI_OK);
        EXPECT(REPROJECT(ctx, F, P, J, xyz, SNOWTRI_F64, RAW, pix, SNOWTRI_F64, SNOWTRI_HOST), SNOWTRI_OK);
        EXPECT(pix[2] == 1.0 && pix[0] != 0.0, 1);
        memcpy(kp, pix, sizeof(double) * 3 * J);                                              /* detection 0 of (f 0, c 0) = person 0 as projected */
        EXPECT(COST(ctx, F, P, J, xyz, SNOWTRI_F64, Pm, kp, SNOWTRI_F64, np, 0.5, RAW, cs, cn, SNOWTRI_HOST), SNOWTRI_OK);
        EXPECT(cn[0] == J && cs[0] == 0.0, 1);
        EXPECT(snowtri_ctx_destroy(ctx), SNOWTRI_OK);
        EXPECT(snowtri_ctx_destroy(none), SNOWTRI_OK);
        EXPECT(snowtri_ctx_destroy(odd), SNOWTRI_OK);
    }
    printf("abi_badargs_reproject: %d failure(s)\n", failures);
    return failures;
}
