/* Drives snowtri_assign_detections with invalid arguments: the C ABI must report, never crash or read through a bad pointer.  Plain
 * C99, its own main (tests/abi_badargs_reproject.c covers the entries that write the costs).
 *
 *   - without a GPU (tests/test_assign_host.py builds it against the AddressSanitizer build of the library, `make asan`): every
 *     refusal, told apart by the argument snowtri_last_error() names -- the entry looks at its context last, so each is reached with
 *     a null context too -- then the null context itself, also for n == 0;
 *   - with a GPU (tests/test_gpu_assign.py runs it against libsnowtri.so): the same on a real context, where each refusal is the
 *     refusal of its argument alone, nothing is written, n == 0 is SNOWTRI_OK without a pointer, and one good call in each memory
 *     space's reach (HOST) returns the matching worked out by hand.
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
#define NAMES(word) EXPECT(snowtri_last_error() != NULL && strstr(snowtri_last_error(), word) != NULL, 1)

enum { N = 3, P = 2, PM = 2 };

static double cs[N * P * PM + 1], total[N + 1];
static int32_t cn[N * P * PM + 1], det[N * P + 1], per[N * PM + 1];

#define ASSIGN(ctx_, n_, P_, Pm_, cs_, cn_, g_, mj_, d_, p_, t_, ms_) \
    snowtri_assign_detections(ctx_, n_, P_, Pm_, cs_, cn_, g_, mj_, d_, p_, t_, ms_, NULL)
#define GOOD(ctx_) ASSIGN(ctx_, N, P, PM, cs, cn, 6.0, 8, det, per, total, SNOWTRI_HOST)

/* every refusal that needs no device, on `ctx` (null, or a real one) */
static void refusals(snowtri_ctx *ctx) {
    volatile double zero = 0.0;
    const double nan = zero / zero;
    EXPECT(ASSIGN(ctx, N, P, PM, cs, cn, 6.0, 8, det, per, total, 5), SNOWTRI_ERR_BAD_ARG);
    NAMES("memspace");
    EXPECT(ASSIGN(ctx, -1, P, PM, cs, cn, 6.0, 8, det, per, total, SNOWTRI_HOST), SNOWTRI_ERR_BAD_ARG);
    NAMES("n < 0");
    EXPECT(ASSIGN(ctx, N, 0, PM, cs, cn, 6.0, 8, det, per, total, SNOWTRI_HOST), SNOWTRI_ERR_BAD_ARG);
    NAMES("P < 1");
    EXPECT(ASSIGN(ctx, N, P, 0, cs, cn, 6.0, 8, det, per, total, SNOWTRI_HOST), SNOWTRI_ERR_BAD_ARG);
    NAMES("Pmax < 1");
    EXPECT(ASSIGN(ctx, N, -3, PM, cs, cn, 6.0, 8, det, per, total, SNOWTRI_HOST), SNOWTRI_ERR_BAD_ARG);
    EXPECT(ASSIGN(ctx, N, 32, 33, cs, cn, 6.0, 8, det, per, total, SNOWTRI_HOST), SNOWTRI_ERR_BAD_ARG);
    NAMES("P + Pmax");
    EXPECT(ASSIGN(ctx, N, 2000000000, 2000000000, cs, cn, 6.0, 8, det, per, total, SNOWTRI_HOST), SNOWTRI_ERR_BAD_ARG);
    NAMES("P + Pmax");
    EXPECT(ASSIGN(ctx, N, P, PM, cs, cn, 6.0, 0, det, per, total, SNOWTRI_HOST), SNOWTRI_ERR_BAD_ARG);
    NAMES("min_joints");
    EXPECT(ASSIGN(ctx, N, P, PM, cs, cn, -0.5, 8, det, per, total, SNOWTRI_HOST), SNOWTRI_ERR_BAD_ARG);
    NAMES("gate_px");
    EXPECT(ASSIGN(ctx, N, P, PM, cs, cn, nan, 8, det, per, total, SNOWTRI_HOST), SNOWTRI_ERR_BAD_ARG);
    NAMES("gate_px");
    EXPECT(ASSIGN(ctx, 0, P, PM, NULL, NULL, nan, 8, NULL, NULL, NULL, SNOWTRI_HOST), SNOWTRI_ERR_BAD_ARG);   /* ... even on an empty batch */
    /* a gate above 1e150: staying unmatched costs gate_px^2, which must stay finite */
    EXPECT(ASSIGN(ctx, N, P, PM, cs, cn, 1.0 / zero, 8, det, per, total, SNOWTRI_HOST), SNOWTRI_ERR_BAD_ARG);
    NAMES("1e150");
    EXPECT(ASSIGN(ctx, N, P, PM, cs, cn, 1e200, 8, det, per, total, SNOWTRI_HOST), SNOWTRI_ERR_BAD_ARG);
    NAMES("1e150");
    EXPECT(ASSIGN(ctx, N, P, PM, cs, cn, 1.0000001e150, 8, det, per, total, SNOWTRI_DEVICE), SNOWTRI_ERR_BAD_ARG);
    NAMES("1e150");
    EXPECT(ASSIGN(ctx, N, P, PM, NULL, cn, 6.0, 8, det, per, total, SNOWTRI_HOST), SNOWTRI_ERR_BAD_ARG);
    NAMES("null array");
    EXPECT(ASSIGN(ctx, N, P, PM, cs, NULL, 6.0, 8, det, per, total, SNOWTRI_HOST), SNOWTRI_ERR_BAD_ARG);
    NAMES("null array");
    EXPECT(ASSIGN(ctx, N, P, PM, cs, cn, 6.0, 8, NULL, per, total, SNOWTRI_DEVICE), SNOWTRI_ERR_BAD_ARG);
    NAMES("null array");
    EXPECT(ASSIGN(ctx, N, P, PM, (double *)((char *)cs + 4), cn, 6.0, 8, det, per, total, SNOWTRI_DEVICE), SNOWTRI_ERR_BAD_ARG);
    NAMES("aligned");
    EXPECT(ASSIGN(ctx, N, P, PM, cs, (int32_t *)((char *)cn + 2), 6.0, 8, det, per, total, SNOWTRI_DEVICE), SNOWTRI_ERR_BAD_ARG);
    NAMES("aligned");
    EXPECT(ASSIGN(ctx, N, P, PM, cs, cn, 6.0, 8, (int32_t *)((char *)det + 1), per, total, SNOWTRI_DEVICE), SNOWTRI_ERR_BAD_ARG);
    NAMES("aligned");
    EXPECT(ASSIGN(ctx, N, P, PM, cs, cn, 6.0, 8, det, (int32_t *)((char *)per + 2), total, SNOWTRI_DEVICE), SNOWTRI_ERR_BAD_ARG);
    NAMES("aligned");
    EXPECT(ASSIGN(ctx, N, P, PM, cs, cn, 6.0, 8, det, per, (double *)((char *)total + 4), SNOWTRI_DEVICE), SNOWTRI_ERR_BAD_ARG);
    NAMES("aligned");
    EXPECT(ASSIGN(ctx, ((int64_t)1 << 48) / (32 * 32) + 1, 32, 32, cs, cn, 6.0, 8, det, per, total, SNOWTRI_HOST), SNOWTRI_ERR_BAD_ARG);
    NAMES("2^48");
    EXPECT(ASSIGN(ctx, ((int64_t)1 << 62), 1, 1, cs, cn, 6.0, 8, det, per, total, SNOWTRI_HOST), SNOWTRI_ERR_BAD_ARG);
    NAMES("2^48");
    EXPECT(ASSIGN(ctx, ((int64_t)1 << 44), 1, 1, cs, cn, 6.0, 8, det, per, total, SNOWTRI_HOST), SNOWTRI_ERR_BAD_ARG);
    NAMES("workgroups");
}

int main(void) {
    int i;
    /* three problems, means over 10 joints against gate2 = 36:
     *   0: [[4, 20], [9, 16]]  both persons closest to detection 0 -> (0, 1), total 20
     *   1: [[4, 50], [9, 40]]  detection 1 outside the gate      -> (0, -1), total 4
     *   2: nothing admissible (too few joints)                    -> (-1, -1), total 0 */
    const double m[N * P * PM] = {4, 20, 9, 16, 4, 50, 9, 40, 1, 1, 1, 1};
    for (i = 0; i < N * P * PM; i++) {
        cn[i] = i < 8 ? 10 : 7;
        cs[i] = m[i] * cn[i];
    }
    for (i = 0; i < N * P; i++) det[i] = 77;
    for (i = 0; i < N * PM; i++) per[i] = 77;
    for (i = 0; i < N; i++) total[i] = 77.0;

    /* ---- null context ---------------------------------------------------------------------------------------- */
    refusals(NULL);
    EXPECT(GOOD(NULL), SNOWTRI_ERR_BAD_ARG);
    NAMES("null context");
    EXPECT(ASSIGN(NULL, 0, P, PM, NULL, NULL, 6.0, 8, NULL, NULL, NULL, SNOWTRI_HOST), SNOWTRI_ERR_BAD_ARG);
    NAMES("null context");
    NAMES("snowtri_assign_detections");

    /* ---- a real context (GPU box only) ------------------------------------------------------------------------- */
    if (snowtri_device_count() > 0) {
        snowtri_ctx *ctx = NULL;
        const int32_t want_det[N * P] = {0, 1, 0, -1, -1, -1}, want_per[N * PM] = {0, 1, 0, -1, -1, -1};
        const double want_total[N] = {20.0, 4.0, 0.0};
        EXPECT(snowtri_ctx_create(0, NULL, NULL, NULL, 0, &ctx), SNOWTRI_OK);                 /* the rig is not used */
        refusals(ctx);
        EXPECT(ASSIGN(ctx, 0, P, PM, NULL, NULL, 6.0, 8, NULL, NULL, NULL, SNOWTRI_HOST), SNOWTRI_OK);     /* empty: no pointer is looked at */
        EXPECT(ASSIGN(ctx, 0, 1, 63, NULL, NULL, 0.0, 1, NULL, NULL, NULL, SNOWTRI_DEVICE), SNOWTRI_OK);
        for (i = 0; i < N * P; i++) failures += det[i] != 77;                                 /* nothing was written */
        for (i = 0; i < N * PM; i++) failures += per[i] != 77;
        for (i = 0; i < N; i++) failures += total[i] != 77.0;
        /* one good call, so that the refusals above are refusals of their argument and not of everything */
        EXPECT(GOOD(ctx), SNOWTRI_OK);
        EXPECT(memcmp(det, want_det, sizeof want_det), 0);
        EXPECT(memcmp(per, want_per, sizeof want_per), 0);
        EXPECT(memcmp(total, want_total, sizeof want_total), 0);
        for (i = 0; i < N * P; i++) det[i] = 77;
        EXPECT(ASSIGN(ctx, N, P, PM, cs, cn, 6.0, 8, det, NULL, NULL, SNOWTRI_HOST), SNOWTRI_OK);      /* the optional outputs left out */
        EXPECT(memcmp(det, want_det, sizeof want_det), 0);
        /* the largest gate still taken: everything with enough joints is admissible -> (0, 1), (0, 1), (-1, -1) */
        {
            const int32_t want_wide[N * P] = {0, 1, 0, 1, -1, -1};
            EXPECT(ASSIGN(ctx, N, P, PM, cs, cn, 1e150, 8, det, NULL, NULL, SNOWTRI_HOST), SNOWTRI_OK);
            EXPECT(memcmp(det, want_wide, sizeof want_wide), 0);
        }
        EXPECT(snowtri_ctx_destroy(ctx), SNOWTRI_OK);
    }
    printf("abi_badargs_assign: %d failure(s)\n", failures);
    return failures;
}
