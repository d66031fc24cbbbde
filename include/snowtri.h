/*
 * snowtri.h -- C ABI of the MI355X-native multi-view triangulation core (libsnowtri.so).
 *
 * Drop-in boundary for ONE path of liaochikon/SnowMocap: 2D keypoints from C calibrated cameras
 * -> pairwise two-ray triangulation + scoring -> cross-view association / fusion ("condense").
 * The reference has no FFI of its own (it is pure Python); each entry point below names the
 * reference interface it replaces (file:line relative to the reference tree).  A maintainer binds
 * them with ctypes -- see INTEGRATION.md; snowmocap_amd/_lib.py is that binding.
 *
 * Conventions
 *   - plain pointers and sizes only; caller allocates every input and output buffer;
 *   - the library owns only the opaque context (rig constants + device scratch);
 *   - every function returns a snowtri_status; nothing throws across the ABI;
 *   - `memspace` says whether the data pointers are host (SNOWTRI_HOST: staged through the
 *     context's device scratch, synchronous) or device (SNOWTRI_DEVICE: used in place,
 *     asynchronous on `stream`, a hipStream_t passed as void*; NULL = the null stream);
 *   - all arithmetic is IEEE fp64 on the GPU (the reference is NumPy float64); only the I/O
 *     element type is selectable (snowtri_dtype);
 *   - a context is not thread-safe; distinct contexts may be used concurrently.
 *
 * Layouts (row-major, innermost last)
 *   kpts       [F][C][Pmax][J][3]   (u, v, score) per detected keypoint; persons p >= n_persons[f][c] ignored
 *   n_persons  [F][C] int32         detections per camera in add_human_2D_points call order; NULL = Pmax everywhere
 *   candidates slot k = pair(mc<sc) * Pmax*Pmax + pm * Pmax + ps, pairs in the reference's loop order
 *              (triangulation.py:56-65), so increasing k over valid slots IS the reference's list order
 *   out_xyzs   [F][Pout_max][keypoint_num][4]  (x, y, z, keypoint score)
 */
#ifndef SNOWTRI_H
#define SNOWTRI_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define SNOWTRI_VERSION 100 /* 0.1.0 */

typedef struct snowtri_ctx snowtri_ctx;

/* Thresholds of Human_Triangulation (triangulation.py:50) and Human_Triangulation_Condense
 * (triangulation.py:95-100); JSON keys of configs/snowmocap_default_config.json:10-17. */
typedef struct snowtri_params {
    double keypoint_score_threshold;
    double average_score_threshold;
    double distance_threshold;
    double condense_distance_tol;
    double condense_person_num_tol;
    double condense_score_tol;
    int32_t center_point_index;
    int32_t keypoint_num;
} snowtri_params;

typedef enum snowtri_status {
    SNOWTRI_OK = 0,
    SNOWTRI_ERR_BAD_ARG = 1,    /* null pointer, non-positive size, unsupported dtype/method        */
    SNOWTRI_ERR_BAD_INDEX = 2,  /* center_point_index / keypoint_num outside [0, J]  (IndexError)   */
    SNOWTRI_ERR_HIP = 3,        /* a HIP call failed: see snowtri_last_error()                      */
    SNOWTRI_ERR_SINGULAR = 4,   /* an exactly singular ray pair was met (np.linalg.LinAlgError)     */
    SNOWTRI_ERR_OVERFLOW = 5,   /* more output persons than Pout_max in some frame (count is true)  */
    SNOWTRI_ERR_NO_DEVICE = 6   /* no HIP device visible                                            */
} snowtri_status;

typedef enum snowtri_dtype { SNOWTRI_F32 = 0, SNOWTRI_F64 = 1 } snowtri_dtype;
typedef enum snowtri_memspace { SNOWTRI_HOST = 0, SNOWTRI_DEVICE = 1 } snowtri_memspace;
typedef enum snowtri_method {
    SNOWTRI_PAIRWISE = 0, /* the reference's algorithm: pairwise skew-ray midpoints, score-weighted */
    SNOWTRI_DLT = 1,      /* N-view DLT (A^T A smallest eigenvector; NOT reference behaviour), solved in the RIG'S OWN
                           * FRAME: c = the fp64 mean of the camera centres (summed in camera order, divided by C),
                           * s = max over cameras and axes of |t_c - c| (1 when that is 0); the rows u P'[2] - P'[0],
                           * v P'[2] - P'[1] come from P'_c = K_c [R_c^T | -R_c^T (t_c - c) / s]; with e the smallest
                           * eigenvector of A^T A, X = c + s e[0:3] / e[3].  The constraint |e| = 1 is not invariant
                           * under moving or rescaling the world, so the frame is part of the definition: in this one
                           * the same footage gives the same joints wherever the calibration put its origin and
                           * whatever its unit, and A^T A in fp64 keeps its accuracy (2.5e-10 s tested) there.
                           * One detection per camera: no association.  Several: the reference's association (candidates +
                           * greedy clustering: the streaming kernels of the pairwise method), then one DLT per
                           * cluster over its distinct observations (k_cluster_dlt; with condense_score_tol > 0,
                           * which is decided on the DLT joint scores, every frame inside k_frame_recompute<1>).
                           * Shape limits of that multi-detection route (and of DLT with more than 8 cameras):
                           * at most 16 cameras, C * Pmax <= 1024 detections per frame, keypoint_num <= 256;
                           * beyond them snowtri_triangulate_condense returns SNOWTRI_ERR_BAD_ARG and
                           * snowtri_last_error() says why.  SNOWTRI_PAIRWISE has no such limit (larger rigs
                           * fall back to the kernel that spills its candidates to HBM). */
    SNOWTRI_DLT_ROBUST = 2 /* SNOWTRI_DLT with a leave-one-out gate on the reprojection residual (NOT reference behaviour): the
                            * rule is stated at snowtri_triangulate_robust below.  One detection per camera (Pmax == 1) on 2 to 8
                            * cameras; anything else is SNOWTRI_ERR_BAD_ARG and snowtri_last_error() names the limit.  Through
                            * snowtri_triangulate_condense[_ex] it runs with the context's settings (snowtri_ctx_set_robust). */
} snowtri_method;

/* per-frame flag bits written to out_flags */
#define SNOWTRI_FLAG_SINGULAR 1u /* exactly singular pair in this frame                  */
#define SNOWTRI_FLAG_OVERFLOW 2u /* more than Pout_max persons; extra persons not written */
#define SNOWTRI_FLAG_FASTPATH 4u /* frame was resolved by the single-cluster fast path    */

int snowtri_version(void);
const char *snowtri_status_string(int status);
/* Message of the last failing HIP call on this thread ("" if none). */
const char *snowtri_last_error(void);
/* Number of visible HIP devices (0 on a CPU-only box; never fails). */
int snowtri_device_count(void);

/* What this binary is: "version=<n>;arch=gfx950;variants=<comma-separated build variants>".  The production library
 * reports an empty variant list; the test build libsnowtri_dbg.so reports SNOWTRI_DEBUG_BOUNDS,SNOWTRI_TEST_KNOBS; development
 * builds name their switches (snowmocap_amd/csrc/snowtri_math.hpp lists them).  Never fails; the string lives as long as the library. */
const char *snowtri_build_info(void);

/* Rig constants.  Replaces Camera.__init__/CameraGroup.__init__ state used by the path
 * (camera.py:17-44,142-157): K[C][9], R[C][9] (camera->world), t[C][3] (camera centre), fp64.
 * C == 0 gives a scratch-only context (enough for snowtri_condense / snowtri_skew_ray_batch). */
int snowtri_ctx_create(int32_t C, const double *K, const double *R, const double *t, int device,
                       snowtri_ctx **out);
int snowtri_ctx_destroy(snowtri_ctx *ctx);
int snowtri_ctx_num_cameras(const snowtri_ctx *ctx);
/* Host copy of the per-camera ray matrices M_c = R_c * inv(K_c), [C][9] fp64. */
int snowtri_ctx_ray_matrices(const snowtri_ctx *ctx, double *M_out);
/* Block until everything queued by this context has finished. */
int snowtri_ctx_synchronize(snowtri_ctx *ctx);
/* Test knobs.  The PRODUCTION library reads no environment and snowtri_ctx_overrides() returns "" for every context of it.
 * The TEST build (-DSNOWTRI_TEST_KNOBS: snowmocap_amd/libsnowtri_dbg.so, which also carries the device-side bounds checks;
 * snowtri_build_info() names both variants) reads these environment variables ONCE, when a context is created, and names the
 * ones that were set as "NAME=value,..." (tests assert on it):
 *   SNOWTRI_GENERAL_MODE=1|2        multi-person batches on the spill kernel / on k_frame_recompute
 *   SNOWTRI_LEAN_MODE=0             float32-output single-detection batches stay on k_fused_single (DLT: off k_dlt_coop)
 *   SNOWTRI_LEAN_COOP=0             small launches stay on k_fused_lean
 *   SNOWTRI_SUMLESS_MODE=0          single-detection batches on the streaming route keep its candidate pass
 *   SNOWTRI_HANDOVER_MODE=0|2       0: the whole multi-person path inside k_frame_recompute; 2: its descriptors to k_cluster_fuse
 *   SNOWTRI_HANDOVER_SEG_FRAMES=n   frames per segment of the streaming multi-person route
 *   SNOWTRI_SPLIT_SEGMENTS=1|n      1: one multi-person call stays on the caller's stream; n >= 2: at least n segments alternating
 *                                   between the caller's stream and an internal one, also for small batches (default: 2
 *                                   segments once a segment holds >= 4 frames per CU)
 *   SNOWTRI_SUMS_THREADS, SNOWTRI_SUMS_LDS_KB, SNOWTRI_LEAN_TILES_PER_WAVE   launch shapes (tests force the rare ones)
 *   SNOWTRI_DEBUG=1                 launch shapes on stderr
 * Results never depend on a knob (that is what the tests that set them check); only the route does. */
const char *snowtri_ctx_overrides(const snowtri_ctx *ctx);

/* OVERLAP MODE for SNOWTRI_DEVICE calls of snowtri_triangulate_condense (off = 1 by default).  With n_streams = 2..4 the
 * context issues consecutive calls round-robin on n internal streams, each behind whatever `stream` held at the time of the
 * call: the ramp-up of one launch overlaps the tail of the previous one (a 10 000-frame step of the single-person path:
 * 26 -> 20 us per call), without the caller creating streams or twin contexts.  The calls must be independent (distinct
 * output buffers; inputs ready on `stream` when the call is made).  Results become visible to the caller's stream at
 * snowtri_ctx_join(ctx, stream) -- `stream` then waits for every call issued since the last join -- or after
 * snowtri_ctx_synchronize.  SNOWTRI_HOST calls are synchronous and ignore the mode.  An overlapped call whose `stream` is
 * capturing a hipGraph is refused with SNOWTRI_ERR_BAD_ARG (GRAPH CAPTURE below).
 * Ordering rule: an overlapped call owns the scratch set of ITS internal stream (one set per stream, none of them the
 * caller's); every other entry point -- host calls, snowtri_triangulate / snowtri_condense_resident, device calls made
 * with the mode off -- works on the caller's own set, ordered by the stream it is given.  So entry points may be mixed
 * freely with overlapped calls in flight; only the OUTPUTS of an overlapped call need the join before they are read. */
int snowtri_ctx_set_overlap(snowtri_ctx *ctx, int n_streams);
int snowtri_ctx_join(snowtri_ctx *ctx, void *stream);
/* Settings of method = SNOWTRI_DLT_ROBUST through snowtri_triangulate_condense[_ex]: the residual gate in pixels and the number of
 * views one joint may lose.  A fresh context has 6.0 px and 1 drop.  THOSE DEFAULTS COME FROM A SYNTHETIC CHECK, NOT FROM RECORDED
 * FOOTAGE: the project's generator (ring rigs and the floor rig, 1 px of pixel noise, one camera shifted by 20-150 px on 10 % of
 * the joints), where 6 px removed every shifted view and no clean one; a detector with heavier tails wants its own value.
 * A negative or NaN threshold is SNOWTRI_ERR_BAD_ARG, +infinity is allowed (nothing is dropped: the result is SNOWTRI_DLT's);
 * max_drops outside [0, 6] is SNOWTRI_ERR_BAD_ARG (0: SNOWTRI_DLT's result). */
int snowtri_ctx_set_robust(snowtri_ctx *ctx, double reproj_threshold_px, int32_t max_drops);
/* THE SPLIT of one multi-person call (several detections per camera, the streaming route).  By default a call whose batch fills
 * the chip at least twice (a segment holds >= 4 frames per CU) runs as two segments that alternate between the caller's stream
 * and ONE internal stream (fork / join events inside the call, results ordered behind `stream` as always): the latency-bound
 * kernels of one segment run beside the VALU-bound ones of the other (8 cameras x 4 persons: +8 %).  Outputs do not depend on
 * the cut (tested bit for bit).  segments = 1: the whole call stays on the caller's stream -- for a caller that profiles its
 * kernels one at a time (scripts/pmc_multi.sh), and what a capture of the call into a hipGraph on one stream would need (such a
 * capture is NOT among the tested ones: GRAPH CAPTURE below); segments = 2 .. 64: at least that many segments (rounded up to an
 * even count), small batches included; 0: the default policy again.  Not used in overlap mode (whole calls alternate there). */
int snowtri_ctx_set_split(snowtri_ctx *ctx, int segments);

/* GRAPH CAPTURE.  A SNOWTRI_DEVICE call whose entry says "asynchronous on `stream`, no host read, no allocation, no internal
 * stream" may be captured into a hipGraph (hipStreamBeginCapture on `stream`, or torch.cuda.graph) and replayed: every per-call
 * reset (counters, flags, tickets, the tracker's state) is a node of the graph, and launch shapes come from the call's shapes and
 * the device, never from its data.  Replays give the bits of the eager call on the same inputs (tests/test_gpu_graph_capture.py).
 * Captured and replayed there: snowtri_triangulate_condense[_ex] and snowtri_triangulate_robust on the single-launch routes (one
 * detection per camera: k_fused_lean_coop, k_fused_lean, k_fused_single, k_dlt_coop, k_dlt_robust), snowtri_undistort_keypoints,
 * snowtri_reproject, snowtri_reproject_cost, snowtri_assign_detections, snowtri_triangulate_matched, snowtri_pair_cost,
 * snowtri_seed_persons, snowtri_refine_joints[_ex], snowtri_refine_cameras, snowtri_track_persons, snowtri_track_gather,
 * snowtri_fill_joint_track, snowtri_despike_joint_track.  NOT verified, keep these calls outside a graph: the multi-person routes
 * of the fused call (several detections per camera, or five and more cameras off the lean shapes: the streaming association and
 * k_frame_recompute) and the smoothing entries (snowtri_smooth_track, snowtri_smooth_joint_track, snowtri_blender_points,
 * snowtri_blender_smooth and the shard passes).  A graph of either kind ended the test process while the graph was destroyed;
 * what the two share is a hipMemsetAsync node (the counter words, the scan's ticket and flags), and the cause is not established.
 * Preconditions:
 *   - ONE EAGER WARM-UP CALL with the same shapes, dtypes and options on the same context before the capture: scratch buffers,
 *     the workspaces of snowtri_refine_cameras and snowtri_refine_cameras_k, the coefficient table of snowtri_blender_smooth and the raised LDS limits are
 *     created by the first call (hipMalloc, a blocking copy), which a capturing stream forbids;
 *   - overlap mode off (snowtri_ctx_set_overlap(ctx, 1)): with n_streams >= 2 a call on a capturing stream is refused with
 *     SNOWTRI_ERR_BAD_ARG before any other runtime call (the capture stays valid; snowtri_last_error() names overlap mode);
 *   - timing off (snowtri_set_timing(ctx, 0)): the event pairs belong to the context, not to the graph;
 *   - SNOWTRI_DEVICE only: a SNOWTRI_HOST call stages and synchronises.
 * A graph holds POINTERS INTO THE CONTEXT'S SCRATCH: a later eager call on that context that grows the scratch (a larger shape)
 * or snowtri_ctx_destroy ends the graph's life -- destroy the graph first, never replay it afterwards.
 * ONE REPLAY PER CONTEXT may be in flight (replays on one stream are ordered; two graphs of one context on two streams share its
 * scratch unordered).  The status a captured call returns is that of the capture, not of a replay. */

/* Test hook (no reference counterpart): evaluates the fast reciprocal / reciprocal-square-root helpers
 * the throughput kernels use (v_rcp_f64 / v_rsq_f64 + Newton steps) on x[n]; host pointers. */
int snowtri_fastmath_probe(snowtri_ctx *ctx, int64_t n, const double *x, double *rcp_nr2_out,
                           double *rcp_nr1_out, double *rsq_nr1_out);

/* Test hook: the RAW v_rcp_f64 / v_rsq_f64 results (no Newton step) on x[n]; host pointers.  The float32-output
 * kernels use the raw 1/sqrt for 1/dist: tests pin its accuracy (<= 2^-23 relative over the normal range). */
int snowtri_fastmath_probe_raw(snowtri_ctx *ctx, int64_t n, const double *x, double *rcp_raw_out, double *rsq_raw_out);
/* Measurement aid: streams a KNOWN number of bytes with the access shapes of the fused kernels -- read_bytes from src
 * as 12-byte records per lane, write_bytes to dst as 16-byte records per lane (device pointers; either may be 0) --
 * so that HBM counters (rocprofv3 FETCH_SIZE / WRITE_SIZE) are calibrated on a kernel other than the one measured. */
int snowtri_calib_stream(snowtri_ctx *ctx, const void *src, int64_t read_bytes, void *dst, int64_t write_bytes,
                         void *stream);

/* A1  CameraGroup.add_human_2D_points (camera.py:234-253): uv[n][2] pixels of camera `cam`
 * -> rays[n][3] = R . inv(K) . [u, v, 1] (un-normalised, world frame).  Host pointers, fp64. */
int snowtri_rays_from_pixels(snowtri_ctx *ctx, int32_t cam, int64_t n, const double *uv, double *rays);

/* A2  Skew_Ray_Solver (triangulation.py:24-31), batched: hm, hs, tm, ts [n][3] -> dist[n], W[n][3].
 * Host pointers, fp64.  *n_singular (optional) counts exactly singular pairs (reference raises). */
int snowtri_skew_ray_batch(snowtri_ctx *ctx, int64_t n, const double *hm, const double *hs,
                           const double *tm, const double *ts, double *dist, double *W,
                           int64_t *n_singular);

/* A1+A3  Human_Triangulation (triangulation.py:50-93), candidates materialised.
 * Outputs are indexed by candidate SLOT (see Layouts), fp64:
 *   cand_xyz[F][Kc][J][3], cand_kscore[F][Kc][J], cand_pscore[F][Kc] (np.mean of kscore),
 *   cand_keep[F][Kc] uint8 = slot is a real pair AND NOT (pscore < average_score_threshold).
 * Kc = snowtri_num_candidate_slots(C, Pmax).  Returns SNOWTRI_ERR_SINGULAR (outputs still
 * written) if any valid pair was exactly singular. */
int snowtri_triangulate(snowtri_ctx *ctx, int64_t F, int32_t Pmax, int32_t J, const void *kpts,
                        int in_dtype, const int32_t *n_persons, const snowtri_params *params,
                        double *cand_xyz, double *cand_kscore, double *cand_pscore, uint8_t *cand_keep,
                        int memspace, void *stream);
int64_t snowtri_num_candidate_slots(int32_t C, int32_t Pmax);

/* A4  Human_Triangulation_Condense (triangulation.py:95-162) on materialised candidates.
 * cand_xyz[F][N][J][3], cand_kscore[F][N][J] fp64; cand_keep[F][N] (NULL = every slot is a
 * candidate) selects, in slot order, the candidate list the reference would hold.
 * Outputs fp64: out_xyz[F][Pout_max][kn][3], out_kscore[F][Pout_max][kn], out_pscore[F][Pout_max],
 * out_count[F] (true number of persons), out_flags[F] (optional). */
int snowtri_condense(snowtri_ctx *ctx, int64_t F, int32_t N, int32_t J, const double *cand_xyz,
                     const double *cand_kscore, const uint8_t *cand_keep, const snowtri_params *params,
                     int32_t Pout_max, double *out_xyz, double *out_kscore, double *out_pscore,
                     int32_t *out_count, uint32_t *out_flags, int memspace, void *stream);

/* The candidates of the last SNOWTRI_HOST snowtri_triangulate call on a context stay on the device.
 * snowtri_candidates_token names them (0 = none; any later snowtri_triangulate call on the context replaces them);
 * snowtri_condense_resident runs A4 on them -- the kept slots in slot order, i.e. exactly the list Human_Triangulation
 * returned -- without uploading them again: the reference calls Human_Triangulation and Human_Triangulation_Condense
 * back to back (main.py:62-71), and the second upload was a quarter of the per-frame latency.  Host outputs as
 * snowtri_condense (out_flags may be NULL); SNOWTRI_ERR_BAD_ARG if `token` is not the resident one (the caller then uses
 * snowtri_condense on its own arrays). */
int64_t snowtri_candidates_token(const snowtri_ctx *ctx);
int snowtri_condense_resident(snowtri_ctx *ctx, int64_t token, const snowtri_params *params, int32_t Pout_max, double *out_xyz,
                              double *out_kscore, double *out_pscore, int32_t *out_count, uint32_t *out_flags);

/* A1..A4 fused over a batch of frames -- the hot path.  Replaces the per-frame sequence
 * add_human_2D_points x (C*P) -> Human_Triangulation -> Human_Triangulation_Condense of
 * main.py:50-71,106.  No candidate list ever reaches HBM on the fast path.
 *   kpts [F][C][Pmax][J][3] of in_dtype;  out_xyzs [F][Pout_max][kn][4] of out_dtype
 *   (SNOWTRI_DEVICE: kpts aligned to its element size, out_xyzs to 16 bytes -- else SNOWTRI_ERR_BAD_ARG)
 *   out_pscore [F][Pout_max] of out_dtype (may be NULL), out_count[F] int32, out_flags[F] (may be NULL)
 * Entries of persons >= out_count[f] are zero-filled.  Returns OK / ERR_SINGULAR / ERR_OVERFLOW only
 * for SNOWTRI_HOST calls (device calls are asynchronous: inspect out_flags).
 * Accuracy: all arithmetic is fp64; SNOWTRI_F64 outputs are within 1e-8 m of the reference's.  Against the EXACT rule (this method in
 * 50-digit arithmetic on the stored fp64 rig and the stored pixels, oracle/skew_exact.py) and in rig units, as the SNOWTRI_DLT wording
 * below: with (c, s) the rig frame of that definition, a SNOWTRI_F64 joint is within 2.5e-10 s of the exact one (+ 1e-9 of what its
 * distance from c exceeds s by), a score within 1e-9 relative plus the conditioning of 1 / dist, wherever the rig stands and whatever
 * its unit -- tested on every route on rolled rigs with per-camera intrinsics, in metres and millimetres, at the origin, 47 m and
 * 1 km out (tests/test_gpu_skew_exact.py; measured: under 1 % of that bound, the reference's own fp64 arithmetic likewise), where no
 * decision of the exact rule is closer than 1e-9 relative to its threshold.  SNOWTRI_F32 outputs are the
 * fp64 results rounded to float32, i.e. exact to ONE UNIT IN THE LAST PLACE OF THE VALUE: 6e-8 relative -- below the 1e-4 m
 * of the project's parity bar only for coordinates under ~840 m.  Real joints are metres from the origin (error < 1e-6 m);
 * the ghost clusters near-parallel rays produce under a wide condense_distance_tol can lie hundreds of metres out, where
 * a float32 cannot hold 1e-4 m: ask for SNOWTRI_F64 outputs if such points matter.
 * out_pscore (triangulation.py:150, the mean of a person's keypoint scores): where it is taken from the STORED joint scores --
 * keypoint_num < J, SNOWTRI_F64 outputs, one detection per camera on five and more cameras (k_person_scores) -- a SNOWTRI_F32
 * value is the mean of the already rounded scores, up to 2 float32 ulp from the fp64 mean rounded once.
 * SNOWTRI_FLAG_SINGULAR: a pair is exactly singular when a c == b b in separately rounded products (a = hm.hm, b = hm.hs,
 * c = hs.hs: what the reference's LU of [[a, b], [b, c]] sees for equal rays, np.linalg.inv raises, triangulation.py:26). */
int snowtri_triangulate_condense(snowtri_ctx *ctx, int64_t F, int32_t Pmax, int32_t J,
                                 const void *kpts, int in_dtype, const int32_t *n_persons,
                                 const snowtri_params *params, int method, int32_t Pout_max,
                                 void *out_xyzs, void *out_pscore, int out_dtype, int32_t *out_count,
                                 uint32_t *out_flags, int memspace, void *stream);

/* The same call with flags (0 = exactly snowtri_triangulate_condense; an unknown bit is SNOWTRI_ERR_BAD_ARG).
 * SNOWTRI_CALL_NO_ZERO_FILL: the slots of persons >= out_count[f] -- out_xyzs[f][p >= count][.][.] and out_pscore[f][p >= count] --
 * are UNSPECIFIED after the call: the library does not spend HBM writes on them (whatever the caller's buffer held may still be
 * there, or what a kernel writes there anyway: zeros, or -- the lean kernels in a frame that resolves to nobody -- the joint records
 * they solved before the frame's count was known).  The reference returns LISTS of out_count[f] persons
 * (triangulation.py:154-160); the [F][Pout_max] padding is this ABI's artefact, and on a multi-person batch with a generous
 * Pout_max the zeros are most of what the call writes (BASELINE configs[2], 8 cameras x 4 persons resolving to ~5 persons per
 * frame, Pout_max 16: 234 MB of zeros beside 106 MB of results per 10 000 frames).  A caller that reads out_count[f] first --
 * snowmocap_amd/sharded.py's compact gather, BatchTriangulator(zero_fill=False) -- loses nothing.  SNOWTRI_HOST calls copy the
 * whole padded block back either way (their device staging is not cleared: the unused slots then hold earlier results). */
#define SNOWTRI_CALL_NO_ZERO_FILL 1u
int snowtri_triangulate_condense_ex(snowtri_ctx *ctx, int64_t F, int32_t Pmax, int32_t J,
                                    const void *kpts, int in_dtype, const int32_t *n_persons,
                                    const snowtri_params *params, int method, int32_t Pout_max,
                                    void *out_xyzs, void *out_pscore, int out_dtype, int32_t *out_count,
                                    uint32_t *out_flags, int memspace, void *stream, uint32_t call_flags);

/* Outlier-robust N-view triangulation (no reference counterpart; SURVEY.md 8f N3 "robust variants"): SNOWTRI_DLT for one detection per
 * camera, except that a view whose reprojection residual shows it to be wrong about a joint is left out of that joint.  Per frame f
 * and joint j < keypoint_num, on inputs converted to fp64, with (c, s) the rig frame of SNOWTRI_DLT, P[c] = K_c [R_c^T | -R_c^T (t_c - c) / s]
 * the matrices from that frame to pixels (the residuals below do not depend on the frame) and tau = reproj_threshold_px:
 *   1. S = { c : (n_persons == NULL or n_persons[f][c] > 0) and not (s_c < keypoint_score_threshold) }.  |S| < 2: the record is
 *      (0, 0, 0, 0), views = 0, resid = 0.
 *   2. solve(S): x = the DLT solution over the views in S exactly as SNOWTRI_DLT defines it (rows u P[c][2] - P[c][0],
 *      v P[c][2] - P[c][1]; smallest right singular vector, dehomogenised; X = c + s x in the world); for c in S, p = P[c] (x, 1) and
 *      r_c^2 = (p0 / p2 - u_c)^2 + (p1 / p2 - v_c)^2;  m(S) = max_c r_c^2 (NaN if any r_c^2 is).
 *   3. d = 0.  While |S| >= 3 and d < max_drops and m(S) > tau^2:  for every c in S in increasing c, m_c = m(S \ {c});  drop
 *      c* = argmin m_c -- the lowest c starts as the best, a later candidate replaces it only if its m_c is strictly smaller (ties go
 *      to the lowest c) or if the best so far is NaN and m_c is not (a NaN never wins against a number);  S = S \ {c*}, d += 1.
 *      The comparisons are exactly these, so a NaN m(S) ends the loop.
 *   4. The joint is X(S); its score the mean of s_c over the final S; views = bit mask of S (bit c); resid = sqrt(mean_{c in S} r_c^2)
 *      in pixels.  Person score = mean of the keypoint_num joint scores; count = 1; flags as SNOWTRI_DLT writes them (FASTPATH).
 * With max_drops = 0 or tau = +infinity this is SNOWTRI_DLT.  Leave-one-out instead of "drop the largest residual": the algebraic
 * solve spreads one view's error over all views, and on 3-4 cameras the largest residual sits on a wrong view about one time in four.
 * snowmocap_amd/robust.py::triangulate_robust_reference is this rule in NumPy (SVD); the kernel (k_dlt_robust,
 * snowmocap_amd/csrc/snowtri_robust.hpp) takes the same decisions wherever they are not within rounding of a tie.
 *   kpts [F][C][1][J][3] of in_dtype, n_persons [F][C] or NULL, out_xyzs [F][Pout_max][kn][4], out_pscore [F][Pout_max] (may be NULL),
 *   out_count [F], out_flags [F] (may be NULL): as snowtri_triangulate_condense, same validation and alignment rules; slots >= 1 are
 *   zero-filled;
 *   out_views [F][kn] uint32 (may be NULL), out_resid [F][kn] of out_dtype (may be NULL): the two diagnostics; a NULL one costs nothing.
 * reproj_threshold_px and max_drops as snowtri_ctx_set_robust takes them (the context's settings are not read).  F == 0 is SNOWTRI_OK
 * and touches nothing.  SNOWTRI_DEVICE: asynchronous on `stream`, no host read, no internal stream (the overlap mode does not apply).
 * snowtri_last_kernel_names reports k_dlt_robust<...> after the call. */
int snowtri_triangulate_robust(snowtri_ctx *ctx, int64_t F, int32_t J, const void *kpts, int in_dtype, const int32_t *n_persons,
                               const snowtri_params *params, double reproj_threshold_px, int32_t max_drops, int32_t Pout_max,
                               void *out_xyzs, void *out_pscore, int out_dtype, int32_t *out_count, uint32_t *out_flags,
                               uint32_t *out_views, void *out_resid, int memspace, void *stream);

/* N1  Human_Triangulation_Smooth / SecondOrderDynamic (triangulation.py:4-22,164-186) over a whole track.
 * x[T][n] fp64, frame-major, n = persons * joints * 3 lanes (persons matched by index, as the reference does)
 * -> y[T][n].  Frame 0 passes through and seeds xp = y = x0, yd = 0; f, z, r, dt as in the reference
 * (main.py:72-77).  Evaluated as ONE pass over HBM -- a chained scan over 256-frame blocks with decoupled look-back: x is read
 * once, y written once.  T <= 1 + 256 * 65535 frames, n <= 2^22 lanes.
 * ACCURACY AND REPEATABILITY OF THE SCAN (this entry and every other one that runs k_smooth_scan: snowtri_smooth_joint_track,
 * snowtri_smooth_shard_reduce / _scan, snowtri_blender_smooth, snowtri_blender_smooth_shard_reduce / _scan).  The scan is a
 * re-association of the recurrence's sum: the state crosses a 32-frame wave through R = A^32 and a 256-frame block through
 * P = A^256 (A: the one-frame update, snowtri_smooth_coeffs).  For every STABLE filter (spectral radius of A at most 1: slow,
 * overdamped and undamped ones, high frame rates) the result equals the recurrence evaluated in exact arithmetic on the same
 * fp64 inputs and coefficients within 16 x the rounding error the sequential fp64 recurrence itself makes on that track;
 * measured: at most 2.3 x that error, 2.6e-14 m on tracks of metres and up to 2100 frames, from f = 0.05 Hz at 30 fps (max|P| = 1.1)
 * and an undamped filter (max|P| = 3.1) to the reference's profiles at 240 fps (tests/test_gpu_smooth_carry.py).  The "~1e-13 m"
 * this header used to quote was measured at the reference's 30 fps profiles only (f = 1.5 ... 4.5 Hz), where max|P| < 1e-20.
 * A block's look-back adds up either the aggregates of the blocks before it or an inclusive state one of them has already
 * published -- whichever it finds -- and the two orders agree in exact arithmetic only.  So two calls on the same input are
 * BIT-FOR-BIT equal where P underflows against the state (max|P| below ~1e-17: the reference's 30 fps profiles, tested over
 * 782 chained blocks), and otherwise equal to the bound above: each within it, any two within twice it (measured spread:
 * 2.7e-15 m at max|P| = 3.1).  A caller that needs bitwise repeatability at a slow filter has the five-pass shard form
 * (_shard_local / _combine / _fix, also on one shard), whose order is fixed.  An unstable filter overflows, here as in the reference. */
int snowtri_smooth_track(snowtri_ctx *ctx, int64_t T, int64_t n, const double *x, double f, double z, double r,
                         double dt, double *y, int memspace, void *stream);
/* The same on a track of JOINT RECORDS as snowtri_triangulate_condense writes them with SNOWTRI_F64 outputs: xyzs[T][m][4] =
 * (x, y, z, score), m = persons * keypoint_num -> out[T][m][4] with the three coordinates filtered and the score COPIED (the
 * reference filters the points only, triangulation.py:169-184: a caller of snowtri_smooth_track had to filter the score lane
 * for nothing and copy the scores over afterwards).  out may not alias xyzs.  Accuracy and repeatability: as stated at
 * snowtri_smooth_track (the same scan). */
int snowtri_smooth_joint_track(snowtri_ctx *ctx, int64_t T, int64_t m, const double *xyzs, double f, double z, double r,
                               double dt, double *out, int memspace, void *stream);

/* N1 on a FRAME-SHARDED track (one contiguous frame block per rank).  The filter is linear in its state, so a
 * shard is processed in two calls around ONE small exchange of carries (3n doubles per rank):
 *   snowtri_smooth_shard_local  y = response of the shard from a ZERO entering state (first != 0: this shard
 *                               starts the track, its frame 0 passes through; otherwise every frame is
 *                               filtered and the first one takes xd = 0), end_state[2n] = that response's
 *                               final (y, yd) per lane;
 *   snowtri_smooth_shard_fix    y += response of the true entering state start_state[2n].
 * Between the two, snowtri_smooth_shard_combine turns what the ranks all-gathered -- gathered[world][4n + 1] doubles,
 * per shard in frame order: end_state[2n] | first input row [n] | last input row [n] | its length T_q -- into the
 * start_state[2n] of shard `rank`, on the device and on `stream` (no host round trip between the all-gather and the
 * fix; empty shards have T_q = 0).  CONTRACT on `first`: combine takes the first NON-EMPTY shard of `gathered` as the
 * start of the track (seed (x_first, 0), its frame 0 passes through), so `first != 0` must be given to _local and _fix
 * on exactly that shard -- which is rank 0 only when no leading shard is empty (true for contiguous blocks of
 * ceil(F / world) frames, where only trailing blocks can be empty; a caller with another layout passes first on the
 * rank that holds frame 0).  snowmocap_amd/sharded.py::combine_carries is the same arithmetic on the host
 * (the gloo tests); snowtri_smooth_coeffs returns {a00,a01,a10,a11,cx,cxd} of the update
 * s_t = A s_{t-1} + (0, cx x_t + cxd (x_t - x_{t-1})) it needs. */
int snowtri_smooth_coeffs(double f, double z, double r, double dt, double out[6]);
int snowtri_smooth_shard_local(snowtri_ctx *ctx, int64_t T, int64_t n, const double *x, int first, double f,
                               double z, double r, double dt, double *y, double *end_state, int memspace,
                               void *stream);
int snowtri_smooth_shard_fix(snowtri_ctx *ctx, int64_t T, int64_t n, int first, const double *start_state, double f,
                             double z, double r, double dt, double *y, int memspace, void *stream);
int snowtri_smooth_shard_combine(snowtri_ctx *ctx, int32_t world, int32_t rank, int64_t n, const double *gathered, double f,
                                 double z, double r, double dt, double *start_state, int memspace, void *stream);
/* The same exchange in TWO passes over the shard instead of five (round 6; DEVICE pointers, asynchronous on `stream`):
 *   snowtri_smooth_shard_reduce  end_state[2n] of the shard's zero-state response -- what _local returns -- from ONE read of x,
 *                                without writing a track;
 *   (the all-gather and snowtri_smooth_shard_combine as above)
 *   snowtri_smooth_shard_scan    y = the shard filtered from its true entering state start_state[2n]: x read once, y written once.
 * 24 bytes moved per lane-frame against the 40 of _local + _fix; same `first` contract.  Both run the scan of snowtri_smooth_track:
 * its accuracy and repeatability statement holds for the entering states snowtri_smooth_shard_combine returns (y and yd, each
 * against 16 x the sequential recurrence's own error on that component; A^m with m up to 700 at max|P| = 3.1 tested) and for the
 * assembled track -- bit-for-bit repeatable where P = A^256 underflows against the state, to that bound otherwise.
 * snowmocap_amd/sharded.py::smooth_exchange2 drives it. */
int snowtri_smooth_shard_reduce(snowtri_ctx *ctx, int64_t T, int64_t n, const double *x, int first, double f, double z, double r,
                                double dt, double *end_state, void *stream);
int snowtri_smooth_shard_scan(snowtri_ctx *ctx, int64_t T, int64_t n, const double *x, int first, const double *start_state, double f,
                              double z, double r, double dt, double *y, void *stream);

/* N2  Blender IK control points (blender.py:98-143; names and order of configs/blender_armature_profile.json:
 * root_position, root_rotation, clavicle_r_ik, clavicle_l_ik, arm_r_ik, arm_r_pole, arm_l_ik, arm_l_pole,
 * leg_r_ik, leg_r_pole, leg_l_ik, leg_l_pole, hand_r_ik, hand_r_pole, hand_l_ik, hand_l_pole, foot_r_ik,
 * foot_r_pole, foot_l_ik, foot_l_pole, chest_ik, chest_pole, head_ik, head_pole).
 *   xyzs [n][keypoint_num][4] of xyz_dtype -- n skeletons as written by snowtri_triangulate_condense
 *        (x, y, z, score; the score is not read); keypoint_num >= 130 (COCO-WholeBody joints up to 129 are used),
 *        otherwise SNOWTRI_ERR_BAD_INDEX (the reference raises IndexError);
 *   out_points [n][24][4] fp64: 3-vectors padded with 0, root_rotation as the quaternion (w, x, y, z)
 *        (blender.py:28-29);  out_valid [n][24]: 0 where the point has a NaN component (blender.py:135-139).
 * A NaN root_rotation (coincident hips, or spine parallel to the pelvis axis) makes the reference raise inside
 * SciPy's SVD; here it is reported as out_valid = 0 and the Python mirror raises. */
#define SNOWTRI_BLENDER_POINTS 24
int snowtri_blender_points(snowtri_ctx *ctx, int64_t n, int32_t keypoint_num, const void *xyzs, int xyz_dtype,
                           double *out_points, uint8_t *out_valid, int memspace, void *stream);

/* N2  Human_Triangulation_Blender_Smooth (blender.py:145-178) over a whole track of control points:
 *   points [T][n_persons][24][4] fp64, valid [T][n_persons][24], fzr [24][3] = per-point (f, z, r) of
 *   configs/blender_smooth_profile.json, dt = delta_time  ->  out [T][n_persons][24][4].
 * Frame 0 is returned as given (NaNs included) and seeds every filter with the point, or with zeros when it is
 * invalid; a later invalid point feeds the filter its previous input.  Evaluated as chunked scans over frames: the hold first,
 * then the scan of snowtri_smooth_track with per-point coefficients -- its accuracy and repeatability statement holds per
 * control point (bit-for-bit repeatable for the points whose P = A^256 underflows, to the rounding bound for slower ones). */
int snowtri_blender_smooth(snowtri_ctx *ctx, int64_t T, int64_t n_persons, const double *points,
                           const uint8_t *valid, const double *fzr, double dt, double *out, int memspace,
                           void *stream);

/* N2 on a FRAME-SHARDED track (one contiguous frame block per rank; DEVICE pointers, asynchronous on `stream`).  An invalid
 * point feeds a filter its previous input (blender.py:157-160), i.e. the filters run on the HELD sequence
 * x_eff[t] = valid[t] ? x[t] : x_eff[t-1] (x_eff[-1] = 0: a filter whose first point is invalid is seeded with zeros,
 * :172-173) -- and on x_eff they are plain linear filters, so a shard takes TWO small exchanges:
 *   1. snowtri_blender_hold_shard_last   payload[2n] = last valid input of the shard per lane | found (1.0 / 0.0) per lane,
 *                                        n = n_persons * 24 * 4 (an empty shard: all zeros);  all-gather the payloads;
 *      snowtri_blender_hold_shard_apply  held[T][n] = x_eff of the shard, entering with the last valid input of the nearest
 *                                        shard before `rank` that has one (gathered[world][2n], frame order);
 *   2. the carry exchange of row N1 on `held` with the per-point coefficients fzr[24][3]:
 *      snowtri_blender_smooth_shard_local / _combine / _fix = snowtri_smooth_shard_local / _combine / _fix (same payload
 *      gathered[world][4n + 1]: end state | first row of held | last row of held | T; same contract on `first`).
 * The shard that starts the track returns its frame 0 as the filter saw it (x_eff[0]); the reference returns the RAW points
 * of frame 0 (NaNs included, blender.py:176): the caller copies that row over (snowmocap_amd/sharded.py does).
 * snowmocap_amd/sharded.py::blender_smooth_sharded drives the protocol; tests compare it with snowtri_blender_smooth. */
int snowtri_blender_hold_shard_last(snowtri_ctx *ctx, int64_t T, int64_t n_persons, const double *points, const uint8_t *valid,
                                    double *payload, void *stream);
int snowtri_blender_hold_shard_apply(snowtri_ctx *ctx, int32_t world, int32_t rank, int64_t T, int64_t n_persons, const double *points,
                                     const uint8_t *valid, const double *gathered, double *held, void *stream);
int snowtri_blender_smooth_shard_local(snowtri_ctx *ctx, int64_t T, int64_t n_persons, const double *held, int first, const double *fzr,
                                       double dt, double *y, double *end_state, void *stream);
int snowtri_blender_smooth_shard_combine(snowtri_ctx *ctx, int32_t world, int32_t rank, int64_t n_persons, const double *gathered,
                                         const double *fzr, double dt, double *start_state, void *stream);
int snowtri_blender_smooth_shard_fix(snowtri_ctx *ctx, int64_t T, int64_t n_persons, int first, const double *start_state, const double *fzr,
                                     double dt, double *y, void *stream);
/* ... and its two-pass form on `held` (snowtri_smooth_shard_reduce / _scan with the per-point coefficients; the same accuracy
 * and repeatability statement, per control point). */
int snowtri_blender_smooth_shard_reduce(snowtri_ctx *ctx, int64_t T, int64_t n_persons, const double *held, int first, const double *fzr,
                                        double dt, double *end_state, void *stream);
int snowtri_blender_smooth_shard_scan(snowtri_ctx *ctx, int64_t T, int64_t n_persons, const double *held, int first, const double *start_state,
                                      const double *fzr, double dt, double *y, void *stream);

/* Person tracking: stable identities across frames (no reference counterpart: SnowMocap identifies persons by list index,
 * triangulation.py:169-171, and the condense step lists a frame's persons in the order its clusters formed).
 * snowtri_track_persons assigns every person of every frame to one of S SLOTS by greedy nearest-centre matching and gives
 * every new appearance a fresh TRACK ID.  State per slot s < S: live, pos[3] (fp64), missed, id; one next_id counter; a fresh
 * state has no live slot and next_id = 0.  For each frame f, in order:
 *   1. VALID PERSONS  p < count[f] whose centre joint xyzs[f][p][center_point_index] has score != 0 and three finite
 *      coordinates (a fused joint with score 0 is the all-zero record the condense step leaves: not a position).  Invalid
 *      persons get slot_of = -1.
 *   2. DISTANCES  for every slot live at the START of the frame and every valid person, d = centre - pos[s] on inputs
 *      converted to fp64, d2 = (dx*dx + dy*dy) + dz*dz with every product and sum rounded separately (no FMA contraction:
 *      the same rule as for the singular test above).
 *   3. GREEDY MATCHING  repeatedly the smallest d2 <= gate*gate among unassigned (slot, person) pairs, ties to the lowest s,
 *      then the lowest p: the pair is assigned, pos[s] = centre, missed[s] = 0; until no pair qualifies.
 *   4. BIRTHS  each valid person still unassigned, in increasing p, takes the lowest slot that was not live at the start of
 *      the frame and has not been taken in this step, under id = next_id++.  No such slot: slot_of = -1 and the frame gets
 *      SNOWTRI_TRACK_FLAG_OVERFLOW.
 *   5. AGEING  every slot that was live at the start and got no person: missed += 1, freed when missed > max_missed.  A slot
 *      freed in frame f can be re-used from frame f + 1 on.
 * snowmocap_amd/tracking.py::track_persons_reference is this rule in NumPy; every integer output agrees with it bit for bit.
 *   xyzs [F][Pout_max][keypoint_num][4] of xyz_dtype and count [F]: exactly what snowtri_triangulate_condense writes
 *   slot_of   [F][Pout_max] int32   slot of person p, -1 = untracked (invalid, or no slot left)
 *   person_of [F][S] int32          person in slot s in this frame, -1 = slot empty in this frame
 *   track_id  [F][S] int32          id of that person's track, -1 where person_of is -1
 *   flags     [F] uint32            SNOWTRI_TRACK_FLAG_* (may be NULL)
 *   state     opaque, snowtri_track_state_bytes(S) bytes in the same memspace (8-byte aligned), in/out: all-zero for a fresh
 *             start; calls over consecutive frame blocks with the same state give the outputs of one call over the whole
 *             range (a recording processed in batches keeps its identities).  NULL = fresh start, not saved.
 * S and Pout_max outside 1..16, a negative or non-finite gate, max_missed < 0: SNOWTRI_ERR_BAD_ARG; center_point_index outside
 * [0, keypoint_num): SNOWTRI_ERR_BAD_INDEX; snowtri_last_error() says which.  F == 0 is SNOWTRI_OK and touches nothing (state
 * included).  SNOWTRI_DEVICE: asynchronous on `stream`, no host read, no internal stream; xyzs aligned to 16 bytes.
 * SNOWTRI_HOST: staged and synchronous.  snowtri_track_state_bytes is 0 for S outside 1..16.
 * Kernels (snowmocap_amd/csrc/snowtri_track.hpp): k_track_centres, parallel over (f, p), extracts the centres; k_track_chain
 * walks the frames on one wave whose lanes hold the <= 256 (slot, person) pairs four each, while the other waves of its
 * workgroup stage blocks of snowtri_track_block_frames() frames through LDS and write the results out. */
#define SNOWTRI_TRACK_FLAG_OVERFLOW 1u /* a valid person of this frame found no free slot */
size_t snowtri_track_state_bytes(int32_t S);
int snowtri_track_block_frames(void);
int snowtri_track_persons(snowtri_ctx *ctx, int64_t F, int32_t Pout_max, int32_t keypoint_num, const void *xyzs, int xyz_dtype,
                          const int32_t *count, int32_t S, int32_t center_point_index, double gate, int32_t max_missed, void *state,
                          int32_t *slot_of, int32_t *person_of, int32_t *track_id, uint32_t *flags, int memspace, void *stream);
/* Measurement aid: with snowtri_set_timing(ctx, 1) a snowtri_track_persons call brackets its two kernels with HIP events;
 * kernel_ms[0] = k_track_centres, kernel_ms[1] = k_track_chain of the last such call (blocks until they have finished;
 * SNOWTRI_ERR_BAD_ARG if that call was not timed). */
int snowtri_track_last_ms(snowtri_ctx *ctx, float kernel_ms[2]);
/* The tracks as arrays: xyzs_tracked [F][S][keypoint_num][4] of xyz_dtype = xyzs[f][person_of[f][s]] where person_of[f][s] >= 0,
 * zeros elsewhere.  Records are copied bit for bit (NaN payloads survive).  xyzs and xyzs_tracked aligned to 16 bytes
 * (SNOWTRI_DEVICE) and distinct. */
int snowtri_track_gather(snowtri_ctx *ctx, int64_t F, int32_t Pout_max, int32_t keypoint_num, const void *xyzs, int xyz_dtype,
                         int32_t S, const int32_t *person_of, void *xyzs_tracked, int memspace, void *stream);

/* Gap filling: short dropouts in a track of joint records bridged before smoothing (no reference counterpart: the condense step
 * leaves a joint too few views saw as the record (0, 0, 0, 0), triangulation.py:136-148, and the reference's filter takes it for a
 * position at the origin).  xyzs[T][m][4] of xyz_dtype, m = persons * keypoint_num lanes of records (x, y, z, score), as
 * snowtri_triangulate_condense and snowtri_track_gather write them -> out[T][m][4] of the same type, fill[T][m] uint8 codes (may be
 * NULL: it then costs nothing).  All decisions and arithmetic are made on the values converted to fp64:
 *   1. MISSING  record (t, l) is missing if its score == 0 (so -0.0 counts) or any of its four values is not finite; otherwise it
 *      is MEASURED (rec_is_missing, snowmocap_amd/csrc/snowtri_record.hpp).
 *   2. INTERIOR GAP  a measured record at frame a and the next measured record of the same lane at frame b, g = b - a - 1 with
 *      1 <= g <= max_gap: for k = 1..g record a + k becomes the linear interpolation of the two in all four components (the score
 *      included): w = (double)k / (double)(g + 1), d = B - A, p = w * d, v = A + p with every operation rounded separately (no FMA
 *      contraction: the same rule as for the tracker's distances and the singular test above), v rounded once to xyz_dtype.
 *      Code SNOWTRI_FILL_LERP.
 *   3. ENDS OF THE ARRAY  b = the first measured frame of a lane: if 1 <= b <= max_gap, frames 0..b-1 become copies of record b;
 *      a = the last measured frame: if 1 <= T - 1 - a <= max_gap, frames a+1..T-1 become copies of record a.  Code
 *      SNOWTRI_FILL_HOLD.  Nothing else is held.
 *   4. EVERYTHING ELSE is copied bit for bit: a measured record with code SNOWTRI_FILL_MEASURED, a missing record that no rule
 *      filled with code SNOWTRI_FILL_MISSING (its NaN payloads survive the copy).
 *   5. Lanes are independent: the result of a lane depends on nothing but that lane.
 * snowmocap_amd/fill.py::fill_joint_track_reference is this rule in NumPy; the kernel (k_fill_gaps, snowmocap_amd/csrc/snowtri_fill.hpp)
 * agrees with it bit for bit.  What the rule does NOT do: a joint that is missing in the first frame of a track and stays missing for
 * more than max_gap frames is left alone, so a filter that starts there is still seeded with zeros.
 * max_gap outside 1..255, an unknown dtype or memspace, negative T or m, a NULL xyzs or out: SNOWTRI_ERR_BAD_ARG.  out must not
 * overlap xyzs (a tile of the kernel reads records of its neighbours that those have already overwritten): SNOWTRI_ERR_BAD_ARG.
 * Sizes: T * m <= 2^58 records (64-bit byte offsets) and ceil(T / (4 * snowtri_fill_block_frames())) * ceil(m / 64) <= 2^31 - 1
 * workgroups (a one-dimensional grid); beyond either SNOWTRI_ERR_BAD_ARG and snowtri_last_error() names the limit.  T == 0 (or
 * m == 0) is SNOWTRI_OK and touches nothing.  A scratch-only context (C == 0) is enough.
 * SNOWTRI_DEVICE: asynchronous on `stream`, no host read, no internal stream; xyzs and out aligned to 16 bytes (else
 * SNOWTRI_ERR_BAD_ARG).  SNOWTRI_HOST: staged and synchronous.
 * snowtri_fill_block_frames(): frames per tile of the kernel (results do not depend on it; tests aim gaps at its multiples). */
#define SNOWTRI_FILL_MEASURED 0 /* measured record, copied                                  */
#define SNOWTRI_FILL_LERP 1     /* interpolated between two measured records                */
#define SNOWTRI_FILL_HOLD 2     /* copy of the nearest measured record, at an end of the array */
#define SNOWTRI_FILL_MISSING 3  /* missing record that no rule filled, copied               */
int snowtri_fill_joint_track(snowtri_ctx *ctx, int64_t T, int64_t m, const void *xyzs, int xyz_dtype, int32_t max_gap,
                             void *out, uint8_t *fill /* [T][m], may be NULL */, int memspace, void *stream);
int snowtri_fill_block_frames(void);

/* Despiking: one- and two-frame jumps taken out of a track of joint records before gap filling (no reference counterpart).  A joint
 * that was SEEN in the wrong place for a frame or two -- a flipped limb, a hand found on the neighbour -- is a measured record: the
 * gap filler leaves it alone and the second-order filter rings on it for many frames.  The test is temporal, so it does not care
 * which triangulation route produced the record.  xyzs[T][m][4] of xyz_dtype, the records snowtri_fill_joint_track takes ->
 * out[T][m][4] of the same type, codes[T][m] uint8 (may be NULL: it then costs nothing).  All decisions are made on the values
 * converted to fp64:
 *   1. MISSING / MEASURED  exactly as for gap filling: record (t, l) is missing if its score == 0 (so -0.0 counts) or any of its four
 *      values is not finite; otherwise it is measured (rec_is_missing, snowmocap_amd/csrc/snowtri_record.hpp).
 *   2. WINDOW  for record (t, l) the window W holds the measured records of lane l at frames max(0, t - h) .. min(T - 1, t + h), the
 *      record itself included; h = half_window (1..4), n = |W|.
 *   3. MEDIAN  for each of x, y, z: the n values sorted ascending, med = (v[(n - 1) / 2] + v[n / 2]) * 0.5 (integer division; one
 *      addition and one multiplication, each rounded once).
 *   4. DEVIATION  d = value - med per coordinate, d2 = (dx * dx + dy * dy) + dz * dz, every operation rounded separately (no FMA
 *      contraction: the same rule as for the tracker's distances).
 *   5. SPIKE TEST  a measured record is a SPIKE iff n >= 3 and d2 > tol * tol, the product formed once in fp64.  The comparison is
 *      exactly that: d2 == tol * tol is not a spike, and neither is a NaN d2 (from a sum that overflowed).
 *   6. ALL SPIKES ARE DECIDED ON THE INPUT: removing one spike never changes the verdict on another; there is no iteration.
 *   7. OUTPUT  mode SNOWTRI_DESPIKE_MARK: a spike is written as four +0.0 -- the condense step's zero record, which
 *      snowtri_fill_joint_track bridges.  mode SNOWTRI_DESPIKE_REPLACE: a spike is written as (med_x + 0.0, med_y + 0.0, med_z + 0.0),
 *      each rounded once to xyz_dtype, with the record's own score bits (the + 0.0 makes a zero median +0.0 whichever zero the sort
 *      left in the middle).  Every other record is copied bit for bit (NaN payloads of missing records survive).
 *   8. CODES  SNOWTRI_DESPIKE_KEPT: measured, tested, copied.  SNOWTRI_DESPIKE_SPIKE.  SNOWTRI_DESPIKE_MISSING: missing, copied.
 *      SNOWTRI_DESPIKE_UNSUPPORTED: measured with n < 3, copied untested.
 *   9. Lanes are independent: the result of a lane depends on nothing but that lane.
 * snowmocap_amd/despike.py::despike_joint_track_reference is this rule in NumPy; the kernel (k_despike,
 * snowmocap_amd/csrc/snowtri_despike.hpp) agrees with it bit for bit.  What the rule does NOT do: a run of more than h wrong records
 * in a window outvotes the right ones, and on a fast path (more than about tol / h per frame) the median of a window with holes
 * sits off-centre, so clean records next to dropouts are flagged.
 * half_window outside 1..4, tol negative or NaN (+infinity is allowed: nothing is a spike), an unknown mode, dtype or memspace,
 * negative T or m, a NULL xyzs or out: SNOWTRI_ERR_BAD_ARG, and snowtri_last_error() names the argument.  out must not overlap
 * xyzs (a tile of the kernel reads records of its neighbours): SNOWTRI_ERR_BAD_ARG.  Sizes: T * m <= 2^58 records and
 * ceil(T / (4 * snowtri_despike_block_frames())) * ceil(m / 64) <= 2^31 - 1 workgroups; beyond either SNOWTRI_ERR_BAD_ARG and
 * snowtri_last_error() names the limit.  T == 0 (or m == 0) is SNOWTRI_OK and touches nothing.  A scratch-only context (C == 0)
 * is enough.  SNOWTRI_DEVICE: asynchronous on `stream`, no host read, no internal stream; xyzs and out aligned to 16 bytes (else
 * SNOWTRI_ERR_BAD_ARG).  SNOWTRI_HOST: staged and synchronous.
 * snowtri_despike_block_frames(): frames per tile of the kernel (results do not depend on it; tests aim spikes at its multiples). */
#define SNOWTRI_DESPIKE_MARK 0    /* mode: a spike becomes the zero record                     */
#define SNOWTRI_DESPIKE_REPLACE 1 /* mode: a spike becomes the window median, its score kept    */
#define SNOWTRI_DESPIKE_KEPT 0        /* measured, tested, copied                               */
#define SNOWTRI_DESPIKE_SPIKE 1       /* measured, further than tol from the window median      */
#define SNOWTRI_DESPIKE_MISSING 2     /* missing, copied                                        */
#define SNOWTRI_DESPIKE_UNSUPPORTED 3 /* measured with fewer than 3 measured records in its window, copied untested */
int snowtri_despike_joint_track(snowtri_ctx *ctx, int64_t T, int64_t m, const void *xyzs, int xyz_dtype, int32_t half_window,
                                double tol, int32_t mode, void *out, uint8_t *codes /* [T][m], may be NULL */, int memspace,
                                void *stream);
int snowtri_despike_block_frames(void);

/* N4  Keypoint-level lens undistortion, for detections made on RAW frames (the reference undistorts whole
 * images before detection: main.py:52 cv2.undistort(frame, K, D)).  OpenCV's 5-coefficient Brown-Conrady model,
 * D[C][5] = (k1, k2, p1, p2, k3) per camera (camera_group_floor.json:53-61; Camera.D, camera.py:24,44); K as
 * given to snowtri_ctx_create, which must be [[fx, s, cx], [0, fy, cy], [0, 0, 1]].
 * snowtri_undistort_keypoints maps every (u, v) of kpts [F][C][Pmax][J][3] from the raw image to the
 * undistorted image (exact inverse of the forward model, Newton, 5e-13 px on the shipped rig) and copies the
 * score; kpts_out may alias kpts_in; the result feeds snowtri_triangulate_condense unchanged. */
int snowtri_ctx_set_distortion(snowtri_ctx *ctx, const double *D);
int snowtri_undistort_keypoints(snowtri_ctx *ctx, int64_t F, int32_t Pmax, int32_t J, const void *kpts_in,
                                void *kpts_out, int dtype, int memspace, void *stream);

/* Reprojection: 3D joint records back into the cameras' images, and what each camera's detections cost against them (no reference
 * counterpart; the direction opposite to triangulation and to snowtri_undistort_keypoints).  How well does camera c agree with a
 * result, which of its detections belongs to 3D person p, where is the skeleton drawn on the frame.  The rule, in fp64, per camera c,
 * frame f, person p and joint j < kn, with K, R, t as given to snowtri_ctx_create and the record (X, score) = xyzs[f][p][j] of
 * xyz_dtype converted to fp64:
 *   1. d = X - t_c, pc = R_c^T d, x = pc0 / pc2, y = pc1 / pc2.
 *   2. With SNOWTRI_REPROJECT_RAW in `flags`: (x, y) goes through the forward lens model (x_d, y_d of the header of
 *      snowmocap_amd/csrc/snowtri_undistort.hpp) with the D of snowtri_ctx_set_distortion -- the pixel on the RAW frame, the exact
 *      opposite of snowtri_undistort_keypoints.
 *   3. u = fx x + s y + cx, v = fy y + cy.
 *   4. The projection is VALID iff the record is measured (rule 1 of gap filling: score != 0 and four finite values), pc2 > 0 (the
 *      point lies in front of the camera) and u, v are finite.
 * snowmocap_amd/reproject.py::reproject_reference / reprojection_cost_reference are this rule in NumPy, plain operations in this
 * order; the kernels (snowmocap_amd/csrc/snowtri_reproject.hpp: fused multiply-adds, one 1 / pc2 for x and y) stay within 1e-11 px of
 * the exact value of the rule (2e-11 px with RAW) on rigs with fx <= 760 and points within |d| / pc2 <= 1.8 (tests/test_gpu_reproject.py).
 *
 * snowtri_reproject: xyzs [F][P][kn][4] -> pix [F][C][P][kn][3] of pix_dtype, the layout of kpts: the output feeds
 * snowtri_triangulate_condense unchanged.  A valid projection writes (u, v, score), each rounded once to pix_dtype; an invalid one
 * writes (0, 0, 0), which every score gate downstream drops.  A pixel's bits depend on its own record and camera only, never on the
 * batch around it (k_reproject: one lane per observation, no loop).
 *
 * snowtri_reproject_cost: the same projections compared with the detections kpts [F][C][Pmax][kn][3] of kpts_dtype (n_persons
 * [F][C] int32 or NULL = Pmax everywhere) without being written anywhere: cost_sum [F][C][P][Pmax] float64, cost_n the same shape
 * int32.  Joint j of detection q COUNTS iff q < n_persons[f][c], not (score < keypoint_score_threshold), and its u, v are finite.
 * cost_n[f][c][p][q] = the joints j whose projection of (p, j) is valid and whose detection (q, j) counts; cost_sum = the sum over
 * those joints of (u - u_det)^2 + (v - v_det)^2 in fp64, px^2, and 0 when cost_n is 0.  With SNOWTRI_REPROJECT_RAW the comparison
 * is made on the raw frame against raw detections: no undistorted copy of the keypoints is needed.  The sum of an item is formed in
 * an order that depends on kn alone (k_reproject_cost: one wave per (f, c, p), lane l adds joints l, l + 64, ... in turn, then a
 * fixed butterfly over the wave): not on F, the item's place in the launch or how a batch is cut into calls; it is NOT joint order,
 * so it agrees with the NumPy rule to rounding (128 eps of the sum), not bit for bit.  Both kernels share one projection function:
 * the cost of a person against its own float64 snowtri_reproject output is exactly 0.
 *
 * Refusals (SNOWTRI_ERR_BAD_ARG, snowtri_last_error() names the argument; nothing is enqueued or written): a NULL or camera-less
 * context, an unknown dtype, memspace or flag bit, F < 0, P, kn or Pmax < 1, a K that is not [[fx, s, cx], [0, fy, cy], [0, 0, 1]]
 * with fx, fy != 0 (the condition of snowtri_ctx_set_distortion), SNOWTRI_REPROJECT_RAW before snowtri_ctx_set_distortion, a NaN
 * threshold, a NULL array other than n_persons, a device pointer that is not aligned to its element size.  Sizes: snowtri_reproject
 * F * C * P * kn <= (2^31 - 1) * 256 observations; snowtri_reproject_cost kn <= 256 (a lane holds four joints), F * C * P <=
 * (2^31 - 1) * 4 and F * C * P * Pmax <= 2^48.  F == 0 is SNOWTRI_OK and looks at no pointer.  SNOWTRI_DEVICE: asynchronous on
 * `stream`, no host read, no allocation, no internal stream.  SNOWTRI_HOST: staged and synchronous. */
#define SNOWTRI_REPROJECT_RAW 1u /* flags: pixels on the raw (distorted) frame */
int snowtri_reproject(snowtri_ctx *ctx, int64_t F, int32_t P, int32_t kn, const void *xyzs, int xyz_dtype, uint32_t flags,
                      void *pix, int pix_dtype, int memspace, void *stream);
int snowtri_reproject_cost(snowtri_ctx *ctx, int64_t F, int32_t P, int32_t kn, const void *xyzs, int xyz_dtype, int32_t Pmax,
                           const void *kpts, int kpts_dtype, const int32_t *n_persons /* [F][C], may be NULL */,
                           double keypoint_score_threshold, uint32_t flags, double *cost_sum, int32_t *cost_n, int memspace,
                           void *stream);

/* Assignment: the optimal ONE-TO-ONE matching of a camera's detections to the 3D persons, on the costs snowtri_reproject_cost wrote
 * (no reference counterpart).  Picking each person's cheapest detection on its own lets two persons claim one detection -- one
 * behind the other in a view, a ghost beside a real person -- and everything built on the match then pulls both towards the same 2D
 * skeleton.  The rule, in fp64, per problem i < n (one frame and camera: n = F * C, the layout of snowtri_reproject_cost consumed
 * unchanged) with P persons (rows), Pmax detections (columns) and gate2 = gate_px * gate_px:
 *   1. mean[p][q] = cost_sum[i][p][q] / cost_n[i][p][q], one correctly rounded division.  The pair (p, q) is ADMISSIBLE iff
 *      cost_n >= min_joints, the mean is not NaN and -inf < mean <= gate2; every other pair costs +inf.  (A detection behind
 *      n_persons[f][c] has cost_n == 0 already: n_persons is no input.)
 *   2. Staying unmatched costs gate2: the cost matrix is a[P][Pmax + P], columns q < Pmax hold the means, column Pmax + p is person
 *      p's private dummy (gate2 in row p, +inf elsewhere).  A perfect matching of the rows always exists; the rule returns one of
 *      minimum sum, and a person on its dummy is unmatched.  Two persons that both fit detection 0 get detections 0 and 1 if the
 *      second fits either of them inside the gate, otherwise the worse-fitting one goes unmatched: the standard gated assignment.
 *   3. WHICH optimum is fixed by the algorithm, the shortest-augmenting-path (Hungarian / Jonker-Volgenant) method in its textbook
 *      form: rows inserted in order p = 0, 1, ..., duals u (rows) and v (columns), all 0 at the start.  Inserting row i: minv[j] =
 *      +inf, no column used, j0 = a virtual column holding row i; then, until j0 is a column without a row: mark j0 used, i0 = its
 *      row; for the unused columns j in increasing order cur = (a[i0][j] - u[i0]) - v[j], in that order; if cur < minv[j] then
 *      minv[j] = cur and way[j] = j0; if minv[j] < delta (+inf at the start of the scan) then delta = minv[j], j1 = j -- both
 *      comparisons strict, so ties go to the lowest column; then u of every used column's row += delta and its v -= delta, every
 *      other minv -= delta, j0 = j1.  At the end the columns along way[] from j0 back to the virtual one each take the row of the
 *      column before them.  Only additions, subtractions and comparisons of fp64 values: there is no product that could contract
 *      into a fused multiply-add, +inf never meets -inf, and delta is always finite (row i's own dummy, at the finite gate2, is outside the tree).
 *   4. det_of[i][p] = the detection of person p or -1; person_of[i][q] = the person that took detection q or -1 (the detections
 *      nobody claimed); total[i] = the sum of mean over the matched pairs, added in increasing p with plain additions from 0.
 * snowmocap_amd/reproject.py::assign_detections_reference is this rule in NumPy, and the kernel (snowmocap_amd/csrc/snowtri_assign.hpp,
 * k_assign: a lane is a column, delta by a butterfly on the pair (minv, column), whose minimum is exact in any order) performs the
 * same operations on the same values: EVERY OUTPUT AGREES WITH IT BIT FOR BIT, the integers and the bits of total.  A problem's
 * output depends on its own P x Pmax costs, gate_px and min_joints only: not on n, its place in the launch, the problems packed into
 * the same wave (64 / W of them, W = the smallest of 8, 16, 32, 64 >= P + Pmax) or how a batch is cut into calls.
 *
 * person_of and total may be NULL (not wanted).  Refusals (SNOWTRI_ERR_BAD_ARG, snowtri_last_error() names the argument; nothing is
 * enqueued or written): a NULL context, an unknown memspace, n < 0, P or Pmax < 1, P + Pmax > 64 (a problem's columns are the lanes
 * of one wave), min_joints < 1, a gate_px that is negative or NaN, a gate_px above 1e150 (rule 2 needs a finite cost of staying
 * unmatched and the duals are sums of a few of them; the infinite gate that means "no gate" elsewhere is not offered here), a NULL
 * cost_sum, cost_n or det_of, a device pointer that is not aligned to its element size, n * P * Pmax > 2^48, n > (2^31 - 1) * 4 * (64 / W) (the grid).  n == 0 is SNOWTRI_OK and looks at
 * no pointer.  SNOWTRI_DEVICE: asynchronous on `stream`, no host read, no allocation, no internal stream.  SNOWTRI_HOST: staged and
 * synchronous.  The context needs no cameras.  With snowtri_set_timing on, snowtri_last_kernel_ms gives k_assign's time in
 * kernel_ms[0] (kernel_ms[1] is 0: there is no second phase). */
int snowtri_assign_detections(snowtri_ctx *ctx, int64_t n, int32_t P, int32_t Pmax, const double *cost_sum, const int32_t *cost_n,
                              double gate_px, int32_t min_joints, int32_t *det_of /* [n][P] */,
                              int32_t *person_of /* [n][Pmax] or NULL */, double *total /* [n] or NULL */, int memspace, void *stream);

/* Refinement: joint records of ANY route moved to a local minimum of their weighted reprojection error, in pixels (no reference
 * counterpart).  Every route ends in a closed-form estimate -- the score-weighted mean of two-ray midpoints (SNOWTRI_PAIRWISE), the
 * minimiser of an algebraic error (the DLT methods) -- and none of them minimises the distance between the joint's projections and
 * the detections, which is the quantity the detector's noise lives in and the one snowtri_reproject_cost reports.  A few
 * Gauss-Newton steps from the closed-form point on a 3 x 3 system per joint find the maximum-likelihood point under pixel noise.
 * The rule, in fp64 throughout (PD = positive definite), per record (f, p, j) of xyzs [F][P][kn][4], X0 = its (x, y, z), with the
 * keypoints kpts [F][C][Pmax][kn][3] ON THE UNDISTORTED FRAME:
 *   1. The view set V, fixed once at X0.  Camera c is in V iff ALL of:
 *        - its detection q = det_of[f][c][p] satisfies 0 <= q < n_persons[f][c] (det_of NULL: q = p, which requires P <= Pmax;
 *          n_persons NULL: Pmax everywhere; an n_persons above Pmax counts as Pmax);
 *        - the observation (u, v, s) = kpts[f][c][q][j] has finite u, v and not (s < keypoint_score_threshold);
 *        - bit c of views[f][p][j] is set, when `views` is given (the mask snowtri_triangulate_robust writes: refine over the
 *          views the robust method kept);
 *        - the projection of X0 into c is VALID by rule 4 of "Reprojection" (measured record, pc2 > 0, finite pixel).
 *      Weight w_c = 1, or w_c = s with SNOWTRI_REFINE_SCORE_WEIGHTS.
 *   2. A missing record is copied bit for bit (code SNOWTRI_REFINE_MISSING).  A measured record with |V| < 2 is copied bit for bit
 *      (SNOWTRI_REFINE_FEW_VIEWS).
 *   3. Cost E(X) = sum over c in V of w_c ((u_c(X) - u_c)^2 + (v_c(X) - v_c)^2) with the undistorted projection of rules 1 and 3 of
 *      "Reprojection".  Analytic 2 x 3 Jacobian: dx = (R^T row 0 - x R^T row 2) / pc2, dy likewise, du = fx dx + s dy, dv = fy dy.
 *   4. At most `iters` steps (1..16): H = sum w J^T J, g = sum w J^T r; H d = -g by a 3 x 3 LDL^T; a pivot that is not finite or not
 *      > 0 ends the record's iteration.  The trial X + d is ACCEPTED iff every view of V is valid at it and E(X + d) < E(X),
 *      strictly.  A rejected trial ends the record's iteration (no damping, no step halving).  So the output cost never exceeds the
 *      input cost, and the iteration stops by itself at the rounding floor of E.
 *   5. Output record = (X, the input score), rounded once to xyz_dtype; a record no step moved is the input's bits.  Code
 *      SNOWTRI_REFINE_KEPT if no step was accepted, SNOWTRI_REFINE_MOVED otherwise.
 * cost [F][P][kn][2] float64 (may be NULL): E at the input and at the output, (0, 0) for copied records.  codes [F][P][kn] uint8
 * (may be NULL).  snowmocap_amd/refine.py::refine_joints_reference is this rule in NumPy, plain operations in this order; the kernel
 * (snowmocap_amd/csrc/snowtri_refine.hpp: k_refine, one lane per record) fixes V with project_record itself and forms E in exactly
 * these plain operations -- E at a given point is the NumPy rule's bit for bit, so the cost a caller recomputes that way never rises
 * either, even at exact detections where E is nothing but rounding; only H and g use fused multiply-adds -- and reaches the
 * same minimum to the rule's own floor -- strict decrease of E stops resolving a step d once d^T H d < eps E -- which
 * tests/refine_cases.py measures against a 50-digit minimiser.  A record's output bits depend on its own record, its own
 * observations and the rig only: not on F, its place in the launch, or how a batch is cut into calls.
 *
 * Refusals as for snowtri_reproject_cost (SNOWTRI_ERR_BAD_ARG, snowtri_last_error() names the argument; nothing is enqueued or
 * written), and: iters outside 1..16, an unknown flag bit, more than 32 cameras, det_of == NULL with P > Pmax, out_xyzs overlapping
 * xyzs other than exactly (out_xyzs == xyzs refines in place).  F * P * kn <= (2^31 - 1) * 256 records.  F == 0 is SNOWTRI_OK and
 * looks at no pointer.  SNOWTRI_DEVICE: asynchronous on `stream`, no host read, no allocation, no internal stream.  SNOWTRI_HOST:
 * staged and synchronous.
 *
 * ROBUST LOSS (snowtri_refine_joints_ex, snowtri_refine_cameras_ex): one more parameter, huber_px = delta in pixels, of this rule
 * and of "Camera pose refinement".  Everything not named here stays word for word as the two rules state it: the view and
 * observation sets fixed once at the input, the at-least-two-views clause (a record's views are counted whatever regime they are
 * in), fp64, a step taken only if every view stays valid and the cost falls strictly, no damping, the codes, records and poses
 * copied bit for bit.  Per view (joints) or observation (cameras), ru and rv the pixel residuals as above, s = ru ru + rv rv:
 *     quadratic regime, s <= delta delta:   rho = s,                            kappa = 1;
 *     linear regime, otherwise:             r = sqrt(s), rho = (2 delta) r - delta delta,   kappa = delta / r;
 *     E = sum w rho (in the order the rule sums);   H = sum (w kappa) J^T J,   g = sum (w kappa) J^T r.
 * 2 delta and delta delta are formed once, in fp64, on the host; sqrt is the correctly rounded fp64 one; w is 1 or the score.  The
 * w kappa are IRLS weights: no second-order term of rho is used, so H stays positive semi-definite.  E decides every step and is
 * what is reported, so it is formed in plain, separately rounded operations in this order, and at a given point equals
 * refine_joints_reference(huber_px=...)'s bit for bit.  CONSEQUENCES: huber_px == 0 is the squared loss and returns the bits of
 * snowtri_refine_joints / snowtri_refine_cameras, which are calls of the _ex entries with huber_px = 0 and a NULL new output.  A
 * delta so large that no view is in the linear regime (1e6 px, say) returns those bits too -- w * 1.0 is w: the quadratic regime
 * is the squared rule operation for operation.  huber_px must be finite, >= 0 and <= 1e150 (delta delta must not overflow: the
 * bound of snowtri_assign_detections' gate); anything else is refused.
 * NEW OUTPUTS.  Joints: outliers [F][P][kn] uint32 (may be NULL): bit c is set iff camera c is in the record's view set V and in
 * the linear regime at the OUTPUT point; 0 for a copied record, and all 0 with huber_px == 0.  V & ~outliers is an inlier mask in
 * the format of `views`: a producer of that mask for the routes that have none (SNOWTRI_PAIRWISE).  It must not overlap xyzs or
 * out_xyzs.  Cameras: n_outliers [C] int64 (may be NULL): the observations of S_c in the linear regime at the output pose; 0 for
 * FIXED and FEW_OBS cameras.
 * WHAT THE LOSS DOES NOT PROMISE.  IRLS converges linearly, not quadratically.  Measured for the NumPy rule on the test cases
 * (tests/huber_cases.py: 10 % of the detections moved by 20..150 px, shape (2, 3, 21), iters = 16) against up to 200 steps of
 * 50-digit IRLS on the same cost from the rule's output: a record with three or more views in the quadratic regime is within
 * 5.6e-10 .. 2.8e-7 of the rig's scale of that minimiser; with exactly two the convergence is sometimes slow (up to 1.7e-5); with
 * FEWER THAN TWO (0.8 % of the refined records with 5 cameras, 4 .. 5 % with 4, 15 .. 17 % with 3) the rule is up to 7e-2 of the
 * rig's scale away after 16 steps, and a fifth of those records have not settled after 200 steps in 50 digits: such a record is
 * ambiguous, not badly solved -- the inliers do not fix its point.  popcount(V & ~outliers) < 2 marks it; treat it as unmeasured or
 * keep the closed-form point.  Camera poses have hundreds of observations each and do not show this.
 * NOT offered: refinement on the raw frame (undistort first: snowtri_undistort_keypoints is an exact inverse); other losses
 * (Cauchy, Tukey), an automatic delta, the Triggs second-order correction of the Huber loss, damping; more than 32 cameras. */
#define SNOWTRI_REFINE_SCORE_WEIGHTS 1u /* flags: w_c = the observation's score instead of 1 */
#define SNOWTRI_REFINE_MISSING 0
#define SNOWTRI_REFINE_FEW_VIEWS 1
#define SNOWTRI_REFINE_KEPT 2
#define SNOWTRI_REFINE_MOVED 3
int snowtri_refine_joints(snowtri_ctx *ctx, int64_t F, int32_t P, int32_t kn, const void *xyzs, int xyz_dtype, int32_t Pmax,
                          const void *kpts, int kpts_dtype, const int32_t *n_persons /* [F][C] or NULL */,
                          const int32_t *det_of /* [F][C][P] or NULL */, const uint32_t *views /* [F][P][kn] or NULL */,
                          double keypoint_score_threshold, int32_t iters, uint32_t flags, void *out_xyzs /* xyz_dtype; may be xyzs itself */,
                          double *cost /* or NULL */, uint8_t *codes /* or NULL */, int memspace, void *stream);
/* ... with the loss of ROBUST LOSS above (huber_px == 0: the squared loss, the entry above bit for bit) and `outliers`.  Further
 * refusals: huber_px NaN, negative or above 1e150; outliers misaligned (SNOWTRI_DEVICE) or overlapping xyzs / out_xyzs. */
int snowtri_refine_joints_ex(snowtri_ctx *ctx, int64_t F, int32_t P, int32_t kn, const void *xyzs, int xyz_dtype, int32_t Pmax,
                             const void *kpts, int kpts_dtype, const int32_t *n_persons /* [F][C] or NULL */,
                             const int32_t *det_of /* [F][C][P] or NULL */, const uint32_t *views /* [F][P][kn] or NULL */,
                             double keypoint_score_threshold, int32_t iters, uint32_t flags, double huber_px,
                             void *out_xyzs /* xyz_dtype; may be xyzs itself */, double *cost /* or NULL */, uint8_t *codes /* or NULL */,
                             uint32_t *outliers /* [F][P][kn] or NULL */, int memspace, void *stream);

/* Camera pose refinement: each camera's six pose parameters moved to a local minimum of its weighted reprojection error, with the
 * joints held fixed (no reference counterpart).  K, R, t come from a calibration file and are trusted for a whole recording; a rig
 * does not hold still -- a tripod is nudged, a mount sags -- and snowtri_reproject_cost shows the camera that moved without being
 * able to repair it.  This is the cost of "Refinement" minimised over the other block of unknowns; alternated with triangulation
 * it is block-coordinate bundle adjustment of the extrinsics (snowmocap_amd/pose.py::refine_rig).  The rule, in fp64 throughout,
 * per camera c, with the inputs of snowtri_refine_joints (xyzs [F][P][kn][4], kpts [F][C][Pmax][kn][3] ON THE UNDISTORTED FRAME,
 * n_persons, det_of, views, keypoint_score_threshold, SNOWTRI_REFINE_SCORE_WEIGHTS) and free_mask (bit c: camera c may move),
 * min_obs (>= 3), iters (1..16):
 *   1. The observation set S_c, fixed once at the input pose.  Record (f, p, j) is in S_c iff ALL of: the record is measured; its
 *      detection q = det_of[f][c][p] is listed (0 <= q < n_persons[f][c], as in rule 1 of "Refinement"); the observation
 *      (u_obs, v_obs, s) = kpts[f][c][q][j] has finite u, v and not (s < keypoint_score_threshold); bit c of views[f][p][j] is
 *      set, when `views` is given; the projection of the record into c is VALID by rule 4 of "Reprojection".  These are exactly the
 *      per-view conditions of rule 1 of "Refinement"; there is no "at least two views" clause, which belongs to a joint and not to
 *      a camera.  n_c = |S_c|.  Weight w = 1, or w = s with SNOWTRI_REFINE_SCORE_WEIGHTS.
 *   2. Pose parameters delta = (omega, tau): R(delta) = Exp(omega) R_c, t(delta) = t_c + tau, R_c camera -> world as given to
 *      snowtri_ctx_create.  Exp is Rodrigues' formula I + a [omega]x + b [omega]x^2 with th = |omega|, a = sin(th) / th,
 *      b = 2 sin^2(th / 2) / th^2, and a = 1, b = 1/2 at th = 0.
 *   3. Cost E_c = sum over S_c of w ((u - u_obs)^2 + (v - v_obs)^2) with rules 1 and 3 of "Reprojection" under the current pose.
 *      Analytic 2 x 6 Jacobian at delta = 0: dpc / domega = R^T [d]x, dpc / dtau = -R^T with d = X - t;
 *      dx = (dpc0 - x dpc2) / pc2, dy likewise; du = fx dx + s dy, dv = fy dy.
 *   4. At most `iters` steps: H = sum w J^T J (21 values, the lower triangle row by row), g = sum w J^T r; H delta = -g by a 6 x 6
 *      LDL^T; a pivot that is not finite or not > 0 ends the camera's iteration.  The trial pose is ACCEPTED iff every observation
 *      of S_c is valid at it and E is strictly lower.  A rejected trial ends the camera's iteration (no damping, as in
 *      "Refinement").  So a camera's cost never rises.
 *   5. A camera outside free_mask keeps its pose bit for bit (code SNOWTRI_POSE_FIXED), and so does one with n_c < min_obs
 *      (SNOWTRI_POSE_FEW_OBS).  Otherwise SNOWTRI_POSE_KEPT (no step accepted: the input's bits) or SNOWTRI_POSE_MOVED.
 *   6. R_out [C][9] (row-major, camera -> world), t_out [C][3] float64.  cost [C][2]: E at the input and at the output, (0, 0) for
 *      FIXED and FEW_OBS.  n_obs [C] int64.  codes [C] uint8.  normal [C][28]: E, g[6], H[21] at the INPUT pose, for every camera,
 *      the fixed ones too.  cost, n_obs, codes and normal may each be NULL.
 * SUMMATION.  The sums over S_c are formed in an order that depends on (F, P, kn, C) alone -- fixed partial sums: a lane adds the
 * records i = (b + k G) 256 + lane of its block b in turn, G = min(ceil(F P kn / 256), 1024); a fixed butterfly over the wave, the
 * four waves in order; then the blocks of a camera in 32 runs of consecutive blocks, each in block order, and the runs in order; no
 * floating-point atomics -- so two runs give the same bits.  It is NOT record order: E, g and H agree with the NumPy rule
 * (snowmocap_amd/pose.py::refine_cameras_reference, plain operations, observations summed in record order) to rounding, not bit for
 * bit, as snowtri_reproject_cost's sum does.  snowtri_pose_sweep_records() = 1024 * 256: the records one sweep of the grid covers.
 *
 * THE CONTEXT'S OWN RIG IS NOT MODIFIED: the rig constants of every other kernel are derived at snowtri_ctx_create, so the caller
 * builds a new context from the returned poses.
 * Refusals as for snowtri_refine_joints (SNOWTRI_ERR_BAD_ARG, snowtri_last_error() names the argument; nothing is enqueued or
 * written), and: min_obs < 3, more than 32 cameras, a free_mask bit at or above C, a NULL R_out or t_out.  F == 0 is SNOWTRI_OK:
 * every pose is copied, the codes are FIXED or FEW_OBS, and no input pointer is looked at.
 * SNOWTRI_DEVICE: asynchronous on `stream`, no host read -- the solve and the accept decision happen on the device -- and
 * 2 (iters + 1) launches whatever the data does.  The context owns a small workspace (the trial poses and the partial sums, 256 KB
 * per camera), allocated by the FIRST call on that context and by no later call; it is why only ONE CALL MAY BE IN FLIGHT PER
 * CONTEXT.  SNOWTRI_HOST: staged and synchronous.
 * ROBUST LOSS (snowtri_refine_cameras_ex): huber_px = delta in pixels, the loss stated under "Refinement", ROBUST LOSS, applied per
 * observation of S_c: E_c = sum w rho, H = sum (w kappa) J^T J, g = sum (w kappa) J^T r, in the SUMMATION order above; rule 4's
 * accept test compares that E_c.  huber_px == 0 is the squared loss and returns snowtri_refine_cameras' bits (which is this entry
 * with huber_px = 0 and a NULL n_outliers), and so does a delta that puts no observation in the linear regime.  n_outliers [C]
 * int64 (may be NULL): the observations of S_c in the linear regime at the OUTPUT pose, 0 for FIXED and FEW_OBS cameras; it
 * travels with the partial sums (a count in a double, exact up to 2^53).  `normal` is E, g, H of the loss at the input pose.  Unlike
 * a `views` mask from SNOWTRI_DLT_ROBUST, whose leave-one-out gate removes exactly a nudged camera's views, the loss keeps every
 * observation and down-weights the far ones.  Refused as well: huber_px NaN, negative or above 1e150, a misaligned n_outliers.
 * INTRINSICS (snowtri_refine_cameras_k): four more parameters per camera and two more inputs of this rule.  A chessboard K that is
 * a percent or two off, or a lens refocused after calibration, is as common as a nudged tripod, and pose-only refinement of a
 * camera whose K is wrong lowers its RMS by MOVING THE CAMERA.  Everything not named here stays word for word as stated above.
 *   PARAMETERS, per camera, in this order: omega[3], tau[3], fx, fy, cx, cy.  The four intrinsics are additive: fx + d6, fy + d7,
 *     cx + d8, cy + d9.  The skew K[0][1] and the last row of K are never changed.
 *   intr_flags: SNOWTRI_INTR_FOCAL frees fx and fy, SNOWTRI_INTR_CENTRE frees cx and cy.  intr_mask: bit c says camera c's
 *     intrinsics may move; it is independent of free_mask (the camera that holds the gauge of an alternation may still have its
 *     intrinsics refined).  A camera's FREE SET is the six pose parameters if it is in free_mask, plus the flagged intrinsics if it
 *     is in intr_mask: n = 0, 2, 4, 6, 8 or 10 parameters.
 *   S_c is rule 1 unchanged, fixed once at the input pose and the input K.
 *   JACOBIAN: the six pose columns of rule 3, and du/dfx = x, dv/dfx = 0; du/dfy = 0, dv/dfy = y; du/dcx = 1, dv/dcx = 0;
 *     du/dcy = 0, dv/dcy = 1 (x = pc0 / pc2, y = pc1 / pc2).
 *   NORMAL EQUATIONS: E, g[10], H[55] over all ten parameters whichever of them are free; H is the lower triangle of the 10 x 10
 *     matrix row by row in the order above.  The loss of ROBUST LOSS applies as stated: w rho in E, w kappa in g and H.
 *   A STEP: the rows and columns of the free set, in order; the same plain-operation LDL^T at size n, and a pivot that is not
 *     finite or not > 0 ends the camera's iteration; the trial is Exp(omega) R, t + tau, fx + d6, fy + d7, cx + d8, cy + d9 (a
 *     parameter outside the free set keeps its bits); it is ACCEPTED iff every observation of S_c is valid at it, its fx and fy are
 *     finite and > 0, and E is strictly lower.  A rejected trial ends the iteration.
 *   CODES: n = 0 is SNOWTRI_POSE_FIXED, n_c < min_obs SNOWTRI_POSE_FEW_OBS, otherwise KEPT or MOVED as in rule 5.
 *   OUTPUTS: K_out [C][9] row-major, required when intr_flags != 0 (the context's K with fx, fy, cx, cy of a MOVED camera
 *     replaced); R_out, t_out; cost, n_obs, codes, n_outliers as above; normal [C][66]: E, g[10], H[55] at the input.
 * SUMMATION of this entry: a lane adds its records as stated under SUMMATION, the same butterfly over the wave and the four waves
 * in order; then the blocks of a camera in 32 runs of consecutive blocks, each in block order, and the runs in order, slot by slot
 * of the 72-double partial (three passes of 32 slots); no floating-point atomics.  It depends on (F, P, kn, C) alone: two runs give
 * the same bits.  The sums of the six pose parameters are formed by the operations and in the order of snowtri_refine_cameras_ex.
 * The entries of H that are structurally zero (fx.fy, fx.cy, fy.cx, cx.cy) are stored as 0.0, and cy.cy is cx.cx: both are sum w.
 * CONSEQUENCES.  With intr_flags == 0 or intr_mask == 0 this entry is snowtri_refine_cameras_ex bit for bit on every output (of
 * `normal` the 28 values of E, g[6] and the 6 x 6 block of H, which stand at 0, 1..6 and 11..31 of the 66), and K_out, if given, is
 * the context's K.  A camera with its pose fixed and its intrinsics free returns R and t bit for bit; a camera outside intr_mask
 * returns K bit for bit.  snowtri_refine_cameras and snowtri_refine_cameras_ex keep their signatures, kernels, workspace and bits.
 * The intrinsics path has ITS OWN WORKSPACE (576 KB per camera), allocated by the first call of THIS entry on a context and by no
 * later call; the workspace of the two entries above and its "first call only" behaviour are untouched.  ONE CALL IN FLIGHT PER
 * CONTEXT, 2 (iters + 1) launches whatever the data does, SNOWTRI_DEVICE asynchronous with no host read.  THE CONTEXT'S OWN RIG IS
 * NOT MODIFIED: build a new context from K_out, R_out, t_out.
 * WHAT IT DOES NOT PROMISE.  Ten parameters need thousands of observations: the principal point and the rotation are strongly
 * correlated (a shift of the centre and a small pan move the pixels almost alike), so with a few hundred noisy observations per
 * camera the ten-parameter minimum is as far from the truth as a percent-level calibration error (EXPERIMENTS.md has the figures);
 * free fewer parameters, hold the pose, or record longer.  With a lens (a distortion set on the context) the detections were
 * undistorted with the OLD K and must be undistorted again from the raw frame once K has moved; nothing here does that.
 * Refused as well: an unknown intr_flags bit, an intr_mask bit at or above C, intr_flags != 0 with a NULL K_out, a misaligned K_out.
 * NOT offered: lens coefficients, the skew, a focal length shared between cameras; other losses (Cauchy, Tukey), an automatic
 * delta, the Triggs second-order correction; damping; points and cameras adjusted in one system; more than 32 cameras. */
#define SNOWTRI_POSE_FIXED 0
#define SNOWTRI_POSE_FEW_OBS 1
#define SNOWTRI_POSE_KEPT 2
#define SNOWTRI_POSE_MOVED 3
int snowtri_pose_sweep_records(void);
int snowtri_refine_cameras(snowtri_ctx *ctx, int64_t F, int32_t P, int32_t kn, const void *xyzs, int xyz_dtype, int32_t Pmax,
                           const void *kpts, int kpts_dtype, const int32_t *n_persons /* [F][C] or NULL */,
                           const int32_t *det_of /* [F][C][P] or NULL */, const uint32_t *views /* [F][P][kn] or NULL */,
                           double keypoint_score_threshold, uint32_t free_mask, int32_t min_obs, int32_t iters, uint32_t flags,
                           double *R_out /* [C][9] */, double *t_out /* [C][3] */, double *cost /* [C][2] or NULL */,
                           int64_t *n_obs /* [C] or NULL */, uint8_t *codes /* [C] or NULL */, double *normal /* [C][28] or NULL */,
                           int memspace, void *stream);
int snowtri_refine_cameras_ex(snowtri_ctx *ctx, int64_t F, int32_t P, int32_t kn, const void *xyzs, int xyz_dtype, int32_t Pmax,
                              const void *kpts, int kpts_dtype, const int32_t *n_persons /* [F][C] or NULL */,
                              const int32_t *det_of /* [F][C][P] or NULL */, const uint32_t *views /* [F][P][kn] or NULL */,
                              double keypoint_score_threshold, uint32_t free_mask, int32_t min_obs, int32_t iters, uint32_t flags,
                              double huber_px, double *R_out /* [C][9] */, double *t_out /* [C][3] */, double *cost /* [C][2] or NULL */,
                              int64_t *n_obs /* [C] or NULL */, uint8_t *codes /* [C] or NULL */, double *normal /* [C][28] or NULL */,
                              int64_t *n_outliers /* [C] or NULL */, int memspace, void *stream);
#define SNOWTRI_INTR_FOCAL 1u  /* intr_flags: fx and fy may move */
#define SNOWTRI_INTR_CENTRE 2u /* intr_flags: cx and cy may move */
int snowtri_refine_cameras_k(snowtri_ctx *ctx, int64_t F, int32_t P, int32_t kn, const void *xyzs, int xyz_dtype, int32_t Pmax,
                             const void *kpts, int kpts_dtype, const int32_t *n_persons /* [F][C] or NULL */,
                             const int32_t *det_of /* [F][C][P] or NULL */, const uint32_t *views /* [F][P][kn] or NULL */,
                             double keypoint_score_threshold, uint32_t free_mask, uint32_t intr_mask, uint32_t intr_flags,
                             int32_t min_obs, int32_t iters, uint32_t flags, double huber_px,
                             double *K_out /* [C][9]; may be NULL only with intr_flags == 0 */, double *R_out /* [C][9] */,
                             double *t_out /* [C][3] */, double *cost /* [C][2] or NULL */, int64_t *n_obs /* [C] or NULL */,
                             uint8_t *codes /* [C] or NULL */, double *normal /* [C][66] or NULL */,
                             int64_t *n_outliers /* [C] or NULL */, int memspace, void *stream);

/* Matched triangulation: the robust N-view DLT of 3D person p over the detections that det_of names (no reference counterpart).
 * The matching chain -- snowtri_reproject_cost, snowtri_assign_detections -- ends in det_of[f][c][p], the detection of camera c that
 * belongs to person p; this entry triangulates from that answer, so that a person is fused from EVERY view that saw it, with
 * SNOWTRI_DLT_ROBUST's leave-one-out gate on each joint, and its `views` output is the mask snowtri_refine_joints and
 * snowtri_refine_cameras take.  Inputs: kpts [F][C][Pmax][kn][3] ON THE UNDISTORTED FRAME, n_persons [F][C] or NULL, det_of
 * [F][C][P] or NULL.  The rule, per frame f, person p < P and joint j < kn:
 *   1. Camera c LISTS person p iff q = det_of[f][c][p] satisfies 0 <= q < n_persons[f][c] -- the first condition of rule 1 of
 *      "Refinement", word for word: det_of NULL means q = p, which requires P <= Pmax; n_persons NULL means Pmax everywhere; an
 *      n_persons above Pmax counts as Pmax.  Its observation is then (u_c, v_c, s_c) = kpts[f][c][q][j]; a camera that does not
 *      list the person has the observation (0, 0, 0) and is in no set below.
 *   2. The record is what rules 1-4 of snowtri_triangulate_robust give on these C observations, with "camera c lists person p" in
 *      the place of n_persons[f][c] > 0: the start set S = { c listed : not (s_c < keypoint_score_threshold) }; |S| < 2 gives the
 *      record (0, 0, 0, 0), views = 0, resid = 0; the same rig-frame DLT, the same leave-one-out loop with reproj_threshold_px and
 *      max_drops, the same NaN and tie behaviour (there is NO finite-pixel condition: as there, a non-finite pixel of a listed
 *      camera reaches the solve); joint score = mean of s_c over the final S; views = bit mask of the final S; resid = the RMS pixel
 *      residual over it.  out_pscore[f][p] = the mean of the kn joint scores.
 * Two persons may name the same detection and then get the same record: one-to-one is the matcher's business.  Every (f, p) slot
 * is written; there are no count or flags outputs, P is the caller's.  snowmocap_amd/matched.py::triangulate_matched_reference is
 * this rule in NumPy (it gathers per person and calls triangulate_robust_reference).  The kernel (k_dlt_matched,
 * snowmocap_amd/csrc/snowtri_matched.hpp: one lane per (f, p, j), the tile's det_of / n_persons resolved once into LDS) runs
 * k_dlt_robust's own item -- one device function, robust_item, serves both -- so person p's xyzs, pscore, views and resid equal
 * snowtri_triangulate_robust's on that person's gathered [F][C][1][kn][3] keypoints (n_persons = listed) BIT FOR BIT, and agree with
 * the NumPy rule as that entry does.  A person's bits depend on its own observations, the rig and the settings only: not on F, P,
 * Pmax, its slot, its neighbours, the order of a camera's list, or how a batch is cut into calls.
 *   out_xyzs [F][P][kn][4] and out_pscore [F][P] (may be NULL) of out_dtype, out_views [F][P][kn] uint32 (may be NULL), out_resid
 *   [F][P][kn] of out_dtype (may be NULL); a NULL output costs nothing and nothing is written for it.
 * Refusals (SNOWTRI_ERR_BAD_ARG, snowtri_last_error() names the argument; nothing is enqueued or written): a NULL context, an
 * unknown dtype or memspace, F < 0, P, kn or Pmax < 1, fewer than 2 or more than 8 cameras, a reproj_threshold_px or max_drops that
 * snowtri_ctx_set_robust refuses, a NaN keypoint_score_threshold, det_of == NULL with P > Pmax, a NULL kpts or out_xyzs, a device
 * pointer that is not aligned (out_xyzs: 16 bytes, every other array: its element), the size limits of snowtri_refine_joints,
 * one frame's P * kn joint scores (8 bytes each) that do not fit the LDS of a CU beside the kernel's tables.  F == 0 is
 * SNOWTRI_OK and looks at no pointer.  SNOWTRI_DEVICE: asynchronous on `stream`, no host read, no allocation, no internal stream.
 * SNOWTRI_HOST: staged and synchronous.
 * snowtri_last_kernel_names reports k_dlt_matched<...> after the call; with snowtri_set_timing on, snowtri_last_kernel_ms gives its
 * time in kernel_ms[0] (kernel_ms[1] is 0).
 * NOT offered: more than 8 cameras; matching against the previous frame's persons.  (Seeding new persons from the detections nobody
 * claimed, person_of of snowtri_assign_detections, is "Seeding" below.) */
int snowtri_triangulate_matched(snowtri_ctx *ctx, int64_t F, int32_t P, int32_t kn, int32_t Pmax, const void *kpts, int kpts_dtype,
                                const int32_t *n_persons /* [F][C] or NULL */, const int32_t *det_of /* [F][C][P] or NULL */,
                                double keypoint_score_threshold, double reproj_threshold_px, int32_t max_drops,
                                void *out_xyzs /* [F][P][kn][4] */, void *out_pscore /* [F][P] or NULL */, int out_dtype,
                                uint32_t *out_views /* [F][P][kn] or NULL */, void *out_resid /* [F][P][kn] or NULL */, int memspace,
                                void *stream);

/* Seeding: 3D persons from the detections nobody claimed (no reference counterpart).  The matching chain improves the persons the
 * first triangulation found; a detection no person took (person_of[f][c][q] == -1 of snowtri_assign_detections) is a candidate for a
 * person it missed.  Two entries: the PAIR COST of every two detections of two cameras, and the GROUPING of a frame's free detections
 * into seeds, sets of mutually close detections of different cameras, written in the layout of det_of so that
 * snowtri_triangulate_matched triangulates them unchanged.  With claimed == NULL every detection is free and the two calls are an
 * association of their own, in ray space.
 *
 * snowtri_pair_cost.  kpts [F][C][Pmax][kn][3] on the undistorted frame, n_persons [F][C] or NULL (Pmax everywhere; a value above
 * Pmax counts as Pmax), claimed [F][C][Pmax] or NULL: claimed >= 0 means the detection is taken (person_of consumed unchanged).
 * Outputs pair_sum (float64) and pair_n (int32) [F][NP][Pmax][Pmax], NP = C (C - 1) / 2, camera pairs k = (a < b) in the reference's
 * loop order (the order of the candidate slots); entry [f][k][q][r] belongs to detection q of camera a and detection r of camera b.
 * The rule, in fp64, per joint j:
 *   1. the ray h_c = M_c (u, v, 1), M_c = R_c K_c^-1 as snowtri_ctx_ray_matrices returns it;
 *   2. n = h_a x h_b, nn = n . n, w = (t_b - t_a) . n, d2 = w * w / nn: the squared distance between the two LINES, the square of
 *      the skew-ray method's distance.  No midpoint, no square root, no cheirality test;
 *   3. the joint COUNTS iff both detections count by the words of snowtri_reproject_cost (q < n_persons, not score < threshold,
 *      finite u and v), nn > 0 (parallel rays do not count) and d2 is finite;
 *   4. pair_n = the number of counting joints, pair_sum = the sum of their d2 (world units squared), 0 when pair_n is 0;
 *   5. a pair with a claimed member, or a member behind n_persons, is (0, 0) and its keypoints are not read.
 * As for snowtri_reproject_cost an item's sum is formed in an order that depends on kn alone -- not on F, Pmax, the item's place in
 * the launch or how a batch is cut into calls -- and the kernel (snowmocap_amd/csrc/snowtri_seed.hpp, k_pair_cost) writes its
 * products as fused multiply-adds: it agrees with snowmocap_amd/seed.py::pair_cost_reference to rounding, not bit for bit; pair_n
 * agrees exactly.
 * Refusals (SNOWTRI_ERR_BAD_ARG, snowtri_last_error() names the argument; nothing is enqueued or written): a NULL context, an unknown
 * dtype or memspace, F < 0, kn or Pmax < 1, fewer than 2 or more than 8 cameras, kn > 256, a NaN keypoint_score_threshold, a NULL
 * kpts, pair_sum or pair_n, a device pointer that is not aligned to its element size, F * NP > 2^31 - 1 (the grid), more than 2^48
 * costs or keypoints.  F == 0 is SNOWTRI_OK and looks at no pointer.  SNOWTRI_DEVICE: asynchronous on `stream`, no host read, no
 * allocation, no internal stream.  SNOWTRI_HOST: staged and synchronous.  With snowtri_set_timing on, snowtri_last_kernel_ms gives
 * the kernel's time in kernel_ms[0] (kernel_ms[1] is 0); the same holds for snowtri_seed_persons.
 *
 * snowtri_seed_persons.  One frame's NODES are x = c * Pmax + q, C * Pmax <= 64 (the lanes of one wave).  gate is an RMS line
 * distance in world units, gate2 = gate * gate; S is the number of seed slots.  The rule, per frame:
 *   1. node (c, q) is FREE iff q < n_persons[f][c] and claimed[f][c][q] < 0 (NULL: Pmax, nothing claimed);
 *   2. the edge between nodes of different cameras weighs mean = pair_sum / pair_n, one correctly rounded division; it is ADMISSIBLE
 *      iff pair_n >= min_joints, the mean is not NaN and mean <= gate2.  Every other edge, and every edge inside a camera, is +inf
 *      ("finite" below: less than +inf);
 *   3. until S seeds are emitted: among the edges between two free nodes take the one of smallest weight, ties to the lowest (x, y)
 *      with x < y, lexicographic; if none is finite, stop;
 *   4. M = {x, y}, then grow M: a candidate z is a free node outside M in a camera M does not hold with finite edges to ALL members
 *      (M stays a clique: two persons are never chained together through a third view); take the z whose LARGEST edge to a member
 *      is smallest, ties to the lowest node; stop when there is no candidate;
 *   5. |M| < min_views: no seed; the starting edge (x, y) becomes +inf for the rest of this frame, its members stay free, go to 3
 *      (every turn removes an edge or at least two free nodes, so the loop ends);
 *   6. otherwise seed s = n_seeds++ gets seed_det_of[f][c][s] = q for its member in camera c, -1 in every other camera, and its
 *      members are no longer free;
 *   7. slots at or behind n_seeds[f] hold -1.
 * flags[f] (optional) has SNOWTRI_SEED_FLAG_FULL iff the frame stopped at S seeds while step 3 still found a finite edge.
 * After the one division there are only comparisons: EVERY OUTPUT, flags included, EQUALS snowmocap_amd/seed.py::
 * seed_persons_reference BIT FOR BIT on the same pair_sum / pair_n (the kernel, k_seed_group, finds each minimum by a butterfly on
 * a totally ordered tuple, exact in any order).  A frame's output depends on its own inputs and the settings only.
 * Refusals: an unknown memspace, F < 0, Pmax < 1, S outside 1..64, min_joints < 1, a gate that is negative, NaN or above 1e150, a
 * NULL context, a context of fewer than 2 cameras (the context is needed for C alone), C * Pmax > 64, min_views outside 2..C, a NULL
 * pair_sum, pair_n, seed_det_of or n_seeds, a device pointer that is not aligned to its element size, F > 2^31 - 1.  F == 0 is
 * SNOWTRI_OK and looks at no pointer.  HOST / DEVICE as above.
 * NOT offered: more than 8 cameras in snowtri_pair_cost, C * Pmax > 64, seeding across time (a seed knows nothing of the frame
 * before it). */
#define SNOWTRI_SEED_FLAG_FULL 1u
int snowtri_pair_cost(snowtri_ctx *ctx, int64_t F, int32_t kn, int32_t Pmax, const void *kpts, int kpts_dtype,
                      const int32_t *n_persons /* [F][C] or NULL */, const int32_t *claimed /* [F][C][Pmax] or NULL */,
                      double keypoint_score_threshold, double *pair_sum /* [F][NP][Pmax][Pmax] */, int32_t *pair_n, int memspace,
                      void *stream);
int snowtri_seed_persons(snowtri_ctx *ctx, int64_t F, int32_t Pmax, const double *pair_sum, const int32_t *pair_n,
                         const int32_t *n_persons /* [F][C] or NULL */, const int32_t *claimed /* [F][C][Pmax] or NULL */, double gate,
                         int32_t min_joints, int32_t min_views, int32_t S, int32_t *seed_det_of /* [F][C][S] */,
                         int32_t *n_seeds /* [F] */, uint32_t *flags /* [F] or NULL */, int memspace, void *stream);

/* Measurement aid: HIP-event time (ms) of the kernels launched by the LAST
 * snowtri_triangulate_condense call on this context, measured on the stream they ran on
 * (blocks until they finish).  kernel_ms[0] = dominant fused kernel, [1] = everything else. */
int snowtri_last_kernel_ms(snowtri_ctx *ctx, float kernel_ms[2]);
/* With timing enabled every fused call also records a (begin, end) HIP-event pair in a ring (1024 deep), so a
 * caller can queue many launches back to back on one stream and read their individual durations afterwards:
 * writes up to `cap` durations (ms, oldest first) of the calls recorded since the last collect, returns how
 * many (blocks until they have finished; -1 on error). */
int snowtri_timing_collect(snowtri_ctx *ctx, float *kernel_ms, int32_t cap);
/* Toggle per-call event timing (off by default: it adds two event records per launch).  enabled = 1: the ring's pair
 * BRACKETS the call (an event record before its first and after its last kernel: the interval includes the command
 * processor's hand-over from the begin event to the dispatch and from the kernel's end to the end event, ~1 us).
 * enabled = 2: when the call is ONE kernel (the single-detection fast kernels, and k_dlt_coop / k_dlt_robust of the DLT methods) the pair is ATTACHED to that dispatch
 * (hipExtLaunchKernelGGL's start / stop events): the kernel's own begin and end, the duration a rocprofv3 kernel
 * trace reports, and no event record -- a barrier packet -- sits between consecutive launches, so a timing loop stays
 * back to back (snowtri_last_kernel_ms is not available for such a call); calls of several kernels are bracketed as with 1. */
int snowtri_set_timing(snowtri_ctx *ctx, int enabled);
/* Frames of the last SNOWTRI_HOST fused call that were resolved by the general routine instead of
 * the single-cluster fast path (-1 after a SNOWTRI_DEVICE call: count the frames whose out_flags
 * lack SNOWTRI_FLAG_FASTPATH instead). */
int64_t snowtri_last_slow_frames(snowtri_ctx *ctx);

/* Diagnostics: the kernels the LAST snowtri_triangulate_condense call on this context launched, in launch order,
 * as their template names joined by " + " (e.g. "k_fused_lean<4,float,133>"); "" before the first call.  The string
 * stays valid until the next fused call on this context.  bench.py names the kernel its roofline belongs to with it. */
const char *snowtri_last_kernel_names(const snowtri_ctx *ctx);

/* Device-side bounds checks (debug builds only: `make -C snowmocap_amd/csrc debug` compiles the kernels with
 * -DSNOWTRI_DEBUG_BOUNDS into snowmocap_amd/libsnowtri_dbg.so): every index a kernel derives -- tile and frame ranges,
 * LDS arena offsets, candidate slots, descriptor and member-list positions, person fields -- is checked where it is
 * used.  Returns the number of violated checks since the last call and clears it (0 = clean); *first (may be NULL)
 * receives (check code << 32 | source line) of the first one.  -1: this library was built without the checks
 * (the production build); -2: HIP error.  Synchronises the device. */
int64_t snowtri_debug_faults(snowtri_ctx *ctx, uint64_t *first);
/* Debug builds: launches one wave in which exactly three lanes violate a check with code 99, so that a test can see the
 * mechanism report (snowtri_debug_faults then returns 3).  -1 in the production build. */
int snowtri_debug_selftest(snowtri_ctx *ctx);

/* Test / diagnostics hook for the multi-person path: output persons of the last snowtri_triangulate_condense call
 * (its last segment) whose fusion (triangulation.py:136-152) was handed from the association kernel to the streaming
 * cluster kernels.  Returns the persons whose cluster is the complete graph over one detection per camera, and in
 * *n_other (may be NULL) those of any other shape; -1 / -1 if that call did not arm the hand-over (single-person
 * batches, DLT, more than 16 cameras or 16 persons per camera, a negative keypoint threshold).  Synchronises the device. */
int64_t snowtri_last_handover_persons(snowtri_ctx *ctx, int64_t *n_other);
/* Diagnostics of the streaming multi-person route, last call (its last segment): counts[0] = frames the association
 * kernel could not finish in its first launch (kept list larger than its LDS), counts[1] = frames with a candidate whose sum
 * was re-done with the exact arithmetic, counts[2] = frames left to k_frame_recompute.  All three are 0 on the reference's
 * workloads (tests assert it: a regression that sends every frame down a fall-back still passes parity, but not this);
 * -1 each if that call did not take the route.  Synchronises the device. */
int snowtri_last_stream_counts(snowtri_ctx *ctx, int64_t counts[3]);
/* The context's internal streams (the second stream of the multi-person split, the streams of the overlap mode) are
 * checked when they are created: the HIP runtime multiplexes a process's streams over a few hardware queues, and an
 * internal stream that shares the caller's queue runs one after the other with it.  A pair of one-thread kernels tells
 * (<= 300 us, once per stream; the first call that needs the stream synchronises it and the caller's); a stream that fails
 * is replaced, up to six candidates.  out[0] = probes run, out[1] = streams discarded, out[2] = verdict on the stream kept
 * last (1 side by side, 0 none of the candidates was, -1 no stream created yet or the probe could not run: a caller
 * stream under graph capture is never probed).  That synchronisation happens ONCE per context, in the call that creates
 * the internal stream; a caller stream the context meets later is probed only while it is idle (never waited for), and a
 * context runs at most 16 probes in its life.  No device work. */
int snowtri_ctx_stream_probes(const snowtri_ctx *ctx, int64_t out[3]);

#ifdef __cplusplus
}
#endif
#endif /* SNOWTRI_H */
