// snowtri.hip -- C ABI of libsnowtri.so (declared in include/snowtri.h) over the HIP kernels.
//
// Built for gfx950 only:  hipcc --offload-arch=gfx950 -O3 -std=c++17 -shared -fPIC snowtri.hip
// No torch types, no exceptions across the boundary; every entry point returns a snowtri_status.
#include "../../include/snowtri.h"

#include <hip/hip_runtime.h>
#include <hip/hip_ext.h>

#include <algorithm>
#include <atomic>
#include <chrono>
#include <thread>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <limits>
#include <map>
#include <mutex>
#include <new>
#include <string>
#include <vector>

#include "snowtri_fused.hpp"
#include "snowtri_lean.hpp"
#include "snowtri_cluster.hpp"
#include "snowtri_general.hpp"
#include "snowtri_assoc.hpp"
#include "snowtri_dlt_lean.hpp"
#include "snowtri_robust.hpp"
#include "snowtri_matched.hpp"
#include "snowtri_smooth.hpp"
#include "snowtri_blender.hpp"
#include "snowtri_undistort.hpp"
#include "snowtri_reproject.hpp"
#include "snowtri_assign.hpp"
#include "snowtri_seed.hpp"
#include "snowtri_refine.hpp"
#include "snowtri_pose.hpp"
#include "snowtri_pose_intr.hpp"
#include "snowtri_track.hpp"
#include "snowtri_fill.hpp"
#include "snowtri_despike.hpp"
#include "snowtri_kernels.hpp"

using namespace snowtri;

namespace {

thread_local std::string g_last_error;

#define HIP_TRY(expr)                                                                            \
    do {                                                                                         \
        hipError_t _e = (expr);                                                                  \
        if (_e != hipSuccess) {                                                                  \
            char _buf[512];                                                                      \
            snprintf(_buf, sizeof(_buf), "%s failed: %s (%s:%d)", #expr, hipGetErrorString(_e),  \
                     __FILE__, __LINE__);                                                        \
            g_last_error = _buf;                                                                 \
            return SNOWTRI_ERR_HIP;                                                              \
        }                                                                                        \
    } while (0)

// Every entry point runs on its context's device and leaves the caller's current device as it found it
// (one process may drive several GPUs, or torch may have selected another device for the thread).
struct DeviceGuard {
    int prev = -1;
    hipError_t err = hipSuccess;
    explicit DeviceGuard(int device) {
        err = hipGetDevice(&prev);
        if (err == hipSuccess && prev != device) err = hipSetDevice(device);
        else if (err != hipSuccess) prev = -1;
    }
    ~DeviceGuard() {
        int cur = -1;
        if (prev >= 0 && hipGetDevice(&cur) == hipSuccess && cur != prev) (void)hipSetDevice(prev);
    }
    DeviceGuard(const DeviceGuard &) = delete;
    DeviceGuard &operator=(const DeviceGuard &) = delete;
};
#define ENTER_DEVICE(device)              \
    DeviceGuard _device_guard(device);    \
    HIP_TRY(_device_guard.err)

// Is the caller's stream recording a hipGraph?  (A stream whose status cannot be read counts as capturing: whatever the question
// guards -- a query of the stream, a fork onto an internal one -- is then left undone.)
static bool stream_is_capturing(hipStream_t st) {
    hipStreamCaptureStatus cs = hipStreamCaptureStatusNone;
    if (hipStreamIsCapturing(st, &cs) != hipSuccess) {
        (void)hipGetLastError();
        return true;
    }
    return cs != hipStreamCaptureStatusNone;
}

struct Scratch {
    void *p = nullptr;
    size_t cap = 0;
    int ensure(size_t bytes) {
        if (bytes <= cap) return SNOWTRI_OK;
        if (p) {
            HIP_TRY(hipFree(p));
            p = nullptr;
            cap = 0;
        }
        size_t want = std::max(bytes, (size_t)1 << 20);
        HIP_TRY(hipMalloc(&p, want));
        cap = want;
        return SNOWTRI_OK;
    }
    void release() {
        if (p) (void)hipFree(p);
        p = nullptr;
        cap = 0;
    }
};

// Page-locked host staging for the small per-frame calls: one H2D and one D2H per call, both truly asynchronous
// (a pageable copy is staged and synchronised by the runtime, ~10-20 us each).
struct PinnedScratch {
    void *p = nullptr;
    void *dev = nullptr;   // the same memory as the device sees it (mapped: the small calls' kernels read / write it in place)
    size_t cap = 0;
    int ensure(size_t bytes) {
        if (bytes <= cap) return SNOWTRI_OK;
        if (p) {
            HIP_TRY(hipHostFree(p));
            p = dev = nullptr;
            cap = 0;
        }
        size_t want = std::max(bytes, (size_t)64 << 10);
        HIP_TRY(hipHostMalloc(&p, want, hipHostMallocMapped));
        HIP_TRY(hipHostGetDevicePointer(&dev, p, 0));
        std::memset(p, 0, want);   // (completion words are compared with a sequence number: never start from stale memory)
        cap = want;
        return SNOWTRI_OK;
    }
    void release() {
        if (p) (void)hipHostFree(p);
        p = dev = nullptr;
        cap = 0;
    }
};
constexpr size_t kPinnedMaxBytes = (size_t)4 << 20;   // larger host batches keep the direct copies
// The per-frame calls (main.py hands over 6 KB of keypoints and takes back 30 KB of candidates): below this size the kernels
// read their inputs from, and mirror their outputs into, the mapped page-locked buffers directly -- no copy engine in the chain
// (H2D + D2H were ~20 of the 39 us of a snowtri_triangulate call).
constexpr size_t kZeroCopyMaxBytes = (size_t)256 << 10;

int inv3(const double *m, double *o) {
    const double c00 = m[4] * m[8] - m[5] * m[7];
    const double c01 = m[5] * m[6] - m[3] * m[8];
    const double c02 = m[3] * m[7] - m[4] * m[6];
    const double det = m[0] * c00 + m[1] * c01 + m[2] * c02;
    if (det == 0.0 || !std::isfinite(det)) return 1;
    const double id = 1.0 / det;
    o[0] = c00 * id;
    o[1] = (m[2] * m[7] - m[1] * m[8]) * id;
    o[2] = (m[1] * m[5] - m[2] * m[4]) * id;
    o[3] = c01 * id;
    o[4] = (m[0] * m[8] - m[2] * m[6]) * id;
    o[5] = (m[2] * m[3] - m[0] * m[5]) * id;
    o[6] = c02 * id;
    o[7] = (m[1] * m[6] - m[0] * m[7]) * id;
    o[8] = (m[0] * m[4] - m[1] * m[3]) * id;
    return 0;
}

// K = [[fx, s, cx], [0, fy, cy], [0, 0, 1]] with fx, fy != 0: the pinhole part the lens model and the reprojection take apart
bool pinhole_K(const double *K) { return K[3] == 0.0 && K[6] == 0.0 && K[7] == 0.0 && K[8] == 1.0 && K[0] != 0.0 && K[4] != 0.0; }

constexpr int kTimingRing = 1024;
// ctx->d_counters: [0] singular pairs, [1] slow frames, [2] frame queue of k_frame_recompute, [6..9] slow / exact / slow
// (second pass) frame counts and the frame tickets of k_candidate_sums, [16 .. 32] the two hand-over list counters
// (snowtri_cluster.hpp: kHandComplete, kHandMembers -- 128 bytes apart)
constexpr int kHandCountersAt = 16, kCounterWords = 48, kTriangulateSingularAt = 40, kHostDoneCountAt = 42;   // [40]: singular pairs of the zero-copy snowtri_triangulate (self-resetting)

// Everything a fused call writes besides its outputs: the slabs of the fall-back routines, the hand-over lists and
// candidate sums of the multi-person path, the frame queue / list counters, the flags of a call that did not ask for
// them.  A context owns kMaxSets of them: set 0 is the caller's stream; the others carry an internal stream each, so that
// (a) the segments of ONE multi-person call alternate between two sets -- the latency-bound kernels of one segment
// (k_associate, the member lists) run beside the VALU-bound ones of the other -- and (b) in overlap mode
// (snowtri_ctx_set_overlap) consecutive calls run on different sets, i.e. the tail of one launch overlaps the ramp-up of
// the next without the caller managing streams.  Work on one set is ordered by its stream, so a set's scratch is never
// shared by two launches in flight.
struct StreamSet {
    Scratch work, desc, sums, misc;
    unsigned long long *d_counters = nullptr;   // kCounterWords
    hipStream_t stream = nullptr;               // internal stream (set 0 never has one: it is ordered by the caller's stream)
    hipEvent_t done = nullptr;                  // recorded behind the last launch the set received
    bool pending = false;                       // `done` has been recorded and not yet joined
};
constexpr int kMaxSets = 5;   // set 0 = the caller's stream; sets 1..4 carry an internal stream each
constexpr int kMaxOverlap = kMaxSets - 1;

// hipFuncAttributeMaxDynamicSharedMemorySize is a property of the FUNCTION (per device, process-wide) and the call SETS
// it: two contexts with different rigs in one process must not lower each other's limit.  One monotone
// cache per (device, kernel) for the whole process.
std::mutex g_lds_mutex;
std::map<std::pair<int, const void *>, int> g_lds_raised;
int raise_dynamic_lds(int device, const void *kern, int lds) {
    std::lock_guard<std::mutex> lock(g_lds_mutex);
    int &have = g_lds_raised[{device, kern}];
    if (have >= lds) return 0;
    if (hipFuncSetAttribute(kern, hipFuncAttributeMaxDynamicSharedMemorySize, lds) != hipSuccess) return 1;
    have = lds;
    return 0;
}

int grid_for(int64_t work_items, int per_block, int cap_blocks) {
    int64_t b = (work_items + per_block - 1) / per_block;
    return (int)std::max<int64_t>(1, std::min<int64_t>(b, cap_blocks));
}

}  // namespace

struct snowtri_ctx {
    int device = 0;
    int32_t C = 0, npairs = 0;
    int num_cus = 256;
    std::vector<double> hM, ht, hK;
    double *dLens = nullptr;  // [C][kLensStride], set by snowtri_ctx_set_distortion
    double *dProj = nullptr;  // [C][kProjStride] of snowtri_reproject[_cost]: R, t, the pinhole part of K; the lens once one is set
    std::vector<double> hProj;
    void *dBlenderTab = nullptr;          // 24 SmoothCoef of the last (fzr, dt) given to snowtri_blender_smooth
    std::vector<double> blender_key;      // that (fzr[72], dt)
    std::vector<int32_t> hpairs;
    double *dM = nullptr, *dt = nullptr, *dpairc = nullptr, *dP = nullptr;
    int32_t *dpairs = nullptr;
    StreamSet sets[kMaxSets];
    StreamSet *cur = &sets[0];        // the set the launch in progress writes to (set 0 between fused calls)
    StreamSet *last_set = &sets[0];   // the set of the last fused call's last segment (diagnostics read its counters)
    // set 0 under the names every other entry point uses
    unsigned long long *&d_counters = sets[0].d_counters;  // [0] singular pairs, [1] slow frames, [2..] spare
    Scratch &work = sets[0].work, &misc = sets[0].misc;
    Scratch &desc = sets[0].desc;             // cluster descriptors handed from k_frame_recompute / k_associate to k_cluster_fuse
    Scratch &sums = sets[0].sums;             // candidate sums of k_candidate_sums [frames][Kc] + the frames k_associate left behind
    Scratch in, out, aux;
    double *pose_ws = nullptr;                // workspace of snowtri_refine_cameras (pose_ws_doubles(C)): allocated by the first call, by no later one
    double *pose_kws = nullptr;               // ... and of snowtri_refine_cameras_k (pose_kws_doubles(C)), with the context's K in it: likewise
    Scratch track;                            // centres [F][Pout_max][4] fp64 of snowtri_track_persons (k_track_centres -> k_track_chain)
    hipEvent_t track_ev[3] = {nullptr, nullptr, nullptr};   // with timing on: before k_track_centres | between | behind k_track_chain
    bool track_ev_valid = false;
    PinnedScratch pin_in, pin_out;            // host staging of the per-frame and fused calls (Staging)
    PinnedScratch pin_done;                   // the completion word of the small host calls (HostDone, snowtri_kernels.hpp)
    unsigned long long done_seq = 0;
    std::vector<uint32_t> flags_host;         // the flags of a SNOWTRI_HOST fused call that passed no out_flags (it only grows)
    Scratch cand;                             // candidates of the last SNOWTRI_HOST snowtri_triangulate call (device-resident hand-over)
    int64_t cand_token = 0, cand_F = 0, cand_Kc = 0, cand_J = 0;   // token 0: none
    const double *cand_xyz = nullptr, *cand_ks = nullptr;          // ... where that call left them in `cand`
    const uint8_t *cand_keep = nullptr;
    int overlap = 1;                  // snowtri_ctx_set_overlap: device calls rotate over this many sets (1 = the caller's stream)
    int64_t call_index = 0;
    hipEvent_t ev_fork = nullptr;     // the caller's stream at the time of a call / a split: the internal streams wait for it
    int split_segments = 2;           // one multi-person call is cut into >= this many segments on two sets (1: no split)
    bool split_forced = false;        // SNOWTRI_SPLIT_SEGMENTS given: also batches that would not fill the chip twice
    // Internal streams are only worth having on hardware queues of their own (k_probe_wait, snowtri_kernels.hpp):
    PinnedScratch pin_probe;
    int64_t probes = 0, probe_replaced = 0;   // snowtri_ctx_stream_probes
    int probe_verdict = -1;                   // of the stream kept last: 1 side by side, 0 none of the candidates was, -1 no probe yet
    hipStream_t split_beside[4];              // the caller streams sets[1].stream has been probed against (a ring of the last four)
    int n_split_beside = 0;
    bool split_knows(hipStream_t caller) const {
        for (int i = 0; i < std::min(n_split_beside, 4); ++i)
            if (split_beside[i] == caller) return true;
        return false;
    }
    // The probe SYNCHRONISES both streams (<= 300 us).  Policy: when a context CREATES its internal stream -- its
    // first split call -- the caller's stream is waited for once (documented in include/snowtri.h); a caller stream the
    // context meets LATER is probed only while it is idle (`only_if_idle`: a stream with work in flight is never waited for
    // -- the internal stream is kept, and the question is asked again at a later call); and a context probes at most
    // kMaxProbes times in its life: a caller that rotates many streams, or a box whose queues never come out side by side,
    // keeps what it has instead of paying a synchronisation per call.
    static constexpr int64_t kMaxProbes = 16;
    int probe_side_by_side(hipStream_t a, hipStream_t b, bool only_if_idle = false) {   // 1 / 0, -1: not probed
        hipStreamCaptureStatus cs = hipStreamCaptureStatusNone;   // never put the probe into a graph under capture
        if (hipStreamIsCapturing(a, &cs) != hipSuccess || cs != hipStreamCaptureStatusNone) return -1;
        if (probes >= kMaxProbes) return -1;
        if (only_if_idle && hipStreamQuery(a) != hipSuccess) {
            (void)hipGetLastError();
            return -2;   // busy: ask again later
        }
        if (pin_probe.ensure(64)) return -1;
        volatile unsigned int *w = (volatile unsigned int *)pin_probe.p;
        w[0] = 0u;
        w[1] = 2u;
        ++probes;
        hipLaunchKernelGGL(k_probe_wait, dim3(1), dim3(1), 0, a, (volatile unsigned int *)pin_probe.dev, 30000ull);   // <= 300 us
        hipLaunchKernelGGL(k_probe_set, dim3(1), dim3(1), 0, b, (volatile unsigned int *)pin_probe.dev);
        if (hipStreamSynchronize(a) != hipSuccess || hipStreamSynchronize(b) != hipSuccess) return -1;
        return w[1] == 1u ? 1 : 0;
    }
    // a new non-blocking stream that runs beside `caller` (when `with_caller`) and beside the internal streams of the other
    // sets; up to 6 candidates (each rejected one stays alive until the end, so that the next lands on another queue)
    int fresh_stream(hipStream_t *out, int k, bool with_caller, hipStream_t caller) {
        hipStream_t rejected[6];
        int nrej = 0, rc = 0;
        for (int attempt = 0; attempt < 6 && !rc; ++attempt) {
            hipStream_t s = nullptr;
            if (hipStreamCreateWithFlags(&s, hipStreamNonBlocking) != hipSuccess) {
                rc = 1;
                break;
            }
            int ok = with_caller ? probe_side_by_side(caller, s) : 1;
            for (int j = 0; j < kMaxSets && ok == 1; ++j)
                if (j != k && sets[j].stream) ok = probe_side_by_side(sets[j].stream, s);
            if (ok < 0) {   // the probe itself failed (a caller stream that cannot be synchronised now, e.g. under capture):
                (void)hipGetLastError();   // keep the stream unprobed rather than fail the call
                probe_verdict = -1;
                *out = s;
                break;
            }
            probe_verdict = ok == 1 ? 1 : 0;
            if (ok == 1 || attempt == 5) {
                *out = s;
                break;
            }
            rejected[nrej++] = s;
            ++probe_replaced;
        }
        for (int i = 0; i < nrej; ++i) (void)hipStreamDestroy(rejected[i]);
        return rc;
    }
    int ensure_set(int k, bool with_caller = false, hipStream_t caller = nullptr) {   // counters, stream and event of set k
        StreamSet &S = sets[k];
        if (!S.d_counters) {
            if (hipMalloc(&S.d_counters, sizeof(unsigned long long) * kCounterWords) != hipSuccess) return 1;
            if (hipMemset(S.d_counters, 0, sizeof(unsigned long long) * kCounterWords) != hipSuccess) return 1;
        }
        if (S.stream && with_caller && !split_knows(caller)) {
            // the split of a call that arrives on another stream than the last one did: still side by side?
            const int ok = probe_side_by_side(caller, S.stream, true);
            if (ok == -2) with_caller = false;     // the caller's stream is busy: keep the stream, probe at a later call
            if (ok < 0) (void)hipGetLastError();   // unprobed: keep the stream
            if (ok == 0) {
                if (hipStreamSynchronize(S.stream) != hipSuccess) return 1;
                hipStream_t old = S.stream;
                S.stream = nullptr;
                const int rc = fresh_stream(&S.stream, k, true, caller);
                (void)hipStreamDestroy(old);
                ++probe_replaced;
                n_split_beside = 0;
                if (rc) return 1;
            } else if (ok != -2)
                probe_verdict = ok == 1 ? 1 : -1;
        } else if (!S.stream && fresh_stream(&S.stream, k, with_caller, caller))
            return 1;
        if (with_caller && !split_knows(caller)) split_beside[n_split_beside++ & 3] = caller;
        if (!S.done && hipEventCreateWithFlags(&S.done, hipEventDisableTiming) != hipSuccess) return 1;
        if (!ev_fork && hipEventCreateWithFlags(&ev_fork, hipEventDisableTiming) != hipSuccess) return 1;
        return 0;
    }
    // measurement
    bool timing = false;
    bool timing_attach = false;   // snowtri_set_timing(ctx, 2): single-kernel launches carry their ring events themselves
    bool ev_attached = false;     // the last launcher did (fused_dispatch then records no end event of its own)
    hipEvent_t ev[4] = {nullptr, nullptr, nullptr, nullptr};
    bool ev_valid = false;
    hipStream_t ev_stream = nullptr;
    std::vector<hipEvent_t> ev_ring;  // 2 events per recorded fused call (begin, end), kTimingRing calls deep
    int64_t ev_count = 0;             // fused calls recorded since the last snowtri_timing_collect
    int64_t last_slow_frames = 0;
    bool last_handover = false;  // the last fused call went through k_frame_recompute with the cluster hand-over armed
    // test knobs (environment, read at creation; snowtri_ctx_overrides names the ones that are set)
    int general_mode = 0;        // SNOWTRI_GENERAL_MODE: 0 auto, 1 force the spill kernel, 2 force the recompute kernel
    int lean_mode = 1;           // SNOWTRI_LEAN_MODE: 0 keeps float32-output batches (and DLT batches) on k_fused_single
    int lean_coop = 1;           // SNOWTRI_LEAN_COOP: 0 keeps small launches on k_fused_lean
    int sumless_mode = 1;        // SNOWTRI_SUMLESS_MODE: 0 keeps the candidate pass for single-detection batches on the streaming route
    int handover_mode = 1;       // SNOWTRI_HANDOVER_MODE: 1 streaming association (k_candidate_sums / k_associate / k_cluster_fuse), 2 hand-over
                                 // from inside k_frame_recompute, 0 the whole multi-person path inside k_frame_recompute
    int handover_seg_frames = 0; // SNOWTRI_HANDOVER_SEG_FRAMES: short segments of the streaming route
    int sums_threads = 0, sums_lds_kb = 0;   // SNOWTRI_SUMS_THREADS / _LDS_KB: workgroup shape of k_candidate_sums (0: automatic)
    int lean_tiles_per_wave = 0; // SNOWTRI_LEAN_TILES_PER_WAVE
    int debug = 0;               // SNOWTRI_DEBUG: launch shapes on stderr
    std::string overrides;
    // method = SNOWTRI_DLT_ROBUST through the fused call (snowtri_ctx_set_robust)
    double robust_threshold_px = 6.0;
    int32_t robust_max_drops = 1;
    static constexpr int assoc_wg_per_cu = 4 * kAssocWaves, lean_wg_per_cu = 2, lean_scratch_mb = 256;   // (settled by measurement: EXPERIMENTS.md)
    struct OccCache {
        size_t lds = 0;
        int per_cu = -1;
    } recompute_occ[8];   // resident workgroups per CU of the k_frame_recompute instantiations (queried once per LDS size)
    int raise_lds(const void *kern, int lds) { return raise_dynamic_lds(device, kern, lds); }   // once per (device, kernel, size), process-wide
    bool last_stream = false;        // the last fused call went through the streaming association (snowtri_last_stream_counts)
    // names of the kernels the last fused call launched (snowtri_last_kernel_names): a pointer to a string that lives as
    // long as the library (one per template instantiation) or to `names_buf`, rebuilt only when the route changes
    const char *last_kernels = "";
    std::string names_buf;
    long long names_key = -1;
    Rig rig() const { return Rig{dM, dt, dpairs, dpairc, dP, C, npairs}; }
};

namespace {

static inline void cpu_relax() {   // spin-wait hint of the host CPU
#if defined(__x86_64__) || defined(__i386__)
    __builtin_ia32_pause();
#elif defined(__aarch64__)
    asm volatile("yield" ::: "memory");
#else
    std::this_thread::yield();
#endif
}

// The host arrays of one call staged through two Scratch buffers: `ins` holds what the kernels only read, `outs` what they
// write.  The entry point declares each array by the address of its own device-pointer variable, which holds the caller's
// pointer until begin() puts the staged address there (a null pointer declares nothing and stays null); begin() goes before
// the first launch, end() behind the last.  Every buffer is sized before any base pointer is taken -- ensure() frees and
// reallocates -- and the layout is the declared order, every array on a 16-byte boundary (the uint4 kernels).  With
// host == false (a SNOWTRI_DEVICE call) nothing happens at all: the caller's pointers pass through and the buffers, which may
// hold a host caller's data, are not touched.
//
// The arrays travel by one of three routes.  kDirect: one hipMemcpyAsync per array each way, between the caller's arrays and
// the scratch -- what every entry point gets that names no other.  The per-frame and fused calls pass their context and the
// furthest route they allow, and begin() chooses by the declared totals.  kPinned, while inputs and outputs are each within
// kPinnedMaxBytes: the arrays are memcpy'd into ctx->pin_in and uploaded in one copy, the output block comes back in one copy
// into ctx->pin_out and is memcpy'd out (a pageable copy is staged and synchronised by the runtime, ~10-20 us each).  kMapped,
// while inputs plus outputs are within kZeroCopyMaxBytes: no copy engine at all -- the staged inputs ARE ctx->pin_in as the
// device sees it, mapped() gives the twin of a staged output in ctx->pin_out for the kernels to write as well as (or instead
// of) the scratch, and `done` is the armed completion word a single launch may signal (HostDone, snowtri_kernels.hpp).
struct Staging {
    enum Kind { kIn, kOut, kInOut };
    enum Route { kDirect, kPinned, kMapped };
    struct Entry {
        void *var, *host, *dev;   // the entry point's variable, the caller's array, its staged copy
        size_t bytes, off;
        Kind kind;
    };
    static constexpr int kMaxArrays = 16;
    static constexpr size_t kSlack = 256;   // behind each block
    Scratch &ins, &outs;
    const bool host;
    const hipStream_t st;
    snowtri_ctx *const ctx;
    Route route;   // until begin(): the furthest route allowed; then: the route taken
    HostDone done{nullptr, nullptr, 0ull};
    Entry e[kMaxArrays];
    int n = 0;
    size_t in_bytes = 0, out_bytes = 0;

    Staging(Scratch &ins_, Scratch &outs_, bool host_, hipStream_t st_, snowtri_ctx *ctx_ = nullptr, Route allow = kDirect)
        : ins(ins_), outs(outs_), host(host_), st(st_), ctx(ctx_), route(host_ && ctx_ ? allow : kDirect) {}
    template <typename T> void in(const T **var, size_t bytes) { add(var, (void *)*var, bytes, kIn); }
    template <typename T> void out(T **var, size_t bytes) { add(var, (void *)*var, bytes, kOut); }
    template <typename T> void inout(T **var, size_t bytes) { add(var, (void *)*var, bytes, kInOut); }
    void add(void *var, void *host_array, size_t bytes, Kind kind) {
        if (!host || !host_array) return;
        if (kind == kInOut) route = kDirect;   // (no entry point on the page-locked routes has one)
        size_t &total = kind == kIn ? in_bytes : out_bytes;
        if (n < kMaxArrays) e[n] = Entry{var, host_array, nullptr, bytes, total, kind};
        ++n;
        total += (bytes + 15) & ~(size_t)15;
    }
    int begin() {
        if (n > kMaxArrays) {
            g_last_error = "Staging: more arrays than kMaxArrays";
            return SNOWTRI_ERR_BAD_ARG;
        }
        if (in_bytes > kPinnedMaxBytes || out_bytes > kPinnedMaxBytes) route = kDirect;   // larger host batches keep the direct copies
        else if (route == kMapped && in_bytes + out_bytes > kZeroCopyMaxBytes) route = kPinned;
        if (int rc = in_bytes ? ins.ensure(in_bytes + kSlack) : 0) return rc;
        if (int rc = out_bytes ? outs.ensure(out_bytes + kSlack) : 0) return rc;
        if (int rc = (route != kDirect && in_bytes) ? ctx->pin_in.ensure(in_bytes + kSlack) : 0) return rc;
        if (int rc = (route != kDirect && out_bytes) ? ctx->pin_out.ensure(out_bytes + kSlack) : 0) return rc;
        if (route == kMapped) {   // arm the completion word
            if (int rc = ctx->pin_done.ensure(64)) return rc;
            done = HostDone{(unsigned int *)(ctx->d_counters + kHostDoneCountAt), (unsigned long long *)ctx->pin_done.dev, ++ctx->done_seq};
        }
        for (int i = 0; i < n; i++) {
            e[i].dev = (char *)(e[i].kind != kIn ? outs.p : route == kMapped ? ctx->pin_in.dev : ins.p) + e[i].off;
            if (e[i].kind != kOut && e[i].bytes) {
                if (route == kDirect) HIP_TRY(hipMemcpyAsync(e[i].dev, e[i].host, e[i].bytes, hipMemcpyHostToDevice, st));
                else std::memcpy((char *)ctx->pin_in.p + e[i].off, e[i].host, e[i].bytes);
            }
            std::memcpy(e[i].var, &e[i].dev, sizeof(void *));   // (the variable is a pointer to some T: all of one representation)
        }
        if (route == kPinned && in_bytes) HIP_TRY(hipMemcpyAsync(ins.p, ctx->pin_in.p, in_bytes, hipMemcpyHostToDevice, st));   // one staged upload
        return SNOWTRI_OK;
    }
    // the twin of a staged output in mapped host memory as the device sees it; null unless the mapped route was taken
    template <typename T> T *mapped(T *dev) const {
        return route == kMapped ? (T *)((char *)ctx->pin_out.dev + ((char *)dev - (char *)outs.p)) : nullptr;
    }
    // zeros in the whole output block (not on the mapped route: its kernels write every byte of both copies)
    int clear_outputs() {
        if (out_bytes && route != kMapped) HIP_TRY(hipMemsetAsync(outs.p, 0, out_bytes, st));
        return SNOWTRI_OK;
    }
    // The downloads of the declared outputs, then the call's one synchronisation.  signalled: the launch signals `done` (its
    // outputs are in mapped host memory by then), so a mapped call spins on the word instead of sleeping on the runtime's interrupt.
    int end(bool signalled = false) {
        if (!host) return SNOWTRI_OK;
        if (route == kPinned && out_bytes) HIP_TRY(hipMemcpyAsync(ctx->pin_out.p, outs.p, out_bytes, hipMemcpyDeviceToHost, st));   // one staged download
        for (int i = 0; i < n && route == kDirect; i++)
            if (e[i].kind != kIn && e[i].bytes) HIP_TRY(hipMemcpyAsync(e[i].host, e[i].dev, e[i].bytes, hipMemcpyDeviceToHost, st));
        if (route == kMapped && signalled) {
            if (int rc = wait_done()) return rc;
        } else {
            HIP_TRY(hipStreamSynchronize(st));
        }
        for (int i = 0; i < n && route != kDirect; i++)
            if (e[i].kind != kIn && e[i].bytes) std::memcpy(e[i].host, (const char *)ctx->pin_out.p + e[i].off, e[i].bytes);
        return SNOWTRI_OK;
    }
    // spin on the completion word; hipStreamSynchronize stays as the fall-back after 50 ms of spinning
    int wait_done() {
        const volatile unsigned long long *w = (const volatile unsigned long long *)ctx->pin_done.p;
        const auto t0 = std::chrono::steady_clock::now();
        for (unsigned spins = 0; *w != done.seq; spins++) {
            cpu_relax();
            if ((spins & 0xfff) == 0xfff && std::chrono::steady_clock::now() - t0 > std::chrono::milliseconds(50)) {
                HIP_TRY(hipStreamSynchronize(st));   // (a failed launch never writes the word: the runtime reports it here)
                if (*w != done.seq) {
                    g_last_error = "a per-frame kernel finished without its completion word";
                    return SNOWTRI_ERR_HIP;
                }
                break;
            }
        }
        std::atomic_thread_fence(std::memory_order_acquire);
        return SNOWTRI_OK;
    }
};

}  // namespace

extern "C" {

int snowtri_version(void) { return SNOWTRI_VERSION; }

const char *snowtri_status_string(int s) {
    switch (s) {
        case SNOWTRI_OK: return "ok";
        case SNOWTRI_ERR_BAD_ARG: return "bad argument";
        case SNOWTRI_ERR_BAD_INDEX: return "center_point_index / keypoint_num out of range";
        case SNOWTRI_ERR_HIP: return "HIP runtime error";
        case SNOWTRI_ERR_SINGULAR: return "singular ray pair (parallel rays)";
        case SNOWTRI_ERR_OVERFLOW: return "more output persons than Pout_max";
        case SNOWTRI_ERR_NO_DEVICE: return "no HIP device";
        default: return "unknown status";
    }
}

const char *snowtri_last_error(void) { return g_last_error.c_str(); }

const char *snowtri_build_info(void) {
    // what this binary was compiled as: the production library reports no variant at all
    static const std::string info = [] {
        std::string v;
        auto add = [&](const char *name) { v += (v.empty() ? "" : ",") + std::string(name); };
        (void)add;
#ifdef SNOWTRI_DEBUG_BOUNDS
        add("SNOWTRI_DEBUG_BOUNDS");
#endif
#ifdef SNOWTRI_TEST_KNOBS
        add("SNOWTRI_TEST_KNOBS");
#endif
#ifdef SNOWTRI_DEV_MIN
        add("SNOWTRI_DEV_MIN");
#endif
#ifdef SNOWTRI_DEV_EXPERIMENTS
        add("SNOWTRI_DEV_EXPERIMENTS");
#endif
#ifdef SNOWTRI_POSE_PER_RECORD
        add("SNOWTRI_POSE_PER_RECORD");
#endif
#ifdef SNOWTRI_LEAN_TRACE
        add("SNOWTRI_LEAN_TRACE");
#endif
#ifdef SNOWTRI_SUMS_TRACE
        add("SNOWTRI_SUMS_TRACE");
#endif
#ifdef SNOWTRI_ASSOC_TRACE
        add("SNOWTRI_ASSOC_TRACE");
#endif
        return "version=" + std::to_string(SNOWTRI_VERSION) + ";arch=gfx950;variants=" + v;
    }();
    return info.c_str();
}

const char *snowtri_ctx_overrides(const snowtri_ctx *ctx) { return ctx ? ctx->overrides.c_str() : ""; }

int snowtri_device_count(void) {
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess) return 0;
    return n;
}

int snowtri_ctx_create(int32_t C, const double *K, const double *R, const double *t, int device,
                       snowtri_ctx **out) {
    if (!out || C < 0 || (C > 0 && (!K || !R || !t))) return SNOWTRI_ERR_BAD_ARG;
    *out = nullptr;
    if (snowtri_device_count() <= 0) return SNOWTRI_ERR_NO_DEVICE;
    snowtri_ctx *ctx = new (std::nothrow) snowtri_ctx();
    if (!ctx) return SNOWTRI_ERR_BAD_ARG;
    ctx->device = device;
    ctx->C = C;
    // Test knobs (include/snowtri.h lists them) exist ONLY in a -DSNOWTRI_TEST_KNOBS build (libsnowtri_dbg.so, which the tests that
    // force a route load): the production library reads no environment.  There they are read HERE, once -- nothing on the launch
    // path calls getenv -- and every one that is set is named by snowtri_ctx_overrides().
#ifdef SNOWTRI_TEST_KNOBS
    auto knob = [&](const char *name, int *field, int lo) {
        if (const char *e = getenv(name)) {
            *field = std::max(lo, atoi(e));
            ctx->overrides += (ctx->overrides.empty() ? "" : ",") + std::string(name) + "=" + std::to_string(*field);
        }
    };
    knob("SNOWTRI_GENERAL_MODE", &ctx->general_mode, 0);
    knob("SNOWTRI_LEAN_MODE", &ctx->lean_mode, 0);
    knob("SNOWTRI_LEAN_COOP", &ctx->lean_coop, 0);
    knob("SNOWTRI_SUMLESS_MODE", &ctx->sumless_mode, 0);
    knob("SNOWTRI_HANDOVER_MODE", &ctx->handover_mode, 0);
    knob("SNOWTRI_HANDOVER_SEG_FRAMES", &ctx->handover_seg_frames, 1);
    knob("SNOWTRI_SPLIT_SEGMENTS", &ctx->split_segments, 1);
    ctx->split_forced = getenv("SNOWTRI_SPLIT_SEGMENTS") != nullptr && ctx->split_segments >= 2;
    knob("SNOWTRI_SUMS_THREADS", &ctx->sums_threads, 0);
    knob("SNOWTRI_SUMS_LDS_KB", &ctx->sums_lds_kb, 0);
    knob("SNOWTRI_LEAN_TILES_PER_WAVE", &ctx->lean_tiles_per_wave, 1);
    knob("SNOWTRI_DEBUG", &ctx->debug, 0);
#endif
    ctx->hM.resize((size_t)C * 9);
    ctx->ht.assign(t, t + (size_t)C * 3);
    ctx->hK.assign(K, K + (size_t)C * 9);
    for (int c = 0; c < C; c++) {
        double Ki[9];
        if (inv3(K + 9 * c, Ki)) {  // np.linalg.inv(K) raises on a singular K (camera.py:242)
            delete ctx;
            return SNOWTRI_ERR_SINGULAR;
        }
        const double *Rc = R + 9 * c;
        for (int i = 0; i < 3; i++)
            for (int j = 0; j < 3; j++)
                ctx->hM[9 * c + 3 * i + j] = Rc[3 * i] * Ki[j] + Rc[3 * i + 1] * Ki[3 + j] + Rc[3 * i + 2] * Ki[6 + j];
    }
    for (int mc = 0; mc < C - 1; mc++)  // triangulation.py:56-58 loop order
        for (int sc = mc + 1; sc < C; sc++) {
            ctx->hpairs.push_back(mc);
            ctx->hpairs.push_back(sc);
        }
    ctx->npairs = (int32_t)(ctx->hpairs.size() / 2);
    std::vector<double> hpairc((size_t)ctx->npairs * 6);
    for (int q = 0; q < ctx->npairs; q++) {
        const double *tm = &ctx->ht[3 * ctx->hpairs[2 * q]], *ts = &ctx->ht[3 * ctx->hpairs[2 * q + 1]];
        for (int i = 0; i < 3; i++) {
            hpairc[6 * q + i] = ts[i] - tm[i];
            hpairc[6 * q + 3 + i] = tm[i] + ts[i];
        }
    }
    auto fail = [&](int rc) {
        snowtri_ctx_destroy(ctx);
        return rc;
    };
#define CTX_TRY(expr)                                         \
    do {                                                      \
        if ((expr) != hipSuccess) {                           \
            g_last_error = std::string(#expr) + " failed";    \
            return fail(SNOWTRI_ERR_HIP);                     \
        }                                                     \
    } while (0)
    DeviceGuard _device_guard(device);
    CTX_TRY(_device_guard.err);
    hipDeviceProp_t prop;
    CTX_TRY(hipGetDeviceProperties(&prop, device));
    ctx->num_cus = prop.multiProcessorCount > 0 ? prop.multiProcessorCount : 256;
    CTX_TRY(hipMalloc(&ctx->dM, sizeof(double) * std::max<size_t>(9, ctx->hM.size())));
    CTX_TRY(hipMalloc(&ctx->dt, sizeof(double) * std::max<size_t>(3, ctx->ht.size())));
    CTX_TRY(hipMalloc(&ctx->dpairs, sizeof(int32_t) * std::max<size_t>(2, ctx->hpairs.size())));
    CTX_TRY(hipMalloc(&ctx->d_counters, sizeof(unsigned long long) * kCounterWords));
    CTX_TRY(hipMalloc(&ctx->dpairc, sizeof(double) * std::max<size_t>(6, hpairc.size())));
    {   // The DLT method solves in the rig's own frame (include/snowtri.h, SNOWTRI_DLT): centre = the mean of the camera centres
        // (summed in camera order), scale = max |t_c - centre| over cameras and axes (1 when that is 0), and the frame -> pixel
        // matrices P_c = K_c [R_c^T | -R_c^T (t_c - centre) / scale].  A^T A squares the translation column f |t|: formed in world
        // coordinates its fp64 error reaches metres for a millimetre rig in site coordinates.
        // The four doubles (centre, scale) follow P in the same buffer: the kernels keep them in LDS beside P.
        std::vector<double> hP((size_t)std::max(1, C) * 12 + kDltFrame, 0.0);
        double *fc = hP.data() + (size_t)12 * C, &fs = hP[(size_t)12 * C + 3];
        for (int i = 0; i < 3; i++) {
            double sum = 0.0;
            for (int c = 0; c < C; c++) sum += t[3 * c + i];
            fc[i] = C > 0 ? sum / (double)C : 0.0;
        }
        double ext = 0.0;
        for (int c = 0; c < C; c++)
            for (int i = 0; i < 3; i++) ext = std::max(ext, std::fabs(t[3 * c + i] - fc[i]));
        fs = ext > 0.0 ? ext : 1.0;   // (a NaN centre: 1)
        for (int c = 0; c < C; c++) {
            const double *Kc = K + 9 * c, *Rc = R + 9 * c;
            const double tc[3] = {(t[3 * c] - fc[0]) / fs, (t[3 * c + 1] - fc[1]) / fs, (t[3 * c + 2] - fc[2]) / fs};
            double Rt[12];  // [R^T | -R^T (t - centre) / scale]
            for (int i = 0; i < 3; i++) {
                for (int j = 0; j < 3; j++) Rt[4 * i + j] = Rc[3 * j + i];
                Rt[4 * i + 3] = -(Rc[0 + i] * tc[0] + Rc[3 + i] * tc[1] + Rc[6 + i] * tc[2]);
            }
            for (int i = 0; i < 3; i++)
                for (int j = 0; j < 4; j++)
                    hP[12 * c + 4 * i + j] = Kc[3 * i] * Rt[j] + Kc[3 * i + 1] * Rt[4 + j] + Kc[3 * i + 2] * Rt[8 + j];
        }
        CTX_TRY(hipMalloc(&ctx->dP, sizeof(double) * hP.size()));
        CTX_TRY(hipMemcpy(ctx->dP, hP.data(), sizeof(double) * hP.size(), hipMemcpyHostToDevice));
    }
    ctx->hProj.assign((size_t)std::max(1, C) * kProjStride, 0.0);
    for (int c = 0; c < C; c++) {   // (whether K has the form the reprojection needs is the reprojection's question: checked there)
        double *q = &ctx->hProj[(size_t)c * kProjStride];
        std::memcpy(q, R + 9 * c, sizeof(double) * 9);
        std::memcpy(q + 9, t + 3 * c, sizeof(double) * 3);
        const double *Kc = K + 9 * c;
        q[12] = Kc[0]; q[13] = Kc[1]; q[14] = Kc[2]; q[15] = Kc[4]; q[16] = Kc[5];
    }
    CTX_TRY(hipMalloc(&ctx->dProj, sizeof(double) * ctx->hProj.size()));
    CTX_TRY(hipMemcpy(ctx->dProj, ctx->hProj.data(), sizeof(double) * ctx->hProj.size(), hipMemcpyHostToDevice));
    if (ctx->npairs > 0)
        CTX_TRY(hipMemcpy(ctx->dpairc, hpairc.data(), sizeof(double) * hpairc.size(), hipMemcpyHostToDevice));
    if (C > 0) {
        CTX_TRY(hipMemcpy(ctx->dM, ctx->hM.data(), sizeof(double) * ctx->hM.size(), hipMemcpyHostToDevice));
        CTX_TRY(hipMemcpy(ctx->dt, ctx->ht.data(), sizeof(double) * ctx->ht.size(), hipMemcpyHostToDevice));
    }
    if (ctx->npairs > 0)
        CTX_TRY(hipMemcpy(ctx->dpairs, ctx->hpairs.data(), sizeof(int32_t) * ctx->hpairs.size(), hipMemcpyHostToDevice));
    CTX_TRY(hipMemset(ctx->d_counters, 0, sizeof(unsigned long long) * kCounterWords));
    for (auto &e : ctx->ev) CTX_TRY(hipEventCreate(&e));
#undef CTX_TRY
    *out = ctx;
    return SNOWTRI_OK;
}

int snowtri_ctx_destroy(snowtri_ctx *ctx) {
    if (!ctx) return SNOWTRI_OK;
    DeviceGuard _device_guard(ctx->device);
    (void)hipDeviceSynchronize();
    if (ctx->dM) (void)hipFree(ctx->dM);
    if (ctx->dt) (void)hipFree(ctx->dt);
    if (ctx->dpairs) (void)hipFree(ctx->dpairs);
    if (ctx->dpairc) (void)hipFree(ctx->dpairc);
    if (ctx->dP) (void)hipFree(ctx->dP);
    if (ctx->dLens) (void)hipFree(ctx->dLens);
    if (ctx->dProj) (void)hipFree(ctx->dProj);
    if (ctx->pose_ws) (void)hipFree(ctx->pose_ws);
    if (ctx->pose_kws) (void)hipFree(ctx->pose_kws);
    if (ctx->dBlenderTab) (void)hipFree(ctx->dBlenderTab);
    for (auto &S : ctx->sets) {
        if (S.d_counters) (void)hipFree(S.d_counters);
        S.work.release();
        S.misc.release();
        S.desc.release();
        S.sums.release();
        if (S.stream) (void)hipStreamDestroy(S.stream);
        if (S.done) (void)hipEventDestroy(S.done);
    }
    if (ctx->ev_fork) (void)hipEventDestroy(ctx->ev_fork);
    ctx->in.release();
    ctx->out.release();
    ctx->aux.release();
    ctx->track.release();
    for (auto &e : ctx->track_ev)
        if (e) (void)hipEventDestroy(e);
    ctx->cand.release();
    ctx->pin_done.release();
    ctx->pin_probe.release();
    ctx->pin_in.release();
    ctx->pin_out.release();
    for (auto &e : ctx->ev)
        if (e) (void)hipEventDestroy(e);
    for (auto &e : ctx->ev_ring)
        if (e) (void)hipEventDestroy(e);
    delete ctx;
    return SNOWTRI_OK;
}

int snowtri_ctx_num_cameras(const snowtri_ctx *ctx) { return ctx ? ctx->C : -1; }

int snowtri_ctx_ray_matrices(const snowtri_ctx *ctx, double *M_out) {
    if (!ctx || !M_out) return SNOWTRI_ERR_BAD_ARG;
    std::memcpy(M_out, ctx->hM.data(), sizeof(double) * ctx->hM.size());
    return SNOWTRI_OK;
}

int snowtri_ctx_synchronize(snowtri_ctx *ctx) {
    if (!ctx) return SNOWTRI_ERR_BAD_ARG;
    ENTER_DEVICE(ctx->device);
    HIP_TRY(hipDeviceSynchronize());
    return SNOWTRI_OK;
}

int snowtri_ctx_set_overlap(snowtri_ctx *ctx, int n_streams) {
    if (!ctx || n_streams < 1 || n_streams > kMaxOverlap) return SNOWTRI_ERR_BAD_ARG;
    ENTER_DEVICE(ctx->device);
    for (auto &S : ctx->sets)   // calls still in flight on the internal streams finish under the old mode
        if (S.pending) {
            HIP_TRY(hipStreamSynchronize(S.stream));
            S.pending = false;
        }
    ctx->overlap = n_streams;
    ctx->call_index = 0;
    return SNOWTRI_OK;
}

int snowtri_ctx_set_split(snowtri_ctx *ctx, int segments) {
    if (!ctx || segments < 0 || segments > 64) return SNOWTRI_ERR_BAD_ARG;
    ctx->split_segments = segments == 0 ? 2 : segments;
    ctx->split_forced = segments >= 2;
    return SNOWTRI_OK;
}

int snowtri_ctx_set_robust(snowtri_ctx *ctx, double reproj_threshold_px, int32_t max_drops) {
    if (!ctx) return SNOWTRI_ERR_BAD_ARG;
    if (!(reproj_threshold_px >= 0.0)) {   // (negative or NaN; +inf is allowed: nothing is ever dropped)
        g_last_error = "reproj_threshold_px must be >= 0 (+inf allowed), not negative or NaN";
        return SNOWTRI_ERR_BAD_ARG;
    }
    if (max_drops < 0 || max_drops > kRobustMaxDrops) {
        g_last_error = "max_drops must be in [0, 6]";
        return SNOWTRI_ERR_BAD_ARG;
    }
    ctx->robust_threshold_px = reproj_threshold_px;
    ctx->robust_max_drops = max_drops;
    return SNOWTRI_OK;
}

int snowtri_ctx_join(snowtri_ctx *ctx, void *stream) {
    if (!ctx) return SNOWTRI_ERR_BAD_ARG;
    ENTER_DEVICE(ctx->device);
    for (auto &S : ctx->sets)
        if (S.pending) {
            HIP_TRY(hipEventRecord(S.done, S.stream));
            HIP_TRY(hipStreamWaitEvent((hipStream_t)stream, S.done, 0));
            S.pending = false;
        }
    return SNOWTRI_OK;
}

int snowtri_set_timing(snowtri_ctx *ctx, int enabled) {
    if (!ctx) return SNOWTRI_ERR_BAD_ARG;
    ctx->timing = enabled != 0;
    ctx->timing_attach = enabled == 2;
    ctx->ev_valid = false;
    ctx->ev_count = 0;
    if (ctx->timing && ctx->ev_ring.empty()) {
        ENTER_DEVICE(ctx->device);
        ctx->ev_ring.resize(2 * kTimingRing, nullptr);
        for (auto &e : ctx->ev_ring) HIP_TRY(hipEventCreate(&e));
    }
    return SNOWTRI_OK;
}

int snowtri_timing_collect(snowtri_ctx *ctx, float *kernel_ms, int32_t cap) {
    if (!ctx || !kernel_ms || cap < 0) return -1;
    const int64_t n = std::min<int64_t>(std::min<int64_t>(ctx->ev_count, kTimingRing), cap);
    const int64_t first = ctx->ev_count - n;
    for (int64_t i = 0; i < n; i++) {
        const int64_t slot = (first + i) % kTimingRing;
        if (hipEventSynchronize(ctx->ev_ring[2 * slot + 1]) != hipSuccess) return -1;
        if (hipEventElapsedTime(&kernel_ms[i], ctx->ev_ring[2 * slot], ctx->ev_ring[2 * slot + 1]) != hipSuccess) return -1;
    }
    ctx->ev_count = 0;
    return (int)n;
}

int snowtri_last_kernel_ms(snowtri_ctx *ctx, float kernel_ms[2]) {
    if (!ctx || !kernel_ms) return SNOWTRI_ERR_BAD_ARG;
    kernel_ms[0] = kernel_ms[1] = 0.f;
    if (!ctx->ev_valid) return SNOWTRI_ERR_BAD_ARG;
    HIP_TRY(hipEventSynchronize(ctx->ev[3]));
    float a = 0.f, b = 0.f;
    HIP_TRY(hipEventElapsedTime(&a, ctx->ev[0], ctx->ev[1]));
    HIP_TRY(hipEventElapsedTime(&b, ctx->ev[2], ctx->ev[3]));
    kernel_ms[0] = a;
    kernel_ms[1] = b;
    return SNOWTRI_OK;
}

int64_t snowtri_last_slow_frames(snowtri_ctx *ctx) { return ctx ? ctx->last_slow_frames : -1; }

int64_t snowtri_last_handover_persons(snowtri_ctx *ctx, int64_t *n_other) {
    if (n_other) *n_other = -1;
    if (!ctx || !ctx->last_handover) return -1;
    DeviceGuard guard(ctx->device);
    unsigned long long n[kHandMembers + 1] = {0};   // [kHandComplete] complete-graph clusters, [kHandMembers] >> 32 clusters of any other shape
    if (hipDeviceSynchronize() != hipSuccess) return -1;
    if (hipMemcpy(n, ctx->last_set->d_counters + kHandCountersAt, sizeof(n), hipMemcpyDeviceToHost) != hipSuccess) return -1;
    if (n_other) *n_other = (int64_t)hand_member_descs(n[kHandMembers]);
    return (int64_t)n[kHandComplete];
}

int snowtri_last_stream_counts(snowtri_ctx *ctx, int64_t counts[3]) {
    if (!ctx || !counts) return SNOWTRI_ERR_BAD_ARG;
    counts[0] = counts[1] = counts[2] = -1;
    if (!ctx->last_stream) return SNOWTRI_OK;
    ENTER_DEVICE(ctx->device);
    unsigned long long n[3] = {0, 0, 0};   // d_counters[6..8]: slow frames, frames with an exact candidate sum, slow frames of the second pass
    HIP_TRY(hipDeviceSynchronize());
    HIP_TRY(hipMemcpy(n, ctx->last_set->d_counters + 6, sizeof(n), hipMemcpyDeviceToHost));
    counts[0] = (int64_t)n[0];
    counts[1] = (int64_t)n[1];
    counts[2] = (int64_t)n[2];
    return SNOWTRI_OK;
}

int snowtri_ctx_stream_probes(const snowtri_ctx *ctx, int64_t out[3]) {
    if (!ctx || !out) return SNOWTRI_ERR_BAD_ARG;
    out[0] = ctx->probes;
    out[1] = ctx->probe_replaced;
    out[2] = ctx->probe_verdict;
    return SNOWTRI_OK;
}

const char *snowtri_last_kernel_names(const snowtri_ctx *ctx) { return ctx ? ctx->last_kernels : ""; }

#ifdef SNOWTRI_DEBUG_BOUNDS
namespace {
__global__ void k_debug_selftest(int n) { SNOWTRI_DEV_CHECK((int)threadIdx.x < n, 99); }   // lanes n .. 63 violate it
}
#endif
#ifdef SNOWTRI_LEAN_TRACE
extern "C" int snowtri_debug_read_scratch(snowtri_ctx *ctx, void *dst, size_t bytes) {   // dev build only: the stamps of k_fused_lean_coop
    if (!ctx || bytes > ctx->work.cap) return SNOWTRI_ERR_BAD_ARG;
    return hipMemcpy(dst, ctx->work.p, bytes, hipMemcpyDeviceToHost) == hipSuccess ? SNOWTRI_OK : SNOWTRI_ERR_HIP;
}
#endif
#ifdef SNOWTRI_SUMS_TRACE
extern "C" int snowtri_debug_read_sums_trace(void *dst) {   // dev build only: the stamps of k_candidate_sums
    (void)hipDeviceSynchronize();
    return hipMemcpyFromSymbol(dst, HIP_SYMBOL(snowtri::g_sums_trace), sizeof(unsigned long long) * 4096 * 4 * 16) == hipSuccess ? 0 : 3;
}
#endif
#ifdef SNOWTRI_ASSOC_TRACE
extern "C" int snowtri_debug_read_assoc_trace(void *dst) {   // dev build only: the stamps of k_associate
    (void)hipDeviceSynchronize();
    return hipMemcpyFromSymbol(dst, HIP_SYMBOL(snowtri::g_assoc_trace), sizeof(unsigned long long) * 4096 * 16) == hipSuccess ? 0 : 3;
}
#endif
int snowtri_debug_selftest(snowtri_ctx *ctx) {
#ifdef SNOWTRI_DEBUG_BOUNDS
    if (!ctx) return SNOWTRI_ERR_BAD_ARG;
    ENTER_DEVICE(ctx->device);
    hipLaunchKernelGGL(k_debug_selftest, dim3(1), dim3(64), 0, nullptr, 61);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipDeviceSynchronize());
    return SNOWTRI_OK;
#else
    (void)ctx;
    return -1;
#endif
}

int64_t snowtri_debug_faults(snowtri_ctx *ctx, uint64_t *first) {
    if (first) *first = 0;
#ifdef SNOWTRI_DEBUG_BOUNDS
    if (!ctx) return -2;
    DeviceGuard guard(ctx->device);
    if (guard.err != hipSuccess || hipDeviceSynchronize() != hipSuccess) return -2;
    unsigned long long v[2] = {0ull, 0ull}, zero[2] = {0ull, 0ull};
    if (hipMemcpyFromSymbol(v, HIP_SYMBOL(snowtri::g_dev_fault), sizeof(v)) != hipSuccess) return -2;
    if (hipMemcpyToSymbol(HIP_SYMBOL(snowtri::g_dev_fault), zero, sizeof(zero)) != hipSuccess) return -2;
    if (first) *first = v[1];
    return (int64_t)v[0];
#else
    (void)ctx;
    return -1;   // this build has no device-side checks
#endif
}

int64_t snowtri_num_candidate_slots(int32_t C, int32_t Pmax) {
    if (C < 0 || Pmax < 0) return -1;
    return (int64_t)C * (C - 1) / 2 * Pmax * Pmax;
}

// Test hook: the fast-math helpers of the throughput kernels on caller-supplied values.
int snowtri_fastmath_probe(snowtri_ctx *ctx, int64_t n, const double *x, double *rcp_nr2_out,
                           double *rcp_nr1_out, double *rsq_nr1_out) {
    if (!ctx || n < 1 || !x || !rcp_nr2_out || !rcp_nr1_out || !rsq_nr1_out) return SNOWTRI_ERR_BAD_ARG;
    ENTER_DEVICE(ctx->device);
    const size_t b = sizeof(double) * n;
    Staging sg(ctx->in, ctx->out, true, nullptr);
    sg.in(&x, b);
    sg.out(&rcp_nr2_out, b);
    sg.out(&rcp_nr1_out, b);
    sg.out(&rsq_nr1_out, b);
    if (int rc = sg.begin()) return rc;
    hipLaunchKernelGGL(k_fastmath_probe, dim3(grid_for(n, kBlock, ctx->num_cus * 8)), dim3(kBlock), 0, 0, n, x, rcp_nr2_out, rcp_nr1_out,
                       rsq_nr1_out);
    HIP_TRY(hipGetLastError());
    return sg.end();
}

int snowtri_fastmath_probe_raw(snowtri_ctx *ctx, int64_t n, const double *x, double *rcp_raw_out, double *rsq_raw_out) {
    if (!ctx || n < 1 || !x || !rcp_raw_out || !rsq_raw_out) return SNOWTRI_ERR_BAD_ARG;
    ENTER_DEVICE(ctx->device);
    const size_t b = sizeof(double) * n;
    Staging sg(ctx->in, ctx->out, true, nullptr);
    sg.in(&x, b);
    sg.out(&rcp_raw_out, b);
    sg.out(&rsq_raw_out, b);
    if (int rc = sg.begin()) return rc;
    hipLaunchKernelGGL(k_fastmath_probe_raw, dim3(grid_for(n, kBlock, ctx->num_cus * 8)), dim3(kBlock), 0, 0, n, x, rcp_raw_out, rsq_raw_out);
    HIP_TRY(hipGetLastError());
    return sg.end();
}

int snowtri_calib_stream(snowtri_ctx *ctx, const void *src, int64_t read_bytes, void *dst, int64_t write_bytes, void *stream) {
    if (!ctx || read_bytes < 0 || write_bytes < 0 || (read_bytes > 0 && !src) || (write_bytes > 0 && !dst)) return SNOWTRI_ERR_BAD_ARG;
    ENTER_DEVICE(ctx->device);
    hipStream_t st = (hipStream_t)stream;
    if (read_bytes >= 12) {
        int rc = ctx->misc.ensure(64);
        if (rc) return rc;
        hipLaunchKernelGGL(k_calib_read12, dim3(ctx->num_cus * 8), dim3(kBlock), 0, st, read_bytes / 12, (const Rec12 *)src,
                           (float *)ctx->misc.p);
    }
    if (write_bytes >= 16)
        hipLaunchKernelGGL(k_calib_write16, dim3(ctx->num_cus * 8), dim3(kBlock), 0, st, write_bytes / 16, (float4 *)dst);
    HIP_TRY(hipGetLastError());
    return SNOWTRI_OK;
}

// ------------------------------------------------------------------------------------------ A1
int snowtri_rays_from_pixels(snowtri_ctx *ctx, int32_t cam, int64_t n, const double *uv, double *rays) {
    if (!ctx || n < 0 || (n > 0 && (!uv || !rays))) return SNOWTRI_ERR_BAD_ARG;
    if (cam < 0 || cam >= ctx->C) return SNOWTRI_ERR_BAD_INDEX;   // cameras[camera_index] raises IndexError (camera.py:236)
    if (n == 0) return SNOWTRI_OK;
    ENTER_DEVICE(ctx->device);
    Staging sg(ctx->in, ctx->out, true, nullptr);
    sg.in(&uv, sizeof(double) * 2 * n);
    sg.out(&rays, sizeof(double) * 3 * n);
    if (int rc = sg.begin()) return rc;
    hipLaunchKernelGGL(k_rays, dim3(grid_for(n, kBlock, ctx->num_cus * 8)), dim3(kBlock), 0, 0, n, ctx->dM + 9 * cam, uv, rays);
    HIP_TRY(hipGetLastError());
    return sg.end();
}

// ------------------------------------------------------------------------------------------ A2
int snowtri_skew_ray_batch(snowtri_ctx *ctx, int64_t n, const double *hm, const double *hs,
                           const double *tm, const double *ts, double *dist, double *W,
                           int64_t *n_singular) {
    if (!ctx || n < 0 || (n > 0 && (!hm || !hs || !tm || !ts || !dist || !W))) return SNOWTRI_ERR_BAD_ARG;
    if (n_singular) *n_singular = 0;
    if (n == 0) return SNOWTRI_OK;
    ENTER_DEVICE(ctx->device);
    const size_t v = sizeof(double) * 3 * n;
    Staging sg(ctx->in, ctx->out, true, nullptr);
    sg.in(&hm, v);
    sg.in(&hs, v);
    sg.in(&tm, v);
    sg.in(&ts, v);
    sg.out(&W, v);
    sg.out(&dist, sizeof(double) * n);
    if (int rc = sg.begin()) return rc;
    HIP_TRY(hipMemset(ctx->d_counters, 0, sizeof(unsigned long long)));
    hipLaunchKernelGGL(k_skew, dim3(grid_for(n, kBlock, ctx->num_cus * 8)), dim3(kBlock), 0, 0, n, hm, hs, tm, ts, dist, W, ctx->d_counters);
    HIP_TRY(hipGetLastError());
    if (int rc = sg.end()) return rc;
    unsigned long long ns = 0;
    HIP_TRY(hipMemcpy(&ns, ctx->d_counters, sizeof(ns), hipMemcpyDeviceToHost));
    if (n_singular) *n_singular = (int64_t)ns;
    return ns ? SNOWTRI_ERR_SINGULAR : SNOWTRI_OK;
}

}  // extern "C"

// ---------------------------------------------------------------------------------- helpers
namespace {

int validate_params(const snowtri_params *p, int J, Params *out, bool need_condense) {
    if (!p) return SNOWTRI_ERR_BAD_ARG;
    Params q;
    q.kthr = p->keypoint_score_threshold;
    q.avg_thr = p->average_score_threshold;
    q.dthr = p->distance_threshold;
    q.ctol = p->condense_distance_tol;
    q.num_tol = p->condense_person_num_tol;
    q.score_tol = p->condense_score_tol;
    q.center = p->center_point_index;
    q.kn = p->keypoint_num;
    if (need_condense) {
        if (q.center < 0) q.center += J;  // Python negative indexing (triangulation.py:112)
        if (q.center < 0 || q.center >= J || q.kn < 0 || q.kn > J) return SNOWTRI_ERR_BAD_INDEX;
        if (q.kn > kCondenseMaxJointsPerThread * kBlock) return SNOWTRI_ERR_BAD_ARG;
    }
    q.dthr2 = (q.dthr < 0.0) ? -1.0 : q.dthr * q.dthr;
    {
        float kf = (float)q.kthr;  // round to nearest, then step up if that landed below kthr
        if ((double)kf < q.kthr) kf = std::nextafter(kf, std::numeric_limits<float>::infinity());
        q.kthr_f32 = kf;            // NaN stays NaN: every comparison false, as in NumPy
    }
    q.no_zero_fill = 0;             // (snowtri_triangulate_condense_ex sets it from its call flags)
    *out = q;
    return SNOWTRI_OK;
}

size_t dtype_size(int dt) { return dt == SNOWTRI_F32 ? 4 : 8; }

// m*: the mapped twins of the outputs and of the singular count, which the kernels fill as well (Staging::mapped; null: no mirror)
template <typename TIn>
void launch_triangulate(snowtri_ctx *ctx, hipStream_t st, int64_t F, int Pmax, int J, int Kc,
                        const void *kpts, const int32_t *n_persons, const Params &prm, double *cxyz,
                        double *cks, double *cps, uint8_t *ckeep, unsigned long long *n_singular, double *mx = nullptr,
                        double *mk = nullptr, double *mp = nullptr, uint8_t *mkeep = nullptr, unsigned long long *mns = nullptr,
                        HostDone done = HostDone{nullptr, nullptr, 0ull}, bool *one_launch = nullptr) {
    const int64_t total = F * (int64_t)Kc * J;
    if (mx && F * (int64_t)Kc <= 4096 && J <= 4096) {   // the per-frame call: one launch, a workgroup per candidate slot
        hipLaunchKernelGGL((k_triangulate_slots<TIn>), dim3((unsigned)(F * Kc)), dim3(kBlock), sizeof(double) * J, st, F, Pmax, J, Kc, ctx->rig(),
                           (const TIn *)kpts, n_persons, prm, cxyz, cks, cps, ckeep, n_singular, mx, mk, mp, mkeep,
                           mns, (unsigned int *)(n_singular + 1), done);
        if (one_launch) *one_launch = true;
        return;
    }
    hipLaunchKernelGGL((k_triangulate<TIn>), dim3(grid_for(total, kBlock, ctx->num_cus * 16)), dim3(kBlock), 0,
                       st, F, Pmax, J, Kc, ctx->rig(), (const TIn *)kpts, n_persons, prm, cxyz, cks,
                       n_singular, mx, mk);
    hipLaunchKernelGGL(k_cand_mean, dim3(grid_for(F * (int64_t)Kc, kBlock / 64, ctx->num_cus * 16)),
                       dim3(kBlock), 0, st, F, Pmax, J, Kc, ctx->rig(), n_persons, prm, (const double *)cks,
                       cps, ckeep, mp, mkeep, n_singular, mns);
}

constexpr int kCondenseMaxN = 9000;  // condense_lds_bytes(N) <= 160 KiB

template <typename Writer>
int launch_condense(snowtri_ctx *ctx, hipStream_t st, int64_t nframes, int N, int J, const double *cxyz,
                    const double *cks, const uint8_t *ckeep, const Params &prm, int Pout, Writer wr,
                    int32_t *out_count, uint32_t *out_flags, HostDone done = HostDone{nullptr, nullptr, 0ull}) {
    if (N > kCondenseMaxN) return SNOWTRI_ERR_BAD_ARG;
    const size_t lds = condense_lds_bytes(N);
    auto kern = k_condense<Writer>;
    if (lds > 48 * 1024)
        {
            if (ctx->raise_lds((const void *)kern, (int)lds)) {
                g_last_error = "hipFuncSetAttribute(MaxDynamicSharedMemorySize) failed";
                return SNOWTRI_ERR_HIP;
            }
        }
    hipLaunchKernelGGL(kern, dim3(grid_for(nframes, 1, ctx->num_cus * 8)), dim3(kBlock), lds, st, nframes, N, J,
                       cxyz, cks, ckeep, prm, Pout, wr, out_count, out_flags, done);
    HIP_TRY(hipGetLastError());
    return SNOWTRI_OK;
}

}  // namespace

extern "C" {

// --------------------------------------------------------------------------------------- A1+A3
int snowtri_triangulate(snowtri_ctx *ctx, int64_t F, int32_t Pmax, int32_t J, const void *kpts,
                        int in_dtype, const int32_t *n_persons, const snowtri_params *params,
                        double *cand_xyz, double *cand_kscore, double *cand_pscore, uint8_t *cand_keep,
                        int memspace, void *stream) {
    if (!ctx || ctx->C < 1 || F < 0 || Pmax < 1 || J < 1 || !params) return SNOWTRI_ERR_BAD_ARG;
    if (in_dtype != SNOWTRI_F32 && in_dtype != SNOWTRI_F64) return SNOWTRI_ERR_BAD_ARG;
    if (memspace != SNOWTRI_HOST && memspace != SNOWTRI_DEVICE) return SNOWTRI_ERR_BAD_ARG;
    const int64_t Kc = snowtri_num_candidate_slots(ctx->C, Pmax);
    if (F == 0 || Kc == 0) return SNOWTRI_OK;
    if (!kpts || !cand_xyz || !cand_kscore || !cand_pscore || !cand_keep) return SNOWTRI_ERR_BAD_ARG;
    Params prm;
    int rc = validate_params(params, J, &prm, false);
    if (rc) return rc;
    ENTER_DEVICE(ctx->device);
    hipStream_t st = (hipStream_t)stream;
    const bool host = memspace == SNOWTRI_HOST;
    const size_t slots = (size_t)F * Kc, nx = slots * J;
    const void *d_kpts = kpts;
    const int32_t *d_np = n_persons;
    double *d_xyz = cand_xyz, *d_ks = cand_kscore, *d_ps = cand_pscore;
    uint8_t *d_keep = cand_keep;
    unsigned long long ns = 0, *d_nsing = host ? &ns : ctx->d_counters;   // (a host call's singular-pair counter rides behind its outputs)
    // The outputs in a scratch of their own: the candidates stay resident for snowtri_condense_resident.  The per-frame call takes
    // the mapped route: its kernels read the staged inputs and mirror their outputs in mapped page-locked memory, no copy engine.
    Staging sg(ctx->in, ctx->cand, host, st, ctx, Staging::kMapped);
    sg.in(&d_kpts, (size_t)F * ctx->C * Pmax * J * 3 * dtype_size(in_dtype));
    sg.in(&d_np, sizeof(int32_t) * F * ctx->C);
    sg.out(&d_xyz, sizeof(double) * nx * 3);
    sg.out(&d_ks, sizeof(double) * nx);
    sg.out(&d_ps, sizeof(double) * slots);
    sg.out(&d_keep, slots);
    sg.out(&d_nsing, sizeof(ns));
    if (host) ctx->cand_token = 0;
    rc = sg.begin();
    if (rc) return rc;
    unsigned long long *const m_nsing = sg.mapped(d_nsing);
    if (m_nsing) d_nsing = ctx->d_counters + kTriangulateSingularAt;   // (left at 0 by every call: the kernels hand it over to the twin)
    if (host) rc = sg.clear_outputs();   // invalid slots read back as zeros; counter = 0
    else HIP_TRY(hipMemsetAsync(d_nsing, 0, sizeof(unsigned long long), st));
    if (rc) return rc;
    bool polled = false;   // the one-launch kernel signals the completion word
    if (in_dtype == SNOWTRI_F32)
        launch_triangulate<float>(ctx, st, F, Pmax, J, (int)Kc, d_kpts, d_np, prm, d_xyz, d_ks, d_ps, d_keep, d_nsing, sg.mapped(d_xyz),
                                  sg.mapped(d_ks), sg.mapped(d_ps), sg.mapped(d_keep), m_nsing, sg.done, &polled);
    else
        launch_triangulate<double>(ctx, st, F, Pmax, J, (int)Kc, d_kpts, d_np, prm, d_xyz, d_ks, d_ps, d_keep, d_nsing, sg.mapped(d_xyz),
                                   sg.mapped(d_ks), sg.mapped(d_ps), sg.mapped(d_keep), m_nsing, sg.done, &polled);
    HIP_TRY(hipGetLastError());
    rc = sg.end(polled);
    if (rc) return rc;
    if (host) {
        // the candidates stay on the device under a fresh token (snowtri_condense_resident)
        static std::atomic<int64_t> next_token{1};
        ctx->cand_token = next_token.fetch_add(1);
        ctx->cand_F = F;
        ctx->cand_Kc = Kc;
        ctx->cand_J = J;
        ctx->cand_xyz = d_xyz;
        ctx->cand_ks = d_ks;
        ctx->cand_keep = d_keep;
        if (ns) return SNOWTRI_ERR_SINGULAR;
    }
    return SNOWTRI_OK;
}

int64_t snowtri_candidates_token(const snowtri_ctx *ctx) { return ctx ? ctx->cand_token : 0; }

// ------------------------------------------------------------------------------------------ A4
int snowtri_condense(snowtri_ctx *ctx, int64_t F, int32_t N, int32_t J, const double *cand_xyz,
                     const double *cand_kscore, const uint8_t *cand_keep, const snowtri_params *params,
                     int32_t Pout_max, double *out_xyz, double *out_kscore, double *out_pscore,
                     int32_t *out_count, uint32_t *out_flags, int memspace, void *stream) {
    if (!ctx || F < 0 || N < 0 || J < 1 || Pout_max < 1 || !params) return SNOWTRI_ERR_BAD_ARG;
    if (memspace != SNOWTRI_HOST && memspace != SNOWTRI_DEVICE) return SNOWTRI_ERR_BAD_ARG;
    if (F == 0) return SNOWTRI_OK;
    if (!out_xyz || !out_kscore || !out_pscore || !out_count) return SNOWTRI_ERR_BAD_ARG;
    if (N > 0 && (!cand_xyz || !cand_kscore)) return SNOWTRI_ERR_BAD_ARG;
    Params prm;
    int rc = validate_params(params, J, &prm, true);
    if (rc) return rc;
    ENTER_DEVICE(ctx->device);
    hipStream_t st = (hipStream_t)stream;
    const size_t nx = (size_t)F * N * J, no = (size_t)F * Pout_max * prm.kn;
    const double *d_xyz = cand_xyz, *d_ks = cand_kscore;
    const uint8_t *d_keep = cand_keep;
    double *o_xyz = out_xyz, *o_ks = out_kscore, *o_ps = out_pscore;
    int32_t *o_cnt = out_count;
    uint32_t *o_fl = out_flags;
    const bool host = memspace == SNOWTRI_HOST;
    Staging sg(ctx->in, ctx->out, host, st, ctx, Staging::kPinned);
    sg.in(&d_xyz, sizeof(double) * nx * 3);
    sg.in(&d_ks, sizeof(double) * nx);
    sg.in(&d_keep, (size_t)F * N);
    sg.out(&o_xyz, sizeof(double) * no * 3);
    sg.out(&o_ks, sizeof(double) * no);
    sg.out(&o_ps, sizeof(double) * F * Pout_max);
    sg.out(&o_cnt, sizeof(int32_t) * F);
    sg.out(&o_fl, sizeof(uint32_t) * F);
    rc = sg.begin();
    if (rc) return rc;
    if (o_fl) HIP_TRY(hipMemsetAsync(o_fl, 0, sizeof(uint32_t) * F, st));
    rc = launch_condense(ctx, st, F, N, J, d_xyz, d_ks, d_keep, prm, Pout_max, SplitWriter{o_xyz, o_ks, o_ps},
                         o_cnt, o_fl);
    if (rc) return rc;
    rc = sg.end();
    if (rc) return rc;
    for (int64_t f = 0; host && f < F; f++)
        if (out_count[f] > Pout_max) return SNOWTRI_ERR_OVERFLOW;
    return SNOWTRI_OK;
}

// A4 on the candidates the last SNOWTRI_HOST snowtri_triangulate call left on the device: what Human_Triangulation_Condense
// does when it is handed the unmodified result of Human_Triangulation (main.py:62-71) -- no second trip over PCIe for the
// candidates (25 KB per frame at 4 x 1 x 133: the upload was a quarter of the per-frame latency).
int snowtri_condense_resident(snowtri_ctx *ctx, int64_t token, const snowtri_params *params, int32_t Pout_max, double *out_xyz,
                              double *out_kscore, double *out_pscore, int32_t *out_count, uint32_t *out_flags) {
    if (!ctx || !params || Pout_max < 1 || !out_xyz || !out_kscore || !out_pscore || !out_count) return SNOWTRI_ERR_BAD_ARG;
    if (token == 0 || token != ctx->cand_token) return SNOWTRI_ERR_BAD_ARG;   // (another triangulate call replaced them)
    const int64_t F = ctx->cand_F, N = ctx->cand_Kc;
    const int J = (int)ctx->cand_J;
    Params prm;
    int rc = validate_params(params, J, &prm, true);
    if (rc) return rc;
    ENTER_DEVICE(ctx->device);
    hipStream_t st = nullptr;
    const size_t no = (size_t)F * Pout_max * prm.kn;
    double *o_xyz = out_xyz, *o_ks = out_kscore, *o_ps = out_pscore;
    int32_t *o_cnt = out_count;
    // (the only flag of this entry is the overflow bit: derived from the counts below, no atomics on mapped memory)
    Staging sg(ctx->in, ctx->out, true, st, ctx, Staging::kMapped);
    sg.out(&o_xyz, sizeof(double) * no * 3);
    sg.out(&o_ks, sizeof(double) * no);
    sg.out(&o_ps, sizeof(double) * F * Pout_max);
    sg.out(&o_cnt, sizeof(int32_t) * F);
    rc = sg.begin();
    if (rc) return rc;
    if (sg.mapped(o_cnt))   // the kernel writes the page-locked staging buffer itself, and nothing else
        o_xyz = sg.mapped(o_xyz), o_ks = sg.mapped(o_ks), o_ps = sg.mapped(o_ps), o_cnt = sg.mapped(o_cnt);
    rc = launch_condense(ctx, st, F, (int)N, J, ctx->cand_xyz, ctx->cand_ks, ctx->cand_keep, prm, Pout_max, SplitWriter{o_xyz, o_ks, o_ps}, o_cnt,
                         (uint32_t *)nullptr, sg.done);
    if (rc) return rc;
    rc = sg.end(true);   // (k_condense signals the completion word it is given)
    if (rc) return rc;
    int status = SNOWTRI_OK;
    for (int64_t f = 0; f < F; f++) {
        const bool over = out_count[f] > Pout_max;
        if (out_flags) out_flags[f] = over ? SNOWTRI_FLAG_OVERFLOW : 0u;
        if (over) status = SNOWTRI_ERR_OVERFLOW;
    }
    return status;
}

}  // extern "C"

// ---------------------------------------------------------------------------------------- N1
namespace {

constexpr int kSmoothChunk = 256;

// p = A^L by repeated multiplication (fp64), row-major
void smooth_power(const SmoothCoef &k, int L, double p[4]) {
    p[0] = p[3] = 1.0;
    p[1] = p[2] = 0.0;
    for (int i = 0; i < L; i++) {
        const double q0 = k.a00 * p[0] + k.a01 * p[2], q1 = k.a00 * p[1] + k.a01 * p[3];
        const double q2 = k.a10 * p[0] + k.a11 * p[2], q3 = k.a10 * p[1] + k.a11 * p[3];
        p[0] = q0; p[1] = q1; p[2] = q2; p[3] = q3;
    }
}

SmoothCoef smooth_coef(double f, double z, double r, double dt) {
    const double pi = 3.141592653589793;
    const double k1 = z / (pi * f), k2 = 1.0 / ((2 * pi * f) * (2 * pi * f)), k3 = r * z / (2 * pi * f);
    SmoothCoef k;
    k.a00 = 1.0;
    k.a01 = dt;
    k.a10 = -dt / k2;
    k.a11 = 1.0 - dt * dt / k2 - dt * k1 / k2;
    k.cx = dt / k2;
    k.cxd = k3 / k2;  // (T/k2) * k3 * (x - xp)/T
    double p[4];
    smooth_power(k, kSmoothChunk, p);
    k.p00 = p[0]; k.p01 = p[1]; k.p10 = p[2]; k.p11 = p[3];
    smooth_power(k, kScanL, p);  // A^32: the frames one wave of the one-pass scan holds (k_smooth_scan)
    k.r00 = p[0]; k.r01 = p[1]; k.r10 = p[2]; k.r11 = p[3];
    return k;
}

dim3 smooth_grid(int64_t n, int64_t nchunks) {
    return dim3((unsigned)((n + kSmoothBlock - 1) / kSmoothBlock), (unsigned)std::max<int64_t>(1, nchunks));
}

// Zero-state response of frames [tb, T) into dy (frame 0 passes through when first); optional end state.
// This is the first half of the two-call protocol of a frame-sharded track.
template <typename KS>
int smooth_local_dev(snowtri_ctx *ctx, hipStream_t st, int64_t T, int64_t n, const double *dx, double *dy,
                     bool first, const KS &k, double *d_end) {
    const int tb = first ? 1 : 0;
    const int64_t m = T - tb, nchunks = (m + kSmoothChunk - 1) / kSmoothChunk;
    if (nchunks > 65535) return SNOWTRI_ERR_BAD_ARG;
    if (m <= 0) {  // a one-frame first shard: nothing is filtered
        HIP_TRY(hipMemcpyAsync(dy, dx, sizeof(double) * (size_t)T * n, hipMemcpyDeviceToDevice, st));
        if (d_end) HIP_TRY(hipMemsetAsync(d_end, 0, sizeof(double) * 2 * n, st));
        return SNOWTRI_OK;
    }
    int rc = ctx->work.ensure(sizeof(double) * 4 * (size_t)nchunks * n + 64);
    if (rc) return rc;
    double *E = (double *)ctx->work.p, *S = E + 2 * (size_t)nchunks * n;
    const dim3 g2 = smooth_grid(n, nchunks), g1 = smooth_grid(n, 1);
    hipLaunchKernelGGL((k_smooth_local<KS, NoHold>), g2, dim3(kSmoothBlock), 0, st, T, n, kSmoothChunk, tb, k, NoHold{}, dx,
                       (const double *)nullptr, dy, E);
    hipLaunchKernelGGL(k_smooth_carry<KS>, g1, dim3(kSmoothBlock), 0, st, n, nchunks, k, (const double *)nullptr,
                       (const double *)E, S);
    hipLaunchKernelGGL(k_smooth_fix<KS>, g2, dim3(kSmoothBlock), 0, st, T, n, kSmoothChunk, tb, k, (const double *)S, dy,
                       (double *)nullptr);
    if (d_end)
        hipLaunchKernelGGL(k_smooth_shard_end<KS>, g1, dim3(kSmoothBlock), 0, st, T, n, kSmoothChunk, tb, nchunks, k,
                           (const double *)S, (const double *)E, d_end);
    HIP_TRY(hipGetLastError());
    return SNOWTRI_OK;
}

// dy += homogeneous response of the state `d_start` entering frame tb (second half of the sharded protocol).
template <typename KS>
int smooth_fix_dev(snowtri_ctx *ctx, hipStream_t st, int64_t T, int64_t n, double *dy, bool first,
                   const double *d_start, const KS &k) {
    const int tb = first ? 1 : 0;
    const int64_t m = T - tb, nchunks = (m + kSmoothChunk - 1) / kSmoothChunk;
    if (m <= 0) return SNOWTRI_OK;
    if (nchunks > 65535) return SNOWTRI_ERR_BAD_ARG;
    int rc = ctx->work.ensure(sizeof(double) * 2 * (size_t)nchunks * n + 64);
    if (rc) return rc;
    double *S = (double *)ctx->work.p;
    hipLaunchKernelGGL(k_smooth_carry<KS>, smooth_grid(n, 1), dim3(kSmoothBlock), 0, st, n, nchunks, k, d_start,
                       (const double *)nullptr, S);
    hipLaunchKernelGGL(k_smooth_fix<KS>, smooth_grid(n, nchunks), dim3(kSmoothBlock), 0, st, T, n, kSmoothChunk, tb, k,
                       (const double *)S, dy, (double *)nullptr);
    HIP_TRY(hipGetLastError());
    return SNOWTRI_OK;
}

// A whole (unsharded) track in ONE pass over HBM: the chained scan with decoupled look-back of snowtri_smooth.hpp
// (k_smooth_scan) -- x read once, y written once.  d_seed_row: [n] inputs of frame 0 as the filters see them (x[0] itself for
// N1; the held x_eff[0] for N2).  skip4: every fourth lane (the score of a joint record) is copied instead of filtered.
// (Rounds 1-5 ran three passes -- chunk-end states, the carry over the chunks, the recurrence again: 24 bytes moved per 16
// algorithmic; the sharded protocol below still does, its entering state is not known before the exchange.)
// tb / d_start / d_end: the frame-shard forms (k_smooth_scan): tb = 0 filters every frame, d_start [2n] is the state entering the
// first filtered frame, d_end [2n] receives the state behind the last frame, dy == nullptr stores no track (the "reduce" pass).
template <typename KS, typename HS>
int smooth_whole_dev(snowtri_ctx *ctx, hipStream_t st, int64_t T, int64_t n, const double *dx, double *dy,
                     const double *d_seed_row, const KS &k, const HS &hs, bool skip4 = false, int tb = 1, const double *d_start = nullptr,
                     double *d_end = nullptr) {
    const int64_t m = T - tb, nsuper = (m + kScanSuper - 1) / kScanSuper, ncols = (n + 63) / 64;
    if (nsuper > 65535) return SNOWTRI_ERR_BAD_ARG;   // (the documented limit of the track length: 1 + 256 * 65535 frames)
    if (m <= 0) {   // a one-frame track / first shard: nothing is filtered; the state behind it is the entering one
        if (dy) HIP_TRY(hipMemcpyAsync(dy, dx, sizeof(double) * (size_t)T * n, hipMemcpyDeviceToDevice, st));
        if (d_end) {
            if (d_start)
                HIP_TRY(hipMemcpyAsync(d_end, d_start, sizeof(double) * 2 * n, hipMemcpyDeviceToDevice, st));
            else
                HIP_TRY(hipMemsetAsync(d_end, 0, sizeof(double) * 2 * n, st));
        }
        return SNOWTRI_OK;
    }
    if (nsuper * ncols >= ((int64_t)1 << 31) || n > ((int64_t)1 << 22)) return SNOWTRI_ERR_BAD_ARG;   // (lanes: the 32-bit buffer offsets of k_smooth_scan)
    const size_t nwg = (size_t)nsuper * ncols;
    const size_t off_flags = 256, off_agg = (off_flags + 4 * nwg + 255) & ~(size_t)255, off_incl = off_agg + sizeof(double) * 128 * nwg;
    int rc = ctx->work.ensure(off_incl + sizeof(double) * 128 * nwg);
    if (rc) return rc;
    char *base = (char *)ctx->work.p;
    HIP_TRY(hipMemsetAsync(base, 0, off_agg, st));   // the ticket and the flags
    unsigned int *ticket = (unsigned int *)base, *flags = (unsigned int *)(base + off_flags);
    double *agg = (double *)(base + off_agg), *incl = (double *)(base + off_incl);
    if (skip4)
        hipLaunchKernelGGL((k_smooth_scan<KS, HS, true>), dim3((unsigned)nwg), dim3(kScanThreads), 0, st, T, n, k, hs, dx, d_seed_row, dy, ticket, flags, agg, incl,
                           tb, d_start, d_end);
    else
        hipLaunchKernelGGL((k_smooth_scan<KS, HS, false>), dim3((unsigned)nwg), dim3(kScanThreads), 0, st, T, n, k, hs, dx, d_seed_row, dy, ticket, flags, agg, incl,
                           tb, d_start, d_end);
    HIP_TRY(hipGetLastError());
    return SNOWTRI_OK;
}

// per-bone coefficient table of the context, as the filters take it (*k): rebuilt and uploaded only when (fzr, dt) change -- the
// common caller passes the same smooth profile every time, and an upload has to drain the stream first
int blender_table(snowtri_ctx *ctx, hipStream_t st, const double *fzr, double dt, TableCoef *k) {
    std::vector<double> key(fzr, fzr + 3 * kBlenderPoints);
    key.push_back(dt);
    if (!ctx->dBlenderTab) HIP_TRY(hipMalloc(&ctx->dBlenderTab, sizeof(SmoothCoef) * kBlenderPoints));
    if (key != ctx->blender_key) {
        SmoothCoef tab[kBlenderPoints];
        for (int i = 0; i < kBlenderPoints; i++) tab[i] = smooth_coef(fzr[3 * i], fzr[3 * i + 1], fzr[3 * i + 2], dt);
        HIP_TRY(hipStreamSynchronize(st));   // kernels of an earlier call may still read the old table
        HIP_TRY(hipMemcpy(ctx->dBlenderTab, tab, sizeof(tab), hipMemcpyHostToDevice));
        ctx->blender_key = key;
    }
    *k = TableCoef{(const SmoothCoef *)ctx->dBlenderTab, 4, kBlenderPoints};
    return SNOWTRI_OK;
}

// ---- The smoothing entry layer.  A FILTER SOURCE says where a call's coefficients come from: one (f, z, r) for every lane
// (row N1) or the per-bone table of row N2.  Both have one shape -- ok(), Coef, coef() -- and every pass of the C ABI is
// written once over it; the exported entries below and in the N2 section only name their source and their lane count.
struct UniformFilter {
    using Coef = UniformCoef;
    double f, z, r, dt;
    bool ok() const { return f > 0.0 && dt > 0.0; }
    int coef(snowtri_ctx *, hipStream_t, Coef *k) const {
        *k = UniformCoef{smooth_coef(f, z, r, dt)};
        return SNOWTRI_OK;
    }
};
struct BoneFilter {
    using Coef = TableCoef;
    const double *fzr;   // [kBlenderPoints][3]
    double dt;
    bool ok() const {
        if (!fzr || !(dt > 0.0)) return false;
        for (int i = 0; i < kBlenderPoints; i++)
            if (!(fzr[3 * i] > 0.0)) return false;
        return true;
    }
    int coef(snowtri_ctx *ctx, hipStream_t st, Coef *k) const { return blender_table(ctx, st, fzr, dt, k); }
};
int64_t blender_lanes(int64_t n_persons) { return n_persons * kBlenderPoints * 4; }

// Every pass checks in this order: the arguments (below), an empty shard (SNOWTRI_OK before any pointer is looked at), the
// required pointers; then it enters the device, takes its coefficients, stages host arrays (a SNOWTRI_DEVICE call stages
// nothing) and runs its device function.
template <typename F>
bool smooth_args_ok(snowtri_ctx *ctx, int64_t T, int64_t n, const F &src, int memspace) {
    return ctx && T >= 0 && n >= 0 && src.ok() && (memspace == SNOWTRI_HOST || memspace == SNOWTRI_DEVICE);
}

template <typename F>
int smooth_pass_local(snowtri_ctx *ctx, const F &src, int64_t T, int64_t n, const double *x, int first, double *y, double *end_state,
                      int memspace, void *stream) {
    if (!smooth_args_ok(ctx, T, n, src, memspace)) return SNOWTRI_ERR_BAD_ARG;
    if (T == 0 || n == 0) return SNOWTRI_OK;
    if (!x || !y) return SNOWTRI_ERR_BAD_ARG;
    ENTER_DEVICE(ctx->device);
    hipStream_t st = (hipStream_t)stream;
    typename F::Coef k;
    if (int rc = src.coef(ctx, st, &k)) return rc;
    const size_t bytes = sizeof(double) * (size_t)T * n;
    Staging sg(ctx->in, ctx->out, memspace == SNOWTRI_HOST, st);
    sg.in(&x, bytes);
    sg.out(&y, bytes);
    sg.out(&end_state, sizeof(double) * 2 * n);
    if (int rc = sg.begin()) return rc;
    if (int rc = smooth_local_dev(ctx, st, T, n, x, y, first != 0, k, end_state)) return rc;
    return sg.end();
}

template <typename F>
int smooth_pass_fix(snowtri_ctx *ctx, const F &src, int64_t T, int64_t n, int first, const double *start_state, double *y, int memspace,
                    void *stream) {
    if (!smooth_args_ok(ctx, T, n, src, memspace)) return SNOWTRI_ERR_BAD_ARG;
    if (T == 0 || n == 0) return SNOWTRI_OK;
    if (!start_state || !y) return SNOWTRI_ERR_BAD_ARG;
    ENTER_DEVICE(ctx->device);
    hipStream_t st = (hipStream_t)stream;
    typename F::Coef k;
    if (int rc = src.coef(ctx, st, &k)) return rc;
    Staging sg(ctx->in, ctx->out, memspace == SNOWTRI_HOST, st);
    sg.inout(&y, sizeof(double) * (size_t)T * n);
    sg.in(&start_state, sizeof(double) * 2 * n);
    if (int rc = sg.begin()) return rc;
    if (int rc = smooth_fix_dev(ctx, st, T, n, y, first != 0, start_state, k)) return rc;
    return sg.end();
}

// The two-pass form of the sharded protocol (round 6), one k_smooth_scan pass each, device pointers.  _reduce (y and start_state
// null): the shard's zero-state end state from ONE read of x.  _scan (end_state null): the shard filtered from its true entering
// state in one more pass.
template <typename F>
int smooth_pass_scan(snowtri_ctx *ctx, const F &src, bool reduce, int64_t T, int64_t n, const double *x, int first,
                     const double *start_state, double *y, double *end_state, void *stream) {
    if (!smooth_args_ok(ctx, T, n, src, SNOWTRI_DEVICE)) return SNOWTRI_ERR_BAD_ARG;
    if (T == 0 || n == 0) return SNOWTRI_OK;
    if (!x || (reduce ? !end_state : (!y || !start_state))) return SNOWTRI_ERR_BAD_ARG;
    ENTER_DEVICE(ctx->device);
    hipStream_t st = (hipStream_t)stream;
    typename F::Coef k;
    if (int rc = src.coef(ctx, st, &k)) return rc;
    return smooth_whole_dev(ctx, st, T, n, x, y, (const double *)nullptr, k, NoHold{}, false, first ? 1 : 0, start_state, end_state);
}

template <typename F>
int smooth_pass_combine(snowtri_ctx *ctx, const F &src, int32_t world, int32_t rank, int64_t n, const double *gathered,
                        double *start_state, int memspace, void *stream) {
    if (!smooth_args_ok(ctx, 0, n, src, memspace) || world < 1 || rank < 0 || rank >= world) return SNOWTRI_ERR_BAD_ARG;
    if (n == 0) return SNOWTRI_OK;
    if (!gathered || !start_state) return SNOWTRI_ERR_BAD_ARG;
    ENTER_DEVICE(ctx->device);
    hipStream_t st = (hipStream_t)stream;
    typename F::Coef k;
    if (int rc = src.coef(ctx, st, &k)) return rc;
    Staging sg(ctx->in, ctx->out, memspace == SNOWTRI_HOST, st);
    sg.in(&gathered, sizeof(double) * (size_t)world * (4 * (size_t)n + 1));
    sg.out(&start_state, sizeof(double) * 2 * (size_t)n);
    if (int rc = sg.begin()) return rc;
    hipLaunchKernelGGL(k_smooth_combine<typename F::Coef>, dim3((unsigned)((n + kSmoothBlock - 1) / kSmoothBlock)), dim3(kSmoothBlock), 0, st,
                       (int)world, (int)rank, n, gathered, k, start_state);
    HIP_TRY(hipGetLastError());
    return sg.end();
}

// A whole uniform track (snowtri_smooth_track; skip4: the joint records of snowtri_smooth_joint_track)
int smooth_track_impl(snowtri_ctx *ctx, int64_t T, int64_t n, const double *x, const UniformFilter &src, double *y, int memspace,
                      void *stream, bool skip4) {
    if (!smooth_args_ok(ctx, T, n, src, memspace)) return SNOWTRI_ERR_BAD_ARG;
    if (T == 0 || n == 0) return SNOWTRI_OK;
    if (!x || !y) return SNOWTRI_ERR_BAD_ARG;
    ENTER_DEVICE(ctx->device);
    hipStream_t st = (hipStream_t)stream;
    UniformCoef k;
    if (int rc = src.coef(ctx, st, &k)) return rc;
    const size_t bytes = sizeof(double) * (size_t)T * n;
    Staging sg(ctx->in, ctx->out, memspace == SNOWTRI_HOST, st);
    sg.in(&x, bytes);
    sg.out(&y, bytes);
    if (int rc = sg.begin()) return rc;
    if (int rc = smooth_whole_dev(ctx, st, T, n, x, y, x, k, NoHold{}, skip4)) return rc;
    return sg.end();
}

}  // namespace

extern "C" {

int snowtri_smooth_coeffs(double f, double z, double r, double dt, double out[6]) {
    if (!out || !(f > 0.0) || !(dt > 0.0)) return SNOWTRI_ERR_BAD_ARG;
    const SmoothCoef k = smooth_coef(f, z, r, dt);
    out[0] = k.a00; out[1] = k.a01; out[2] = k.a10; out[3] = k.a11; out[4] = k.cx; out[5] = k.cxd;
    return SNOWTRI_OK;
}

int snowtri_smooth_shard_local(snowtri_ctx *ctx, int64_t T, int64_t n, const double *x, int first, double f,
                               double z, double r, double dt, double *y, double *end_state, int memspace,
                               void *stream) {
    return smooth_pass_local(ctx, UniformFilter{f, z, r, dt}, T, n, x, first, y, end_state, memspace, stream);
}

int snowtri_smooth_shard_fix(snowtri_ctx *ctx, int64_t T, int64_t n, int first, const double *start_state, double f,
                             double z, double r, double dt, double *y, int memspace, void *stream) {
    return smooth_pass_fix(ctx, UniformFilter{f, z, r, dt}, T, n, first, start_state, y, memspace, stream);
}

int snowtri_smooth_shard_reduce(snowtri_ctx *ctx, int64_t T, int64_t n, const double *x, int first, double f, double z, double r,
                                double dt, double *end_state, void *stream) {
    return smooth_pass_scan(ctx, UniformFilter{f, z, r, dt}, true, T, n, x, first, nullptr, nullptr, end_state, stream);
}

int snowtri_smooth_shard_scan(snowtri_ctx *ctx, int64_t T, int64_t n, const double *x, int first, const double *start_state, double f,
                              double z, double r, double dt, double *y, void *stream) {
    return smooth_pass_scan(ctx, UniformFilter{f, z, r, dt}, false, T, n, x, first, start_state, y, nullptr, stream);
}

int snowtri_smooth_shard_combine(snowtri_ctx *ctx, int32_t world, int32_t rank, int64_t n, const double *gathered, double f,
                                 double z, double r, double dt, double *start_state, int memspace, void *stream) {
    return smooth_pass_combine(ctx, UniformFilter{f, z, r, dt}, world, rank, n, gathered, start_state, memspace, stream);
}

int snowtri_smooth_joint_track(snowtri_ctx *ctx, int64_t T, int64_t m, const double *xyzs, double f, double z, double r,
                               double dt, double *out, int memspace, void *stream) {
    if (m < 0 || m > ((int64_t)1 << 40)) return SNOWTRI_ERR_BAD_ARG;
    return smooth_track_impl(ctx, T, 4 * m, xyzs, UniformFilter{f, z, r, dt}, out, memspace, stream, true);
}

int snowtri_smooth_track(snowtri_ctx *ctx, int64_t T, int64_t n, const double *x, double f, double z, double r,
                         double dt, double *y, int memspace, void *stream) {
    return smooth_track_impl(ctx, T, n, x, UniformFilter{f, z, r, dt}, y, memspace, stream, false);
}

}  // extern "C"

extern "C" {

// ---------------------------------------------------------------------------------------- N4
int snowtri_ctx_set_distortion(snowtri_ctx *ctx, const double *D) {
    if (!ctx || !D || ctx->C <= 0) return SNOWTRI_ERR_BAD_ARG;
    std::vector<double> lens((size_t)ctx->C * kLensStride, 0.0);
    for (int c = 0; c < ctx->C; c++) {
        const double *K = &ctx->hK[9 * (size_t)c];
        if (!pinhole_K(K)) return SNOWTRI_ERR_BAD_ARG;
        double *L = &lens[(size_t)c * kLensStride];
        L[0] = K[0]; L[1] = K[1]; L[2] = K[2]; L[3] = K[4]; L[4] = K[5];
        L[5] = 1.0 / K[0]; L[6] = 1.0 / K[4];
        for (int i = 0; i < 5; i++) {
            if (!std::isfinite(D[5 * c + i])) return SNOWTRI_ERR_BAD_ARG;
            L[7 + i] = D[5 * c + i];
        }
    }
    ENTER_DEVICE(ctx->device);
    if (!ctx->dLens) HIP_TRY(hipMalloc(&ctx->dLens, sizeof(double) * lens.size()));
    HIP_TRY(hipMemcpy(ctx->dLens, lens.data(), sizeof(double) * lens.size(), hipMemcpyHostToDevice));
    for (int c = 0; c < ctx->C; c++)   // the same coefficients for the forward direction (SNOWTRI_REPROJECT_RAW)
        std::memcpy(&ctx->hProj[(size_t)c * kProjStride + 17], D + 5 * c, sizeof(double) * 5);
    HIP_TRY(hipMemcpy(ctx->dProj, ctx->hProj.data(), sizeof(double) * ctx->hProj.size(), hipMemcpyHostToDevice));
    return SNOWTRI_OK;
}

int snowtri_undistort_keypoints(snowtri_ctx *ctx, int64_t F, int32_t Pmax, int32_t J, const void *kpts_in,
                                void *kpts_out, int dtype, int memspace, void *stream) {
    if (!ctx || F < 0 || Pmax <= 0 || J <= 0 || (dtype != SNOWTRI_F32 && dtype != SNOWTRI_F64) ||
        (memspace != SNOWTRI_HOST && memspace != SNOWTRI_DEVICE) || ctx->C <= 0 || !ctx->dLens)
        return SNOWTRI_ERR_BAD_ARG;
    if (F == 0) return SNOWTRI_OK;
    if (!kpts_in || !kpts_out) return SNOWTRI_ERR_BAD_ARG;
    ENTER_DEVICE(ctx->device);
    hipStream_t st = (hipStream_t)stream;
    const int64_t per_cam = (int64_t)Pmax * J, n_obs = F * ctx->C * per_cam;
    if (per_cam > INT32_MAX) return SNOWTRI_ERR_BAD_ARG;
    const size_t bytes = (size_t)n_obs * 3 * (dtype == SNOWTRI_F32 ? 4 : 8);
    const void *din = kpts_in;
    void *dout = kpts_out;
    Staging sg(ctx->in, ctx->out, memspace == SNOWTRI_HOST, st);
    sg.in(&din, bytes);
    sg.out(&dout, bytes);
    if (int rc = sg.begin()) return rc;
    const dim3 grid((unsigned)((n_obs + 255) / 256));
    if (dtype == SNOWTRI_F32)
        hipLaunchKernelGGL(k_undistort<float>, grid, dim3(256), 0, st, n_obs, (int)ctx->C, (int)per_cam,
                           (const double *)ctx->dLens, (const float *)din, (float *)dout);
    else
        hipLaunchKernelGGL(k_undistort<double>, grid, dim3(256), 0, st, n_obs, (int)ctx->C, (int)per_cam,
                           (const double *)ctx->dLens, (const double *)din, (double *)dout);
    HIP_TRY(hipGetLastError());
    return sg.end();
}

// ---------------------------------------------------------------------------------------- N2
int snowtri_blender_points(snowtri_ctx *ctx, int64_t n, int32_t keypoint_num, const void *xyzs, int xyz_dtype,
                           double *out_points, uint8_t *out_valid, int memspace, void *stream) {
    if (!ctx || n < 0 || (xyz_dtype != SNOWTRI_F32 && xyz_dtype != SNOWTRI_F64) ||
        (memspace != SNOWTRI_HOST && memspace != SNOWTRI_DEVICE))
        return SNOWTRI_ERR_BAD_ARG;
    if (keypoint_num < kBlenderMinJoints) return SNOWTRI_ERR_BAD_INDEX;  // person[129] would raise IndexError
    if (n == 0) return SNOWTRI_OK;
    if (!xyzs || !out_points || !out_valid) return SNOWTRI_ERR_BAD_ARG;
    ENTER_DEVICE(ctx->device);
    hipStream_t st = (hipStream_t)stream;
    const size_t esz = xyz_dtype == SNOWTRI_F32 ? 4 : 8;
    const size_t in_bytes = esz * 4 * (size_t)keypoint_num * n, pt_bytes = sizeof(double) * 4 * kBlenderPoints * n;
    const void *dx = xyzs;
    double *dp = out_points;
    uint8_t *dv = out_valid;
    Staging sg(ctx->in, ctx->out, memspace == SNOWTRI_HOST, st);
    sg.in(&dx, in_bytes);
    sg.out(&dp, pt_bytes);
    sg.out(&dv, (size_t)kBlenderPoints * n);
    if (int rc = sg.begin()) return rc;
    const dim3 grid((unsigned)((n + 255) / 256));
    if (xyz_dtype == SNOWTRI_F32)
        hipLaunchKernelGGL(k_blender_points<float>, grid, dim3(256), 0, st, n, (int)keypoint_num, (const float *)dx, dp, dv);
    else
        hipLaunchKernelGGL(k_blender_points<double>, grid, dim3(256), 0, st, n, (int)keypoint_num, (const double *)dx, dp, dv);
    HIP_TRY(hipGetLastError());
    return sg.end();
}

// The hold's scratch in ctx->aux for n lanes over the filter's nchunks chunks: [4096 bytes | H | start | Hf | entering], with
// H and start [max(1, nchunks)][n] doubles, Hf as many bytes and entering [n] doubles on a 256-byte boundary.
struct HoldScratch {
    double *H, *start;
    uint8_t *Hf;
    double *entering;
};
static int hold_scratch(snowtri_ctx *ctx, int64_t nchunks, int64_t n, HoldScratch *hs) {
    const size_t cn = (size_t)std::max<int64_t>(1, nchunks) * n;
    const size_t off_H = 4096, off_start = off_H + sizeof(double) * cn, off_Hf = off_start + sizeof(double) * cn,
                 off_ent = (off_Hf + cn + 255) & ~(size_t)255;
    int rc = ctx->aux.ensure(off_ent + sizeof(double) * (size_t)n);
    if (rc) return rc;
    char *aux = (char *)ctx->aux.p;
    *hs = HoldScratch{(double *)(aux + off_H), (double *)(aux + off_start), (uint8_t *)(aux + off_Hf), (double *)(aux + off_ent)};
    return SNOWTRI_OK;
}

// ---- N2 on a FRAME-SHARDED track (device pointers only; include/snowtri.h describes the protocol)
int snowtri_blender_hold_shard_last(snowtri_ctx *ctx, int64_t T, int64_t n_persons, const double *points, const uint8_t *valid,
                                    double *payload, void *stream) {
    if (!ctx || T < 0 || n_persons < 0 || !payload) return SNOWTRI_ERR_BAD_ARG;
    const int64_t n = blender_lanes(n_persons);
    if (n == 0) return SNOWTRI_OK;
    ENTER_DEVICE(ctx->device);
    hipStream_t st = (hipStream_t)stream;
    if (T == 0) {   // an empty shard: nothing found
        HIP_TRY(hipMemsetAsync(payload, 0, sizeof(double) * 2 * (size_t)n, st));
        return SNOWTRI_OK;
    }
    if (!points || !valid) return SNOWTRI_ERR_BAD_ARG;
    hipLaunchKernelGGL(k_hold_block_last, smooth_grid(n, 1), dim3(256), 0, st, T, n, 4, points, valid, payload);
    HIP_TRY(hipGetLastError());
    return SNOWTRI_OK;
}

int snowtri_blender_hold_shard_apply(snowtri_ctx *ctx, int32_t world, int32_t rank, int64_t T, int64_t n_persons, const double *points,
                                     const uint8_t *valid, const double *gathered, double *held, void *stream) {
    if (!ctx || T < 0 || n_persons < 0 || world < 1 || rank < 0 || rank >= world) return SNOWTRI_ERR_BAD_ARG;
    const int64_t n = blender_lanes(n_persons);
    if (T == 0 || n == 0) return SNOWTRI_OK;
    if (!points || !valid || !gathered || !held) return SNOWTRI_ERR_BAD_ARG;
    ENTER_DEVICE(ctx->device);
    hipStream_t st = (hipStream_t)stream;
    const int64_t nchunks = (T - 1 + kSmoothChunk - 1) / kSmoothChunk;   // the filter's chunks: frames 1 .. T-1
    if (nchunks + 1 > 65535) return SNOWTRI_ERR_BAD_ARG;   // (k_hold_fill runs nchunks + 1 block rows: checked BEFORE anything is queued)
    HoldScratch h;
    if (int rc = hold_scratch(ctx, nchunks, n, &h)) return rc;
    const dim3 g1 = smooth_grid(n, 1);
    hipLaunchKernelGGL(k_hold_entering, g1, dim3(256), 0, st, (int)world, (int)rank, n, gathered, h.entering);
    if (nchunks > 0)
        hipLaunchKernelGGL(k_hold_last, smooth_grid(n, nchunks), dim3(256), 0, st, T, n, kSmoothChunk, 4, points, valid, h.H, h.Hf);
    hipLaunchKernelGGL(k_hold_carry, g1, dim3(256), 0, st, n, nchunks, 4, points, valid, (const double *)h.H, (const uint8_t *)h.Hf, h.start,
                       (const double *)h.entering);
    hipLaunchKernelGGL(k_hold_fill, smooth_grid(n, nchunks + 1), dim3(256), 0, st, T, n, kSmoothChunk, 4, points, valid,
                       (const double *)h.start, (const double *)h.entering, held);
    HIP_TRY(hipGetLastError());
    return SNOWTRI_OK;
}

// the per-bone passes: the smoothing entry layer of row N1 over BoneFilter, device pointers
int snowtri_blender_smooth_shard_local(snowtri_ctx *ctx, int64_t T, int64_t n_persons, const double *held, int first, const double *fzr,
                                       double dt, double *y, double *end_state, void *stream) {
    return smooth_pass_local(ctx, BoneFilter{fzr, dt}, T, blender_lanes(n_persons), held, first, y, end_state, SNOWTRI_DEVICE, stream);
}

int snowtri_blender_smooth_shard_reduce(snowtri_ctx *ctx, int64_t T, int64_t n_persons, const double *held, int first, const double *fzr,
                                        double dt, double *end_state, void *stream) {
    return smooth_pass_scan(ctx, BoneFilter{fzr, dt}, true, T, blender_lanes(n_persons), held, first, nullptr, nullptr, end_state, stream);
}

int snowtri_blender_smooth_shard_scan(snowtri_ctx *ctx, int64_t T, int64_t n_persons, const double *held, int first, const double *start_state,
                                      const double *fzr, double dt, double *y, void *stream) {
    return smooth_pass_scan(ctx, BoneFilter{fzr, dt}, false, T, blender_lanes(n_persons), held, first, start_state, y, nullptr, stream);
}

int snowtri_blender_smooth_shard_combine(snowtri_ctx *ctx, int32_t world, int32_t rank, int64_t n_persons, const double *gathered,
                                         const double *fzr, double dt, double *start_state, void *stream) {
    return smooth_pass_combine(ctx, BoneFilter{fzr, dt}, world, rank, blender_lanes(n_persons), gathered, start_state, SNOWTRI_DEVICE, stream);
}

int snowtri_blender_smooth_shard_fix(snowtri_ctx *ctx, int64_t T, int64_t n_persons, int first, const double *start_state, const double *fzr,
                                     double dt, double *y, void *stream) {
    return smooth_pass_fix(ctx, BoneFilter{fzr, dt}, T, blender_lanes(n_persons), first, start_state, y, SNOWTRI_DEVICE, stream);
}

int snowtri_blender_smooth(snowtri_ctx *ctx, int64_t T, int64_t n_persons, const double *points,
                           const uint8_t *valid, const double *fzr, double dt, double *out, int memspace,
                           void *stream) {
    const BoneFilter src{fzr, dt};
    const int64_t n = blender_lanes(n_persons), nv = n_persons * kBlenderPoints;
    if (!smooth_args_ok(ctx, T, n, src, memspace)) return SNOWTRI_ERR_BAD_ARG;
    if (T == 0 || n == 0) return SNOWTRI_OK;
    if (!points || !valid || !out) return SNOWTRI_ERR_BAD_ARG;
    ENTER_DEVICE(ctx->device);
    hipStream_t st = (hipStream_t)stream;
    const int64_t nchunks = (T - 1 + kSmoothChunk - 1) / kSmoothChunk;  // the filter's chunks: frames 1..T-1
    if (nchunks > 65535) return SNOWTRI_ERR_BAD_ARG;
    const size_t bytes = sizeof(double) * (size_t)T * n;
    HoldScratch h;
    if (int rc = hold_scratch(ctx, nchunks, n, &h)) return rc;
    TableCoef k;
    if (int rc = src.coef(ctx, st, &k)) return rc;
    const double *dx = points;
    const uint8_t *dv = valid;
    double *dy = out;
    Staging sg(ctx->in, ctx->out, memspace == SNOWTRI_HOST, st);
    sg.in(&dx, bytes);
    sg.in(&dv, (size_t)T * nv);
    sg.out(&dy, bytes);
    if (int rc = sg.begin()) return rc;
    if (nchunks > 0)
        hipLaunchKernelGGL(k_hold_last, smooth_grid(n, nchunks), dim3(256), 0, st, T, n, kSmoothChunk, 4, dx, dv, h.H, h.Hf);
    hipLaunchKernelGGL(k_hold_carry, smooth_grid(n, 1), dim3(256), 0, st, n, nchunks, 4, dx, dv, (const double *)h.H, (const uint8_t *)h.Hf,
                       h.start);
    HIP_TRY(hipGetLastError());
    const HoldInput hs{dv, (const double *)h.start, 4};
    // frame 0 is returned as given, NaNs included (blender.py:176); the filters are seeded with the held row
    if (int rc = smooth_whole_dev(ctx, st, T, n, dx, dy, (const double *)h.start, k, hs)) return rc;
    return sg.end();
}

// ------------------------------------------------------------------------------- person tracking
static int arg_fail(int status, const char *msg) {
    g_last_error = msg;
    return status;
}

size_t snowtri_track_state_bytes(int32_t S) { return (S < 1 || S > kTrackMax) ? 0 : track_state_bytes(S); }
int snowtri_track_block_frames(void) { return kTrackBlockFrames; }

int snowtri_track_persons(snowtri_ctx *ctx, int64_t F, int32_t Pout_max, int32_t keypoint_num, const void *xyzs, int xyz_dtype,
                          const int32_t *count, int32_t S, int32_t center_point_index, double gate, int32_t max_missed, void *state,
                          int32_t *slot_of, int32_t *person_of, int32_t *track_id, uint32_t *flags, int memspace, void *stream) {
    if (!ctx) return arg_fail(SNOWTRI_ERR_BAD_ARG, "snowtri_track_persons: null context");
    if ((xyz_dtype != SNOWTRI_F32 && xyz_dtype != SNOWTRI_F64) || (memspace != SNOWTRI_HOST && memspace != SNOWTRI_DEVICE))
        return arg_fail(SNOWTRI_ERR_BAD_ARG, "snowtri_track_persons: unknown dtype or memory space");
    if (F < 0 || keypoint_num < 1) return arg_fail(SNOWTRI_ERR_BAD_ARG, "snowtri_track_persons: F < 0 or keypoint_num < 1");
    if (S < 1 || S > kTrackMax || Pout_max < 1 || Pout_max > kTrackMax)
        return arg_fail(SNOWTRI_ERR_BAD_ARG, "snowtri_track_persons: S and Pout_max must lie in 1..16");
    if (!(gate >= 0.0) || !std::isfinite(gate)) return arg_fail(SNOWTRI_ERR_BAD_ARG, "snowtri_track_persons: gate must be finite and >= 0");
    if (max_missed < 0) return arg_fail(SNOWTRI_ERR_BAD_ARG, "snowtri_track_persons: max_missed must be >= 0");
    if (center_point_index < 0 || center_point_index >= keypoint_num)
        return arg_fail(SNOWTRI_ERR_BAD_INDEX, "snowtri_track_persons: center_point_index outside [0, keypoint_num)");
    if (F == 0) return SNOWTRI_OK;
    if (!xyzs || !count || !slot_of || !person_of || !track_id) return arg_fail(SNOWTRI_ERR_BAD_ARG, "snowtri_track_persons: null array");
    if (memspace == SNOWTRI_DEVICE && (((uintptr_t)xyzs & 15u) || (state && ((uintptr_t)state & 7u))))
        return arg_fail(SNOWTRI_ERR_BAD_ARG, "snowtri_track_persons: xyzs must be aligned to 16 bytes, state to 8");
    ENTER_DEVICE(ctx->device);
    hipStream_t st = (hipStream_t)stream;
    const int P = Pout_max;
    const size_t esz = dtype_size(xyz_dtype);
    const size_t x_bytes = esz * 4 * (size_t)keypoint_num * P * F, c_bytes = sizeof(int32_t) * (size_t)F;
    const size_t so_bytes = sizeof(int32_t) * (size_t)F * P, po_bytes = sizeof(int32_t) * (size_t)F * S, st_bytes = track_state_bytes(S);
    if (int rc = ctx->track.ensure(sizeof(double) * 4 * (size_t)F * P)) return rc;
    if ((int64_t)F * P > (int64_t)0x7fffffff * 256) return arg_fail(SNOWTRI_ERR_BAD_ARG, "snowtri_track_persons: too many frames for one call");
    const void *dx = xyzs;
    const int32_t *dc = count;
    int32_t *d_so = slot_of, *d_po = person_of, *d_id = track_id;
    uint32_t *d_fl = flags;
    unsigned char *d_state = (unsigned char *)state;
    Staging sg(ctx->in, ctx->out, memspace == SNOWTRI_HOST, st);
    sg.in(&dx, x_bytes);
    sg.in(&dc, c_bytes);
    sg.out(&d_so, so_bytes);
    sg.out(&d_po, po_bytes);
    sg.out(&d_id, po_bytes);
    sg.out(&d_fl, c_bytes);
    sg.inout(&d_state, st_bytes);
    if (int rc = sg.begin()) return rc;
    double *d_cen = (double *)ctx->track.p;
    const dim3 grid((unsigned)(((int64_t)F * P + 255) / 256));
    const bool timed = ctx->timing;
    ctx->track_ev_valid = false;
    if (timed) {
        for (auto &e : ctx->track_ev)
            if (!e) HIP_TRY(hipEventCreate(&e));
        HIP_TRY(hipEventRecord(ctx->track_ev[0], st));
    }
    if (xyz_dtype == SNOWTRI_F32)
        hipLaunchKernelGGL(k_track_centres<float>, grid, dim3(256), 0, st, F, P, (int)keypoint_num, (int)center_point_index, (const float *)dx, dc, d_cen);
    else
        hipLaunchKernelGGL(k_track_centres<double>, grid, dim3(256), 0, st, F, P, (int)keypoint_num, (int)center_point_index, (const double *)dx, dc, d_cen);
    if (timed) HIP_TRY(hipEventRecord(ctx->track_ev[1], st));
    hipLaunchKernelGGL(k_track_chain, dim3(1), dim3(kTrackChainThreads), 0, st, F, P, (int)S, gate * gate, (int)max_missed, (const double *)d_cen, d_state,
                       d_so, d_po, d_id, d_fl);
    HIP_TRY(hipGetLastError());
    if (timed) {
        HIP_TRY(hipEventRecord(ctx->track_ev[2], st));
        ctx->track_ev_valid = true;
    }
    return sg.end();
}

int snowtri_track_last_ms(snowtri_ctx *ctx, float kernel_ms[2]) {
    if (!ctx || !kernel_ms) return SNOWTRI_ERR_BAD_ARG;
    kernel_ms[0] = kernel_ms[1] = 0.f;
    if (!ctx->track_ev_valid) return SNOWTRI_ERR_BAD_ARG;
    ENTER_DEVICE(ctx->device);
    HIP_TRY(hipEventSynchronize(ctx->track_ev[2]));
    HIP_TRY(hipEventElapsedTime(&kernel_ms[0], ctx->track_ev[0], ctx->track_ev[1]));
    HIP_TRY(hipEventElapsedTime(&kernel_ms[1], ctx->track_ev[1], ctx->track_ev[2]));
    return SNOWTRI_OK;
}

int snowtri_track_gather(snowtri_ctx *ctx, int64_t F, int32_t Pout_max, int32_t keypoint_num, const void *xyzs, int xyz_dtype, int32_t S,
                         const int32_t *person_of, void *xyzs_tracked, int memspace, void *stream) {
    if (!ctx) return arg_fail(SNOWTRI_ERR_BAD_ARG, "snowtri_track_gather: null context");
    if ((xyz_dtype != SNOWTRI_F32 && xyz_dtype != SNOWTRI_F64) || (memspace != SNOWTRI_HOST && memspace != SNOWTRI_DEVICE))
        return arg_fail(SNOWTRI_ERR_BAD_ARG, "snowtri_track_gather: unknown dtype or memory space");
    if (F < 0 || keypoint_num < 1) return arg_fail(SNOWTRI_ERR_BAD_ARG, "snowtri_track_gather: F < 0 or keypoint_num < 1");
    if (S < 1 || S > kTrackMax || Pout_max < 1 || Pout_max > kTrackMax)
        return arg_fail(SNOWTRI_ERR_BAD_ARG, "snowtri_track_gather: S and Pout_max must lie in 1..16");
    if (F == 0) return SNOWTRI_OK;
    if (!xyzs || !person_of || !xyzs_tracked) return arg_fail(SNOWTRI_ERR_BAD_ARG, "snowtri_track_gather: null array");
    if (memspace == SNOWTRI_DEVICE && ((((uintptr_t)xyzs) | ((uintptr_t)xyzs_tracked)) & 15u))
        return arg_fail(SNOWTRI_ERR_BAD_ARG, "snowtri_track_gather: xyzs and xyzs_tracked must be aligned to 16 bytes");
    ENTER_DEVICE(ctx->device);
    hipStream_t st = (hipStream_t)stream;
    const size_t person_bytes = dtype_size(xyz_dtype) * 4 * (size_t)keypoint_num;
    const size_t x_bytes = person_bytes * Pout_max * F, o_bytes = person_bytes * S * F, po_bytes = sizeof(int32_t) * (size_t)F * S;
    const void *dx = xyzs;
    const int32_t *d_po = person_of;
    void *d_out = xyzs_tracked;
    Staging sg(ctx->in, ctx->out, memspace == SNOWTRI_HOST, st);
    sg.in(&dx, x_bytes);
    sg.in(&d_po, po_bytes);
    sg.out(&d_out, o_bytes);
    if (int rc = sg.begin()) return rc;
    const int rec_per_person = (int)(person_bytes / 16);
    const int64_t total = (int64_t)F * S * rec_per_person;
    hipLaunchKernelGGL(k_track_gather, dim3(grid_for(total, 256, ctx->num_cus * 16)), dim3(256), 0, st, F, (int)Pout_max, (int)S, rec_per_person,
                       (const uint4 *)dx, d_po, (uint4 *)d_out);
    HIP_TRY(hipGetLastError());
    return sg.end();
}

}  // extern "C"

// ------------------------------------------------------------------------------- record passes: gap filling, despiking
namespace {

// A refusal by the entry point `who`: "<who>: <what>" is what snowtri_last_error() then says.  -> the status.
struct Refuse {
    const char *who;
    int operator()(const char *what, int status = SNOWTRI_ERR_BAD_ARG) const { return arg_fail(status, (std::string(who) + ": " + what).c_str()); }
};

// The host side of a pass xyzs[T][m][4] -> out[T][m][4] (+ codes[T][m], may be null) over a track of joint records, after the
// entry point `who` has checked its context and its own parameters: every other refusal (nothing is written or enqueued on one),
// an empty track (OK before any pointer is looked at), the staging of host arrays through ctx->in / ctx->out, and between the
// two halves of that launch(grid, block, st, ncols, dx, d_out, d_codes) for the kernel.
template <typename Launch>
int record_pass(const char *who, snowtri_ctx *ctx, int64_t T, int64_t m, const void *xyzs, int xyz_dtype, void *out, uint8_t *codes, int memspace,
                void *stream, Launch launch) {
    const Refuse refuse{who};
    if (xyz_dtype != SNOWTRI_F32 && xyz_dtype != SNOWTRI_F64) return refuse("unknown xyz_dtype");
    if (memspace != SNOWTRI_HOST && memspace != SNOWTRI_DEVICE) return refuse("unknown memspace");
    if (T < 0 || m < 0) return refuse("T < 0 or m < 0");
    if (T == 0 || m == 0) return SNOWTRI_OK;
    if (!xyzs || !out) return refuse("null array (xyzs or out)");
    // one workgroup per 64 lanes x (kRecWaves * kRecBlockFrames) frames on a one-dimensional grid; 64-bit byte offsets of 32-byte records
    const int64_t wg_frames = (int64_t)kRecWaves * kRecBlockFrames;
    const int64_t ncols = (m + 63) / 64, nrows = (T + wg_frames - 1) / wg_frames;
    if (T > ((int64_t)1 << 58) / m) return refuse("T * m must not exceed 2^58 records");
    if (nrows > (int64_t)0x7fffffff / ncols) return refuse("ceil(T / 256) * ceil(m / 64) must not exceed 2^31 - 1 workgroups");
    const size_t bytes = dtype_size(xyz_dtype) * 4 * (size_t)T * (size_t)m, c_bytes = (size_t)T * (size_t)m;
    if (memspace == SNOWTRI_DEVICE && ((((uintptr_t)xyzs) | ((uintptr_t)out)) & 15u)) return refuse("xyzs and out must be aligned to 16 bytes");
    // (a neighbouring tile reads through xyzs what this one writes through out)
    if ((uintptr_t)xyzs < (uintptr_t)out + bytes && (uintptr_t)out < (uintptr_t)xyzs + bytes) return refuse("out must not overlap xyzs");
    ENTER_DEVICE(ctx->device);
    hipStream_t st = (hipStream_t)stream;
    const void *dx = xyzs;
    void *d_out = out;
    uint8_t *d_codes = codes;
    Staging sg(ctx->in, ctx->out, memspace == SNOWTRI_HOST, st);
    sg.in(&dx, bytes);
    sg.out(&d_out, bytes);
    sg.out(&d_codes, c_bytes);
    if (int rc = sg.begin()) return rc;
    launch(dim3((unsigned)(ncols * nrows)), dim3(64, kRecWaves), st, ncols, (const uint4 *)dx, (uint4 *)d_out, d_codes);
    HIP_TRY(hipGetLastError());
    return sg.end();
}

template <typename IO>
void launch_despike(int half_window, dim3 grid, dim3 block, hipStream_t st, int64_t T, int64_t m, double tol2, int mode, int64_t ncols,
                    const uint4 *dx, uint4 *d_out, uint8_t *d_codes) {
    switch (half_window) {
    case 1: hipLaunchKernelGGL((k_despike<IO, 1>), grid, block, 0, st, T, m, tol2, mode, ncols, dx, d_out, d_codes); break;
    case 2: hipLaunchKernelGGL((k_despike<IO, 2>), grid, block, 0, st, T, m, tol2, mode, ncols, dx, d_out, d_codes); break;
    case 3: hipLaunchKernelGGL((k_despike<IO, 3>), grid, block, 0, st, T, m, tol2, mode, ncols, dx, d_out, d_codes); break;
    default: hipLaunchKernelGGL((k_despike<IO, 4>), grid, block, 0, st, T, m, tol2, mode, ncols, dx, d_out, d_codes); break;
    }
}

}  // namespace

extern "C" {

int snowtri_fill_block_frames(void) { return kRecBlockFrames; }
int snowtri_despike_block_frames(void) { return kRecBlockFrames; }

int snowtri_fill_joint_track(snowtri_ctx *ctx, int64_t T, int64_t m, const void *xyzs, int xyz_dtype, int32_t max_gap, void *out, uint8_t *fill,
                             int memspace, void *stream) {
    if (!ctx) return arg_fail(SNOWTRI_ERR_BAD_ARG, "snowtri_fill_joint_track: null context");
    if (max_gap < 1 || max_gap > kFillMaxGap) return arg_fail(SNOWTRI_ERR_BAD_ARG, "snowtri_fill_joint_track: max_gap must lie in 1..255");
    return record_pass("snowtri_fill_joint_track", ctx, T, m, xyzs, xyz_dtype, out, fill, memspace, stream,
                       [=](dim3 grid, dim3 block, hipStream_t st, int64_t ncols, const uint4 *dx, uint4 *d_out, uint8_t *d_fill) {
                           if (xyz_dtype == SNOWTRI_F32)
                               hipLaunchKernelGGL(k_fill_gaps<float>, grid, block, 0, st, T, m, (int)max_gap, ncols, dx, d_out, d_fill);
                           else
                               hipLaunchKernelGGL(k_fill_gaps<double>, grid, block, 0, st, T, m, (int)max_gap, ncols, dx, d_out, d_fill);
                       });
}

int snowtri_despike_joint_track(snowtri_ctx *ctx, int64_t T, int64_t m, const void *xyzs, int xyz_dtype, int32_t half_window, double tol,
                                int32_t mode, void *out, uint8_t *codes, int memspace, void *stream) {
    if (!ctx) return arg_fail(SNOWTRI_ERR_BAD_ARG, "snowtri_despike_joint_track: null context");
    if (half_window < 1 || half_window > kDespikeMaxHalf)
        return arg_fail(SNOWTRI_ERR_BAD_ARG, "snowtri_despike_joint_track: half_window must lie in 1..4");
    if (!(tol >= 0.0)) return arg_fail(SNOWTRI_ERR_BAD_ARG, "snowtri_despike_joint_track: tol must be >= 0 and not NaN");
    if (mode != SNOWTRI_DESPIKE_MARK && mode != SNOWTRI_DESPIKE_REPLACE) return arg_fail(SNOWTRI_ERR_BAD_ARG, "snowtri_despike_joint_track: unknown mode");
    const double tol2 = tol * tol;   // formed once, in fp64
    return record_pass("snowtri_despike_joint_track", ctx, T, m, xyzs, xyz_dtype, out, codes, memspace, stream,
                       [=](dim3 grid, dim3 block, hipStream_t st, int64_t ncols, const uint4 *dx, uint4 *d_out, uint8_t *d_codes) {
                           if (xyz_dtype == SNOWTRI_F32)
                               launch_despike<float>((int)half_window, grid, block, st, T, m, tol2, (int)mode, ncols, dx, d_out, d_codes);
                           else
                               launch_despike<double>((int)half_window, grid, block, st, T, m, tol2, (int)mode, ncols, dx, d_out, d_codes);
                       });
}

}  // extern "C"

// ------------------------------------------------------------------------------- reprojection
namespace {

// What snowtri_reproject and snowtri_reproject_cost check alike, before anything is enqueued or written.  -> 0, or the status.
int reproject_args(const char *who, snowtri_ctx *ctx, int64_t F, int32_t P, int32_t kn, int xyz_dtype, uint32_t flags, int other_dtype,
                   int memspace) {
    const Refuse refuse{who};
    if (!ctx) return refuse("null context");
    if (ctx->C <= 0) return refuse("the context has no cameras");
    if ((xyz_dtype != SNOWTRI_F32 && xyz_dtype != SNOWTRI_F64) || (other_dtype != SNOWTRI_F32 && other_dtype != SNOWTRI_F64))
        return refuse("unknown dtype");
    if (memspace != SNOWTRI_HOST && memspace != SNOWTRI_DEVICE) return refuse("unknown memspace");
    if (flags & ~(uint32_t)SNOWTRI_REPROJECT_RAW) return refuse("unknown flag bit");
    if (F < 0 || P < 1 || kn < 1) return refuse("F < 0, P < 1 or kn < 1");
    for (int c = 0; c < ctx->C; c++)
        if (!pinhole_K(&ctx->hK[9 * (size_t)c])) return refuse("K must be [[fx, s, cx], [0, fy, cy], [0, 0, 1]] for every camera");
    if ((flags & SNOWTRI_REPROJECT_RAW) && !ctx->dLens) return refuse("SNOWTRI_REPROJECT_RAW needs snowtri_ctx_set_distortion first");
    return 0;
}

// fn(a, b) with two zero values whose TYPES are the pair that two SNOWTRI_F32 / SNOWTRI_F64 codes name: a generic lambda takes
// them with decltype and launches the kernel instantiated for that pair.
template <typename Fn>
void with_float_pair(int dtype_a, int dtype_b, Fn fn) {
    if (dtype_a == SNOWTRI_F32) {
        if (dtype_b == SNOWTRI_F32) fn(float(), float());
        else fn(float(), double());
    } else {
        if (dtype_b == SNOWTRI_F32) fn(double(), float());
        else fn(double(), double());
    }
}

}  // namespace

extern "C" {

int snowtri_reproject(snowtri_ctx *ctx, int64_t F, int32_t P, int32_t kn, const void *xyzs, int xyz_dtype, uint32_t flags, void *pix,
                      int pix_dtype, int memspace, void *stream) {
    const char *who = "snowtri_reproject";
    if (int rc = reproject_args(who, ctx, F, P, kn, xyz_dtype, flags, pix_dtype, memspace)) return rc;
    const Refuse refuse{who};
    // one lane per observation, 256 per workgroup on a one-dimensional grid; 64-bit element offsets
    if (F == 0) return SNOWTRI_OK;
    const int64_t max_obs = (int64_t)0x7fffffff * 256, per_person_frame = (int64_t)P * kn;   // (two int32: no overflow)
    if (per_person_frame > max_obs / ctx->C || F > max_obs / (per_person_frame * ctx->C))
        return refuse("F * C * P * kn must not exceed (2^31 - 1) * 256 observations");
    const int64_t per_frame = per_person_frame * ctx->C;
    if (!xyzs || !pix) return refuse("null array (xyzs or pix)");
    if (memspace == SNOWTRI_DEVICE && ((((uintptr_t)xyzs) & (dtype_size(xyz_dtype) - 1)) || (((uintptr_t)pix) & (dtype_size(pix_dtype) - 1))))
        return refuse("xyzs and pix must be aligned to their element size");
    ENTER_DEVICE(ctx->device);
    hipStream_t st = (hipStream_t)stream;
    const int64_t n_obs = F * per_frame;
    const size_t x_bytes = dtype_size(xyz_dtype) * 4 * (size_t)F * P * kn, p_bytes = dtype_size(pix_dtype) * 3 * (size_t)n_obs;
    const void *dx = xyzs;
    void *dp = pix;
    Staging sg(ctx->in, ctx->out, memspace == SNOWTRI_HOST, st);
    sg.in(&dx, x_bytes);
    sg.out(&dp, p_bytes);
    if (int rc = sg.begin()) return rc;
    const dim3 grid((unsigned)((n_obs + 255) / 256));
    const int raw = (flags & SNOWTRI_REPROJECT_RAW) ? 1 : 0;
    with_float_pair(xyz_dtype, pix_dtype, [&](auto tx, auto tp) {
        using TX = decltype(tx);
        using TP = decltype(tp);
        hipLaunchKernelGGL((k_reproject<TX, TP>), grid, dim3(256), 0, st, n_obs, (int)ctx->C, (int)P, (int)kn, raw, (const double *)ctx->dProj,
                           (const TX *)dx, (TP *)dp);
    });
    HIP_TRY(hipGetLastError());
    return sg.end();
}

int snowtri_reproject_cost(snowtri_ctx *ctx, int64_t F, int32_t P, int32_t kn, const void *xyzs, int xyz_dtype, int32_t Pmax, const void *kpts,
                           int kpts_dtype, const int32_t *n_persons, double keypoint_score_threshold, uint32_t flags, double *cost_sum,
                           int32_t *cost_n, int memspace, void *stream) {
    const char *who = "snowtri_reproject_cost";
    if (int rc = reproject_args(who, ctx, F, P, kn, xyz_dtype, flags, kpts_dtype, memspace)) return rc;
    const Refuse refuse{who};
    if (Pmax < 1) return refuse("Pmax < 1");
    if (kn > kCostMaxJoints) return refuse("kn must not exceed 256 joints (four per lane of the wave that owns a person)");
    if (keypoint_score_threshold != keypoint_score_threshold) return refuse("keypoint_score_threshold is NaN");
    // one wave per (f, c, p), four per workgroup on a one-dimensional grid; 64-bit element offsets
    if (F == 0) return SNOWTRI_OK;
    const int64_t max_items = (int64_t)0x7fffffff * kCostWaves, cp = (int64_t)ctx->C * P;   // (two int32: no overflow)
    if (cp > max_items || F > max_items / cp || Pmax > ((int64_t)1 << 48) / (F * cp))
        return refuse("F * C * P must not exceed (2^31 - 1) * 4 persons in view, F * C * P * Pmax 2^48 costs");
    if (!xyzs || !kpts || !cost_sum || !cost_n) return refuse("null array (xyzs, kpts, cost_sum or cost_n)");
    if (memspace == SNOWTRI_DEVICE && ((((uintptr_t)xyzs) & (dtype_size(xyz_dtype) - 1)) || (((uintptr_t)kpts) & (dtype_size(kpts_dtype) - 1)) ||
                                       (((uintptr_t)cost_sum) & 7u) || (((uintptr_t)cost_n) & 3u) || (((uintptr_t)n_persons) & 3u)))
        return refuse("xyzs, kpts, n_persons, cost_sum and cost_n must be aligned to their element size");
    ENTER_DEVICE(ctx->device);
    hipStream_t st = (hipStream_t)stream;
    const int64_t n_items = F * cp, n_cost = n_items * Pmax;
    const size_t x_bytes = dtype_size(xyz_dtype) * 4 * (size_t)F * P * kn, k_bytes = dtype_size(kpts_dtype) * 3 * (size_t)F * ctx->C * Pmax * kn;
    const size_t np_bytes = sizeof(int32_t) * (size_t)F * ctx->C, s_bytes = sizeof(double) * (size_t)n_cost, n_bytes = sizeof(int32_t) * (size_t)n_cost;
    const void *dx = xyzs, *dk = kpts;
    const int32_t *dnp = n_persons;
    double *ds = cost_sum;
    int32_t *dn = cost_n;
    Staging sg(ctx->in, ctx->out, memspace == SNOWTRI_HOST, st);
    sg.in(&dx, x_bytes);
    sg.in(&dk, k_bytes);
    sg.in(&dnp, np_bytes);
    sg.out(&ds, s_bytes);
    sg.out(&dn, n_bytes);
    if (int rc = sg.begin()) return rc;
    const dim3 grid((unsigned)((n_items + kCostWaves - 1) / kCostWaves));
    const int raw = (flags & SNOWTRI_REPROJECT_RAW) ? 1 : 0;
    with_float_pair(xyz_dtype, kpts_dtype, [&](auto tx, auto tk) {
        using TX = decltype(tx);
        using TK = decltype(tk);
        hipLaunchKernelGGL((k_reproject_cost<TX, TK>), grid, dim3(64 * kCostWaves), 0, st, n_items, (int)ctx->C, (int)P, (int)Pmax, (int)kn, raw,
                           keypoint_score_threshold, (const double *)ctx->dProj, (const TX *)dx, (const TK *)dk, dnp, ds, dn);
    });
    HIP_TRY(hipGetLastError());
    return sg.end();
}

}  // extern "C"

// ------------------------------------------------------------------------------- assignment
extern "C" {

int snowtri_assign_detections(snowtri_ctx *ctx, int64_t n, int32_t P, int32_t Pmax, const double *cost_sum, const int32_t *cost_n, double gate_px,
                              int32_t min_joints, int32_t *det_of, int32_t *person_of, double *total, int memspace, void *stream) {
    const Refuse refuse{"snowtri_assign_detections"};
    // (the context is looked at last: every other refusal names its argument with or without one)
    if (memspace != SNOWTRI_HOST && memspace != SNOWTRI_DEVICE) return refuse("unknown memspace");
    if (n < 0) return refuse("n < 0");
    if (P < 1 || Pmax < 1) return refuse("P < 1 or Pmax < 1");
    if ((int64_t)P + Pmax > kAssignMaxColumns) return refuse("P + Pmax must not exceed 64 (the columns of a problem are the lanes of one wave)");
    if (min_joints < 1) return refuse("min_joints < 1");
    if (!(gate_px >= 0.0)) return refuse("gate_px must be >= 0 and not NaN");
    // (staying unmatched costs gate_px^2: an infinite one leaves the rule without a finite column to fall back on, and the duals are
    // sums of a few such costs: 1e300 leaves them room)
    if (!(gate_px <= kAssignMaxGate)) return refuse("gate_px must not exceed 1e150 (staying unmatched costs gate_px^2, which must stay finite)");
    // 64 / W problems per wave, four waves per workgroup on a one-dimensional grid; 64-bit element offsets
    const int cols = P + Pmax, W = cols <= 8 ? 8 : cols <= 16 ? 16 : cols <= 32 ? 32 : 64;
    const int64_t per_wg = (int64_t)kAssignWaves * (64 / W), pq = (int64_t)P * Pmax;
    if (n > 0) {   // (n == 0 looks at no pointer)
        if (n > ((int64_t)1 << 48) / pq) return refuse("n * P * Pmax must not exceed 2^48 costs");
        if (n > (int64_t)0x7fffffff * per_wg) return refuse("n must not exceed (2^31 - 1) workgroups of 4 * (64 / W) problems");
        if (!cost_sum || !cost_n || !det_of) return refuse("null array (cost_sum, cost_n or det_of)");
        if (memspace == SNOWTRI_DEVICE && ((((uintptr_t)cost_sum | (uintptr_t)total) & 7u) ||
                                           (((uintptr_t)cost_n | (uintptr_t)det_of | (uintptr_t)person_of) & 3u)))
            return refuse("cost_sum, cost_n, det_of, person_of and total must be aligned to their element size");
    }
    if (!ctx) return refuse("null context");
    if (n == 0) return SNOWTRI_OK;
    ENTER_DEVICE(ctx->device);
    hipStream_t st = (hipStream_t)stream;
    const double *ds = cost_sum;
    const int32_t *dn = cost_n;
    int32_t *dd = det_of, *dp = person_of;
    double *dt = total;
    Staging sg(ctx->in, ctx->out, memspace == SNOWTRI_HOST, st);
    sg.in(&ds, sizeof(double) * (size_t)(n * pq));
    sg.in(&dn, sizeof(int32_t) * (size_t)(n * pq));
    sg.out(&dd, sizeof(int32_t) * (size_t)n * P);
    sg.out(&dp, sizeof(int32_t) * (size_t)n * Pmax);
    sg.out(&dt, sizeof(double) * (size_t)n);
    if (int rc = sg.begin()) return rc;
    const dim3 grid((unsigned)((n + per_wg - 1) / per_wg));
    const double gate2 = gate_px * gate_px;
    auto launch = [&](auto w) {   // w: the sub-wave width the kernel is compiled for, as a std::integral_constant
        hipLaunchKernelGGL((k_assign<decltype(w)::value>), grid, dim3(64 * kAssignWaves), 0, st, n, (int)P, (int)Pmax, gate2, (int)min_joints, ds, dn,
                           dd, dp, dt);
    };
    if (ctx->timing) HIP_TRY(hipEventRecord(ctx->ev[0], st));   // snowtri_set_timing: the kernel between the pair snowtri_last_kernel_ms reads
    if (W == 8) launch(std::integral_constant<int, 8>());
    else if (W == 16) launch(std::integral_constant<int, 16>());
    else if (W == 32) launch(std::integral_constant<int, 32>());
    else launch(std::integral_constant<int, 64>());
    HIP_TRY(hipGetLastError());
    if (ctx->timing) {
        HIP_TRY(hipEventRecord(ctx->ev[1], st));
        HIP_TRY(hipEventRecord(ctx->ev[2], st));   // (no second phase: the pair (2, 3) is empty)
        HIP_TRY(hipEventRecord(ctx->ev[3], st));
        ctx->ev_valid = true;
        ctx->ev_stream = st;
    }
    return sg.end();
}

}  // extern "C"

// ------------------------------------------------------------------------------- seeding
extern "C" {

int snowtri_pair_cost(snowtri_ctx *ctx, int64_t F, int32_t kn, int32_t Pmax, const void *kpts, int kpts_dtype, const int32_t *n_persons,
                      const int32_t *claimed, double keypoint_score_threshold, double *pair_sum, int32_t *pair_n, int memspace, void *stream) {
    const Refuse refuse{"snowtri_pair_cost"};
    if (!ctx) return refuse("null context");
    if (kpts_dtype != SNOWTRI_F32 && kpts_dtype != SNOWTRI_F64) return refuse("unknown dtype");
    if (memspace != SNOWTRI_HOST && memspace != SNOWTRI_DEVICE) return refuse("unknown memspace");
    if (F < 0 || kn < 1) return refuse("F < 0 or kn < 1");
    if (Pmax < 1) return refuse("Pmax < 1");
    if (ctx->C < 2 || ctx->C > kSeedMaxCams) return refuse("the pair cost takes 2 to 8 cameras");
    if (kn > kSeedMaxJoints) return refuse("kn must not exceed 256 joints (four per lane of the wave that owns a detection)");
    if (keypoint_score_threshold != keypoint_score_threshold) return refuse("keypoint_score_threshold is NaN");
    if (F == 0) return SNOWTRI_OK;   // (looks at no pointer)
    // one workgroup per (frame, camera pair) on a one-dimensional grid; 64-bit element offsets
    const int C = ctx->C, NP = ctx->npairs;
    const int64_t pp = (int64_t)Pmax * Pmax;
    if (F > (int64_t)0x7fffffff / NP) return refuse("F * C (C - 1) / 2 must not exceed 2^31 - 1 workgroups");
    if (pp > ((int64_t)1 << 48) / (F * NP) || (int64_t)Pmax * kn > ((int64_t)1 << 48) / (F * C))
        return refuse("F * NP * Pmax * Pmax must not exceed 2^48 costs, F * C * Pmax * kn 2^48 keypoints");
    if (!kpts || !pair_sum || !pair_n) return refuse("null array (kpts, pair_sum or pair_n)");
    if (memspace == SNOWTRI_DEVICE && ((((uintptr_t)kpts) & (dtype_size(kpts_dtype) - 1)) || (((uintptr_t)pair_sum) & 7u) ||
                                       ((((uintptr_t)pair_n) | ((uintptr_t)n_persons) | ((uintptr_t)claimed)) & 3u)))
        return refuse("kpts, n_persons, claimed, pair_sum and pair_n must be aligned to their element size");
    ENTER_DEVICE(ctx->device);
    hipStream_t st = (hipStream_t)stream;
    const int64_t n_wg = F * NP, n_cost = n_wg * pp;
    const void *dk = kpts;
    const int32_t *dnp = n_persons, *dcl = claimed;
    double *ds = pair_sum;
    int32_t *dn = pair_n;
    Staging sg(ctx->in, ctx->out, memspace == SNOWTRI_HOST, st);
    sg.in(&dk, dtype_size(kpts_dtype) * 3 * (size_t)F * C * Pmax * kn);
    sg.in(&dnp, sizeof(int32_t) * (size_t)F * C);
    sg.in(&dcl, sizeof(int32_t) * (size_t)F * C * Pmax);
    sg.out(&ds, sizeof(double) * (size_t)n_cost);
    sg.out(&dn, sizeof(int32_t) * (size_t)n_cost);
    if (int rc = sg.begin()) return rc;
    const int RT = seed_tile_dets(Pmax, kn), waves = std::min<int>(kSeedMaxWaves, Pmax);
    const size_t lds = sizeof(double) * 3 * (size_t)RT * kn;
    if (ctx->timing) HIP_TRY(hipEventRecord(ctx->ev[0], st));   // snowtri_set_timing: the kernel between the pair snowtri_last_kernel_ms reads
    if (kpts_dtype == SNOWTRI_F32)
        hipLaunchKernelGGL((k_pair_cost<float>), dim3((unsigned)n_wg), dim3(64 * waves), lds, st, n_wg, C, NP, (int)Pmax, (int)kn, RT,
                           keypoint_score_threshold, ctx->rig(), (const float *)dk, dnp, dcl, ds, dn);
    else
        hipLaunchKernelGGL((k_pair_cost<double>), dim3((unsigned)n_wg), dim3(64 * waves), lds, st, n_wg, C, NP, (int)Pmax, (int)kn, RT,
                           keypoint_score_threshold, ctx->rig(), (const double *)dk, dnp, dcl, ds, dn);
    HIP_TRY(hipGetLastError());
    if (ctx->timing) {
        HIP_TRY(hipEventRecord(ctx->ev[1], st));
        HIP_TRY(hipEventRecord(ctx->ev[2], st));   // (no second phase: the pair (2, 3) is empty)
        HIP_TRY(hipEventRecord(ctx->ev[3], st));
        ctx->ev_valid = true;
        ctx->ev_stream = st;
    }
    return sg.end();
}

int snowtri_seed_persons(snowtri_ctx *ctx, int64_t F, int32_t Pmax, const double *pair_sum, const int32_t *pair_n, const int32_t *n_persons,
                         const int32_t *claimed, double gate, int32_t min_joints, int32_t min_views, int32_t S, int32_t *seed_det_of,
                         int32_t *n_seeds, uint32_t *flags, int memspace, void *stream) {
    const Refuse refuse{"snowtri_seed_persons"};
    // (the context is looked at after the arguments that need none)
    if (memspace != SNOWTRI_HOST && memspace != SNOWTRI_DEVICE) return refuse("unknown memspace");
    if (F < 0) return refuse("F < 0");
    if (Pmax < 1) return refuse("Pmax < 1");
    if (S < 1 || S > 64) return refuse("S must lie in 1..64");
    if (min_joints < 1) return refuse("min_joints < 1");
    if (!(gate >= 0.0)) return refuse("gate must be >= 0 and not NaN");
    if (!(gate <= kSeedMaxGate)) return refuse("gate must not exceed 1e150 (the means are compared with gate * gate, which must stay finite)");
    if (!ctx) return refuse("null context");
    const int C = ctx->C;
    if (C < 2) return refuse("the context needs at least 2 cameras");
    if ((int64_t)C * Pmax > kSeedMaxNodes) return refuse("C * Pmax must not exceed 64 (the nodes of a frame are the lanes of one wave)");
    if (min_views < 2 || min_views > C) return refuse("min_views must lie in 2..C");
    if (F == 0) return SNOWTRI_OK;   // (looks at no pointer)
    if (F > 0x7fffffffll) return refuse("F must not exceed 2^31 - 1 workgroups");
    if (!pair_sum || !pair_n || !seed_det_of || !n_seeds) return refuse("null array (pair_sum, pair_n, seed_det_of or n_seeds)");
    if (memspace == SNOWTRI_DEVICE &&
        ((((uintptr_t)pair_sum) & 7u) || ((((uintptr_t)pair_n) | ((uintptr_t)n_persons) | ((uintptr_t)claimed) | ((uintptr_t)seed_det_of) |
                                            ((uintptr_t)n_seeds) | ((uintptr_t)flags)) & 3u)))
        return refuse("pair_sum, pair_n, n_persons, claimed, seed_det_of, n_seeds and flags must be aligned to their element size");
    ENTER_DEVICE(ctx->device);
    hipStream_t st = (hipStream_t)stream;
    const int N = C * Pmax;
    const size_t n_cost = (size_t)F * ctx->npairs * Pmax * Pmax;
    const double *ds = pair_sum;
    const int32_t *dn = pair_n, *dnp = n_persons, *dcl = claimed;
    int32_t *dso = seed_det_of, *dns = n_seeds;
    uint32_t *dfl = flags;
    Staging sg(ctx->in, ctx->out, memspace == SNOWTRI_HOST, st);
    sg.in(&ds, sizeof(double) * n_cost);
    sg.in(&dn, sizeof(int32_t) * n_cost);
    sg.in(&dnp, sizeof(int32_t) * (size_t)F * C);
    sg.in(&dcl, sizeof(int32_t) * (size_t)F * C * Pmax);
    sg.out(&dso, sizeof(int32_t) * (size_t)F * C * S);
    sg.out(&dns, sizeof(int32_t) * (size_t)F);
    sg.out(&dfl, sizeof(uint32_t) * (size_t)F);
    if (int rc = sg.begin()) return rc;
    if (ctx->timing) HIP_TRY(hipEventRecord(ctx->ev[0], st));
    hipLaunchKernelGGL(k_seed_group, dim3((unsigned)F), dim3(64), sizeof(double) * (size_t)N * N, st, F, C, (int)Pmax, (int)S, gate * gate,
                       (int)min_joints, (int)min_views, (const int32_t *)ctx->dpairs, ds, dn, dnp, dcl, dso, dns, dfl);
    HIP_TRY(hipGetLastError());
    if (ctx->timing) {
        HIP_TRY(hipEventRecord(ctx->ev[1], st));
        HIP_TRY(hipEventRecord(ctx->ev[2], st));   // (no second phase: the pair (2, 3) is empty)
        HIP_TRY(hipEventRecord(ctx->ev[3], st));
        ctx->ev_valid = true;
        ctx->ev_stream = st;
    }
    return sg.end();
}

}  // extern "C"

// ------------------------------------------------------------------------------- refinement
namespace {

// The inputs that snowtri_refine_joints and snowtri_refine_cameras take alike -- the joint records, the detections of every camera
// and what matches one to the other (n_persons, det_of, views) -- with the checks, sizes and staging the two share.
struct ObservedInputs {
    int64_t n_rec = 0;   // F * P * kn; 0 is the empty batch, of which no input pointer is looked at (the five below stay null)
    size_t x_bytes = 0, k_bytes = 0, np_bytes = 0, det_bytes = 0, views_bytes = 0;
    const void *dx = nullptr, *dk = nullptr;   // the caller's arrays; behind stage() and Staging::begin() what the kernels read
    const int32_t *dnp = nullptr, *ddet = nullptr;
    const uint32_t *dviews = nullptr;

    // After reproject_args.  -> 0, or the status of a refusal; F == 0 is none, and what it means is the entry's to say.
    int check(const Refuse &refuse, const snowtri_ctx *ctx, int64_t F, int32_t P, int32_t kn, const void *xyzs, int xyz_dtype, int32_t Pmax,
              const void *kpts, int kpts_dtype, const int32_t *n_persons, const int32_t *det_of, const uint32_t *views,
              double keypoint_score_threshold, int32_t iters, uint32_t flags, uint32_t known_flags, int memspace) {
        if (flags & ~known_flags) return refuse("unknown flag bit");
        if (Pmax < 1) return refuse("Pmax < 1");
        if (keypoint_score_threshold != keypoint_score_threshold) return refuse("keypoint_score_threshold is NaN");
        if (iters < 1 || iters > kRefineMaxIters) return refuse("iters must lie in 1..16");
        if (ctx->C > kRefineMaxCams) return refuse("more than 32 cameras (a set of cameras is a 32-bit mask)");
        if (!det_of && P > Pmax) return refuse("det_of == NULL pairs person p with detection p: P must not exceed Pmax");
        if (F == 0) return 0;
        // one lane per record, 256 per workgroup on a one-dimensional grid; 64-bit element offsets
        const int64_t max_rec = (int64_t)0x7fffffff * kRefineBlock, per_frame = (int64_t)P * kn;   // (two int32: no overflow)
        if (F > max_rec / per_frame) return refuse("F * P * kn must not exceed (2^31 - 1) * 256 records");
        const int64_t per_view = (int64_t)Pmax * kn, cp = (int64_t)ctx->C * std::max(P, Pmax);
        if (F > (((int64_t)1 << 56) / per_view) / ctx->C || F > ((int64_t)1 << 56) / cp)
            return refuse("F * C * Pmax * kn and F * C * P must not exceed 2^56 elements");
        if (!xyzs || !kpts) return refuse("null array (xyzs or kpts)");
        const size_t xs = dtype_size(xyz_dtype), ks = dtype_size(kpts_dtype);
        if (memspace == SNOWTRI_DEVICE && ((((uintptr_t)xyzs) & (xs - 1)) || (((uintptr_t)kpts) & (ks - 1)) ||
                                           (((uintptr_t)n_persons | (uintptr_t)det_of | (uintptr_t)views) & 3u)))
            return refuse("xyzs, kpts, n_persons, det_of and views must be aligned to their element size");
        n_rec = F * per_frame;
        x_bytes = xs * 4 * (size_t)n_rec;
        k_bytes = ks * 3 * (size_t)F * ctx->C * (size_t)per_view;
        np_bytes = sizeof(int32_t) * (size_t)F * ctx->C;
        det_bytes = np_bytes * P;
        views_bytes = sizeof(uint32_t) * (size_t)n_rec;
        dx = xyzs, dk = kpts, dnp = n_persons, ddet = det_of, dviews = views;
        return 0;
    }
    void stage(Staging &sg) {   // (in this order: it is the layout of ctx->in)
        sg.in(&dx, x_bytes);
        sg.in(&dk, k_bytes);
        sg.in(&dnp, np_bytes);
        sg.in(&ddet, det_bytes);
        sg.in(&dviews, views_bytes);
    }
};

constexpr double kHuberMaxPx = 1e150;   // delta * delta must stay finite (the bound of snowtri_assign_detections' gate)

// huber_px of the two _ex entries -> 0, or the status of a refusal; hc: the loss' constants, formed once here in fp64
// (all 0 for huber_px == 0, the squared loss).
int huber_check(const Refuse &refuse, double huber_px, HuberConst &hc) {
    if (!(huber_px >= 0.0)) return refuse("huber_px must be >= 0 and not NaN");
    if (!(huber_px <= kHuberMaxPx)) return refuse("huber_px must not exceed 1e150 (huber_px * huber_px must stay finite)");
    hc.d = huber_px;
    hc.two_d = 2.0 * huber_px;
    hc.dd = huber_px * huber_px;
    return 0;
}

}  // namespace

extern "C" {

namespace {
int refine_joints_impl(const char *who, snowtri_ctx *ctx, int64_t F, int32_t P, int32_t kn, const void *xyzs, int xyz_dtype, int32_t Pmax,
                       const void *kpts, int kpts_dtype, const int32_t *n_persons, const int32_t *det_of, const uint32_t *views,
                       double keypoint_score_threshold, int32_t iters, uint32_t flags, double huber_px, void *out_xyzs, double *cost,
                       uint8_t *codes, uint32_t *outliers, int memspace, void *stream);
}

int snowtri_refine_joints(snowtri_ctx *ctx, int64_t F, int32_t P, int32_t kn, const void *xyzs, int xyz_dtype, int32_t Pmax, const void *kpts,
                          int kpts_dtype, const int32_t *n_persons, const int32_t *det_of, const uint32_t *views,
                          double keypoint_score_threshold, int32_t iters, uint32_t flags, void *out_xyzs, double *cost, uint8_t *codes,
                          int memspace, void *stream) {
    return refine_joints_impl("snowtri_refine_joints", ctx, F, P, kn, xyzs, xyz_dtype, Pmax, kpts, kpts_dtype, n_persons, det_of, views,
                              keypoint_score_threshold, iters, flags, 0.0, out_xyzs, cost, codes, nullptr, memspace, stream);
}

int snowtri_refine_joints_ex(snowtri_ctx *ctx, int64_t F, int32_t P, int32_t kn, const void *xyzs, int xyz_dtype, int32_t Pmax, const void *kpts,
                             int kpts_dtype, const int32_t *n_persons, const int32_t *det_of, const uint32_t *views,
                             double keypoint_score_threshold, int32_t iters, uint32_t flags, double huber_px, void *out_xyzs, double *cost,
                             uint8_t *codes, uint32_t *outliers, int memspace, void *stream) {
    return refine_joints_impl("snowtri_refine_joints_ex", ctx, F, P, kn, xyzs, xyz_dtype, Pmax, kpts, kpts_dtype, n_persons, det_of, views,
                              keypoint_score_threshold, iters, flags, huber_px, out_xyzs, cost, codes, outliers, memspace, stream);
}

}  // extern "C"

namespace {

int refine_joints_impl(const char *who, snowtri_ctx *ctx, int64_t F, int32_t P, int32_t kn, const void *xyzs, int xyz_dtype, int32_t Pmax,
                       const void *kpts, int kpts_dtype, const int32_t *n_persons, const int32_t *det_of, const uint32_t *views,
                       double keypoint_score_threshold, int32_t iters, uint32_t flags, double huber_px, void *out_xyzs, double *cost,
                       uint8_t *codes, uint32_t *outliers, int memspace, void *stream) {
    if (int rc = reproject_args(who, ctx, F, P, kn, xyz_dtype, 0u, kpts_dtype, memspace)) return rc;
    const Refuse refuse{who};
    HuberConst hc{};
    if (int rc = huber_check(refuse, huber_px, hc)) return rc;
    ObservedInputs in;
    if (int rc = in.check(refuse, ctx, F, P, kn, xyzs, xyz_dtype, Pmax, kpts, kpts_dtype, n_persons, det_of, views, keypoint_score_threshold, iters,
                          flags, SNOWTRI_REFINE_SCORE_WEIGHTS, memspace))
        return rc;
    if (F == 0) return SNOWTRI_OK;
    if (!out_xyzs) return refuse("null array (out_xyzs)");
    if (memspace == SNOWTRI_DEVICE &&
        ((((uintptr_t)out_xyzs) & (dtype_size(xyz_dtype) - 1)) || (((uintptr_t)cost) & 7u) || (((uintptr_t)outliers) & 3u)))
        return refuse("out_xyzs, cost and outliers must be aligned to their element size");
    // a lane reads its record and writes it at the same place: out_xyzs == xyzs is that; any other overlap lets one lane's store
    // reach another lane's load
    if (out_xyzs != xyzs && (uintptr_t)xyzs < (uintptr_t)out_xyzs + in.x_bytes && (uintptr_t)out_xyzs < (uintptr_t)xyzs + in.x_bytes)
        return refuse("out_xyzs must be xyzs itself or not overlap it");
    // outliers is written by the lane that read record i: it must not reach any lane's record, in xyzs or in out_xyzs
    const size_t o_bytes = sizeof(uint32_t) * (size_t)in.n_rec;
    auto overlaps = [](const void *a, size_t na, const void *b, size_t nb) {
        return (uintptr_t)a < (uintptr_t)b + nb && (uintptr_t)b < (uintptr_t)a + na;
    };
    if (outliers && (overlaps(outliers, o_bytes, xyzs, in.x_bytes) || overlaps(outliers, o_bytes, out_xyzs, in.x_bytes)))
        return refuse("outliers must not overlap xyzs or out_xyzs");
    ENTER_DEVICE(ctx->device);
    hipStream_t st = (hipStream_t)stream;
    const int64_t n_rec = in.n_rec;
    void *d_out = out_xyzs;
    double *d_cost = cost;
    uint8_t *d_codes = codes;
    uint32_t *d_outl = outliers;
    const bool huber = huber_px > 0.0;
    Staging sg(ctx->in, ctx->out, memspace == SNOWTRI_HOST, st);
    in.stage(sg);
    sg.out(&d_out, in.x_bytes);
    sg.out(&d_cost, sizeof(double) * 2 * (size_t)n_rec);
    sg.out(&d_codes, (size_t)n_rec);
    sg.out(&d_outl, o_bytes);
    if (int rc = sg.begin()) return rc;
    // the squared loss (huber_px == 0) has no view in the linear regime: its kernel writes no outliers, they are zeros
    if (!huber && d_outl) HIP_TRY(hipMemsetAsync(d_outl, 0, o_bytes, st));
    // (a DEVICE call with out_xyzs == xyzs passes one pointer twice: the kernel declares neither of the two restrict)
    const dim3 grid((unsigned)((n_rec + kRefineBlock - 1) / kRefineBlock));
    const int C = ctx->C;
    auto launch = [&](auto ct) {   // ct: the camera count the kernel is compiled for (0: any) as a std::integral_constant
        with_float_pair(xyz_dtype, kpts_dtype, [&](auto tx, auto tk) {
            using TX = decltype(tx);
            using TK = decltype(tk);
            const auto kernel = huber ? k_refine<decltype(ct)::value, TX, TK, true> : k_refine<decltype(ct)::value, TX, TK, false>;
            hipLaunchKernelGGL(kernel, grid, dim3(kRefineBlock), 0, st, n_rec, C, (int)P, (int)Pmax, (int)kn, keypoint_score_threshold,
                               (int)iters, flags, (const double *)ctx->dProj, (const TX *)in.dx, (const TK *)in.dk, in.dnp, in.ddet, in.dviews,
                               (TX *)d_out, d_cost, d_codes, hc, huber ? d_outl : nullptr);
        });
    };
    if (C == 4) launch(std::integral_constant<int, 4>());
    else if (C == 8) launch(std::integral_constant<int, 8>());
    else launch(std::integral_constant<int, 0>());
    HIP_TRY(hipGetLastError());
    return sg.end();
}

}  // namespace

// ------------------------------------------------------------------------------- camera pose refinement
namespace {
int refine_cameras_impl(const char *who, snowtri_ctx *ctx, int64_t F, int32_t P, int32_t kn, const void *xyzs, int xyz_dtype, int32_t Pmax,
                        const void *kpts, int kpts_dtype, const int32_t *n_persons, const int32_t *det_of, const uint32_t *views,
                        double keypoint_score_threshold, uint32_t free_mask, int32_t min_obs, int32_t iters, uint32_t flags, double huber_px,
                        double *R_out, double *t_out, double *cost, int64_t *n_obs, uint8_t *codes, double *normal, int64_t *n_outliers,
                        int memspace, void *stream);
}

extern "C" {

int snowtri_pose_sweep_records(void) { return kPoseGridCap * kPoseBlock; }

int snowtri_refine_cameras(snowtri_ctx *ctx, int64_t F, int32_t P, int32_t kn, const void *xyzs, int xyz_dtype, int32_t Pmax, const void *kpts,
                           int kpts_dtype, const int32_t *n_persons, const int32_t *det_of, const uint32_t *views,
                           double keypoint_score_threshold, uint32_t free_mask, int32_t min_obs, int32_t iters, uint32_t flags, double *R_out,
                           double *t_out, double *cost, int64_t *n_obs, uint8_t *codes, double *normal, int memspace, void *stream) {
    return refine_cameras_impl("snowtri_refine_cameras", ctx, F, P, kn, xyzs, xyz_dtype, Pmax, kpts, kpts_dtype, n_persons, det_of, views,
                               keypoint_score_threshold, free_mask, min_obs, iters, flags, 0.0, R_out, t_out, cost, n_obs, codes, normal, nullptr,
                               memspace, stream);
}

int snowtri_refine_cameras_ex(snowtri_ctx *ctx, int64_t F, int32_t P, int32_t kn, const void *xyzs, int xyz_dtype, int32_t Pmax, const void *kpts,
                              int kpts_dtype, const int32_t *n_persons, const int32_t *det_of, const uint32_t *views,
                              double keypoint_score_threshold, uint32_t free_mask, int32_t min_obs, int32_t iters, uint32_t flags,
                              double huber_px, double *R_out, double *t_out, double *cost, int64_t *n_obs, uint8_t *codes, double *normal,
                              int64_t *n_outliers, int memspace, void *stream) {
    return refine_cameras_impl("snowtri_refine_cameras_ex", ctx, F, P, kn, xyzs, xyz_dtype, Pmax, kpts, kpts_dtype, n_persons, det_of, views,
                               keypoint_score_threshold, free_mask, min_obs, iters, flags, huber_px, R_out, t_out, cost, n_obs, codes, normal,
                               n_outliers, memspace, stream);
}

}  // extern "C"

namespace {

int refine_cameras_impl(const char *who, snowtri_ctx *ctx, int64_t F, int32_t P, int32_t kn, const void *xyzs, int xyz_dtype, int32_t Pmax,
                        const void *kpts, int kpts_dtype, const int32_t *n_persons, const int32_t *det_of, const uint32_t *views,
                        double keypoint_score_threshold, uint32_t free_mask, int32_t min_obs, int32_t iters, uint32_t flags, double huber_px,
                        double *R_out, double *t_out, double *cost, int64_t *n_obs, uint8_t *codes, double *normal, int64_t *n_outliers,
                        int memspace, void *stream) {
    if (int rc = reproject_args(who, ctx, F, P, kn, xyz_dtype, 0u, kpts_dtype, memspace)) return rc;
    const Refuse refuse{who};
    HuberConst hc{};
    if (int rc = huber_check(refuse, huber_px, hc)) return rc;
    const bool huber = huber_px > 0.0;
#ifdef SNOWTRI_POSE_PER_RECORD
    if (huber) return refuse("the per-record development kernel has no Huber instantiation");
#endif
    ObservedInputs in;   // (F == 0 is work here: no input pointer is looked at, only k_pose_step runs, every pose is copied)
    if (int rc = in.check(refuse, ctx, F, P, kn, xyzs, xyz_dtype, Pmax, kpts, kpts_dtype, n_persons, det_of, views, keypoint_score_threshold, iters,
                          flags, SNOWTRI_REFINE_SCORE_WEIGHTS, memspace))
        return rc;
    if (min_obs < 3) return refuse("min_obs must be at least 3 (six parameters, two equations per observation)");
    if (ctx->C < 32 && (free_mask >> ctx->C)) return refuse("free_mask has a bit at or above the number of cameras");
    if (!R_out || !t_out) return refuse("null array (R_out or t_out)");
    if (memspace == SNOWTRI_DEVICE &&
        (((uintptr_t)R_out | (uintptr_t)t_out | (uintptr_t)cost | (uintptr_t)n_obs | (uintptr_t)normal | (uintptr_t)n_outliers) & 7u))
        return refuse("R_out, t_out, cost, n_obs, normal and n_outliers must be aligned to their element size");
    const int C = ctx->C;
    const int64_t n_rec = in.n_rec;
    ENTER_DEVICE(ctx->device);
    hipStream_t st = (hipStream_t)stream;
    if (!ctx->pose_ws) HIP_TRY(hipMalloc(&ctx->pose_ws, sizeof(double) * pose_ws_doubles(C)));   // the first call on this context, and no later one
    double *dR = R_out, *dt = t_out, *d_cost = cost, *d_normal = normal;
    int64_t *d_nobs = n_obs, *d_noutl = n_outliers;
    uint8_t *d_codes = codes;
    Staging sg(ctx->in, ctx->out, memspace == SNOWTRI_HOST, st);
    in.stage(sg);
    sg.out(&dR, sizeof(double) * 9 * (size_t)C);
    sg.out(&dt, sizeof(double) * 3 * (size_t)C);
    sg.out(&d_cost, sizeof(double) * 2 * (size_t)C);
    sg.out(&d_nobs, sizeof(int64_t) * (size_t)C);
    sg.out(&d_codes, (size_t)C);
    sg.out(&d_normal, sizeof(double) * 28 * (size_t)C);
    sg.out(&d_noutl, sizeof(int64_t) * (size_t)C);
    if (int rc = sg.begin()) return rc;
    double *ws = ctx->pose_ws;
    const double *base = (const double *)ctx->dProj;
    const int G = n_rec ? grid_for(n_rec, kPoseBlock, kPoseGridCap) : 0;
    const int n_eval = n_rec ? (int)iters : 0;   // evaluations behind the one at the input pose: 2 (iters + 1) launches whatever the data does
    for (int e = 0; e <= n_eval; e++) {
        const double *trial = e ? ws + pose_ws_trial(C) : base;
        const int32_t *active = e ? reinterpret_cast<const int32_t *>(ws + pose_ws_active(C)) : nullptr;
        if (G)
            with_float_pair(xyz_dtype, kpts_dtype, [&](auto tx, auto tk) {
                using TX = decltype(tx);
                using TK = decltype(tk);
#ifdef SNOWTRI_POSE_PER_RECORD   // (a development build: the shape that lost, EXPERIMENTS.md round 22)
                const auto kernel = k_pose_normal_rec<TX, TK>;
                const dim3 grid((unsigned)G);
                hipLaunchKernelGGL(kernel, grid, dim3(kPoseBlock), 0, st, n_rec, C, (int)P, (int)Pmax, (int)kn, keypoint_score_threshold, flags, base,
                                   trial, active, (const TX *)in.dx, (const TK *)in.dk, in.dnp, in.ddet, in.dviews, ws + pose_ws_partials(C));
#else
                const auto kernel = huber ? k_pose_normal<TX, TK, true> : k_pose_normal<TX, TK, false>;
                const dim3 grid((unsigned)G, (unsigned)C);
                hipLaunchKernelGGL(kernel, grid, dim3(kPoseBlock), 0, st, n_rec, C, (int)P, (int)Pmax, (int)kn, keypoint_score_threshold, flags, base,
                                   trial, active, (const TX *)in.dx, (const TK *)in.dk, in.dnp, in.ddet, in.dviews, ws + pose_ws_partials(C), hc);
#endif
            });
        hipLaunchKernelGGL(k_pose_step, dim3(1), dim3(kPoseStepBlock), 0, st, C, G, e, e == n_eval ? 1 : 0, free_mask, (int)min_obs, base, ws, dR, dt,
                           d_cost, d_nobs, d_codes, d_normal, d_noutl);
    }
    HIP_TRY(hipGetLastError());
    return sg.end();
}

}  // namespace

// ------------------------------------------------------------------------------- camera refinement with intrinsics
extern "C" {

int snowtri_refine_cameras_k(snowtri_ctx *ctx, int64_t F, int32_t P, int32_t kn, const void *xyzs, int xyz_dtype, int32_t Pmax, const void *kpts,
                             int kpts_dtype, const int32_t *n_persons, const int32_t *det_of, const uint32_t *views,
                             double keypoint_score_threshold, uint32_t free_mask, uint32_t intr_mask, uint32_t intr_flags, int32_t min_obs,
                             int32_t iters, uint32_t flags, double huber_px, double *K_out, double *R_out, double *t_out, double *cost,
                             int64_t *n_obs, uint8_t *codes, double *normal, int64_t *n_outliers, int memspace, void *stream) {
    const char *who = "snowtri_refine_cameras_k";
    if (int rc = reproject_args(who, ctx, F, P, kn, xyz_dtype, 0u, kpts_dtype, memspace)) return rc;
    const Refuse refuse{who};
    HuberConst hc{};
    if (int rc = huber_check(refuse, huber_px, hc)) return rc;
    const bool huber = huber_px > 0.0;
    ObservedInputs in;   // (F == 0 is work here, as in snowtri_refine_cameras: only k_pose_step_k runs, every camera is copied)
    if (int rc = in.check(refuse, ctx, F, P, kn, xyzs, xyz_dtype, Pmax, kpts, kpts_dtype, n_persons, det_of, views, keypoint_score_threshold, iters,
                          flags, SNOWTRI_REFINE_SCORE_WEIGHTS, memspace))
        return rc;
    if (min_obs < 3) return refuse("min_obs must be at least 3 (six parameters, two equations per observation)");
    if (ctx->C < 32 && (free_mask >> ctx->C)) return refuse("free_mask has a bit at or above the number of cameras");
    if (intr_flags & ~(uint32_t)(SNOWTRI_INTR_FOCAL | SNOWTRI_INTR_CENTRE)) return refuse("intr_flags has an unknown flag bit");
    if (ctx->C < 32 && (intr_mask >> ctx->C)) return refuse("intr_mask has a bit at or above the number of cameras");
    if (!R_out || !t_out) return refuse("null array (R_out or t_out)");
    if (intr_flags && !K_out) return refuse("null array (K_out is required when intr_flags != 0)");
    if (memspace == SNOWTRI_DEVICE && (((uintptr_t)K_out | (uintptr_t)R_out | (uintptr_t)t_out | (uintptr_t)cost | (uintptr_t)n_obs |
                                        (uintptr_t)normal | (uintptr_t)n_outliers) & 7u))
        return refuse("K_out, R_out, t_out, cost, n_obs, normal and n_outliers must be aligned to their element size");
    const int C = ctx->C;
    const int64_t n_rec = in.n_rec;
    ENTER_DEVICE(ctx->device);
    hipStream_t st = (hipStream_t)stream;
    if (!ctx->pose_kws) {   // the first intrinsics call on this context, and no later one
        double *p = nullptr;
        HIP_TRY(hipMalloc(&p, sizeof(double) * pose_kws_doubles(C)));
        if (hipMemcpy(p + pose_kws_K(C), ctx->hK.data(), sizeof(double) * 9 * (size_t)C, hipMemcpyHostToDevice) != hipSuccess) {
            (void)hipFree(p);
            g_last_error = "hipMemcpy of K into the intrinsics workspace failed";
            return SNOWTRI_ERR_HIP;
        }
        ctx->pose_kws = p;
    }
    double *dK = K_out, *dR = R_out, *dt = t_out, *d_cost = cost, *d_normal = normal;
    int64_t *d_nobs = n_obs, *d_noutl = n_outliers;
    uint8_t *d_codes = codes;
    Staging sg(ctx->in, ctx->out, memspace == SNOWTRI_HOST, st);
    in.stage(sg);
    sg.out(&dK, sizeof(double) * 9 * (size_t)C);
    sg.out(&dR, sizeof(double) * 9 * (size_t)C);
    sg.out(&dt, sizeof(double) * 3 * (size_t)C);
    sg.out(&d_cost, sizeof(double) * 2 * (size_t)C);
    sg.out(&d_nobs, sizeof(int64_t) * (size_t)C);
    sg.out(&d_codes, (size_t)C);
    sg.out(&d_normal, sizeof(double) * kPoseKNormal * (size_t)C);
    sg.out(&d_noutl, sizeof(int64_t) * (size_t)C);
    if (int rc = sg.begin()) return rc;
    double *ws = ctx->pose_kws;
    const double *base = (const double *)ctx->dProj;
    const int G = n_rec ? grid_for(n_rec, kPoseBlock, kPoseGridCap) : 0;
    const int n_eval = n_rec ? (int)iters : 0;   // evaluations behind the one at the input: 2 (iters + 1) launches whatever the data does
    for (int e = 0; e <= n_eval; e++) {
        const double *trial = e ? ws + pose_kws_trial(C) : base;
        const int32_t *active = e ? reinterpret_cast<const int32_t *>(ws + pose_kws_active(C)) : nullptr;
        if (G)
            with_float_pair(xyz_dtype, kpts_dtype, [&](auto tx, auto tk) {
                using TX = decltype(tx);
                using TK = decltype(tk);
                const auto kernel = huber ? k_pose_normal_k<TX, TK, true> : k_pose_normal_k<TX, TK, false>;
                const dim3 grid((unsigned)G, (unsigned)C);
                hipLaunchKernelGGL(kernel, grid, dim3(kPoseBlock), 0, st, n_rec, C, (int)P, (int)Pmax, (int)kn, keypoint_score_threshold, flags, base,
                                   trial, active, (const TX *)in.dx, (const TK *)in.dk, in.dnp, in.ddet, in.dviews, ws + pose_kws_partials(C), hc);
            });
        hipLaunchKernelGGL(k_pose_step_k, dim3(1), dim3(kPoseStepBlock), 0, st, C, G, e, e == n_eval ? 1 : 0, free_mask, intr_mask, intr_flags,
                           (int)min_obs, base, ws, dK, dR, dt, d_cost, d_nobs, d_codes, d_normal, d_noutl);
    }
    HIP_TRY(hipGetLastError());
    return sg.end();
}

}  // extern "C"

// ------------------------------------------------------------------------------- fused A1..A4
namespace {

constexpr size_t kMaxScratchBytes = (size_t)8 << 30;

template <typename T>
const char *type_name() {
    return sizeof(T) == 4 ? "float" : "double";
}

// "k_name<a,b,...>": a kernel as snowtri_last_kernel_names spells it, its template arguments without spaces.
std::string kernel_name(const char *kernel, const std::vector<std::string> &args) {
    std::string s = std::string(kernel) + "<";
    for (size_t i = 0; i < args.size(); i++) s += (i ? "," : "") + args[i];
    return s + ">";
}

// fn(std::integral_constant<int, CC>()) for the one camera count CC == C in [Lo, Hi]; false when there is none.  A generic lambda
// takes the constant with decltype and launches the kernel instantiated for it, so [Lo, Hi] is what a route instantiates.
// Kernel-development builds (-DSNOWTRI_DEV_MIN, scripts/ab_build.sh): 4 cameras only.
template <int Lo, int Hi, typename Fn>
bool with_cameras(int C, Fn &&fn) {
    if constexpr (Lo > Hi) {
        return false;
    } else {
#ifdef SNOWTRI_DEV_MIN
        constexpr bool kept = Lo == 4;
#else
        constexpr bool kept = true;
#endif
        if constexpr (kept)
            if (C == Lo) {
                fn(std::integral_constant<int, Lo>());
                return true;
            }
        return with_cameras<Lo + 1, Hi>(C, fn);
    }
}

// ... and fn(std::integral_constant<int, TT>()) for the instantiated workgroup shape of k_candidate_sums that `threads` names
// (sums_launch_shape rounds to one of them).
template <typename Fn>
void with_sums_threads(int threads, Fn &&fn) {
    if (threads == 256) fn(std::integral_constant<int, 256>());
    else if (threads == 512) fn(std::integral_constant<int, 512>());
    else fn(std::integral_constant<int, 1024>());
}

// A kernel that asks for more dynamic LDS than the 48 KB every kernel may have: the limit is raised first (snowtri_ctx::raise_lds).
int raise_lds_or_fail(snowtri_ctx *ctx, const void *kern, size_t lds) {
    if (lds > 48 * 1024 && ctx->raise_lds(kern, (int)lds)) {
        g_last_error = "hipFuncSetAttribute(MaxDynamicSharedMemorySize) failed";
        return SNOWTRI_ERR_HIP;
    }
    return SNOWTRI_OK;
}

// Every launch of the fused call.  `may_attach`: this dispatch is the call's ONE kernel, so with snowtri_set_timing(ctx, 2) the
// ring's event pair rides on the dispatch itself: begin and end of THIS kernel as its completion signal records them (what
// rocprofv3's kernel trace reads), without the two barrier packets of a bracketing pair in the interval.
template <typename... KArgs, typename... Args>
int launch_kernel(snowtri_ctx *ctx, hipStream_t st, void (*kern)(KArgs...), dim3 grid, dim3 block, size_t lds, bool may_attach,
                  const Args &...args) {
    static_assert(sizeof...(KArgs) == sizeof...(Args), "one argument per kernel parameter");
    if (int rc = raise_lds_or_fail(ctx, (const void *)kern, lds)) return rc;
    if (may_attach && ctx->timing && ctx->timing_attach) {
        const int64_t slot = ctx->ev_count % kTimingRing;
        hipExtLaunchKernelGGL(kern, grid, block, lds, st, ctx->ev_ring[2 * slot], ctx->ev_ring[2 * slot + 1], 0, args...);
        ctx->ev_attached = true;
    } else {
        hipLaunchKernelGGL(kern, grid, block, lds, st, args...);
    }
    HIP_TRY(hipGetLastError());
    return SNOWTRI_OK;
}

// Frames per tile for the fast kernel: maximise (lane utilisation of the item loop: T*J items in
// 256-wide passes) x (balance of the tiles over the CUs -- the kernel is fp64-VALU-bound, so a CU
// with one more tile than its neighbours sets the launch time), under the LDS budget.  Prefer
// >= 2 workgroups per CU (latency hiding) unless that costs more than 5 %.
int choose_tile_frames(int64_t F, int J, int kn, int NP, int num_cus, int forced, int wg_per_cu) {
    const size_t lds_cap = wg_per_cu >= 3 ? 52 * 1024 : 64 * 1024;   // (three workgroups share a CU's 160 KB; 53 KB admits two: kRecomputeLdsBytes)
    if (forced >= 1 && forced <= 64 && fused_single_lds_bytes(forced, kn, NP) <= lds_cap) return forced;
    int best = 1;
    double best_score = -1.0;
    for (int T = 1; T <= 64; T++) {
        if (T > 1 && fused_single_lds_bytes(T, kn, NP) > lds_cap) break;
        const int64_t items = (int64_t)T * J;
        const double eff_pass = (double)items / (double)(((items + kBlock - 1) / kBlock) * kBlock);
        const int64_t ntiles = (F + T - 1) / T;
        const int64_t per_cu = (ntiles + num_cus - 1) / num_cus;
        const double eff_bal = (double)ntiles / (double)(per_cu * num_cus);
        double score = eff_pass * eff_bal;
        score *= (double)T / ((double)T + 1.0);  // fixed per-tile work (barriers, centre check, epilogue) ~ one frame
        if (per_cu < 2) score *= 0.80;  // one workgroup per CU = one wave per SIMD: no latency hiding (measured: 51 us vs 42 us)
        if (score > best_score + 1e-9) {
            best_score = score;
            best = T;
        }
    }
    return best;
}

template <int C, int METHOD, typename TIn, typename TOut>
int launch_fused_single(snowtri_ctx *ctx, hipStream_t st, int64_t F, int J, const TIn *d_kpts,
                        const int32_t *d_np, const Params &prm, int Pout, TOut *d_xyzs, TOut *d_ps,
                        int32_t *d_cnt, uint32_t *d_fl) {
    constexpr int NP = C * (C - 1) / 2;
    constexpr int kWgPerCu = FusedShape<C, METHOD, TIn>::kWaves;   // workgroups of four waves = waves per SIMD
    const int resident = ctx->num_cus * 2 * kWgPerCu;  // as many again queued even out the tail (measured at 2 per CU)
    const int T = choose_tile_frames(F, J, prm.kn, NP, ctx->num_cus, 0, kWgPerCu);
    const int64_t ntiles = (F + T - 1) / T;
    const int grid = (int)std::min<int64_t>(ntiles, resident);
    const size_t per_block = general_scratch_bytes(NP, J);
    int rc = ctx->cur->work.ensure(per_block * (size_t)grid);
    if (rc) return rc;
    const size_t lds = fused_single_lds_bytes(T, prm.kn, NP);
    rc = launch_kernel(ctx, st, k_fused_single<C, METHOD, TIn, TOut>, dim3(grid), dim3(kBlock), lds, false, F, J, T, ctx->rig(), d_kpts, d_np,
                       prm, Pout, d_xyzs, d_ps, d_cnt, d_fl, (char *)ctx->cur->work.p, per_block);
    if (rc) return rc;
    static const std::string name = kernel_name("k_fused_single", {std::to_string(C), std::to_string(METHOD), type_name<TIn>(), type_name<TOut>()});
    ctx->last_kernels = name.c_str();
    return SNOWTRI_OK;
}

// Production shape of the fast path (snowtri_lean.hpp): float32 outputs, keypoint_num == J == 133, one slot.
// Work is cut into wave tiles of <= kLeanTw frames of equal size (+-1 frame).
//   small batch (<= one full tile per resident wave): one tile per wave over 2 workgroups per CU;
//   larger batch: ~kLeanTilesPerWave tiles per wave and as many workgroups as that takes -- far more than fit on
//   the chip at once, so the hardware dispatcher evens out the tail (measured +3.5 % on a 2 000 000-frame launch
//   against exactly-resident persistent workgroups).
constexpr int kLeanJ = 133;
constexpr int kFusedSingleMaxCams = 4;   // k_fused_single's pairwise item (everything in registers): up to six pairs
constexpr int kLeanTilesPerWave = 4;

// The two lean kernels name their output type only where it is not float.
template <int C, typename TIn, typename TOut>
std::string lean_kernel_name(const char *kernel) {
    std::vector<std::string> args{std::to_string(C), type_name<TIn>(), std::to_string(kLeanJ)};
    if (sizeof(TOut) == 8) args.push_back("double");
    return kernel_name(kernel, args);
}

template <int C, typename TIn, typename TOut = float>
int launch_fused_lean(snowtri_ctx *ctx, hipStream_t st, int64_t F, const TIn *d_kpts, const int32_t *d_np,
                      const Params &prm, TOut *d_xyzs, TOut *d_ps, int32_t *d_cnt, uint32_t *d_fl) {
    constexpr int kScoreBytes = (int)sizeof(TOut);
    constexpr int NP = C * (C - 1) / 2;
    const int wg_small = ctx->lean_wg_per_cu, tpw = ctx->lean_tiles_per_wave > 0 ? ctx->lean_tiles_per_wave : kLeanTilesPerWave;
    const size_t per_block = general_scratch_bytes(NP, kLeanJ);
    auto kern = k_fused_lean<C, TIn, kLeanJ, TOut>;
    const int64_t W_small = (int64_t)ctx->num_cus * wg_small * kLeanWaves;
    const int64_t seg_max = (int64_t)kLeanTw * kLeanWaves * 512 * ((int64_t)ctx->num_cus * 6);  // <= 512 tiles per wave
    // lean_item's lengths in units of lambda = distance_threshold (snowtri_lean.hpp); the rolled item takes none of this
    LeanUnits<C, TOut> un{};
    if constexpr (LeanUnits<C, TOut>::kUsed) {
        un.lam = prm.dthr;
        un.inv = 1.0 / prm.dthr;
        un.kos = (0.00025 / (double)NP) / prm.dthr;
        for (int q = 0; q < NP; q++)
            for (int i = 0; i < 3; i++)   // d = t_s - t_m as snowtri_ctx_create subtracted them for Rig::pairc, times 1 / lambda
                un.d[3 * q + i] = (ctx->ht[3 * ctx->hpairs[2 * q + 1] + i] - ctx->ht[3 * ctx->hpairs[2 * q] + i]) * un.inv;
    }
    // small launch (at most kCoopMaxFrames frames per resident workgroup): workgroup tiles, passes dealt to the waves,
    // cooperative epilogue (k_fused_lean_coop)
    if (ctx->lean_coop != 0 && F <= (int64_t)ctx->num_cus * wg_small * kCoopMaxFrames) {
        const int grid = (int)std::min<int64_t>(F, (int64_t)ctx->num_cus * wg_small);
        const int base = (int)(F / grid);
        const int64_t rem = F % grid;
        const int nf_max = base + (rem ? 1 : 0);
        const size_t lds = lean_coop_lds_bytes(C, kLeanJ, nf_max, kScoreBytes);
        int rc = ctx->cur->work.ensure(per_block * (size_t)grid);
        if (rc) return rc;
        if (ctx->debug) fprintf(stderr, "k_fused_lean_coop: F %lld grid %d frames per tile %d (+1 for %lld) lds %zu\n", (long long)F, grid, base, (long long)rem, lds);
        rc = launch_kernel(ctx, st, k_fused_lean_coop<C, TIn, kLeanJ, TOut>, dim3(grid), dim3(kBlock), lds, true, F, base, rem, nf_max, ctx->rig(),
                           d_kpts, d_np, prm, un, d_xyzs, d_ps, d_cnt, d_fl, (char *)ctx->cur->work.p, per_block);
        if (rc) return rc;
        static const std::string cname = lean_kernel_name<C, TIn, TOut>("k_fused_lean_coop");
        ctx->last_kernels = cname.c_str();
        return SNOWTRI_OK;
    }
    if (ctx->timing && ctx->timing_attach && F > seg_max) {   // several kernels: bracketed (fused_dispatch records the end)
        HIP_TRY(hipEventRecord(ctx->ev[0], st));
        HIP_TRY(hipEventRecord(ctx->ev_ring[2 * (ctx->ev_count % kTimingRing)], st));
    }
    for (int64_t s0 = 0; s0 < F; s0 += seg_max) {
        const int64_t Fs = std::min<int64_t>(seg_max, F - s0);
        int64_t W;  // waves of the launch
        if (Fs <= W_small * kLeanTw) {
            W = std::min<int64_t>(W_small, Fs);
        } else {
            const int64_t tiles0 = (Fs + kLeanTw - 1) / kLeanTw;
            W = std::max<int64_t>(W_small, (tiles0 + tpw - 1) / tpw);
        }
        // every workgroup owns a slab for the frames it has to re-do: keep that scratch under 256 MB
        const size_t scratch_mb = (size_t)ctx->lean_scratch_mb;
        const int64_t grid_cap = std::max<int64_t>((int64_t)ctx->num_cus * 6, (int64_t)((scratch_mb << 20) / per_block));
        const int grid = (int)std::min<int64_t>(grid_cap, (W + kLeanWaves - 1) / kLeanWaves);
        W = (int64_t)grid * kLeanWaves;
        const int64_t tiles_per_wave = (Fs + W * kLeanTw - 1) / (W * kLeanTw);
        const int64_t ntiles = std::min<int64_t>(Fs, W * tiles_per_wave);
        const int base = (int)(Fs / ntiles);
        const int64_t rem = Fs % ntiles;
        const int slow_words = (int)((tiles_per_wave * kLeanWaves * (1 << kLeanSlowShift) + 31) / 32);
        const size_t lds = lean_lds_bytes(C, kLeanJ, slow_words, kScoreBytes);
        int rc = ctx->cur->work.ensure(per_block * (size_t)grid);
        if (rc) return rc;
        // one segment = one kernel (Fs == F, so s0 == 0): its own begin / end, as k_fused_lean_coop above
        rc = launch_kernel(ctx, st, kern, dim3(grid), dim3(kBlock), lds, Fs == F, Fs, ntiles, base, rem, slow_words, ctx->rig(),
                           d_kpts + s0 * (int64_t)(C * kLeanJ * 3), d_np ? d_np + s0 * C : nullptr, prm, un,
                           d_xyzs + s0 * (int64_t)(kLeanJ * 4), d_ps ? d_ps + s0 : nullptr, d_cnt + s0,
                           d_fl ? d_fl + s0 : nullptr, (char *)ctx->cur->work.p, per_block);
        if (rc) return rc;
        if (ctx->debug) {   // (behind the launch: the limit of a launch above 48 KB is raised by then)
            int occ = 0;
            (void)hipOccupancyMaxActiveBlocksPerMultiprocessor(&occ, kern, kBlock, lds);
            fprintf(stderr, "k_fused_lean: F %lld grid %d tiles %lld (%d frames +1 for %lld) lds %zu occupancy/CU %d\n",
                    (long long)Fs, grid, (long long)ntiles, base, (long long)rem, lds, occ);
        }
    }
    static const std::string name = lean_kernel_name<C, TIn, TOut>("k_fused_lean");
    ctx->last_kernels = name.c_str();
    return SNOWTRI_OK;
}

template <typename TIn, typename TOut>
int launch_frame_general(snowtri_ctx *ctx, hipStream_t st, int64_t F, int Pmax, int J, const TIn *d_kpts,
                         const int32_t *d_np, const Params &prm, int Pout, TOut *d_xyzs, TOut *d_ps,
                         int32_t *d_cnt, uint32_t *d_fl) {
    const int64_t Kc = snowtri_num_candidate_slots(ctx->C, Pmax);
    if (Kc > kCondenseMaxN) return SNOWTRI_ERR_BAD_ARG;
    // a single camera has no pair (Kc == 0): the kernel then writes count = 0 and zero-filled slots, like the
    // reference's empty candidate list; keep the slab size non-zero for the division below
    const size_t per_block = std::max<size_t>(256, general_scratch_bytes(Kc, J));
    int64_t grid = std::min<int64_t>(F, (int64_t)ctx->num_cus * 2);
    grid = std::max<int64_t>(1, std::min<int64_t>(grid, (int64_t)(kMaxScratchBytes / per_block)));
    int rc = ctx->cur->work.ensure(per_block * (size_t)grid);
    if (rc) return rc;
    rc = launch_kernel(ctx, st, k_frame_general<TIn, TOut>, dim3((int)grid), dim3(kBlock), condense_lds_bytes((int)Kc), false, F, Pmax, J, (int)Kc,
                       ctx->rig(), d_kpts, d_np, prm, Pout, d_xyzs, d_ps, d_cnt, d_fl, (char *)ctx->cur->work.p, per_block);
    if (rc) return rc;
    static const std::string name = kernel_name("k_frame_general", {type_name<TIn>(), type_name<TOut>()});
    ctx->last_kernels = name.c_str();
    return SNOWTRI_OK;
}

// method = SNOWTRI_DLT, one detection per camera, keypoint_num == J == 133, one slot: k_dlt_coop (snowtri_dlt_lean.hpp).  Workgroup
// tiles of equal size (+-1 frame): as many as the resident workgroups for a small batch, tiles of kCoopMaxFrames frames beyond.
template <int C, typename TIn, typename TOut>
int launch_dlt_coop(snowtri_ctx *ctx, hipStream_t st, int64_t F, const TIn *d_kpts, const int32_t *d_np, const Params &prm, TOut *d_xyzs,
                    TOut *d_ps, int32_t *d_cnt, uint32_t *d_fl) {
    const int64_t resident = (int64_t)ctx->num_cus * kDltCoopWaves;   // (2 / 3 / 4 / 6 tiles per CU: 27.2 / 26.7 / 26.5 / 27.8 us per 10 000 frames of 4 x 1)
    const int64_t tiles = std::max<int64_t>((F + kCoopMaxFrames - 1) / kCoopMaxFrames, std::min<int64_t>(F, resident));
    const int base = (int)(F / tiles);
    const int64_t rem = F % tiles;
    const int nf_max = base + (rem ? 1 : 0);
    const size_t lds = dlt_coop_lds_bytes(C, kLeanJ, nf_max, (int)sizeof(TOut));
    // one kernel: the ring's event pair rides on its dispatch
    int rc = launch_kernel(ctx, st, k_dlt_coop<C, TIn, kLeanJ, TOut>, dim3((unsigned)tiles), dim3(kBlock), lds, true, F, base, rem, nf_max,
                           ctx->rig(), d_kpts, d_np, prm, d_xyzs, d_ps, d_cnt, d_fl);
    if (rc) return rc;
    static const std::string name = kernel_name("k_dlt_coop", {std::to_string(C), type_name<TIn>(), std::to_string(kLeanJ), type_name<TOut>()});
    ctx->last_kernels = name.c_str();
    return SNOWTRI_OK;
}

// Launch shape of k_candidate_sums for a rig: threads per workgroup, LDS per workgroup, workgroups per CU.
struct SumsLaunch {
    int threads, lds, per_cu, Jc;
};
SumsLaunch sums_launch_shape(const snowtri_ctx *ctx, int Pmax, int J) {
    const int C = ctx->C, gs = p1_group_size(Pmax);
    const int64_t nitems = (int64_t)ctx->npairs * (Pmax / (gs >= 2 ? kSumsGA : 1)) * (Pmax / gs);   // (k_candidate_sums: GA x GS tiles)
    SumsLaunch L;
    // one pass over the items should keep every wave busy: 256 threads for the small rigs, the whole CU for the large.
    L.threads = ctx->sums_threads > 0 ? ctx->sums_threads : (nitems <= 256 ? 256 : (nitems <= 768 ? 512 : 1024));
    L.threads = L.threads <= 256 ? 256 : (L.threads <= 512 ? 512 : 1024);   // the instantiated shapes
    L.lds = ctx->sums_lds_kb > 0 ? ctx->sums_lds_kb * 1024 : (L.threads <= 256 ? 52 * 1024 : (L.threads <= 512 ? 80 * 1024 : 160 * 1024));
    L.lds = std::min(L.lds, 160 * 1024);
    L.per_cu = std::max(1, std::min((160 * 1024) / L.lds, 2048 / L.threads));
    const int pf = L.threads == 256 ? SumsShape<256>::kPrefetch : (L.threads == 512 ? SumsShape<512>::kPrefetch : SumsShape<1024>::kPrefetch);
    L.Jc = sums_chunk_joints(C, Pmax, J, ctx->npairs, L.threads, pf, L.lds);
    return L;
}

// Multi-person path without HBM candidate spill: k_frame_recompute (snowtri_general.hpp), or -- float32 outputs,
// pairwise method, <= 16 cameras -- the streaming association of snowtri_assoc.hpp with k_frame_recompute for the frames
// it leaves behind.  What a call of launch_frame_recompute does is decided here, from its shape and the context's settings
// alone (no HIP call, no scratch); the stages below read it.
struct RecomputeRoute {
    bool can_hand, sumless, sums_kn, post_scores, stream, handover;
    bool split;          // the segments alternate between the caller's stream set and an internal one
    SumsLaunch SL;       // (stream)
    int64_t seg;         // frames per segment
    long long names_key; // what the route's kernel names depend on (snowtri_ctx::names_key)
};
RecomputeRoute recompute_route(const snowtri_ctx *ctx, int METHOD, size_t in_size, size_t out_size, int64_t F, int Pmax, int J, const Params &prm,
                               int Pout) {
    const int64_t Kc = snowtri_num_candidate_slots(ctx->C, Pmax);
    const int C = ctx->C, R = C * Pmax;
    RecomputeRoute r{};
    // Hand-over of the output persons to the streaming fusion kernels (snowtri_cluster.hpp): pairwise method, 4-bit person
    // fields, non-negative scores (kthr >= 0).  A person's mean score (:150) is derived from the candidate means when
    // keypoint_num == J and the outputs are float32; otherwise k_person_scores takes it from the fused joints afterwards.  The
    // filter of :151-152 -- which the association must decide BEFORE it assigns the slots -- is vacuous for condense_score_tol
    // <= 0 (the reference's default); keypoint_num < J with an active filter costs a second launch of k_candidate_sums over
    // the first keypoint_num joints (kn / J of the first).
    // handover_mode 1: the streaming association (<= 16 cameras); 2: descriptors written by k_frame_recompute itself
    // (<= 8 cameras, float32 outputs, keypoint_num == J: register-resident rays in k_cluster_fuse), staged in its arena.
    // METHOD = 1 (DLT behind the reference's association, row N3): the streaming association too, then k_cluster_dlt on its
    // descriptors.  A person's mean score there is the mean of the DLT joint scores (mean confidences >= keypoint_score_threshold
    // >= 0), which the association cannot know: the route is taken when the filter of :151-152 cannot drop anybody
    // (condense_score_tol <= 0, the reference's default); otherwise the frames stay on k_frame_recompute<1>.
    r.can_hand = C >= 2 && Pmax <= kClusterMaxPersons && prm.kn >= 1 && J <= 256 && prm.kthr >= 0.0 && Pout >= 1 &&
                 (size_t)Pout * 24 + 80 <= (size_t)kRayChunkBytes && !(prm.score_tol != prm.score_tol) &&
                 (METHOD == 0 || prm.score_tol <= 0.0);
    // ONE detection per camera with average_score_threshold <= 0 <= keypoint_score_threshold and no mean-score filter: every
    // listed candidate is kept whatever its mean (:80-81; scores that pass the keypoint gate are >= 0), so the candidate pass
    // has nothing to decide.  It is skipped (`sumless`): k_associate reads a constant positive sum for every slot, the
    // persons' mean scores come from the fused joints (k_person_scores), and a singular pair is flagged where its joint is
    // fused (cluster_joint_sequential / cluster_member_passes).  This is the route of single-person rigs of five and more
    // cameras on the shapes the lean kernels do not take (fused_dispatch).
    r.sumless = METHOD == 0 && Pmax == 1 && prm.avg_thr <= 0.0 && prm.kthr >= 0.0 && prm.score_tol <= 0.0 && ctx->sumless_mode != 0;
    r.sums_kn = !r.sumless && prm.kn != J && !(prm.score_tol <= 0.0);   // second candidate-sum launch over the first keypoint_num joints
    r.post_scores = r.sumless || out_size == 8 || prm.kn != J || METHOD == 1;   // the persons' mean scores by k_person_scores
    // (distance_threshold >= 0: k_candidate_sums reads its distance gate off a sign bit, p1_tile_sums)
    r.stream = r.can_hand && ctx->handover_mode == 1 && C <= 16 && Kc < ((int64_t)1 << 24) && Pout <= 1024 && (r.sumless || prm.dthr >= 0.0);
    if (r.stream) {
        r.SL = sums_launch_shape(ctx, Pmax, J);
        r.stream = r.SL.Jc >= 1;
    }
    r.handover = METHOD == 0 && !r.stream && r.can_hand && out_size == 4 && prm.kn == J && ctx->handover_mode != 0 && C <= kClusterMaxCams;
    // the two descriptor lists hold Pout persons for every frame of a segment (<= 2 M entries each, 64 MB together), the
    // member list Kc words per frame (<= 64 M words, 256 MB); row indices are 32-bit; the candidate sums of the
    // streaming association 8 Kc bytes per frame (<= 1 GB).  Sized for the LARGE rigs: a frame of 16 x 8 holds a CU for
    // ~225 us of its candidate pass, a launch ends with up to one such frame per CU in its tail, and 12 500 frames in
    // four segments of 3 125 (12 frames per CU) paid that tail four times -- now two segments of 6 250.
    int64_t seg_frames = F;
    if (r.stream || r.handover)
        seg_frames = std::max<int64_t>(1, std::min<int64_t>(std::min<int64_t>(((int64_t)2 << 20) / Pout, ((int64_t)64 << 20) / Kc),
                                                          ((int64_t)1 << 31) / R));
    if (r.stream) seg_frames = std::max<int64_t>(1, std::min<int64_t>(seg_frames, ((int64_t)128 << 20) / Kc));
    const int64_t seg_cap = ctx->handover_seg_frames > 0 ? ctx->handover_seg_frames : seg_frames;
    r.seg = (r.stream || r.handover) ? std::min(seg_frames, seg_cap) : F;
    // ONE call in (at least) two segments on two stream sets: every kernel of the streaming route holds the whole chip
    // while it runs, and a third of the route's time is latency-bound (k_associate: VALU busy ~20 %, the member lists);
    // with the segments alternating between the caller's stream and an internal one, those kernels of one segment run
    // beside the VALU-bound ones of the other (8 x 4: +8 % against one stream; what round 3 measured with two CALLS in
    // flight on two contexts, now inside the call).  Outputs do not depend on the cut (tests/test_gpu_handover.py).  Not
    // in overlap mode (whole calls already alternate over the sets) and not for batches too small to fill the chip twice.
    // (rigs whose candidate pass holds a whole CU per workgroup -- 16 x 8: 1024 threads, 160 KB -- gain little, only the tails
    // of the kernels fill one another: 17.20 -> 17.01 ms per 12 500 frames, six interleaved runs.  Staggering the segments --
    // the second candidate pass waiting for the first so that it runs beside the first's latency-bound kernels -- LOSES:
    // 8 x 4 1.10 -> 1.24 ms; two half-size candidate passes side by side fill each other's tails, one alone does not.)
    r.split = r.stream && ctx->split_segments >= 2 && ctx->overlap <= 1 && ctx->cur == &ctx->sets[0];
    if (r.split) {
        int64_t nseg = std::max<int64_t>((F + r.seg - 1) / r.seg, ctx->split_segments);
        nseg += nseg & 1;
        const int64_t even = (F + nseg - 1) / nseg;
        if (even >= (ctx->split_forced ? 1 : (int64_t)ctx->num_cus * 4))   // (the knob set explicitly: tests split small batches too)
            r.seg = even;
        else
            r.split = false;
    }
    r.names_key = ((long long)C << 8) | (METHOD << 7) | ((int)in_size << 3) | ((int)out_size >> 2 << 2) | (r.stream ? 2 : 0) |
                  (r.handover ? 1 : 0) | ((long long)r.SL.threads << 16) | ((long long)(r.sumless ? 1 : 0) << 32) | ((long long)Pmax << 34);
    return r;
}

// The kernels of a route, in launch order (rebuilt only when the route changes).
template <int METHOD, typename TIn, typename TOut>
void recompute_route_names(snowtri_ctx *ctx, const RecomputeRoute &r) {
    if (r.names_key != ctx->names_key) {
        const int C = ctx->C;
        const std::string tin = type_name<TIn>(), tout = type_name<TOut>();
        const std::string rec = kernel_name("k_frame_recompute", {std::to_string(METHOD), tin, tout});
        const std::string fuse = (C <= kClusterMaxCams ? kernel_name("k_cluster_fuse", {std::to_string(C), tin}) : kernel_name("k_cluster_fuse_wide", {tin})) +
                                 " + " + kernel_name("k_cluster_members", {tin});
        const std::string sums = kernel_name("k_candidate_sums", {tin, std::to_string(r.SL.threads)}) + " + " + kernel_name("k_candidate_sums_exact", {tin});
        const std::string assoc = kernel_name("k_associate", {tin}), scores = kernel_name("k_person_scores", {tout});
        if (r.stream && METHOD == 1)
            ctx->names_buf = sums + " + " + assoc + " + " + kernel_name("k_cluster_dlt", {std::to_string(C <= kClusterMaxCams ? C : 0), tin, tout}) +
                             " + " + scores + " + " + rec + " (frames left behind)";
        else if (r.stream && r.sumless)
            ctx->names_buf = kernel_name("k_singular_scan", {tin}) + " + " + assoc + " + " + fuse + " + " + scores + " + " + rec + " (frames left behind)";
        else if (r.stream)
            ctx->names_buf = sums + " + " + assoc + " + " + fuse + " + " + rec + " (frames left behind)";
        else if (r.handover)
            ctx->names_buf = rec + " + " + fuse;
        else
            ctx->names_buf = rec;
        ctx->names_key = r.names_key;
    }
    ctx->last_kernels = ctx->names_buf.c_str();
}

// Resident workgroups per CU of k_frame_recompute<METHOD, TIn, TOut> at `lds` bytes (queried once per LDS size).
template <int METHOD, typename TIn, typename TOut>
int recompute_per_cu(snowtri_ctx *ctx, size_t lds, int R, int64_t Kc, int *per_cu) {
    auto kern = k_frame_recompute<METHOD, TIn, TOut>;
    snowtri_ctx::OccCache &oc = ctx->recompute_occ[METHOD * 4 + (sizeof(TIn) == 8 ? 2 : 0) + (sizeof(TOut) == 8 ? 1 : 0)];
    if (oc.per_cu < 0 || oc.lds != lds) {
        // exactly the workgroups that are resident at once (registers and the ~50 KB of LDS decide: 3 per CU);
        // they pull frames from an atomic counter until none are left
        if (int rc = raise_lds_or_fail(ctx, (const void *)kern, lds)) return rc;
        int q = 0;
        HIP_TRY(hipOccupancyMaxActiveBlocksPerMultiprocessor(&q, kern, kBlock, lds));
        oc.lds = lds;
        oc.per_cu = q;
        if (ctx->debug) fprintf(stderr, "k_frame_recompute: R %d Kc %lld lds %zu occupancy/CU %d\n", R, (long long)Kc, lds, q);
    }
    *per_cu = oc.per_cu;
    return SNOWTRI_OK;
}

// A launch_frame_recompute call: its shape, what k_frame_recompute needs at that shape, and the caller's arrays.
template <typename TIn, typename TOut>
struct RecomputeCall {
    int Pmax, J, Pout;
    int64_t Kc;
    const Params &prm;
    size_t lds, per_block;      // k_frame_recompute's LDS and slab
    int per_cu;                 // ... and resident workgroups per CU
    unsigned long long kmagic;  // item / keypoint_num
    const TIn *kpts;
    const int32_t *np;
    TOut *xyzs, *ps;
    int32_t *cnt;
    uint32_t *fl;
};

// One segment of it: stream, stream set, frames, the segment's part of the arrays, its lists and counters, and what one stage
// leaves for the next.
template <typename TIn, typename TOut>
struct RecomputeSegment {
    const RecomputeCall<TIn, TOut> &call;
    hipStream_t st;
    StreamSet *set;
    int64_t Fs, grid;           // frames; workgroups of a k_frame_recompute launch over all of them
    const TIn *kpts;
    const int32_t *np;
    TOut *xyzs, *ps;
    int32_t *cnt;
    uint32_t *fl;
    ClusterDesc *desc;          // the descriptor lists: complete graphs in desc[0, cap), the others in desc[cap, 2 cap) with their
    uint32_t *words;            // member words in `words` (word_cap of them)
    uint32_t cap, word_cap;
    unsigned long long *next_frame, *hand_counters, *slow_count, *exact_count, *slow_count2, *sums_ticket;
    // candidate stage -> association
    double *csum, *csum_kn;
    uint32_t *slow_list, *exact_list;
    // association -> k_frame_recompute: the frames left behind
    const uint32_t *final_slow_list;
    const unsigned long long *final_slow_count;
};

// Segment [s0, s0 + Fs) of g.call on stream set S: the slabs and descriptor lists it needs, its counters cleared on `st`.
template <typename TIn, typename TOut>
int open_segment(snowtri_ctx *ctx, const RecomputeRoute &r, StreamSet &S, hipStream_t st, int64_t s0, int64_t Fs, RecomputeSegment<TIn, TOut> &g) {
    const RecomputeCall<TIn, TOut> &call = g.call;
    const int C = ctx->C, R = C * call.Pmax;
    ctx->cur = &S;
    ctx->last_set = &S;
    g.st = st;
    g.set = &S;
    g.Fs = Fs;
    g.next_frame = S.d_counters + 2, g.hand_counters = S.d_counters + kHandCountersAt, g.slow_count = S.d_counters + 6;
    g.exact_count = S.d_counters + 7, g.slow_count2 = S.d_counters + 8, g.sums_ticket = S.d_counters + 9;
    g.grid = std::min<int64_t>(Fs, (int64_t)ctx->num_cus * std::max(1, call.per_cu));
    g.grid = std::max<int64_t>(1, std::min<int64_t>(g.grid, (int64_t)(kMaxScratchBytes / call.per_block)));
    int rc = S.work.ensure(call.per_block * (size_t)g.grid);
    if (rc) return rc;
    g.cap = 0, g.word_cap = 0;
    g.desc = nullptr;
    g.words = nullptr;
    if (r.stream || r.handover) {
        ctx->last_handover = true;
        g.cap = (uint32_t)(Fs * call.Pout);
        g.word_cap = (uint32_t)(Fs * call.Kc);
        rc = S.desc.ensure((size_t)2 * g.cap * sizeof(ClusterDesc) + (size_t)g.word_cap * 4);
        if (rc) return rc;
        g.desc = (ClusterDesc *)S.desc.p;
        g.words = (uint32_t *)(g.desc + (size_t)2 * g.cap);
    }
    HIP_TRY(hipMemsetAsync(g.next_frame, 0, (kCounterWords - 2) * sizeof(unsigned long long), st));   // next_frame, slow / exact / slow (second pass) frames, the frame tickets of k_candidate_sums, the hand-over list counters
    g.kpts = call.kpts + s0 * (int64_t)R * call.J * 3;
    g.np = call.np ? call.np + s0 * C : nullptr;
    g.xyzs = call.xyzs + s0 * (int64_t)call.Pout * call.prm.kn * 4;
    g.ps = call.ps ? call.ps + s0 * call.Pout : nullptr;
    g.cnt = call.cnt + s0;
    g.fl = call.fl ? call.fl + s0 : nullptr;
    return SNOWTRI_OK;
}

// ---- the stages of a segment.  Streaming route: candidates -> association -> fusion (-> person scores) -> k_frame_recompute on
// the frames left behind.

// The candidate pass: k_candidate_sums (and again over the first keypoint_num joints) + k_candidate_sums_exact; without one
// (`sumless`) the constant sums and k_singular_scan.
template <typename TIn, typename TOut>
int stage_candidates(snowtri_ctx *ctx, const RecomputeRoute &r, RecomputeSegment<TIn, TOut> &g) {
    const RecomputeCall<TIn, TOut> &c = g.call;
    const int64_t Fs = g.Fs, Kc = c.Kc;
    const SumsLaunch &SL = r.SL;
    const size_t sum_bytes = ((size_t)Fs * Kc * 8 + 255) & ~(size_t)255;
    int rc = g.set->sums.ensure((r.sums_kn ? 2 : 1) * sum_bytes + (size_t)Fs * 12 + 256);   // + the frames left behind (two passes) + the frames to re-do exactly
    if (rc) return rc;
    g.csum = (double *)g.set->sums.p;
    g.csum_kn = r.sums_kn ? (double *)((char *)g.set->sums.p + sum_bytes) : nullptr;
    g.slow_list = (uint32_t *)((char *)g.set->sums.p + (r.sums_kn ? 2 : 1) * sum_bytes);
    g.exact_list = g.slow_list + Fs;
    const int grid1 = (int)std::min<int64_t>(Fs, (int64_t)ctx->num_cus * SL.per_cu);
    if (ctx->debug) {
        const AssocShape ash = associate_shape(ctx->C, ctx->npairs, c.Pout, Kc);
        fprintf(stderr, "k_candidate_sums: threads %d lds %d per_cu %d grid %d Jc %d | k_associate rounds in registers %d lds %zu\n",
                SL.threads, SL.lds, SL.per_cu, grid1, SL.Jc, ash.rc, ash.lds);
    }
    if (r.sumless) {
        // every byte 0x3f: the double 4.7e-4 in every slot -- positive, finite, kept by :80-81 for any threshold <= 0
        HIP_TRY(hipMemsetAsync(g.csum, 0x3f, (size_t)Fs * Kc * 8, g.st));
        if (!g.fl) return SNOWTRI_OK;
        HIP_TRY(hipMemsetAsync(g.fl, 0, (size_t)Fs * sizeof(uint32_t), g.st));   // (the candidate pass clears the flags otherwise)
        // ... and finds every singular pair of every listed candidate and joint; here a scan asks that one question
        // (the flag must not depend on the route: k_singular_scan, snowtri_assoc.hpp)
        return launch_kernel(ctx, g.st, k_singular_scan<TIn>, dim3(grid_for(Fs * (int64_t)c.J, kBlock, ctx->num_cus * 16)), dim3(kBlock), 0, false, Fs,
                             c.J, ctx->rig(), g.kpts, g.np, g.fl);
    }
    with_sums_threads(SL.threads, [&](auto tt) {
        constexpr int TT = decltype(tt)::value;
        auto k1 = k_candidate_sums<TIn, TT>;
        rc = launch_kernel(ctx, g.st, k1, dim3(grid1), dim3(TT), (size_t)SL.lds, false, Fs, c.Pmax, c.J, c.J, (int)Kc, ctx->rig(), g.kpts, g.np, c.prm,
                           g.csum, g.fl, g.exact_list, g.exact_count, g.sums_ticket, SL.lds);
        if (!rc && r.sums_kn)   // the sums over the first keypoint_num joints, on a ticket counter of their own
            rc = launch_kernel(ctx, g.st, k1, dim3(grid1), dim3(TT), (size_t)SL.lds, false, Fs, c.Pmax, c.prm.kn, c.J, (int)Kc, ctx->rig(), g.kpts,
                               g.np, c.prm, g.csum_kn, (uint32_t *)nullptr, (uint32_t *)nullptr, g.exact_count, g.sums_ticket + 1, SL.lds);
    });
    if (rc) return rc;
    // the frames it listed (exact_count of them, known on the device only; normally none)
    return launch_kernel(ctx, g.st, k_candidate_sums_exact<TIn>, dim3((int)std::min<int64_t>(Fs, ctx->num_cus)), dim3(kBlock), 0, false, c.Pmax, c.J,
                         (int)Kc, ctx->rig(), g.kpts, g.np, c.prm, g.csum, g.fl, (const uint32_t *)g.exact_list,
                         (const unsigned long long *)g.exact_count);
}

// k_associate: the persons of every frame into the descriptor lists; the frames it cannot take are listed for k_frame_recompute.
template <typename TIn, typename TOut>
int stage_associate(snowtri_ctx *ctx, const RecomputeRoute &r, RecomputeSegment<TIn, TOut> &g) {
    const RecomputeCall<TIn, TOut> &c = g.call;
    const int C = ctx->C;
    const int64_t Fs = g.Fs, Kc = c.Kc;
    // first launch: centres in registers where the rig's true pairs fit 4 / 16 rounds of 64 (snowtri_assoc.hpp)
    const AssocShape ash = associate_shape(C, ctx->npairs, c.Pout, Kc);
    auto k2 = k_associate<TIn, TOut, 0>;   // the second launch (every slot in LDS)
    auto k2a = ash.rc == 4 ? k_associate<TIn, TOut, 4> : (ash.rc == 16 ? k_associate<TIn, TOut, 16> : k2);
    const size_t lds2 = ash.lds;
    // small rigs: 16 waves per CU, each striding over the frames; large rigs (a frame takes > 100 us and only a few
    // fit a CU's LDS): one frame per workgroup, the dispatcher evens out the tail
    const int grid2 = (int)std::min<int64_t>(Fs, lds2 > 10 * 1024 ? Fs : (int64_t)ctx->num_cus * ctx->assoc_wg_per_cu);
    int rc = launch_kernel(ctx, g.st, k2a, dim3(grid2), dim3(64), lds2, false, Fs, c.Pmax, c.J, (int)Kc, ctx->rig(), g.kpts, g.np, c.prm, c.Pout,
                           g.csum, g.xyzs, g.ps, g.cnt, g.fl, g.desc, g.words, g.hand_counters, g.cap, g.word_cap, g.slow_list, g.slow_count,
                           (int)lds2, 1, (const uint32_t *)nullptr, (const unsigned long long *)nullptr, r.post_scores ? 0 : 1,
                           (const double *)g.csum_kn);
    if (rc) return rc;
    // the frames whose kept candidates did not fit that LDS (slow_count of them, known on the device only; none on
    // the reference's workloads): again with room for every slot, one wave per CU; what this launch lists is
    // left to k_frame_recompute
    g.final_slow_list = g.slow_list;
    g.final_slow_count = g.slow_count;
    const size_t lds2_full = associate_lds_bytes_full(C, ctx->npairs, c.Pout, Kc);
    if (lds2_full <= lds2) return SNOWTRI_OK;
    uint32_t *slow_list2 = g.exact_list + Fs;
    const int per_cu2 = (int)std::max<size_t>(1, std::min<size_t>(8, (160 * 1024) / lds2_full));
    rc = launch_kernel(ctx, g.st, k2, dim3((int)std::min<int64_t>(Fs, (int64_t)ctx->num_cus * per_cu2)), dim3(64), lds2_full, false, Fs, c.Pmax, c.J,
                       (int)Kc, ctx->rig(), g.kpts, g.np, c.prm, c.Pout, g.csum, g.xyzs, g.ps, g.cnt, g.fl, g.desc, g.words, g.hand_counters, g.cap,
                       g.word_cap, slow_list2, g.slow_count2, (int)lds2_full, 1, (const uint32_t *)g.slow_list,
                       (const unsigned long long *)g.slow_count, r.post_scores ? 0 : 1, (const double *)g.csum_kn);
    if (rc) return rc;
    g.final_slow_list = slow_list2;
    g.final_slow_count = g.slow_count2;
    return SNOWTRI_OK;
}

// The streaming kernels for the descriptors the association (or a k_frame_recompute launch over Fs frames) left behind
// (snowtri_cluster.hpp): `cnt[0]` complete-graph clusters in desc[0, cap), `cnt[1]` clusters of any other shape in desc[cap, 2 cap)
// with their member words in `words`.  Pairwise method: k_cluster_fuse (up to 8 cameras: register-resident rays) or
// k_cluster_fuse_wide for the complete graphs, then k_cluster_members; DLT: k_cluster_dlt for both lists.
template <int METHOD, typename TIn, typename TOut>
int stage_fusion(snowtri_ctx *ctx, const RecomputeRoute &r, RecomputeSegment<TIn, TOut> &g) {
    const RecomputeCall<TIn, TOut> &c = g.call;
    const int C = ctx->C, kn = c.prm.kn;
    const int64_t Fs = g.Fs;
    const int64_t passes_max = (Fs * c.Pout * (int64_t)kn + 63) / 64;
    int rc = SNOWTRI_OK;
    if constexpr (METHOD == 1) {
        // both descriptor lists in one launch: an N-view DLT per (output person, joint)
        const int gridd = (int)std::max<int64_t>(1, std::min<int64_t>((passes_max + 3) / 4, (int64_t)ctx->num_cus * kClusterDltWaves));
        auto dlt = [&](auto cc) {
            rc = launch_kernel(ctx, g.st, k_cluster_dlt<decltype(cc)::value, TIn, TOut>, dim3(gridd), dim3(kBlock), cluster_dlt_lds_bytes(C), false,
                               g.desc, g.words, g.hand_counters, g.cap, ctx->rig(), g.kpts, c.prm, c.Pmax, c.J, kn, c.kmagic, c.Pout, g.xyzs);
        };
        if (!with_cameras<2, kClusterMaxCams>(C, dlt)) dlt(std::integral_constant<int, 0>());   // more than 8 cameras
        return rc;
    } else {
        const bool narrow = with_cameras<2, kClusterMaxCams>(C, [&](auto cc) {
            // exactly the waves that are resident at once (kClusterWaves per SIMD at this kernel's registers), each striding over
            // the passes: with the member lists in a kernel of their own every pass costs the same, and short-lived workgroups only
            // added their start-up (8 x 4: 334 -> 312 us).  (k_cluster_members on a second stream beside this kernel: measured, no gain.)
            const int64_t W = std::min<int64_t>(passes_max, (int64_t)ctx->num_cus * 4 * kClusterWaves);
            const int grid = (int)std::max<int64_t>(1, std::min<int64_t>((W + kBlock / 64 - 1) / (kBlock / 64), (int64_t)ctx->num_cus * 64));
            rc = launch_kernel(ctx, g.st, k_cluster_fuse<decltype(cc)::value, TIn, TOut>, dim3(grid), dim3(kBlock), cluster_lds_bytes(C), false, g.desc,
                               g.hand_counters, g.cap, ctx->rig(), g.kpts, c.prm, c.Pmax, c.J, kn, c.kmagic, c.Pout, g.xyzs, g.fl);
        });
        // (the hand-over from inside k_frame_recompute has no wide kernel: only a build without this camera count gets here)
        if (!narrow && !r.stream) return SNOWTRI_ERR_BAD_ARG;
        if (!narrow) {   // more than 8 cameras: complete graphs with their rays in LDS
            const int64_t wpasses = (Fs * c.Pout * (int64_t)kn + 15) / 16;   // 16 items per wave pass
            const int ppw_wide = 8;   // (many short-lived workgroups here: 6 -> 886, 24 -> 906, 400 -> 1042 us per 4 000 frames of 16 x 8)
            const int gridw = (int)std::max<int64_t>(1, std::min<int64_t>((wpasses + 4 * ppw_wide - 1) / (4 * ppw_wide), (int64_t)ctx->num_cus * 64));
            rc = launch_kernel(ctx, g.st, k_cluster_fuse_wide<TIn, TOut>, dim3(gridw), dim3(kBlock), cluster_wide_lds_bytes(C), false, g.desc,
                               g.hand_counters, g.cap, ctx->rig(), g.kpts, c.prm, c.Pmax, c.J, kn, c.kmagic, c.Pout, g.xyzs, g.fl);
        }
        if (rc) return rc;
        // ... then the member lists
        const int gridm = (int)std::max<int64_t>(1, std::min<int64_t>((passes_max + 3) / 4, (int64_t)ctx->num_cus * 16));
        return launch_kernel(ctx, g.st, k_cluster_members<TIn, TOut>, dim3(gridm), dim3(kBlock), cluster_members_lds_bytes(C, ctx->npairs), false, g.desc,
                             g.words, g.hand_counters, g.cap, ctx->rig(), g.kpts, c.prm, c.Pmax, c.J, kn, c.kmagic, c.Pout, g.xyzs, g.fl);
    }
}

// The persons' mean scores from the fused joints (keypoint_num < J, float64 outputs).
template <typename TIn, typename TOut>
int stage_person_scores(snowtri_ctx *ctx, RecomputeSegment<TIn, TOut> &g) {
    const RecomputeCall<TIn, TOut> &c = g.call;
    const int gridp = (int)std::max<int64_t>(1, std::min<int64_t>((g.Fs * c.Pout + 3) / 4, (int64_t)ctx->num_cus * 32));
    return launch_kernel(ctx, g.st, k_person_scores<TOut>, dim3(gridp), dim3(kBlock), 0, false, g.Fs, c.Pout, c.prm.kn, (const TOut *)g.xyzs, g.ps,
                         (const int32_t *)g.cnt);
}

// k_frame_recompute: over the whole segment (writing the descriptor lists where the route hands over), or -- `left_behind` -- over
// the frames k_associate listed (slow_count of them, known on the device only): phase 3 inside the kernel.
template <int METHOD, typename TIn, typename TOut>
int stage_recompute(snowtri_ctx *ctx, RecomputeSegment<TIn, TOut> &g, bool left_behind) {
    const RecomputeCall<TIn, TOut> &c = g.call;
    const int64_t grid = left_behind ? std::max<int64_t>(1, std::min<int64_t>(g.grid, ctx->num_cus)) : g.grid;
    return launch_kernel(ctx, g.st, k_frame_recompute<METHOD, TIn, TOut>, dim3((int)grid), dim3(kBlock), c.lds, false, g.Fs, c.Pmax, c.J, (int)c.Kc,
                         ctx->rig(), g.kpts, g.np, c.prm, c.Pout, g.xyzs, g.ps, g.cnt, g.fl, (char *)g.set->work.p, c.per_block, g.next_frame,
                         (int)c.lds, left_behind ? (ClusterDesc *)nullptr : g.desc, left_behind ? (uint32_t *)nullptr : g.words, g.hand_counters,
                         left_behind ? 0u : g.cap, left_behind ? 0u : g.word_cap, left_behind ? g.final_slow_list : (const uint32_t *)nullptr,
                         left_behind ? g.final_slow_count : (const unsigned long long *)nullptr);
}

template <int METHOD, typename TIn, typename TOut>
int launch_frame_recompute(snowtri_ctx *ctx, hipStream_t st_call, int64_t F, int Pmax, int J, const TIn *d_kpts,
                           const int32_t *d_np, const Params &prm, int Pout, TOut *d_xyzs, TOut *d_ps,
                           int32_t *d_cnt, uint32_t *d_fl) {
    const int64_t Kc = snowtri_num_candidate_slots(ctx->C, Pmax);
    const int C = ctx->C;
    const unsigned long long kn1 = (unsigned long long)std::max(1, prm.kn);
    // three workgroups per CU share the 160 KB of LDS (snowtri_general.hpp: the arena behind the tables is reused
    // phase by phase)
    RecomputeCall<TIn, TOut> call{Pmax, J, Pout, Kc, prm, recompute_launch_lds(C, ctx->npairs), recompute_scratch_bytes(Kc, C * Pmax, prm.kn), 0,
                                  (((unsigned long long)1 << 40) + kn1 - 1) / kn1, d_kpts, d_np, d_xyzs, d_ps, d_cnt, d_fl};
    int rc = recompute_per_cu<METHOD, TIn, TOut>(ctx, call.lds, C * Pmax, Kc, &call.per_cu);
    if (rc) return rc;
    const RecomputeRoute r = recompute_route(ctx, METHOD, sizeof(TIn), sizeof(TOut), F, Pmax, J, prm, Pout);
    StreamSet *const set_call = ctx->cur;
    if (r.split) {
        if (ctx->ensure_set(1, true, st_call)) {
            g_last_error = "creating the internal stream of the multi-person split failed";
            return SNOWTRI_ERR_HIP;
        }
        HIP_TRY(hipEventRecord(ctx->ev_fork, st_call));
        HIP_TRY(hipStreamWaitEvent(ctx->sets[1].stream, ctx->ev_fork, 0));
    }
    // Whatever way this function is left, the caller's stream continues BEHIND the internal one: a segment already queued
    // there writes the caller's outputs, and an error return in the middle of the loop must not leave it unordered with the
    // caller's stream.  The regular exit joins explicitly and disarms the guard.
    struct SplitJoin {
        snowtri_ctx *ctx;
        hipStream_t caller;
        StreamSet *set_call;
        bool armed;
        ~SplitJoin() {
            ctx->cur = set_call;
            if (armed && hipEventRecord(ctx->sets[1].done, ctx->sets[1].stream) == hipSuccess)
                (void)hipStreamWaitEvent(caller, ctx->sets[1].done, 0);
        }
    } split_join{ctx, st_call, set_call, r.split};
    recompute_route_names<METHOD, TIn, TOut>(ctx, r);
    RecomputeSegment<TIn, TOut> g{call};
    int seg_index = 0;
    for (int64_t s0 = 0; s0 < F; s0 += r.seg, seg_index++) {
        const bool internal = r.split && (seg_index & 1);
        StreamSet &S = internal ? ctx->sets[1] : *set_call;
        if ((rc = open_segment(ctx, r, S, internal ? S.stream : st_call, s0, std::min<int64_t>(r.seg, F - s0), g))) return rc;
        if (r.stream) {
            if ((rc = stage_candidates(ctx, r, g))) return rc;
            if ((rc = stage_associate(ctx, r, g))) return rc;
        } else if ((rc = stage_recompute<METHOD>(ctx, g, false))) {
            return rc;
        }
        if (r.stream || r.handover)
            if ((rc = stage_fusion<METHOD>(ctx, r, g))) return rc;
        if (r.stream && r.post_scores && g.ps)
            if ((rc = stage_person_scores(ctx, g))) return rc;
        if (r.stream)
            if ((rc = stage_recompute<METHOD>(ctx, g, true))) return rc;
    }
    ctx->cur = set_call;
    if (r.split) {   // the caller's stream continues behind the internal one
        split_join.armed = false;
        HIP_TRY(hipEventRecord(ctx->sets[1].done, ctx->sets[1].stream));
        HIP_TRY(hipStreamWaitEvent(st_call, ctx->sets[1].done, 0));
    }
    ctx->last_stream = r.stream;
    return SNOWTRI_OK;
}

// What method = SNOWTRI_DLT_ROBUST needs beyond the fused call's arguments: the settings (the context's, or the explicit ones of
// snowtri_triangulate_robust) and the two optional per-joint diagnostics (device pointers by the time the launcher sees them).
struct RobustCall {
    double threshold_px = 6.0;
    int32_t max_drops = 1;
    uint32_t *views = nullptr;   // [F][kn]
    void *resid = nullptr;       // [F][kn] of the output type
};

// method = SNOWTRI_DLT_ROBUST: k_dlt_robust (snowtri_robust.hpp), one workgroup per tile of T frames.  T fills the chip for a small
// batch and is capped by kRobustMaxTile and by the LDS stash of the tile's joint scores; results do not depend on it.
template <int C, typename TIn, typename TOut>
int launch_dlt_robust(snowtri_ctx *ctx, hipStream_t st, int64_t F, int J, const TIn *d_kpts, const int32_t *d_np, const Params &prm,
                      const RobustCall &rb, int Pout, TOut *d_xyzs, TOut *d_ps, int32_t *d_cnt, uint32_t *d_fl) {
    const int kn = std::max(1, prm.kn);
    const int64_t resident = (int64_t)ctx->num_cus * kRobustWaves;
    int64_t T = std::min<int64_t>(kRobustMaxTile, (F + resident - 1) / resident);
    T = std::max<int64_t>(1, std::min<int64_t>(T, (int64_t)(32 * 1024) / (8 * (int64_t)kn)));
    const int64_t tiles = (F + T - 1) / T;
    const size_t lds = robust_lds_bytes(C, (int)T, prm.kn);
    if (lds > (size_t)160 * 1024 || tiles > 0x7fffffffll) {
        g_last_error = "SNOWTRI_DLT_ROBUST: keypoint_num too large for the LDS stash of one frame (or more than 2^31 tiles)";
        return SNOWTRI_ERR_BAD_ARG;
    }
    const double tau2 = rb.threshold_px * rb.threshold_px;
    // one kernel: the ring's event pair rides on its dispatch
    int rc = launch_kernel(ctx, st, k_dlt_robust<C, TIn, TOut>, dim3((unsigned)tiles), dim3(kBlock), lds, true, F, J, (int)T, ctx->rig(), d_kpts, d_np,
                           prm, tau2, (int)rb.max_drops, Pout, d_xyzs, d_ps, d_cnt, d_fl, rb.views, (TOut *)rb.resid);
    if (rc) return rc;
    static const std::string name = kernel_name("k_dlt_robust", {std::to_string(C), type_name<TIn>(), type_name<TOut>()});
    ctx->last_kernels = name.c_str();
    return SNOWTRI_OK;
}

template <typename TIn, typename TOut>
int fused_dispatch(snowtri_ctx *ctx, hipStream_t st, int64_t F, int Pmax, int J, const void *kpts,
                   const int32_t *d_np, const Params &prm, int Pout, void *xyzs, void *ps, int32_t *d_cnt,
                   uint32_t *d_fl, int method, const RobustCall &rb) {
    const TIn *d_kpts = (const TIn *)kpts;
    TOut *d_xyzs = (TOut *)xyzs, *d_ps = (TOut *)ps;
    const int C = ctx->C;
    // kthr >= 0: scores that pass the keypoint gate are non-negative, so no candidate mean can fall
    // below avg_thr <= 0 and the fast kernel needs no negative-score check
    const bool fast = Pmax == 1 && C >= 3 && C <= 8 && prm.kn >= 1 && prm.avg_thr <= 0.0 && prm.kthr >= 0.0 &&
                      !((double)ctx->npairs < prm.num_tol) && ctx->general_mode == 0;
    const int64_t ring_slot = ctx->ev_count % kTimingRing;
    ctx->ev_attached = false;
    // (float64 outputs -- the reference's own output type -- on the lean kernels from five cameras on: the rolled item's
    // Newton-refined branch; up to four cameras they stay on k_fused_single<C,0,TIn,double>)
    // (lean_item -- float32 outputs up to five cameras -- measures lengths in units of distance_threshold: a threshold outside
    // lean_units_ok, i.e. not in [2^-64, 2^64] m or NaN, takes the route below as if there were no lean kernel; the rolled item keeps metres)
    constexpr bool out_f32 = std::is_same<TOut, float>::value;
    const bool lean_item_shape = out_f32 && C <= 5;
    const bool lean = method != SNOWTRI_DLT && fast && (out_f32 || C >= 5) && J == kLeanJ && prm.kn == kLeanJ &&
                      Pout == 1 && ctx->lean_mode != 0 && (!lean_item_shape || lean_units_ok(prm.dthr));
    // Five cameras and more on any other shape (float64 outputs, keypoint_num < J, other skeletons, several slots): the
    // unrolled pairwise_item of k_fused_single does not fit the register file there (10-28 pairs: 41-1 075 spilled VGPRs, round-4
    // review).  Those calls take the streaming route WITHOUT its candidate pass (launch_frame_recompute: `sumless`): with one
    // detection per camera and average_score_threshold <= 0 <= keypoint_score_threshold every candidate is kept whatever its
    // mean, k_associate clusters the C(C,2) centre joints, k_cluster_fuse runs the complete-graph item (cluster_item, no
    // scratch) and k_person_scores the mean of :150.
    const bool single_small = fast && C <= kFusedSingleMaxCams;
    // attached timing of a fast-kernel call: NO event record around the dispatch (a record is a barrier packet: the launches of a
    // timing loop would no longer be back to back); launch_fused_lean attaches the ring's pair to the kernel, or brackets a
    // call of several segments itself
    const bool dlt_coop = method == SNOWTRI_DLT && Pmax == 1 && C <= 8 && J == kLeanJ && prm.kn == kLeanJ && Pout == 1 && ctx->lean_mode != 0;
    const bool attach = ctx->timing && ctx->timing_attach && (lean || dlt_coop || method == SNOWTRI_DLT_ROBUST);
    if (ctx->timing && !attach) {
        HIP_TRY(hipEventRecord(ctx->ev[0], st));
        HIP_TRY(hipEventRecord(ctx->ev_ring[2 * ring_slot], st));
    }
    int rc = SNOWTRI_ERR_BAD_ARG;   // (what a camera count outside a route's instantiations gets)
    if (method == SNOWTRI_DLT_ROBUST) {
        // one detection per camera, two to eight cameras (checked by the entry point)
        with_cameras<2, kRobustMaxCams>(C, [&](auto cc) {
            rc = launch_dlt_robust<decltype(cc)::value, TIn, TOut>(ctx, st, F, J, d_kpts, d_np, prm, rb, Pout, d_xyzs, d_ps, d_cnt, d_fl);
        });
    } else if (method == SNOWTRI_DLT && (Pmax > 1 || C > 8)) {
        // several detections per camera: the reference's association (phases 1-2), then DLT per cluster
        if (prm.kn > kRecomputeMaxKn || !recompute_shape_ok(C, Pmax, J, ctx->npairs, (int)sizeof(TIn))) {
            g_last_error = "SNOWTRI_DLT with several detections per camera (or more than 8 cameras) supports at most 16 cameras, "
                           "C * Pmax <= 1024 detections per frame and keypoint_num <= 256 (include/snowtri.h); the pairwise method "
                           "has no such limit";
            return SNOWTRI_ERR_BAD_ARG;
        }
        rc = launch_frame_recompute<1, TIn, TOut>(ctx, st, F, Pmax, J, d_kpts, d_np, prm, Pout, d_xyzs, d_ps, d_cnt, d_fl);
    } else if (method == SNOWTRI_DLT) {
        // one detection per camera: no association needed.  The Wholebody skeleton with every joint asked for and one slot: k_dlt_coop
        with_cameras<2, 8>(C, [&](auto cc) {
            constexpr int CC = decltype(cc)::value;
            rc = dlt_coop ? launch_dlt_coop<CC, TIn, TOut>(ctx, st, F, d_kpts, d_np, prm, d_xyzs, d_ps, d_cnt, d_fl)
                          : launch_fused_single<CC, 1, TIn, TOut>(ctx, st, F, J, d_kpts, d_np, prm, Pout, d_xyzs, d_ps, d_cnt, d_fl);
        });
    } else if (lean) {
        with_cameras<out_f32 ? 3 : 5, 8>(C, [&](auto cc) {
            rc = launch_fused_lean<decltype(cc)::value, TIn, TOut>(ctx, st, F, d_kpts, d_np, prm, d_xyzs, d_ps, d_cnt, d_fl);
        });
    } else if (single_small) {
        with_cameras<3, kFusedSingleMaxCams>(C, [&](auto cc) {
            rc = launch_fused_single<decltype(cc)::value, 0, TIn, TOut>(ctx, st, F, J, d_kpts, d_np, prm, Pout, d_xyzs, d_ps, d_cnt, d_fl);
        });
    } else if (prm.kn <= kRecomputeMaxKn && recompute_shape_ok(C, Pmax, J, ctx->npairs, (int)sizeof(TIn)) &&
               ctx->general_mode != 1) {
        rc = launch_frame_recompute<0, TIn, TOut>(ctx, st, F, Pmax, J, d_kpts, d_np, prm, Pout, d_xyzs, d_ps, d_cnt, d_fl);
    } else {
        rc = launch_frame_general<TIn, TOut>(ctx, st, F, Pmax, J, d_kpts, d_np, prm, Pout, d_xyzs, d_ps, d_cnt, d_fl);
    }
    if (rc) return rc;
    if (ctx->timing && ctx->ev_attached) {
        ctx->ev_count++;
        ctx->ev_valid = false;   // (snowtri_last_kernel_ms has no pair of its own for this call)
    } else if (ctx->timing) {
        HIP_TRY(hipEventRecord(ctx->ev_ring[2 * ring_slot + 1], st));
        ctx->ev_count++;
        HIP_TRY(hipEventRecord(ctx->ev[1], st));
        HIP_TRY(hipEventRecord(ctx->ev[2], st));
        HIP_TRY(hipEventRecord(ctx->ev[3], st));
        ctx->ev_valid = true;
        ctx->ev_stream = st;
    }
    return SNOWTRI_OK;
}

// The fused call.  explicit_rb: snowtri_triangulate_robust (its own settings and diagnostics; always on the caller's stream);
// nullptr: snowtri_triangulate_condense[_ex], where method = SNOWTRI_DLT_ROBUST takes the context's settings and no diagnostics.
int fused_call(snowtri_ctx *ctx, int64_t F, int32_t Pmax, int32_t J, const void *kpts, int in_dtype, const int32_t *n_persons,
               const snowtri_params *params, int method, int32_t Pout_max, void *out_xyzs, void *out_pscore, int out_dtype,
               int32_t *out_count, uint32_t *out_flags, int memspace, void *stream, uint32_t call_flags, const RobustCall *explicit_rb) {
    if (!ctx || ctx->C < 1 || F < 0 || Pmax < 1 || J < 1 || Pout_max < 1 || !params) return SNOWTRI_ERR_BAD_ARG;
    if (call_flags & ~(uint32_t)SNOWTRI_CALL_NO_ZERO_FILL) return SNOWTRI_ERR_BAD_ARG;   // (an unknown flag is refused, not ignored)
    if ((in_dtype != SNOWTRI_F32 && in_dtype != SNOWTRI_F64) || (out_dtype != SNOWTRI_F32 && out_dtype != SNOWTRI_F64))
        return SNOWTRI_ERR_BAD_ARG;
    if (memspace != SNOWTRI_HOST && memspace != SNOWTRI_DEVICE) return SNOWTRI_ERR_BAD_ARG;
    if (method != SNOWTRI_PAIRWISE && method != SNOWTRI_DLT && method != SNOWTRI_DLT_ROBUST) return SNOWTRI_ERR_BAD_ARG;
    if (method == SNOWTRI_DLT && ctx->C < 2) return SNOWTRI_ERR_BAD_ARG;
    if (method == SNOWTRI_DLT_ROBUST && (Pmax != 1 || ctx->C < 2 || ctx->C > kRobustMaxCams)) {
        g_last_error = "SNOWTRI_DLT_ROBUST takes one detection per camera (Pmax == 1) on 2 to 8 cameras (include/snowtri.h)";
        return SNOWTRI_ERR_BAD_ARG;
    }
    RobustCall rb;
    if (explicit_rb) {
        rb = *explicit_rb;
    } else {
        rb.threshold_px = ctx->robust_threshold_px;
        rb.max_drops = ctx->robust_max_drops;
    }
    if (F == 0) return SNOWTRI_OK;
    if (!kpts || !out_xyzs || !out_count) return SNOWTRI_ERR_BAD_ARG;
    // device buffers: keypoints aligned to their element, joint records [x, y, z, s] to 16 bytes (vector stores)
    if (memspace == SNOWTRI_DEVICE && (((uintptr_t)kpts & (dtype_size(in_dtype) - 1)) != 0 || ((uintptr_t)out_xyzs & 15) != 0))
        return SNOWTRI_ERR_BAD_ARG;
    // ... and the diagnostics of snowtri_triangulate_robust to their elements
    if (memspace == SNOWTRI_DEVICE && ((rb.views && ((uintptr_t)rb.views & 3) != 0) || (rb.resid && ((uintptr_t)rb.resid & (dtype_size(out_dtype) - 1)) != 0)))
        return SNOWTRI_ERR_BAD_ARG;
    Params prm;
    int rc = validate_params(params, J, &prm, true);
    if (rc) return rc;
    prm.no_zero_fill = (call_flags & SNOWTRI_CALL_NO_ZERO_FILL) ? 1 : 0;
    hipStream_t st = (hipStream_t)stream;
    // overlap mode queries the caller's stream and runs the call on an internal one: neither can go into a hipGraph that `stream`
    // is recording.  Refused before any other runtime call, so the caller's capture stays valid.
    if (memspace == SNOWTRI_DEVICE && ctx->overlap >= 2 && !explicit_rb && stream_is_capturing(st)) {
        g_last_error = "overlap mode (snowtri_ctx_set_overlap >= 2) cannot be captured into a hipGraph: `stream` is capturing";
        return SNOWTRI_ERR_BAD_ARG;
    }
    ENTER_DEVICE(ctx->device);
    ctx->cur = &ctx->sets[0];
    ctx->last_set = &ctx->sets[0];
    ctx->last_stream = false;
    StreamSet *oset = nullptr;
    if (memspace == SNOWTRI_DEVICE && ctx->overlap >= 2 && !explicit_rb) {
        // overlap mode: this call runs on the next internal stream behind everything `stream` holds now; the caller's
        // stream sees its results after snowtri_ctx_join
        // (sets 1 .. n: set 0 -- scratch, lists, counters -- stays with the caller's stream, where the host calls, the per-frame
        // entry points and the calls made outside overlap mode use it; ADVICE r4: an overlapped call on set 0 shared them unordered)
        const int k = 1 + (int)(ctx->call_index++ % ctx->overlap);
        if (ctx->ensure_set(k)) {
            g_last_error = "creating an internal stream of the overlap mode failed";
            return SNOWTRI_ERR_HIP;
        }
        oset = &ctx->sets[k];
        // the internal stream runs behind whatever the caller's stream holds now; an idle caller stream (the usual loop of
        // calls on resident inputs) needs no event pair: one query instead of a record + a wait per call
        if (hipStreamQuery(st) != hipSuccess) {
            (void)hipGetLastError();
            HIP_TRY(hipEventRecord(ctx->ev_fork, st));
            HIP_TRY(hipStreamWaitEvent(oset->stream, ctx->ev_fork, 0));
        }
        ctx->cur = ctx->last_set = oset;
        st = oset->stream;
    }
    const int kn = prm.kn;
    const size_t isz = dtype_size(in_dtype), osz = dtype_size(out_dtype);
    const bool host = memspace == SNOWTRI_HOST;
    const void *d_kpts = kpts;
    const int32_t *d_np = n_persons;
    void *d_xyzs = out_xyzs, *d_ps = out_pscore;
    int32_t *d_cnt = out_count;
    uint32_t *d_fl = out_flags;
    if (host && !d_fl) {   // the return status and last_slow_frames come from the flags: a host call always takes them back
        if (ctx->flags_host.size() < (size_t)F) ctx->flags_host.resize(F);
        d_fl = ctx->flags_host.data();
    }
    const uint32_t *const fl = d_fl;   // (a host call's flags on the host)
    Staging sg(ctx->in, ctx->out, host, st, ctx, Staging::kPinned);
    sg.in(&d_kpts, (size_t)F * ctx->C * Pmax * J * 3 * isz);
    sg.in(&d_np, sizeof(int32_t) * F * ctx->C);
    sg.out(&d_xyzs, (size_t)F * Pout_max * kn * 4 * osz);
    sg.out(&d_ps, (size_t)F * Pout_max * osz);
    sg.out(&d_cnt, sizeof(int32_t) * F);
    sg.out(&d_fl, sizeof(uint32_t) * F);
    sg.out(&rb.views, sizeof(uint32_t) * F * kn);   // the diagnostics of snowtri_triangulate_robust: staged like everything else
    sg.out(&rb.resid, osz * F * kn);
    rc = sg.begin();
    if (rc) return rc;
    if (!d_fl) {   // a device call that takes no flags
        rc = ctx->cur->misc.ensure(sizeof(uint32_t) * F);
        if (rc) return rc;
        d_fl = (uint32_t *)ctx->cur->misc.p;
    }
    // no memsets: the kernels own every output word, including the per-frame flags
    ctx->last_slow_frames = -1;
    ctx->last_handover = false;
    if (in_dtype == SNOWTRI_F32 && out_dtype == SNOWTRI_F32)
        rc = fused_dispatch<float, float>(ctx, st, F, Pmax, J, d_kpts, d_np, prm, Pout_max, d_xyzs, d_ps, d_cnt, d_fl, method, rb);
#ifdef SNOWTRI_DEV_MIN  // kernel-development builds (scripts/ab_build.sh): float32 I/O, 4 cameras only
    else
        rc = SNOWTRI_ERR_BAD_ARG;
#else
    else if (in_dtype == SNOWTRI_F32)
        rc = fused_dispatch<float, double>(ctx, st, F, Pmax, J, d_kpts, d_np, prm, Pout_max, d_xyzs, d_ps, d_cnt, d_fl, method, rb);
    else if (out_dtype == SNOWTRI_F32)
        rc = fused_dispatch<double, float>(ctx, st, F, Pmax, J, d_kpts, d_np, prm, Pout_max, d_xyzs, d_ps, d_cnt, d_fl, method, rb);
    else
        rc = fused_dispatch<double, double>(ctx, st, F, Pmax, J, d_kpts, d_np, prm, Pout_max, d_xyzs, d_ps, d_cnt, d_fl, method, rb);
#endif
    ctx->cur = &ctx->sets[0];
    if (rc) return rc;
    if (oset) oset->pending = true;   // (its `done` event is recorded once, by snowtri_ctx_join)
    rc = sg.end();
    if (rc) return rc;
    if (host) {
        uint32_t any = 0;
        int64_t slow = 0;
        for (int64_t f = 0; f < F; f++) {
            any |= fl[f];
            slow += (fl[f] & SNOWTRI_FLAG_FASTPATH) ? 0 : 1;
        }
        ctx->last_slow_frames = slow;
        if (any & SNOWTRI_FLAG_SINGULAR) return SNOWTRI_ERR_SINGULAR;
        if (any & SNOWTRI_FLAG_OVERFLOW) return SNOWTRI_ERR_OVERFLOW;
    }
    return SNOWTRI_OK;
}

}  // namespace

extern "C" int snowtri_triangulate_condense(snowtri_ctx *ctx, int64_t F, int32_t Pmax, int32_t J,
                                            const void *kpts, int in_dtype, const int32_t *n_persons,
                                            const snowtri_params *params, int method, int32_t Pout_max,
                                            void *out_xyzs, void *out_pscore, int out_dtype,
                                            int32_t *out_count, uint32_t *out_flags, int memspace,
                                            void *stream) {
    return snowtri_triangulate_condense_ex(ctx, F, Pmax, J, kpts, in_dtype, n_persons, params, method, Pout_max, out_xyzs, out_pscore,
                                           out_dtype, out_count, out_flags, memspace, stream, 0u);
}

extern "C" int snowtri_triangulate_condense_ex(snowtri_ctx *ctx, int64_t F, int32_t Pmax, int32_t J,
                                               const void *kpts, int in_dtype, const int32_t *n_persons,
                                               const snowtri_params *params, int method, int32_t Pout_max,
                                               void *out_xyzs, void *out_pscore, int out_dtype,
                                               int32_t *out_count, uint32_t *out_flags, int memspace,
                                               void *stream, uint32_t call_flags) {
    return fused_call(ctx, F, Pmax, J, kpts, in_dtype, n_persons, params, method, Pout_max, out_xyzs, out_pscore, out_dtype, out_count,
                      out_flags, memspace, stream, call_flags, nullptr);
}

extern "C" int snowtri_triangulate_robust(snowtri_ctx *ctx, int64_t F, int32_t J, const void *kpts, int in_dtype, const int32_t *n_persons,
                                          const snowtri_params *params, double reproj_threshold_px, int32_t max_drops, int32_t Pout_max,
                                          void *out_xyzs, void *out_pscore, int out_dtype, int32_t *out_count, uint32_t *out_flags,
                                          uint32_t *out_views, void *out_resid, int memspace, void *stream) {
    if (!ctx) return SNOWTRI_ERR_BAD_ARG;
    if (!(reproj_threshold_px >= 0.0)) {
        g_last_error = "reproj_threshold_px must be >= 0 (+inf allowed), not negative or NaN";
        return SNOWTRI_ERR_BAD_ARG;
    }
    if (max_drops < 0 || max_drops > kRobustMaxDrops) {
        g_last_error = "max_drops must be in [0, 6]";
        return SNOWTRI_ERR_BAD_ARG;
    }
    RobustCall rb;
    rb.threshold_px = reproj_threshold_px;
    rb.max_drops = max_drops;
    rb.views = out_views;
    rb.resid = out_resid;
    return fused_call(ctx, F, 1, J, kpts, in_dtype, n_persons, params, SNOWTRI_DLT_ROBUST, Pout_max, out_xyzs, out_pscore, out_dtype,
                      out_count, out_flags, memspace, stream, 0u, &rb);
}


// ------------------------------------------------------------------------------- matched triangulation
namespace {

// k_dlt_matched (snowtri_matched.hpp), one workgroup per tile of T frames.  A tile holds T * P single-person frames, and those are
// sized as launch_dlt_robust sizes its tile: enough to fill the chip for a small batch, at most kRobustMaxTile of them (a tile of
// 16 frames x 2 persons measured 1.23 x k_dlt_robust on the pre-gathered frames: 667 workgroups on 512 slots are two uneven rounds)
// and at most 32 KB of joint scores in the LDS stash (two workgroups share a CU); a frame whose P * kn scores are more than that is
// a tile of its own, up to the 160 KB of a CU (the P matrices, the frame's det_of table and the scores share them).  Results do
// not depend on T.  -> 0: one frame does not fit.
int matched_tile_frames(int64_t F, int C, int P, int kn, int num_cus) {
    const int64_t resident = (int64_t)num_cus * kRobustWaves, per_frame = 8 * (int64_t)P * kn;
    const int64_t rows = std::min<int64_t>(kRobustMaxTile, (F * P + resident - 1) / resident);   // (F * P <= F * P * kn: checked by the caller)
    int64_t T = std::max<int64_t>(1, rows / P);
    T = std::max<int64_t>(1, std::min<int64_t>(T, (int64_t)(32 * 1024) / per_frame));
    if (per_frame > (int64_t)160 * 1024 || matched_lds_bytes(C, (int)T, P, kn) > (size_t)160 * 1024) return 0;
    return (int)T;
}

}  // namespace

extern "C" int snowtri_triangulate_matched(snowtri_ctx *ctx, int64_t F, int32_t P, int32_t kn, int32_t Pmax, const void *kpts, int kpts_dtype,
                                           const int32_t *n_persons, const int32_t *det_of, double keypoint_score_threshold,
                                           double reproj_threshold_px, int32_t max_drops, void *out_xyzs, void *out_pscore, int out_dtype,
                                           uint32_t *out_views, void *out_resid, int memspace, void *stream) {
    const Refuse refuse{"snowtri_triangulate_matched"};
    if (!ctx) return refuse("null context");
    if ((kpts_dtype != SNOWTRI_F32 && kpts_dtype != SNOWTRI_F64) || (out_dtype != SNOWTRI_F32 && out_dtype != SNOWTRI_F64)) return refuse("unknown dtype");
    if (memspace != SNOWTRI_HOST && memspace != SNOWTRI_DEVICE) return refuse("unknown memspace");
    if (F < 0 || P < 1 || kn < 1) return refuse("F < 0, P < 1 or kn < 1");
    if (ctx->C < 2 || ctx->C > kRobustMaxCams) return refuse("the robust DLT takes 2 to 8 cameras");
    if (!(reproj_threshold_px >= 0.0)) return refuse("reproj_threshold_px must be >= 0 (+inf allowed), not negative or NaN");
    if (max_drops < 0 || max_drops > kRobustMaxDrops) return refuse("max_drops must be in [0, 6]");
    if (F > 0 && !out_xyzs) return refuse("null array (out_xyzs)");
    // Pmax, the NaN threshold, det_of == NULL with P > Pmax, the size limits, null kpts, the alignment of the inputs: as the refinement
    // entries check them (the records of this call are its OUTPUT: out_xyzs stands where they take xyzs)
    ObservedInputs in;
    if (int rc = in.check(refuse, ctx, F, P, kn, out_xyzs, out_dtype, Pmax, kpts, kpts_dtype, n_persons, det_of, nullptr, keypoint_score_threshold, 1,
                          0u, 0u, memspace))
        return rc;
    if (F == 0) return SNOWTRI_OK;
    const size_t osz = dtype_size(out_dtype);
    if (memspace == SNOWTRI_DEVICE && ((((uintptr_t)out_xyzs) & 15u) || ((((uintptr_t)out_pscore) | ((uintptr_t)out_resid)) & (osz - 1)) || (((uintptr_t)out_views) & 3u)))
        return refuse("out_xyzs must be aligned to 16 bytes, out_pscore, out_views and out_resid to their element size");
    const int C = ctx->C, T = matched_tile_frames(F, C, P, kn, ctx->num_cus);
    if (T < 1) return refuse("P * kn joint scores of one frame and the kernel's tables must fit the LDS of a CU");
    const int64_t tiles = (F + T - 1) / T;
    if (tiles > 0x7fffffffll) return refuse("more than 2^31 - 1 tiles");
    ENTER_DEVICE(ctx->device);
    hipStream_t st = (hipStream_t)stream;
    const void *dk = kpts;
    const int32_t *dnp = n_persons, *ddet = det_of;
    void *d_xyzs = out_xyzs, *d_ps = out_pscore, *d_resid = out_resid;
    uint32_t *d_views = out_views;
    Staging sg(ctx->in, ctx->out, memspace == SNOWTRI_HOST, st);
    sg.in(&dk, in.k_bytes);
    sg.in(&dnp, in.np_bytes);
    sg.in(&ddet, in.det_bytes);
    sg.out(&d_xyzs, in.x_bytes);
    sg.out(&d_ps, osz * (size_t)F * P);
    sg.out(&d_views, in.views_bytes);
    sg.out(&d_resid, osz * (size_t)in.n_rec);
    if (int rc = sg.begin()) return rc;
    const size_t lds = matched_lds_bytes(C, T, P, kn);
    const double tau2 = reproj_threshold_px * reproj_threshold_px;
    int rc = SNOWTRI_ERR_BAD_ARG;   // (a build without this camera count: the kernel-development builds)
    if (ctx->timing) HIP_TRY(hipEventRecord(ctx->ev[0], st));   // snowtri_set_timing: the kernel between the pair snowtri_last_kernel_ms reads
    with_cameras<2, kRobustMaxCams>(C, [&](auto cc) {
        with_float_pair(kpts_dtype, out_dtype, [&](auto tk, auto to) {
            constexpr int CC = decltype(cc)::value;
            using TK = decltype(tk);
            using TO = decltype(to);
            rc = raise_lds_or_fail(ctx, (const void *)k_dlt_matched<CC, TK, TO>, lds);
            if (rc) return;
            hipLaunchKernelGGL((k_dlt_matched<CC, TK, TO>), dim3((unsigned)tiles), dim3(kBlock), lds, st, F, (int)P, (int)Pmax, (int)kn, T, ctx->rig(),
                               (const TK *)dk, dnp, ddet, keypoint_score_threshold, tau2, (int)max_drops, (TO *)d_xyzs, (TO *)d_ps, d_views, (TO *)d_resid);
            static const std::string name = kernel_name("k_dlt_matched", {std::to_string(CC), type_name<TK>(), type_name<TO>()});
            ctx->last_kernels = name.c_str();
        });
    });
    if (rc) return rc == SNOWTRI_ERR_BAD_ARG ? refuse("this build has no k_dlt_matched for the context's camera count") : rc;
    HIP_TRY(hipGetLastError());
    if (ctx->timing) {
        HIP_TRY(hipEventRecord(ctx->ev[1], st));
        HIP_TRY(hipEventRecord(ctx->ev[2], st));   // (no second phase: the pair (2, 3) is empty)
        HIP_TRY(hipEventRecord(ctx->ev[3], st));
        ctx->ev_valid = true;
        ctx->ev_stream = st;
    }
    return sg.end();
}
