// sgx_tracker.cpp — the pipelined per-frame host of the tracking hot path, in C++ behind the C ABI (include/sgx.h: sgx_tracker_*).
//
// One object = S independent RGB-D streams tracked in lock-step on one GPU, one frame per stream per step, every stage device-resident.
// It mirrors the call order of the reference's tracking thread for one frame,
//     Tracking::GrabImageRGBD (src/sg-slam/src/Tracking.cc:206-251)  ->  Frame::Frame (src/sg-slam/src/Frame.cc:100-200: ExtractORB, the detector
//     hand-shake, RmDynamicPointWithSemanticAndGeometry, ComputeStereoFromRGBD)  ->  Tracking::Track / TrackWithMotionModel / TrackLocalMap
//     (Tracking.cc:906-1013),
// in "visual odometry" form (the map points a frame is tracked against are the previous frame's keypoints unprojected with their measured depth,
// Tracking::UpdateLastFrame :840-904; the local map is the points of frames t-2 and t-3), with the stages spread over three HIP streams:
//     D  Detector2D::detect of frame t            (the reference runs it on its own thread, Detector2D::Run; Frame.cc:478 waits for it)
//     E  ORB detect -> LK flow -> RANSAC F -> [event: detector done] -> dynamic mask + erase -> ORB orientation + descriptors of the survivors -> [UndistortKeyPoints +] stereo-from-RGBD   of frame t + 1
//        (the reference describes every keypoint first, ORBextractor::operator(), and erases descriptor rows with the keypoints; nothing in between reads them, so the bytes are the same)
//     T  motion model -> SearchByProjection(cur,last) -> PoseOptimization -> SearchLocalPoints -> PoseOptimization -> unproject -> map points   of frame t
// Frame state is triple-buffered (frame t lives in slot t % 3); events order the streams; nothing synchronises with the host inside a step.
// An optional upload stream U takes host frames (pinned staging buffers the caller fills, as cv::imread would) to the device and converts
// BGR -> gray (Tracking.cc:214-227) ahead of the step (sgx_tracker_step_host).
// This is the harness / integration host for bench.py, example_track.cpp and the tests — it replaces sg_slam_amd/tracker.py's orchestration, not
// ORB_SLAM2::Tracking's state machine (keyframe decisions, relocalisation and the map stay with the caller).
//
// Layout of this file: runtime wrappers and the two test taps; the handle (FrameSlot x 3, DetSlot x 2, HostSlot x 2, everything it acquired); create; the step as a
// context (Step: slots, detector set and streams of frame i, resolved once) handed through eight stage functions; the host-input path; read-backs.
#include "sgx_rt.h"
#include "../../include/sgx.h"
#ifdef SGX_DEBUG_TAPS
#include "../../include/sgx_debug.h"      // test / tuning taps: compiled into tests/taps/libsgx_taps.so and the emulator only
#endif
#include <math.h>
#include <stdio.h>
#include <string.h>
#include <stdlib.h>
#include <atomic>
#include <new>
#include <vector>

#ifndef SGX_EMU
typedef hipEvent_t sgx_ev;
typedef hipStream_t sgx_st;
static int ev_create(sgx_ev *e) { return hipEventCreateWithFlags(e, hipEventDisableTiming) == hipSuccess ? 0 : 1; }
static void ev_destroy(sgx_ev e) { (void)hipEventDestroy(e); }
static void ev_record(sgx_ev e, sgx_st s) { (void)hipEventRecord(e, s); }
static void st_wait(sgx_st s, sgx_ev e) { (void)hipStreamWaitEvent(s, e, 0); }
static int st_create(sgx_st *s, int high_priority)
{
    if (high_priority) { int lo = 0, hi = 0; (void)hipDeviceGetStreamPriorityRange(&lo, &hi); return hipStreamCreateWithPriority(s, hipStreamNonBlocking, hi) == hipSuccess ? 0 : 1; }
    return hipStreamCreateWithFlags(s, hipStreamNonBlocking) == hipSuccess ? 0 : 1;
}
static void st_destroy(sgx_st s) { (void)hipStreamDestroy(s); }
static void st_sync(sgx_st s) { (void)hipStreamSynchronize(s); }
static void ev_sync(sgx_ev e) { (void)hipEventSynchronize(e); }
static void *host_alloc(size_t n) { void *p = nullptr; return hipHostMalloc(&p, n, hipHostMallocDefault) == hipSuccess ? p : nullptr; }
static void host_free(void *p) { (void)hipHostFree(p); }
#else
// The emulator runs every launch in the calling thread and its entries ignore their stream argument.  Streams and events are distinct tokens all the same, so that the
// schedule this host issues can be read back there (sgx_tracker_debug_sync_trace).
typedef void *sgx_ev;
typedef void *sgx_st;
static std::atomic<uintptr_t> g_emu_token{0x1000};
static int ev_create(sgx_ev *e) { *e = (sgx_ev)++g_emu_token; return 0; }
static void ev_destroy(sgx_ev) {}
static void ev_record(sgx_ev, sgx_st) {}
static void st_wait(sgx_st, sgx_ev) {}
static int st_create(sgx_st *s, int) { *s = (sgx_st)++g_emu_token; return 0; }
static void st_destroy(sgx_st) {}
static void st_sync(sgx_st) {}
static void ev_sync(sgx_ev) {}
static void *host_alloc(size_t n) { return calloc(1, n ? n : 1); }
static void host_free(void *p) { free(p); }
#endif

// ---- the two test taps (include/sgx_debug.h); both fold to nothing in the product build
// sgx_tracker_debug_fail_after: one counter per thread, consulted by the six places a tracker entry acquires something or checks a call (alloc, pinned allocation,
// new_stream, new_event, TRK_HIP, TRK_CHECK); the n-th consultation fails with the status the runtime's refusal would have given.
// sgx_tracker_debug_sync_trace: the (op, stream, event) triples of everything that orders streams, in issue order.
enum { TRK_OP_RECORD = 0, TRK_OP_WAIT = 1, TRK_OP_EV_SYNC = 2, TRK_OP_ST_SYNC = 3, TRK_OP_DEV_SYNC = 4, TRK_OP_MARK = 5 };
enum { TRK_MARK_DETECTOR = 1, TRK_MARK_ORB = 2, TRK_MARK_MASK = 3, TRK_MARK_STEREO = 4, TRK_MARK_MOTION = 5, TRK_MARK_UNPROJECT = 6, TRK_MARK_UPLOAD = 7, TRK_MARK_GRAY = 8, TRK_MARK_PACK = 9 };
#ifdef SGX_DEBUG_TAPS
static thread_local int g_trk_fail_after = 0, g_trk_fail_status = SGX_OK;
static bool trk_fail(int status) { if (g_trk_fail_after <= 0 || --g_trk_fail_after > 0) return false; g_trk_fail_status = status; return true; }
struct TrkTrace {
    std::vector<int32_t> log; std::vector<const void *> streams, events;      // streams / events: numbered in order of first appearance; the host is stream -1
    static int32_t index(std::vector<const void *> &seen, const void *p) { for (size_t k = 0; k < seen.size(); k++) if (seen[k] == p) return (int32_t)k; seen.push_back(p); return (int32_t)seen.size() - 1; }
    void add(int op, bool host, const void *s, const void *e, int id = -1) { log.push_back(op); log.push_back(host ? -1 : index(streams, s)); log.push_back(e ? index(events, e) : id); }
};
#else
static bool trk_fail(int) { return false; }
struct TrkTrace { void add(int, bool, const void *, const void *, int = -1) {} };
#endif

#define TRK_CHECK(expr) do { const int _rc = trk_fail(SGX_ERR_DEVICE) ? SGX_ERR_DEVICE : (expr); if (_rc != SGX_OK) return _rc; } while (0)
#define TRK_HIP(expr) do { if (trk_fail(SGX_ERR_DEVICE) || (expr) != hipSuccess) return SGX_ERR_DEVICE; } while (0)
template <class F> static int trk_no_throw(F f) { try { return f(); } catch (const std::bad_alloc &) { return SGX_ERR_NOMEM; } }      // nothing is thrown across the C ABI

// per-frame record of BASELINE config 5 / SURVEY.md §8(e): 16 B header (n, 3 pad) + cap x cv::KeyPoint (28 B) + cap x 32 B descriptors + 64 B pose
SGX_KERNEL(256) k_pack_frame_records(int cap, const int32_t *n, const uint32_t *keys, const uint32_t *desc, const uint32_t *Tcw, uint32_t *rec, int rec_words)
{
    SGX_THREADS_BEGIN(tid)
    const int f = (int)blockIdx.x;
    uint32_t *r = rec + (size_t)f * rec_words;
    const uint32_t *k = keys + (size_t)f * cap * 7, *d = desc + (size_t)f * cap * 8, *T = Tcw + (size_t)f * 16;
    if (tid < 4) r[tid] = tid == 0 ? (uint32_t)n[f] : 0u;
    for (int i = tid; i < cap * 7; i += 256) r[4 + i] = k[i];
    for (int i = tid; i < cap * 8; i += 256) r[4 + cap * 7 + i] = d[i];
    if (tid < 16) r[4 + cap * 15 + tid] = T[tid];
    SGX_THREADS_END
}

// The tuning switches of the tracker, read from the environment once per process.  The product build has no environment switches (sgx_rt.h: sgx_getenv() is a constant
// NULL): every member folds to its default there.
struct TrkSwitches {
    // SGX_TRK_PRIO: stream priorities (bit 0 extraction, 1 tracking, 2 detector).  Default: all equal.  Rounds 2-5 gave the tracking stream the high priority (latency of a
    // single camera); no throughput difference was ever measured.  Round 6 first blamed mixed priorities for a rare LK difference between co-running trackers; they only
    // changed how often the LK kernel met the detector's bf16 blocks on a CU — the cause was compiler-generated packed fp32 (profiles/r6_lk_priority_diagnosis.md).
    int prio = 0;
    int share = 0;                  // SGX_TRK_SHARE: 1 = tracking on the DETECTOR's stream (det(t), then track(t) behind it), 2 = tracking on the EXTRACTION stream (the round-1 serial order)
    bool describe_early = false;    // SGX_TRK_DESCRIBE_EARLY: A/B arm, orientation + descriptors of every raw keypoint before the mask, erased rows copied out by the compaction
};
static const TrkSwitches &trk_switches()
{
    static const TrkSwitches sw = [] {
        TrkSwitches s;
        s.prio = sgx_getenv("SGX_TRK_PRIO") ? atoi(sgx_getenv("SGX_TRK_PRIO")) : 0;
        s.share = sgx_getenv("SGX_TRK_SHARE") ? atoi(sgx_getenv("SGX_TRK_SHARE")) : 0;
        s.describe_early = sgx_getenv("SGX_TRK_DESCRIBE_EARLY") != nullptr;
        return s;
    }();
    return sw;
}
static thread_local int g_trk_describe_early = -1;      // test tap: the next sgx_tracker_create of this thread; -1 = SGX_TRK_DESCRIBE_EARLY (tap build) or off
SGX_TAP int sgx_tracker_debug_set_describe_early(int on) { g_trk_describe_early = on < 0 ? -1 : (on ? 1 : 0); return SGX_OK; }

struct Boxes { float *xywh = nullptr; int32_t *n = nullptr, *have = nullptr; };      // person rectangles of one frame of every stream: S x max_boxes x 4, S counts, S have-dynamic flags

// State of one frame; frame t lives in slot t % 3.  The events exist in the pipelined mode only; in the other they stay NULL and recording or waiting for them does nothing.
struct FrameSlot {
    sgx_keypoint *keys = nullptr; uint8_t *desc = nullptr; int32_t *n = nullptr; float *uright = nullptr, *zdepth = nullptr, *xw = nullptr; uint8_t *has = nullptr;
    sgx_keypoint *keys_un = nullptr;        // lens distortion (sgx_tracker_set_distortion): mvKeysUn; NULL and unused while the camera has none
    sgx_ev ev_extract = nullptr;            // the extraction stream has written the slot (keys .. zdepth) and is done with detector set and previous-frame boxes
    sgx_ev ev_track = nullptr;              // the tracking stream is done with the step that had this slot as current
    sgx_ev ev_pack = nullptr;               // the caller's stream has packed the slot's record
    // ev_consumed: every reader of the INPUT images of the step that used this slot on the extraction stream (ORB, LK pyramid, stereo-from-RGBD) is done.
    // ev_det_read: the detector stream's reader of the same step (the forward reads d_bgr).  Kept apart from ev_consumed so that the extraction stream never waits for the
    // detector only to publish "inputs consumed" (with dynamic_mask == 0 that serialised ORB / LK of frame i + 1 behind the forward of frame i).
    sgx_ev ev_consumed = nullptr, ev_det_read = nullptr;
    bool consumed = false, det_read = false, packed = false;      // the event of that name has a record that nobody has waited for on the slot's behalf yet
};
struct DetSlot { sgx_det_result *res = nullptr; Boxes boxes; sgx_ev ev_done = nullptr; };      // detector results of one frame, double-buffered; ev_done: the forward has written them
// Host-input staging, double-buffered: pinned host + device copies.  ev_up: the H2D copies out of the pinned buffers are done (the caller may refill them); both modes.
struct HostSlot {
    uint8_t *h_bgr = nullptr; uint16_t *h_depth = nullptr; uint8_t *d_bgr = nullptr, *d_gray = nullptr; uint16_t *d_depth = nullptr;
    sgx_ev ev_up = nullptr; bool up_pending = false;
};
struct TrkStreams { sgx_st E = nullptr, T = nullptr, D = nullptr; };

struct sgx_tracker {
    sgx_tracker_config cfg = {};
    int S = 0, cap = 0, nlevels = 0, MB = 0;
    sgx_orb *ex = nullptr; sgx_flow *flow = nullptr; sgx_det *det = nullptr;      // the detector is the caller's
    float scale[16] = {}, inv_sigma2[16] = {}; float log_scale = 0.f;
    // everything the handle acquired, in order of acquisition; released by the destructor or, for a set-up call that fails half way, by release_to()
    std::vector<void *> dev, pinned; std::vector<sgx_ev> events; std::vector<sgx_st> streams;
    struct Owned { size_t dev = 0, pinned = 0, events = 0, streams = 0; };
    FrameSlot fs[3]; DetSlot ds[2]; HostSlot hs[2];
    float *Tcw[3] = {};                     // cur, last, last-last (rotating)
    float dist[8] = {}; int ndist = 0; bool undistort = false;      // undistort: set_distortion succeeded, every slot has its keys_un
    int32_t *match = nullptr, *nmatch = nullptr, *ninl = nullptr, *zero_i4 = nullptr; uint8_t *outlier = nullptr, *zero_u8 = nullptr, *vel_valid = nullptr;
    float *lm_xw = nullptr, *lm_normal = nullptr, *lm_min = nullptr, *lm_max = nullptr; uint8_t *lm_desc = nullptr, *lm_skip = nullptr; int32_t *lm_obs = nullptr, *lm_n = nullptr;
    int32_t *match_local = nullptr, *nmatch_local = nullptr, *merged = nullptr, *cur_mp_obs = nullptr, *ninl2 = nullptr; uint8_t *in_view = nullptr, *outlier2 = nullptr; float *xw_all = nullptr;
    // mask stage
    // rkeys / rn: the frame's keypoints before the erase step (positions final, orientation pending: sgx_orb_detect_batch_dev); src: raw index of every survivor
    sgx_keypoint *rkeys = nullptr; uint8_t *keep = nullptr, *lk_status = nullptr; int32_t *rn = nullptr, *src = nullptr; float *prev_xy = nullptr; double *F = nullptr; int32_t *f_ok = nullptr, *f_stats = nullptr;
    uint8_t *rdesc = nullptr;               // tap build, describe_early only: the descriptors of all raw keypoints (the order before describe-after-mask, kept as its A/B arm)
    bool describe_early = false;
    Boxes pre, none;                        // the previous frame's detector results (Frame.cc:482-499); the empty set a tracker without a detector masks with
    int bgr_pitch = 0; bool host_ready = false;      // host_ready: sgx_tracker_host_buffers succeeded, both staging slots and the upload stream exist
    sgx_st sE = nullptr, sT = nullptr, sD = nullptr, sU = nullptr;      // sT may alias sD or sE (SGX_TRK_SHARE): an alias is not in `streams`.  All NULL when not pipelined
    sgx_ev ev_in = nullptr;                 // pipelined: the caller's stream has produced the step's inputs
    sgx_ev ev_step = nullptr;               // non-pipelined: end of the step on the caller's stream
    sgx_st last_stream = nullptr;           // non-pipelined mode: the caller stream of the last step (snapshots and the record pack are ordered behind it)
    int frame_idx = 0;                      // frames issued so far
    int poisoned = SGX_OK;                  // the status of the first step that failed after enqueueing had begun; the step and pack entries refuse with it from then on
    bool pipelined = false;
    TrkTrace trace;

    // ---- the only places that map a frame index to a slot, a detector set or a local-map ring slice (frame >= -3: the frames before the first have a slot too)
    FrameSlot &frame_slot(int frame) { return fs[(frame + 3) % 3]; }
    DetSlot &det_slot(int frame) { return ds[frame & 1]; }
    static int ring_slice(int frame) { return frame % 2; }
    FrameSlot &cur() { return frame_slot(frame_idx - 1); }      // the frame tracked last
    // ---- the only place that chooses between the tracker's streams and the caller's
    TrkStreams working_streams(sgx_st caller) const { return pipelined ? TrkStreams{ sE, sT, sD } : TrkStreams{ caller, caller, caller }; }

    template <class Tp> int alloc(Tp **p, size_t count)
    {
        const size_t bytes = (count ? count : 1) * sizeof(Tp);
        dev.push_back(nullptr);
        if (trk_fail(SGX_ERR_NOMEM) || hipMalloc(&dev.back(), bytes) != hipSuccess) { dev.pop_back(); return SGX_ERR_NOMEM; }
        if (hipMemset(dev.back(), 0, bytes) != hipSuccess) return SGX_ERR_DEVICE;
        *p = (Tp *)dev.back(); return SGX_OK;
    }
    template <class Tp> int alloc_pinned(Tp **p, size_t bytes)
    {
        pinned.push_back(nullptr);
        if (trk_fail(SGX_ERR_NOMEM) || !(pinned.back() = host_alloc(bytes))) { pinned.pop_back(); return SGX_ERR_NOMEM; }
        *p = (Tp *)pinned.back(); return SGX_OK;
    }
    int alloc(Boxes *b) { int rc = alloc(&b->xywh, (size_t)S * MB * 4); if (!rc) rc = alloc(&b->n, S); if (!rc) rc = alloc(&b->have, S); return rc; }
    int new_event(sgx_ev *e)
    {
        events.push_back(nullptr);
        if (trk_fail(SGX_ERR_DEVICE) || ev_create(&events.back())) { events.pop_back(); return SGX_ERR_DEVICE; }
        *e = events.back(); return SGX_OK;
    }
    int new_stream(sgx_st *s, int high_priority)
    {
        streams.push_back(nullptr);
        if (trk_fail(SGX_ERR_DEVICE) || st_create(&streams.back(), high_priority)) { streams.pop_back(); return SGX_ERR_DEVICE; }
        *s = streams.back(); return SGX_OK;
    }
    Owned owned() const { Owned o; o.dev = dev.size(); o.pinned = pinned.size(); o.events = events.size(); o.streams = streams.size(); return o; }
    void release_to(const Owned &o)         // buffers, events, streams: everything acquired after owned() returned `o`
    {
        for (; dev.size() > o.dev; dev.pop_back()) (void)hipFree(dev.back());
        for (; pinned.size() > o.pinned; pinned.pop_back()) host_free(pinned.back());
        for (; events.size() > o.events; events.pop_back()) ev_destroy(events.back());
        for (; streams.size() > o.streams; streams.pop_back()) st_destroy(streams.back());
    }
    ~sgx_tracker()
    {
        for (sgx_st s : streams) sync_stream(s);
        (void)device_sync();
        if (ex) sgx_orb_destroy(ex);
        if (flow) sgx_flow_destroy(flow);
        release_to(Owned());
    }

    // ---- everything that orders streams goes through these six (and into the sync trace of the tap build).  A NULL event is one the mode does not have.
    void record(sgx_ev e, sgx_st s) { if (e) { trace.add(TRK_OP_RECORD, false, s, e); ev_record(e, s); } }
    void wait(sgx_st s, sgx_ev e) { if (e) { trace.add(TRK_OP_WAIT, false, s, e); st_wait(s, e); } }
    void sync_event(sgx_ev e) { if (e) { trace.add(TRK_OP_EV_SYNC, true, nullptr, e); ev_sync(e); } }
    void sync_stream(sgx_st s) { if (s) { trace.add(TRK_OP_ST_SYNC, false, s, nullptr); st_sync(s); } }
    hipError_t device_sync() { trace.add(TRK_OP_DEV_SYNC, true, nullptr, nullptr); return hipDeviceSynchronize(); }
    void mark(sgx_st s, int id) { trace.add(TRK_OP_MARK, false, s, nullptr, id); }      // a fixed point of the schedule, for the trace only
};

extern "C" void sgx_tracker_destroy(sgx_tracker *t) { if (t) delete t; }

static int tracker_setup(sgx_tracker *t)
{
    const sgx_tracker_config &cfg = t->cfg;
    sgx_orb_config oc; memset(&oc, 0, sizeof oc);
    oc.nfeatures = cfg.nfeatures; oc.scale_factor = cfg.scale_factor; oc.nlevels = cfg.nlevels; oc.ini_th_fast = cfg.ini_th_fast; oc.min_th_fast = cfg.min_th_fast;
    oc.width = cfg.width; oc.height = cfg.height; oc.max_batch = cfg.streams;
    TRK_CHECK(sgx_orb_create(&oc, &t->ex));
    t->cap = sgx_orb_keypoint_capacity(t->ex); t->nlevels = cfg.nlevels;
    if (t->nlevels > 16) return SGX_ERR_INVALID;
    TRK_CHECK(sgx_orb_get_tables(t->ex, t->scale, nullptr, nullptr, t->inv_sigma2, nullptr));
    t->log_scale = logf(t->scale[1]);                             // Frame::mfLogScaleFactor = log(mfScaleFactor) (Frame.cc:139)
    const TrkSwitches &sw = trk_switches();
    t->describe_early = g_trk_describe_early < 0 ? sw.describe_early : g_trk_describe_early != 0;
    const size_t S = (size_t)t->S, cap = (size_t)t->cap;
    int rc = SGX_OK;                        // the first failure; nothing is acquired after it
    auto A = [&](auto **p, size_t count) { if (!rc) rc = t->alloc(p, count); };
    auto B = [&](Boxes *b) { if (!rc) rc = t->alloc(b); };
    for (FrameSlot &f : t->fs) { A(&f.keys, S * cap); A(&f.desc, S * cap * 32); A(&f.n, S); A(&f.uright, S * cap); A(&f.zdepth, S * cap); A(&f.xw, S * cap * 3); A(&f.has, S * cap); }
    for (float *&T : t->Tcw) A(&T, S * 16);
    A(&t->match, S * cap); A(&t->nmatch, S); A(&t->ninl, S); A(&t->zero_i4, S * cap); A(&t->outlier, S * cap); A(&t->zero_u8, S * cap); A(&t->vel_valid, S);
    A(&t->lm_xw, S * 2 * cap * 3); A(&t->lm_normal, S * 2 * cap * 3); A(&t->lm_min, S * 2 * cap); A(&t->lm_max, S * 2 * cap); A(&t->lm_desc, S * 2 * cap * 32);
    A(&t->lm_skip, S * 2 * cap); A(&t->lm_obs, S * 2 * cap); A(&t->lm_n, S);
    A(&t->match_local, S * cap); A(&t->nmatch_local, S); A(&t->merged, S * cap); A(&t->cur_mp_obs, S * cap); A(&t->ninl2, S); A(&t->in_view, S * 2 * cap); A(&t->outlier2, S * cap);
    A(&t->xw_all, S * 3 * cap * 3);
    if (t->describe_early) A(&t->rdesc, S * cap * 32);
    A(&t->rkeys, S * cap); A(&t->src, S * cap); A(&t->keep, S * cap); A(&t->lk_status, S * cap); A(&t->rn, S); A(&t->prev_xy, S * cap * 2); A(&t->F, S * 9); A(&t->f_ok, S); A(&t->f_stats, S * 4);
    B(&t->pre); B(&t->none);
    for (DetSlot &d : t->ds) { A(&d.res, S); B(&d.boxes); }
    if (rc) return rc;
    {   // the local-map ring starts empty: every record skipped, Observations() = 1, 2 * cap records per stream
        std::vector<uint8_t> ones(S * 2 * cap, 1); std::vector<int32_t> one(S * 2 * cap, 1), full(S, 2 * (int32_t)cap);
        TRK_HIP(hipMemcpy(t->lm_skip, ones.data(), ones.size(), hipMemcpyHostToDevice));
        TRK_HIP(hipMemcpy(t->lm_obs, one.data(), one.size() * 4, hipMemcpyHostToDevice));
        TRK_HIP(hipMemcpy(t->lm_n, full.data(), full.size() * 4, hipMemcpyHostToDevice));
    }
    if (cfg.dynamic_mask) {
        sgx_flow_config fc; memset(&fc, 0, sizeof fc);
        fc.width = cfg.width; fc.height = cfg.height; fc.max_batch = t->S; fc.win_size = 21; fc.max_level = 3; fc.max_count = 30; fc.epsilon = 0.01;      // Frame.cc:445
        TRK_CHECK(sgx_flow_create(&fc, &t->flow));
    }
    t->pipelined = cfg.pipelined != 0;
    if (t->pipelined) {
        TRK_CHECK(t->new_stream(&t->sE, sw.prio & 1)); TRK_CHECK(t->new_stream(&t->sD, (sw.prio >> 2) & 1));
        if (sw.share == 1) t->sT = t->sD; else if (sw.share == 2) t->sT = t->sE; else TRK_CHECK(t->new_stream(&t->sT, (sw.prio >> 1) & 1));
        for (FrameSlot &f : t->fs)
            for (sgx_ev *e : { &f.ev_extract, &f.ev_track, &f.ev_pack, &f.ev_consumed, &f.ev_det_read }) TRK_CHECK(t->new_event(e));
        for (DetSlot &d : t->ds) TRK_CHECK(t->new_event(&d.ev_done));
        TRK_CHECK(t->new_event(&t->ev_in));
    } else TRK_CHECK(t->new_event(&t->ev_step));
    for (HostSlot &h : t->hs) TRK_CHECK(t->new_event(&h.ev_up));      // both modes: the refill contract of sgx_tracker_host_buffers
    TRK_HIP(hipDeviceSynchronize());        // the zero-fills above ran on the null stream, which the tracker's non-blocking streams do not wait for
    return SGX_OK;
}

extern "C" int sgx_tracker_create(const sgx_tracker_config *cfg, sgx_det *detector, sgx_tracker **out)
{
    if (out) *out = nullptr;
    if (!cfg || !out || cfg->streams < 1 || cfg->width < 32 || cfg->height < 32 || cfg->nfeatures < 1 || cfg->max_boxes < 1 || cfg->max_boxes > SGX_DET_MAX) return SGX_ERR_INVALID;
    sgx_tracker *t = new (std::nothrow) sgx_tracker();
    if (!t) return SGX_ERR_NOMEM;
    t->cfg = *cfg; t->S = cfg->streams; t->MB = cfg->max_boxes; t->det = detector;
    const int rc = trk_no_throw([&] { return tracker_setup(t); });
    if (rc) { delete t; return rc; }        // the single failure exit: the handle owns whatever was acquired so far
    *out = t;
    return SGX_OK;
}

extern "C" int sgx_tracker_keypoint_capacity(const sgx_tracker *t) { return t ? t->cap : 0; }
extern "C" int sgx_tracker_record_bytes(const sgx_tracker *t) { return t ? 16 + t->cap * 28 + t->cap * 32 + 64 : 0; }

extern "C" int sgx_tracker_set_initial_pose(sgx_tracker *t, const float *Tcw)
{
    if (!t || !Tcw) return SGX_ERR_INVALID;
    for (float *T : t->Tcw) TRK_HIP(hipMemcpy(T, Tcw, (size_t)t->S * 16 * 4, hipMemcpyHostToDevice));
    return SGX_OK;
}

// mDistCoef (Tracking.cc:66-77) before the first frame.  dist[0] == 0 leaves the tracker exactly as it was (the reference skips UndistortKeyPoints and
// ComputeImageBounds then, Frame.cc:656-660 / :707-713); otherwise Frame::ComputeImageBounds replaces the grid / frustum bounds and mvKeysUn is allocated.
// All or nothing: a call that fails releases what it acquired and leaves the tracker as it was.
extern "C" int sgx_tracker_set_distortion(sgx_tracker *t, const float *dist, int ndist, sgx_camera *out_cam)
{
    if (!t || !dist || (ndist != 4 && ndist != 5 && ndist != 8) || t->frame_idx > 0) return SGX_ERR_INVALID;
    if (dist[0] != 0.0f) {
        const float K4[4] = { t->cfg.cam.fx, t->cfg.cam.fy, t->cfg.cam.cx, t->cfg.cam.cy };
        sgx_camera cam = t->cfg.cam;
        TRK_CHECK(sgx_frame_image_bounds(t->cfg.width, t->cfg.height, K4, dist, ndist, &cam));
        if (!t->undistort) {
            const sgx_tracker::Owned before = t->owned();
            sgx_keypoint *kun[3] = {};
            const int rc = trk_no_throw([&]() -> int {
                for (sgx_keypoint *&k : kun) TRK_CHECK(t->alloc(&k, (size_t)t->S * t->cap));
                TRK_HIP(t->device_sync());         // zero-fills on the null stream, which the tracker's non-blocking streams do not wait for
                return SGX_OK;
            });
            if (rc) { t->release_to(before); return rc; }
            for (int i = 0; i < 3; i++) t->fs[i].keys_un = kun[i];
        }
        t->cfg.cam = cam;
        memcpy(t->dist, dist, (size_t)ndist * sizeof(float)); t->ndist = ndist; t->undistort = true;
    }
    if (out_cam) *out_cam = t->cfg.cam;
    return SGX_OK;
}

// ---- one step = one frame of every stream.  Step is everything the stages need to know about WHERE frame i lives and WHICH streams it runs on, worked out once.
struct Step {
    int i;                                  // the frame's index
    FrameSlot &c, &l, &ll;                  // the slots of frames i (written by this step), i - 1 (tracked against) and i - 2 (= the slot frame i + 1 will take)
    DetSlot &d;                             // the detector result set of frame i (last used by frame i - 2)
    sgx_st caller; TrkStreams st;           // the caller's stream; the three working streams (the tracker's own, or the caller's when not pipelined)
    bool with_det;                          // this step runs Detector2D::detect
    const Boxes &boxes;                     // what the mask of this frame reads: d.boxes, or the tracker's empty set
    const uint8_t *gray; int gray_pitch; const uint16_t *depth; const uint8_t *bgr; int bgr_pitch;
    float *Tc, *Tl, *Tll;                   // poses of frames i, i - 1, i - 2
    const sgx_keypoint *ku_c, *ku_l;        // the keypoints the tracking stages read: mvKeysUn with distortion, mvKeys without
};

// Admit the inputs: the working streams start behind the caller's, the caller's behind the readers of the inputs this step's slot had three steps ago, and the extraction
// stream behind everybody who still reads the slot it is about to overwrite.
static int stage_admit(sgx_tracker *t, Step &x)
{
    t->record(t->ev_in, x.caller);                                    // d_gray / d_depth / d_bgr: the frames may have been produced on the caller's stream
    t->wait(x.st.E, t->ev_in); t->wait(x.st.D, t->ev_in);
    if (x.i == 0) t->wait(x.st.T, t->ev_in);                          // the initial poses (later steps reach the tracking stream through ev_extract)
    if (x.c.consumed) t->wait(x.caller, x.c.ev_consumed);             // the inputs of step i - 3: later work on the caller's stream may overwrite them
    if (x.c.det_read) { t->wait(x.caller, x.c.ev_det_read); x.c.det_read = false; }      // the same inputs, read by that step's detector forward
    if (x.i >= 2) t->wait(x.st.E, x.ll.ev_track);                     // slot c: it was "last" of step i - 2, whose tracking stages must have read it
    if (x.c.packed) { t->wait(x.st.E, x.c.ev_pack); x.c.packed = false; }      // slot c: ... and its record must have been packed for the gather
    return SGX_OK;
}

// D: Detector2D::detect of this frame (Frame.cc:170-176 hands the image to the detector thread)
static int stage_detector(sgx_tracker *t, Step &x)
{
    if (!x.with_det) return SGX_OK;
    if (x.i >= 2) t->wait(x.st.D, x.ll.ev_extract);                   // result set d: last read by the mask / pre-box copy of step i - 2 (extraction stream)
    t->mark(x.st.D, TRK_MARK_DETECTOR);
    TRK_CHECK(sgx_det_detect_batch_dev(t->det, x.bgr, x.bgr_pitch, t->S, x.d.res, x.d.boxes.xywh, x.d.boxes.n, t->MB, x.d.boxes.have, x.st.D));
    t->record(x.d.ev_done, x.st.D);                                   // result set d is written
    t->record(x.c.ev_det_read, x.st.D); x.c.det_read = true;          // d_bgr is read
    return SGX_OK;
}

// E: Frame::ExtractORB.  With the mask (after the first frame, whose imGrayPre is empty: Frame.cc:155-163) only the positions, then LK into the previous frame and RANSAC
static int stage_extract(sgx_tracker *t, Step &x)
{
    const int S = t->S, cap = t->cap;
    t->mark(x.st.E, TRK_MARK_ORB);
    if (!t->cfg.dynamic_mask || x.i == 0) {
        TRK_CHECK(sgx_orb_extract_batch_dev(t->ex, x.gray, x.gray_pitch, S, x.c.keys, x.c.desc, x.c.n, cap, x.st.E));
        if (t->cfg.dynamic_mask) TRK_CHECK(sgx_flow_lk_batch_dev(t->flow, x.gray, x.gray_pitch, S, nullptr, nullptr, cap, nullptr, nullptr, nullptr, x.st.E));      // first frame: pyramid only
        return SGX_OK;
    }
    // LK, RANSAC and the mask read positions only: orientation and descriptors wait until the erase step has decided who survives
    if (t->describe_early) TRK_CHECK(sgx_orb_extract_batch_dev(t->ex, x.gray, x.gray_pitch, S, t->rkeys, t->rdesc, t->rn, cap, x.st.E));
    else TRK_CHECK(sgx_orb_detect_batch_dev(t->ex, x.gray, x.gray_pitch, S, t->rkeys, t->rn, cap, x.st.E));
    TRK_CHECK(sgx_flow_lk_batch_dev(t->flow, x.gray, x.gray_pitch, S, t->rkeys, t->rn, cap, t->prev_xy, t->lk_status, nullptr, x.st.E));
    TRK_CHECK(sgx_fundamental_ransac_batch_dev(S, cap, t->rkeys, t->rn, t->prev_xy, t->pre.have, t->pre.xywh, t->pre.n, t->MB, 1.0, 0.99, t->F, t->f_ok, t->f_stats, x.st.E));
    return SGX_OK;
}

// E: Frame::RmDynamicPointWithSemanticAndGeometry, the erase step, orientation + descriptors of the survivors
static int stage_mask(sgx_tracker *t, Step &x)
{
    if (!t->cfg.dynamic_mask || x.i == 0) return SGX_OK;
    const int S = t->S, cap = t->cap, MB = t->MB;
    const Boxes &bx = x.boxes;
    if (x.with_det) t->wait(x.st.E, x.d.ev_done);                     // result set d.  Frame.cc:478: while(!isDetectImageFinished())
    t->mark(x.st.E, TRK_MARK_MASK);
    TRK_CHECK(sgx_dynamic_mask_batch_dev(S, cap, t->rkeys, t->rn, t->prev_xy, t->F, bx.xywh, bx.n, MB, t->keep, x.st.E));
    if (t->describe_early) TRK_CHECK(sgx_frame_compact_keys_batch_dev(S, cap, t->rkeys, t->rdesc, t->rn, t->keep, bx.have, t->cfg.nfeatures, x.c.keys, x.c.desc, x.c.n, x.st.E));
    else {
        TRK_CHECK(sgx_frame_compact_keys_src_batch_dev(S, cap, t->rkeys, t->rn, t->keep, bx.have, t->cfg.nfeatures, x.c.keys, t->src, x.c.n, x.st.E));
        TRK_CHECK(sgx_orb_describe_batch_dev(t->ex, x.gray, x.gray_pitch, S, t->src, x.c.n, x.c.keys, x.c.desc, cap, x.st.E));
    }
    // Frame.cc:482-499: this frame's detector results become the "previous frame" state of the next call
    TRK_HIP(hipMemcpyAsync(t->pre.xywh, bx.xywh, (size_t)S * MB * 16, hipMemcpyDeviceToDevice, x.st.E));
    TRK_HIP(hipMemcpyAsync(t->pre.n, bx.n, (size_t)S * 4, hipMemcpyDeviceToDevice, x.st.E));
    TRK_HIP(hipMemcpyAsync(t->pre.have, bx.have, (size_t)S * 4, hipMemcpyDeviceToDevice, x.st.E));
    return SGX_OK;
}

// E: Frame.cc:172-173: UndistortKeyPoints (fused with ComputeStereoFromRGBD in one kernel when the camera has distortion); the tracking stages read mvKeysUn
static int stage_stereo(sgx_tracker *t, Step &x)
{
    const sgx_tracker_config &cf = t->cfg;
    t->mark(x.st.E, TRK_MARK_STEREO);
    if (t->undistort)
        TRK_CHECK(sgx_frame_undistort_stereo_rgbd_batch_dev(t->S, t->cap, x.c.keys, x.c.n, t->dist, t->ndist, &cf.cam, x.depth, cf.width, cf.height, cf.depth_map_factor,
                                                            x.c.keys_un, x.c.uright, x.c.zdepth, x.st.E));
    else
        TRK_CHECK(sgx_frame_stereo_from_rgbd_batch_dev(t->S, t->cap, x.c.keys, x.c.n, x.depth, cf.width, cf.height, cf.depth_map_factor, cf.cam.bf, x.c.uright, x.c.zdepth, x.st.E));
    t->record(x.c.ev_extract, x.st.E);                                // slot c is written; result set d and the previous-frame boxes are read
    // "inputs consumed" by the extraction stream's readers; the detector's forward read d_bgr on its own stream and has its own event (ev_det_read): whoever wants to
    // overwrite the inputs waits for both, the extraction stream for neither
    t->record(x.c.ev_consumed, x.st.E); x.c.consumed = true;          // d_gray / d_depth are read
    return SGX_OK;
}

// T: Tracking::TrackWithMotionModel (Tracking.cc:906-967)
static int stage_motion_model(sgx_tracker *t, Step &x)
{
    const sgx_tracker_config &cf = t->cfg;
    const int S = t->S, cap = t->cap;
    t->wait(x.st.T, x.c.ev_extract);                                  // slot c
    if (x.i == 0) return SGX_OK;
    t->mark(x.st.T, TRK_MARK_MOTION);
    TRK_CHECK(sgx_frame_motion_model_batch_dev(S, x.Tl, x.Tll, t->vel_valid, x.Tc, x.st.T));              // frame 1 has no velocity yet: it starts from the last pose
    TRK_CHECK(sgx_match_project_frame_batch_dev(S, cap, x.ku_c, x.c.desc, x.c.uright, x.c.n, x.Tc, x.ku_l, x.l.n, x.l.has, t->zero_u8, x.l.xw, t->zero_i4,
                                                x.l.desc, x.Tl, &cf.cam, t->scale, t->nlevels, cf.th_projection, 0, 1, t->match, t->nmatch, x.st.T));
    TRK_CHECK(sgx_pose_optimization_batch_dev(S, cap, x.ku_c, x.c.uright, x.c.n, t->match, nullptr, x.l.xw, cap, t->inv_sigma2, t->nlevels, &cf.cam, x.Tc, t->outlier, t->ninl, x.st.T));
    if (x.i == 1) TRK_HIP(hipMemsetAsync(t->vel_valid, 1, (size_t)S, x.st.T));
    return SGX_OK;
}

// T: Tracking::TrackLocalMap (:969-1013): SearchLocalPoints (isInFrustum + SearchByProjection th = 3) and the second PoseOptimization
static int stage_local_map(sgx_tracker *t, Step &x)
{
    if (x.i == 0 || !t->cfg.local_map) return SGX_OK;
    const sgx_tracker_config &cf = t->cfg;
    const int S = t->S, cap = t->cap;
    TRK_CHECK(sgx_frame_merge_matches_batch_dev(S, cap, x.c.n, t->match, t->outlier, nullptr, nullptr, nullptr, nullptr, t->cur_mp_obs, nullptr, x.st.T));
    TRK_CHECK(sgx_match_project_local_batch_dev(S, cap, x.ku_c, x.c.desc, x.c.uright, x.c.n, x.Tc, t->cur_mp_obs, 2 * cap, t->lm_n, t->lm_xw, t->lm_normal, t->lm_min, t->lm_max,
                                                t->lm_desc, t->lm_obs, t->lm_skip, &cf.cam, t->scale, t->nlevels, t->log_scale, 3.0f, 0.8f, 0.5f, t->match_local, t->nmatch_local, t->in_view, x.st.T));
    TRK_CHECK(sgx_frame_merge_matches_batch_dev(S, cap, x.c.n, t->match, t->outlier, t->match_local, x.l.xw, t->lm_xw, t->merged, nullptr, t->xw_all, x.st.T));
    TRK_CHECK(sgx_pose_optimization_batch_dev(S, cap, x.ku_c, x.c.uright, x.c.n, t->merged, nullptr, t->xw_all, 3 * cap, t->inv_sigma2, t->nlevels, &cf.cam, x.Tc, t->outlier2, t->ninl2, x.st.T));
    return SGX_OK;
}

// T: the frame's own points, the last frame's points into the local map; then the step is over: rotate the poses, advance the frame index
static int stage_finish(sgx_tracker *t, Step &x)
{
    const int S = t->S, cap = t->cap;
    t->mark(x.st.T, TRK_MARK_UNPROJECT);
    TRK_CHECK(sgx_frame_unproject_batch_dev(S, cap, x.ku_c, x.c.n, x.c.zdepth, x.Tc, &t->cfg.cam, x.c.xw, x.c.has, x.st.T));
    if (x.i > 0 && t->cfg.local_map)        // the last frame's points join the local map for the NEXT frames (ring slice of frame i - 1)
        TRK_CHECK(sgx_frame_make_map_points_batch_dev(S, cap, sgx_tracker::ring_slice(x.i - 1), x.ku_l, x.l.n, x.l.xw, x.l.has, x.l.desc, x.Tl, t->scale, t->nlevels, t->lm_xw, t->lm_normal,
                                                      t->lm_min, t->lm_max, t->lm_desc, t->lm_skip, x.st.T));
    t->record(x.c.ev_track, x.st.T);                                  // slot l is read (and slot c tracked: the record pack and the snapshots wait for this)
    t->last_stream = x.caller; t->record(t->ev_step, x.caller);       // non-pipelined: everything above ran on the caller's stream
    t->Tcw[0] = x.Tll; t->Tcw[1] = x.Tc; t->Tcw[2] = x.Tl;            // rotate poses: cur -> last, last -> last-last
    t->frame_idx = x.i + 1;
    return SGX_OK;
}

// One frame of every stream.  d_gray: S x H x gray_pitch u8; d_depth: S x H x W u16 (raw, Tracking.cc:229-230 divides by DepthMapFactor);
// d_bgr (optional, with a detector): S x H x bgr_pitch interleaved 3-channel u8 — what Detector2D::detect sees.  Asynchronous: the inputs are read on the
// tracker's streams after everything already enqueued on `caller_stream`.  Issuing a step only ENQUEUES work, so "three more steps were issued" says nothing about
// the device having read the inputs: the inputs of a step may be rewritten (a) by work enqueued on `caller_stream` after the third following
// sgx_tracker_step_dev call — that call makes `caller_stream` wait for the readers' event —, or (b) from the host after sgx_tracker_wait_inputs / sgx_tracker_sync returned.
// A stage that fails leaves events recorded and flags set for a frame that was never finished: the tracker is poisoned, and steps no more.
extern "C" int sgx_tracker_step_dev(sgx_tracker *t, const uint8_t *d_gray, int gray_pitch, const uint16_t *d_depth, const uint8_t *d_bgr, int bgr_pitch, void *caller_stream)
{
    if (!t || !d_gray || !d_depth || gray_pitch < t->cfg.width) return SGX_ERR_INVALID;
    if (t->poisoned) return t->poisoned;
    const int i = t->frame_idx;
    const bool with_det = t->det != nullptr && d_bgr != nullptr;
    FrameSlot &c = t->frame_slot(i), &l = t->frame_slot(i - 1);
    DetSlot &d = t->det_slot(i);
    Step x = { i, c, l, t->frame_slot(i - 2), d, (sgx_st)caller_stream, t->working_streams((sgx_st)caller_stream), with_det, with_det ? d.boxes : t->none,
               d_gray, gray_pitch, d_depth, d_bgr, bgr_pitch, t->Tcw[0], t->Tcw[1], t->Tcw[2], t->undistort ? c.keys_un : c.keys, t->undistort ? l.keys_un : l.keys };
    int rc = SGX_OK;
    for (int (*stage)(sgx_tracker *, Step &) : { stage_admit, stage_detector, stage_extract, stage_mask, stage_stereo, stage_motion_model, stage_local_map, stage_finish })
        if ((rc = stage(t, x)) != SGX_OK) return t->poisoned = rc;
    return SGX_OK;
}

// ---- host-input path: the caller fills the pinned staging buffers of a slot (as cv::imread + the TUM loader would, rgbd_tum.cc:114-115), the tracker uploads
// them on its own stream, converts the colour image to gray on the device (Tracking.cc:214-227) and steps.  Two slots.  The upload of a slot is asynchronous: before
// REFILLING a slot the caller asks for it again with sgx_tracker_host_buffers(slot), which returns once the slot's pending H2D copies have completed (or calls
// sgx_tracker_sync).  Refilling on the strength of "two further steps were issued" was unsafe: issuing is not executing.
// The first call sets the staging up, all or nothing: a call that fails releases what it acquired, and the next one starts from scratch.
static int host_setup(sgx_tracker *t)
{
    const size_t S = (size_t)t->S, W = (size_t)t->cfg.width, H = (size_t)t->cfg.height, pitch = (3 * W + 3) & ~(size_t)3;
    const sgx_tracker::Owned before = t->owned();
    HostSlot hs[2] = { t->hs[0], t->hs[1] };          // their events exist since create
    sgx_st sU = nullptr;
    const int rc = trk_no_throw([&]() -> int {
        for (HostSlot &h : hs) {
            TRK_CHECK(t->alloc_pinned(&h.h_bgr, S * H * pitch)); TRK_CHECK(t->alloc_pinned(&h.h_depth, S * H * W * 2));
            TRK_CHECK(t->alloc(&h.d_bgr, S * H * pitch)); TRK_CHECK(t->alloc(&h.d_gray, S * H * W)); TRK_CHECK(t->alloc(&h.d_depth, S * H * W));
        }
        if (t->pipelined) TRK_CHECK(t->new_stream(&sU, 0));
        TRK_HIP(t->device_sync());          // zero-fills of the new staging buffers (null stream) before the upload stream touches them
        return SGX_OK;
    });
    if (rc) { t->release_to(before); return rc; }
    t->hs[0] = hs[0]; t->hs[1] = hs[1]; t->sU = sU; t->bgr_pitch = (int)pitch; t->host_ready = true;
    return SGX_OK;
}

extern "C" int sgx_tracker_host_buffers(sgx_tracker *t, int slot, uint8_t **bgr, int *bgr_pitch, uint16_t **depth)
{
    if (!t || slot < 0 || slot > 1) return SGX_ERR_INVALID;
    if (!t->host_ready) TRK_CHECK(host_setup(t));
    HostSlot &h = t->hs[slot];
    if (h.up_pending) { t->sync_event(h.ev_up); h.up_pending = false; }      // the pinned buffers: the slot's last upload has left them
    if (bgr) *bgr = h.h_bgr; if (bgr_pitch) *bgr_pitch = t->bgr_pitch; if (depth) *depth = h.h_depth;
    return SGX_OK;
}

static int upload_and_step(sgx_tracker *t, HostSlot &h, int rgb_order)
{
    const int S = t->S, W = t->cfg.width, H = t->cfg.height;
    const sgx_st sU = t->sU;                // NULL when not pipelined: the upload and the step run on the null stream
    // the device staging slot was read by the step issued two calls ago, on the extraction AND the detector stream: ev_consumed + ev_det_read (ev_extract alone does not
    // cover the detector when that step ran without the mask's detector wait — first frame, dynamic_mask == 0)
    if (t->frame_idx >= 2) { FrameSlot &p = t->frame_slot(t->frame_idx - 2); t->wait(sU, p.ev_consumed); if (p.det_read) t->wait(sU, p.ev_det_read); }
    t->mark(sU, TRK_MARK_UPLOAD);
    TRK_HIP(hipMemcpyAsync(h.d_bgr, h.h_bgr, (size_t)S * H * t->bgr_pitch, hipMemcpyHostToDevice, sU));
    TRK_HIP(hipMemcpyAsync(h.d_depth, h.h_depth, (size_t)S * H * W * 2, hipMemcpyHostToDevice, sU));
    t->record(h.ev_up, sU); h.up_pending = true;          // the pinned buffers are read.  Non-pipelined too: the copies out of pinned memory on the null stream are asynchronous to the host
    t->mark(sU, TRK_MARK_GRAY);
    TRK_CHECK(sgx_frame_gray_from_color_batch_dev(S, W, H, h.d_bgr, t->bgr_pitch, 3, rgb_order ? 0 : 1, h.d_gray, W, sU));
    TRK_CHECK(sgx_tracker_step_dev(t, h.d_gray, W, h.d_depth, t->det ? h.d_bgr : nullptr, t->bgr_pitch, sU));
    return SGX_OK;
}

extern "C" int sgx_tracker_step_host(sgx_tracker *t, int slot, int rgb_order)
{
    if (!t || slot < 0 || slot > 1 || !t->host_ready) return SGX_ERR_INVALID;
    if (t->poisoned) return t->poisoned;
    return t->poisoned = upload_and_step(t, t->hs[slot], rgb_order);
}

// Blocks the host until the device has read the INPUT images of the step issued `steps_back` calls ago (0 = the last one; at most 2): the caller may then rewrite
// those buffers from the host.  (Stream-ordered writers need nothing: see sgx_tracker_step_dev.)
extern "C" int sgx_tracker_wait_inputs(sgx_tracker *t, int steps_back)
{
    if (!t || steps_back < 0 || steps_back > 2) return SGX_ERR_INVALID;
    if (t->frame_idx - 1 - steps_back < 0) return SGX_OK;
    if (!t->pipelined) { TRK_HIP(t->device_sync()); return SGX_OK; }
    FrameSlot &c = t->frame_slot(t->frame_idx - 1 - steps_back);
    if (c.consumed) t->sync_event(c.ev_consumed);
    if (c.det_read) t->sync_event(c.ev_det_read);
    return SGX_OK;
}

extern "C" int sgx_tracker_sync(sgx_tracker *t)
{
    if (!t) return SGX_ERR_INVALID;
    if (t->pipelined) { t->sync_stream(t->sE); t->sync_stream(t->sT); t->sync_stream(t->sD); t->sync_stream(t->sU); }
    else TRK_HIP(t->device_sync());
    t->hs[0].up_pending = t->hs[1].up_pending = false;
    return SGX_OK;
}

// results of the frame tracked last (synchronises): Tcw (S x 16), keypoints after the mask, motion-model matches / inliers, local-map matches / inliers of the
// second PoseOptimization, keypoints before the mask, findFundamentalMat success and RANSAC iteration count.  Any pointer may be NULL.
extern "C" int sgx_tracker_read(sgx_tracker *t, float *Tcw, int32_t *nkeys, int32_t *nmatches, int32_t *ninliers, int32_t *nmatches_local, int32_t *ninliers2, int32_t *nkeys_raw,
                                int32_t *f_ok, int32_t *f_stats)
{
    if (!t) return SGX_ERR_INVALID;
    TRK_CHECK(sgx_tracker_sync(t));
    const struct { void *dst; const void *src; size_t bytes_per_stream; } out[9] = {
        { Tcw, t->Tcw[1], 64 }, { nkeys, t->cur().n, 4 }, { nmatches, t->nmatch, 4 }, { ninliers, t->ninl, 4 }, { nmatches_local, t->nmatch_local, 4 }, { ninliers2, t->ninl2, 4 },
        { nkeys_raw, t->rn, 4 }, { f_ok, t->f_ok, 4 }, { f_stats, t->f_stats, 16 } };
    for (const auto &o : out) if (o.dst) TRK_HIP(hipMemcpy(o.dst, o.src, (size_t)t->S * o.bytes_per_stream, hipMemcpyDeviceToHost));
    return SGX_OK;
}

// device copy of the pose of the frame just tracked (S x 16 floats), ordered on the tracking stream: trajectory files / ATE without a host sync per frame
extern "C" int sgx_tracker_snapshot_pose_dev(sgx_tracker *t, float *d_out)
{
    if (!t || !d_out) return SGX_ERR_INVALID;
    TRK_HIP(hipMemcpyAsync(d_out, t->Tcw[1], (size_t)t->S * 64, hipMemcpyDeviceToDevice, t->working_streams(t->last_stream).T));      // non-pipelined: the step ran on the caller's stream
    return SGX_OK;
}

// device copy of one stream's person boxes of the frame just issued (max_boxes x 4 floats + count), ordered on the detector stream (oracle-chain comparison)
extern "C" int sgx_tracker_snapshot_boxes_dev(sgx_tracker *t, int stream_index, float *d_boxes, int32_t *d_nboxes)
{
    if (!t || !d_boxes || !d_nboxes || stream_index < 0 || stream_index >= t->S || t->frame_idx < 1) return SGX_ERR_INVALID;
    const Boxes &b = t->det_slot(t->frame_idx - 1).boxes;
    const sgx_st sD = t->working_streams(t->last_stream).D;
    TRK_HIP(hipMemcpyAsync(d_boxes, b.xywh + (size_t)stream_index * t->MB * 4, (size_t)t->MB * 16, hipMemcpyDeviceToDevice, sD));
    TRK_HIP(hipMemcpyAsync(d_nboxes, b.n + stream_index, 4, hipMemcpyDeviceToDevice, sD));
    return SGX_OK;
}

// BASELINE config 5: the per-frame records {n, cv::KeyPoint[cap], descriptors[cap][32], Tcw} of the frame just tracked, packed by ONE kernel into
// d_records (S x sgx_tracker_record_bytes) on `stream`, which first waits for the frame's tracking event; the frame slot is not reused before the pack ran.
extern "C" int sgx_tracker_pack_records_dev(sgx_tracker *t, uint8_t *d_records, void *stream)
{
    if (!t || !d_records || t->frame_idx < 1 || ((uintptr_t)d_records & 3)) return SGX_ERR_INVALID;
    if (t->poisoned) return t->poisoned;
    FrameSlot &c = t->cur();
    const int words = sgx_tracker_record_bytes(t) / 4;
    const sgx_st st = (sgx_st)stream;
    t->wait(st, c.ev_track);                                          // slot c is tracked (pipelined)
    if (st != t->last_stream) t->wait(st, t->ev_step);                // non-pipelined: the step ran on the caller's stream, `stream` may be another (non-blocking) one
    t->mark(st, TRK_MARK_PACK);
    SGX_LAUNCH(k_pack_frame_records, dim3(t->S), dim3(256), st, t->cap, c.n, (const uint32_t *)c.keys, (const uint32_t *)c.desc, (const uint32_t *)t->Tcw[1], (uint32_t *)d_records, words);
    TRK_HIP(hipGetLastError());
    t->record(c.ev_pack, st); c.packed = true;        // slot c: the extraction stream of the step that reuses it waits for the pack
    return SGX_OK;
}

// device pointers of the frame tracked last (valid until two more steps have been issued): tests and callers that read keypoints / descriptors in place
extern "C" int sgx_tracker_frame_dev(sgx_tracker *t, const int32_t **d_n, const sgx_keypoint **d_keys, const uint8_t **d_desc, const float **d_Tcw, const float **d_xw, const uint8_t **d_has)
{
    if (!t || t->frame_idx < 1) return SGX_ERR_INVALID;
    const FrameSlot &c = t->cur();
    if (d_n) *d_n = c.n; if (d_keys) *d_keys = c.keys; if (d_desc) *d_desc = c.desc; if (d_Tcw) *d_Tcw = t->Tcw[1]; if (d_xw) *d_xw = c.xw; if (d_has) *d_has = c.has;
    return SGX_OK;
}

extern "C" int sgx_tracker_frame_keys_un_dev(sgx_tracker *t, const sgx_keypoint **d_keys_un)
{
    if (!t || !d_keys_un || t->frame_idx < 1) return SGX_ERR_INVALID;
    *d_keys_un = t->undistort ? t->cur().keys_un : t->cur().keys;
    return SGX_OK;
}

// test tap: person rectangles of the steps that follow for a tracker WITHOUT a detector (host arrays: S x max_boxes x (x, y, w, h), S counts, S have-dynamic flags), in
// place of the empty set such a tracker masks with
SGX_TAP int sgx_tracker_debug_set_boxes(sgx_tracker *t, const float *boxes, const int32_t *nboxes, const int32_t *have_dynamic)
{
    if (!t || !boxes || !nboxes || !have_dynamic) return SGX_ERR_INVALID;
    TRK_CHECK(sgx_tracker_sync(t));
    TRK_HIP(hipMemcpy(t->none.xywh, boxes, (size_t)t->S * t->MB * 16, hipMemcpyHostToDevice));
    TRK_HIP(hipMemcpy(t->none.n, nboxes, (size_t)t->S * 4, hipMemcpyHostToDevice));
    TRK_HIP(hipMemcpy(t->none.have, have_dynamic, (size_t)t->S * 4, hipMemcpyHostToDevice));
    return SGX_OK;
}

#ifdef SGX_DEBUG_TAPS
// test tap: reads and clears the tracker's sync trace: *n int32 values, three per entry (op, stream, event or mark id).  dst == NULL asks for the size only (and keeps the log)
extern "C" int sgx_tracker_debug_sync_trace(sgx_tracker *t, int32_t *dst, int cap, int *n)
{
    if (!t || !n) return SGX_ERR_INVALID;
    *n = (int)t->trace.log.size();
    if (!dst) return SGX_OK;
    if (cap < *n) return SGX_ERR_OVERFLOW;
    if (*n) memcpy(dst, t->trace.log.data(), (size_t)*n * 4);
    t->trace.log.clear();
    return SGX_OK;
}
// test tap: the n-th acquisition or checked call of this thread's tracker entries fails (n <= 0: off).  Returns the status the previous arming delivered, SGX_OK if it never fired
extern "C" int sgx_tracker_debug_fail_after(int n)
{
    const int delivered = g_trk_fail_status;
    g_trk_fail_after = n > 0 ? n : 0; g_trk_fail_status = SGX_OK;
    return delivered;
}
#endif

extern "C" sgx_orb *sgx_tracker_extractor(sgx_tracker *t) { return t ? t->ex : nullptr; }
