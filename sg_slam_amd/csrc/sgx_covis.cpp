// sgx_covis.cpp — the covisibility graph behind the C ABI (sgx_covis_*): the relation keyframe x map point as a heap the host mirrors and patches on the device
// (KeyFrame::AddMapPoint / EraseMapPointMatch, MapPoint::AddObservation / EraseObservation / SetBadFlag / Replace, src/sg-slam/src/MapPoint.cc:98-215), the graph
// (weights, list modes, spanning tree, loop edges) as device state, and the walks of it (UpdateConnections, UpdateLocalMap, the culling votes, the bundle-adjustment graph,
// loop closing's group / LoopConnections / essential graph) as the launch sequences of sgx_covis_kernels.h and sgx_covis_loop_kernels.h.
#include "sgx_covis_kernels.h"
#include "sgx_covis_loop_kernels.h"
#include "sgx_covis_detect_kernels.h"
#include "sgx_covis_gba_kernels.h"
#include "sgx_devmem.h"
#include "../../include/sgx.h"
#include <stdio.h>
#include <string.h>
#include <algorithm>
#include <map>
#include <set>
#include <utility>
#include <vector>

static_assert(sizeof(sgx_covis_report) == sizeof(SgxCovisReport), "the kernels write sgx_covis_report records");
static_assert(sizeof(sgx_covis_ba_report) == sizeof(SgxCovisBaReport), "the kernels write sgx_covis_ba_report records");
static_assert(sizeof(sgx_covis_loop_report) == sizeof(SgxCovisLoopReport), "the kernels write sgx_covis_loop_report records");
static_assert(sizeof(sgx_covis_consistency_report) == sizeof(SgxCovisCgReport), "the kernels write sgx_covis_consistency_report records");
static_assert(sizeof(sgx_covis_gba_report) == sizeof(SgxCovisGbaReport), "the kernels write sgx_covis_gba_report records");
static_assert(SGX_ERR_INVALID == -1 && SGX_ERR_NOMEM == -3 && (int)SGX_COVIS_GBA_ORIGIN_NOT_IN_GBA == (int)SGX_GBA_ORIGIN_NOT_IN_GBA, "the kernels write these statuses as numbers");

enum { H_FREE = 0, H_LIVE = 1, H_HDR = 2, COVIS_JCAP = 1 << 16, COVIS_GRID = 128 };

struct sgx_covis {
    int max_kf = 0, cap = 0, max_points = 0, max_obs = 0, max_q = 0, mono = 0, nchunks = 0;
    float th_depth = 0.0f;
    // the relation: the host's copy of the device heap; a mutation pokes it, remembers what it overwrote, and flushes the words it changed
    std::vector<int32_t> heap; std::vector<unsigned char> attr;
    size_t o_head = 0, o_cnt = 0, o_nobs = 0, o_next = 0, o_ent = 0, o_mp = 0;
    std::vector<std::pair<size_t, int32_t>> undo;
    // keyframe slots
    struct Slot { int32_t id = -1; int state = SGX_COVIS_FREE, n = 0; };
    std::vector<Slot> slot; std::vector<int> free_slots;      // lowest last
    std::map<int32_t, int> by_id; std::set<int32_t> dead_ids;
    int nslots = 0; bool tables_dirty = true;
    // device
    int *d_heap = nullptr, *d_kf = nullptr, *d_sorted_id = nullptr, *d_sorted_slot = nullptr, *d_jidx = nullptr, *d_jval = nullptr, *d_refs = nullptr;
    unsigned char *d_attr = nullptr; unsigned short *d_W = nullptr;
    int *ws_q = nullptr, *ws_cnt = nullptr, *ws_ord = nullptr, *ws_ordw = nullptr, *ws_lkf = nullptr, *ws_pcnt = nullptr, *ws_top = nullptr, *ws_ntop = nullptr, *d_stamp = nullptr;
    int *s_kf = nullptr;
    int64_t device_bytes = 0, workspace_bytes = 0;
    // loop closing: mspLoopEdges as slot pairs in insertion order (a keyframe with a loop edge is not erased, so its slot stays), and the workspace of the loop
    // sequences, allocated by the first loop call
    std::vector<std::pair<int, int>> loop_edges;
    int *d_le = nullptr, *lw_s = nullptr, *lw_q = nullptr, *lw_qkf = nullptr, *lw_ord = nullptr, *lw_gslot = nullptr, *lw_grank = nullptr, *lw_rowg = nullptr, *lw_gof = nullptr,
        *lw_vidx = nullptr, *lw_vcnt = nullptr, *lw_vbase = nullptr, *lw_flags = nullptr;
    SgxCovisReport *lw_rep = nullptr;
    int64_t loop_bytes = 0;
    // DetectLoop: mvConsistentGroups (sgx_covis_detect_kernels.h), allocated by sgx_covis_consistency_reserve or the first consistency call; sgx_covis_clear releases it
    int cg_G = 0;
    int *cg_st = nullptr, *cg_cnt = nullptr, *cg_size = nullptr, *cg_mem = nullptr, *cg_cvalid = nullptr, *cg_nd_cand = nullptr, *cg_nd_cnt = nullptr, *cg_tmp = nullptr;
    unsigned char *cg_flags = nullptr;
    int64_t cg_bytes = 0;
    // RunGlobalBundleAdjustment's map update (sgx_covis_gba_kernels.h): 16 max_keyframes + 32 bytes, allocated by the first call
    int *gb_row_of = nullptr, *gb_orig = nullptr, *gb_level = nullptr, *gb_prow = nullptr, *gb_gs = nullptr;
    SgxDevMem mem;

    int32_t &H(size_t i) { return heap[i]; }
    void poke(size_t i, int32_t v) { if (heap[i] != v) { undo.emplace_back(i, heap[i]); heap[i] = v; } }
    void rollback() { for (size_t j = undo.size(); j-- > 0;) heap[undo[j].first] = undo[j].second; undo.clear(); }
};

static SgxCovisArgs covis_args(sgx_covis *h)
{
    SgxCovisArgs A{};
    A.nslots = h->nslots; A.max_kf = h->max_kf; A.cap = h->cap; A.max_points = h->max_points; A.nlive = (int)h->by_id.size(); A.monocular = h->mono;
    A.heap = h->d_heap; A.o_head = h->o_head; A.o_cnt = h->o_cnt; A.o_nobs = h->o_nobs; A.o_next = h->o_next; A.o_ent = h->o_ent; A.o_mp = h->o_mp;
    A.attr = h->d_attr; A.kf = h->d_kf; A.W = h->d_W; A.sorted_id = h->d_sorted_id; A.sorted_slot = h->d_sorted_slot;
    A.ws_q = h->ws_q; A.ws_cnt = h->ws_cnt; A.ws_ord = h->ws_ord; A.ws_ordw = h->ws_ordw; A.ws_lkf = h->ws_lkf; A.ws_pcnt = h->ws_pcnt; A.ws_top = h->ws_top; A.ws_ntop = h->ws_ntop;
    A.stamp = h->d_stamp;
    return A;
}

// the words a mutation changed, each once with its final value, as one or more scatter launches; the mutation has returned only when they are on the device
static int covis_flush(sgx_covis *h)
{
    std::vector<int32_t> idx; idx.reserve(h->undo.size());
    for (const auto &u : h->undo) idx.push_back((int32_t)u.first);
    h->undo.clear();
    std::sort(idx.begin(), idx.end()); idx.erase(std::unique(idx.begin(), idx.end()), idx.end());
    std::vector<int32_t> val(idx.size());
    for (size_t j = 0; j < idx.size(); j++) val[j] = h->heap[(size_t)idx[j]];
    for (size_t at = 0; at < idx.size(); at += COVIS_JCAP) {
        const int n = (int)std::min((size_t)COVIS_JCAP, idx.size() - at);
        SGX_CHECK_HIP(hipMemcpy(h->d_jidx, idx.data() + at, (size_t)n * 4, hipMemcpyHostToDevice));
        SGX_CHECK_HIP(hipMemcpy(h->d_jval, val.data() + at, (size_t)n * 4, hipMemcpyHostToDevice));
        SGX_LAUNCH(k_covis_scatter, dim3((unsigned)((n + 255) / 256)), dim3(256), (sgx_stream_t)0, h->d_heap, (const int *)h->d_jidx, (const int *)h->d_jval, n);
        SGX_CHECK_HIP(hipGetLastError());
        SGX_CHECK_HIP(hipStreamSynchronize((sgx_stream_t)0));
    }
    return SGX_OK;
}

// ---- the observation lists: a chain of 8-entry chunks per point, the head chunk holding the remainder; per-point order means nothing to any result
static void obs_add(sgx_covis *h, int p, int t, int i)
{
    const int cnt = h->H(h->o_cnt + p);
    if (cnt % SGX_COVIS_CHUNK == 0) {
        const int c = h->H(H_FREE);
        h->poke(H_FREE, h->H(h->o_next + c));
        h->poke(h->o_next + c, cnt ? h->H(h->o_head + p) : -1);
        h->poke(h->o_head + p, c);
    }
    h->poke(h->o_ent + (size_t)h->H(h->o_head + p) * SGX_COVIS_CHUNK + cnt % SGX_COVIS_CHUNK, t << 16 | i);
    h->poke(h->o_cnt + p, cnt + 1);
    h->poke(h->o_nobs + p, h->H(h->o_nobs + p) + ((h->attr[(size_t)t * h->cap + i] & SGX_COVIS_ATTR_RIGHT) ? 2 : 1));      // MapPoint.cc:105-108
    h->poke(H_LIVE, h->H(H_LIVE) + 1);
}

template <class F> static void obs_each(const sgx_covis *h, int p, F f)          // f(entry address, slot, index) -> true to stop
{
    int left = h->heap[h->o_cnt + p], m = ((left - 1) & (SGX_COVIS_CHUNK - 1)) + 1;
    for (int c = h->heap[h->o_head + p]; left > 0 && c >= 0; c = h->heap[h->o_next + c], m = SGX_COVIS_CHUNK) {
        for (int j = 0; j < m; j++) { const size_t at = h->o_ent + (size_t)c * SGX_COVIS_CHUNK + j; const int e = h->heap[at]; if (f(at, e >> 16, e & 0xffff)) return; }
        left -= m;
    }
}

static int obs_index(const sgx_covis *h, int p, int t)                           // GetIndexInKeyFrame
{
    int r = -1;
    obs_each(h, p, [&](size_t, int tt, int i) { if (tt == t) { r = i; return true; } return false; });
    return r;
}

static void obs_clear(sgx_covis *h, int p)
{
    const int cnt = h->H(h->o_cnt + p);
    if (!cnt) return;
    for (int c = h->H(h->o_head + p), left = cnt; left > 0 && c >= 0;) {
        const int nx = h->H(h->o_next + c);
        h->poke(h->o_next + c, h->H(H_FREE)); h->poke(H_FREE, c);
        left -= left == cnt ? ((cnt - 1) & (SGX_COVIS_CHUNK - 1)) + 1 : SGX_COVIS_CHUNK;
        c = nx;
    }
    h->poke(h->o_cnt + p, 0); h->poke(h->o_nobs + p, 0); h->poke(h->o_head + p, -1);
    h->poke(H_LIVE, h->H(H_LIVE) - cnt);
}

static void point_set_bad(sgx_covis *h, int p)                                   // MapPoint::SetBadFlag (:151-168)
{
    obs_each(h, p, [&](size_t, int t, int i) { h->poke(h->o_mp + (size_t)t * h->cap + i, -1); return false; });
    obs_clear(h, p);
}

static void point_erase_observation(sgx_covis *h, int p, int t)                  // MapPoint::EraseObservation (:111-137)
{
    size_t at = 0; int idx = -1;
    obs_each(h, p, [&](size_t a, int tt, int i) { if (tt == t) { at = a; idx = i; return true; } return false; });
    if (idx < 0) return;
    const int cnt = h->H(h->o_cnt + p), head = h->H(h->o_head + p);
    const size_t last = h->o_ent + (size_t)head * SGX_COVIS_CHUNK + (cnt - 1) % SGX_COVIS_CHUNK;
    h->poke(at, h->H(last));
    if ((cnt - 1) % SGX_COVIS_CHUNK == 0) {                                      // the head chunk is empty now
        h->poke(h->o_head + p, cnt > 1 ? h->H(h->o_next + head) : -1);
        h->poke(h->o_next + head, h->H(H_FREE)); h->poke(H_FREE, head);
    }
    h->poke(h->o_cnt + p, cnt - 1);
    h->poke(h->o_nobs + p, h->H(h->o_nobs + p) - ((h->attr[(size_t)t * h->cap + idx] & SGX_COVIS_ATTR_RIGHT) ? 2 : 1));
    h->poke(H_LIVE, h->H(H_LIVE) - 1);
    if (h->H(h->o_nobs + p) <= 2) point_set_bad(h, p);                           // "If only 2 observations or less, discard point"
}

static void covis_reset_host(sgx_covis *h)
{
    std::fill(h->heap.begin(), h->heap.end(), 0);
    for (int p = 0; p < h->max_points; p++) h->heap[h->o_head + p] = -1;
    for (int c = 0; c < h->nchunks; c++) h->heap[h->o_next + c] = c + 1 < h->nchunks ? c + 1 : -1;
    std::fill(h->heap.begin() + (long)h->o_mp, h->heap.end(), -1);
    h->heap[H_FREE] = 0; h->heap[H_LIVE] = 0;
    std::fill(h->attr.begin(), h->attr.end(), 0);
    for (auto &s : h->slot) s = sgx_covis::Slot();
    h->free_slots.clear();
    for (int s = h->max_kf - 1; s >= 0; s--) h->free_slots.push_back(s);
    h->by_id.clear(); h->dead_ids.clear(); h->undo.clear(); h->nslots = 0; h->tables_dirty = true;
    h->loop_edges.clear();
    void *cg[] = { h->cg_st, h->cg_cnt, h->cg_size, h->cg_mem, h->cg_cvalid, h->cg_nd_cand, h->cg_nd_cnt, h->cg_tmp, h->cg_flags };
    for (void *q : cg) h->mem.release(q);
    h->cg_st = h->cg_cnt = h->cg_size = h->cg_mem = h->cg_cvalid = h->cg_nd_cand = h->cg_nd_cnt = h->cg_tmp = nullptr; h->cg_flags = nullptr;
    h->cg_G = 0; h->cg_bytes = 0;
}

static int covis_reset_device(sgx_covis *h)
{
    SGX_CHECK_HIP(hipMemcpy(h->d_heap, h->heap.data(), h->heap.size() * 4, hipMemcpyHostToDevice));
    SGX_CHECK_HIP(hipMemset(h->d_W, 0, (size_t)h->max_kf * h->max_kf * 2));
    SGX_CHECK_HIP(hipMemset(h->d_kf, 0, (size_t)h->max_kf * CV_FIELDS * 4));
    SGX_CHECK_HIP(hipMemset(h->d_attr, 0, (size_t)h->max_kf * h->cap));
    SGX_CHECK_HIP(hipStreamSynchronize((sgx_stream_t)0));                         // a fill may return before it is done; the caller's next batch runs on another stream
    return SGX_OK;
}

extern "C" int sgx_covis_create(int max_keyframes, int cap, int max_points, int max_observations, int max_queries, int monocular, float th_depth, sgx_covis **out)
{
    if (out) *out = nullptr;
    if (!out || max_keyframes < 1 || cap < 1 || max_points < 1 || max_observations < 1 || max_queries < 1 || th_depth != th_depth) return SGX_ERR_INVALID;
    if (max_keyframes > SGX_COVIS_MAX_KF || cap > SGX_COVIS_MAX_CAP) return SGX_ERR_UNSUPPORTED;      // a slot and an index share one word; a histogram over the slots sits in LDS
    sgx_covis *h = new sgx_covis;
    h->max_kf = max_keyframes; h->cap = cap; h->max_points = max_points; h->max_obs = max_observations; h->max_q = max_queries; h->mono = monocular != 0; h->th_depth = th_depth;
    // every point with an observation holds ceil(cnt / 8) <= 1 + cnt / 8 chunks, so this many never run out while the observations are within max_observations
    h->nchunks = max_observations / SGX_COVIS_CHUNK + std::min(max_points, max_observations) + 1;
    const size_t P = (size_t)max_points, N = (size_t)max_keyframes, Qn = (size_t)max_queries;
    h->o_head = H_HDR; h->o_cnt = h->o_head + P; h->o_nobs = h->o_cnt + P; h->o_next = h->o_nobs + P; h->o_ent = h->o_next + (size_t)h->nchunks;
    h->o_mp = h->o_ent + (size_t)h->nchunks * SGX_COVIS_CHUNK;
    const size_t heap_n = h->o_mp + N * (size_t)cap;
    if (heap_n >= (size_t)INT_MAX || Qn * std::max(N, P) >= (size_t)INT_MAX) { delete h; return SGX_ERR_UNSUPPORTED; }
    h->heap.resize(heap_n); h->attr.resize(N * (size_t)cap); h->slot.resize(N);
    covis_reset_host(h);
    SgxDevMem &m = h->mem;
    int rc;
    if ((rc = m.alloc(&h->d_heap, heap_n)) || (rc = m.alloc(&h->d_attr, N * (size_t)cap)) || (rc = m.alloc(&h->d_kf, N * CV_FIELDS)) || (rc = m.alloc(&h->d_W, N * N)) ||
        (rc = m.alloc(&h->d_sorted_id, N)) || (rc = m.alloc(&h->d_sorted_slot, N)) || (rc = m.alloc(&h->d_jidx, (size_t)COVIS_JCAP)) || (rc = m.alloc(&h->d_jval, (size_t)COVIS_JCAP)) ||
        (rc = m.alloc(&h->d_refs, N)) || (rc = m.alloc(&h->s_kf, 1)) ||
        (rc = m.alloc(&h->ws_q, Qn * CQ_FIELDS)) || (rc = m.alloc(&h->ws_cnt, Qn * N)) || (rc = m.alloc(&h->ws_ord, Qn * N)) || (rc = m.alloc(&h->ws_ordw, Qn * N)) ||
        (rc = m.alloc(&h->ws_lkf, Qn * N)) || (rc = m.alloc(&h->ws_pcnt, Qn * N)) || (rc = m.alloc(&h->ws_top, Qn * SGX_COVIS_LOCAL_LIMIT * SGX_COVIS_BEST)) ||
        (rc = m.alloc(&h->ws_ntop, Qn * SGX_COVIS_LOCAL_LIMIT)) || (rc = m.alloc(&h->d_stamp, Qn * P))) { delete h; return rc; }
    h->workspace_bytes = (int64_t)(Qn * 4 * (CQ_FIELDS + 5 * N + SGX_COVIS_LOCAL_LIMIT * (SGX_COVIS_BEST + 1) + P));
    h->device_bytes = h->workspace_bytes + (int64_t)(heap_n * 4 + N * (size_t)cap + N * CV_FIELDS * 4 + N * N * 2 + N * 12 + (size_t)COVIS_JCAP * 8 + 4);
    if ((rc = covis_reset_device(h)) != SGX_OK) { delete h; return rc; }
    *out = h;
    return SGX_OK;
}

extern "C" void sgx_covis_destroy(sgx_covis *h) { delete h; }

extern "C" int sgx_covis_size(const sgx_covis *h) { return h ? (int)h->by_id.size() : SGX_ERR_INVALID; }

extern "C" int sgx_covis_info(const sgx_covis *h, int64_t *device_bytes, int64_t *workspace_bytes, int32_t *n_observations)
{
    if (!h) return SGX_ERR_INVALID;
    if (device_bytes) *device_bytes = h->device_bytes;
    if (workspace_bytes) *workspace_bytes = h->workspace_bytes;
    if (n_observations) *n_observations = h->heap[H_LIVE];
    return SGX_OK;
}

extern "C" int sgx_covis_clear(sgx_covis *h)
{
    if (!h) return SGX_ERR_INVALID;
    covis_reset_host(h);
    return covis_reset_device(h);
}

static int covis_upload_record(sgx_covis *h, int s, int mode, int first)
{
    const sgx_covis::Slot &S = h->slot[(size_t)s];
    int32_t rec[CV_FIELDS] = {};
    rec[CV_ID] = S.id; rec[CV_STATE] = S.state; rec[CV_N] = S.n; rec[CV_MODE] = mode; rec[CV_SINGLE] = -1; rec[CV_PARENT] = -1; rec[CV_FIRST] = first;
    SGX_CHECK_HIP(hipMemcpy(h->d_kf + (size_t)s * CV_FIELDS, rec, sizeof(rec), hipMemcpyHostToDevice));
    return SGX_OK;
}

// erased keyframes that no row lists any more give their slots back
static int covis_reclaim(sgx_covis *h)
{
    if (h->dead_ids.empty()) return SGX_OK;
    SgxCovisArgs A = covis_args(h);
    SGX_LAUNCH(k_covis_refs, dim3((unsigned)((h->nslots + 255) / 256)), dim3(256), (sgx_stream_t)0, A, h->d_refs);
    SGX_CHECK_HIP(hipGetLastError());
    SGX_CHECK_HIP(hipStreamSynchronize((sgx_stream_t)0));
    std::vector<int32_t> refs((size_t)h->nslots);
    SGX_CHECK_HIP(hipMemcpy(refs.data(), h->d_refs, refs.size() * 4, hipMemcpyDeviceToHost));
    for (int s = h->nslots - 1; s >= 0; s--) {
        sgx_covis::Slot &S = h->slot[(size_t)s];
        if (S.state != SGX_COVIS_DEAD || refs[(size_t)s]) continue;
        h->dead_ids.erase(S.id);
        S = sgx_covis::Slot();
        const int rc = covis_upload_record(h, s, SGX_COVIS_ALL, 0);
        if (rc != SGX_OK) return rc;
        h->free_slots.insert(std::lower_bound(h->free_slots.begin(), h->free_slots.end(), s, [](int a, int b) { return a > b; }), s);
    }
    return SGX_OK;
}

extern "C" int sgx_covis_add_keyframe(sgx_covis *h, int32_t kf_id, int n, const int32_t *octave, const float *uright, const float *depth)
{
    if (!h || kf_id < 0 || n < 0 || n > h->cap || (n > 0 && (!octave || !uright || !depth)) || h->by_id.count(kf_id) || h->dead_ids.count(kf_id)) return SGX_ERR_INVALID;
    for (int i = 0; i < n; i++) if (octave[i] < 0 || octave[i] > SGX_COVIS_ATTR_OCTAVE) return SGX_ERR_INVALID;
    if (h->free_slots.empty()) { const int rc = covis_reclaim(h); if (rc != SGX_OK) return rc; }
    if (h->free_slots.empty()) return SGX_ERR_NOMEM;
    const int s = h->free_slots.back();
    unsigned char *a = &h->attr[(size_t)s * h->cap];
    for (int i = 0; i < n; i++) {
        const bool close = !(depth[i] > h->th_depth || depth[i] < 0);                                          // LocalMapping.cc:660, in float as written
        a[i] = (unsigned char)(octave[i] | (uright[i] >= 0 ? SGX_COVIS_ATTR_RIGHT : 0) | (close ? SGX_COVIS_ATTR_CLOSE : 0));
    }
    if (n) SGX_CHECK_HIP(hipMemcpy(h->d_attr + (size_t)s * h->cap, a, (size_t)n, hipMemcpyHostToDevice));
    SGX_CHECK_HIP(hipMemset(h->d_W + (size_t)s * h->max_kf, 0, (size_t)h->max_kf * 2));
    SGX_CHECK_HIP(hipStreamSynchronize((sgx_stream_t)0));
    h->free_slots.pop_back();
    sgx_covis::Slot &S = h->slot[(size_t)s];
    S.id = kf_id; S.state = SGX_COVIS_LIVE; S.n = n;
    if (s + 1 > h->nslots) h->nslots = s + 1;
    h->by_id[kf_id] = s; h->tables_dirty = true;
    return covis_upload_record(h, s, SGX_COVIS_ALL, 1);
}

extern "C" int sgx_covis_set_observations(sgx_covis *h, int32_t kf_id, int n, const int32_t *idx, const int32_t *point_id)
{
    if (!h || n < 0 || (n > 0 && (!idx || !point_id))) return SGX_ERR_INVALID;
    const auto it = h->by_id.find(kf_id);
    if (it == h->by_id.end()) return SGX_ERR_INVALID;
    const int s = it->second, N = h->slot[(size_t)s].n;
    int rc = SGX_OK;
    for (int j = 0; j < n && rc == SGX_OK; j++) {
        const int i = idx[j], p = point_id[j];
        if (i < 0 || i >= N || p < -1 || p >= h->max_points) { rc = SGX_ERR_INVALID; break; }
        const size_t at = h->o_mp + (size_t)s * h->cap + i;
        const int cur = h->H(at);
        if (p < 0) {                                                             // EraseMapPointMatch + EraseObservation
            if (cur >= 0) { h->poke(at, -1); point_erase_observation(h, cur, s); }
        } else if (cur != p) {                                                   // AddMapPoint + AddObservation; the same point at the same index again is nothing
            if (cur >= 0 || obs_index(h, p, s) >= 0) rc = SGX_ERR_INVALID;       // one relation: an index holds one point, a keyframe sees a point once
            else if (h->H(H_LIVE) >= h->max_obs) rc = SGX_ERR_NOMEM;
            else { h->poke(at, p); obs_add(h, p, s, i); }
        }
    }
    if (rc != SGX_OK) { h->rollback(); return rc; }
    return covis_flush(h);
}

extern "C" int sgx_covis_set_points_bad(sgx_covis *h, int n, const int32_t *ids)
{
    if (!h || n < 0 || (n > 0 && !ids)) return SGX_ERR_INVALID;
    for (int j = 0; j < n; j++) if (ids[j] < 0 || ids[j] >= h->max_points) return SGX_ERR_INVALID;
    for (int j = 0; j < n; j++) point_set_bad(h, ids[j]);
    return covis_flush(h);
}

extern "C" int sgx_covis_replace_point(sgx_covis *h, int32_t old_id, int32_t new_id)
{
    if (!h || old_id < 0 || old_id >= h->max_points || new_id < 0 || new_id >= h->max_points) return SGX_ERR_INVALID;
    if (old_id == new_id) return SGX_OK;                                          // MapPoint.cc:179-180
    std::vector<std::pair<int, int>> obs;
    obs_each(h, old_id, [&](size_t, int t, int i) { obs.emplace_back(t, i); return false; });
    obs_clear(h, old_id);                                                         // obs = mObservations; mObservations.clear(); mbBad = true
    for (const auto &o : obs) {
        const size_t at = h->o_mp + (size_t)o.first * h->cap + o.second;
        if (obs_index(h, new_id, o.first) < 0) { h->poke(at, new_id); obs_add(h, new_id, o.first, o.second); }      // ReplaceMapPointMatch + AddObservation
        else h->poke(at, -1);                                                     // EraseMapPointMatch
    }
    return covis_flush(h);
}

extern "C" int sgx_covis_erase_keyframe(sgx_covis *h, int32_t kf_id)
{
    if (!h) return SGX_ERR_INVALID;
    const auto it = h->by_id.find(kf_id);
    if (it == h->by_id.end()) return SGX_ERR_INVALID;
    if (kf_id == 0) return SGX_OK;                                                // KeyFrame.cc:458-459
    const int s = it->second, N = h->slot[(size_t)s].n;
    for (const auto &e : h->loop_edges) if (e.first == s || e.second == s) return SGX_ERR_INVALID;      // rule 10: AddLoopEdge set mbNotErase (KeyFrame.cc:419-424, :460-464)
    for (int i = 0; i < N; i++) {
        const size_t at = h->o_mp + (size_t)s * h->cap + i;
        const int p = h->H(at);
        if (p < 0) continue;
        h->poke(at, -1);                                                          // the erased keyframe keeps nothing (the reference leaves its mvpMapPoints stale)
        point_erase_observation(h, p, s);
    }
    int rc = covis_flush(h);
    if (rc != SGX_OK) return rc;
    SgxCovisArgs A = covis_args(h);
    SGX_LAUNCH(k_covis_erase_graph, dim3(1), dim3(256), (sgx_stream_t)0, A, s);
    SGX_CHECK_HIP(hipGetLastError());
    SGX_CHECK_HIP(hipStreamSynchronize((sgx_stream_t)0));
    h->slot[(size_t)s].state = SGX_COVIS_DEAD; h->slot[(size_t)s].n = 0;
    h->dead_ids.insert(kf_id); h->by_id.erase(it); h->tables_dirty = true;
    return SGX_OK;
}

static int covis_sync_tables(sgx_covis *h)
{
    if (!h->tables_dirty) return SGX_OK;
    std::vector<int32_t> sid, sslot;
    for (const auto &e : h->by_id) { sid.push_back(e.first); sslot.push_back(e.second); }
    if (!sid.empty()) {
        SGX_CHECK_HIP(hipMemcpy(h->d_sorted_id, sid.data(), sid.size() * 4, hipMemcpyHostToDevice));
        SGX_CHECK_HIP(hipMemcpy(h->d_sorted_slot, sslot.data(), sslot.size() * 4, hipMemcpyHostToDevice));
    }
    h->tables_dirty = false;
    return SGX_OK;
}

// ---- getters: host pointers, synchronous
static int covis_slot_of(const sgx_covis *h, int32_t kf_id) { const auto it = h->by_id.find(kf_id); return it == h->by_id.end() ? -1 : it->second; }

extern "C" int sgx_covis_get_weights(sgx_covis *h, int32_t kf_id, int32_t *kf_ids, int32_t *weights, int32_t *n)
{
    if (!h || !n) return SGX_ERR_INVALID;
    const int s = covis_slot_of(h, kf_id);
    if (s < 0) return SGX_ERR_INVALID;
    std::vector<unsigned short> row((size_t)h->nslots);
    SGX_CHECK_HIP(hipMemcpy(row.data(), h->d_W + (size_t)s * h->max_kf, row.size() * 2, hipMemcpyDeviceToHost));
    std::vector<std::pair<int32_t, int32_t>> v;
    for (int t = 0; t < h->nslots; t++) if (row[(size_t)t]) v.emplace_back(h->slot[(size_t)t].id, (int32_t)row[(size_t)t]);
    std::sort(v.begin(), v.end());
    if (!v.empty() && (!kf_ids || !weights)) return SGX_ERR_INVALID;
    for (size_t j = 0; j < v.size(); j++) { kf_ids[j] = v[j].first; weights[j] = v[j].second; }
    *n = (int32_t)v.size();
    return SGX_OK;
}

static int covis_ordered(sgx_covis *h, int32_t kf_id, std::vector<int32_t> &ids, std::vector<int32_t> &w)
{
    if (covis_slot_of(h, kf_id) < 0) return SGX_ERR_INVALID;
    int rc = covis_sync_tables(h);
    if (rc != SGX_OK) return rc;
    SGX_CHECK_HIP(hipMemcpy(h->s_kf, &kf_id, 4, hipMemcpyHostToDevice));
    SgxCovisArgs A = covis_args(h);
    A.Q = 1; A.q_kf = h->s_kf;
    SGX_LAUNCH(k_covis_ordered, dim3(1), dim3(256), (sgx_stream_t)0, A);
    SGX_CHECK_HIP(hipGetLastError());
    SGX_CHECK_HIP(hipStreamSynchronize((sgx_stream_t)0));
    int32_t wq[CQ_FIELDS];
    SGX_CHECK_HIP(hipMemcpy(wq, h->ws_q, sizeof(wq), hipMemcpyDeviceToHost));
    ids.resize((size_t)wq[CQ_NORD]); w.resize(ids.size());
    if (!ids.empty()) {
        SGX_CHECK_HIP(hipMemcpy(ids.data(), h->ws_ord, ids.size() * 4, hipMemcpyDeviceToHost));
        SGX_CHECK_HIP(hipMemcpy(w.data(), h->ws_ordw, ids.size() * 4, hipMemcpyDeviceToHost));
        for (auto &x : ids) x = h->slot[(size_t)x].id;
    }
    return SGX_OK;
}

extern "C" int sgx_covis_get_ordered(sgx_covis *h, int32_t kf_id, int32_t *kf_ids, int32_t *weights, int32_t *n)
{
    if (!h || !n) return SGX_ERR_INVALID;
    std::vector<int32_t> ids, w;
    const int rc = covis_ordered(h, kf_id, ids, w);
    if (rc != SGX_OK) return rc;
    if (!ids.empty() && (!kf_ids || !weights)) return SGX_ERR_INVALID;
    for (size_t j = 0; j < ids.size(); j++) { kf_ids[j] = ids[j]; weights[j] = w[j]; }
    *n = (int32_t)ids.size();
    return SGX_OK;
}

extern "C" int sgx_covis_best_covisibles(sgx_covis *h, int32_t kf_id, int N, int32_t *kf_ids, int32_t *n)
{
    if (!h || !n || N < 0) return SGX_ERR_INVALID;
    std::vector<int32_t> ids, w;
    const int rc = covis_ordered(h, kf_id, ids, w);
    if (rc != SGX_OK) return rc;
    const size_t m = std::min(ids.size(), (size_t)N);
    if (m && !kf_ids) return SGX_ERR_INVALID;
    for (size_t j = 0; j < m; j++) kf_ids[j] = ids[j];
    *n = (int32_t)m;
    return SGX_OK;
}

extern "C" int sgx_covis_get_tree(sgx_covis *h, int32_t kf_id, int32_t *parent, int32_t *first_connection, int32_t *children, int32_t *n_children)
{
    if (!h) return SGX_ERR_INVALID;
    const int s = covis_slot_of(h, kf_id);
    if (s < 0) return SGX_ERR_INVALID;
    std::vector<int32_t> rec((size_t)h->nslots * CV_FIELDS);
    SGX_CHECK_HIP(hipMemcpy(rec.data(), h->d_kf, rec.size() * 4, hipMemcpyDeviceToHost));
    const int p = rec[(size_t)s * CV_FIELDS + CV_PARENT];
    if (parent) *parent = p >= 0 ? h->slot[(size_t)p].id : -1;
    if (first_connection) *first_connection = rec[(size_t)s * CV_FIELDS + CV_FIRST];
    std::vector<int32_t> c;
    for (int t = 0; t < h->nslots; t++) if (h->slot[(size_t)t].state == SGX_COVIS_LIVE && rec[(size_t)t * CV_FIELDS + CV_PARENT] == s) c.push_back(h->slot[(size_t)t].id);
    std::sort(c.begin(), c.end());
    if (n_children) *n_children = (int32_t)c.size();
    if (children) for (size_t j = 0; j < c.size(); j++) children[j] = c[j];
    return SGX_OK;
}

extern "C" int sgx_covis_get_observations(const sgx_covis *h, int32_t point_id, int32_t *kf_ids, int32_t *idx, int32_t *n, int32_t *n_obs)
{
    if (!h || !n || point_id < 0 || point_id >= h->max_points) return SGX_ERR_INVALID;
    std::vector<std::pair<int32_t, int32_t>> v;
    obs_each(h, point_id, [&](size_t, int t, int i) { v.emplace_back(h->slot[(size_t)t].id, i); return false; });
    std::sort(v.begin(), v.end());
    if (!v.empty() && (!kf_ids || !idx)) return SGX_ERR_INVALID;
    for (size_t j = 0; j < v.size(); j++) { kf_ids[j] = v[j].first; idx[j] = v[j].second; }
    *n = (int32_t)v.size();
    if (n_obs) *n_obs = h->heap[h->o_nobs + (size_t)point_id];
    return SGX_OK;
}

extern "C" int sgx_covis_get_keyframe_points(const sgx_covis *h, int32_t kf_id, int32_t *point_ids, int32_t *n)
{
    if (!h || !n) return SGX_ERR_INVALID;
    const int s = covis_slot_of(h, kf_id);
    if (s < 0) return SGX_ERR_INVALID;
    const int N = h->slot[(size_t)s].n;
    if (N && !point_ids) return SGX_ERR_INVALID;
    if (N) memcpy(point_ids, &h->heap[h->o_mp + (size_t)s * h->cap], (size_t)N * 4);
    *n = N;
    return SGX_OK;
}

// ---- the queries: device pointers, asynchronous on `stream`
extern "C" int sgx_covis_update_connections_batch_dev(sgx_covis *h, int Q, const int32_t *kf_ids_dev, sgx_covis_report *report_dev, void *stream)
{
    if (!h || Q < 0 || Q > h->max_q) return SGX_ERR_INVALID;
    if (Q == 0) return SGX_OK;
    if (!kf_ids_dev || !report_dev) return SGX_ERR_INVALID;
    const int rc = covis_sync_tables(h);
    if (rc != SGX_OK) return rc;
    const sgx_stream_t s = (sgx_stream_t)stream;
    SgxCovisArgs A = covis_args(h);
    A.Q = Q; A.q_kf = kf_ids_dev; A.report = (SgxCovisReport *)report_dev;
    SGX_LAUNCH(k_covis_count, dim3((unsigned)Q), dim3(256), s, A);
    SGX_LAUNCH(k_covis_apply, dim3(1), dim3(256), s, A);
    SGX_CHECK_HIP(hipGetLastError());
    return SGX_OK;
}

extern "C" int sgx_covis_local_map_batch_dev(sgx_covis *h, int Q, int cap, int32_t *frame_mp_dev, const int32_t *n_dev, const int32_t *min_obs_dev, int32_t *local_kf_dev,
                                             int32_t *n_local_kf_dev, int32_t *ref_kf_dev, int32_t *ref_tracked_dev, int mcap, int32_t *local_points_dev, int32_t *local_obs_dev,
                                             int32_t *n_local_points_dev, sgx_covis_report *report_dev, void *stream)
{
    if (!h || Q < 0 || Q > h->max_q || cap < 0 || mcap < 0) return SGX_ERR_INVALID;
    if (Q == 0) return SGX_OK;
    if (!frame_mp_dev || !n_dev || !min_obs_dev || !local_kf_dev || !n_local_kf_dev || !ref_kf_dev || !ref_tracked_dev || !local_points_dev || !local_obs_dev ||
        !n_local_points_dev || !report_dev) return SGX_ERR_INVALID;
    const int rc = covis_sync_tables(h);
    if (rc != SGX_OK) return rc;
    const sgx_stream_t s = (sgx_stream_t)stream;
    SgxCovisArgs A = covis_args(h);
    A.Q = Q; A.report = (SgxCovisReport *)report_dev;
    A.f_cap = cap; A.frame_mp = frame_mp_dev; A.f_n = n_dev; A.min_obs = min_obs_dev; A.local_kf = local_kf_dev; A.n_local_kf = n_local_kf_dev; A.ref_kf = ref_kf_dev;
    A.ref_tracked = ref_tracked_dev; A.mcap = mcap; A.local_points = local_points_dev; A.local_obs = local_obs_dev; A.n_local_points = n_local_points_dev;
    const unsigned G = (unsigned)std::max(1, std::min(h->nslots, (int)COVIS_GRID));
    SGX_CHECK_HIP(hipMemsetAsync(h->d_stamp, 0x7f, (size_t)Q * h->max_points * 4, s));
    SGX_LAUNCH(k_covis_lm_votes, dim3((unsigned)Q), dim3(256), s, A);
    SGX_LAUNCH(k_covis_lm_top, dim3((unsigned)SGX_COVIS_LOCAL_LIMIT, (unsigned)Q), dim3(256), s, A);
    SGX_LAUNCH(k_covis_lm_stage2, dim3((unsigned)Q), dim3(64), s, A);
    SGX_LAUNCH(k_covis_lm_stamp, dim3(G, (unsigned)Q), dim3(256), s, A);
    SGX_LAUNCH(k_covis_lm_count, dim3(G, (unsigned)Q), dim3(256), s, A);
    SGX_LAUNCH(k_covis_lm_emit, dim3(G, (unsigned)Q), dim3(256), s, A);
    SGX_CHECK_HIP(hipGetLastError());
    return SGX_OK;
}

extern "C" int sgx_covis_keyframe_culling_batch_dev(sgx_covis *h, int Q, const int32_t *kf_ids_dev, int max_cand, int32_t *cand_dev, int32_t *n_cand_dev,
                                                    int32_t *n_redundant_dev, int32_t *n_mps_dev, int32_t *cull_dev, void *stream)
{
    if (!h || Q < 0 || Q > h->max_q || max_cand < 1) return SGX_ERR_INVALID;
    if (Q == 0) return SGX_OK;
    if (!kf_ids_dev || !cand_dev || !n_cand_dev || !n_redundant_dev || !n_mps_dev || !cull_dev) return SGX_ERR_INVALID;
    const int rc = covis_sync_tables(h);
    if (rc != SGX_OK) return rc;
    const sgx_stream_t s = (sgx_stream_t)stream;
    SgxCovisArgs A = covis_args(h);
    A.Q = Q; A.q_kf = kf_ids_dev; A.max_cand = max_cand; A.cand = cand_dev; A.n_cand = n_cand_dev; A.n_red = n_redundant_dev; A.n_mps = n_mps_dev; A.cull = cull_dev;
    SGX_LAUNCH(k_covis_ordered, dim3((unsigned)Q), dim3(256), s, A);
    const unsigned G = (unsigned)std::max(1, std::min(h->nslots, max_cand));
    SGX_LAUNCH(k_covis_cull, dim3(G, (unsigned)Q), dim3(256), s, A);
    SGX_CHECK_HIP(hipGetLastError());
    return SGX_OK;
}

extern "C" int sgx_covis_ba_graph_batch_dev(sgx_covis *h, int Q, int mode, const int32_t *kf_ids_dev, int32_t *pose_id_dev, uint8_t *pose_fixed_dev, int pcap,
                                            int32_t *point_id_dev, int32_t *point_edge_begin_dev, int ecap, int32_t *edge_pose_dev, int32_t *edge_point_dev,
                                            int32_t *edge_kp_dev, uint8_t *edge_attr_dev, sgx_covis_ba_report *report_dev, void *stream)
{
    if (!h || Q < 0 || Q > h->max_q || (mode != SGX_COVIS_BA_LOCAL && mode != SGX_COVIS_BA_GLOBAL) || (mode == SGX_COVIS_BA_GLOBAL && Q != 1)) return SGX_ERR_INVALID;
    if (Q == 0) return SGX_OK;
    if ((mode == SGX_COVIS_BA_LOCAL && !kf_ids_dev) || !pose_id_dev || !pose_fixed_dev || !point_edge_begin_dev || !report_dev || (pcap > 0 && !point_id_dev) ||
        (ecap > 0 && (!edge_pose_dev || !edge_point_dev || !edge_kp_dev || !edge_attr_dev))) return SGX_ERR_INVALID;
    const int rc = covis_sync_tables(h);
    if (rc != SGX_OK) return rc;
    const sgx_stream_t s = (sgx_stream_t)stream;
    SgxCovisArgs A = covis_args(h);
    A.Q = Q; A.q_kf = kf_ids_dev; A.ba_global = mode == SGX_COVIS_BA_GLOBAL; A.pcap = pcap; A.ecap = ecap; A.pose_id = pose_id_dev; A.pose_fixed = pose_fixed_dev;
    A.point_id = point_id_dev; A.point_begin = point_edge_begin_dev; A.edge_pose = edge_pose_dev; A.edge_point = edge_point_dev; A.edge_kp = edge_kp_dev;
    A.edge_attr = edge_attr_dev; A.ba_report = (SgxCovisBaReport *)report_dev;
    const unsigned G = (unsigned)std::max(1, std::min(h->nslots, (int)COVIS_GRID));
    SGX_LAUNCH(k_covis_ba_begin, dim3((unsigned)Q), dim3(256), s, A);
    if (A.ba_global) {
        SGX_LAUNCH(k_covis_ba_all_count, dim3((unsigned)std::max(1, std::min((h->max_points + 255) / 256, 4 * (int)COVIS_GRID))), dim3(256), s, A);
        SGX_LAUNCH(k_covis_ba_all_points, dim3(1), dim3(256), s, A);
    } else {
        SGX_CHECK_HIP(hipMemsetAsync(h->d_stamp, 0x7f, (size_t)Q * h->max_points * 4, s));
        SGX_LAUNCH(k_covis_lm_stamp, dim3(G, (unsigned)Q), dim3(256), s, A);
        SGX_LAUNCH(k_covis_ba_count, dim3(G, (unsigned)Q), dim3(256), s, A);
    }
    SGX_LAUNCH(k_covis_ba_poses, dim3((unsigned)Q), dim3(256), s, A);
    if (!A.ba_global) SGX_LAUNCH(k_covis_ba_points, dim3(G, (unsigned)Q), dim3(256), s, A);
    SGX_LAUNCH(k_covis_ba_scan, dim3((unsigned)Q), dim3(256), s, A);
    SGX_LAUNCH(k_covis_ba_edges, dim3((unsigned)std::max(1, std::min(std::max(pcap, 0) / 4 + 1, 8 * (int)COVIS_GRID)), (unsigned)Q), dim3(256), s, A);
    SGX_CHECK_HIP(hipGetLastError());
    return SGX_OK;
}

// ---- one query from host memory through the batch entries: staged in device buffers of the call, run on the legacy stream, read back
template <class T> static int covis_stage(SgxDevMem &m, T **d, const T *src, size_t n, size_t cap)
{
    const int rc = m.alloc(d, cap);
    if (rc != SGX_OK) return rc;
    if (n && src) SGX_CHECK_HIP(hipMemcpy(*d, src, n * sizeof(T), hipMemcpyHostToDevice));
    return SGX_OK;
}

extern "C" int sgx_covis_update_connections(sgx_covis *h, int32_t kf_id, sgx_covis_report *report)
{
    if (!h) return SGX_ERR_INVALID;
    SgxDevMem m; int32_t *d_id = nullptr; sgx_covis_report *d_rep = nullptr; int rc;
    if ((rc = covis_stage(m, &d_id, &kf_id, 1, 1)) || (rc = m.alloc(&d_rep, 1))) return rc;
    if ((rc = sgx_covis_update_connections_batch_dev(h, 1, d_id, d_rep, nullptr)) != SGX_OK) return rc;
    sgx_covis_report R;
    SGX_CHECK_HIP(hipStreamSynchronize((sgx_stream_t)0));
    SGX_CHECK_HIP(hipMemcpy(&R, d_rep, sizeof(R), hipMemcpyDeviceToHost));
    if (report) *report = R;
    return R.status;
}

extern "C" int sgx_covis_local_map(sgx_covis *h, int n, int32_t *frame_mp, int min_obs, int32_t *local_kf, int32_t *n_local_kf, int32_t *ref_kf, int32_t *ref_tracked,
                                   int mcap, int32_t *local_points, int32_t *local_obs, int32_t *n_local_points, sgx_covis_report *report)
{
    if (!h || n < 0 || (n > 0 && !frame_mp) || !local_kf || !n_local_kf || !ref_kf || mcap < 0 || (mcap > 0 && (!local_points || !local_obs)) || !n_local_points) return SGX_ERR_INVALID;
    if (*n_local_kf < 0 || *n_local_kf > h->max_kf) return SGX_ERR_INVALID;
    SgxDevMem m; int rc;
    int32_t *d_f = nullptr, *d_n = nullptr, *d_mo = nullptr, *d_lk = nullptr, *d_nlk = nullptr, *d_ref = nullptr, *d_rt = nullptr, *d_pts = nullptr, *d_obs = nullptr, *d_np = nullptr;
    sgx_covis_report *d_rep = nullptr;
    const int32_t n32 = n, mo32 = min_obs;
    if ((rc = covis_stage(m, &d_f, (const int32_t *)frame_mp, (size_t)n, (size_t)n)) || (rc = covis_stage(m, &d_n, &n32, 1, 1)) || (rc = covis_stage(m, &d_mo, &mo32, 1, 1)) ||
        (rc = covis_stage(m, &d_lk, (const int32_t *)local_kf, (size_t)*n_local_kf, (size_t)h->max_kf)) || (rc = covis_stage(m, &d_nlk, (const int32_t *)n_local_kf, 1, 1)) ||
        (rc = covis_stage(m, &d_ref, (const int32_t *)ref_kf, 1, 1)) || (rc = m.alloc(&d_rt, 1)) || (rc = m.alloc(&d_pts, (size_t)mcap)) || (rc = m.alloc(&d_obs, (size_t)mcap)) ||
        (rc = m.alloc(&d_np, 1)) || (rc = m.alloc(&d_rep, 1))) return rc;
    if ((rc = sgx_covis_local_map_batch_dev(h, 1, n, d_f, d_n, d_mo, d_lk, d_nlk, d_ref, d_rt, mcap, d_pts, d_obs, d_np, d_rep, nullptr)) != SGX_OK) return rc;
    SGX_CHECK_HIP(hipStreamSynchronize((sgx_stream_t)0));
    sgx_covis_report R;
    SGX_CHECK_HIP(hipMemcpy(&R, d_rep, sizeof(R), hipMemcpyDeviceToHost));
    if (report) *report = R;
    if (R.status == SGX_ERR_INVALID) return R.status;                              // nothing of the query was written
    int32_t np = 0;
    SGX_CHECK_HIP(hipMemcpy(&np, d_np, 4, hipMemcpyDeviceToHost));
    SGX_CHECK_HIP(hipMemcpy(n_local_kf, d_nlk, 4, hipMemcpyDeviceToHost));
    SGX_CHECK_HIP(hipMemcpy(ref_kf, d_ref, 4, hipMemcpyDeviceToHost));
    if (ref_tracked) SGX_CHECK_HIP(hipMemcpy(ref_tracked, d_rt, 4, hipMemcpyDeviceToHost));
    if (n) SGX_CHECK_HIP(hipMemcpy(frame_mp, d_f, (size_t)n * 4, hipMemcpyDeviceToHost));
    if (*n_local_kf) SGX_CHECK_HIP(hipMemcpy(local_kf, d_lk, (size_t)*n_local_kf * 4, hipMemcpyDeviceToHost));
    const size_t w = (size_t)std::min(np, mcap);
    if (w) { SGX_CHECK_HIP(hipMemcpy(local_points, d_pts, w * 4, hipMemcpyDeviceToHost)); SGX_CHECK_HIP(hipMemcpy(local_obs, d_obs, w * 4, hipMemcpyDeviceToHost)); }
    *n_local_points = np;
    return R.status;                                                               // SGX_OK, or SGX_ERR_NOMEM with the first mcap points written
}

extern "C" int sgx_covis_keyframe_culling(sgx_covis *h, int32_t kf_id, int max_cand, int32_t *cand, int32_t *n_cand, int32_t *n_redundant, int32_t *n_mps, int32_t *cull)
{
    if (!h || max_cand < 1 || !cand || !n_cand || !n_redundant || !n_mps || !cull) return SGX_ERR_INVALID;
    SgxDevMem m; int rc;
    int32_t *d_id = nullptr, *d_c = nullptr, *d_nc = nullptr, *d_r = nullptr, *d_m = nullptr, *d_v = nullptr;
    if ((rc = covis_stage(m, &d_id, &kf_id, 1, 1)) || (rc = m.alloc(&d_c, (size_t)max_cand)) || (rc = m.alloc(&d_nc, 1)) || (rc = m.alloc(&d_r, (size_t)max_cand)) ||
        (rc = m.alloc(&d_m, (size_t)max_cand)) || (rc = m.alloc(&d_v, (size_t)max_cand))) return rc;
    if ((rc = sgx_covis_keyframe_culling_batch_dev(h, 1, d_id, max_cand, d_c, d_nc, d_r, d_m, d_v, nullptr)) != SGX_OK) return rc;
    SGX_CHECK_HIP(hipStreamSynchronize((sgx_stream_t)0));
    int32_t nc = 0;
    SGX_CHECK_HIP(hipMemcpy(&nc, d_nc, 4, hipMemcpyDeviceToHost));
    if (nc < 0) return nc;
    const size_t w = (size_t)std::min(nc, max_cand);
    if (w) {
        SGX_CHECK_HIP(hipMemcpy(cand, d_c, w * 4, hipMemcpyDeviceToHost)); SGX_CHECK_HIP(hipMemcpy(n_redundant, d_r, w * 4, hipMemcpyDeviceToHost));
        SGX_CHECK_HIP(hipMemcpy(n_mps, d_m, w * 4, hipMemcpyDeviceToHost)); SGX_CHECK_HIP(hipMemcpy(cull, d_v, w * 4, hipMemcpyDeviceToHost));
    }
    *n_cand = nc;
    return SGX_OK;
}

extern "C" int sgx_covis_ba_graph(sgx_covis *h, int mode, int32_t kf_id, int32_t *pose_id, uint8_t *pose_fixed, int pcap, int32_t *point_id, int32_t *point_edge_begin,
                                  int ecap, int32_t *edge_pose, int32_t *edge_point, int32_t *edge_kp, uint8_t *edge_attr, sgx_covis_ba_report *report)
{
    if (!h || !pose_id || !pose_fixed || !point_edge_begin || (pcap > 0 && !point_id) || (ecap > 0 && (!edge_pose || !edge_point || !edge_kp || !edge_attr))) return SGX_ERR_INVALID;
    SgxDevMem m; int rc;
    const size_t pc = (size_t)std::max(pcap, 0), ec = (size_t)std::max(ecap, 0);
    int32_t *d_id = nullptr, *d_pid = nullptr, *d_pts = nullptr, *d_beg = nullptr, *d_ep = nullptr, *d_el = nullptr, *d_ek = nullptr;
    uint8_t *d_pf = nullptr, *d_ea = nullptr; sgx_covis_ba_report *d_rep = nullptr;
    if ((rc = covis_stage(m, &d_id, &kf_id, 1, 1)) || (rc = m.alloc(&d_pid, (size_t)h->max_kf)) || (rc = m.alloc(&d_pf, (size_t)h->max_kf)) || (rc = m.alloc(&d_pts, pc)) ||
        (rc = m.alloc(&d_beg, pc + 1)) || (rc = m.alloc(&d_ep, ec)) || (rc = m.alloc(&d_el, ec)) || (rc = m.alloc(&d_ek, ec)) || (rc = m.alloc(&d_ea, ec)) ||
        (rc = m.alloc(&d_rep, 1))) return rc;
    if ((rc = sgx_covis_ba_graph_batch_dev(h, 1, mode, d_id, d_pid, d_pf, pcap, d_pts, d_beg, ecap, d_ep, d_el, d_ek, d_ea, d_rep, nullptr)) != SGX_OK) return rc;
    SGX_CHECK_HIP(hipStreamSynchronize((sgx_stream_t)0));
    sgx_covis_ba_report R;
    SGX_CHECK_HIP(hipMemcpy(&R, d_rep, sizeof(R), hipMemcpyDeviceToHost));
    if (report) *report = R;
    if (R.status == SGX_ERR_INVALID) return R.status;                              // nothing of the query was written
    const size_t np = (size_t)std::min(R.n_points, pcap);
    if (R.n_poses) { SGX_CHECK_HIP(hipMemcpy(pose_id, d_pid, (size_t)R.n_poses * 4, hipMemcpyDeviceToHost)); SGX_CHECK_HIP(hipMemcpy(pose_fixed, d_pf, (size_t)R.n_poses, hipMemcpyDeviceToHost)); }
    if (np) SGX_CHECK_HIP(hipMemcpy(point_id, d_pts, np * 4, hipMemcpyDeviceToHost));
    SGX_CHECK_HIP(hipMemcpy(point_edge_begin, d_beg, (np + 1) * 4, hipMemcpyDeviceToHost));
    size_t ne = 0;                                                                 // the edges of the leading points that fit wholly
    for (size_t i = 0; i < np && point_edge_begin[i + 1] <= ecap; i++) ne = (size_t)point_edge_begin[i + 1];
    if (ne) {
        SGX_CHECK_HIP(hipMemcpy(edge_pose, d_ep, ne * 4, hipMemcpyDeviceToHost)); SGX_CHECK_HIP(hipMemcpy(edge_point, d_el, ne * 4, hipMemcpyDeviceToHost));
        SGX_CHECK_HIP(hipMemcpy(edge_kp, d_ek, ne * 4, hipMemcpyDeviceToHost)); SGX_CHECK_HIP(hipMemcpy(edge_attr, d_ea, ne, hipMemcpyDeviceToHost));
    }
    return R.status;                                                               // SGX_OK, or SGX_ERR_NOMEM with what fits written
}

// ---- loop closing: mspLoopEdges, and CorrectLoop's group, LoopConnections and essential graph as launch sequences (sgx_covis_loop_kernels.h)
// a buffer the handle does not hold yet; its size goes into loop_bytes where it is taken, so a call that fails half way is continued by the next one
template <class T> static int covis_loop_take(sgx_covis *h, T **p, size_t n)
{
    if (*p) return SGX_OK;
    const int rc = h->mem.alloc(p, n);
    if (rc == SGX_OK) h->loop_bytes += (int64_t)(n * sizeof(T));
    return rc;
}

static int covis_loop_ws(sgx_covis *h)
{
    const size_t N = (size_t)h->max_kf;
    int rc;
    if ((rc = covis_loop_take(h, &h->lw_s, (size_t)LS_FIELDS)) || (rc = covis_loop_take(h, &h->lw_q, N * CQ_FIELDS)) || (rc = covis_loop_take(h, &h->lw_qkf, N)) ||
        (rc = covis_loop_take(h, &h->lw_ord, N)) || (rc = covis_loop_take(h, &h->lw_gslot, N)) || (rc = covis_loop_take(h, &h->lw_grank, N)) ||
        (rc = covis_loop_take(h, &h->lw_rowg, N)) || (rc = covis_loop_take(h, &h->lw_gof, N)) || (rc = covis_loop_take(h, &h->lw_vidx, N)) ||
        (rc = covis_loop_take(h, &h->lw_vcnt, N)) || (rc = covis_loop_take(h, &h->lw_vbase, N)) || (rc = covis_loop_take(h, &h->lw_flags, N * N)) ||
        (rc = covis_loop_take(h, &h->lw_rep, N)) || (rc = covis_loop_take(h, &h->d_le, 2 * N))) return rc;
    return SGX_OK;
}

extern "C" int sgx_covis_loop_info(const sgx_covis *h, int64_t *loop_bytes, int32_t *n_loop_edges)
{
    if (!h) return SGX_ERR_INVALID;
    if (loop_bytes) *loop_bytes = h->loop_bytes;
    if (n_loop_edges) *n_loop_edges = (int32_t)h->loop_edges.size();
    return SGX_OK;
}

extern "C" int sgx_covis_add_loop_edge(sgx_covis *h, int32_t kf_a, int32_t kf_b)
{
    if (!h || kf_a == kf_b) return SGX_ERR_INVALID;
    const int a = covis_slot_of(h, kf_a), b = covis_slot_of(h, kf_b);
    if (a < 0 || b < 0) return SGX_ERR_INVALID;
    for (const auto &e : h->loop_edges) if ((e.first == a && e.second == b) || (e.first == b && e.second == a)) return SGX_OK;      // a set: nothing changes
    if ((int)h->loop_edges.size() >= h->max_kf) return SGX_ERR_NOMEM;
    const int rc = covis_loop_ws(h);
    if (rc != SGX_OK) return rc;
    const int32_t pair[2] = { a, b };
    SGX_CHECK_HIP(hipMemcpy(h->d_le + 2 * h->loop_edges.size(), pair, sizeof(pair), hipMemcpyHostToDevice));      // the changed words only
    h->loop_edges.emplace_back(a, b);
    return SGX_OK;
}

extern "C" int sgx_covis_get_loop_edges(const sgx_covis *h, int32_t kf_id, int32_t *kf_ids, int32_t *n)
{
    if (!h || !n) return SGX_ERR_INVALID;
    const int s = covis_slot_of(h, kf_id);
    if (s < 0) return SGX_ERR_INVALID;
    std::vector<int32_t> v;
    for (const auto &e : h->loop_edges) if (e.first == s || e.second == s) v.push_back(h->slot[(size_t)(e.first == s ? e.second : e.first)].id);
    std::sort(v.begin(), v.end());
    if (!v.empty() && !kf_ids) return SGX_ERR_INVALID;
    for (size_t j = 0; j < v.size(); j++) kf_ids[j] = v[j];
    *n = (int32_t)v.size();
    return SGX_OK;
}

static SgxCovisLoopArgs covis_loop_args(sgx_covis *h)
{
    SgxCovisLoopArgs L{};
    L.n_le = (int)h->loop_edges.size(); L.le = h->d_le; L.s = h->lw_s; L.qkf = h->lw_qkf; L.ord = h->lw_ord; L.gslot = h->lw_gslot; L.grank = h->lw_grank; L.rowg = h->lw_rowg;
    L.gof = h->lw_gof; L.vidx = h->lw_vidx; L.vcnt = h->lw_vcnt; L.vbase = h->lw_vbase; L.flags = h->lw_flags;
    return L;
}

// the argument block of the UpdateConnections queries of a loop sequence: Q queries whose ids, scalars, count rows and reports live in the loop workspace
static SgxCovisArgs covis_loop_uc_args(sgx_covis *h, int Q)
{
    SgxCovisArgs A = covis_args(h);
    A.Q = Q; A.q_kf = h->lw_qkf; A.ws_q = h->lw_q; A.ws_cnt = h->lw_flags; A.report = h->lw_rep;
    return A;
}

extern "C" int sgx_covis_loop_begin_dev(sgx_covis *h, int32_t cur, int32_t *group_id_dev, int32_t *group_vertex_dev, int pcap, int32_t *point_id_dev, int32_t *point_ref_dev,
                                        sgx_covis_loop_report *report_dev, void *stream)
{
    if (!h || covis_slot_of(h, cur) < 0 || !group_id_dev || !group_vertex_dev || pcap < 0 || (pcap > 0 && (!point_id_dev || !point_ref_dev)) || !report_dev) return SGX_ERR_INVALID;
    int rc;
    if ((rc = covis_loop_ws(h)) != SGX_OK || (rc = covis_sync_tables(h)) != SGX_OK) return rc;
    const sgx_stream_t s = (sgx_stream_t)stream;
    const int nlive = (int)h->by_id.size();
    SgxCovisArgs A = covis_args(h);
    SgxCovisLoopArgs L = covis_loop_args(h);
    L.cur = cur; L.pcap = pcap; L.group_id = group_id_dev; L.group_vertex = group_vertex_dev; L.point_id = point_id_dev; L.point_ref = point_ref_dev;
    L.report = (SgxCovisLoopReport *)report_dev;
    const unsigned G = (unsigned)std::max(1, std::min(h->nslots, (int)COVIS_GRID));
    SgxCovisArgs U1 = covis_loop_uc_args(h, 1), Un = covis_loop_uc_args(h, nlive);
    SGX_LAUNCH(k_covis_loop_fill, dim3(1), dim3(256), s, h->lw_qkf, 1, (int)cur, -1);
    SGX_LAUNCH(k_covis_count, dim3(1), dim3(256), s, U1);                          // mpCurrentKF->UpdateConnections() (:433)
    SGX_LAUNCH(k_covis_apply, dim3(1), dim3(256), s, U1);
    SGX_LAUNCH(k_covis_loop_group, dim3(1), dim3(256), s, A, L);
    SGX_LAUNCH(k_covis_count, dim3((unsigned)nlive), dim3(256), s, Un);            // pKFi->UpdateConnections() of :515 in the order of CorrectedSim3; the queries
    SGX_LAUNCH(k_covis_apply, dim3(1), dim3(256), s, Un);                          // behind the group name no keyframe
    SGX_CHECK_HIP(hipMemsetAsync(h->d_stamp, 0x7f, (size_t)h->max_points * 4, s));
    SGX_LAUNCH(k_covis_lm_stamp, dim3(G, 1), dim3(256), s, A);
    SGX_LAUNCH(k_covis_lm_count, dim3(G, 1), dim3(256), s, A);
    SGX_LAUNCH(k_covis_loop_points, dim3(G), dim3(256), s, A, L);
    SGX_CHECK_HIP(hipGetLastError());
    return SGX_OK;
}

extern "C" int sgx_covis_loop_connections_dev(sgx_covis *h, int32_t cur, int n_group, const int32_t *group_id_dev, int lcap, int32_t *lc_begin_dev, int32_t *lc_j_dev,
                                              sgx_covis_loop_report *report_dev, void *stream)
{
    if (!h || covis_slot_of(h, cur) < 0 || n_group < 1 || n_group > (int)h->by_id.size() || !group_id_dev || lcap < 0 || !lc_begin_dev || (lcap > 0 && !lc_j_dev) || !report_dev)
        return SGX_ERR_INVALID;
    int rc;
    if ((rc = covis_loop_ws(h)) != SGX_OK || (rc = covis_sync_tables(h)) != SGX_OK) return rc;
    const sgx_stream_t s = (sgx_stream_t)stream;
    SgxCovisArgs A = covis_args(h), U = covis_loop_uc_args(h, n_group);
    SgxCovisLoopArgs L = covis_loop_args(h);
    L.cur = cur; L.n_group = n_group; L.group_id = (int32_t *)group_id_dev; L.lcap = lcap; L.lc_begin = lc_begin_dev; L.lc_j = lc_j_dev; L.report = (SgxCovisLoopReport *)report_dev;
    SGX_LAUNCH(k_covis_lc_begin, dim3(1), dim3(256), s, A, L);
    SGX_LAUNCH(k_covis_count, dim3((unsigned)n_group), dim3(256), s, U);
    SGX_LAUNCH(k_covis_lc_apply, dim3(1), dim3(256), s, U, L);
    SGX_LAUNCH(k_covis_lc_emit, dim3((unsigned)std::min(n_group, (int)COVIS_GRID)), dim3(256), s, A, L);
    SGX_CHECK_HIP(hipGetLastError());
    return SGX_OK;
}

extern "C" int sgx_covis_essential_graph_dev(sgx_covis *h, int32_t cur, int32_t loop, int n_group, const int32_t *group_id_dev, int lcap, const int32_t *lc_begin_dev,
                                             const int32_t *lc_j_dev, int32_t *vertex_id_dev, uint8_t *vertex_fixed_dev, int32_t *vertex_group_dev, int ecap, int32_t *e_i_dev,
                                             int32_t *e_j_dev, uint8_t *e_kind_dev, sgx_covis_loop_report *report_dev, void *stream)
{
    if (!h || covis_slot_of(h, cur) < 0 || covis_slot_of(h, loop) < 0 || n_group < 1 || n_group > (int)h->by_id.size() || !group_id_dev || lcap < 0 || !lc_begin_dev ||
        (lcap > 0 && !lc_j_dev) || !vertex_id_dev || !vertex_fixed_dev || !vertex_group_dev || ecap < 0 || (ecap > 0 && (!e_i_dev || !e_j_dev || !e_kind_dev)) || !report_dev)
        return SGX_ERR_INVALID;
    int rc;
    if ((rc = covis_loop_ws(h)) != SGX_OK || (rc = covis_sync_tables(h)) != SGX_OK) return rc;
    const sgx_stream_t s = (sgx_stream_t)stream;
    SgxCovisArgs A = covis_args(h);
    SgxCovisLoopArgs L = covis_loop_args(h);
    L.cur = cur; L.loop = loop; L.n_group = n_group; L.group_id = (int32_t *)group_id_dev; L.lcap = lcap; L.lc_begin = (int32_t *)lc_begin_dev; L.lc_j = (int32_t *)lc_j_dev;
    L.vertex_id = vertex_id_dev; L.vertex_fixed = vertex_fixed_dev; L.vertex_group = vertex_group_dev; L.ecap = ecap; L.e_i = e_i_dev; L.e_j = e_j_dev; L.e_kind = e_kind_dev;
    L.report = (SgxCovisLoopReport *)report_dev;
    const unsigned G = (unsigned)std::max(1, std::min((int)h->by_id.size(), (int)COVIS_GRID));
    SGX_LAUNCH(k_covis_eg_begin, dim3(1), dim3(256), s, A, L);
    SGX_LAUNCH(k_covis_eg_vertex<0>, dim3(G), dim3(256), s, A, L);
    SGX_LAUNCH(k_covis_eg_scan, dim3(1), dim3(256), s, A, L);
    SGX_LAUNCH(k_covis_eg_vertex<1>, dim3(G), dim3(256), s, A, L);
    SGX_CHECK_HIP(hipGetLastError());
    return SGX_OK;
}

// one call from host memory: staged, run on the legacy stream, read back; the return value is the report's status
extern "C" int sgx_covis_loop_begin(sgx_covis *h, int32_t cur, int32_t *group_id, int32_t *group_vertex, int pcap, int32_t *point_id, int32_t *point_ref, sgx_covis_loop_report *report)
{
    if (!h || !group_id || !group_vertex || pcap < 0 || (pcap > 0 && (!point_id || !point_ref))) return SGX_ERR_INVALID;
    SgxDevMem m; int rc;
    int32_t *d_g = nullptr, *d_v = nullptr, *d_p = nullptr, *d_r = nullptr; sgx_covis_loop_report *d_rep = nullptr;
    if ((rc = m.alloc(&d_g, (size_t)h->max_kf)) || (rc = m.alloc(&d_v, (size_t)h->max_kf)) || (rc = m.alloc(&d_p, (size_t)pcap)) || (rc = m.alloc(&d_r, (size_t)pcap)) ||
        (rc = m.alloc(&d_rep, 1))) return rc;
    if ((rc = sgx_covis_loop_begin_dev(h, cur, d_g, d_v, pcap, d_p, d_r, d_rep, nullptr)) != SGX_OK) return rc;
    SGX_CHECK_HIP(hipStreamSynchronize((sgx_stream_t)0));
    sgx_covis_loop_report R;
    SGX_CHECK_HIP(hipMemcpy(&R, d_rep, sizeof(R), hipMemcpyDeviceToHost));
    if (report) *report = R;
    SGX_CHECK_HIP(hipMemcpy(group_id, d_g, (size_t)R.n_group * 4, hipMemcpyDeviceToHost));
    SGX_CHECK_HIP(hipMemcpy(group_vertex, d_v, (size_t)R.n_group * 4, hipMemcpyDeviceToHost));
    const size_t np = (size_t)std::min(R.n_points, pcap);
    if (np) { SGX_CHECK_HIP(hipMemcpy(point_id, d_p, np * 4, hipMemcpyDeviceToHost)); SGX_CHECK_HIP(hipMemcpy(point_ref, d_r, np * 4, hipMemcpyDeviceToHost)); }
    return R.status;                                                               // SGX_OK, or SGX_ERR_NOMEM with the first pcap points written
}

extern "C" int sgx_covis_loop_connections(sgx_covis *h, int32_t cur, int n_group, const int32_t *group_id, int lcap, int32_t *lc_begin, int32_t *lc_j, sgx_covis_loop_report *report)
{
    if (!h || n_group < 1 || n_group > h->max_kf || !group_id || lcap < 0 || !lc_begin || (lcap > 0 && !lc_j)) return SGX_ERR_INVALID;
    SgxDevMem m; int rc;
    int32_t *d_g = nullptr, *d_b = nullptr, *d_j = nullptr; sgx_covis_loop_report *d_rep = nullptr;
    if ((rc = covis_stage(m, &d_g, group_id, (size_t)n_group, (size_t)n_group)) || (rc = m.alloc(&d_b, (size_t)n_group + 1)) || (rc = m.alloc(&d_j, (size_t)lcap)) ||
        (rc = m.alloc(&d_rep, 1))) return rc;
    if ((rc = sgx_covis_loop_connections_dev(h, cur, n_group, d_g, lcap, d_b, d_j, d_rep, nullptr)) != SGX_OK) return rc;
    SGX_CHECK_HIP(hipStreamSynchronize((sgx_stream_t)0));
    sgx_covis_loop_report R;
    SGX_CHECK_HIP(hipMemcpy(&R, d_rep, sizeof(R), hipMemcpyDeviceToHost));
    if (report) *report = R;
    if (R.status == SGX_ERR_INVALID) return R.status;                              // nothing of the call was written, and the handle is unchanged
    SGX_CHECK_HIP(hipMemcpy(lc_begin, d_b, ((size_t)n_group + 1) * 4, hipMemcpyDeviceToHost));
    size_t nw = 0;                                                                 // the rows that fit wholly
    for (int r = 0; r < n_group && lc_begin[r + 1] <= lcap; r++) nw = (size_t)lc_begin[r + 1];
    if (nw) SGX_CHECK_HIP(hipMemcpy(lc_j, d_j, nw * 4, hipMemcpyDeviceToHost));
    return R.status;
}

extern "C" int sgx_covis_essential_graph(sgx_covis *h, int32_t cur, int32_t loop, int n_group, const int32_t *group_id, const int32_t *lc_begin, const int32_t *lc_j,
                                         int32_t *vertex_id, uint8_t *vertex_fixed, int32_t *vertex_group, int ecap, int32_t *e_i, int32_t *e_j, uint8_t *e_kind,
                                         sgx_covis_loop_report *report)
{
    if (!h || n_group < 1 || n_group > h->max_kf || !group_id || !lc_begin || lc_begin[n_group] < 0 || (lc_begin[n_group] > 0 && !lc_j) || !vertex_id || !vertex_fixed ||
        !vertex_group || ecap < 0 || (ecap > 0 && (!e_i || !e_j || !e_kind))) return SGX_ERR_INVALID;
    SgxDevMem m; int rc;
    const int lcap = lc_begin[n_group];
    int32_t *d_g = nullptr, *d_b = nullptr, *d_j = nullptr, *d_vi = nullptr, *d_vg = nullptr, *d_ei = nullptr, *d_ej = nullptr; uint8_t *d_vf = nullptr, *d_ek = nullptr;
    sgx_covis_loop_report *d_rep = nullptr;
    if ((rc = covis_stage(m, &d_g, group_id, (size_t)n_group, (size_t)n_group)) || (rc = covis_stage(m, &d_b, lc_begin, (size_t)n_group + 1, (size_t)n_group + 1)) ||
        (rc = covis_stage(m, &d_j, lc_j, (size_t)lcap, (size_t)lcap)) || (rc = m.alloc(&d_vi, (size_t)h->max_kf)) || (rc = m.alloc(&d_vf, (size_t)h->max_kf)) ||
        (rc = m.alloc(&d_vg, (size_t)h->max_kf)) || (rc = m.alloc(&d_ei, (size_t)ecap)) || (rc = m.alloc(&d_ej, (size_t)ecap)) || (rc = m.alloc(&d_ek, (size_t)ecap)) ||
        (rc = m.alloc(&d_rep, 1))) return rc;
    if ((rc = sgx_covis_essential_graph_dev(h, cur, loop, n_group, d_g, lcap, d_b, d_j, d_vi, d_vf, d_vg, ecap, d_ei, d_ej, d_ek, d_rep, nullptr)) != SGX_OK) return rc;
    SGX_CHECK_HIP(hipStreamSynchronize((sgx_stream_t)0));
    sgx_covis_loop_report R;
    SGX_CHECK_HIP(hipMemcpy(&R, d_rep, sizeof(R), hipMemcpyDeviceToHost));
    if (report) *report = R;
    if (R.status == SGX_ERR_INVALID) return R.status;                              // nothing of the call was written
    const size_t nv = (size_t)R.n_vertices, ne = (size_t)std::min(R.n_edges, ecap);
    if (nv) { SGX_CHECK_HIP(hipMemcpy(vertex_id, d_vi, nv * 4, hipMemcpyDeviceToHost)); SGX_CHECK_HIP(hipMemcpy(vertex_fixed, d_vf, nv, hipMemcpyDeviceToHost));
              SGX_CHECK_HIP(hipMemcpy(vertex_group, d_vg, nv * 4, hipMemcpyDeviceToHost)); }
    if (ne) { SGX_CHECK_HIP(hipMemcpy(e_i, d_ei, ne * 4, hipMemcpyDeviceToHost)); SGX_CHECK_HIP(hipMemcpy(e_j, d_ej, ne * 4, hipMemcpyDeviceToHost));
              SGX_CHECK_HIP(hipMemcpy(e_kind, d_ek, ne, hipMemcpyDeviceToHost)); }
    return R.status;                                                               // SGX_OK, or SGX_ERR_NOMEM with the first ecap edges written
}

// ---- DetectLoop's consistency groups (sgx_covis_detect_kernels.h): mvConsistentGroups as device state, allocated on demand, and GetConnectedKeyFrames as a CSR
extern "C" int sgx_covis_consistency_reserve(sgx_covis *h, int max_groups)
{
    if (!h || max_groups < 1) return SGX_ERR_INVALID;
    if (max_groups > SGX_COVIS_MAX_GROUPS) return SGX_ERR_UNSUPPORTED;
    if (h->cg_G) return h->cg_G == max_groups ? SGX_OK : SGX_ERR_INVALID;         // the capacity is fixed by the first reservation; sgx_covis_clear drops it
    const size_t N = (size_t)h->max_kf, G = (size_t)max_groups;
    SgxDevMem m;                                                                  // all or nothing: the buffers move to the handle once every one is there
    int *st = nullptr, *cnt = nullptr, *size = nullptr, *mem = nullptr, *cvalid = nullptr, *nd_cand = nullptr, *nd_cnt = nullptr, *tmp = nullptr; unsigned char *flags = nullptr;
    int rc;
    if ((rc = m.alloc(&st, (size_t)CG_FIELDS)) || (rc = m.alloc(&cnt, 2 * G)) || (rc = m.alloc(&size, 2 * G)) || (rc = m.alloc(&mem, 2 * G * N)) || (rc = m.alloc(&cvalid, N)) ||
        (rc = m.alloc(&nd_cand, G)) || (rc = m.alloc(&nd_cnt, G)) || (rc = m.alloc(&tmp, N)) || (rc = m.alloc(&flags, N * G))) return rc;
    SGX_CHECK_HIP(hipMemset(st, 0, CG_FIELDS * 4));
    SGX_CHECK_HIP(hipStreamSynchronize((sgx_stream_t)0));
    h->mem.owned.insert(h->mem.owned.end(), m.owned.begin(), m.owned.end()); m.owned.clear();
    h->cg_st = st; h->cg_cnt = cnt; h->cg_size = size; h->cg_mem = mem; h->cg_cvalid = cvalid; h->cg_nd_cand = nd_cand; h->cg_nd_cnt = nd_cnt; h->cg_tmp = tmp; h->cg_flags = flags;
    h->cg_G = max_groups;
    h->cg_bytes = (int64_t)(G * (9 * N + 24) + 8 * N + 4 * CG_FIELDS);
    return SGX_OK;
}

extern "C" int sgx_covis_consistency_clear(sgx_covis *h)
{
    if (!h) return SGX_ERR_INVALID;
    if (!h->cg_G) return SGX_OK;
    SGX_CHECK_HIP(hipMemset(h->cg_st, 0, CG_FIELDS * 4));
    SGX_CHECK_HIP(hipStreamSynchronize((sgx_stream_t)0));
    return SGX_OK;
}

// the scalars of the groups as they stand (a blocking copy: the calls enqueued before it have run)
static int covis_cg_state(const sgx_covis *h, int32_t st[CG_FIELDS])
{
    for (int i = 0; i < CG_FIELDS; i++) st[i] = 0;
    if (h->cg_G) SGX_CHECK_HIP(hipMemcpy(st, h->cg_st, CG_FIELDS * 4, hipMemcpyDeviceToHost));
    return SGX_OK;
}

extern "C" int sgx_covis_consistency_info(const sgx_covis *h, int64_t *bytes, int32_t *n_groups, int32_t *max_groups)
{
    if (!h) return SGX_ERR_INVALID;
    int32_t st[CG_FIELDS];
    const int rc = covis_cg_state(h, st);
    if (rc != SGX_OK) return rc;
    if (bytes) *bytes = h->cg_bytes;
    if (n_groups) *n_groups = st[CG_N];
    if (max_groups) *max_groups = h->cg_G;
    return SGX_OK;
}

extern "C" int sgx_covis_get_consistent_groups(const sgx_covis *h, int32_t *n_groups, int32_t *counter, int32_t *off, int cap, int32_t *ids)
{
    if (!h || !n_groups || !off || cap < 0 || (cap > 0 && !ids)) return SGX_ERR_INVALID;
    int32_t st[CG_FIELDS];
    int rc = covis_cg_state(h, st);
    if (rc != SGX_OK) return rc;
    const size_t n = (size_t)st[CG_N], G = (size_t)h->cg_G, base = (size_t)st[CG_CUR] * G;
    if (n && !counter) return SGX_ERR_INVALID;
    std::vector<int32_t> size(n);
    if (n) {
        SGX_CHECK_HIP(hipMemcpy(counter, h->cg_cnt + base, n * 4, hipMemcpyDeviceToHost));
        SGX_CHECK_HIP(hipMemcpy(size.data(), h->cg_size + base, n * 4, hipMemcpyDeviceToHost));
    }
    *n_groups = (int32_t)n; off[0] = 0;
    for (size_t g = 0; g < n; g++) off[g + 1] = off[g] + size[g];
    rc = SGX_OK;
    for (size_t g = 0; g < n; g++) {                                              // the rows that fit wholly
        if (off[g + 1] > cap) { rc = SGX_ERR_NOMEM; break; }
        if (size[g]) SGX_CHECK_HIP(hipMemcpy(ids + off[g], h->cg_mem + (base + g) * (size_t)h->max_kf, (size_t)size[g] * 4, hipMemcpyDeviceToHost));
    }
    return rc;
}

extern "C" int sgx_covis_consistency_dev(sgx_covis *h, const int32_t *cand_dev, const int32_t *n_cand_dev, int th, int32_t *enough_dev, int32_t *n_enough_dev,
                                         sgx_covis_consistency_report *report_dev, void *stream)
{
    if (!h || !cand_dev || !n_cand_dev || !enough_dev || !n_enough_dev || !report_dev) return SGX_ERR_INVALID;
    int rc;
    if (!h->cg_G && (rc = sgx_covis_consistency_reserve(h, SGX_COVIS_DEFAULT_GROUPS)) != SGX_OK) return rc;
    if ((rc = covis_sync_tables(h)) != SGX_OK) return rc;
    const sgx_stream_t s = (sgx_stream_t)stream;
    SgxCovisArgs A = covis_args(h);
    SgxCovisCgArgs D{};
    D.G = h->cg_G; D.th = th; D.st = h->cg_st; D.cnt = h->cg_cnt; D.size = h->cg_size; D.mem = h->cg_mem; D.flags = h->cg_flags; D.cvalid = h->cg_cvalid;
    D.nd_cand = h->cg_nd_cand; D.nd_cnt = h->cg_nd_cnt; D.tmp_enough = h->cg_tmp; D.cand = cand_dev; D.n_cand = n_cand_dev; D.enough = enough_dev; D.n_enough = n_enough_dev;
    D.report = (SgxCovisCgReport *)report_dev;
    const unsigned G = (unsigned)std::max(1, std::min(h->max_kf, (int)COVIS_GRID));
    SGX_LAUNCH(k_covis_cg_match, dim3(G), dim3(256), s, A, D);
    SGX_LAUNCH(k_covis_cg_replay, dim3(1), dim3(64), s, A, D);
    SGX_LAUNCH(k_covis_cg_store, dim3((unsigned)std::min(h->cg_G, (int)COVIS_GRID)), dim3(256), s, A, D);
    SGX_CHECK_HIP(hipGetLastError());
    return SGX_OK;
}

extern "C" int sgx_covis_consistency(sgx_covis *h, int n_cand, const int32_t *cand, int th, int32_t *enough, int32_t *n_enough, sgx_covis_consistency_report *report)
{
    if (!h || n_cand < 0 || n_cand > h->max_kf || (n_cand > 0 && (!cand || !enough)) || !n_enough) return SGX_ERR_INVALID;
    SgxDevMem m; int rc;
    int32_t *d_c = nullptr, *d_n = nullptr, *d_e = nullptr, *d_ne = nullptr; sgx_covis_consistency_report *d_rep = nullptr;
    const int32_t n32 = n_cand;
    if ((rc = covis_stage(m, &d_c, cand, (size_t)n_cand, (size_t)n_cand)) || (rc = covis_stage(m, &d_n, &n32, 1, 1)) || (rc = m.alloc(&d_e, (size_t)h->max_kf)) ||
        (rc = m.alloc(&d_ne, 1)) || (rc = m.alloc(&d_rep, 1))) return rc;
    if ((rc = sgx_covis_consistency_dev(h, d_c, d_n, th, d_e, d_ne, d_rep, nullptr)) != SGX_OK) return rc;
    SGX_CHECK_HIP(hipStreamSynchronize((sgx_stream_t)0));
    sgx_covis_consistency_report R;
    SGX_CHECK_HIP(hipMemcpy(&R, d_rep, sizeof(R), hipMemcpyDeviceToHost));
    if (report) *report = R;
    if (R.status != SGX_OK) return R.status;                                      // rule 13: nothing was written
    if (R.n_enough) SGX_CHECK_HIP(hipMemcpy(enough, d_e, (size_t)R.n_enough * 4, hipMemcpyDeviceToHost));
    *n_enough = R.n_enough;
    return SGX_OK;
}

extern "C" int sgx_covis_connected_batch_dev(sgx_covis *h, int Q, const int32_t *kf_ids_dev, int32_t *off_dev, int32_t *ids_dev, int cap, sgx_covis_report *report_dev, void *stream)
{
    if (!h || Q < 0 || Q > h->max_q || cap < 0) return SGX_ERR_INVALID;
    if (Q == 0) return SGX_OK;
    if (!kf_ids_dev || !off_dev || (cap > 0 && !ids_dev) || !report_dev) return SGX_ERR_INVALID;
    const int rc = covis_sync_tables(h);
    if (rc != SGX_OK) return rc;
    const sgx_stream_t s = (sgx_stream_t)stream;
    SgxCovisArgs A = covis_args(h);
    A.Q = Q; A.q_kf = kf_ids_dev; A.report = (SgxCovisReport *)report_dev;
    SGX_LAUNCH(k_covis_conn_count, dim3((unsigned)Q), dim3(256), s, A);
    SGX_LAUNCH(k_covis_conn_emit, dim3((unsigned)Q), dim3(256), s, A, off_dev, ids_dev, cap);
    SGX_CHECK_HIP(hipGetLastError());
    return SGX_OK;
}

extern "C" int sgx_covis_connected_batch(sgx_covis *h, int Q, const int32_t *kf_ids, int32_t *off, int32_t *ids, int cap, sgx_covis_report *report)
{
    if (!h || Q < 1 || Q > h->max_q || !kf_ids || !off || cap < 0 || (cap > 0 && !ids)) return SGX_ERR_INVALID;
    SgxDevMem m; int rc;
    int32_t *d_k = nullptr, *d_o = nullptr, *d_i = nullptr; sgx_covis_report *d_rep = nullptr;
    if ((rc = covis_stage(m, &d_k, kf_ids, (size_t)Q, (size_t)Q)) || (rc = m.alloc(&d_o, (size_t)Q + 1)) || (rc = m.alloc(&d_i, (size_t)cap)) || (rc = m.alloc(&d_rep, (size_t)Q))) return rc;
    if ((rc = sgx_covis_connected_batch_dev(h, Q, d_k, d_o, d_i, cap, d_rep, nullptr)) != SGX_OK) return rc;
    SGX_CHECK_HIP(hipStreamSynchronize((sgx_stream_t)0));
    std::vector<sgx_covis_report> R((size_t)Q);
    SGX_CHECK_HIP(hipMemcpy(R.data(), d_rep, R.size() * sizeof(sgx_covis_report), hipMemcpyDeviceToHost));
    SGX_CHECK_HIP(hipMemcpy(off, d_o, ((size_t)Q + 1) * 4, hipMemcpyDeviceToHost));
    rc = SGX_OK;
    for (int q = 0; q < Q; q++) {
        if (report) report[q] = R[(size_t)q];
        if (R[(size_t)q].status != SGX_OK) { if (rc == SGX_OK) rc = R[(size_t)q].status; continue; }
        if (off[q + 1] > off[q]) SGX_CHECK_HIP(hipMemcpy(ids + off[q], d_i + off[q], (size_t)(off[q + 1] - off[q]) * 4, hipMemcpyDeviceToHost));
    }
    return rc;                                                                    // SGX_OK, or the first query status that is not
}

// ---- RunGlobalBundleAdjustment's map update (sgx_covis_gba_kernels.h)
extern "C" int sgx_covis_gba_update_dev(sgx_covis *h, int n_origins, const int32_t *origins_dev, int nk, const int32_t *kf_ids_dev, const uint8_t *in_gba_dev, const float *Tcw_dev,
                                        const float *TcwGBA_dev, float *Tcw_out_dev, float *TcwBef_dev, uint8_t *kf_state_dev, sgx_covis_gba_report *report_dev, void *stream)
{
    if (!h || n_origins < 1 || n_origins > h->max_kf || !origins_dev || nk < 1 || nk > h->max_kf || !kf_ids_dev || !in_gba_dev || !Tcw_dev || !TcwGBA_dev || !Tcw_out_dev ||
        !TcwBef_dev || !kf_state_dev || !report_dev || Tcw_out_dev == Tcw_dev) return SGX_ERR_INVALID;
    const size_t N = (size_t)h->max_kf;
    int rc;
    if (!h->gb_gs) {
        SgxDevMem m;                                                              // all or nothing
        int *a = nullptr, *b = nullptr, *c = nullptr, *d = nullptr, *e = nullptr;
        if ((rc = m.alloc(&a, N)) || (rc = m.alloc(&b, N)) || (rc = m.alloc(&c, N)) || (rc = m.alloc(&d, N)) || (rc = m.alloc(&e, (size_t)GS_FIELDS))) return rc;
        h->mem.owned.insert(h->mem.owned.end(), m.owned.begin(), m.owned.end()); m.owned.clear();
        h->gb_row_of = a; h->gb_orig = b; h->gb_level = c; h->gb_prow = d; h->gb_gs = e;
    }
    if ((rc = covis_sync_tables(h)) != SGX_OK) return rc;
    const sgx_stream_t s = (sgx_stream_t)stream;
    SgxCovisArgs A = covis_args(h);
    SgxCovisGbaArgs B{};
    B.n_origins = n_origins; B.nk = nk; B.origins = origins_dev; B.kf_ids = kf_ids_dev; B.in_gba = in_gba_dev; B.Tcw = Tcw_dev; B.TcwGBA = TcwGBA_dev; B.Tcw_out = Tcw_out_dev;
    B.TcwBef = TcwBef_dev; B.kf_state = kf_state_dev; B.report = (SgxCovisGbaReport *)report_dev;
    B.row_of = h->gb_row_of; B.orig = h->gb_orig; B.level = h->gb_level; B.prow = h->gb_prow; B.gs = h->gb_gs;
    SGX_LAUNCH(k_covis_gba_begin, dim3(1), dim3(256), s, A, B);
    SGX_LAUNCH(k_covis_gba_depth, dim3((unsigned)((nk + 255) / 256)), dim3(256), s, A, B);
    SGX_LAUNCH(k_covis_gba_levels, dim3(1), dim3(256), s, A, B);
    SGX_CHECK_HIP(hipGetLastError());
    return SGX_OK;
}

extern "C" int sgx_gba_correct_points_dev(int n, const float *xw_dev, const uint8_t *in_gba_dev, const float *xw_gba_dev, const int32_t *ref_dev, const uint8_t *kf_state_dev,
                                          const float *TcwBef_dev, const float *Tcw_out_dev, float *xw_out_dev, void *stream)
{
    if (n < 0) return SGX_ERR_INVALID;
    if (n == 0) return SGX_OK;
    if (!xw_dev || !in_gba_dev || !xw_gba_dev || !ref_dev || !kf_state_dev || !TcwBef_dev || !Tcw_out_dev || !xw_out_dev) return SGX_ERR_INVALID;
    SGX_LAUNCH(k_gba_correct_points, dim3((unsigned)((n + 255) / 256)), dim3(256), (sgx_stream_t)stream, n, xw_dev, in_gba_dev, xw_gba_dev, ref_dev, kf_state_dev, TcwBef_dev,
               Tcw_out_dev, xw_out_dev);
    SGX_CHECK_HIP(hipGetLastError());
    return SGX_OK;
}

extern "C" int sgx_covis_gba_update(sgx_covis *h, int n_origins, const int32_t *origins, int nk, const int32_t *kf_ids, const uint8_t *in_gba, const float *Tcw, const float *TcwGBA,
                                    float *Tcw_out, float *TcwBef, uint8_t *kf_state, sgx_covis_gba_report *report)
{
    if (!h || n_origins < 1 || n_origins > h->max_kf || !origins || nk < 1 || nk > h->max_kf || !kf_ids || !in_gba || !Tcw || !TcwGBA || !Tcw_out || !TcwBef || !kf_state) return SGX_ERR_INVALID;
    SgxDevMem m; int rc;
    const size_t K = (size_t)nk;
    int32_t *d_o = nullptr, *d_k = nullptr; uint8_t *d_g = nullptr, *d_s = nullptr; float *d_T = nullptr, *d_G = nullptr, *d_O = nullptr, *d_B = nullptr; sgx_covis_gba_report *d_rep = nullptr;
    if ((rc = covis_stage(m, &d_o, origins, (size_t)n_origins, (size_t)n_origins)) || (rc = covis_stage(m, &d_k, kf_ids, K, K)) || (rc = covis_stage(m, &d_g, in_gba, K, K)) ||
        (rc = covis_stage(m, &d_T, Tcw, 12 * K, 12 * K)) || (rc = covis_stage(m, &d_G, TcwGBA, 12 * K, 12 * K)) || (rc = m.alloc(&d_O, 12 * K)) || (rc = m.alloc(&d_B, 12 * K)) ||
        (rc = m.alloc(&d_s, K)) || (rc = m.alloc(&d_rep, 1))) return rc;
    SGX_CHECK_HIP(hipMemcpy(d_B, TcwBef, 12 * K * 4, hipMemcpyHostToDevice));     // a row of a keyframe that is not visited stays the caller's
    if ((rc = sgx_covis_gba_update_dev(h, n_origins, d_o, nk, d_k, d_g, d_T, d_G, d_O, d_B, d_s, d_rep, nullptr)) != SGX_OK) return rc;
    SGX_CHECK_HIP(hipStreamSynchronize((sgx_stream_t)0));
    sgx_covis_gba_report R;
    SGX_CHECK_HIP(hipMemcpy(&R, d_rep, sizeof(R), hipMemcpyDeviceToHost));
    if (report) *report = R;
    if (R.status != SGX_OK) return R.status;                                      // nothing was written
    SGX_CHECK_HIP(hipMemcpy(Tcw_out, d_O, 12 * K * 4, hipMemcpyDeviceToHost));
    SGX_CHECK_HIP(hipMemcpy(TcwBef, d_B, 12 * K * 4, hipMemcpyDeviceToHost));
    SGX_CHECK_HIP(hipMemcpy(kf_state, d_s, K, hipMemcpyDeviceToHost));
    return SGX_OK;
}

extern "C" int sgx_gba_correct_points(int n, const float *xw, const uint8_t *in_gba, const float *xw_gba, const int32_t *ref, int nk, const uint8_t *kf_state, const float *TcwBef,
                                      const float *Tcw_out, float *xw_out)
{
    if (n < 0 || nk < 0) return SGX_ERR_INVALID;
    if (n == 0) return SGX_OK;
    if (!xw || !in_gba || !xw_gba || !ref || !xw_out || (nk > 0 && (!kf_state || !TcwBef || !Tcw_out))) return SGX_ERR_INVALID;
    for (int i = 0; i < n; i++) if (ref[i] < -1 || ref[i] >= nk) return SGX_ERR_INVALID;      // the host form checks the rows the device form trusts
    SgxDevMem m; int rc;
    const size_t P = (size_t)n, K = (size_t)nk;
    float *d_x = nullptr, *d_g = nullptr, *d_B = nullptr, *d_O = nullptr, *d_y = nullptr; uint8_t *d_f = nullptr, *d_s = nullptr; int32_t *d_r = nullptr;
    if ((rc = covis_stage(m, &d_x, xw, 3 * P, 3 * P)) || (rc = covis_stage(m, &d_f, in_gba, P, P)) || (rc = covis_stage(m, &d_g, xw_gba, 3 * P, 3 * P)) || (rc = covis_stage(m, &d_r, ref, P, P)) ||
        (rc = covis_stage(m, &d_s, kf_state, K, K)) || (rc = covis_stage(m, &d_B, TcwBef, 12 * K, 12 * K)) || (rc = covis_stage(m, &d_O, Tcw_out, 12 * K, 12 * K)) ||
        (rc = m.alloc(&d_y, 3 * P))) return rc;
    if ((rc = sgx_gba_correct_points_dev(n, d_x, d_f, d_g, d_r, d_s, d_B, d_O, d_y, nullptr)) != SGX_OK) return rc;
    SGX_CHECK_HIP(hipStreamSynchronize((sgx_stream_t)0));
    SGX_CHECK_HIP(hipMemcpy(xw_out, d_y, 3 * P * 4, hipMemcpyDeviceToHost));
    return SGX_OK;
}
