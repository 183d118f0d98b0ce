// sgx_kfdb.cpp — KeyFrameDatabase (src/sg-slam/src/KeyFrameDatabase.cc) behind the C ABI: the forward file and the per-keyframe state on the device, add / erase / clear
// (:40-73) as host bookkeeping over it, and the two queries (:76-197, :199-309) as the launch sequence of sgx_kfdb_kernels.h; sgx_voc_bow_batch_dev, the BowVector a query
// is made of, sits in sgx_voc.cpp beside the transform it completes.
#include "sgx_kfdb_kernels.h"
#include "sgx_devmem.h"
#include "../../include/sgx.h"
#ifdef SGX_DEBUG_TAPS
#include "../../include/sgx_debug.h"      // test / tuning taps: compiled into tests/taps/libsgx_taps.so and the emulator only
#endif
#include <math.h>
#include <cmath>
#include <stdio.h>
#include <string.h>
#include <algorithm>
#include <map>
#include <vector>

static_assert(sizeof(sgx_kfdb_report) == sizeof(SgxKfdbReport), "the kernels write sgx_kfdb_report records");

struct sgx_kfdb {
    int nwords = 0, max_kf = 0, max_ent = 0, max_qw = 0, max_q = 0;
    // host bookkeeping: slot s holds keyframe kf_id[s] (-1 = free); the entries of the live keyframes occupy [0, top) of the pool, with holes where keyframes were erased
    struct Slot { std::vector<int32_t> ids; std::vector<double> w; std::vector<int32_t> covis; };
    std::vector<Slot> slot;
    std::vector<int32_t> kf_id, off, cnt, seq;
    std::vector<int> free_slots;                  // free slots, lowest last
    std::map<int32_t, int> by_id;                 // caller id -> slot, ascending: the device's lookup table is this map written out
    int nslots = 0, top = 0, live_ent = 0, next_seq = 0;
    bool tables_dirty = true;
    // device
    int *d_ent_id = nullptr; double *d_ent_w = nullptr;
    int *d_off = nullptr, *d_cnt = nullptr, *d_seq = nullptr, *d_kf_id = nullptr, *d_covis = nullptr, *d_sorted_id = nullptr, *d_sorted_slot = nullptr;
    float *d_reloc = nullptr;
    unsigned char *d_conn = nullptr;
    int *d_words = nullptr, *d_first = nullptr, *d_order = nullptr, *d_best = nullptr, *d_firstrank = nullptr; float *d_score = nullptr, *d_acc = nullptr;
    unsigned long long *d_key = nullptr;
    // staging of the single-query entries
    int *s_ids = nullptr, *s_cnt = nullptr, *s_conn_off = nullptr, *s_conn = nullptr, *s_cand = nullptr, *s_ncand = nullptr, *s_slots = nullptr;
    double *s_w = nullptr; float *s_min = nullptr; SgxKfdbReport *s_report = nullptr;
    SgxDevMem mem;
};

extern "C" int sgx_kfdb_create(const sgx_voc *voc, int max_keyframes, int max_bow_entries, int max_query_words, int max_queries, sgx_kfdb **out)
{
    if (out) *out = nullptr;
    if (!out || !voc || max_keyframes < 1 || max_bow_entries < 1 || max_query_words < 0 || max_queries < 1) return SGX_ERR_INVALID;
    int32_t scoring = 0, nwords = 0;
    if (sgx_voc_info(voc, nullptr, nullptr, &scoring, nullptr, nullptr, &nwords) != SGX_OK) return SGX_ERR_INVALID;
    if (scoring != 0) return SGX_ERR_UNSUPPORTED;                 // L1Scoring only, as sgx_voc_score
    if (max_query_words == 0) max_query_words = 2048;             // 24 KB of LDS
    if (max_query_words > 4096) return SGX_ERR_UNSUPPORTED;       // the query sits in LDS: 12 bytes a word
    sgx_kfdb *h = new sgx_kfdb;
    h->nwords = nwords; h->max_kf = max_keyframes; h->max_ent = max_bow_entries; h->max_qw = max_query_words; h->max_q = max_queries;
    const size_t N = (size_t)max_keyframes, QN = N * (size_t)max_queries;
    h->slot.resize(N); h->kf_id.assign(N, -1); h->off.assign(N, 0); h->cnt.assign(N, 0); h->seq.assign(N, 0);
    SgxDevMem &m = h->mem;
    int rc;
    if ((rc = m.alloc(&h->d_ent_id, (size_t)max_bow_entries)) || (rc = m.alloc(&h->d_ent_w, (size_t)max_bow_entries)) || (rc = m.alloc(&h->d_off, N)) || (rc = m.alloc(&h->d_cnt, N)) ||
        (rc = m.alloc(&h->d_seq, N)) || (rc = m.alloc(&h->d_kf_id, N)) || (rc = m.alloc(&h->d_covis, N * SGX_KFDB_COVIS)) || (rc = m.alloc(&h->d_sorted_id, N)) ||
        (rc = m.alloc(&h->d_sorted_slot, N)) || (rc = m.alloc(&h->d_reloc, N)) || (rc = m.alloc(&h->d_conn, QN)) || (rc = m.alloc(&h->d_words, QN)) || (rc = m.alloc(&h->d_first, QN)) ||
        (rc = m.alloc(&h->d_order, QN)) || (rc = m.alloc(&h->d_best, QN)) || (rc = m.alloc(&h->d_firstrank, QN)) || (rc = m.alloc(&h->d_score, QN)) || (rc = m.alloc(&h->d_acc, QN)) ||
        (rc = m.alloc(&h->d_key, QN)) || (rc = m.alloc(&h->s_ids, (size_t)max_query_words)) || (rc = m.alloc(&h->s_w, (size_t)max_query_words)) || (rc = m.alloc(&h->s_cnt, 1)) ||
        (rc = m.alloc(&h->s_conn_off, 2)) || (rc = m.alloc(&h->s_conn, N)) || (rc = m.alloc(&h->s_cand, N)) || (rc = m.alloc(&h->s_ncand, 1)) || (rc = m.alloc(&h->s_slots, N)) ||
        (rc = m.alloc(&h->s_min, 1)) || (rc = m.alloc(&h->s_report, 1))) { delete h; return rc; }
    if (hipMemset(h->d_reloc, 0, N * sizeof(float)) != hipSuccess) { delete h; return SGX_ERR_DEVICE; }
    for (int s = max_keyframes - 1; s >= 0; s--) h->free_slots.push_back(s);
    *out = h;
    return SGX_OK;
}

extern "C" void sgx_kfdb_destroy(sgx_kfdb *db) { delete db; }

extern "C" int sgx_kfdb_size(const sgx_kfdb *db) { return db ? (int)db->by_id.size() : SGX_ERR_INVALID; }

// a BowVector as the database takes it: ids strictly ascending and below nwords, weights finite
static bool kfdb_bow_ok(const sgx_kfdb *db, int n, const int32_t *ids, const double *w)
{
    if (n < 0 || (n > 0 && (!ids || !w))) return false;
    for (int i = 0; i < n; i++) if (ids[i] < 0 || ids[i] >= db->nwords || (i > 0 && ids[i] <= ids[i - 1]) || !std::isfinite(w[i])) return false;
    return true;
}

// the pool without its holes: every live keyframe's entries again, in slot order, from the host copies
static int kfdb_compact(sgx_kfdb *db)
{
    std::vector<int32_t> ids((size_t)db->live_ent); std::vector<double> w((size_t)db->live_ent);
    int top = 0;
    for (int s = 0; s < db->nslots; s++) {
        if (db->kf_id[(size_t)s] < 0) continue;
        const sgx_kfdb::Slot &S = db->slot[(size_t)s];
        db->off[(size_t)s] = top;
        if (!S.ids.empty()) { memcpy(&ids[(size_t)top], S.ids.data(), S.ids.size() * 4); memcpy(&w[(size_t)top], S.w.data(), S.w.size() * 8); }
        top += (int)S.ids.size();
    }
    if (top) {
        SGX_CHECK_HIP(hipMemcpy(db->d_ent_id, ids.data(), (size_t)top * 4, hipMemcpyHostToDevice));
        SGX_CHECK_HIP(hipMemcpy(db->d_ent_w, w.data(), (size_t)top * 8, hipMemcpyHostToDevice));
    }
    db->top = top; db->tables_dirty = true;
    return SGX_OK;
}

extern "C" int sgx_kfdb_add(sgx_kfdb *db, int32_t kf_id, int nbow, const int32_t *ids, const double *weights)
{
    if (!db || kf_id < 0 || !kfdb_bow_ok(db, nbow, ids, weights) || db->by_id.count(kf_id)) return SGX_ERR_INVALID;
    if (db->free_slots.empty() || db->live_ent + nbow > db->max_ent) return SGX_ERR_NOMEM;
    if (db->top + nbow > db->max_ent) { const int rc = kfdb_compact(db); if (rc != SGX_OK) return rc; }      // erased keyframes give their entries back here
    const int s = db->free_slots.back();
    if (nbow) {
        SGX_CHECK_HIP(hipMemcpy(db->d_ent_id + db->top, ids, (size_t)nbow * 4, hipMemcpyHostToDevice));
        SGX_CHECK_HIP(hipMemcpy(db->d_ent_w + db->top, weights, (size_t)nbow * 8, hipMemcpyHostToDevice));
    }
    db->free_slots.pop_back();
    sgx_kfdb::Slot &S = db->slot[(size_t)s];
    S.ids.assign(ids, ids + nbow); S.w.assign(weights, weights + nbow); S.covis.clear();
    db->kf_id[(size_t)s] = kf_id; db->off[(size_t)s] = db->top; db->cnt[(size_t)s] = nbow; db->seq[(size_t)s] = db->next_seq++;
    db->top += nbow; db->live_ent += nbow;
    if (s + 1 > db->nslots) db->nslots = s + 1;
    db->by_id[kf_id] = s; db->tables_dirty = true;
    return SGX_OK;
}

extern "C" int sgx_kfdb_erase(sgx_kfdb *db, int32_t kf_id)
{
    if (!db) return SGX_ERR_INVALID;
    const auto it = db->by_id.find(kf_id);
    if (it == db->by_id.end()) return SGX_ERR_INVALID;
    const int s = it->second;
    SGX_CHECK_HIP(hipMemset(db->d_reloc + s, 0, sizeof(float)));                                            // the slot's next keyframe is one no query has scored: mRelocScore 0
    sgx_kfdb::Slot &S = db->slot[(size_t)s];
    db->live_ent -= db->cnt[(size_t)s];
    if (db->off[(size_t)s] + db->cnt[(size_t)s] == db->top) db->top = db->off[(size_t)s];                   // the last keyframe of the pool: no hole
    S = sgx_kfdb::Slot();
    db->kf_id[(size_t)s] = -1; db->cnt[(size_t)s] = 0; db->off[(size_t)s] = 0;
    db->by_id.erase(it);
    db->free_slots.insert(std::lower_bound(db->free_slots.begin(), db->free_slots.end(), s, [](int a, int b) { return a > b; }), s);
    while (db->nslots > 0 && db->kf_id[(size_t)db->nslots - 1] < 0) db->nslots--;
    if (db->by_id.empty()) db->top = 0;
    db->tables_dirty = true;
    return SGX_OK;
}

extern "C" int sgx_kfdb_clear(sgx_kfdb *db)
{
    if (!db) return SGX_ERR_INVALID;
    SGX_CHECK_HIP(hipMemset(db->d_reloc, 0, (size_t)db->max_kf * sizeof(float)));
    for (int s = 0; s < db->max_kf; s++) db->slot[(size_t)s] = sgx_kfdb::Slot();
    std::fill(db->kf_id.begin(), db->kf_id.end(), -1); std::fill(db->cnt.begin(), db->cnt.end(), 0); std::fill(db->off.begin(), db->off.end(), 0);
    db->free_slots.clear();
    for (int s = db->max_kf - 1; s >= 0; s--) db->free_slots.push_back(s);
    db->by_id.clear(); db->nslots = 0; db->top = 0; db->live_ent = 0; db->next_seq = 0; db->tables_dirty = true;
    return SGX_OK;
}

extern "C" int sgx_kfdb_set_covisibility(sgx_kfdb *db, int32_t kf_id, int n, const int32_t *neighbour_ids)
{
    if (!db || n < 0 || n > SGX_KFDB_COVIS || (n > 0 && !neighbour_ids)) return SGX_ERR_INVALID;
    const auto it = db->by_id.find(kf_id);
    if (it == db->by_id.end()) return SGX_ERR_INVALID;
    db->slot[(size_t)it->second].covis.assign(neighbour_ids, neighbour_ids + n);
    db->tables_dirty = true;
    return SGX_OK;
}

extern "C" int sgx_kfdb_slots(const sgx_kfdb *db, int32_t *kf_ids, int32_t *n_slots)
{
    if (!db || !kf_ids || !n_slots) return SGX_ERR_INVALID;
    memcpy(kf_ids, db->kf_id.data(), (size_t)db->max_kf * 4);
    *n_slots = db->nslots;
    return SGX_OK;
}

// the per-slot tables as the kernels read them, after any change of the database: neighbours resolved to slots (an id that is not in the database: -1), ids sorted
static int kfdb_sync_tables(sgx_kfdb *db)
{
    if (!db->tables_dirty) return SGX_OK;
    const size_t n = (size_t)db->nslots;
    std::vector<int32_t> covis(n * SGX_KFDB_COVIS + 1, -1), sid, sslot;
    for (size_t s = 0; s < n; s++) {
        const std::vector<int32_t> &c = db->slot[s].covis;
        for (size_t j = 0; j < c.size(); j++) { const auto it = db->by_id.find(c[j]); if (it != db->by_id.end()) covis[s * SGX_KFDB_COVIS + j] = it->second; }
    }
    for (const auto &e : db->by_id) { sid.push_back(e.first); sslot.push_back(e.second); }
    if (n) {
        SGX_CHECK_HIP(hipMemcpy(db->d_off, db->off.data(), n * 4, hipMemcpyHostToDevice));
        SGX_CHECK_HIP(hipMemcpy(db->d_cnt, db->cnt.data(), n * 4, hipMemcpyHostToDevice));
        SGX_CHECK_HIP(hipMemcpy(db->d_seq, db->seq.data(), n * 4, hipMemcpyHostToDevice));
        SGX_CHECK_HIP(hipMemcpy(db->d_kf_id, db->kf_id.data(), n * 4, hipMemcpyHostToDevice));
        SGX_CHECK_HIP(hipMemcpy(db->d_covis, covis.data(), n * SGX_KFDB_COVIS * 4, hipMemcpyHostToDevice));
        SGX_CHECK_HIP(hipMemcpy(db->d_sorted_id, sid.data(), sid.size() * 4, hipMemcpyHostToDevice));
        SGX_CHECK_HIP(hipMemcpy(db->d_sorted_slot, sslot.data(), sslot.size() * 4, hipMemcpyHostToDevice));
    }
    db->tables_dirty = false;
    return SGX_OK;
}

static SgxKfdbArgs kfdb_args(sgx_kfdb *db)
{
    SgxKfdbArgs A{};
    A.nslots = db->nslots; A.max_kf = db->max_kf; A.max_qw = db->max_qw; A.nlive = (int)db->by_id.size();
    A.ent_id = db->d_ent_id; A.ent_w = db->d_ent_w; A.off = db->d_off; A.cnt = db->d_cnt; A.seq = db->d_seq; A.kf_id = db->d_kf_id; A.covis = db->d_covis;
    A.sorted_id = db->d_sorted_id; A.sorted_slot = db->d_sorted_slot; A.reloc = db->d_reloc;
    A.conn = db->d_conn; A.words = db->d_words; A.first = db->d_first; A.score = db->d_score; A.key = db->d_key;
    A.order = db->d_order; A.best = db->d_best; A.firstrank = db->d_firstrank; A.acc = db->d_acc;
    return A;
}

static size_t kfdb_query_lds(const sgx_kfdb *db) { return (size_t)db->max_qw * 12; }

extern "C" int sgx_kfdb_detect_batch_dev(sgx_kfdb *db, int mode, int Q, const int32_t *ids_dev, const double *weights_dev, int pitch, const int32_t *counts_dev,
                                         const int32_t *conn_offsets_dev, const int32_t *conn_ids_dev, const float *min_score_dev,
                                         int32_t *cand_dev, int32_t *n_cand_dev, sgx_kfdb_report *report_dev, int32_t *words_dev, float *score_dev, void *stream)
{
    if (!db || (mode != SGX_KFDB_RELOC && mode != SGX_KFDB_LOOP) || Q < 0 || Q > db->max_q || pitch < 0) return SGX_ERR_INVALID;
    if (Q == 0) return SGX_OK;
    if (!ids_dev || !weights_dev || !counts_dev || !cand_dev || !n_cand_dev || !report_dev) return SGX_ERR_INVALID;
    if (mode == SGX_KFDB_LOOP && (!conn_offsets_dev || !conn_ids_dev || !min_score_dev)) return SGX_ERR_INVALID;
    int rc = kfdb_sync_tables(db);
    if (rc != SGX_OK) return rc;
    const sgx_stream_t s = (sgx_stream_t)stream;
    SgxKfdbArgs A = kfdb_args(db);
    A.mode = mode; A.Q = Q; A.q_pitch = pitch; A.q_ids = ids_dev; A.q_w = weights_dev; A.q_cnt = counts_dev;
    A.conn_off = conn_offsets_dev; A.conn_ids = conn_ids_dev; A.min_score = min_score_dev;
    A.cand = cand_dev; A.n_cand = n_cand_dev; A.report = (SgxKfdbReport *)report_dev;
    if (words_dev) A.words = words_dev;                           // the caller's arrays take the place of the workspace: Q x max_keyframes, by slot
    if (score_dev) A.score = score_dev;
    const size_t QN = (size_t)Q * db->max_kf;
    if (words_dev) SGX_CHECK_HIP(hipMemsetAsync(words_dev, 0, QN * 4, s));          // slots past the last keyframe read as untouched
    if (score_dev) SGX_CHECK_HIP(hipMemsetAsync(score_dev, 0, QN * 4, s));
    if (mode == SGX_KFDB_LOOP) {
        SGX_CHECK_HIP(hipMemsetAsync(db->d_conn, 0, QN, s));
        if (A.nlive) SGX_LAUNCH(k_kfdb_connected, dim3((unsigned)Q), dim3(256), s, A);
    }
    if (A.nslots) SGX_LAUNCH_DYN(k_kfdb_pairs, dim3((unsigned)((A.nslots + SGX_KFDB_TILE - 1) / SGX_KFDB_TILE), (unsigned)Q), dim3(256), kfdb_query_lds(db), s, A);
    SGX_LAUNCH(k_kfdb_gate, dim3((unsigned)Q), dim3(256), s, A);
    if (mode == SGX_KFDB_RELOC && A.nslots) SGX_LAUNCH(k_kfdb_stale, dim3((unsigned)((A.nslots + 255) / 256)), dim3(256), s, A);
    SGX_LAUNCH(k_kfdb_select, dim3((unsigned)Q), dim3(256), s, A);
    SGX_CHECK_HIP(hipGetLastError());
    return SGX_OK;
}

// one query from host memory through the batch entry: staged into the handle's buffers, run on the legacy stream, read back
static int kfdb_detect_one(sgx_kfdb *db, int mode, int nbow, const int32_t *ids, const double *weights, int n_connected, const int32_t *connected_ids, float min_score,
                           int32_t *cand, int32_t *n_cand, sgx_kfdb_report *report)
{
    if (!db || !n_cand || !kfdb_bow_ok(db, nbow, ids, weights) || nbow > db->max_qw || n_connected < 0 || (n_connected > 0 && !connected_ids)) return SGX_ERR_INVALID;
    *n_cand = 0;
    if (nbow) {
        SGX_CHECK_HIP(hipMemcpy(db->s_ids, ids, (size_t)nbow * 4, hipMemcpyHostToDevice));
        SGX_CHECK_HIP(hipMemcpy(db->s_w, weights, (size_t)nbow * 8, hipMemcpyHostToDevice));
    }
    SGX_CHECK_HIP(hipMemcpy(db->s_cnt, &nbow, 4, hipMemcpyHostToDevice));
    if (mode == SGX_KFDB_LOOP) {
        // only the connected keyframes that are in the database matter, and those are at most max_keyframes
        std::vector<int32_t> c;
        for (int i = 0; i < n_connected; i++) if (db->by_id.count(connected_ids[i])) c.push_back(connected_ids[i]);
        std::sort(c.begin(), c.end()); c.erase(std::unique(c.begin(), c.end()), c.end());
        const int32_t co[2] = { 0, (int32_t)c.size() };
        SGX_CHECK_HIP(hipMemcpy(db->s_conn_off, co, 8, hipMemcpyHostToDevice));
        if (!c.empty()) SGX_CHECK_HIP(hipMemcpy(db->s_conn, c.data(), c.size() * 4, hipMemcpyHostToDevice));
        SGX_CHECK_HIP(hipMemcpy(db->s_min, &min_score, 4, hipMemcpyHostToDevice));
    }
    const int rc = sgx_kfdb_detect_batch_dev(db, mode, 1, db->s_ids, db->s_w, db->max_qw, db->s_cnt, db->s_conn_off, db->s_conn, db->s_min, db->s_cand, db->s_ncand,
                                             (sgx_kfdb_report *)db->s_report, nullptr, nullptr, nullptr);
    if (rc != SGX_OK) return rc;
    SgxKfdbReport R;
    SGX_CHECK_HIP(hipMemcpy(&R, db->s_report, sizeof(R), hipMemcpyDeviceToHost));
    if (R.n_candidates > 0) {
        if (!cand) return SGX_ERR_INVALID;
        SGX_CHECK_HIP(hipMemcpy(cand, db->s_cand, (size_t)R.n_candidates * 4, hipMemcpyDeviceToHost));
    }
    *n_cand = R.n_candidates;
    if (report) memcpy(report, &R, sizeof(R));
    return SGX_OK;
}

extern "C" int sgx_kfdb_detect_relocalization_candidates(sgx_kfdb *db, int nbow, const int32_t *ids, const double *weights, int32_t *cand, int32_t *n_cand, sgx_kfdb_report *report)
{
    return kfdb_detect_one(db, SGX_KFDB_RELOC, nbow, ids, weights, 0, nullptr, 0.0f, cand, n_cand, report);
}

extern "C" int sgx_kfdb_detect_loop_candidates(sgx_kfdb *db, int nbow, const int32_t *ids, const double *weights, int n_connected, const int32_t *connected_ids, float min_score,
                                               int32_t *cand, int32_t *n_cand, sgx_kfdb_report *report)
{
    return kfdb_detect_one(db, SGX_KFDB_LOOP, nbow, ids, weights, n_connected, connected_ids, min_score, cand, n_cand, report);
}

extern "C" int sgx_kfdb_min_score(sgx_kfdb *db, int nbow, const int32_t *ids, const double *weights, int n, const int32_t *kf_ids, float *min_score)
{
    if (!db || !min_score || !kfdb_bow_ok(db, nbow, ids, weights) || nbow > db->max_qw || n < 0 || (n > 0 && !kf_ids)) return SGX_ERR_INVALID;
    *min_score = 1.0f;
    std::vector<int32_t> slots;                                   // a keyframe is scored as often as it is listed; the minimum does not care, the buffer does
    for (int i = 0; i < n; i++) { const auto it = db->by_id.find(kf_ids[i]); if (it != db->by_id.end()) slots.push_back(it->second); }
    std::sort(slots.begin(), slots.end()); slots.erase(std::unique(slots.begin(), slots.end()), slots.end());
    if (slots.empty()) return SGX_OK;
    int rc = kfdb_sync_tables(db);
    if (rc != SGX_OK) return rc;
    if (nbow) {
        SGX_CHECK_HIP(hipMemcpy(db->s_ids, ids, (size_t)nbow * 4, hipMemcpyHostToDevice));
        SGX_CHECK_HIP(hipMemcpy(db->s_w, weights, (size_t)nbow * 8, hipMemcpyHostToDevice));
    }
    SGX_CHECK_HIP(hipMemcpy(db->s_cnt, &nbow, 4, hipMemcpyHostToDevice));
    SGX_CHECK_HIP(hipMemcpy(db->s_slots, slots.data(), slots.size() * 4, hipMemcpyHostToDevice));
    SgxKfdbArgs A = kfdb_args(db);
    A.mode = SGX_KFDB_RELOC; A.Q = 1; A.q_pitch = db->max_qw; A.q_ids = db->s_ids; A.q_w = db->s_w; A.q_cnt = db->s_cnt;
    SGX_LAUNCH_DYN(k_kfdb_pairs, dim3((unsigned)((A.nslots + SGX_KFDB_TILE - 1) / SGX_KFDB_TILE), 1u), dim3(256), kfdb_query_lds(db), (sgx_stream_t)0, A);
    SGX_LAUNCH(k_kfdb_min_score, dim3(1), dim3(64), (sgx_stream_t)0, A, (const int *)db->s_slots, (int)slots.size(), db->s_min);
    SGX_CHECK_HIP(hipGetLastError());
    SGX_CHECK_HIP(hipMemcpy(min_score, db->s_min, 4, hipMemcpyDeviceToHost));
    return SGX_OK;
}
