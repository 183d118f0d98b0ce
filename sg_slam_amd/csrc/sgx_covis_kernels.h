// sgx_covis_kernels.h — the covisibility graph on the device: KeyFrame::UpdateConnections (src/sg-slam/src/KeyFrame.cc:290-380), Tracking::UpdateLocalKeyFrames +
// UpdateLocalPoints (Tracking.cc:1324-1458), the votes of LocalMapping::KeyFrameCulling (LocalMapping.cc:632-696), and the graph of the bundle adjustments: the set
// selection and the edge loop of Optimizer::LocalBundleAdjustment (Optimizer.cc:453-504, :572-653) and the edge loop of Optimizer::BundleAdjustment (:49-150).
//
// The relation "keyframe k observes point p at index i" is one int32 heap the host mirrors and patches (k_covis_scatter): per point the head of a chain of 8-entry chunks,
// its length and nObs; per keyframe slot the row mvpMapPoints[cap].  An entry is (slot << 16 | index).  The graph is device state: W[slot][slot] uint16 =
// mConnectedKeyFrameWeights, and a record per slot (id, state, N, list mode, single neighbour, parent, mbFirstConnection).  mvpOrderedConnectedKeyFrames is not stored: it is
// the entries of a row that the slot's MODE admits (all / the >= 15 ones / one neighbour), sorted by (weight, id) descending; children are the slots whose parent is k.
//
// No step depends on which workgroup or wave finishes first: integer counts, integer atomicMin / atomicMax / atomicAdd, and every order taken from keys (keyframe id,
// (weight, id), (position, index)), never from arrival.  Where a list is compacted by arrival (sgx_covis_ordered_wg) it is ranked by its keys before anything reads it.
#pragma once
#include "sgx_rt.h"
#include <limits.h>

enum { SGX_COVIS_MAX_KF = 4096, SGX_COVIS_MAX_CAP = 8192, SGX_COVIS_CHUNK = 8, SGX_COVIS_TH = 15, SGX_COVIS_BEST = 10, SGX_COVIS_LOCAL_LIMIT = 80 };
enum { SGX_COVIS_ALL = 0, SGX_COVIS_GATED = 1, SGX_COVIS_SINGLE = 2 };                    // which entries of a weight row are in the ordered list
enum { SGX_COVIS_FREE = 0, SGX_COVIS_LIVE = 1, SGX_COVIS_DEAD = 2 };                      // DEAD: erased, but another keyframe's row still lists it (isBad())
enum { CV_ID = 0, CV_STATE, CV_N, CV_MODE, CV_SINGLE, CV_PARENT, CV_FIRST, CV_PAD, CV_FIELDS };   // the record of a slot
enum { CQ_SLOT = 0, CQ_N, CQ_MAX, CQ_ARG, CQ_NORD, CQ_NL, CQ_VALID, CQ_PAD, CQ_FIELDS };          // per-query scalars between the kernels of one sequence
#ifndef SGX_COVIS_ATTR_BITS                                                               // include/sgx.h names the same bits for the edge_attr row of the BA graph
#define SGX_COVIS_ATTR_BITS
enum { SGX_COVIS_ATTR_OCTAVE = 31, SGX_COVIS_ATTR_RIGHT = 32, SGX_COVIS_ATTR_CLOSE = 64 };
#endif
enum { BQ_POINTS = CQ_N, BQ_EDGES = CQ_MAX, BQ_STEREO = CQ_ARG, BQ_NP = CQ_PAD };         // the per-query scalars as the BA graph uses them
enum { SGX_COVIS_BA_NONE = 0, SGX_COVIS_BA_FIXED = 1, SGX_COVIS_BA_LOCALKF = 2, SGX_COVIS_BA_WAVE = 64 };

struct SgxCovisReport {                   // sgx_covis_report
    int status, n_counter, max_weight, max_kf, n_ordered, parent, n_stage1, n_local_kf, n_local_points, ref_tracked;
};

struct SgxCovisBaReport {                 // sgx_covis_ba_report
    int status, n_local_kf, n_fixed_kf, n_poses, n_points, n_edges, n_mono_edges, n_stereo_edges;
};

struct SgxCovisArgs {
    int nslots, max_kf, cap, max_points, nlive, monocular;
    int *heap; size_t o_head, o_cnt, o_nobs, o_next, o_ent, o_mp;        // the relation (offsets into heap)
    const unsigned char *attr;                                           // max_kf x cap: octave | RIGHT | CLOSE
    int *kf; unsigned short *W;                                          // the graph
    const int *sorted_id, *sorted_slot;                                  // the live keyframes by ascending id (nlive)
    // workspace, one row per query
    int *ws_q, *ws_cnt, *ws_ord, *ws_ordw, *ws_lkf, *ws_pcnt, *ws_top, *ws_ntop, *stamp;
    // the batch
    int Q; const int *q_kf; SgxCovisReport *report;
    int f_cap; int *frame_mp; const int *f_n, *min_obs; int *local_kf, *n_local_kf, *ref_kf, *ref_tracked; int mcap; int *local_points, *local_obs, *n_local_points;
    int max_cand; int *cand, *n_cand, *n_red, *n_mps, *cull;
    // the bundle-adjustment graph
    int ba_global, pcap, ecap; int *pose_id; unsigned char *pose_fixed; int *point_id, *point_begin, *edge_pose, *edge_point, *edge_kp; unsigned char *edge_attr;
    SgxCovisBaReport *ba_report;
};

SGX_DEV int sgx_covis_lookup(const SgxCovisArgs &A, int id)                // slot of a live keyframe, -1 if there is none
{
    int lo = 0, hi = A.nlive;
    while (lo < hi) { const int mid = (lo + hi) >> 1; if (A.sorted_id[mid] < id) lo = mid + 1; else hi = mid; }
    return lo < A.nlive && A.sorted_id[lo] == id ? A.sorted_slot[lo] : -1;
}

// every observation (slot T, index I) of an existing point P: the head chunk holds the remainder, the chunks behind it are full
#define SGX_COVIS_FOR_OBS(A, P, T, I, BODY) do { int _left = (A).heap[(A).o_cnt + (size_t)(P)], _m = ((_left - 1) & (SGX_COVIS_CHUNK - 1)) + 1;               \
    for (int _c = (A).heap[(A).o_head + (size_t)(P)]; _left > 0 && _c >= 0; _c = (A).heap[(A).o_next + (size_t)_c], _m = SGX_COVIS_CHUNK) {                  \
        for (int _j = 0; _j < _m; _j++) { const int _e = (A).heap[(A).o_ent + (size_t)_c * SGX_COVIS_CHUNK + _j]; const int T = _e >> 16, I = _e & 0xffff; BODY } \
        _left -= _m; } } while (0)

SGX_DEV bool sgx_covis_listed(const SgxCovisArgs &A, int k, int t)
{
    const int w = A.W[(size_t)k * A.max_kf + t], mode = A.kf[k * CV_FIELDS + CV_MODE];
    return w > 0 && (mode == SGX_COVIS_ALL || (mode == SGX_COVIS_GATED && w >= SGX_COVIS_TH) || (mode == SGX_COVIS_SINGLE && t == A.kf[k * CV_FIELDS + CV_SINGLE]));
}

// the host's patches of the relation: distinct heap indices, so no two lanes write one word
SGX_KERNEL(256) k_covis_scatter(int *heap, const int *idx, const int *val, int n)
{
    SGX_THREADS_BEGIN(tid)
    const int j = (int)blockIdx.x * 256 + tid;
    if (j < n) heap[idx[j]] = val[j];
    SGX_THREADS_END
}

// mvpOrderedConnectedKeyFrames of slot k by one workgroup: out_slot / out_w [0, min(n, limit)), *out_n = n.  The members are gathered in arrival order and then ranked by
// counting the greater keys ((weight << 32) | id: sort ascending on (weight, keyframe), then reversed, KeyFrame.cc:147-157); lists are tens to hundreds long.
SGX_DEV void sgx_covis_ordered_wg(const SgxCovisArgs &A, int k, int limit, int *out_slot, int *out_w, int *out_n)
{
    SGX_LDS unsigned long long s_key[SGX_COVIS_MAX_KF];
    SGX_LDS int s_slot[SGX_COVIS_MAX_KF];
    SGX_LDS int s_n;
    SGX_THREADS_BEGIN(tid)
    if (tid == 0) s_n = 0;
    SGX_THREADS_END
    SGX_SYNC();
    if (k >= 0 && A.kf[k * CV_FIELDS + CV_STATE] == SGX_COVIS_LIVE) {
        SGX_THREADS_BEGIN(tid)
        for (int t = tid; t < A.nslots; t += (int)blockDim.x)
            if (sgx_covis_listed(A, k, t)) {
                const int pos = sgx_atomic_add(&s_n, 1);
                s_key[pos] = ((unsigned long long)A.W[(size_t)k * A.max_kf + t] << 32) | (unsigned)A.kf[t * CV_FIELDS + CV_ID];
                s_slot[pos] = t;
            }
        SGX_THREADS_END
    }
    SGX_SYNC();
    const int n = s_n;
    SGX_THREADS_BEGIN(tid)
    for (int i = tid; i < n; i += (int)blockDim.x) {
        const unsigned long long key = s_key[i];
        int rank = 0;
        for (int j = 0; j < n; j++) rank += s_key[j] > key;
        if (rank < limit) { out_slot[rank] = s_slot[i]; if (out_w) out_w[rank] = (int)(key >> 32); }
    }
    if (tid == 0) *out_n = n;
    SGX_THREADS_END
    SGX_SYNC();
}

// ------------------------------------------------------------------------------------------------------------------------------------------ UpdateConnections
// KFcounter of query q (:303-321): one workgroup, an LDS histogram over the slots; every lane takes points of the keyframe and walks their observation lists.
// Then KFcounter.size(), nmax and pKFmax (the first maximum in key order = the smallest id, :337-341).
SGX_KERNEL(256) k_covis_count(SgxCovisArgs A)
{
    SGX_LDS int s_hist[SGX_COVIS_MAX_KF];
    SGX_LDS int s_n, s_max, s_arg;
    const int q = (int)blockIdx.x;
    const int s = sgx_covis_lookup(A, A.q_kf[q]);
    int *cnt = A.ws_cnt + (size_t)q * A.max_kf;
    SGX_THREADS_BEGIN(tid)
    for (int t = tid; t < A.nslots; t += 256) s_hist[t] = 0;
    if (tid == 0) { s_n = 0; s_max = 0; s_arg = INT_MAX; }
    SGX_THREADS_END
    SGX_SYNC();
    if (s >= 0) {
        SGX_THREADS_BEGIN(tid)
        const int n = A.kf[s * CV_FIELDS + CV_N];
        for (int i = tid; i < n; i += 256) {
            const int p = A.heap[A.o_mp + (size_t)s * A.cap + i];
            if (p < 0) continue;
            SGX_COVIS_FOR_OBS(A, p, t, j, if (t != s) sgx_atomic_add(&s_hist[t], 1););
        }
        SGX_THREADS_END
    }
    SGX_SYNC();
    SGX_THREADS_BEGIN(tid)
    int n = 0, mx = 0;
    for (int t = tid; t < A.nslots; t += 256) { const int c = s_hist[t]; cnt[t] = c; if (c > 0) { n++; if (c > mx) mx = c; } }
    if (n) { sgx_atomic_add(&s_n, n); sgx_atomic_max(&s_max, mx); }
    SGX_THREADS_END
    SGX_SYNC();
    SGX_THREADS_BEGIN(tid)
    for (int t = tid; t < A.nslots; t += 256) if (s_hist[t] > 0 && s_hist[t] == s_max) sgx_atomic_min_i32(&s_arg, A.kf[t * CV_FIELDS + CV_ID]);
    SGX_THREADS_END
    SGX_SYNC();
    SGX_THREADS_BEGIN(tid)
    if (tid == 0) { int *w = A.ws_q + q * CQ_FIELDS; w[CQ_SLOT] = s; w[CQ_N] = s_n; w[CQ_MAX] = s_max; w[CQ_ARG] = s_n ? s_arg : -1; }
    SGX_THREADS_END
}

// What UpdateConnections writes (:335-379), for the queries of the batch in their order by ONE workgroup: query q's AddConnection into a neighbour and query q + 1's
// overwrite of that neighbour's whole map touch the same words, and the later one must win.  Within a query the lanes take a slot each.
SGX_DEV void sgx_covis_apply_one(const SgxCovisArgs &A, int q)
{
    SGX_LDS int s_nord, s_front;
    {
        const int *w = A.ws_q + q * CQ_FIELDS;
        const int s = w[CQ_SLOT], n = w[CQ_N], nmax = w[CQ_MAX];
        const int *cnt = A.ws_cnt + (size_t)q * A.max_kf;
        if (s < 0 || n == 0) {                                            // an unknown keyframe; an empty KFcounter returns early and leaves the old connections (:324-325)
            SGX_THREADS_BEGIN(tid)
            if (tid == 0) {
                SgxCovisReport R = {};
                R.status = s < 0 ? -1 : 0; R.max_kf = -1; R.parent = -1;
                if (s >= 0) { const int p = A.kf[s * CV_FIELDS + CV_PARENT]; R.parent = p >= 0 ? A.kf[p * CV_FIELDS + CV_ID] : -1; }
                A.report[q] = R;
            }
            SGX_THREADS_END
            return;
        }
        const bool any = nmax >= SGX_COVIS_TH;
        const int tmax = sgx_covis_lookup(A, w[CQ_ARG]);
        SGX_THREADS_BEGIN(tid)
        if (tid == 0) { s_nord = 0; s_front = -1; }
        SGX_THREADS_END
        SGX_SYNC();
        SGX_THREADS_BEGIN(tid)
        int nord = 0, front = -1;
        for (int t = tid; t < A.nslots; t += 256) {
            const int c = cnt[t];
            if (c > 0 && (any ? c >= SGX_COVIS_TH : t == tmax)) {
                unsigned short *wt = &A.W[(size_t)t * A.max_kf + s];      // (mit->first)->AddConnection(this, weight): nothing on an unchanged weight (:124-137)
                if (*wt != c) { *wt = (unsigned short)c; A.kf[t * CV_FIELDS + CV_MODE] = SGX_COVIS_ALL; }
                nord++;
                if (c == nmax && A.kf[t * CV_FIELDS + CV_ID] > front) front = A.kf[t * CV_FIELDS + CV_ID];
            }
            A.W[(size_t)s * A.max_kf + t] = (unsigned short)c;            // mConnectedKeyFrameWeights = KFcounter
        }
        if (nord) { sgx_atomic_add(&s_nord, nord); sgx_atomic_max(&s_front, front); }
        SGX_THREADS_END
        SGX_SYNC();
        SGX_THREADS_BEGIN(tid)
        if (tid == 0) {
            int *k = A.kf + s * CV_FIELDS;
            k[CV_MODE] = any ? SGX_COVIS_GATED : SGX_COVIS_SINGLE; k[CV_SINGLE] = tmax;
            SgxCovisReport R = {};
            if (k[CV_FIRST] && k[CV_ID] != 0) { k[CV_PARENT] = sgx_covis_lookup(A, s_front); k[CV_FIRST] = 0; }       // mvpOrderedConnectedKeyFrames.front() (:372-377)
            R.n_counter = n; R.max_weight = nmax; R.max_kf = w[CQ_ARG]; R.n_ordered = s_nord;
            R.parent = k[CV_PARENT] >= 0 ? A.kf[k[CV_PARENT] * CV_FIELDS + CV_ID] : -1;
            A.report[q] = R;
        }
        SGX_THREADS_END
        SGX_SYNC();
    }
}

SGX_KERNEL(256) k_covis_apply(SgxCovisArgs A)
{
    for (int q = 0; q < A.Q; q++) sgx_covis_apply_one(A, q);
}

// ------------------------------------------------------------------------------------------------------------------------------------------ ordered lists, culling
// the ordered list of query q's keyframe into its workspace row; with cand: also as ids into the caller's row (the first max_cand) and the true count
SGX_KERNEL(256) k_covis_ordered(SgxCovisArgs A)
{
    const int q = (int)blockIdx.x;
    const int s = sgx_covis_lookup(A, A.q_kf[q]);
    int *ord = A.ws_ord + (size_t)q * A.max_kf, *w = A.ws_q + q * CQ_FIELDS;
    sgx_covis_ordered_wg(A, s, A.max_kf, ord, A.ws_ordw + (size_t)q * A.max_kf, &w[CQ_NORD]);
    const int n = w[CQ_NORD];
    SGX_THREADS_BEGIN(tid)
    if (tid == 0) w[CQ_SLOT] = s;
    if (A.cand) {
        for (int r = tid; r < n && r < A.max_cand; r += 256) A.cand[(size_t)q * A.max_cand + r] = A.kf[ord[r] * CV_FIELDS + CV_ID];
        if (tid == 0) A.n_cand[q] = s < 0 ? -1 : n;
    }
    SGX_THREADS_END
}

// One workgroup per (candidate, query): nMPs and nRedundantObservations of LocalMapping.cc:645-691 over the candidate's points, the vote of :693 as written.  The early
// break of :680-681 stops the walk once three are found and changes no count; the walk here runs to the end of the list.
SGX_KERNEL(256) k_covis_cull(SgxCovisArgs A)
{
    SGX_LDS int s_mps, s_red;
    const int r = (int)blockIdx.x, q = (int)blockIdx.y;
    const int n = A.ws_q[q * CQ_FIELDS + CQ_NORD];
    if (r >= n || r >= A.max_cand) return;
    const int c = A.ws_ord[(size_t)q * A.max_kf + r];
    SGX_THREADS_BEGIN(tid)
    if (tid == 0) { s_mps = 0; s_red = 0; }
    SGX_THREADS_END
    SGX_SYNC();
    if (A.kf[c * CV_FIELDS + CV_STATE] == SGX_COVIS_LIVE && A.kf[c * CV_FIELDS + CV_ID] != 0) {      // mnId == 0 is passed over (:643); an erased keyframe has no points
        SGX_THREADS_BEGIN(tid)
        const int np = A.kf[c * CV_FIELDS + CV_N];
        int mps = 0, red = 0;
        for (int i = tid; i < np; i += 256) {
            const int p = A.heap[A.o_mp + (size_t)c * A.cap + i];
            if (p < 0) continue;
            const int a = A.attr[(size_t)c * A.cap + i];
            if (!A.monocular && !(a & SGX_COVIS_ATTR_CLOSE)) continue;
            mps++;
            if (A.heap[A.o_nobs + (size_t)p] > 3) {
                const int own = a & SGX_COVIS_ATTR_OCTAVE;
                int k = 0;
                SGX_COVIS_FOR_OBS(A, p, t, j, if (t != c && (A.attr[(size_t)t * A.cap + j] & SGX_COVIS_ATTR_OCTAVE) <= own + 1) k++;);
                if (k >= 3) red++;
            }
        }
        if (mps) sgx_atomic_add(&s_mps, mps);
        if (red) sgx_atomic_add(&s_red, red);
        SGX_THREADS_END
        SGX_SYNC();
    }
    SGX_THREADS_BEGIN(tid)
    if (tid == 0) {
        const size_t o = (size_t)q * A.max_cand + r;
        const int nRedundantObservations = s_red, nMPs = s_mps;
        A.n_red[o] = nRedundantObservations; A.n_mps[o] = nMPs;
        A.cull[o] = nRedundantObservations > 0.9 * nMPs ? 1 : 0;
    }
    SGX_THREADS_END
}

// ------------------------------------------------------------------------------------------------------------------------------------------ UpdateLocalMap
// keyframeCounter (:1353-1370) and stage 1 (:1382-1397) of query q: an LDS histogram over the frame's points, then the voted keyframes in key order = ascending id, which
// is the order of the sorted table: every lane counts the voted ones of its stretch of the table, lane 0 scans the 256 counts, every lane writes its stretch.
SGX_KERNEL(256) k_covis_lm_votes(SgxCovisArgs A)
{
    SGX_LDS int s_hist[SGX_COVIS_MAX_KF];
    SGX_LDS int s_part[256];
    SGX_LDS int s_bad, s_n, s_max, s_arg;
    const int q = (int)blockIdx.x;
    const int n = A.f_n[q], nk = A.n_local_kf[q];
    int *w = A.ws_q + q * CQ_FIELDS, *lkf = A.ws_lkf + (size_t)q * A.max_kf, *row = A.local_kf + (size_t)q * A.max_kf, *fmp = A.frame_mp + (size_t)q * A.f_cap;
    const bool shape_ok = n >= 0 && n <= A.f_cap && nk >= 0 && nk <= A.max_kf;
    SGX_THREADS_BEGIN(tid)
    for (int t = tid; t < A.nslots; t += 256) s_hist[t] = 0;
    if (tid == 0) { s_bad = shape_ok ? 0 : 1; s_n = 0; s_max = 0; s_arg = INT_MAX; }
    SGX_THREADS_END
    SGX_SYNC();
    if (shape_ok) {
        SGX_THREADS_BEGIN(tid)
        int bad = 0;
        for (int i = tid; i < n; i += 256) { const int p = fmp[i]; if (p < -1 || p >= A.max_points) bad = 1; }
        if (bad) sgx_atomic_or(&s_bad, 1);
        SGX_THREADS_END
        SGX_SYNC();
    }
    if (s_bad) {                                                          // a malformed query: its status, and nothing else of it is written by any kernel
        SGX_THREADS_BEGIN(tid)
        if (tid == 0) { SgxCovisReport R = {}; R.status = -1; R.max_kf = -1; R.parent = -1; A.report[q] = R; w[CQ_VALID] = 0; w[CQ_N] = 0; w[CQ_NL] = 0; }
        SGX_THREADS_END
        return;
    }
    SGX_THREADS_BEGIN(tid)
    for (int i = tid; i < n; i += 256) {
        const int p = fmp[i];
        if (p < 0) continue;
        if (A.heap[A.o_cnt + (size_t)p] == 0) { fmp[i] = -1; continue; }      // isBad(): mCurrentFrame.mvpMapPoints[i] = NULL (:1367)
        SGX_COVIS_FOR_OBS(A, p, t, j, sgx_atomic_add(&s_hist[t], 1););
    }
    SGX_THREADS_END
    SGX_SYNC();
    const int seg = (A.nlive + 255) / 256;
    SGX_THREADS_BEGIN(tid)
    int c = 0, mx = 0;
    for (int j = tid * seg; j < A.nlive && j < (tid + 1) * seg; j++) { const int h = s_hist[A.sorted_slot[j]]; if (h > 0) { c++; if (h > mx) mx = h; } }
    s_part[tid] = c;
    if (c) sgx_atomic_max(&s_max, mx);
    SGX_THREADS_END
    SGX_SYNC();
    SGX_THREADS_BEGIN(tid)
    if (tid == 0) { int o = 0; for (int i = 0; i < 256; i++) { const int c = s_part[i]; s_part[i] = o; o += c; } s_n = o; }
    SGX_THREADS_END
    SGX_SYNC();
    const int n1 = s_n;
    if (n1 > 0) {
        SGX_THREADS_BEGIN(tid)
        int o = s_part[tid];
        for (int j = tid * seg; j < A.nlive && j < (tid + 1) * seg; j++) {
            const int sl = A.sorted_slot[j], h = s_hist[sl];
            if (h > 0) { lkf[o] = sl; row[o] = A.sorted_id[j]; o++; if (h == s_max) sgx_atomic_min_i32(&s_arg, A.sorted_id[j]); }
        }
        SGX_THREADS_END
    } else {                                                              // no vote: mvpLocalKeyFrames stays (:1372-1373); an id that is not a live keyframe contributes nothing
        SGX_THREADS_BEGIN(tid)
        for (int j = tid; j < nk; j += 256) lkf[j] = sgx_covis_lookup(A, row[j]);
        SGX_THREADS_END
    }
    SGX_SYNC();
    SGX_THREADS_BEGIN(tid)
    if (tid == 0) { w[CQ_VALID] = 1; w[CQ_N] = n1; w[CQ_MAX] = s_max; w[CQ_ARG] = n1 ? s_arg : -1; w[CQ_NL] = n1 ? n1 : nk; }
    SGX_THREADS_END
}

// GetBestCovisibilityKeyFrames(10) of the stage-1 keyframes stage 2 can reach: it tests size() > 80 before each, so it visits at most the first 80, and none at all when
// stage 1 gave more than 80.  One workgroup per (keyframe, query).
SGX_KERNEL(256) k_covis_lm_top(SgxCovisArgs A)
{
    const int j = (int)blockIdx.x, q = (int)blockIdx.y;
    const int *w = A.ws_q + q * CQ_FIELDS;
    if (!w[CQ_VALID] || j >= w[CQ_N] || w[CQ_N] > SGX_COVIS_LOCAL_LIMIT) return;
    const size_t o = (size_t)q * SGX_COVIS_LOCAL_LIMIT + j;
    sgx_covis_ordered_wg(A, A.ws_lkf[(size_t)q * A.max_kf + j], SGX_COVIS_BEST, A.ws_top + o * SGX_COVIS_BEST, nullptr, &A.ws_ntop[o]);
}

// Stage 2 (:1401-1451) is serial by construction: what a keyframe adds depends on what the ones before it added.  One wave per query walks it; the lanes share only the
// search for the first unmarked child in key order (an atomicMin of ids over the slots).  Then mpReferenceKF, its TrackedMapPoints(min_obs) and the report.
SGX_KERNEL(64) k_covis_lm_stage2(SgxCovisArgs A)
{
    SGX_LDS unsigned char s_mark[SGX_COVIS_MAX_KF];
    SGX_LDS int s_nl, s_break, s_child, s_cnt;
    const int q = (int)blockIdx.x;
    const int *w = A.ws_q + q * CQ_FIELDS;
    if (!w[CQ_VALID]) return;
    const int n1 = w[CQ_N];
    int *lkf = A.ws_lkf + (size_t)q * A.max_kf, *row = A.local_kf + (size_t)q * A.max_kf;
    SGX_THREADS_BEGIN(tid)
    for (int t = tid; t < A.nslots; t += 64) s_mark[t] = 0;
    if (tid == 0) { s_nl = w[CQ_NL]; s_break = 0; s_cnt = 0; }
    SGX_THREADS_END
    SGX_SYNC();
    SGX_THREADS_BEGIN(tid)
    for (int j = tid; j < n1; j += 64) s_mark[lkf[j]] = 1;
    SGX_THREADS_END
    SGX_SYNC();
    for (int j = 0; j < n1; j++) {
        if (s_nl > SGX_COVIS_LOCAL_LIMIT || s_break) break;
        const int k = lkf[j];
        SGX_THREADS_BEGIN(tid)
        if (tid == 0) {
            const size_t o = (size_t)q * SGX_COVIS_LOCAL_LIMIT + j;
            const int nt = A.ws_ntop[o] < SGX_COVIS_BEST ? A.ws_ntop[o] : SGX_COVIS_BEST;
            for (int r = 0; r < nt; r++) {
                const int t = A.ws_top[o * SGX_COVIS_BEST + r];
                if (A.kf[t * CV_FIELDS + CV_STATE] == SGX_COVIS_LIVE && !s_mark[t]) { lkf[s_nl] = t; row[s_nl] = A.kf[t * CV_FIELDS + CV_ID]; s_nl++; s_mark[t] = 1; break; }
            }
            s_child = INT_MAX;
        }
        SGX_THREADS_END
        SGX_SYNC();
        SGX_THREADS_BEGIN(tid)
        for (int t = tid; t < A.nslots; t += 64)
            if (A.kf[t * CV_FIELDS + CV_STATE] == SGX_COVIS_LIVE && A.kf[t * CV_FIELDS + CV_PARENT] == k && !s_mark[t]) sgx_atomic_min_i32(&s_child, A.kf[t * CV_FIELDS + CV_ID]);
        SGX_THREADS_END
        SGX_SYNC();
        SGX_THREADS_BEGIN(tid)
        if (tid == 0) {
            if (s_child != INT_MAX) { const int t = sgx_covis_lookup(A, s_child); lkf[s_nl] = t; row[s_nl] = s_child; s_nl++; s_mark[t] = 1; }
            const int p = A.kf[k * CV_FIELDS + CV_PARENT];
            if (p >= 0 && !s_mark[p]) { lkf[s_nl] = p; row[s_nl] = A.kf[p * CV_FIELDS + CV_ID]; s_nl++; s_mark[p] = 1; s_break = 1; }      // and leaves the outer loop (:1447)
        }
        SGX_THREADS_END
        SGX_SYNC();
    }
    if (n1 > 0) {
        SGX_THREADS_BEGIN(tid)
        if (tid == 0) { A.n_local_kf[q] = s_nl; A.ref_kf[q] = w[CQ_ARG]; A.ws_q[q * CQ_FIELDS + CQ_NL] = s_nl; }
        SGX_THREADS_END
        SGX_SYNC();
    }
    const int rs = sgx_covis_lookup(A, A.ref_kf[q]);
    if (rs >= 0) {
        SGX_THREADS_BEGIN(tid)
        const int np = A.kf[rs * CV_FIELDS + CV_N], mo = A.min_obs[q];
        int c = 0;
        for (int i = tid; i < np; i += 64) { const int p = A.heap[A.o_mp + (size_t)rs * A.cap + i]; if (p >= 0 && (mo > 0 ? A.heap[A.o_nobs + (size_t)p] >= mo : true)) c++; }
        if (c) sgx_atomic_add(&s_cnt, c);
        SGX_THREADS_END
        SGX_SYNC();
    }
    SGX_THREADS_BEGIN(tid)
    if (tid == 0) {
        SgxCovisReport R = {};
        R.n_counter = n1; R.max_weight = w[CQ_MAX]; R.max_kf = w[CQ_ARG]; R.parent = -1; R.n_stage1 = n1; R.n_local_kf = s_nl; R.ref_tracked = s_cnt;
        A.report[q] = R; A.ref_tracked[q] = s_cnt; A.n_local_points[q] = 0;
    }
    SGX_THREADS_END
}

// UpdateLocalPoints (:1324-1347): keyframes in list order, indices ascending, the first occurrence of a point stands.  A point's first occurrence is the minimum of
// (position in the list) * cap + index over its occurrences: an integer atomicMin into the query's stamp row (reset to 0x7f7f7f7f before the sequence).
SGX_KERNEL(256) k_covis_lm_stamp(SgxCovisArgs A)
{
    const int q = (int)blockIdx.y;
    const int *w = A.ws_q + q * CQ_FIELDS;
    if (!w[CQ_VALID]) return;
    const int nl = w[CQ_NL];
    int *stamp = A.stamp + (size_t)q * A.max_points;
    for (int pos = (int)blockIdx.x; pos < nl; pos += (int)gridDim.x) {
        const int k = A.ws_lkf[(size_t)q * A.max_kf + pos];
        if (k < 0 || A.kf[k * CV_FIELDS + CV_STATE] != SGX_COVIS_LIVE) continue;
        SGX_THREADS_BEGIN(tid)
        const int np = A.kf[k * CV_FIELDS + CV_N];
        for (int i = tid; i < np; i += 256) { const int p = A.heap[A.o_mp + (size_t)k * A.cap + i]; if (p >= 0) sgx_atomic_min_i32(&stamp[p], pos * A.cap + i); }
        SGX_THREADS_END
    }
}

// how many points each position of the list contributes
SGX_KERNEL(256) k_covis_lm_count(SgxCovisArgs A)
{
    SGX_LDS int s_c;
    const int q = (int)blockIdx.y;
    const int *w = A.ws_q + q * CQ_FIELDS;
    if (!w[CQ_VALID]) return;
    const int nl = w[CQ_NL];
    const int *stamp = A.stamp + (size_t)q * A.max_points;
    for (int pos = (int)blockIdx.x; pos < nl; pos += (int)gridDim.x) {
        const int k = A.ws_lkf[(size_t)q * A.max_kf + pos];
        const bool live = k >= 0 && A.kf[k * CV_FIELDS + CV_STATE] == SGX_COVIS_LIVE;
        SGX_THREADS_BEGIN(tid)
        if (tid == 0) s_c = 0;
        SGX_THREADS_END
        SGX_SYNC();
        if (live) {
            SGX_THREADS_BEGIN(tid)
            const int np = A.kf[k * CV_FIELDS + CV_N];
            int c = 0;
            for (int i = tid; i < np; i += 256) { const int p = A.heap[A.o_mp + (size_t)k * A.cap + i]; if (p >= 0 && stamp[p] == pos * A.cap + i) c++; }
            if (c) sgx_atomic_add(&s_c, c);
            SGX_THREADS_END
            SGX_SYNC();
        }
        SGX_THREADS_BEGIN(tid)
        if (tid == 0) A.ws_pcnt[(size_t)q * A.max_kf + pos] = s_c;
        SGX_THREADS_END
        SGX_SYNC();
    }
}

// Emission in the reference's order by prefix sums: a position starts where the positions before it end (their counts summed by the workgroup), and within a keyframe
// every lane takes a stretch of indices, lane 0 scans the 256 counts, every lane writes its stretch.  The last position also leaves the total and the overflow status.
SGX_KERNEL(256) k_covis_lm_emit(SgxCovisArgs A)
{
    SGX_LDS int s_part[256];
    SGX_LDS int s_base;
    const int q = (int)blockIdx.y;
    const int *w = A.ws_q + q * CQ_FIELDS;
    if (!w[CQ_VALID]) return;
    const int nl = w[CQ_NL];
    const int *stamp = A.stamp + (size_t)q * A.max_points, *pcnt = A.ws_pcnt + (size_t)q * A.max_kf;
    for (int pos = (int)blockIdx.x; pos < nl; pos += (int)gridDim.x) {
        const int k = A.ws_lkf[(size_t)q * A.max_kf + pos];
        const bool live = k >= 0 && A.kf[k * CV_FIELDS + CV_STATE] == SGX_COVIS_LIVE;
        const int np = live ? A.kf[k * CV_FIELDS + CV_N] : 0, seg = (np + 255) / 256;
        SGX_THREADS_BEGIN(tid)
        int c = 0;
        for (int j = tid; j < pos; j += 256) c += pcnt[j];
        s_part[tid] = c;
        SGX_THREADS_END
        SGX_SYNC();
        SGX_THREADS_BEGIN(tid)
        if (tid == 0) { int b = 0; for (int i = 0; i < 256; i++) b += s_part[i]; s_base = b; }
        SGX_THREADS_END
        SGX_SYNC();
        SGX_THREADS_BEGIN(tid)
        int c = 0;
        for (int i = tid * seg; i < np && i < (tid + 1) * seg; i++) { const int p = A.heap[A.o_mp + (size_t)k * A.cap + i]; if (p >= 0 && stamp[p] == pos * A.cap + i) c++; }
        s_part[tid] = c;
        SGX_THREADS_END
        SGX_SYNC();
        SGX_THREADS_BEGIN(tid)
        if (tid == 0) {
            int o = s_base;
            for (int i = 0; i < 256; i++) { const int c = s_part[i]; s_part[i] = o; o += c; }
            if (pos == nl - 1) { A.n_local_points[q] = o; A.report[q].n_local_points = o; if (o > A.mcap) A.report[q].status = -3; }      // SGX_ERR_NOMEM
        }
        SGX_THREADS_END
        SGX_SYNC();
        SGX_THREADS_BEGIN(tid)
        int o = s_part[tid];
        for (int i = tid * seg; i < np && i < (tid + 1) * seg; i++) {
            const int p = A.heap[A.o_mp + (size_t)k * A.cap + i];
            if (p >= 0 && stamp[p] == pos * A.cap + i) { if (o < A.mcap) { A.local_points[(size_t)q * A.mcap + o] = p; A.local_obs[(size_t)q * A.mcap + o] = A.heap[A.o_nobs + (size_t)p]; } o++; }
        }
        SGX_THREADS_END
        SGX_SYNC();
    }
}

// ------------------------------------------------------------------------------------------------------------------------------------------ KeyFrame::SetBadFlag
// The graph part of erasing slot s (:467-541) by one workgroup: EraseConnection in every keyframe of its own map, then the spanning-tree loop: of the children, the
// (child, parent candidate) pair of the greatest weight is joined, the earliest child in key order on a tie (strictly greater, :509) and within a child the first in
// its ordered list; the child becomes a candidate; children that reach no candidate go to the erased keyframe's parent.
SGX_KERNEL(256) k_covis_erase_graph(SgxCovisArgs A, int s)
{
    SGX_LDS unsigned char s_cand[SGX_COVIS_MAX_KF];
    SGX_LDS int s_bw[256], s_bc[256], s_bp[256];
    SGX_LDS int s_go;
    const int parent = A.kf[s * CV_FIELDS + CV_PARENT];
    SGX_THREADS_BEGIN(tid)
    for (int t = tid; t < A.nslots; t += 256) {
        s_cand[t] = t == parent;
        if (A.W[(size_t)s * A.max_kf + t] > 0) {
            unsigned short *wt = &A.W[(size_t)t * A.max_kf + s];
            if (*wt > 0) { *wt = 0; A.kf[t * CV_FIELDS + CV_MODE] = SGX_COVIS_ALL; }      // EraseConnection + UpdateBestCovisibles (:554-568)
            A.W[(size_t)s * A.max_kf + t] = 0;
        }
    }
    SGX_THREADS_END
    SGX_SYNC();
    for (int round = 0; round < A.nslots; round++) {
        SGX_THREADS_BEGIN(tid)
        int bw = -1, bc = -1, bp = -1;
        for (int c = tid; c < A.nslots; c += 256) {
            if (A.kf[c * CV_FIELDS + CV_STATE] != SGX_COVIS_LIVE || A.kf[c * CV_FIELDS + CV_PARENT] != s) continue;
            int cw = -1, cp = -1;                                         // this child's first-best candidate in its list order: weight descending, the later id first
            for (int t = 0; t < A.nslots; t++)
                if (s_cand[t] && sgx_covis_listed(A, c, t)) {
                    const int wv = A.W[(size_t)c * A.max_kf + t];
                    if (wv > cw || (wv == cw && A.kf[t * CV_FIELDS + CV_ID] > A.kf[cp * CV_FIELDS + CV_ID])) { cw = wv; cp = t; }
                }
            if (cw > bw || (cw == bw && cw >= 0 && A.kf[c * CV_FIELDS + CV_ID] < A.kf[bc * CV_FIELDS + CV_ID])) { bw = cw; bc = c; bp = cp; }
        }
        s_bw[tid] = bw; s_bc[tid] = bc; s_bp[tid] = bp;
        SGX_THREADS_END
        SGX_SYNC();
        SGX_THREADS_BEGIN(tid)
        if (tid == 0) {
            int bw = -1, bc = -1, bp = -1;
            for (int i = 0; i < 256; i++)
                if (s_bw[i] > bw || (s_bw[i] == bw && bw >= 0 && A.kf[s_bc[i] * CV_FIELDS + CV_ID] < A.kf[bc * CV_FIELDS + CV_ID])) { bw = s_bw[i]; bc = s_bc[i]; bp = s_bp[i]; }
            s_go = bw >= 0;
            if (bw >= 0) { A.kf[bc * CV_FIELDS + CV_PARENT] = bp; s_cand[bc] = 1; }      // pC->ChangeParent(pP)
        }
        SGX_THREADS_END
        SGX_SYNC();
        if (!s_go) break;
    }
    SGX_THREADS_BEGIN(tid)
    for (int c = tid; c < A.nslots; c += 256)
        if (c != s && A.kf[c * CV_FIELDS + CV_PARENT] == s) A.kf[c * CV_FIELDS + CV_PARENT] = parent;
    SGX_THREADS_END
    SGX_SYNC();
    SGX_THREADS_BEGIN(tid)
    if (tid == 0) { int *k = A.kf + s * CV_FIELDS; k[CV_STATE] = SGX_COVIS_DEAD; k[CV_PARENT] = -1; k[CV_MODE] = SGX_COVIS_ALL; k[CV_N] = 0; }
    SGX_THREADS_END
}

// how many rows still list each slot (a DEAD slot with none can be given out again)
SGX_KERNEL(256) k_covis_refs(SgxCovisArgs A, int *refs)
{
    SGX_THREADS_BEGIN(tid)
    const int t = (int)blockIdx.x * 256 + tid;
    if (t < A.nslots) { int c = 0; for (int k = 0; k < A.nslots; k++) c += A.W[(size_t)k * A.max_kf + t] > 0; refs[t] = c; }
    SGX_THREADS_END
}

// ------------------------------------------------------------------------------------------------------------------------------------------ the bundle-adjustment graph
// The set selection of Optimizer::LocalBundleAdjustment (Optimizer.cc:453-504) and its edge loop (:572-653), and the same edge loop over the whole map for
// Optimizer::BundleAdjustment (:49-150).  Per query the five workspace rows hold: ws_cnt the ROLE of every slot (none / fixed camera / local keyframe), ws_ord the ordered
// list and later the pose index of every slot, ws_lkf lLocalKeyFrames as slots (-1 where the list names an erased keyframe), ws_pcnt the points every position contributes;
// the stamp row is UpdateLocalPoints' (k_covis_lm_stamp is launched as it is).  The scalars BQ_* are summed with integer atomics.
//
// Query q's validity, lLocalKeyFrames = the keyframe and then its ordered list without the isBad() entries (:458-468), and the roles.  Global mode: every live slot is local.
SGX_KERNEL(256) k_covis_ba_begin(SgxCovisArgs A)
{
    const int q = (int)blockIdx.x;
    int *w = A.ws_q + q * CQ_FIELDS, *role = A.ws_cnt + (size_t)q * A.max_kf, *ord = A.ws_ord + (size_t)q * A.max_kf, *lkf = A.ws_lkf + (size_t)q * A.max_kf;
    const int s = A.ba_global ? -1 : sgx_covis_lookup(A, A.q_kf[q]);
    if (A.pcap < 0 || A.ecap < 0 || (!A.ba_global && s < 0)) {          // its status, and nothing else of it is written by any kernel
        SGX_THREADS_BEGIN(tid)
        if (tid == 0) { SgxCovisBaReport R = {}; R.status = -1; A.ba_report[q] = R; w[CQ_VALID] = 0; }
        SGX_THREADS_END
        return;
    }
    sgx_covis_ordered_wg(A, s, A.max_kf, ord, nullptr, &w[CQ_NORD]);
    const int n = A.ba_global ? 0 : (w[CQ_NORD] < A.max_kf ? w[CQ_NORD] : A.max_kf - 1);
    SGX_THREADS_BEGIN(tid)
    for (int t = tid; t < A.nslots; t += 256) role[t] = A.ba_global && A.kf[t * CV_FIELDS + CV_STATE] == SGX_COVIS_LIVE ? SGX_COVIS_BA_LOCALKF : SGX_COVIS_BA_NONE;
    SGX_THREADS_END
    SGX_SYNC();
    SGX_THREADS_BEGIN(tid)
    if (!A.ba_global) {
        if (tid == 0) { lkf[0] = s; role[s] = SGX_COVIS_BA_LOCALKF; }
        for (int r = tid; r < n; r += 256) {                              // pKFi->mnBALocalForKF is set for a bad one too (:465), which has no observation to be met through again
            const int t = ord[r];
            const bool live = A.kf[t * CV_FIELDS + CV_STATE] == SGX_COVIS_LIVE;
            lkf[1 + r] = live ? t : -1;
            if (live) role[t] = SGX_COVIS_BA_LOCALKF;
        }
    }
    if (tid == 0) { w[CQ_SLOT] = s; w[CQ_VALID] = 1; w[CQ_NL] = A.ba_global ? 0 : 1 + n; w[BQ_POINTS] = 0; w[BQ_EDGES] = 0; w[BQ_STEREO] = 0; w[BQ_NP] = 0; }
    SGX_THREADS_END
}

// Per position of lLocalKeyFrames: the points it contributes to lLocalMapPoints (those whose stamp it holds), their observations = edges, the stereo ones among them, and
// lFixedCameras (:489-504): every observing slot without a role gets the fixed one.  A lane takes a point and walks its chain; the marks are idempotent.
SGX_KERNEL(256) k_covis_ba_count(SgxCovisArgs A)
{
    SGX_LDS int s_c, s_e, s_s;
    const int q = (int)blockIdx.y;
    int *w = A.ws_q + q * CQ_FIELDS;
    if (!w[CQ_VALID]) return;
    const int nl = w[CQ_NL];
    const int *stamp = A.stamp + (size_t)q * A.max_points;
    int *role = A.ws_cnt + (size_t)q * A.max_kf;
    for (int pos = (int)blockIdx.x; pos < nl; pos += (int)gridDim.x) {
        const int k = A.ws_lkf[(size_t)q * A.max_kf + pos];
        SGX_THREADS_BEGIN(tid)
        if (tid == 0) { s_c = 0; s_e = 0; s_s = 0; }
        SGX_THREADS_END
        SGX_SYNC();
        if (k >= 0 && A.kf[k * CV_FIELDS + CV_STATE] == SGX_COVIS_LIVE) {
            SGX_THREADS_BEGIN(tid)
            const int np = A.kf[k * CV_FIELDS + CV_N];
            int c = 0, e = 0, st = 0;
            for (int i = tid; i < np; i += 256) {
                const int p = A.heap[A.o_mp + (size_t)k * A.cap + i];
                if (p < 0 || stamp[p] != pos * A.cap + i) continue;
                c++; e += A.heap[A.o_cnt + (size_t)p];
                SGX_COVIS_FOR_OBS(A, p, t, j, if (A.attr[(size_t)t * A.cap + j] & SGX_COVIS_ATTR_RIGHT) st++;
                                              if (role[t] == SGX_COVIS_BA_NONE) sgx_atomic_max(&role[t], (int)SGX_COVIS_BA_FIXED););
            }
            if (c) sgx_atomic_add(&s_c, c);
            if (e) sgx_atomic_add(&s_e, e);
            if (st) sgx_atomic_add(&s_s, st);
            SGX_THREADS_END
            SGX_SYNC();
        }
        SGX_THREADS_BEGIN(tid)
        if (tid == 0) {
            A.ws_pcnt[(size_t)q * A.max_kf + pos] = s_c;
            if (s_e) sgx_atomic_add(&w[BQ_EDGES], s_e);
            if (s_s) sgx_atomic_add(&w[BQ_STEREO], s_s);
        }
        SGX_THREADS_END
        SGX_SYNC();
    }
}

// Global mode: the existing points of the whole map, their observations and the stereo ones, by a grid over the point ids
SGX_KERNEL(256) k_covis_ba_all_count(SgxCovisArgs A)
{
    SGX_LDS int s_c, s_e, s_s;
    int *w = A.ws_q;
    if (!w[CQ_VALID]) return;
    SGX_THREADS_BEGIN(tid)
    if (tid == 0) { s_c = 0; s_e = 0; s_s = 0; }
    SGX_THREADS_END
    SGX_SYNC();
    SGX_THREADS_BEGIN(tid)
    int c = 0, e = 0, st = 0;
    for (long long p = (long long)blockIdx.x * 256 + tid; p < A.max_points; p += (long long)gridDim.x * 256) {
        const int n = A.heap[A.o_cnt + (size_t)p];
        if (n <= 0) continue;
        c++; e += n;
        SGX_COVIS_FOR_OBS(A, p, t, j, if (A.attr[(size_t)t * A.cap + j] & SGX_COVIS_ATTR_RIGHT) st++;);
    }
    if (c) sgx_atomic_add(&s_c, c);
    if (e) sgx_atomic_add(&s_e, e);
    if (st) sgx_atomic_add(&s_s, st);
    SGX_THREADS_END
    SGX_SYNC();
    SGX_THREADS_BEGIN(tid)
    if (tid == 0) {
        if (s_c) sgx_atomic_add(&w[BQ_POINTS], s_c);
        if (s_e) sgx_atomic_add(&w[BQ_EDGES], s_e);
        if (s_s) sgx_atomic_add(&w[BQ_STEREO], s_s);
    }
    SGX_THREADS_END
}

// Global mode: the existing points in ascending id by one workgroup: every lane counts its stretch of the ids, lane 0 scans the 256 counts, every lane writes its stretch
// (the first pcap); point_begin holds every written point's number of observations until k_covis_ba_scan turns it into the prefix.
SGX_KERNEL(256) k_covis_ba_all_points(SgxCovisArgs A)
{
    SGX_LDS int s_part[256];
    if (!A.ws_q[CQ_VALID]) return;
    const long long seg = ((long long)A.max_points + 255) / 256;
    SGX_THREADS_BEGIN(tid)
    int c = 0;
    for (long long p = tid * seg; p < A.max_points && p < (tid + 1) * seg; p++) c += A.heap[A.o_cnt + (size_t)p] > 0;
    s_part[tid] = c;
    SGX_THREADS_END
    SGX_SYNC();
    SGX_THREADS_BEGIN(tid)
    if (tid == 0) { int o = 0; for (int i = 0; i < 256; i++) { const int c = s_part[i]; s_part[i] = o; o += c; } }
    SGX_THREADS_END
    SGX_SYNC();
    SGX_THREADS_BEGIN(tid)
    int o = s_part[tid];
    for (long long p = tid * seg; p < A.max_points && p < (tid + 1) * seg; p++) {
        const int n = A.heap[A.o_cnt + (size_t)p];
        if (n > 0) { if (o < A.pcap) { A.point_id[o] = (int)p; A.point_begin[o] = n; } o++; }
    }
    SGX_THREADS_END
}

// The poses: the slots with a role in ascending keyframe id = the order of the sorted table (every lane counts its stretch, lane 0 scans, every lane writes), the pose
// index of every slot for the edges, and the report with the true counts.
SGX_KERNEL(256) k_covis_ba_poses(SgxCovisArgs A)
{
    SGX_LDS int s_part[256];
    SGX_LDS int s_n, s_loc, s_pts;
    const int q = (int)blockIdx.x;
    int *w = A.ws_q + q * CQ_FIELDS;
    if (!w[CQ_VALID]) return;
    const int nl = w[CQ_NL];
    const int *role = A.ws_cnt + (size_t)q * A.max_kf, *pcnt = A.ws_pcnt + (size_t)q * A.max_kf;
    int *pidx = A.ws_ord + (size_t)q * A.max_kf, *pose_id = A.pose_id + (size_t)q * A.max_kf;
    unsigned char *pose_fixed = A.pose_fixed + (size_t)q * A.max_kf;
    const int seg = (A.nlive + 255) / 256;
    SGX_THREADS_BEGIN(tid)
    for (int t = tid; t < A.nslots; t += 256) pidx[t] = -1;
    if (tid == 0) { s_loc = 0; s_pts = 0; }
    SGX_THREADS_END
    SGX_SYNC();
    SGX_THREADS_BEGIN(tid)
    int c = 0, loc = 0, pc = 0;
    for (int j = tid * seg; j < A.nlive && j < (tid + 1) * seg; j++) { const int r = role[A.sorted_slot[j]]; if (r != SGX_COVIS_BA_NONE) { c++; loc += r == SGX_COVIS_BA_LOCALKF; } }
    for (int j = tid; j < nl; j += 256) pc += pcnt[j];
    s_part[tid] = c;
    if (loc) sgx_atomic_add(&s_loc, loc);
    if (pc) sgx_atomic_add(&s_pts, pc);
    SGX_THREADS_END
    SGX_SYNC();
    SGX_THREADS_BEGIN(tid)
    if (tid == 0) { int o = 0; for (int i = 0; i < 256; i++) { const int c = s_part[i]; s_part[i] = o; o += c; } s_n = o; }
    SGX_THREADS_END
    SGX_SYNC();
    SGX_THREADS_BEGIN(tid)
    int o = s_part[tid];
    for (int j = tid * seg; j < A.nlive && j < (tid + 1) * seg; j++) {
        const int sl = A.sorted_slot[j], r = role[sl], id = A.sorted_id[j];
        if (r == SGX_COVIS_BA_NONE) continue;
        pose_id[o] = id; pose_fixed[o] = (unsigned char)(r == SGX_COVIS_BA_FIXED ? 1 : id == 0 ? 2 : 0);      // vSE3->setFixed(pKFi->mnId==0) (:529)
        pidx[sl] = o; o++;
    }
    if (tid == 0) {
        const int n_points = A.ba_global ? w[BQ_POINTS] : s_pts, n_edges = w[BQ_EDGES];
        w[BQ_POINTS] = n_points; w[BQ_NP] = n_points < A.pcap ? n_points : A.pcap;
        SgxCovisBaReport R = {};
        R.status = n_points > A.pcap || n_edges > A.ecap ? -3 : 0;          // SGX_ERR_NOMEM
        R.n_local_kf = s_loc; R.n_fixed_kf = s_n - s_loc; R.n_poses = s_n; R.n_points = n_points; R.n_edges = n_edges;
        R.n_stereo_edges = w[BQ_STEREO]; R.n_mono_edges = n_edges - w[BQ_STEREO];
        A.ba_report[q] = R;
    }
    SGX_THREADS_END
}

// lLocalMapPoints (:472-486) in the reference's order, as k_covis_lm_emit does it: a position starts where the positions before it end, within a keyframe every lane takes
// a stretch of indices.  point_begin holds every written point's number of observations until k_covis_ba_scan turns it into the prefix.
SGX_KERNEL(256) k_covis_ba_points(SgxCovisArgs A)
{
    SGX_LDS int s_part[256];
    SGX_LDS int s_base;
    const int q = (int)blockIdx.y;
    const int *w = A.ws_q + q * CQ_FIELDS;
    if (!w[CQ_VALID]) return;
    const int nl = w[CQ_NL];
    const int *stamp = A.stamp + (size_t)q * A.max_points, *pcnt = A.ws_pcnt + (size_t)q * A.max_kf;
    int *point_id = A.point_id + (size_t)q * A.pcap, *point_begin = A.point_begin + (size_t)q * ((size_t)A.pcap + 1);
    for (int pos = (int)blockIdx.x; pos < nl; pos += (int)gridDim.x) {
        const int k = A.ws_lkf[(size_t)q * A.max_kf + pos];
        const bool live = k >= 0 && A.kf[k * CV_FIELDS + CV_STATE] == SGX_COVIS_LIVE;
        const int np = live ? A.kf[k * CV_FIELDS + CV_N] : 0, seg = (np + 255) / 256;
        SGX_THREADS_BEGIN(tid)
        int c = 0;
        for (int j = tid; j < pos; j += 256) c += pcnt[j];
        s_part[tid] = c;
        SGX_THREADS_END
        SGX_SYNC();
        SGX_THREADS_BEGIN(tid)
        if (tid == 0) { int b = 0; for (int i = 0; i < 256; i++) b += s_part[i]; s_base = b; }
        SGX_THREADS_END
        SGX_SYNC();
        SGX_THREADS_BEGIN(tid)
        int c = 0;
        for (int i = tid * seg; i < np && i < (tid + 1) * seg; i++) { const int p = A.heap[A.o_mp + (size_t)k * A.cap + i]; if (p >= 0 && stamp[p] == pos * A.cap + i) c++; }
        s_part[tid] = c;
        SGX_THREADS_END
        SGX_SYNC();
        SGX_THREADS_BEGIN(tid)
        if (tid == 0) { int o = s_base; for (int i = 0; i < 256; i++) { const int c = s_part[i]; s_part[i] = o; o += c; } }
        SGX_THREADS_END
        SGX_SYNC();
        SGX_THREADS_BEGIN(tid)
        int o = s_part[tid];
        for (int i = tid * seg; i < np && i < (tid + 1) * seg; i++) {
            const int p = A.heap[A.o_mp + (size_t)k * A.cap + i];
            if (p >= 0 && stamp[p] == pos * A.cap + i) { if (o < A.pcap) { point_id[o] = p; point_begin[o] = A.heap[A.o_cnt + (size_t)p]; } o++; }
        }
        SGX_THREADS_END
        SGX_SYNC();
    }
}

// point_edge_begin: the exclusive prefix of the written points' observation counts, and their total behind the last one
SGX_KERNEL(256) k_covis_ba_scan(SgxCovisArgs A)
{
    SGX_LDS int s_part[256];
    SGX_LDS int s_total;
    const int q = (int)blockIdx.x;
    const int *w = A.ws_q + q * CQ_FIELDS;
    if (!w[CQ_VALID]) return;
    const int np = w[BQ_NP], seg = (np + 255) / 256;
    int *point_begin = A.point_begin + (size_t)q * ((size_t)A.pcap + 1);
    SGX_THREADS_BEGIN(tid)
    int c = 0;
    for (int i = tid * seg; i < np && i < (tid + 1) * seg; i++) c += point_begin[i];
    s_part[tid] = c;
    SGX_THREADS_END
    SGX_SYNC();
    SGX_THREADS_BEGIN(tid)
    if (tid == 0) { int o = 0; for (int i = 0; i < 256; i++) { const int c = s_part[i]; s_part[i] = o; o += c; } s_total = o; }
    SGX_THREADS_END
    SGX_SYNC();
    SGX_THREADS_BEGIN(tid)
    int o = s_part[tid];
    for (int i = tid * seg; i < np && i < (tid + 1) * seg; i++) { const int c = point_begin[i]; point_begin[i] = o; o += c; }
    SGX_THREADS_END
    SGX_SYNC();
    SGX_THREADS_BEGIN(tid)
    if (tid == 0) point_begin[np] = s_total;
    SGX_THREADS_END
}

// the entries first, first + stride, ... (stride a power of two) of point p's chain, at their chain positions: the observing keyframe's id and the entry itself
SGX_DEV void sgx_covis_ba_stage(const SgxCovisArgs &A, int p, int n, int first, int stride, int *s_id, int *s_e)
{
    int j0 = 0, left = n, m = ((n - 1) & (SGX_COVIS_CHUNK - 1)) + 1;          // the walk of SGX_COVIS_FOR_OBS over the chunks alone: only the lane's own entries are loaded
    for (int c = A.heap[A.o_head + (size_t)p]; left > 0 && c >= 0; c = A.heap[A.o_next + (size_t)c], m = SGX_COVIS_CHUNK) {
        for (int j = j0 + ((first - j0) & (stride - 1)); j < j0 + m; j += stride) {
            const int e = A.heap[A.o_ent + (size_t)c * SGX_COVIS_CHUNK + (j - j0)];
            s_id[j] = A.kf[(e >> 16) * CV_FIELDS + CV_ID]; s_e[j] = e;
        }
        j0 += m; left -= m;
    }
}

// one edge of point number i: the observation staged at s_id[k] / s_e[k] of n goes behind those of a smaller keyframe id (map<KeyFrame*, size_t> order, rule 1)
SGX_DEV void sgx_covis_ba_edge(const SgxCovisArgs &A, int q, int i, int begin, int n, int k, const int *s_id, const int *s_e, const int *pidx)
{
    const int id = s_id[k], e = s_e[k], t = e >> 16, ix = e & 0xffff;
    int rank = 0;
    for (int m = 0; m < n; m++) rank += s_id[m] < id;
    if (begin + rank >= A.ecap) return;
    const size_t o = (size_t)q * A.ecap + begin + rank;
    A.edge_pose[o] = pidx[t]; A.edge_point[o] = i; A.edge_kp[o] = ix; A.edge_attr[o] = A.attr[(size_t)t * A.cap + ix];
}

// The edges (:572-653): point i's observations in ascending keyframe id at point_begin[i] ...  A point seen by at most 64 keyframes is a wave's: the workgroup takes four
// points at a time, lane l stages observation l of its wave's point in LDS and ranks it against the others.  A longer list (up to every keyframe) is the whole
// workgroup's.  Only the points whose edges fit wholly are written.
SGX_KERNEL(256) k_covis_ba_edges(SgxCovisArgs A)
{
    SGX_LDS int s_id[SGX_COVIS_MAX_KF];
    SGX_LDS int s_e[SGX_COVIS_MAX_KF];
    const int q = (int)blockIdx.y;
    const int *w = A.ws_q + q * CQ_FIELDS;
    if (!w[CQ_VALID]) return;
    const int np = w[BQ_NP];
    const int *point_id = A.point_id + (size_t)q * A.pcap, *point_begin = A.point_begin + (size_t)q * ((size_t)A.pcap + 1), *pidx = A.ws_ord + (size_t)q * A.max_kf;
    for (int base = (int)blockIdx.x * 4; base < np; base += (int)gridDim.x * 4) {
        SGX_THREADS_BEGIN(tid)
        const int wv = tid >> 6, lane = tid & 63, i = base + wv;
        if (i < np) {
            const int p = point_id[i], n = A.heap[A.o_cnt + (size_t)p];
            if (n <= SGX_COVIS_BA_WAVE && lane < n) sgx_covis_ba_stage(A, p, n, lane, SGX_COVIS_BA_WAVE, s_id + wv * SGX_COVIS_BA_WAVE, s_e + wv * SGX_COVIS_BA_WAVE);
        }
        SGX_THREADS_END
        SGX_SYNC();
        SGX_THREADS_BEGIN(tid)
        const int wv = tid >> 6, lane = tid & 63, i = base + wv;
        if (i < np) {
            const int n = A.heap[A.o_cnt + (size_t)point_id[i]];
            if (n <= SGX_COVIS_BA_WAVE && lane < n && point_begin[i + 1] <= A.ecap)
                sgx_covis_ba_edge(A, q, i, point_begin[i], n, lane, s_id + wv * SGX_COVIS_BA_WAVE, s_e + wv * SGX_COVIS_BA_WAVE, pidx);
        }
        SGX_THREADS_END
        SGX_SYNC();
    }
    for (int i = (int)blockIdx.x; i < np; i += (int)gridDim.x) {
        const int p = point_id[i], n = A.heap[A.o_cnt + (size_t)p];
        if (n <= SGX_COVIS_BA_WAVE || n > SGX_COVIS_MAX_KF || point_begin[i + 1] > A.ecap) continue;
        SGX_THREADS_BEGIN(tid)
        sgx_covis_ba_stage(A, p, n, tid, 256, s_id, s_e);
        SGX_THREADS_END
        SGX_SYNC();
        SGX_THREADS_BEGIN(tid)
        for (int k = tid; k < n; k += 256) sgx_covis_ba_edge(A, q, i, point_begin[i], n, k, s_id, s_e, pidx);
        SGX_THREADS_END
        SGX_SYNC();
    }
}
