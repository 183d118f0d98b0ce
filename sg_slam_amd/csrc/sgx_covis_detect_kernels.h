// sgx_covis_detect_kernels.h — LoopClosing::DetectLoop's covisibility consistency (src/sg-slam/src/LoopClosing.cc:152-225) with mvConsistentGroups as device state of the
// covisibility handle, and KeyFrame::GetConnectedKeyFrames (KeyFrame.cc:159-166) of a batch of keyframes as a CSR.  Everything is integer.
//
// A group is stored as its members' keyframe IDS in ascending order (include/sgx.h rule 12), one row of max_kf per group, in one half of a double buffer; the half in use,
// the number of groups and each group's counter are device words (CG_*), so a call needs no read-back to follow the one before it.  A stored id is resolved through the
// table of the live keyframes when it is tested: the id of a keyframe erased since is not in it and never matches, whoever holds its slot now.
// A candidate's group is the candidate and every LIVE keyframe with a count >= 1 in its weight row, taken in the order of that table, i.e. in ascending id.
//
// No result depends on which wave finishes first: a flag is only ever set to 1, the replay is one lane in candidate order then group order, and every row is written in
// the order of the sorted table.
#pragma once
#include "sgx_covis_kernels.h"

enum { SGX_COVIS_MAX_GROUPS = 4096 };                                                      // the marks and counters of the replay sit in LDS
enum { CG_CUR = 0, CG_N, CG_OK, CG_FIELDS = 8 };                                           // the half in use, the groups in it, "the last call left new groups to store"

struct SgxCovisCgReport {                 // sgx_covis_consistency_report
    int status, n_before, n_after, n_consistent, n_pushed_zero, n_pushed_nothing, n_enough, n_cand;
};

struct SgxCovisCgArgs {
    int G, th;                            // max_groups; mnCovisibilityConsistencyTh
    int *st;                              // CG_*
    int *cnt, *size, *mem;                // 2 x G counters, 2 x G member counts, 2 x G rows of max_kf ids
    unsigned char *flags;                 // max_kf rows of G: candidate c is consistent with stored group g
    int *cvalid, *nd_cand, *nd_cnt, *tmp_enough;      // per candidate: live and not named before; per new group: its candidate and counter; the enough-list before it is final
    const int *cand, *n_cand;
    int *enough, *n_enough;
    SgxCovisCgReport *report;
};

SGX_DEV int sgx_covis_rank_of(const SgxCovisArgs &A, int id)               // place of a live keyframe in the sorted table, -1 if there is none
{
    int lo = 0, hi = A.nlive;
    while (lo < hi) { const int mid = (lo + hi) >> 1; if (A.sorted_id[mid] < id) lo = mid + 1; else hi = mid; }
    return lo < A.nlive && A.sorted_id[lo] == id ? lo : -1;
}

// ------------------------------------------------------------------------------------------------------------------------------------------ DetectLoop :160-182
// One workgroup per candidate (grid-stride): spCandidateGroup as a byte per place of the sorted table in LDS (max_kf <= 4096: 4 KB), then every stored group against it,
// a wave per group, a lane per stored member: a binary search of the member's id and one LDS byte.  Bounded by the stored members (groups x their sizes) it resolves.
SGX_KERNEL(256) k_covis_cg_match(SgxCovisArgs A, SgxCovisCgArgs D)
{
    SGX_LDS unsigned char s_mem[SGX_COVIS_MAX_KF];
    SGX_LDS int s_bad;
    const int n = *D.n_cand;
    if (n < 0 || n > A.max_kf) return;                                       // the replay refuses the call
    const int cur = D.st[CG_CUR], ng = D.st[CG_N];
    for (int c = (int)blockIdx.x; c < n; c += (int)gridDim.x) {
        const int id = D.cand[c], s = sgx_covis_lookup(A, id);
        unsigned char *frow = D.flags + (size_t)c * D.G;
        SGX_THREADS_BEGIN(tid)
        for (int j = tid; j < A.nlive; j += 256) { const int t = A.sorted_slot[j]; s_mem[j] = s >= 0 && (t == s || A.W[(size_t)s * A.max_kf + t] > 0); }
        for (int g = tid; g < ng; g += 256) frow[g] = 0;
        if (tid == 0) s_bad = s < 0;
        SGX_THREADS_END
        SGX_SYNC();
        SGX_THREADS_BEGIN(tid)
        int dup = 0;
        for (int c2 = tid; c2 < c; c2 += 256) dup |= D.cand[c2] == id;
        if (dup) sgx_atomic_or(&s_bad, 1);
        if (s >= 0)
            for (int g = tid >> 6; g < ng; g += 4) {
                const int *row = D.mem + ((size_t)cur * D.G + g) * A.max_kf;
                const int m = D.size[cur * D.G + g];
                for (int k = tid & 63; k < m; k += 64) { const int j = sgx_covis_rank_of(A, row[k]); if (j >= 0 && s_mem[j]) frow[g] = 1; }
            }
        SGX_THREADS_END
        SGX_SYNC();
        SGX_THREADS_BEGIN(tid)
        if (tid == 0) D.cvalid[c] = !s_bad;
        SGX_THREADS_END
        SGX_SYNC();
    }
}

// ------------------------------------------------------------------------------------------------------------------------------------------ DetectLoop :160-211
// The rule replayed over the flags by one wave: the lanes bring a candidate's flag row into LDS, lane 0 walks it in group order (vbConsistentGroup and the counters are
// LDS too), serial by construction as k_covis_lm_stage2 is.  Nothing of the caller's and nothing of the state is written before the call is known to succeed: the
// enough-list is staged, the new descriptors go to the workspace, and the switch to the other half is the last thing done.  Bounded by candidates x groups LDS reads of
// one lane; a row without a set flag is skipped.
SGX_KERNEL(64) k_covis_cg_replay(SgxCovisArgs A, SgxCovisCgArgs D)
{
    SGX_LDS int s_cnt[SGX_COVIS_MAX_GROUPS];
    SGX_LDS unsigned char s_mark[SGX_COVIS_MAX_GROUPS], s_f[SGX_COVIS_MAX_GROUPS];
    SGX_LDS int s_bad, s_any, s_k, s_ne, s_cons, s_zero, s_nothing;
    const int n = *D.n_cand;
    const int cur = D.st[CG_CUR], ng = D.st[CG_N];
    const bool range_ok = n >= 0 && n <= A.max_kf;
    SGX_THREADS_BEGIN(tid)
    for (int g = tid; g < ng; g += 64) { s_cnt[g] = D.cnt[cur * D.G + g]; s_mark[g] = 0; }
    if (tid == 0) { s_bad = !range_ok; s_k = 0; s_ne = 0; s_cons = 0; s_zero = 0; s_nothing = 0; }
    SGX_THREADS_END
    SGX_SYNC();
    if (range_ok) {
        SGX_THREADS_BEGIN(tid)
        int bad = 0;
        for (int c = tid; c < n; c += 64) bad |= !D.cvalid[c];
        if (bad) sgx_atomic_or(&s_bad, 1);
        SGX_THREADS_END
        SGX_SYNC();
    }
    if (s_bad || n == 0) {                                                   // rule 13: nothing is touched; no candidate: mvConsistentGroups.clear() (:147)
        const int bad = s_bad;
        SGX_THREADS_BEGIN(tid)
        if (tid == 0) {
            SgxCovisCgReport R = {};
            R.status = bad ? -1 : 0; R.n_before = ng; R.n_after = bad ? ng : 0; R.n_cand = bad ? 0 : n;
            D.st[CG_OK] = 0;
            if (!bad) { D.st[CG_N] = 0; *D.n_enough = 0; }
            *D.report = R;
        }
        SGX_THREADS_END
        return;
    }
    for (int c = 0; c < n; c++) {
        const unsigned char *frow = D.flags + (size_t)c * D.G;
        SGX_THREADS_BEGIN(tid)
        if (tid == 0) s_any = 0;
        SGX_THREADS_END
        SGX_SYNC();
        SGX_THREADS_BEGIN(tid)
        int any = 0;
        for (int g = tid; g < ng; g += 64) { const unsigned char f = frow[g]; s_f[g] = f; any |= f; }
        if (any) sgx_atomic_or(&s_any, 1);
        SGX_THREADS_END
        SGX_SYNC();
        SGX_THREADS_BEGIN(tid)
        if (tid == 0) {
            int k = s_k;
            if (!s_any) {                                                    // :203-207
                if (k < D.G) { D.nd_cand[k] = c; D.nd_cnt[k] = 0; }
                k++; s_zero++;
            } else {
                bool enough = false; int pushed = 0;
                for (int g = 0; g < ng; g++) {
                    if (!s_f[g]) continue;
                    const int now = s_cnt[g] + 1;
                    if (!s_mark[g]) { if (k < D.G) { D.nd_cand[k] = c; D.nd_cnt[k] = now; } k++; pushed++; s_mark[g] = 1; }
                    if (now >= D.th && !enough) { D.tmp_enough[s_ne++] = D.cand[c]; enough = true; }
                }
                s_cons++; s_nothing += !pushed;
            }
            s_k = k;
        }
        SGX_THREADS_END
        SGX_SYNC();
    }
    const int k = s_k, ne = s_ne;
    if (k > D.G) {                                                           // rule 13: more groups than max_groups
        SGX_THREADS_BEGIN(tid)
        if (tid == 0) {
            SgxCovisCgReport R = {};
            R.status = -3; R.n_before = ng; R.n_after = ng; R.n_cand = n;
            D.st[CG_OK] = 0; *D.report = R;
        }
        SGX_THREADS_END
        return;
    }
    SGX_THREADS_BEGIN(tid)
    for (int e = tid; e < ne; e += 64) D.enough[e] = D.tmp_enough[e];
    for (int g = tid; g < k; g += 64) D.cnt[(1 - cur) * D.G + g] = D.nd_cnt[g];
    if (tid == 0) {
        SgxCovisCgReport R = {};
        R.n_before = ng; R.n_after = k; R.n_consistent = s_cons; R.n_pushed_zero = s_zero; R.n_pushed_nothing = s_nothing; R.n_enough = ne; R.n_cand = n;
        *D.n_enough = ne; *D.report = R;
        D.st[CG_CUR] = 1 - cur; D.st[CG_N] = k; D.st[CG_OK] = 1;
    }
    SGX_THREADS_END
}

// ------------------------------------------------------------------------------------------------------------------------------------------ DetectLoop :211
// mvConsistentGroups = vCurrentConsistentGroups: new group k is the group of its candidate, written into the half the replay switched to as the sorted table's ids
// whose weight-row entry is set: per lane a stretch of the table, counted, scanned and written.  One workgroup per new group (grid-stride); bounded by the row reads
// (2 bytes per live keyframe, twice) and the id writes.
SGX_KERNEL(256) k_covis_cg_store(SgxCovisArgs A, SgxCovisCgArgs D)
{
    SGX_LDS int s_part[256];
    if (!D.st[CG_OK]) return;
    const int cur = D.st[CG_CUR], nn = D.st[CG_N], seg = (A.nlive + 255) / 256;
    for (int k = (int)blockIdx.x; k < nn; k += (int)gridDim.x) {
        const int s = sgx_covis_lookup(A, D.cand[D.nd_cand[k]]);             // live: the replay accepted the call
        int *row = D.mem + ((size_t)cur * D.G + k) * A.max_kf;
        SGX_THREADS_BEGIN(tid)
        int c = 0;
        for (int j = tid * seg; j < A.nlive && j < (tid + 1) * seg; j++) { const int t = A.sorted_slot[j]; c += t == s || A.W[(size_t)s * A.max_kf + t] > 0; }
        s_part[tid] = c;
        SGX_THREADS_END
        SGX_SYNC();
        SGX_THREADS_BEGIN(tid)
        if (tid == 0) { int o = 0; for (int i = 0; i < 256; i++) { const int c = s_part[i]; s_part[i] = o; o += c; } D.size[cur * D.G + k] = o; }
        SGX_THREADS_END
        SGX_SYNC();
        SGX_THREADS_BEGIN(tid)
        int o = s_part[tid];
        for (int j = tid * seg; j < A.nlive && j < (tid + 1) * seg; j++) { const int t = A.sorted_slot[j]; if (t == s || A.W[(size_t)s * A.max_kf + t] > 0) row[o++] = A.sorted_id[j]; }
        SGX_THREADS_END
        SGX_SYNC();
    }
}

// ------------------------------------------------------------------------------------------------------------------------------------------ GetConnectedKeyFrames
// Per query (one workgroup each) the number of live keyframes with a count >= 1 in its row, left in the query's scalars; an unknown keyframe has none.
SGX_KERNEL(256) k_covis_conn_count(SgxCovisArgs A)
{
    SGX_LDS int s_c;
    const int q = (int)blockIdx.x;
    const int s = sgx_covis_lookup(A, A.q_kf[q]);
    SGX_THREADS_BEGIN(tid)
    if (tid == 0) s_c = 0;
    SGX_THREADS_END
    SGX_SYNC();
    SGX_THREADS_BEGIN(tid)
    int c = 0;
    if (s >= 0) for (int j = tid; j < A.nlive; j += 256) { const int t = A.sorted_slot[j]; c += t != s && A.W[(size_t)s * A.max_kf + t] > 0; }
    if (c) sgx_atomic_add(&s_c, c);
    SGX_THREADS_END
    SGX_SYNC();
    SGX_THREADS_BEGIN(tid)
    if (tid == 0) { int *w = A.ws_q + q * CQ_FIELDS; w[CQ_SLOT] = s; w[CQ_N] = s_c; }
    SGX_THREADS_END
}

// The CSR: a query's row starts where the rows before it end (off is whole, off[Q] the need), its ids in the order of the sorted table; a row is written only if it
// fits wholly (off[q + 1] <= cap), otherwise the query's status is SGX_ERR_NOMEM and nothing of it is written.  Memory-bound: the row, twice, and the ids.
SGX_KERNEL(256) k_covis_conn_emit(SgxCovisArgs A, int *off, int *ids, int cap)
{
    SGX_LDS int s_part[256];
    SGX_LDS int s_base;
    const int q = (int)blockIdx.x, seg = (A.nlive + 255) / 256;
    const int s = A.ws_q[q * CQ_FIELDS + CQ_SLOT], n = A.ws_q[q * CQ_FIELDS + CQ_N];
    SGX_THREADS_BEGIN(tid)
    int c = 0;
    for (int j = tid; j < q; j += 256) c += A.ws_q[j * CQ_FIELDS + CQ_N];
    s_part[tid] = c;
    SGX_THREADS_END
    SGX_SYNC();
    SGX_THREADS_BEGIN(tid)
    if (tid == 0) {
        int b = 0; for (int i = 0; i < 256; i++) b += s_part[i];
        s_base = b; off[q] = b;
        if (q == A.Q - 1) off[A.Q] = b + n;
        SgxCovisReport R = {};
        R.status = s < 0 ? -1 : (b + n > cap ? -3 : 0); R.n_counter = n; R.max_kf = -1; R.parent = -1;
        A.report[q] = R;
    }
    SGX_THREADS_END
    SGX_SYNC();
    if (s < 0 || s_base + n > cap) return;
    const int base = s_base;
    SGX_THREADS_BEGIN(tid)
    int c = 0;
    for (int j = tid * seg; j < A.nlive && j < (tid + 1) * seg; j++) { const int t = A.sorted_slot[j]; c += t != s && A.W[(size_t)s * A.max_kf + t] > 0; }
    s_part[tid] = c;
    SGX_THREADS_END
    SGX_SYNC();
    SGX_THREADS_BEGIN(tid)
    if (tid == 0) { int o = base; for (int i = 0; i < 256; i++) { const int c = s_part[i]; s_part[i] = o; o += c; } }
    SGX_THREADS_END
    SGX_SYNC();
    SGX_THREADS_BEGIN(tid)
    int o = s_part[tid];
    for (int j = tid * seg; j < A.nlive && j < (tid + 1) * seg; j++) { const int t = A.sorted_slot[j]; if (t != s && A.W[(size_t)s * A.max_kf + t] > 0) ids[o++] = A.sorted_id[j]; }
    SGX_THREADS_END
}
