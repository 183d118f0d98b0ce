// sgx_kfdb_kernels.h — KeyFrameDatabase::DetectRelocalizationCandidates (src/sg-slam/src/KeyFrameDatabase.cc:199-309) and DetectLoopCandidates (:76-197) on the device.
//
// The reference searches an inverted file (per word, the keyframes holding it in add() order).  The device keeps only the forward file (per keyframe its BowVector, ids
// ascending) and scans it: one launch over (keyframe tiles x queries) intersects every keyframe with every query.  What the inverted file contributes beyond the set of
// sharing keyframes is the ORDER of lKFsSharingWords: the query's words ascending and, within a word, that word's list in add() order; a keyframe enters at its first common
// word, so its position is the pair (first common word, add sequence number) ascending.  lScoreAndMatch, lAccScoreAndMatch and the returned vector keep that order.
//
// Per (keyframe, query):  k_kfdb_pairs   common-word count, first common word, L1 score (ScoringObject.cpp:23-67) as a sequential double sum in ascending word order
// Per query:              k_kfdb_gate    lKFsSharingWords.size(), maxCommonWords, minCommonWords = (int)(maxCommonWords * 0.8f)
// Per keyframe:           k_kfdb_stale   mRelocScore as every query of the batch sees it (relocalisation only): one lane per keyframe walks q = 0 .. Q-1
// Per query:              k_kfdb_select  rank by (first word, sequence), covisibility accumulation, bestAccScore, retention, first-occurrence dedup, emission
// No step depends on the order in which workgroups or waves finish: integer counts and maxima, an integer atomicMin, and sums that one lane forms in the reference's order.
#pragma once
#include "sgx_rt.h"
#include <limits.h>

enum { SGX_KFDB_RELOC = 0, SGX_KFDB_LOOP = 1, SGX_KFDB_COVIS = 10, SGX_KFDB_TILE = 16 };

struct SgxKfdbReport {                    // sgx_kfdb_report
    int n_sharing, max_common_words, min_common_words, n_scores, n_score_and_match;
    float best_acc_score, min_score_to_retain;
    int n_candidates, status;
};

struct SgxKfdbArgs {
    // the database: slot s in [0, nslots) holds a keyframe (cnt[s] entries at off[s]) or is free (cnt 0, kf_id -1)
    int nslots, max_kf, max_qw, nlive;
    const int *ent_id; const double *ent_w;
    const int *off, *cnt, *seq, *kf_id, *covis;      // covis: SGX_KFDB_COVIS slots per keyframe in the caller's order, -1 = absent from the database
    const int *sorted_id, *sorted_slot;              // the live keyframes by ascending caller id (nlive), for the connected-set lookup
    float *reloc;                                    // mRelocScore per slot, persistent
    // the batch
    int mode, Q, q_pitch;
    const int *q_ids; const double *q_w; const int *q_cnt;
    const int *conn_off, *conn_ids; const float *min_score;
    unsigned char *conn;                             // Q x max_kf: 1 = in spConnectedKeyFrames (loop)
    int *words, *first; float *score;                // Q x max_kf
    unsigned long long *key;                         // Q x max_kf: (first word, sequence) of a keyframe in lScoreAndMatch, ~0 otherwise
    int *order, *best, *firstrank; float *acc;       // Q x max_kf, by rank (firstrank by slot)
    int *cand, *n_cand; SgxKfdbReport *report;
};

// a query is usable if its length fits its row and the LDS buffer; anything else is reported per query (status) and behaves as an empty one
SGX_DEV bool sgx_kfdb_qvalid(const SgxKfdbArgs &A, int q) { const int n = A.q_cnt[q]; return n >= 0 && n <= A.max_qw && n <= A.q_pitch; }
SGX_DEV int sgx_kfdb_qlen(const SgxKfdbArgs &A, int q) { return sgx_kfdb_qvalid(A, q) ? A.q_cnt[q] : 0; }

// spConnectedKeyFrames as a flag per slot: every connected id is looked up in the id-sorted table
SGX_KERNEL(256) k_kfdb_connected(SgxKfdbArgs A)
{
    const int q = (int)blockIdx.x;
    const int j0 = A.conn_off[q], j1 = A.conn_off[q + 1];
    SGX_THREADS_BEGIN(tid)
    for (int j = j0 + tid; j < j1; j += 256) {
        const int id = A.conn_ids[j];
        int lo = 0, hi = A.nlive;
        while (lo < hi) { const int mid = (lo + hi) >> 1; if (A.sorted_id[mid] < id) lo = mid + 1; else hi = mid; }
        if (lo < A.nlive && A.sorted_id[lo] == id) A.conn[(size_t)q * A.max_kf + A.sorted_slot[lo]] = 1;
    }
    SGX_THREADS_END
}

// One workgroup = one query (ids and weights in LDS) against SGX_KFDB_TILE keyframes, four at a time, a wave each.  A wave walks its keyframe's entries 64 at a time in
// ascending order: every lane binary-searches its entry's word in the query; the hits of the 64 form a mask; lane 0 adds their terms in lane order = ascending word order,
// which is the order in which L1Scoring::score's merge loop meets them (ScoringObject.cpp:34-59).  The sum is a double, rounded to float only at the end (:133, :249).
// Every sharing keyframe is scored here; the 0.8 gate, which needs the maximum over all keyframes, is applied afterwards to terms that are then already located.
SGX_KERNEL(256) k_kfdb_pairs(SgxKfdbArgs A)
{
    SGX_DYN_LDS(lds);
    SGX_LDS double s_term[256];
    SGX_LDS int s_word[256];
    SGX_LDS unsigned long long s_mask[4];
    SGX_LDS double s_sum[4];
    SGX_LDS int s_n[4], s_first[4];
    const int q = (int)blockIdx.y, tile = (int)blockIdx.x;
    const int nq = sgx_kfdb_qlen(A, q);
    double *qw = (double *)lds; int *qid = (int *)(lds + (size_t)A.max_qw * 8);
    SGX_THREADS_BEGIN(tid)
    for (int i = tid; i < nq; i += 256) { qid[i] = A.q_ids[(size_t)q * A.q_pitch + i]; qw[i] = A.q_w[(size_t)q * A.q_pitch + i]; }
    SGX_THREADS_END
    SGX_SYNC();
    for (int round = 0; round < SGX_KFDB_TILE / 4; round++) {
        const int s0 = tile * SGX_KFDB_TILE + round * 4;
        if (s0 >= A.nslots) break;
        int longest = 0;
        for (int w = 0; w < 4; w++) if (s0 + w < A.nslots && A.cnt[s0 + w] > longest) longest = A.cnt[s0 + w];
        SGX_THREADS_BEGIN(tid)
        if ((tid & 63) == 0) { const int w = tid >> 6; s_mask[w] = 0ull; s_sum[w] = 0.0; s_n[w] = 0; s_first[w] = INT_MAX; }
        SGX_THREADS_END
        SGX_SYNC();
        for (int c = 0; c < longest && nq > 0; c += 64) {
            SGX_THREADS_BEGIN(tid)
            const int w = tid >> 6, lane = tid & 63, s = s0 + w, e = c + lane;
            if (s < A.nslots && e < A.cnt[s]) {
                const size_t at = (size_t)A.off[s] + e;
                const int word = A.ent_id[at];
                int lo = 0, hi = nq;
                while (lo < hi) { const int mid = (lo + hi) >> 1; if (qid[mid] < word) lo = mid + 1; else hi = mid; }
                if (lo < nq && qid[lo] == word) {
                    const double vi = qw[lo], wi = A.ent_w[at];                     // v1 = the query, v2 = the keyframe (:133, :249)
                    s_term[tid] = fabs(vi - wi) - fabs(vi) - fabs(wi);
                    s_word[tid] = word;
                    sgx_atomic_or(&s_mask[w], 1ull << lane);
                }
            }
            SGX_THREADS_END
            SGX_SYNC();
            SGX_THREADS_BEGIN(tid)
            if ((tid & 63) == 0) {
                const int w = tid >> 6;
                unsigned long long m = s_mask[w];
                if (m) {
                    s_n[w] += (int)SGX_POPCLL(m);
                    if (s_first[w] == INT_MAX) s_first[w] = s_word[tid + __builtin_ctzll(m)];
                    double sum = s_sum[w];
                    while (m) { sum += s_term[tid + __builtin_ctzll(m)]; m &= m - 1; }
                    s_sum[w] = sum; s_mask[w] = 0ull;
                }
            }
            SGX_THREADS_END
            SGX_SYNC();
        }
        SGX_THREADS_BEGIN(tid)
        if ((tid & 63) == 0 && s0 + (tid >> 6) < A.nslots) {
            const int w = tid >> 6; const size_t o = (size_t)q * A.max_kf + s0 + w;
            A.words[o] = s_n[w]; A.first[o] = s_first[w];
            A.score[o] = (float)(-s_sum[w] / 2.0);                                  // ScoringObject.cpp:65, then float si = ...
        }
        SGX_THREADS_END
        SGX_SYNC();
    }
}

// lKFsSharingWords: every keyframe with a common word, for a loop query without the connected ones (:93-102); maxCommonWords over that list (:113-118, :228-233)
SGX_DEV bool sgx_kfdb_listed(const SgxKfdbArgs &A, size_t o) { return A.words[o] > 0 && !(A.mode == SGX_KFDB_LOOP && A.conn[o]); }

SGX_KERNEL(256) k_kfdb_gate(SgxKfdbArgs A)
{
    SGX_LDS int s_share, s_max;
    const int q = (int)blockIdx.x;
    SGX_THREADS_BEGIN(tid)
    if (tid == 0) { s_share = 0; s_max = 0; }
    SGX_THREADS_END
    SGX_SYNC();
    SGX_THREADS_BEGIN(tid)
    int share = 0, mx = 0;
    for (int s = tid; s < A.nslots; s += 256) {
        const size_t o = (size_t)q * A.max_kf + s;
        if (sgx_kfdb_listed(A, o)) { share++; if (A.words[o] > mx) mx = A.words[o]; }
        else if (A.words[o] > 0) A.words[o] = 1;                                    // a connected keyframe's mnLoopWords is reset at every word it shares (:93-102)
    }
    if (share) { sgx_atomic_add(&s_share, share); sgx_atomic_max(&s_max, mx); }
    SGX_THREADS_END
    SGX_SYNC();
    SGX_THREADS_BEGIN(tid)
    if (tid == 0) {
        SgxKfdbReport R;
        R.n_sharing = s_share; R.max_common_words = s_max;
        R.min_common_words = (int)((float)s_max * 0.8f);                            // int minCommonWords = maxCommonWords*0.8f (:120, :235)
        R.n_scores = 0; R.n_score_and_match = 0; R.best_acc_score = 0.0f; R.min_score_to_retain = 0.0f; R.n_candidates = 0;
        R.status = sgx_kfdb_qvalid(A, q) ? 0 : -1;                                  // SGX_ERR_INVALID
        A.report[q] = R;
        A.n_cand[q] = 0;
    }
    SGX_THREADS_END
}

// mRelocScore is written only for a keyframe that passes the word gate (:246-250) and read for every neighbour that shares a word (:273-276): a neighbour that shared
// a word but failed the gate contributes what an EARLIER query left in it.  Query q of a batch must see the state queries 0 .. q-1 left: one lane per keyframe walks the
// queries in order with the last score in a register; score[q][s] becomes mRelocScore of s as query q's accumulation reads it, reloc[s] what the batch leaves behind.
SGX_KERNEL(256) k_kfdb_stale(SgxKfdbArgs A)
{
    SGX_THREADS_BEGIN(tid)
    const int s = (int)blockIdx.x * 256 + tid;
    if (s < A.nslots) {
        float r = A.reloc[s];
        for (int q = 0; q < A.Q; q++) {
            const size_t o = (size_t)q * A.max_kf + s;
            if (A.words[o] > A.report[q].min_common_words) r = A.score[o]; else A.score[o] = r;
        }
        A.reloc[s] = r;
    }
    SGX_THREADS_END
}

SGX_KERNEL(256) k_kfdb_select(SgxKfdbArgs A)
{
    SGX_LDS int s_scores, s_list;
    const int q = (int)blockIdx.x;
    const size_t q0 = (size_t)q * A.max_kf;
    const bool loop = A.mode == SGX_KFDB_LOOP;
    const int minw = A.report[q].min_common_words;
    const float min_score = loop ? A.min_score[q] : 0.0f;
    SGX_THREADS_BEGIN(tid)
    if (tid == 0) { s_scores = 0; s_list = 0; }
    SGX_THREADS_END
    SGX_SYNC();
    // the scored keyframes (:129, :246), lScoreAndMatch (loop: si >= minScore, :136) and their place in it
    SGX_THREADS_BEGIN(tid)
    int scored = 0, listed = 0;
    for (int s = tid; s < A.nslots; s += 256) {
        const size_t o = q0 + s;
        const bool sc = sgx_kfdb_listed(A, o) && A.words[o] > minw;
        if (loop && !sc) A.score[o] = 0.0f;                                         // mLoopScore is never read where this query has not written it
        const bool in = sc && (!loop || A.score[o] >= min_score);
        A.key[o] = in ? ((unsigned long long)(unsigned)A.first[o] << 32) | (unsigned)A.seq[s] : ~0ull;
        A.firstrank[o] = INT_MAX;
        scored += sc; listed += in;
    }
    if (scored) sgx_atomic_add(&s_scores, scored);
    if (listed) sgx_atomic_add(&s_list, listed);
    SGX_THREADS_END
    SGX_SYNC();
    const int M = s_list;
    SGX_THREADS_BEGIN(tid)
    if (tid == 0) { A.report[q].n_scores = s_scores; A.report[q].n_score_and_match = M; }
    SGX_THREADS_END
    if (M == 0) return;                                                             // lKFsSharingWords empty (:107-108, :224-225) or lScoreAndMatch empty (:141-142, :255-256)
    // rank in lScoreAndMatch = keys below this one (pairwise; the list is tens of keyframes), then the covisibility accumulation of :148-173 / :262-287 for that keyframe
    SGX_THREADS_BEGIN(tid)
    for (int s = tid; s < A.nslots; s += 256) {
        const unsigned long long k = A.key[q0 + s];
        if (k == ~0ull) continue;
        int rank = 0;
        for (int t = 0; t < A.nslots; t++) rank += A.key[q0 + t] < k;
        float best_score = A.score[q0 + s], acc = best_score; int best = s;
        for (int j = 0; j < SGX_KFDB_COVIS; j++) {
            const int nb = A.covis[s * SGX_KFDB_COVIS + j];
            if (nb < 0) continue;
            const size_t o = q0 + nb;
            if (loop ? !(sgx_kfdb_listed(A, o) && A.words[o] > minw) : !(A.words[o] > 0)) continue;      // :159 / :273
            const float sc = A.score[o];
            acc += sc;
            if (sc > best_score) { best = nb; best_score = sc; }
        }
        A.order[q0 + rank] = s; A.acc[q0 + rank] = acc; A.best[q0 + rank] = best;
    }
    SGX_THREADS_END
    SGX_SYNC();
    SGX_THREADS_BEGIN(tid)
    if (tid == 0) {
        float best_acc = min_score;                                                 // minScore for a loop query, 0 for relocalisation (:145, :259)
        for (int r = 0; r < M; r++) if (A.acc[q0 + r] > best_acc) best_acc = A.acc[q0 + r];
        A.report[q].best_acc_score = best_acc;
        A.report[q].min_score_to_retain = 0.75f * best_acc;
    }
    SGX_THREADS_END
    SGX_SYNC();
    // retained entries (strictly above 0.75 best); of several entries naming the same pBestKF the first in list order stands (spAlreadyAddedKF)
    SGX_THREADS_BEGIN(tid)
    const float retain = A.report[q].min_score_to_retain;
    for (int r = tid; r < M; r += 256)
        if (A.acc[q0 + r] > retain) sgx_atomic_min_i32(&A.firstrank[q0 + A.best[q0 + r]], r);
    SGX_THREADS_END
    SGX_SYNC();
    SGX_THREADS_BEGIN(tid)
    if (tid == 0) {
        int n = 0;
        for (int r = 0; r < M; r++) { const int b = A.best[q0 + r]; if (A.firstrank[q0 + b] == r) A.cand[q0 + n++] = A.kf_id[b]; }
        A.report[q].n_candidates = n; A.n_cand[q] = n;
    }
    SGX_THREADS_END
}

// min over the listed keyframes of the float-cast score, starting from the float 1 (src/sg-slam/src/LoopClosing.cc:126-138), after k_kfdb_pairs on query 0
SGX_KERNEL(64) k_kfdb_min_score(SgxKfdbArgs A, const int *slots, int n, float *out)
{
    SGX_THREADS_BEGIN(tid)
    if (tid == 0) {
        float m = 1.0f;
        for (int i = 0; i < n; i++) { const float sc = A.score[slots[i]]; if (sc < m) m = sc; }
        *out = m;
    }
    SGX_THREADS_END
}
