// sgx_voc_kernels.h — the DBoW2 vocabulary descent of Frame::ComputeBoW / KeyFrame::ComputeBoW (src/sg-slam/src/Frame.cc:422-429:
// mpORBvocabulary->transform(vCurrentDesc, mBowVec, mFeatVec, 4)), per feature:
//   TemplatedVocabulary::transform(feature, word_id, weight, nid, levelsup)    src/sg-slam/Thirdparty/DBoW2/DBoW2/TemplatedVocabulary.h:1231-1273
//   FORB::distance                                                              src/sg-slam/Thirdparty/DBoW2/DBoW2/FORB.cpp:81-101
// One thread per feature walks the k-ary tree from the root: at every level the Hamming distance to each child's descriptor, first minimum wins (strict '<' in child order).
// The tree lives in HBM as flat arrays (children as CSR in insertion order, descriptors as 8 dwords per node); ORBvoc (k = 10, L = 6, 1.1 M nodes) is 35 MB of descriptors,
// a frame's 1 000 features touch 60 k of them.  B frames per launch (grid.y), ragged counts.
#pragma once
#include "sgx_match_common.h"
#include <limits.h>

struct SgxVocDev {
    int L, nnodes;
    const int *child_start, *child_idx, *word_id;
    const uint32_t *desc;
    const double *weight;
};

SGX_KERNEL(256) k_voc_transform(SgxVocDev V, int levelsup, const uint8_t *desc, size_t desc_pitch, const int *n_arr, int n_fixed, int cap,
                                int *word_id, double *weight, int *feat_node)
{
    SGX_THREADS_BEGIN(tid)
    const int b = (int)blockIdx.y, i = (int)blockIdx.x * 256 + tid;
    const int n = n_arr ? min(n_arr[b], cap) : n_fixed;
    if (i < n) {
        const uint32_t *f = (const uint32_t *)(desc + (size_t)b * desc_pitch) + (size_t)i * 8;
        uint32_t fv[8];
#pragma unroll
        for (int k = 0; k < 8; k++) fv[k] = f[k];
        const int nid_level = V.L - levelsup;
        int nid = 0; bool nid_set = nid_level <= 0;
        int final_id = 0, level = 0;
        for (;;) {
            ++level;
            const int s = V.child_start[final_id], e = V.child_start[final_id + 1];
            int best = V.child_idx[s], best_d = sgx_hamming256(fv, V.desc + (size_t)best * 8);
            for (int c = s + 1; c < e; c++) {
                const int id = V.child_idx[c];
                const int d = sgx_hamming256(fv, V.desc + (size_t)id * 8);
                if (d < best_d) { best_d = d; best = id; }
            }
            final_id = best;
            if (level == nid_level) { nid = final_id; nid_set = true; }
            if (V.child_start[final_id + 1] <= V.child_start[final_id]) break;       // isLeaf()
        }
        if (!nid_set) nid = final_id;             // the reference leaves *nid unassigned when the descent ends above level L - levelsup; the leaf is the evident intent
        const double w = V.weight[final_id];
        const size_t o = (size_t)b * cap + i;
        word_id[o] = V.word_id[final_id]; weight[o] = w; feat_node[o] = w > 0 ? nid : -1;
    }
    SGX_THREADS_END
}

// ---- the BowVector of one frame from its per-feature (word, weight) arrays: what the std::map of TemplatedVocabulary::transform ends up holding --------------------------
// One workgroup per frame.  The words sit in LDS (stopped ones, !(w > 0), as INT_MAX: :1170); a feature is the head of its word if no earlier feature has the word; a
// head's place in the map is the number of heads with a smaller word (pairwise, stable by construction), its weight the sum over its word's features in feature order
// (addWeight, BowVector.cpp:33-45) or the first one's alone (addIfNotExist :49-57 for IDF / BINARY).  Then the /nd step of :1177-1183 or BowVector::normalize (:61-86) with
// the norm summed by one lane in ascending word order.
SGX_KERNEL(256) k_voc_bow(int cap, int tf, int must, int l2, const int *n_arr, const int *word_id, const double *weight, int *bow_ids, double *bow_w, int *bow_n)
{
    SGX_DYN_LDS(lds);
    SGX_LDS int s_m;
    SGX_LDS double s_norm;
    const int b = (int)blockIdx.x;
    int n = n_arr[b]; if (n > cap) n = cap; if (n < 0) n = 0;
    int *wl = (int *)lds; unsigned char *head = lds + (size_t)cap * 4;
    const size_t r0 = (size_t)b * cap;
    SGX_THREADS_BEGIN(tid)
    if (tid == 0) s_m = 0;
    for (int i = tid; i < n; i += 256) wl[i] = weight[r0 + i] > 0 ? word_id[r0 + i] : INT_MAX;
    SGX_THREADS_END
    SGX_SYNC();
    SGX_THREADS_BEGIN(tid)
    for (int i = tid; i < n; i += 256) {
        const int w = wl[i]; bool h = w != INT_MAX;
        for (int j = 0; h && j < i; j++) h = wl[j] != w;
        head[i] = h ? 1 : 0;
    }
    SGX_THREADS_END
    SGX_SYNC();
    SGX_THREADS_BEGIN(tid)
    int heads = 0;
    for (int i = tid; i < n; i += 256) {
        if (!head[i]) continue;
        const int w = wl[i]; int rank = 0; double v = weight[r0 + i];
        for (int j = 0; j < n; j++) {
            rank += head[j] && wl[j] < w;
            if (tf && j > i && wl[j] == w) v += weight[r0 + j];
        }
        bow_ids[r0 + rank] = w; bow_w[r0 + rank] = v; heads++;
    }
    if (heads) sgx_atomic_add(&s_m, heads);
    SGX_THREADS_END
    SGX_SYNC();
    const int m = s_m;
    SGX_THREADS_BEGIN(tid)
    if (tid == 0) {
        bow_n[b] = m;
        double norm = 0.0;
        if (must) {
            if (!l2) for (int i = 0; i < m; i++) norm += fabs(bow_w[r0 + i]);
            else { for (int i = 0; i < m; i++) norm += bow_w[r0 + i] * bow_w[r0 + i]; norm = sqrt(norm); }
        } else if (tf) norm = (double)m;
        s_norm = norm;
    }
    SGX_THREADS_END
    SGX_SYNC();
    SGX_THREADS_BEGIN(tid)
    const double norm = s_norm;
    if (norm > 0.0) for (int i = tid; i < m; i += 256) bow_w[r0 + i] /= norm;
    SGX_THREADS_END
}
