// sgx_newpoints_kernels.h — LocalMapping::CreateNewMapPoints (src/sg-slam/src/LocalMapping.cc:207-452) over the device-resident keyframe store (sgx_kfstore, include/sgx.h):
//   k_create_new_map_points     one workgroup per query walks the query's neighbours in order; per neighbour the baseline gate (:244-261), ComputeF12 (:536-553), the
//                               epipole (ORBmatcher.cc:666-674), the join of the two keyframes' node lists, SearchForTriangulation (sgx_tri_search_node), the per-pair body
//                               (sgx_triangulate_pair), the commit in ascending idx1 (:433-447) and the two MapPoint post-steps of every new point (:442-444).
// The neighbours of a query are a serial chain (a keypoint filled by neighbour i is skipped for neighbour i + 1), the queries are independent: no global synchronisation,
// no per-neighbour launch, nothing read back.  Every count is formed by an order-preserving scan over fixed chunks, never by the order in which waves finish, so two runs
// are byte-identical.  Phase style of sgx_rt.h: the same source runs in the emulator.
#pragma once
#include "sgx_match2_bodies.h"
#include "../../include/sgx.h"

// the store as the kernel sees it: slot s holds keyframe slot_id[s] (-1 free); every per-keypoint array has pitch cap
struct SgxKfStoreDev {
    int max_kf, cap, nlevels;
    const int *slot_id;                      /* [max_kf] */
    const int *meta;                         /* [max_kf][2]: keypoints, vocabulary nodes */
    const uint8_t *keys_un, *keys;           /* mvKeysUn, mvKeys (28-byte cv::KeyPoint) */
    const uint32_t *desc;
    const float *uright, *depth;
    const int *items;                        /* feature indices grouped by node (FeatureVector order) */
    const int *node_id, *node_start;         /* [max_kf][cap], [max_kf][cap + 1]: the nodes ascending, and where each begins in items */
    const float *Tcw;                        /* [max_kf][12], row-major 3 x 4 */
    float fx, fy, cx, cy, bf;
    float KinvT[9], Kinv[9];                 /* K1.t().inv() and K2.inv(): OpenCV's closed 3 x 3 form, formed once on the host in double */
    SgxScales scale, sigma2;
};

struct SgxNewPointsArgs {
    SgxKfStoreDev S;
    const int *cur_ids, *nb_off, *nb_ids, *first_new_id;
    const float *median_depth;               /* NULL: the stereo / RGB-D gate */
    int *rows;                               /* in/out, pitch cap: query q owns rows q + nb_off[q] (current keyframe) .. q + nb_off[q + 1] (its neighbours in order) */
    int *n_new, *new_kf2, *new_idx1, *new_idx2;
    float *new_x3d; uint32_t *new_desc; float *new_normal, *new_min_dist, *new_max_dist;
    sgx_newpoints_report *report;
    int *pair_idx1, *pair_idx2; uint8_t *pair_ok;       /* optional, one row of pitch cap per neighbour */
    int *w_match12; uint8_t *w_matched2; int *w_pairs; uint8_t *w_ok; float *w_x3d;      /* workspace, per query: cap, cap, 2 cap, cap, 3 cap */
};

// Ow = -Rwc * tcw with Rwc = Rcw.t() stored (KeyFrame::SetPose, KeyFrame.cc:71-79): a cv::gemm without flags: float products left to right, alpha = -1 last
SGX_DEV void sgx_np_centre_float(const float *T, float *Ow)
{
    for (int i = 0; i < 3; i++) { const float d = T[i] * T[3] + T[4 + i] * T[7] + T[8 + i] * T[11]; Ow[i] = (float)((double)d * -1.0); }
}
// the centre sgx_triangulate_new_map_points forms (camera_centre, sgx_match2.cpp): -R.t() * t as one expression, the transpose flag taking the double accumulation
SGX_DEV void sgx_np_centre_double(const float *T, float *Ow)
{
    for (int i = 0; i < 3; i++) { double s = 0; for (int k = 0; k < 3; k++) s += (double)T[4 * k + i] * (double)T[4 * k + 3]; Ow[i] = (float)(s * -1.0); }
}
// C = A * B, 3 x 3, cv::gemm without flags: float products left to right, (float)(double(dot) * 1.0)
SGX_DEV void sgx_np_mul33(const float *A, const float *B, float *C)
{
    for (int r = 0; r < 3; r++) for (int c = 0; c < 3; c++) { const float d = A[3 * r] * B[c] + A[3 * r + 1] * B[3 + c] + A[3 * r + 2] * B[6 + c]; C[3 * r + c] = (float)((double)d * 1.0); }
}

// LocalMapping::ComputeF12 (:536-553) for the poses T1, T2 (3 x 4): R12 = R1w * R2w.t() and -R1w * R2w.t() are gemms with a transposed operand (double accumulation,
// alpha last), (-R1w * R2w.t()) * t2w + t1w one gemm without flags with beta = 1, then K1.t().inv() * t12x * R12 * K2.inv() left to right
SGX_DEV void sgx_np_compute_f12(const float *T1, const float *T2, const float *KinvT, const float *Kinv, float *F)
{
    float R12[9], nR12[9], t12[3], tx[9], M1[9], M2[9];
    for (int r = 0; r < 3; r++) for (int c = 0; c < 3; c++) {
        double s = 0; for (int k = 0; k < 3; k++) s += (double)T1[4 * r + k] * (double)T2[4 * c + k];
        R12[3 * r + c] = (float)(s * 1.0); nR12[3 * r + c] = (float)(s * -1.0);
    }
    for (int r = 0; r < 3; r++) {
        const float d = nR12[3 * r] * T2[3] + nR12[3 * r + 1] * T2[7] + nR12[3 * r + 2] * T2[11];
        t12[r] = (float)((double)d * 1.0 + 1.0 * (double)T1[4 * r + 3]);
    }
    tx[0] = 0.f; tx[1] = -t12[2]; tx[2] = t12[1]; tx[3] = t12[2]; tx[4] = 0.f; tx[5] = -t12[0]; tx[6] = -t12[1]; tx[7] = t12[0]; tx[8] = 0.f;      // SkewSymmetricMatrix
    sgx_np_mul33(KinvT, tx, M1); sgx_np_mul33(M1, R12, M2); sgx_np_mul33(M2, Kinv, F);
}

// exclusive scan of s_cnt[0..256) by one thread; returns the total
SGX_DEV int sgx_np_scan256(int *cnt)
{
    int run = 0;
    for (int t = 0; t < 256; t++) { const int x = cnt[t]; cnt[t] = run; run += x; }
    return run;
}

SGX_KERNEL(256) k_create_new_map_points(SgxNewPointsArgs A)
{
    SGX_LDS SgxTriArgs T;
    SGX_LDS SgxNewPointArgs N;
    SGX_LDS int s_slot1, s_slot2, s_go, s_npairs, s_nnew, s_add, s_total, s_cnt[256];
    SGX_LDS float s_Ow1[3], s_Ow2[3];
    const SgxKfStoreDev &S = A.S;
    const int q = (int)blockIdx.x, cap = S.cap;
    const int cur = A.cur_ids[q], nb0 = A.nb_off[q], nnb = A.nb_off[q + 1] - nb0, first = A.first_new_id[q];
    int *row1 = A.rows + (size_t)(q + nb0) * cap;
    int *w_match12 = A.w_match12 + (size_t)q * cap, *w_pairs = A.w_pairs + (size_t)q * cap * 2;
    uint8_t *w_matched2 = A.w_matched2 + (size_t)q * cap, *w_ok = A.w_ok + (size_t)q * cap;
    float *w_x3d = A.w_x3d + (size_t)q * cap * 3;
    SGX_THREADS_BEGIN(tid)
    if (tid == 0) { s_slot1 = -1; s_nnew = 0; }
    SGX_THREADS_END
    SGX_SYNC();
    SGX_THREADS_BEGIN(tid)
    if (cur >= 0) for (int s = tid; s < S.max_kf; s += 256) if (S.slot_id[s] == cur) s_slot1 = s;             // an id stands in one slot at most
    SGX_THREADS_END
    SGX_SYNC();
    const int slot1 = s_slot1;
    for (int j = 0; j < nnb; j++) {
        const int kf2 = A.nb_ids[nb0 + j];
        int *row2 = row1 + (size_t)(j + 1) * cap;
        SGX_THREADS_BEGIN(tid)
        if (tid == 0) s_slot2 = -1;
        SGX_THREADS_END
        SGX_SYNC();
        SGX_THREADS_BEGIN(tid)
        if (kf2 >= 0 && kf2 != cur) for (int s = tid; s < S.max_kf; s += 256) if (S.slot_id[s] == kf2) s_slot2 = s;
        SGX_THREADS_END
        SGX_SYNC();
        SGX_THREADS_BEGIN(tid)
        if (tid == 0) {
            sgx_newpoints_report r;
            r.status = SGX_NEWPOINTS_PROCESSED; r.kf2 = kf2; r.n_pairs = 0; r.n_new = 0; r.baseline = 0.f;
            for (int i = 0; i < 9; i++) r.F12[i] = 0.f;
            for (int i = 0; i < 3; i++) { r.Ow1[i] = 0.f; r.Ow2[i] = 0.f; }
            s_go = 0; s_npairs = 0; s_add = 0; s_total = 0;
            if (slot1 < 0 || s_slot2 < 0) r.status = SGX_ERR_INVALID;
            else {
                const int slot2 = s_slot2;
                const float *T1 = S.Tcw + (size_t)slot1 * 12, *T2 = S.Tcw + (size_t)slot2 * 12;
                sgx_np_centre_float(T1, s_Ow1); sgx_np_centre_float(T2, s_Ow2);
                const float b0 = s_Ow2[0] - s_Ow1[0], b1 = s_Ow2[1] - s_Ow1[1], b2 = s_Ow2[2] - s_Ow1[2];                    // vBaseline = Ow2 - Ow1
                const float baseline = (float)sqrt((double)b0 * b0 + (double)b1 * b1 + (double)b2 * b2);                   // cv::norm: double accumulation
                r.baseline = baseline;
                for (int i = 0; i < 3; i++) { r.Ow1[i] = s_Ow1[i]; r.Ow2[i] = s_Ow2[i]; }
                bool skip;
                if (!A.median_depth) skip = baseline < S.bf / S.fx;                                                        // pKF2->mb = mbf / fx
                else { const float ratio = baseline / A.median_depth[nb0 + j]; skip = (double)ratio < 0.01; }
                if (skip) r.status = SGX_NEWPOINTS_SKIPPED;
                else {
                    sgx_np_compute_f12(T1, T2, S.KinvT, S.Kinv, r.F12);
                    const int n1 = S.meta[2 * slot1], n2 = S.meta[2 * slot2];
                    T.n1 = n1; T.n2 = n2; T.nnodes = 0;
                    T.keys1 = S.keys_un + (size_t)slot1 * cap * 28; T.keys2 = S.keys_un + (size_t)slot2 * cap * 28;
                    T.desc1 = S.desc + (size_t)slot1 * cap * 8; T.desc2 = S.desc + (size_t)slot2 * cap * 8;
                    T.uright1 = S.uright + (size_t)slot1 * cap; T.uright2 = S.uright + (size_t)slot2 * cap;
                    T.has_mp1 = nullptr; T.has_mp2 = nullptr;
                    T.items1 = S.items + (size_t)slot1 * cap; T.items2 = S.items + (size_t)slot2 * cap; T.job = nullptr;
                    for (int i = 0; i < 9; i++) T.F12[i] = r.F12[i];
                    {                                                                                                      // the epipole, as sgx_match_search_for_triangulation
                        float C2[3];
                        for (int a = 0; a < 3; a++) {
                            const float *row = T2 + 4 * a; const float t = row[0] * s_Ow1[0] + row[1] * s_Ow1[1] + row[2] * s_Ow1[2];
                            C2[a] = (float)((double)t * 1.0 + 1.0 * (double)row[3]);
                        }
                        const float invz = 1.0f / C2[2];
                        T.ex = S.fx * C2[0] * invz + S.cx; T.ey = S.fy * C2[1] * invz + S.cy;
                    }
                    T.scale2 = S.scale; T.sigma2_2 = S.sigma2; T.only_stereo = 0; T.check_ori = 0;                         // ORBmatcher matcher(0.6, false), bOnlyStereo = false
                    T.match12 = w_match12; T.matched2 = w_matched2; T.nmatches = nullptr;
                    N.npairs = 0; N.pairs = w_pairs;
                    N.keys1_un = T.keys1; N.keys1 = S.keys + (size_t)slot1 * cap * 28; N.keys2_un = T.keys2; N.keys2 = S.keys + (size_t)slot2 * cap * 28;
                    N.ur1 = T.uright1; N.dp1 = S.depth + (size_t)slot1 * cap; N.ur2 = T.uright2; N.dp2 = S.depth + (size_t)slot2 * cap;
                    for (int i = 0; i < 16; i++) { N.Tcw1[i] = i < 12 ? T1[i] : 0.f; N.Tcw2[i] = i < 12 ? T2[i] : 0.f; }
                    sgx_np_centre_double(T1, N.Ow1); sgx_np_centre_double(T2, N.Ow2);
                    N.fx = S.fx; N.fy = S.fy; N.cx = S.cx; N.cy = S.cy; N.mbf = S.bf; N.ratio_factor = 1.5f * S.scale.s[1];
                    N.scale = S.scale; N.sigma2 = S.sigma2; N.ok = w_ok; N.x3d = w_x3d;
                    s_go = 1;
                }
            }
            A.report[nb0 + j] = r;
        }
        SGX_THREADS_END
        SGX_SYNC();
        if (!s_go) continue;
        const int slot2 = s_slot2, n1 = T.n1, n2 = T.n2;
        const int nn1 = S.meta[2 * slot1 + 1], nn2 = S.meta[2 * slot2 + 1];
        const int *id1 = S.node_id + (size_t)slot1 * cap, *id2 = S.node_id + (size_t)slot2 * cap;
        const int *st1 = S.node_start + (size_t)slot1 * (cap + 1), *st2 = S.node_start + (size_t)slot2 * (cap + 1);
        SGX_THREADS_BEGIN(tid)
        for (int i = tid; i < n1; i += 256) w_match12[i] = -1;
        for (int i = tid; i < n2; i += 256) w_matched2[i] = 0;
        SGX_THREADS_END
        SGX_SYNC();
        // the join: a node of the current keyframe that the neighbour holds too is one job; the vbMatched2 lock couples only features of one node, so the jobs are independent
        SGX_THREADS_BEGIN(tid)
        for (int a = tid; a < nn1; a += 256) {
            const int id = id1[a];
            int lo = 0, hi = nn2;
            while (lo < hi) { const int mid = (lo + hi) >> 1; if (id2[mid] < id) lo = mid + 1; else hi = mid; }
            if (lo < nn2 && id2[lo] == id) sgx_tri_search_node(T, (const int *)row1, (const int *)row2, st1[a], st1[a + 1], st2[lo], st2[lo + 1], &s_total, (int *)nullptr);
        }
        SGX_THREADS_END
        SGX_SYNC();
        // vMatchedPairs in ascending idx1 (ORBmatcher.cc:815-822): thread t owns the indices [t * chunk, (t + 1) * chunk)
        const int chunk = (n1 + 255) / 256;
        SGX_THREADS_BEGIN(tid)
        int c = 0;
        for (int i = tid * chunk; i < n1 && i < (tid + 1) * chunk; i++) c += w_match12[i] >= 0;
        s_cnt[tid] = c;
        SGX_THREADS_END
        SGX_SYNC();
        SGX_THREADS_BEGIN(tid)
        if (tid == 0) s_npairs = sgx_np_scan256(s_cnt);
        SGX_THREADS_END
        SGX_SYNC();
        SGX_THREADS_BEGIN(tid)
        int o = s_cnt[tid];
        for (int i = tid * chunk; i < n1 && i < (tid + 1) * chunk; i++) if (w_match12[i] >= 0) { w_pairs[2 * o] = i; w_pairs[2 * o + 1] = w_match12[i]; o++; }
        SGX_THREADS_END
        SGX_SYNC();
        const int npairs = s_npairs;
        SGX_THREADS_BEGIN(tid)
        for (int k = tid; k < npairs; k += 256) {
            float X[3] = { 0.f, 0.f, 0.f };
            const int i1 = w_pairs[2 * k], i2 = w_pairs[2 * k + 1];
            const uint8_t ok = sgx_triangulate_pair(N, i1, i2, X);
            w_ok[k] = ok;
            w_x3d[3 * k] = ok ? X[0] : 0.f; w_x3d[3 * k + 1] = ok ? X[1] : 0.f; w_x3d[3 * k + 2] = ok ? X[2] : 0.f;
            if (A.pair_idx1) A.pair_idx1[(size_t)(nb0 + j) * cap + k] = i1;
            if (A.pair_idx2) A.pair_idx2[(size_t)(nb0 + j) * cap + k] = i2;
            if (A.pair_ok) A.pair_ok[(size_t)(nb0 + j) * cap + k] = ok;
        }
        SGX_THREADS_END
        SGX_SYNC();
        // the commit (:433-447) in pair order = ascending idx1
        const int chunk2 = (npairs + 255) / 256;
        SGX_THREADS_BEGIN(tid)
        int c = 0;
        for (int k = tid * chunk2; k < npairs && k < (tid + 1) * chunk2; k++) c += w_ok[k];
        s_cnt[tid] = c;
        SGX_THREADS_END
        SGX_SYNC();
        SGX_THREADS_BEGIN(tid)
        if (tid == 0) s_add = sgx_np_scan256(s_cnt);
        SGX_THREADS_END
        SGX_SYNC();
        SGX_THREADS_BEGIN(tid)
        int o = s_nnew + s_cnt[tid];
        for (int k = tid * chunk2; k < npairs && k < (tid + 1) * chunk2; k++) {
            if (!w_ok[k] || o >= cap) continue;                               // o < n1 <= cap: every accepted pair fills a free keypoint of the current keyframe
            const int i1 = w_pairs[2 * k], i2 = w_pairs[2 * k + 1];
            const size_t g = (size_t)q * cap + o;
            row1[i1] = first + o; row2[i2] = first + o;
            A.new_kf2[g] = kf2; A.new_idx1[g] = i1; A.new_idx2[g] = i2;
            const float X[3] = { w_x3d[3 * k], w_x3d[3 * k + 1], w_x3d[3 * k + 2] };
            A.new_x3d[3 * g] = X[0]; A.new_x3d[3 * g + 1] = X[1]; A.new_x3d[3 * g + 2] = X[2];
            // mObservations in ascending keyframe id (rule 1 of the covisibility section)
            const bool cur_first = cur < kf2;
            uint32_t d[16]; float oc[6];
            const uint32_t *da = cur_first ? T.desc1 + (size_t)i1 * 8 : T.desc2 + (size_t)i2 * 8, *db = cur_first ? T.desc2 + (size_t)i2 * 8 : T.desc1 + (size_t)i1 * 8;
            for (int w = 0; w < 8; w++) { d[w] = da[w]; d[8 + w] = db[w]; }
            for (int a = 0; a < 3; a++) { oc[a] = cur_first ? s_Ow1[a] : s_Ow2[a]; oc[3 + a] = cur_first ? s_Ow2[a] : s_Ow1[a]; }
            // ComputeDistinctiveDescriptors over the two observations: the row with the least median, the first on ties
            int key = 0x7FFFFFFF;
            for (int i = 0; i < 2; i++) { const int m = (sgx_mp_row_median(d, 2, i, (int)(0.5 * (double)(2 - 1))) << 16) | i; if (m < key) key = m; }
            for (int w = 0; w < 8; w++) A.new_desc[8 * g + w] = d[8 * (key & 0xFFFF) + w];
            // UpdateNormalAndDepth: mpRefKF = the current keyframe, level = kp1.octave
            const int oct1 = ((const int *)(T.keys1 + (size_t)i1 * 28))[5];
            sgx_mp_normal_depth(X, oc, 2, s_Ow1, S.scale.s[oct1], S.scale.s[S.nlevels - 1], A.new_normal + 3 * g, A.new_min_dist + g, A.new_max_dist + g);
            o++;
        }
        SGX_THREADS_END
        SGX_SYNC();
        SGX_THREADS_BEGIN(tid)
        if (tid == 0) { A.report[nb0 + j].n_pairs = npairs; A.report[nb0 + j].n_new = s_add; s_nnew += s_add; }
        SGX_THREADS_END
        SGX_SYNC();
    }
    SGX_THREADS_BEGIN(tid)
    if (tid == 0) A.n_new[q] = s_nnew;
    SGX_THREADS_END
}
