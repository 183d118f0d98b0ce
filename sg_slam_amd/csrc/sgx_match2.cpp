// sgx_match2.cpp — host side of the LocalMapping / LoopClosing / initialiser matcher gates and the MapPoint post-steps (include/sgx.h), host pointers, synchronous.
// Every entry: validate, build the kernel argument struct, stage each buffer where its argument is set (SgxStaging, sgx_stage.h), launch, read back.
// Reference behaviour: src/sg-slam/src/ORBmatcher.cc:659-827, :1649-1665.
#include "sgx_match2_kernels.h"
#include "sgx_host_args.h"
#include "sgx_stage.h"
#include "../../include/sgx.h"
#ifdef SGX_DEBUG_TAPS
#include "../../include/sgx_debug.h"      // test / tuning taps: compiled into tests/taps/libsgx_taps.so and the emulator only
#endif
#include <stdio.h>
#include <string.h>
#include <algorithm>
#include <vector>


extern "C" int sgx_hamming_matrix_dev(const uint8_t *d_desc_a, int na, const uint8_t *d_desc_b, int nb, uint16_t *d_out, void *stream)
{
    if (na < 0 || nb < 0 || (na > 0 && !d_desc_a) || (nb > 0 && !d_desc_b) || (na > 0 && nb > 0 && !d_out)) return SGX_ERR_INVALID;
    if (na == 0 || nb == 0) return SGX_OK;
    SGX_LAUNCH(k_hamming_matrix, dim3((nb + 15) / 16, (na + 15) / 16), dim3(256), (sgx_stream_t)stream, (const uint32_t *)d_desc_a, na, (const uint32_t *)d_desc_b, nb, d_out);
    SGX_CHECK_HIP(hipGetLastError());
    return SGX_OK;
}

extern "C" int sgx_hamming_matrix(const uint8_t *desc_a, int na, const uint8_t *desc_b, int nb, uint16_t *out)
{
    if (na < 0 || nb < 0 || (na > 0 && !desc_a) || (nb > 0 && !desc_b) || (na > 0 && nb > 0 && !out)) return SGX_ERR_INVALID;
    if (na == 0 || nb == 0) return SGX_OK;
    SgxStaging st(SGX_STAGE_SHARED);
    const uint8_t *dA = st.in(desc_a, (size_t)na * 32), *dB = st.in(desc_b, (size_t)nb * 32);
    uint16_t *dO = st.out<uint16_t>((size_t)na * nb);
    if (st.rc != SGX_OK) return st.rc;
    const int rc = sgx_hamming_matrix_dev(dA, na, dB, nb, dO, nullptr);
    if (rc != SGX_OK) return rc;
    st.back(out, dO, (size_t)na * nb);
    return st.rc;
}

// FeatureVector (std::map<NodeId, std::vector<unsigned>>) of one keyframe from the per-feature node ids: nodes ascending, feature indices ascending inside a node
static void group_by_node(const int32_t *node, int n, std::vector<int> &items, std::vector<int> &ids, std::vector<int> &start)
{
    items.clear(); ids.clear(); start.clear();
    for (int i = 0; i < n; i++) if (node[i] >= 0) items.push_back(i);
    std::stable_sort(items.begin(), items.end(), [&](int x, int y) { return node[x] < node[y]; });
    for (size_t q = 0; q < items.size(); q++) if (q == 0 || node[items[q]] != node[items[q - 1]]) { ids.push_back(node[items[q]]); start.push_back((int)q); }
    start.push_back((int)items.size());
}

// the lock-step walk of the two FeatureVectors (ORBmatcher.cc:692-776, :184-281): one job (begin1, end1, begin2, end2 into items1 / items2) per node both keyframes have
static std::vector<int> common_node_jobs(const int32_t *node1, int n1, std::vector<int> &items1, const int32_t *node2, int n2, std::vector<int> &items2)
{
    std::vector<int> id1, st1, id2, st2, job;
    group_by_node(node1, n1, items1, id1, st1); group_by_node(node2, n2, items2, id2, st2);
    for (size_t a = 0, b = 0; a < id1.size() && b < id2.size();) {
        if (id1[a] == id2[b]) { job.push_back(st1[a]); job.push_back(st1[a + 1]); job.push_back(st2[b]); job.push_back(st2[b + 1]); a++; b++; }
        else if (id1[a] < id2[b]) a++; else b++;
    }
    if (items1.empty()) items1.push_back(0);          // the kernels get no empty buffer: one unused element
    if (items2.empty()) items2.push_back(0);
    if (job.empty()) job.push_back(0);
    return job;
}

// keypoint octaves index the per-level tables of the kernel arguments (12 entries): reject frames whose octaves fall outside the extractor's levels
static bool octaves_ok(const sgx_keypoint *k, int n, int nlevels)
{
    for (int i = 0; i < n; i++) if (k[i].octave < 0 || k[i].octave >= nlevels) return false;
    return true;
}

// Ow = -R.t() * t as one cv::Mat expression (ORBmatcher.cc:305, :994, :1480): the transpose flag takes the generic gemm, which accumulates in double and applies
// alpha = -1 last.  Rows of R are rstride floats apart, elements of t tstride.
static void camera_centre(const float *R, int rstride, const float *t, int tstride, float Ow[3])
{
    for (int i = 0; i < 3; i++) {
        double s = 0; for (int k = 0; k < 3; k++) s += (double)R[rstride * k + i] * (double)t[tstride * k];
        Ow[i] = (float)(s * -1.0);
    }
}

// Frame::mGrid / KeyFrame::mGrid (KeyFrame.cc:39-47 copies Frame::mGrid, built by AssignFeaturesToGrid / PosInGrid with round(), Frame.cc:257-272, :409-419) as CSR:
// cell (ix, iy) -> ix * SGX_GRID_ROWS + iy, index order inside a cell; `items` holds one unused element when no keypoint falls into the grid
enum { SGX_GRID_COLS = 64, SGX_GRID_ROWS = 48, SGX_GRID_CELLS = SGX_GRID_COLS * SGX_GRID_ROWS };
struct SgxKfGrid { std::vector<int> start, items; };
static SgxKfGrid build_kf_grid(int n, const sgx_keypoint *keys, const SgxCam &cam)
{
    const float invW = (float)SGX_GRID_COLS / (cam.maxX - cam.minX), invH = (float)SGX_GRID_ROWS / (cam.maxY - cam.minY);
    std::vector<int> cell((size_t)n, -1), fill(SGX_GRID_CELLS, 0);
    SgxKfGrid g;
    g.start.assign(SGX_GRID_CELLS + 1, 0);
    for (int i = 0; i < n; i++) {
        const int px = (int)round((keys[i].x - cam.minX) * invW), py = (int)round((keys[i].y - cam.minY) * invH);
        if (px < 0 || px >= SGX_GRID_COLS || py < 0 || py >= SGX_GRID_ROWS) continue;
        cell[(size_t)i] = px * SGX_GRID_ROWS + py; g.start[(size_t)cell[(size_t)i] + 1]++;
    }
    for (int c = 0; c < SGX_GRID_CELLS; c++) g.start[(size_t)c + 1] += g.start[(size_t)c];
    g.items.assign(g.start[SGX_GRID_CELLS] > 0 ? (size_t)g.start[SGX_GRID_CELLS] : 1, 0);
    for (int i = 0; i < n; i++) if (cell[(size_t)i] >= 0) g.items[(size_t)g.start[(size_t)cell[(size_t)i]] + fill[(size_t)cell[(size_t)i]]++] = i;
    return g;
}

extern "C" int sgx_match_search_for_triangulation(
    int n1, const sgx_keypoint *keys1_un, const uint8_t *desc1, const float *uright1, const uint8_t *has_mp1, const int32_t *feat_node1, const float *cam_center1,
    int n2, const sgx_keypoint *keys2_un, const uint8_t *desc2, const float *uright2, const uint8_t *has_mp2, const int32_t *feat_node2, const float *Tcw2,
    const float *F12, const sgx_camera *cam2, const float *scale_factors2, const float *level_sigma2_2, int nlevels, int only_stereo, int check_orientation,
    int32_t *pairs, int32_t *npairs)
{
    if (n1 < 0 || n2 < 0 || !npairs || !F12 || !cam2 || !scale_factors2 || !level_sigma2_2 || nlevels < 1 || nlevels > 12 || !cam_center1 || !Tcw2) return SGX_ERR_INVALID;
    *npairs = 0;
    if (n1 == 0 || n2 == 0) return SGX_OK;
    if (!keys1_un || !desc1 || !uright1 || !has_mp1 || !feat_node1 || !keys2_un || !desc2 || !uright2 || !has_mp2 || !feat_node2 || !pairs) return SGX_ERR_INVALID;
    if (!octaves_ok(keys1_un, n1, nlevels) || !octaves_ok(keys2_un, n2, nlevels)) return SGX_ERR_INVALID;
    std::vector<int> it1, it2;
    const std::vector<int> job = common_node_jobs(feat_node1, n1, it1, feat_node2, n2, it2);
    SgxTriArgs A; memset(&A, 0, sizeof A);
    A.n1 = n1; A.n2 = n2; A.nnodes = (int)(job.size() / 4);
    // epipole of KF1's centre in KF2 (:666-674): cv::Mat float products, left to right
    {
        float C2[3];
        for (int r = 0; r < 3; r++) {           // cv::Mat C2 = R2w*Cw + t2w: one cv::gemm(alpha = 1, beta = 1): float dot left to right, then (float)(dot + t) in double
            const float *row = Tcw2 + 4 * r; const float t = row[0] * cam_center1[0] + row[1] * cam_center1[1] + row[2] * cam_center1[2];
            C2[r] = (float)((double)t * 1.0 + 1.0 * (double)row[3]);
        }
        const float invz = 1.0f / C2[2];
        A.ex = cam2->fx * C2[0] * invz + cam2->cx; A.ey = cam2->fy * C2[1] * invz + cam2->cy;
    }
    for (int i = 0; i < 9; i++) A.F12[i] = F12[i];
    A.scale2 = to_scales(scale_factors2, nlevels); A.sigma2_2 = to_scales(level_sigma2_2, nlevels);
    A.only_stereo = only_stereo; A.check_ori = check_orientation;
    SgxStaging st(SGX_STAGE_SHARED);
    A.keys1 = st.keys(keys1_un, n1); A.desc1 = st.desc(desc1, n1); A.uright1 = st.in(uright1, n1); A.has_mp1 = st.in(has_mp1, n1);
    A.keys2 = st.keys(keys2_un, n2); A.desc2 = st.desc(desc2, n2); A.uright2 = st.in(uright2, n2); A.has_mp2 = st.in(has_mp2, n2);
    A.items1 = st.in(it1.data(), it1.size()); A.items2 = st.in(it2.data(), it2.size()); A.job = st.in(job.data(), job.size());
    A.match12 = st.out<int>(n1); A.matched2 = st.out<uint8_t>(n2); A.nmatches = st.out<int>(1);
    if (st.rc != SGX_OK) return st.rc;
    SGX_LAUNCH(k_search_triangulation, dim3(1), dim3(256), (sgx_stream_t)0, A);
    SGX_CHECK_HIP(hipGetLastError());
    std::vector<int> m12((size_t)n1);
    st.back(m12.data(), A.match12, n1);
    if (st.rc != SGX_OK) return st.rc;
    int n = 0;
    for (int i = 0; i < n1; i++) if (m12[(size_t)i] >= 0) { pairs[2 * n] = i; pairs[2 * n + 1] = m12[(size_t)i]; n++; }      // vMatchedPairs in ascending idx1 (:815-822)
    *npairs = n;
    return SGX_OK;
}

// shared body of the two SearchByBoW overloads (ORBmatcher.cc:167-290 KeyFrame-Frame, :524-655 KeyFrame-KeyFrame)
static int search_by_bow_impl(
    int nk, const sgx_keypoint *keys_kf_un, const uint8_t *desc_kf, const uint8_t *kf_good_mp, const int32_t *feat_node_kf,
    int nf, const sgx_keypoint *keys_f_un, const uint8_t *desc_f, const uint8_t *good_f, const int32_t *feat_node_f, float nnratio, int check_orientation, int th_low,
    int32_t *match_f, int32_t *nmatches)
{
    std::vector<int> it1, it2;
    const std::vector<int> job = common_node_jobs(feat_node_kf, nk, it1, feat_node_f, nf, it2);
    SgxBowArgs A; memset(&A, 0, sizeof A);
    A.nk = nk; A.nf = nf; A.nnodes = (int)(job.size() / 4); A.nnratio = nnratio; A.check_ori = check_orientation; A.th_low = th_low;
    SgxStaging st(SGX_STAGE_SHARED);
    A.keys_k = st.keys(keys_kf_un, nk); A.desc_k = st.desc(desc_kf, nk); A.good_k = st.in(kf_good_mp, nk);
    A.keys_f = st.keys(keys_f_un, nf); A.desc_f = st.desc(desc_f, nf);
    A.items_k = st.in(it1.data(), it1.size()); A.items_f = st.in(it2.data(), it2.size()); A.job = st.in(job.data(), job.size());
    A.match_f = st.out<int>(nf); A.nmatches = st.out<int>(1);
    if (good_f) A.good_f = st.in(good_f, nf);
    if (st.rc != SGX_OK) return st.rc;
    SGX_LAUNCH(k_search_bow, dim3(1), dim3(256), (sgx_stream_t)0, A);
    SGX_CHECK_HIP(hipGetLastError());
    st.back(match_f, A.match_f, nf); st.back(nmatches, A.nmatches, 1);
    return st.rc;
}

extern "C" int sgx_match_search_by_bow(
    int nk, const sgx_keypoint *keys_kf_un, const uint8_t *desc_kf, const uint8_t *kf_good_mp, const int32_t *feat_node_kf,
    int nf, const sgx_keypoint *keys_f_un, const uint8_t *desc_f, const int32_t *feat_node_f, float nnratio, int check_orientation,
    int32_t *match_f, int32_t *nmatches)
{
    if (nk < 0 || nf < 0 || !nmatches || (nf > 0 && !match_f)) return SGX_ERR_INVALID;
    *nmatches = 0;
    for (int j = 0; j < nf; j++) match_f[j] = -1;
    if (nk == 0 || nf == 0) return SGX_OK;
    if (!keys_kf_un || !desc_kf || !kf_good_mp || !feat_node_kf || !keys_f_un || !desc_f || !feat_node_f) return SGX_ERR_INVALID;
    return search_by_bow_impl(nk, keys_kf_un, desc_kf, kf_good_mp, feat_node_kf, nf, keys_f_un, desc_f, nullptr, feat_node_f, nnratio, check_orientation, SGX_TH_LOW, match_f, nmatches);
}

extern "C" int sgx_match_search_by_bow_kf(
    int n1, const sgx_keypoint *keys1_un, const uint8_t *desc1, const uint8_t *good1, const int32_t *feat_node1,
    int n2, const sgx_keypoint *keys2_un, const uint8_t *desc2, const uint8_t *good2, const int32_t *feat_node2, float nnratio, int check_orientation,
    int32_t *match12, int32_t *nmatches)
{
    if (n1 < 0 || n2 < 0 || !nmatches || (n1 > 0 && !match12)) return SGX_ERR_INVALID;
    *nmatches = 0;
    for (int i = 0; i < n1; i++) match12[i] = -1;
    if (n1 == 0 || n2 == 0) return SGX_OK;
    if (!keys1_un || !desc1 || !good1 || !feat_node1 || !keys2_un || !desc2 || !good2 || !feat_node2) return SGX_ERR_INVALID;
    std::vector<int32_t> m2((size_t)n2, -1);
    const int rc = search_by_bow_impl(n1, keys1_un, desc1, good1, feat_node1, n2, keys2_un, desc2, good2, feat_node2, nnratio, check_orientation, SGX_TH_LOW - 1, m2.data(), nmatches);
    if (rc != SGX_OK) return rc;
    for (int j = 0; j < n2; j++) if (m2[(size_t)j] >= 0) match12[m2[(size_t)j]] = j;     // vbMatched2 makes the relation one-to-one, so the inverse is vpMatches12 (:600)
    return SGX_OK;
}

extern "C" int sgx_match_fuse_search(
    int nk, const sgx_keypoint *keys_un, const uint8_t *desc, const float *uright, const float *Tcw,
    int nm, const float *m_xw, const float *m_normal, const float *m_min_dist, const float *m_max_dist, const uint8_t *m_desc, const uint8_t *m_skip,
    const sgx_camera *cam, const float *scale_factors, const float *inv_level_sigma2, int nlevels, float log_scale_factor, float th,
    int32_t *best_idx, int32_t *best_dist, int32_t *nfused)
{
    if (nk < 0 || nm < 0 || !cam || !Tcw || !scale_factors || !inv_level_sigma2 || nlevels < 1 || nlevels > 12 || !nfused || (nm > 0 && (!best_idx || !best_dist))) return SGX_ERR_INVALID;
    *nfused = 0;
    for (int i = 0; i < nm; i++) { best_idx[i] = -1; best_dist[i] = 256; }
    if (nk == 0 || nm == 0) return SGX_OK;
    if (!keys_un || !desc || !uright || !m_xw || !m_normal || !m_min_dist || !m_max_dist || !m_desc || !m_skip) return SGX_ERR_INVALID;
    if (!octaves_ok(keys_un, nk, nlevels)) return SGX_ERR_INVALID;
    SgxFuseArgs A; memset(&A, 0, sizeof A);
    A.nk = nk; A.nm = nm; A.nlevels = nlevels; A.log_scale_factor = log_scale_factor; A.th = th;
    for (int r = 0; r < 3; r++) { for (int c = 0; c < 3; c++) A.Rcw[r][c] = Tcw[4 * r + c]; A.tcw[r] = Tcw[4 * r + 3]; }
    // deliberately the float form, not camera_centre(): Fuse reads pKF->GetCameraCenter() (ORBmatcher.cc:840), a float product on a stored transpose; test_fuse_search_* pins it against the oracle
    for (int r = 0; r < 3; r++) A.Ow[r] = -(A.Rcw[0][r] * A.tcw[0] + A.Rcw[1][r] * A.tcw[1] + A.Rcw[2][r] * A.tcw[2]);
    A.cam = to_cam(cam); A.scale = to_scales(scale_factors, nlevels); A.inv_sigma2 = to_scales(inv_level_sigma2, nlevels);
    const SgxKfGrid g = build_kf_grid(nk, keys_un, A.cam);                 // the keyframe's mGrid
    SgxStaging st(SGX_STAGE_SHARED);
    A.keys = st.keys(keys_un, nk); A.desc = st.desc(desc, nk); A.uright = st.in(uright, nk);
    A.cell_start = st.in(g.start.data(), g.start.size()); A.cell_items = st.in(g.items.data(), g.items.size());
    A.m_xw = st.in(m_xw, (size_t)nm * 3); A.m_normal = st.in(m_normal, (size_t)nm * 3); A.m_min_dist = st.in(m_min_dist, nm); A.m_max_dist = st.in(m_max_dist, nm);
    A.m_desc = st.desc(m_desc, nm); A.m_skip = st.in(m_skip, nm);
    A.best_idx = st.out<int>(nm); A.best_dist = st.out<int>(nm);
    if (st.rc != SGX_OK) return st.rc;
    SGX_LAUNCH(k_fuse_search, dim3((nm + 255) / 256), dim3(256), (sgx_stream_t)0, A);
    SGX_CHECK_HIP(hipGetLastError());
    st.back(best_idx, A.best_idx, nm); st.back(best_dist, A.best_dist, nm);
    if (st.rc != SGX_OK) return st.rc;
    int n = 0; for (int i = 0; i < nm; i++) n += best_idx[i] >= 0;
    *nfused = n;
    return SGX_OK;
}

extern "C" int sgx_match_project_keyframe(
    int nc, const sgx_keypoint *ckeys_un, const uint8_t *cdesc, const uint8_t *c_has_mp, const float *cTcw,
    int nk, const sgx_keypoint *kf_keys_un, const uint8_t *kf_ok, const float *m_xw, const float *m_min_dist, const float *m_max_dist, const uint8_t *m_desc,
    const sgx_camera *cam, const float *scale_factors, int nlevels, float log_scale_factor, float th, int orb_dist, int check_orientation,
    int32_t *cur_match, int32_t *nmatches)
{
    if (nc < 0 || nk < 0 || !cam || !cTcw || !scale_factors || nlevels < 1 || nlevels > 12 || !nmatches || (nc > 0 && !cur_match)) return SGX_ERR_INVALID;
    *nmatches = 0;
    for (int k = 0; k < nc; k++) cur_match[k] = -1;
    if (nc == 0 || nk == 0) return SGX_OK;
    if (!ckeys_un || !cdesc || !c_has_mp || !kf_keys_un || !kf_ok || !m_xw || !m_min_dist || !m_max_dist || !m_desc) return SGX_ERR_INVALID;
    SgxKfProjArgs A; memset(&A, 0, sizeof A);
    A.nc = nc; A.nk = nk; A.nlevels = nlevels; A.orb_dist = orb_dist; A.check_ori = check_orientation; A.log_scale_factor = log_scale_factor; A.th = th;
    for (int r = 0; r < 3; r++) { for (int c = 0; c < 3; c++) A.Rcw[r][c] = cTcw[4 * r + c]; A.tcw[r] = cTcw[4 * r + 3]; }
    camera_centre(&A.Rcw[0][0], 3, A.tcw, 1, A.Ow);
    A.cam = to_cam(cam); A.scale = to_scales(scale_factors, nlevels);
    const SgxKfGrid g = build_kf_grid(nc, ckeys_un, A.cam);                // CurrentFrame.mGrid
    SgxStaging st(SGX_STAGE_SHARED);
    A.ckeys = st.keys(ckeys_un, nc); A.cdesc = st.desc(cdesc, nc); A.c_has_mp = st.in(c_has_mp, nc);
    A.cell_start = st.in(g.start.data(), g.start.size()); A.cell_items = st.in(g.items.data(), g.items.size());
    A.kf_keys = st.keys(kf_keys_un, nk); A.kf_ok = st.in(kf_ok, nk); A.m_xw = st.in(m_xw, (size_t)nk * 3); A.m_min_dist = st.in(m_min_dist, nk); A.m_max_dist = st.in(m_max_dist, nk);
    A.m_desc = st.desc(m_desc, nk);
    A.lock_a = st.out<int>(nc); A.lock_b = st.out<int>(nc); A.choice = st.out<int>(nk); A.cur_match = st.out<int>(nc); A.nmatches = st.out<int>(1);
    if (st.rc != SGX_OK) return st.rc;
    SGX_LAUNCH(k_match_project_kf, dim3(1), dim3(1024), (sgx_stream_t)0, A);
    SGX_CHECK_HIP(hipGetLastError());
    st.back(cur_match, A.cur_match, nc); st.back(nmatches, A.nmatches, 1);
    return st.rc;
}

// ---- loop-closing matchers that project through a Sim3 -------------------------------------------------------------------------------------------------------------

// "Decompose Scw" (ORBmatcher.cc:301-306, :990-995).  cv::Mat arithmetic: Mat::dot accumulates in double; Mat / double is a convertTo by the float of 1/scw
static void decompose_scw(const float *Scw, float R[3][3], float t[3], float Ow[3])
{
    double s = 0; for (int c = 0; c < 3; c++) s += (double)Scw[c] * (double)Scw[c];
    const float scw = (float)sqrt(s), inv = (float)(1.0 / (double)scw);
    for (int r = 0; r < 3; r++) { for (int c = 0; c < 3; c++) R[r][c] = Scw[4 * r + c] * inv; t[r] = Scw[4 * r + 3] * inv; }
    camera_centre(&R[0][0], 3, t, 1, Ow);
}

static void sim3_fill_common(SgxSim3ProjArgs &A, const sgx_camera *cam, const float *scale_factors, int nlevels, float log_scale_factor, float th)
{
    A.nlevels = nlevels; A.log_scale_factor = log_scale_factor; A.th = th;
    A.cam = to_cam(cam); A.scale = to_scales(scale_factors, nlevels);
}

extern "C" int sgx_match_fuse_search_sim3(
    int nk, const sgx_keypoint *keys_un, const uint8_t *desc, const float *Scw,
    int nm, const float *m_xw, const float *m_normal, const float *m_min_dist, const float *m_max_dist, const uint8_t *m_desc, const uint8_t *m_skip,
    const sgx_camera *cam, const float *scale_factors, int nlevels, float log_scale_factor, float th,
    int32_t *best_idx, int32_t *best_dist, int32_t *nfused)
{
    if (nk < 0 || nm < 0 || !cam || !Scw || !scale_factors || nlevels < 1 || nlevels > 12 || !nfused || (nm > 0 && (!best_idx || !best_dist))) return SGX_ERR_INVALID;
    *nfused = 0;
    for (int i = 0; i < nm; i++) { best_idx[i] = -1; best_dist[i] = 256; }
    if (nk == 0 || nm == 0) return SGX_OK;
    if (!keys_un || !desc || !m_xw || !m_normal || !m_min_dist || !m_max_dist || !m_desc || !m_skip) return SGX_ERR_INVALID;
    SgxSim3ProjArgs A; memset(&A, 0, sizeof A);
    A.nk = nk; A.nm = nm; A.flags = SGX_S3_NORMAL; A.th_accept = SGX_TH_LOW;
    sim3_fill_common(A, cam, scale_factors, nlevels, log_scale_factor, th);
    decompose_scw(Scw, A.R1, A.t1, A.Ow);
    const SgxKfGrid g = build_kf_grid(nk, keys_un, A.cam);
    SgxStaging st(SGX_STAGE_SHARED);
    A.keys = st.keys(keys_un, nk); A.desc = st.desc(desc, nk); A.cell_start = st.in(g.start.data(), g.start.size()); A.cell_items = st.in(g.items.data(), g.items.size());
    A.m_xw = st.in(m_xw, (size_t)nm * 3); A.m_normal = st.in(m_normal, (size_t)nm * 3); A.m_min_dist = st.in(m_min_dist, nm); A.m_max_dist = st.in(m_max_dist, nm);
    A.m_desc = st.desc(m_desc, nm); A.m_skip = st.in(m_skip, nm); A.best_idx = st.out<int>(nm); A.best_dist = st.out<int>(nm);
    if (st.rc != SGX_OK) return st.rc;
    SGX_LAUNCH(k_sim3_search, dim3((nm + 255) / 256), dim3(256), (sgx_stream_t)0, A);
    SGX_CHECK_HIP(hipGetLastError());
    st.back(best_idx, A.best_idx, nm); st.back(best_dist, A.best_dist, nm);
    if (st.rc != SGX_OK) return st.rc;
    int n = 0; for (int i = 0; i < nm; i++) n += best_idx[i] >= 0;
    *nfused = n;
    return SGX_OK;
}

extern "C" int sgx_match_project_sim3(
    int nk, const sgx_keypoint *keys_un, const uint8_t *desc, const uint8_t *matched_in, const float *Scw,
    int nm, const float *m_xw, const float *m_normal, const float *m_min_dist, const float *m_max_dist, const uint8_t *m_desc, const uint8_t *m_skip,
    const sgx_camera *cam, const float *scale_factors, int nlevels, float log_scale_factor, int th,
    int32_t *matched_out, int32_t *nmatches)
{
    if (nk < 0 || nm < 0 || !cam || !Scw || !scale_factors || nlevels < 1 || nlevels > 12 || !nmatches || (nk > 0 && !matched_out)) return SGX_ERR_INVALID;
    *nmatches = 0;
    for (int k = 0; k < nk; k++) matched_out[k] = -1;
    if (nk == 0 || nm == 0) return SGX_OK;
    if (!keys_un || !desc || !matched_in || !m_xw || !m_normal || !m_min_dist || !m_max_dist || !m_desc || !m_skip) return SGX_ERR_INVALID;
    SgxSim3ProjArgs A; memset(&A, 0, sizeof A);
    A.nk = nk; A.nm = nm; A.flags = SGX_S3_NORMAL | SGX_S3_FLOAT_INVZ; A.th_accept = SGX_TH_LOW;
    sim3_fill_common(A, cam, scale_factors, nlevels, log_scale_factor, (float)th);
    decompose_scw(Scw, A.R1, A.t1, A.Ow);
    const SgxKfGrid g = build_kf_grid(nk, keys_un, A.cam);
    SgxStaging st(SGX_STAGE_SHARED);
    A.keys = st.keys(keys_un, nk); A.desc = st.desc(desc, nk); A.cell_start = st.in(g.start.data(), g.start.size()); A.cell_items = st.in(g.items.data(), g.items.size());
    A.m_xw = st.in(m_xw, (size_t)nm * 3); A.m_normal = st.in(m_normal, (size_t)nm * 3); A.m_min_dist = st.in(m_min_dist, nm); A.m_max_dist = st.in(m_max_dist, nm);
    A.m_desc = st.desc(m_desc, nm); A.m_skip = st.in(m_skip, nm); A.best_idx = st.out<int>(nm); A.best_dist = st.out<int>(nm);
    A.taken_in = st.in(matched_in, nk); A.lock_a = st.out<int>(nk); A.lock_b = st.out<int>(nk); A.matched_out = st.out<int>(nk); A.nmatches = st.out<int>(1);
    if (st.rc != SGX_OK) return st.rc;
    SGX_LAUNCH(k_sim3_search_locked, dim3(1), dim3(1024), (sgx_stream_t)0, A);
    SGX_CHECK_HIP(hipGetLastError());
    st.back(matched_out, A.matched_out, nk); st.back(nmatches, A.nmatches, 1);
    return st.rc;
}

extern "C" int sgx_match_search_by_sim3(
    int n1, const sgx_keypoint *keys1_un, const uint8_t *desc1, const float *Tcw1, const uint8_t *mp_ok1, const float *m_xw1, const float *m_min_dist1, const float *m_max_dist1, const uint8_t *m_desc1,
    int n2, const sgx_keypoint *keys2_un, const uint8_t *desc2, const float *Tcw2, const uint8_t *mp_ok2, const float *m_xw2, const float *m_min_dist2, const float *m_max_dist2, const uint8_t *m_desc2,
    const sgx_camera *cam, const float *scale_factors, int nlevels, float log_scale_factor, float s12, const float *R12, const float *t12, float th,
    int32_t *match12, int32_t *nfound)
{
    if (n1 < 0 || n2 < 0 || !cam || !scale_factors || nlevels < 1 || nlevels > 12 || !nfound || !R12 || !t12 || !Tcw1 || !Tcw2 || (n1 > 0 && !match12)) return SGX_ERR_INVALID;
    *nfound = 0;
    if (n1 == 0 || n2 == 0) return SGX_OK;
    if (!keys1_un || !desc1 || !mp_ok1 || !m_xw1 || !m_min_dist1 || !m_max_dist1 || !m_desc1 || !keys2_un || !desc2 || !mp_ok2 || !m_xw2 || !m_min_dist2 || !m_max_dist2 || !m_desc2) return SGX_ERR_INVALID;
    // vbAlreadyMatched1 / vbAlreadyMatched2 (:1136-1147) folded into the per-point skip flags
    std::vector<uint8_t> skip1((size_t)n1), skip2((size_t)n2);
    for (int i = 0; i < n2; i++) skip2[(size_t)i] = !mp_ok2[i];
    for (int i = 0; i < n1; i++) {
        skip1[(size_t)i] = !mp_ok1[i] || match12[i] != -1;
        if (match12[i] >= 0 && match12[i] < n2) skip2[(size_t)match12[i]] = 1;
    }
    // s12*R12, (1.0/s12)*R12.t(), -sR21*t12 (:1124-1126): float scaling by the float of the factor; the 3x3 * 3x1 product goes through cv::gemm's small path
    float sR12[3][3], sR21[3][3], t21[3];
    const float inv_s = (float)(1.0 / (double)s12);
    for (int r = 0; r < 3; r++) for (int c = 0; c < 3; c++) { sR12[r][c] = R12[3 * r + c] * s12; sR21[r][c] = R12[3 * c + r] * inv_s; }
    for (int r = 0; r < 3; r++) { const float t = sR21[r][0] * t12[0] + sR21[r][1] * t12[1] + sR21[r][2] * t12[2]; t21[r] = (float)((double)t * -1.0 + 0.0); }
    // A: KF1's points into KF2 (:1150-1224); B: KF2's points into KF1 (:1227-1301)
    SgxSim3ProjArgs A; memset(&A, 0, sizeof A);
    A.flags = SGX_S3_TWO_STEP | SGX_S3_CAM_DIST; A.th_accept = SGX_TH_HIGH;
    sim3_fill_common(A, cam, scale_factors, nlevels, log_scale_factor, th);
    SgxSim3ProjArgs B = A;
    A.nk = n2; A.nm = n1; B.nk = n1; B.nm = n2;
    for (int r = 0; r < 3; r++) { for (int c = 0; c < 3; c++) { A.R1[r][c] = Tcw1[4 * r + c]; A.R2[r][c] = sR21[r][c]; } A.t1[r] = Tcw1[4 * r + 3]; A.t2[r] = t21[r]; }
    for (int r = 0; r < 3; r++) { for (int c = 0; c < 3; c++) { B.R1[r][c] = Tcw2[4 * r + c]; B.R2[r][c] = sR12[r][c]; } B.t1[r] = Tcw2[4 * r + 3]; B.t2[r] = t12[r]; }
    const SgxKfGrid g1 = build_kf_grid(n1, keys1_un, A.cam), g2 = build_kf_grid(n2, keys2_un, A.cam);
    SgxStaging st(SGX_STAGE_SHARED);
    // KF1: its keypoints and grid are what B searches, its map points are what A projects
    B.keys = st.keys(keys1_un, n1); B.desc = st.desc(desc1, n1); B.cell_start = st.in(g1.start.data(), g1.start.size()); B.cell_items = st.in(g1.items.data(), g1.items.size());
    A.m_xw = st.in(m_xw1, (size_t)n1 * 3); A.m_min_dist = st.in(m_min_dist1, n1); A.m_max_dist = st.in(m_max_dist1, n1); A.m_desc = st.desc(m_desc1, n1); A.m_skip = st.in(skip1.data(), n1);
    A.best_idx = st.out<int>(n1); A.best_dist = st.out<int>(n1);
    // KF2: the other way round
    A.keys = st.keys(keys2_un, n2); A.desc = st.desc(desc2, n2); A.cell_start = st.in(g2.start.data(), g2.start.size()); A.cell_items = st.in(g2.items.data(), g2.items.size());
    B.m_xw = st.in(m_xw2, (size_t)n2 * 3); B.m_min_dist = st.in(m_min_dist2, n2); B.m_max_dist = st.in(m_max_dist2, n2); B.m_desc = st.desc(m_desc2, n2); B.m_skip = st.in(skip2.data(), n2);
    B.best_idx = st.out<int>(n2); B.best_dist = st.out<int>(n2);
    if (st.rc != SGX_OK) return st.rc;
    SGX_LAUNCH(k_sim3_search, dim3((n1 + 255) / 256), dim3(256), (sgx_stream_t)0, A);
    SGX_CHECK_HIP(hipGetLastError());
    SGX_LAUNCH(k_sim3_search, dim3((n2 + 255) / 256), dim3(256), (sgx_stream_t)0, B);
    SGX_CHECK_HIP(hipGetLastError());
    std::vector<int> m1((size_t)n1), m2((size_t)n2);
    st.back(m1.data(), A.best_idx, n1); st.back(m2.data(), B.best_idx, n2);
    if (st.rc != SGX_OK) return st.rc;
    int n = 0;
    for (int i1 = 0; i1 < n1; i1++) {                                   // check agreement (:1305-1320)
        const int idx2 = m1[(size_t)i1];
        if (idx2 >= 0 && m2[(size_t)idx2] == i1) { match12[i1] = idx2; n++; }
    }
    *nfound = n;
    return SGX_OK;
}

extern "C" int sgx_match_search_for_initialization(
    int n1, const sgx_keypoint *keys1_un, const uint8_t *desc1, int n2, const sgx_keypoint *keys2_un, const uint8_t *desc2,
    float *prev_matched, int window_size, float nnratio, int check_orientation, const sgx_camera *cam, int32_t *matches12, int32_t *nmatches)
{
    if (n1 < 0 || n2 < 0 || !cam || !nmatches || window_size < 0 || (n1 > 0 && (!matches12 || !prev_matched))) return SGX_ERR_INVALID;
    *nmatches = 0;
    for (int i = 0; i < n1; i++) matches12[i] = -1;
    if (n1 == 0 || n2 == 0) return SGX_OK;
    if (!keys1_un || !desc1 || !keys2_un || !desc2 || n2 >= (1 << 22)) return SGX_ERR_INVALID;
    SgxInitSearchArgs A; memset(&A, 0, sizeof A);
    A.n1 = n1; A.n2 = n2; A.window = window_size; A.check_ori = check_orientation; A.nnratio = nnratio;
    A.cam = to_cam(cam);
    const SgxKfGrid g = build_kf_grid(n2, keys2_un, A.cam);              // F2.mGrid (Frame::AssignFeaturesToGrid, same round() cell rule)
    SgxStaging st(SGX_STAGE_SHARED);
    A.keys1 = st.keys(keys1_un, n1); A.desc1 = st.desc(desc1, n1); A.keys2 = st.keys(keys2_un, n2); A.desc2 = st.desc(desc2, n2);
    A.cell_start = st.in(g.start.data(), g.start.size()); A.cell_items = st.in(g.items.data(), g.items.size()); A.prev_matched = st.inout(prev_matched, (size_t)n1 * 2);
    A.matches12 = st.out<int>(n1); A.matches21 = st.out<int>(n2); A.dist21 = st.out<int>(n2); A.nmatches = st.out<int>(1);
    if (st.rc != SGX_OK) return st.rc;
    SGX_LAUNCH(k_search_initialization, dim3(1), dim3(256), (sgx_stream_t)0, A);
    SGX_CHECK_HIP(hipGetLastError());
    st.back(matches12, A.matches12, n1); st.back(prev_matched, A.prev_matched, (size_t)n1 * 2); st.back(nmatches, A.nmatches, 1);
    return st.rc;
}

// ---- MapPoint post-steps (MapPoint.cc:242-307, :330-371), batched over points; host pointers, synchronous ------------------------------------------------------------
extern "C" int sgx_mappoint_update_normal_and_depth(int n, const float *xw, const int32_t *obs_start, const float *obs_center, const float *ref_center, const int32_t *ref_level,
                                                    const float *scale_factors, int nlevels, float *normal, float *min_dist, float *max_dist)
{
    if (n < 0 || nlevels < 1 || nlevels > 12 || !scale_factors || (n > 0 && (!xw || !obs_start || !ref_center || !ref_level || !normal || !min_dist || !max_dist))) return SGX_ERR_INVALID;
    if (n == 0) return SGX_OK;
    const int total = obs_start[n];
    if (total < 0 || (total > 0 && !obs_center)) return SGX_ERR_INVALID;
    for (int p = 0; p < n; p++) if (obs_start[p] > obs_start[p + 1] || ref_level[p] < 0 || ref_level[p] >= nlevels) return SGX_ERR_INVALID;
    SgxStaging st(SGX_STAGE_SHARED);
    const float *d_xw = st.in(xw, (size_t)n * 3); const int *d_start = st.in(obs_start, (size_t)n + 1);
    const float *d_oc = st.in(obs_center, (size_t)total * 3), *d_rc = st.in(ref_center, (size_t)n * 3); const int *d_rl = st.in(ref_level, n);
    float *d_normal = st.inout(normal, (size_t)n * 3), *d_min = st.inout(min_dist, n), *d_max = st.inout(max_dist, n);          // points without observations keep the caller's values
    if (st.rc != SGX_OK) return st.rc;
    SGX_LAUNCH(k_mappoint_normal_depth, dim3((n + 255) / 256), dim3(256), (sgx_stream_t)0, n, d_xw, d_start, d_oc, d_rc, d_rl, to_scales(scale_factors, nlevels), nlevels, d_normal, d_min, d_max);
    SGX_CHECK_HIP(hipGetLastError());
    st.back(normal, d_normal, (size_t)n * 3); st.back(min_dist, d_min, n); st.back(max_dist, d_max, n);
    return st.rc;
}

extern "C" int sgx_mappoint_distinctive_descriptors(int n, const int32_t *obs_start, const uint8_t *obs_desc, int32_t *best, uint8_t *desc_out)
{
    if (n < 0 || (n > 0 && (!obs_start || !best))) return SGX_ERR_INVALID;
    if (n == 0) return SGX_OK;
    const int total = obs_start[n];
    if (total < 0 || (total > 0 && !obs_desc)) return SGX_ERR_INVALID;
    for (int p = 0; p < n; p++) if (obs_start[p] > obs_start[p + 1] || obs_start[p + 1] - obs_start[p] > 65535) return SGX_ERR_INVALID;
    SgxStaging st(SGX_STAGE_SHARED);
    const int *d_start = st.in(obs_start, (size_t)n + 1); const uint32_t *d_desc = st.desc(obs_desc, total); int *d_best = st.out<int>(n);
    if (st.rc != SGX_OK) return st.rc;
    SGX_LAUNCH(k_mappoint_distinctive, dim3(n), dim3(64), (sgx_stream_t)0, n, d_start, d_desc, d_best);
    SGX_CHECK_HIP(hipGetLastError());
    st.back(best, d_best, n);
    if (st.rc != SGX_OK) return st.rc;
    if (desc_out) for (int p = 0; p < n; p++) if (best[p] >= 0) memcpy(desc_out + 32 * (size_t)p, obs_desc + 32 * (size_t)(obs_start[p] + best[p]), 32);      // mDescriptor = vDescriptors[BestIdx].clone()
    return SGX_OK;
}

extern "C" int sgx_triangulate_new_map_points(
    int npairs, const int32_t *pairs,
    int n1, const sgx_keypoint *keys1_un, const sgx_keypoint *keys1, const float *uright1, const float *depth1, const float *Tcw1,
    int n2, const sgx_keypoint *keys2_un, const sgx_keypoint *keys2, const float *uright2, const float *depth2, const float *Tcw2,
    const sgx_camera *cam, const float *scale_factors, const float *level_sigma2, int nlevels, uint8_t *ok, float *x3d, int32_t *nnew)
{
    if (npairs < 0 || n1 < 0 || n2 < 0 || !cam || !scale_factors || !level_sigma2 || nlevels < 2 || nlevels > 12 || !Tcw1 || !Tcw2 || !nnew || (npairs > 0 && (!pairs || !ok || !x3d))) return SGX_ERR_INVALID;
    *nnew = 0;
    if (npairs == 0) return SGX_OK;
    if (!keys1_un || !keys1 || !uright1 || !depth1 || !keys2_un || !keys2 || !uright2 || !depth2) return SGX_ERR_INVALID;
    if (!octaves_ok(keys1_un, n1, nlevels) || !octaves_ok(keys2_un, n2, nlevels)) return SGX_ERR_INVALID;
    for (int q = 0; q < npairs; q++) if (pairs[2 * q] < 0 || pairs[2 * q] >= n1 || pairs[2 * q + 1] < 0 || pairs[2 * q + 1] >= n2) return SGX_ERR_INVALID;
    SgxNewPointArgs A; memset(&A, 0, sizeof A);
    A.npairs = npairs; memcpy(A.Tcw1, Tcw1, 64); memcpy(A.Tcw2, Tcw2, 64);
    camera_centre(Tcw1, 4, Tcw1 + 3, 4, A.Ow1); camera_centre(Tcw2, 4, Tcw2 + 3, 4, A.Ow2);            // the two keyframes' camera centres
    A.fx = cam->fx; A.fy = cam->fy; A.cx = cam->cx; A.cy = cam->cy; A.mbf = cam->bf; A.ratio_factor = 1.5f * scale_factors[1];       // ratioFactor = 1.5f * mfScaleFactor (:233)
    A.scale = to_scales(scale_factors, nlevels); A.sigma2 = to_scales(level_sigma2, nlevels);
    SgxStaging st(SGX_STAGE_SHARED);
    A.pairs = st.in(pairs, (size_t)npairs * 2);
    A.keys1_un = st.keys(keys1_un, n1); A.keys1 = st.keys(keys1, n1); A.ur1 = st.in(uright1, n1); A.dp1 = st.in(depth1, n1);
    A.keys2_un = st.keys(keys2_un, n2); A.keys2 = st.keys(keys2, n2); A.ur2 = st.in(uright2, n2); A.dp2 = st.in(depth2, n2);
    A.ok = st.out<uint8_t>(npairs); A.x3d = st.out<float>((size_t)npairs * 3);
    if (st.rc != SGX_OK) return st.rc;
    SGX_LAUNCH(k_triangulate_pairs, dim3((npairs + 255) / 256), dim3(256), (sgx_stream_t)0, A);
    SGX_CHECK_HIP(hipGetLastError());
    st.back(ok, A.ok, npairs); st.back(x3d, A.x3d, (size_t)npairs * 3);
    if (st.rc != SGX_OK) return st.rc;
    int n = 0; for (int q = 0; q < npairs; q++) n += ok[q];
    *nnew = n;
    return SGX_OK;
}
