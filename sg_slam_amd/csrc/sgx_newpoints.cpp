// sgx_newpoints.cpp — host side of the keyframe store (sgx_kfstore_*) and of LocalMapping::CreateNewMapPoints over it (include/sgx.h).
// The store keeps what the LocalMapping entries read of a keyframe on the device, one slot per keyframe: mvKeysUn, mvKeys, descriptors, mvuRight, mvDepth, the pose and
// the features grouped by vocabulary node (the per-keyframe half of common_node_jobs, sgx_match2.cpp).  Mutations take host pointers and are synchronous; an add uploads
// its keyframe only and publishes the slot last, so a failed add leaves the handle as it was.  Device buffers are owned by SgxDevMem (sgx_devmem.h).
// Reference behaviour: src/sg-slam/src/LocalMapping.cc:207-452, :536-553.
#include "sgx_newpoints_kernels.h"
#include "sgx_host_args.h"
#include "sgx_devmem.h"
#include "../../include/sgx.h"
#include <stdio.h>
#include <string.h>
#include <algorithm>
#include <map>
#include <vector>

enum { SGX_KFSTORE_MAX_KF = 4096, SGX_KFSTORE_MAX_CAP = 8192 };

struct sgx_kfstore {
    SgxDevMem mem;
    SgxKfStoreDev dev;                       // the device pointers are the handle's own (non-const) arrays below
    int *slot_id = nullptr, *meta = nullptr; uint8_t *keys_un = nullptr, *keys = nullptr; uint32_t *desc = nullptr; float *uright = nullptr, *depth = nullptr;
    int *items = nullptr, *node_id = nullptr, *node_start = nullptr; float *Tcw = nullptr;
    std::map<int32_t, int> by_id;
    std::vector<int> free_slots;
    int64_t device_bytes = 0, workspace_bytes = 0;
    // workspace of the batched call, grown to the largest Q seen
    int ws_q = 0; int *w_match12 = nullptr, *w_pairs = nullptr; uint8_t *w_matched2 = nullptr, *w_ok = nullptr; float *w_x3d = nullptr;
};

// cv::invert of a 3 x 3 CV_32F matrix (DECOMP_LU takes the closed form for n <= 3): determinant and cofactors in double, one rounding to float per element
static bool invert33(const float *S, float *D)
{
    double d = (double)S[0] * ((double)S[4] * S[8] - (double)S[5] * S[7]) - (double)S[1] * ((double)S[3] * S[8] - (double)S[5] * S[6]) + (double)S[2] * ((double)S[3] * S[7] - (double)S[4] * S[6]);
    if (d == 0.) return false;
    d = 1. / d;
    double t[9];
    t[0] = ((double)S[4] * S[8] - (double)S[5] * S[7]) * d; t[1] = ((double)S[2] * S[7] - (double)S[1] * S[8]) * d; t[2] = ((double)S[1] * S[5] - (double)S[2] * S[4]) * d;
    t[3] = ((double)S[5] * S[6] - (double)S[3] * S[8]) * d; t[4] = ((double)S[0] * S[8] - (double)S[2] * S[6]) * d; t[5] = ((double)S[2] * S[3] - (double)S[0] * S[5]) * d;
    t[6] = ((double)S[3] * S[7] - (double)S[4] * S[6]) * d; t[7] = ((double)S[1] * S[6] - (double)S[0] * S[7]) * d; t[8] = ((double)S[0] * S[4] - (double)S[1] * S[3]) * d;
    for (int i = 0; i < 9; i++) D[i] = (float)t[i];
    return true;
}

static void kfstore_reset_host(sgx_kfstore *h)
{
    h->by_id.clear(); h->free_slots.clear();
    for (int s = h->dev.max_kf - 1; s >= 0; s--) h->free_slots.push_back(s);          // slot 0 first
}

extern "C" int sgx_kfstore_create(int max_keyframes, int cap, const sgx_camera *cam, const float *scale_factors, const float *level_sigma2, int nlevels, sgx_kfstore **out)
{
    if (out) *out = nullptr;
    if (!out || !cam || !scale_factors || !level_sigma2 || max_keyframes < 1 || cap < 1 || nlevels < 2 || nlevels > 12) return SGX_ERR_INVALID;      // ratioFactor reads level 1
    if (max_keyframes > SGX_KFSTORE_MAX_KF || cap > SGX_KFSTORE_MAX_CAP) return SGX_ERR_UNSUPPORTED;
    const float K[9] = { cam->fx, 0.f, cam->cx, 0.f, cam->fy, cam->cy, 0.f, 0.f, 1.f }, Kt[9] = { cam->fx, 0.f, 0.f, 0.f, cam->fy, 0.f, cam->cx, cam->cy, 1.f };
    sgx_kfstore *h = new sgx_kfstore;
    SgxKfStoreDev &D = h->dev; memset(&D, 0, sizeof D);
    if (!invert33(K, D.Kinv) || !invert33(Kt, D.KinvT)) { delete h; return SGX_ERR_INVALID; }
    D.max_kf = max_keyframes; D.cap = cap; D.nlevels = nlevels;
    D.fx = cam->fx; D.fy = cam->fy; D.cx = cam->cx; D.cy = cam->cy; D.bf = cam->bf;
    D.scale = to_scales(scale_factors, nlevels); D.sigma2 = to_scales(level_sigma2, nlevels);
    const size_t N = (size_t)max_keyframes, C = (size_t)cap;
    const std::vector<int> none(N, -1);
    int rc = h->mem.upload(&h->slot_id, none);
    if (rc == SGX_OK) rc = h->mem.alloc(&h->meta, N * 2);
    if (rc == SGX_OK) rc = h->mem.alloc(&h->keys_un, N * C * 28);
    if (rc == SGX_OK) rc = h->mem.alloc(&h->keys, N * C * 28);
    if (rc == SGX_OK) rc = h->mem.alloc(&h->desc, N * C * 8);
    if (rc == SGX_OK) rc = h->mem.alloc(&h->uright, N * C);
    if (rc == SGX_OK) rc = h->mem.alloc(&h->depth, N * C);
    if (rc == SGX_OK) rc = h->mem.alloc(&h->items, N * C);
    if (rc == SGX_OK) rc = h->mem.alloc(&h->node_id, N * C);
    if (rc == SGX_OK) rc = h->mem.alloc(&h->node_start, N * (C + 1));
    if (rc == SGX_OK) rc = h->mem.alloc(&h->Tcw, N * 12);
    if (rc != SGX_OK) { delete h; return rc; }
    h->device_bytes = (int64_t)(4 * N + 8 * N + 2 * 28 * N * C + 32 * N * C + 4 * (4 * N * C + N * (C + 1)) + 48 * N);
    D.slot_id = h->slot_id; D.meta = h->meta; D.keys_un = h->keys_un; D.keys = h->keys; D.desc = h->desc; D.uright = h->uright; D.depth = h->depth;
    D.items = h->items; D.node_id = h->node_id; D.node_start = h->node_start; D.Tcw = h->Tcw;
    kfstore_reset_host(h);
    *out = h;
    return SGX_OK;
}

extern "C" void sgx_kfstore_destroy(sgx_kfstore *h) { delete h; }

extern "C" int sgx_kfstore_size(const sgx_kfstore *h) { return h ? (int)h->by_id.size() : SGX_ERR_INVALID; }

extern "C" int sgx_kfstore_info(const sgx_kfstore *h, int64_t *device_bytes, int64_t *workspace_bytes)
{
    if (!h) return SGX_ERR_INVALID;
    if (device_bytes) *device_bytes = h->device_bytes + h->workspace_bytes;
    if (workspace_bytes) *workspace_bytes = h->workspace_bytes;
    return SGX_OK;
}

extern "C" int sgx_kfstore_clear(sgx_kfstore *h)
{
    if (!h) return SGX_ERR_INVALID;
    const std::vector<int> none((size_t)h->dev.max_kf, -1);
    SGX_CHECK_HIP(hipMemcpy(h->slot_id, none.data(), none.size() * sizeof(int), hipMemcpyHostToDevice));
    kfstore_reset_host(h);
    return SGX_OK;
}

extern "C" int sgx_kfstore_add(sgx_kfstore *h, int32_t kf_id, int n, const sgx_keypoint *keys_un, const sgx_keypoint *keys, const uint8_t *desc, const float *uright,
                               const float *depth, const int32_t *feat_node, const float *Tcw)
{
    if (!h || kf_id < 0 || n < 0 || n > h->dev.cap || !Tcw || (n > 0 && (!keys_un || !desc || !uright || !depth || !feat_node))) return SGX_ERR_INVALID;
    if (h->by_id.count(kf_id)) return SGX_ERR_INVALID;
    for (int i = 0; i < n; i++) if (keys_un[i].octave < 0 || keys_un[i].octave >= h->dev.nlevels) return SGX_ERR_INVALID;
    if (h->free_slots.empty()) return SGX_ERR_NOMEM;
    if (!keys) keys = keys_un;
    // the keyframe's FeatureVector: nodes ascending, feature indices ascending inside a node, features without a node left out
    std::vector<int> items, ids, start;
    for (int i = 0; i < n; i++) if (feat_node[i] >= 0) items.push_back(i);
    std::stable_sort(items.begin(), items.end(), [&](int x, int y) { return feat_node[x] < feat_node[y]; });
    for (size_t k = 0; k < items.size(); k++) if (k == 0 || feat_node[items[k]] != feat_node[items[k - 1]]) { ids.push_back(feat_node[items[k]]); start.push_back((int)k); }
    start.push_back((int)items.size());
    const int slot = h->free_slots.back();
    const size_t s = (size_t)slot, C = (size_t)h->dev.cap, m = (size_t)n;
    const int meta[2] = { n, (int)ids.size() };
    if (m) {
        SGX_CHECK_HIP(hipMemcpy(h->keys_un + s * C * 28, keys_un, m * 28, hipMemcpyHostToDevice));
        SGX_CHECK_HIP(hipMemcpy(h->keys + s * C * 28, keys, m * 28, hipMemcpyHostToDevice));
        SGX_CHECK_HIP(hipMemcpy(h->desc + s * C * 8, desc, m * 32, hipMemcpyHostToDevice));
        SGX_CHECK_HIP(hipMemcpy(h->uright + s * C, uright, m * 4, hipMemcpyHostToDevice));
        SGX_CHECK_HIP(hipMemcpy(h->depth + s * C, depth, m * 4, hipMemcpyHostToDevice));
    }
    if (!items.empty()) {
        SGX_CHECK_HIP(hipMemcpy(h->items + s * C, items.data(), items.size() * 4, hipMemcpyHostToDevice));
        SGX_CHECK_HIP(hipMemcpy(h->node_id + s * C, ids.data(), ids.size() * 4, hipMemcpyHostToDevice));
    }
    SGX_CHECK_HIP(hipMemcpy(h->node_start + s * (C + 1), start.data(), start.size() * 4, hipMemcpyHostToDevice));
    SGX_CHECK_HIP(hipMemcpy(h->meta + s * 2, meta, sizeof meta, hipMemcpyHostToDevice));
    SGX_CHECK_HIP(hipMemcpy(h->Tcw + s * 12, Tcw, 48, hipMemcpyHostToDevice));
    SGX_CHECK_HIP(hipMemcpy(h->slot_id + s, &kf_id, 4, hipMemcpyHostToDevice));               // the slot is published last
    h->free_slots.pop_back();
    h->by_id[kf_id] = slot;
    return SGX_OK;
}

extern "C" int sgx_kfstore_set_pose(sgx_kfstore *h, int32_t kf_id, const float *Tcw)
{
    if (!h || !Tcw) return SGX_ERR_INVALID;
    const auto it = h->by_id.find(kf_id);
    if (it == h->by_id.end()) return SGX_ERR_INVALID;
    SGX_CHECK_HIP(hipMemcpy(h->Tcw + (size_t)it->second * 12, Tcw, 48, hipMemcpyHostToDevice));
    return SGX_OK;
}

extern "C" int sgx_kfstore_erase(sgx_kfstore *h, int32_t kf_id)
{
    if (!h) return SGX_ERR_INVALID;
    const auto it = h->by_id.find(kf_id);
    if (it == h->by_id.end()) return SGX_ERR_INVALID;
    const int none = -1;
    SGX_CHECK_HIP(hipMemcpy(h->slot_id + (size_t)it->second, &none, 4, hipMemcpyHostToDevice));
    h->free_slots.push_back(it->second);
    h->by_id.erase(it);
    return SGX_OK;
}

// the workspace of Q queries; a larger one replaces the smaller (the handle serves one call at a time, so nothing in flight reads the old one)
static int kfstore_workspace(sgx_kfstore *h, int Q)
{
    if (Q <= h->ws_q) return SGX_OK;
    const size_t n = (size_t)Q * (size_t)h->dev.cap;
    int *m12 = nullptr, *pairs = nullptr; uint8_t *m2 = nullptr, *ok = nullptr; float *x3d = nullptr;
    int rc = h->mem.alloc(&m12, n);
    if (rc == SGX_OK) rc = h->mem.alloc(&pairs, 2 * n);
    if (rc == SGX_OK) rc = h->mem.alloc(&m2, n);
    if (rc == SGX_OK) rc = h->mem.alloc(&ok, n);
    if (rc == SGX_OK) rc = h->mem.alloc(&x3d, 3 * n);
    if (rc != SGX_OK) { h->mem.release(m12); h->mem.release(pairs); h->mem.release(m2); h->mem.release(ok); h->mem.release(x3d); return rc; }
    h->mem.release(h->w_match12); h->mem.release(h->w_pairs); h->mem.release(h->w_matched2); h->mem.release(h->w_ok); h->mem.release(h->w_x3d);
    h->w_match12 = m12; h->w_pairs = pairs; h->w_matched2 = m2; h->w_ok = ok; h->w_x3d = x3d;
    h->ws_q = Q; h->workspace_bytes = (int64_t)(26 * n);
    return SGX_OK;
}

extern "C" int sgx_create_new_map_points_batch_dev(
    sgx_kfstore *h, int Q, const int32_t *cur_ids_dev, const int32_t *nb_offsets_dev, const int32_t *nb_ids_dev, const int32_t *first_new_id_dev, const float *median_depth_dev,
    int32_t *mp_rows_dev, int32_t *n_new_dev, int32_t *new_kf2_dev, int32_t *new_idx1_dev, int32_t *new_idx2_dev, float *new_x3d_dev, uint8_t *new_desc_dev,
    float *new_normal_dev, float *new_min_dist_dev, float *new_max_dist_dev, sgx_newpoints_report *report_dev,
    int32_t *pair_idx1_dev, int32_t *pair_idx2_dev, uint8_t *pair_ok_dev, void *stream)
{
    if (!h || Q < 0) return SGX_ERR_INVALID;
    if (Q == 0) return SGX_OK;
    if (!cur_ids_dev || !nb_offsets_dev || !nb_ids_dev || !first_new_id_dev || !mp_rows_dev || !n_new_dev || !new_kf2_dev || !new_idx1_dev || !new_idx2_dev || !new_x3d_dev ||
        !new_desc_dev || !new_normal_dev || !new_min_dist_dev || !new_max_dist_dev || !report_dev || ((uintptr_t)new_desc_dev & 3)) return SGX_ERR_INVALID;
    const int rc = kfstore_workspace(h, Q);
    if (rc != SGX_OK) return rc;
    SgxNewPointsArgs A; memset(&A, 0, sizeof A);
    A.S = h->dev;
    A.cur_ids = cur_ids_dev; A.nb_off = nb_offsets_dev; A.nb_ids = nb_ids_dev; A.first_new_id = first_new_id_dev; A.median_depth = median_depth_dev; A.rows = mp_rows_dev;
    A.n_new = n_new_dev; A.new_kf2 = new_kf2_dev; A.new_idx1 = new_idx1_dev; A.new_idx2 = new_idx2_dev; A.new_x3d = new_x3d_dev; A.new_desc = (uint32_t *)new_desc_dev;
    A.new_normal = new_normal_dev; A.new_min_dist = new_min_dist_dev; A.new_max_dist = new_max_dist_dev; A.report = report_dev;
    A.pair_idx1 = pair_idx1_dev; A.pair_idx2 = pair_idx2_dev; A.pair_ok = pair_ok_dev;
    A.w_match12 = h->w_match12; A.w_matched2 = h->w_matched2; A.w_pairs = h->w_pairs; A.w_ok = h->w_ok; A.w_x3d = h->w_x3d;
    SGX_LAUNCH(k_create_new_map_points, dim3((unsigned)Q), dim3(256), (sgx_stream_t)stream, A);
    SGX_CHECK_HIP(hipGetLastError());
    return SGX_OK;
}

extern "C" int sgx_create_new_map_points(
    sgx_kfstore *h, int32_t cur_id, int n_nb, const int32_t *nb_ids, int32_t first_new_id, const float *median_depth, int32_t *mp_rows,
    int32_t *n_new, int32_t *new_kf2, int32_t *new_idx1, int32_t *new_idx2, float *new_x3d, uint8_t *new_desc, float *new_normal, float *new_min_dist, float *new_max_dist,
    sgx_newpoints_report *report, int32_t *pair_idx1, int32_t *pair_idx2, uint8_t *pair_ok)
{
    if (!h || n_nb < 0 || !mp_rows || !n_new || !new_kf2 || !new_idx1 || !new_idx2 || !new_x3d || !new_desc || !new_normal || !new_min_dist || !new_max_dist ||
        (n_nb > 0 && (!nb_ids || !report))) return SGX_ERR_INVALID;
    const size_t C = (size_t)h->dev.cap, nb = (size_t)n_nb;
    const int32_t off[2] = { 0, n_nb };
    SgxDevMem m;                                                         // the buffers of this call; freed on every exit
    int32_t *d_cur = nullptr, *d_off = nullptr, *d_nb = nullptr, *d_first = nullptr, *d_rows = nullptr, *d_n = nullptr, *d_kf2 = nullptr, *d_i1 = nullptr, *d_i2 = nullptr,
            *d_p1 = nullptr, *d_p2 = nullptr;
    float *d_med = nullptr, *d_x = nullptr, *d_nr = nullptr, *d_mn = nullptr, *d_mx = nullptr;
    uint8_t *d_desc = nullptr, *d_pok = nullptr; sgx_newpoints_report *d_rep = nullptr;
    int rc = m.upload(&d_cur, &cur_id, 1);
    if (rc == SGX_OK) rc = m.upload(&d_off, off, 2);
    if (rc == SGX_OK) rc = m.upload(&d_nb, nb_ids, nb);
    if (rc == SGX_OK) rc = m.upload(&d_first, &first_new_id, 1);
    if (rc == SGX_OK && median_depth) rc = m.upload(&d_med, median_depth, nb);
    if (rc == SGX_OK) rc = m.upload(&d_rows, mp_rows, (nb + 1) * C);
    if (rc == SGX_OK) rc = m.alloc(&d_n, 1);
    if (rc == SGX_OK) rc = m.alloc(&d_kf2, C);
    if (rc == SGX_OK) rc = m.alloc(&d_i1, C);
    if (rc == SGX_OK) rc = m.alloc(&d_i2, C);
    if (rc == SGX_OK) rc = m.alloc(&d_x, 3 * C);
    if (rc == SGX_OK) rc = m.alloc(&d_desc, 32 * C);
    if (rc == SGX_OK) rc = m.alloc(&d_nr, 3 * C);
    if (rc == SGX_OK) rc = m.alloc(&d_mn, C);
    if (rc == SGX_OK) rc = m.alloc(&d_mx, C);
    if (rc == SGX_OK) rc = m.alloc(&d_rep, nb);
    if (rc == SGX_OK && pair_idx1) rc = m.alloc(&d_p1, nb * C);
    if (rc == SGX_OK && pair_idx2) rc = m.alloc(&d_p2, nb * C);
    if (rc == SGX_OK && pair_ok) rc = m.alloc(&d_pok, nb * C);
    if (rc != SGX_OK) return rc;
    rc = sgx_create_new_map_points_batch_dev(h, 1, d_cur, d_off, d_nb, d_first, d_med, d_rows, d_n, d_kf2, d_i1, d_i2, d_x, d_desc, d_nr, d_mn, d_mx, d_rep, d_p1, d_p2, d_pok, nullptr);
    if (rc != SGX_OK) return rc;
    int32_t nn = 0;
    std::vector<sgx_newpoints_report> rep(nb);
    SGX_CHECK_HIP(hipMemcpy(&nn, d_n, 4, hipMemcpyDeviceToHost));        // blocking: the launch sequence has ended
    if (nb) SGX_CHECK_HIP(hipMemcpy(rep.data(), d_rep, nb * sizeof(sgx_newpoints_report), hipMemcpyDeviceToHost));
    if (nn < 0 || (size_t)nn > C) return SGX_ERR_DEVICE;
    const size_t k = (size_t)nn;
    std::vector<int32_t> rows((nb + 1) * C);
    SGX_CHECK_HIP(hipMemcpy(rows.data(), d_rows, rows.size() * 4, hipMemcpyDeviceToHost));
    // outputs are written past this point only: a failed call leaves them as they came
    if (k) {
        SGX_CHECK_HIP(hipMemcpy(new_kf2, d_kf2, k * 4, hipMemcpyDeviceToHost)); SGX_CHECK_HIP(hipMemcpy(new_idx1, d_i1, k * 4, hipMemcpyDeviceToHost));
        SGX_CHECK_HIP(hipMemcpy(new_idx2, d_i2, k * 4, hipMemcpyDeviceToHost)); SGX_CHECK_HIP(hipMemcpy(new_x3d, d_x, k * 12, hipMemcpyDeviceToHost));
        SGX_CHECK_HIP(hipMemcpy(new_desc, d_desc, k * 32, hipMemcpyDeviceToHost)); SGX_CHECK_HIP(hipMemcpy(new_normal, d_nr, k * 12, hipMemcpyDeviceToHost));
        SGX_CHECK_HIP(hipMemcpy(new_min_dist, d_mn, k * 4, hipMemcpyDeviceToHost)); SGX_CHECK_HIP(hipMemcpy(new_max_dist, d_mx, k * 4, hipMemcpyDeviceToHost));
    }
    for (size_t j = 0; j < nb; j++) {
        const size_t np = rep[j].n_pairs > 0 ? (size_t)rep[j].n_pairs : 0;
        if (!np) continue;
        if (pair_idx1) SGX_CHECK_HIP(hipMemcpy(pair_idx1 + j * C, d_p1 + j * C, np * 4, hipMemcpyDeviceToHost));
        if (pair_idx2) SGX_CHECK_HIP(hipMemcpy(pair_idx2 + j * C, d_p2 + j * C, np * 4, hipMemcpyDeviceToHost));
        if (pair_ok) SGX_CHECK_HIP(hipMemcpy(pair_ok + j * C, d_pok + j * C, np, hipMemcpyDeviceToHost));
    }
    memcpy(mp_rows, rows.data(), rows.size() * 4);
    for (size_t j = 0; j < nb; j++) report[j] = rep[j];
    *n_new = nn;
    return SGX_OK;
}
