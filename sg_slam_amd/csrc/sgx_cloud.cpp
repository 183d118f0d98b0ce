// sgx_cloud.cpp — host side of PointCloudMapping's keyframe cloud (src/sg-slam/src/PointcloudMapping.cc) behind the C ABI: the handle owns the per-keyframe
// workspace; build_batch_dev enqueues the kernels of sgx_cloud_kernels.h on the caller's stream and reads nothing back; the single build is a batch of one fed
// from host memory.  camera_to_map_tf is host code.
#include "sgx_cloud_kernels.h"
#include "sgx_devmem.h"
#include "../../include/sgx.h"
#include <math.h>
#include <stdio.h>
#include <string.h>
#include <vector>
#ifdef SGX_DEBUG_TAPS
#include "../../include/sgx_debug.h"      // test taps: compiled into tests/taps/libsgx_taps.so and the emulator only
#endif

static_assert(sizeof(SgxCloudResult) == sizeof(sgx_cloud_result) && sizeof(SgxCloudPoint) == sizeof(sgx_cloud_point), "the kernels write sgx_cloud_result and sgx_cloud_point");
static_assert(SGX_CLOUD_BOXES == SGX_CLOUD_MAX_BOXES, "the rect table in LDS");

struct sgx_cloud {
    int width = 0, height = 0, N = 0, max_images = 0, max_boxes = 0, mode = 0, tiles = 0, nblk = 0, last_images = 0;
    sgx_cloud_params p;
    SgxCloudPoint *pts = nullptr, *spts = nullptr, *vox = nullptr;
    uint32_t *k0 = nullptr, *k1 = nullptr;
    int *v0 = nullptr, *v1 = nullptr, *tab = nullptr, *vstart = nullptr, *ci = nullptr;
    float *dist = nullptr; double *cd = nullptr;
    SgxCloudGrid *grid = nullptr;                                                           // 2 x max_images: the VoxelGrid, the search grid
    float *one_depth = nullptr, *one_boxes = nullptr; uint8_t *one_color = nullptr; double *one_twc = nullptr; int *one_int = nullptr;      // the synchronous entry's staging
    SgxCloudPoint *one_points = nullptr; SgxCloudResult *one_result = nullptr;
    SgxDevMem mem;
};

static bool cloud_finite(double v) { return v == v && v - v == 0; }

extern "C" int sgx_cloud_create(int width, int height, int max_images, int max_boxes, int mode, const sgx_cloud_params *params, sgx_cloud **out)
{
    if (out) *out = nullptr;
    if (!out || !params || width < 1 || height < 1 || (long long)width * height > (1 << 20) || max_images < 1 || max_boxes < 0 || max_boxes > SGX_CLOUD_MAX_BOXES) return SGX_ERR_INVALID;
    if (mode != SGX_CLOUD_LOCAL && mode != SGX_CLOUD_WORLD) return SGX_ERR_INVALID;
    if (params->sor_mean_k < 1 || !cloud_finite(params->voxel_leaf_size) || !(params->voxel_leaf_size > 0) || !cloud_finite(params->camera_valid_depth_min) ||
        !cloud_finite(params->camera_valid_depth_max)) return SGX_ERR_INVALID;
    sgx_cloud *h = new sgx_cloud;
    h->width = width; h->height = height; h->N = width * height; h->max_images = max_images; h->max_boxes = max_boxes; h->mode = mode; h->p = *params;
    h->tiles = (h->N + SGX_CLOUD_TILE - 1) / SGX_CLOUD_TILE; h->nblk = (h->N + 255) / 256;
    const size_t B = (size_t)max_images, P = B * (size_t)h->N, T = B * (size_t)(16 * h->tiles > h->nblk ? 16 * h->tiles : h->nblk);
    SgxDevMem &m = h->mem;
    int rc;
    if ((rc = m.alloc(&h->pts, P)) || (rc = m.alloc(&h->spts, P)) || (rc = m.alloc(&h->vox, P)) || (rc = m.alloc(&h->k0, P)) || (rc = m.alloc(&h->k1, P)) ||
        (rc = m.alloc(&h->v0, P)) || (rc = m.alloc(&h->v1, P)) || (rc = m.alloc(&h->tab, T)) || (rc = m.alloc(&h->vstart, P + B)) || (rc = m.alloc(&h->ci, SGX_CLOUD_CI * B)) ||
        (rc = m.alloc(&h->dist, P)) || (rc = m.alloc(&h->cd, 2 * B)) || (rc = m.alloc(&h->grid, 2 * B)) ||
        (rc = m.alloc(&h->one_depth, (size_t)h->N)) || (rc = m.alloc(&h->one_color, 3 * (size_t)h->N)) || (rc = m.alloc(&h->one_twc, 16)) ||
        (rc = m.alloc(&h->one_boxes, 4 * (size_t)max_boxes)) || (rc = m.alloc(&h->one_int, 2)) || (rc = m.alloc(&h->one_points, (size_t)h->N)) ||
        (rc = m.alloc(&h->one_result, 1))) { delete h; return rc; }
    *out = h;
    return SGX_OK;
}

extern "C" void sgx_cloud_destroy(sgx_cloud *h) { delete h; }

extern "C" int sgx_cloud_build_batch_dev(sgx_cloud *h, const float *depth_dev, int depth_pitch, const uint8_t *color_dev, int color_pitch, int n_images, const float *cam4,
                                         const double *twc_dev, const float *boxes_dev, const int32_t *n_boxes_dev, const int32_t *have_dynamic_dev,
                                         sgx_cloud_point *points_dev, sgx_cloud_result *results_dev, void *stream)
{
    if (!h || !depth_dev || !color_dev || !cam4 || !points_dev || !results_dev || n_images < 1 || n_images > h->max_images || depth_pitch < h->width ||
        color_pitch < 3 * h->width) return SGX_ERR_INVALID;
    if (h->mode == SGX_CLOUD_WORLD && !twc_dev) return SGX_ERR_INVALID;
    const sgx_stream_t s = (sgx_stream_t)stream;
    SgxCloudArgs A; memset(&A, 0, sizeof A);
    A.B = n_images; A.W = h->width; A.H = h->height; A.N = h->N; A.dpitch = depth_pitch; A.cpitch = color_pitch; A.max_boxes = h->max_boxes; A.mode = h->mode;
    A.consider = h->p.consider_dynamic != 0; A.mean_k = h->p.sor_mean_k; A.tiles = h->tiles; A.nblk = h->nblk;
    int r0 = 1; while ((2 * r0 + 1) * (2 * r0 + 1) < 2 * (A.mean_k + 1) && r0 < SGX_CLOUD_RMAX) r0++;         // the first window's rows hold twice the neighbours asked for
    A.r0 = r0;
    A.fx = cam4[0]; A.fy = cam4[1]; A.cx = cam4[2]; A.cy = cam4[3]; A.dmin = h->p.camera_valid_depth_min; A.dmax = h->p.camera_valid_depth_max; A.leaf = h->p.voxel_leaf_size;
    A.mul = h->p.sor_stddev_mul;
    A.depth = depth_dev; A.color = color_dev; A.twc = twc_dev; A.boxes = boxes_dev; A.nboxes = n_boxes_dev; A.have = have_dynamic_dev;
    A.pts = h->pts; A.spts = h->spts; A.vox = h->vox; A.out = (SgxCloudPoint *)points_dev; A.k0 = h->k0; A.k1 = h->k1; A.v0 = h->v0; A.v1 = h->v1; A.tab = h->tab;
    A.vstart = h->vstart; A.ci = h->ci; A.dist = h->dist; A.cd = h->cd; A.results = (SgxCloudResult *)results_dev;
    h->last_images = n_images;
    const unsigned B = (unsigned)n_images;
    const dim3 per_kf((B + 63) / 64), points((unsigned)h->nblk, B), tiles((unsigned)h->tiles, B), lanes((unsigned)((h->N + 63) / 64), B);
    SGX_LAUNCH(k_cloud_prep, per_kf, dim3(64), s, A);
    SGX_LAUNCH(k_cloud_points, points, dim3(256), s, A);
    for (int stage = 0; stage < 2; stage++) {
        A.stage = stage; A.g = h->grid + (size_t)stage * h->max_images;
        SGX_LAUNCH(k_cloud_grid, per_kf, dim3(64), s, A);
        SGX_LAUNCH(k_cloud_keys, points, dim3(256), s, A);
        for (int pass = 0; pass < 8; pass++) {                                               // 8 x 4 bits; an even number of passes ends in k0 / v0
            A.shift = 4 * pass; A.cur = pass & 1; A.scan_len = 16 * h->tiles; A.scan_slot = -1;
            SGX_LAUNCH(k_cloud_hist, tiles, dim3(256), s, A);
            SGX_LAUNCH(k_cloud_scan, dim3(B), dim3(256), s, A);
            SGX_LAUNCH(k_cloud_scatter, tiles, dim3(256), s, A);
        }
        SGX_LAUNCH(k_cloud_gather, points, dim3(256), s, A);
        if (stage == 0) {
            A.scan_len = h->nblk; A.scan_slot = SGX_CLOUD_NVOX;
            SGX_LAUNCH(k_cloud_flagcount, points, dim3(256), s, A);
            SGX_LAUNCH(k_cloud_scan, dim3(B), dim3(256), s, A);
            SGX_LAUNCH(k_cloud_flagapply, points, dim3(256), s, A);
            SGX_LAUNCH(k_cloud_centroid, lanes, dim3(64), s, A);
        }
    }
    SGX_LAUNCH(k_cloud_sor, lanes, dim3(64), s, A);
    SGX_LAUNCH(k_cloud_sor_whole, dim3(256, B), dim3(256), s, A);
    SGX_LAUNCH(k_cloud_stats, dim3(B), dim3(256), s, A);
    A.scan_len = h->nblk; A.scan_slot = SGX_CLOUD_KEPT;
    SGX_LAUNCH(k_cloud_flagcount, points, dim3(256), s, A);
    SGX_LAUNCH(k_cloud_scan, dim3(B), dim3(256), s, A);
    SGX_LAUNCH(k_cloud_flagapply, points, dim3(256), s, A);
    SGX_LAUNCH(k_cloud_result, per_kf, dim3(64), s, A);
    SGX_CHECK_HIP(hipGetLastError());
    return SGX_OK;
}

extern "C" int sgx_cloud_build(sgx_cloud *h, const float *depth, const uint8_t *color, const float *cam4, const double *twc, const float *boxes, int n_boxes, int have_dynamic,
                               sgx_cloud_point *points, int cap, sgx_cloud_result *result)
{
    if (!h || !depth || !color || !cam4 || !result || cap < 0 || (cap > 0 && !points) || n_boxes < 0 || n_boxes > h->max_boxes || (n_boxes > 0 && !boxes)) return SGX_ERR_INVALID;
    if (h->mode == SGX_CLOUD_WORLD && !twc) return SGX_ERR_INVALID;
    if (twc) for (int i = 0; i < 16; i++) if (twc[i] != twc[i]) return SGX_ERR_INVALID;
    const size_t px = (size_t)h->N;
    const int32_t ints[2] = { n_boxes, have_dynamic ? 1 : 0 };
    SGX_CHECK_HIP(hipMemcpy(h->one_depth, depth, 4 * px, hipMemcpyHostToDevice));
    SGX_CHECK_HIP(hipMemcpy(h->one_color, color, 3 * px, hipMemcpyHostToDevice));
    if (twc) SGX_CHECK_HIP(hipMemcpy(h->one_twc, twc, 8 * 16, hipMemcpyHostToDevice));
    if (n_boxes) SGX_CHECK_HIP(hipMemcpy(h->one_boxes, boxes, 16 * (size_t)n_boxes, hipMemcpyHostToDevice));
    SGX_CHECK_HIP(hipMemcpy(h->one_int, ints, sizeof ints, hipMemcpyHostToDevice));
    const int r = sgx_cloud_build_batch_dev(h, h->one_depth, h->width, h->one_color, 3 * h->width, 1, cam4, twc ? h->one_twc : nullptr, h->one_boxes, h->one_int, h->one_int + 1,
                                            (sgx_cloud_point *)h->one_points, (sgx_cloud_result *)h->one_result, nullptr);
    if (r != SGX_OK) return r;
    SGX_CHECK_HIP(hipStreamSynchronize((sgx_stream_t)0));
    SGX_CHECK_HIP(hipMemcpy(result, h->one_result, sizeof(SgxCloudResult), hipMemcpyDeviceToHost));
    if (result->n_points < 0 || result->n_points > h->N) return SGX_ERR_DEVICE;
    if (result->n_points > cap) return SGX_ERR_OVERFLOW;
    if (result->n_points) SGX_CHECK_HIP(hipMemcpy(points, h->one_points, sizeof(SgxCloudPoint) * (size_t)result->n_points, hipMemcpyDeviceToHost));
    return SGX_OK;
}

// MapViewer's camera_to_map_tf (:254-265).  Eigen::Quaterniond(Matrix3d) is Eigen's quaternionbase_assign_impl<Matrix3d, 3, 3>: the trace branch, else the largest
// diagonal element
extern "C" int sgx_cloud_camera_to_map_tf(const float *tcw, double origin[3], double rotation[4])
{
    if (!tcw || !origin || !rotation) return SGX_ERR_INVALID;
    float Rwc[3][3], twc[3];
    for (int i = 0; i < 3; i++) for (int j = 0; j < 3; j++) Rwc[i][j] = tcw[4 * j + i];
    for (int i = 0; i < 3; i++) {                                                            // cv::gemm on floats accumulates in double, then alpha = -1
        double a = 0;
        for (int k = 0; k < 3; k++) a += (double)Rwc[i][k] * (double)tcw[4 * k + 3];
        twc[i] = (float)(-a);
    }
    double m[3][3], q[4];                                                                    // q = x, y, z, w
    for (int i = 0; i < 3; i++) for (int j = 0; j < 3; j++) m[i][j] = (double)Rwc[i][j];
    double t = m[0][0] + m[1][1] + m[2][2];
    if (t > 0) {
        t = sqrt(t + 1.0); q[3] = 0.5 * t; t = 0.5 / t;
        q[0] = (m[2][1] - m[1][2]) * t; q[1] = (m[0][2] - m[2][0]) * t; q[2] = (m[1][0] - m[0][1]) * t;
    } else {
        int i = 0;
        if (m[1][1] > m[0][0]) i = 1;
        if (m[2][2] > m[i][i]) i = 2;
        const int j = (i + 1) % 3, k = (j + 1) % 3;
        t = sqrt(m[i][i] - m[j][j] - m[k][k] + 1.0); q[i] = 0.5 * t; t = 0.5 / t;
        q[3] = (m[k][j] - m[j][k]) * t; q[j] = (m[j][i] + m[i][j]) * t; q[k] = (m[k][i] + m[i][k]) * t;
    }
    origin[0] = (double)twc[2]; origin[1] = -(double)twc[0]; origin[2] = -(double)twc[1];
    rotation[0] = q[2]; rotation[1] = -q[0]; rotation[2] = -q[1]; rotation[3] = q[3];
    return SGX_OK;
}

#ifdef SGX_DEBUG_TAPS
// test tap: the voxel cloud of keyframe `image` of the handle's last batch before the outlier filter, its distances and kept flags.  Synchronises the device.
SGX_TAP int sgx_cloud_debug_read(sgx_cloud *h, int image, sgx_cloud_point *voxels, float *dist, uint8_t *kept, int cap, int *n)
{
    if (!h || image < 0 || image >= h->last_images || !n || cap < 0) return SGX_ERR_INVALID;
    SGX_CHECK_HIP(hipDeviceSynchronize());
    int ci[SGX_CLOUD_CI]; double cd[2];
    SGX_CHECK_HIP(hipMemcpy(ci, h->ci + (size_t)SGX_CLOUD_CI * image, sizeof ci, hipMemcpyDeviceToHost));
    SGX_CHECK_HIP(hipMemcpy(cd, h->cd + 2 * (size_t)image, sizeof cd, hipMemcpyDeviceToHost));
    const int nv = ci[SGX_CLOUD_NVOX];
    if (nv < 0 || nv > h->N) return SGX_ERR_DEVICE;
    *n = nv;
    if (nv > cap) return SGX_ERR_OVERFLOW;
    if (nv == 0) return SGX_OK;
    const size_t o = (size_t)image * h->N;
    if (voxels) SGX_CHECK_HIP(hipMemcpy(voxels, h->vox + o, sizeof(SgxCloudPoint) * (size_t)nv, hipMemcpyDeviceToHost));
    std::vector<float> d((size_t)nv, 0.0f);
    const bool filtered = nv > h->p.sor_mean_k;                                              // otherwise no distance was computed
    if (filtered) SGX_CHECK_HIP(hipMemcpy(d.data(), h->dist + o, 4 * (size_t)nv, hipMemcpyDeviceToHost));
    for (int i = 0; i < nv; i++) {
        if (dist) dist[i] = d[(size_t)i];
        if (kept) kept[i] = filtered && !((double)d[(size_t)i] > cd[1]) ? 1 : 0;
    }
    return SGX_OK;
}
#endif
