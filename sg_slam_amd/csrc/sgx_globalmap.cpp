// sgx_globalmap.cpp — host side of MapViewer's accumulating global cloud (src/sg-slam/src/PointcloudMapping.cc:332-360) behind the C ABI: the handle owns the map, its
// device count and the consolidation workspace; append_batch_dev and consolidate_dev enqueue the kernels of sgx_globalmap_kernels.h on the caller's stream and read
// nothing back; the synchronous entries are the same launches fed from host memory.  The schedule (count, pending, threshold) is the caller's host code.
#include "sgx_globalmap_kernels.h"
#include "sgx_devmem.h"
#include "../../include/sgx.h"
#include <math.h>
#include <stdio.h>
#include <string.h>
#include <vector>
#ifdef SGX_DEBUG_TAPS
#include "../../include/sgx_debug.h"      // test taps: compiled into tests/taps/libsgx_taps.so and the emulator only
#endif

static_assert(sizeof(SgxGmapResult) == sizeof(sgx_globalmap_result) && sizeof(SgxGmapAppendRecord) == sizeof(sgx_globalmap_append_record) &&
              sizeof(SgxCloudPoint) == sizeof(sgx_cloud_point), "the kernels write the records of sgx.h");
static_assert(SGX_GMAP_FEW_POINTS == SGX_CLOUD_FEW_POINTS && SGX_GMAP_LEAF_TOO_SMALL == SGX_CLOUD_LEAF_TOO_SMALL && SGX_GMAP_FULL == 4, "the flags the kernels set");
static_assert(SGX_GMAP_RCAP == SGX_GMAP_MAX_RADIUS, "the widest window");

struct sgx_globalmap {
    sgx_globalmap_params p;
    int cap = 0, tiles = 0, nblk = 0, max_radius = SGX_GMAP_RCAP;
    SgxGmapArgs G;                                                                             // the map's pointers and the derived parameters
    SgxCloudGrid *grid = nullptr;                                                             // 2: the VoxelGrid, the search grid
    int32_t *one_n = nullptr; SgxGmapAppendRecord *one_arec = nullptr; SgxGmapResult *one_result = nullptr;      // the synchronous entries' staging
    SgxDevMem mem;
};

static bool gmap_finite(double v) { return v == v && v - v == 0; }

extern "C" int sgx_globalmap_create(int max_points, const sgx_globalmap_params *params, sgx_globalmap **out)
{
    if (out) *out = nullptr;
    if (!out || !params || max_points < 1 || max_points > SGX_GMAP_MAX_POINTS) return SGX_ERR_INVALID;
    if (params->sor_mean_k < 1 || !gmap_finite(params->voxel_leaf_size) || !(params->voxel_leaf_size > 0) || params->sor_stddev_mul != params->sor_stddev_mul) return SGX_ERR_INVALID;
    sgx_globalmap *h = new sgx_globalmap;
    h->p = *params; h->cap = max_points;
    h->tiles = (max_points + SGX_CLOUD_TILE - 1) / SGX_CLOUD_TILE; h->nblk = (max_points + 255) / 256;
    const size_t P = (size_t)max_points, T = (size_t)(16 * h->tiles > h->nblk ? 16 * h->tiles : h->nblk);
    SgxGmapArgs &G = h->G; memset(&G, 0, sizeof G);
    SgxCloudArgs &A = G.C;
    SgxDevMem &m = h->mem;
    int rc;
    if ((rc = m.alloc(&A.pts, P)) || (rc = m.alloc(&A.spts, P)) || (rc = m.alloc(&A.vox, P)) || (rc = m.alloc(&A.k0, P)) || (rc = m.alloc(&A.k1, P)) ||
        (rc = m.alloc(&A.v0, P)) || (rc = m.alloc(&A.v1, P)) || (rc = m.alloc(&A.tab, T)) || (rc = m.alloc(&A.vstart, P + 1)) || (rc = m.alloc(&A.ci, SGX_CLOUD_CI)) ||
        (rc = m.alloc(&A.dist, P)) || (rc = m.alloc(&A.cd, 2)) || (rc = m.alloc(&h->grid, 2)) || (rc = m.alloc(&G.count, 1)) || (rc = m.alloc(&G.wlist, P)) ||
        (rc = m.alloc(&G.tier, P)) || (rc = m.alloc(&h->one_n, 1)) || (rc = m.alloc(&h->one_arec, 1)) || (rc = m.alloc(&h->one_result, 1))) { delete h; return rc; }
    A.B = 1; A.N = max_points; A.mode = 1; A.out = A.pts; A.tiles = h->tiles; A.nblk = h->nblk;
    A.mean_k = params->sor_mean_k; A.leaf = params->voxel_leaf_size; A.mul = params->sor_stddev_mul;
    int r0 = 1; while ((2 * r0 + 1) * (2 * r0 + 1) < 2 * (A.mean_k + 1) && r0 < SGX_CLOUD_RMAX) r0++;         // §9f's rule: the first window's rows hold twice the neighbours asked for
    A.r0 = r0;
    G.cap = max_points;
    if (hipMemset(G.count, 0, sizeof(int)) != hipSuccess || hipMemset(A.ci, 0, sizeof(int) * SGX_CLOUD_CI) != hipSuccess || hipMemset(A.cd, 0, 2 * sizeof(double)) != hipSuccess) {
        delete h; return SGX_ERR_DEVICE;
    }
    *out = h;
    return SGX_OK;
}

extern "C" void sgx_globalmap_destroy(sgx_globalmap *h) { delete h; }

extern "C" int sgx_globalmap_reset(sgx_globalmap *h)
{
    if (!h) return SGX_ERR_INVALID;
    SGX_LAUNCH(k_gmap_reset, dim3(1), dim3(64), (sgx_stream_t)0, h->G);
    SGX_CHECK_HIP(hipGetLastError());
    SGX_CHECK_HIP(hipStreamSynchronize((sgx_stream_t)0));
    return SGX_OK;
}

extern "C" int sgx_globalmap_append_batch_dev(sgx_globalmap *h, const sgx_cloud_point *points_dev, int64_t point_stride, const int32_t *n_points_dev, int64_t n_points_stride_bytes,
                                              int n_clouds, sgx_globalmap_append_record *records_dev, void *stream)
{
    if (!h || !points_dev || !n_points_dev || !records_dev || n_clouds < 1 || n_clouds > 65535 || point_stride < 0 || n_points_stride_bytes < 0 || (n_points_stride_bytes & 3))
        return SGX_ERR_INVALID;
    const sgx_stream_t s = (sgx_stream_t)stream;
    SgxGmapArgs G = h->G;
    G.src = (const SgxCloudPoint *)points_dev; G.src_stride = point_stride; G.n_src = n_points_dev; G.n_stride = n_points_stride_bytes; G.n_clouds = n_clouds;
    G.arec = (SgxGmapAppendRecord *)records_dev;
    const unsigned nb = (unsigned)(h->nblk < 1024 ? h->nblk : 1024);
    SGX_LAUNCH(k_gmap_append_plan, dim3(1), dim3(64), s, G);
    SGX_LAUNCH(k_gmap_append_copy, dim3(nb, (unsigned)n_clouds), dim3(256), s, G);
    SGX_CHECK_HIP(hipGetLastError());
    return SGX_OK;
}

extern "C" int sgx_globalmap_append(sgx_globalmap *h, const sgx_cloud_point *points, int n_points, sgx_globalmap_append_record *record)
{
    if (!h || n_points < 0 || (n_points > 0 && !points) || !record) return SGX_ERR_INVALID;
    const int take = n_points <= h->cap ? n_points : 0;                                        // a cloud beyond the capacity is refused whole: nothing to stage
    SgxCloudPoint *dev = nullptr;
    int rc = h->mem.alloc(&dev, (size_t)take);
    if (rc != SGX_OK) return rc;
    const int32_t n = n_points;
    if ((take && hipMemcpy(dev, points, sizeof(SgxCloudPoint) * (size_t)take, hipMemcpyHostToDevice) != hipSuccess) ||
        hipMemcpy(h->one_n, &n, 4, hipMemcpyHostToDevice) != hipSuccess) rc = SGX_ERR_DEVICE;
    if (rc == SGX_OK) rc = sgx_globalmap_append_batch_dev(h, (const sgx_cloud_point *)dev, 0, h->one_n, 0, 1, (sgx_globalmap_append_record *)h->one_arec, nullptr);
    if (rc == SGX_OK && (hipStreamSynchronize((sgx_stream_t)0) != hipSuccess ||
                         hipMemcpy(record, h->one_arec, sizeof(SgxGmapAppendRecord), hipMemcpyDeviceToHost) != hipSuccess)) rc = SGX_ERR_DEVICE;
    h->mem.release(dev);
    return rc;
}

extern "C" int sgx_globalmap_consolidate_dev(sgx_globalmap *h, sgx_globalmap_result *result_dev, void *stream)
{
    if (!h || !result_dev) return SGX_ERR_INVALID;
    const sgx_stream_t s = (sgx_stream_t)stream;
    SgxGmapArgs G = h->G;
    SgxCloudArgs &A = G.C;
    G.result = (SgxGmapResult *)result_dev; G.max_radius = h->max_radius;
    const dim3 one(1), points((unsigned)h->nblk, 1), tiles((unsigned)h->tiles, 1), lanes((unsigned)((h->cap + 63) / 64), 1);
    SGX_LAUNCH(k_gmap_prep, one, dim3(64), s, G);
    SGX_LAUNCH(k_gmap_extremes, dim3((unsigned)h->nblk), dim3(256), s, G);
    for (int stage = 0; stage < 2; stage++) {
        A.stage = stage; A.g = h->grid + stage;
        SGX_LAUNCH(k_gmap_grid, one, dim3(64), s, G);
        SGX_LAUNCH(k_cloud_keys, points, dim3(256), s, A);
        for (int pass = 0; pass < 8; pass++) {                                               // 8 x 4 bits; an even number of passes ends in k0 / v0
            A.shift = 4 * pass; A.cur = pass & 1; A.scan_len = 16 * h->tiles; A.scan_slot = -1;
            SGX_LAUNCH(k_cloud_hist, tiles, dim3(256), s, A);
            SGX_LAUNCH(k_cloud_scan, one, dim3(256), s, A);
            SGX_LAUNCH(k_cloud_scatter, tiles, dim3(256), s, A);
        }
        SGX_LAUNCH(k_cloud_gather, points, dim3(256), s, A);
        if (stage == 0) {
            A.scan_len = h->nblk; A.scan_slot = SGX_CLOUD_NVOX;
            SGX_LAUNCH(k_cloud_flagcount, points, dim3(256), s, A);
            SGX_LAUNCH(k_cloud_scan, one, dim3(256), s, A);
            SGX_LAUNCH(k_cloud_flagapply, points, dim3(256), s, A);
            SGX_LAUNCH(k_cloud_centroid, lanes, dim3(64), s, A);
        }
    }
    SGX_LAUNCH(k_gmap_sor, dim3(lanes.x), dim3(64), s, G);
    SGX_LAUNCH(k_gmap_sor_wide, dim3(1024), dim3(256), s, G);
    SGX_LAUNCH(k_cloud_sor_whole, dim3(256, 1), dim3(256), s, A);
    SGX_LAUNCH(k_cloud_stats, one, dim3(256), s, A);
    A.scan_len = h->nblk; A.scan_slot = SGX_CLOUD_KEPT;                                       // keep / stable compaction back into the map (WORLD mode: no axis map)
    SGX_LAUNCH(k_cloud_flagcount, points, dim3(256), s, A);
    SGX_LAUNCH(k_cloud_scan, one, dim3(256), s, A);
    SGX_LAUNCH(k_cloud_flagapply, points, dim3(256), s, A);
    SGX_LAUNCH(k_gmap_commit, one, dim3(64), s, G);
    SGX_CHECK_HIP(hipGetLastError());
    return SGX_OK;
}

extern "C" int sgx_globalmap_consolidate(sgx_globalmap *h, sgx_globalmap_result *result)
{
    if (!h || !result) return SGX_ERR_INVALID;
    const int rc = sgx_globalmap_consolidate_dev(h, (sgx_globalmap_result *)h->one_result, nullptr);
    if (rc != SGX_OK) return rc;
    SGX_CHECK_HIP(hipStreamSynchronize((sgx_stream_t)0));
    SGX_CHECK_HIP(hipMemcpy(result, h->one_result, sizeof(SgxGmapResult), hipMemcpyDeviceToHost));
    return SGX_OK;
}

extern "C" int sgx_globalmap_size(sgx_globalmap *h, int32_t *n_points)
{
    if (!h || !n_points) return SGX_ERR_INVALID;
    SGX_CHECK_HIP(hipStreamSynchronize((sgx_stream_t)0));
    int32_t n = 0;
    SGX_CHECK_HIP(hipMemcpy(&n, h->G.count, 4, hipMemcpyDeviceToHost));
    if (n < 0 || n > h->cap) return SGX_ERR_DEVICE;
    *n_points = n;
    return SGX_OK;
}

extern "C" int sgx_globalmap_read(sgx_globalmap *h, sgx_cloud_point *points, int cap, int32_t *n_points)
{
    if (!h || cap < 0 || (cap > 0 && !points) || !n_points) return SGX_ERR_INVALID;
    const int rc = sgx_globalmap_size(h, n_points);
    if (rc != SGX_OK) return rc;
    const int take = *n_points < cap ? *n_points : cap;
    if (take > 0) SGX_CHECK_HIP(hipMemcpy(points, h->G.C.pts, sizeof(SgxCloudPoint) * (size_t)take, hipMemcpyDeviceToHost));
    return *n_points > cap ? SGX_ERR_OVERFLOW : SGX_OK;
}

extern "C" int sgx_globalmap_points_dev(sgx_globalmap *h, const sgx_cloud_point **points_dev, const int32_t **n_points_dev)
{
    if (!h || !points_dev || !n_points_dev) return SGX_ERR_INVALID;
    *points_dev = (const sgx_cloud_point *)h->G.C.pts; *n_points_dev = h->G.count;
    return SGX_OK;
}

#ifdef SGX_DEBUG_TAPS
// test tap: the voxel cloud of the handle's last consolidation before the outlier filter, its distances, kept flags and window tiers.  Synchronises the device.
SGX_TAP int sgx_globalmap_debug_read(sgx_globalmap *h, sgx_cloud_point *voxels, float *dist, uint8_t *kept, uint8_t *tier, int cap, int *n)
{
    if (!h || !n || cap < 0) return SGX_ERR_INVALID;
    SGX_CHECK_HIP(hipDeviceSynchronize());
    int ci[SGX_CLOUD_CI]; double cd[2];
    SGX_CHECK_HIP(hipMemcpy(ci, h->G.C.ci, sizeof ci, hipMemcpyDeviceToHost));
    SGX_CHECK_HIP(hipMemcpy(cd, h->G.C.cd, sizeof cd, hipMemcpyDeviceToHost));
    const int nv = ci[SGX_CLOUD_NVOX];
    if (nv < 0 || nv > h->cap) return SGX_ERR_DEVICE;
    *n = nv;
    if (nv > cap) return SGX_ERR_OVERFLOW;
    if (nv == 0) return SGX_OK;
    if (voxels) SGX_CHECK_HIP(hipMemcpy(voxels, h->G.C.vox, sizeof(SgxCloudPoint) * (size_t)nv, hipMemcpyDeviceToHost));
    std::vector<float> d((size_t)nv, 0.0f);
    const bool filtered = nv > h->p.sor_mean_k;                                                // otherwise no distance was computed
    if (filtered) SGX_CHECK_HIP(hipMemcpy(d.data(), h->G.C.dist, 4 * (size_t)nv, hipMemcpyDeviceToHost));
    if (tier) { if (filtered) SGX_CHECK_HIP(hipMemcpy(tier, h->G.tier, (size_t)nv, hipMemcpyDeviceToHost)); else memset(tier, 0, (size_t)nv); }
    for (int i = 0; i < nv; i++) {
        if (dist) dist[i] = d[(size_t)i];
        if (kept) kept[i] = filtered && !((double)d[(size_t)i] > cd[1]) ? 1 : 0;
    }
    return SGX_OK;
}

// test tap: the widest window k_gmap_sor_wide may try (default SGX_GMAP_MAX_RADIUS); at or below the first window every not-proven point searches the whole cloud
SGX_TAP int sgx_globalmap_debug_max_radius(sgx_globalmap *h, int max_radius)
{
    if (!h || max_radius < 0 || max_radius > SGX_GMAP_RCAP) return SGX_ERR_INVALID;
    h->max_radius = max_radius;
    return SGX_OK;
}
#endif
