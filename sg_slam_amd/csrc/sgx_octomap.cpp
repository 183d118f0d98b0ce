// sgx_octomap.cpp — host side of the occupancy map (octomap_server's insertCloudCallback / insertScan / publishAll, src/octomap_server/src/OctomapServer.cpp) behind
// the C ABI: the handle owns the brick table, the bricks and the query workspace; insert_batch_dev enqueues the kernels of sgx_octomap_kernels.h scan after scan on the
// caller's stream and reads nothing back; the synchronous entries are the same launches fed from host memory.  grid_header and sensor_to_world are host code.
#include "sgx_octomap_kernels.h"
#include "sgx_devmem.h"
#include "../../include/sgx.h"
#include <math.h>
#include <stdio.h>
#include <string.h>

static_assert(sizeof(SgxOctoRecord) == sizeof(sgx_octomap_record) && sizeof(SgxOctoCell) == sizeof(sgx_octomap_cell) && sizeof(SgxOctoBounds) == sizeof(sgx_octomap_bounds_t) &&
              sizeof(SgxOctoPoint) == sizeof(sgx_cloud_point), "the kernels write the records of sgx.h");
static_assert(OCTO_ORIGIN_OUT_OF_RANGE == SGX_OCTOMAP_ORIGIN_OUT_OF_RANGE && OCTO_RAY_LEFT_KEYSPACE == SGX_OCTOMAP_RAY_LEFT_KEYSPACE && OCTO_MAP_FULL == SGX_OCTOMAP_MAP_FULL &&
              OCTO_TOO_MANY_POINTS == SGX_OCTOMAP_TOO_MANY_POINTS, "the flags of sgx.h");

struct sgx_octomap {
    sgx_octomap_params p;
    int max_bricks = 0, max_points = 0, T = 0;
    SgxOctoArgs A;                                                                             // the map's pointers and the derived parameters
    SgxOctoPoint *one_points = nullptr; int32_t *one_n = nullptr; float *one_s2w = nullptr; SgxOctoRecord *one_rec = nullptr; SgxOctoBounds *one_bounds = nullptr;
    SgxDevMem mem;
};

static bool octo_fin(double v) { return v == v && v - v == 0; }
static bool octo_prob(double v) { return v > 0.0 && v < 1.0; }
static float octo_logodds(double p) { return (float)log(p / (1.0 - p)); }

static int octo_reset(sgx_octomap *h, sgx_stream_t s)
{
    const unsigned n = (unsigned)((h->T > OCTO_STATE_INTS ? h->T : OCTO_STATE_INTS) + 255) / 256;
    SGX_LAUNCH(k_octo_reset, dim3(n), dim3(256), s, h->A);
    SGX_CHECK_HIP(hipGetLastError());
    return SGX_OK;
}

extern "C" int sgx_octomap_create(const sgx_octomap_params *p, int max_bricks, int max_points_per_scan, sgx_octomap **out)
{
    if (out) *out = nullptr;
    if (!out || !p || max_bricks < 1 || max_bricks > (1 << 17) || max_points_per_scan < 1 || max_points_per_scan > (1 << 24)) return SGX_ERR_INVALID;
    if (!octo_fin(p->res) || !(p->res > 0) || !octo_prob(p->prob_hit) || !octo_prob(p->prob_miss) || !octo_prob(p->thres_min) || !octo_prob(p->thres_max) ||
        !(p->thres_min < p->thres_max)) return SGX_ERR_INVALID;
    const double bounds[] = { p->max_range, p->pointcloud_min_x, p->pointcloud_max_x, p->pointcloud_min_y, p->pointcloud_max_y, p->pointcloud_min_z, p->pointcloud_max_z,
                              p->occupancy_min_z, p->occupancy_max_z, p->min_size_x, p->min_size_y };
    for (double b : bounds) if (b != b) return SGX_ERR_INVALID;
    sgx_octomap *h = new sgx_octomap;
    h->p = *p; h->max_bricks = max_bricks; h->max_points = max_points_per_scan;
    int T = 64; while (T < 2 * max_bricks) T *= 2;
    h->T = T;
    SgxOctoArgs &A = h->A; memset(&A, 0, sizeof A);
    SgxDevMem &m = h->mem;
    int rc;
    if ((rc = m.alloc(&A.tab_key, (size_t)T)) || (rc = m.alloc(&A.tab_idx, (size_t)T)) || (rc = m.alloc(&A.fmask, 16 * (size_t)T)) || (rc = m.alloc(&A.omask, 16 * (size_t)T)) ||
        (rc = m.alloc(&A.cells, 512 * (size_t)max_bricks)) || (rc = m.alloc(&A.brick_key, (size_t)max_bricks)) || (rc = m.alloc(&A.st, (size_t)OCTO_STATE_INTS)) ||
        (rc = m.alloc(&A.touched, (size_t)T)) || (rc = m.alloc(&A.rays, (size_t)h->max_points)) || (rc = m.alloc(&A.morton, (size_t)max_bricks)) ||
        (rc = m.alloc(&A.order, (size_t)max_bricks)) || (rc = m.alloc(&A.cnt, (size_t)max_bricks)) ||
        (rc = m.alloc(&h->one_points, (size_t)h->max_points)) || (rc = m.alloc(&h->one_n, 2)) || (rc = m.alloc(&h->one_s2w, 16)) || (rc = m.alloc(&h->one_rec, 1)) ||
        (rc = m.alloc(&h->one_bounds, 1))) { delete h; return rc; }
    A.T = T; A.max_bricks = max_bricks; A.max_points = h->max_points;
    A.res = p->res; A.rf = 1.0 / p->res; A.max_range = p->max_range;
    A.hit = octo_logodds(p->prob_hit); A.miss = octo_logodds(p->prob_miss); A.cmin = octo_logodds(p->thres_min); A.cmax = octo_logodds(p->thres_max);
    A.lo[0] = (float)p->pointcloud_min_x; A.hi[0] = (float)p->pointcloud_max_x; A.lo[1] = (float)p->pointcloud_min_y; A.hi[1] = (float)p->pointcloud_max_y;
    A.lo[2] = (float)p->pointcloud_min_z; A.hi[2] = (float)p->pointcloud_max_z;
    A.zmin = p->occupancy_min_z; A.zmax = p->occupancy_max_z;
    if ((rc = octo_reset(h, nullptr)) != SGX_OK || hipStreamSynchronize((sgx_stream_t)0) != hipSuccess) { delete h; return rc ? rc : SGX_ERR_DEVICE; }
    *out = h;
    return SGX_OK;
}

extern "C" void sgx_octomap_destroy(sgx_octomap *h) { delete h; }

extern "C" int sgx_octomap_reset(sgx_octomap *h)
{
    if (!h) return SGX_ERR_INVALID;
    const int rc = octo_reset(h, nullptr);
    if (rc != SGX_OK) return rc;
    SGX_CHECK_HIP(hipStreamSynchronize((sgx_stream_t)0));
    return SGX_OK;
}

extern "C" int sgx_octomap_insert_batch_dev(sgx_octomap *h, const sgx_cloud_point *points_dev, int64_t point_stride, const int32_t *n_points_dev, int64_t n_points_stride_bytes,
                                            const float *sensor_to_world_dev, int n_scans, sgx_octomap_record *records_dev, void *stream)
{
    if (!h || !points_dev || !n_points_dev || !sensor_to_world_dev || !records_dev || n_scans < 1 || point_stride < 0 || n_points_stride_bytes < 0 ||
        (n_points_stride_bytes & 3)) return SGX_ERR_INVALID;
    const sgx_stream_t s = (sgx_stream_t)stream;
    SgxOctoArgs A = h->A;
    const unsigned T = (unsigned)h->T, P = (unsigned)h->max_points;
    const dim3 one(1), pts((P + 255) / 256), rays((P + 63) / 64), slots((T + 255) / 256), bricks(T < 1024 ? T : 1024), enter(((unsigned)h->max_bricks + 255) / 256);
    for (int i = 0; i < n_scans; i++) {
        A.points = (const SgxOctoPoint *)points_dev + (size_t)i * (size_t)point_stride;
        A.n_points = (const int32_t *)((const char *)n_points_dev + (size_t)i * (size_t)n_points_stride_bytes);
        A.s2w = sensor_to_world_dev + 16 * (size_t)i;
        A.record = (SgxOctoRecord *)records_dev + i;
        SGX_LAUNCH(k_octo_begin, one, dim3(64), s, A);
        SGX_LAUNCH(k_octo_points, pts, dim3(256), s, A);
        SGX_LAUNCH(k_octo_rays, rays, dim3(64), s, A);
        SGX_LAUNCH(k_octo_assign, slots, dim3(256), s, A);
        SGX_LAUNCH(k_octo_apply, bricks, dim3(64), s, A);
        SGX_LAUNCH(k_octo_finish, one, dim3(64), s, A);
        SGX_LAUNCH(k_octo_rollback_clear, slots, dim3(256), s, A);
        SGX_LAUNCH(k_octo_rollback_enter, enter, dim3(256), s, A);
    }
    SGX_CHECK_HIP(hipGetLastError());
    return SGX_OK;
}

extern "C" int sgx_octomap_insert(sgx_octomap *h, const sgx_cloud_point *points, int n_points, const float *sensor_to_world, sgx_octomap_record *record)
{
    if (!h || n_points < 0 || (n_points > 0 && !points) || !sensor_to_world || !record) return SGX_ERR_INVALID;
    for (int i = 0; i < 16; i++) if (sensor_to_world[i] != sensor_to_world[i]) return SGX_ERR_INVALID;
    const int take = n_points < h->max_points ? n_points : h->max_points;
    const int32_t n = n_points;
    if (take) SGX_CHECK_HIP(hipMemcpy(h->one_points, points, sizeof(SgxOctoPoint) * (size_t)take, hipMemcpyHostToDevice));
    SGX_CHECK_HIP(hipMemcpy(h->one_n, &n, 4, hipMemcpyHostToDevice));
    SGX_CHECK_HIP(hipMemcpy(h->one_s2w, sensor_to_world, 64, hipMemcpyHostToDevice));
    const int rc = sgx_octomap_insert_batch_dev(h, (const sgx_cloud_point *)h->one_points, 0, h->one_n, 0, h->one_s2w, 1, (sgx_octomap_record *)h->one_rec, nullptr);
    if (rc != SGX_OK) return rc;
    SGX_CHECK_HIP(hipStreamSynchronize((sgx_stream_t)0));
    SGX_CHECK_HIP(hipMemcpy(record, h->one_rec, sizeof(SgxOctoRecord), hipMemcpyDeviceToHost));
    return SGX_OK;
}

extern "C" int sgx_octomap_bounds(sgx_octomap *h, sgx_octomap_bounds_t *out)
{
    if (!h || !out) return SGX_ERR_INVALID;
    SgxOctoArgs A = h->A; A.bounds = h->one_bounds;
    const unsigned nb = (unsigned)(h->max_bricks < 1024 ? h->max_bricks : 1024);
    SGX_LAUNCH(k_octo_bounds_init, dim3(1), dim3(64), (sgx_stream_t)0, A);
    SGX_LAUNCH(k_octo_bounds, dim3(nb), dim3(64), (sgx_stream_t)0, A);
    SGX_CHECK_HIP(hipGetLastError());
    SGX_CHECK_HIP(hipStreamSynchronize((sgx_stream_t)0));
    SGX_CHECK_HIP(hipMemcpy(out, h->one_bounds, sizeof(SgxOctoBounds), hipMemcpyDeviceToHost));
    return SGX_OK;
}

extern "C" int sgx_octomap_cells_dev(sgx_octomap *h, int occupied, sgx_octomap_cell *cells_dev, int cap, int32_t *n_cells_dev, void *stream)
{
    if (!h || cap < 0 || (cap > 0 && !cells_dev) || !n_cells_dev) return SGX_ERR_INVALID;
    const sgx_stream_t s = (sgx_stream_t)stream;
    SgxOctoArgs A = h->A; A.want_occupied = occupied ? 1 : 0; A.cap = cap; A.out = (SgxOctoCell *)cells_dev; A.n_out = n_cells_dev;
    const unsigned B = (unsigned)h->max_bricks, nb = B < 2048 ? B : 2048;
    SGX_LAUNCH(k_octo_morton, dim3((B + 255) / 256), dim3(256), s, A);
    SGX_LAUNCH(k_octo_rank, dim3(nb), dim3(64), s, A);
    SGX_LAUNCH(k_octo_scan, dim3(1), dim3(256), s, A);
    SGX_LAUNCH(k_octo_cells, dim3(nb), dim3(64), s, A);
    SGX_CHECK_HIP(hipGetLastError());
    return SGX_OK;
}

extern "C" int sgx_octomap_cells(sgx_octomap *h, int occupied, sgx_octomap_cell *cells, int cap, int32_t *n_cells)
{
    if (!h || cap < 0 || (cap > 0 && !cells) || !n_cells) return SGX_ERR_INVALID;
    SgxOctoCell *dev = nullptr;
    int rc = h->mem.alloc(&dev, (size_t)cap);
    if (rc != SGX_OK) return rc;
    rc = sgx_octomap_cells_dev(h, occupied, (sgx_octomap_cell *)dev, cap, h->one_n + 1, nullptr);
    int32_t n = 0;
    if (rc == SGX_OK && (hipStreamSynchronize((sgx_stream_t)0) != hipSuccess || hipMemcpy(&n, h->one_n + 1, 4, hipMemcpyDeviceToHost) != hipSuccess)) rc = SGX_ERR_DEVICE;
    if (rc == SGX_OK) {
        *n_cells = n;
        const int take = n < cap ? n : cap;
        if (take > 0 && hipMemcpy(cells, dev, sizeof(SgxOctoCell) * (size_t)take, hipMemcpyDeviceToHost) != hipSuccess) rc = SGX_ERR_DEVICE;
        else if (n > cap) rc = SGX_ERR_OVERFLOW;
    }
    h->mem.release(dev);
    return rc;
}

extern "C" int sgx_octomap_search_dev(sgx_octomap *h, const uint16_t *keys_dev, const float *points_dev, int m, float *logodds_dev, void *stream)
{
    if (!h || m < 0 || (!keys_dev) == (!points_dev) || !logodds_dev) return SGX_ERR_INVALID;
    if (m == 0) return SGX_OK;
    SgxOctoArgs A = h->A; A.qkeys = keys_dev; A.qpts = points_dev; A.m = m; A.qout = logodds_dev;
    SGX_LAUNCH(k_octo_search, dim3(((unsigned)m + 255) / 256), dim3(256), (sgx_stream_t)stream, A);
    SGX_CHECK_HIP(hipGetLastError());
    return SGX_OK;
}

// handlePreNodeTraversal (:942-990) from the bounds at leaf level
extern "C" int sgx_octomap_grid_header(const sgx_octomap *h, const sgx_octomap_bounds_t *b, sgx_octomap_grid_header_t *out)
{
    if (!h || !b || !out) return SGX_ERR_INVALID;
    memset(out, 0, sizeof *out);
    const double res = h->p.res, rf = 1.0 / res;
    out->resolution = res;
    if (b->n_known <= 0) { out->flags = SGX_OCTOMAP_GRID_EMPTY; return SGX_OK; }
    double lo[3], hi[3];
    for (int a = 0; a < 3; a++) {
        if (b->key_min[a] < 0 || b->key_max[a] > 65535 || b->key_min[a] > b->key_max[a]) return SGX_ERR_INVALID;
        lo[a] = octo_coord(res, b->key_min[a]) - res / 2.0; hi[a] = octo_coord(res, b->key_max[a]) - res / 2.0 + res;
    }
    const double hp[2] = { 0.5 * h->p.min_size_x, 0.5 * h->p.min_size_y };
    for (int a = 0; a < 2; a++) { lo[a] = lo[a] < -hp[a] ? lo[a] : -hp[a]; hi[a] = hi[a] > hp[a] ? hi[a] : hp[a]; }
    int kmin[3], kmax[3]; bool ok = true;
    for (int a = 0; a < 3; a++) { ok = octo_key1(rf, (float)lo[a], &kmin[a]) && ok; ok = octo_key1(rf, (float)hi[a], &kmax[a]) && ok; }
    if (!ok) { out->flags = SGX_OCTOMAP_GRID_KEY_OUT_OF_RANGE; return SGX_OK; }
    for (int a = 0; a < 2; a++) { out->pad_min_key[a] = kmin[a]; out->pad_max_key[a] = kmax[a]; }
    out->width = kmax[0] - kmin[0] + 1; out->height = kmax[1] - kmin[1] + 1;
    if (out->width < 1 || out->height < 1) { out->width = out->height = 0; out->flags = SGX_OCTOMAP_GRID_KEY_OUT_OF_RANGE; return SGX_OK; }
    out->key_min_z = b->key_min[2]; out->key_max_z = b->key_max[2];
    out->origin_x = (double)(float)octo_coord(res, kmin[0]) - res * 0.5;                     // keyToCoord(OcTreeKey) is a point3d: floats
    out->origin_y = (double)(float)octo_coord(res, kmin[1]) - res * 0.5;
    return SGX_OK;
}

extern "C" int sgx_octomap_project_dev(sgx_octomap *h, const sgx_octomap_grid_header_t *hd, int8_t *grid_dev, void *stream)
{
    if (!h || !hd || hd->width < 0 || hd->height < 0 || hd->width > 65536 || hd->height > 65536) return SGX_ERR_INVALID;
    const long long n = (long long)hd->width * hd->height;
    if (n == 0) return SGX_OK;
    if (!grid_dev || hd->pad_min_key[0] < 0 || hd->pad_min_key[1] < 0 || hd->pad_min_key[0] + hd->width > 65536 || hd->pad_min_key[1] + hd->height > 65536 ||
        hd->key_min_z < 0 || hd->key_max_z > 65535) return SGX_ERR_INVALID;
    SgxOctoArgs A = h->A; A.grid = grid_dev; A.gw = hd->width; A.gh = hd->height; A.gx0 = hd->pad_min_key[0]; A.gy0 = hd->pad_min_key[1]; A.gz0 = hd->key_min_z; A.gz1 = hd->key_max_z;
    SGX_LAUNCH(k_octo_project, dim3((unsigned)((n + 255) / 256)), dim3(256), (sgx_stream_t)stream, A);
    SGX_CHECK_HIP(hipGetLastError());
    return SGX_OK;
}

extern "C" int sgx_octomap_project(sgx_octomap *h, sgx_octomap_grid_header_t *header, int8_t *grid, int64_t cap)
{
    if (!h || !header || cap < 0 || (cap > 0 && !grid)) return SGX_ERR_INVALID;
    sgx_octomap_bounds_t b;
    int rc = sgx_octomap_bounds(h, &b);
    if (rc != SGX_OK || (rc = sgx_octomap_grid_header(h, &b, header)) != SGX_OK) return rc;
    const long long n = (long long)header->width * header->height;
    if (n == 0) return SGX_OK;
    if (n > cap) return SGX_ERR_OVERFLOW;
    int8_t *dev = nullptr;
    if ((rc = h->mem.alloc(&dev, (size_t)n)) != SGX_OK) return rc;
    rc = sgx_octomap_project_dev(h, header, dev, nullptr);
    if (rc == SGX_OK && (hipStreamSynchronize((sgx_stream_t)0) != hipSuccess || hipMemcpy(grid, dev, (size_t)n, hipMemcpyDeviceToHost) != hipSuccess)) rc = SGX_ERR_DEVICE;
    h->mem.release(dev);
    return rc;
}

// tf::Transform(tf::Quaternion, tf::Vector3) as pcl_ros::transformAsMatrix writes it: tf::Matrix3x3::setRotation in double, every entry cast to float
extern "C" int sgx_octomap_sensor_to_world(const double origin[3], const double rotation[4], float out[16])
{
    if (!origin || !rotation || !out) return SGX_ERR_INVALID;
    const double x = rotation[0], y = rotation[1], z = rotation[2], w = rotation[3];
    const double d = x * x + y * y + z * z + w * w;
    if (!octo_fin(d) || !(d > 0) || !octo_fin(origin[0]) || !octo_fin(origin[1]) || !octo_fin(origin[2])) return SGX_ERR_INVALID;
    const double s = 2.0 / d;
    const double xs = x * s, ys = y * s, zs = z * s, wx = w * xs, wy = w * ys, wz = w * zs, xx = x * xs, xy = x * ys, xz = x * zs, yy = y * ys, yz = y * zs, zz = z * zs;
    const double m[9] = { 1.0 - (yy + zz), xy - wz, xz + wy, xy + wz, 1.0 - (xx + zz), yz - wx, xz - wy, yz + wx, 1.0 - (xx + yy) };
    for (int r = 0; r < 3; r++) { for (int c = 0; c < 3; c++) out[4 * r + c] = (float)m[3 * r + c]; out[4 * r + 3] = (float)origin[r]; }
    out[12] = out[13] = out[14] = 0.0f; out[15] = 1.0f;
    return SGX_OK;
}
