// sgx_cloud_kernels.h — the cloud of a keyframe (PointCloudMapping::generatePointCloud*, src/sg-slam/src/PointcloudMapping.cc:69-194, and MapViewer's voxel_local /
// sor_local, voxel_global / sor_global filters, :252-286, :332-338) on the device: every pixel as a coloured point, pcl::VoxelGrid by a stable radix sort of
// (idx, point), the voxel centroids as running float sums in ascending point order, pcl::StatisticalOutlierRemoval on the voxel cloud with the sorted cloud as its
// own search structure, the stable compaction of the survivors and the axis map.  One launch sequence for B keyframes (grid.y = keyframe), no host read-back.
// DESIGN.md §9f has the semantics, the defined cases and the window proof.
#pragma once
#include "sgx_rt.h"
#include <math.h>

#define SGX_CLOUD_CI 24                 /* ints per keyframe */
#define SGX_CLOUD_USED 0                /* pixels not skipped */
#define SGX_CLOUD_NVOX 1                /* voxel points */
#define SGX_CLOUD_LARGER 2              /* voxel points whose search left the first window */
#define SGX_CLOUD_KEPT 3                /* points written */
#define SGX_CLOUD_FLAGS 4
#define SGX_CLOUD_MM0 8                 /* ordered-int min x, y, z, max x, y, z of the cloud */
#define SGX_CLOUD_MM1 14                /* the same of the voxel cloud */
#define SGX_CLOUD_TILE 2048             /* keys per workgroup and radix pass: 256 lanes x 8 consecutive keys */
#define SGX_CLOUD_RMAX 5                /* largest cell window whose rows a lane keeps in LDS */
#define SGX_CLOUD_ROWS 121              /* (2 * RMAX + 1)^2 */
#define SGX_CLOUD_BOXES 128             /* = SGX_CLOUD_MAX_BOXES (include/sgx.h) */

struct SgxCloudPoint { float x, y, z; uint32_t rgba; };                                      // = sgx_cloud_point
struct SgxCloudResult { int n_points, n_pixels_used, n_voxels, flags, larger_window_points, reserved; double mean, thr; };      // = sgx_cloud_result
// the grid of one sort: stage 0 the VoxelGrid of the cloud, stage 1 the search grid of the voxel centroids.  n = keys to sort, total = div0 * div1 * div2 = the
// key of a point that is in no cell (it sorts behind every cell), ok = 0: no grid (refused, or nothing finite)
struct SgxCloudGrid { float inv; int min_b[3], div[3], total, ok, n; };

struct SgxCloudArgs {
    int B, W, H, N, dpitch, cpitch, max_boxes, mode, consider, mean_k, r0, tiles, nblk;      // N = W * H; tiles = radix tiles, nblk = 256-point blocks per keyframe
    int stage, shift, cur, scan_len, scan_slot;                                              // what changes between the launches of a sequence
    float fx, fy, cx, cy, dmin, dmax, leaf;
    double mul;
    const float *depth; const uint8_t *color; const double *twc; const float *boxes; const int *nboxes, *have;
    SgxCloudPoint *pts, *spts, *vox, *out;
    uint32_t *k0, *k1; int *v0, *v1, *tab, *vstart, *ci;
    float *dist; double *cd;                                                                 // cd: mean, thr per keyframe
    SgxCloudGrid *g;                                                                         // the grids of the current stage
    SgxCloudResult *results;
};

SGX_DEV float sgx_cloud_bits_f32(uint32_t b) { float f; __builtin_memcpy(&f, &b, 4); return f; }
SGX_DEV uint32_t sgx_cloud_f32_bits(float f) { uint32_t b; __builtin_memcpy(&b, &f, 4); return b; }
// floats in an integer order (-0 below +0), as in sgx_obj3d_kernels.h: min / max of them are integer atomics, exact and order-free
SGX_DEV int sgx_cloud_ordered(float f) { const int i = (int)sgx_cloud_f32_bits(f); return i < 0 ? (int)((uint32_t)i ^ 0x7fffffffu) : i; }
SGX_DEV float sgx_cloud_unordered(int i) { return sgx_cloud_bits_f32((uint32_t)(i < 0 ? (int)((uint32_t)i ^ 0x7fffffffu) : i)); }
// d2 as PCL's L2_Simple evaluates it in float: x, y, z order
SGX_DEV float sgx_cloud_d2(float ax, float ay, float az, float bx, float by, float bz)
{
    const float dx = ax - bx, dy = ay - by, dz = az - bz;
    return (dx * dx + dy * dy) + dz * dz;
}
SGX_DEV bool sgx_cloud_finite(float v) { return v - v == 0; }
// (int)f of the reference where it is defined; the nearest int where no int holds f, 0 for NaN
SGX_DEV int sgx_cloud_f2i(float f)
{
    if (!(f == f)) return 0;
    if (f >= 2147483648.0f) return 0x7fffffff;
    if (f <= -2147483648.0f) return (int)0x80000000;
    return (int)f;
}
SGX_DEV float sgx_cloud_pz(float v) { return v == 0 ? 0.0f : v; }                            // a zero of either sign as +0

// slam_to_ros_mode_transform (:364-375): (z, -x, -y)
SGX_DEV SgxCloudPoint sgx_cloud_ros(SgxCloudPoint p)
{
    SgxCloudPoint o; o.x = sgx_cloud_pz(p.z); o.y = sgx_cloud_pz(-p.x); o.z = sgx_cloud_pz(-p.y); o.rgba = p.rgba;
    return o;
}

SGX_KERNEL(64) k_cloud_prep(SgxCloudArgs A)
{
    SGX_THREADS_BEGIN(tid)
    const int f = (int)blockIdx.x * 64 + tid;
    if (f < A.B) {
        int *ci = A.ci + SGX_CLOUD_CI * f;
        for (int i = 0; i < SGX_CLOUD_CI; i++) ci[i] = 0;
        for (int i = 0; i < 3; i++) { ci[SGX_CLOUD_MM0 + i] = 0x7fffffff; ci[SGX_CLOUD_MM0 + 3 + i] = (int)0x80000000; ci[SGX_CLOUD_MM1 + i] = 0x7fffffff; ci[SGX_CLOUD_MM1 + 3 + i] = (int)0x80000000; }
        A.cd[2 * f] = 0; A.cd[2 * f + 1] = 0;
    }
    SGX_THREADS_END
}

// generatePointCloud / generatePointCloudForDyamic's camera_pc_ (:72-138, :163-183), transformPointCloud by Twc and the axis map in WORLD mode; the extremes of
// getMinMax3D as integer atomics on ordered ints (a workgroup reduces in LDS first)
SGX_KERNEL(256) k_cloud_points(SgxCloudArgs A)
{
    SGX_LDS int rect[4 * SGX_CLOUD_BOXES];
    SGX_LDS int red[8];
    const int f = (int)blockIdx.y;
    int nb = 0;
    if (A.consider && A.have && A.boxes && A.nboxes && A.have[f]) { nb = A.nboxes[f]; if (nb > A.max_boxes) nb = A.max_boxes; if (nb < 0) nb = 0; }
    SGX_THREADS_BEGIN(tid)
    for (int b = tid; b < nb; b += 256) {
        const float *r = A.boxes + 4 * ((size_t)f * A.max_boxes + b);
        rect[4 * b] = sgx_cloud_f2i(r[0]); rect[4 * b + 1] = sgx_cloud_f2i(r[0] + r[2]); rect[4 * b + 2] = sgx_cloud_f2i(r[1]); rect[4 * b + 3] = sgx_cloud_f2i(r[1] + r[3]);
    }
    if (tid < 3) red[tid] = 0x7fffffff; else if (tid < 6) red[tid] = (int)0x80000000; else if (tid == 6) red[6] = 0;
    SGX_THREADS_END
    SGX_SYNC();
    SGX_THREADS_BEGIN(tid)
    const int i = (int)blockIdx.x * 256 + tid;
    if (i < A.N) {
        const int m = i / A.W, n = i % A.W;
        const float d = A.depth[((size_t)f * A.H + m) * A.dpitch + n];
        bool skip = d < A.dmin || d > A.dmax || d != d;
        for (int b = 0; b < nb && !skip; b++) skip = n > rect[4 * b] && n < rect[4 * b + 1] && m > rect[4 * b + 2] && m < rect[4 * b + 3];
        SgxCloudPoint p; p.x = 0; p.y = 0; p.z = 0; p.rgba = 0xff000000u;
        if (!skip) {
            const uint8_t *c = A.color + ((size_t)f * A.H + m) * A.cpitch + 3 * n;
            p.z = d; p.x = ((float)n - A.cx) * d / A.fx; p.y = ((float)m - A.cy) * d / A.fy;
            p.rgba = 0xff000000u | (uint32_t)c[2] << 16 | (uint32_t)c[1] << 8 | (uint32_t)c[0];
            sgx_atomic_add(&red[6], 1);
        }
        if (A.mode == 1) {
            const double *T = A.twc + 16 * (size_t)f;
            const double x = (double)p.x, y = (double)p.y, z = (double)p.z;
            SgxCloudPoint w;
            w.x = (float)(((T[0] * x + T[1] * y) + T[2] * z) + T[3]);
            w.y = (float)(((T[4] * x + T[5] * y) + T[6] * z) + T[7]);
            w.z = (float)(((T[8] * x + T[9] * y) + T[10] * z) + T[11]);
            w.rgba = p.rgba;
            p = sgx_cloud_ros(w);
        }
        A.pts[(size_t)f * A.N + i] = p;
        if (sgx_cloud_finite(p.x) && sgx_cloud_finite(p.y) && sgx_cloud_finite(p.z)) {
            const int ox = sgx_cloud_ordered(p.x), oy = sgx_cloud_ordered(p.y), oz = sgx_cloud_ordered(p.z);
            sgx_atomic_min_i32(&red[0], ox); sgx_atomic_min_i32(&red[1], oy); sgx_atomic_min_i32(&red[2], oz);
            sgx_atomic_max(&red[3], ox); sgx_atomic_max(&red[4], oy); sgx_atomic_max(&red[5], oz);
        }
    }
    SGX_THREADS_END
    SGX_SYNC();
    SGX_THREADS_BEGIN(tid)
    int *ci = A.ci + SGX_CLOUD_CI * f;
    if (tid < 3) sgx_atomic_min_i32(&ci[SGX_CLOUD_MM0 + tid], red[tid]);
    else if (tid < 6) sgx_atomic_max(&ci[SGX_CLOUD_MM0 + tid], red[tid]);
    else if (tid == 6) sgx_atomic_add(&ci[SGX_CLOUD_USED], red[6]);
    SGX_THREADS_END
}

// VoxelGrid::applyFilter's header (min_b, div, the refusal test) from the extremes of the stage's points: one lane per keyframe
SGX_KERNEL(64) k_cloud_grid(SgxCloudArgs A)
{
    SGX_THREADS_BEGIN(tid)
    const int f = (int)blockIdx.x * 64 + tid;
    if (f < A.B) {
        int *ci = A.ci + SGX_CLOUD_CI * f;
        const int *mm = ci + (A.stage ? SGX_CLOUD_MM1 : SGX_CLOUD_MM0);
        SgxCloudGrid g;
        g.inv = 1.0f / A.leaf; g.total = 0; g.ok = 0; g.n = A.stage ? ci[SGX_CLOUD_NVOX] : 0;
        for (int a = 0; a < 3; a++) { g.min_b[a] = 0; g.div[a] = 1; }
        if (mm[0] <= mm[3]) {                                  // something finite
            bool bad = false;
            long long dd[3] = { 1, 1, 1 }, dv[3] = { 1, 1, 1 };
            for (int a = 0; a < 3; a++) {
                const float lo = sgx_cloud_unordered(mm[a]), hi = sgx_cloud_unordered(mm[3 + a]);
                const float ext = (hi - lo) * g.inv;
                const float bl = floorf(lo * g.inv), bh = floorf(hi * g.inv);
                if (!(ext < 2147483648.0f) || !(fabsf(bl) < 2147483648.0f) || !(fabsf(bh) < 2147483648.0f)) { bad = true; continue; }
                dd[a] = (long long)ext + 1;
                g.min_b[a] = (int)bl;
                dv[a] = (long long)(int)bh - (long long)(int)bl + 1;
            }
            if (!bad && (dd[0] * dd[1] > 0x7fffffffLL || dd[0] * dd[1] * dd[2] > 0x7fffffffLL)) bad = true;
            if (!bad && (dv[0] * dv[1] > 0x7fffffffLL || dv[0] * dv[1] * dv[2] > 0x7fffffffLL)) bad = true;
            if (!bad) {
                g.ok = 1; g.total = (int)(dv[0] * dv[1] * dv[2]);
                for (int a = 0; a < 3; a++) g.div[a] = (int)dv[a];
                if (!A.stage) g.n = A.N;
            } else if (!A.stage) ci[SGX_CLOUD_FLAGS] |= 2;     // SGX_CLOUD_LEAF_TOO_SMALL
        }
        A.g[f] = g;
    }
    SGX_THREADS_END
}

// the cell index of every point of the stage (VoxelGrid::applyFilter's first pass) and the identity as the value to carry
SGX_KERNEL(256) k_cloud_keys(SgxCloudArgs A)
{
    SGX_THREADS_BEGIN(tid)
    const int f = (int)blockIdx.y; const SgxCloudGrid g = A.g[f];
    const int i = (int)blockIdx.x * 256 + tid;
    if (i < g.n) {
        const SgxCloudPoint p = (A.stage ? A.vox : A.pts)[(size_t)f * A.N + i];
        uint32_t key = (uint32_t)g.total;
        if (g.ok && sgx_cloud_finite(p.x) && sgx_cloud_finite(p.y) && sgx_cloud_finite(p.z)) {
            const int ijk0 = (int)(floorf(p.x * g.inv) - (float)g.min_b[0]);
            const int ijk1 = (int)(floorf(p.y * g.inv) - (float)g.min_b[1]);
            const int ijk2 = (int)(floorf(p.z * g.inv) - (float)g.min_b[2]);
            key = (uint32_t)(ijk0 + ijk1 * g.div[0] + ijk2 * g.div[0] * g.div[1]);
        }
        A.k0[(size_t)f * A.N + i] = key; A.v0[(size_t)f * A.N + i] = i;
    }
    SGX_THREADS_END
}

// ---- the sort: least-significant-digit radix sort, 4 bits a pass, every pass stable, so (idx, point) comes out in ascending (idx, point index) -----------------------
// pass, part 1: the digit counts of every tile
SGX_KERNEL(256) k_cloud_hist(SgxCloudArgs A)
{
    SGX_LDS int cnt[16];
    const int f = (int)blockIdx.y, tile = (int)blockIdx.x, n = A.g[f].n;
    const uint32_t *src = (A.cur ? A.k1 : A.k0) + (size_t)f * A.N;
    SGX_THREADS_BEGIN(tid)
    if (tid < 16) cnt[tid] = 0;
    SGX_THREADS_END
    SGX_SYNC();
    SGX_THREADS_BEGIN(tid)
    const int b = tile * SGX_CLOUD_TILE + tid * 8;
    for (int e = 0; e < 8; e++) if (b + e < n) sgx_atomic_add(&cnt[(src[b + e] >> A.shift) & 15u], 1);
    SGX_THREADS_END
    SGX_SYNC();
    SGX_THREADS_BEGIN(tid)
    if (tid < 16) A.tab[((size_t)f * 16 + tid) * A.tiles + tile] = cnt[tid];
    SGX_THREADS_END
}

// exclusive scan of the scan_len counts of every keyframe (one workgroup each: 256 consecutive runs, their sums in order, the runs again); the total goes to
// counter scan_slot when that is >= 0
SGX_KERNEL(256) k_cloud_scan(SgxCloudArgs A)
{
    SGX_LDS int part[256];
    const int f = (int)blockIdx.x, len = A.scan_len, chunk = (len + 255) / 256;
    int *t = A.tab + (size_t)f * len;
    SGX_THREADS_BEGIN(tid)
    int s = 0;
    const int e = (tid + 1) * chunk < len ? (tid + 1) * chunk : len;
    for (int c = tid * chunk; c < e; c++) s += t[c];
    part[tid] = s;
    SGX_THREADS_END
    SGX_SYNC();
    SGX_THREADS_BEGIN(tid)
    if (tid == 0) {
        int run = 0;
        for (int i = 0; i < 256; i++) { const int v = part[i]; part[i] = run; run += v; }
        if (A.scan_slot >= 0) A.ci[SGX_CLOUD_CI * f + A.scan_slot] = run;
    }
    SGX_THREADS_END
    SGX_SYNC();
    SGX_THREADS_BEGIN(tid)
    int run = part[tid];
    const int e = (tid + 1) * chunk < len ? (tid + 1) * chunk : len;
    for (int c = tid * chunk; c < e; c++) { const int v = t[c]; t[c] = run; run += v; }
    SGX_THREADS_END
}

// pass, part 2: every lane counts the digits of its 8 consecutive keys, the (digit, lane) table is scanned digit-major, and a key goes to the start of its
// (digit, tile) run plus the keys of that digit before it in the tile: equal digits keep their order.  A pass above the key's highest bit is a copy.
SGX_KERNEL(256) k_cloud_scatter(SgxCloudArgs A)
{
    SGX_LDS int c[16 * 256];
    SGX_LDS int tot[256];
    SGX_LDS int base[16];
    const int f = (int)blockIdx.y, tile = (int)blockIdx.x; const SgxCloudGrid g = A.g[f];
    const int n = g.n, t0 = tile * SGX_CLOUD_TILE;
    const uint32_t *ks = (A.cur ? A.k1 : A.k0) + (size_t)f * A.N; uint32_t *kd = (A.cur ? A.k0 : A.k1) + (size_t)f * A.N;
    const int *vs = (A.cur ? A.v1 : A.v0) + (size_t)f * A.N; int *vd = (A.cur ? A.v0 : A.v1) + (size_t)f * A.N;
    if (t0 >= n) return;
    if (((uint32_t)g.total >> A.shift) == 0) {
        SGX_THREADS_BEGIN(tid)
        for (int e = 0; e < 8; e++) { const int i = t0 + e * 256 + tid; if (i < n) { kd[i] = ks[i]; vd[i] = vs[i]; } }
        SGX_THREADS_END
        return;
    }
    SGX_THREADS_BEGIN(tid)
    for (int d = 0; d < 16; d++) c[d * 256 + tid] = 0;
    const int b = t0 + tid * 8;
    for (int e = 0; e < 8; e++) if (b + e < n) c[(int)((ks[b + e] >> A.shift) & 15u) * 256 + tid]++;
    SGX_THREADS_END
    SGX_SYNC();
    SGX_THREADS_BEGIN(tid)
    int run = 0;
    for (int q = 0; q < 16; q++) { const int v = c[16 * tid + q]; c[16 * tid + q] = run; run += v; }
    tot[tid] = run;
    SGX_THREADS_END
    SGX_SYNC();
    SGX_THREADS_BEGIN(tid)
    if (tid == 0) { int run = 0; for (int i = 0; i < 256; i++) { const int v = tot[i]; tot[i] = run; run += v; } }
    SGX_THREADS_END
    SGX_SYNC();
    SGX_THREADS_BEGIN(tid)
    if (tid < 16) base[tid] = A.tab[((size_t)f * 16 + tid) * A.tiles + tile] - (c[tid * 256] + tot[tid * 16]);
    SGX_THREADS_END
    SGX_SYNC();
    SGX_THREADS_BEGIN(tid)
    const int b = t0 + tid * 8;
    for (int e = 0; e < 8; e++) if (b + e < n) {
        const uint32_t k = ks[b + e];
        const int fl = (int)((k >> A.shift) & 15u) * 256 + tid;
        const int pos = base[fl >> 8] + c[fl] + tot[fl >> 4];
        c[fl]++;
        if ((unsigned)pos < (unsigned)n) { kd[pos] = k; vd[pos] = vs[b + e]; }
    }
    SGX_THREADS_END
}

// the stage's points in sorted order, so that a run (stage 0) or a row of cells (stage 1) is consecutive memory
SGX_KERNEL(256) k_cloud_gather(SgxCloudArgs A)
{
    SGX_THREADS_BEGIN(tid)
    const int f = (int)blockIdx.y, n = A.g[f].n;
    const int i = (int)blockIdx.x * 256 + tid;
    if (i < n) {
        const int v = A.v0[(size_t)f * A.N + i];
        if ((unsigned)v < (unsigned)A.N) A.spts[(size_t)f * A.N + i] = (A.stage ? A.vox : A.pts)[(size_t)f * A.N + v];
    }
    SGX_THREADS_END
}

// stage 0: sorted position i starts a voxel; stage 1: the outlier filter keeps voxel point i (a point goes when dist > thr; a NaN threshold removes nothing)
SGX_DEV bool sgx_cloud_flag(const SgxCloudArgs &A, int f, int i)
{
    if (!A.stage) {
        const SgxCloudGrid g = A.g[f];
        if (i >= g.n) return false;
        const uint32_t *k = A.k0 + (size_t)f * A.N;
        return k[i] != (uint32_t)g.total && (i == 0 || k[i] != k[i - 1]);
    }
    const int nv = A.ci[SGX_CLOUD_CI * f + SGX_CLOUD_NVOX];
    return i < nv && nv > A.mean_k && !((double)A.dist[(size_t)f * A.N + i] > A.cd[2 * f + 1]);
}

SGX_KERNEL(256) k_cloud_flagcount(SgxCloudArgs A)
{
    SGX_LDS int cnt;
    const int f = (int)blockIdx.y;
    SGX_THREADS_BEGIN(tid)
    if (tid == 0) cnt = 0;
    SGX_THREADS_END
    SGX_SYNC();
    SGX_THREADS_BEGIN(tid)
    const int i = (int)blockIdx.x * 256 + tid;
    if (i < A.N && sgx_cloud_flag(A, f, i)) sgx_atomic_add(&cnt, 1);
    SGX_THREADS_END
    SGX_SYNC();
    SGX_THREADS_BEGIN(tid)
    if (tid == 0) A.tab[(size_t)f * A.nblk + blockIdx.x] = cnt;
    SGX_THREADS_END
}

// the flagged positions numbered in order.  Stage 0: vstart[v] = first sorted position of voxel v, and the end of the last one; stage 1: the kept voxel points
// to the output, in ascending idx, through the axis map in LOCAL mode
SGX_KERNEL(256) k_cloud_flagapply(SgxCloudArgs A)
{
    SGX_LDS int fl[256];
    SGX_LDS int pre[256];
    const int f = (int)blockIdx.y;
    SGX_THREADS_BEGIN(tid)
    const int i = (int)blockIdx.x * 256 + tid;
    fl[tid] = i < A.N && sgx_cloud_flag(A, f, i) ? 1 : 0;
    SGX_THREADS_END
    SGX_SYNC();
    SGX_THREADS_BEGIN(tid)
    if (tid == 0) { int run = 0; for (int t = 0; t < 256; t++) { pre[t] = run; run += fl[t]; } }
    SGX_THREADS_END
    SGX_SYNC();
    SGX_THREADS_BEGIN(tid)
    const int i = (int)blockIdx.x * 256 + tid;
    const int pos = A.tab[(size_t)f * A.nblk + blockIdx.x] + pre[tid];
    if (!A.stage) {
        const SgxCloudGrid g = A.g[f];
        int *vstart = A.vstart + (size_t)f * (A.N + 1);
        if (i < g.n && pos >= 0 && pos < A.N) {
            const uint32_t *k = A.k0 + (size_t)f * A.N;
            if (fl[tid]) vstart[pos] = i;
            if (k[i] != (uint32_t)g.total && (i + 1 == g.n || k[i + 1] == (uint32_t)g.total)) vstart[pos + fl[tid]] = i + 1;      // the last point that is in a cell
        }
    } else if (fl[tid] && pos >= 0 && pos < A.N) {
        const SgxCloudPoint p = A.vox[(size_t)f * A.N + i];
        A.out[(size_t)f * A.N + pos] = A.mode == 0 ? sgx_cloud_ros(p) : p;
    }
    SGX_THREADS_END
}

// CentroidPoint<PointXYZRGB>: the running float sums of a voxel's points in ascending point index, / (float)n.  One lane per voxel: the order is the result.  The
// sorted copy makes a run consecutive memory; the loads of a step do not depend on the sums.  Also the extremes of the centroids, for the search grid.
SGX_KERNEL(64) k_cloud_centroid(SgxCloudArgs A)
{
    SGX_LDS int red[6];
    const int f = (int)blockIdx.y; const int nv = A.ci[SGX_CLOUD_CI * f + SGX_CLOUD_NVOX];
    if ((int)blockIdx.x * 64 >= nv) return;
    SGX_THREADS_BEGIN(tid)
    if (tid < 3) red[tid] = 0x7fffffff; else if (tid < 6) red[tid] = (int)0x80000000;
    SGX_THREADS_END
    SGX_SYNC();
    SGX_THREADS_BEGIN(tid)
    const int v = (int)blockIdx.x * 64 + tid;
    if (v < nv) {
        const int *vstart = A.vstart + (size_t)f * (A.N + 1);
        int b = vstart[v], e = vstart[v + 1];
        if (b < 0) b = 0;
        if (e > A.N) e = A.N;
        const SgxCloudPoint *P = A.spts + (size_t)f * A.N;
        float x = 0, y = 0, z = 0, r = 0, g = 0, bl = 0, a = 0;
        int i = b;
        for (; i + 8 <= e; i += 8) {
            SgxCloudPoint q[8];
            for (int u = 0; u < 8; u++) q[u] = P[i + u];
            for (int u = 0; u < 8; u++) {
                x += q[u].x; y += q[u].y; z += q[u].z;
                r += (float)((q[u].rgba >> 16) & 255u); g += (float)((q[u].rgba >> 8) & 255u); bl += (float)(q[u].rgba & 255u); a += (float)(q[u].rgba >> 24);
            }
        }
        for (; i < e; i++) {
            const SgxCloudPoint q = P[i];
            x += q.x; y += q.y; z += q.z;
            r += (float)((q.rgba >> 16) & 255u); g += (float)((q.rgba >> 8) & 255u); bl += (float)(q.rgba & 255u); a += (float)(q.rgba >> 24);
        }
        const float n = (float)(e - b);
        SgxCloudPoint o;
        o.x = x / n; o.y = y / n; o.z = z / n;
        o.rgba = (uint32_t)(a / n) << 24 | (uint32_t)(r / n) << 16 | (uint32_t)(g / n) << 8 | (uint32_t)(bl / n);
        A.vox[(size_t)f * A.N + v] = o;
        if (sgx_cloud_finite(o.x) && sgx_cloud_finite(o.y) && sgx_cloud_finite(o.z)) {
            const int ox = sgx_cloud_ordered(o.x), oy = sgx_cloud_ordered(o.y), oz = sgx_cloud_ordered(o.z);
            sgx_atomic_min_i32(&red[0], ox); sgx_atomic_min_i32(&red[1], oy); sgx_atomic_min_i32(&red[2], oz);
            sgx_atomic_max(&red[3], ox); sgx_atomic_max(&red[4], oy); sgx_atomic_max(&red[5], oz);
        }
    }
    SGX_THREADS_END
    SGX_SYNC();
    SGX_THREADS_BEGIN(tid)
    int *ci = A.ci + SGX_CLOUD_CI * f;
    if (tid < 3) sgx_atomic_min_i32(&ci[SGX_CLOUD_MM1 + tid], red[tid]);
    else if (tid < 6) sgx_atomic_max(&ci[SGX_CLOUD_MM1 + tid], red[tid]);
    SGX_THREADS_END
}

// first sorted position whose key is >= t
SGX_DEV int sgx_cloud_lower_bound(const uint32_t *key, int n, uint32_t t)
{
    int lo = 0, hi = n;
    while (lo < hi) { const int mid = (lo + hi) >> 1; if (key[mid] < t) lo = mid + 1; else hi = mid; }
    return lo;
}

// StatisticalOutlierRemoval, the mean distance to the mean_k nearest neighbours: one lane per voxel centroid, in the order of the SEARCH grid (the centroids binned
// by their own coordinates: a running float sum can leave its voxel).  The keys ascend with x fastest, so every (j, k) row of the (2r + 1)^3 cell window is one
// consecutive range, found by one binary search; the lane keeps its non-empty rows in LDS.  The K = mean_k + 1 smallest d2 by bisection on the bit pattern as in
// k_obj3d_sor.  The window is accepted when every centroid outside it is proven farther than the K-th found; otherwise the point goes on the list of
// k_cloud_sor_whole (v1, free after the sort).
SGX_KERNEL(64) k_cloud_sor(SgxCloudArgs A)
{
    SGX_LDS uint32_t rows[SGX_CLOUD_ROWS * 64];
    const int f = (int)blockIdx.y; const int nv = A.ci[SGX_CLOUD_CI * f + SGX_CLOUD_NVOX]; const int K = A.mean_k + 1;
    if (nv < K || (int)blockIdx.x * 64 >= nv) return;
    const SgxCloudGrid g = A.g[f];
    const uint32_t *key = A.k0 + (size_t)f * A.N; const int *val = A.v0 + (size_t)f * A.N;
    const SgxCloudPoint *P = A.spts + (size_t)f * A.N;
    const int *mm = A.ci + SGX_CLOUD_CI * f + SGX_CLOUD_MM1;
    float M = 0;
    for (int a = 0; a < 6; a++) { const float v = fabsf(sgx_cloud_unordered(mm[a])); if (v > M) M = v; }
    // E: how far a centroid can lie outside the box of its search cell (the rounding of p * inv and of inv itself), with room to spare
    const double E = (1.0 / 4194304.0) * ((double)M + 16.0 * (double)A.leaf);
    const double bound = (double)A.r0 * (double)A.leaf - 2.0 * E;
    SGX_THREADS_BEGIN(tid)
    const int s = (int)blockIdx.x * 64 + tid;
    if (s < nv) {
        const SgxCloudPoint q = P[s];
        const uint32_t ks = key[s];
        bool whole = !g.ok || ks >= (uint32_t)g.total || !(M * g.inv < 8388608.0f);
        uint32_t kth = 0; int nrows = 0;
        if (!whole) {
            const int r = A.r0;
            const int ci = (int)(ks % (uint32_t)g.div[0]), rest = (int)(ks / (uint32_t)g.div[0]), cj = rest % g.div[1], ck = rest / g.div[1];
            const int i0 = ci - r < 0 ? 0 : ci - r, i1 = ci + r > g.div[0] - 1 ? g.div[0] - 1 : ci + r;
            const int j0 = cj - r < 0 ? 0 : cj - r, j1 = cj + r > g.div[1] - 1 ? g.div[1] - 1 : cj + r;
            const int k0 = ck - r < 0 ? 0 : ck - r, k1 = ck + r > g.div[2] - 1 ? g.div[2] - 1 : ck + r;
            for (int kk = k0; kk <= k1 && !whole; kk++) for (int jj = j0; jj <= j1; jj++) {
                const uint32_t rb = (uint32_t)(kk * g.div[1] + jj) * (uint32_t)g.div[0];
                const int lo = sgx_cloud_lower_bound(key, nv, rb + (uint32_t)i0);
                int c = 0;
                while (lo + c < nv && key[lo + c] <= rb + (uint32_t)i1) c++;
                if (c > 4095 || nrows >= SGX_CLOUD_ROWS) { whole = true; break; }
                if (c) { rows[nrows * 64 + tid] = (uint32_t)lo | (uint32_t)c << 20; nrows++; }
            }
        }
        if (!whole) {
            for (int bit = 30; bit >= 0; bit--) {
                const uint32_t t = kth | (1u << bit);
                int cnt = 0;
                for (int rw = 0; rw < nrows; rw++) {
                    const uint32_t e = rows[rw * 64 + tid]; const int lo = (int)(e & 0xfffffu), c = (int)(e >> 20);
                    for (int u = 0; u < c; u++) if (sgx_cloud_f32_bits(sgx_cloud_d2(q.x, q.y, q.z, P[lo + u].x, P[lo + u].y, P[lo + u].z)) < t) cnt++;
                }
                if (cnt < K) kth = t;
            }
            whole = !(kth < 0x7f800000u && bound > 0 && (double)sgx_cloud_bits_f32(kth) < bound * bound * (1.0 - 1.0 / 1048576.0));
        }
        if (whole) {                                          // to k_cloud_sor_whole, a workgroup a point; the list's order is free, every entry writes its own dist
            const int e = sgx_atomic_add(&A.ci[SGX_CLOUD_CI * f + SGX_CLOUD_LARGER], 1);
            if ((unsigned)e < (unsigned)A.N) A.v1[(size_t)f * A.N + e] = s;
        } else {
            double sum = 0; int cnt = 0;
            for (int rw = 0; rw < nrows; rw++) {
                const uint32_t e = rows[rw * 64 + tid]; const int lo = (int)(e & 0xfffffu), c = (int)(e >> 20);
                for (int u = 0; u < c; u++) {
                    const float d2 = sgx_cloud_d2(q.x, q.y, q.z, P[lo + u].x, P[lo + u].y, P[lo + u].z);
                    if (sgx_cloud_f32_bits(d2) < kth) { sum += (double)sqrtf(d2); cnt++; }
                }
            }
            // the K smallest: everything below the K-th value and the K-th value as often as is left; the smallest is the point's own 0.  The sum is exact in
            // double on every input whose reference sum is (tests/cloud_cases.py asserts it), so its order is free
            sum += (double)(K - cnt) * (double)sqrtf(sgx_cloud_bits_f32(kth));
            const int v = val[s];
            if ((unsigned)v < (unsigned)A.N) A.dist[(size_t)f * A.N + v] = (float)(sum / (double)A.mean_k);
        }
    }
    SGX_THREADS_END
}

// the points whose first window was not proven: the same K-th smallest and sum over the whole voxel cloud, one workgroup per point (its lanes share the scan;
// 256 strided partial counts / sums, combined in lane order)
SGX_KERNEL(256) k_cloud_sor_whole(SgxCloudArgs A)
{
    SGX_LDS int pc[256];
    SGX_LDS double ps[256];
    SGX_LDS uint32_t kth_s;
    const int f = (int)blockIdx.y; const int nv = A.ci[SGX_CLOUD_CI * f + SGX_CLOUD_NVOX]; const int K = A.mean_k + 1;
    if (nv < K) return;
    int nfail = A.ci[SGX_CLOUD_CI * f + SGX_CLOUD_LARGER]; if (nfail > nv) nfail = nv;
    const int *val = A.v0 + (size_t)f * A.N; const int *list = A.v1 + (size_t)f * A.N;
    const SgxCloudPoint *P = A.spts + (size_t)f * A.N;
    for (int e = (int)blockIdx.x; e < nfail; e += (int)gridDim.x) {
        const int s = list[e];
        if (s < 0 || s >= nv) continue;
        const SgxCloudPoint q = P[s];
        SGX_THREADS_BEGIN(tid)
        if (tid == 0) kth_s = 0;
        SGX_THREADS_END
        SGX_SYNC();
        for (int bit = 30; bit >= 0; bit--) {
            const uint32_t t = kth_s | (1u << bit);
            SGX_THREADS_BEGIN(tid)
            int c = 0;
            for (int u = tid; u < nv; u += 256) if (sgx_cloud_f32_bits(sgx_cloud_d2(q.x, q.y, q.z, P[u].x, P[u].y, P[u].z)) < t) c++;
            pc[tid] = c;
            SGX_THREADS_END
            SGX_SYNC();
            SGX_THREADS_BEGIN(tid)
            if (tid == 0) { int c = 0; for (int i = 0; i < 256; i++) c += pc[i]; if (c < K) kth_s = t; }
            SGX_THREADS_END
            SGX_SYNC();
        }
        const uint32_t kth = kth_s;
        SGX_THREADS_BEGIN(tid)
        double sum = 0; int c = 0;
        for (int u = tid; u < nv; u += 256) {
            const float d2 = sgx_cloud_d2(q.x, q.y, q.z, P[u].x, P[u].y, P[u].z);
            if (sgx_cloud_f32_bits(d2) < kth) { sum += (double)sqrtf(d2); c++; }
        }
        ps[tid] = sum; pc[tid] = c;
        SGX_THREADS_END
        SGX_SYNC();
        SGX_THREADS_BEGIN(tid)
        if (tid == 0) {
            double sum = 0; int c = 0;
            for (int i = 0; i < 256; i++) { sum += ps[i]; c += pc[i]; }
            sum += (double)(K - c) * (double)sqrtf(sgx_cloud_bits_f32(kth));
            const int v = val[s];
            if ((unsigned)v < (unsigned)A.N) A.dist[(size_t)f * A.N + v] = (float)(sum / (double)A.mean_k);
        }
        SGX_THREADS_END
        SGX_SYNC();
    }
}

// mean, variance and threshold of the distances (one workgroup per keyframe; a fixed order: 256 consecutive runs in voxel order, then their sums in order)
SGX_KERNEL(256) k_cloud_stats(SgxCloudArgs A)
{
    SGX_LDS double s1[256];
    SGX_LDS double s2[256];
    const int f = (int)blockIdx.x; const int nv = A.ci[SGX_CLOUD_CI * f + SGX_CLOUD_NVOX];
    if (nv <= A.mean_k) return;
    const int run = (nv + 255) / 256;
    SGX_THREADS_BEGIN(tid)
    double a = 0, b = 0;
    const int e = (tid + 1) * run < nv ? (tid + 1) * run : nv;
    for (int c = tid * run; c < e; c++) { const float d = A.dist[(size_t)f * A.N + c]; a += (double)d; b += (double)(d * d); }
    s1[tid] = a; s2[tid] = b;
    SGX_THREADS_END
    SGX_SYNC();
    SGX_THREADS_BEGIN(tid)
    if (tid == 0) {
        double sum = 0, sq = 0;
        for (int i = 0; i < 256; i++) { sum += s1[i]; sq += s2[i]; }
        const double n = (double)nv;
        const double mean = sum / n, var = (sq - sum * sum / n) / (n - 1.0);
        A.cd[2 * f] = mean; A.cd[2 * f + 1] = mean + A.mul * sqrt(var);
    }
    SGX_THREADS_END
}

SGX_KERNEL(64) k_cloud_result(SgxCloudArgs A)
{
    SGX_THREADS_BEGIN(tid)
    const int f = (int)blockIdx.x * 64 + tid;
    if (f < A.B) {
        const int *ci = A.ci + SGX_CLOUD_CI * f;
        SgxCloudResult R;
        R.n_points = ci[SGX_CLOUD_KEPT]; R.n_pixels_used = ci[SGX_CLOUD_USED]; R.n_voxels = ci[SGX_CLOUD_NVOX]; R.flags = ci[SGX_CLOUD_FLAGS];
        if (!(R.flags & 2) && R.n_voxels <= A.mean_k) R.flags |= 1;                         // SGX_CLOUD_FEW_POINTS
        R.larger_window_points = ci[SGX_CLOUD_LARGER]; R.reserved = 0;
        R.mean = A.cd[2 * f]; R.thr = A.cd[2 * f + 1];
        A.results[f] = R;
    }
    SGX_THREADS_END
}
