// sgx_globalmap_kernels.h — MapViewer's accumulating global cloud (src/sg-slam/src/PointcloudMapping.cc:332-360) on the device: `*globalMap += *temp_globalMap` as an
// ordered append, and voxel_global + sor_global over the WHOLE map.  The voxel grid, the sort, the centroids, the statistics and the whole-cloud scan are the kernels of
// sgx_cloud_kernels.h launched with B = 1 and N = the map's capacity (they take their counts from SgxCloudGrid.n and the device counters); what a map needs differently
// is here: the append, the extremes of stored points, a grid header whose point count lives on the device, and the neighbour search at map scale in two kernels
// (k_gmap_sor, k_gmap_sor_wide).  DESIGN.md §9j has the semantics, the defined cases and the tier proof.
#pragma once
#include "sgx_rt.h"
#include <math.h>
namespace {                                 // this unit's own copy of the keyframe kernels (a kernel defined in two units would be two symbols of one name)
#include "sgx_cloud_kernels.h"
}

#define SGX_GMAP_WIDER 5                    /* slot of SgxCloudArgs.ci: voxel points whose first window was not proven (the list of k_gmap_sor_wide) */
#define SGX_GMAP_NIN 6                      /* slot: the map's size when the consolidation began */
#define SGX_GMAP_RCAP 16                    /* the widest window of k_gmap_sor_wide: E of the proof is stated for r <= 16 */
#define SGX_GMAP_WROWS 1089                 /* (2 * RCAP + 1)^2 */
#define SGX_GMAP_TIER_WHOLE 0               /* tier of a voxel point that searched the whole cloud; otherwise the radius that was proven */

struct SgxGmapAppendRecord { int n_in, offset, map_size, flags; };                                                                 // = sgx_globalmap_append_record
struct SgxGmapResult { int n_points_in, n_voxels, n_points, flags, wider_window_points, whole_cloud_points; double mean, thr; };   // = sgx_globalmap_result

#if defined(__GNUC__) && !defined(__clang__)
#pragma GCC diagnostic ignored "-Wsubobject-linkage"      /* the emulator build: SgxGmapArgs is as private to the unit as the types it holds */
#endif
struct SgxGmapArgs {
    SgxCloudArgs C;                         // B = 1, N = capacity, pts = out = the map, mode = WORLD (no axis map)
    int cap, max_radius, n_clouds;
    int *count;                             // the map's size, on the device
    int *wlist;                             // the not-proven list of k_gmap_sor
    uint8_t *tier;                          // per voxel point: the proven radius, or SGX_GMAP_TIER_WHOLE
    const SgxCloudPoint *src; long long src_stride; const int32_t *n_src; long long n_stride;      // the clouds of an append
    SgxGmapAppendRecord *arec;
    SgxGmapResult *result;
};

SGX_DEV int sgx_gmap_count(const SgxGmapArgs &G) { const int n = *G.count; return n < 0 ? 0 : n > G.cap ? G.cap : n; }

// ---- append ---------------------------------------------------------------------------------------------------------------------------------------------------------
// the ordered prefix over the batch's counts, one lane: cloud i goes behind what is there when it fits, else SGX_GMAP_FULL and the later clouds are still tried against
// the running size; the outcome is a function of the sizes alone.  A negative count is an empty cloud.
SGX_KERNEL(64) k_gmap_append_plan(SgxGmapArgs G)
{
    SGX_THREADS_BEGIN(tid)
    if (tid == 0) {
        int run = sgx_gmap_count(G);
        for (int i = 0; i < G.n_clouds; i++) {
            int n = *(const int32_t *)((const char *)G.n_src + (size_t)i * (size_t)G.n_stride);
            if (n < 0) n = 0;
            SgxGmapAppendRecord R; R.n_in = n; R.flags = 0; R.offset = run;
            if (n > G.cap - run) { R.flags = 4; R.offset = -1; } else run += n;                     // SGX_GMAP_FULL
            R.map_size = run;
            G.arec[i] = R;
        }
        *G.count = run;
    }
    SGX_THREADS_END
}

// the copy (grid.y = cloud, grid-stride over its points): points that are not finite are stored as they are, as PCL's operator+= does
SGX_KERNEL(256) k_gmap_append_copy(SgxGmapArgs G)
{
    const int c = (int)blockIdx.y;
    const SgxGmapAppendRecord R = G.arec[c];
    if (R.flags || R.offset < 0 || R.n_in > G.cap - R.offset) return;
    const SgxCloudPoint *src = G.src + (size_t)c * (size_t)G.src_stride;
    SGX_THREADS_BEGIN(tid)
    for (int i = (int)blockIdx.x * 256 + tid; i < R.n_in; i += (int)gridDim.x * 256) G.C.pts[R.offset + i] = src[i];
    SGX_THREADS_END
}

SGX_KERNEL(64) k_gmap_reset(SgxGmapArgs G)
{
    SGX_THREADS_BEGIN(tid)
    if (tid == 0) *G.count = 0;
    SGX_THREADS_END
}

// ---- consolidation --------------------------------------------------------------------------------------------------------------------------------------------------
SGX_KERNEL(64) k_gmap_prep(SgxGmapArgs G)
{
    SGX_THREADS_BEGIN(tid)
    int *ci = G.C.ci;
    if (tid < SGX_CLOUD_CI) ci[tid] = 0;
    SGX_THREADS_END
    SGX_SYNC();
    SGX_THREADS_BEGIN(tid)
    int *ci = G.C.ci;
    if (tid < 3) { ci[SGX_CLOUD_MM0 + tid] = 0x7fffffff; ci[SGX_CLOUD_MM1 + tid] = 0x7fffffff; }
    else if (tid < 6) { ci[SGX_CLOUD_MM0 + tid] = (int)0x80000000; ci[SGX_CLOUD_MM1 + tid] = (int)0x80000000; }
    else if (tid == 6) { ci[SGX_GMAP_NIN] = sgx_gmap_count(G); G.C.cd[0] = 0; G.C.cd[1] = 0; }
    SGX_THREADS_END
}

// getMinMax3D over the map's finite points: ordered-int min / max, reduced in LDS first
SGX_KERNEL(256) k_gmap_extremes(SgxGmapArgs G)
{
    SGX_LDS int red[6];
    const int n = G.C.ci[SGX_GMAP_NIN];
    if ((int)blockIdx.x * 256 >= n) return;
    SGX_THREADS_BEGIN(tid)
    if (tid < 3) red[tid] = 0x7fffffff; else if (tid < 6) red[tid] = (int)0x80000000;
    SGX_THREADS_END
    SGX_SYNC();
    SGX_THREADS_BEGIN(tid)
    const int i = (int)blockIdx.x * 256 + tid;
    if (i < n) {
        const SgxCloudPoint p = G.C.pts[i];
        if (sgx_cloud_finite(p.x) && sgx_cloud_finite(p.y) && sgx_cloud_finite(p.z)) {
            const int ox = sgx_cloud_ordered(p.x), oy = sgx_cloud_ordered(p.y), oz = sgx_cloud_ordered(p.z);
            sgx_atomic_min_i32(&red[0], ox); sgx_atomic_min_i32(&red[1], oy); sgx_atomic_min_i32(&red[2], oz);
            sgx_atomic_max(&red[3], ox); sgx_atomic_max(&red[4], oy); sgx_atomic_max(&red[5], oz);
        }
    }
    SGX_THREADS_END
    SGX_SYNC();
    SGX_THREADS_BEGIN(tid)
    int *ci = G.C.ci;
    if (tid < 3) sgx_atomic_min_i32(&ci[SGX_CLOUD_MM0 + tid], red[tid]);
    else if (tid < 6) sgx_atomic_max(&ci[SGX_CLOUD_MM0 + tid], red[tid]);
    SGX_THREADS_END
}

// k_cloud_grid's header and refusal test for one cloud whose stage-0 point count is the map's device count (k_cloud_grid hard-wires A.N)
SGX_KERNEL(64) k_gmap_grid(SgxGmapArgs G)
{
    SGX_THREADS_BEGIN(tid)
    if (tid == 0 && blockIdx.x == 0) {
        const SgxCloudArgs &A = G.C;
        int *ci = A.ci;
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
                if (!A.stage) g.n = ci[SGX_GMAP_NIN];
            } else if (!A.stage) ci[SGX_CLOUD_FLAGS] |= 2;     // SGX_GMAP_LEAF_TOO_SMALL
        }
        A.g[0] = g;
    }
    SGX_THREADS_END
}

// E and the proof bound of a window of radius r: two centroids whose search cells differ by more than r in an axis are more than r * L - 2E apart
SGX_DEV double sgx_gmap_bound(double M, double leaf, int r) { return (double)r * leaf - 2.0 * ((1.0 / 4194304.0) * (M + 16.0 * leaf)); }
SGX_DEV bool sgx_gmap_proven(uint32_t kth, double bound)
{
    return kth < 0x7f800000u && bound > 0 && (double)sgx_cloud_bits_f32(kth) < bound * bound * (1.0 - 1.0 / 1048576.0);
}
SGX_DEV float sgx_gmap_absmax(const int *mm)
{
    float M = 0;
    for (int a = 0; a < 6; a++) { const float v = fabsf(sgx_cloud_unordered(mm[a])); if (v > M) M = v; }
    return M;
}

// StatisticalOutlierRemoval's neighbour search, first tier: one lane per centroid in search-grid order, window r0 by §9f's rule, the lane's non-empty rows in LDS as a
// 32-bit start and a 16-bit count (121 rows x 64 lanes x 6 B = 45.4 KiB; no 20-bit position, no 4095-a-row cap: a row of more than 65535 centroids sends the point to
// the wide kernel, which counts in 32 bits).  Proven: dist and the tier are written.  Not proven: the point goes on the list of k_gmap_sor_wide.  No search grid (refused,
// M * inv >= 2^23, a centroid in no cell): straight to the whole-cloud list of k_cloud_sor_whole.
SGX_KERNEL(64) k_gmap_sor(SgxGmapArgs G)
{
    SGX_LDS uint32_t row_lo[SGX_CLOUD_ROWS * 64];
    SGX_LDS uint16_t row_n[SGX_CLOUD_ROWS * 64];
    const SgxCloudArgs &A = G.C;
    const int nv = A.ci[SGX_CLOUD_NVOX]; const int K = A.mean_k + 1;
    if (nv < K || (int)blockIdx.x * 64 >= nv) return;
    const SgxCloudGrid g = A.g[0];
    const uint32_t *key = A.k0; const int *val = A.v0;
    const SgxCloudPoint *P = A.spts;
    const float M = sgx_gmap_absmax(A.ci + SGX_CLOUD_MM1);
    const double bound = sgx_gmap_bound((double)M, (double)A.leaf, A.r0);
    SGX_THREADS_BEGIN(tid)
    const int s = (int)blockIdx.x * 64 + tid;
    if (s < nv) {
        const SgxCloudPoint q = P[s];
        const uint32_t ks = key[s];
        const bool whole = !g.ok || ks >= (uint32_t)g.total || !(M * g.inv < 8388608.0f);
        bool wide = false;
        uint32_t kth = 0; int nrows = 0;
        if (!whole) {
            const int r = A.r0;
            const int ci = (int)(ks % (uint32_t)g.div[0]), rest = (int)(ks / (uint32_t)g.div[0]), cj = rest % g.div[1], ck = rest / g.div[1];
            const int i0 = ci - r < 0 ? 0 : ci - r, i1 = ci + r > g.div[0] - 1 ? g.div[0] - 1 : ci + r;
            const int j0 = cj - r < 0 ? 0 : cj - r, j1 = cj + r > g.div[1] - 1 ? g.div[1] - 1 : cj + r;
            const int k0 = ck - r < 0 ? 0 : ck - r, k1 = ck + r > g.div[2] - 1 ? g.div[2] - 1 : ck + r;
            for (int kk = k0; kk <= k1 && !wide; kk++) for (int jj = j0; jj <= j1; jj++) {
                const uint32_t rb = (uint32_t)(kk * g.div[1] + jj) * (uint32_t)g.div[0];
                const int lo = sgx_cloud_lower_bound(key, nv, rb + (uint32_t)i0);
                int c = 0;
                while (lo + c < nv && c <= 65535 && key[lo + c] <= rb + (uint32_t)i1) c++;
                if (c > 65535 || nrows >= SGX_CLOUD_ROWS) { wide = true; break; }
                if (c) { row_lo[nrows * 64 + tid] = (uint32_t)lo; row_n[nrows * 64 + tid] = (uint16_t)c; nrows++; }
            }
        }
        if (!whole && !wide) {
            for (int bit = 30; bit >= 0; bit--) {
                const uint32_t t = kth | (1u << bit);
                int cnt = 0;
                for (int rw = 0; rw < nrows; rw++) {
                    const int lo = (int)row_lo[rw * 64 + tid], c = (int)row_n[rw * 64 + tid];
                    for (int u = 0; u < c; u++) if (sgx_cloud_f32_bits(sgx_cloud_d2(q.x, q.y, q.z, P[lo + u].x, P[lo + u].y, P[lo + u].z)) < t) cnt++;
                }
                if (cnt < K) kth = t;
            }
            wide = !sgx_gmap_proven(kth, bound);
        }
        const int v = val[s];
        if (whole) {                                           // the list's order is free: every entry writes its own dist
            const int e = sgx_atomic_add(&A.ci[SGX_CLOUD_LARGER], 1);
            if ((unsigned)e < (unsigned)A.N) A.v1[e] = s;
            if ((unsigned)v < (unsigned)A.N) G.tier[v] = SGX_GMAP_TIER_WHOLE;
        } else if (wide) {
            const int e = sgx_atomic_add(&A.ci[SGX_GMAP_WIDER], 1);
            if ((unsigned)e < (unsigned)A.N) G.wlist[e] = s;
        } else {
            double sum = 0; int cnt = 0;
            for (int rw = 0; rw < nrows; rw++) {
                const int lo = (int)row_lo[rw * 64 + tid], c = (int)row_n[rw * 64 + tid];
                for (int u = 0; u < c; u++) {
                    const float d2 = sgx_cloud_d2(q.x, q.y, q.z, P[lo + u].x, P[lo + u].y, P[lo + u].z);
                    if (sgx_cloud_f32_bits(d2) < kth) { sum += (double)sqrtf(d2); cnt++; }
                }
            }
            sum += (double)(K - cnt) * (double)sqrtf(sgx_cloud_bits_f32(kth));                      // the tie rule of k_cloud_sor
            if ((unsigned)v < (unsigned)A.N) { A.dist[v] = (float)(sum / (double)A.mean_k); G.tier[v] = (uint8_t)A.r0; }
        }
    }
    SGX_THREADS_END
}

// second tier: one workgroup per point of the not-proven list.  Radii double from 2 * r0 and are capped at 16 (and at max_radius, a test tap); the lanes share the rows
// of the (2r + 1)^2 window, a row's start and end by binary search; K-th smallest by bisection on the bit pattern, tie rule and sum as in k_cloud_sor_whole (256 partial
// counts / sums, combined in lane order).  A radius is accepted under §9f's proof with that r; what r = 16 does not prove goes to the whole-cloud list.
SGX_KERNEL(256) k_gmap_sor_wide(SgxGmapArgs G)
{
    SGX_LDS uint32_t rlo[SGX_GMAP_WROWS];
    SGX_LDS uint32_t rcn[SGX_GMAP_WROWS];
    SGX_LDS int pc[256];
    SGX_LDS double ps[256];
    SGX_LDS uint32_t kth_s;
    const SgxCloudArgs &A = G.C;
    const int nv = A.ci[SGX_CLOUD_NVOX]; const int K = A.mean_k + 1;
    if (nv < K) return;
    int nl = A.ci[SGX_GMAP_WIDER]; if (nl > nv) nl = nv;
    const SgxCloudGrid g = A.g[0];
    if (!g.ok) return;                                         // no point is on the list without a search grid
    const uint32_t *key = A.k0; const int *val = A.v0;
    const SgxCloudPoint *P = A.spts;
    const float M = sgx_gmap_absmax(A.ci + SGX_CLOUD_MM1);
    for (int e = (int)blockIdx.x; e < nl; e += (int)gridDim.x) {
        const int s = G.wlist[e];
        if (s < 0 || s >= nv) continue;
        const SgxCloudPoint q = P[s];
        const uint32_t ks = key[s];
        if (ks >= (uint32_t)g.total) continue;
        const int ci = (int)(ks % (uint32_t)g.div[0]), rest = (int)(ks / (uint32_t)g.div[0]), cj = rest % g.div[1], ck = rest / g.div[1];
        bool done = false;
        int r = 2 * A.r0;
        while (!done) {
            if (r > SGX_GMAP_RCAP) r = SGX_GMAP_RCAP;
            if (r > G.max_radius) break;
            const int i0 = ci - r < 0 ? 0 : ci - r, i1 = ci + r > g.div[0] - 1 ? g.div[0] - 1 : ci + r;
            const int j0 = cj - r < 0 ? 0 : cj - r, j1 = cj + r > g.div[1] - 1 ? g.div[1] - 1 : cj + r;
            const int k0 = ck - r < 0 ? 0 : ck - r, k1 = ck + r > g.div[2] - 1 ? g.div[2] - 1 : ck + r;
            const int nj = j1 - j0 + 1, nrows = nj * (k1 - k0 + 1);                               // <= 33 * 33
            SGX_THREADS_BEGIN(tid)
            for (int rw = tid; rw < nrows; rw += 256) {
                const int jj = j0 + rw % nj, kk = k0 + rw / nj;
                const uint32_t rb = (uint32_t)(kk * g.div[1] + jj) * (uint32_t)g.div[0];
                const int lo = sgx_cloud_lower_bound(key, nv, rb + (uint32_t)i0), hi = sgx_cloud_lower_bound(key, nv, rb + (uint32_t)i1 + 1u);
                rlo[rw] = (uint32_t)lo; rcn[rw] = (uint32_t)(hi - lo);
            }
            if (tid == 0) kth_s = 0;
            SGX_THREADS_END
            SGX_SYNC();
            for (int bit = 30; bit >= 0; bit--) {
                const uint32_t t = kth_s | (1u << bit);
                SGX_THREADS_BEGIN(tid)
                int c = 0;
                for (int rw = tid; rw < nrows; rw += 256) {
                    const int lo = (int)rlo[rw], n = (int)rcn[rw];
                    for (int u = 0; u < n; u++) if (sgx_cloud_f32_bits(sgx_cloud_d2(q.x, q.y, q.z, P[lo + u].x, P[lo + u].y, P[lo + u].z)) < t) c++;
                }
                pc[tid] = c;
                SGX_THREADS_END
                SGX_SYNC();
                SGX_THREADS_BEGIN(tid)
                if (tid == 0) { int c = 0; for (int i = 0; i < 256; i++) c += pc[i]; if (c < K) kth_s = t; }
                SGX_THREADS_END
                SGX_SYNC();
            }
            const uint32_t kth = kth_s;
            SGX_SYNC();                                        // every lane has read kth before lane 0 clears it for the next radius
            if (sgx_gmap_proven(kth, sgx_gmap_bound((double)M, (double)A.leaf, r))) {
                SGX_THREADS_BEGIN(tid)
                double sum = 0; int c = 0;
                for (int rw = tid; rw < nrows; rw += 256) {
                    const int lo = (int)rlo[rw], n = (int)rcn[rw];
                    for (int u = 0; u < n; u++) {
                        const float d2 = sgx_cloud_d2(q.x, q.y, q.z, P[lo + u].x, P[lo + u].y, P[lo + u].z);
                        if (sgx_cloud_f32_bits(d2) < kth) { sum += (double)sqrtf(d2); c++; }
                    }
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
                    if ((unsigned)v < (unsigned)A.N) { A.dist[v] = (float)(sum / (double)A.mean_k); G.tier[v] = (uint8_t)r; }
                }
                SGX_THREADS_END
                SGX_SYNC();
                done = true;
            } else if (r >= SGX_GMAP_RCAP) break;
            else r *= 2;
        }
        if (!done) {
            SGX_THREADS_BEGIN(tid)
            if (tid == 0) {
                const int w = sgx_atomic_add(&A.ci[SGX_CLOUD_LARGER], 1);
                if ((unsigned)w < (unsigned)A.N) A.v1[w] = s;
                const int v = val[s];
                if ((unsigned)v < (unsigned)A.N) G.tier[v] = SGX_GMAP_TIER_WHOLE;
            }
            SGX_THREADS_END
        }
    }
}

// the record, and the map's new size: the compaction (k_cloud_flagapply, WORLD mode: no axis map) has written the survivors into the map from 0 on; a refused
// consolidation wrote nothing and leaves the size as it was
SGX_KERNEL(64) k_gmap_commit(SgxGmapArgs G)
{
    SGX_THREADS_BEGIN(tid)
    if (tid == 0 && blockIdx.x == 0) {
        const int *ci = G.C.ci;
        SgxGmapResult R;
        R.n_points_in = ci[SGX_GMAP_NIN]; R.n_voxels = ci[SGX_CLOUD_NVOX]; R.flags = ci[SGX_CLOUD_FLAGS];
        if (!(R.flags & 2) && R.n_voxels <= G.C.mean_k) R.flags |= 1;                               // SGX_GMAP_FEW_POINTS
        R.wider_window_points = ci[SGX_GMAP_WIDER]; R.whole_cloud_points = ci[SGX_CLOUD_LARGER];
        R.mean = G.C.cd[0]; R.thr = G.C.cd[1];
        if (R.flags) R.n_points = R.n_points_in;
        else { R.n_points = ci[SGX_CLOUD_KEPT]; *G.count = R.n_points; }
        *G.result = R;
    }
    SGX_THREADS_END
}
