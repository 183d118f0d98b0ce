// sgx_obj3d_kernels.h — Detector3D::DetectOne (src/sg-slam/src/Detector3D.cc:41-168) on the device: the box crop of the organised world cloud, PCL's
// StatisticalOutlierRemoval and EuclideanClusterExtraction restated on the pixel grid (no kd-tree, no sort, no neighbour lists), the per-cluster reductions and the
// reference's selection loop.  One launch sequence for J jobs (grid.y = job); every per-point array is in GRID layout: cell c = row-in-crop * cw + column-in-crop, which is
// ascending in the reference's flat index j, so "ascending point order" is ascending cell order.  DESIGN.md §9c has the semantics and the window proof.
#pragma once
#include "sgx_rt.h"
#include <math.h>

#define SGX_OBJ_JI 8            /* ints per job: crop points, kept points, components, surviving clusters, points that needed a larger window */
#define SGX_OBJ_N 0
#define SGX_OBJ_KEPT 1
#define SGX_OBJ_COMP 2
#define SGX_OBJ_SLOTS 3
#define SGX_OBJ_LARGER 4
#define SGX_OBJ_JD 4            /* doubles per job: c1 (metres per pixel step and metre of depth, lower bound), E2 (twice the rounding radius of a world point), thr */
#define SGX_OBJ_MM 10           /* per surviving cluster: pixel min x, max x, min y, max y; ordered-int world min x, y, z, max x, y, z */
#define SGX_OBJ_VALID 1
#define SGX_OBJ_KEEP 2

struct SgxObjJob { int image, class_id, x0, y0, cw, ch; float prob, rx, ry, rw, rh; };     // x0, y0: image column / row of cell 0; cw x ch cells

struct SgxObjResult {                                                                       // = sgx_obj3d_result (include/sgx.h)
    int found, class_id; float prob, centroid[3], size[3];
    int crop_points, kept_points, components, clusters, best_cluster_size, larger_window_points;
    float best_similar1, best_similar2, best_roi[4];
};

struct SgxObjArgs {
    int J, width, height, pitch, cap, slot_cap;          // pitch in floats; cap = cells per job, slot_cap = surviving clusters per job that the slot arrays hold
    int mean_k, min_size, max_size, w0;                  // w0: first SOR window half-width
    float fx, fy, cx, cy, dmin, dmax, tol2, ratio;       // tol2 = (float)((double)tol * (double)tol)
    double mul, tol, inv_fr, dabs_r;                     // inv_fr = 1 / (max(fx, fy) * Rmax); dabs_r = max |valid depth| * Rmax
    const float *depth; const double *twc; const SgxObjJob *jobs;
    float *wx, *wy, *wz, *dist, *scen;
    int *state, *parent, *label, *csize, *ji, *sroot, *ssize, *smm, *sorder;
    double *jd;
    SgxObjResult *results;
};

#ifndef SGX_EMU
#define sgx_obj_load(p) __hip_atomic_load((p), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)
#else
#define sgx_obj_load(p) (*(p))
#endif

SGX_DEV float sgx_obj_bits_f32(uint32_t b) { float f; __builtin_memcpy(&f, &b, 4); return f; }
SGX_DEV uint32_t sgx_obj_f32_bits(float f) { uint32_t b; __builtin_memcpy(&b, &f, 4); return b; }
// floats in an integer order (-0 below +0): min / max of them are integer atomics, exact and order-free
SGX_DEV int sgx_obj_ordered(float f) { const int i = (int)sgx_obj_f32_bits(f); return i < 0 ? (int)((uint32_t)i ^ 0x7fffffffu) : i; }
SGX_DEV float sgx_obj_unordered(int i) { return sgx_obj_bits_f32((uint32_t)(i < 0 ? (int)((uint32_t)i ^ 0x7fffffffu) : i)); }

// d2 as PCL's L2_Simple / squaredEuclideanDistance evaluate it in float: x, y, z order
SGX_DEV float sgx_obj_d2(float ax, float ay, float az, float bx, float by, float bz)
{
    const float dx = ax - bx, dy = ay - by, dz = az - bz;
    return (dx * dx + dy * dy) + dz * dz;
}

// Lower bound, less the rounding of both world points and of d2 itself, of the distance from a point at depth d to ANY point whose pixel is more than w pixels away
// in x or in y: every float d2 to such a point is >= bound * bound
SGX_DEV double sgx_obj_window_bound(double dabs, int w, double c1, double e2)
{
    return (dabs * (double)(w + 1) * c1 - e2) * (1.0 - 1.0 / 1048576.0);
}

// per job: counters to zero; the window constants from the job's Twc.  s = sqrt of Gershgorin's lower bound of the smallest eigenvalue of R^T R (1 for a rotation),
// S likewise the upper bound: |R v| >= s |v|, |R v| <= S |v|
SGX_KERNEL(64) k_obj3d_prep(SgxObjArgs A)
{
    SGX_THREADS_BEGIN(tid)
    const int j = (int)blockIdx.x * 64 + tid;
    if (j < A.J) {
        for (int i = 0; i < SGX_OBJ_JI; i++) A.ji[SGX_OBJ_JI * j + i] = 0;
        const double *T = A.twc + 16 * (size_t)A.jobs[j].image;
        double lo = 1e300, hi = 0;
        for (int a = 0; a < 3; a++) {
            double diag = 0, off = 0;
            for (int b = 0; b < 3; b++) {
                double g = 0;
                for (int r = 0; r < 3; r++) g += T[4 * r + a] * T[4 * r + b];
                if (a == b) diag = g; else off += fabs(g);
            }
            if (diag - off < lo) lo = diag - off;
            if (diag + off > hi) hi = diag + off;
        }
        const double s = lo > 0 ? sqrt(lo) : 0.0, S = sqrt(hi);
        const double tn = sqrt(T[3] * T[3] + T[7] * T[7] + T[11] * T[11]);
        double *d = A.jd + SGX_OBJ_JD * j;
        d[0] = s * A.inv_fr;
        d[1] = 2.0 * 1.01 * (1.0 / 16777216.0) * (4.0 * S * A.dabs_r + tn);
        if (!(d[0] == d[0]) || !(d[1] == d[1])) { d[0] = 0; d[1] = 0; }      // a Twc that is not finite: no window is ever proven, every search covers the crop
        d[2] = 0;
    }
    SGX_THREADS_END
}

// crop (Detector3D.cc:45-65) + camera point and world point (PointcloudMapping.cc:176-186) of every cell
SGX_KERNEL(256) k_obj3d_points(SgxObjArgs A)
{
    SGX_THREADS_BEGIN(tid)
    const int j = (int)blockIdx.y; const SgxObjJob jb = A.jobs[j];
    const int c = (int)blockIdx.x * 256 + tid;
    if (c < jb.cw * jb.ch) {
        const int n = jb.x0 + c % jb.cw, m = jb.y0 + c / jb.cw;
        const float d = A.depth[((size_t)jb.image * A.height + m) * A.pitch + n];
        const bool valid = !(d < A.dmin || d > A.dmax || d != d);
        const size_t o = (size_t)j * A.cap + c;
        float X = 0, Y = 0, Z = 0;
        if (valid) {
            const double *T = A.twc + 16 * (size_t)jb.image;
            const float z = d, x = ((float)n - A.cx) * d / A.fx, y = ((float)m - A.cy) * d / A.fy;
            X = (float)(T[0] * (double)x + T[1] * (double)y + T[2] * (double)z + T[3]);
            Y = (float)(T[4] * (double)x + T[5] * (double)y + T[6] * (double)z + T[7]);
            Z = (float)(T[8] * (double)x + T[9] * (double)y + T[10] * (double)z + T[11]);
            sgx_atomic_add(&A.ji[SGX_OBJ_JI * j + SGX_OBJ_N], 1);
        }
        A.wx[o] = X; A.wy[o] = Y; A.wz[o] = Z; A.dist[o] = 0; A.state[o] = valid ? SGX_OBJ_VALID : 0;
    }
    SGX_THREADS_END
}

// StatisticalOutlierRemoval, the mean distance to the mean_k nearest neighbours: one lane per point.  The K = mean_k + 1 smallest d2 of the point (its own 0 included)
// are found in a pixel window by bisection on the bit pattern of the K-th smallest (non-negative floats order as unsigned integers): 31 compare-and-count scans, no
// list.  The window is accepted when every point outside it is proven to be at least as far as the K-th found inside; otherwise it is doubled, up to the whole crop.
SGX_KERNEL(256) k_obj3d_sor(SgxObjArgs A)
{
    SGX_THREADS_BEGIN(tid)
    const int j = (int)blockIdx.y; const SgxObjJob jb = A.jobs[j];
    const int c = (int)blockIdx.x * 256 + tid;
    const int K = A.mean_k + 1;
    const size_t base = (size_t)j * A.cap;
    if (c < jb.cw * jb.ch && A.ji[SGX_OBJ_JI * j + SGX_OBJ_N] >= K && (A.state[base + c] & SGX_OBJ_VALID)) {
        const int u = c % jb.cw, v = c / jb.cw;
        const float px = A.wx[base + c], py = A.wy[base + c], pz = A.wz[base + c];
        const double dabs = fabs((double)A.depth[((size_t)jb.image * A.height + jb.y0 + v) * A.pitch + jb.x0 + u]);
        const double c1 = A.jd[SGX_OBJ_JD * j], e2 = A.jd[SGX_OBJ_JD * j + 1];
        int w = A.w0, rounds = 0, u0, u1, v0, v1;
        uint32_t kth;
        for (;;) {
            u0 = u - w < 0 ? 0 : u - w; u1 = u + w > jb.cw - 1 ? jb.cw - 1 : u + w;
            v0 = v - w < 0 ? 0 : v - w; v1 = v + w > jb.ch - 1 ? jb.ch - 1 : v + w;
            kth = 0;
            for (int bit = 30; bit >= 0; bit--) {
                const uint32_t t = kth | (1u << bit);
                int cnt = 0;
                for (int y = v0; y <= v1; y++) for (int x = u0; x <= u1; x++) {
                    const size_t q = base + (size_t)y * jb.cw + x;
                    if ((A.state[q] & SGX_OBJ_VALID) && sgx_obj_f32_bits(sgx_obj_d2(px, py, pz, A.wx[q], A.wy[q], A.wz[q])) < t) cnt++;
                }
                if (cnt < K) kth = t;                 // the K-th smallest is the largest t with fewer than K values below it
            }
            if (u0 == 0 && v0 == 0 && u1 == jb.cw - 1 && v1 == jb.ch - 1) break;
            if (kth < 0x7f800000u) {                  // K points found (else all ones)
                const double bound = sgx_obj_window_bound(dabs, w, c1, e2);
                if (bound > 0 && (double)sgx_obj_bits_f32(kth) < bound * bound) break;
            }
            w = 2 * w + 1; rounds++;
        }
        // the K smallest: everything below the K-th value, and the K-th value as often as is left.  The smallest is the point's own 0, so dropping it changes
        // nothing; the sum is exact in double on every input whose reference sum is (tests/obj3d_cases.py asserts it), so its order is free.
        double sum = 0; int cnt = 0;
        for (int y = v0; y <= v1; y++) for (int x = u0; x <= u1; x++) {
            const size_t q = base + (size_t)y * jb.cw + x;
            if (!(A.state[q] & SGX_OBJ_VALID)) continue;
            const float d2 = sgx_obj_d2(px, py, pz, A.wx[q], A.wy[q], A.wz[q]);
            if (sgx_obj_f32_bits(d2) < kth) { sum += (double)sqrtf(d2); cnt++; }
        }
        sum += (double)(K - cnt) * (double)sqrtf(sgx_obj_bits_f32(kth));
        A.dist[base + c] = (float)(sum / (double)A.mean_k);
        if (rounds) sgx_atomic_add(&A.ji[SGX_OBJ_JI * j + SGX_OBJ_LARGER], 1);
    }
    SGX_THREADS_END
}

// mean and variance of the distances and the removal threshold (one block per job; a fixed summation order: 256 contiguous runs, then their partial sums in order)
SGX_KERNEL(256) k_obj3d_stats(SgxObjArgs A)
{
    SGX_LDS double s1[256];
    SGX_LDS double s2[256];
    const int j = (int)blockIdx.x; const SgxObjJob jb = A.jobs[j];
    const int G = jb.cw * jb.ch, run = (G + 255) / 256;
    SGX_THREADS_BEGIN(tid)
    double a = 0, b = 0;
    const int e = (tid + 1) * run < G ? (tid + 1) * run : G;
    for (int c = tid * run; c < e; c++) {
        const size_t q = (size_t)j * A.cap + c;
        if (A.state[q] & SGX_OBJ_VALID) { const float d = A.dist[q]; a += (double)d; b += (double)(d * d); }
    }
    s1[tid] = a; s2[tid] = b;
    SGX_THREADS_END
    SGX_SYNC();
    SGX_THREADS_BEGIN(tid)
    if (tid == 0) {
        double sum = 0, sq = 0;
        for (int i = 0; i < 256; i++) { sum += s1[i]; sq += s2[i]; }
        const double n = (double)A.ji[SGX_OBJ_JI * j + SGX_OBJ_N];
        const double mean = sum / n, var = (sq - sum * sum / n) / (n - 1.0);
        A.jd[SGX_OBJ_JD * j + 2] = mean + A.mul * sqrt(var);
    }
    SGX_THREADS_END
}

// the filter (a point goes when its distance is above the threshold; a NaN threshold removes nothing, as in PCL) and every kept point as its own component
SGX_KERNEL(256) k_obj3d_keep(SgxObjArgs A)
{
    SGX_THREADS_BEGIN(tid)
    const int j = (int)blockIdx.y; const SgxObjJob jb = A.jobs[j];
    const int c = (int)blockIdx.x * 256 + tid;
    if (c < jb.cw * jb.ch) {
        const size_t q = (size_t)j * A.cap + c;
        const bool alive = A.ji[SGX_OBJ_JI * j + SGX_OBJ_N] > A.mean_k;             // n <= mean_k: no object (the reference reads past the neighbour list)
        const bool keep = alive && (A.state[q] & SGX_OBJ_VALID) && !((double)A.dist[q] > A.jd[SGX_OBJ_JD * j + 2]);
        if (keep) { A.state[q] |= SGX_OBJ_KEEP; sgx_atomic_add(&A.ji[SGX_OBJ_JI * j + SGX_OBJ_KEPT], 1); }
        A.parent[q] = keep ? c : -1; A.label[q] = -1; A.csize[q] = 0;
    }
    SGX_THREADS_END
}

// union-find whose links always point to the smaller cell, so the root of a finished component is its smallest cell whatever the order of the unions
SGX_DEV int sgx_obj_find(int *par, int x)
{
    for (;;) {
        const int p = sgx_obj_load(&par[x]);
        if (p == x) return x;
        const int gp = sgx_obj_load(&par[p]);
        if (gp == p) return p;
        sgx_atomic_min_i32(&par[x], gp);              // path halving; a parent only ever decreases
        x = gp;
    }
}

SGX_DEV void sgx_obj_union(int *par, int a, int b)
{
    for (;;) {
        a = sgx_obj_find(par, a); b = sgx_obj_find(par, b);
        if (a == b) return;
        if (a < b) { const int t = a; a = b; b = t; }
        const int old = sgx_atomic_min_i32(&par[a], b);
        if (old == a) return;                          // a was still a root: linked
        a = old;                                       // a had been linked to `old` meanwhile: old and b are still to be joined
    }
}

// EuclideanClusterExtraction's graph (d2 < tol2 on the kept points): every lane joins its point to the earlier points of the smallest window outside of which
// d2 >= tol2 is proven
SGX_KERNEL(256) k_obj3d_union(SgxObjArgs A)
{
    SGX_THREADS_BEGIN(tid)
    const int j = (int)blockIdx.y; const SgxObjJob jb = A.jobs[j];
    const int c = (int)blockIdx.x * 256 + tid;
    const size_t base = (size_t)j * A.cap;
    if (c < jb.cw * jb.ch && (A.state[base + c] & SGX_OBJ_KEEP)) {
        const int u = c % jb.cw, v = c / jb.cw;
        const float px = A.wx[base + c], py = A.wy[base + c], pz = A.wz[base + c];
        const double dabs = fabs((double)A.depth[((size_t)jb.image * A.height + jb.y0 + v) * A.pitch + jb.x0 + u]);
        const double c1 = A.jd[SGX_OBJ_JD * j], e2 = A.jd[SGX_OBJ_JD * j + 1];
        const int wmax = jb.cw > jb.ch ? jb.cw : jb.ch;
        const double need = A.tol * (1.0 + 1.0 / 1048576.0);
        const double guess = (need + e2) / (dabs * c1);
        int w = guess < (double)wmax ? (int)guess - 2 : wmax;      // NaN or infinite guess: the whole crop
        if (w < 0) w = 0;
        while (w < wmax && !(sgx_obj_window_bound(dabs, w, c1, e2) >= need)) w++;
        const int u0 = u - w < 0 ? 0 : u - w, u1 = u + w > jb.cw - 1 ? jb.cw - 1 : u + w, v0 = v - w < 0 ? 0 : v - w;
        for (int y = v0; y <= v; y++) for (int x = u0; x <= u1; x++) {
            const int c2 = y * jb.cw + x;
            if (c2 >= c) break;
            const size_t q = base + c2;
            if ((A.state[q] & SGX_OBJ_KEEP) && sgx_obj_d2(px, py, pz, A.wx[q], A.wy[q], A.wz[q]) < A.tol2) sgx_obj_union(A.parent + base, c, c2);
        }
    }
    SGX_THREADS_END
}

// component id = its smallest cell; sizes by a count
SGX_KERNEL(256) k_obj3d_label(SgxObjArgs A)
{
    SGX_THREADS_BEGIN(tid)
    const int j = (int)blockIdx.y; const SgxObjJob jb = A.jobs[j];
    const int c = (int)blockIdx.x * 256 + tid;
    const size_t base = (size_t)j * A.cap;
    if (c < jb.cw * jb.ch && (A.state[base + c] & SGX_OBJ_KEEP)) {
        int r = c;
        for (;;) { const int p = sgx_obj_load(&A.parent[base + r]); if (p == r) break; r = p; }      // read only: other lanes are still chasing
        A.label[base + c] = r;
        sgx_atomic_add(&A.csize[base + r], 1);
    }
    SGX_THREADS_END
}

// a component survives iff min <= size <= max; a survivor gets a slot for its reductions (the slot order is whatever the atomics give: k_obj3d_select orders them).
// csize[root] becomes the slot, or -1
SGX_KERNEL(256) k_obj3d_slots(SgxObjArgs A)
{
    SGX_THREADS_BEGIN(tid)
    const int j = (int)blockIdx.y; const SgxObjJob jb = A.jobs[j];
    const int c = (int)blockIdx.x * 256 + tid;
    const size_t base = (size_t)j * A.cap;
    if (c < jb.cw * jb.ch && (A.state[base + c] & SGX_OBJ_KEEP) && A.label[base + c] == c) {
        sgx_atomic_add(&A.ji[SGX_OBJ_JI * j + SGX_OBJ_COMP], 1);
        const int sz = A.csize[base + c];
        int slot = -1;
        if (sz >= A.min_size && sz <= A.max_size) {
            slot = sgx_atomic_add(&A.ji[SGX_OBJ_JI * j + SGX_OBJ_SLOTS], 1);
            if (slot < A.slot_cap) {                   // at most cells / min_size components can survive, which is what slot_cap holds
                const size_t s = (size_t)j * A.slot_cap + slot;
                A.sroot[s] = c; A.ssize[s] = sz;
                int *mm = A.smm + SGX_OBJ_MM * s;
                mm[0] = 0x7fffffff; mm[1] = -1; mm[2] = 0x7fffffff; mm[3] = -1;
                for (int i = 4; i < 7; i++) { mm[i] = 0x7fffffff; mm[i + 3] = (int)0x80000000; }
            } else slot = -1;
        }
        A.csize[base + c] = slot;
    }
    SGX_THREADS_END
}

// GetProjectedROI's pixel extremes and getMinMax3D of every surviving cluster
SGX_KERNEL(256) k_obj3d_minmax(SgxObjArgs A)
{
    SGX_THREADS_BEGIN(tid)
    const int j = (int)blockIdx.y; const SgxObjJob jb = A.jobs[j];
    const int c = (int)blockIdx.x * 256 + tid;
    const size_t base = (size_t)j * A.cap;
    if (c < jb.cw * jb.ch && (A.state[base + c] & SGX_OBJ_KEEP)) {
        const int slot = A.csize[base + A.label[base + c]];
        if (slot >= 0) {
            int *mm = A.smm + SGX_OBJ_MM * ((size_t)j * A.slot_cap + slot);
            const int x = jb.x0 + c % jb.cw, y = jb.y0 + c / jb.cw;
            sgx_atomic_min_i32(&mm[0], x); sgx_atomic_max(&mm[1], x); sgx_atomic_min_i32(&mm[2], y); sgx_atomic_max(&mm[3], y);
            const int ox = sgx_obj_ordered(A.wx[base + c]), oy = sgx_obj_ordered(A.wy[base + c]), oz = sgx_obj_ordered(A.wz[base + c]);
            sgx_atomic_min_i32(&mm[4], ox); sgx_atomic_min_i32(&mm[5], oy); sgx_atomic_min_i32(&mm[6], oz);
            sgx_atomic_max(&mm[7], ox); sgx_atomic_max(&mm[8], oy); sgx_atomic_max(&mm[9], oz);
        }
    }
    SGX_THREADS_END
}

// pcl::compute3DCentroid on a dense cloud: a running float sum in ascending point order, divided by (float)n.  One lane per surviving cluster: the order is the result
SGX_KERNEL(64) k_obj3d_centroid(SgxObjArgs A)
{
    SGX_THREADS_BEGIN(tid)
    const int j = (int)blockIdx.y; const SgxObjJob jb = A.jobs[j];
    const int slot = (int)blockIdx.x * 64 + tid;
    int ns = A.ji[SGX_OBJ_JI * j + SGX_OBJ_SLOTS]; if (ns > A.slot_cap) ns = A.slot_cap;
    if (slot < ns) {
        const size_t base = (size_t)j * A.cap, s = (size_t)j * A.slot_cap + slot;
        const int root = A.sroot[s], G = jb.cw * jb.ch;
        float x = 0, y = 0, z = 0;
        for (int c = root; c < G; c++)
            if (A.label[base + c] == root) { x += A.wx[base + c]; y += A.wy[base + c]; z += A.wz[base + c]; }
        const float n = (float)A.ssize[s];
        A.scen[3 * s] = x / n; A.scen[3 * s + 1] = y / n; A.scen[3 * s + 2] = z / n;
    }
    SGX_THREADS_END
}

// Detector3D::GetSimilarity (:204-218) in float; cv::Rect_ intersection (empty when a side is <= 0); powf(x, 2) taken as x * x; deviate == 0 divides in IEEE
SGX_DEV float sgx_obj_similarity(float x1, float y1, float w1, float h1, float x2, float y2, float w2, float h2, int points)
{
    const float c1x = x1 + w1 / 2, c1y = y1 + h1 / 2, c2x = x2 + w2 / 2, c2y = y2 + h2 / 2;
    const float area1 = w1 * h1, area2 = w2 * h2;
    const float ix = x1 > x2 ? x1 : x2, iy = y1 > y2 ? y1 : y2;                      // std::max(a, b) = a < b ? b : a
    const float r1 = x1 + w1, r2 = x2 + w2, b1 = y1 + h1, b2 = y2 + h2;
    float iw = (r2 < r1 ? r2 : r1) - ix, ih = (b2 < b1 ? b2 : b1) - iy;              // std::min(a, b) = b < a ? b : a
    if (iw <= 0 || ih <= 0) { iw = 0; ih = 0; }
    const float area0 = iw * ih;
    const float overlap = area0 / (area1 + area2 - area0);
    const float dx = c1x - c2x, dy = c1y - c2y;
    const float deviate = dx * dx + dy * dy;
    const float score = (float)((double)(float)points / 10.0);
    return (overlap * score) / deviate;
}

// the selection loop (:101-140) over the surviving clusters in PCL's order (size descending; equal sizes by smallest point), and the result record
SGX_KERNEL(64) k_obj3d_select(SgxObjArgs A)
{
    const int j = (int)blockIdx.x;
    int ns = A.ji[SGX_OBJ_JI * j + SGX_OBJ_SLOTS]; if (ns > A.slot_cap) ns = A.slot_cap;
    const size_t s0 = (size_t)j * A.slot_cap;
    SGX_THREADS_BEGIN(tid)
    for (int s = tid; s < ns; s += 64) {
        const int sz = A.ssize[s0 + s], root = A.sroot[s0 + s];
        int rank = 0;
        for (int t = 0; t < ns; t++) { const int tz = A.ssize[s0 + t]; if (tz > sz || (tz == sz && A.sroot[s0 + t] < root)) rank++; }
        A.sorder[s0 + rank] = s;
    }
    SGX_THREADS_END
    SGX_SYNC();
    SGX_THREADS_BEGIN(tid)
    if (tid == 0) {
        const SgxObjJob jb = A.jobs[j];
        float best1 = -1.0f, best2 = -1.0f; int best = -1; float broi[4] = { 0, 0, 0, 0 };
        for (int r = 0; r < ns; r++) {
            const size_t s = s0 + A.sorder[s0 + r];
            if (A.scen[3 * s + 2] < A.dmin) continue;                               // the reference compares the WORLD z with the camera's minimum depth: kept
            const int *mm = A.smm + SGX_OBJ_MM * s;
            const float rx = (float)(uint32_t)mm[0], ry = (float)(uint32_t)mm[2];
            const float rw = (float)(uint32_t)mm[1] - rx, rh = (float)(uint32_t)mm[3] - ry;
            const float similar = sgx_obj_similarity(jb.rx, jb.ry, jb.rw, jb.rh, rx, ry, rw, rh, A.ssize[s]);
            if (similar > best1) { best = (int)(s - s0); best1 = similar; broi[0] = rx; broi[1] = ry; broi[2] = rw; broi[3] = rh; }
            else if (similar > best2) best2 = similar;
        }
        SgxObjResult R;
        R.found = best >= 0 && !(best1 * A.ratio < best2 && best2 > 0) ? 1 : 0;
        R.class_id = jb.class_id; R.prob = jb.prob;
        for (int i = 0; i < 3; i++) { R.centroid[i] = 0; R.size[i] = 0; }
        if (R.found) {
            const int *mm = A.smm + SGX_OBJ_MM * (s0 + best);
            for (int i = 0; i < 3; i++) { R.centroid[i] = A.scen[3 * (s0 + best) + i]; R.size[i] = sgx_obj_unordered(mm[7 + i]) - sgx_obj_unordered(mm[4 + i]); }
        }
        const int *ji = A.ji + SGX_OBJ_JI * j;
        R.crop_points = ji[SGX_OBJ_N]; R.kept_points = ji[SGX_OBJ_KEPT]; R.components = ji[SGX_OBJ_COMP]; R.clusters = ns;
        R.best_cluster_size = best >= 0 ? A.ssize[s0 + best] : 0; R.larger_window_points = ji[SGX_OBJ_LARGER];
        R.best_similar1 = best1; R.best_similar2 = best2;
        for (int i = 0; i < 4; i++) R.best_roi[i] = broi[i];
        A.results[j] = R;
    }
    SGX_THREADS_END
}
