// sgx_octomap_kernels.h — octomap_server's insertScan and the tree queries of publishAll (src/octomap_server/src/OctomapServer.cpp:261-480, :484-, :934-1107) on a
// device-resident map of depth-16 cells.  The map is a hash of 8 x 8 x 8 bricks: an open-addressing table of brick keys (64-bit CAS), per table slot two
// 512-bit masks (the scan's free and occupied sets), per brick 512 log-odds in Morton order of the local cell (bit 3i = x bit i, 3i+1 = y, 3i+2 = z), one reserved
// NaN pattern for unknown.  Every atomic is an integer or / min / max / add / CAS; a cell is written once per scan, by the one lane that owns it in k_octo_apply.
// Phase style of sgx_rt.h: the same source is the emulator's.
#pragma once
#include "sgx_rt.h"
#include <math.h>
#include <float.h>

#define SGX_OCTO_EMPTY 0xFFFFFFFFFFFFFFFFull     /* no brick key: a key has 39 bits */
#define SGX_OCTO_UNKNOWN 0xFFFFFFFFu             /* the cell pattern for unknown; arithmetic never produces it (values are clamped finite floats) */
#define SGX_OCTO_QNAN 0x7FC00000u                /* what search answers for unknown */
enum { OCTO_ORIGIN_OUT_OF_RANGE = 1, OCTO_RAY_LEFT_KEYSPACE = 2, OCTO_MAP_FULL = 4, OCTO_TOO_MANY_POINTS = 8 };
// device state of the handle (ints)
enum { OCTO_COUNT = 0,      // committed bricks
       OCTO_NEW,            // bricks this scan adds
       OCTO_FAIL,           // the table had no place for a key of this scan
       OCTO_OK,             // the scan is applied
       OCTO_NTOUCHED,       // table slots with a mask bit
       OCTO_N,              // points of the scan taken (0 when there are too many)
       OCTO_OKEY,           // +0..2 origin key, +3 valid
       OCTO_REC = 12,       // the record being built (SgxOctoRecord, 16 ints)
       OCTO_STATE_INTS = 32 };

struct SgxOctoPoint { float x, y, z; uint32_t rgba; };
struct SgxOctoRecord { int32_t n_in, n_passed, n_truncated, n_bad_end_key, n_invalid_rays, n_free_updates, n_occupied_updates, n_new_cells, bbx_min[3], bbx_max[3], flags, reserved; };
struct SgxOctoCell { uint16_t key[3], reserved; float x, y, z, logodds; };
struct SgxOctoBounds { int32_t n_known, n_occupied, n_free, n_bricks, key_min[3], key_max[3]; };
struct SgxOctoRay { float ex, ey, ez; int32_t mode; };        // mode 0: no ray, 1: ray to the point, 2: ray to new_end, whose key joins the free set

struct SgxOctoArgs {
    // the map
    unsigned long long *tab_key; int *tab_idx; uint32_t *fmask, *omask; int T;          // T a power of two; masks 16 words per table slot
    uint32_t *cells; unsigned long long *brick_key; int max_bricks;                     // 512 words per brick, the brick's key
    int *st; int *touched; SgxOctoRay *rays; int max_points;
    // the scan
    const SgxOctoPoint *points; const int32_t *n_points; const float *s2w; SgxOctoRecord *record;
    double res, rf, max_range; float hit, miss, cmin, cmax; float lo[3], hi[3];
    // queries
    double zmin, zmax; int want_occupied, cap, m;
    unsigned long long *morton; int *order, *cnt; SgxOctoCell *out; int32_t *n_out; SgxOctoBounds *bounds;
    const uint16_t *qkeys; const float *qpts; float *qout;
    int8_t *grid; int gw, gh, gx0, gy0, gz0, gz1;
};

#ifndef SGX_EMU
SGX_DEV unsigned long long octo_cas64(unsigned long long *p, unsigned long long cmp, unsigned long long v) { return atomicCAS(p, cmp, v); }
SGX_DEV unsigned long long octo_load64(const unsigned long long *p) { return __atomic_load_n(p, __ATOMIC_RELAXED); }
SGX_DEV int octo_load32(const int *p) { return __atomic_load_n(p, __ATOMIC_RELAXED); }
// a mask word that other lanes or into: a relaxed atomic load of workgroup scope, so the compiler does not take the word for race-free and the CU's cache may still serve it
SGX_DEV uint32_t octo_load_word(const uint32_t *p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP); }
#else
static inline unsigned long long octo_cas64(unsigned long long *p, unsigned long long cmp, unsigned long long v) { unsigned long long o = *p; if (o == cmp) *p = v; return o; }
static inline unsigned long long octo_load64(const unsigned long long *p) { return *p; }
static inline int octo_load32(const int *p) { return *p; }
static inline uint32_t octo_load_word(const uint32_t *p) { return *p; }
#endif

#ifndef SGX_EMU
#define OCTO_HD __host__ __device__ __forceinline__      /* the key arithmetic is also the host's (grid_header) */
#else
#define OCTO_HD static inline
#endif
SGX_DEV float octo_bits_f(uint32_t u) { float f; memcpy(&f, &u, 4); return f; }
SGX_DEV uint32_t octo_f_bits(float f) { uint32_t u; memcpy(&u, &f, 4); return u; }
SGX_DEV bool octo_finite(float v) { return (octo_f_bits(v) & 0x7F800000u) != 0x7F800000u; }
// coordToKeyChecked of one coordinate: floor(rf * (double)c) + 32768 in [0, 65536)
OCTO_HD bool octo_key1(double rf, float c, int *k)
{
    const double f = floor(rf * (double)c);
    if (!(f >= -32768.0 && f < 32768.0)) { *k = 0; return false; }                          // NaN fails too
    *k = (int)f + 32768; return true;
}
OCTO_HD double octo_coord(double res, int k) { return ((double)(k - 32768) + 0.5) * res; }
SGX_DEV unsigned long long octo_brick(int kx, int ky, int kz) { return ((unsigned long long)(kx >> 3) << 26) | ((unsigned long long)(ky >> 3) << 13) | (unsigned long long)(kz >> 3); }
SGX_DEV int octo_spread3(int v) { return (v & 1) | ((v & 2) << 2) | ((v & 4) << 4); }
SGX_DEV int octo_squeeze3(int m) { return (m & 1) | ((m >> 2) & 2) | ((m >> 4) & 4); }
SGX_DEV int octo_local(int kx, int ky, int kz) { return octo_spread3(kx & 7) | (octo_spread3(ky & 7) << 1) | (octo_spread3(kz & 7) << 2); }
SGX_DEV unsigned octo_hash(unsigned long long k) { k ^= k >> 33; k *= 0xff51afd7ed558ccdull; k ^= k >> 29; return (unsigned)k; }
// Morton code of a brick's 13-bit coordinates
SGX_DEV unsigned long long octo_morton(unsigned long long bk)
{
    const unsigned bx = (unsigned)(bk >> 26) & 8191u, by = (unsigned)(bk >> 13) & 8191u, bz = (unsigned)bk & 8191u;
    unsigned long long m = 0;
    for (int i = 0; i < 13; i++) m |= ((unsigned long long)((bx >> i) & 1u) << (3 * i)) | ((unsigned long long)((by >> i) & 1u) << (3 * i + 1)) | ((unsigned long long)((bz >> i) & 1u) << (3 * i + 2));
    return m;
}
// the table slot of a brick key, -1 if absent
SGX_DEV int octo_find(const SgxOctoArgs &A, unsigned long long bk)
{
    unsigned h = octo_hash(bk) & (unsigned)(A.T - 1);
    for (int i = 0; i < A.T; i++) {
        const unsigned long long cur = octo_load64(A.tab_key + h);
        if (cur == bk) return (int)h;
        if (cur == SGX_OCTO_EMPTY) return -1;
        h = (h + 1) & (unsigned)(A.T - 1);
    }
    return -1;
}
// the same, taking the first empty slot when absent; -1 and OCTO_FAIL when the table is full
SGX_DEV int octo_insert(const SgxOctoArgs &A, unsigned long long bk)
{
    unsigned h = octo_hash(bk) & (unsigned)(A.T - 1);
    for (int i = 0; i < A.T; i++) {
        unsigned long long cur = octo_load64(A.tab_key + h);
        if (cur == SGX_OCTO_EMPTY) cur = octo_cas64(A.tab_key + h, SGX_OCTO_EMPTY, bk);
        if (cur == bk || cur == SGX_OCTO_EMPTY) return (int)h;
        h = (h + 1) & (unsigned)(A.T - 1);
    }
    sgx_atomic_max(A.st + OCTO_FAIL, 1);
    return -1;
}
SGX_DEV void octo_mark(uint32_t *mask, int slot, int kx, int ky, int kz)
{
    const int b = octo_local(kx, ky, kz);
    sgx_atomic_or(mask + 16 * (size_t)slot + (b >> 5), 1u << (b & 31));
}
// a ray's marks: a mask word is a block of 4 x 4 x 2 cells, so successive cells of a ray mostly fall into one word.  The lane gathers their bits and writes a word
// once, and not at all when a load already shows the bits (near the sensor every ray of the scan crosses the same cells; a bit is only ever set during a
// scan, so a stale load can cost a redundant atomic, never a lost mark)
struct OctoMarks { uint32_t *word; uint32_t bits; };
SGX_DEV void octo_marks_flush(OctoMarks &mk)
{
    if (mk.word && (octo_load_word(mk.word) & mk.bits) != mk.bits) sgx_atomic_or(mk.word, mk.bits);
    mk.word = nullptr; mk.bits = 0;
}
SGX_DEV void octo_marks_add(OctoMarks &mk, uint32_t *mask, int slot, int kx, int ky, int kz)
{
    const int b = octo_local(kx, ky, kz);
    uint32_t *w = mask + 16 * (size_t)slot + (b >> 5);
    if (w != mk.word) { octo_marks_flush(mk); mk.word = w; }
    mk.bits |= 1u << (b & 31);
}

// ---- one scan -------------------------------------------------------------------------------------------------------------------------------------------------
// the scan's state: point count, origin key, an empty record
SGX_KERNEL(64) k_octo_begin(SgxOctoArgs A)
{
    SGX_THREADS_BEGIN(t)
    if (t == 0 && blockIdx.x == 0) {
        int *st = A.st; int *r = st + OCTO_REC;
        for (int i = 0; i < 16; i++) r[i] = 0;
        for (int i = 0; i < 3; i++) { r[8 + i] = 65535; r[11 + i] = 0; }
        const int n = A.n_points[0];
        r[0] = n;
        int flags = 0, take = n < 0 ? 0 : n;
        if (n > A.max_points) { flags |= OCTO_TOO_MANY_POINTS; take = 0; }
        int k[3]; bool ok = true;
        for (int i = 0; i < 3; i++) ok = octo_key1(A.rf, A.s2w[4 * i + 3], &k[i]) && ok;
        if (!ok) flags |= OCTO_ORIGIN_OUT_OF_RANGE;
        else if (take > 0 || n == 0) for (int i = 0; i < 3; i++) { r[8 + i] = k[i]; r[11 + i] = k[i]; }
        for (int i = 0; i < 3; i++) st[OCTO_OKEY + i] = k[i];
        st[OCTO_OKEY + 3] = ok ? 1 : 0;
        r[14] = flags;
        st[OCTO_NEW] = 0; st[OCTO_FAIL] = 0; st[OCTO_OK] = 0; st[OCTO_NTOUCHED] = 0; st[OCTO_N] = take;
    }
    SGX_THREADS_END
}

// pcl::transformPointCloud, the three PassThrough filters, the range test, the end key into the occupied set and the update box; leaves the ray of the point
SGX_KERNEL(256) k_octo_points(SgxOctoArgs A)
{
    SGX_LDS int lds_r[16];                                                                  // this workgroup's share of the record (the same slots)
    if ((int)blockIdx.x * 256 >= A.st[OCTO_N]) return;
    SGX_THREADS_BEGIN(t)
    if (t < 16) lds_r[t] = t >= 8 && t < 11 ? 65535 : 0;
    SGX_THREADS_END
    SGX_SYNC();
    SGX_THREADS_BEGIN(t)
    const int i = (int)blockIdx.x * 256 + t;
    if (i < A.st[OCTO_N]) {
        int *r = lds_r;
        const SgxOctoPoint q = A.points[i];
        const float *m = A.s2w;
        float p[3];
        for (int a = 0; a < 3; a++) p[a] = ((m[4 * a] * q.x + m[4 * a + 1] * q.y) + m[4 * a + 2] * q.z) + m[4 * a + 3];
        bool keep = true;
        for (int a = 0; a < 3; a++) keep = keep && octo_finite(p[a]) && !(p[a] < A.lo[a] || p[a] > A.hi[a]);
        SgxOctoRay ray; ray.ex = p[0]; ray.ey = p[1]; ray.ez = p[2]; ray.mode = 0;
        if (keep) {
            sgx_atomic_add(r + 1, 1);
            const float o[3] = { m[3], m[7], m[11] };
            const float dx = p[0] - o[0], dy = p[1] - o[1], dz = p[2] - o[2];
            const float n2 = (dx * dx + dy * dy) + dz * dz;
            const double norm = sqrt((double)n2);
            if (A.max_range < 0.0 || norm <= A.max_range) {
                ray.mode = 1;
                int k[3]; bool ok = true;
                for (int a = 0; a < 3; a++) ok = octo_key1(A.rf, p[a], &k[a]) && ok;
                if (ok) {
                    const int slot = octo_insert(A, octo_brick(k[0], k[1], k[2]));
                    if (slot >= 0) octo_mark(A.omask, slot, k[0], k[1], k[2]);
                    for (int a = 0; a < 3; a++) { sgx_atomic_min_i32(r + 8 + a, k[a]); sgx_atomic_max(r + 11 + a, k[a]); }
                } else sgx_atomic_add(r + 3, 1);
            } else {
                const float len = (float)norm, mr = (float)A.max_range;
                ray.ex = o[0] + (dx / len) * mr; ray.ey = o[1] + (dy / len) * mr; ray.ez = o[2] + (dz / len) * mr; ray.mode = 2;
                sgx_atomic_add(r + 2, 1);
            }
        }
        A.rays[i] = ray;
    }
    SGX_THREADS_END
    SGX_SYNC();
    SGX_THREADS_BEGIN(t)
    int *r = A.st + OCTO_REC;
    if (t >= 1 && t < 4 && lds_r[t]) sgx_atomic_add(r + t, lds_r[t]);
    if (t >= 8 && t < 11) sgx_atomic_min_i32(r + t, lds_r[t]);
    if (t >= 11 && t < 14) sgx_atomic_max(r + t, lds_r[t]);
    SGX_THREADS_END
}

// computeRayKeys, one lane per ray: the double DDA in registers, the table slot cached while key >> 3 stands, the marks gathered per mask word (OctoMarks); the
// count of refused rays and the update box of truncated rays are reduced in LDS, one set of global atomics a workgroup
SGX_KERNEL(64) k_octo_rays(SgxOctoArgs A)
{
    SGX_LDS int lds_r[16];                                                                  // this workgroup's share of the record (the same slots)
    if ((int)blockIdx.x * 64 >= A.st[OCTO_N]) return;
    SGX_THREADS_BEGIN(t)
    if (t < 16) lds_r[t] = t >= 8 && t < 11 ? 65535 : 0;
    SGX_THREADS_END
    SGX_SYNC();
    SGX_THREADS_BEGIN(t)
    const int i = (int)blockIdx.x * 64 + t;
    if (i < A.st[OCTO_N] && A.rays[i].mode != 0) {
        int *r = lds_r;
        const SgxOctoRay ray = A.rays[i];
        const float o[3] = { A.s2w[3], A.s2w[7], A.s2w[11] }, e[3] = { ray.ex, ray.ey, ray.ez };
        int key[3], kend[3]; bool ok = A.st[OCTO_OKEY + 3] != 0;
        for (int a = 0; a < 3; a++) { key[a] = A.st[OCTO_OKEY + a]; ok = octo_key1(A.rf, e[a], &kend[a]) && ok; }
        if (!ok) sgx_atomic_add(r + 4, 1);
        else {
            unsigned long long cached = SGX_OCTO_EMPTY; int slot = -1;
            OctoMarks mk; mk.word = nullptr; mk.bits = 0;
            if (ray.mode == 2) {                                                            // new_end's key joins the free set and the update box
                slot = octo_insert(A, cached = octo_brick(kend[0], kend[1], kend[2]));
                if (slot >= 0) octo_mark(A.fmask, slot, kend[0], kend[1], kend[2]);
                for (int a = 0; a < 3; a++) { sgx_atomic_min_i32(r + 8 + a, kend[a]); sgx_atomic_max(r + 11 + a, kend[a]); }
            }
            if (!(key[0] == kend[0] && key[1] == kend[1] && key[2] == kend[2])) {
                float d[3] = { e[0] - o[0], e[1] - o[1], e[2] - o[2] };
                const float n2 = (d[0] * d[0] + d[1] * d[1]) + d[2] * d[2];
                const float length = (float)sqrt((double)n2);
                int step[3]; double tmax[3], tdelta[3];
                for (int a = 0; a < 3; a++) {
                    d[a] = d[a] / length;
                    step[a] = d[a] > 0.0f ? 1 : (d[a] < 0.0f ? -1 : 0);
                    if (step[a] != 0) {
                        const double border = octo_coord(A.res, key[a]) + (double)(float)((double)step[a] * A.res * 0.5);
                        tmax[a] = (border - (double)o[a]) / (double)d[a];
                        tdelta[a] = A.res / fabs((double)d[a]);
                    } else { tmax[a] = DBL_MAX; tdelta[a] = DBL_MAX; }
                }
                bool left = false;
                for (int guard = 0; guard < 3 * 65536; guard++) {
                    const unsigned long long bk = octo_brick(key[0], key[1], key[2]);       // append key
                    if (bk != cached) {
                        if (octo_load32(A.st + OCTO_FAIL)) break;                           // a full table: the scan is refused, nothing more to mark
                        cached = bk; slot = octo_insert(A, bk);
                    }
                    if (slot < 0) break;
                    octo_marks_add(mk, A.fmask, slot, key[0], key[1], key[2]);
                    int dim;
                    if (tmax[0] < tmax[1]) dim = tmax[0] < tmax[2] ? 0 : 2; else dim = tmax[1] < tmax[2] ? 1 : 2;
                    const int nk = key[dim] + step[dim];
                    if (nk < 0 || nk > 65535) { left = true; break; }
                    key[dim] = nk; tmax[dim] += tdelta[dim];
                    if (key[0] == kend[0] && key[1] == kend[1] && key[2] == kend[2]) break;
                    const double dist = fmin(fmin(tmax[0], tmax[1]), tmax[2]);
                    if (dist > (double)length) break;
                }
                octo_marks_flush(mk);
                if (left) sgx_atomic_or(r + 14, (int)OCTO_RAY_LEFT_KEYSPACE);
            }
        }
    }
    SGX_THREADS_END
    SGX_SYNC();
    SGX_THREADS_BEGIN(t)
    int *r = A.st + OCTO_REC;
    if (t == 4 && lds_r[t]) sgx_atomic_add(r + t, lds_r[t]);
    if (t >= 8 && t < 11 && lds_r[t] != 65535) sgx_atomic_min_i32(r + t, lds_r[t]);
    if (t >= 11 && t < 14 && lds_r[t] != 0) sgx_atomic_max(r + t, lds_r[t]);
    if (t == 14 && lds_r[t]) sgx_atomic_or(r + t, lds_r[t]);
    SGX_THREADS_END
}

// every table slot with a mask bit joins the touched list; one without a brick gets the next brick index
SGX_KERNEL(256) k_octo_assign(SgxOctoArgs A)
{
    SGX_THREADS_BEGIN(t)
    const int s = (int)blockIdx.x * 256 + t;
    if (s < A.T && A.st[OCTO_N] > 0 && A.tab_key[s] != SGX_OCTO_EMPTY) {
        uint32_t any = 0;
        for (int w = 0; w < 16; w++) any |= A.fmask[16 * (size_t)s + w] | A.omask[16 * (size_t)s + w];
        if (any) {
            A.touched[sgx_atomic_add(A.st + OCTO_NTOUCHED, 1)] = s;
            if (A.tab_idx[s] < 0) {
                const int idx = A.st[OCTO_COUNT] + sgx_atomic_add(A.st + OCTO_NEW, 1);
                if (idx < A.max_bricks) { A.tab_idx[s] = idx; A.brick_key[idx] = A.tab_key[s]; }
            }
        }
    }
    SGX_THREADS_END
}

// the scan is refused when the table had no place for a key or committed + new bricks exceed max_bricks: a count of distinct keys, whatever the arrival order
SGX_DEV bool octo_full(const SgxOctoArgs &A) { return A.st[OCTO_FAIL] != 0 || A.st[OCTO_COUNT] + A.st[OCTO_NEW] > A.max_bricks; }

// one pass of 64 lanes per touched brick, 8 cells a lane: free and not occupied gets miss, occupied gets hit; the masks are cleared.  A refused scan only clears.
SGX_KERNEL(64) k_octo_apply(SgxOctoArgs A)
{
    const int nt = A.st[OCTO_NTOUCHED], ok = octo_full(A) ? 0 : 1, count = A.st[OCTO_COUNT];
    for (int j = (int)blockIdx.x; j < nt; j += (int)gridDim.x) {
        SGX_THREADS_BEGIN(t)
        const int s = A.touched[j];
        const int w = t >> 2, sh = (t & 3) * 8;
        const uint32_t f = (A.fmask[16 * (size_t)s + w] >> sh) & 255u, oc = (A.omask[16 * (size_t)s + w] >> sh) & 255u;
        if (ok) {
            const int idx = A.tab_idx[s];
            uint32_t *cell = A.cells + 512 * (size_t)idx + 8 * t;
            const bool fresh = idx >= count;
            int nf = 0, no = 0, nn = 0;
            for (int c = 0; c < 8; c++) {
                uint32_t bits = fresh ? SGX_OCTO_UNKNOWN : cell[c];
                const bool isf = ((f >> c) & 1u) && !((oc >> c) & 1u), iso = (oc >> c) & 1u;
                if (isf || iso) {
                    float v = 0.0f;
                    if (bits == SGX_OCTO_UNKNOWN) nn++; else v = octo_bits_f(bits);
                    v = v + (iso ? A.hit : A.miss);
                    v = v < A.cmin ? A.cmin : (v > A.cmax ? A.cmax : v);
                    bits = octo_f_bits(v);
                    if (iso) no++; else nf++;
                }
                if (fresh || isf || iso) cell[c] = bits;
            }
            int *r = A.st + OCTO_REC;
            if (nf) sgx_atomic_add(r + 5, nf);
            if (no) sgx_atomic_add(r + 6, no);
            if (nn) sgx_atomic_add(r + 7, nn);
        }
        SGX_THREADS_END
        SGX_SYNC();
        SGX_THREADS_BEGIN(t)
        if (t < 16) { const int s = A.touched[j]; A.fmask[16 * (size_t)s + t] = 0; A.omask[16 * (size_t)s + t] = 0; }
        SGX_THREADS_END
        SGX_SYNC();
    }
}

// the verdict and the record go out; an applied scan commits its bricks
SGX_KERNEL(64) k_octo_finish(SgxOctoArgs A)
{
    SGX_THREADS_BEGIN(t)
    if (t == 0 && blockIdx.x == 0) {
        int *st = A.st;
        const bool full = octo_full(A);
        // a refused scan's walks end early in an order that is not defined, so whether one of them would have left the key space is not reported for it
        if (full) st[OCTO_REC + 14] = (st[OCTO_REC + 14] & ~(int)OCTO_RAY_LEFT_KEYSPACE) | OCTO_MAP_FULL;
        st[OCTO_OK] = full ? 0 : 1;
        if (!full) st[OCTO_COUNT] += st[OCTO_NEW];
        SgxOctoRecord rec; memcpy(&rec, st + OCTO_REC, sizeof rec);
        *A.record = rec;
    }
    SGX_THREADS_END
}

// a refused scan leaves keys without a brick in the table: the table is emptied and the committed bricks entered again, so that what a later scan finds there does not
// depend on the order in which the refused one arrived
SGX_KERNEL(256) k_octo_rollback_clear(SgxOctoArgs A)
{
    SGX_THREADS_BEGIN(t)
    const int s = (int)blockIdx.x * 256 + t;
    if (s < A.T && !A.st[OCTO_OK] && A.st[OCTO_N] > 0) { A.tab_key[s] = SGX_OCTO_EMPTY; A.tab_idx[s] = -1; }
    SGX_THREADS_END
}
SGX_KERNEL(256) k_octo_rollback_enter(SgxOctoArgs A)
{
    SGX_THREADS_BEGIN(t)
    const int b = (int)blockIdx.x * 256 + t;
    if (b < A.st[OCTO_COUNT] && !A.st[OCTO_OK] && A.st[OCTO_N] > 0) {
        const int s = octo_insert(A, A.brick_key[b]);
        if (s >= 0) A.tab_idx[s] = b;
    }
    SGX_THREADS_END
}

SGX_KERNEL(256) k_octo_reset(SgxOctoArgs A)
{
    SGX_THREADS_BEGIN(t)
    const int s = (int)blockIdx.x * 256 + t;
    if (s < A.T) {
        A.tab_key[s] = SGX_OCTO_EMPTY; A.tab_idx[s] = -1;
        for (int w = 0; w < 16; w++) { A.fmask[16 * (size_t)s + w] = 0; A.omask[16 * (size_t)s + w] = 0; }
    }
    if (s < OCTO_STATE_INTS) A.st[s] = 0;
    SGX_THREADS_END
}

// ---- queries --------------------------------------------------------------------------------------------------------------------------------------------------
SGX_DEV void octo_brick_origin(unsigned long long bk, int *k) { k[0] = (int)((bk >> 26) & 8191u) << 3; k[1] = (int)((bk >> 13) & 8191u) << 3; k[2] = (int)(bk & 8191u) << 3; }

SGX_KERNEL(64) k_octo_bounds_init(SgxOctoArgs A)
{
    SGX_THREADS_BEGIN(t)
    if (t == 0 && blockIdx.x == 0) {
        SgxOctoBounds b; b.n_known = b.n_occupied = b.n_free = 0; b.n_bricks = A.st[OCTO_COUNT];
        for (int i = 0; i < 3; i++) { b.key_min[i] = 65535; b.key_max[i] = 0; }
        *A.bounds = b;
    }
    SGX_THREADS_END
}
SGX_KERNEL(64) k_octo_bounds(SgxOctoArgs A)
{
    SGX_LDS int lds_b[9];                                                                   // known, occupied, free, min x y z, max x y z of this workgroup's bricks
    const int nb = A.st[OCTO_COUNT];
    if ((int)blockIdx.x >= nb) return;
    SGX_THREADS_BEGIN(t)
    if (t < 9) lds_b[t] = t >= 3 && t < 6 ? 65535 : 0;
    SGX_THREADS_END
    SGX_SYNC();
    for (int j = (int)blockIdx.x; j < nb; j += (int)gridDim.x) {
        SGX_THREADS_BEGIN(t)
        int k0[3]; octo_brick_origin(A.brick_key[j], k0);
        int nk = 0, no = 0, lo[3] = { 65535, 65535, 65535 }, hi[3] = { 0, 0, 0 };
        for (int c = 0; c < 8; c++) {
            const int m = 8 * t + c;
            const uint32_t bits = A.cells[512 * (size_t)j + m];
            if (bits == SGX_OCTO_UNKNOWN) continue;
            nk++; if (octo_bits_f(bits) >= 0.0f) no++;
            const int k[3] = { k0[0] + octo_squeeze3(m), k0[1] + octo_squeeze3(m >> 1), k0[2] + octo_squeeze3(m >> 2) };
            for (int a = 0; a < 3; a++) { lo[a] = k[a] < lo[a] ? k[a] : lo[a]; hi[a] = k[a] > hi[a] ? k[a] : hi[a]; }
        }
        if (nk) {
            sgx_atomic_add(lds_b + 0, nk); sgx_atomic_add(lds_b + 1, no); sgx_atomic_add(lds_b + 2, nk - no);
            for (int a = 0; a < 3; a++) { sgx_atomic_min_i32(lds_b + 3 + a, lo[a]); sgx_atomic_max(lds_b + 6 + a, hi[a]); }
        }
        SGX_THREADS_END
        SGX_SYNC();
    }
    SGX_THREADS_BEGIN(t)
    if (t == 0 && lds_b[0]) {
        sgx_atomic_add(&A.bounds->n_known, lds_b[0]); sgx_atomic_add(&A.bounds->n_occupied, lds_b[1]); sgx_atomic_add(&A.bounds->n_free, lds_b[2]);
        for (int a = 0; a < 3; a++) { sgx_atomic_min_i32(&A.bounds->key_min[a], lds_b[3 + a]); sgx_atomic_max(&A.bounds->key_max[a], lds_b[6 + a]); }
    }
    SGX_THREADS_END
}

// a cell of the list: of the wanted kind and inside the z window (publishAll :560-570: z + half > occupancy_min_z && z - half < occupancy_max_z)
SGX_DEV bool octo_cell_passes(const SgxOctoArgs &A, uint32_t bits, int kz, int want_occupied)
{
    if (bits == SGX_OCTO_UNKNOWN) return false;
    if ((octo_bits_f(bits) >= 0.0f) != (want_occupied != 0)) return false;
    const double z = octo_coord(A.res, kz), half = A.res / 2.0;
    return z + half > A.zmin && z - half < A.zmax;
}

SGX_KERNEL(256) k_octo_morton(SgxOctoArgs A)
{
    SGX_THREADS_BEGIN(t)
    const int b = (int)blockIdx.x * 256 + t;
    if (b < A.st[OCTO_COUNT]) A.morton[b] = octo_morton(A.brick_key[b]);
    SGX_THREADS_END
}
// the rank of a brick among the Morton codes (the codes are distinct); order[rank] = brick, cnt[rank] = its cells in the list
SGX_KERNEL(64) k_octo_rank(SgxOctoArgs A)
{
    SGX_LDS int lds_n[64];
    const int nb = A.st[OCTO_COUNT];
    for (int j = (int)blockIdx.x; j < nb; j += (int)gridDim.x) {
        SGX_THREADS_BEGIN(t)
        const unsigned long long mine = A.morton[j];
        int less = 0;
        for (int o = t; o < nb; o += 64) less += A.morton[o] < mine ? 1 : 0;
        int k0[3]; octo_brick_origin(A.brick_key[j], k0);
        int n = 0;
        for (int c = 0; c < 8; c++) { const int m = 8 * t + c; n += octo_cell_passes(A, A.cells[512 * (size_t)j + m], k0[2] + octo_squeeze3(m >> 2), A.want_occupied) ? 1 : 0; }
        lds_n[t] = less | (n << 20);
        SGX_THREADS_END
        SGX_SYNC();
        SGX_THREADS_BEGIN(t)
        if (t == 0) {
            int less = 0, n = 0;
            for (int o = 0; o < 64; o++) { less += lds_n[o] & 0xFFFFF; n += lds_n[o] >> 20; }
            A.order[less] = j; A.cnt[less] = n;
        }
        SGX_THREADS_END
        SGX_SYNC();
    }
}
// exclusive prefix of cnt in rank order by one workgroup; the total goes to n_out
SGX_KERNEL(256) k_octo_scan(SgxOctoArgs A)
{
    SGX_LDS int lds_s[256];
    const int nb = A.st[OCTO_COUNT], per = (nb + 255) / 256;
    SGX_THREADS_BEGIN(t)
    int s = 0;
    for (int o = t * per; o < nb && o < (t + 1) * per; o++) s += A.cnt[o];
    lds_s[t] = s;
    SGX_THREADS_END
    SGX_SYNC();
    SGX_THREADS_BEGIN(t)
    if (t == 0) { int run = 0; for (int o = 0; o < 256; o++) { const int v = lds_s[o]; lds_s[o] = run; run += v; } A.n_out[0] = run; }
    SGX_THREADS_END
    SGX_SYNC();
    SGX_THREADS_BEGIN(t)
    int run = lds_s[t];
    for (int o = t * per; o < nb && o < (t + 1) * per; o++) { const int v = A.cnt[o]; A.cnt[o] = run; run += v; }
    SGX_THREADS_END
}
SGX_KERNEL(64) k_octo_cells(SgxOctoArgs A)
{
    SGX_LDS int lds_c[64];
    const int nb = A.st[OCTO_COUNT];
    for (int j = (int)blockIdx.x; j < nb; j += (int)gridDim.x) {
        const int b = A.order[j];
        SGX_THREADS_BEGIN(t)
        int k0[3]; octo_brick_origin(A.brick_key[b], k0);
        int n = 0;
        for (int c = 0; c < 8; c++) { const int m = 8 * t + c; n += octo_cell_passes(A, A.cells[512 * (size_t)b + m], k0[2] + octo_squeeze3(m >> 2), A.want_occupied) ? 1 : 0; }
        lds_c[t] = n;
        SGX_THREADS_END
        SGX_SYNC();
        SGX_THREADS_BEGIN(t)
        int k0[3]; octo_brick_origin(A.brick_key[b], k0);
        int at = A.cnt[j];
        for (int o = 0; o < t; o++) at += lds_c[o];
        for (int c = 0; c < 8; c++) {
            const int m = 8 * t + c;
            const uint32_t bits = A.cells[512 * (size_t)b + m];
            const int k[3] = { k0[0] + octo_squeeze3(m), k0[1] + octo_squeeze3(m >> 1), k0[2] + octo_squeeze3(m >> 2) };
            if (!octo_cell_passes(A, bits, k[2], A.want_occupied)) continue;
            if (at < A.cap) {
                SgxOctoCell e; e.reserved = 0; e.logodds = octo_bits_f(bits);
                for (int a = 0; a < 3; a++) e.key[a] = (uint16_t)k[a];
                e.x = (float)octo_coord(A.res, k[0]); e.y = (float)octo_coord(A.res, k[1]); e.z = (float)octo_coord(A.res, k[2]);
                A.out[at] = e;
            }
            at++;
        }
        SGX_THREADS_END
        SGX_SYNC();
    }
}

// OcTree::search at depth 16 for keys (3 x uint16) or points (3 floats): the log-odds, a quiet NaN for unknown or for a point outside the key range
SGX_KERNEL(256) k_octo_search(SgxOctoArgs A)
{
    SGX_THREADS_BEGIN(t)
    const int i = (int)blockIdx.x * 256 + t;
    if (i < A.m) {
        int k[3]; bool ok = true;
        if (A.qkeys) for (int a = 0; a < 3; a++) k[a] = A.qkeys[3 * (size_t)i + a];
        else for (int a = 0; a < 3; a++) ok = octo_key1(A.rf, A.qpts[3 * (size_t)i + a], &k[a]) && ok;
        uint32_t bits = SGX_OCTO_UNKNOWN;
        if (ok) {
            const int s = octo_find(A, octo_brick(k[0], k[1], k[2]));
            const int idx = s >= 0 ? A.tab_idx[s] : -1;
            if (idx >= 0 && idx < A.st[OCTO_COUNT]) bits = A.cells[512 * (size_t)idx + octo_local(k[0], k[1], k[2])];
        }
        A.qout[i] = octo_bits_f(bits == SGX_OCTO_UNKNOWN ? SGX_OCTO_QNAN : bits);
    }
    SGX_THREADS_END
}

// update2DMap with m_projectCompleteMap: one lane per grid cell walks its column of bricks; 100 when a passing occupied cell is in the column, 0 when only free ones
SGX_KERNEL(256) k_octo_project(SgxOctoArgs A)
{
    SGX_THREADS_BEGIN(t)
    const long long i = (long long)blockIdx.x * 256 + t;
    if (i < (long long)A.gw * A.gh) {
        const int kx = A.gx0 + (int)(i % A.gw), ky = A.gy0 + (int)(i / A.gw);
        int v = -1;
        const int nb = A.st[OCTO_COUNT];
        for (int bz = A.gz0 >> 3; bz <= (A.gz1 >> 3) && v != 100 && nb > 0; bz++) {
            const int s = octo_find(A, octo_brick(kx, ky, bz << 3));
            const int idx = s >= 0 ? A.tab_idx[s] : -1;
            if (idx < 0 || idx >= nb) continue;
            for (int lz = 0; lz < 8; lz++) {
                const int kz = (bz << 3) + lz;
                const uint32_t bits = A.cells[512 * (size_t)idx + octo_local(kx, ky, kz)];
                if (octo_cell_passes(A, bits, kz, 1)) v = 100;
                else if (v < 0 && octo_cell_passes(A, bits, kz, 0)) v = 0;
            }
        }
        A.grid[i] = (int8_t)v;
    }
    SGX_THREADS_END
}
