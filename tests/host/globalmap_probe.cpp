// globalmap_probe.cpp — stand-alone host program: the sgx_globalmap_* entries over a refused create, a map that is full, strided batches, a read buffer smaller than
// the map, a reset between sequences and destroy after a failed call.  tests/test_globalmap_probe.py builds this file and the emulator unit with AddressSanitizer /
// UBSan.  Every buffer is a heap allocation of exactly the size the entry is documented to use and the emulator's device memory is the heap too, so a point, a count or
// a workspace entry read or written outside its array ends the program.  Every refused call must leave the map as it was: it is read back after each.
#include "../../include/sgx.h"
#include "../../include/sgx_debug.h"
#include "../../sg_slam_amd/csrc/sgx_rt.h"
#include <math.h>
#include <stdio.h>
#include <string.h>
#include <vector>

thread_local sgx_dim3 blockIdx, blockDim, gridDim;          // the emulator's launch state (the extractor's unit holds it in the full library)

static int g_bad = 0;
#define EXPECT(cond) do { if (!(cond)) { fprintf(stderr, "globalmap_probe: line %d: %s\n", __LINE__, #cond); g_bad++; } } while (0)

static const int CAP = 64;

// n points on a 0.1 m lattice in the plane x = 1, from lattice position `first` on (8 a row), the last `far` of them 3 m away
static std::vector<sgx_cloud_point> cloud(int n, int first, int far = 0)
{
    std::vector<sgx_cloud_point> p((size_t)n);
    for (int i = 0; i < n; i++) {
        const int k = first + i;
        p[(size_t)i].x = 1.05f; p[(size_t)i].y = 0.05f + 0.1f * (float)(k % 8); p[(size_t)i].z = 0.05f + 0.1f * (float)(k / 8); p[(size_t)i].rgba = 0xff000000u | (uint32_t)k;
        if (i >= n - far) p[(size_t)i].x = 4.05f;
    }
    return p;
}

static std::vector<sgx_cloud_point> read_all(sgx_globalmap *h)
{
    int32_t n = -1;
    EXPECT(sgx_globalmap_size(h, &n) == SGX_OK && n >= 0 && n <= CAP);
    std::vector<sgx_cloud_point> p((size_t)(n > 0 ? n : 0)); int32_t m = -1;
    EXPECT(sgx_globalmap_read(h, p.data(), (int)p.size(), &m) == SGX_OK && m == n);
    return p;
}

static bool same(const std::vector<sgx_cloud_point> &a, const std::vector<sgx_cloud_point> &b)
{
    return a.size() == b.size() && (a.empty() || memcmp(a.data(), b.data(), a.size() * sizeof(sgx_cloud_point)) == 0);
}

int main()
{
    sgx_globalmap_params p; memset(&p, 0, sizeof p);
    p.sor_stddev_mul = 1.0; p.sor_mean_k = 3; p.voxel_leaf_size = 0.1f;
    sgx_globalmap *h = (sgx_globalmap *)(uintptr_t)0x10;
    // a refused create clears *out
    sgx_globalmap_params bad = p; bad.sor_mean_k = 0;
    EXPECT(sgx_globalmap_create(CAP, &bad, &h) == SGX_ERR_INVALID && h == NULL);
    bad = p; bad.voxel_leaf_size = 0; h = (sgx_globalmap *)(uintptr_t)0x10;
    EXPECT(sgx_globalmap_create(CAP, &bad, &h) == SGX_ERR_INVALID && h == NULL);
    bad = p; bad.voxel_leaf_size = NAN; h = (sgx_globalmap *)(uintptr_t)0x10;
    EXPECT(sgx_globalmap_create(CAP, &bad, &h) == SGX_ERR_INVALID && h == NULL);
    h = (sgx_globalmap *)(uintptr_t)0x10; EXPECT(sgx_globalmap_create(0, &p, &h) == SGX_ERR_INVALID && h == NULL);
    h = (sgx_globalmap *)(uintptr_t)0x10; EXPECT(sgx_globalmap_create(SGX_GMAP_MAX_POINTS + 1, &p, &h) == SGX_ERR_INVALID && h == NULL);
    EXPECT(sgx_globalmap_create(CAP, &p, NULL) == SGX_ERR_INVALID);
    sgx_globalmap_destroy(NULL);
    EXPECT(sgx_globalmap_create(CAP, &p, &h) == SGX_OK && h != NULL);
    if (!h) return 1;

    // the full map: 40 fit, 30 do not, 24 fill it, 1 does not
    sgx_globalmap_append_record r;
    std::vector<sgx_cloud_point> a = cloud(40, 0, 1), b = cloud(30, 40), c = cloud(24, 40), one = cloud(1, 70);
    EXPECT(sgx_globalmap_append(h, a.data(), 40, &r) == SGX_OK && r.n_in == 40 && r.offset == 0 && r.map_size == 40 && r.flags == 0);
    std::vector<sgx_cloud_point> before = read_all(h);
    EXPECT(same(before, a));
    EXPECT(sgx_globalmap_append(h, b.data(), 30, &r) == SGX_OK && r.n_in == 30 && r.offset == -1 && r.map_size == 40 && r.flags == SGX_GMAP_FULL);
    EXPECT(same(read_all(h), before));
    EXPECT(sgx_globalmap_append(h, c.data(), 24, &r) == SGX_OK && r.offset == 40 && r.map_size == CAP && r.flags == 0);
    EXPECT(sgx_globalmap_append(h, one.data(), 1, &r) == SGX_OK && r.flags == SGX_GMAP_FULL && r.map_size == CAP);
    EXPECT(sgx_globalmap_append(h, NULL, 0, &r) == SGX_OK && r.n_in == 0 && r.offset == CAP && r.flags == 0);                  // an empty cloud fits a full map
    std::vector<sgx_cloud_point> big = cloud(CAP + 1, 0);
    EXPECT(sgx_globalmap_append(h, big.data(), CAP + 1, &r) == SGX_OK && r.flags == SGX_GMAP_FULL);
    before = read_all(h);
    EXPECT((int)before.size() == CAP && memcmp(before.data() + 40, c.data(), 24 * sizeof(sgx_cloud_point)) == 0);
    // a read buffer smaller than the map: the first cap points, the true size, SGX_ERR_OVERFLOW
    { std::vector<sgx_cloud_point> few(10); int32_t n = -1;
      EXPECT(sgx_globalmap_read(h, few.data(), 10, &n) == SGX_ERR_OVERFLOW && n == CAP && memcmp(few.data(), before.data(), 10 * sizeof(sgx_cloud_point)) == 0);
      EXPECT(sgx_globalmap_read(h, NULL, 0, &n) == SGX_ERR_OVERFLOW && n == CAP); }
    // refused calls leave the map as it was
    EXPECT(sgx_globalmap_append(h, NULL, 3, &r) == SGX_ERR_INVALID && sgx_globalmap_append(h, a.data(), -1, &r) == SGX_ERR_INVALID && sgx_globalmap_append(h, a.data(), 3, NULL) == SGX_ERR_INVALID);
    EXPECT(sgx_globalmap_consolidate(h, NULL) == SGX_ERR_INVALID && sgx_globalmap_consolidate_dev(h, NULL, NULL) == SGX_ERR_INVALID);
    EXPECT(same(read_all(h), before));
    // the consolidation of the full map: 64 lattice points, one of them far away
    sgx_globalmap_result res;
    EXPECT(sgx_globalmap_consolidate(h, &res) == SGX_OK && res.n_points_in == CAP && res.n_voxels == CAP && res.flags == 0 && res.n_points == CAP - 1 && res.thr > res.mean);
    { std::vector<sgx_cloud_point> vox((size_t)res.n_voxels); std::vector<float> dist((size_t)res.n_voxels); std::vector<uint8_t> kept((size_t)res.n_voxels), tier((size_t)res.n_voxels); int n = -1;
      EXPECT(sgx_globalmap_debug_read(h, vox.data(), dist.data(), kept.data(), tier.data(), res.n_voxels, &n) == SGX_OK && n == res.n_voxels);
      int k = 0; for (uint8_t v : kept) k += v;
      EXPECT(k == res.n_points);
      EXPECT(sgx_globalmap_debug_read(h, vox.data(), dist.data(), kept.data(), tier.data(), res.n_voxels - 1, &n) == SGX_ERR_OVERFLOW && n == res.n_voxels);
      EXPECT(sgx_globalmap_debug_read(h, NULL, NULL, NULL, NULL, res.n_voxels, &n) == SGX_OK); }
    EXPECT((int)read_all(h).size() == CAP - 1);
    // a reset between sequences; a consolidation of an empty map and of <= mean_k voxel points is refused and changes nothing
    EXPECT(sgx_globalmap_reset(h) == SGX_OK && read_all(h).empty());
    EXPECT(sgx_globalmap_consolidate(h, &res) == SGX_OK && res.flags == SGX_GMAP_FEW_POINTS && res.n_points_in == 0 && res.n_points == 0 && res.n_voxels == 0);
    std::vector<sgx_cloud_point> three = cloud(3, 0);
    EXPECT(sgx_globalmap_append(h, three.data(), 3, &r) == SGX_OK && r.offset == 0 && r.map_size == 3);
    EXPECT(sgx_globalmap_consolidate(h, &res) == SGX_OK && res.flags == SGX_GMAP_FEW_POINTS && res.n_points == 3 && res.n_voxels == 3 && same(read_all(h), three));
    EXPECT(sgx_globalmap_reset(h) == SGX_OK);
    // strides: three clouds 11 points apart, their counts 12 bytes apart, the middle one too large; every array ends with its last element
    { const int stride = 11, n0 = 9, n1 = CAP, n2 = 5;
      std::vector<sgx_cloud_point> pts((size_t)(2 * stride + n2));                                   // cloud 1 claims CAP points but is refused before one is read
      std::vector<sgx_cloud_point> c0 = cloud(n0, 0), c2 = cloud(n2, 20);
      memcpy(pts.data(), c0.data(), n0 * sizeof(sgx_cloud_point)); memcpy(pts.data() + 2 * stride, c2.data(), n2 * sizeof(sgx_cloud_point));
      std::vector<int32_t> cnt(2 * 3 + 1, -7); cnt[0] = n0; cnt[3] = n1; cnt[6] = n2;
      std::vector<sgx_globalmap_append_record> rec(3);
      EXPECT(sgx_globalmap_append_batch_dev(h, pts.data(), stride, cnt.data(), 12, 3, rec.data(), NULL) == SGX_OK);
      EXPECT(rec[0].offset == 0 && rec[0].map_size == n0 && rec[1].flags == SGX_GMAP_FULL && rec[1].offset == -1 && rec[1].map_size == n0 && rec[2].offset == n0 && rec[2].map_size == n0 + n2);
      std::vector<sgx_cloud_point> got = read_all(h);
      EXPECT((int)got.size() == n0 + n2 && memcmp(got.data(), c0.data(), n0 * sizeof(sgx_cloud_point)) == 0 && memcmp(got.data() + n0, c2.data(), n2 * sizeof(sgx_cloud_point)) == 0);
      EXPECT(sgx_globalmap_append_batch_dev(h, pts.data(), -1, cnt.data(), 12, 3, rec.data(), NULL) == SGX_ERR_INVALID);
      EXPECT(sgx_globalmap_append_batch_dev(h, pts.data(), stride, cnt.data(), 10, 3, rec.data(), NULL) == SGX_ERR_INVALID);
      EXPECT(sgx_globalmap_append_batch_dev(h, pts.data(), stride, cnt.data(), 12, 0, rec.data(), NULL) == SGX_ERR_INVALID);
      EXPECT(sgx_globalmap_append_batch_dev(h, NULL, stride, cnt.data(), 12, 3, rec.data(), NULL) == SGX_ERR_INVALID);
      EXPECT(same(read_all(h), got));
      const sgx_cloud_point *pd = NULL; const int32_t *nd = NULL;
      EXPECT(sgx_globalmap_points_dev(h, &pd, &nd) == SGX_OK && pd && nd && *nd == n0 + n2 && memcmp(pd, got.data(), got.size() * sizeof(sgx_cloud_point)) == 0);
      sgx_globalmap_result rd;
      EXPECT(sgx_globalmap_consolidate_dev(h, &rd, NULL) == SGX_OK && rd.n_points_in == n0 + n2 && rd.flags == 0 && *nd == rd.n_points); }
    // destroy after a failed call
    EXPECT(sgx_globalmap_append(h, NULL, 5, &r) == SGX_ERR_INVALID);
    EXPECT(sgx_globalmap_debug_max_radius(h, SGX_GMAP_MAX_RADIUS + 1) == SGX_ERR_INVALID && sgx_globalmap_debug_max_radius(h, 0) == SGX_OK);
    sgx_globalmap_destroy(h);
    if (g_bad) { fprintf(stderr, "globalmap_probe: %d failed\n", g_bad); return 1; }
    printf("globalmap_probe: ok\n");
    return 0;
}
