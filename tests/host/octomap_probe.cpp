// octomap_probe.cpp — stand-alone host program: the sgx_octomap_* entries over zero points, scans whose points are all filtered, keys at 0 and 65535, a full brick
// table, and reset and reuse.  tests/test_octomap_probe.py builds this file and the emulator unit with AddressSanitizer / UBSan.  Every buffer is a heap allocation of
// exactly the size the entry is documented to use and the emulator's device memory is the heap too, so a mask word, a brick or a list entry read or written outside
// its array ends the program.
#include "../../include/sgx.h"
#include "../../sg_slam_amd/csrc/sgx_rt.h"
#include <float.h>
#include <math.h>
#include <stdio.h>
#include <string.h>
#include <vector>

thread_local sgx_dim3 blockIdx, blockDim, gridDim;          // the emulator's launch state (the extractor's unit holds it in the full library)

static int g_bad = 0;
#define EXPECT(cond) do { if (!(cond)) { fprintf(stderr, "octomap_probe: line %d: %s\n", __LINE__, #cond); g_bad++; } } while (0)

static sgx_octomap_params defaults(double res)
{
    sgx_octomap_params p; memset(&p, 0, sizeof p);
    p.res = res; p.prob_hit = 0.7; p.prob_miss = 0.4; p.thres_min = 0.12; p.thres_max = 0.97; p.max_range = -1.0;
    p.pointcloud_min_x = p.pointcloud_min_y = p.pointcloud_min_z = p.occupancy_min_z = -DBL_MAX;
    p.pointcloud_max_x = p.pointcloud_max_y = p.pointcloud_max_z = p.occupancy_max_z = DBL_MAX;
    return p;
}

static void pose(float m[16], float x, float y, float z) { memset(m, 0, 64); m[0] = m[5] = m[10] = m[15] = 1.f; m[3] = x; m[7] = y; m[11] = z; }

static sgx_octomap_record insert(sgx_octomap *h, const std::vector<sgx_cloud_point> &pts, const float m[16])
{
    sgx_octomap_record r; memset(&r, 0xff, sizeof r);
    std::vector<sgx_cloud_point> exact(pts);                                                  // exactly n records
    EXPECT(sgx_octomap_insert(h, exact.empty() ? NULL : exact.data(), (int)exact.size(), m, &r) == SGX_OK);
    return r;
}

// every query into buffers of exactly the sizes the counts name
static sgx_octomap_bounds_t queries(sgx_octomap *h)
{
    sgx_octomap_bounds_t b; EXPECT(sgx_octomap_bounds(h, &b) == SGX_OK);
    EXPECT(b.n_known == b.n_occupied + b.n_free);
    for (int occ = 0; occ < 2; occ++) {
        const int want = occ ? b.n_occupied : b.n_free;
        std::vector<sgx_octomap_cell> cells((size_t)want); int32_t n = -1;
        EXPECT(sgx_octomap_cells(h, occ, want ? cells.data() : NULL, want, &n) == SGX_OK && n == want);
        if (want > 1) { std::vector<sgx_octomap_cell> few((size_t)want - 1); EXPECT(sgx_octomap_cells(h, occ, few.data(), want - 1, &n) == SGX_ERR_OVERFLOW && n == want); }
    }
    sgx_octomap_grid_header_t hd; EXPECT(sgx_octomap_grid_header(h, &b, &hd) == SGX_OK);
    const size_t cells = (size_t)hd.width * (size_t)hd.height;
    std::vector<int8_t> grid(cells); sgx_octomap_grid_header_t hd2;
    EXPECT(sgx_octomap_project(h, &hd2, cells ? grid.data() : NULL, (int64_t)cells) == SGX_OK && hd2.width == hd.width && hd2.height == hd.height);
    if (b.n_known == 0) EXPECT(hd.flags == SGX_OCTOMAP_GRID_EMPTY && cells == 0);
    const uint16_t keys[12] = { 0, 0, 0, 65535, 65535, 65535, 32768, 32768, 32768, 1, 65534, 7 }; float out[4];
    EXPECT(sgx_octomap_search_dev(h, keys, NULL, 4, out, NULL) == SGX_OK);
    const float pts[6] = { 1e30f, 0.f, 0.f, 0.05f, 0.05f, 0.05f };
    EXPECT(sgx_octomap_search_dev(h, NULL, pts, 2, out, NULL) == SGX_OK && out[0] != out[0]);
    return b;
}

int main()
{
    sgx_octomap *h = NULL;
    sgx_octomap_params p = defaults(0.1);
    EXPECT(sgx_octomap_create(&p, 4, 8, &h) == SGX_OK && h);
    float m[16]; pose(m, 0.05f, 0.05f, 0.05f);
    // the empty map, zero points
    queries(h);
    sgx_octomap_record r = insert(h, {}, m);
    EXPECT(r.n_in == 0 && r.flags == 0 && r.n_new_cells == 0 && r.bbx_min[0] == 32768 && r.bbx_max[2] == 32768);
    EXPECT(queries(h).n_known == 0);
    // every point filtered: NaN, inf
    r = insert(h, { { NAN, 0, 0, 0 }, { 0, INFINITY, 0, 0 }, { 0, 0, -INFINITY, 0 } }, m);
    EXPECT(r.n_in == 3 && r.n_passed == 0 && r.n_new_cells == 0);
    EXPECT(queries(h).n_known == 0);
    // too many points: the buffer holds exactly max_points_per_scan + 1
    r = insert(h, std::vector<sgx_cloud_point>(9, sgx_cloud_point{ 0.3f, 0, 0, 0 }), m);
    EXPECT(r.flags == SGX_OCTOMAP_TOO_MANY_POINTS && r.n_in == 9 && queries(h).n_known == 0);
    // one brick, then a scan that needs more than four: refused, the map as before, then room again
    r = insert(h, { { 0.3f, 0, 0, 0 } }, m);
    EXPECT(r.flags == 0 && r.n_occupied_updates == 1 && r.n_free_updates == 3);
    const sgx_octomap_bounds_t before = queries(h);
    EXPECT(before.n_known == 4 && before.n_bricks == 1);
    r = insert(h, { { 3.f, 0, 0, 0 }, { 0, 3.f, 0, 0 }, { 0, 0, 3.f, 0 }, { -3.f, 0, 0, 0 } }, m);
    EXPECT(r.flags == SGX_OCTOMAP_MAP_FULL && r.n_free_updates == 0 && r.n_new_cells == 0);
    sgx_octomap_bounds_t after = queries(h);
    EXPECT(memcmp(&before, &after, sizeof after) == 0);
    r = insert(h, { { 0, 0.3f, 0, 0 } }, m);
    EXPECT(r.flags == 0 && queries(h).n_known == 7);
    // more distinct bricks than the table's 64 slots: the 26 directions of a cube, 6 m each (at least six bricks of its own a ray); refused, the map as before
    {
        sgx_octomap *g = NULL; EXPECT(sgx_octomap_create(&p, 4, 32, &g) == SGX_OK && g);
        EXPECT(insert(g, { { 0.3f, 0, 0, 0 } }, m).flags == 0);
        const sgx_octomap_bounds_t b0 = queries(g);
        std::vector<sgx_cloud_point> cube;
        for (int x = -1; x <= 1; x++) for (int y = -1; y <= 1; y++) for (int z = -1; z <= 1; z++) if (x || y || z) cube.push_back(sgx_cloud_point{ 6.f * (float)x, 6.f * (float)y, 6.f * (float)z, 0 });
        r = insert(g, cube, m);
        EXPECT(r.flags == SGX_OCTOMAP_MAP_FULL && r.n_passed == 26 && r.n_free_updates == 0 && r.n_new_cells == 0);
        const sgx_octomap_bounds_t b1 = queries(g);
        EXPECT(memcmp(&b0, &b1, sizeof b1) == 0);
        r = insert(g, { { 0, 0.3f, 0, 0 } }, m);
        EXPECT(r.flags == 0 && queries(g).n_known == 7);
        sgx_octomap_destroy(g);
    }
    // reset and reuse
    EXPECT(sgx_octomap_reset(h) == SGX_OK && queries(h).n_known == 0);
    r = insert(h, { { 0.3f, 0, 0, 0 } }, m);
    EXPECT(r.flags == 0 && queries(h).n_known == 4);
    sgx_octomap_destroy(h);
    // keys at 0 and 65535: the corners of the key range, the grid header whose padded corner has no key
    EXPECT(sgx_octomap_create(&p, 16, 8, &h) == SGX_OK && h);
    pose(m, 3276.55f, 3276.55f, 3276.55f);
    r = insert(h, { { 0.2f, 0.2f, 0.2f, 0 }, { 0.2f, 0, 0, 0 }, { 0.4f, 0, 0, 0 } }, m);
    EXPECT(r.flags == 0 && r.bbx_max[0] == 65535 && r.bbx_max[1] == 65535 && r.n_bad_end_key == 1 && r.n_invalid_rays == 1);
    sgx_octomap_bounds_t b = queries(h);
    EXPECT(b.key_max[0] == 65535 && b.key_max[2] == 65535);
    sgx_octomap_grid_header_t hd; EXPECT(sgx_octomap_grid_header(h, &b, &hd) == SGX_OK && hd.flags == SGX_OCTOMAP_GRID_KEY_OUT_OF_RANGE && hd.width == 0);
    EXPECT(sgx_octomap_reset(h) == SGX_OK);
    pose(m, -3276.55f, -3276.55f, -3276.55f);
    r = insert(h, { { -0.2f, -0.2f, -0.2f, 0 }, { -0.2f, 0, 0, 0 }, { -0.4f, 0, 0, 0 } }, m);
    EXPECT(r.flags == 0 && r.bbx_min[0] == 0 && r.bbx_min[2] == 0 && r.n_bad_end_key == 1);
    b = queries(h);
    EXPECT(b.key_min[0] == 0 && b.key_min[1] == 0 && b.key_min[2] == 0);
    EXPECT(sgx_octomap_grid_header(h, &b, &hd) == SGX_OK && hd.flags == SGX_OCTOMAP_GRID_KEY_OUT_OF_RANGE && hd.width == 0);      // (float)-3276.8 lies below the key range
    // an origin without a key: end cells only
    EXPECT(sgx_octomap_reset(h) == SGX_OK);
    pose(m, 5000.f, 0.f, 0.f);
    r = insert(h, { { -4999.5f, 0.3f, 0.2f, 0 } }, m);
    EXPECT(r.flags == SGX_OCTOMAP_ORIGIN_OUT_OF_RANGE && r.n_invalid_rays == 1 && r.n_occupied_updates == 1 && r.n_free_updates == 0);
    queries(h);
    sgx_octomap_destroy(h);
    // a batch from "device" memory with strides: three scans, counts 40 bytes apart as in sgx_cloud_result
    EXPECT(sgx_octomap_create(&p, 64, 4, &h) == SGX_OK && h);
    {
        std::vector<sgx_cloud_point> pts(3 * 4, sgx_cloud_point{ 0.5f, 0.1f, 0.2f, 0 });
        std::vector<int32_t> counts(2 * 10 + 1, -7); counts[0] = 4; counts[10] = 0; counts[20] = 2;
        std::vector<float> mats(48); for (int i = 0; i < 3; i++) pose(mats.data() + 16 * i, 0.05f + 0.3f * (float)i, 0.05f, 0.05f);
        std::vector<sgx_octomap_record> recs(3);
        EXPECT(sgx_octomap_insert_batch_dev(h, pts.data(), 4, counts.data(), 40, mats.data(), 3, recs.data(), NULL) == SGX_OK);
        EXPECT(recs[0].n_in == 4 && recs[1].n_in == 0 && recs[2].n_in == 2 && recs[2].n_occupied_updates == 1);
        queries(h);
    }
    sgx_octomap_destroy(h);
    sgx_octomap_destroy(NULL);
    if (g_bad) { fprintf(stderr, "octomap_probe: %d failed\n", g_bad); return 1; }
    printf("octomap_probe: ok\n");
    return 0;
}
