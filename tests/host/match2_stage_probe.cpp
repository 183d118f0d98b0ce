// match2_stage_probe.cpp — stand-alone host program: calls every host-pointer matcher entry once on heap buffers of exactly the documented sizes, so that
// AddressSanitizer / UBSan (tests/test_match2_stage_probe.py builds this file and the emulator units with them) see any upload or read-back that leaves the
// caller's buffer or the staging slot.  It checks sizes only: results are the business of the oracle tests.
#include "../../include/sgx.h"
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <math.h>
#include <vector>

// the staging slots are never freed, on purpose (sg_slam_amd/csrc/sgx_stage.h)
extern "C" const char *__asan_default_options() { return "detect_leaks=0"; }

static uint32_t g_seed = 12345;
static uint32_t rnd() { g_seed = g_seed * 1664525u + 1013904223u; return g_seed >> 8; }
static float uni(float a, float b) { return a + (b - a) * (float)(rnd() & 0xFFFF) / 65535.0f; }

static std::vector<void *> g_bufs;
template <class T> static T *buf(size_t n)                       // exactly n elements, random bytes
{
    T *p = (T *)malloc(n * sizeof(T) ? n * sizeof(T) : 1);
    for (size_t i = 0; i < n * sizeof(T); i++) ((uint8_t *)p)[i] = (uint8_t)rnd();
    g_bufs.push_back(p);
    return p;
}
static float *floats(size_t n, float a, float b) { float *p = buf<float>(n); for (size_t i = 0; i < n; i++) p[i] = uni(a, b); return p; }
static uint8_t *flags(size_t n) { uint8_t *p = buf<uint8_t>(n); for (size_t i = 0; i < n; i++) p[i] = rnd() & 1; return p; }
static sgx_keypoint *keypoints(int n, int nlevels)
{
    sgx_keypoint *k = buf<sgx_keypoint>((size_t)n);
    for (int i = 0; i < n; i++) { k[i].x = uni(20, 620); k[i].y = uni(20, 460); k[i].size = 31; k[i].angle = uni(0, 359); k[i].response = uni(1, 100); k[i].octave = (int)(rnd() % (unsigned)nlevels); k[i].class_id = -1; }
    return k;
}
static float *points(int n) { float *p = buf<float>((size_t)n * 3); for (int i = 0; i < n; i++) { p[3 * i] = uni(-2, 2); p[3 * i + 1] = uni(-1.5f, 1.5f); p[3 * i + 2] = uni(2, 8); } return p; }
static float *pose() { float *T = buf<float>(16); for (int i = 0; i < 16; i++) T[i] = i % 5 == 0 ? 1.0f : 0.0f; T[3] = uni(-0.1f, 0.1f); T[7] = uni(-0.1f, 0.1f); T[11] = uni(-0.1f, 0.1f); return T; }
static int32_t *nodes(int n) { int32_t *p = buf<int32_t>((size_t)n); for (int i = 0; i < n; i++) p[i] = (int32_t)(rnd() % 6) - 1; return p; }

#define RUN(call) do { const int rc_ = (call); if (rc_ != SGX_OK) { fprintf(stderr, "%s -> %d\n", #call, rc_); return 1; } } while (0)

int main()
{
    const int n1 = 37, n2 = 23, nm = 29, L = 8;
    sgx_camera cam = { 535.4f, 539.2f, 320.1f, 247.6f, 40.0f, 0.0f, 640.0f, 0.0f, 480.0f };
    float *sf = buf<float>(L), *sg = buf<float>(L), *is2 = buf<float>(L);
    for (int i = 0; i < L; i++) { sf[i] = powf(1.2f, (float)i); sg[i] = sf[i] * sf[i]; is2[i] = 1.0f / sg[i]; }
    const float lsf = logf(1.2f);
    const sgx_keypoint *k1 = keypoints(n1, L), *k2 = keypoints(n2, L);
    const uint8_t *d1 = buf<uint8_t>((size_t)n1 * 32), *d2 = buf<uint8_t>((size_t)n2 * 32), *md = buf<uint8_t>((size_t)nm * 32);
    const float *u1 = floats(n1, -1, 600), *u2 = floats(n2, -1, 600), *T1 = pose(), *T2 = pose();
    const float *xw = points(nm), *nr = floats((size_t)nm * 3, -1, 1), *mind = floats(nm, 0.1f, 1), *maxd = floats(nm, 10, 50);
    int32_t *cnt = buf<int32_t>(1);

    RUN(sgx_hamming_matrix(d1, n1, d2, n2, buf<uint16_t>((size_t)n1 * n2)));
    {
        const float *cc = floats(3, -0.1f, 0.1f), *F12 = floats(9, -1, 1);
        RUN(sgx_match_search_for_triangulation(n1, k1, d1, u1, flags(n1), nodes(n1), cc, n2, k2, d2, u2, flags(n2), nodes(n2), T2, F12, &cam, sf, sg, L, 0, 1, buf<int32_t>((size_t)n1 * 2), cnt));
    }
    RUN(sgx_match_search_by_bow(n1, k1, d1, flags(n1), nodes(n1), n2, k2, d2, nodes(n2), 0.7f, 1, buf<int32_t>(n2), cnt));
    RUN(sgx_match_search_by_bow_kf(n1, k1, d1, flags(n1), nodes(n1), n2, k2, d2, flags(n2), nodes(n2), 0.75f, 1, buf<int32_t>(n1), cnt));
    RUN(sgx_match_fuse_search(n1, k1, d1, u1, T1, nm, xw, nr, mind, maxd, md, flags(nm), &cam, sf, is2, L, lsf, 3.0f, buf<int32_t>(nm), buf<int32_t>(nm), cnt));
    RUN(sgx_match_project_keyframe(n1, k1, d1, flags(n1), T1, n2, k2, flags(n2), points(n2), floats(n2, 0.1f, 1), floats(n2, 10, 50), d2, &cam, sf, L, lsf, 10.0f, 100, 1, buf<int32_t>(n1), cnt));
    RUN(sgx_match_fuse_search_sim3(n1, k1, d1, T1, nm, xw, nr, mind, maxd, md, flags(nm), &cam, sf, L, lsf, 4.0f, buf<int32_t>(nm), buf<int32_t>(nm), cnt));
    RUN(sgx_match_project_sim3(n1, k1, d1, flags(n1), T1, nm, xw, nr, mind, maxd, md, flags(nm), &cam, sf, L, lsf, 10, buf<int32_t>(n1), cnt));
    {
        int32_t *m12 = buf<int32_t>(n1); for (int i = 0; i < n1; i++) m12[i] = i % 5 ? -1 : i % n2;
        const float R12[9] = { 1, 0, 0, 0, 1, 0, 0, 0, 1 }, t12[3] = { 0.01f, 0.0f, -0.02f };
        RUN(sgx_match_search_by_sim3(n1, k1, d1, T1, flags(n1), points(n1), floats(n1, 0.1f, 1), floats(n1, 10, 50), buf<uint8_t>((size_t)n1 * 32),
                                     n2, k2, d2, T2, flags(n2), points(n2), floats(n2, 0.1f, 1), floats(n2, 10, 50), buf<uint8_t>((size_t)n2 * 32),
                                     &cam, sf, L, lsf, 1.0f, R12, t12, 7.5f, m12, cnt));
    }
    RUN(sgx_match_search_for_initialization(n1, k1, d1, n2, k2, d2, floats((size_t)n1 * 2, 20, 600), 100, 0.9f, 1, &cam, buf<int32_t>(n1), cnt));
    {
        const int n = 31; int32_t *st = buf<int32_t>((size_t)n + 1), *rl = buf<int32_t>(n);
        st[0] = 0; for (int p = 0; p < n; p++) { st[p + 1] = st[p] + (int)(rnd() % 5); rl[p] = (int)(rnd() % L); }
        const int total = st[n];
        RUN(sgx_mappoint_update_normal_and_depth(n, points(n), st, floats((size_t)total * 3, -1, 1), floats((size_t)n * 3, -1, 1), rl, sf, L, floats((size_t)n * 3, -1, 1), floats(n, 0, 1), floats(n, 1, 9)));
        RUN(sgx_mappoint_distinctive_descriptors(n, st, buf<uint8_t>((size_t)total * 32), buf<int32_t>(n), buf<uint8_t>((size_t)n * 32)));
    }
    {
        const int np = 19; int32_t *pairs = buf<int32_t>((size_t)np * 2);
        for (int q = 0; q < np; q++) { pairs[2 * q] = (int)(rnd() % n1); pairs[2 * q + 1] = (int)(rnd() % n2); }
        RUN(sgx_triangulate_new_map_points(np, pairs, n1, k1, keypoints(n1, L), u1, floats(n1, -1, 8), T1, n2, k2, keypoints(n2, L), u2, floats(n2, -1, 8), T2, &cam, sf, sg, L,
                                           buf<uint8_t>(np), buf<float>((size_t)np * 3), cnt));
    }
    {
        int32_t *obs = buf<int32_t>(n2); for (int i = 0; i < n2; i++) obs[i] = (int32_t)(rnd() % 9);
        RUN(sgx_match_project_frame(n1, k1, d1, u1, T1, n2, k2, flags(n2), flags(n2), points(n2), obs, d2, T2, &cam, sf, L, 15.0f, 0, 1, buf<int32_t>(n1), cnt));
        int32_t *mobs = buf<int32_t>(nm); for (int i = 0; i < nm; i++) mobs[i] = (int32_t)(rnd() % 9);
        RUN(sgx_match_project_local(n1, k1, d1, u1, T1, nullptr, nm, xw, nr, mind, maxd, md, mobs, flags(nm), &cam, sf, L, lsf, 3.0f, 0.8f, 0.5f, buf<int32_t>(n1), cnt, buf<uint8_t>(nm)));
    }
    {
        const int n = 17; double *S12 = buf<double>(8); const double s0[8] = { 0, 0, 0, 1, 0.01, 0, 0, 1 }; memcpy(S12, s0, sizeof s0);
        const float K[4] = { cam.fx, cam.fy, cam.cx, cam.cy };
        float *p = points(n), *o = buf<float>((size_t)n * 2);
        for (int i = 0; i < n; i++) { o[2 * i] = cam.fx * p[3 * i] / p[3 * i + 2] + cam.cx; o[2 * i + 1] = cam.fy * p[3 * i + 1] / p[3 * i + 2] + cam.cy; }
        RUN(sgx_optimize_sim3(n, p, p, o, o, floats(n, 0.2f, 1), floats(n, 0.2f, 1), K, K, S12, 10.0f, 0, buf<uint8_t>(n), buf<int32_t>(2), cnt));
    }
    {
        float *T = buf<float>(16); memcpy(T, T1, 64);
        RUN(sgx_pose_optimization(n1, k1, u1, flags(n1), points(n1), is2, L, &cam, T, buf<uint8_t>(n1), cnt));
    }
    for (void *p : g_bufs) free(p);
    printf("match2_stage_probe: 17 entries ok\n");
    return 0;
}
