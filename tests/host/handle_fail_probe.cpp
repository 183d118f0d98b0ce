// handle_fail_probe.cpp — stand-alone host program: walks the failure exits of the handles whose device buffers one owner holds (sg_slam_amd/csrc/sgx_devmem.h) with
// sgx_debug_devmem_fail_after, which makes the n-th allocation or upload copy of the calling thread fail.  tests/test_handle_fail_probe.py builds this file and the
// emulator units with AddressSanitizer / UBSan; in the emulator hipMalloc is calloc and device pointers are host pointers, so LeakSanitizer sees what a failed call
// leaves behind, and ASan a later call that reads a half-built handle or writes past a buffer that should have grown.  One line per sweep; the first violation ends the
// program.
#include "../../include/sgx.h"
#include "../../include/sgx_debug.h"
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <vector>

#define REQUIRE(cond, ...) do { if (!(cond)) { fprintf(stderr, "handle_fail_probe: %s:%d: ", __FILE__, __LINE__); fprintf(stderr, __VA_ARGS__); fprintf(stderr, "\n"); exit(1); } } while (0)
enum { MAX_STEPS = 200 };
static const float CAM[4] = { 535.4f, 539.2f, 320.1f, 247.6f };

// arms the injection, runs `call`, disarms: the call's status, which must be the status that was injected (a call the injection did not reach must succeed)
template <class F> static int injected(const char *what, int n, F call)
{
    sgx_debug_devmem_fail_after(n);
    const int rc = call();
    const int delivered = sgx_debug_devmem_fail_after(0);
    REQUIRE(rc == delivered, "%s n = %d: the call returned %d, the injected failure was %d", what, n, rc, delivered);
    REQUIRE(rc == SGX_OK || rc == SGX_ERR_NOMEM || rc == SGX_ERR_DEVICE, "%s n = %d: status %d", what, n, rc);
    return rc;
}

// create(&handle) under the n-th injected failure, n = 1, 2, ... until it succeeds: the handle is NULL exactly when the call failed
template <class H, class Create, class Destroy> static void sweep_create(const char *what, Create create, Destroy destroy)
{
    int nomem = 0, device = 0, n = 1;
    for (;; n++) {
        REQUIRE(n <= MAX_STEPS, "%s: still failing after %d steps", what, MAX_STEPS);
        H *h = (H *)&nomem;                        // anything but NULL: a failed create must clear it
        const int rc = injected(what, n, [&] { return create(&h); });
        REQUIRE((rc == SGX_OK) == (h != nullptr), "%s n = %d: status %d with handle %s", what, n, rc, h ? "set" : "NULL");
        if (rc == SGX_OK) { destroy(h); break; }
        (rc == SGX_ERR_NOMEM ? nomem : device)++;
    }
    REQUIRE(n > 1, "%s: the injection reached nothing", what);
    printf("%s: succeeds at n = %d (%d allocations refused with NOMEM, %d upload copies with DEVICE)\n", what, n, nomem, device);
}

// n points in front of a camera at the origin, their pixels, and their pixels from a camera moved by (0.3, 0.05, 0.02)
struct Scene {
    std::vector<float> X, px1, px2, ones;
    explicit Scene(int n) : X(3 * (size_t)n), px1(2 * (size_t)n), px2(2 * (size_t)n), ones((size_t)n, 1.0f)
    {
        for (int i = 0; i < n; i++) {
            const float x = (float)((i * 37) % 11 - 5) * 0.25f, y = (float)((i * 53) % 7 - 3) * 0.3f, z = 3.0f + (float)(i % 5) * 0.6f + (float)(i % 3) * 0.17f;
            X[3 * i] = x; X[3 * i + 1] = y; X[3 * i + 2] = z;
            px1[2 * i] = CAM[0] * x / z + CAM[2]; px1[2 * i + 1] = CAM[1] * y / z + CAM[3];
            px2[2 * i] = CAM[0] * (x + 0.3f) / (z + 0.02f) + CAM[2]; px2[2 * i + 1] = CAM[1] * (y + 0.05f) / (z + 0.02f) + CAM[3];
        }
    }
    std::vector<sgx_keypoint> keys(const std::vector<float> &px, int n) const
    {
        std::vector<sgx_keypoint> k((size_t)n);
        for (int i = 0; i < n; i++) { memset(&k[(size_t)i], 0, sizeof(sgx_keypoint)); k[(size_t)i].x = px[2 * (size_t)i]; k[(size_t)i].y = px[2 * (size_t)i + 1]; k[(size_t)i].class_id = -1; }
        return k;
    }
};

static void sweep_creates()
{
    const Scene sc(12);
    sweep_create<sgx_pnp_batch>("sgx_pnp_batch_create", [](sgx_pnp_batch **o) { return sgx_pnp_batch_create(2, 8, o); }, sgx_pnp_batch_destroy);
    sweep_create<sgx_pnp_solver>("sgx_pnp_solver_create",
                                 [&](sgx_pnp_solver **o) { return sgx_pnp_solver_create(8, sc.px1.data(), sc.ones.data(), sc.X.data(), CAM, 3u, o); }, sgx_pnp_solver_destroy);
    sweep_create<sgx_init_batch>("sgx_init_batch_create", [](sgx_init_batch **o) { return sgx_init_batch_create(1, 16, 16, 8, o); }, sgx_init_batch_destroy);
    const std::vector<sgx_keypoint> k1 = sc.keys(sc.px1, 12);
    sweep_create<sgx_initializer>("sgx_initializer_create", [&](sgx_initializer **o) { return sgx_initializer_create(12, k1.data(), CAM, 1.0f, 8, 5u, o); }, sgx_initializer_destroy);
    std::vector<float> X2(sc.X);
    for (int i = 0; i < 6; i++) { X2[3 * (size_t)i] += 0.3f; X2[3 * (size_t)i + 1] += 0.05f; X2[3 * (size_t)i + 2] += 0.02f; }
    const std::vector<float> err(6, 9.210f);
    sweep_create<sgx_sim3_solver>("sgx_sim3_solver_create",
                                  [&](sgx_sim3_solver **o) { return sgx_sim3_solver_create(6, sc.X.data(), X2.data(), err.data(), err.data(), CAM, CAM, 0, 1u, o); }, sgx_sim3_solver_destroy);
    sgx_obj3d_params p; memset(&p, 0, sizeof p);
    p.sor_stddev_mul = 1.0; p.sor_mean_k = 5; p.cluster_min_size = 10; p.cluster_max_size = 1000; p.voxel_leaf_size = 0.01f; p.cluster_tolerance = 0.05f;
    p.similar_compare_ratio = 0.5f; p.camera_valid_depth_min = 0.3f; p.camera_valid_depth_max = 5.0f;
    sweep_create<sgx_obj3d>("sgx_obj3d_create", [&](sgx_obj3d **o) { return sgx_obj3d_create(32, 24, 1, 2, 0, &p, o); }, sgx_obj3d_destroy);
    // a vocabulary of a root and two words (k = 2, L = 1, L1 scoring), and a keyframe database on it
    const int32_t parent[3] = { 0, 0, 0 }; const double weight[3] = { 0.0, 1.0, 1.0 }; const uint8_t leaf[3] = { 0, 1, 1 };
    uint8_t desc[3 * 32]; memset(desc, 0, sizeof desc); memset(desc + 64, 0xff, 32);
    const auto voc_create = [&](sgx_voc **o) { return sgx_voc_create(2, 1, 0, 0, 3, parent, desc, weight, leaf, o); };
    sweep_create<sgx_voc>("sgx_voc_create", voc_create, sgx_voc_destroy);
    sgx_voc *voc = nullptr;
    REQUIRE(voc_create(&voc) == SGX_OK && voc, "sgx_voc_create failed");
    sweep_create<sgx_kfdb>("sgx_kfdb_create", [&](sgx_kfdb **o) { return sgx_kfdb_create(voc, 4, 16, 8, 2, o); }, sgx_kfdb_destroy);
    sgx_voc_destroy(voc);
    sgx_orb_config cfg; memset(&cfg, 0, sizeof cfg);
    cfg.nfeatures = 100; cfg.scale_factor = 1.2f; cfg.nlevels = 1; cfg.ini_th_fast = 20; cfg.min_th_fast = 7; cfg.width = 64; cfg.height = 64; cfg.max_batch = 1;
    sweep_create<sgx_orb>("sgx_orb_create", [&](sgx_orb **o) { return sgx_orb_create(&cfg, o); }, sgx_orb_destroy);
}

// ---------------------------------------------------------------------------------------------------------------------------------------------------- Initializer regrow
struct InitOut { float R[9], t[3], p3d[36]; uint8_t tri[12], inl[12]; int32_t ok; sgx_init_report rep; };
static int initialize(sgx_initializer *s, const std::vector<sgx_keypoint> &k2, int n2, const int32_t *draws, InitOut *o)
{
    int32_t m12[12]; for (int i = 0; i < 12; i++) m12[i] = i;
    memset(o, 0, sizeof *o);
    return sgx_initializer_initialize(s, n2, k2.data(), m12, draws, o->R, o->t, o->p3d, o->tri, o->inl, &o->ok, &o->rep);
}

static void sweep_initializer_regrow()
{
    const Scene sc(40);
    const std::vector<sgx_keypoint> k1 = sc.keys(sc.px1, 12), k2 = sc.keys(sc.px2, 40);
    int32_t draws[64]; for (int i = 0; i < 64; i++) draws[i] = (int32_t)((1103515245u * (unsigned)(i + 1) + 12345u) >> 1);
    const auto create = [&] { sgx_initializer *s = nullptr; REQUIRE(sgx_initializer_create(12, k1.data(), CAM, 1.0f, 8, 5u, &s) == SGX_OK && s, "sgx_initializer_create failed"); return s; };
    // the undisturbed initializer: 12 keys, then 40 under its own replica; and what a 12-key call with caller draws returns
    InitOut first, want40, want12, got;
    sgx_initializer *ref = create();
    REQUIRE(initialize(ref, k2, 12, nullptr, &first) == SGX_OK && initialize(ref, k2, 40, nullptr, &want40) == SGX_OK, "Initialize failed");
    sgx_initializer_destroy(ref);
    ref = create();
    REQUIRE(initialize(ref, k2, 12, nullptr, &got) == SGX_OK && memcmp(&got, &first, sizeof got) == 0, "two initializers with one seed differ");
    REQUIRE(initialize(ref, k2, 12, draws, &want12) == SGX_OK, "Initialize with caller draws failed");
    sgx_initializer_destroy(ref);
    REQUIRE(first.rep.n_matches == 12 && want40.rep.n_matches == 12, "the scene's 12 matches were not all used");

    sgx_initializer *s = create();
    REQUIRE(initialize(s, k2, 12, nullptr, &got) == SGX_OK, "Initialize failed");
    int n = 1;
    for (;; n++) {
        REQUIRE(n <= MAX_STEPS, "Initialize regrow: still failing after %d steps", MAX_STEPS);
        const int rc = injected("Initialize regrow", n, [&] { return initialize(s, k2, 40, nullptr, &got); });
        if (rc == SGX_OK) break;
        InitOut again;                             // caller draws: the replica stays where it is
        REQUIRE(initialize(s, k2, 12, draws, &again) == SGX_OK, "Initialize regrow n = %d: the initializer is not usable at its old size", n);
        REQUIRE(memcmp(&again, &want12, sizeof again) == 0, "Initialize regrow n = %d: a 12-key call differs from an initializer that never failed", n);
    }
    REQUIRE(n > 1, "Initialize regrow: the injection reached nothing");
    REQUIRE(memcmp(&got, &want40, sizeof got) == 0, "Initialize regrow: the failed calls moved the replica");
    REQUIRE(initialize(s, k2, 40, nullptr, &got) == SGX_OK, "Initialize regrow: a second 40-key call failed");
    sgx_initializer_destroy(s);
    printf("Initialize regrow: %d failing calls; after each the 12-key call equals the undisturbed initializer's, and the 40-key call that succeeds drew from an unmoved replica\n", n - 1);
}

// ---------------------------------------------------------------------------------------------------------------------------------------------------- PnP
struct PnpOut { int32_t res[4]; float tcw[16]; uint8_t inl[8]; };

static void sweep_pnp_reserve()
{
    const Scene sc(8);
    const int32_t off[2] = { 0, 8 };
    const double ransac[6] = { 0.99, 6, 20, 4, 0.5, 5.991 };
    const uint32_t seed = 7;
    const auto create = [&] {
        sgx_pnp_batch *t = nullptr;
        REQUIRE(sgx_pnp_batch_create(2, 8, &t) == SGX_OK && t, "sgx_pnp_batch_create failed");
        PnpOut o;
        REQUIRE(sgx_pnp_batch_iterate_dev(t, 5, nullptr, 0, o.res, o.tcw, o.inl, nullptr) == SGX_ERR_INVALID, "iterate_dev accepts a batch that was never set");
        REQUIRE(sgx_pnp_batch_set_dev(t, 1, off, sc.px1.data(), sc.ones.data(), sc.X.data(), CAM, ransac, &seed, nullptr) == SGX_OK, "sgx_pnp_batch_set_dev failed");
        return t;
    };
    PnpOut want, got;
    memset(&want, 0, sizeof want);
    sgx_pnp_batch *ref = create();
    REQUIRE(sgx_pnp_batch_iterate_dev(ref, 5, nullptr, 0, want.res, want.tcw, want.inl, nullptr) == SGX_OK, "iterate_dev failed");
    sgx_pnp_batch_destroy(ref);
    REQUIRE(want.res[3] > 0, "iterate_dev ran no hypothesis");
    int n = 1;
    for (;; n++) {
        REQUIRE(n <= MAX_STEPS, "pnp_reserve: still failing after %d steps", MAX_STEPS);
        sgx_pnp_batch *t = create();
        memset(&got, 0, sizeof got);
        const int rc = injected("pnp_reserve", n, [&] { return sgx_pnp_batch_iterate_dev(t, 5, nullptr, 0, got.res, got.tcw, got.inl, nullptr); });
        if (rc != SGX_OK) {
            memset(&got, 0, sizeof got);
            REQUIRE(sgx_pnp_batch_iterate_dev(t, 5, nullptr, 0, got.res, got.tcw, got.inl, nullptr) == SGX_OK, "pnp_reserve n = %d: the retry failed", n);
        }
        REQUIRE(memcmp(&got, &want, sizeof got) == 0, "pnp_reserve n = %d: the result differs from a batch that never failed", n);
        sgx_pnp_batch_destroy(t);
        if (rc == SGX_OK) break;
    }
    REQUIRE(n > 1, "pnp_reserve: the injection reached nothing");
    printf("pnp_reserve: %d failing first iterate_dev calls, each retried and equal to the undisturbed batch\n", n - 1);
}

// caller draws of growing, then shrinking length: the solver's device copy grows when it must and is reused when it can
static void pnp_solver_caller_draws()
{
    const Scene sc(8);
    sgx_pnp_solver *s = nullptr;
    REQUIRE(sgx_pnp_solver_create(8, sc.px1.data(), sc.ones.data(), sc.X.data(), CAM, 3u, &s) == SGX_OK && s, "sgx_pnp_solver_create failed");
    int total = 0;
    for (const int n_it : { 2, 6, 3 }) {
        std::vector<int32_t> draws(4 * (size_t)n_it);          // exactly what the call may read: ASan sees a read past it
        for (size_t i = 0; i < draws.size(); i++) draws[i] = (int32_t)((1103515245u * (unsigned)(i + 1 + (size_t)total) + 12345u) >> 1);
        float tcw[16]; uint8_t inl[8]; int32_t no_more = 0, n_inl = 0, found = 0, run = 0;
        REQUIRE(sgx_pnp_solver_iterate(s, n_it, draws.data(), tcw, &no_more, inl, &n_inl, &found, &run) == SGX_OK, "sgx_pnp_solver_iterate(%d) failed", n_it);
        REQUIRE(run >= 1 && run <= n_it, "sgx_pnp_solver_iterate(%d) ran %d hypotheses", n_it, run);
        total += run;
    }
    sgx_pnp_solver_destroy(s);
    printf("sgx_pnp_solver_iterate: caller draws of 2, 6 and 3 hypotheses, %d run\n", total);
}

int main()
{
    setvbuf(stdout, nullptr, _IOLBF, 0);          // a sanitizer report ends the program without flushing
    sweep_creates();
    sweep_initializer_regrow();
    sweep_pnp_reserve();
    pnp_solver_caller_draws();
    printf("handle_fail_probe: ok\n");
    return 0;
}
