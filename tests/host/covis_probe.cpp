// covis_probe.cpp — stand-alone host program: the sgx_covis_* entries over ids out of range, capacities that are full, and keyframes erased while lists, rows and
// reference slots still name them.  tests/test_covis_probe.py builds this file and the emulator unit with AddressSanitizer / UBSan.  Every buffer is a heap allocation of
// exactly the size the entry is documented to use and the emulator's device memory is the heap too, so a chunk, a row or a workspace entry read or written outside its
// array ends the program.  Every refused call must leave the handle as it was: the observation count and the lists are read back after each.
#include "../../include/sgx.h"
#include "../../sg_slam_amd/csrc/sgx_rt.h"
#include <stdio.h>
#include <string.h>
#include <vector>

thread_local sgx_dim3 blockIdx, blockDim, gridDim;          // the emulator's launch state (the extractor's unit holds it in the full library)

static int g_bad = 0;
#define EXPECT(cond) do { if (!(cond)) { fprintf(stderr, "covis_probe: line %d: %s\n", __LINE__, #cond); g_bad++; } } while (0)

static const int NKF = 6, CAP = 32, NPTS = 40, NOBS = 120, NQ = 3;

static int live_obs(sgx_covis *h) { int32_t n = -1; EXPECT(sgx_covis_info(h, NULL, NULL, &n) == SGX_OK); return n; }

static int add_kf(sgx_covis *h, int id, int n)
{
    const size_t m = n > 0 ? (size_t)n : 1;
    std::vector<int32_t> o(m, 1); std::vector<float> u(m, -1.f), d(m, 2.f);
    for (int i = 0; i < n; i += 3) u[(size_t)i] = 4.f;
    return sgx_covis_add_keyframe(h, id, n, o.data(), u.data(), d.data());
}

static int observe(sgx_covis *h, int id, int first_idx, int first_pt, int n)
{
    std::vector<int32_t> i((size_t)n), p((size_t)n);
    for (int j = 0; j < n; j++) { i[(size_t)j] = first_idx + j; p[(size_t)j] = first_pt + j; }
    return sgx_covis_set_observations(h, id, n, i.data(), p.data());
}

// every query over the handle as it stands, into buffers of exactly the documented sizes
static void queries(sgx_covis *h, const std::vector<int32_t> &kf, const char *what)
{
    const int Q = (int)kf.size();
    std::vector<sgx_covis_report> rep((size_t)Q);
    EXPECT(sgx_covis_update_connections_batch_dev(h, Q, kf.data(), rep.data(), NULL) == SGX_OK);
    for (int mcap : { 0, 1, 7, NPTS }) {
        std::vector<int32_t> frame((size_t)Q * CAP, -1), n((size_t)Q), mo((size_t)Q, 2), lkf((size_t)Q * NKF, -1), nlkf((size_t)Q, 0), ref((size_t)Q, -1), rt((size_t)Q, -9), np((size_t)Q, -9);
        std::vector<int32_t> pts((size_t)Q * mcap + 1, -9), obs((size_t)Q * mcap + 1, -9);
        pts.resize((size_t)Q * mcap); obs.resize((size_t)Q * mcap);
        for (int q = 0; q < Q; q++) {
            n[(size_t)q] = q == 0 ? CAP : 5 * q;
            for (int i = 0; i < n[(size_t)q]; i++) frame[(size_t)q * CAP + i] = (i * 7 + q) % (NPTS + 1) - 1;          // -1 .. NPTS - 1, bad ids among them
            if (q == 1) { lkf[(size_t)q * NKF] = kf[0]; lkf[(size_t)q * NKF + 1] = 999; nlkf[(size_t)q] = 2; ref[(size_t)q] = 999; n[(size_t)q] = 0; }      // a kept row with an unknown id
        }
        EXPECT(sgx_covis_local_map_batch_dev(h, Q, CAP, frame.data(), n.data(), mo.data(), lkf.data(), nlkf.data(), ref.data(), rt.data(), mcap, pts.data(), obs.data(), np.data(),
                                             rep.data(), NULL) == SGX_OK);
        for (int q = 0; q < Q; q++) {
            EXPECT(rep[(size_t)q].status == SGX_OK || rep[(size_t)q].status == SGX_ERR_NOMEM);
            EXPECT((rep[(size_t)q].status == SGX_ERR_NOMEM) == (np[(size_t)q] > mcap));
            EXPECT(np[(size_t)q] >= 0 && np[(size_t)q] <= NPTS && nlkf[(size_t)q] >= 0 && nlkf[(size_t)q] <= NKF && rt[(size_t)q] >= 0);
            for (int i = 0; i < np[(size_t)q] && i < mcap; i++) EXPECT(pts[(size_t)q * mcap + i] >= 0 && pts[(size_t)q * mcap + i] < NPTS && obs[(size_t)q * mcap + i] >= 1);
        }
    }
    for (int max_cand : { 1, NKF }) {
        std::vector<int32_t> cand((size_t)Q * max_cand, -9), nc((size_t)Q, -9), red((size_t)Q * max_cand, -9), mps((size_t)Q * max_cand, -9), cull((size_t)Q * max_cand, -9);
        EXPECT(sgx_covis_keyframe_culling_batch_dev(h, Q, kf.data(), max_cand, cand.data(), nc.data(), red.data(), mps.data(), cull.data(), NULL) == SGX_OK);
        for (int q = 0; q < Q; q++) {
            EXPECT(nc[(size_t)q] >= -1 && nc[(size_t)q] < NKF);
            for (int r = 0; r < nc[(size_t)q] && r < max_cand; r++) EXPECT(red[(size_t)q * max_cand + r] >= 0 && mps[(size_t)q * max_cand + r] >= red[(size_t)q * max_cand + r] && (cull[(size_t)q * max_cand + r] | 1) == 1);
        }
    }
    std::vector<int32_t> a(NKF), b(NKF); int32_t n = 0, parent = 0, first = 0;
    for (int id : kf) {
        const int rc = sgx_covis_get_ordered(h, id, a.data(), b.data(), &n);
        EXPECT(rc == SGX_OK || rc == SGX_ERR_INVALID);
        if (rc == SGX_OK) { EXPECT(n >= 0 && n < NKF); EXPECT(sgx_covis_get_weights(h, id, a.data(), b.data(), &n) == SGX_OK); EXPECT(sgx_covis_get_tree(h, id, &parent, &first, a.data(), &n) == SGX_OK); }
    }
    if (g_bad) fprintf(stderr, "covis_probe: after \"%s\"\n", what);
}

int main()
{
    sgx_covis *h = NULL;
    EXPECT(sgx_covis_create(0, CAP, NPTS, NOBS, NQ, 0, 40.f, &h) == SGX_ERR_INVALID && !h);
    EXPECT(sgx_covis_create(4097, CAP, NPTS, NOBS, NQ, 0, 40.f, &h) == SGX_ERR_UNSUPPORTED && !h);
    EXPECT(sgx_covis_create(NKF, CAP, NPTS, NOBS, NQ, 0, 40.f, NULL) == SGX_ERR_INVALID);
    if (sgx_covis_create(NKF, CAP, NPTS, NOBS, NQ, 0, 40.f, &h) != SGX_OK) { fprintf(stderr, "create failed\n"); return 1; }
    queries(h, { 1, 2, 3 }, "an empty handle");
    // ids out of range, before and after there is anything to damage
    for (int round = 0; round < 2; round++) {
        const int before = live_obs(h);
        const int32_t i0[] = { 0, CAP }, p0[] = { 1, 2 }, ineg[] = { -1 }, pbig[] = { NPTS }, pneg[] = { -2 }, one[] = { 0 };
        EXPECT(add_kf(h, -1, 4) == SGX_ERR_INVALID && add_kf(h, 50, CAP + 1) == SGX_ERR_INVALID && add_kf(h, 50, -1) == SGX_ERR_INVALID);
        EXPECT(sgx_covis_set_observations(h, 77, 1, one, one) == SGX_ERR_INVALID);
        if (round) {
            EXPECT(sgx_covis_set_observations(h, 1, 2, i0, p0) == SGX_ERR_INVALID && sgx_covis_set_observations(h, 1, 1, ineg, one) == SGX_ERR_INVALID);
            EXPECT(sgx_covis_set_observations(h, 1, 1, one, pbig) == SGX_ERR_INVALID && sgx_covis_set_observations(h, 1, 1, one, pneg) == SGX_ERR_INVALID);
            EXPECT(sgx_covis_set_observations(h, 1, -1, one, one) == SGX_ERR_INVALID && sgx_covis_set_observations(h, 1, 1, NULL, one) == SGX_ERR_INVALID);
        }
        EXPECT(sgx_covis_set_points_bad(h, 1, pbig) == SGX_ERR_INVALID && sgx_covis_set_points_bad(h, 1, pneg) == SGX_ERR_INVALID && sgx_covis_set_points_bad(h, -1, one) == SGX_ERR_INVALID);
        EXPECT(sgx_covis_replace_point(h, 0, NPTS) == SGX_ERR_INVALID && sgx_covis_replace_point(h, -1, 0) == SGX_ERR_INVALID);
        EXPECT(sgx_covis_erase_keyframe(h, 77) == SGX_ERR_INVALID && sgx_covis_erase_keyframe(NULL, 1) == SGX_ERR_INVALID);
        EXPECT(live_obs(h) == before);
        if (!round) { EXPECT(add_kf(h, 1, CAP) == SGX_OK && add_kf(h, 2, CAP) == SGX_OK && observe(h, 1, 0, 0, 20) == SGX_OK && observe(h, 2, 0, 0, 20) == SGX_OK); EXPECT(live_obs(h) == 40); }
    }
    queries(h, { 1, 2, 77 }, "two keyframes and an unknown one");
    // full capacities: keyframes, then observations (the refused call is rolled back as a whole)
    for (int id = 3; id <= NKF; id++) EXPECT(add_kf(h, id, CAP) == SGX_OK);
    EXPECT(add_kf(h, 50, 4) == SGX_ERR_NOMEM && sgx_covis_size(h) == NKF);
    EXPECT(observe(h, 3, 0, 0, 32) == SGX_OK && observe(h, 4, 0, 8, 32) == SGX_OK && live_obs(h) == 104);
    EXPECT(observe(h, 5, 0, 0, 17) == SGX_ERR_NOMEM && live_obs(h) == 104);
    EXPECT(observe(h, 5, 0, 0, 16) == SGX_OK && live_obs(h) == NOBS && observe(h, 6, 0, 0, 1) == SGX_ERR_NOMEM);
    queries(h, { 5, 1, 3 }, "full");
    // batches that are too large or have no arrays
    { std::vector<int32_t> kf(NQ + 1, 1); std::vector<sgx_covis_report> rep(NQ + 1);
      EXPECT(sgx_covis_update_connections_batch_dev(h, NQ + 1, kf.data(), rep.data(), NULL) == SGX_ERR_INVALID && sgx_covis_update_connections_batch_dev(h, 1, NULL, rep.data(), NULL) == SGX_ERR_INVALID);
      EXPECT(sgx_covis_keyframe_culling_batch_dev(h, 1, kf.data(), 0, kf.data(), kf.data(), kf.data(), kf.data(), kf.data(), NULL) == SGX_ERR_INVALID); }
    // malformed frames: a count beyond the row, a negative one, an id out of range: that query's status, nothing of it written
    { std::vector<int32_t> frame((size_t)3 * 4, 1), n = { 5, -1, 2 }, mo(3, 0), lkf((size_t)3 * NKF, -1), nlkf(3, 0), ref(3, -1), rt(3, -9), np(3, -9), pts((size_t)3 * 4, -9), obs((size_t)3 * 4, -9);
      std::vector<sgx_covis_report> rep(3);
      frame[(size_t)2 * 4 + 1] = NPTS;
      EXPECT(sgx_covis_local_map_batch_dev(h, 3, 4, frame.data(), n.data(), mo.data(), lkf.data(), nlkf.data(), ref.data(), rt.data(), 4, pts.data(), obs.data(), np.data(), rep.data(), NULL) == SGX_OK);
      for (int q = 0; q < 3; q++) EXPECT(rep[(size_t)q].status == SGX_ERR_INVALID && np[(size_t)q] == -9 && rt[(size_t)q] == -9 && pts[(size_t)q * 4] == -9);
      nlkf[0] = NKF + 1; n = { 1, 1, 1 };
      EXPECT(sgx_covis_local_map_batch_dev(h, 3, 4, frame.data(), n.data(), mo.data(), lkf.data(), nlkf.data(), ref.data(), rt.data(), 4, pts.data(), obs.data(), np.data(), rep.data(), NULL) == SGX_OK);
      EXPECT(rep[0].status == SGX_ERR_INVALID && rep[1].status == SGX_ERR_NOMEM && np[1] > 4 && pts[4] >= 0 && pts[7] >= 0); }      // point 1 is seen by four keyframes of 16 points and more
    // erased while referenced: lists, rows and reference slots name the erased keyframes; slots come back and are taken again, over and over
    for (int round = 0; round < 40; round++) {
        const int fresh = 100 + round;
        std::vector<int32_t> ids;
        for (int id = 1; id < fresh; id++) if (sgx_covis_get_tree(h, id, NULL, NULL, NULL, NULL) == SGX_OK) ids.push_back(id);
        if (ids.empty()) { EXPECT(!"no keyframe left"); break; }
        const int gone = ids[(size_t)round % ids.size()];
        EXPECT(sgx_covis_erase_keyframe(h, gone) == SGX_OK);
        EXPECT(sgx_covis_erase_keyframe(h, gone) == SGX_ERR_INVALID);
        EXPECT(add_kf(h, gone, 4) == SGX_ERR_INVALID || sgx_covis_erase_keyframe(h, gone) == SGX_OK);          // held by a list: refused; otherwise it is a new keyframe
        queries(h, { gone, ids[0], ids.back() }, "after an erase");
        const int rc = add_kf(h, fresh, CAP);
        EXPECT(rc == SGX_OK || rc == SGX_ERR_NOMEM);
        if (rc == SGX_OK) {
            const int room = NOBS - live_obs(h), m = room < 24 ? room : 24;
            if (m > 0) EXPECT(observe(h, fresh, 0, (round * 5) % (NPTS - 24), m) == SGX_OK);
            queries(h, { fresh, ids.back(), gone }, "after a fresh keyframe");
        }
        if (round % 7 == 3) { const int32_t p[] = { 3, 4, 5, 3 }; EXPECT(sgx_covis_set_points_bad(h, 4, p) == SGX_OK); EXPECT(sgx_covis_replace_point(h, 6, 7) == SGX_OK); }
    }
    EXPECT(sgx_covis_clear(h) == SGX_OK && sgx_covis_size(h) == 0 && live_obs(h) == 0);
    queries(h, { 1, 2, 3 }, "cleared");
    sgx_covis_destroy(h);
    if (!g_bad) printf("covis_probe: ok\n");
    return g_bad ? 1 : 0;
}
