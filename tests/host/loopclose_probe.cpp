// loopclose_probe.cpp — stand-alone host program: sgx_covis_consistency_reserve / _clear / _info, sgx_covis_consistency*, sgx_covis_get_consistent_groups and
// sgx_covis_connected_batch*, sgx_covis_gba_update* and sgx_gba_correct_points_dev over capacities of 0 and one short of the need, candidate ids out of range and twice, counts out of range, a full group table and missing
// arrays.  tests/test_loopclose_probe.py builds this file and the emulator unit with AddressSanitizer / UBSan.  Every buffer is a heap allocation of exactly the size the
// entry is documented to use (max_keyframes, max_groups, max_groups + 1, cap, Q + 1) and the emulator's device memory is the heap too, so a row or a workspace entry
// read or written outside its array ends the program.
#include "../../include/sgx.h"
#include "../../sg_slam_amd/csrc/sgx_rt.h"
#include <stdio.h>
#include <string.h>
#include <vector>

thread_local sgx_dim3 blockIdx, blockDim, gridDim;          // the emulator's launch state (the extractor's unit holds it in the full library)

static int g_bad = 0;
#define EXPECT(cond) do { if (!(cond)) { fprintf(stderr, "loopclose_probe: line %d: %s\n", __LINE__, #cond); g_bad++; } } while (0)

static const int NKF = 70, CAP = 40, NPTS = 400, NOBS = 1000, NQ = 3, NG = 5;

static int add_kf(sgx_covis *h, int id)
{
    std::vector<int32_t> o((size_t)CAP, 1); std::vector<float> u((size_t)CAP, -1.f), d((size_t)CAP, 2.f);
    return sgx_covis_add_keyframe(h, id, CAP, o.data(), u.data(), d.data());
}

static int observe(sgx_covis *h, int id, int first_idx, int first_pt, int n)
{
    std::vector<int32_t> i((size_t)n), p((size_t)n);
    for (int j = 0; j < n; j++) { i[(size_t)j] = first_idx + j; p[(size_t)j] = first_pt + j; }
    return sgx_covis_set_observations(h, id, n, i.data(), p.data());
}

// one consistency call through the device-pointer entry: the candidate row has exactly n entries, the enough row max_keyframes; a refused call leaves both outputs alone
static sgx_covis_consistency_report consistency(sgx_covis *h, const std::vector<int32_t> &cand, int n_claimed, int th, std::vector<int32_t> *enough_out = nullptr)
{
    std::vector<int32_t> c(cand), n(1, n_claimed), enough((size_t)NKF, -9), ne(1, -9);
    sgx_covis_consistency_report R; memset(&R, 0x55, sizeof(R));
    EXPECT(sgx_covis_consistency_dev(h, c.data(), n.data(), th, enough.data(), ne.data(), &R, NULL) == SGX_OK);
    if (R.status != SGX_OK) { EXPECT(ne[0] == -9); for (int32_t e : enough) EXPECT(e == -9); EXPECT(R.n_after == R.n_before); }
    else {
        EXPECT(ne[0] == R.n_enough && R.n_enough >= 0 && R.n_enough <= n_claimed && R.n_cand == n_claimed && R.n_after <= NG);
        for (int j = 0; j < NKF; j++) EXPECT(j < ne[0] ? enough[(size_t)j] >= 0 : enough[(size_t)j] == -9);
        if (enough_out) enough_out->assign(enough.begin(), enough.begin() + ne[0]);
    }
    return R;
}

// the stored groups into rows of exactly the documented sizes
static int groups(sgx_covis *h, int cap, std::vector<int32_t> *counter, std::vector<int32_t> *off, std::vector<int32_t> *ids, int *rc_out = nullptr)
{
    int32_t n = -9;
    counter->assign(NG, -9); off->assign(NG + 1, -9); ids->assign((size_t)cap, -9);
    const int rc = sgx_covis_get_consistent_groups(h, &n, counter->data(), off->data(), cap, ids->data());
    if (rc_out) *rc_out = rc;
    EXPECT(rc == SGX_OK || rc == SGX_ERR_NOMEM);
    EXPECT(n >= 0 && n <= NG && (*off)[0] == 0);
    for (int g = 0; g < n; g++) EXPECT((*off)[(size_t)g + 1] > (*off)[(size_t)g] && (*counter)[(size_t)g] >= 0);
    return n;
}

int main()
{
    sgx_covis *h = nullptr;
    EXPECT(sgx_covis_create(NKF, CAP, NPTS, NOBS, NQ, 0, 40.f, &h) == SGX_OK && h);
    for (int k = 0; k < NKF; k++) EXPECT(add_kf(h, 100 + k) == SGX_OK);
    // 100 sees 101 (20 points), 102 (3) and 103 (1); 104 sees 103 (2)
    EXPECT(observe(h, 100, 0, 0, 24) == SGX_OK && observe(h, 101, 0, 0, 20) == SGX_OK && observe(h, 102, 0, 20, 3) == SGX_OK && observe(h, 103, 0, 23, 1) == SGX_OK);
    EXPECT(observe(h, 104, 0, 30, 2) == SGX_OK && observe(h, 103, 1, 30, 2) == SGX_OK);
    sgx_covis_report ur;
    EXPECT(sgx_covis_update_connections(h, 100, &ur) == SGX_OK && sgx_covis_update_connections(h, 104, &ur) == SGX_OK);

    // ---- the state before it exists, and the reservation
    int64_t bytes = -1; int32_t ng = -1, mg = -1;
    EXPECT(sgx_covis_consistency_info(h, &bytes, &ng, &mg) == SGX_OK && bytes == 0 && ng == 0 && mg == 0);
    EXPECT(sgx_covis_consistency_info(h, NULL, NULL, NULL) == SGX_OK && sgx_covis_consistency_info(NULL, &bytes, &ng, &mg) == SGX_ERR_INVALID);
    EXPECT(sgx_covis_consistency_clear(h) == SGX_OK && sgx_covis_consistency_clear(NULL) == SGX_ERR_INVALID);
    { int32_t n = -9, off1[1] = { -9 }; EXPECT(sgx_covis_get_consistent_groups(h, &n, NULL, off1, 0, NULL) == SGX_OK && n == 0 && off1[0] == 0); }
    EXPECT(sgx_covis_consistency_reserve(h, 0) == SGX_ERR_INVALID && sgx_covis_consistency_reserve(h, 4097) == SGX_ERR_UNSUPPORTED && sgx_covis_consistency_reserve(NULL, 4) == SGX_ERR_INVALID);
    EXPECT(sgx_covis_consistency_reserve(h, NG) == SGX_OK && sgx_covis_consistency_reserve(h, NG) == SGX_OK && sgx_covis_consistency_reserve(h, NG + 1) == SGX_ERR_INVALID);
    EXPECT(sgx_covis_consistency_info(h, &bytes, &ng, &mg) == SGX_OK && bytes == (int64_t)NG * (9 * NKF + 24) + 8 * NKF + 32 && ng == 0 && mg == NG);

    // ---- missing arrays: refused for the call
    { int32_t c[1] = { 100 }, n[1] = { 1 }, e[NKF], ne[1]; sgx_covis_consistency_report R;
      EXPECT(sgx_covis_consistency_dev(h, NULL, n, 3, e, ne, &R, NULL) == SGX_ERR_INVALID && sgx_covis_consistency_dev(h, c, NULL, 3, e, ne, &R, NULL) == SGX_ERR_INVALID);
      EXPECT(sgx_covis_consistency_dev(h, c, n, 3, NULL, ne, &R, NULL) == SGX_ERR_INVALID && sgx_covis_consistency_dev(h, c, n, 3, e, NULL, &R, NULL) == SGX_ERR_INVALID);
      EXPECT(sgx_covis_consistency_dev(h, c, n, 3, e, ne, NULL, NULL) == SGX_ERR_INVALID && sgx_covis_consistency_dev(NULL, c, n, 3, e, ne, &R, NULL) == SGX_ERR_INVALID);
      EXPECT(sgx_covis_consistency(h, -1, c, 3, e, ne, &R) == SGX_ERR_INVALID && sgx_covis_consistency(h, NKF + 1, c, 3, e, ne, &R) == SGX_ERR_INVALID);
      EXPECT(sgx_covis_consistency(h, 1, NULL, 3, e, ne, &R) == SGX_ERR_INVALID && sgx_covis_consistency(h, 1, c, 3, e, NULL, &R) == SGX_ERR_INVALID); }

    // ---- groups: {103}, then 100 and 104 both consistent with it; the rows at exactly their sizes and one short
    std::vector<int32_t> counter, off, ids, enough;
    sgx_covis_consistency_report R = consistency(h, { 103 }, 1, 1);
    EXPECT(R.status == SGX_OK && R.n_before == 0 && R.n_after == 1 && R.n_pushed_zero == 1);
    R = consistency(h, { 100, 104 }, 2, 1, &enough);
    EXPECT(R.status == SGX_OK && R.n_after == 1 && R.n_consistent == 2 && R.n_pushed_nothing == 1 && enough.size() == 2 && enough[0] == 100 && enough[1] == 104);
    EXPECT(groups(h, 4, &counter, &off, &ids) == 1 && counter[0] == 1 && off[1] == 4 && ids[0] == 100 && ids[1] == 101 && ids[2] == 102 && ids[3] == 103);
    { int rc = 0; groups(h, 3, &counter, &off, &ids, &rc); EXPECT(rc == SGX_ERR_NOMEM && off[1] == 4); for (int32_t x : ids) EXPECT(x == -9); }
    { int rc = 0; groups(h, 0, &counter, &off, &ids, &rc); EXPECT(rc == SGX_ERR_NOMEM); }
    // refused: unknown, negative, twice, counts out of range; the group stays
    EXPECT(consistency(h, { 100, 5 }, 2, 1).status == SGX_ERR_INVALID && consistency(h, { -1 }, 1, 1).status == SGX_ERR_INVALID && consistency(h, { 0x7fffffff }, 1, 1).status == SGX_ERR_INVALID);
    EXPECT(consistency(h, { 104, 100, 104 }, 3, 1).status == SGX_ERR_INVALID && consistency(h, { 100 }, -1, 1).status == SGX_ERR_INVALID && consistency(h, { 100 }, NKF + 1, 1).status == SGX_ERR_INVALID);
    EXPECT(groups(h, 4, &counter, &off, &ids) == 1 && counter[0] == 1);
    // max_groups at the need and one short; all max_keyframes candidates at once
    EXPECT(consistency(h, { 110, 111, 112, 113, 114, 115 }, 6, 3).status == SGX_ERR_NOMEM && groups(h, 4, &counter, &off, &ids) == 1);
    R = consistency(h, { 110, 111, 112, 113, 114 }, 5, 3);
    EXPECT(R.status == SGX_OK && R.n_after == NG && groups(h, NG, &counter, &off, &ids) == NG && off[NG] == NG);
    { std::vector<int32_t> all; for (int k = 0; k < NKF; k++) all.push_back(100 + k); EXPECT(consistency(h, all, NKF, 3).status == SGX_ERR_NOMEM); }
    // the host form, and no candidate
    { int32_t c[2] = { 110, 100 }, e[2] = { -9, -9 }, ne = -9;
      EXPECT(sgx_covis_consistency(h, 2, c, 1, e, &ne, &R) == SGX_OK && ne == 1 && e[0] == 110 && e[1] == -9 && R.n_after == 2);
      EXPECT(sgx_covis_consistency(h, 0, NULL, 3, NULL, &ne, NULL) == SGX_OK && ne == 0); }
    EXPECT(sgx_covis_consistency_info(h, &bytes, &ng, &mg) == SGX_OK && ng == 0 && mg == NG);
    EXPECT(consistency(h, { 103 }, 1, 3).n_after == 1 && sgx_covis_consistency_clear(h) == SGX_OK && groups(h, 0, &counter, &off, &ids) == 0);

    // ---- connected_batch: rows of exactly cap, Q + 1 offsets
    for (int cap : { 5, 4, 3, 0 }) {
        std::vector<int32_t> q = { 100, 999, 104 }, o(4, -9), row((size_t)cap, -9); std::vector<sgx_covis_report> rep(3);
        EXPECT(sgx_covis_connected_batch_dev(h, 3, q.data(), o.data(), cap ? row.data() : NULL, cap, rep.data(), NULL) == SGX_OK);
        EXPECT(o[0] == 0 && o[1] == 3 && o[2] == 3 && o[3] == 4 && rep[0].n_counter == 3 && rep[1].status == SGX_ERR_INVALID && rep[2].n_counter == 1);
        EXPECT(rep[0].status == (cap >= 3 ? SGX_OK : SGX_ERR_NOMEM) && rep[2].status == (cap >= 4 ? SGX_OK : SGX_ERR_NOMEM));
        for (int e = 0; e < cap; e++) EXPECT(e < (cap >= 4 ? 4 : cap >= 3 ? 3 : 0) ? row[(size_t)e] >= 100 : row[(size_t)e] == -9);
        std::vector<int32_t> o2(4, -9), row2((size_t)cap, -9);
        EXPECT(sgx_covis_connected_batch(h, 3, q.data(), o2.data(), cap ? row2.data() : NULL, cap, rep.data()) == (cap >= 3 ? SGX_ERR_INVALID : SGX_ERR_NOMEM) && o2 == o && row2 == row);
    }
    { std::vector<int32_t> q = { 100 }, o(2, -9), row(3, -9); sgx_covis_report rep;
      EXPECT(sgx_covis_connected_batch(h, 1, q.data(), o.data(), row.data(), 3, &rep) == SGX_OK && row[0] == 101 && row[1] == 102 && row[2] == 103);
      EXPECT(sgx_covis_connected_batch_dev(h, NQ + 1, q.data(), o.data(), row.data(), 3, &rep, NULL) == SGX_ERR_INVALID && sgx_covis_connected_batch_dev(h, 1, q.data(), o.data(), row.data(), -1, &rep, NULL) == SGX_ERR_INVALID);
      EXPECT(sgx_covis_connected_batch_dev(h, 1, NULL, o.data(), row.data(), 3, &rep, NULL) == SGX_ERR_INVALID && sgx_covis_connected_batch_dev(h, 1, q.data(), NULL, row.data(), 3, &rep, NULL) == SGX_ERR_INVALID);
      EXPECT(sgx_covis_connected_batch_dev(h, 1, q.data(), o.data(), NULL, 3, &rep, NULL) == SGX_ERR_INVALID && sgx_covis_connected_batch_dev(h, 1, q.data(), o.data(), row.data(), 3, NULL, NULL) == SGX_ERR_INVALID);
      EXPECT(sgx_covis_connected_batch_dev(h, 0, NULL, NULL, NULL, 0, NULL, NULL) == SGX_OK && sgx_covis_connected_batch(h, 0, q.data(), o.data(), row.data(), 3, &rep) == SGX_ERR_INVALID); }

    // ---- gba_update / correct_points: tables of exactly nk rows, malformed tables, an origin outside the GBA; a refused call writes nothing
    {
        const int nk = sgx_covis_size(h);
        std::vector<int32_t> ids((size_t)nk), org(1, 100); std::vector<uint8_t> ing((size_t)nk, 1), st((size_t)nk, 0x55);
        for (int k = 0; k < nk; k++) ids[(size_t)k] = 100 + k;
        std::vector<float> T((size_t)nk * 12, 0.f), G, O((size_t)nk * 12, -9.f), B((size_t)nk * 12, -9.f);
        for (int k = 0; k < nk; k++) { T[(size_t)k * 12] = T[(size_t)k * 12 + 5] = T[(size_t)k * 12 + 10] = 1.f; T[(size_t)k * 12 + 3] = (float)k; }
        G = T; for (int k = 0; k < nk; k++) G[(size_t)k * 12 + 7] = 0.5f;
        ing[4] = 0;                                                           // 104's parent is 103 (its only neighbour); 103 and 100 .. 102 hang together, the rest are roots
        sgx_covis_gba_report GR; memset(&GR, 0x55, sizeof(GR));
        auto untouched = [&]() { for (float x : O) EXPECT(x == -9.f); for (float x : B) EXPECT(x == -9.f); for (uint8_t x : st) EXPECT(x == 0x55); };
        EXPECT(sgx_covis_gba_update_dev(h, 1, org.data(), nk, ids.data(), ing.data(), T.data(), G.data(), O.data(), B.data(), st.data(), &GR, NULL) == SGX_OK && GR.status == SGX_OK);
        EXPECT(GR.n_visited >= 1 && GR.n_visited + GR.n_unreached == nk && GR.max_depth <= 1);
        for (int k = 0; k < nk; k++) EXPECT(st[(size_t)k] == 3 || st[(size_t)k] == 2 || st[(size_t)k] == 0);
        for (int k = 0; k < nk; k++) EXPECT(st[(size_t)k] == 3 ? B[(size_t)k * 12 + 3] == (float)k : B[(size_t)k * 12 + 3] == -9.f);
        { std::vector<float> x(9, 1.f), xg(9, 2.f), xo(9, -9.f); std::vector<uint8_t> pg = { 1, 0, 0 }; std::vector<int32_t> rf = { 0, -1, nk - 1 };
          EXPECT(sgx_gba_correct_points_dev(3, x.data(), pg.data(), xg.data(), rf.data(), st.data(), B.data(), O.data(), xo.data(), NULL) == SGX_OK && xo[0] == 2.f && xo[3] == 1.f);
          EXPECT(sgx_gba_correct_points_dev(0, NULL, NULL, NULL, NULL, NULL, NULL, NULL, NULL, NULL) == SGX_OK && sgx_gba_correct_points_dev(-1, x.data(), pg.data(), xg.data(), rf.data(), st.data(), B.data(), O.data(), xo.data(), NULL) == SGX_ERR_INVALID);
          EXPECT(sgx_gba_correct_points_dev(3, x.data(), pg.data(), xg.data(), NULL, st.data(), B.data(), O.data(), xo.data(), NULL) == SGX_ERR_INVALID);
          std::vector<float> xh(9, -9.f);
          EXPECT(sgx_gba_correct_points(3, x.data(), pg.data(), xg.data(), rf.data(), nk, st.data(), B.data(), O.data(), xh.data()) == SGX_OK && xh == xo);
          rf[2] = nk; xh.assign(9, -9.f);                                     // a reference row out of range: refused, nothing written
          EXPECT(sgx_gba_correct_points(3, x.data(), pg.data(), xg.data(), rf.data(), nk, st.data(), B.data(), O.data(), xh.data()) == SGX_ERR_INVALID && xh[0] == -9.f);
          rf[2] = -2; EXPECT(sgx_gba_correct_points(3, x.data(), pg.data(), xg.data(), rf.data(), nk, st.data(), B.data(), O.data(), xh.data()) == SGX_ERR_INVALID);
          EXPECT(sgx_gba_correct_points(0, NULL, NULL, NULL, NULL, 0, NULL, NULL, NULL, NULL) == SGX_OK && sgx_gba_correct_points(3, x.data(), pg.data(), xg.data(), NULL, nk, st.data(), B.data(), O.data(), xh.data()) == SGX_ERR_INVALID); }
        O.assign(O.size(), -9.f); B.assign(B.size(), -9.f); st.assign(st.size(), 0x55);
        ing[0] = 0;                                                           // rule 14
        EXPECT(sgx_covis_gba_update_dev(h, 1, org.data(), nk, ids.data(), ing.data(), T.data(), G.data(), O.data(), B.data(), st.data(), &GR, NULL) == SGX_OK && GR.status == SGX_COVIS_GBA_ORIGIN_NOT_IN_GBA); untouched();
        ing[0] = 1; org[0] = 5;                                               // an origin that is no keyframe
        EXPECT(sgx_covis_gba_update_dev(h, 1, org.data(), nk, ids.data(), ing.data(), T.data(), G.data(), O.data(), B.data(), st.data(), &GR, NULL) == SGX_OK && GR.status == SGX_ERR_INVALID); untouched();
        org[0] = 100; ids[3] = ids[2];                                        // an id twice
        EXPECT(sgx_covis_gba_update_dev(h, 1, org.data(), nk, ids.data(), ing.data(), T.data(), G.data(), O.data(), B.data(), st.data(), &GR, NULL) == SGX_OK && GR.status == SGX_ERR_INVALID); untouched();
        ids[3] = -4;                                                          // an id out of range
        EXPECT(sgx_covis_gba_update_dev(h, 1, org.data(), nk, ids.data(), ing.data(), T.data(), G.data(), O.data(), B.data(), st.data(), &GR, NULL) == SGX_OK && GR.status == SGX_ERR_INVALID); untouched();
        ids[3] = 103;                                                         // one row short
        EXPECT(sgx_covis_gba_update_dev(h, 1, org.data(), nk - 1, ids.data(), ing.data(), T.data(), G.data(), O.data(), B.data(), st.data(), &GR, NULL) == SGX_OK && GR.status == SGX_ERR_INVALID); untouched();
        EXPECT(sgx_covis_gba_update_dev(h, 0, org.data(), nk, ids.data(), ing.data(), T.data(), G.data(), O.data(), B.data(), st.data(), &GR, NULL) == SGX_ERR_INVALID);
        EXPECT(sgx_covis_gba_update_dev(h, 1, org.data(), 0, ids.data(), ing.data(), T.data(), G.data(), O.data(), B.data(), st.data(), &GR, NULL) == SGX_ERR_INVALID);
        EXPECT(sgx_covis_gba_update_dev(h, 1, org.data(), NKF + 1, ids.data(), ing.data(), T.data(), G.data(), O.data(), B.data(), st.data(), &GR, NULL) == SGX_ERR_INVALID);
        EXPECT(sgx_covis_gba_update_dev(h, 1, org.data(), nk, ids.data(), ing.data(), T.data(), G.data(), T.data(), B.data(), st.data(), &GR, NULL) == SGX_ERR_INVALID);
        EXPECT(sgx_covis_gba_update_dev(h, 1, NULL, nk, ids.data(), ing.data(), T.data(), G.data(), O.data(), B.data(), st.data(), &GR, NULL) == SGX_ERR_INVALID);
        EXPECT(sgx_covis_gba_update_dev(h, 1, org.data(), nk, ids.data(), ing.data(), T.data(), G.data(), O.data(), B.data(), st.data(), NULL, NULL) == SGX_ERR_INVALID); untouched();
        EXPECT(sgx_covis_gba_update(h, 1, org.data(), nk, ids.data(), ing.data(), T.data(), G.data(), O.data(), B.data(), st.data(), &GR) == SGX_OK && GR.n_visited >= 1 && st[0] == 3 && O[7] == 0.5f);
        ing[0] = 0; O.assign(O.size(), -9.f); B.assign(B.size(), -9.f); st.assign(st.size(), 0x55);
        EXPECT(sgx_covis_gba_update(h, 1, org.data(), nk, ids.data(), ing.data(), T.data(), G.data(), O.data(), B.data(), st.data(), &GR) == SGX_COVIS_GBA_ORIGIN_NOT_IN_GBA); untouched();
    }

    // ---- sgx_covis_clear releases the groups; the next call reserves the default again
    EXPECT(sgx_covis_clear(h) == SGX_OK && sgx_covis_consistency_info(h, &bytes, &ng, &mg) == SGX_OK && bytes == 0 && mg == 0);
    EXPECT(add_kf(h, 7) == SGX_OK);
    { std::vector<int32_t> c(1, 7), n(1, 1), e((size_t)NKF, -9), ne(1, -9);
      EXPECT(sgx_covis_consistency_dev(h, c.data(), n.data(), 3, e.data(), ne.data(), &R, NULL) == SGX_OK && R.status == SGX_OK && R.n_after == 1);
      EXPECT(sgx_covis_consistency_info(h, &bytes, &ng, &mg) == SGX_OK && mg == SGX_COVIS_DEFAULT_GROUPS && ng == 1); }
    sgx_covis_destroy(h);
    if (g_bad) { fprintf(stderr, "loopclose_probe: %d failed expectations\n", g_bad); return 1; }
    printf("loopclose_probe: ok\n");
    return 0;
}
