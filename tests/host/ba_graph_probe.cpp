// ba_graph_probe.cpp — stand-alone host program: sgx_covis_ba_graph_batch_dev / sgx_covis_ba_graph over ids out of range, capacities of 0 and one short of the need, a
// full max_queries and a keyframe erased while lists still name it.  tests/test_ba_graph_probe.py builds this file and the emulator unit with AddressSanitizer / UBSan.
// Every buffer is a heap allocation of exactly the size the entry is documented to use (rows of max_keyframes, pcap, pcap + 1 and ecap) and the emulator's device memory
// is the heap too, so a row or a workspace entry read or written outside its array ends the program.
#include "../../include/sgx.h"
#include "../../sg_slam_amd/csrc/sgx_rt.h"
#include <stdio.h>
#include <string.h>
#include <vector>

thread_local sgx_dim3 blockIdx, blockDim, gridDim;          // the emulator's launch state (the extractor's unit holds it in the full library)

static int g_bad = 0;
#define EXPECT(cond) do { if (!(cond)) { fprintf(stderr, "ba_graph_probe: line %d: %s\n", __LINE__, #cond); g_bad++; } } while (0)

static const int NKF = 12, CAP = 24, NPTS = 64, NOBS = 288, NQ = 4;

static int add_kf(sgx_covis *h, int id, int n)
{
    std::vector<int32_t> o((size_t)n, 2); std::vector<float> u((size_t)n, -1.f), d((size_t)n, 2.f);
    for (int i = 0; i < n; i += 3) u[(size_t)i] = 4.f;
    return sgx_covis_add_keyframe(h, id, n, o.data(), u.data(), d.data());
}

static int observe(sgx_covis *h, int id, int first_idx, int first_pt, int n)
{
    std::vector<int32_t> i((size_t)n), p((size_t)n);
    for (int j = 0; j < n; j++) { i[(size_t)j] = first_idx + j; p[(size_t)j] = first_pt + j; }
    return sgx_covis_set_observations(h, id, n, i.data(), p.data());
}

struct Rows {
    std::vector<int32_t> pose_id, point_id, begin, ep, el, ek; std::vector<uint8_t> pose_fixed, ea; std::vector<sgx_covis_ba_report> rep;
    Rows(int Q, int pcap, int ecap) : pose_id((size_t)Q * NKF, -9), point_id((size_t)Q * pcap, -9), begin((size_t)Q * (pcap + 1), -9), ep((size_t)Q * ecap, -9), el((size_t)Q * ecap, -9),
                                      ek((size_t)Q * ecap, -9), pose_fixed((size_t)Q * NKF, 9), ea((size_t)Q * ecap, 9), rep((size_t)Q) {}
};

// one batch into rows of exactly pcap / ecap; the written part is checked for consistency, the rest for being untouched
static void batch(sgx_covis *h, int mode, const std::vector<int32_t> &kf, int pcap, int ecap, const char *what)
{
    const int Q = (int)kf.size();
    Rows r(Q, pcap, ecap);
    EXPECT(sgx_covis_ba_graph_batch_dev(h, Q, mode, kf.data(), r.pose_id.data(), r.pose_fixed.data(), pcap, r.point_id.data(), r.begin.data(), ecap, r.ep.data(), r.el.data(),
                                        r.ek.data(), r.ea.data(), r.rep.data(), NULL) == SGX_OK);
    for (int q = 0; q < Q; q++) {
        const sgx_covis_ba_report &R = r.rep[(size_t)q];
        const int32_t *begin = &r.begin[(size_t)q * (pcap + 1)];
        EXPECT(R.status == SGX_OK || R.status == SGX_ERR_NOMEM || R.status == SGX_ERR_INVALID);
        if (R.status == SGX_ERR_INVALID) { EXPECT(r.pose_id[(size_t)q * NKF] == -9 && begin[0] == -9 && R.n_poses == 0); continue; }
        EXPECT((R.status == SGX_ERR_NOMEM) == (R.n_points > pcap || R.n_edges > ecap));
        EXPECT(R.n_poses >= (mode == SGX_COVIS_BA_LOCAL ? 1 : 0) && R.n_poses <= NKF && R.n_local_kf + R.n_fixed_kf == R.n_poses && R.n_points >= 0 && R.n_points <= NPTS && R.n_mono_edges + R.n_stereo_edges == R.n_edges);
        for (int j = 0; j < NKF; j++) EXPECT(j < R.n_poses ? (r.pose_id[(size_t)q * NKF + j] >= 0 && r.pose_fixed[(size_t)q * NKF + j] <= 2 && (j == 0 || r.pose_id[(size_t)q * NKF + j] > r.pose_id[(size_t)q * NKF + j - 1]))
                                                           : (r.pose_id[(size_t)q * NKF + j] == -9 && r.pose_fixed[(size_t)q * NKF + j] == 9));
        const int np = R.n_points < pcap ? R.n_points : pcap;
        EXPECT(begin[0] == 0);
        for (int i = 0; i < pcap; i++) EXPECT(i < np ? (r.point_id[(size_t)q * pcap + i] >= 0 && r.point_id[(size_t)q * pcap + i] < NPTS && begin[i + 1] > begin[i]) : (r.point_id[(size_t)q * pcap + i] == -9 && begin[i + 1] == -9));
        if (R.status == SGX_OK) EXPECT(begin[np] == R.n_edges);
        int ne = 0;
        for (int i = 0; i < np && begin[i + 1] <= ecap; i++) ne = begin[i + 1];
        for (int e = 0; e < ecap; e++) {
            const size_t o = (size_t)q * ecap + e;
            EXPECT(e < ne ? (r.ep[o] >= 0 && r.ep[o] < R.n_poses && r.el[o] >= 0 && r.el[o] < np && begin[r.el[o]] <= e && e < begin[r.el[o] + 1] && r.ek[o] >= 0 && r.ek[o] < CAP && (r.ea[o] & 31) == 2)
                          : (r.ep[o] == -9 && r.el[o] == -9 && r.ek[o] == -9 && r.ea[o] == 9));
        }
    }
    if (g_bad) fprintf(stderr, "ba_graph_probe: after \"%s\" (mode %d, pcap %d, ecap %d)\n", what, mode, pcap, ecap);
}

// the need of one query, then every capacity around it
static void around_the_need(sgx_covis *h, int mode, int32_t kf, const char *what)
{
    std::vector<int32_t> pose_id(NKF), begin(1); std::vector<uint8_t> pose_fixed(NKF);
    sgx_covis_ba_report R;
    const int rc = sgx_covis_ba_graph(h, mode, kf, pose_id.data(), pose_fixed.data(), 0, NULL, begin.data(), 0, NULL, NULL, NULL, NULL, &R);
    if (rc == SGX_ERR_INVALID) { batch(h, mode, { kf }, 3, 3, what); return; }
    EXPECT(rc == (R.n_points > 0 ? SGX_ERR_NOMEM : SGX_OK) && begin[0] == 0);
    for (int pcap : { 0, R.n_points - 1, R.n_points, R.n_points + 1 })
        for (int ecap : { 0, R.n_edges - 1, R.n_edges, R.n_edges + 1 })
            if (pcap >= 0 && ecap >= 0) batch(h, mode, { kf }, pcap, ecap, what);
    // the host-pointer entry with buffers of exactly the need
    std::vector<int32_t> pts((size_t)R.n_points), beg((size_t)R.n_points + 1), ep((size_t)R.n_edges), el((size_t)R.n_edges), ek((size_t)R.n_edges); std::vector<uint8_t> ea((size_t)R.n_edges);
    sgx_covis_ba_report R2;
    EXPECT(sgx_covis_ba_graph(h, mode, kf, pose_id.data(), pose_fixed.data(), R.n_points, pts.data(), beg.data(), R.n_edges, ep.data(), el.data(), ek.data(), ea.data(), &R2) == SGX_OK);
    EXPECT(R2.status == SGX_OK && memcmp(&R.n_local_kf, &R2.n_local_kf, sizeof(R) - sizeof(R.status)) == 0 && beg[(size_t)R.n_points] == R.n_edges);      // only the status differs
}

int main()
{
    sgx_covis *h = NULL;
    if (sgx_covis_create(NKF, CAP, NPTS, NOBS, NQ, 0, 40.f, &h) != SGX_OK) { fprintf(stderr, "create failed\n"); return 1; }
    batch(h, SGX_COVIS_BA_LOCAL, { 1, 2, 3, 4 }, 4, 4, "an empty handle");
    batch(h, SGX_COVIS_BA_GLOBAL, { 0 }, 4, 4, "an empty handle");
    // keyframe t sees the points [4 t, 4 t + 24): neighbours share 20, 16, ... points; keyframe 0 is among them
    for (int t = 0; t < 10; t++) { EXPECT(add_kf(h, t * 3, CAP) == SGX_OK); EXPECT(observe(h, t * 3, 0, 4 * t, CAP) == SGX_OK); }
    { std::vector<sgx_covis_report> rep(NQ);
      for (int at = 0; at < 10; at += NQ) { std::vector<int32_t> ids; for (int t = at; t < 10 && t < at + NQ; t++) ids.push_back(t * 3);
          EXPECT(sgx_covis_update_connections_batch_dev(h, (int)ids.size(), ids.data(), rep.data(), NULL) == SGX_OK); } }
    // calls refused as a whole: too many queries, two global queries, an unknown mode, missing arrays
    { Rows r(NQ + 1, 4, 4); std::vector<int32_t> kf(NQ + 1, 3);
      EXPECT(sgx_covis_ba_graph_batch_dev(h, NQ + 1, 0, kf.data(), r.pose_id.data(), r.pose_fixed.data(), 4, r.point_id.data(), r.begin.data(), 4, r.ep.data(), r.el.data(), r.ek.data(), r.ea.data(), r.rep.data(), NULL) == SGX_ERR_INVALID);
      EXPECT(sgx_covis_ba_graph_batch_dev(h, 2, 1, kf.data(), r.pose_id.data(), r.pose_fixed.data(), 4, r.point_id.data(), r.begin.data(), 4, r.ep.data(), r.el.data(), r.ek.data(), r.ea.data(), r.rep.data(), NULL) == SGX_ERR_INVALID);
      EXPECT(sgx_covis_ba_graph_batch_dev(h, 1, 2, kf.data(), r.pose_id.data(), r.pose_fixed.data(), 4, r.point_id.data(), r.begin.data(), 4, r.ep.data(), r.el.data(), r.ek.data(), r.ea.data(), r.rep.data(), NULL) == SGX_ERR_INVALID);
      EXPECT(sgx_covis_ba_graph_batch_dev(h, 1, 0, NULL, r.pose_id.data(), r.pose_fixed.data(), 4, r.point_id.data(), r.begin.data(), 4, r.ep.data(), r.el.data(), r.ek.data(), r.ea.data(), r.rep.data(), NULL) == SGX_ERR_INVALID);
      EXPECT(sgx_covis_ba_graph_batch_dev(h, 1, 0, kf.data(), r.pose_id.data(), r.pose_fixed.data(), 4, r.point_id.data(), NULL, 4, r.ep.data(), r.el.data(), r.ek.data(), r.ea.data(), r.rep.data(), NULL) == SGX_ERR_INVALID);
      EXPECT(sgx_covis_ba_graph_batch_dev(h, 1, 0, kf.data(), r.pose_id.data(), r.pose_fixed.data(), 4, r.point_id.data(), r.begin.data(), 4, r.ep.data(), r.el.data(), r.ek.data(), r.ea.data(), NULL, NULL) == SGX_ERR_INVALID);
      for (int q = 0; q < NQ + 1; q++) EXPECT(r.pose_id[(size_t)q * NKF] == -9 && r.begin[(size_t)q * 5] == -9); }
    // negative capacities: every query's status, nothing written (the rows are empty here)
    { std::vector<int32_t> kf = { 3, 6 }, pose_id(2 * NKF, -9), begin(2, -9); std::vector<uint8_t> pose_fixed(2 * NKF, 9); std::vector<sgx_covis_ba_report> rep(2);
      EXPECT(sgx_covis_ba_graph_batch_dev(h, 2, 0, kf.data(), pose_id.data(), pose_fixed.data(), -1, NULL, begin.data(), 0, NULL, NULL, NULL, NULL, rep.data(), NULL) == SGX_OK);
      EXPECT(rep[0].status == SGX_ERR_INVALID && rep[1].status == SGX_ERR_INVALID && pose_id[0] == -9 && begin[0] == -9);
      EXPECT(sgx_covis_ba_graph_batch_dev(h, 2, 0, kf.data(), pose_id.data(), pose_fixed.data(), 0, NULL, begin.data(), -5, NULL, NULL, NULL, NULL, rep.data(), NULL) == SGX_OK);
      EXPECT(rep[0].status == SGX_ERR_INVALID && rep[1].status == SGX_ERR_INVALID && pose_id[0] == -9 && begin[0] == -9); }
    // ids out of range beside good ones, a full max_queries
    batch(h, SGX_COVIS_BA_LOCAL, { 3, -1, 1 << 30, 27 }, NPTS, NOBS, "ids out of range");
    batch(h, SGX_COVIS_BA_LOCAL, { 0, 9, 15, 27 }, NPTS, NOBS, "a full batch");
    batch(h, SGX_COVIS_BA_LOCAL, { 0, 9, 15, 27 }, 7, 40, "a full batch short of room");
    for (int32_t kf : { 0, 12, 27, 5 }) around_the_need(h, SGX_COVIS_BA_LOCAL, kf, "the need");
    around_the_need(h, SGX_COVIS_BA_GLOBAL, 0, "the need, global");
    // a keyframe erased while lists still name it: as the query (no keyframe) and inside the lists of the others; then a new keyframe in a slot that came back
    EXPECT(sgx_covis_erase_keyframe(h, 12) == SGX_OK);
    batch(h, SGX_COVIS_BA_LOCAL, { 12, 9, 15, 18 }, NPTS, NOBS, "after an erase");
    for (int32_t kf : { 12, 9, 15 }) around_the_need(h, SGX_COVIS_BA_LOCAL, kf, "after an erase");
    around_the_need(h, SGX_COVIS_BA_GLOBAL, 0, "after an erase, global");
    EXPECT(sgx_covis_erase_keyframe(h, 21) == SGX_OK && add_kf(h, 40, CAP) == SGX_OK && add_kf(h, 41, 0) == SGX_OK);
    { int32_t n = 0; EXPECT(sgx_covis_info(h, NULL, NULL, &n) == SGX_OK); const int m = NOBS - n < CAP ? NOBS - n : CAP; EXPECT(m > 0 && observe(h, 40, 0, 30, m) == SGX_OK); }
    batch(h, SGX_COVIS_BA_LOCAL, { 40, 41, 18, 24 }, NPTS, NOBS, "a fresh keyframe");
    for (int32_t kf : { 40, 41, 24 }) around_the_need(h, SGX_COVIS_BA_LOCAL, kf, "a fresh keyframe");
    around_the_need(h, SGX_COVIS_BA_GLOBAL, 0, "a fresh keyframe, global");
    EXPECT(sgx_covis_clear(h) == SGX_OK);
    batch(h, SGX_COVIS_BA_GLOBAL, { 0 }, 0, 0, "cleared");
    sgx_covis_destroy(h);
    if (!g_bad) printf("ba_graph_probe: ok\n");
    return g_bad ? 1 : 0;
}
