// example_backend.cpp — the LocalMapping / detector-thread side of the C++ mirror (sgx_host.hpp): Optimizer::LocalBundleAdjustment on a flattened local
// graph and Detector2D::detect, driven from files so tests/test_host_cpp_gpu.py can compare against the oracle / the Python mirror.
//   example_backend ba  graph.bin                       graph.bin = int32 np, nl, ne | poses f32 | fixed u8 | points f32 | edge_pose i32 | edge_point i32 | obs f32 | info f32
//   example_backend det model.param model.bin frame.raw   frame.raw = 480 x 640 x 3 u8 (BGR)
//   example_backend flow cur.raw prev.raw pts.bin          two 480 x 640 u8 frames, pts.bin = int32 n | n x 2 f32: calcOpticalFlowPyrLK + findFundamentalMat (Frame.cc:445, :469-472)
//   example_backend sim3 pairs.bin                        int32 n, fix_scale | p1c p2c (n x 3 f32) obs1 obs2 (n x 2 f32) info1 info2 (n f32) | K1 K2 (4 f32) | S12 (8 f64): OptimizeSim3
//   example_backend stereo left.raw right.raw width height nfeatures scale nlevels fx bf   two rectified gray images: the stereo Frame constructor up to ComputeStereoMatches (Frame.cc:70-99, :716-890)
//   example_backend covis map.bin                        int32 monocular, nkf | per keyframe: int32 id, n, octave[n], f32 uright[n], depth[n], int32 points[n] (-1 none) | int32 nuc, ids |
//                                                        int32 nframe, frame | int32 current keyframe: UpdateConnections, the lists, UpdateLocalMap, the culling votes and loop
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <map>
#include "sgx_host.hpp"

static std::vector<uint8_t> slurp(const char *p)
{
    FILE *f = fopen(p, "rb");
    if (!f) { fprintf(stderr, "cannot read %s\n", p); exit(2); }
    fseek(f, 0, SEEK_END); const long n = ftell(f); fseek(f, 0, SEEK_SET);
    std::vector<uint8_t> b((size_t)n);
    if (n && fread(b.data(), 1, (size_t)n, f) != (size_t)n) { fprintf(stderr, "short read %s\n", p); exit(2); }
    fclose(f);
    return b;
}

int main(int argc, char **argv)
{
    const sgx_camera cam{535.4f, 539.2f, 320.1f, 247.6f, 40.0f, 0.f, 640.f, 0.f, 480.f};
    if (argc >= 3 && !strcmp(argv[1], "ba")) {
        const std::vector<uint8_t> b = slurp(argv[2]);
        const int32_t *hdr = (const int32_t *)b.data(); const int np = hdr[0], nl = hdr[1], ne = hdr[2];
        const uint8_t *p = b.data() + 12;
        sgx::Optimizer::LocalGraph g;
        auto take = [&](auto &v, size_t n) { v.resize(n); memcpy(v.data(), p, n * sizeof(v[0])); p += n * sizeof(v[0]); };
        take(g.poses, (size_t)np * 16); take(g.pose_fixed, (size_t)np); take(g.points, (size_t)nl * 3); take(g.edge_pose, (size_t)ne); take(g.edge_point, (size_t)ne);
        take(g.edge_obs, (size_t)ne * 3); take(g.edge_info, (size_t)ne);
        sgx_ba_stats st;
        const std::vector<uint8_t> erase = sgx::Optimizer::LocalBundleAdjustment(g, cam, nullptr, &st);
        int nerase = 0; for (uint8_t e : erase) nerase += e;
        printf("iterations %d %d chi2 %.17g erased %d\n", st.iterations_first, st.iterations_second, st.chi2_second, nerase);
        printf("pose1"); for (int i = 0; i < 16; i++) printf(" %.9g", g.poses[16 + i]); printf("\n");
        return 0;
    }
    if (argc >= 5 && !strcmp(argv[1], "det")) {
        const std::vector<uint8_t> param = slurp(argv[2]), bin = slurp(argv[3]), img = slurp(argv[4]);
        sgx::Detector2D det(0.9f, 0.01f, std::string(param.begin(), param.end()), bin);
        det.detect(img.data(), 640 * 3);
        printf("raw %zu objects %zu map_boxes %zu rm_boxes %zu dyn_map %d dyn_rm %d\n", det.raw.size(), det.mvObjects2D.size(), det.mvPotentialDynamicBorderForMapping.size(),
               det.mvPotentialDynamicBorderForRmDynamicFeature.size(), (int)det.mbHaveDynamicObjectForMapping, (int)det.mbHaveDynamicObjectForRmDynamicFeature);
        for (size_t i = 0; i < det.raw.size() && i < 5; i++) printf("row %g %.9g %.9g %.9g %.9g %.9g\n", det.raw[i].label, det.raw[i].score, det.raw[i].xmin, det.raw[i].ymin, det.raw[i].xmax, det.raw[i].ymax);
        return 0;
    }
    if (argc >= 5 && !strcmp(argv[1], "flow")) {
        const std::vector<uint8_t> cur = slurp(argv[2]), prev = slurp(argv[3]), pb = slurp(argv[4]);
        const int n = *(const int32_t *)pb.data();
        std::vector<float> pts((size_t)2 * n), next; std::vector<uint8_t> st;
        memcpy(pts.data(), pb.data() + 4, sizeof(float) * 2 * (size_t)n);
        sgx::OpticalFlowLK lk(640, 480);
        lk(cur.data(), prev.data(), pts, next, st);
        std::vector<float> a, b; int ntr = 0;
        for (int i = 0; i < n; i++) if (st[(size_t)i]) { ntr++; a.push_back(pts[2 * (size_t)i]); a.push_back(pts[2 * (size_t)i + 1]); b.push_back(next[2 * (size_t)i]); b.push_back(next[2 * (size_t)i + 1]); }
        double F[9]; const bool ok = sgx::findFundamentalMat(a, b, F);
        printf("tracked %d ok %d\n", ntr, (int)ok);
        printf("first"); for (int i = 0; i < 8 && i < 2 * n; i++) printf(" %.9g", next[(size_t)i]); printf("\n");
        printf("F"); for (int i = 0; i < 9; i++) printf(" %.17g", F[i]); printf("\n");
        return 0;
    }
    if (argc >= 3 && !strcmp(argv[1], "sim3")) {
        const std::vector<uint8_t> b = slurp(argv[2]);
        const int32_t *hdr = (const int32_t *)b.data(); const int n = hdr[0], fix = hdr[1];
        const uint8_t *p = b.data() + 8;
        sgx::Optimizer::Sim3Pairs c; float K1[4], K2[4]; sgx::Optimizer::Sim3 S;
        auto take = [&](std::vector<float> &v, size_t m) { v.resize(m); memcpy(v.data(), p, m * 4); p += m * 4; };
        take(c.p1c, (size_t)n * 3); take(c.p2c, (size_t)n * 3); take(c.obs1, (size_t)n * 2); take(c.obs2, (size_t)n * 2); take(c.info1, (size_t)n); take(c.info2, (size_t)n);
        memcpy(K1, p, 16); p += 16; memcpy(K2, p, 16); p += 16; memcpy(S.v, p, 64);
        std::vector<uint8_t> inl;
        const int nin = sgx::Optimizer::OptimizeSim3(c, K1, K2, S, 10.0f, fix != 0, inl);
        int kept = 0; for (uint8_t e : inl) kept += e;
        printf("nin %d kept %d\n", nin, kept);
        printf("S12"); for (int i = 0; i < 8; i++) printf(" %.17g", S.v[i]); printf("\n");
        return 0;
    }
    if (argc >= 4 && !strcmp(argv[1], "voc")) {                     // Frame::ComputeBoW: vocabulary file (.txt = text, else binary), descriptors (N x 32 bytes)
        sgx::ORBVocabulary voc;
        const std::string vf(argv[2]);
        const bool okload = vf.size() >= 4 && vf.compare(vf.size() - 4, 4, ".txt") == 0 ? voc.loadFromTextFile(vf) : voc.loadFromBinaryFile(vf);
        if (!okload) { fprintf(stderr, "Wrong path to vocabulary.\n"); return 1; }        // System.cc:74-79
        const std::vector<uint8_t> d = slurp(argv[3]);
        sgx::ORBVocabulary::BowVector v; std::vector<int32_t> fn;
        voc.transform(d, v, fn, 4);
        double wsum = 0; long long idsum = 0, nodesum = 0; for (auto &e : v) { wsum += e.second; idsum += e.first; } for (int32_t x : fn) nodesum += x;
        printf("words %u bow %zu idsum %lld nodesum %lld wsum %.17g self %.17g\n", voc.size(), v.size(), idsum, nodesum, wsum, voc.score(v, v));
        return 0;
    }
    if (argc >= 3 && !strcmp(argv[1], "s3solver")) {               // Sim3Solver: n, fix, then x3dc1, x3dc2 (n x 3), maxErr1, maxErr2 (n), K1, K2 (4 floats each)
        const std::vector<uint8_t> b = slurp(argv[2]);
        const int32_t *hdr = (const int32_t *)b.data(); const int n = hdr[0], fix = hdr[1];
        const uint8_t *p = b.data() + 8;
        std::vector<float> x1, x2, e1, e2; float K1[4], K2[4];
        auto take = [&](std::vector<float> &v, size_t m) { v.resize(m); memcpy(v.data(), p, m * 4); p += m * 4; };
        take(x1, (size_t)n * 3); take(x2, (size_t)n * 3); take(e1, (size_t)n); take(e2, (size_t)n); memcpy(K1, p, 16); p += 16; memcpy(K2, p, 16);
        std::vector<int32_t> idx((size_t)n); for (int i = 0; i < n; i++) idx[(size_t)i] = 2 * i;          // pretend every second keypoint of pKF1 carries a usable pair
        sgx::Sim3Solver solver(x1, x2, e1, e2, K1, K2, idx, 2 * n, fix != 0, 7);
        solver.SetRansacParameters(0.99, 20, 300);
        bool bNoMore = false; std::vector<bool> vbInliers; int nInliers = 0, calls = 0; float T12[16]; bool found = false;
        while (!found && !bNoMore) { found = solver.iterate(5, bNoMore, vbInliers, nInliers, T12); calls++; }     // the loop of LoopClosing::ComputeSim3 (:296-335) for one candidate
        int marked = 0, odd = 0; for (size_t i = 0; i < vbInliers.size(); i++) { marked += vbInliers[i]; if ((i & 1) && vbInliers[i]) odd++; }
        printf("found %d calls %d inliers %d marked %d odd %d\n", (int)found, calls, nInliers, marked, odd);
        printf("T12"); for (int i = 0; i < 16; i++) printf(" %.9g", found ? T12[i] : 0.f); printf("\n");
        return 0;
    }
    if (argc >= 3 && !strcmp(argv[1], "covis")) {
        const std::vector<uint8_t> b = slurp(argv[2]);
        const int32_t *p = (const int32_t *)b.data();
        const int mono = *p++, nkf = *p++;
        sgx::CovisibilityGraph G(nkf + 1, 256, 1 << 14, nkf * 256, 4, mono != 0, 40.0f);
        for (int k = 0; k < nkf; k++) {
            const int32_t id = *p++, n = *p++;
            const std::vector<int32_t> oct(p, p + n); p += n;
            const float *f = (const float *)p; const std::vector<float> ur(f, f + n), dp(f + n, f + 2 * n); p += 2 * n;
            G.AddKeyFrame(id, oct, ur, dp);
            std::vector<int32_t> idx, pts;
            for (int i = 0; i < n; i++) if (p[i] >= 0) { idx.push_back(i); pts.push_back(p[i]); }
            p += n;
            G.SetObservations(id, idx, pts);
        }
        const int nuc = *p++;
        for (int k = 0; k < nuc; k++) {
            const int32_t id = *p++; const sgx_covis_report r = G.UpdateConnections(id);
            printf("uc %d: %d %d %d %d %d %d |", id, r.status, r.n_counter, r.max_weight, r.max_kf, r.n_ordered, r.parent);
            for (auto &e : G.GetOrderedConnectedKeyFrames(id)) printf(" %d:%d", e.first, e.second);
            printf(" |"); for (int32_t c : G.GetBestCovisibilityKeyFrames(id, 10)) printf(" %d", c);
            printf("\n");
        }
        const int nf = *p++; const std::vector<int32_t> frame(p, p + nf); p += nf;
        const sgx::CovisibilityGraph::LocalMap L = G.UpdateLocalMap(frame, 3, {}, -1, 1 << 14);
        printf("local_kf %d ref %d tracked %d:", (int)L.mvpLocalKeyFrames.size(), L.mpReferenceKF, L.trackedMapPoints); for (int32_t k : L.mvpLocalKeyFrames) printf(" %d", k);
        printf("\nlocal_points %d:", (int)L.mvpLocalMapPoints.size()); for (size_t i = 0; i < L.mvpLocalMapPoints.size(); i++) printf(" %d/%d", L.mvpLocalMapPoints[i], L.observations[i]);
        const int32_t cur = *p++;
        printf("\nvotes:"); for (auto &v : G.KeyFrameCullingVotes(cur)) printf(" %d:%d/%d/%d", v.mnId, v.nRedundantObservations, v.nMPs, v.cull);
        printf("\nculled:"); for (int32_t k : G.KeyFrameCulling(cur)) printf(" %d", k);
        printf("\nparent of %d: %d, children:", cur, G.GetParent(cur)); for (int32_t c : G.GetChilds(cur)) printf(" %d", c);
        printf("\n");
        // the essential graph of a loop between cur and its parent with no new connection yet (a query: the handle does not change): the spanning tree and the
        // covisibility edges of weight 100 and more
        {
            const int32_t loop = G.GetParent(cur) >= 0 ? G.GetParent(cur) : cur;
            const sgx::CovisibilityGraph::EssentialGraph e = G.essential_graph(cur, loop, { cur }, { 0, 0 }, {});
            printf("eg vertices %d fixed", (int)e.vertex_id.size()); for (size_t j = 0; j < e.vertex_id.size(); j++) if (e.vertex_fixed[j]) printf(" %d", e.vertex_id[j]);
            printf(" edges"); for (size_t j = 0; j < e.e_i.size(); j++) printf(" %d:%d:%d", e.vertex_id[(size_t)e.e_i[j]], e.vertex_id[(size_t)e.e_j[j]], e.e_kind[j]);
            printf("\n");
        }
        // the graph of LocalBundleAdjustment(cur) after the culling, every third edge erased as vToErase, and the graph again
        for (int round = 0; round < 2; round++) {
            const sgx::CovisibilityGraph::BaGraph g = G.ba_graph(cur);
            printf("ba poses"); for (size_t j = 0; j < g.pose_id.size(); j++) printf(" %d/%d", g.pose_id[j], g.pose_fixed[j]);
            printf(" points"); for (int32_t q : g.point_id) printf(" %d", q);
            printf(" edges"); for (size_t j = 0; j < g.edge_pose.size(); j++) printf(" %d:%d:%d:%d", g.edge_pose[j], g.edge_point[j], g.edge_kp[j], g.edge_attr[j]);
            printf("\n");
            if (round) break;
            std::vector<uint8_t> erase(g.edge_pose.size(), 0);
            for (size_t j = 0; j < erase.size(); j += 3) erase[j] = 1;
            G.apply_ba_erase(g, erase);
        }
        return 0;
    }
    if (argc >= 2 && !strcmp(argv[1], "loop")) {                    // LoopClosing::CorrectLoop on a map of three keyframes: 1 shares 16 points with 2 and 14 with 3; the loop is 1 - 3
        sgx::CovisibilityGraph G(8, 32, 64, 256, 2, false, 40.0f);
        const std::vector<int32_t> oct(32, 0); const std::vector<float> ur(32, -1.f), dp(32, 1.f);
        for (int32_t k : { 1, 2, 3 }) G.AddKeyFrame(k, oct, ur, dp);
        auto iota = [](int n, int from) { std::vector<int32_t> v((size_t)n); for (int i = 0; i < n; i++) v[(size_t)i] = from + i; return v; };
        G.SetObservations(1, iota(30, 0), iota(30, 0)); G.SetObservations(2, iota(16, 0), iota(16, 0)); G.SetObservations(3, iota(14, 0), iota(14, 16));
        std::vector<float> T(4 * 12, 0.f), xw(3 * 64);
        for (int k = 1; k <= 3; k++) { T[12 * (size_t)k] = T[12 * (size_t)k + 5] = T[12 * (size_t)k + 10] = 1.f; T[12 * (size_t)k + 3] = -0.5f * k; T[12 * (size_t)k + 11] = 0.1f * k; }
        for (int i = 0; i < 64; i++) { xw[3 * (size_t)i] = 0.1f * i; xw[3 * (size_t)i + 1] = 1.f - 0.05f * i; xw[3 * (size_t)i + 2] = 4.f; }
        const sgx::Optimizer::Sim3 Scw{{0, 0, 0, 1, -0.45, 0.02, 0.1, 1}};
        const sgx::Optimizer::LoopResult r = sgx::Optimizer::CorrectLoop(G, 1, 3, Scw, [&](int32_t id, float *o) { memcpy(o, &T[12 * (size_t)id], 48); },
                                                                        [&](int32_t id, const float *o) { memcpy(&T[12 * (size_t)id], o, 48); }, xw,
                                                                        [](const sgx::CovisibilityGraph::LoopGroup &, const std::vector<sgx::Optimizer::Sim3> &) {});
        printf("group"); for (int32_t k : r.group.group_id) printf(" %d", k);
        printf(" lc"); for (int32_t k : r.connections.lc_begin) printf(" %d", k); printf(" /"); for (int32_t k : r.connections.lc_j) printf(" %d", k);
        printf(" edges"); for (size_t j = 0; j < r.graph.e_i.size(); j++) printf(" %d:%d:%d", r.graph.e_i[j], r.graph.e_j[j], r.graph.e_kind[j]);
        printf(" loop edges of 1:"); for (int32_t k : G.GetLoopEdges(1)) printf(" %d", k);
        printf("\nposes"); for (int k = 1; k <= 3; k++) for (int i = 0; i < 12; i++) printf(" %.9g", T[12 * (size_t)k + i]);
        printf("\npoints"); for (int i = 0; i < 3 * 30; i++) printf(" %.9g", xw[(size_t)i]);
        printf("\n");
        return 0;
    }
    if (argc >= 4 && !strcmp(argv[1], "loopclose")) {               // the loop-closing thread on a ring: loopclose voc.txt ring.bin (tests/test_loopclose_host_cpp_gpu.py writes it)
        sgx::ORBVocabulary voc;
        if (!voc.loadFromTextFile(argv[2])) { fprintf(stderr, "Wrong path to vocabulary.\n"); return 1; }
        const std::vector<uint8_t> raw = slurp(argv[3]); size_t at = 0;
        auto geti = [&]() { int32_t v; memcpy(&v, &raw[at], 4); at += 4; return v; };
        auto getf = [&](size_t n) { std::vector<float> v(n); if (n) memcpy(v.data(), &raw[at], 4 * n); at += 4 * n; return v; };
        auto getv = [&](size_t n) { std::vector<int32_t> v(n); if (n) memcpy(v.data(), &raw[at], 4 * n); at += 4 * n; return v; };
        const int nkf = geti(), nextra = geti(), cap = geti(), npts = geti(), ndup = geti(), cur = geti(), loop = geti();
        struct KF { int32_t id, parent, i0; std::vector<float> uright, depth, uv, T; std::vector<int32_t> pts, words; };
        std::vector<KF> kfs((size_t)(nkf + nextra));
        for (KF &k : kfs) {
            k.id = geti(); k.parent = geti(); k.i0 = geti(); const size_t n = (size_t)geti();
            k.uright = getf((size_t)cap); k.depth = getf((size_t)cap); k.uv = getf(2 * (size_t)cap); k.pts = getv(n); k.T = getf(12); k.words = getv((size_t)geti());
        }
        std::vector<float> xw = getf(3 * (size_t)npts); const std::vector<int32_t> pref = getv((size_t)npts), dup = getv(2 * (size_t)ndup);
        sgx::Optimizer::Sim3 Scw; memcpy(Scw.v, &raw[at], 64); at += 64;
        const std::vector<float> camv = getf(5), inv = getf(8);
        const sgx_camera cam{camv[0], camv[1], camv[2], camv[3], camv[4], 0.f, 640.f, 0.f, 480.f};
        sgx::CovisibilityGraph G(64, cap, npts, 8 * npts, 8, false, 40.0f);
        sgx::KeyFrameDatabase db(voc, 64);
        sgx::LoopClosing L(G, db);
        std::map<int32_t, const KF *> by_id; std::map<int32_t, std::vector<float>> T;
        auto iota = [](size_t n, int from) { std::vector<int32_t> v(n); for (size_t i = 0; i < n; i++) v[i] = from + (int)i; return v; };
        auto add = [&](const KF &k) {
            G.AddKeyFrame(k.id, std::vector<int32_t>((size_t)cap, 0), k.uright, k.depth); G.SetObservations(k.id, iota(k.pts.size(), 0), k.pts);
            if (k.parent >= 0) G.SetObservations(k.parent, iota(k.pts.size(), k.i0), k.pts);
            G.UpdateConnections(k.id); by_id[k.id] = &k; T[k.id] = k.T;
        };
        auto bow = [](const KF &k) { sgx::LoopClosing::BowVector v; for (int32_t w : k.words) v.emplace_back(w, 1.0 / (double)k.words.size()); return v; };
        printf("accepted");
        for (int t = 0; t < nkf; t++) { add(kfs[(size_t)t]); if (L.DetectLoop(kfs[(size_t)t].id, bow(kfs[(size_t)t]))) { printf(" %d enough", kfs[(size_t)t].id); for (int32_t c : L.mvpEnoughConsistentCandidates) printf(" %d", c); } }
        printf(" groups"); for (const auto &g : G.GetConsistentGroups()) { printf(" ["); for (int32_t k : g.first) printf(" %d", k); printf(" ]:%d", g.second); }
        const sgx::Optimizer::LoopResult r = L.CorrectLoop(cur, loop, Scw, [&](int32_t id, float *o) { memcpy(o, T[id].data(), 48); }, [&](int32_t id, const float *o) { memcpy(T[id].data(), o, 48); }, xw,
                                                           [&](const sgx::CovisibilityGraph::LoopGroup &, const std::vector<sgx::Optimizer::Sim3> &) { for (int i = 0; i < ndup; i++) G.Replace(dup[2 * (size_t)i], dup[2 * (size_t)i + 1]); });
        printf("\nloop last %ld group", L.mLastLoopKFid); for (int32_t k : r.group.group_id) printf(" %d", k);
        printf(" edges %zu loop edges of %d:", r.graph.e_i.size(), cur); for (int32_t k : G.GetLoopEdges(cur)) printf(" %d", k);
        const auto u = L.RunGlobalBundleAdjustment((unsigned long)cur, cam, { 0 },
            [&](int32_t id, float *o) { memcpy(o, T[id].data(), 48); },
            [&](int32_t id, int32_t idx, float *o) { const KF &k = *by_id[id]; o[0] = k.uv[2 * (size_t)idx]; o[1] = k.uv[2 * (size_t)idx + 1]; o[2] = k.uright[(size_t)idx]; },
            [&](int octave) { return inv[(size_t)octave]; },
            [&](int32_t id, float *o) { memcpy(o, &xw[3 * (size_t)id], 12); },
            [&](int32_t id) { return pref[(size_t)id]; },
            [&]() { for (int t = nkf; t < nkf + nextra; t++) add(kfs[(size_t)t]); });
        printf("\ngba visited %d propagated %d unreached %d depth %d state", u.update.report.n_visited, u.update.report.n_propagated, u.update.report.n_unreached, u.update.report.max_depth);
        for (uint8_t v : u.update.kf_state) printf(" %d", v);
        printf(" ids"); for (int32_t k : u.kf_ids) printf(" %d", k);
        printf(" early");
        for (int t = nkf; t < nkf + nextra; t++) { L.DetectLoop(kfs[(size_t)t].id, bow(kfs[(size_t)t])); printf(" %d", L.early ? 1 : 0); }
        printf(" db %d", db.size());
        printf("\nposes"); for (float v : u.update.Tcw) printf(" %.9g", v);
        printf("\npoints"); for (size_t i = 0; i < u.point_ids.size(); i++) printf(" %d %.9g %.9g %.9g", u.point_ids[i], u.update.xw[3 * i], u.update.xw[3 * i + 1], u.update.xw[3 * i + 2]);
        printf("\n");
        return 0;
    }
    if (argc >= 11 && !strcmp(argv[1], "stereo")) {                 // the stereo Frame constructor up to ComputeStereoMatches (Frame.cc:70-99): left.raw right.raw width height nfeatures scale nlevels fx bf
        const int W = atoi(argv[4]), H = atoi(argv[5]);
        const std::vector<uint8_t> l = slurp(argv[2]), r = slurp(argv[3]);
        if (l.size() != (size_t)W * H || r.size() != l.size()) { fprintf(stderr, "stereo: the images are not %d x %d bytes\n", W, H); return 2; }
        sgx::ORBextractor exl(atoi(argv[6]), (float)atof(argv[7]), atoi(argv[8]), 20, 7, W, H), exr(atoi(argv[6]), (float)atof(argv[7]), atoi(argv[8]), 20, 7, W, H);
        sgx::StereoMatcher stereo(exl, exr);
        sgx::StereoMatches m;
        stereo(sgx::GrayView{l.data(), H, W, W}, sgx::GrayView{r.data(), H, W, W}, (float)atof(argv[9]), (float)atof(argv[10]), m);
        printf("keys %d right %d matched %d\n", (int)m.mvKeys.size(), (int)m.mvKeysRight.size(), m.nmatched);
        for (size_t i = 0; i < m.mvKeys.size(); i++) printf("%.9g %.9g %.9g %.9g\n", m.mvKeys[i].x, m.mvKeys[i].y, m.mvuRight[i], m.mvDepth[i]);
        return 0;
    }
    fprintf(stderr, "usage: %s ba graph.bin | det model.param model.bin frame.raw | flow cur.raw prev.raw pts.bin | sim3 pairs.bin | voc voc.txt desc.bin | s3solver pairs.bin |"
                    " stereo left.raw right.raw width height nfeatures scale nlevels fx bf | covis map.bin | loop\n", argv[0]);
    return 2;
}
