// example_relocalization.cpp — sgx::KeyFrameDatabase (sgx_host.hpp) as Tracking::Relocalization (Tracking.cc:1467) and LoopClosing::DetectLoop (LoopClosing.cc:126-141) use
// the reference class: the keyframes of a map are added with their covisibility, then one query asks for candidates.
// usage: example_relocalization vocabulary.txt database.bin query.bin
//   database.bin: int32 n, then per keyframe int32 mnId, nbow, ncov; int32 ids[nbow]; double weights[nbow]; int32 neighbours[ncov]
//   query.bin:    int32 mode (0 relocalisation, 1 loop), nbow; int32 ids[nbow]; double weights[nbow]; loop only: int32 nconn; int32 connected[nconn]
// A loop query takes its minScore from the connected keyframes, as LoopClosing::DetectLoop does.  Prints the candidates and the report (floats with 9 digits).
#include "sgx_host.hpp"
#include <cstdio>
#include <cstdlib>

template <class T> static std::vector<T> rd(FILE *f, size_t n)
{
    std::vector<T> v(n);
    if (n && fread(v.data(), sizeof(T), n, f) != n) { fprintf(stderr, "short file\n"); exit(3); }
    return v;
}

static sgx::ORBVocabulary::BowVector bow(FILE *f, int n)
{
    const std::vector<int32_t> ids = rd<int32_t>(f, (size_t)n); const std::vector<double> w = rd<double>(f, (size_t)n);
    sgx::ORBVocabulary::BowVector v;
    for (int i = 0; i < n; i++) v.emplace_back(ids[(size_t)i], w[(size_t)i]);
    return v;
}

int main(int argc, char **argv)
{
    if (argc != 4) { fprintf(stderr, "usage: see the head of example_relocalization.cpp\n"); return 2; }
    sgx::ORBVocabulary voc;
    if (!voc.loadFromTextFile(argv[1])) { fprintf(stderr, "cannot load %s\n", argv[1]); return 3; }
    FILE *f = fopen(argv[2], "rb"); if (!f) return 3;
    const int n = rd<int32_t>(f, 1)[0];
    sgx::KeyFrameDatabase db(voc, n > 0 ? n : 1);
    std::vector<std::pair<int32_t, std::vector<int32_t>>> covis;
    for (int k = 0; k < n; k++) {
        const std::vector<int32_t> hd = rd<int32_t>(f, 3);
        db.add(hd[0], bow(f, hd[1]));
        covis.emplace_back(hd[0], rd<int32_t>(f, (size_t)hd[2]));
    }
    fclose(f);
    for (auto &c : covis) db.setBestCovisibilityKeyFrames(c.first, c.second);
    f = fopen(argv[3], "rb"); if (!f) return 3;
    const std::vector<int32_t> hd = rd<int32_t>(f, 2);
    const sgx::ORBVocabulary::BowVector q = bow(f, hd[1]);
    sgx_kfdb_report rep; std::vector<int32_t> cand;
    if (hd[0] == 0) cand = db.DetectRelocalizationCandidates(q, &rep);
    else {
        const int nc = rd<int32_t>(f, 1)[0]; const std::vector<int32_t> conn = rd<int32_t>(f, (size_t)nc);
        const float minScore = db.MinScore(q, conn);
        printf("minScore %.9g\n", minScore);
        cand = db.DetectLoopCandidates(q, conn, minScore, &rep);
    }
    fclose(f);
    printf("candidates %d:", (int)cand.size());
    for (int32_t c : cand) printf(" %d", c);
    printf("\nreport %d %d %d %d %d %.9g %.9g %d\n", rep.n_sharing, rep.max_common_words, rep.min_common_words, rep.n_scores, rep.n_score_and_match, rep.best_acc_score,
           rep.min_score_to_retain, rep.n_candidates);
    return 0;
}
