// example_initializer.cpp — sgx::Initializer (sgx_host.hpp) as Tracking::MonocularInitialization uses the reference class (Tracking.cc:619, :653): the initializer of the
// reference frame, then Initialize(current frame, matches).
// usage: example_initializer keys1.f32 n1 keys2.f32 n2 matches.i32 draws.i32 iterations fx fy cx cy   (keys = n x (x, y); draws = 8 x iterations raw rand() values)
#include "sgx_host.hpp"
#include <cstdio>
#include <cstdlib>

static sgx::FrameView frame(const char *path, int n)
{
    std::vector<float> xy((size_t)2 * n);
    FILE *f = fopen(path, "rb"); if (!f || fread(xy.data(), 4, xy.size(), f) != xy.size()) { fprintf(stderr, "cannot read %s\n", path); exit(3); } fclose(f);
    sgx::FrameView F; F.N = n; F.mvKeysUn.resize((size_t)n);
    for (int i = 0; i < n; i++) F.mvKeysUn[(size_t)i] = sgx_keypoint{ xy[(size_t)2 * i], xy[(size_t)2 * i + 1], 31.f, 0.f, 0.f, 0, -1 };
    return F;
}

int main(int argc, char **argv)
{
    if (argc != 12) { fprintf(stderr, "usage: see the head of example_initializer.cpp\n"); return 2; }
    const int n1 = atoi(argv[2]), n2 = atoi(argv[4]), iterations = atoi(argv[7]);
    const float K[4] = { (float)atof(argv[8]), (float)atof(argv[9]), (float)atof(argv[10]), (float)atof(argv[11]) };
    const sgx::FrameView F1 = frame(argv[1], n1), F2 = frame(argv[3], n2);
    std::vector<int32_t> vMatches12((size_t)n1), draws((size_t)8 * iterations);
    FILE *f = fopen(argv[5], "rb"); if (!f || fread(vMatches12.data(), 4, vMatches12.size(), f) != vMatches12.size()) return 3; fclose(f);
    f = fopen(argv[6], "rb"); if (!f || fread(draws.data(), 4, draws.size(), f) != draws.size()) return 3; fclose(f);
    sgx::Initializer init(F1, K, 1.0f, iterations);
    float R21[9], t21[3]; std::vector<float> vP3D; std::vector<bool> vbTriangulated; sgx_init_report rep;
    const bool ok = init.Initialize(F2, vMatches12, R21, t21, vP3D, vbTriangulated, &draws, &rep);
    int ntri = 0; for (bool b : vbTriangulated) ntri += b ? 1 : 0;
    printf("ok %d model %d triangulated %d\n", ok ? 1 : 0, rep.model, ntri);
    if (ok) printf("%.9g %.9g %.9g %.9g %.9g %.9g %.9g %.9g %.9g %.9g %.9g %.9g\n", R21[0], R21[1], R21[2], R21[3], R21[4], R21[5], R21[6], R21[7], R21[8], t21[0], t21[1], t21[2]);
    return 0;
}
