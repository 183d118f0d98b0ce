// example_objects.cpp — sgx::Detector3D / sgx::ObjectDatabase (sgx_host.hpp) as PointCloudMapping::generatePointCloud uses the reference classes
// (PointcloudMapping.cc:189-190): Detect() on the boxes of one keyframe, twice, then the database.
// usage: example_objects depth.f32 width height fx fy cx cy twc.f64 class prob x y w h   (Detector3D parameters of tests/obj3d_cases.py)
#include "sgx_host.hpp"
#include <cstdio>
#include <cstdlib>

int main(int argc, char **argv)
{
    if (argc != 15) { fprintf(stderr, "usage: see the head of example_objects.cpp\n"); return 2; }
    const int W = atoi(argv[2]), H = atoi(argv[3]);
    const float cam[4] = { (float)atof(argv[4]), (float)atof(argv[5]), (float)atof(argv[6]), (float)atof(argv[7]) };
    std::vector<float> depth((size_t)W * H); double Twc[16];
    FILE *f = fopen(argv[1], "rb"); if (!f || fread(depth.data(), 4, depth.size(), f) != depth.size()) return 3; fclose(f);
    f = fopen(argv[8], "rb"); if (!f || fread(Twc, 8, 16, f) != 16) return 3; fclose(f);
    sgx::Detector3D det(10, 1.0, 0.01f, 0.05f, 50, 30000, 0.1f, 0.5f, 5.0f, W, H, cam);
    sgx::Object2D o{ (float)atof(argv[11]), (float)atof(argv[12]), (float)atof(argv[13]), (float)atof(argv[14]), (float)atof(argv[10]), atoi(argv[9]) };
    std::vector<sgx::Object2D> v{ o, o };
    det.Detect(v, depth.data(), Twc);
    printf("objects %d\n", det.mpObjectDatabase->getDataBaseSize());
    for (int id = 1; id <= det.mpObjectDatabase->getDataBaseSize(); id++) {
        const sgx::SemanticObject s = det.mpObjectDatabase->getObjectByID(id);
        printf("%d %d %.9g %.9g %.9g %.9g %.9g %.9g %.9g\n", s.object_id, s.class_id, s.prob, s.centroid[0], s.centroid[1], s.centroid[2], s.size[0], s.size[1], s.size[2]);
    }
    return 0;
}
