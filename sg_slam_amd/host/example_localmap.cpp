// example_localmap.cpp — sgx::PointCloudMapping (sgx_host.hpp) as MapViewer uses the reference class (PointcloudMapping.cc:225-286): one keyframe in, the filtered
// local-map cloud in ROS axes and camera_to_map_tf out.
// usage: example_localmap depth.f32 color.u8 width height fx fy cx cy tcw.f32 have_dynamic [x y w h]...   (the parameters of tests/cloud_cases.py)
#include "sgx_host.hpp"
#include <cstdio>
#include <cstdlib>

int main(int argc, char **argv)
{
    if (argc < 11 || (argc - 11) % 4) { fprintf(stderr, "usage: see the head of example_localmap.cpp\n"); return 2; }
    const int W = atoi(argv[3]), H = atoi(argv[4]);
    const float cam[4] = { (float)atof(argv[5]), (float)atof(argv[6]), (float)atof(argv[7]), (float)atof(argv[8]) };
    std::vector<float> depth((size_t)W * H), boxes; std::vector<uint8_t> color((size_t)W * H * 3); float Tcw[16];
    FILE *f = fopen(argv[1], "rb"); if (!f || fread(depth.data(), 4, depth.size(), f) != depth.size()) return 3; fclose(f);
    f = fopen(argv[2], "rb"); if (!f || fread(color.data(), 1, color.size(), f) != color.size()) return 3; fclose(f);
    f = fopen(argv[9], "rb"); if (!f || fread(Tcw, 4, 16, f) != 16) return 3; fclose(f);
    for (int i = 11; i < argc; i++) boxes.push_back((float)atof(argv[i]));
    sgx::PointCloudMapping mapping(true, 0.5f, 5.0f, 8, 1.0, 0.05f, W, H, cam, 4);
    sgx::LocalMap m;
    mapping.insertKeyFrame(color.data(), depth.data(), Tcw, boxes, atoi(argv[10]) != 0, m);
    printf("points %d used %d voxels %d flags %d mean %.17g thr %.17g\n", m.record.n_points, m.record.n_pixels_used, m.record.n_voxels, m.record.flags, m.record.mean, m.record.thr);
    printf("tf %.17g %.17g %.17g %.17g %.17g %.17g %.17g\n", m.origin[0], m.origin[1], m.origin[2], m.rotation[0], m.rotation[1], m.rotation[2], m.rotation[3]);
    for (const sgx_cloud_point &p : m.points) printf("%.9g %.9g %.9g %u\n", p.x, p.y, p.z, p.rgba);
    return 0;
}
