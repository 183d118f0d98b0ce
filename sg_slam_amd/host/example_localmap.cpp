// example_localmap.cpp — sgx::PointCloudMapping (sgx_host.hpp) as MapViewer uses the reference class (PointcloudMapping.cc:225-286): one keyframe in, the filtered
// local-map cloud in ROS axes and camera_to_map_tf out; with --octomap the cloud goes on into sgx::OctomapServer as octomap_server receives it, and the scan's record,
// the map's cell counts and the projected grid follow.
// usage: example_localmap [--octomap resolution] depth.f32 color.u8 width height fx fy cx cy tcw.f32 have_dynamic [x y w h]...   (the parameters of tests/cloud_cases.py)
#include "sgx_host.hpp"
#include <cstdio>
#include <cstdlib>

int main(int argc, char **argv)
{
    double octomap_res = 0;
    if (argc > 2 && std::string(argv[1]) == "--octomap") { octomap_res = atof(argv[2]); argv += 2; argc -= 2; }
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
    if (octomap_res > 0) {
        sgx_octomap_params p = sgx::OctomapServer::defaults(); p.res = octomap_res;
        sgx::OctomapServer server(p, 1 << 12, W * H);
        const sgx_octomap_record r = server.insertCloud(m);
        printf("octomap record: %d %d %d %d %d %d\n", r.n_in, r.n_passed, r.n_free_updates, r.n_occupied_updates, r.n_new_cells, r.flags);
        const sgx_octomap_bounds_t b = server.bounds();
        printf("octomap bounds: %d %d %d\n", b.n_known, b.n_occupied, b.n_free);
        const sgx::OccupancyGrid g = server.projectedMap();
        int n100 = 0, n0 = 0, nu = 0;
        for (int8_t v : g.data) { n100 += v == 100; n0 += v == 0; nu += v == -1; }
        printf("octomap grid: %d %d %d %d %d\n", g.info.width, g.info.height, n100, n0, nu);
    }
    return 0;
}
