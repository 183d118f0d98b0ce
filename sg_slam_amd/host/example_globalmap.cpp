// example_globalmap.cpp — sgx::GlobalMap (sgx_host.hpp) as MapViewer keeps the reference's globalMap (PointcloudMapping.cc:332-360): the filtered temp_globalMap of
// every keyframe is appended, and the schedule decides when voxel_global + sor_global run over the whole map and the map is published.
// usage: example_globalmap leaf mean_k stddev_mul threshold max_points cloud.bin pending [cloud.bin pending]...
//        cloud.bin = sgx_cloud_point records (x, y, z float, rgba uint32), pending = what CheckNewKeyFrames() answers after that keyframe (0 / 1)
#include "sgx_host.hpp"
#include <cstdio>
#include <cstdlib>

int main(int argc, char **argv)
{
    if (argc < 8 || (argc - 6) % 2) { fprintf(stderr, "usage: see the head of example_globalmap.cpp\n"); return 2; }
    sgx::GlobalMap map((float)atof(argv[1]), atoi(argv[2]), atof(argv[3]), atoi(argv[4]), atoi(argv[5]));
    std::vector<sgx_cloud_point> published;
    for (int a = 6; a + 1 < argc; a += 2) {
        FILE *f = fopen(argv[a], "rb"); if (!f) return 3;
        fseek(f, 0, SEEK_END); const long bytes = ftell(f); fseek(f, 0, SEEK_SET);
        std::vector<sgx_cloud_point> cloud((size_t)bytes / sizeof(sgx_cloud_point));
        if (fread(cloud.data(), sizeof(sgx_cloud_point), cloud.size(), f) != cloud.size()) return 3;
        fclose(f);
        const sgx_globalmap_append_record r = map.append(cloud);
        sgx_globalmap_result c;
        const bool pub = map.update(atoi(argv[a + 1]) != 0, published, &c);
        printf("keyframe %d in %d offset %d size %d flags %d published %d count %d\n", (a - 6) / 2, r.n_in, r.offset, r.map_size, r.flags, pub ? 1 : 0, map.count());
        if (pub) printf("record in %d voxels %d points %d flags %d wider %d whole %d mean %.17g thr %.17g\n", c.n_points_in, c.n_voxels, c.n_points, c.flags,
                        c.wider_window_points, c.whole_cloud_points, c.mean, c.thr);
    }
    const std::vector<sgx_cloud_point> all = map.points();
    printf("map %d\n", (int)all.size());
    for (const sgx_cloud_point &p : all) printf("%.9g %.9g %.9g %u\n", p.x, p.y, p.z, p.rgba);
    return 0;
}
