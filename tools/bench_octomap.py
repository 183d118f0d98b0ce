"""Times OctomapServer (sgx_octomap_*: one ray per cloud point through a device-resident map of 3 cm cells) on the eight scenes of tools/bench_cloud.py: TUM3's cloud
parameters, about 41 000 points a scan, the launch file's resolution, the poses along a walk so that the map grows.  Insertion of 1, 16 and 64 scans into an empty
map, then the occupied-cells query and the projection of the largest map; HIP events around the launch sequence alone (inputs on the device, no read-back), median
of the timed repetitions after 3 warm-up runs.  sgx_cloud_build_batch_dev is timed for the same keyframes in the same run, and the ratio insertion : cloud build is
reported.  Also the mean and maximum ray length in cells and the brick count.
With --trace-one N the tool builds the clouds, runs one warmed-up insertion of N scans with one cells query and one projection, and exits: under
`rocprofv3 --kernel-trace --stats -- python tools/bench_octomap.py --trace-one 16` that gives the kernels' shares.
Usage: python tools/bench_octomap.py [--reps 20] [--out FILE.json] [--scans 1,16,64] [--trace-one N]"""
import argparse
import ctypes as C
import json
import os
import sys
import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, 'tests')); sys.path.insert(0, os.path.join(ROOT, 'tools'))
import sg_slam_amd
import cloud_cases as cc
import bench_cloud
from obj3d_cases import cam_for, pose
from sg_slam_amd.capi import _vp, CLOUD_POINT_DTYPE, CLOUD_RESULT_DTYPE, OCTOMAP_CELL_DTYPE
from sg_slam_amd.pointcloudmapping import PointCloudMappingBatch, camera_to_map_tf
from sg_slam_amd.octomapserver import OctomapServer, sensor_to_world

W, H = bench_cloud.W, bench_cloud.H
PARAMS = dict(res=0.03, max_range=-1.0, occupancy_min_z=-1.5, occupancy_max_z=1.5, pointcloud_min_z=-5.0, pointcloud_max_z=5.0)      # the values of the reference's launch file


def timed(fn, reps, warm=3):
    t = []
    for r in range(warm + reps):
        e0 = torch.cuda.Event(enable_timing=True); e1 = torch.cuda.Event(enable_timing=True)
        pre = fn(None)
        e0.record(); fn(pre); e1.record(); torch.cuda.synchronize()
        if r >= warm: t.append(e0.elapsed_time(e1))
    return dict(ms_median=float(np.median(t)), ms_min=float(np.min(t)), ms_max=float(np.max(t)))


def main():
    ap = argparse.ArgumentParser(); ap.add_argument('--reps', type=int, default=20); ap.add_argument('--out', default=None); ap.add_argument('--scans', default='1,16,64')
    ap.add_argument('--trace-one', type=int, default=0)
    a = ap.parse_args()
    lib = sg_slam_amd.load(); out = {'device': torch.cuda.get_device_name(0), 'cloud_parameters': cc.TUM3_PARAMS, 'octomap_parameters': PARAMS, 'configs': []}
    depths, cols, boxes, have = bench_cloud.keyframes(); cam = cam_for(W, H)
    reps = 1 if a.trace_one else a.reps; warm = 1 if a.trace_one else 3
    S = None
    for n in ([a.trace_one] if a.trace_one else [int(v) for v in a.scans.split(',')]):
        idx = [i % bench_cloud.SCENES for i in range(n)]
        B = PointCloudMappingBatch(cc.TUM3_PARAMS, W, H, cam, n, cc.LOCAL, max_boxes=4, lib=lib)
        d_dev = torch.from_numpy(depths[idx]).cuda(); c_dev = torch.from_numpy(cols[idx]).cuda(); bx = [boxes[i] for i in idx]; hv = [have[i] for i in idx]
        cloud = timed(lambda pre: B.launch(d_dev, c_dev, None, bx, hv) if pre is not None else 1, reps, warm)       # the yardstick: the producer of the scans
        mats = []
        for j in range(n):                                                                       # a walk: 4 cm and 1.2 degrees a keyframe
            o, q = camera_to_map_tf(np.linalg.inv(pose(rvec=(0.0, 0.021 * j, 0.0), t=(0.04 * j, 0.01 * j, 0.0))).astype('f4'), lib=lib); mats.append(sensor_to_world(o, q, lib=lib))
        m_dev = torch.from_numpy(np.array(mats, 'f4').reshape(n, 16)).cuda(); r_dev = torch.zeros(n * 64, dtype=torch.uint8, device='cuda')
        if S is not None: S.close()
        S = OctomapServer(PARAMS, max_bricks=1 << 16, max_points_per_scan=W * H, lib=lib)

        def insert(pre):
            if pre is None: S.reset(); return 1
            S.insert_batch_dev(B.points, B.N, B.results, CLOUD_RESULT_DTYPE.itemsize, m_dev, n, r_dev)
        ins = timed(insert, reps, warm)
        recs = S.read_records(r_dev); b = S.bounds()
        assert (recs['flags'] == 0).all(), recs['flags']
        # ray lengths in cells: the DDA makes one step per unit of key distance
        res = B.read(); lens = []
        for j in range(min(n, 8)):
            p = res[j][0]; xyz = np.stack([p['x'], p['y'], p['z']], 1); mw = mats[j]
            wpt = (xyz @ mw[:3, :3].T + mw[:3, 3]).astype('f8')
            lens.append(np.abs(np.floor(wpt / PARAMS['res']) - np.floor(mw[:3, 3].astype('f8') / PARAMS['res'])).sum(1))
        lens = np.concatenate(lens)
        cfg = {'scans': n, 'insert': ins, 'insert_ms_per_scan': ins['ms_median'] / n, 'cloud_build': cloud, 'cloud_ms_per_keyframe': cloud['ms_median'] / n,
               'ratio_insert_to_cloud_build': ins['ms_median'] / cloud['ms_median'], 'points_per_scan_mean': float(recs['n_passed'].mean()),
               'free_updates_per_scan_mean': float(recs['n_free_updates'].mean()), 'ray_cells_mean': float(lens.mean()), 'ray_cells_max': float(lens.max()),
               'bricks': int(b['n_bricks']), 'known_cells': int(b['n_known']), 'occupied_cells': int(b['n_occupied'])}
        out['configs'].append(cfg); print(json.dumps(cfg), flush=True)
        B.close()
    # the queries on the last (largest) map
    b = S.bounds(); cap = int(b['n_occupied']); cells = torch.zeros(max(cap, 1) * OCTOMAP_CELL_DTYPE.itemsize, dtype=torch.uint8, device='cuda'); cnt = torch.zeros(1, dtype=torch.int32, device='cuda')
    stream = lambda: C.c_void_p(torch.cuda.current_stream().cuda_stream)
    q = timed(lambda pre: lib.check(lib.dll.sgx_octomap_cells_dev(S.h, 1, _vp(cells), cap, _vp(cnt), stream()), 'cells') if pre is not None else 1, reps, warm)
    hd = S.grid_header(b); grid = torch.zeros(max(hd.width * hd.height, 1), dtype=torch.int8, device='cuda')
    pr = timed(lambda pre: lib.check(lib.dll.sgx_octomap_project_dev(S.h, C.byref(hd), _vp(grid), stream()), 'project') if pre is not None else 1, reps, warm)
    out['queries'] = {'bricks': int(b['n_bricks']), 'occupied_cells_listed': int(cnt.cpu()[0]), 'cells_query': q, 'grid': [hd.width, hd.height], 'projection': pr}
    print(json.dumps(out['queries']), flush=True)
    S.close()
    if a.out: json.dump(out, open(a.out, 'w'), indent=1)


if __name__ == '__main__':
    main()
