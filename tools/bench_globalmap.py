"""Times GlobalMap (sgx_globalmap_*: MapViewer's accumulating cloud) on the eight scenes of tools/bench_cloud.py along the walk of tools/bench_octomap.py:
64 keyframes, TUM3's parameters, the world clouds built by one SGX_CLOUD_WORLD batch and appended keyframe by keyframe straight from its device buffers, a
consolidation whenever the reference's schedule asks for one with a keyframe always waiting (count > 25) and one at the end.  HIP events around the launch sequence
alone (inputs on the device, no read-back).  The append is timed once per keyframe (its state moves on): the median over the keyframes after the first three.  Every
consolidation is timed as the median of the timed repetitions after 3 warm-up runs, the map restored from a host snapshot before each (not timed); a consolidation
that takes long gets fewer repetitions (at least 3), and the count is reported.  sgx_cloud_build_batch_dev is timed for one keyframe in the same run, and the
consolidation's cost per voxel point is reported as a ratio to it.
--ab: on the largest map, on the tap library, the tiers as built against debug_max_radius = r0 (every not-proven point straight to the whole-cloud scan), same call,
alternating.  --trace-one: one warmed-up walk and exit, for `rocprofv3 --kernel-trace --stats -- python tools/bench_globalmap.py --trace-one`.
Usage: python tools/bench_globalmap.py [--reps 20] [--keyframes 64] [--out FILE.json] [--ab] [--trace-one]"""
import argparse
import json
import os
import sys
import time
import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, 'tests')); sys.path.insert(0, os.path.join(ROOT, 'tools'))
import sg_slam_amd
import cloud_cases as cc
import bench_cloud
from obj3d_cases import cam_for, pose
from sg_slam_amd.capi import SgxLib, CLOUD_RESULT_DTYPE, CLOUD_POINT_DTYPE
from sg_slam_amd.pointcloudmapping import PointCloudMappingBatch
from sg_slam_amd.globalmap import GlobalMap

W, H = bench_cloud.W, bench_cloud.H
GP = dict(mean_k=cc.TUM3_PARAMS['mean_k'], stddev_mul=cc.TUM3_PARAMS['stddev_mul'], leaf=cc.TUM3_PARAMS['leaf'])
THRESHOLD = 25                                                           # Detector3D.global_pc_update_kf_threshold of TUM3.yaml
CAP = 1 << 22                                                            # SGX_GMAP_MAX_POINTS: 64 world clouds of about 43 000 points overlap little along the walk


def event_ms(fn):
    e0 = torch.cuda.Event(enable_timing=True); e1 = torch.cuda.Event(enable_timing=True)
    e0.record(); fn(); e1.record(); torch.cuda.synchronize()
    return e0.elapsed_time(e1)


def stats(t):
    return dict(ms_median=float(np.median(t)), ms_min=float(np.min(t)), ms_max=float(np.max(t)), reps=len(t))


def timed_consolidation(M, snapshot, reps, warm=3, budget_s=25.0):
    """the consolidation of the map `snapshot` (host records): restore, then time the launch sequence; returns (stats, record)"""
    t = []; t0 = time.perf_counter(); r = 0
    while r < warm + reps:
        M.reset(); M.append(snapshot)
        ms = event_ms(M.launch); r += 1
        if r > warm: t.append(ms)
        if len(t) >= 3 and time.perf_counter() - t0 > budget_s: break
    return stats(t), M.read()


def main():
    ap = argparse.ArgumentParser(); ap.add_argument('--reps', type=int, default=20); ap.add_argument('--out', default=None); ap.add_argument('--keyframes', type=int, default=64)
    ap.add_argument('--ab', action='store_true'); ap.add_argument('--trace-one', action='store_true')
    a = ap.parse_args()
    lib = sg_slam_amd.load(); n = a.keyframes
    out = {'device': torch.cuda.get_device_name(0), 'cloud_parameters': cc.TUM3_PARAMS, 'globalmap_parameters': GP, 'threshold': THRESHOLD, 'capacity': CAP, 'keyframes': n}
    depths, cols, boxes, have = bench_cloud.keyframes(); cam = cam_for(W, H)
    idx = [i % bench_cloud.SCENES for i in range(n)]
    d_dev = torch.from_numpy(depths[idx]).cuda(); c_dev = torch.from_numpy(cols[idx]).cuda(); bx = [boxes[i] for i in idx]; hv = [have[i] for i in idx]
    Twcs = np.stack([pose(rvec=(0.0, 0.021 * j, 0.0), t=(0.04 * j, 0.01 * j, 0.0)) for j in range(n)])      # a walk: 4 cm and 1.2 degrees a keyframe
    if not a.trace_one:                                                   # the yardstick: the parent's keyframe cloud, one keyframe, LOCAL mode (profiles/cloud_bench.json)
        B1 = PointCloudMappingBatch(cc.TUM3_PARAMS, W, H, cam, 1, cc.LOCAL, max_boxes=4, lib=lib)
        t = [event_ms(lambda: B1.launch(d_dev[:1], c_dev[:1], None, bx[:1], hv[:1])) for _ in range(3 + a.reps)][3:]
        kf = stats(t); kf['voxels'] = int(B1.read()[0][1]['n_voxels']); B1.close()
        out['keyframe_cloud'] = kf; print(json.dumps({'keyframe_cloud': kf}), flush=True)
    B = PointCloudMappingBatch(cc.TUM3_PARAMS, W, H, cam, n, cc.WORLD, max_boxes=4, lib=lib)
    B.launch(d_dev, c_dev, Twcs, bx, hv); torch.cuda.synchronize()
    M = GlobalMap(GP, CAP, lib=lib)
    rec_dev = torch.zeros(16, dtype=torch.uint8, device='cuda')
    off_n = CLOUD_RESULT_DTYPE.fields['n_points'][1]

    def append(j):                                                        # keyframe j straight from the batch's device buffers
        M.append_dev(B.points[j * B.N * CLOUD_POINT_DTYPE.itemsize:], B.N, B.results[j * CLOUD_RESULT_DTYPE.itemsize:], CLOUD_RESULT_DTYPE.itemsize, 1, rec_dev, n_points_offset_bytes=off_n)

    if a.trace_one:                                                       # one warm-up consolidation of one keyframe, then the walk
        append(0); M.launch(); torch.cuda.synchronize(); M.reset()
    t_app = []; cons = []; count = 0; largest = None
    for j in range(n):
        t_app.append(event_ms(lambda: append(j)))
        assert int(rec_dev.cpu().numpy().view('i4')[3]) == 0, 'keyframe %d does not fit into the map' % j
        last = j == n - 1
        if last or count > THRESHOLD:                                     # :342 with a keyframe always waiting, and the last keyframe with none
            if a.trace_one: M.launch(); torch.cuda.synchronize(); r = M.read()
            else:
                snap = M.points()
                s, r = timed_consolidation(M, snap, a.reps)
                if largest is None or len(snap) > len(largest): largest = snap
                c = dict(keyframe=j, map_points_in=int(r['n_points_in']), voxel_points=int(r['n_voxels']), map_points_out=int(r['n_points']), flags=int(r['flags']),
                         wider_window_points=int(r['wider_window_points']), whole_cloud_points=int(r['whole_cloud_points']), **s)
                c['us_per_voxel_point'] = 1e3 * s['ms_median'] / max(1, c['voxel_points'])
                c['ratio_to_keyframe_cloud_per_voxel_point'] = c['us_per_voxel_point'] / (1e3 * out['keyframe_cloud']['ms_median'] / out['keyframe_cloud']['voxels'])
                cons.append(c); print(json.dumps(c), flush=True)
            if int(r['n_points']): count = 0
        count += 1
    if a.trace_one: return
    out['append'] = dict(stats(t_app[3:]), keyframes_timed=len(t_app) - 3, points_per_keyframe_mean=float(np.mean([int(x['n_points']) for _, x in B.read()])))
    out['consolidations'] = cons; print(json.dumps({'append': out['append']}), flush=True)
    M.close(); B.close()
    if a.ab:
        T = SgxLib(os.path.join(ROOT, 'tests', 'taps', 'libsgx_taps.so')); MT = GlobalMap(GP, CAP, lib=T)
        r0 = 1
        while (2 * r0 + 1) ** 2 < 2 * (GP['mean_k'] + 1) and r0 < 5: r0 += 1
        ta, tb = [], []; ra = rb = None; t0 = time.perf_counter()
        for rep in range(2 + a.reps):
            for radius, tt in ((16, ta), (r0, tb)):
                MT.debug_max_radius(radius); MT.reset(); MT.append(largest)
                ms = event_ms(MT.launch)
                if rep >= 2: tt.append(ms)
                if radius == 16: ra = MT.read()
                else: rb = MT.read()
            if len(tb) >= 3 and time.perf_counter() - t0 > 60: break
        same = all(ra[k] == rb[k] for k in ('n_points_in', 'n_voxels', 'n_points', 'flags', 'mean', 'thr'))
        out['window_tier_ab'] = dict(map_points_in=int(ra['n_points_in']), voxel_points=int(ra['n_voxels']), first_window_radius=r0, tiers_as_built=stats(ta), max_radius_r0=stats(tb),
                                     wider_window_points=int(ra['wider_window_points']), whole_cloud_points_as_built=int(ra['whole_cloud_points']),
                                     whole_cloud_points_max_radius_r0=int(rb['whole_cloud_points']), same_result=bool(same))
        print(json.dumps({'window_tier_ab': out['window_tier_ab']}), flush=True); MT.close()
    if a.out: json.dump(out, open(a.out, 'w'), indent=1)


if __name__ == '__main__':
    main()
