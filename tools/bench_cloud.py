"""Times PointCloudMappingBatch (the filtered local-map cloud of a keyframe: every pixel as a point, VoxelGrid, StatisticalOutlierRemoval, the axis map) with TUM3's
parameters on 640 x 480 keyframes, for 1, 16 and 64 keyframes per batch; HIP events around the launch sequence alone (inputs on the device, no read-back), median of
the timed repetitions after warm-up.  The kernel-logic emulator on one core times one keyframe as the CPU stand-in (for scale only).
With --trace-one the tool runs one warmed-up batch and exits: under `rocprofv3 --kernel-trace --stats -- python tools/bench_cloud.py --trace-one 16` that gives the
kernels' shares.
Usage: python tools/bench_cloud.py [--reps 20] [--out FILE.json] [--keyframes 1,16,64] [--trace-one N]"""
import argparse
import json
import os
import sys
import time
import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, 'tests'))
import sg_slam_amd
import cloud_cases as cc
from obj3d_cases import scene, cam_for
from sg_slam_amd.capi import SgxLib
from sg_slam_amd.pointcloudmapping import PointCloudMappingBatch

W, H, SCENES = 640, 480, 8


def keyframes():
    """eight scenes (a wall, an object, noise, holes), every second one with a person box"""
    depths = np.stack([scene(200 + i, W, H, wall=(1.7 + 0.05 * i, 0.0006, 0.0003), boxes=[(250 + 3 * i, 160, 400, 330, 1.3, 0.0003)], noise=0.0005, outliers=40, holes=0.02)
                       for i in range(SCENES)])
    cols = np.stack([cc.colors(200 + i, W, H) for i in range(SCENES)])
    boxes = [[(280.5, 100.25, 150.0, 350.5)] if i % 2 else [] for i in range(SCENES)]
    return depths, cols, boxes, [i % 2 for i in range(SCENES)]


def main():
    ap = argparse.ArgumentParser(); ap.add_argument('--reps', type=int, default=20); ap.add_argument('--out', default=None); ap.add_argument('--keyframes', default='1,16,64')
    ap.add_argument('--trace-one', type=int, default=0)
    a = ap.parse_args()
    lib = sg_slam_amd.load(); out = {'device': torch.cuda.get_device_name(0), 'parameters': cc.TUM3_PARAMS, 'configs': []}
    depths, cols, boxes, have = keyframes(); cam = cam_for(W, H)
    for n in ([a.trace_one] if a.trace_one else [int(v) for v in a.keyframes.split(',')]):
        idx = [i % SCENES for i in range(n)]
        B = PointCloudMappingBatch(cc.TUM3_PARAMS, W, H, cam, n, cc.LOCAL, max_boxes=4, lib=lib)
        d_dev = torch.from_numpy(depths[idx]).cuda(); c_dev = torch.from_numpy(cols[idx]).cuda()
        bx = [boxes[i] for i in idx]; hv = [have[i] for i in idx]
        times = []
        for r in range(2 if a.trace_one else a.reps + 3):
            e0 = torch.cuda.Event(enable_timing=True); e1 = torch.cuda.Event(enable_timing=True)
            e0.record(); B.launch(d_dev, c_dev, None, bx, hv); e1.record(); torch.cuda.synchronize()
            if a.trace_one or r >= 3: times.append(e0.elapsed_time(e1))
        res = B.read(); med = float(np.median(times)); rec = np.array([r for _, r in res])
        out['configs'].append({'keyframes': n, 'ms_median': med, 'ms_min': float(np.min(times)), 'ms_max': float(np.max(times)), 'ms_per_keyframe': med / n,
                               'voxels_mean': float(rec['n_voxels'].mean()), 'points_mean': float(rec['n_points'].mean()),
                               'larger_window_fraction': float(rec['larger_window_points'].sum() / max(1, rec['n_voxels'].sum()))})
        print(json.dumps(out['configs'][-1]), flush=True)
        B.close()
    emu_so = os.path.join(ROOT, 'tests', 'emu', 'libsgx_emu.so')
    if os.path.exists(emu_so) and not a.trace_one:
        E = PointCloudMappingBatch(cc.TUM3_PARAMS, W, H, cam, 1, cc.LOCAL, max_boxes=4, lib=SgxLib(emu_so))
        t0 = time.perf_counter(); E.build(depths[:1], cols[:1], None, boxes[:1], have[:1]); dt = time.perf_counter() - t0
        out['emulator_one_core_ms_per_keyframe'] = dt * 1e3; E.close()
        print(json.dumps({'emulator_one_core_ms_per_keyframe': dt * 1e3}))
    if a.out: json.dump(out, open(a.out, 'w'), indent=1)


if __name__ == '__main__':
    main()
