"""Times Detector3DBatch (semantic objects from detector boxes and depth) with TUM3's parameters on 640 x 480 keyframes: a typical box of 120 x 180 (crop 72 x 108) and the largest crop there is, 384 x 288 cells,
of a box that is the whole image (Detector2D only clamps its boxes to the image), for 1, 64 and 512 jobs spread over 8 keyframes; HIP events around the launch sequence alone (no read-back), median of the timed
repetitions after warm-up.  The kernel-logic emulator on one core times one job of each box as the CPU stand-in (for scale only).
Usage: python tools/bench_obj3d.py [--reps 20] [--out FILE.json] [--jobs 1,64,512]"""
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
import obj3d_cases as oc
from sg_slam_amd.capi import SgxLib
from sg_slam_amd.detector3d import Detector3DBatch

W, H, IMAGES = 640, 480, 8
BOXES = {'typical_box_120x180': (260.0, 150.0, 120.0, 180.0), 'maximal_crop_384x288': (0.0, 0.0, 640.0, 480.0)}


def keyframes():
    depths = np.stack([oc.scene(100 + i, W, H, wall=(2.2 + 0.05 * i, 0.0006, 0.0003), boxes=[(250 + 3 * i, 160, 400, 330, 1.4, 0.0003)], noise=0.0005, outliers=40, holes=0.02)
                       for i in range(IMAGES)])
    return depths, np.stack([oc.pose((0.01 * i, -0.1, 0.03), (0.3, -0.2, 0.1 * i)) for i in range(IMAGES)])


def main():
    ap = argparse.ArgumentParser(); ap.add_argument('--reps', type=int, default=20); ap.add_argument('--out', default=None); ap.add_argument('--jobs', default='1,64,512')
    a = ap.parse_args()
    lib = sg_slam_amd.load(); out = {'device': torch.cuda.get_device_name(0), 'parameters': oc.TUM3_PARAMS, 'configs': []}
    depths, Twcs = keyframes(); cam = oc.cam_for(W, H)
    d_dev = torch.from_numpy(depths).cuda(); t_dev = torch.from_numpy(Twcs.reshape(IMAGES, 16)).cuda()
    for name, rect in BOXES.items():
        for J in [int(v) for v in a.jobs.split(',')]:
            B = Detector3DBatch(oc.TUM3_PARAMS, W, H, cam, IMAGES, J, lib=lib)
            jobs = [(i % IMAGES, (9, 0.8, rect)) for i in range(J)]
            times = []
            for r in range(a.reps + 3):
                e0 = torch.cuda.Event(enable_timing=True); e1 = torch.cuda.Event(enable_timing=True)
                e0.record(); B.launch(d_dev, t_dev, jobs); e1.record(); torch.cuda.synchronize()
                if r >= 3: times.append(e0.elapsed_time(e1))
            res = B.read(); med = float(np.median(times))
            out['configs'].append({'box': name, 'jobs': J, 'ms_median': med, 'ms_min': float(np.min(times)), 'ms_max': float(np.max(times)), 'ms_per_job': med / J,
                                   'crop_points_mean': float(res['crop_points'].mean()), 'found_fraction': float(res['found'].mean()),
                                   'larger_window_fraction': float(res['larger_window_points'].sum() / max(1, res['crop_points'].sum()))})
            print(json.dumps(out['configs'][-1]), flush=True)
            B.close()
    emu_so = os.path.join(ROOT, 'tests', 'emu', 'libsgx_emu.so')
    if os.path.exists(emu_so):
        emu = SgxLib(emu_so)
        for name, rect in BOXES.items():
            E = Detector3DBatch(oc.TUM3_PARAMS, W, H, cam, 1, 1, lib=emu)
            t0 = time.perf_counter(); E.detect(depths[:1], Twcs[:1], [(0, (9, 0.8, rect))]); dt = time.perf_counter() - t0
            out['emulator_one_core_ms_' + name] = dt * 1e3; E.close()
            print(json.dumps({'emulator_one_core_ms_' + name: dt * 1e3}))
    if a.out: json.dump(out, open(a.out, 'w'), indent=1)


if __name__ == '__main__':
    main()
