"""Cost of lens distortion in the tracker: TrackerNative (detector + dynamic mask, as bench.py's plain run) at S streams on the bench's synthetic
scene, without distortion and with TUM1.yaml's coefficients (Frame::UndistortKeyPoints fused into the stereo-from-RGBD kernel), alternating the two
configurations so that host noise lands on both.  Prints one JSON line: ms per step of each run and the difference of the medians.

    python tools/bench_distortion.py [--streams 512] [--steps 60] [--warmup 8] [--reps 2] [--out FILE]
"""
import argparse
import json
import os
import sys
import time
import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--streams', type=int, default=512)
    ap.add_argument('--steps', type=int, default=60)
    ap.add_argument('--warmup', type=int, default=8)
    ap.add_argument('--reps', type=int, default=2, help='timed runs of each configuration, alternating')
    ap.add_argument('--frames', type=int, default=6, help='distinct frames per stream (ping-pong replay, as bench.py)')
    ap.add_argument('--distinct', type=int, default=32, help='distinct stream offsets rendered; the streams cycle through them')
    ap.add_argument('--out', default='')
    args = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        print('bench_distortion.py needs a GPU', file=sys.stderr); sys.exit(2)
    import sg_slam_amd
    from sg_slam_amd import synth, settings
    from sg_slam_amd.detector import Detector2D
    from sg_slam_amd.tracker_native import TrackerNative
    lib = sg_slam_amd.load()
    cam = dict(synth.TUM3)
    dist = settings.load(os.path.join(ROOT, 'tests', 'golden', 'settings', 'TUM1.yaml'))['dist']
    S, T = args.streams, args.frames
    gen = synth.LayeredStream(seed=1234)
    offs = [37 * i for i in range(args.distinct)]
    fr = [[gen.frame(o + t)[:2] for t in range(T)] for o in offs]
    idx = [s % len(offs) for s in range(S)]
    gray = [torch.from_numpy(np.stack([fr[i][t][0] for i in idx])).cuda() for t in range(T)]
    depth = [torch.from_numpy(np.stack([fr[i][t][1] for i in idx]).view(np.int16)).cuda() for t in range(T)]
    bgr = [g.unsqueeze(-1).expand(S, 480, 640, 3).contiguous() for g in gray]
    order = list(range(T)) + list(range(T - 2, 0, -1))             # ping-pong
    T0 = np.stack([gen.Tcw(offs[i]) for i in idx])
    param = os.path.join(ROOT, 'tests', 'golden', 'mobilenetv3_ssdlite_voc.param')
    layers = synth.parse_ncnn_param(param)
    _, blob = synth.synth_ncnn_weights(layers, seed=7, person_logit=-0.5)
    param_text = open(param).read()

    def run(d):
        det = Detector2D(0.9, 0.01, param_text=param_text, bin_bytes=blob, max_batch=S, lib=lib)
        tr = TrackerNative(lib, S, cam, dynamic_mask=True, detector=det, dist=d)
        tr.set_initial_pose(T0)
        st = torch.cuda.current_stream().cuda_stream
        for k in range(args.warmup):
            j = order[k % len(order)]; tr.step(gray[j], depth[j], d_bgr=bgr[j], stream=st)
        tr.synchronize(); torch.cuda.synchronize()
        t0 = time.perf_counter()
        for k in range(args.steps):
            j = order[(args.warmup + k) % len(order)]; tr.step(gray[j], depth[j], d_bgr=bgr[j], stream=st)
        tr.synchronize(); torch.cuda.synchronize()
        ms = (time.perf_counter() - t0) * 1e3 / args.steps
        r = tr.read(); tr.close()
        return ms, int(r['nkeys'].sum()), int(r['ninl2'].sum()), tr.bounds

    res = {'plain': [], 'tum1': []}
    info = {}
    for rep in range(args.reps):
        for name, d in (('plain', None), ('tum1', dist)):
            ms, nk, ni, b = run(d)
            res[name].append(round(ms, 3)); info[name] = dict(nkeys=nk, ninl2=ni, bounds=b)
    med = {k: float(np.median(v)) for k, v in res.items()}
    line = dict(metric='tracker ms/step with and without lens distortion', streams=S, steps=args.steps, warmup=args.warmup, ms_per_step=res,
                median=med, delta_ms=round(med['tum1'] - med['plain'], 3), last_step=info, version=lib.version())
    s = json.dumps(line)
    print(s)
    if args.out:
        with open(args.out, 'w') as f: f.write(s + '\n')


if __name__ == '__main__':
    main()
