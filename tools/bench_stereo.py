"""Times the stereo Frame constructor's device work (sg_slam_amd/stereo.py) with TUM-style ORB settings (1000 features, 8 levels / 1.2) at 640 x 480 and at 752 x 480
(EuRoC), for 1 and 64 pairs per batch: the stereo match alone (sgx_stereo_match_batch_dev), the extraction of the 2B images it follows, and both together.  HIP events
around the launch sequences alone (images on the device, no read-back), median of the timed repetitions after warm-up.  The figure to read the match against is the
extraction of the same run.  Pairs are slanted planes of smoothed random texture (tests/stereo_cases.py).
With --trace-one the tool runs one warmed-up batch and exits: under `rocprofv3 --kernel-trace --stats -- python tools/bench_stereo.py --trace-one 64` that gives the
kernels' shares.
Usage: python tools/bench_stereo.py [--reps 20] [--out FILE.json] [--pairs 1,64] [--trace-one N]"""
import argparse
import json
import os
import sys
import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, 'tests'))
import sg_slam_amd
import stereo_cases as sc
from sg_slam_amd.stereo import StereoFrameBatch

SCENES = 8
SIZES = ((640, 480), (752, 480))


def pairs(W, H):
    L, R = [], []
    for i in range(SCENES):
        T = sc.texture(H, W + 96, 500 + i)
        xr = np.arange(W)[None, :].astype(np.float64); y = np.arange(H)[:, None].astype(np.float64)
        L.append(T[:, :W].copy()); R.append(sc._sample(T, (xr + 2.0 + i + 0.004 * (i + 1) * y) / (1.0 - 0.005 * (i + 1))))
    return np.stack(L), np.stack(R)


def timed(fn, reps, warm):
    t = []
    for r in range(warm + reps):
        e0 = torch.cuda.Event(enable_timing=True); e1 = torch.cuda.Event(enable_timing=True)
        e0.record(); fn(); e1.record(); torch.cuda.synchronize()
        if r >= warm: t.append(e0.elapsed_time(e1))
    return float(np.median(t)), float(np.min(t)), float(np.max(t))


def main():
    ap = argparse.ArgumentParser(); ap.add_argument('--reps', type=int, default=20); ap.add_argument('--out', default=None); ap.add_argument('--pairs', default='1,64')
    ap.add_argument('--trace-one', type=int, default=0)
    a = ap.parse_args()
    lib = sg_slam_amd.load(); out = {'device': torch.cuda.get_device_name(0), 'orb': dict(nfeatures=1000, scaleFactor=1.2, nlevels=8), 'configs': []}
    for (W, H) in (SIZES[:1] if a.trace_one else SIZES):
        L, R = pairs(W, H)
        cam = dict(fx=0.8 * W, fy=0.8 * W, cx=W / 2, cy=H / 2, bf=0.08 * W)
        for B in ([a.trace_one] if a.trace_one else [int(v) for v in a.pairs.split(',')]):
            idx = [i % SCENES for i in range(B)]
            F = StereoFrameBatch(W, H, cam, batch=B, lib=lib)
            dl = torch.from_numpy(L[idx]).cuda(); dr = torch.from_numpy(R[idx]).cuda()
            s = torch.cuda.current_stream().cuda_stream; ex = F.extractor
            res = F(dl, dr); torch.cuda.synchronize()
            n = res['n'].cpu().numpy(); nm = res['nmatched'].cpu().numpy()

            def extract(): ex.extract_batch_dev(F.gray, F.pitch, 2 * B, F.keys, F.desc, F.n, stream=s)

            def match(): F.matcher.match_batch_dev(B, ex, 0, F.gray, F.pitch, ex, B, F.gray, F.pitch, F.keys, F.desc, F.n, F.keys[B:], F.desc[B:], F.n[B:], cam['fx'], cam['bf'],
                                                   F.uright, F.depth, F.nmatched, stream=s)

            def both(): extract(); match()
            if a.trace_one:
                both(); torch.cuda.synchronize(); F.close(); return
            rec = {'width': W, 'height': H, 'pairs': B, 'keys_mean': float(n.mean()), 'matched_mean': float(nm.mean())}
            for name, fn in (('extract_2B', extract), ('match', match), ('both', both)):
                med, lo, hi = timed(fn, a.reps, 3)
                rec[name + '_ms'] = med; rec[name + '_ms_min'] = lo; rec[name + '_ms_max'] = hi; rec[name + '_ms_per_pair'] = med / B
            rec['match_share_of_extraction'] = rec['match_ms'] / rec['extract_2B_ms']
            out['configs'].append(rec); print(json.dumps(rec), flush=True)
            F.close()
    if a.out: json.dump(out, open(a.out, 'w'), indent=1)


if __name__ == '__main__':
    main()
