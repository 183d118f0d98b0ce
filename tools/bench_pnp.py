"""Times PnPsolverBatch (the EPnP RANSAC of Tracking::Relocalization) for frames x candidates = 1 x 16, 64 x 16, 512 x 16 solvers, N drawn from 15-300 with 30 % outliers,
the relocalisation parameters (0.99, 10, 300, 4, 0.5, 5.991); HIP events, median of the timed repetitions after warm-up.  A round = one iterate(5) of every solver on
fresh solvers (the first call runs up to mRansacMaxIts hypotheses), timed around the launch sequence alone (no read-back); a full relocalisation = rounds until every solver
has a model or bNoMore, with the read-back of each round (the caller needs it to decide).  The kernel-logic emulator on one core times one 1 x 16 round as the CPU stand-in.
Usage: python tools/bench_pnp.py [--reps 20] [--out FILE.json]"""
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
import pnp_cases as pc
from sg_slam_amd.capi import SgxLib
from sg_slam_amd.pnpsolver import PnPsolverBatch, RELOCALIZATION_RANSAC


def main():
    ap = argparse.ArgumentParser(); ap.add_argument('--reps', type=int, default=20); ap.add_argument('--out', default=None)
    a = ap.parse_args()
    lib = sg_slam_amd.load(); out = {'device': torch.cuda.get_device_name(0), 'configs': []}
    for frames in (1, 64, 512):
        B = frames * 16
        rng = np.random.RandomState(frames)
        ns = rng.randint(15, 301, B)
        data = [pc.make_case(b, int(ns[b]), 0.3)[:3] for b in range(B)]
        Bt = PnPsolverBatch(B, int(ns.sum()), lib=lib)
        times = []; hyps = []
        for r in range(a.reps + 3):
            Bt.set([(d[0], d[1], d[2], pc.CAM) for d in data], RELOCALIZATION_RANSAC, rand_seeds=np.arange(B) + 1000 * r)
            e0 = torch.cuda.Event(enable_timing=True); e1 = torch.cuda.Event(enable_timing=True)
            e0.record(); Bt.launch(5); e1.record(); torch.cuda.synchronize()          # the launch sequence alone: no read-back in the timed region
            res = Bt.result.cpu().numpy()
            if r >= 3: times.append(e0.elapsed_time(e1)); hyps.append(int(res[:, 3].sum()))
            if r == 3:                                                             # a full relocalisation: rounds of iterate(5) until every solver has a model or bNoMore
                Bt.set([(d[0], d[1], d[2], pc.CAM) for d in data], RELOCALIZATION_RANSAC, rand_seeds=np.arange(B) + 77)
                done = np.zeros(B, bool); rounds = 0; f0 = torch.cuda.Event(enable_timing=True); f1 = torch.cuda.Event(enable_timing=True); f0.record()
                while not done.all() and rounds < 100:
                    Bt.launch(5); rr = Bt.result.cpu().numpy(); done |= (rr[:, 0] != 0) | (rr[:, 1] != 0); rounds += 1
                f1.record(); torch.cuda.synchronize(); full_ms = f0.elapsed_time(f1); full_rounds = rounds
        med = float(np.median(times))
        out['configs'].append({'frames': frames, 'candidates': 16, 'solvers': B, 'mean_N': float(ns.mean()), 'ms_per_round_median': med,
                               'ms_full_relocalisation': full_ms, 'rounds_full_relocalisation': full_rounds,
                               'ms_min': float(np.min(times)), 'ms_max': float(np.max(times)), 'hypotheses_per_round': float(np.mean(hyps)),
                               'hypotheses_per_s': float(np.mean(hyps)) / (med * 1e-3), 'found_fraction': float(res[:, 0].mean())})
        print(json.dumps(out['configs'][-1]), flush=True)
        Bt.close()
    emu_so = os.path.join(ROOT, 'tests', 'emu', 'libsgx_emu.so')
    if os.path.exists(emu_so):
        emu = SgxLib(emu_so); rng = np.random.RandomState(1); ns = rng.randint(15, 301, 16)
        data = [pc.make_case(b, int(ns[b]), 0.3)[:3] for b in range(16)]
        Bt = pc.batch_for(emu, 16, int(ns.sum())); Bt.set([(d[0], d[1], d[2], pc.CAM) for d in data], RELOCALIZATION_RANSAC, rand_seeds=np.arange(16))
        t0 = time.perf_counter(); res, T, inl = Bt.iterate(5); dt = time.perf_counter() - t0
        out['emulator_one_core_1x16_ms'] = dt * 1e3; out['emulator_hypotheses'] = int(res[:, 3].sum())
        print(json.dumps({'emulator_one_core_1x16_ms': dt * 1e3}))
    if a.out: json.dump(out, open(a.out, 'w'), indent=1)


if __name__ == '__main__':
    main()
