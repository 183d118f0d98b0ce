"""Times InitializerBatch (the two-view initialisation of Tracking::MonocularInitialization) for one pair and for B = 512 pairs, N drawn from 100-400 matches, 200
iterations, half general scenes (F path) and half planar ones (H path); HIP events around the launch sequence alone (no read-back), median of the timed repetitions
after warm-up, and the per-kernel-class times of the library's profiler (sgx_profile_*) in a run of their own.  The kernel-logic emulator on one core times one pair
as the CPU stand-in.  Writes profiles/init_bench.json.
Usage: python tools/bench_init.py [--reps 20] [--out FILE.json]"""
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
import init_cases as ic
from sg_slam_amd.capi import SgxLib
from sg_slam_amd.initializer import Initializer, InitializerBatch


def scenes(B):
    rng = np.random.RandomState(11); ns = rng.randint(100, 401, B)
    kw = lambda b: (dict(seed=1000 + b, n=int(ns[b]), noise=0.2, outliers=0.1, unmatched=0.1) if b % 2 == 0 else
                    dict(seed=1000 + b, n=int(ns[b]), scene='planar', noise=0.2, baseline=1.0, tseed=64))
    return [ic.make_scene(**kw(b)) for b in range(B)], ns


def main():
    ap = argparse.ArgumentParser(); ap.add_argument('--reps', type=int, default=20); ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'init_bench.json'))
    a = ap.parse_args()
    lib = sg_slam_amd.load(); out = {'device': torch.cuda.get_device_name(0), 'iterations': 200, 'configs': []}
    for B in (1, 512):
        scs, ns = scenes(B)
        n1 = sum(len(s[0]) for s in scs); n2 = sum(len(s[1]) for s in scs)
        Bt = InitializerBatch(B, max(n1, n2), n1, 200, lib=lib)
        Bt.set([(s[0], s[1], s[2], ic.CAM) for s in scs])
        times = []
        for r in range(a.reps + 3):
            e0 = torch.cuda.Event(enable_timing=True); e1 = torch.cuda.Event(enable_timing=True)
            e0.record(); Bt.launch(rand_seeds=np.arange(B) + 1000 * r); e1.record(); torch.cuda.synchronize()
            if r >= 3: times.append(e0.elapsed_time(e1))
        lib.profile_read(reset=True); lib.profile_enable(True)
        for r in range(5): Bt.launch(rand_seeds=np.arange(B))
        torch.cuda.synchronize(); lib.profile_enable(False)
        prof = {k: v[0] / v[1] for k, v in lib.profile_read().items() if v[1] and k.startswith('init_')}
        res = Bt.run(rand_seeds=np.arange(B))
        med = float(np.median(times))
        out['configs'].append({'pairs': B, 'mean_N': float(ns.mean()), 'ms_median': med, 'ms_min': float(np.min(times)), 'ms_max': float(np.max(times)),
                               'pairs_per_s': B / (med * 1e-3), 'hypotheses_per_s': B * 2 * 200 / (med * 1e-3), 'ms_per_launch_by_kernel_class': prof,
                               'ok_h': sum(1 for x in res if x[0] and x[6]['model'] == 0), 'ok_f': sum(1 for x in res if x[0] and x[6]['model'] == 1)})
        print(json.dumps(out['configs'][-1]), flush=True)
        Bt.close()
    emu_so = os.path.join(ROOT, 'tests', 'emu', 'libsgx_emu.so')
    if os.path.exists(emu_so):
        emu = SgxLib(emu_so); scs, ns = scenes(1); s = scs[0]
        S = Initializer(s[0], ic.CAM, 1.0, 200, lib=emu)
        t0 = time.perf_counter(); S.Initialize(s[1], s[2]); dt = time.perf_counter() - t0
        out['emulator_one_core_one_pair_ms'] = dt * 1e3
        print(json.dumps({'emulator_one_core_one_pair_ms': dt * 1e3}))
    json.dump(out, open(a.out, 'w'), indent=1)


if __name__ == '__main__':
    main()
