"""Times KeyFrameDatabase.detect_batch_dev (the candidate search of Tracking::Relocalization and LoopClosing::DetectLoop) for N = 256, 2 048, 8 192 keyframes of about
600 words (100 000-word vocabulary, the "places" generator of tests/kfdb_cases.py) and Q = 1, 64, 512 queries per batch, both modes; HIP events around the launch
sequence alone (queries resident on the device, no read-back), median of the timed repetitions after warm-up.  A relocalisation batch changes mRelocScore, so every
repetition starts from the state the previous one left: the work per repetition is the same.
Usage: python tools/bench_kfdb.py [--reps 20] [--out profiles/kfdb_bench.json] [--kernel-stats]
--kernel-stats runs one configuration (N = 2 048, Q = 64, both modes) a few times and nothing else, for a separate profiler run of its own:
    rocprofv3 --kernel-trace --stats -d /tmp/kfdb_prof -- python tools/bench_kfdb.py --kernel-stats      (the *_kernel_stats.csv it writes -> profiles/kfdb_kernel_stats.csv)"""
import argparse
import ctypes as C
import json
import os
import sys
import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, 'tests'))
import sg_slam_amd
import kfdb_cases as kc
from sg_slam_amd.capi import _vp, KFDB_REPORT_DTYPE
from sg_slam_amd.keyframedatabase import KeyFrameDatabase, RELOCALIZATION, LOOP_CLOSING

NWORDS = 100000


def database(lib, N, max_queries):
    case = kc.places_script(N, RELOCALIZATION, N=N, nwords=NWORDS, places=max(N // 32, 1), per_place=1500, nq=512, lo=550, hi=650)
    adds = [o for o in case['ops'] if o[0] == 'add']
    voc = kc.make_voc(lib, NWORDS)
    D = KeyFrameDatabase(voc, max_keyframes=N, max_bow_entries=sum(len(o[2][0]) for o in adds), max_query_words=1024, max_queries=max_queries)
    for op in case['ops']:
        if op[0] == 'add': D.add(op[1], op[2])
        elif op[0] == 'cov': D.set_covisibility(op[1], op[2])
    queries = [o[1] for o in case['ops'] if o[0] == 'reloc'][:512]
    ids = [o[1] for o in adds]
    return voc, D, queries, ids, float(np.mean([len(o[2][0]) for o in adds]))


def resident(D, queries, Q):
    pitch = max(len(b[0]) for b in queries[:Q])
    ids = np.zeros((Q, pitch), 'i4'); w = np.zeros((Q, pitch), 'f8'); cnt = np.zeros(Q, 'i4')
    for q, b in enumerate(queries[:Q]): ids[q, :len(b[0])] = b[0]; w[q, :len(b[0])] = b[1]; cnt[q] = len(b[0])
    return D._dev(ids), D._dev(w), pitch, D._dev(cnt)


def time_config(D, queries, kf_ids, Q, mode, reps):
    """the C entry alone between the events: every array it takes is resident before the first repetition"""
    d_ids, d_w, pitch, d_cnt = resident(D, queries, Q)
    rng = np.random.RandomState(Q)
    conn_off = conn_ids = ms = None
    if mode == LOOP_CLOSING:
        conn = [rng.choice(kf_ids, min(len(kf_ids), 20), replace=False) for _ in range(Q)]
        conn_off = D._dev(np.arange(Q + 1, dtype='i4') * len(conn[0])); conn_ids = D._dev(np.concatenate(conn).astype('i4')); ms = D._dev(np.full(Q, 0.02, 'f4'))
    cand = D._dev(np.zeros((Q, D.max_keyframes), 'i4')); ncand = D._dev(np.zeros(Q, 'i4')); rep = D._dev(np.zeros(Q * KFDB_REPORT_DTYPE.itemsize, 'u1'))
    stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    times = []
    for r in range(reps + 3):
        e0 = torch.cuda.Event(enable_timing=True); e1 = torch.cuda.Event(enable_timing=True)
        e0.record()
        D.lib.check(D.lib.dll.sgx_kfdb_detect_batch_dev(D.h, mode, Q, _vp(d_ids), _vp(d_w), pitch, _vp(d_cnt), _vp(conn_off), _vp(conn_ids), _vp(ms), _vp(cand), _vp(ncand), _vp(rep),
                                                        None, None, stream), 'sgx_kfdb_detect_batch_dev')
        e1.record(); torch.cuda.synchronize()
        if r >= 3: times.append(e0.elapsed_time(e1))
    return dict(ms_per_batch_median=float(np.median(times)), ms_min=float(np.min(times)), ms_max=float(np.max(times)), candidates_per_query=float(ncand.cpu().numpy().mean()))


def main():
    ap = argparse.ArgumentParser(); ap.add_argument('--reps', type=int, default=20); ap.add_argument('--out', default=None); ap.add_argument('--kernel-stats', action='store_true')
    a = ap.parse_args()
    lib = sg_slam_amd.load(); out = {'device': torch.cuda.get_device_name(0), 'nwords': NWORDS, 'configs': []}
    sizes, batches, reps = ((2048,), (64,), 3) if a.kernel_stats else ((256, 2048, 8192), (1, 64, 512), a.reps)
    for N in sizes:
        voc, D, queries, kf_ids, mean_words = database(lib, N, max(batches))
        for Q in batches:
            for mode, name in ((RELOCALIZATION, 'relocalization'), (LOOP_CLOSING, 'loop')):
                r = dict(keyframes=N, mean_words=mean_words, queries=Q, mode=name, **time_config(D, queries, kf_ids, Q, mode, reps))
                r['us_per_query'] = 1e3 * r['ms_per_batch_median'] / Q
                out['configs'].append(r); print(json.dumps(r), flush=True)
        D.close(); voc.close()
    if a.out: json.dump(out, open(a.out, 'w'), indent=1)


if __name__ == '__main__':
    main()
