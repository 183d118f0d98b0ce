"""Times LocalMapping::CreateNewMapPoints over the keyframe store (sgx_create_new_map_points_batch_dev): one keyframe of about 1000 keypoints with 10 neighbours, as
Q = 1, 8 and 64 independent queries of one launch.  HIP events around the launch alone (everything resident, the in/out rows restored before each repetition outside the
events, no read-back), median of the timed repetitions after 3 warm-up runs, min / max kept.  Beside it, in the same run, the same work through the chain of the
single-pair entries it replaces: per neighbour the baseline gate and F12 in numpy, sgx_match_search_for_triangulation, sgx_triangulate_new_map_points and the row
updates, as host wall-clock ending in the entries' own blocking read-backs (median of 5 runs), and whether both create the same points.
The scene: a wall of 1400 points 3 to 6 m away, keyframes 0.45 m apart each seeing a seeded 1000 of them (stereo projections with 0.15 px noise, up to 10 flipped
descriptor bits per observation, node = a hash of the point index modulo 97, one keypoint in five monocular), half of the points in the map already.
bench.py does not call this feature.
Usage: python tools/bench_newpoints.py [--reps 20] [--out profiles/newpoints_bench.json] [--kernel-stats]
--kernel-stats runs the batch of one a few times and nothing else, for a profiler run of its own:
    rocprofv3 --kernel-trace --stats --output-format csv -d /tmp/np_prof -- python tools/bench_newpoints.py --kernel-stats"""
import argparse
import json
import os
import sys
import time
import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import sg_slam_amd
from sg_slam_amd import mappoint, synth
from sg_slam_amd.capi import KP_DTYPE, NEWPOINTS_REPORT_DTYPE
from sg_slam_amd.keyframestore import KeyFrameStore
from sg_slam_amd.localmapping import camera_centre
from sg_slam_amd.matcher import ORBmatcher

CAM = dict(synth.TUM3)
NL = 8
SF = (1.2 ** np.arange(NL)).astype('f4'); SG = (SF * SF).astype('f4')
NPTS, PER, NNB, STEP = 1400, 1000, 10, 0.45


def scene(seed=0):
    rng = np.random.RandomState(seed)
    X = np.stack([rng.uniform(-1.5, 1.5, NPTS), rng.uniform(-1.0, 1.0, NPTS), rng.uniform(3.0, 6.0, NPTS)], 1)
    base = rng.randint(0, 256, (NPTS, 32)).astype(np.uint8); node = ((np.arange(NPTS) * 2654435761 >> 7) % 97).astype('i4'); exists = rng.rand(NPTS) < 0.5
    kfs = {}; rows = {}
    for t in range(NNB + 1):
        ids = np.sort(rng.choice(NPTS, PER, replace=False)); c = X[ids] - np.array([STEP * (t - NNB // 2), 0.02 * t, 0.0])
        k = np.zeros(PER, KP_DTYPE)
        k['x'] = CAM['fx'] * c[:, 0] / c[:, 2] + CAM['cx'] + rng.normal(0, 0.15, PER); k['y'] = CAM['fy'] * c[:, 1] / c[:, 2] + CAM['cy'] + rng.normal(0, 0.15, PER)
        k['size'] = 31; k['octave'] = np.clip(np.floor(np.log(c[:, 2] / 3.0) / np.log(1.2)), 0, NL - 1)
        z = c[:, 2].astype('f4'); ur = (k['x'] - CAM['bf'] / z).astype('f4'); mono = rng.rand(PER) < 0.2; ur[mono] = -1; z[mono] = -1
        flip = rng.rand(PER, 256) < (rng.randint(0, 11, (PER, 1)) / 256.0)
        d = np.packbits(np.unpackbits(base[ids], axis=1) ^ flip.astype(np.uint8), axis=1)
        T = np.eye(4, dtype='f4'); T[0, 3] = -STEP * (t - NNB // 2); T[1, 3] = -0.02 * t
        kfs[t] = dict(keys_un=k, desc=d, uright=ur, depth=z, feat_node=node[ids], Tcw=T)
        rows[t] = np.where(exists[ids] & (rng.rand(PER) < 0.6), ids, -1).astype('i4')
    cur = NNB // 2
    nbs = sorted([t for t in kfs if t != cur], key=lambda t: abs(t - cur))
    return kfs, rows, cur, nbs


def f12_numpy(T1, T2):
    K = np.array([[CAM['fx'], 0, CAM['cx']], [0, CAM['fy'], CAM['cy']], [0, 0, 1.0]])
    R1, t1, R2, t2 = T1[:3, :3].astype('f8'), T1[:3, 3].astype('f8'), T2[:3, :3].astype('f8'), T2[:3, 3].astype('f8')
    R12 = R1 @ R2.T; t12 = -R12 @ t2 + t1
    tx = np.array([[0, -t12[2], t12[1]], [t12[2], 0, -t12[0]], [-t12[1], t12[0], 0]])
    return (np.linalg.inv(K).T @ tx @ R12 @ np.linalg.inv(K)).astype('f4')


def chain(lib, kfs, rows, cur, nbs, first):
    """the loop a caller writes without the new entry: one keyframe pair at a time through the host-pointer entries"""
    m = ORBmatcher(0.6, False, lib=lib); a = kfs[cur]; row1 = rows[cur].copy(); Ow1 = camera_centre(a['Tcw']); mb = CAM['bf'] / CAM['fx']; new = []
    for kf2 in nbs:
        b = kfs[kf2]; Ow2 = camera_centre(b['Tcw'])
        if np.linalg.norm(Ow2 - Ow1) < mb: continue
        F12 = f12_numpy(a['Tcw'], b['Tcw']); row2 = rows[kf2].copy()
        k1 = dict(keys=a['keys_un'], desc=a['desc'], uright=a['uright'], has_mp=(row1 >= 0).astype(np.uint8), feat_node=a['feat_node'], cam_center=Ow1)
        k2 = dict(keys=b['keys_un'], desc=b['desc'], uright=b['uright'], has_mp=(row2 >= 0).astype(np.uint8), feat_node=b['feat_node'], Tcw=b['Tcw'])
        _, pairs = m.SearchForTriangulation(k1, k2, F12, False, CAM, SF, SG)
        _, ok, x = mappoint.TriangulateNewMapPoints(pairs, a, b, CAM, SF, SG, lib=lib)
        for (i1, i2), good in zip(pairs, ok):
            if good: row1[i1] = first + len(new); new.append((kf2, int(i1), int(i2)))
    return new


def main():
    ap = argparse.ArgumentParser(); ap.add_argument('--reps', type=int, default=20); ap.add_argument('--out', default=None); ap.add_argument('--kernel-stats', action='store_true')
    a = ap.parse_args()
    lib = sg_slam_amd.load()
    kfs, rows, cur, nbs = scene()
    S = KeyFrameStore(CAM, SF, SG, max_keyframes=16, cap=1024, lib=lib)
    for t, d in kfs.items(): S.add(t, d['keys_un'], d['desc'], d['uright'], d['depth'], d['feat_node'], d['Tcw'])
    out = {'device': torch.cuda.get_device_name(0), 'keypoints': PER, 'neighbours': NNB, 'store_bytes': S.info()[0], 'configs': []}
    for Q in ((1,) if a.kernel_stats else (1, 8, 64)):
        qs = [(cur, nbs, [rows[cur]] + [rows[k] for k in nbs], 100000 * (q + 1), None) for q in range(Q)]
        h = S.batch_buffers(qs, pairs=False)
        d = [None if x is None else torch.from_numpy(x).cuda() for x in h]
        rows0 = d[5].clone(); times = []
        for r in range((a.reps if not a.kernel_stats else 5) + 3):
            d[5].copy_(rows0); torch.cuda.synchronize()
            e0 = torch.cuda.Event(enable_timing=True); e1 = torch.cuda.Event(enable_timing=True)
            e0.record(); S.create_new_map_points_batch_dev(Q, *d); e1.record(); torch.cuda.synchronize()
            if r >= 3: times.append(e0.elapsed_time(e1))
        n_new = d[6].cpu().numpy(); rep = d[15].cpu().numpy().view(NEWPOINTS_REPORT_DTYPE)
        assert (n_new == n_new[0]).all() and n_new[0] > 0
        cfg = dict(entry='create_new_map_points_batch_dev', queries=Q, ms_median=float(np.median(times)), ms_min=float(np.min(times)), ms_max=float(np.max(times)),
                   new_points_per_query=int(n_new[0]), pairs_per_query=int(rep['n_pairs'][:NNB].sum()), neighbours_processed=int((rep['status'][:NNB] == 0).sum()))
        if Q == 1 and not a.kernel_stats:
            dev_new = list(zip(d[7][0, :n_new[0]].cpu().tolist(), d[8][0, :n_new[0]].cpu().tolist(), d[9][0, :n_new[0]].cpu().tolist()))
            host = []
            for r in range(5 + 1):
                t0 = time.perf_counter(); got = chain(lib, kfs, rows, cur, nbs, 100000); t1 = time.perf_counter()
                if r: host.append((t1 - t0) * 1e3)
            cfg.update(ms_chain_of_single_pair_entries=float(np.median(host)), chain_runs=5, chain_creates_the_same_points=bool(got == dev_new),
                       chain_over_batch_of_one=float(np.median(host) / np.median(times)))
            t0 = time.perf_counter(); S.create_new_map_points(*qs[0]); cfg['ms_host_form_wall'] = float((time.perf_counter() - t0) * 1e3)
        out['configs'].append(cfg); print(json.dumps(cfg))
    S.close()
    if a.out:
        with open(a.out, 'w') as f: json.dump(out, f, indent=1)


if __name__ == '__main__':
    main()
