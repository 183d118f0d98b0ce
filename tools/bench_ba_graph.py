"""Times the bundle-adjustment graph query of the covisibility handle (sgx_covis_ba_graph_batch_dev) on the map of tools/bench_covis.py: 500 keyframes of 1 000 points (a
camera walking along a wall of points, keyframe t sees 1 000 of the 1 300 points in front of it, 26 points further on than keyframe t - 1; about 95 listed neighbours).
Local mode at Q = 1 and Q = 64, global mode once, the problem sizes, and in the same run the two figures to read them against: sgx_covis_local_map_batch_dev at the same
Q, and sgx_local_bundle_adjustment (host wall-clock, one run) on the problem the Q = 1 query produced.  HIP events around the launch sequence alone (everything resident,
no read-back), median of the timed repetitions after 3 warm-up runs, min / max kept.  bench.py does not call this feature.
Usage: python tools/bench_ba_graph.py [--reps 20] [--out profiles/ba_graph_bench.json] [--kernel-stats]
--kernel-stats runs the local mode at Q = 64 and the global mode a few times and nothing else, for a separate profiler run of its own:
    rocprofv3 --kernel-trace --stats --output-format csv -d /tmp/ba_graph_prof -- python tools/bench_ba_graph.py --kernel-stats   (its *_kernel_stats.csv -> profiles/ba_graph_kernel_stats.csv)"""
import argparse
import ctypes as C
import json
import os
import sys
import time
import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tools'))
import sg_slam_amd
from sg_slam_amd.capi import _vp, COVIS_REPORT_DTYPE, COVIS_BA_REPORT_DTYPE
from sg_slam_amd.covisibility import CovisibilityGraph
from sg_slam_amd.optimizer import Optimizer
from bench_covis import timed, world, PER, WIN, STEP, CAP

NKF, PCAP, ECAP, MCAP = 500, 8192, 1 << 18, 8192
CAM = dict(fx=500.0, fy=500.0, cx=320.0, cy=240.0, bf=40.0)


def main():
    ap = argparse.ArgumentParser(); ap.add_argument('--reps', type=int, default=20); ap.add_argument('--out', default=None); ap.add_argument('--kernel-stats', action='store_true')
    a = ap.parse_args()
    lib = sg_slam_amd.load(); dev = 'cuda'
    out = {'device': torch.cuda.get_device_name(0), 'keyframes': NKF, 'points_per_keyframe': PER, 'configs': []}
    rng = np.random.RandomState(0)
    npts = STEP * NKF + WIN
    xw, _ = world(npts, rng)
    G = CovisibilityGraph(max_keyframes=512, cap=CAP, max_points=npts, max_observations=512 * PER, max_queries=64, lib=lib)
    KF = {}
    for t in range(NKF):                                                       # the walk of bench_covis.grow, the keypoints kept for the flattening
        o = rng.randint(0, 8, PER).astype('i4'); seen = (t * STEP + rng.choice(WIN, PER, replace=False)).astype('i4')
        x0 = 0.02 * (t * STEP + WIN // 2); z = xw[seen, 2]
        uv = np.stack([CAM['fx'] * (xw[seen, 0] - x0) / z + CAM['cx'], CAM['fy'] * xw[seen, 1] / z + CAM['cy']], 1) + rng.randn(PER, 2) * 0.5
        ur = np.where(rng.rand(PER) < 0.3, uv[:, 0] - CAM['bf'] / z, -1.0).astype('f4')
        T = np.eye(4, dtype='f4'); T[0, 3] = -x0
        KF[t] = dict(Tcw=T, uv=uv.astype('f4'), uright=ur)
        G.add_keyframe(t, o, ur, z.astype('f4')); G.set_observations(t, np.arange(PER, dtype='i4'), seen)
    ids = np.arange(NKF, dtype='i4')
    for at in range(0, NKF, 64): G.update_connections(ids[at:at + 64])
    out['observations'] = G.info()[2]
    out['mean_ordered'] = float(np.mean([len(G.ordered(int(k))[0]) for k in ids[::25]]))
    stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    i32 = dict(dtype=torch.int32, device=dev); u8 = dict(dtype=torch.uint8, device=dev)

    def rows(Q, pcap, ecap):
        return dict(pid=torch.zeros((Q, 512), **i32), pf=torch.zeros((Q, 512), **u8), pts=torch.zeros((Q, pcap), **i32), beg=torch.zeros((Q, pcap + 1), **i32),
                    ep=torch.zeros((Q, ecap), **i32), el=torch.zeros((Q, ecap), **i32), ek=torch.zeros((Q, ecap), **i32), ea=torch.zeros((Q, ecap), **u8),
                    rep=torch.zeros(Q * COVIS_BA_REPORT_DTYPE.itemsize, **u8))

    def ba_graph(Q, mode, kq, d, pcap, ecap):
        lib.check(lib.dll.sgx_covis_ba_graph_batch_dev(G.h, Q, mode, _vp(kq), _vp(d['pid']), _vp(d['pf']), pcap, _vp(d['pts']), _vp(d['beg']), ecap, _vp(d['ep']), _vp(d['el']),
                                                       _vp(d['ek']), _vp(d['ea']), _vp(d['rep']), stream), 'sgx_covis_ba_graph_batch_dev')

    reps = 3 if a.kernel_stats else a.reps
    for Q in ((64,) if a.kernel_stats else (1, 64)):
        kq = torch.from_numpy(np.linspace(60, NKF - 60, Q).astype('i4')).to(dev)
        d = rows(Q, PCAP, ECAP)
        r = dict(entry='ba_graph_local', queries=Q, **timed(lambda: ba_graph(Q, 0, kq, d, PCAP, ECAP), reps))
        rep = d['rep'].cpu().numpy().view(COVIS_BA_REPORT_DTYPE)
        assert (rep['status'] == 0).all(), rep
        for k in ('n_local_kf', 'n_fixed_kf', 'n_poses', 'n_points', 'n_edges'): r[k + '_mean'] = float(rep[k].mean())
        out['configs'].append(r); print(json.dumps(r), flush=True)
        if a.kernel_stats: continue
        # the figure to read it against: UpdateLocalMap of Q frames that track 500 points of the same keyframes
        kqh = kq.cpu().numpy()
        frames = np.stack([(int(k) * STEP + rng.choice(WIN, 500, replace=False)).astype('i4') for k in kqh])
        f = dict(frame=torch.from_numpy(frames).to(dev), n=torch.full((Q,), 500, **i32), mo=torch.zeros(Q, **i32), lkf=torch.full((Q, 512), -1, **i32), nlkf=torch.zeros(Q, **i32),
                 ref=torch.full((Q,), -1, **i32), rt=torch.zeros(Q, **i32), pts=torch.zeros((Q, MCAP), **i32), obs=torch.zeros((Q, MCAP), **i32), npts=torch.zeros(Q, **i32),
                 rep=torch.zeros(Q * COVIS_REPORT_DTYPE.itemsize, **u8))
        def local_map():
            lib.check(lib.dll.sgx_covis_local_map_batch_dev(G.h, Q, 500, _vp(f['frame']), _vp(f['n']), _vp(f['mo']), _vp(f['lkf']), _vp(f['nlkf']), _vp(f['ref']), _vp(f['rt']), MCAP,
                                                            _vp(f['pts']), _vp(f['obs']), _vp(f['npts']), _vp(f['rep']), stream), 'sgx_covis_local_map_batch_dev')
        m = dict(entry='local_map', queries=Q, **timed(local_map, reps))
        lrep = f['rep'].cpu().numpy().view(COVIS_REPORT_DTYPE)
        assert (lrep['status'] == 0).all(), lrep['status']
        m['local_keyframes_mean'] = float(lrep['n_local_kf'].mean()); m['local_points_mean'] = float(lrep['n_local_points'].mean())
        m['ba_graph_over_local_map'] = r['ms_median'] / m['ms_median']
        out['configs'].append(m); print(json.dumps(m), flush=True)
        if Q == 1:
            # the consumer: the solver on the problem this query produced (host pointers, one run, wall clock)
            g = G.local_ba_graph(int(kqh[0]), PCAP, ECAP)
            prob = Optimizer.flatten_ba_problem(g, KF, xw, (1.0 / 1.2 ** (2 * np.arange(8))).astype('f4'))
            torch.cuda.synchronize(); t0 = time.perf_counter()
            erase, st = Optimizer.LocalBundleAdjustment(prob, CAM, lib=lib)
            s = dict(entry='local_bundle_adjustment', ms_wall=1e3 * (time.perf_counter() - t0), poses=len(prob['poses']), points=len(prob['points']), edges=len(prob['edge_pose']),
                     iterations=list(st['iterations']), erased=int(erase.sum()))
            s['solver_over_ba_graph'] = s['ms_wall'] / r['ms_median']
            out['configs'].append(s); print(json.dumps(s), flush=True)
    nobs = out['observations']
    d = rows(1, npts, nobs); kq = torch.zeros(1, **i32)
    r = dict(entry='ba_graph_global', queries=1, **timed(lambda: ba_graph(1, 1, kq, d, npts, nobs), 3 if a.kernel_stats else a.reps))
    rep = d['rep'].cpu().numpy().view(COVIS_BA_REPORT_DTYPE)
    assert (rep['status'] == 0).all(), rep
    for k in ('n_poses', 'n_points', 'n_edges'): r[k] = int(rep[k][0])
    out['configs'].append(r); print(json.dumps(r), flush=True)
    G.close()
    if a.out: json.dump(out, open(a.out, 'w'), indent=1)


if __name__ == '__main__':
    main()
