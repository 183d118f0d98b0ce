"""Times the covisibility graph (sgx_covis_*): local_map and update_connections at Q = 1 and Q = 64 on a map of 500 keyframes of 1 000 points (a camera walking along
a wall of points: keyframe t sees 1 000 of the 1 300 points in front of it, 26 points further on than keyframe t - 1), and in the same run
sgx_match_project_local_batch_dev on the local maps just produced (the per-point attributes gathered by the returned ids): the step the local map feeds and the figure to
read it against.  HIP events around the launch sequence alone (everything resident, no read-back), median of the timed repetitions after 3 warm-up runs, min / max kept.
Mutations: host wall-clock of add_keyframe + set_observations (both synchronous) for the keyframes around the 100th and the 2 000th of one growing map.
Usage: python tools/bench_covis.py [--reps 20] [--out profiles/covis_bench.json] [--kernel-stats]
--kernel-stats runs local_map, update_connections and keyframe_culling at Q = 64 a few times and nothing else, for a separate profiler run of its own:
    rocprofv3 --kernel-trace --stats --output-format csv -d /tmp/covis_prof -- python tools/bench_covis.py --kernel-stats      (the *_kernel_stats.csv it writes -> profiles/covis_kernel_stats.csv)"""
import argparse
import ctypes as C
import json
import math
import os
import sys
import time
import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import sg_slam_amd
from sg_slam_amd.capi import _vp, Camera, KP_DTYPE, COVIS_REPORT_DTYPE
from sg_slam_amd.covisibility import CovisibilityGraph

PER, WIN, STEP, CAP, MCAP = 1000, 1300, 26, 1024, 4096


def grow(G, first, last, rng, timings=None):
    """keyframes first .. last - 1 of the walk; ids = their number"""
    for t in range(first, last):
        o = rng.randint(0, 8, PER).astype('i4'); u = np.where(rng.rand(PER) < 0.3, 5.0, -1.0).astype('f4'); d = rng.uniform(0.5, 80.0, PER).astype('f4')
        seen = (t * STEP + rng.choice(WIN, PER, replace=False)).astype('i4'); idx = np.arange(PER, dtype='i4')
        t0 = time.perf_counter()
        G.add_keyframe(t, o, u, d); G.set_observations(t, idx, seen)
        if timings is not None: timings.append(1e3 * (time.perf_counter() - t0))


def timed(fn, reps):
    times = []
    for r in range(reps + 3):
        e0 = torch.cuda.Event(enable_timing=True); e1 = torch.cuda.Event(enable_timing=True)
        e0.record(); fn(); e1.record(); torch.cuda.synchronize()
        if r >= 3: times.append(e0.elapsed_time(e1))
    return dict(ms_median=float(np.median(times)), ms_min=float(np.min(times)), ms_max=float(np.max(times)))


def world(npts, rng):
    """the wall: point i at x = 0.02 i, seen from 6 m; a descriptor each"""
    xw = np.stack([0.02 * np.arange(npts), rng.uniform(-1.4, 1.4, npts), 6.0 + rng.uniform(0, 0.5, npts)], 1).astype('f4')
    desc = rng.randint(0, 256, (npts, 32)).astype(np.uint8)
    return xw, desc


def main():
    ap = argparse.ArgumentParser(); ap.add_argument('--reps', type=int, default=20); ap.add_argument('--out', default=None); ap.add_argument('--kernel-stats', action='store_true')
    a = ap.parse_args()
    lib = sg_slam_amd.load(); dev = 'cuda'
    out = {'device': torch.cuda.get_device_name(0), 'keyframes': 500, 'points_per_keyframe': PER, 'configs': []}
    rng = np.random.RandomState(0)
    nkf = 500; npts = STEP * 2000 + WIN
    G = CovisibilityGraph(max_keyframes=512, cap=CAP, max_points=npts, max_observations=512 * PER, max_queries=64, lib=lib)
    grow(G, 0, nkf, rng)
    ids = np.arange(nkf, dtype='i4')
    for at in range(0, nkf, 64): G.update_connections(ids[at:at + 64])
    out['device_bytes'], out['workspace_bytes'], out['observations'] = G.info()
    out['mean_ordered'] = float(np.mean([len(G.ordered(int(k))[0]) for k in ids[::25]]))
    stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    xw, desc = world(npts, rng)
    cam = Camera(500.0, 500.0, 320.0, 240.0, 40.0, 0.0, 640.0, 0.0, 480.0)
    sf = (1.2 ** np.arange(8)).astype('f4')
    d_xw = torch.from_numpy(xw).to(dev); d_desc = torch.from_numpy(desc).to(dev)
    for Q in ((64,) if a.kernel_stats else (1, 64)):
        reps = 3 if a.kernel_stats else a.reps
        # Q frames along the walk: the points in front of the camera that fall into the image are its keypoints; every second one is tracked already
        frames = np.full((Q, CAP), -1, 'i4'); n = np.zeros(Q, 'i4'); keys = np.zeros((Q, CAP), KP_DTYPE); kdesc = np.zeros((Q, CAP, 32), np.uint8); Tcw = np.zeros((Q, 4, 4), 'f4')
        for q in range(Q):
            t = int(rng.randint(20, nkf - 20)); c = t * STEP + WIN // 2; x0 = 0.02 * c
            win = np.arange(t * STEP, t * STEP + WIN)
            u = 500.0 * (xw[win, 0] - x0) / xw[win, 2] + 320.0; v = 500.0 * xw[win, 1] / xw[win, 2] + 240.0
            vis = win[(u > 8) & (u < 632) & (v > 8) & (v < 472)][:CAP]
            n[q] = len(vis); frames[q, :len(vis):2] = vis[::2]
            keys['x'][q, :len(vis)] = 500.0 * (xw[vis, 0] - x0) / xw[vis, 2] + 320.0 + rng.uniform(-0.5, 0.5, len(vis))
            keys['y'][q, :len(vis)] = 500.0 * xw[vis, 1] / xw[vis, 2] + 240.0 + rng.uniform(-0.5, 0.5, len(vis))
            keys['octave'][q] = 1; keys['size'][q] = 31
            kdesc[q, :len(vis)] = desc[vis] ^ (rng.rand(len(vis), 32) < 0.05).astype(np.uint8)
            Tcw[q] = np.eye(4); Tcw[q, 0, 3] = -x0
        d = dict(frame=torch.from_numpy(frames).to(dev), n=torch.from_numpy(n).to(dev), mo=torch.zeros(Q, dtype=torch.int32, device=dev),
                 lkf=torch.full((Q, 512), -1, dtype=torch.int32, device=dev), nlkf=torch.zeros(Q, dtype=torch.int32, device=dev), ref=torch.full((Q,), -1, dtype=torch.int32, device=dev),
                 rt=torch.zeros(Q, dtype=torch.int32, device=dev), pts=torch.zeros((Q, MCAP), dtype=torch.int32, device=dev), obs=torch.zeros((Q, MCAP), dtype=torch.int32, device=dev),
                 npts=torch.zeros(Q, dtype=torch.int32, device=dev), rep=torch.zeros(Q * COVIS_REPORT_DTYPE.itemsize, dtype=torch.uint8, device=dev))
        frame0 = d['frame'].clone()
        def local_map():
            lib.check(lib.dll.sgx_covis_local_map_batch_dev(G.h, Q, CAP, _vp(d['frame']), _vp(d['n']), _vp(d['mo']), _vp(d['lkf']), _vp(d['nlkf']), _vp(d['ref']), _vp(d['rt']), MCAP,
                                                            _vp(d['pts']), _vp(d['obs']), _vp(d['npts']), _vp(d['rep']), stream), 'sgx_covis_local_map_batch_dev')
        r = dict(entry='local_map', queries=Q, **timed(local_map, reps))
        rep = d['rep'].cpu().numpy().view(COVIS_REPORT_DTYPE)
        assert (rep['status'] == 0).all() and (d['frame'] == frame0).all(), rep['status']
        r['local_keyframes_mean'] = float(rep['n_local_kf'].mean()); r['local_points_mean'] = float(rep['n_local_points'].mean())
        out['configs'].append(r); print(json.dumps(r), flush=True)
        kq = torch.from_numpy(rng.choice(ids, Q, replace=False).astype('i4')).to(dev); urep = torch.zeros(Q * COVIS_REPORT_DTYPE.itemsize, dtype=torch.uint8, device=dev)
        def update_connections():
            lib.check(lib.dll.sgx_covis_update_connections_batch_dev(G.h, Q, _vp(kq), _vp(urep), stream), 'sgx_covis_update_connections_batch_dev')
        r = dict(entry='update_connections', queries=Q, **timed(update_connections, reps))
        r['ordered_mean'] = float(urep.cpu().numpy().view(COVIS_REPORT_DTYPE)['n_ordered'].mean())
        out['configs'].append(r); print(json.dumps(r), flush=True)
        cand = torch.zeros((Q, 512), dtype=torch.int32, device=dev); nc = torch.zeros(Q, dtype=torch.int32, device=dev)
        red = torch.zeros_like(cand); mps = torch.zeros_like(cand); cull = torch.zeros_like(cand)
        def culling():
            lib.check(lib.dll.sgx_covis_keyframe_culling_batch_dev(G.h, Q, _vp(kq), 512, _vp(cand), _vp(nc), _vp(red), _vp(mps), _vp(cull), stream), 'sgx_covis_keyframe_culling_batch_dev')
        r = dict(entry='keyframe_culling', queries=Q, **timed(culling, reps)); r['candidates_mean'] = float(nc.float().mean())
        out['configs'].append(r); print(json.dumps(r), flush=True)
        if a.kernel_stats: continue
        # the consumer, on the local maps just produced: attributes gathered by id (rows past the count gather point 0 and are skipped by the count)
        pid = d['pts'].long().clamp(0, npts - 1)
        m_xw = d_xw[pid].contiguous(); m_desc = d_desc[pid].contiguous(); m_n = d['npts'].clamp(max=MCAP).contiguous()
        m_normal = torch.zeros_like(m_xw); m_normal[..., 2] = 1.0      # the mean viewing direction, camera to point
        m_min = torch.full((Q, MCAP), 1.0, device=dev); m_max = torch.full((Q, MCAP), 7.5, device=dev)
        m_skip = torch.stack([torch.zeros(npts, dtype=torch.uint8, device=dev).index_fill_(0, d['frame'][q][d['frame'][q] >= 0].long(), 1)[pid[q]] for q in range(Q)]).contiguous()
        cur_obs = torch.where(d['frame'] >= 0, 2, -1).to(torch.int32).contiguous()
        d_keys = torch.from_numpy(keys.view(np.uint8).reshape(Q, CAP, KP_DTYPE.itemsize)).to(dev); d_kdesc = torch.from_numpy(kdesc).to(dev)
        d_ur = torch.full((Q, CAP), -1.0, device=dev); d_T = torch.from_numpy(Tcw).to(dev); d_sf = torch.from_numpy(sf).to(dev)
        match = torch.zeros((Q, CAP), dtype=torch.int32, device=dev); nm = torch.zeros(Q, dtype=torch.int32, device=dev); inview = torch.zeros((Q, MCAP), dtype=torch.uint8, device=dev)
        def matcher():
            lib.check(lib.dll.sgx_match_project_local_batch_dev(Q, CAP, _vp(d_keys), _vp(d_kdesc), _vp(d_ur), _vp(d['n']), _vp(d_T), _vp(cur_obs), MCAP, _vp(m_n), _vp(m_xw), _vp(m_normal),
                                                                _vp(m_min), _vp(m_max), _vp(m_desc), _vp(d['obs']), _vp(m_skip), C.byref(cam), _vp(d_sf), 8, float(math.log(1.2)),
                                                                3.0, 0.8, 0.5, _vp(match), _vp(nm), _vp(inview), stream), 'sgx_match_project_local_batch_dev')
        r = dict(entry='match_project_local', queries=Q, **timed(matcher, reps))
        r['matches_mean'] = float(nm.float().mean()); r['in_view_mean'] = float(inview.float().sum(1).mean()); r['keypoints_mean'] = float(n.mean())
        out['configs'].append(r); print(json.dumps(r), flush=True)
    G.close()
    if not a.kernel_stats:
        # one growing map: what a keyframe costs to add when 100 and when 2 000 are there
        G = CovisibilityGraph(max_keyframes=2048, cap=CAP, max_points=npts, max_observations=2048 * PER, max_queries=1, lib=lib)
        tm = []; grow(G, 0, 2000, np.random.RandomState(1), tm)
        out['mutation'] = dict(add_keyframe_set_observations_ms_at_100=float(np.median(tm[90:110])), at_2000=float(np.median(tm[1980:2000])),
                               observations_per_keyframe=PER)
        print(json.dumps(out['mutation']), flush=True)
        G.close()
    if a.out: json.dump(out, open(a.out, 'w'), indent=1)


if __name__ == '__main__':
    main()
