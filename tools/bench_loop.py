"""Times the loop-closing sequences of the covisibility handle (sgx_covis_loop_begin_dev, sgx_covis_loop_connections_dev, sgx_covis_essential_graph_dev) on the map of
tools/bench_covis.py: 500 keyframes of 1 000 points (keyframe t sees 1 000 of the 1 300 points in front of it, 26 points further on than keyframe t - 1; about 95 listed
neighbours), a loop closed between keyframe 499 and keyframe 0 after fusing 60 points.  HIP events around each launch sequence alone (everything resident, no read-back),
median of the timed repetitions after 3 warm-up runs, min / max kept; the two sequences that change the handle reach their fixed point with the first call, which is
timed on its own (ms_first).  In the same run, for scale: sgx_optimize_essential_graph (host wall-clock, one run) on the produced graph with measurements composed from the
keyframe poses, and the host wall-clock of building the same graph through the getters (ordered / weights / tree per keyframe and Python sets), which is what a caller
does without these entries.  bench.py does not call this feature.
Usage: python tools/bench_loop.py [--reps 20] [--out profiles/loop_bench.json] [--kernel-stats]
--kernel-stats runs the three sequences a few times and nothing else, for a separate profiler run of its own:
    rocprofv3 --kernel-trace --stats --output-format csv -d /tmp/loop_prof -- python tools/bench_loop.py --kernel-stats   (its *_kernel_stats.csv -> profiles/loop_kernel_stats.csv)"""
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
from sg_slam_amd.capi import _vp, COVIS_LOOP_REPORT_DTYPE
from sg_slam_amd.covisibility import CovisibilityGraph
from sg_slam_amd.optimizer import Optimizer
from bench_covis import timed, PER, WIN, STEP, CAP

NKF, CUR, LOOP, FUSED, PCAP, LCAP, ECAP = 500, 499, 0, 60, 1 << 17, 1 << 16, 1 << 16


def once(fn):
    e0 = torch.cuda.Event(enable_timing=True); e1 = torch.cuda.Event(enable_timing=True)
    e0.record(); fn(); e1.record(); torch.cuda.synchronize()
    return float(e0.elapsed_time(e1))


def host_graph(G, ids, cur, loop, group, lc):
    """the edges of OptimizeEssentialGraph from the synchronous getters, as a caller without the entries builds them (no loop edges in this map)"""
    order = {}; weight = {}; parent = {}; children = {}
    for k in ids:
        order[k] = G.ordered(k); w = G.weights(k); weight[k] = dict(zip(*w)); p, _, ch = G.tree(k); parent[k] = p; children[k] = set(ch)
    vi = {k: j for j, k in enumerate(ids)}; edges = []; inserted = set()
    for i in sorted(group):
        for j in lc.get(i, []):
            if (i != cur or j != loop) and weight[i].get(j, 0) < 100: continue
            edges.append((vi[i], vi[j], 0)); inserted.add((min(i, j), max(i, j)))
    for k in ids:
        if parent[k] >= 0: edges.append((vi[k], vi[parent[k]], 1))
        o, w = order[k]
        cut = next((n for n, x in enumerate(w) if 100 > x), None)
        for n in (o[:cut] if cut is not None else []):
            if n == parent[k] or n in children[k] or n not in vi or n >= k or (n, k) in inserted: continue
            edges.append((vi[k], vi[n], 3))
    return edges


def main():
    ap = argparse.ArgumentParser(); ap.add_argument('--reps', type=int, default=20); ap.add_argument('--out', default=None); ap.add_argument('--kernel-stats', action='store_true')
    a = ap.parse_args()
    lib = sg_slam_amd.load(); dev = 'cuda'
    out = {'device': torch.cuda.get_device_name(0), 'keyframes': NKF, 'points_per_keyframe': PER, 'fused_points': FUSED, 'configs': []}
    rng = np.random.RandomState(0)
    npts = STEP * NKF + WIN
    G = CovisibilityGraph(max_keyframes=512, cap=CAP, max_points=npts, max_observations=512 * PER, max_queries=64, lib=lib)
    seen_of = {}
    for t in range(NKF):
        o = rng.randint(0, 8, PER).astype('i4'); seen = (t * STEP + rng.choice(WIN, PER, replace=False)).astype('i4'); seen_of[t] = seen
        G.add_keyframe(t, o, np.full(PER, -1, 'f4'), np.full(PER, 6.0, 'f4')); G.set_observations(t, np.arange(PER, dtype='i4'), seen)
    ids = np.arange(NKF, dtype='i4')
    for at in range(0, NKF, 64): G.update_connections(ids[at:at + 64])
    out['mean_ordered'] = float(np.mean([len(G.ordered(int(k))[0]) for k in ids[::25]]))
    stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    i32 = dict(dtype=torch.int32, device=dev); u8 = dict(dtype=torch.uint8, device=dev)
    rep = torch.zeros(COVIS_LOOP_REPORT_DTYPE.itemsize, **u8)
    report = lambda: rep.cpu().numpy().view(COVIS_LOOP_REPORT_DTYPE)[0]
    reps = 3 if a.kernel_stats else a.reps
    gid = torch.zeros(512, **i32); gv = torch.zeros(512, **i32); pid = torch.zeros(PCAP, **i32); pref = torch.zeros(PCAP, **i32)
    def begin(): lib.check(lib.dll.sgx_covis_loop_begin_dev(G.h, CUR, _vp(gid), _vp(gv), PCAP, _vp(pid), _vp(pref), _vp(rep), stream), 'sgx_covis_loop_begin_dev')
    first = once(begin)
    r = dict(entry='loop_begin', ms_first=first, **timed(begin, reps)); rb = report(); assert int(rb['status']) == 0, rb
    r['n_group'] = int(rb['n_group']); r['n_points'] = int(rb['n_points']); r['loop_bytes'] = G.loop_info()[0]
    out['configs'].append(r); print(json.dumps(r), flush=True)
    ng = r['n_group']; group = [int(x) for x in gid[:ng].cpu().numpy()]
    # the fusion: FUSED points of the current keyframe become points of the loop keyframe
    for old, new in zip([int(p) for p in seen_of[CUR][:FUSED]], [int(p) for p in seen_of[LOOP][:FUSED]]): G.replace_point(old, new)
    beg = torch.zeros(ng + 1, **i32); lj = torch.zeros(LCAP, **i32)
    def conn(): lib.check(lib.dll.sgx_covis_loop_connections_dev(G.h, CUR, ng, _vp(gid), LCAP, _vp(beg), _vp(lj), _vp(rep), stream), 'sgx_covis_loop_connections_dev')
    first = once(conn); rc = report(); assert int(rc['status']) == 0, rc
    nlc = int(rc['n_connections']); beg1 = beg.clone(); lj1 = lj[:max(nlc, 1)].clone()
    r = dict(entry='loop_connections', ms_first=first, n_connections=nlc, **timed(conn, reps))
    out['configs'].append(r); print(json.dumps(r), flush=True)
    vid = torch.zeros(512, **i32); vfx = torch.zeros(512, **u8); vgr = torch.zeros(512, **i32); ei = torch.zeros(ECAP, **i32); ej = torch.zeros(ECAP, **i32); ek = torch.zeros(ECAP, **u8)
    def graph(): lib.check(lib.dll.sgx_covis_essential_graph_dev(G.h, CUR, LOOP, ng, _vp(gid), nlc, _vp(beg1), _vp(lj1), _vp(vid), _vp(vfx), _vp(vgr), ECAP, _vp(ei), _vp(ej), _vp(ek),
                                                                 _vp(rep), stream), 'sgx_covis_essential_graph_dev')
    r = dict(entry='essential_graph', **timed(graph, reps)); rg = report(); assert int(rg['status']) == 0, rg
    r['n_vertices'] = int(rg['n_vertices']); r['n_edges'] = int(rg['n_edges']); r['n_kind'] = [int(x) for x in rg['n_kind']]
    out['configs'].append(r); print(json.dumps(r), flush=True)
    if not a.kernel_stats:
        ne = r['n_edges']; e_i = ei[:ne].cpu().numpy(); e_j = ej[:ne].cpu().numpy(); e_k = ek[:ne].cpu().numpy()
        # the caller's way without the entries: the getters and Python sets
        b = beg1.cpu().numpy(); j = lj1.cpu().numpy(); lcd = {g: [int(x) for x in j[b[r_]:b[r_ + 1]]] for r_, g in enumerate(sorted(group))}
        t0 = time.perf_counter(); edges = host_graph(G, [int(k) for k in ids], CUR, LOOP, group, lcd); ms = 1e3 * (time.perf_counter() - t0)
        h = dict(entry='host_getters_graph', ms_wall=ms, edges=len(edges), equals_device=edges == list(zip(e_i.tolist(), e_j.tolist(), e_k.tolist())), over_essential_graph=ms / r['ms_median'])
        out['configs'].append(h); print(json.dumps(h), flush=True)
        # for scale: the optimiser on this graph; poses along the wall with a drift the loop closes, measurements from the uncorrected poses
        S = np.zeros((NKF, 8)); S[:, 3] = 1; S[:, 7] = 1; S[:, 4] = -0.02 * (np.arange(NKF) * STEP + WIN // 2)
        meas = np.zeros((ne, 8)); meas[:, 3] = 1; meas[:, 7] = 1; meas[:, 4] = S[e_j, 4] - S[e_i, 4]
        meas[e_k == 0, 4] += 0.05
        torch.cuda.synchronize(); t0 = time.perf_counter()
        _, st = Optimizer.OptimizeEssentialGraph(S, vfx[:NKF].cpu().numpy(), e_i, e_j, meas, True, 20, lib=lib)
        s = dict(entry='optimize_essential_graph', ms_wall=1e3 * (time.perf_counter() - t0), vertices=NKF, edges=ne, iterations=float(st[0]))
        s['solver_over_three_sequences'] = s['ms_wall'] / sum(c['ms_median'] for c in out['configs'][:3])
        out['configs'].append(s); print(json.dumps(s), flush=True)
    G.close()
    if a.out: json.dump(out, open(a.out, 'w'), indent=1)


if __name__ == '__main__':
    main()
