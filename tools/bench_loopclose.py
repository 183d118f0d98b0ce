"""Times DetectLoop's consistency groups and the connected-keyframe CSR of the covisibility handle (sgx_covis_consistency_dev, sgx_covis_connected_batch_dev) on walks
of 100, 500 and 2 000 keyframes (keyframe t sees 200 of the 260 points in front of it, 5 points further on than keyframe t - 1: about 100 keyframes with a count >= 1 in
a row), for 1, 8 and 64 candidates drawn from the first 80 keyframes.  HIP events around each launch sequence alone (everything resident, no read-back), median of the
timed repetitions after 3 warm-up runs, min / max kept.  A consistency call replaces the groups, so the repetitions run in the steady state the same candidates reach
after the first call (every candidate consistent with its own group of the call before).  In the same run, the host wall-clock of the same answers assembled through
the getter a caller has without these entries, weights() per keyframe, with Python sets for the rule of LoopClosing.cc:160-211, and whether they are equal (the
median of 5 host runs).  Then the map update after global BA, sgx_covis_gba_update_dev + sgx_gba_correct_points_dev as one sequence, with 50 000 and 500 000 points and
0, 10 and 100 keyframes outside the GBA (the last of the walk), against tree() per keyframe and numpy float32 products (median of 3 host runs).
bench.py does not call this feature.
Usage: python tools/bench_loopclose.py [--reps 20] [--sizes 100,500,2000] [--out profiles/loopclose_bench.json] [--kernel-stats]
--kernel-stats runs the two sequences a few times on the 500-keyframe map and nothing else, for a separate profiler run of its own:
    rocprofv3 --kernel-trace --stats --output-format csv -d /tmp/lc_prof -- python tools/bench_loopclose.py --kernel-stats   (its *_kernel_stats.csv -> profiles/loopclose_kernel_stats.csv)"""
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
from sg_slam_amd.capi import _vp, COVIS_REPORT_DTYPE, COVIS_CONSISTENCY_REPORT_DTYPE, COVIS_GBA_REPORT_DTYPE
from sg_slam_amd.covisibility import CovisibilityGraph
from bench_covis import timed

PER, WIN, STEP, CAP, TH, MAX_GROUPS = 200, 260, 5, 256, 3, 128


def build(lib, nkf):
    rng = np.random.RandomState(0)
    N = 1 << int(np.ceil(np.log2(nkf + 1)))
    G = CovisibilityGraph(max_keyframes=N, cap=CAP, max_points=STEP * nkf + WIN, max_observations=N * PER, max_queries=64, lib=lib)
    for t in range(nkf):
        seen = (t * STEP + rng.choice(WIN, PER, replace=False)).astype('i4')
        G.add_keyframe(t, np.zeros(PER, 'i4'), np.full(PER, -1, 'f4'), np.full(PER, 6.0, 'f4')); G.set_observations(t, np.arange(PER, dtype='i4'), seen)
        G.update_connections([t])                                             # as LocalMapping does: the parent is the strongest keyframe before it, and 0 is the root
    ids = np.arange(nkf, dtype='i4')
    for at in range(0, nkf, 64): G.update_connections(ids[at:at + 64])
    G.consistency_reserve(MAX_GROUPS)
    return G


def host_consistency(G, cands, groups, th):
    """the rule of :160-211 with the candidate groups taken from weights() per candidate"""
    cur = []; enough = []; marked = [False] * len(groups)
    for c in cands:
        grp = set(G.weights(c)[0]); grp.add(c)
        some = False; en = False
        for g, (s, n) in enumerate(groups):
            if grp & s:
                some = True
                if not marked[g]: cur.append((grp, n + 1)); marked[g] = True
                if n + 1 >= th and not en: enough.append(c); en = True
        if not some: cur.append((grp, 0))
    return cur, enough


def host_gba(G, ids, in_gba, T, TG, xw, pg, xg, ref):
    """the same update with the tree taken from tree() per keyframe (the getter path) and numpy float32 products"""
    row = {k: r for r, k in enumerate(ids)}
    parent = [G.tree(k)[0] for k in ids]
    def inv(P): R = P[:, :3].T; return np.concatenate([R, -(R @ P[:, 3:4])], 1).astype('f4')
    def mul(A, B): return np.concatenate([A[:, :3] @ B[:, :3], A[:, :3] @ B[:, 3:4] + A[:, 3:4]], 1).astype('f4')
    out = T.copy(); done = np.array(in_gba, bool); out[done] = TG[done]
    order = sorted(range(len(ids)), key=lambda r: ids[r])
    changed = True
    while changed:                                                            # passes until no keyframe below a finished parent is left
        changed = False
        for r in order:
            if not done[r] and parent[r] >= 0 and done[row[parent[r]]]:
                p = row[parent[r]]; out[r] = mul(mul(T[r], inv(T[p])), out[p]); done[r] = True; changed = True
    x = xw.copy(); x[pg] = xg[pg]
    m = ~pg & (ref >= 0); r = ref[m]
    xc = np.einsum('nij,nj->ni', T[r][:, :, :3], xw[m]) + T[r][:, :, 3]
    Rw = np.transpose(out[r][:, :, :3], (0, 2, 1)); x[m] = np.einsum('nij,nj->ni', Rw, xc - out[r][:, :, 3])
    return out, x


def main():
    ap = argparse.ArgumentParser(); ap.add_argument('--reps', type=int, default=20); ap.add_argument('--sizes', default='100,500,2000'); ap.add_argument('--out', default=None)
    ap.add_argument('--kernel-stats', action='store_true')
    a = ap.parse_args()
    lib = sg_slam_amd.load(); dev = 'cuda'
    out = {'device': torch.cuda.get_device_name(0), 'points_per_keyframe': PER, 'th': TH, 'max_groups': MAX_GROUPS, 'configs': []}
    stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    i32 = dict(dtype=torch.int32, device=dev); u8 = dict(dtype=torch.uint8, device=dev)
    reps = 3 if a.kernel_stats else a.reps
    for nkf in ([500] if a.kernel_stats else [int(x) for x in a.sizes.split(',')]):
        t0 = time.perf_counter(); G = build(lib, nkf); build_s = time.perf_counter() - t0
        N = G.max_keyframes
        rng = np.random.RandomState(1)
        for nc in (1, 8, 64):
            cands = [int(x) for x in rng.choice(min(80, nkf), nc, replace=False)]
            cd = torch.tensor(cands, **i32); ncd = torch.tensor([nc], **i32); en = torch.zeros(N, **i32); nen = torch.zeros(1, **i32)
            rep = torch.zeros(COVIS_CONSISTENCY_REPORT_DTYPE.itemsize, **u8)
            def cons(): lib.check(lib.dll.sgx_covis_consistency_dev(G.h, _vp(cd), _vp(ncd), TH, _vp(en), _vp(nen), _vp(rep), stream), 'sgx_covis_consistency_dev')
            G.consistency_clear(); cons(); torch.cuda.synchronize()
            r = dict(entry='consistency', keyframes=nkf, candidates=nc, **timed(cons, reps))
            R = rep.cpu().numpy().view(COVIS_CONSISTENCY_REPORT_DTYPE)[0]; assert int(R['status']) == 0, R
            r['groups'] = int(R['n_after']); r['enough'] = int(R['n_enough'])
            if not a.kernel_stats:
                groups = [(set(s), n) for s, n in G.consistent_groups()]
                hs = []
                for _ in range(5):
                    t0 = time.perf_counter(); hg, he = host_consistency(G, cands, groups, TH); hs.append(1e3 * (time.perf_counter() - t0))
                r['ms_host_getters'] = float(np.median(hs)); r['host_runs'] = 5
                cons(); torch.cuda.synchronize()
                r['equals_device'] = [(sorted(s), n) for s, n in hg] == G.consistent_groups() and he == [int(x) for x in en[:int(nen[0])].cpu().numpy()]
                r['host_over_device'] = r['ms_host_getters'] / r['ms_median']
            out['configs'].append(r); print(json.dumps(r), flush=True)
            Q = nc; q = torch.tensor(cands, **i32); off = torch.zeros(Q + 1, **i32); ids = torch.zeros(Q * N, **i32); crep = torch.zeros(Q * COVIS_REPORT_DTYPE.itemsize, **u8)
            def conn(): lib.check(lib.dll.sgx_covis_connected_batch_dev(G.h, Q, _vp(q), _vp(off), _vp(ids), Q * N, _vp(crep), stream), 'sgx_covis_connected_batch_dev')
            r = dict(entry='connected_batch', keyframes=nkf, queries=Q, **timed(conn, reps))
            o = off.cpu().numpy(); r['ids'] = int(o[-1])
            if not a.kernel_stats:
                hs = []
                for _ in range(5):
                    t0 = time.perf_counter(); rows = [G.weights(c)[0] for c in cands]; hs.append(1e3 * (time.perf_counter() - t0))
                r['ms_host_getters'] = float(np.median(hs)); r['host_runs'] = 5
                got = ids.cpu().numpy()
                r['equals_device'] = all([int(x) for x in got[o[j]:o[j + 1]]] == rows[j] for j in range(Q))
                r['host_over_device'] = r['ms_host_getters'] / r['ms_median']
            out['configs'].append(r); print(json.dumps(r), flush=True)
        # the map update after global BA: the last n_out keyframes of the walk were created while the solver ran
        ids = list(range(nkf)); idd = torch.tensor(ids, **i32); org = torch.tensor([0], **i32)
        rs = np.random.RandomState(2)
        T = np.zeros((nkf, 3, 4), 'f4'); T[:, :, :3] = np.eye(3); T[:, 0, 3] = -0.02 * np.arange(nkf); TG = T.copy(); TG[:, :, 3] += rs.normal(size=(nkf, 3)).astype('f4') * 0.01
        Td = torch.from_numpy(T).cuda(); TGd = torch.from_numpy(TG).cuda(); To = torch.zeros_like(Td); Tb = torch.zeros_like(Td); st = torch.zeros(nkf, **u8)
        grep = torch.zeros(COVIS_GBA_REPORT_DTYPE.itemsize, **u8)
        for npts in ((50000,) if a.kernel_stats else (50000, 500000)):
            xw = rs.normal(size=(npts, 3)).astype('f4'); xg = xw + 0.01; pg = rs.rand(npts) < 0.5; ref = rs.randint(-1, nkf, npts).astype('i4')
            xd = torch.from_numpy(xw).cuda(); xgd = torch.from_numpy(xg.astype('f4')).cuda(); pgd = torch.from_numpy(pg.astype('u1')).cuda(); rfd = torch.from_numpy(ref).cuda(); xo = torch.zeros_like(xd)
            for n_out in (0, 10, 100):
                if n_out >= nkf: continue
                in_gba = np.ones(nkf, 'u1'); in_gba[nkf - n_out:] = 0 if n_out else 1; gd = torch.from_numpy(in_gba).cuda()
                def upd():
                    lib.check(lib.dll.sgx_covis_gba_update_dev(G.h, 1, _vp(org), nkf, _vp(idd), _vp(gd), _vp(Td), _vp(TGd), _vp(To), _vp(Tb), _vp(st), _vp(grep), stream), 'sgx_covis_gba_update_dev')
                    lib.check(lib.dll.sgx_gba_correct_points_dev(npts, _vp(xd), _vp(pgd), _vp(xgd), _vp(rfd), _vp(st), _vp(Tb), _vp(To), _vp(xo), stream), 'sgx_gba_correct_points_dev')
                r = dict(entry='gba_update+correct_points', keyframes=nkf, points=npts, outside_gba=n_out, **timed(upd, reps))
                R = grep.cpu().numpy().view(COVIS_GBA_REPORT_DTYPE)[0]; assert int(R['status']) == 0, R
                r['visited'] = int(R['n_visited']); r['max_depth'] = int(R['max_depth']); assert r['visited'] == nkf, R
                if not a.kernel_stats:
                    hs = []
                    for _ in range(3):
                        t0 = time.perf_counter(); ho, hx = host_gba(G, ids, in_gba, T, TG, xw, pg, xg.astype('f4'), ref); hs.append(1e3 * (time.perf_counter() - t0))
                    r['ms_host_getters'] = float(np.median(hs)); r['host_runs'] = 3
                    vis = st.cpu().numpy() == 3
                    r['max_abs_diff_pose'] = float(np.abs(To.cpu().numpy()[vis] - ho[vis]).max()); r['host_over_device'] = r['ms_host_getters'] / r['ms_median']
                out['configs'].append(r); print(json.dumps(r), flush=True)
        out.setdefault('build_seconds', {})[str(nkf)] = build_s
        G.close()
    if a.out: json.dump(out, open(a.out, 'w'), indent=1)


if __name__ == '__main__':
    main()
