"""Shared cases for the device covisibility graph (sgx_covis_*): a builder for hand-made maps, the hand-made cases (one per rule, each with its written answer), a
generator (a camera walking over a point cloud, interleaved with mutations) and the runner that plays a script on the device (or the emulator) and on the restatement of
tests/covis_ref.py and compares them: every comparison is equality of integers.  A script is a list of
  ('kf', id, octave, uright, depth) ('obs', id, idx, points) ('bad', ids) ('replace', old, new) ('erasekf', id)
  ('uc', ids[, expect]) ('lm', frames, min_obs, mcap[, dict(rows=, expect=)]) ('cull', ids[, expect]) ('cullloop', id[, erased])
  ('x', getter, args, value): the written answer of a getter, asserted of the restatement (which the device has to equal)."""
import numpy as np
import covis_ref
from sg_slam_amd.covisibility import CovisibilityGraph

TH_DEPTH = 40.0
REPORT_UC = ('status', 'n_counter', 'max_weight', 'max_kf', 'n_ordered', 'parent')


class Builder:
    """keyframes whose keypoints are handed out in index order; a point is observed at the next free index of each of its keyframes"""
    def __init__(self):
        self.ops = []; self.free = {}; self.pending = {}; self.pid = 0

    def kf(self, kf_id, n=64, octave=0, uright=-1.0, depth=1.0):
        self.flush()
        o = np.broadcast_to(np.asarray(octave, 'i4'), (n,)).copy(); u = np.broadcast_to(np.asarray(uright, 'f4'), (n,)).copy()
        d = np.broadcast_to(np.asarray(depth, 'f4'), (n,)).copy()
        self.ops.append(('kf', kf_id, o, u, d)); self.free[kf_id] = 0

    def pt(self, kfs):
        p = self.pid; self.pid += 1
        for k in kfs:
            self.pending.setdefault(k, ([], []))
            self.pending[k][0].append(self.free[k]); self.pending[k][1].append(p); self.free[k] += 1
        return p

    def pts(self, count, kfs):
        return [self.pt(kfs) for _ in range(count)]

    def flush(self):
        for k in sorted(self.pending): self.ops.append(('obs', k, self.pending[k][0], self.pending[k][1]))
        self.pending = {}

    def op(self, *o):
        self.flush(); self.ops.append(tuple(o))

    def x(self, getter, args, value):
        self.op('x', getter, args if isinstance(args, tuple) else (args,), value)

    def case(self, name, **kw):
        self.flush()
        return dict(name=name, ops=self.ops, **kw)


# ---- hand-made cases ------------------------------------------------------------------------------------------------------------------------------------------------
def hand_cases():
    C = []
    # weights 14 / 15 / 16 around the gate: the map holds all three, the list the two that reach 15; only those two neighbours get the connection back
    b = Builder()
    for k in (1, 2, 3, 4): b.kf(k)
    b.pts(14, [1, 2]); b.pts(15, [1, 3]); b.pts(16, [1, 4])
    b.op('uc', [1], [dict(status=0, n_counter=3, max_weight=16, max_kf=4, n_ordered=2, parent=4)])
    b.x('weights', 1, ([2, 3, 4], [14, 15, 16])); b.x('ordered', 1, ([4, 3], [16, 15])); b.x('weights', 2, ([], [])); b.x('weights', 3, ([1], [15]))
    b.x('ordered', 3, ([1], [15])); b.x('tree', 1, (4, False, [])); b.x('tree', 4, (-1, True, [1]))
    C.append(b.case('gate-14-15-16'))
    # nothing reaches 15: the single maximum, the smallest id on a tie (pKFmax moves on a strictly greater count in key order)
    b = Builder()
    for k in (1, 2, 3, 4): b.kf(k)
    b.pts(5, [1, 2]); b.pts(5, [1, 3]); b.pts(3, [1, 4])
    b.op('uc', [1], [dict(status=0, n_counter=3, max_weight=5, max_kf=2, n_ordered=1, parent=2)])
    b.x('weights', 1, ([2, 3, 4], [5, 5, 3])); b.x('ordered', 1, ([2], [5])); b.x('weights', 2, ([1], [5])); b.x('weights', 3, ([], []))
    C.append(b.case('single-maximum-tie'))
    # equal weights across the top-10 boundary: among equals the later key comes first, so of 30, 31, 32 at weight 16 it is 32 that makes the ten
    b = Builder()
    b.kf(1, n=256)
    for k in list(range(10, 19)) + [30, 31, 32]: b.kf(k, n=32)
    for k in range(10, 19): b.pts(20, [1, k])
    for k in (30, 31, 32): b.pts(16, [1, k])
    b.op('uc', [1])
    b.x('best_covisibles', (1, 10), [18, 17, 16, 15, 14, 13, 12, 11, 10, 32])
    b.x('ordered', 1, ([18, 17, 16, 15, 14, 13, 12, 11, 10, 32, 31, 30], [20] * 9 + [16] * 3))
    C.append(b.case('top10-equal-weights'))
    # AddConnection with the same weight leaves the gated list alone; with a new weight UpdateBestCovisibles rebuilds it from the WHOLE map, weight 3 included
    b = Builder()
    for k in (1, 2, 3): b.kf(k)
    b.pts(15, [1, 2]); b.pts(3, [1, 3])
    b.op('uc', [1]); b.x('ordered', 1, ([2], [15])); b.x('weights', 1, ([2, 3], [15, 3]))
    b.op('uc', [2]); b.x('ordered', 1, ([2], [15]))
    b.pts(1, [1, 2])
    b.op('uc', [2]); b.x('ordered', 1, ([2, 3], [16, 3])); b.x('weights', 1, ([2, 3], [16, 3]))
    C.append(b.case('addconnection-same-and-new-weight'))
    # an empty KFcounter returns early: the connections made before the points went bad are still there
    b = Builder()
    for k in (1, 2): b.kf(k)
    P = b.pts(15, [1, 2])
    b.op('uc', [1]); b.x('weights', 1, ([2], [15]))
    b.op('bad', P)
    b.op('uc', [1], [dict(status=0, n_counter=0, max_weight=0, max_kf=-1, n_ordered=0, parent=2)])
    b.x('weights', 1, ([2], [15])); b.x('ordered', 1, ([2], [15])); b.x('keyframe_points', 1, [-1] * 64)
    C.append(b.case('empty-counter-keeps-connections'))
    # the parent is the front of the list at the first connection; keyframe 0 never gets one and keeps mbFirstConnection
    b = Builder()
    for k in (0, 1, 2): b.kf(k, n=128)
    b.pts(20, [0, 1]); b.pts(30, [1, 2]); b.pts(16, [0, 2])
    b.op('uc', [0]); b.x('ordered', 0, ([1, 2], [20, 16])); b.x('tree', 0, (-1, True, []))
    b.op('uc', [1]); b.x('ordered', 1, ([2, 0], [30, 20])); b.x('tree', 1, (2, False, []))
    b.op('uc', [2]); b.x('tree', 2, (1, False, [1])); b.x('tree', 1, (2, False, [2]))
    b.op('bad', list(range(20, 50)))                                       # the 30 points of 1 and 2: 1's strongest is now 0, its parent stays 2
    b.op('uc', [1]); b.x('ordered', 1, ([0], [20])); b.x('tree', 1, (2, False, [2]))
    C.append(b.case('first-connection-parent-and-id0'))
    # 79 / 80 / 81 / 82 stage-1 keyframes: size() > 80 is tested before each stage-1 keyframe, so 79 lets two neighbours in, 80 one, 81 and 82 none
    b = Builder()
    for k in range(1, 83): b.kf(k, n=32)
    b.kf(101, n=32); b.kf(102, n=32)
    own = [b.pt([k]) for k in range(1, 83)]
    b.pts(15, [1, 101]); b.pts(15, [2, 102])
    b.op('uc', [101, 102]); b.x('ordered', 1, ([101], [15])); b.x('tree', 101, (1, False, []))
    b.op('lm', [own[:79], own[:80], own[:81], own[:82]], 0, 4096,
         dict(expect=[dict(local_kf=list(range(1, 80)) + [101, 102], ref_kf=1, n_stage1=79), dict(local_kf=list(range(1, 81)) + [101], ref_kf=1, n_stage1=80),
                      dict(local_kf=list(range(1, 82)), n_stage1=81), dict(local_kf=list(range(1, 83)), n_stage1=82)]))
    C.append(b.case('stage2-limit-80'))
    # the parent break: keyframe 1 adds its neighbour 7 and its unmarked parent 5 and LEAVES the loop, so keyframe 2's neighbour 6 never enters ([1, 2, 7, 5, 6] if it went on)
    b = Builder()
    for k in (1, 2, 5, 6, 7): b.kf(k)
    S = b.pts(20, [1, 5])
    b.op('uc', [1]); b.x('tree', 1, (5, False, []))
    b.pts(30, [1, 7]); b.op('bad', S)
    b.op('uc', [1]); b.x('ordered', 1, ([7], [30])); b.x('tree', 1, (5, False, []))
    b.pts(15, [2, 6])
    b.op('uc', [2]); b.x('ordered', 2, ([6], [15]))
    a = b.pt([1]); c = b.pt([2])
    b.op('lm', [[a, c]], 0, 4096, dict(expect=[dict(local_kf=[1, 2, 7, 5], ref_kf=1, n_stage1=2)]))
    C.append(b.case('stage2-parent-break'))
    # a child that is also the best neighbour: 3 enters as the neighbour, so the first unmarked child in key order is 4
    b = Builder()
    for k in (1, 3, 4): b.kf(k)
    b.pts(20, [1, 3]); b.op('uc', [3])
    b.pts(15, [1, 4]); b.op('uc', [4])
    b.x('ordered', 1, ([3, 4], [20, 15])); b.x('tree', 1, (-1, True, [3, 4]))
    a = b.pt([1])
    b.op('lm', [[a]], 0, 4096, dict(expect=[dict(local_kf=[1, 3, 4], ref_kf=1)]))
    C.append(b.case('stage2-child-is-neighbour'))
    # a frame with a point twice (two votes), an id that is no point (becomes -1) and an empty entry
    b = Builder()
    for k in (1, 2): b.kf(k)
    p = b.pt([1]); p2 = b.pt([2])
    b.op('lm', [[p2, p, 999, -1, p]], 0, 4096,
         dict(expect=[dict(frame=[p2, p, -1, -1, p], local_kf=[1, 2], ref_kf=1, ref_tracked=1, points=[p, p2], obs=[1, 1], n_counter=2, max_weight=2, max_kf=1)]))
    C.append(b.case('frame-bad-points-and-duplicates'))
    # no vote: the row and the reference keyframe stay and the points are rebuilt from the row; the erased keyframe 9 in it contributes nothing
    b = Builder()
    for k in (1, 2, 9): b.kf(k)
    p1 = b.pts(3, [1]); p2 = b.pts(2, [2]); b.pts(2, [9]); s = b.pt([1, 2])
    b.op('erasekf', 9)
    b.op('lm', [[-1, 999], [-1], []], 2, 4096,
         dict(rows=[([2, 9, 1], 2), ([2, 9, 1], 9), ([], -1)],
              expect=[dict(frame=[-1, -1], local_kf=[2, 9, 1], ref_kf=2, ref_tracked=1, points=p2 + [s] + p1, obs=[1, 1, 2, 1, 1, 1], n_counter=0, n_stage1=0),
                      dict(local_kf=[2, 9, 1], ref_kf=9, ref_tracked=0, points=p2 + [s] + p1), dict(local_kf=[], ref_kf=-1, ref_tracked=0, points=[], n_points=0)]))
    C.append(b.case('no-votes-kept-row'))
    # more points than mcap: the true count, the first mcap of them, SGX_ERR_NOMEM in the report
    b = Builder()
    b.kf(1)
    p = b.pts(5, [1])
    b.op('lm', [[p[4]], [p[0]]], 0, 3, dict(expect=[dict(points=p[:3], n_points=5, status=-3), dict(points=p[:3], n_points=5, status=-3)]))
    b.op('lm', [[p[4]]], 0, 5, dict(expect=[dict(points=p, n_points=5, status=0)]))
    C.append(b.case('mcap-overflow'))
    # culling counts: Observations() 3 and 4 out of stereo and mono observations, octave own + 1 and own + 2, a point beyond mThDepth and one of negative depth
    for mono in (False, True):
        b = Builder()
        b.kf(10); b.kf(11, octave=2, depth=[1.0] * 4 + [50.0, -1.0] + [50.0] * 58); b.kf(13, octave=3); b.kf(14, octave=3)
        b.kf(15, octave=[3, 4] + [3] * 62); b.kf(16, uright=5.0)
        b.pt([11, 16]); b.pt([11, 16, 13]); b.pt([11, 13, 14, 15]); b.pt([11, 13, 14, 15]); b.pt([11, 13, 14, 15]); b.pt([11, 13, 14, 15])
        b.pts(15, [10, 11])
        b.op('uc', [10]); b.x('ordered', 10, ([11], [15]))
        b.x('observations', 0, ([(11, 0), (16, 0)], 3)); b.x('observations', 1, ([(11, 1), (13, 0), (16, 1)], 4))
        b.op('cull', [10], [[(11, 3, 21, 0)] if mono else [(11, 1, 4, 0)]])
        C.append(b.case('culling-counts-mono' if mono else 'culling-counts', monocular=mono))
    # nMPs = 10 with exactly 9 redundant: 9 > 0.9 * 10 is false; 10 of 10 votes; keyframe 0, though wholly redundant, is passed over
    b = Builder()
    far = [1.0] * 10 + [50.0] * 54
    b.kf(10, n=128); b.kf(0, depth=far); b.kf(11, depth=far); b.kf(12, depth=far)
    for k in (13, 14, 15): b.kf(k)
    b.pts(10, [0, 13, 14, 15]); b.pts(9, [11, 13, 14, 15]); b.pts(1, [11, 13]); b.pts(10, [12, 13, 14, 15])
    b.pts(20, [10, 0]); b.pts(16, [10, 11]); b.pts(15, [10, 12])
    b.op('uc', [10]); b.x('ordered', 10, ([0, 11, 12], [20, 16, 15]))
    b.op('cull', [10], [[(0, 0, 0, 0), (11, 9, 10, 0), (12, 10, 10, 1)]])
    C.append(b.case('culling-ratio-and-id0'))
    # the cascade: against the map as it stands 11 and 12 are both voted; erasing 11 takes 12's points to three observations, and the literal loop keeps 12
    b = Builder()
    b.kf(10, n=128); b.kf(11, depth=[1.0] * 20 + [50.0] * 44); b.kf(12, depth=[1.0] * 10 + [50.0] * 54)
    for k in (13, 14, 15): b.kf(k)
    b.pts(10, [11, 13, 14, 15]); b.pts(10, [12, 11, 13, 14]); b.pts(16, [10, 11]); b.pts(15, [10, 12])
    b.op('uc', [10]); b.x('ordered', 10, ([11, 12], [16, 15]))
    b.op('cull', [10], [[(11, 20, 20, 1), (12, 10, 10, 1)]])
    b.op('cullloop', 10, [11])
    b.op('cull', [10], [[(12, 0, 10, 0)]])
    C.append(b.case('culling-cascade'))
    # EraseObservation: three mono observations fall to nObs 2 and the point is erased everywhere; stereo + mono + mono falls from 4 to 3 and stays
    b = Builder()
    for k in (1, 2, 3): b.kf(k, n=8)
    b.kf(4, n=8, uright=3.0)
    p = b.pt([1, 2, 3]); q = b.pt([1, 2, 4])
    b.x('observations', p, ([(1, 0), (2, 0), (3, 0)], 3)); b.x('observations', q, ([(1, 1), (2, 1), (4, 0)], 4))
    b.op('obs', 1, [0, 1], [-1, -1])
    b.x('observations', p, ([], 0)); b.x('observations', q, ([(2, 1), (4, 0)], 3))
    b.x('keyframe_points', 2, [-1, q] + [-1] * 6); b.x('keyframe_points', 3, [-1] * 8); b.x('keyframe_points', 1, [-1] * 8)
    C.append(b.case('erase-observation-to-two'))
    # Replace onto a point the keyframe already holds: keyframe 2 loses the old match, keyframe 1 passes to the new point
    b = Builder()
    for k in (1, 2, 3): b.kf(k, n=4)
    old = b.pt([1, 2]); new = b.pt([2, 3])
    b.op('replace', old, new)
    b.x('observations', new, ([(1, 0), (2, 1), (3, 0)], 3)); b.x('observations', old, ([], 0))
    b.x('keyframe_points', 1, [new, -1, -1, -1]); b.x('keyframe_points', 2, [-1, new, -1, -1])
    C.append(b.case('replace-onto-present-point'))
    # SetBadFlag of 2, the parent of 3 and 4: 3 is connected to the grandparent 1 and goes there; 4 is connected only to 3, which is a candidate by then
    b = Builder()
    for k in (1, 2, 3, 4): b.kf(k, n=128)
    b.pts(20, [2, 1]); b.op('uc', [2]); b.x('tree', 2, (1, False, []))
    b.pts(30, [3, 2]); b.pts(15, [3, 1]); b.op('uc', [3]); b.x('ordered', 3, ([2, 1], [30, 15])); b.x('tree', 3, (2, False, []))
    b.pts(30, [4, 2]); b.pts(20, [4, 3]); b.op('uc', [4]); b.x('tree', 4, (2, False, [])); b.x('tree', 2, (1, False, [3, 4]))
    b.op('erasekf', 2)
    b.x('tree', 3, (1, False, [4])); b.x('tree', 4, (3, False, [])); b.x('tree', 1, (-1, True, [3]))
    b.x('ordered', 3, ([4, 1], [20, 15])); b.x('ordered', 4, ([3], [20])); b.x('weights', 1, ([3], [15]))      # 1 lost 2 and keeps what 3's UpdateConnections gave it
    C.append(b.case('erase-keyframe-reparenting'))
    # an erased keyframe stays, flagged bad, in the map and the list of a keyframe that its own map did not hold (no EraseConnection reaches it): 5 keeps 6 at weight 3, the
    # rebuilt list shows it, the local map passes over it and culling counts nothing for it
    b = Builder()
    for k in (5, 6, 7): b.kf(k)
    b.pts(3, [5, 6]); b.pts(15, [5, 7])
    b.op('uc', [5]); b.x('ordered', 5, ([7], [15])); b.x('weights', 5, ([6, 7], [3, 15])); b.x('weights', 6, ([], []))
    b.op('erasekf', 6); b.x('weights', 5, ([6, 7], [3, 15]))
    b.pts(1, [5, 7])
    b.op('uc', [7]); b.x('ordered', 5, ([7, 6], [16, 3])); b.x('best_covisibles', (5, 10), [7, 6])
    a = b.pt([5]); c = b.pt([7])
    b.op('lm', [[a, c], [a]], 0, 4096, dict(expect=[dict(local_kf=[5, 7]), dict(local_kf=[5, 7])]))
    b.op('cull', [5], [[(7, 0, 17, 0), (6, 0, 0, 0)]])
    C.append(b.case('erased-keyframe-stays-listed'))
    return C


# ---- the generator --------------------------------------------------------------------------------------------------------------------------------------------------
def walk_script(seed, nkf=40, npts=500, per_kf=48, cap=64, window=90, monocular=False, Q=5, mutate=True):
    """a camera walks along a line of npts points; keyframe t sees per_kf points of the window around its place (some seen in stereo, at random octaves and depths); after
    every keyframe UpdateConnections, local maps for frames near by, culling votes; interleaved: points going bad, erased observations, replaced points, erased keyframes.
    The restatement is played along to keep the script valid (a free index, a point the keyframe does not hold)."""
    rng = np.random.RandomState(seed)
    R = covis_ref.Map(monocular, TH_DEPTH, npts)
    ops = []
    def emit(op):
        ops.append(op); apply_ref(R, op)
    live = []
    for t in range(nkf):
        kid = 3 * t if t else 0
        n = rng.randint(per_kf, cap + 1)
        emit(('kf', kid, rng.randint(0, 8, n).astype('i4'), np.where(rng.rand(n) < 0.3, 5.0, -1.0).astype('f4'),
              np.where(rng.rand(n) < 0.1, -1.0, rng.uniform(0.5, 80.0, n)).astype('f4')))
        live.append(kid)
        c = int(t * (npts - window) / max(nkf - 1, 1))
        seen = rng.choice(np.arange(c, c + window), min(per_kf, n), replace=False)
        idx = rng.permutation(n)[:len(seen)]
        emit(('obs', kid, [int(i) for i in idx], [int(p) for p in seen]))
        emit(('uc', [kid]))
        if t % 3 == 2:
            emit(('uc', [int(k) for k in rng.choice(live, min(len(live), Q), replace=False)]))
        if t % 2 == 1:
            frames = []
            for _ in range(Q):
                cc = rng.randint(max(0, c - window), c + 1)
                f = [int(p) for p in rng.choice(np.arange(cc, cc + window), rng.randint(0, 40))]
                f += [-1] * rng.randint(0, 4)
                rng.shuffle(f); frames.append(f)
            emit(('lm', frames, int(rng.randint(0, 4)), 4096 if t % 4 == 1 else 50, {}))
        if t % 4 == 3:
            emit(('cull', [int(k) for k in rng.choice(live, min(len(live), 3), replace=False)]))
        if not mutate or t < 4: continue
        r = rng.rand()
        if r < 0.25:
            emit(('bad', [int(p) for p in rng.randint(0, npts, 3)]))
        elif r < 0.5:
            k = int(rng.choice(live)); pts = R.keyframe_points(k); have = [i for i, p in enumerate(pts) if p >= 0]
            if have: emit(('obs', k, [int(i) for i in rng.choice(have, min(len(have), 4), replace=False)], [-1] * min(len(have), 4)))
        elif r < 0.7:
            ex = sorted(R.points)
            if len(ex) >= 2:
                a, bb = rng.choice(ex, 2, replace=False); emit(('replace', int(a), int(bb)))
        elif r < 0.85 and len(live) > 6:
            k = int(rng.choice(live[1:-1])); emit(('erasekf', k)); live.remove(k)
        else:
            votes = R.culling_votes(live[-1])
            if any(v[3] for v in votes):
                emit(('cullloop', live[-1])); live = [k for k in live if k in R.kfs]
    emit(('uc', list(live[:Q])))
    emit(('cull', list(live[-Q:])))
    return dict(name=f'walk-{seed}' + ('-mono' if monocular else ''), ops=ops, monocular=monocular, max_points=npts, cap=cap)


def all_generated():
    return [walk_script(0), walk_script(1, monocular=True), walk_script(2, nkf=70, npts=300, window=120, per_kf=60), walk_script(3, nkf=30, npts=200, window=150, per_kf=40, Q=3)]


def shapes_script(nkf, seed=7):
    """smallest shapes: nkf keyframes holding 0, 1, 63, 64, 65 and cap (= 96) points in turn, over few points, so that observation lists run from 1 and 2 to nkf - 1"""
    rng = np.random.RandomState(seed + nkf)
    cap = 96; sizes = [0, 1, 63, 64, 65, cap]; npts = 130
    ops = []; ids = []
    for t in range(nkf):
        kid = t * 2; ids.append(kid); m = sizes[t % len(sizes)]
        ops.append(('kf', kid, rng.randint(0, 8, cap).astype('i4'), np.where(rng.rand(cap) < 0.3, 2.0, -1.0).astype('f4'), rng.uniform(0.5, 80.0, cap).astype('f4')))
        pts = [0] * (m >= 1) + [int(p) for p in (rng.choice(np.arange(1, npts), m - 1, replace=False) if m > 1 else [])]      # point 0 is seen by every keyframe that sees anything
        ops.append(('obs', kid, list(range(len(pts))), pts))
    for at in range(0, nkf, 17): ops.append(('uc', ids[at:at + 17]))
    frames = [[int(p) for p in rng.randint(0, npts, n)] for n in (0, 1, 63, 64, 65, cap)]
    ops.append(('lm', frames, 2, 4096, {})); ops.append(('lm', frames, 0, 64, {}))
    for at in range(0, nkf, 17): ops.append(('cull', ids[at:at + 17]))
    return dict(name=f'shapes-{nkf}', ops=ops, max_points=npts, cap=cap, max_queries=17)


# ---- the runner -----------------------------------------------------------------------------------------------------------------------------------------------------
def apply_ref(R, op, rows=None):
    """one operation on the restatement; returns what a query returns"""
    k = op[0]
    if k == 'kf': R.add_keyframe(op[1], op[2], op[3], op[4])
    elif k == 'obs': R.set_observations(op[1], op[2], op[3])
    elif k == 'bad': R.set_points_bad(op[1])
    elif k == 'replace': R.replace_point(op[1], op[2])
    elif k == 'erasekf': R.erase_keyframe(op[1])
    elif k == 'uc': return [R.update_connections(i) for i in op[1]]
    elif k == 'lm':
        rows = rows if rows is not None else [([], -1)] * len(op[1])
        return [R.local_map(f, op[2], rows[q][0], rows[q][1], op[3]) for q, f in enumerate(op[1])]
    elif k == 'cull': return [R.culling_votes(i) for i in op[1]]
    elif k == 'cullloop': return R.KeyFrameCulling(op[1])
    return None


def make_graph(lib, case, **kw):
    a = dict(max_keyframes=case.get('max_keyframes', 128), cap=case.get('cap', 256), max_points=case.get('max_points', 2048),
             max_observations=case.get('max_observations', 1 << 16), max_queries=case.get('max_queries', 8), monocular=case.get('monocular', False), th_depth=TH_DEPTH)
    a.update(kw)
    return CovisibilityGraph(lib=lib, **a)


def compare_state(G, R, points):
    assert G.size() == len(R.kfs)
    for k in sorted(R.kfs):
        assert G.weights(k) == R.weights(k), ('weights', k)
        assert G.ordered(k) == R.ordered(k), ('ordered', k)
        assert G.best_covisibles(k, 10) == R.best_covisibles(k, 10), ('best', k)
        assert G.tree(k) == R.tree(k), ('tree', k)
        assert list(G.keyframe_points(k)) == R.keyframe_points(k), ('points', k)
    for p in sorted(points):
        assert G.observations(p) == R.observations(p), ('observations', p)
    assert G.info()[2] == sum(len(p.mObservations) for p in R.points.values())


def culling_caller_loop(G, cur):
    """deviation 5: query, erase the first voted candidate, query again and go on behind it in the candidate list of the first query"""
    votes = G.keyframe_culling([cur])[0]
    L = [v[0] for v in votes]; pos = 0; erased = []
    while True:
        vm = {v[0]: v[3] for v in votes}
        j = next((j for j in range(pos, len(L)) if vm.get(L[j], 0)), None)
        if j is None: return erased
        G.erase_keyframe(L[j]); erased.append(L[j]); pos = j + 1
        votes = G.keyframe_culling([cur])[0]


def check_local(got, ref, mcap):
    assert ref is not None and int(got['report']['status']) == ref['status']
    assert list(got['frame']) == ref['frame'] and got['local_kf'] == ref['local_kf'] and got['ref_kf'] == ref['ref_kf'] and got['ref_tracked'] == ref['ref_tracked']
    assert got['n_points'] == ref['n_points'] and list(got['points']) == ref['points'] and list(got['obs']) == ref['obs']
    for key in ('n_counter', 'max_weight', 'max_kf', 'n_stage1', 'n_local_kf', 'ref_tracked'): assert int(got['report'][key]) == ref[key], key
    assert int(got['report']['n_local_points']) == ref['n_points']


def run_script(lib, case, via='batch', stream=None, state_every=1, G=None):
    """plays the script on both sides; via = 'batch' (a query op is one launch sequence) or 'single' (one call per query).  The full state is compared after every
    state_every-th mutation and at the end; every query result always."""
    own = G is None
    G = G or make_graph(lib, case)
    R = covis_ref.Map(case.get('monocular', False), TH_DEPTH, G.max_points)
    points = set(); rows = {}; nmut = 0; results = []
    for op in case['ops']:
        k = op[0]
        if k == 'x':
            want = getattr(R, op[1])(*op[2])
            assert want == op[3], (case['name'], op[1], op[2], want, op[3])
            got = getattr(G, op[1])(*op[2])
            assert (list(got) if op[1] == 'keyframe_points' else got) == op[3], (case['name'], 'device', op[1], op[2], got, op[3])
            continue
        if k == 'lm':
            extra = op[4] if len(op) > 4 else {}
            Q = len(op[1])
            rin = extra.get('rows') or [rows.get(q, ([], -1)) for q in range(Q)]
            ref = apply_ref(R, op, rin)
            if via == 'batch': got = G.local_map(op[1], op[2], [r[0] for r in rin], [r[1] for r in rin], op[3], stream)
            else: got = [G.local_map([op[1][q]], op[2], [rin[q][0]], [rin[q][1]], op[3], stream)[0] for q in range(Q)]
            for q in range(Q):
                check_local(got[q], ref[q], op[3])
                rows[q] = (ref[q]['local_kf'], ref[q]['ref_kf'])
                for key, v in (extra.get('expect') or [{}] * Q)[q].items(): assert ref[q][key] == v, (case['name'], q, key, ref[q][key], v)
            results.append(got)
            continue
        ref = apply_ref(R, op)
        if k == 'kf': G.add_keyframe(op[1], op[2], op[3], op[4])
        elif k == 'obs': G.set_observations(op[1], op[2], op[3]); points.update(p for p in op[3] if p >= 0)
        elif k == 'bad': G.set_points_bad(op[1])
        elif k == 'replace': G.replace_point(op[1], op[2])
        elif k == 'erasekf': G.erase_keyframe(op[1])
        elif k == 'uc':
            rep = G.update_connections(op[1], stream) if via == 'batch' else np.concatenate([G.update_connections([i], stream) for i in op[1]])
            got = [tuple(int(rep[q][f]) for f in REPORT_UC) for q in range(len(op[1]))]
            assert got == ref, (case['name'], 'uc', op[1], got, ref)
            if len(op) > 2:
                for q, e in enumerate(op[2]): assert dict(zip(REPORT_UC, ref[q])) == e, (case['name'], q, ref[q], e)
            results.append(got)
        elif k == 'cull':
            got = G.keyframe_culling(op[1], stream=stream) if via == 'batch' else [G.keyframe_culling([i], stream=stream)[0] for i in op[1]]
            assert got == ref, (case['name'], 'cull', op[1], got, ref)
            if len(op) > 2: assert ref == op[2], (case['name'], ref, op[2])
            results.append(got)
        elif k == 'cullloop':
            got = culling_caller_loop(G, op[1])
            assert got == ref, (case['name'], 'cullloop', got, ref)
            if len(op) > 2: assert ref == op[2]
        if k not in ('uc', 'cull'): nmut += 1
        if k != 'cull' and (state_every == 1 or (k != 'uc' and nmut % state_every == 0)): compare_state(G, R, points)
    compare_state(G, R, points)
    if own: G.close()
    return R, results


# ---- checks shared by the CPU and the GPU tier ------------------------------------------------------------------------------------------------------------------------
def check_batch_equals_singles(lib, Q, stream=None):
    """the same map twice: Q queries as one batch on one, as Q calls on the other; every output and the state after are equal"""
    case = walk_script(5, nkf=24, mutate=False, Q=Q)
    case['max_queries'] = Q
    ops = [o for o in case['ops'] if o[0] in ('kf', 'obs')]
    ids = [o[1] for o in ops if o[0] == 'kf']
    rng = np.random.RandomState(Q)
    kq = [int(x) for x in rng.choice(ids, Q, replace=Q > len(ids))]      # with repeats at Q = 17 of 24: a keyframe updated twice in one batch
    if Q > 2: kq[1] = kq[0]
    frames = [[int(p) for p in rng.randint(0, 500, rng.randint(0, 60))] for _ in range(Q)]
    A = make_graph(lib, case); B = make_graph(lib, case); R = covis_ref.Map(False, TH_DEPTH, A.max_points)
    for o in ops:
        for g in (A, B): g.add_keyframe(*o[1:]) if o[0] == 'kf' else g.set_observations(*o[1:])
        apply_ref(R, o)
    ra = A.update_connections(kq, stream); rb = np.concatenate([B.update_connections([k], stream) for k in kq])
    assert (ra == rb).all() and [tuple(int(ra[q][f]) for f in REPORT_UC) for q in range(Q)] == [R.update_connections(k) for k in kq]
    for k in ids:
        assert A.weights(k) == B.weights(k) == R.weights(k) and A.ordered(k) == B.ordered(k) == R.ordered(k) and A.tree(k) == B.tree(k) == R.tree(k), k
    la = A.local_map(frames, 2, mcap=300, stream=stream); lb = [B.local_map([f], 2, mcap=300, stream=stream)[0] for f in frames]
    for q in range(Q):
        for key in la[q]: assert (la[q][key] == lb[q][key]) if key == 'report' else np.array_equal(la[q][key], lb[q][key]), (q, key)
        check_local(la[q], R.local_map(frames[q], 2, [], -1, 300), 300)
    assert A.keyframe_culling(kq, stream=stream) == [B.keyframe_culling([k], stream=stream)[0] for k in kq] == [R.culling_votes(k) for k in kq]
    A.close(); B.close()


def check_errors(lib):
    import ctypes as C
    from sg_slam_amd.capi import SgxError, COVIS_REPORT_DTYPE
    h = C.c_void_p()
    mk = lib.dll.sgx_covis_create
    assert mk(0, 8, 8, 8, 1, 0, 1.0, C.byref(h)) == -1 and mk(4, 0, 8, 8, 1, 0, 1.0, C.byref(h)) == -1 and mk(4, 8, 8, 8, 0, 0, 1.0, C.byref(h)) == -1
    assert mk(4, 8, 8, 8, 1, 0, float('nan'), C.byref(h)) == -1 and mk(4097, 8, 8, 8, 1, 0, 1.0, C.byref(h)) == -2 and mk(4, 8193, 8, 8, 1, 0, 1.0, C.byref(h)) == -2
    assert not h.value
    G = CovisibilityGraph(max_keyframes=3, cap=4, max_points=6, max_observations=5, max_queries=2, lib=lib)
    def status(f, *a):
        try: f(*a)
        except SgxError as e: return int(str(e).rsplit('(', 1)[1].rstrip(')'))
        return 0
    z4 = [0] * 4
    assert status(G.add_keyframe, -1, z4, z4, z4) == -1 and status(G.add_keyframe, 1, [0] * 5, [0] * 5, [0] * 5) == -1 and status(G.add_keyframe, 1, [32, 0, 0, 0], z4, z4) == -1
    assert status(G.add_keyframe, 1, z4, [-1] * 4, z4) == 0 and status(G.add_keyframe, 1, z4, z4, z4) == -1
    assert status(G.add_keyframe, 2, z4, [-1] * 4, z4) == 0 and status(G.add_keyframe, 3, [0, 0], [-1, -1], [0, 0]) == 0
    assert status(G.add_keyframe, 4, z4, z4, z4) == -3 and G.size() == 3                     # full
    for bad in (([4], [0]), ([-1], [0]), ([0], [6]), ([0], [-2]), ([2], [0])):               # index / point out of range; keyframe 3 has two keypoints
        assert status(G.set_observations, 3 if bad[0] == [2] else 1, *bad) == -1
    assert status(G.set_observations, 9, [0], [0]) == -1
    assert status(G.set_observations, 1, [0, 1], [0, 1]) == 0
    before = (G.keyframe_points(1).tolist(), G.observations(0), G.observations(1), G.info()[2])
    assert status(G.set_observations, 1, [2, 3], [2, 0]) == -1                                # point 0 at a second index: refused as a whole, the first pair included
    assert status(G.set_observations, 1, [2, 0], [2, 3]) == -1                                # index 0 holds point 0
    assert status(G.set_observations, 2, [0, 1, 2, 3], [0, 1, 2, 3]) == -3                    # 2 + 4 observations > 5
    assert (G.keyframe_points(1).tolist(), G.observations(0), G.observations(1), G.info()[2]) == before and G.keyframe_points(2).tolist() == [-1] * 4
    assert status(G.set_observations, 1, [0, 0], [-1, 3]) == 0 and G.keyframe_points(1).tolist() == [3, 1, -1, -1]      # erase, then the index is free in the same call
    assert status(G.set_points_bad, [0, 6]) == -1 and status(G.set_points_bad, [-1]) == -1 and status(G.set_points_bad, [5, 0]) == 0
    assert status(G.replace_point, 0, 6) == -1 and status(G.replace_point, -1, 0) == -1 and status(G.replace_point, 4, 4) == 0 and status(G.replace_point, 4, 5) == 0
    assert status(G.erase_keyframe, 9) == -1 and status(G.weights, 9) == -1 and status(G.ordered, 9) == -1 and status(G.tree, 9) == -1 and status(G.observations, 6) == -1
    # per-query statuses of a batch: an unknown keyframe beside a good one
    rep = G.update_connections([9, 1])
    assert [int(r['status']) for r in rep] == [-1, 0]
    assert G.keyframe_culling([9, 1]) == [None, []]
    # a frame longer than its row, an id out of range, a negative count: status -1 and nothing else of that query written
    out = G.local_map([[3, 6], [3, 1]], 0, mcap=4)
    assert int(out[0]['report']['status']) == -1 and out[0]['n_points'] == 0 and list(out[0]['frame']) == [3, 6] and out[0]['local_kf'] == []
    assert int(out[1]['report']['status']) == 0 and list(out[1]['points']) == [3, 1] and out[1]['local_kf'] == [1]
    dll = lib.dll
    assert dll.sgx_covis_update_connections_batch_dev(G.h, 3, None, None, None) == -1 and dll.sgx_covis_update_connections_batch_dev(G.h, -1, None, None, None) == -1
    assert dll.sgx_covis_update_connections_batch_dev(G.h, 1, None, None, None) == -1 and dll.sgx_covis_update_connections_batch_dev(G.h, 0, None, None, None) == 0
    assert dll.sgx_covis_keyframe_culling_batch_dev(G.h, 1, None, 0, None, None, None, None, None, None) == -1
    assert dll.sgx_covis_local_map_batch_dev(G.h, 1, -1, *([None] * 7), 4, *([None] * 5)) == -1
    # erase gives the slot back; keyframe 0 is never erased
    assert status(G.erase_keyframe, 2) == 0 and status(G.add_keyframe, 0, z4, [-1] * 4, z4) == 0 and status(G.erase_keyframe, 0) == 0 and G.size() == 3
    G.clear()
    assert G.size() == 0 and G.info()[2] == 0 and status(G.add_keyframe, 1, z4, z4, z4) == 0
    G.close()


def check_slot_reuse(lib):
    """more keyframes over time than slots: an erased keyframe's slot comes back once no list names it, and its stale entries never leak into the keyframe that takes it"""
    case = dict(name='reuse', max_keyframes=6, cap=32, max_points=400, max_queries=4, ops=[])
    b = Builder()
    for t in range(20):
        kid = t + 1
        b.kf(kid, n=32)
        if t: b.pts(15, [kid, kid - 1])
        b.op('uc', [kid])
        if t >= 3: b.op('erasekf', kid - 3)
    case['ops'] = b.case('reuse')['ops']
    run_script(lib, case)


def check_large(lib, stream=None):
    """512 keyframes of about 1 000 points, Q = 64: the device against the restatement (most of the time is the restatement's)"""
    rng = np.random.RandomState(9)
    nkf, npts, per, win = 512, 200000, 1000, 2000      # neighbours at +-5 keyframes share from about 400 points down to about the gate of 15
    G = CovisibilityGraph(max_keyframes=nkf, cap=1024, max_points=npts, max_observations=nkf * per, max_queries=64, lib=lib)
    R = covis_ref.Map(False, TH_DEPTH, npts)
    ids = []
    for t in range(nkf):
        o = rng.randint(0, 8, per).astype('i4'); u = np.where(rng.rand(per) < 0.3, 5.0, -1.0).astype('f4'); d = rng.uniform(0.5, 80.0, per).astype('f4')
        c = int(t * (npts - win) / (nkf - 1)); seen = [int(p) for p in rng.choice(np.arange(c, c + win), per, replace=False)]
        for g in (G, R): g.add_keyframe(t, o, u, d); g.set_observations(t, list(range(per)), seen)
        ids.append(t)
    listed = 0
    for at in range(0, nkf, 64):
        rep = G.update_connections(ids[at:at + 64], stream)
        assert [tuple(int(r[f]) for f in REPORT_UC) for r in rep] == [R.update_connections(k) for k in ids[at:at + 64]]
        listed += int(rep['n_ordered'].sum())
    assert listed > 4 * nkf
    for k in ids[::37]: assert G.ordered(k) == R.ordered(k) and G.weights(k) == R.weights(k) and G.tree(k) == R.tree(k)
    frames = []
    for q in range(64):
        c = rng.randint(0, npts - win); frames.append([int(p) for p in rng.choice(np.arange(c, c + win), 800)])
    got = G.local_map(frames, 3, mcap=20000, stream=stream)
    for q in range(64): check_local(got[q], R.local_map(frames[q], 3, [], -1, 20000), 20000)
    kq = [int(k) for k in rng.choice(ids, 64, replace=False)]
    votes = G.keyframe_culling(kq, stream=stream)
    assert votes == [R.culling_votes(k) for k in kq] and sum(len(v) for v in votes) > 4 * 64 and sum(x[1] for v in votes for x in v) > 0
    G.close()


def check_chain(lib, oracle, S, stream=None):
    """the two consumers.  UpdateConnections -> best_covisibles -> KeyFrameDatabase.set_covisibility gives the relocalisation candidates that feeding it from the
    restatement gives; local_map -> a gather of the per-point attributes by the returned ids -> the local-map matcher gives the matches that the same gather over the
    restatement's local map gives."""
    import kfdb_cases as kc
    from scenes import make_local_map, CAM
    from sg_slam_amd.keyframedatabase import KeyFrameDatabase
    from sg_slam_amd.matcher import ORBmatcher
    cur, lm = make_local_map(oracle, S, 12, seed=1)
    nm = len(lm['xw']); rng = np.random.RandomState(4)
    nkf = 30; per = min(200, nm // 4); win = max(per + 1, nm // 3)
    G = CovisibilityGraph(max_keyframes=64, cap=256, max_points=nm, max_observations=nkf * per, max_queries=4, lib=lib)
    R = covis_ref.Map(False, TH_DEPTH, nm)
    voc = kc.make_voc(lib, 2000); dbs = [KeyFrameDatabase(voc, max_keyframes=64, max_queries=4, lib=lib) for _ in range(2)]
    bows = []
    for t in range(nkf):
        o = rng.randint(0, 8, per).astype('i4'); u = np.full(per, -1, 'f4'); d = np.ones(per, 'f4')
        c = int(t * (nm - win) / (nkf - 1)); seen = [int(p) for p in rng.choice(np.arange(c, c + win), per, replace=False)]
        for g in (G, R): g.add_keyframe(t + 1, o, u, d); g.set_observations(t + 1, list(range(per)), seen)
        bows.append(kc.bow_of(rng.randint(100 * (t // 5), 100 * (t // 5) + 150, 60), rng=rng))
        for db in dbs: db.add(t + 1, bows[-1])
    ids = list(range(1, nkf + 1))
    for at in range(0, nkf, 4):
        G.update_connections(ids[at:at + 4], stream)
        for k in ids[at:at + 4]: R.update_connections(k)
    listed = 0
    for k in ids:
        a, b = G.best_covisibles(k, 10), R.best_covisibles(k, 10)
        listed += len(a); dbs[0].set_covisibility(k, a); dbs[1].set_covisibility(k, b)
    assert listed > nkf
    some = 0
    for t in (3, 11, 17, 29):
        q = kc.bow_of(list(bows[t][0][::2]) + list(bows[(t + 1) % nkf][0][::5]), rng=rng)
        ca, cb = dbs[0].DetectRelocalizationCandidates(q), dbs[1].DetectRelocalizationCandidates(q)
        assert list(ca) == list(cb); some += len(ca)
    assert some
    for db in dbs: db.close()
    voc.close()
    # the frame tracks a few points of the middle of the map; its local map feeds the matcher
    frame = [int(p) for p in rng.choice(np.arange(nm // 3, nm // 3 + win), 40)]
    got = G.local_map([frame], 0, mcap=4096, stream=stream)[0]; ref = R.local_map(frame, 0, [], -1, 4096)
    check_local(got, ref, 4096)
    assert 200 < got['n_points'] <= 4096
    sf = oracle.orb_params()['scale']
    out = []
    for pts, obs in ((got['points'], got['obs']), (np.asarray(ref['points']), np.asarray(ref['obs'], 'i4'))):
        sub = {k: np.ascontiguousarray(lm[k][pts]) for k in ('xw', 'normal', 'min_dist', 'max_dist', 'desc', 'skip')}
        sub['obs'] = np.ascontiguousarray(obs, 'i4')
        c = {k: (v.copy() if hasattr(v, 'copy') else v) for k, v in cur.items()}
        n = ORBmatcher(0.8, True, lib=lib).SearchByProjectionLocal(c, sub, 3.0, CAM, sf)
        out.append((n, c['match_local'].copy(), sub['in_view'].copy()))
    assert out[0][0] == out[1][0] and (out[0][1] == out[1][1]).all() and (out[0][2] == out[1][2]).all()
    exp_match, exp_n, exp_view = oracle.search_by_projection_local(cur, {**{k: np.ascontiguousarray(lm[k][got['points']]) for k in ('xw', 'normal', 'min_dist', 'max_dist', 'desc', 'skip')},
                                                                         'obs': np.ascontiguousarray(got['obs'], 'i4')}, CAM, sf, th=3.0, nnratio=0.8)
    assert out[0][0] == exp_n > 20 and (out[0][1] == exp_match).all()
    G.close()


def check_host_entries(lib):
    """the host-pointer entries (a batch of one, staged and read back) give what the batch entries give"""
    import ctypes as C
    from sg_slam_amd.capi import _vp, COVIS_REPORT_DTYPE
    case = walk_script(6, nkf=20, mutate=False)
    ops = [o for o in case['ops'] if o[0] in ('kf', 'obs')]
    G = make_graph(lib, case); R = covis_ref.Map(False, TH_DEPTH, G.max_points)
    for o in ops:
        G.add_keyframe(*o[1:]) if o[0] == 'kf' else G.set_observations(*o[1:])
        apply_ref(R, o)
    ids = [o[1] for o in ops if o[0] == 'kf']
    rep = np.zeros(1, COVIS_REPORT_DTYPE)
    for k in ids:
        assert lib.dll.sgx_covis_update_connections(G.h, k, _vp(rep)) == 0
        assert tuple(int(rep[0][f]) for f in REPORT_UC) == R.update_connections(k)
    assert lib.dll.sgx_covis_update_connections(G.h, 999, _vp(rep)) == -1
    frame = np.array([5, 40, 41, 499, -1, 120, 120], 'i4'); want = R.local_map([int(p) for p in frame], 2, [], -1, 4096)
    for mcap in (4096, 7):
        f = frame.copy(); lk = np.full(G.max_keyframes, -1, 'i4'); nlk = C.c_int32(0); ref = C.c_int32(-1); rt = C.c_int32(); pts = np.full(mcap, -1, 'i4'); obs = pts.copy(); npts = C.c_int32()
        rc = lib.dll.sgx_covis_local_map(G.h, len(f), _vp(f), 2, _vp(lk), C.byref(nlk), C.byref(ref), C.byref(rt), mcap, _vp(pts), _vp(obs), C.byref(npts), _vp(rep))
        assert rc == (0 if want['n_points'] <= mcap else -3) and npts.value == want['n_points'] > 7
        assert list(f) == want['frame'] and list(lk[:nlk.value]) == want['local_kf'] and ref.value == want['ref_kf'] and rt.value == want['ref_tracked']
        assert list(pts[:min(mcap, npts.value)]) == want['points'][:mcap] and list(obs[:min(mcap, npts.value)]) == want['obs'][:mcap]
    bad = np.array([G.max_points], 'i4'); nlk = C.c_int32(0)
    assert lib.dll.sgx_covis_local_map(G.h, 1, _vp(bad), 0, _vp(lk), C.byref(nlk), C.byref(ref), C.byref(rt), 7, _vp(pts), _vp(obs), C.byref(npts), None) == -1
    M = G.max_keyframes
    for k in ids[::3]:
        cand = np.zeros(M, 'i4'); red = cand.copy(); mps = cand.copy(); cull = cand.copy(); nc = C.c_int32()
        assert lib.dll.sgx_covis_keyframe_culling(G.h, k, M, _vp(cand), C.byref(nc), _vp(red), _vp(mps), _vp(cull)) == 0
        assert [(int(cand[r]), int(red[r]), int(mps[r]), int(cull[r])) for r in range(nc.value)] == R.culling_votes(k)
    assert lib.dll.sgx_covis_keyframe_culling(G.h, 999, M, _vp(cand), C.byref(nc), _vp(red), _vp(mps), _vp(cull)) == -1
    G.close()
