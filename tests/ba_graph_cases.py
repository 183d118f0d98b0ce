"""Shared cases for the bundle-adjustment graph query of the covisibility handle (sgx_covis_ba_graph*): hand-made cases with written answers (one per rule), the generated
walks and shapes of tests/covis_cases.py queried after their mutations, shapes of this query's own, and the runner that plays a script on the device (or the emulator)
and on the restatement of tests/ba_graph_ref.py and compares them: every comparison is equality of integers.  A script is one of covis_cases with
  ('ba', kf ids[, expect dict per query]) ('gba'[, expect]) ('erase', kf id, [(keyframe id, point id)] to flag[, vToErase as written])
added; without any 'ba' op the runner queries the keyframes of every 'uc' op."""
import numpy as np
import covis_ref
import covis_cases as cc
import ba_graph_ref as br

ROWS = ('pose_id', 'pose_fixed', 'point_id', 'point_edge_begin', 'edge_pose', 'edge_point', 'edge_kp', 'edge_attr')
REPORT = ('status', 'n_local_kf', 'n_fixed_kf', 'n_poses', 'n_points', 'n_edges', 'n_mono_edges', 'n_stereo_edges')


def check_graph(got, want, what=''):
    assert got['status'] == want['status'], (what, got['status'], want['status'])
    if want['status'] == -1:
        assert int(got['report']['status']) == -1 and not any(int(got['report'][k]) for k in REPORT[1:]), what
        return
    for k in REPORT: assert int(got['report'][k]) == want['report'][k], (what, k, int(got['report'][k]), want['report'][k])
    for k in ROWS: assert [int(x) for x in got[k]] == [int(x) for x in want[k]], (what, k, list(got[k]), want[k])


def same_graph(a, b):
    assert a['status'] == b['status'] and a['report'].tobytes() == b['report'].tobytes()
    if a['status'] != -1:
        for k in ROWS: assert a[k].dtype == b[k].dtype and a[k].tobytes() == b[k].tobytes(), k


def query(G, R, kf_ids, mode=0, stream=None, caps=False, expect=None, name='', ev=br.EVENTS):
    """the batch on the device against the restatement; with caps also every query alone with pcap / ecap exactly the need and one short of it.  G = None: the
    restatement alone (its rule events are counted in ev)."""
    S = [br.BundleAdjustment(R)] if mode else [br.LocalBundleAdjustment(R, k, ev) for k in kf_ids]
    got = G.ba_graph_batch(kf_ids, mode, stream=stream) if G is not None else [None] * len(S)
    assert len(got) == len(S)
    for q, (g, s) in enumerate(zip(got, S)):
        want = br.flatten(s, ev=ev)
        if G is not None: check_graph(g, want, (name, q))
        for key, v in ((expect or [{}] * len(S))[q]).items():
            w = want['report'][key] if key in REPORT[1:] else want[key]
            assert w == v, (name, q, key, w, v)
        if not caps or s is None: continue
        npt, ne = want['report']['n_points'], want['report']['n_edges']
        for pcap, ecap in ((npt, ne), (npt - 1, ne), (npt, ne - 1), (0, ne), (npt, 0)):
            if pcap < 0 or ecap < 0: continue
            w2 = br.flatten(s, pcap, ecap, ev)
            assert w2['status'] == (-3 if pcap < npt or ecap < ne else 0)
            if G is not None: check_graph(G.ba_graph_batch(kf_ids[q:q + 1], mode, pcap, ecap, stream)[0], w2, (name, q, pcap, ecap))
    return got, S


# ---- hand-made cases ------------------------------------------------------------------------------------------------------------------------------------------------
def hand_cases():
    C = []
    # a dead keyframe in the ordered list is marked but not local: 5's list is [7, 6] with 6 erased; the points 5 shared with 6 went with it (nObs 1)
    b = cc.Builder()
    for k in (5, 6, 7): b.kf(k)
    b.pts(3, [5, 6]); b.pts(15, [5, 7])
    b.op('uc', [5]); b.op('erasekf', 6); b.pts(1, [5, 7]); b.op('uc', [7]); b.x('ordered', 5, ([7, 6], [16, 3]))
    b.op('ba', [5], [dict(pose_id=[5, 7], pose_fixed=[0, 0], point_id=list(range(3, 19)), n_local_kf=2, n_fixed_kf=0, n_edges=32, edge_pose=[0, 1] * 16)])
    C.append(b.case('dead-keyframe-in-the-list'))
    # a list in single-neighbour mode: of 2, 3 (5 points each) and 4 (3 points) only 2 is listed, 3 and 4 are fixed cameras
    b = cc.Builder()
    for k in (1, 2, 3, 4): b.kf(k)
    b.pts(5, [1, 2]); b.pts(5, [1, 3]); b.pts(3, [1, 4])
    b.op('uc', [1]); b.x('ordered', 1, ([2], [5]))
    b.op('ba', [1], [dict(pose_id=[1, 2, 3, 4], pose_fixed=[0, 0, 1, 1], point_id=list(range(13)), n_local_kf=2, n_fixed_kf=2, n_edges=26)])
    C.append(b.case('single-neighbour-list'))
    # a list in all mode: an AddConnection with a new weight rebuilt 1's list from its whole map, so 3 at weight 3 is a local keyframe
    b = cc.Builder()
    for k in (1, 2, 3): b.kf(k)
    b.pts(15, [1, 2]); b.pts(3, [1, 3])
    b.op('uc', [1]); b.x('ordered', 1, ([2], [15]))
    b.op('ba', [1], [dict(pose_id=[1, 2, 3], pose_fixed=[0, 0, 1])])
    b.pts(1, [1, 2]); b.op('uc', [2]); b.x('ordered', 1, ([2, 3], [16, 3]))
    b.op('ba', [1], [dict(pose_id=[1, 2, 3], pose_fixed=[0, 0, 0], n_local_kf=3)])
    C.append(b.case('all-mode-list-under-the-gate'))
    # keyframe 0 as a local keyframe is pose_fixed 2, as a fixed camera 1, and as the query's own keyframe 2
    b = cc.Builder()
    for k in (0, 1, 2): b.kf(k, n=128)
    b.pts(20, [0, 1]); b.pts(16, [1, 2])
    b.op('uc', [1]); b.x('ordered', 1, ([0, 2], [20, 16]))
    b.op('uc', [2]); b.x('ordered', 2, ([1], [16]))
    b.op('ba', [1, 2, 0], [dict(pose_id=[0, 1, 2], pose_fixed=[2, 0, 0]), dict(pose_id=[0, 1, 2], pose_fixed=[1, 0, 0], point_id=list(range(20, 36)) + list(range(20))),
                           dict(pose_id=[0, 1, 2], pose_fixed=[2, 0, 1], point_id=list(range(36)))])      # 1's AddConnection put 1 into 0's list
    b.op('gba', [dict(pose_id=[0, 1, 2], pose_fixed=[2, 0, 0], point_id=list(range(36)), n_fixed_kf=0, n_edges=72)])
    C.append(b.case('keyframe-0-local-and-fixed'))
    # a point reached through two local keyframes keeps its first position: s (31) comes with 2, before y (33) of 2 and x (32) of 3
    b = cc.Builder()
    for k in (1, 2, 3): b.kf(k)
    b.pts(16, [1, 2]); b.pts(15, [1, 3]); s = b.pt([2, 3]); x = b.pt([3]); y = b.pt([2])
    b.op('uc', [1]); b.x('ordered', 1, ([2, 3], [16, 15]))
    b.op('ba', [1], [dict(point_id=list(range(31)) + [s, y, x], n_points=34, n_edges=66)])
    C.append(b.case('first-occurrence-keeps-its-position'))
    # a fixed camera seen only through the last local point
    b = cc.Builder()
    for k in (1, 2, 9): b.kf(k)
    b.pts(15, [1, 2]); z = b.pt([2, 9])
    b.op('uc', [1]); b.x('ordered', 1, ([2], [15]))
    b.op('ba', [1], [dict(pose_id=[1, 2, 9], pose_fixed=[0, 0, 1], point_id=list(range(15)) + [z], edge_pose=[0, 1] * 15 + [1, 2], edge_point=sorted(list(range(16)) * 2))])
    C.append(b.case('fixed-camera-through-the-last-point'))
    # a keyframe with no points and no neighbours: one pose, zero points, zero edges
    b = cc.Builder()
    b.kf(4, n=8); b.kf(5, n=8); b.pts(2, [5])
    b.op('ba', [4], [dict(pose_id=[4], pose_fixed=[0], point_id=[], point_edge_begin=[0], edge_pose=[], n_poses=1, n_points=0, n_edges=0)])
    C.append(b.case('lonely-keyframe'))
    # the attribute byte: octave, RIGHT of a stereo keypoint, CLOSE by depth; a stereo edge counts as one edge
    b = cc.Builder()
    b.kf(1, n=4, octave=[3, 0, 0, 0], uright=[-1.0, 2.0, -1, -1], depth=[1.0, 50.0, 1, 1]); b.kf(2, n=4, octave=7, uright=5.0, depth=-1.0)
    b.pt([1, 2]); b.pt([1])
    b.op('ba', [1], [dict(edge_attr=[3 | 64, 7 | 32, 0 | 32], edge_kp=[0, 0, 1], n_mono_edges=1, n_stereo_edges=2, pose_fixed=[0, 1])])
    C.append(b.case('attribute-byte'))
    # an erase that drives a point to nObs <= 2: its other observations go with it
    b = cc.Builder()
    for k in (1, 2, 3): b.kf(k, n=8)
    p = b.pt([1, 2, 3]); q = b.pt([1, 2])
    b.op('erase', 1, [(2, p)], [(2, p)])
    b.x('observations', p, ([], 0)); b.x('keyframe_points', 1, [-1, q] + [-1] * 6); b.x('keyframe_points', 3, [-1] * 8); b.x('observations', q, ([(1, 1), (2, 1)], 2))
    C.append(b.case('erase-to-two-observations'))
    # a monocular and a stereo flagged edge of one point: the stereo edge of keyframe 1 comes first among the edges, the monocular one of keyframe 4 first in vToErase;
    # it takes the point from nObs 3 to 2, so the stereo pair finds nothing to erase
    b = cc.Builder()
    b.kf(1, n=8, uright=3.0); b.kf(4, n=8); b.kf(6, n=8)
    p = b.pt([1, 4]); q = b.pt([1, 4, 6])
    b.op('erase', 4, [(1, p), (4, p), (6, q)], [(4, p), (6, q), (1, p)])
    b.x('observations', p, ([], 0)); b.x('observations', q, ([(1, 1), (4, 1)], 3))
    C.append(b.case('erase-monocular-before-stereo'))
    return C


# ---- generated ------------------------------------------------------------------------------------------------------------------------------------------------------
def all_generated():
    """the walks and shapes of covis_cases, queried after their mutations (at every UpdateConnections batch)"""
    return cc.all_generated() + [cc.shapes_script(n) for n in (1, 2, 63, 64, 65)]


def long_lists_script(seed=3):
    """points observed by 1, 2, 8, 9, 16, 17, 64, 65 and 257 keyframes (a chunk boundary, a wave, more than a workgroup of 256), the keyframe ids in an order that is
    neither that of the slots nor that of the chains"""
    rng = np.random.RandomState(seed)
    lens = [1, 2, 8, 9, 16, 17, 64, 65, 257]; nkf = 257; cap = 12
    ids = [int(i) for i in rng.permutation(nkf * 3)[:nkf]]
    ops = []
    for t, kid in enumerate(ids):
        ops.append(('kf', kid, rng.randint(0, 8, cap).astype('i4'), np.where(rng.rand(cap) < 0.4, 2.0, -1.0).astype('f4'), rng.uniform(0.5, 80.0, cap).astype('f4')))
    for t in rng.permutation(nkf):
        pts = [j for j, n in enumerate(lens) if t < n]
        if t % 5 == 0: pts.append(len(lens) + int(t))                           # a point of its own
        idx = [int(i) for i in rng.permutation(cap)[:len(pts)]]
        ops.append(('obs', ids[t], idx, pts))
    ops.append(('uc', [ids[0], ids[1], ids[7], ids[200]]))
    ops.append(('ba', [ids[0], ids[1], ids[15], ids[64], ids[256], ids[100]]))
    ops.append(('gba',))
    return dict(name='long-lists', ops=ops, max_keyframes=260, cap=cap, max_points=len(lens) + nkf, max_queries=8)


# ---- the runner -----------------------------------------------------------------------------------------------------------------------------------------------------
def erase(G, R, kf_id, pick, stream, name, ev, points, written=None):
    """the graph of kf_id, the edges pick(S) flags erased on both sides, the states compared"""
    S = br.LocalBundleAdjustment(R, kf_id, ev)
    flags = pick(S)
    g = G.local_ba_graph(kf_id, stream=stream) if G is not None else None
    if G is not None: check_graph(g, br.flatten(S, ev=ev), name)
    want = br.apply_erase(R, S, flags, ev)
    if written is not None: assert want == written, (name, want, written)
    if G is not None:
        done = G.apply_ba_erase(g, flags)
        assert done == want, (name, done, want)
        cc.compare_state(G, R, points)


def run_script(lib, case, stream=None, caps_every=3, erase_every=5, ev=br.EVENTS):
    """lib = None: the restatement alone, which counts its rule events in ev for the same inputs"""
    G = cc.make_graph(lib, case) if lib is not None else None
    R = covis_ref.Map(case.get('monocular', False), cc.TH_DEPTH, case.get('max_points', 2048))
    explicit = any(op[0] in ('ba', 'gba', 'erase') for op in case['ops'])
    max_q = case.get('max_queries', 8)
    points = set(); nq = 0
    for op in case['ops']:
        k = op[0]
        if k == 'x':
            want = getattr(R, op[1])(*op[2])
            assert want == op[3], (case['name'], op[1], op[2], want, op[3])
            if G is None: continue
            got = getattr(G, op[1])(*op[2])
            assert (list(got) if op[1] == 'keyframe_points' else got) == op[3], (case['name'], 'device', op[1], op[2], got, op[3])
        elif k == 'ba':
            query(G, R, op[1], 0, stream, caps=True, expect=op[2] if len(op) > 2 else None, name=case['name'], ev=ev)
        elif k == 'gba':
            query(G, R, [], 1, stream, caps=True, expect=op[1] if len(op) > 1 else None, name=case['name'], ev=ev)
        elif k == 'erase':
            def pick(S, pairs=op[2]):
                flags = [(e[0].mnId, e[1].mnId) in pairs for e in S['edges']]
                assert sum(flags) == len(pairs)
                return flags
            erase(G, R, op[1], pick, stream, case['name'], ev, points, op[3] if len(op) > 3 else None)
        elif k in ('lm', 'cull'): continue
        else:
            ref = cc.apply_ref(R, op)
            if k == 'obs': points.update(p for p in op[3] if p >= 0)
            if G is not None:
                if k == 'kf': G.add_keyframe(op[1], op[2], op[3], op[4])
                elif k == 'obs': G.set_observations(op[1], op[2], op[3])
                elif k == 'bad': G.set_points_bad(op[1])
                elif k == 'replace': G.replace_point(op[1], op[2])
                elif k == 'erasekf': G.erase_keyframe(op[1])
                elif k == 'cullloop': assert cc.culling_caller_loop(G, op[1]) == ref
                elif k == 'uc': G.update_connections(op[1], stream)
            if k == 'uc' and not explicit:                                        # a generated script: the keyframes just updated, now and then the whole map, an erase
                nq += 1; ids = [int(i) for i in op[1]][:max_q]
                query(G, R, ids, 0, stream, caps=nq % caps_every == 0, name=case['name'], ev=ev)
                if nq % caps_every == 1: query(G, R, [], 1, stream, caps=nq % (2 * caps_every) == 1, name=case['name'], ev=ev)
                if nq % caps_every == 2:                                          # keyframes whose lists name an erased keyframe: not those just updated
                    stale = [i for i in sorted(R.kfs) if any(x not in R.kfs for x in R.ordered(i)[0])][:max_q]
                    if stale: query(G, R, stale, 0, stream, name=case['name'], ev=ev)
                if nq % erase_every == 0: erase(G, R, ids[-1], lambda S: [j % 11 == 3 for j in range(len(S['edges']))], stream, case['name'], ev, points)
    if G is not None:
        cc.compare_state(G, R, points); G.close()
    return R


# ---- checks shared by the CPU and the GPU tier ------------------------------------------------------------------------------------------------------------------------
def build_walk(lib, seed, nkf, Q):
    case = cc.walk_script(seed, nkf=nkf, mutate=False, Q=Q)
    case['max_queries'] = max(Q, 5)
    G = cc.make_graph(lib, case); R = covis_ref.Map(False, cc.TH_DEPTH, G.max_points)
    ids = []
    for o in case['ops']:
        if o[0] == 'kf': G.add_keyframe(*o[1:]); ids.append(o[1])
        elif o[0] == 'obs': G.set_observations(*o[1:])
        elif o[0] == 'uc': G.update_connections(o[1])
        else: continue
        cc.apply_ref(R, o)
    return G, R, ids


def check_batch_equals_singles(lib, Q, stream=None):
    """Q queries as one batch equal Q single calls byte for byte, a second run of the batch equals the first, and both equal the restatement"""
    G, R, ids = build_walk(lib, 5, 24, Q)
    G.erase_keyframe(ids[9]); R.erase_keyframe(ids[9])                            # lists that name an erased keyframe, and its id as a query
    rng = np.random.RandomState(Q)
    kq = [int(x) for x in rng.choice(ids, Q, replace=Q > len(ids))]
    if Q > 2: kq[1] = kq[0]; kq[2] = ids[9]
    a = G.ba_graph_batch(kq, stream=stream); b = G.ba_graph_batch(kq, stream=stream); s = [G.local_ba_graph(k, stream=stream) for k in kq]
    for q in range(Q):
        same_graph(a[q], b[q]); same_graph(a[q], s[q])
        check_graph(a[q], br.flatten(br.LocalBundleAdjustment(R, kq[q])), q)
    if Q > 2: assert a[2]['status'] == -1
    assert sum(int(x['report']['n_fixed_kf']) for x in a if x['status'] == 0) > 0
    # capacities short for some queries of a batch and not for others
    need = sorted(int(x['report']['n_points']) for x in a if x['status'] == 0); pcap = need[len(need) // 2]
    c = G.ba_graph_batch(kq, 0, pcap, None, stream)
    for q in range(Q): check_graph(c[q], br.flatten(br.LocalBundleAdjustment(R, kq[q]), pcap), ('pcap', q))
    g1 = G.global_ba_graph(stream=stream); g2 = G.global_ba_graph(stream=stream)
    same_graph(g1, g2); check_graph(g1, br.flatten(br.BundleAdjustment(R)), 'global')
    G.close()


def check_errors(lib):
    import ctypes as C
    from sg_slam_amd.capi import _vp, COVIS_BA_REPORT_DTYPE
    G, R, ids = build_walk(lib, 6, 8, 3)
    dll = lib.dll; N = G.max_keyframes
    def call(Q, mode, kf, pcap=4, ecap=4, drop=()):
        a = dict(kf=G._dev(np.asarray(kf, 'i4')), pid=G._dev(np.full((max(Q, 1), N), -7, 'i4')), pf=G._dev(np.full((max(Q, 1), N), 7, 'u1')), pts=G._dev(np.full((max(Q, 1), 4), -7, 'i4')),
                 beg=G._dev(np.full((max(Q, 1), 5), -7, 'i4')), ep=G._dev(np.full((max(Q, 1), 4), -7, 'i4')), el=G._dev(np.full((max(Q, 1), 4), -7, 'i4')),
                 ek=G._dev(np.full((max(Q, 1), 4), -7, 'i4')), ea=G._dev(np.full((max(Q, 1), 4), 7, 'u1')), rep=G._dev(np.zeros(max(Q, 1) * COVIS_BA_REPORT_DTYPE.itemsize, 'u1')))
        p = {k: (None if k in drop else _vp(v)) for k, v in a.items()}
        rc = dll.sgx_covis_ba_graph_batch_dev(G.h, Q, mode, p['kf'], p['pid'], p['pf'], pcap, p['pts'], p['beg'], ecap, p['ep'], p['el'], p['ek'], p['ea'], p['rep'], G._stream(None))
        G._sync(None)
        return rc, {k: G._host(v) for k, v in a.items()}
    assert call(G.max_queries + 1, 0, [ids[0]] * (G.max_queries + 1))[0] == -1 and call(-1, 0, [ids[0]])[0] == -1 and call(0, 0, [ids[0]])[0] == 0
    assert call(2, 1, [ids[0]] * 2)[0] == -1 and call(1, 2, [ids[0]])[0] == -1 and call(1, -1, [ids[0]])[0] == -1
    for drop in ('kf', 'pid', 'pf', 'pts', 'beg', 'ep', 'el', 'ek', 'ea', 'rep'): assert call(1, 0, [ids[0]], drop=(drop,))[0] == -1, drop
    assert call(1, 1, [ids[0]], drop=('kf',))[0] == 0                             # global mode does not read the ids
    # an unknown id beside a good one: its status, and nothing else of that query written; the good one short of room: the first four points, no row overrun
    rc, o = call(2, 0, [999, ids[1]])
    rep = o['rep'].view(COVIS_BA_REPORT_DTYPE)
    assert rc == 0 and int(rep[0]['status']) == -1 and int(rep[1]['status']) == -3
    for k in ('pid', 'pf', 'pts', 'beg', 'ep', 'el', 'ek', 'ea'): assert (o[k][0] == (7 if o[k].dtype == np.uint8 else -7)).all(), k
    want = br.flatten(br.LocalBundleAdjustment(R, ids[1]), 4, 4)
    assert list(o['pts'][1]) == want['point_id'] and list(o['beg'][1]) == want['point_edge_begin'] and list(o['pid'][1][:len(want['pose_id'])]) == want['pose_id']
    ne = len(want['edge_pose']); assert list(o['ep'][1][:ne]) == want['edge_pose'] and (o['ep'][1][ne:] == -7).all() and (o['ea'][1][ne:] == 7).all()
    # negative capacities: every query's status
    for pcap, ecap in ((-1, 4), (4, -1)):
        rc, o = call(2, 0, [ids[0], ids[1]], pcap, ecap)
        assert rc == 0 and [int(r['status']) for r in o['rep'].view(COVIS_BA_REPORT_DTYPE)] == [-1, -1] and (o['beg'] == -7).all() and (o['pid'] == -7).all()
    # an erased keyframe's id is no keyframe; the single entry returns the status
    G.erase_keyframe(ids[3])
    assert G.local_ba_graph(ids[3])['status'] == -1 and G.local_ba_graph(ids[2])['status'] == 0
    z = np.zeros(N, 'i4'); zb = np.zeros(N, 'u1'); b1 = np.full(1, -7, 'i4'); rp = np.zeros(1, COVIS_BA_REPORT_DTYPE)
    assert dll.sgx_covis_ba_graph(G.h, 0, ids[3], _vp(z), _vp(zb), 0, None, _vp(b1), 0, None, None, None, None, _vp(rp)) == -1 and b1[0] == -7
    assert dll.sgx_covis_ba_graph(G.h, 0, ids[2], _vp(z), _vp(zb), 0, None, _vp(b1), 0, None, None, None, None, _vp(rp)) == -3 and int(rp[0]['n_points']) > 0 and b1[0] == 0
    assert dll.sgx_covis_ba_graph(G.h, 0, ids[2], None, _vp(zb), 0, None, _vp(b1), 0, None, None, None, None, None) == -1
    assert dll.sgx_covis_ba_graph(None, 0, ids[2], _vp(z), _vp(zb), 0, None, _vp(b1), 0, None, None, None, None, None) == -1
    G.close()


def check_host_entry(lib):
    """sgx_covis_ba_graph (host pointers, a batch of one) gives what the batch entry gives, with buffers of exactly the need"""
    from sg_slam_amd.capi import _vp, COVIS_BA_REPORT_DTYPE
    G, R, ids = build_walk(lib, 6, 12, 3)
    for mode, k in ((0, ids[5]), (0, ids[0]), (1, 0)):
        want = br.flatten(br.BundleAdjustment(R) if mode else br.LocalBundleAdjustment(R, k))
        npt, ne = want['report']['n_points'], want['report']['n_edges']
        pid = np.zeros(G.max_keyframes, 'i4'); pf = np.zeros(G.max_keyframes, 'u1'); pts = np.zeros(npt, 'i4'); beg = np.zeros(npt + 1, 'i4')
        ep = np.zeros(ne, 'i4'); el = np.zeros(ne, 'i4'); ek = np.zeros(ne, 'i4'); ea = np.zeros(ne, 'u1'); rp = np.zeros(1, COVIS_BA_REPORT_DTYPE)
        assert lib.dll.sgx_covis_ba_graph(G.h, mode, k, _vp(pid), _vp(pf), npt, _vp(pts), _vp(beg), ne, _vp(ep), _vp(el), _vp(ek), _vp(ea), _vp(rp)) == 0
        npo = int(rp[0]['n_poses'])
        check_graph(dict(status=0, report=rp[0], pose_id=pid[:npo], pose_fixed=pf[:npo], point_id=pts, point_edge_begin=beg, edge_pose=ep, edge_point=el, edge_kp=ek, edge_attr=ea), want, mode)
    G.close()


def check_chain(lib, stream=None):
    """local_ba_graph -> flatten_ba_problem -> sgx_local_bundle_adjustment -> apply_ba_erase on a map of 6 keyframes x 60 points with a few gross outliers: the flattened
    arrays are byte-equal to those gathered over the restatement's lists, and after the erase the handle equals the restatement that applied the same flags with the
    reference's loop.  The solver is not under test."""
    from scenes import CAM
    from sg_slam_amd.covisibility import CovisibilityGraph
    from sg_slam_amd.optimizer import Optimizer
    rng = np.random.RandomState(17)
    nkf, npts, cap = 6, 60, 64
    inv = (1.0 / 1.2 ** (2 * np.arange(8))).astype('f4')
    X = np.stack([rng.uniform(-1.0, 2.0, npts), rng.uniform(-0.8, 0.8, npts), rng.uniform(2.5, 6.0, npts)], 1).astype('f4')
    G = CovisibilityGraph(max_keyframes=8, cap=cap, max_points=npts, max_observations=nkf * cap, max_queries=2, lib=lib)
    R = covis_ref.Map(False, cc.TH_DEPTH, npts)
    KF = {}
    for i in range(nkf):
        T = np.eye(4, dtype='f4'); T[0, 3] = -0.15 * i
        Xc = X @ T[:3, :3].T + T[:3, 3]
        u = CAM['fx'] * Xc[:, 0] / Xc[:, 2] + CAM['cx']; v = CAM['fy'] * Xc[:, 1] / Xc[:, 2] + CAM['cy']
        seen = [int(p) for p in np.flatnonzero((u > 0) & (u < 640) & (v > 0) & (v < 480) & (rng.rand(npts) < 0.85))]
        n = len(seen); octave = rng.randint(0, 8, n).astype('i4')
        uv = np.stack([u[seen], v[seen]], 1) + rng.randn(n, 2) * 0.3
        out = rng.rand(n) < 0.06
        uv[out] += rng.uniform(30, 60, (int(out.sum()), 2))                        # gross outliers
        ur = np.where(rng.rand(n) < 0.7, uv[:, 0] - CAM['bf'] / Xc[seen, 2], -1.0)
        KF[i] = dict(Tcw=T, uv=uv.astype('f4'), uright=ur.astype('f4'))
        for g in (G, R): g.add_keyframe(i, octave, KF[i]['uright'], Xc[seen, 2].astype('f4')); g.set_observations(i, list(range(n)), seen)
    G.update_connections(list(range(nkf))[:2], stream); G.update_connections(list(range(nkf))[2:4], stream); G.update_connections(list(range(nkf))[4:], stream)
    for i in range(nkf): R.update_connections(i)
    cur = nkf - 1
    g = G.local_ba_graph(cur, stream=stream); S = br.LocalBundleAdjustment(R, cur)
    check_graph(g, br.flatten(S), 'chain')
    assert int(g['report']['n_poses']) == nkf and int(g['report']['n_points']) > 40 and int(g['report']['n_stereo_edges']) > 0 < int(g['report']['n_mono_edges'])
    prob = Optimizer.flatten_ba_problem(g, KF, X, inv)
    poses = sorted(S['local'] + S['fixed'], key=lambda k: k.mnId)
    want = dict(poses=np.stack([KF[k.mnId]['Tcw'] for k in poses]), pose_fixed=np.array([1 if k in S['fixed'] else 2 if k.mnId == 0 else 0 for k in poses], 'u1'),
                points=np.stack([X[p.mnId] for p in S['points']]), edge_pose=np.array([poses.index(e[0]) for e in S['edges']], 'i4'),
                edge_point=np.array([S['points'].index(e[1]) for e in S['edges']], 'i4'),
                edge_obs=np.array([[KF[e[0].mnId]['uv'][e[2], 0], KF[e[0].mnId]['uv'][e[2], 1], KF[e[0].mnId]['uright'][e[2]] if e[3] else -1.0] for e in S['edges']], 'f4'),
                edge_info=np.array([inv[e[0].octave[e[2]]] for e in S['edges']], 'f4'))
    for k, v in want.items(): assert prob[k].dtype == v.dtype and prob[k].shape == v.shape and prob[k].tobytes() == v.tobytes(), k
    erase, _ = Optimizer.LocalBundleAdjustment(prob, CAM, lib=lib)
    assert 0 < int(erase.sum()) < len(erase) // 4
    done = G.apply_ba_erase(g, erase)
    assert done == br.apply_erase(R, S, [bool(x) for x in erase])
    cc.compare_state(G, R, set(range(npts)))
    G.close()
