"""Shared cases for loop closing on the covisibility handle (sgx_covis_add_loop_edge, sgx_covis_loop_begin, sgx_covis_loop_connections, sgx_covis_essential_graph):
hand-made cases with written answers, generated walks with loops closed at random, shapes of these entries' own, and the runner that plays a script on the device (or
the emulator) and on the restatement of tests/loop_ref.py and compares them: every comparison is equality of integers.  A script is one of covis_cases with
  ('le', a, b[, status])                       add_loop_edge (status: 0, -1, -3 as written)
  ('begin', cur[, expect])                     loop_begin
  ('conn', cur, group ids[, expect])           loop_connections
  ('eg', cur, loop, group ids, {member id: [target ids]}[, expect edges [(id of vertex 0, id of vertex 1, kind)]])      essential_graph on a hand-made CSR
  ('round', cur, loop, fuse ops[, expect])     begin -> the fuse ops -> connections -> essential graph -> add_loop_edge, every capacity at the need and one short
added."""
import numpy as np
import covis_ref
import covis_cases as cc
import loop_ref as lr
from sg_slam_amd.capi import SgxError

REPORT = ('status', 'n_group', 'n_points', 'n_connections', 'n_vertices', 'n_edges')


def check_report(got, want, what):
    for k in REPORT:
        if k in want: assert int(got[k]) == want[k], (what, k, int(got[k]), want[k])
    if 'n_kind' in want: assert [int(x) for x in got['n_kind']] == want['n_kind'], (what, list(got['n_kind']), want['n_kind'])


def same(got, want, keys, what):
    for k in keys: assert [int(x) for x in got[k]] == [int(x) for x in want[k]], (what, k, list(got[k]), want[k])


def status_of(f, *a):
    try: f(*a)
    except SgxError as e: return int(str(e).rsplit('(', 1)[1].rstrip(')'))
    except covis_ref.Invalid: return -1
    except lr.NoMem: return -3
    return 0


def begin(G, R, cur, pcap=None, stream=None, what='', ev=lr.EVENTS):
    want = lr.flatten_begin(R, lr.loop_begin(R, cur, ev), 1 << 30 if pcap is None else pcap, ev)
    if G is None: return want
    got = G.loop_begin(cur, pcap, stream)
    assert got['status'] == want['status'], (what, got['status'], want['status'])
    check_report(got['report'], want['report'], what); same(got, want, ('group_id', 'group_vertex', 'point_id', 'point_ref'), what)
    return want


def connections(G, R, cur, group, lcap=None, stream=None, what='', ev=lr.EVENTS):
    want = lr.flatten_connections(lr.loop_connections(R, cur, group, ev), 1 << 30 if lcap is None else lcap, ev)
    if G is None: return want
    got = G.loop_connections(cur, group, lcap, stream)
    assert got['status'] == want['status'], (what, got['status'], want['status'])
    if want['status'] == -1:
        assert (got['raw'][0] == -1).all() and (got['raw'][1] == -1).all(), what          # nothing written
        return want
    check_report(got['report'], want['report'], what); same(got, want, ('lc_begin', 'lc_j'), what)
    assert (got['raw'][1][len(want['lc_j']):] == -1).all(), what                           # the remainder of the row is untouched
    return want


def graph(G, R, cur, loop, group, lc_begin, lc_j, ecap=None, stream=None, what='', ev=lr.EVENTS):
    want = lr.flatten_graph(lr.essential_graph(R, cur, loop, group, lc_begin, lc_j, ev), 1 << 30 if ecap is None else ecap, ev)
    if G is None: return want
    got = G.essential_graph(cur, loop, group, lc_begin, lc_j, ecap, stream)
    assert got['status'] == want['status'], (what, got['status'], want['status'])
    vid, vfx, vgr, ei, ej, ek = got['raw']
    if want['status'] == -1:
        assert (vid == -1).all() and (vfx == 255).all() and (vgr == -9).all() and (ei == -1).all() and (ek == 255).all(), what
        return want
    check_report(got['report'], want['report'], what); same(got, want, ('vertex_id', 'vertex_fixed', 'vertex_group', 'e_i', 'e_j', 'e_kind'), what)
    ne = len(want['e_i']); nv = len(want['vertex_id'])
    assert (ei[ne:] == -1).all() and (ej[ne:] == -1).all() and (ek[ne:] == 255).all() and (vid[nv:] == -1).all() and (vgr[nv:] == -9).all(), what
    return want


def csr_of(R, group, lc):
    """a hand-made {member id: [target ids]} as the CSR over the members in ascending id"""
    begin = [0]; j = []
    for i in sorted(group): j += list(lc.get(i, [])); begin.append(len(j))
    return begin, j


def loop_round(G, R, cur, loop, fuse, mode=0, stream=None, what='', ev=lr.EVENTS, points=None, expect=None, add_edge=True):
    """one CorrectLoop.  mode 0: default capacities; 1: every capacity exactly the need; 2: one short of it.  The need is the restatement's, which is played first."""
    expect = expect or {}
    if mode == 0: wb = begin(G, R, cur, None, stream, (what, 'begin'), ev)
    else:
        # the need of the point row: that of a first call with room; the call is played on both sides, and the second call (the state it left) is the one with the cap
        wb0 = begin(G, R, cur, None, stream, (what, 'begin0'), ev)
        npt = wb0['report']['n_points']
        wb = begin(G, R, cur, npt if mode == 1 else max(npt - 1, 0), stream, (what, 'begin', mode), ev)
        assert wb['status'] == (-3 if mode == 2 and npt > 0 else 0)
    group = wb['group_id']
    for key in ('group_id', 'point_id', 'point_ref'):
        if key in expect: assert wb[key] == expect[key], (what, key, wb[key], expect[key])
    for op in fuse:
        cc.apply_ref(R, op)
        if op[0] == 'obs' and points is not None: points.update(p for p in op[3] if p >= 0)
        if G is not None:
            if op[0] == 'replace': G.replace_point(op[1], op[2])
            elif op[0] == 'obs': G.set_observations(op[1], op[2], op[3])
            elif op[0] == 'bad': G.set_points_bad(op[1])
            else: raise ValueError(op[0])
    # the need of the connections: the restatement's (complete whatever the capacity), the device gets the capacity
    LC = lr.loop_connections(R, cur, group, ev)
    full = lr.flatten_connections(LC, ev=dict(ev))
    need = full['report']['n_connections']
    lcap = None if mode == 0 else need if mode == 1 else max(need - 1, 0)
    wc = lr.flatten_connections(LC, 1 << 30 if lcap is None else lcap, ev)
    if G is not None:
        got = G.loop_connections(cur, group, lcap, stream)
        assert got['status'] == wc['status'] == (-3 if mode == 2 and need > 0 else 0), (what, got['status'], wc['status'])
        check_report(got['report'], wc['report'], what); same(got, wc, ('lc_begin', 'lc_j'), (what, 'conn', mode))
        assert (got['raw'][1][len(wc['lc_j']):] == -1).all(), what
    if 'lc' in expect: assert {k.mnId: sorted(x.mnId for x in s) for k, s in LC.items() if s} == expect['lc'], (what, expect['lc'])
    wg = graph(G, R, cur, loop, group, full['lc_begin'], full['full'], None, stream, (what, 'graph'), ev)
    if 'edges' in expect: assert wg['edges_by_id'] == expect['edges'], (what, wg['edges_by_id'], expect['edges'])
    if mode:
        ne = wg['report']['n_edges']
        for ecap in ((ne,) if mode == 1 else (max(ne - 1, 0), 0)):
            w2 = graph(G, R, cur, loop, group, full['lc_begin'], full['full'], ecap, stream, (what, 'graph', ecap), ev)
            assert w2['status'] == (-3 if ecap < ne else 0)
    if add_edge and cur != loop:
        R.add_loop_edge(loop, cur)
        if G is not None: G.add_loop_edge(loop, cur)
    return wb, full, wg


# ---- hand-made cases ------------------------------------------------------------------------------------------------------------------------------------------------
def hand_cases():
    C = []
    # 1. GetCovisiblesByWeight as written.  3 shares 120 points with 2 and 100 with 1: its gated list [2, 1] has no entry below 100, upper_bound runs to the end and
    #    the result is EMPTY.  Then 4 connects to 3 with weight 3 (its single maximum): the AddConnection rebuilds 3's list from the whole row, [2, 1, 4], the same two
    #    weights and one weak entry: now [2, 1] comes back, 2 is the parent, and 1 is a covisibility edge.
    b = cc.Builder()
    for k in (1, 2, 3, 4, 8, 9): b.kf(k, n=256)
    b.pts(100, [3, 1]); b.pts(120, [3, 2])
    b.op('uc', [3]); b.x('ordered', 3, ([2, 1], [120, 100])); b.x('tree', 3, (2, False, []))
    b.op('eg', 9, 8, [9], {9: [8]}, [(9, 8, 0), (3, 2, 1)])
    b.pts(3, [3, 4])
    b.op('uc', [4]); b.x('ordered', 3, ([2, 1, 4], [120, 100, 3])); b.x('tree', 4, (3, False, []))
    b.op('eg', 9, 8, [9], {9: [8]}, [(9, 8, 0), (3, 2, 1), (3, 1, 3), (4, 3, 1)])
    C.append(b.case('covisibles-by-weight-quirk'))
    # 2. cur - loop is kept at weight 20; 10 - 2 at 99 is dropped, 11 - 3 at 100 is kept
    b = cc.Builder()
    for k in (1, 2, 3, 10, 11): b.kf(k, n=256)
    b.pts(20, [10, 1]); b.pts(99, [10, 2]); b.pts(100, [11, 3])
    b.op('uc', [10]); b.op('uc', [11]); b.x('weights', 10, ([1, 2], [20, 99])); b.x('tree', 10, (2, False, [])); b.x('tree', 11, (3, False, []))
    b.op('eg', 10, 1, [11, 10], {10: [1, 2], 11: [3]}, [(10, 1, 0), (11, 3, 0), (10, 2, 1), (11, 3, 1)])
    C.append(b.case('cur-loop-weak-99-100'))
    # 3. 10's list is [2 (120), 1 (100), 3 (20)] and its parent 2.  With 1, 2 and 3 as kept loop connections the tree edge 10 - 2 is emitted all the same, and the
    #    covisibility edge 10 - 1 is suppressed; with only the loop keyframe 3 connected it is there
    b = cc.Builder()
    for k in (1, 2, 3, 10): b.kf(k, n=256)
    b.pts(100, [10, 1]); b.pts(120, [10, 2]); b.pts(20, [10, 3])
    b.op('uc', [10]); b.x('ordered', 10, ([2, 1, 3], [120, 100, 20]))
    b.op('eg', 10, 3, [10], {10: [1, 2, 3]}, [(10, 1, 0), (10, 2, 0), (10, 3, 0), (10, 2, 1)])
    b.op('eg', 10, 3, [10], {10: [3]}, [(10, 3, 0), (10, 2, 1), (10, 1, 3)])
    C.append(b.case('tree-edge-and-inserted-pair'))
    # 4. the neighbours of 10 at 100 or more: its parent 2 (150), the larger id 12 (140), its child 5 (130), its loop edge 3 (110), the dead 4 (105), and 7 (101), the
    #    only one that stays; 6 (20) is the weak entry that lets upper_bound stop.  4 dies without 10 hearing of it: it drops the shared points (10 sees them in stereo
    #    and 20 sees them too, so they live on), updates its connections, which now hold 22 only, and is erased
    b = cc.Builder()
    b.kf(10, n=1024, uright=5.0)
    for k in (2, 3, 4, 5, 6, 7, 12, 20, 22): b.kf(k, n=256)
    b.pts(150, [10, 2]); b.pts(140, [10, 12]); b.pts(130, [10, 5]); b.pts(110, [10, 3]); P4 = b.pts(105, [10, 4, 20]); b.pts(101, [10, 7]); b.pts(20, [10, 6]); b.pts(15, [4, 22])
    b.op('uc', [10]); b.op('uc', [5]); b.x('tree', 5, (10, False, [])); b.x('tree', 10, (2, False, [5]))
    b.op('obs', 4, list(range(105)), [-1] * 105); b.op('uc', [4]); b.x('weights', 4, ([22], [15]))
    b.op('erasekf', 4); b.op('le', 10, 3, 0)
    b.x('ordered', 10, ([2, 12, 5, 3, 20, 4, 7, 6], [150, 140, 130, 110, 105, 105, 101, 20]))
    b.op('eg', 12, 6, [12], {}, [(5, 10, 1), (10, 2, 1), (10, 3, 2), (10, 7, 3)])
    C.append(b.case('covisibility-drop-reasons', max_points=1024, cap=1024))
    # 5. an asymmetric pair: 5 and 1 shared 100 points when 5 was updated (both rows say 100); 86 of them went bad and 1, updated since, holds 5 at 14, below the gate,
    #    so 5 was not told.  As a loop connection of 5 the pair is kept (5's row: 100), as one of 1 it is dropped (1's row: 14)
    b = cc.Builder()
    for k in (1, 2, 5, 6): b.kf(k, n=256)
    P = b.pts(86, [5, 1]); b.pts(14, [5, 1]); b.pts(30, [1, 2])
    b.op('uc', [5]); b.op('bad', P); b.op('uc', [1])
    b.x('weights', 5, ([1], [100])); b.x('weights', 1, ([2, 5], [30, 14])); b.x('tree', 5, (1, False, [])); b.x('tree', 1, (2, False, [5]))
    b.op('eg', 6, 2, [5, 6], {5: [1]}, [(5, 1, 0), (1, 2, 1), (5, 1, 1)])
    b.op('eg', 6, 2, [1, 6], {1: [5]}, [(1, 2, 1), (5, 1, 1)])
    C.append(b.case('asymmetric-rows-reading-side'))
    # 6. loop edges are emitted from the larger id only, in ascending id; the same edge again, either way round, changes nothing
    b = cc.Builder()
    for k in (1, 2, 3): b.kf(k, n=8)
    b.op('le', 3, 1, 0); b.op('le', 1, 3, 0); b.op('le', 3, 1, 0); b.op('le', 2, 3, 0); b.op('le', 1, 1, -1); b.op('le', 1, 99, -1)
    b.x('loop_edges', 3, [1, 2]); b.x('loop_edges', 1, [3]); b.x('loop_edges', 2, [3])
    b.op('eg', 3, 1, [3], {}, [(3, 1, 2), (3, 2, 2)])
    C.append(b.case('loop-edges-from-the-larger-id'))
    # 7. the previous list of a later member is the one an earlier member's update left.  9 holds 7 at 20 and 1 at 5, its gated list is [7].  With a 21st shared point,
    #    7's update writes 21 into 9's row and rebuilds 9's list from the whole row, [7, 1]: 1 is a previous neighbour and no loop connection.  In the twin cluster
    #    nothing changed between 107 and 109, 109's list is still [107], and 101 is a loop connection
    b = cc.Builder()
    for k in (1, 7, 9, 101, 107, 109): b.kf(k)
    b.pts(20, [9, 7]); b.pts(5, [9, 1]); b.pts(20, [109, 107]); b.pts(5, [109, 101])
    b.op('uc', [9, 109]); b.x('ordered', 9, ([7], [20])); b.x('ordered', 109, ([107], [20]))
    b.pts(1, [9, 7])
    b.op('conn', 9, [7, 9], dict(lc={})); b.x('ordered', 9, ([7], [21]))
    b.op('conn', 109, [107, 109], dict(lc={109: [101]}))
    C.append(b.case('previous-list-rebuilt-by-an-earlier-member'))
    # 8. 5's list is [9, 2]; the point s of 9 and 2 is corrected through 2, the smaller id, which stands later in the list
    b = cc.Builder()
    for k in (2, 5, 9): b.kf(k)
    b.pts(30, [5, 9]); b.pts(20, [5, 2]); s_ = b.pt([9, 2]); x_ = b.pt([9])
    b.op('begin', 5, dict(group_id=[9, 2, 5], group_vertex=[2, 0, 1], point_id=list(range(30, 50)) + [s_] + list(range(30)) + [x_], point_ref=[1] * 21 + [2] * 30 + [0]))
    b.x('ordered', 5, ([9, 2], [30, 20]))
    C.append(b.case('reference-is-the-smaller-id'))
    # 9a. a dead entry in the current keyframe's list: 6 was erased unknown to 5 (weight 3, never told), 7's update rebuilt 5's list to [7, 6], and 5's points all went
    #     bad, so its own update returns early and the list stays: the group is [7, 5]
    b = cc.Builder()
    for k in (5, 6, 7): b.kf(k)
    b.pts(3, [5, 6]); b.pts(16, [5, 7])
    b.op('uc', [5]); b.op('erasekf', 6); b.pts(1, [5, 7]); z_ = b.pt([7]); b.op('uc', [7]); b.x('ordered', 5, ([7, 6], [17, 3]))
    b.op('bad', list(range(3, 20)))
    b.op('begin', 5, dict(group_id=[7, 5], group_vertex=[1, 0], point_id=[z_], point_ref=[0]))
    b.x('ordered', 5, ([7, 6], [17, 3]))
    C.append(b.case('dead-entry-in-the-current-list'))
    # 9b. dead keys in a kept old row: 5's update finds no point and leaves the row {6: 3, 7: 16, 8: 2}; the list was [7], so 6 and 8 are new keys, and 6 is dead
    b = cc.Builder()
    for k in (5, 6, 7, 8): b.kf(k)
    b.pts(3, [5, 6]); b.pts(16, [5, 7]); b.pt([7]); b.pts(2, [5, 8])
    b.op('uc', [5]); b.op('erasekf', 6); b.op('bad', list(range(3, 19)) + [20, 21])
    b.x('weights', 5, ([6, 7, 8], [3, 16, 2])); b.x('ordered', 5, ([7], [16]))
    b.op('conn', 5, [7, 5], dict(lc={5: [8]}))
    C.append(b.case('dead-key-in-a-kept-row'))
    # 10. a keyframe with a loop edge is not erased, and nothing of it changes; the others are
    b = cc.Builder()
    for k in (1, 2, 3): b.kf(k)
    b.pts(15, [1, 2]); b.pts(15, [2, 3]); b.op('uc', [1, 2, 3]); b.op('le', 1, 2, 0)
    b.op('erase_refused', 1); b.op('erase_refused', 2); b.op('erasekf', 3); b.x('loop_edges', 1, [2])
    C.append(b.case('erase-refused-with-a-loop-edge'))
    return C


# ---- generated ------------------------------------------------------------------------------------------------------------------------------------------------------
def auto_fuse(R, cur, loop, k):
    """CorrectLoop's fusion as replace_point calls: k points of cur that loop does not hold, each replaced by a point of loop that cur does not hold"""
    pc = [p for p in R.keyframe_points(cur) if p >= 0]; pl = [p for p in R.keyframe_points(loop) if p >= 0]
    a = [p for p in pc if p not in set(pl)][:k]; b = [p for p in pl if p not in set(pc)][:k]
    return [('replace', int(o), int(n)) for o, n in zip(a, b)]


def walk_script(seed, nkf=26):
    """a walk of covis_cases (150 points a keyframe, so that neighbours share 100 and more) with keyframes erased on the way and loops closed between a new keyframe
    and an early one, 0, 20 or 120 points fused"""
    case = cc.walk_script(seed, nkf=nkf, npts=560, per_kf=150, cap=160, window=180, Q=3, mutate=False)
    rng = np.random.RandomState(100 + seed)
    ids = [o[1] for o in case['ops'] if o[0] == 'kf']
    rounds = {9: ids[1], 14: ids[3], 19: ids[2], nkf - 2: ids[5]}; erases = {t: ids[i] for t, i in ((11, 7), (16, 12), (21, 17)) if i < nkf - 3}
    ops = []; t = -1
    for o in case['ops']:
        ops.append(o)
        if o[0] == 'kf': t += 1
        if o[0] == 'uc' and len(o[1]) == 1 and o[1][0] == ids[t]:
            if t in erases: ops.append(('erasekf', erases[t]))
            if t in rounds: ops.append(('round', ids[t], rounds[t], ('auto', int(rng.choice([0, 20, 120])))))
            if t % 7 == 6: ops.append(('bad', [int(p) for p in rng.randint(0, 560, 40)]))
    ops.append(('round', ids[-1], ids[1], ('auto', 120)))                          # a second loop on keyframes that have loop edges
    return dict(name=f'loop-walk-{seed}', ops=ops, max_points=560, cap=160, max_keyframes=64)


def star_script(m, extra=0):
    """m keyframes 0 .. m - 1 that all see the same 15 points: every list holds every other keyframe, the group of the last one is the whole map, every keyframe but 0
    has a parent (m - 1 edges); `extra` keyframes that see nothing"""
    ops = []
    for k in range(m + extra):
        ops.append(('kf', k, np.zeros(16, 'i4'), np.full(16, -1, 'f4'), np.ones(16, 'f4')))
        if k < m: ops.append(('obs', k, list(range(15)), list(range(15))))
    ops.append(('round', m - 1, 0, ()))
    if m > 2: ops.append(('round', m - 2, 1, ()))
    return dict(name=f'star-{m}+{extra}', ops=ops, max_points=16, cap=16, max_keyframes=m + extra + 1, max_observations=16 * (m + 1))


def scenario_script():
    """the drop reasons of hand-made case 4 around keyframe 10, and a loop closed elsewhere in the map between 30 (with 31) and 7: the fused points are 7's, which 10 and
    50 see too, so that 30 and 31 get 7, 10 and 50 as loop connections; 50's list is rebuilt with its weak entry 22 and holds 31, 30 (inserted pairs), 10 (its parent)
    and 7 (an edge); 31 and 12 shared 100 points of which 95 went bad after 12 heard of it (12's row says 100, 31's says 5)"""
    b = cc.Builder()
    b.kf(10, n=1024, uright=5.0)
    for k in (2, 3, 4, 5, 6, 7, 12, 20, 22, 30, 31, 50): b.kf(k, n=512)
    b.pts(150, [10, 2]); b.pts(140, [10, 12]); b.pts(130, [10, 5]); b.pts(110, [10, 3]); b.pts(105, [10, 4, 20]); b.pts(101, [10, 7, 50]); b.pts(20, [10, 6]); b.pts(15, [4, 22])
    b.pts(3, [50, 22]); b.pts(120, [30, 31]); P = b.pts(95, [31, 12]); b.pts(5, [31, 12])
    b.op('uc', [10]); b.op('uc', [5]); b.op('uc', [50]); b.op('uc', [31]); b.op('bad', P)
    b.op('obs', 4, list(range(105)), [-1] * 105); b.op('uc', [4]); b.op('erasekf', 4); b.op('le', 10, 3, 0)
    b.op('round', 30, 7, ('auto', 101))
    b.op('round', 30, 7, ('auto', 0))
    return b.case('scenario', max_points=2048, cap=1024, max_keyframes=32)


def all_generated():
    return [walk_script(0), walk_script(1), scenario_script()] + [star_script(m) for m in (1, 2, 63, 64, 65, 256, 258)] + [star_script(257, 43)]


REQUIRED = ('kind0', 'kind1', 'kind2', 'kind3', 'drop_parent', 'drop_child', 'drop_loop_edge', 'drop_larger_id', 'drop_dead', 'quirk_fired', 'quirk_not_fired', 'lc_row',
            'asymmetric', 'nomem_points', 'nomem_lc', 'nomem_edges')


# ---- the runner -----------------------------------------------------------------------------------------------------------------------------------------------------
def run_script(lib, case, stream=None, ev=lr.EVENTS, state=True):
    """lib = None: the restatement alone, which counts its events in ev for the same inputs"""
    G = cc.make_graph(lib, case) if lib is not None else None
    R = lr.Map(case.get('monocular', False), cc.TH_DEPTH, case.get('max_points', 2048), case.get('max_keyframes', 128))
    points = set(); nround = 0
    def compare():
        if G is None or not state: return
        cc.compare_state(G, R, points)
        assert G.loop_info()[1] == R.n_loop_edges()
        for k in R.kfs:
            if lr.loop_set(R.kfs[k]): assert G.loop_edges(k) == R.loop_edges(k), k
    for op in case['ops']:
        k = op[0]; name = (case['name'], k) + tuple(op[1:3])
        if k == 'x':
            want = getattr(R, op[1])(*op[2])
            assert want == op[3], (case['name'], op[1], op[2], want, op[3])
            if G is not None:
                got = getattr(G, op[1])(*op[2])
                assert (list(got) if op[1] == 'keyframe_points' else got) == op[3], (case['name'], 'device', op[1], op[2], got, op[3])
        elif k == 'le':
            want = status_of(R.add_loop_edge, op[1], op[2])
            if len(op) > 3: assert want == op[3], (name, want)
            if G is not None: assert status_of(G.add_loop_edge, op[1], op[2]) == want, name
            compare()
        elif k == 'erase_refused':
            assert status_of(R.erase_keyframe, op[1]) == -1
            if G is not None: assert status_of(G.erase_keyframe, op[1]) == -1
            compare()
        elif k == 'begin':
            w = begin(G, R, op[1], None, stream, name, ev)
            for key, v in (op[2] if len(op) > 2 else {}).items(): assert w[key] == v, (name, key, w[key], v)
            compare()
        elif k == 'conn':
            LCw = connections(G, R, op[1], op[2], None, stream, name, ev)
            if len(op) > 3 and 'lc' in op[3]:
                rows = {i: LCw['full'][LCw['lc_begin'][r]:LCw['lc_begin'][r + 1]] for r, i in enumerate(sorted(op[2]))}
                assert {i: v for i, v in rows.items() if v} == op[3]['lc'], (name, rows)
            compare()
        elif k == 'eg':
            lb, lj = csr_of(R, op[3], op[4])
            w = graph(G, R, op[1], op[2], op[3], lb, lj, None, stream, name, ev)
            if len(op) > 5: assert w['edges_by_id'] == op[5], (name, w['edges_by_id'], op[5])
            ne = w['report']['n_edges']
            for ecap in (ne, ne - 1, 0):
                if ecap >= 0: graph(G, R, op[1], op[2], op[3], lb, lj, ecap, stream, name + (ecap,), ev)
        elif k == 'round':
            fuse = auto_fuse(R, op[1], op[2], op[3][1]) if op[3] and op[3][0] == 'auto' else list(op[3])
            loop_round(G, R, op[1], op[2], fuse, nround % 3, stream, name, ev, points, op[4] if len(op) > 4 else None)
            nround += 1
            compare()
        elif k in ('lm', 'cull', 'cullloop'): continue
        else:
            cc.apply_ref(R, op)
            if k == 'obs': points.update(p for p in op[3] if p >= 0)
            if G is not None:
                if k == 'kf': G.add_keyframe(op[1], op[2], op[3], op[4])
                elif k == 'obs': G.set_observations(op[1], op[2], op[3])
                elif k == 'bad': G.set_points_bad(op[1])
                elif k == 'replace': G.replace_point(op[1], op[2])
                elif k == 'erasekf': G.erase_keyframe(op[1])
                elif k == 'uc': G.update_connections(op[1], stream)
    compare()
    if G is not None: G.close()
    return R


# ---- checks shared by the CPU and the GPU tier ------------------------------------------------------------------------------------------------------------------------
def check_two_runs_identical(lib, stream=None):
    """the essential graph of one state twice: byte-identical; and against a second handle that was built the same way"""
    case = walk_script(0, nkf=16)
    out = []
    for _ in range(2):
        G = cc.make_graph(lib, case); R = lr.Map(False, cc.TH_DEPTH, 560, 64)
        for o in case['ops']:
            if o[0] in ('kf', 'obs', 'uc', 'erasekf', 'bad'):
                cc.apply_ref(R, o)
                if o[0] == 'kf': G.add_keyframe(*o[1:])
                elif o[0] == 'obs': G.set_observations(*o[1:])
                elif o[0] == 'uc': G.update_connections(o[1], stream)
                elif o[0] == 'erasekf': G.erase_keyframe(o[1])
                else: G.set_points_bad(o[1])
        ids = sorted(R.kfs); cur, loop = ids[-1], ids[1]
        b1 = G.loop_begin(cur, stream=stream)
        for op in auto_fuse(R, cur, loop, 120): G.replace_point(op[1], op[2]); cc.apply_ref(R, op)
        c1 = G.loop_connections(cur, b1['group_id'], stream=stream)
        g1 = G.essential_graph(cur, loop, b1['group_id'], c1['lc_begin'], c1['lc_j'], stream=stream)
        g2 = G.essential_graph(cur, loop, b1['group_id'], c1['lc_begin'], c1['lc_j'], stream=stream)
        for key in ('vertex_id', 'vertex_fixed', 'vertex_group', 'e_i', 'e_j', 'e_kind', 'report'): assert g1[key].tobytes() == g2[key].tobytes(), key
        assert int(g1['report']['n_kind'][0]) > 0 and int(g1['report']['n_kind'][1]) > 0, g1['report']
        out.append((b1, c1, g1)); G.close()
    for a, b in zip(out[0], out[1]):
        for key in a:
            if isinstance(a[key], np.ndarray): assert a[key].tobytes() == b[key].tobytes(), key


def check_errors(lib):
    """every error status, with the untouched remainder of every row"""
    import ctypes as C
    from sg_slam_amd.capi import _vp, COVIS_LOOP_REPORT_DTYPE
    from sg_slam_amd.covisibility import CovisibilityGraph
    G = CovisibilityGraph(max_keyframes=4, cap=32, max_points=64, max_observations=256, max_queries=2, lib=lib)
    z = np.zeros(32, 'i4'); m1 = np.full(32, -1, 'f4'); o1 = np.ones(32, 'f4')
    assert G.loop_info() == (0, 0)                                                 # nothing allocated before the first loop call
    info = G.info()
    for k in (1, 2, 3, 4): G.add_keyframe(k, z, m1, o1)
    G.set_observations(1, range(30), range(30)); G.set_observations(2, range(16), range(16)); G.set_observations(3, range(14), range(16, 30))
    # add_loop_edge: unknown, erased, equal ids; the capacity of max_keyframes pairs
    assert status_of(G.add_loop_edge, 1, 1) == -1 and status_of(G.add_loop_edge, 1, 9) == -1 and status_of(G.add_loop_edge, 9, 1) == -1 and status_of(G.loop_edges, 9) == -1
    for a, b in ((1, 2), (1, 3), (1, 4), (2, 3)): assert status_of(G.add_loop_edge, a, b) == 0
    assert G.loop_info() == (4 * 4 * (4 + 29) + 32, 4) and G.info()[:2] == info[:2]   # create's figures do not change
    assert status_of(G.add_loop_edge, 2, 4) == -3 and G.loop_info()[1] == 4 and G.loop_edges(2) == [1, 3] and G.loop_edges(4) == [1]      # full: unchanged
    assert status_of(G.add_loop_edge, 3, 2) == 0 and G.loop_info()[1] == 4          # an edge that is there is no new pair
    assert status_of(G.erase_keyframe, 4) == -1 and G.size() == 4                   # rule 10
    G.clear()
    assert G.loop_info()[1] == 0 and G.size() == 0                                  # clear drops the edges
    for k in (1, 2, 3, 4): G.add_keyframe(k, z, m1, o1)
    G.set_observations(1, range(30), range(30)); G.set_observations(2, range(16), range(16)); G.set_observations(3, range(14), range(16, 30))
    assert status_of(G.erase_keyframe, 4) == 0 and status_of(G.add_loop_edge, 1, 4) == -1 and G.loop_edges(1) == []
    dll = lib.dll; N = G.max_keyframes
    rep = lambda: G._dev(np.zeros(COVIS_LOOP_REPORT_DTYPE.itemsize, 'u1'))
    row = lambda n, v=-7: G._dev(np.full(max(n, 1), v, 'i4'))
    # loop_begin: calls refused as a whole
    a = [row(N), row(N), row(4), row(4), rep()]
    def lb(cur, pcap, drop=()):
        p = [None if i in drop else _vp(x) for i, x in enumerate(a)]
        return dll.sgx_covis_loop_begin_dev(G.h, cur, p[0], p[1], pcap, p[2], p[3], p[4], G._stream(None))
    assert lb(9, 4) == -1 and lb(4, 4) == -1 and lb(1, -1) == -1 and dll.sgx_covis_loop_begin_dev(None, 1, *([None] * 2), 0, *([None] * 4)) == -1
    for d in range(5): assert lb(1, 4, (d,)) == -1
    G._sync(None)
    for x in a[:4]: assert (G._host(x) == -7).all()
    assert G.ordered(1) == ([], [])                                                # and nothing ran
    # short of room: the first 4 points, no row overrun; pcap 0 needs no point rows
    assert lb(1, 4) == 0; G._sync(None)
    r = G._host(a[4]).view(COVIS_LOOP_REPORT_DTYPE)[0]
    assert (int(r['status']), int(r['n_group']), int(r['n_points'])) == (-3, 2, 30) and list(G._host(a[0])) == [2, 1, -7, -7] and list(G._host(a[1])) == [1, 0, -7, -7]
    assert list(G._host(a[2])) == [0, 1, 2, 3] and list(G._host(a[3])) == [1, 1, 1, 1]
    assert lb(1, 0, (2, 3)) == 0
    # loop_connections: the call refused; the group row refused in the report with nothing written and the handle unchanged
    c = [row(2), row(3), row(4), rep()]
    def lc(cur, group, lcap, drop=(), n=None):
        c[0] = G._dev(np.asarray(group, 'i4')); p = [None if i in drop else _vp(x) for i, x in enumerate(c)]
        rc = dll.sgx_covis_loop_connections_dev(G.h, cur, len(group) if n is None else n, p[0], lcap, p[1], p[2], p[3], G._stream(None)); G._sync(None)
        return rc, int(G._host(c[3]).view(COVIS_LOOP_REPORT_DTYPE)[0]['status'])
    assert lc(9, [2, 1], 4)[0] == -1 and lc(1, [2, 1], -1)[0] == -1 and lc(1, [2, 1], 4, n=0)[0] == -1 and lc(1, [2, 1, 3, 3], 4, n=4)[0] == -1
    for d in (0, 1, 2, 3): assert lc(1, [2, 1], 4, (d,))[0] == -1
    before = [G.weights(k) for k in (1, 2, 3)] + [G.ordered(k) for k in (1, 2, 3)]
    for bad in ([1, 2], [2, 2, 1], [9, 1], [4, 1]): assert lc(1, bad, 4) == (0, -1), bad
    assert (G._host(c[1]) == -7).all() and (G._host(c[2]) == -7).all() and before == [G.weights(k) for k in (1, 2, 3)] + [G.ordered(k) for k in (1, 2, 3)]
    assert lc(1, [2, 1], 0, (2,)) == (0, -3) and list(G._host(c[1])) == [0, 1, 1]   # 1's gated list is [2]: 3 (14) is a new key; lc_begin is whole, no row fits
    # essential_graph: the call refused; group row and CSR refused in the report
    e = [None, None, None, row(N), G._dev(np.full(N, 7, 'u1')), row(N), row(3), row(3), G._dev(np.full(3, 7, 'u1')), rep()]
    def eg(cur, loop, group, begin, lj, ecap, drop=(), lcap=None):
        e[0] = G._dev(np.asarray(group, 'i4')); e[1] = G._dev(np.asarray(begin, 'i4')); e[2] = G._dev(np.asarray(lj if len(lj) else [0], 'i4'))
        p = [None if i in drop else _vp(x) for i, x in enumerate(e)]
        rc = dll.sgx_covis_essential_graph_dev(G.h, cur, loop, len(group), p[0], len(lj) if lcap is None else lcap, p[1], p[2], p[3], p[4], p[5], ecap, p[6], p[7], p[8], p[9],
                                               G._stream(None)); G._sync(None)
        return rc, int(G._host(e[9]).view(COVIS_LOOP_REPORT_DTYPE)[0]['status'])
    ok = (1, 3, [2, 1], [0, 1, 1], [3])
    assert eg(9, 3, *ok[2:], 3)[0] == -1 and eg(1, 4, *ok[2:], 3)[0] == -1 and eg(*ok, -1)[0] == -1 and eg(*ok, 3, lcap=-1)[0] == -1
    for d in (0, 1, 2, 3, 4, 5, 6, 7, 8, 9): assert eg(*ok, 3, (d,))[0] == -1, d
    for group, begin, lj in (([1, 2], [0, 1, 1], [3]), ([2, 2, 1], [0, 0, 1, 1], [3]), ([2, 1], [1, 1, 1], [3]), ([2, 1], [0, 1, 0], [3]), ([2, 1], [0, 1, 2], [3]),
                             ([2, 1], [0, 1, 1], [9]), ([2, 1], [0, 1, 1], [4]), ([2, 1], [0, 2, 2], [3, 3]), ([2, 1], [0, 2, 2], [3, 2])):
        assert eg(1, 3, group, begin, lj, 3) == (0, -1), (group, begin, lj)
    for x in e[3:9]: assert (G._host(x) == 7).all() if G._host(x).dtype == np.uint8 else (G._host(x) == -7).all()
    # short of room: the first ecap edges and nothing behind them
    assert eg(*ok, 1) == (0, -3)
    r = G._host(e[9]).view(COVIS_LOOP_REPORT_DTYPE)[0]
    assert int(r['n_vertices']) == 3 and int(r['n_edges']) > 1 and list(G._host(e[6])[1:]) == [-7, -7] and list(G._host(e[8])[1:]) == [7, 7] and G._host(e[3])[3] == -7
    assert eg(*ok, 0, (6, 7, 8)) == (0, -3)
    # the host-pointer entries return the status
    gid = np.zeros(N, 'i4'); gv = np.zeros(N, 'i4'); rp = np.zeros(1, COVIS_LOOP_REPORT_DTYPE)
    assert dll.sgx_covis_loop_begin(G.h, 1, _vp(gid), _vp(gv), 0, None, None, _vp(rp)) == -3 and int(rp[0]['n_points']) == 30 and list(gid[:2]) == [2, 1]
    assert dll.sgx_covis_loop_begin(G.h, 9, _vp(gid), _vp(gv), 0, None, None, _vp(rp)) == -1 and dll.sgx_covis_loop_begin(G.h, 1, None, _vp(gv), 0, None, None, None) == -1
    beg = np.full(3, -7, 'i4'); g2 = np.array([2, 1], 'i4'); gbad = np.array([1, 2], 'i4')
    assert dll.sgx_covis_loop_connections(G.h, 1, 2, _vp(gbad), 0, _vp(beg), None, _vp(rp)) == -1 and (beg == -7).all()
    lj1 = np.full(1, -7, 'i4')
    assert dll.sgx_covis_loop_connections(G.h, 1, 2, _vp(g2), 1, _vp(beg), _vp(lj1), _vp(rp)) == 0 and list(beg) == [0, 1, 1] and lj1[0] == 3
    vi = np.zeros(N, 'i4'); vf = np.zeros(N, 'u1'); vg = np.zeros(N, 'i4')
    assert dll.sgx_covis_essential_graph(G.h, 1, 3, 2, _vp(g2), _vp(beg), _vp(lj1), _vp(vi), _vp(vf), _vp(vg), 0, None, None, None, _vp(rp)) == -3 and list(vi[:3]) == [1, 2, 3]
    assert list(vf[:3]) == [0, 0, 1] and list(vg[:3]) == [1, 0, -1]
    assert dll.sgx_covis_essential_graph(G.h, 1, 3, 2, _vp(gbad), _vp(beg), _vp(lj1), _vp(vi), _vp(vf), _vp(vg), 0, None, None, None, _vp(rp)) == -1
    G.close()


# ---- the Sim3 glue: every output against the scalar restatement, bit for bit ------------------------------------------------------------------------------------------
def bits(a, b, what):
    a = np.ascontiguousarray(a); b = np.ascontiguousarray(b).astype(a.dtype).reshape(a.shape)
    assert a.tobytes() == b.tobytes(), (what, np.argwhere(a != b)[:3].tolist(), a.reshape(-1)[:4], b.reshape(-1)[:4])


def random_pose(rng, angle=None, axis=None):
    """a float32 pose; angle / axis: rotations with a negative trace, which take Eigen's three other branches of the matrix-to-quaternion conversion"""
    import sim3_cases as sc
    w = rng.normal(0, 1.0, 3) if angle is None else angle * np.eye(3)[axis] + rng.normal(0, 0.05, 3)
    q = sc.quat_from_rotvec(w)
    R = np.array(lr.quat_to_R([float(x) for x in q / np.linalg.norm(q)]))
    return np.concatenate([R, rng.uniform(-3, 3, (3, 1))], 1).astype('f4')


def sim3_problem(seed, ng, nv, ne):
    rng = np.random.RandomState(seed)
    poses = [random_pose(rng) for _ in range(nv)]
    for k, ax in enumerate((0, 1, 2)):
        if k < nv: poses[k] = random_pose(rng, 3.0, ax)
    group = [int(x) for x in rng.permutation(nv)[:ng]]                           # vertex of every group member, cur last
    vg = np.full(nv, -1, 'i4'); vg[group] = np.arange(ng)
    Scw = np.r_[lr.sim3_of_pose(random_pose(rng))[:7], rng.uniform(0.8, 1.25)]
    e_i = rng.randint(0, nv, ne).astype('i4'); e_j = ((e_i + 1 + rng.randint(0, max(nv - 1, 1), ne)) % nv).astype('i4') if nv > 1 else e_i.copy()
    e_k = rng.randint(0, 4, ne).astype('u1')
    return dict(poses=np.array(poses, 'f4'), group=group, vertex_group=vg, Scw=Scw, e_i=e_i, e_j=e_j, e_kind=e_k,
                xw=rng.uniform(-4, 4, (57, 3)).astype('f4'), ref=rng.randint(0, ng, 57).astype('i4'))


def check_sim3_glue(lib):
    import ctypes as C
    from sg_slam_amd.capi import _vp
    from sg_slam_amd.optimizer import Optimizer
    on_host = 'EMULATOR' in lib.version()
    if not on_host: import torch
    dev = (lambda a: np.ascontiguousarray(a).copy()) if on_host else (lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda())
    host = (lambda x: x) if on_host else (lambda x: x.cpu().numpy())
    stream = None if on_host else C.c_void_p(torch.cuda.current_stream().cuda_stream)
    for seed, (ng, nv, ne) in enumerate(((1, 1, 0), (2, 3, 5), (5, 9, 40), (65, 300, 257), (257, 257, 600))):
        P = sim3_problem(seed, ng, nv, ne)
        Tg = P['poses'][P['group']]
        non, cor, cT = Optimizer.PropagateLoopSim3(Tg, P['Scw'], lib=lib)
        rn, rc, rT = lr.propagate_sim3(Tg, P['Scw'])
        bits(non, rn, ('noncorrected', seed)); bits(cor, rc, ('corrected', seed)); bits(cT, rT, ('corrected_Tiw', seed))
        g = dict(vertex_group=P['vertex_group'], e_i=P['e_i'], e_j=P['e_j'], e_kind=P['e_kind'])
        S_in, meas = Optimizer.FlattenEssentialGraph(g, P['poses'], cor, non, lib=lib)
        rS, rm = lr.flatten_sim3(P['vertex_group'], P['poses'], rc, rn, P['e_i'], P['e_j'], P['e_kind'])
        bits(S_in, rS, ('S_in', seed)); bits(meas, rm, ('e_meas', seed))
        S_out = np.array([lr.sim3_mul(list(s), list(P['Scw'])) for s in S_in])      # any Sim3 with a scale that is not 1
        T, inv = Optimizer.RecoverEssentialGraph(S_out, lib=lib)
        rTT, rinv = lr.recover_sim3(S_out)
        bits(T, rTT, ('Tcw', seed)); bits(inv, rinv, ('corrected_Swc', seed))
        cSwi = Optimizer.RecoverEssentialGraph(cor, lib=lib)[1]
        out = lr.correct_points(P['xw'], P['ref'], rn, lr.recover_sim3(rc)[1])          # sgx_correct_map_points_dev below has to give these bits
        # the device-pointer forms give the same bytes
        d = dict(T=dev(Tg), S=dev(P['Scw']), non=dev(np.zeros((ng, 8))), cor=dev(np.zeros((ng, 8))), cT=dev(np.zeros((ng, 3, 4), 'f4')), vg=dev(P['vertex_group']), Tv=dev(P['poses']),
                 ei=dev(P['e_i']), ej=dev(P['e_j']), ek=dev(P['e_kind']), Sin=dev(np.zeros((nv, 8))), m=dev(np.zeros((max(ne, 1), 8))), So=dev(S_out), To=dev(np.zeros((nv, 3, 4), 'f4')),
                 inv=dev(np.zeros((nv, 8))), xw=dev(P['xw']), ref=dev(P['ref']), out=dev(np.zeros((57, 3), 'f4')), cSwi=dev(cSwi))
        p = {k: _vp(v) for k, v in d.items()}
        assert lib.dll.sgx_loop_propagate_sim3_dev(ng, p['T'], p['S'], p['non'], p['cor'], p['cT'], stream) == 0
        assert lib.dll.sgx_eg_flatten_dev(nv, p['vg'], p['Tv'], ng, p['cor'], p['non'], ne, p['ei'], p['ej'], p['ek'], p['Sin'], p['m'], stream) == 0
        assert lib.dll.sgx_eg_recover_dev(nv, p['So'], p['To'], p['inv'], stream) == 0
        assert lib.dll.sgx_correct_map_points_dev(57, p['xw'], p['ref'], p['non'], p['cSwi'], p['out'], stream) == 0
        if not on_host: torch.cuda.synchronize()
        bits(host(d['non']), non, 'dev non'); bits(host(d['cor']), cor, 'dev cor'); bits(host(d['cT']), cT, 'dev cT'); bits(host(d['Sin']), S_in, 'dev S_in')
        bits(host(d['m'])[:ne], meas, 'dev meas'); bits(host(d['To']), T, 'dev T'); bits(host(d['inv']), inv, 'dev inv'); bits(host(d['out']), out, 'dev points')
    # refused calls
    dll = lib.dll; z = np.zeros(64); zf = np.zeros(64, 'f4'); zi = np.zeros(8, 'i4'); zb = np.zeros(8, 'u1')
    assert dll.sgx_loop_propagate_sim3(0, _vp(zf), _vp(z), _vp(z), _vp(z), _vp(zf)) == -1 and dll.sgx_loop_propagate_sim3(1, None, _vp(z), _vp(z), _vp(z), _vp(zf)) == -1
    assert dll.sgx_loop_propagate_sim3_dev(1, _vp(zf), None, _vp(z), _vp(z), _vp(zf), None) == -1
    bad = np.array([0, 2, -1], 'i4'); ok = np.array([0, 1, -1], 'i4')
    assert dll.sgx_eg_flatten(3, _vp(bad), _vp(zf), 2, _vp(z), _vp(z), 0, None, None, None, _vp(z), None) == -1            # a group index beyond the group
    assert dll.sgx_eg_flatten(3, _vp(ok), _vp(zf), 2, _vp(z), _vp(z), 1, _vp(np.array([3], 'i4')), _vp(zi), _vp(zb), _vp(z), _vp(z)) == -1      # an edge end beyond the vertices
    assert dll.sgx_eg_flatten(3, _vp(ok), _vp(zf), 2, _vp(z), _vp(z), 1, _vp(zi), _vp(zi), _vp(np.array([4], 'u1')), _vp(z), _vp(z)) == -1      # no such kind
    assert dll.sgx_eg_flatten(-1, None, None, 0, None, None, 0, None, None, None, None, None) == -1 and dll.sgx_eg_flatten(0, None, None, 0, None, None, 0, None, None, None, None, None) == 0
    assert dll.sgx_eg_recover(-1, None, None, None) == -1 and dll.sgx_eg_recover(1, _vp(z), None, _vp(z)) == -1 and dll.sgx_eg_recover(0, None, None, None) == 0
    assert dll.sgx_correct_map_points_dev(-1, None, None, None, None, None, None) == -1 and dll.sgx_correct_map_points_dev(1, _vp(zf), None, _vp(z), _vp(z), _vp(zf), None) == -1


def check_chain(lib, orc, stream=None):
    """correct_loop on a ring of 40 keyframes with drift (the generator idea of sim3_cases.make_graph, the graph from the handle): keyframe t sees the points
    [20 t, 20 t + 150), so neighbours share 130, 110, 90, ... points; keyframe 39 has come round to keyframe 0 and 120 of its points are duplicates of keyframe 0's, which the
    fusion replaces.  Every row and every Sim3 equals the restatement's, bit for bit; the optimised poses agree with the oracle's optimiser fed the same arrays under the
    criteria of sim3_cases.check_eg."""
    import sim3_cases as sc
    from sg_slam_amd.covisibility import CovisibilityGraph
    nkf, step, per = 40, 20, 150; npts = step * (nkf - 1) + per
    g0 = sc.make_graph(7, nkf, noise=0.01)
    pose = lambda S: np.concatenate([np.array(lr.quat_to_R([float(x) for x in S[:4]])), np.reshape(S[4:7], (3, 1))], 1).astype('f4')
    Tcw = {t: pose(g0['S0'][t]) for t in range(nkf)}                              # the drifted poses; keyframe 0 carries no drift
    Scw = np.r_[lr.sim3_of_pose(pose(g0['truth'][nkf - 1]))[:7], 1.0]             # what ComputeSim3 found for the current keyframe: where it really is
    rng = np.random.RandomState(11); xw = rng.uniform(-3, 3, (npts, 3)).astype('f4')
    G = CovisibilityGraph(max_keyframes=48, cap=160, max_points=npts, max_observations=nkf * per, max_queries=8, lib=lib)
    R = lr.Map(False, cc.TH_DEPTH, npts, 48)
    for t in range(nkf):
        for m in (G, R): m.add_keyframe(t, np.zeros(per, 'i4'), np.full(per, -1, 'f4'), np.ones(per, 'f4')); m.set_observations(t, list(range(per)), list(range(step * t, step * t + per)))
    for at in range(0, nkf, 8): G.update_connections(list(range(at, at + 8)), stream)
    for t in range(nkf): R.update_connections(t)
    cur, loop = nkf - 1, 0
    fuse_ops = [('replace', step * cur + 20 + i, i) for i in range(120)]
    # the restatement's loop
    wb = lr.flatten_begin(R, lr.loop_begin(R, cur))
    rn, rc, rT = lr.propagate_sim3([Tcw[k] for k in wb['group_id']], Scw)
    x1 = xw.copy(); x1[wb['point_id']] = lr.correct_points(xw[wb['point_id']], wb['point_ref'], rn, lr.recover_sim3(rc)[1])
    for op in fuse_ops: cc.apply_ref(R, op)
    wc = lr.flatten_connections(lr.loop_connections(R, cur, wb['group_id']))
    wg = lr.flatten_graph(lr.essential_graph(R, cur, loop, wb['group_id'], wc['lc_begin'], wc['lc_j']))
    rS, rm = lr.flatten_sim3(wg['vertex_group'], [Tcw[k] for k in wg['vertex_id']], rc, rn, wg['e_i'], wg['e_j'], wg['e_kind'])
    assert wg['report']['n_kind'][0] >= 1 and wg['report']['n_kind'][3] > 10 and len(wb['group_id']) > 3
    # the device's
    def fuse(graph, begin_rows, corrected):
        for op in fuse_ops: graph.replace_point(op[1], op[2])
    res = G.correct_loop(cur, loop, Scw, Tcw, xw, fuse=fuse, fix_scale=True, stream=stream)
    same(res['begin'], wb, ('group_id', 'group_vertex', 'point_id', 'point_ref'), 'chain begin'); same(res['connections'], wc, ('lc_begin', 'lc_j'), 'chain connections')
    same(res['graph'], wg, ('vertex_id', 'vertex_fixed', 'vertex_group', 'e_i', 'e_j', 'e_kind'), 'chain graph')
    bits(res['noncorrected'], rn, 'chain noncorrected'); bits(res['corrected'], rc, 'chain corrected'); bits(res['corrected_Tiw'], rT, 'chain corrected poses')
    bits(res['S_in'], rS, 'chain S_in'); bits(res['e_meas'], rm, 'chain e_meas')      # the flattened problem
    eS, est = orc.optimize_essential_graph(rS, np.array(wg['vertex_fixed'], 'u1'), np.array(wg['e_i'], 'i4'), np.array(wg['e_j'], 'i4'), rm, True, 20)
    gst = res['stats']
    if est[2] > 1e-12 * est[1]: assert abs(gst[0] - est[0]) <= 1, (gst, est)
    else: assert gst[2] <= 1e-9 * gst[1], (gst, est)
    assert abs(gst[1] - est[1]) <= 1e-9 * est[1] and est[1] > 0
    for v in range(len(eS)): assert sc.sim3_close(res['S_out'][v], eS[v], 1e-5), (v, res['S_out'][v], eS[v])
    # recovery and the second point correction from the device's own optimum, bit for bit
    T2, inv2 = lr.recover_sim3(res['S_out'])
    bits(np.array([res['Tcw'][k] for k in wg['vertex_id']]), T2, 'chain poses'); bits(res['corrected_Swc'], inv2, 'chain corrected_Swc')
    x2 = x1.copy(); ids = wb['point_id']; x2[ids] = lr.correct_points(x1[ids], [wb['group_vertex'][r] for r in wb['point_ref']], rS, inv2)
    bits(res['xw'], x2, 'chain points')
    assert G.loop_edges(cur) == [loop] and np.abs(res['xw'] - xw).max() > 1e-3
    cc.compare_state(G, R, set(range(npts)))
    G.close()
