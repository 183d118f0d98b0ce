"""Shared cases for DetectLoop's consistency groups on the covisibility handle (sgx_covis_consistency, sgx_covis_get_consistent_groups, sgx_covis_connected_batch): a
World plays every step on the device (or the emulator) and on the restatement of tests/loopclose_ref.py over tests/loop_ref.py's Map and compares them after every call:
status, enough-list, report and the stored groups, integer for integer.  With lib = None only the restatement runs (the event coverage is asserted of it alone).
Below them: the trees of the map update after global BA (sgx_covis_gba_update, sgx_gba_correct_points_dev), compared bit for bit, and the driver on a ring of 40."""
import numpy as np
import loop_ref as lr
import loopclose_ref as ref
from sg_slam_amd.covisibility import CovisibilityGraph

REPORT = ('status', 'n_before', 'n_after', 'n_consistent', 'n_pushed_zero', 'n_pushed_nothing', 'n_enough', 'n_cand')
REQUIRED = ('pushed_twice', 'pushed_nothing', 'enough_but_marked', 'cleared', 'stale_slot', 'pushed_zero', 'dead_in_row', 'weak_member')
POISON = -7


class World:
    def __init__(self, lib, max_keyframes=64, cap=64, max_points=4096, max_groups=None, ev=ref.EVENTS):
        self.R = lr.Map(max_keyframes=max_keyframes)
        self.D = ref.Detector(self.R, 64 if max_groups is None else max_groups)
        self.G = CovisibilityGraph(max_keyframes=max_keyframes, cap=cap, max_points=max_points, max_observations=8 * max_points, max_queries=8, lib=lib) if lib is not None else None
        if self.G is not None and max_groups is not None: self.G.consistency_reserve(max_groups)
        self.cap = cap; self.free = {}; self.pid = 0; self.ev = ev

    def close(self):
        if self.G is not None: self.G.close()

    def kf(self, *ids):
        for i in ids:
            a = (np.zeros(self.cap, 'i4'), np.full(self.cap, -1, 'f4'), np.ones(self.cap, 'f4'))
            self.R.add_keyframe(i, *a)
            if self.G is not None: self.G.add_keyframe(i, *a)
            self.free[i] = 0

    def link(self, a, b, w):
        """w new points seen by a and b"""
        pts = list(range(self.pid, self.pid + w)); self.pid += w
        for k in (a, b):
            idx = list(range(self.free[k], self.free[k] + w)); self.free[k] += w
            self.R.set_observations(k, idx, pts)
            if self.G is not None: self.G.set_observations(k, idx, pts)

    def uc(self, *ids):
        for i in ids: self.R.update_connections(i)
        if self.G is not None and ids: self.G.update_connections(list(ids))

    def erase(self, i):
        self.R.erase_keyframe(i)
        if self.G is not None: self.G.erase_keyframe(i)

    def clear_groups(self):
        self.D.clear()
        if self.G is not None: self.G.consistency_clear()

    def consistency(self, cands, th=3, expect=None, what=''):
        """expect (optional): dict(status=, enough=, groups=[(ids, counter)]) as written by hand, asserted of the restatement"""
        before = self.D.groups()
        want = self.D.consistency(list(cands), th, self.ev)
        if expect is not None:
            for k in ('status', 'enough'):
                if k in expect: assert want[k] == expect[k], (what, k, want[k], expect[k])
            if 'groups' in expect: assert self.D.groups() == [(sorted(s), n) for s, n in expect['groups']], (what, self.D.groups(), expect['groups'])
        if want['status'] != 0: assert self.D.groups() == before, what
        if self.G is None: return want
        got = self.G.consistency(cands, th)
        assert got['status'] == want['status'], (what, got['status'], want['status'])
        for k in REPORT:
            if k in want['report']: assert int(got['report'][k]) == want['report'][k], (what, k, int(got['report'][k]), want['report'][k])
        en, nen = got['raw']
        if want['status'] != 0:
            assert (en == POISON).all() and (nen == POISON).all(), (what, 'a refused call wrote its outputs')
        else:
            assert got['enough'] == want['enough'], (what, got['enough'], want['enough'])
            assert (en[len(want['enough']):] == POISON).all(), what
        assert self.G.consistent_groups() == self.D.groups(), (what, self.G.consistent_groups(), self.D.groups())
        assert self.G.consistency_info()[1] == len(self.D.groups()), what
        return want

    def connected(self, ids, cap=None, what=''):
        want = ref.connected_batch(self.R, ids, 1 << 30 if cap is None else cap)
        if self.G is None: return want
        got = self.G.connected_batch(ids, cap)
        assert got['status'] == want['status'] and got['n'] == want['n'] and [int(x) for x in got['off']] == want['off'], (what, got, want)
        written = np.zeros(len(got['raw']), bool)
        for q, row in enumerate(want['rows']):
            if row is None: assert got['rows'][q] is None, (what, q); continue
            assert [int(x) for x in got['rows'][q]] == row, (what, q, got['rows'][q], row)
            written[want['off'][q]:want['off'][q + 1]] = True
        assert (got['raw'][~written] == -1).all(), (what, 'written outside the rows that fit')
        return want


# ---- hand-made cases: one per semantic item, each with its written answer ---------------------------------------------------------------------------------------------
def case_row_not_list(lib, ev):
    """1 shares 20 points with 2 and ONE with 3: 3 is in 1's weight row and not in its gated list; 3's own row is empty.  The stored group {3} makes candidate 1 consistent."""
    W = World(lib, ev=ev); W.kf(1, 2, 3); W.link(1, 2, 20); W.link(1, 3, 1); W.uc(1)
    assert W.R.ordered(1) == ([2], [20]) and W.R.weights(1) == ([2, 3], [20, 1]) and W.R.weights(3) == ([], [])
    W.consistency([3], expect=dict(status=0, enough=[], groups=[([3], 0)]), what='row-not-list 1')
    W.consistency([1], expect=dict(status=0, enough=[], groups=[([1, 2, 3], 1)]), what='row-not-list 2')
    W.close()


def case_pushed_twice(lib, ev):
    """stored ({3}, 1) and ({4}, 0); candidate 1 holds both 3 and 4 in its row: its own group goes in twice, with counters 2 and 1, and at th = 2 it is enough once"""
    # 3 is 1's maximum, so UpdateConnections(1) told 3 about 1: keep 3 and 4 apart from 1 by giving 1 its row through two weak links and a strong third neighbour
    W = World(lib, ev=ev); W.kf(1, 3, 4, 9); W.link(1, 9, 5); W.link(1, 3, 2); W.link(1, 4, 1); W.uc(1)
    assert W.R.weights(3) == ([], []) and W.R.weights(4) == ([], []) and W.R.weights(1) == ([3, 4, 9], [2, 1, 5])
    W.consistency([3], th=2, expect=dict(enough=[], groups=[([3], 0)]), what='twice 1')
    W.consistency([3, 4], th=2, expect=dict(enough=[], groups=[([3], 1), ([4], 0)]), what='twice 2')
    W.consistency([1], th=2, expect=dict(enough=[1], groups=[([1, 3, 4, 9], 2), ([1, 3, 4, 9], 1)]), what='twice 3')
    W.close()


def case_pushed_nothing(lib, ev):
    """stored ({3}, 0); candidates 1 and 5 both hold 3: 1 takes the group, 5 finds it marked and pushes nothing, not even with 0; at th = 1 the test is made for the
    marked group too and both are enough"""
    W = World(lib, ev=ev); W.kf(1, 3, 5, 8, 9); W.link(1, 9, 5); W.link(1, 3, 1); W.link(5, 8, 5); W.link(5, 3, 1); W.uc(1, 5)
    assert W.R.weights(3) == ([], [])
    W.consistency([3], th=1, expect=dict(enough=[], groups=[([3], 0)]), what='nothing 1')
    want = W.consistency([1, 5], th=1, expect=dict(enough=[1, 5], groups=[([1, 3, 9], 1)]), what='nothing 2')
    assert want['report']['n_pushed_nothing'] == 1 and want['report']['n_consistent'] == 2
    # 5 comes first now and takes the group; 1 finds it marked
    W.consistency([5, 1], th=9, expect=dict(enough=[], groups=[([3, 5, 8], 2)]), what='nothing 3')
    W.close()


def case_order_and_clear(lib, ev):
    """the new list is in candidate order, then iG order; no candidate clears the groups"""
    W = World(lib, ev=ev); W.kf(1, 2, 3, 4, 5)
    W.consistency([4, 2], expect=dict(groups=[([4], 0), ([2], 0)]), what='order 1')
    W.consistency([2, 5, 4], expect=dict(groups=[([2], 1), ([5], 0), ([4], 1)]), what='order 2')
    W.consistency([4, 2], expect=dict(groups=[([4], 2), ([2], 2)]), what='order 3')
    W.consistency([2, 4], expect=dict(enough=[2, 4], groups=[([2], 3), ([4], 3)]), what='order 4')
    W.consistency([], expect=dict(status=0, enough=[], groups=[]), what='clear')
    W.consistency([2], expect=dict(enough=[], groups=[([2], 0)]), what='after clear')
    W.close()


def case_errors(lib, ev):
    """rule 13: an unknown id, an erased id, a duplicate: refused with the groups and the outputs untouched; max_groups at the need and one short"""
    W = World(lib, max_groups=3, ev=ev); W.kf(1, 2, 3, 4, 5, 6); W.link(5, 4, 9); W.link(5, 6, 3); W.uc(5)             # 4, the maximum, hears of 5; 6 does not
    W.consistency([1, 2], expect=dict(groups=[([1], 0), ([2], 0)]), what='err 0')
    W.consistency([1, 99], expect=dict(status=-1), what='unknown')
    W.consistency([2, 1, 2], expect=dict(status=-1), what='duplicate')
    W.erase(6); W.consistency([6], expect=dict(status=-1), what='erased')
    W.consistency([1, 2, 3, 4], expect=dict(status=-3), what='one short')
    W.consistency([1, 2, 3], expect=dict(status=0, groups=[([1], 1), ([2], 1), ([3], 0)]), what='at the need')
    W.consistency([5], expect=dict(groups=[([4, 5], 0)]), what='dead in row')              # 5's row still names the erased 6 (rule 12)
    if W.G is not None:
        assert W.G.consistency_info() == (3 * (9 * 64 + 24) + 8 * 64 + 32, 1, 3)
        W.G.clear(); assert W.G.consistency_info() == (0, 0, 0) and W.G.consistent_groups() == []
    W.close()


def case_counts(lib, ev):
    """candidate counts and stored-group counts of 0, 1, 2, 63, 64, 65 (the wave and its neighbours), max_groups exactly 65"""
    W = World(lib, max_keyframes=80, cap=8, max_groups=65, ev=ev); W.kf(*range(70))
    for stored in (0, 1, 2, 63, 64, 65):
        for n in (0, 1, 2, 63, 64, 65):
            W.clear_groups()
            if stored: W.consistency(list(range(stored)), what=('counts', stored))
            W.consistency(list(range(69, 69 - n, -1)) if n % 2 else list(range(2, 2 + n)), th=1, what=('counts', stored, n))
    W.close()


def case_slots(lib, ev):
    """group members at slots 31, 32, 63, 64 and 257 (keyframes take the slots in the order they are added): candidate 1000 holds them all in its row"""
    W = World(lib, max_keyframes=260, cap=16, ev=ev); W.kf(*[1000 + s for s in range(258)])
    far = [1031, 1032, 1063, 1064, 1257]
    W.link(1000, 1001, 3)
    for k in far: W.link(1000, k, 1)
    W.uc(1000)
    W.consistency(far, what='slots 1')
    want = W.consistency([1000], th=1, what='slots 2')
    assert want['report']['n_after'] == 5 and want['enough'] == [1000] and W.D.groups()[0][0] == [1000, 1001] + far
    W.close()


def case_stale_slot(lib, ev):
    """a full handle of 4: the stored group names keyframe 3; 3 is erased and 7 takes its slot.  Candidate 7 shares the SLOT with the stored group and no id: it is not
    consistent.  The stored group still shows 3."""
    W = World(lib, max_keyframes=4, ev=ev); W.kf(1, 2, 3, 4)
    W.consistency([3], expect=dict(groups=[([3], 0)]), what='stale 1')
    W.erase(3); W.kf(7); W.link(7, 1, 2); W.uc(7)
    if W.G is not None: assert W.G.size() == 4
    W.consistency([7], th=1, expect=dict(enough=[], groups=[([1, 7], 0)]), what='stale 2')
    W.close()


def case_connected(lib, ev):
    """GetConnectedKeyFrames of a batch: every count >= 1, dead entries left out, an unknown keyframe, the capacity at the need and one short"""
    W = World(lib, ev=ev); W.kf(1, 2, 3, 4, 5); W.link(1, 2, 20); W.link(1, 3, 1); W.link(1, 5, 16); W.link(4, 2, 15); W.uc(1, 4)
    want = W.connected([1, 4, 2], what='conn')
    assert want['rows'] == [[2, 3, 5], [2], [1, 4]] and want['off'] == [0, 3, 4, 6]
    W.connected([1, 99, 4], what='conn unknown')
    for cap in (6, 5, 3, 2, 0): W.connected([1, 4, 2], cap, what=('conn cap', cap))
    W.erase(5); assert W.connected([1], what='conn dead')['rows'] == [[2, 3]]
    W.close()


def chain_world(lib, n, ev, seed):
    """a chain: keyframe i shares 20 points with i - 1 and 2 with i - 2, 1 with a random earlier one"""
    rng = np.random.default_rng(seed)
    W = World(lib, max_keyframes=n + 4, cap=64, max_points=32 * n, ev=ev)
    for i in range(n):
        W.kf(i)
        if i >= 1: W.link(i, i - 1, 20)
        if i >= 2: W.link(i, i - 2, 2)
        if i >= 4: W.link(i, int(rng.integers(0, i - 2)), 1)
        W.uc(i)
    return W, rng


def case_walk(lib, ev, seed):
    """30 consecutive keyframes, each with 0 to 4 candidates drawn near an early stretch of a chain of 60; groups, counters and enough-lists after every call"""
    W, rng = chain_world(lib, 60, ev, seed)
    centre = int(rng.integers(3, 10)); n_enough = 0
    for t in range(30, 60):
        k = int(rng.integers(0, 5)) if t % 7 else 0
        cands = [int(c) for c in rng.permutation(np.arange(max(centre - 4, 0), centre + 5))[:k]]
        n_enough += len(W.consistency(cands, what=('walk', seed, t))['enough'])
        if t == 45: W.erase(centre + 6)                                          # an erased keyframe the stored groups and some rows still name
    assert n_enough > 0
    W.close()


HAND = (case_row_not_list, case_pushed_twice, case_pushed_nothing, case_order_and_clear, case_errors, case_counts, case_slots, case_stale_slot, case_connected)
SEEDS = (1, 2, 3)


def check_events():
    ev = dict.fromkeys(ref.EVENTS, 0)
    for c in HAND: c(None, ev)
    for s in SEEDS: case_walk(None, ev, s)
    assert all(ev[k] for k in REQUIRED), ev


def check_two_runs_identical(lib):
    outs = []
    for _ in range(2):
        W, rng = chain_world(lib, 40, dict.fromkeys(ref.EVENTS, 0), 5)
        o = []
        for t in range(8):
            g = W.G.consistency([3 + t % 3, 9, 4 + t % 2 * 20], th=2)
            o += [g['raw'][0].tobytes(), g['raw'][1].tobytes(), g['report'].tobytes(), repr(W.G.consistent_groups()).encode()]
        c = W.G.connected_batch([5, 6, 7, 30])
        o += [c['raw'].tobytes(), c['off'].tobytes()]
        outs.append(b''.join(o)); W.close()
    assert outs[0] == outs[1]


# ---- RunGlobalBundleAdjustment's map update: trees built through UpdateConnections (a keyframe's parent is its only neighbour at its first connection) ---------------
GBA_REQUIRED = ('chain_depth3', 'unreached', 'point_skipped', 'reparented', 'two_origins')
PATTERN = 0x7fc0dead                                                             # what the outputs hold before a call: a NaN with a payload


def bits(a):
    return np.ascontiguousarray(a, 'f4').view('u4')


def random_poses(rng, n, step=0.05):
    """n rigid poses (3 x 4 float32) and a perturbed copy (what global BA would leave)"""
    def rot(v):
        th = np.linalg.norm(v); k = v / th; K = np.array([[0, -k[2], k[1]], [k[2], 0, -k[0]], [-k[1], k[0], 0]])
        return np.eye(3) + np.sin(th) * K + (1 - np.cos(th)) * K @ K
    T = np.zeros((n, 3, 4), 'f4'); G = np.zeros((n, 3, 4), 'f4')
    for i in range(n):
        R = rot(rng.normal(size=3) * 0.7 + 1e-3); t = rng.normal(size=3) * 3
        T[i, :, :3] = R; T[i, :, 3] = t
        G[i, :, :3] = rot(rng.normal(size=3) * step + 1e-3) @ R; G[i, :, 3] = t + rng.normal(size=3) * step
    return T, G


def tree_world(lib, parents, ev, cap=64, extra=0):
    """parents: {id: parent id or None} in insertion order"""
    W = World(lib, max_keyframes=len(parents) + extra + 2, cap=cap, max_points=4 * (len(parents) + extra) + 64, ev=ev)
    for k, p in parents.items():
        W.kf(k)
        if p is not None: W.link(k, p, 2); W.uc(k)
        assert W.R.tree(k)[0] == (p if p is not None else -1), (k, p, W.R.tree(k))
    return W


def play_gba(W, origins, outside, seed, ev, what='', n_points=200, kf_ids=None, expect_status=0):
    """outside: the ids that were not in the GBA"""
    rng = np.random.default_rng(seed)
    ids = sorted(W.R.kfs) if kf_ids is None else list(kf_ids); nk = len(ids)
    in_gba = [k not in outside for k in ids]
    T, G = random_poses(rng, nk)
    xw = rng.normal(size=(n_points, 3)).astype('f4') * 4; xg = (xw + rng.normal(size=(n_points, 3)).astype('f4') * 0.05).astype('f4')
    pg = rng.random(n_points) < 0.5; pref = rng.integers(-1, nk, n_points).astype('i4')
    R_ = ref
    S = R_.gba_update(W.R, list(origins), ids, in_gba, T, G, ev)
    assert S['status'] == expect_status, (what, S['status'])
    want_x = R_.gba_correct_points(xw, pg, xg, pref, S, ev) if S['status'] == 0 else None
    if W.G is None: return S
    got = W.G.gba_update(origins, ids, in_gba, T, G, points=dict(xw=xw, in_gba=pg, xw_gba=xg, ref=pref), poison=PATTERN)
    assert got['status'] == S['status'], (what, got['status'], S['status'])
    if S['status'] != 0:
        assert (bits(got['Tcw_out']) == PATTERN).all() and (bits(got['TcwBef']) == PATTERN).all() and (got['kf_state'] == 0x55).all() and got['xw_out'] is None, (what, 'a refused call wrote')
        return S
    for k in ('n_visited', 'n_propagated', 'n_unreached', 'max_depth'): assert int(got['report'][k]) == S['report'][k], (what, k, int(got['report'][k]), S['report'][k])
    assert [int(x) for x in got['kf_state']] == S['kf_state'], (what, list(got['kf_state']), S['kf_state'])
    assert (bits(got['Tcw_out']) == bits(S['Tcw_out'])).all(), (what, 'Tcw_out', np.argwhere(bits(got['Tcw_out']) != bits(S['Tcw_out']))[:4])
    for r in range(nk):
        if r in S['TcwBef']: assert (bits(got['TcwBef'][r]) == bits(S['TcwBef'][r])).all(), (what, 'TcwBef', r)
        else: assert (bits(got['TcwBef'][r]) == PATTERN).all(), (what, 'TcwBef of a keyframe that was not visited', r)
    assert (bits(got['xw_out']) == bits(want_x)).all(), (what, 'xw_out', np.argwhere(bits(got['xw_out']) != bits(want_x))[:4])
    return S


def chain(n_in, n_out):
    """0 <- 1 <- ... : n_in optimised keyframes, then n_out outside the GBA hung below the last of them"""
    return {k: (k - 1 if k else None) for k in range(n_in + n_out)}, set(range(n_in, n_in + n_out))


def case_gba_single(lib, ev):
    W = tree_world(lib, {0: None}, ev); S = play_gba(W, [0], set(), 1, ev, 'single origin')
    assert S['report'] == dict(status=0, n_visited=1, n_propagated=0, n_unreached=0, max_depth=0); W.close()


def case_gba_chains(lib, ev):
    for n_out in (1, 2, 40):
        P, out = chain(3, n_out); W = tree_world(lib, P, ev)
        S = play_gba(W, [0], out, 10 + n_out, ev, ('chain', n_out))
        assert S['report']['max_depth'] == n_out and S['report']['n_propagated'] == n_out and S['kf_state'] == [3] * (3 + n_out); W.close()


def case_gba_bushy(lib, ev):
    """300 keyframes, each below a random earlier one; a third of them outside the GBA, in runs down the branches"""
    rng = np.random.default_rng(7); P = {0: None}
    for k in range(1, 300): P[k] = int(rng.integers(max(0, k - 40), k))
    out = set()
    for k in range(1, 300):
        if P[k] in out and rng.random() < 0.8 or rng.random() < 0.12: out.add(k)
    W = tree_world(lib, P, ev); S = play_gba(W, [0], out, 8, ev, 'bushy', n_points=600)
    assert S['report']['n_visited'] == 300 and S['report']['max_depth'] >= 3; W.close()


def case_gba_reparented(lib, ev):
    """2 hangs below 1 and also sees 0; 1 is erased and 2 goes to 0; 3 hangs below 2.  2 and 3 are outside the GBA"""
    W = World(lib, max_keyframes=8, ev=ev); W.kf(0, 1); W.link(1, 0, 20); W.uc(1)
    W.kf(2); W.link(2, 1, 20); W.link(2, 0, 16); W.uc(2); W.kf(3); W.link(3, 2, 20); W.uc(3)
    assert W.R.tree(2)[0] == 1
    W.erase(1); assert W.R.tree(2)[0] == 0 and W.R.tree(0)[2] == [2]; ev['reparented'] += 1
    S = play_gba(W, [0], {2, 3}, 3, ev, 'reparented'); assert S['report']['max_depth'] == 2 and S['kf_state'] == [3, 3, 3]
    W.close()


def case_gba_two_origins_and_unreached(lib, ev):
    """two trees with an origin each; a third root that is no origin, optimised (keeps bit 1, copied through), with a child outside the GBA (state 0)"""
    P = {0: None, 1: 0, 2: 1, 100: None, 101: 100, 200: None, 201: 200}
    W = tree_world(lib, P, ev)
    S = play_gba(W, [0, 100], {2, 101, 201}, 4, ev, 'two origins')
    assert S['kf_state'] == [3, 3, 3, 3, 3, 2, 0] and S['report']['n_unreached'] == 2
    S = play_gba(W, [100], {2, 101, 201}, 5, ev, 'one of two')
    assert S['kf_state'] == [2, 2, 0, 3, 3, 2, 0]
    # an origin below another origin (defined beside rule 14): every keyframe is visited once and TcwBef is the pose before the call
    S = play_gba(W, [0, 1, 100], {2, 101, 201}, 9, ev, 'nested origins')
    assert S['kf_state'] == [3, 3, 3, 3, 3, 2, 0] and S['report']['n_visited'] == 5 and S['report']['max_depth'] == 1
    W.close()


def case_gba_errors(lib, ev):
    """rule 14 and the malformed tables: nothing is written"""
    W = tree_world(lib, {0: None, 1: 0, 2: 1}, ev)
    play_gba(W, [0], {0, 2}, 6, ev, 'origin not in the GBA', expect_status=1)
    play_gba(W, [0, 1], {1}, 6, ev, 'second origin not in the GBA', expect_status=1)
    play_gba(W, [9], set(), 6, ev, 'unknown origin', expect_status=-1)
    play_gba(W, [0], set(), 6, ev, 'a keyframe missing', kf_ids=[0, 1], expect_status=-1)
    play_gba(W, [0], set(), 6, ev, 'a keyframe twice', kf_ids=[0, 1, 1], expect_status=-1)
    play_gba(W, [0], set(), 6, ev, 'an unknown keyframe', kf_ids=[0, 1, 7], expect_status=-1)
    play_gba(W, [0], {2}, 6, ev, 'rows in another order', kf_ids=[2, 0, 1])
    W.close()


GBA = (case_gba_single, case_gba_chains, case_gba_bushy, case_gba_reparented, case_gba_two_origins_and_unreached, case_gba_errors)


def check_gba_events():
    ev = dict.fromkeys(ref.GBA_EVENTS, 0)
    for c in GBA: c(None, ev)
    assert all(ev[k] for k in GBA_REQUIRED), ev


def check_gba_two_runs_identical(lib):
    outs = []
    for _ in range(2):
        P, out = chain(4, 9); W = tree_world(lib, P, dict.fromkeys(ref.GBA_EVENTS, 0))
        rng = np.random.default_rng(2); T, G = random_poses(rng, 13); xw = rng.normal(size=(300, 3)).astype('f4')
        g = W.G.gba_update([0], list(range(13)), [k not in out for k in range(13)], T, G, points=dict(xw=xw, in_gba=np.zeros(300), xw_gba=xw, ref=rng.integers(-1, 13, 300)), poison=PATTERN)
        outs.append(b''.join(g[k].tobytes() for k in ('Tcw_out', 'TcwBef', 'kf_state', 'xw_out', 'report'))); W.close()
    assert outs[0] == outs[1]


# ---- the driver: sg_slam_amd.loopclosing.LoopClosing on a ring of 40 keyframes -------------------------------------------------------------------------------------------
def check_driver_chain(lib):
    """LoopClosing on a ring of 40 keyframes with a scene behind it: the camera goes round a circle facing a wall of points, keyframe t sees the points
    [20 t, 20 t + 150) as loop_cases.check_chain has it, 120 points of keyframe 39 are duplicates of keyframe 0's, the poses carry drift, every observation is the stereo
    projection through the true pose.  The BowVector of keyframe t holds the words of its point range and from keyframe 36 on also those of keyframe t - 36.
    DetectLoop for every keyframe in order: no candidates up to 35 (the groups are cleared), counters 0, 1, 2, 3 from 36 on, so with nCurrentConsistency >= 3
    (LoopClosing.cc:187-194) the loop is accepted at keyframe 39 and not before, and every keyframe is in the database afterwards.  CorrectLoop(39, 0) with the fusion of
    the duplicates; RunGlobalBundleAdjustment(39) with ten keyframes and 60 points created while the solver ran (a chain of four among them): the poses and points
    returned equal the restatement's bit for bit, fed the solver's own poses_gba / points_gba.  DetectLoop then returns early for the ids below 39 + 10."""
    import kfdb_cases as kc
    import sim3_cases as sc
    import covis_cases as cc
    from scenes import CAM
    from sg_slam_amd.keyframedatabase import KeyFrameDatabase
    from sg_slam_amd.loopclosing import LoopClosing
    nkf, step, per = 40, 20, 150; base = step * (nkf - 1) + per; npts = base + 400
    ev = dict.fromkeys(ref.EVENTS, 0); gev = dict.fromkeys(ref.GBA_EVENTS, 0)
    rng = np.random.RandomState(5)
    rot = lambda w: np.array(lr.quat_to_R([float(x) for x in sc.quat_from_rotvec(np.asarray(w, 'f8'))]))
    true = {}; Tcw = {}; drift = np.zeros(6)
    for t in range(nkf):                                                        # the camera goes round a circle of radius 1.5 facing a wall 4 to 8 away; drift accumulates
        a = 2 * np.pi * t / nkf; c = np.array([1.5 * np.cos(a), 1.5 * np.sin(a), 0.0]); R = rot(rng.normal(0, 0.02, 3) + 1e-6)
        true[t] = np.concatenate([R, (-R @ c).reshape(3, 1)], 1).astype('f4')
        if t: drift = drift + rng.normal(0, 0.01, 6)
        D = rot(drift[:3] * 0.3 + 1e-9)
        Tcw[t] = np.concatenate([D @ true[t][:, :3], (D @ true[t][:, 3] + drift[3:]).reshape(3, 1)], 1).astype('f4')
    Scw = np.r_[lr.sim3_of_pose(true[nkf - 1])[:7], 1.0]
    to_world = lambda T, Xc: (np.asarray(Xc, 'f8') - T[:, 3].astype('f8')) @ T[:, :3].astype('f8')      # Rwc * (Xc - tcw)
    home = lambda p: int(np.clip((p - 65) // step, 0, nkf - 1))
    Xc = np.stack([rng.uniform(-1, 1, base), rng.uniform(-0.6, 0.6, base), rng.uniform(4, 8, base)], 1)
    Xtrue = np.array([to_world(true[home(p)], Xc[p]) for p in range(base)]); xw = np.zeros((npts, 3), 'f4')
    xw[:base] = np.array([to_world(Tcw[home(p)], Xc[p]) for p in range(base)])                          # the map as the drifted poses triangulated it
    dup = [(step * (nkf - 1) + 20 + i, i) for i in range(120)]
    for a, b in dup: Xtrue[a] = Xtrue[b]
    def observe(T, X):
        c = X @ T[:, :3].astype('f8').T + T[:, 3].astype('f8')
        u = CAM['fx'] * c[:, 0] / c[:, 2] + CAM['cx']; v = CAM['fy'] * c[:, 1] / c[:, 2] + CAM['cy']
        return np.stack([u, v], 1).astype('f4'), (u - CAM['bf'] / c[:, 2]).astype('f4'), c[:, 2].astype('f4')
    W = World(lib, max_keyframes=64, cap=per + 40, max_points=npts, ev=ev)
    V = kc.make_voc(lib, npts); db = KeyFrameDatabase(V, max_keyframes=64, lib=lib)
    L = LoopClosing(W.G, db, V)
    KF = {}; accepted = []
    def add_kf(k, T_true, pts, Xp):
        uv, ur, z = observe(T_true, Xp); assert (z > 0.5).all(), (k, z.min())
        n = len(pts); pad = W.cap - n
        a = (np.zeros(W.cap, 'i4'), np.r_[ur, np.full(pad, -1, 'f4')].astype('f4'), np.r_[z, np.ones(pad, 'f4')].astype('f4'))
        for m in (W.R, W.G): m.add_keyframe(k, *a); m.set_observations(k, list(range(n)), list(pts))
        W.free[k] = n; KF[k] = dict(uv=np.r_[uv, np.zeros((pad, 2), 'f4')].astype('f4'), uright=a[1])
    for t in range(nkf):
        pts = list(range(step * t, step * t + per)); add_kf(t, true[t], pts, Xtrue[pts]); W.uc(t)
        words = list(pts) + (list(range(step * (t - 36), step * (t - 36) + per)) if t >= 36 else [])
        before = W.D.groups()
        ok = L.DetectLoop(t, kc.bow_of(words))
        if t >= 10:                                                             # the restatement on the candidates the database returned
            want = W.D.consistency(L.last['candidates'], 3, ev)
            assert want['status'] == 0 and want['enough'] == L.mvpEnoughConsistentCandidates and W.G.consistent_groups() == W.D.groups(), (t, want, L.last)
            if t < 36: assert L.last['candidates'] == [] and W.D.groups() == [], (t, L.last)
            else: assert L.last['candidates'] and max(n for _, n in W.D.groups()) == t - 36, (t, L.last, W.D.groups())
        else: assert L.last['early'] and W.G.consistent_groups() == before
        if ok: accepted.append(t)
        assert db.size() == t + 1
    assert accepted == [39] and all(c < 10 for c in L.mvpEnoughConsistentCandidates), (accepted, L.mvpEnoughConsistentCandidates)
    # ---- CorrectLoop: the device through the driver, the restatement's map through the same steps
    cur, loop = nkf - 1, 0
    def fuse(graph, begin_rows, corrected):
        for a, b in dup: graph.replace_point(a, b)
    res = L.CorrectLoop(cur, loop, Scw, Tcw, xw, fuse=fuse, point_ref_kf={p: home(p) for p in range(base)})
    assert L.mLastLoopKFid == cur and W.G.loop_edges(cur) == [loop]
    wb = lr.flatten_begin(W.R, lr.loop_begin(W.R, cur))
    for a, b in dup: W.R.replace_point(a, b)
    lr.loop_connections(W.R, cur, wb['group_id']); W.R.add_loop_edge(loop, cur)
    assert [int(x) for x in res['begin']['group_id']] == wb['group_id']
    for t in range(nkf): KF[t]['Tcw'] = np.r_[res['Tcw'][t], [[0, 0, 0, 1]]].astype('f4'); assert W.G.tree(t) == W.R.tree(t)
    xw1 = res['xw']; pref = {p: home(p) for p in range(base)}
    # ---- RunGlobalBundleAdjustment; LocalMapping made ten keyframes and 60 points while the solver ran
    parent = {40: 39, 41: 40, 42: 41, 43: 42, 44: 39, 45: 20, 46: 45, 47: 0, 48: 47, 49: 30}
    new_T = {}; new_x = {}
    def local_mapping():
        newp = base
        for k, p in parent.items():
            Tp = true[p] if p in true else new_true[p]
            Tk = Tp.copy(); Tk[:, 3] += rng.normal(0, 0.05, 3).astype('f4'); new_true[k] = Tk
            pts = list(range(newp, newp + 6)); newp += 6
            Xp = np.array([to_world(Tk, [rng.uniform(-1, 1), rng.uniform(-0.6, 0.6), rng.uniform(4, 8)]) for _ in pts])
            add_kf(k, Tk, pts, Xp)
            i0 = W.free[p]
            for m in (W.R, W.G): m.set_observations(p, list(range(i0, i0 + 6)), pts)
            W.free[p] += 6; W.uc(k)
            assert W.R.tree(k)[0] == p == W.G.tree(k)[0]
            new_T[k] = (Tk + rng.normal(0, 0.01, (3, 4))).astype('f4')
            for j, q in enumerate(pts): new_x[q] = (Xp[j] + rng.normal(0, 0.02, 3)).astype('f4'); pref[q] = k
    new_true = {}
    inv = (1.0 / 1.2 ** (2 * np.arange(8))).astype('f4')
    out = L.RunGlobalBundleAdjustment(cur, KF, xw1, inv, CAM, origins=[0], point_ref=pref, new_Tcw=new_T, new_xw=new_x, while_running=local_mapping)
    assert out['status'] == 0 and len(out['kf_ids']) == 50 and len(out['graph']['pose_id']) == nkf and out['problem']['mnBAGlobalForKF'] == cur
    G4 = np.asarray(out['problem']['poses_gba'], 'f4'); assert np.isfinite(G4).all() and np.isfinite(out['problem']['points_gba']).all()
    assert np.abs(G4[:, :3] - np.asarray(out['problem']['poses'], 'f4')[:, :3]).max() > 1e-4, 'the solver moved nothing'
    assert (bits(out['TcwGBA'][:nkf]) == bits(G4[:, :3])).all()                   # the table holds the solver's own output
    S = ref.gba_update(W.R, [0], out['kf_ids'], out['in_gba'], out['Tcw_in'], out['TcwGBA'], gev)
    P = out['points_in']; wx = ref.gba_correct_points(P['xw'], P['in_gba'], P['xw_gba'], P['ref'], S, gev)
    assert S['report']['n_propagated'] == 10 and S['report']['max_depth'] == 4 and gev['chain_depth3'] and S['kf_state'] == [3] * 50 and (P['in_gba'] == 0).sum() == 60
    assert (bits(out['Tcw_out']) == bits(S['Tcw_out'])).all() and (bits(out['xw_out']) == bits(wx)).all()
    for r in range(50): assert (bits(out['TcwBef'][r]) == bits(S['TcwBef'][r])).all()
    assert (bits(np.array([out['Tcw'][k] for k in out['kf_ids']])) == bits(S['Tcw_out'])).all() and (bits(np.array([out['xw'][p] for p in out['point_ids']])) == bits(wx)).all()
    # ---- mLastLoopKFid = 39: the next keyframes leave DetectLoop at :114, the one at 39 + 10 does not
    for k in parent:
        L.DetectLoop(k, kc.bow_of(range(base + 6 * (k - 40), base + 6 * (k - 40) + 6)))
        assert L.last['early'] == (k < cur + 10) and db.size() == k + 1, (k, L.last)
    db.close(); W.close()


def ring_scene(seed=5, nkf=40, step=20, per=150, pad=40):
    """the ring of check_driver_chain as plain arrays, for the C++ mirror: per keyframe (the 40 of the ring, then ten created while the solver runs, each below `parent`
    with its six points also seen by the parent from index i0) uright / depth / uv rows of `cap`, its points, its drifted pose and its words"""
    import sim3_cases as sc
    from scenes import CAM
    rng = np.random.RandomState(seed); base = step * (nkf - 1) + per; cap = per + pad
    rot = lambda w: np.array(lr.quat_to_R([float(x) for x in sc.quat_from_rotvec(np.asarray(w, 'f8'))]))
    true = {}; Tcw = {}; drift = np.zeros(6)
    for t in range(nkf):
        a = 2 * np.pi * t / nkf; c = np.array([1.5 * np.cos(a), 1.5 * np.sin(a), 0.0]); R = rot(rng.normal(0, 0.02, 3) + 1e-6)
        true[t] = np.concatenate([R, (-R @ c).reshape(3, 1)], 1).astype('f4')
        if t: drift = drift + rng.normal(0, 0.01, 6)
        D = rot(drift[:3] * 0.3 + 1e-9)
        Tcw[t] = np.concatenate([D @ true[t][:, :3], (D @ true[t][:, 3] + drift[3:]).reshape(3, 1)], 1).astype('f4')
    to_world = lambda T, Xc: (np.asarray(Xc, 'f8') - T[:, 3].astype('f8')) @ T[:, :3].astype('f8')
    home = lambda p: int(np.clip((p - 65) // step, 0, nkf - 1))
    Xc = np.stack([rng.uniform(-1, 1, base), rng.uniform(-0.6, 0.6, base), rng.uniform(4, 8, base)], 1)
    Xtrue = np.array([to_world(true[home(p)], Xc[p]) for p in range(base)])
    npts = base + 60; xw = np.zeros((npts, 3), 'f4'); xw[:base] = np.array([to_world(Tcw[home(p)], Xc[p]) for p in range(base)])
    dup = [(step * (nkf - 1) + 20 + i, i) for i in range(120)]
    for a, b in dup: Xtrue[a] = Xtrue[b]
    def rows(T, X):
        c = X @ T[:, :3].astype('f8').T + T[:, 3].astype('f8'); n = len(X)
        u = CAM['fx'] * c[:, 0] / c[:, 2] + CAM['cx']; v = CAM['fy'] * c[:, 1] / c[:, 2] + CAM['cy']
        uv = np.zeros((cap, 2), 'f4'); uv[:n] = np.stack([u, v], 1); ur = np.full(cap, -1, 'f4'); ur[:n] = u - CAM['bf'] / c[:, 2]; z = np.ones(cap, 'f4'); z[:n] = c[:, 2]
        assert (c[:, 2] > 0.5).all()
        return uv, ur, z
    kfs = []; free = {}
    for t in range(nkf):
        pts = list(range(step * t, step * t + per)); uv, ur, z = rows(true[t], Xtrue[pts]); free[t] = per
        words = pts + (list(range(step * (t - 36), step * (t - 36) + per)) if t >= 36 else [])
        kfs.append(dict(id=t, parent=-1, i0=0, uv=uv, uright=ur, depth=z, pts=pts, T=Tcw[t], words=sorted(set(words))))
    pref = np.full(npts, -1, 'i4'); pref[:base] = [home(p) for p in range(base)]
    parent = {40: 39, 41: 40, 42: 41, 43: 42, 44: 39, 45: 20, 46: 45, 47: 0, 48: 47, 49: 30}; newp = base
    for k, p in parent.items():
        Tk = true[p].copy(); Tk[:, 3] += rng.normal(0, 0.05, 3).astype('f4'); true[k] = Tk
        pts = list(range(newp, newp + 6)); newp += 6
        Xp = np.array([to_world(Tk, [rng.uniform(-1, 1), rng.uniform(-0.6, 0.6), rng.uniform(4, 8)]) for _ in pts])
        uv, ur, z = rows(Tk, Xp)
        kfs.append(dict(id=k, parent=p, i0=free[p], uv=uv, uright=ur, depth=z, pts=pts, T=(Tk + rng.normal(0, 0.01, (3, 4))).astype('f4'), words=pts))
        free[p] += 6; free[k] = 6; xw[pts] = Xp + rng.normal(0, 0.02, (6, 3)); pref[pts] = k
    Scw = np.r_[lr.sim3_of_pose(true[nkf - 1])[:7], 1.0]
    return dict(nkf=nkf, cap=cap, npts=npts, kfs=kfs, xw=xw, pref=pref, dup=dup, Scw=Scw, cam=CAM, inv=(1.0 / 1.2 ** (2 * np.arange(8))).astype('f4'), cur=nkf - 1, loop=0)
