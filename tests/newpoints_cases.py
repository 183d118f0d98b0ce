"""Shared cases of the keyframe store and of CreateNewMapPoints over it (sgx_kfstore_*, sgx_create_new_map_points*): scenes, the comparison with the restatement
(newpoints_ref), the margin condition of the device comparison, the chain of the single-pair entries, and the driver walk of sg_slam_amd.localmapping."""
import numpy as np
import newpoints_ref as ref
from scenes import CAM
from sg_slam_amd.capi import KP_DTYPE
from sg_slam_amd.keyframestore import KeyFrameStore

NLEVELS = 8
SF = (1.2 ** np.arange(NLEVELS)).astype('f4'); SG = (SF * SF).astype('f4')
MB = np.float32(CAM['bf']) / np.float32(CAM['fx'])
POISON_I, POISON_F, POISON_B = 0x5A5A5A5A, np.frombuffer(np.array([0x5A5A5A5A], 'u4').tobytes(), 'f4')[0], 0x5A


# ---- scenes ---------------------------------------------------------------------------------------------------------------------------------------------------------------

def rot(w):
    w = np.asarray(w, 'f8'); th = np.linalg.norm(w)
    if th < 1e-12: return np.eye(3)
    k = w / th; K = np.array([[0, -k[2], k[1]], [k[2], 0, -k[0]], [-k[1], k[0], 0]])
    return np.eye(3) + np.sin(th) * K + (1 - np.cos(th)) * K @ K


def pose(centre, w=(0, 0, 0)):
    R = rot(w)
    return np.concatenate([R, (-R @ np.asarray(centre, 'f8')).reshape(3, 1)], 1).astype('f4')


class World:
    """a wall of 3-D points, each with a 256-bit pattern and a vocabulary node"""
    def __init__(self, seed, n_pts, node=lambda p: (p * 2654435761 >> 7) % 97, z=(3.0, 6.0)):
        self.rng = np.random.RandomState(seed)
        self.X = np.stack([self.rng.uniform(-1.5, 1.5, n_pts), self.rng.uniform(-1.0, 1.0, n_pts), self.rng.uniform(z[0], z[1], n_pts)], 1)
        self.desc = self.rng.randint(0, 256, (n_pts, 32)).astype(np.uint8)
        self.node = np.array([node(p) for p in range(n_pts)], 'i4')

    def observe(self, T, ids, noise=0.15, mono_frac=0.2, decoys=0, flips=10, no_node_frac=0.0):
        """a keyframe seeing the points `ids` through pose T: stereo projections with pixel noise, per-observation bit flips, some monocular keypoints, decoy keypoints"""
        rng = self.rng; ids = np.asarray(ids, 'i8'); n = len(ids)
        c = self.X[ids] @ T[:, :3].astype('f8').T + T[:, 3].astype('f8')
        assert n == 0 or (c[:, 2] > 1.0).all()
        u = CAM['fx'] * c[:, 0] / c[:, 2] + CAM['cx'] + rng.normal(0, noise, n); v = CAM['fy'] * c[:, 1] / c[:, 2] + CAM['cy'] + rng.normal(0, noise, n)
        k = np.zeros(n + decoys, KP_DTYPE)
        k['x'][:n] = u; k['y'][:n] = v; k['size'] = 31; k['angle'] = rng.uniform(0, 360, n + decoys); k['octave'][:n] = np.clip(np.floor(np.log(c[:, 2] / 3.0) / np.log(1.2)), 0, NLEVELS - 1)
        k['x'][n:] = rng.uniform(20, 620, decoys); k['y'][n:] = rng.uniform(20, 460, decoys); k['octave'][n:] = rng.randint(0, 3, decoys)
        z = np.r_[c[:, 2], rng.uniform(3, 6, decoys)].astype('f4')
        ur = (k['x'] - CAM['bf'] / z).astype('f4')
        mono = rng.rand(n + decoys) < mono_frac
        ur[mono] = -1; z[mono] = -1
        d = self.desc[ids].copy()
        for r in range(n):
            bits = rng.choice(256, rng.randint(0, flips + 1), replace=False)
            for b in bits: d[r, b >> 3] ^= 1 << (b & 7)
        d = np.concatenate([d, rng.randint(0, 256, (decoys, 32)).astype(np.uint8)])
        node = np.r_[self.node[ids], rng.randint(0, 97, decoys)].astype('i4')
        node[rng.rand(n + decoys) < no_node_frac] = -1
        return dict(keys_un=k, keys=k.copy(), desc=d, uright=ur, depth=z, feat_node=node, Tcw=np.asarray(T, 'f4')[:3, :4].copy(), ids=np.r_[ids, np.full(decoys, -1)])


def random_case(seed, n_cur, n_nb=3, nb_sizes=None, step=0.5, tracked=0.5, node=None, no_node_frac=0.0, decoys=4, mono=False, z=(3.0, 6.0)):
    """a current keyframe of n_cur real keypoints (+ decoys) and n_nb neighbours along a line; a seeded half of the points exists in the map already and is tracked by
    60 % of the keyframes that see it"""
    n_pts = max(n_cur, 1) + 40
    W = World(seed, n_pts, **({} if node is None else dict(node=node)), z=z)
    rng = W.rng; kfs = {}; rows = []
    exists = rng.rand(n_pts) < tracked
    cur = 10; nbs = [3, 7, 1, 5, 8, 2][:n_nb]
    sizes = nb_sizes or [n_cur] * n_nb
    for pos, (kf, n) in enumerate([(cur, n_cur)] + list(zip(nbs, sizes))):
        ids = np.sort(rng.choice(n_pts, n, replace=False)) if n else np.zeros(0, 'i8')
        centre = [0.0, 0.0, 0.0] if pos == 0 else [step * pos * (1 if pos % 2 else -1), 0.03 * pos, 0.02 * pos]
        kfs[kf] = W.observe(pose(centre, rng.normal(0, 0.01, 3)), ids, decoys=decoys if n else 0, no_node_frac=no_node_frac, mono_frac=1.0 if mono else 0.2)
        p = kfs[kf]['ids']
        rows.append(np.where((p >= 0) & exists[np.maximum(p, 0)] & (rng.rand(len(p)) < 0.6), p, -1).astype('i4'))
    md = None
    if mono: md = np.array([4.5] * n_nb, 'f4')
    return dict(kfs=kfs, cur=cur, nbs=nbs, rows=rows, first=1000, median_depth=md)


def hand_case():
    """Four neighbours of 64 keypoints with written answers.  The current keyframe 10 sees the points 0..63 at the keypoints of the same index; all its keypoints but 5
    and 9 hold a point already.  Neighbour 3 (0.5 m to the right) sees point 5 truly and point 9 at a keypoint moved 6 px along the epipolar line with its uright kept, so
    the search accepts both and the triangulation keeps 5 and rejects 9 by the stereo chi-square; neighbour 7 is 2 cm away, below the baseline mb = 7.5 cm; neighbour 1
    (0.5 m to the left) sees both truly: 5 is filled by then and 9 is accepted; neighbour 5 has every feature in a node the current keyframe does not have."""
    W = World(77, 64, node=lambda p: p % 16)
    ids = np.arange(64)
    kfs = {10: W.observe(pose([0, 0, 0]), ids, noise=0.0, mono_frac=0.0), 3: W.observe(pose([0.5, 0, 0]), ids, noise=0.0, mono_frac=0.0),
           7: W.observe(pose([0.02, 0, 0]), ids, noise=0.0, mono_frac=0.0), 1: W.observe(pose([-0.5, 0.01, 0]), ids, noise=0.0, mono_frac=0.0),
           5: W.observe(pose([0.6, 0.1, 0]), ids, noise=0.0, mono_frac=0.0)}
    for k in kfs.values(): k['keys_un']['octave'] = 0; k['keys']['octave'] = 0
    kfs[3]['keys_un']['x'][9] += 6.0; kfs[3]['keys']['x'][9] += 6.0
    kfs[5]['feat_node'] = kfs[5]['feat_node'] + 100
    row = np.arange(64, dtype='i4'); row[[5, 9]] = -1
    rows = [row.copy() for _ in range(5)]
    answers = dict(status=[0, 1, 0, 0], pairs=[[(5, 5), (9, 9)], [], [(9, 9)], []], ok=[[1, 0], [], [1], []], new=[(3, 5, 5), (1, 9, 9)])
    return dict(kfs=kfs, cur=10, nbs=[3, 7, 1, 5], rows=rows, first=500, median_depth=None, answers=answers)


def boundary_cases():
    """name -> case: the smallest shapes at which the kernel can go wrong"""
    out = {'hand': hand_case()}
    out['no_neighbours'] = random_case(1, 40, n_nb=0)
    out['empty_current'] = random_case(2, 0, n_nb=2, nb_sizes=[30, 30])
    for n in (1, 63, 64, 65, 257):
        out['n%d' % n] = random_case(10 + n, n, n_nb=2, decoys=0)
    out['nodes_600'] = random_case(3, 600, n_nb=2, node=lambda p: p, decoys=0)                       # more than 256 common nodes: past the grid-stride
    out['one_node_80'] = random_case(4, 80, n_nb=2, node=lambda p: 0, decoys=0)                      # more than 64 features of one node on each side: past a wave
    out['no_node'] = random_case(5, 90, n_nb=3, no_node_frac=0.3)
    c = random_case(6, 70, n_nb=3); c['nbs'][1] = 999; out['unknown_neighbour'] = c                  # keyframe 999 is not in the store
    c = random_case(7, 70, n_nb=3, step=0.5); c['kfs'][c['nbs'][0]]['Tcw'] = pose([0.03, 0, 0]); out['short_baseline'] = c
    out['mono'] = random_case(8, 80, n_nb=3, mono=True)
    c = random_case(9, 80, n_nb=3, mono=True); c['median_depth'] = np.array([4.5, 200.0, 4.5], 'f4'); out['mono_gate'] = c     # 1 m / 200 m < 0.01
    return out


# ---- running and comparing ------------------------------------------------------------------------------------------------------------------------------------------------

def make_store(lib, case, cap=None, max_keyframes=8):
    cap = cap or max([len(k['keys_un']) for k in case['kfs'].values()] + [1])
    S = KeyFrameStore(CAM, SF, SG, max_keyframes=max_keyframes, cap=cap, lib=lib)
    for kf, d in case['kfs'].items():
        S.add(kf, d['keys_un'], d['desc'], d['uright'], d['depth'], d['feat_node'], d['Tcw'], keys=d['keys'])
    return S


def query_of(case):
    return (case['cur'], case['nbs'], case['rows'], case['first'], case['median_depth'])


def run_ref(orc, case, ev=None, probe=None):
    r = ref.create_new_map_points(orc, case['kfs'], case['cur'], case['nbs'], case['rows'], case['first'], CAM, SF, SG, case['median_depth'], ev)
    return r


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view('u4') if a.dtype == np.float32 else a


def compare(got, want, exact=True, what='', rtol=2e-3):
    """integers for equality; floats bit for bit (exact) or within rtol relative"""
    assert got['n_new'] == want['n_new'], (what, got['n_new'], want['n_new'])
    for k in ('new_kf2', 'new_idx1', 'new_idx2'):
        assert (got[k] == want[k]).all(), (what, k)
    for r, (a, b) in enumerate(zip(got['rows'], want['rows'])):
        assert (a == b).all(), (what, 'row', r)
    gr, wr = got['report'], want['report']
    for k in ('status', 'kf2', 'n_pairs', 'n_new'):
        assert (gr[k] == wr[k]).all(), (what, k, gr[k], wr[k])
    for k in ('baseline', 'F12', 'Ow1', 'Ow2'):                                 # IEEE add / mul / div / sqrt only: bit for bit on the device too
        assert (bits(gr[k]) == bits(wr[k])).all(), (what, k, gr[k], wr[k])
    for j, (g, w) in enumerate(zip(got['pairs'], want['pairs'])):
        for x, y in zip(g, w): assert len(x) == len(y) and (x == y).all(), (what, 'pairs', j)
    assert (got['desc'] == want['desc']).all(), (what, 'desc')
    for k in ('x3d', 'normal', 'min_dist', 'max_dist'):
        if exact: assert (bits(got[k]) == bits(want[k])).all(), (what, k)
        else: assert np.allclose(got[k], want[k], rtol=rtol, atol=0), (what, k, np.abs(got[k] - want[k]).max())


def check_answers(res, case):
    a = case['answers']
    assert list(res['report']['status']) == a['status']
    for j, (p, ok) in enumerate(zip(a['pairs'], a['ok'])):
        assert [(int(x), int(y)) for x, y in zip(res['pairs'][j][0], res['pairs'][j][1])] == p and list(res['pairs'][j][2]) == ok, (j, res['pairs'][j])
    assert [(int(k), int(i), int(j)) for k, i, j in zip(res['new_kf2'], res['new_idx1'], res['new_idx2'])] == a['new']
    for n, (kf2, i1, i2) in enumerate(a['new']):
        assert res['rows'][0][i1] == case['first'] + n and res['rows'][1 + case['nbs'].index(kf2)][i2] == case['first'] + n


def check_poison(S, case, want):
    """outputs that hold nothing stay as they came: the tails of the new-point rows, the pair rows beyond n_pairs, the rows beyond the keyframes' keypoints"""
    r = S.create_new_map_points_batch([query_of(case)], poison=POISON_B, raw=True)[0]
    o = r['raw']; k = want['n_new']; cap = S.cap
    assert (o[7][0, k:] == POISON_I).all() and (o[8][0, k:] == POISON_I).all() and (o[9][0, k:] == POISON_I).all() and (o[11][0, k:] == POISON_B).all()
    for a in (o[10], o[12], o[13], o[14]): assert (a[0, k:].view('u4') == POISON_I).all()
    for j in range(len(case['nbs'])):
        np_ = int(want['report'][j]['n_pairs'])
        assert (o[16][j, np_:] == POISON_I).all() and (o[17][j, np_:] == POISON_I).all() and (o[18][j, np_:] == POISON_B).all()
    for r_, row in enumerate(case['rows']): assert (o[5][r_, len(row):] == -1).all()
    compare(r, want, what='poisoned')


def check_case(lib, orc, name, case, ev=None, exact=True):
    want = run_ref(orc, case, ev)
    S = make_store(lib, case)
    try:
        compare(S.create_new_map_points(*query_of(case)), want, exact, name + ' (host form)')
        got = S.create_new_map_points_batch([query_of(case)])[0]
        compare(got, want, exact, name + ' (batch form)')
        check_poison(S, case, want) if exact else None
        if 'answers' in case: check_answers(want, case); check_answers(got, case)
    finally:
        S.close()
    return want


def check_batch_of_three(lib, orc, exact=True):
    """a batch of 3 queries over one store equals 3 single calls, which equal the restatement"""
    case = random_case(21, 90, n_nb=4)
    qs = [(case['cur'], case['nbs'], case['rows'], 100, None), (case['nbs'][0], [case['cur'], case['nbs'][2]], [case['rows'][1], case['rows'][0], case['rows'][3]], 200, None),
          (case['nbs'][3], [], [case['rows'][4]], 300, None)]
    S = make_store(lib, case)
    try:
        B = S.create_new_map_points_batch(qs)
        for q, b in zip(qs, B):
            compare(b, S.create_new_map_points_batch([q])[0], True, 'batch vs single')
            compare(b, ref.create_new_map_points(orc, case['kfs'], q[0], q[1], q[2], q[3], CAM, SF, SG), exact, 'batch vs restatement')
        assert sum(b['n_new'] for b in B) > 0
    finally:
        S.close()


def check_prefix_and_repeat(lib, case):
    """two runs byte-identical; the first j neighbours' outputs equal a call with j neighbours"""
    S = make_store(lib, case)
    try:
        full = S.create_new_map_points_batch([query_of(case)], poison=POISON_B, raw=True)[0]
        again = S.create_new_map_points_batch([query_of(case)], poison=POISON_B, raw=True)[0]
        for a, b in zip(full['raw'], again['raw']):
            assert (a is None and b is None) or a.tobytes() == b.tobytes()
        for j in range(len(case['nbs']) + 1):
            part = S.create_new_map_points_batch([(case['cur'], case['nbs'][:j], case['rows'][:j + 1], case['first'], None if case['median_depth'] is None else case['median_depth'][:j])])[0]
            k = part['n_new']
            assert k == int(full['report']['n_new'][:j].sum())
            for key in ('new_kf2', 'new_idx1', 'new_idx2', 'x3d', 'desc', 'normal', 'min_dist', 'max_dist'):
                assert bits(part[key]).tobytes() == bits(full[key][:k]).tobytes(), (j, key)
            assert part['report'].tobytes() == full['report'][:j].tobytes()
            for r in range(1, j + 1): assert (part['rows'][r] == full['rows'][r]).all()
    finally:
        S.close()


# ---- the margin condition of the device comparison (b) ---------------------------------------------------------------------------------------------------------------------

def _rel(a, thr):
    return abs(a / thr - 1.0) if thr != 0 else abs(a)


def case_margin(orc, case):
    """the least relative distance between a compared quantity and its threshold over the case, from the restatement's own quantities in float64: the baseline gate, and
    for every candidate pair of a common node the epipolar distance and the epipole distance, for every matched pair the parallax cosines, the depths, the chi-square
    sums and the distance ratio.  Hamming distances are integers on both sides and need no margin."""
    want = run_ref(orc, case)
    worst = [np.inf, None]
    def see(v, what):
        if v < worst[0]: worst[0] = v; worst[1] = what
    rows = [np.array(r, 'i4') for r in case['rows']]
    fx, fy, cx, cy, bf = (float(CAM[k]) for k in ('fx', 'fy', 'cx', 'cy', 'bf')); mb = bf / fx
    a = case['kfs'].get(case['cur'])
    for j, kf2 in enumerate(case['nbs']):
        rp = want['report'][j]
        if rp['status'] == ref.UNKNOWN: continue
        if case['median_depth'] is None: see(_rel(float(rp['baseline']), mb), ('baseline', j))
        else: see(_rel(float(rp['baseline']) / float(case['median_depth'][j]), 0.01), ('baseline ratio', j))
        if rp['status'] != ref.PROCESSED: continue
        b = case['kfs'][kf2]; F = rp['F12'].astype('f8').reshape(3, 3)
        T1 = a['Tcw'].astype('f8'); T2 = b['Tcw'].astype('f8'); O1 = -T1[:, :3].T @ T1[:, 3]; O2 = -T2[:, :3].T @ T2[:, 3]
        with np.errstate(all='ignore'):                                       # a neighbour in the current keyframe's image plane has no finite epipole
            C2 = T2[:, :3] @ O1 + T2[:, 3]; ex = fx * C2[0] / C2[2] + cx; ey = fy * C2[1] / C2[2] + cy
        ka, kb = a['keys_un'], b['keys_un']
        for i1 in range(len(ka)):
            if rows[0][i1] >= 0 or a['feat_node'][i1] < 0: continue
            l = np.array([ka['x'][i1], ka['y'][i1], 1.0]) @ F
            for i2 in np.nonzero((b['feat_node'] == a['feat_node'][i1]) & (rows[j + 1][:len(kb)] < 0))[0]:
                if np.unpackbits(a['desc'][i1] ^ b['desc'][i2]).sum() > 50: continue
                o2 = int(kb['octave'][i2])
                if a['uright'][i1] < 0 and b['uright'][i2] < 0: see(_rel((ex - kb['x'][i2]) ** 2 + (ey - kb['y'][i2]) ** 2, 100 * float(SF[o2])), ('epipole', j, i1, i2))
                num = l[0] * kb['x'][i2] + l[1] * kb['y'][i2] + l[2]
                see(_rel(num * num / (l[0] ** 2 + l[1] ** 2), 3.84 * float(SG[o2])), ('dsqr', j, i1, i2))
        for i1, i2, ok in zip(*want['pairs'][j]):
            s1 = a['uright'][i1] >= 0; s2 = b['uright'][i2] >= 0
            xn1 = np.array([(ka['x'][i1] - cx) / fx, (ka['y'][i1] - cy) / fy, 1.0]); xn2 = np.array([(kb['x'][i2] - cx) / fx, (kb['y'][i2] - cy) / fy, 1.0])
            r1 = T1[:, :3].T @ xn1; r2 = T2[:, :3].T @ xn2; cr = r1 @ r2 / np.linalg.norm(r1) / np.linalg.norm(r2)
            c1 = np.cos(2 * np.arctan2(mb / 2, float(a['depth'][i1]))) if s1 else cr + 1
            c2 = np.cos(2 * np.arctan2(mb / 2, float(b['depth'][i2]))) if (not s1 and s2) else cr + 1
            cs = min(c1, c2)
            see(_rel(cr, cs), ('cosParallaxRays vs stereo', j, i1)); see(abs(cr), ('cosParallaxRays vs 0', j, i1))
            if not (s1 or s2): see(_rel(cr, 0.9998), ('cosParallaxRays vs 0.9998', j, i1))
            if cr < cs and cr > 0 and (s1 or s2 or cr < 0.9998):
                M = np.stack([xn1[0] * T1[2] - T1[0], xn1[1] * T1[2] - T1[1], xn2[0] * T2[2] - T2[0], xn2[1] * T2[2] - T2[1]])
                v = np.linalg.svd(M)[2][3]; X = v[:3] / v[3]
            else:
                if s1 or s2: see(_rel(c1, c2), ('cosParallaxStereo1 vs 2', j, i1))
                if s1 and c1 < c2: z = float(a['depth'][i1]); X = T1[:, :3].T @ (np.array([(a['keys']['x'][i1] - cx) * z / fx, (a['keys']['y'][i1] - cy) * z / fy, z]) - T1[:, 3])
                elif s2 and c2 < c1: z = float(b['depth'][i2]); X = T2[:, :3].T @ (np.array([(b['keys']['x'][i2] - cx) * z / fx, (b['keys']['y'][i2] - cy) * z / fy, z]) - T2[:, 3])
                else: continue
            p1 = T1[:, :3] @ X + T1[:, 3]; p2 = T2[:, :3] @ X + T2[:, 3]
            see(abs(p1[2]), ('z1', j, i1))
            if p1[2] <= 0: continue
            see(abs(p2[2]), ('z2', j, i1))
            if p2[2] <= 0: continue
            dead = False
            for p, kk, idx, st, ur in ((p1, ka, i1, s1, a['uright'][i1]), (p2, kb, i2, s2, b['uright'][i2])):
                u = fx * p[0] / p[2] + cx; v_ = fy * p[1] / p[2] + cy; e = (u - kk['x'][idx]) ** 2 + (v_ - kk['y'][idx]) ** 2
                s2_ = float(SG[int(kk['octave'][idx])])
                if st: e += (u - bf / p[2] - ur) ** 2
                thr = (7.8 if st else 5.991) * s2_
                see(_rel(e, thr), ('chi2', j, i1, idx))
                if e > thr: dead = True; break
            if dead: continue
            d1 = np.linalg.norm(X - O1); d2 = np.linalg.norm(X - O2); rd = d2 / d1; ro = float(SF[int(ka['octave'][i1])]) / float(SF[int(kb['octave'][i2])]); rf = 1.5 * float(SF[1])
            see(_rel(rd * rf, ro), ('ratioDist low', j, i1)); see(_rel(rd, ro * rf), ('ratioDist high', j, i1))
        lo, hi = int(want['report']['n_new'][:j].sum()), int(want['report']['n_new'][:j + 1].sum())
        for n in range(lo, hi):                                                 # the rows as they stand for the next neighbour
            rows[0][want['new_idx1'][n]] = case['first'] + n; rows[j + 1][want['new_idx2'][n]] = case['first'] + n
    return worst[0], worst[1]


def assert_margin(orc, name, case, least=1e-3):
    m, what = case_margin(orc, case)
    assert m >= least, ('case %s has a compared quantity within %g of its threshold' % (name, least), m, what)


# ---- the chain of the single-pair entries on the same library (device comparison (a)) ---------------------------------------------------------------------------------------

def check_against_chain(lib, case, name=''):
    """the batched call equals, bit for bit, sgx_match_search_for_triangulation + sgx_triangulate_new_map_points run neighbour by neighbour on the same library, fed the
    F12 and the centre the new entry reported and the rows as they stood after the previous neighbour: pairs, ok, x3d and the rows"""
    from sg_slam_amd.matcher import ORBmatcher
    from sg_slam_amd import mappoint
    S = make_store(lib, case)
    try:
        got = S.create_new_map_points_batch([query_of(case)])[0]
    finally:
        S.close()
    rows = [np.array(r, 'i4') for r in case['rows']]; a = case['kfs'].get(case['cur']); nnew = 0; total_pairs = 0
    for j, kf2 in enumerate(case['nbs']):
        rp = got['report'][j]
        if rp['status'] != 0: assert rp['n_pairs'] == 0 and rp['n_new'] == 0; continue
        b = case['kfs'][kf2]
        k1 = dict(keys=a['keys_un'], desc=a['desc'], uright=a['uright'], has_mp=(rows[0] >= 0).astype(np.uint8), feat_node=a['feat_node'], cam_center=rp['Ow1'])
        k2 = dict(keys=b['keys_un'], desc=b['desc'], uright=b['uright'], has_mp=(rows[j + 1] >= 0).astype(np.uint8), feat_node=b['feat_node'], Tcw=ref._T44(b['Tcw']))
        n, pairs = ORBmatcher(0.6, False, lib=lib).SearchForTriangulation(k1, k2, rp['F12'], False, CAM, SF, SG)
        assert n == rp['n_pairs'] and (pairs[:, 0] == got['pairs'][j][0]).all() and (pairs[:, 1] == got['pairs'][j][1]).all(), (name, j, n, rp['n_pairs'])
        A = dict(keys_un=a['keys_un'], keys=a['keys'], uright=a['uright'], depth=a['depth'], Tcw=ref._T44(a['Tcw'])); B = dict(keys_un=b['keys_un'], keys=b['keys'], uright=b['uright'], depth=b['depth'], Tcw=ref._T44(b['Tcw']))
        nn, ok, x = mappoint.TriangulateNewMapPoints(pairs, A, B, CAM, SF, SG, lib=lib)
        assert nn == rp['n_new'] and (ok.astype('u1') == got['pairs'][j][2]).all(), (name, j)
        for (i1, i2), good, X in zip(pairs, ok, x):
            if not good: continue
            assert got['new_kf2'][nnew] == kf2 and got['new_idx1'][nnew] == i1 and got['new_idx2'][nnew] == i2 and (bits(got['x3d'][nnew]) == bits(X)).all(), (name, j, nnew)
            rows[0][i1] = case['first'] + nnew; rows[j + 1][i2] = case['first'] + nnew; nnew += 1
        total_pairs += n
    assert nnew == got['n_new']
    for g, w in zip(got['rows'], rows): assert (g == w).all(), name
    return total_pairs, nnew


def stream_case(orc, seed):
    """one current keyframe + 4 neighbours from match2_cases.make_keyframes (ORB on a synthetic stream)"""
    import match2_cases as mc
    kfs = {}; rows = []; ids = [10, 3, 7, 1, 5]
    _, k0, k1 = mc.make_keyframes(orc, seed, 10, 14); _, k2, k3 = mc.make_keyframes(orc, seed, 18, 6); _, k4, _ = mc.make_keyframes(orc, seed, 22, 23)
    for kf, k in zip(ids, (k0, k1, k2, k3, k4)):
        ur = k['uright']; z = np.where(ur >= 0, CAM['bf'] / np.maximum(k['keys']['x'] - ur, 1e-3), -1.0).astype('f4')
        kfs[kf] = dict(keys_un=k['keys'], keys=k['keys'], desc=k['desc'], uright=ur, depth=z, feat_node=k['feat_node'], Tcw=k['Tcw'][:3, :4].copy())
        rows.append(np.where(k['has_mp'] > 0, np.arange(len(ur)) + 100000 * kf, -1).astype('i4'))
    return dict(kfs=kfs, cur=10, nbs=ids[1:], rows=rows, first=7000, median_depth=None)


# ---- the store's own contract ------------------------------------------------------------------------------------------------------------------------------------------------

def check_store_contract(lib):
    """refused mutations leave the store as it was; sizes, bytes, erase / clear / set_pose"""
    from sg_slam_amd.capi import SgxError
    import pytest
    case = random_case(31, 30, n_nb=2, decoys=2); kfs = case['kfs']; cap = 40
    S = KeyFrameStore(CAM, SF, SG, max_keyframes=3, cap=cap, lib=lib)
    try:
        assert S.info() == (3 * (cap * 108 + 64), 0) and S.size() == 0
        for kf, d in kfs.items(): S.add(kf, d['keys_un'], d['desc'], d['uright'], d['depth'], d['feat_node'], d['Tcw'])
        assert S.size() == 3
        d = kfs[case['cur']]; before = S.create_new_map_points(*query_of(case))
        def refused(kf, **over):
            a = dict(d); a.update(over)
            with pytest.raises(SgxError): S.add(kf, a['keys_un'], a['desc'], a['uright'], a['depth'], a['feat_node'], a['Tcw'])
        refused(case['cur'])                                                    # a known id
        refused(77)                                                             # a full store
        S.erase(case['nbs'][1]); assert S.size() == 2
        ko = d['keys_un'].copy(); ko['octave'][3] = NLEVELS; refused(78, keys_un=ko)           # an octave outside the pyramid
        ko['octave'][3] = -1; refused(78, keys_un=ko)
        refused(-1)
        with pytest.raises(SgxError): S.erase(999)
        with pytest.raises(SgxError): S.set_pose(999, d['Tcw'])
        assert S.size() == 2
        after = S.create_new_map_points(*query_of(case))                        # the erased keyframe named as neighbour: its status only
        assert list(after['report']['status']) == [before['report']['status'][0], -1]
        assert after['report'][0].tobytes() == before['report'][0].tobytes() and (after['x3d'][:before['report']['n_new'][0]] == before['x3d'][:before['report']['n_new'][0]]).all()
        e = kfs[case['nbs'][1]]; S.add(case['nbs'][1], e['keys_un'], e['desc'], e['uright'], e['depth'], e['feat_node'], e['Tcw'])      # the slot came back
        compare(S.create_new_map_points(*query_of(case)), before, True, 'after erase + add')
        T = d['Tcw'].copy(); T[0, 3] += 0.05; S.set_pose(case['cur'], T)
        moved = S.create_new_map_points(*query_of(case))
        assert (moved['report']['Ow1'] != before['report']['Ow1']).any() and (moved['report']['baseline'] != before['report']['baseline']).all()
        assert S.info()[1] == 26 * cap
        S.clear(); assert S.size() == 0
        assert list(S.create_new_map_points(*query_of(case))['report']['status']) == [-1, -1]
    finally:
        S.close()
    with pytest.raises(SgxError): KeyFrameStore(CAM, SF, SG, max_keyframes=4097, cap=8, lib=lib)
    with pytest.raises(SgxError): KeyFrameStore(CAM, SF, SG, max_keyframes=4, cap=8193, lib=lib)
    with pytest.raises(SgxError): KeyFrameStore(CAM, SF[:1], SG[:1], max_keyframes=4, cap=8, lib=lib)


# ---- the driver walk -----------------------------------------------------------------------------------------------------------------------------------------------------------

def check_driver_walk(lib, orc, ev, exact=True, n_kf=8, rtol=2e-3):
    """A camera moving past a wall of 400 points, 8 keyframes 0.45 m apart, each seeing a seeded 200 of the points (stereo projections through the true poses, 0.15 px
    noise, at most 10 flipped bits per observation, node = a hash of the point index modulo 97) and 6 decoys.  Keyframe 0's stereo keypoints are Tracking's new points;
    afterwards Tracking gives a seeded 60 % of the keypoints whose point exists that point and creates two new stereo points per keyframe.  Seeded found / visible
    counters, one point removed as the local BA's outlier loop would, and the ages of the points reach every culling branch.  After every ProcessNewKeyFrame /
    MapPointCulling / CreateNewMapPoints the relation, the ordered lists, the recent list and the attribute table equal the restatement's map."""
    from sg_slam_amd.covisibility import CovisibilityGraph
    from sg_slam_amd.localmapping import LocalMapping
    W = World(5, 400); rng = np.random.RandomState(17); cap = 206
    G = CovisibilityGraph(max_keyframes=16, cap=cap, max_points=4096, max_observations=1 << 15, max_queries=2, lib=lib)
    S = KeyFrameStore(CAM, SF, SG, max_keyframes=16, cap=cap, lib=lib)
    L = LocalMapping(G, S); R = ref.LocalMappingRef(orc, CAM, SF, SG); R.ev = ev
    pid_of = {}; next_id = 0; least = (np.inf, None)

    def same(step):
        for kf in R.kf:
            assert list(G.keyframe_points(kf)) == R.R.keyframe_points(kf), (step, kf)
            assert G.ordered(kf) == R.R.ordered(kf), (step, kf)
        assert L.mlpRecentAddedMapPoints == R.recent, step
        assert sorted(L.points) == sorted(R.pt), step
        for pid, p in R.pt.items():
            assert G.observations(pid) == R.R.observations(pid), (step, pid)
            q = L.points[pid]
            for k in ('ref_kf', 'first_kf', 'visible', 'found'): assert q[k] == p[k], (step, pid, k)
            assert (q['desc'] == p['desc']).all(), (step, pid)
            for k in ('xw', 'normal', 'min_dist', 'max_dist'):
                if exact: assert bits(np.asarray(q[k], 'f4')).tobytes() == bits(np.asarray(p[k], 'f4')).tobytes(), (step, pid, k)
                else: assert np.allclose(q[k], p[k], rtol=rtol, atol=1e-6), (step, pid, k)
    try:
        for t in range(n_kf):
            ids = np.sort(rng.choice(400, 200, replace=False))
            d = W.observe(pose([0.45 * t, 0.02 * t, 0.0], rng.normal(0, 0.01, 3)), ids, decoys=6)
            n = len(d['keys_un']); matches = np.full(n, -1, 'i4'); new_stereo = {}
            fresh = [i for i in range(n) if d['ids'][i] >= 0 and d['uright'][i] >= 0 and int(d['ids'][i]) not in pid_of]
            for i in (fresh if t == 0 else fresh[:2]):                          # Tracking's new stereo points
                new_stereo[i] = (next_id, W.X[d['ids'][i]].astype('f4')); matches[i] = next_id; pid_of[int(d['ids'][i])] = next_id; next_id += 1
            for i in range(n):
                w = int(d['ids'][i])
                if matches[i] < 0 and w in pid_of and not R.isBad(pid_of[w]) and rng.rand() < 0.6: matches[i] = pid_of[w]
            kf = dict(d); kf['id'] = t
            L.ProcessNewKeyFrame(kf, matches, new_stereo); R.ProcessNewKeyFrame(t, d, matches, new_stereo); same(('process', t))
            if t == 4:                                                          # an outlier of the local BA among the recent points: the isBad() branch
                victim = R.recent[len(R.recent) // 2]; G.set_points_bad([victim]); R.R.set_points_bad([victim])
            L.MapPointCulling(t); R.MapPointCulling(t); same(('culling', t))
            first = next_id; stop = 2 if t == 5 else None
            nbs = R.R.best_covisibles(t, 10)
            if nbs:
                case = dict(kfs=R.kf, cur=t, nbs=nbs[:stop] if stop else nbs, rows=[R.R.keyframe_points(t)] + [R.R.keyframe_points(k) for k in (nbs[:stop] if stop else nbs)], first=first, median_depth=None)
                least = min(least, case_margin(orc, case), key=lambda m: m[0])
            got = L.CreateNewMapPoints(t, stop_after=stop, first_new_id=first); want = R.CreateNewMapPoints(t, first, stop_after=stop)
            compare(got, want, exact, ('create', t), rtol)
            for k in range(want['n_new']):
                pid = first + k; w = int(d['ids'][want['new_idx1'][k]])
                if w >= 0 and w not in pid_of: pid_of[w] = pid
                vis = int(rng.randint(0, 9)); fnd = int(rng.randint(0, vis + 1)) if rng.rand() < 0.8 else 0        # Tracking's counters
                L.increase_visible(pid, vis); L.increase_found(pid, fnd); R.pt[pid]['visible'] += vis; R.pt[pid]['found'] += fnd
            next_id = first + want['n_new']
            same(('create', t))
        assert least[0] >= 1e-3, ('the walk has a compared quantity within 1e-3 of its threshold', least)
        assert next_id > 300
    finally:
        S.close(); G.close()
