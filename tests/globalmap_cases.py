"""Seeded operation sequences for the global map (tests/test_globalmap_emu.py, tests/test_globalmap_gpu.py) and what the restatement (tests/globalmap_ref.py) answers
to every operation, computed once and shared.  A case is a parameter set, a capacity and a short list of operations over clouds of a few hundred to a few thousand
points: ('append', xyz, rgba), ('consolidate',), ('reset',), ('max_radius', r) (the test tap; only run on a tap library).

The conditions of tests/cloud_cases.py hold here too and are asserted of the INPUTS of every consolidation: the sums that the device takes in another order than
the reference are exact in double in any order, and no distance lies within 1e-5 (relative) of the threshold.  Each case also asserts what it is there for."""
import numpy as np
import cloud_cases as cc
import cloud_ref
import globalmap_ref as ref

f32 = np.float32
PARAMS = dict(mean_k=8, stddev_mul=1.0, leaf=0.05)


def colours(seed, n):
    c = np.random.RandomState(2000 + seed).randint(0, 256, (n, 3)).astype(np.uint32)
    return (np.uint32(0xff000000) | c[:, 0] << 16 | c[:, 1] << 8 | c[:, 2]).astype(np.uint32)


def wall(seed, ny, nz, x=2.0, y0=-0.6, z0=-0.4, step=0.02, jitter=0.004):
    """ny x nz points on the plane x = const (ROS axes: x ahead), jittered in all three axes: several points per 5 cm voxel"""
    rng = np.random.RandomState(seed)
    j, k = np.meshgrid(np.arange(ny), np.arange(nz), indexing='ij')
    P = np.stack([np.full(ny * nz, x), y0 + step * j.reshape(-1), z0 + step * k.reshape(-1)], 1) + rng.normal(0, jitter, (ny * nz, 3))
    return P.astype(f32), colours(seed, ny * nz)


def lattice(nx, ny, nz, L, origin=(0.0, 0.0, 0.0)):
    """one point per voxel at origin + (i + 1/2) * L: every coordinate and every d2 is exact for L a power of two"""
    i, j, k = np.meshgrid(np.arange(nx), np.arange(ny), np.arange(nz), indexing='ij')
    P = (np.stack([i, j, k], -1).reshape(-1, 3) + 0.5) * L + np.asarray(origin)
    return P.astype(f32), colours(nx * ny * nz, len(P))


def _cases():
    C = []

    def add(name, ops, cap=8192, **pp):
        C.append(dict(name=name, ops=ops, cap=cap, params=dict(PARAMS, **pp)))

    A = wall(1, 60, 40, y0=-0.9); B = wall(2, 60, 40, y0=-0.3)
    add('two_views', [('append',) + A, ('consolidate',), ('append',) + B, ('consolidate',)])
    add('append3', [('append',) + wall(3, 40, 30, y0=-1.0), ('append',) + wall(4, 40, 30, y0=-0.5), ('append',) + wall(5, 40, 30, y0=0.0), ('consolidate',)])
    add('consolidate_twice', [('append',) + wall(6, 50, 40), ('consolidate',), ('consolidate',)])
    few = (np.array([[1, 0, 0], [1, 0.2, 0], [1, 0.4, 0], [1.3, 0, 0.2], [1.001, 0.001, 0.001]], f32), colours(7, 5))
    add('empty_and_few', [('consolidate',), ('append',) + few, ('consolidate',), ('append',) + few, ('consolidate',)])
    add('leaf_overflow', [('append',) + wall(8, 30, 30), ('consolidate',)], leaf=1e-4)
    add('capacity', [('append',) + wall(19, 30, 20), ('append',) + wall(10, 25, 20, y0=0.0), ('append',) + wall(11, 20, 15, y0=0.0), ('consolidate',)], cap=1000)
    P, c = wall(12, 40, 20); P = P.copy()
    P[100] = (np.nan, 1, 1); P[500] = (np.inf, 0, 0); P[700] = (2, -np.inf, 0.1); P[701, 2] = np.nan
    add('non_finite', [('append', P, c), ('consolidate',)])
    n = 6000; leaf = 0.01
    d = cc.drift_translation(n, leaf)
    W = wall(13, 30, 20, x=float(d) + 0.1, y0=0.2, z0=-0.3, step=0.004, jitter=0.001)
    D = np.tile(np.array([[d, 0.3, -0.2]], f32), (n, 1))
    add('world_drift', [('append', np.concatenate([D, W[0]]), np.concatenate([colours(14, n), W[1]])), ('consolidate',)], leaf=leaf)
    L = 0.03125
    add('lattice_wall', [('append',) + lattice(1, 32, 24, L, origin=(1.0, 0.0, 0.0)), ('consolidate',)], leaf=L, mean_k=10)
    # a jittered surface of one point per 5 cm cell and four specks 3, 6, 12 and 20 cells in front of it, far from one another: with mean_k = 8 the first window has
    # r0 = 2, and the specks' nine nearest neighbours are proven by r = 4, 8, 16 and by no window
    rng = np.random.RandomState(15)
    j, k = np.meshgrid(np.arange(44), np.arange(44), indexing='ij')
    S = np.stack([np.full(44 * 44, 3.025), 0.025 + 0.05 * j.reshape(-1), 0.025 + 0.05 * k.reshape(-1)], 1) + rng.uniform(-0.01, 0.01, (44 * 44, 3))
    specks = np.array([[3.025 - 0.05 * 3, 0.225, 0.225], [3.025 - 0.05 * 6, 1.975, 0.225], [3.025 - 0.05 * 12, 0.225, 1.975], [3.025 - 0.05 * 20, 1.975, 1.975]])
    SP = (np.concatenate([S, specks]).astype(f32), colours(16, len(S) + 4))
    add('specks', [('append',) + SP, ('consolidate',)])
    add('specks_whole', [('max_radius', 2), ('append',) + SP, ('consolidate',)])
    return C


CASES = _cases()
NAMES = [c['name'] for c in CASES]
CASE = {c['name']: c for c in CASES}
_EXPECTED = {}


def expected(c):
    """[per operation: the restatement's answer, and the map (xyz, rgba) after it], computed once per process; the input conditions are asserted with it"""
    if c['name'] not in _EXPECTED:
        M = ref.GlobalMap(c['params'], c['cap']); out = []
        for op in c['ops']:
            r = None
            if op[0] == 'append': r = M.append(op[1], op[2])
            elif op[0] == 'consolidate':
                r = M.consolidate()
                if r['flags'] == 0: cc.check_input_conditions(c, r)
            elif op[0] == 'reset': M.xyz = M.xyz[:0]; M.rgba = M.rgba[:0]
            out.append((r, M.xyz.copy(), M.rgba.copy()))
        _EXPECTED[c['name']] = out
    return _EXPECTED[c['name']]


def check_case_contents():
    """every case contains what it is for"""
    E = {n: expected(CASE[n]) for n in NAMES}
    e = E['two_views']; n1 = e[1][0]['n_points']; r = e[3][0]
    mixed = [m for m in r['members'] if m[0] < n1 <= m[-1] and len(m) >= 3]
    assert e[1][0]['flags'] == 0 and r['flags'] == 0 and len(mixed) > 50 and all((np.diff(m) > 0).all() for m in mixed)      # an old map point, then the new points: the summation order
    assert r['n_points_in'] == n1 + 2400 and 0 < r['n_points'] < r['n_voxels'] < r['n_points_in']
    e = E['append3']; assert [x[0]['offset'] for x in e[:3]] == [0, 1200, 2400] and e[3][0]['n_points_in'] == 3600 and e[3][0]['flags'] == 0
    e = E['consolidate_twice']; assert e[2][0]['n_points_in'] == e[1][0]['n_points'] and e[2][0]['flags'] == 0 and e[2][0]['n_voxels'] <= e[1][0]['n_points']
    e = E['empty_and_few']
    assert e[0][0]['flags'] == ref.FEW_POINTS and e[0][0]['n_voxels'] == 0 and e[2][0]['flags'] == ref.FEW_POINTS and e[2][0]['n_voxels'] == 4 and e[4][0]['n_voxels'] == 4
    assert len(e[2][1]) == 5 and len(e[4][1]) == 10 and cc.bits(e[4][1][:5]).tobytes() == cc.bits(CASE['empty_and_few']['ops'][1][1]).tobytes()      # the map is as it was
    e = E['leaf_overflow']; assert e[1][0]['flags'] == ref.LEAF_TOO_SMALL and e[1][0]['n_voxels'] == 0 and len(e[1][1]) == 900 == e[1][0]['n_points']
    e = E['capacity']; assert [(x[0]['flags'], x[0]['offset'], x[0]['map_size']) for x in e[:3]] == [(0, 0, 600), (ref.FULL, -1, 600), (0, 600, 900)] and e[3][0]['flags'] == 0
    e = E['non_finite']
    assert (~np.isfinite(e[0][1]).all(1)).sum() == 4 and len(e[0][1]) == 800 and np.isfinite(e[1][1]).all() and e[1][0]['flags'] == 0
    assert sum(len(m) for m in e[1][0]['members']) == 796
    c = CASE['world_drift']; e = E['world_drift'][1][0]; g = e['grid']
    v = int(np.argmax([len(m) for m in e['members']])); centre = c['ops'][0][1][:1]
    assert len(e['members'][v]) == 6000 and cloud_ref.cell_index(e['voxels'][v:v + 1], g)[0] != e['voxel_idx'][v] == cloud_ref.cell_index(centre, g)[0]      # the centroid lies outside its voxel
    assert e['flags'] == 0 and e['n_points'] > 50
    e = E['lattice_wall'][1][0]; L = f32(0.03125)
    i = int(np.argmin(((e['voxels'] - e['voxels'].mean(0)) ** 2).sum(1))); t = e['terms'][i]      # an interior point: 4 at L, 4 at sqrt(2) L, then 2 of the 4 at 2 L, which lie on the border of the r0 = 2 window
    assert e['n_voxels'] == 32 * 24 and (t[:4] == L).all() and (t[8:] == 2 * L).all() and len(t) == 10 and e['dist'][i] == e['dist'].min()
    d2 = ((e['voxels'] - e['voxels'][i]) ** 2).sum(1)
    assert (d2 == f32(4) * L * L).sum() == 4                         # twice as many candidates at the K-th distance as are taken
    e = E['specks'][1][0]; sp = e['voxels'][:, 0] < 2.95
    assert sp.sum() == 4 and not e['kept'][sp].any() and e['kept'][~sp].sum() > 1800 and e['flags'] == 0
    near = e['terms'][sp][:, 0].astype('f8') / 0.05                  # the nearest neighbour of every speck, in cells
    assert sorted(int(round(v)) for v in near) == [3, 6, 12, 20], near
    a, b = E['specks'], E['specks_whole']
    assert a[1][0]['dist'].tobytes() == b[2][0]['dist'].tobytes() and a[1][1].tobytes() == b[2][1].tobytes()


def _xyz(p):
    return np.stack([p['x'], p['y'], p['z']], 1) if len(p) else np.zeros((0, 3), f32)


def assert_map(pts, xyz, rgba, what):
    assert len(pts) == len(xyz), (what, len(pts), len(xyz))
    assert (cc.bits(_xyz(pts)) == cc.bits(xyz)).all() and (pts['rgba'] == rgba).all(), what       # coordinates (NaN payloads and the sign of a zero included), colours, order


def assert_record(rec, e, what):
    for k in ('n_points_in', 'n_voxels', 'n_points', 'flags'): assert int(rec[k]) == int(e[k]), (what, k, int(rec[k]), int(e[k]))
    assert float(rec['mean']) == float(e['mean']) and float(rec['thr']) == float(e['thr']), (what, rec['mean'], e['mean'], rec['thr'], e['thr'])


def assert_taps(tap, e, what):
    vox, dist, kept, tier = tap
    assert len(vox) == e['n_voxels'], what
    assert (cc.bits(_xyz(vox)) == cc.bits(e['voxels'])).all() and (vox['rgba'] == e['voxel_rgba']).all(), what
    assert (cc.bits(dist) == cc.bits(e['dist'])).all() and (kept == e['kept']).all(), what


def run_case(lib, c):
    """the operations of a case on `lib` against the restatement: every record and the whole map after every operation, and with a tap library the voxel cloud, the
    distances and the kept flags of every consolidation.  Returns the consolidation records and the last tap"""
    from sg_slam_amd.globalmap import GlobalMap
    from sg_slam_amd.capi import CLOUD_POINT_DTYPE
    E = expected(c); recs = []; tap = None
    if any(op[0] == 'max_radius' for op in c['ops']) and not lib.has_taps: return None, None
    M = GlobalMap(c['params'], c['cap'], lib=lib)
    for i, (op, (e, xyz, rgba)) in enumerate(zip(c['ops'], E)):
        what = '%s[%d] %s' % (c['name'], i, op[0])
        if op[0] == 'append':
            p = np.zeros(len(op[1]), CLOUD_POINT_DTYPE); p['x'], p['y'], p['z'] = op[1][:, 0], op[1][:, 1], op[1][:, 2]; p['rgba'] = op[2]
            r = M.append(p)
            assert {k: int(r[k]) for k in ('n_in', 'offset', 'map_size', 'flags')} == e, (what, r, e)
        elif op[0] == 'consolidate':
            r = M.consolidate(); recs.append(r)
            assert_record(r, e, what)
            if lib.has_taps:
                tap = M.debug_read(); assert_taps(tap, e, what)
        elif op[0] == 'reset': M.reset()
        elif op[0] == 'max_radius': M.debug_max_radius(op[1])
        assert M.size() == len(xyz), what
        assert_map(M.points(), xyz, rgba, what)
    M.close()
    return recs, tap


def check_case_figures(name, recs, tap):
    """what a case asserts of the implementation's own figures (the window counts and the tiers)"""
    if recs is None: return
    r = recs[-1]
    if name == 'lattice_wall': assert r['wider_window_points'] > 300 and r['whole_cloud_points'] == 0            # the K-th neighbour ties on the border of the first window
    if name == 'specks':
        assert r['wider_window_points'] >= 4 and r['whole_cloud_points'] >= 1
        if tap is not None: assert set(tap[3].tolist()) >= {2, 4, 8, 16, 0}, sorted(set(tap[3].tolist()))      # every tier occurs
    if name == 'specks_whole':
        assert r['whole_cloud_points'] >= 4 and r['wider_window_points'] == r['whole_cloud_points'] and set(tap[3].tolist()) == {2, 0}
    if name in ('empty_and_few', 'leaf_overflow'): assert all(x['wider_window_points'] == 0 and x['whole_cloud_points'] == 0 for x in recs)
