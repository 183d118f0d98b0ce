"""Seeded synthetic keyframes for PointCloudMapping's cloud (tests/test_cloud_emu.py, tests/test_cloud_gpu.py) and the expected cloud of every case from the
restatement (tests/cloud_ref.py), computed once and shared.

The device takes three sums in another order than the reference does (the neighbour sum of a voxel point and the two global sums of the outlier filter), which is
the same value only where the sums are exact in double; and a comparison against the threshold must not sit on a rounding.  These are conditions on the INPUTS,
asserted here for every case: the restatement's sequential sums equal math.fsum and are exact in any order, and no distance lies within 1e-5 (relative) of the
threshold.  Each case also asserts that it contains what it is for."""
import math
import numpy as np
import cloud_ref as ref
import obj3d_ref
from obj3d_cases import scene, pose, cam_for, exact_any_order

f32 = np.float32
LOCAL, WORLD = ref.LOCAL, ref.WORLD
PARAMS = dict(mean_k=8, stddev_mul=1.0, leaf=0.05, consider_dynamic=1, depth_min=0.5, depth_max=5.0)
TUM3_PARAMS = dict(mean_k=50, stddev_mul=3.0, leaf=0.01, consider_dynamic=1, depth_min=0.5, depth_max=5.0)       # PointCloudMapping.* of tests/golden/settings_mapping/TUM3.yaml


def colors(seed, W, H):
    return np.random.RandomState(1000 + seed).randint(0, 256, (H, W, 3)).astype(np.uint8)


def drift_translation(n, leaf):
    """a camera centre c (in ROS axes: the point every skipped pixel becomes in WORLD mode) whose running float sum over n copies, divided by n, lies in another
    cell than c itself: searched over cell borders, first hit"""
    inv = f32(1) / f32(leaf)
    for k in range(150, 400):
        for eps in (1e-6, 3e-6, 1e-5, -1e-6, -3e-6, -1e-5, 3e-5, -3e-5):
            c = f32(k * float(f32(leaf)) + eps)
            s = np.add.accumulate(np.full(n, c, f32), dtype=f32)[-1] / f32(n)
            if np.floor(f32(s * inv)) != np.floor(f32(c * inv)): return c
    raise AssertionError('no drifting camera centre found')


def _cases():
    C = []

    def add(name, W, H, depth, mode=LOCAL, Twc=None, boxes=(), have_dynamic=0, cam=None, seed=0, **pp):
        C.append(dict(name=name, W=W, H=H, cam=cam_for(W, H) if cam is None else cam, depth=np.asarray(depth, f32), color=colors(seed, W, H), mode=mode,
                      Twc=np.eye(4) if Twc is None else Twc, boxes=[tuple(float(f32(v)) for v in b) for b in boxes], have_dynamic=have_dynamic, params=dict(PARAMS, **pp)))

    W, H = 64, 48
    # fronto-parallel plane at depth 1, a camera whose pixel rays are multiples of 1 / 64, a leaf of two pixels: the centroids are an exact lattice
    add('lattice_wall', W, H, np.full((H, W), 1.0), cam=(64.0, 64.0, 32.0, 24.0), leaf=0.03125, seed=1)
    # two slanted planes under a rotated pose, WORLD mode: coordinates of both signs
    add('tilted_planes', W, H, scene(31, W, H, wall=(1.4, 0.006, -0.004), boxes=[(20, 10, 44, 36, 0.9, -0.005)]), mode=WORLD, Twc=pose((0.4, -0.7, 0.3), (0.05, 0.6, -1.0)), seed=2)
    d = scene(32, W, H, wall=(1.2, 0.003, 0.002))
    d[2:6, 3:9] = np.nan; d[10:14, 40:46] = np.inf; d[20:25, 5:10] = 0.3; d[30:34, 50:56] = 6.0; d[40:44, 20:26] = 0.5; d[40:46, 40:46] = 5.0; d[8, 8] = -np.inf; d[9, 9] = -1.0
    add('holes', W, H, d, seed=3)
    add('dynamic_boxes', W, H, scene(33, W, H, wall=(1.3, 0.004, 0.001)), boxes=[(10.6, 8.3, 20.5, 15.7), (25.2, 18.9, 18.4, 14.2)], have_dynamic=1, seed=4)
    d = scene(34, W, H, wall=(1.2, 0.002, 0.001)); d[20:24, 30:34] = 4.0
    add('far_speck', W, H, d, seed=5)
    d = scene(35, W, H, wall=(0.62, 0.001, 0.001), noise=0.002); d[:12, :] = 0
    add('long_runs', W, H, d, leaf=0.2, seed=6)
    add('all_invalid', W, H, np.zeros((H, W)), seed=7)
    d = np.zeros((H, W)); d[20:22, 30:32] = 1.5
    add('few_points', W, H, d, seed=8)
    add('leaf_too_small', W, H, scene(36, W, H, wall=(2.0, 0.02, 0.01)), leaf=1e-4, seed=9)
    W2, H2 = 160, 120
    d = np.zeros((H2, W2)); d[50:64, 70:90] = scene(37, 20, 14, wall=(1.0, 0.002, 0.001))
    c = drift_translation(W2 * H2 - 20 * 14, 0.01)
    T = np.eye(4); T[:3, 3] = (0.3, -0.2, float(c))                  # ROS axes: (z, -x, -y): the drifting coordinate is the cloud's x
    add('world_drift', W2, H2, d, mode=WORLD, Twc=T, leaf=0.01, seed=10)
    add('world_plain', W, H, scene(38, W, H, wall=(1.5, 0.005, 0.002), boxes=[(24, 16, 40, 32, 1.0, 0.0)], outliers=4), mode=WORLD, Twc=pose(), seed=11)
    return C


CASES = _cases()
NAMES = [c['name'] for c in CASES]
CASE = {c['name']: c for c in CASES}
_EXPECTED = {}


def variant(c, **kw):
    """the case with other inputs or parameters (params given as p_<name>)"""
    v = dict(c); v['params'] = dict(c['params'])
    for k, x in kw.items():
        if k.startswith('p_'): v['params'][k[2:]] = x
        else: v[k] = x
    v['name'] = c['name'] + '/' + ','.join('%s=%s' % i for i in sorted(kw.items()))
    return v


def check_input_conditions(c, e):
    """the conditions on the inputs (module docstring) for case c with restatement result e"""
    if e['flags']: return
    dist, terms, thr = e['dist'], e['terms'], e['thr']
    for t in terms[::7]:
        assert obj3d_ref.seq_sum(t) == math.fsum(float(x) for x in t), c['name']
    assert all(exact_any_order(t) for t in terms), c['name']
    sq = (dist * dist).astype(f32)
    assert obj3d_ref.seq_sum(dist) == math.fsum(float(x) for x in dist) and obj3d_ref.seq_sum(sq) == math.fsum(float(x) for x in sq), c['name']
    assert exact_any_order(dist) and exact_any_order(sq), c['name']
    assert np.abs(dist.astype('f8') - thr).min() > 1e-5 * abs(thr), c['name']


def expected(c):
    """the restatement's cloud of a case, computed once per process; the input conditions are asserted with it"""
    if c['name'] not in _EXPECTED:
        e = ref.build(c['depth'], c['color'], c['cam'], c['Twc'], c['boxes'], c['have_dynamic'], c['params'], c['mode'])
        check_input_conditions(c, e)
        _EXPECTED[c['name']] = e
    return _EXPECTED[c['name']]


def check_case_contents():
    """every case contains what it is for"""
    E = {n: expected(CASE[n]) for n in NAMES}
    e = E['lattice_wall']; L = f32(0.03125)
    assert e['n_voxels'] == 32 * 24 and e['flags'] == 0
    ux = np.unique(e['voxels'][:, 0]); assert len(ux) == 32 and (np.diff(ux) == L).all() and (e['voxels'][:, 2] == 1).all()                  # centroids on the lattice, exactly
    interior = e['terms'][np.argmin(e['dist'])]
    assert (interior[:4] == L).all() and (interior[4:] == interior[4]).all() and interior[4] > L                    # four ties at the K-th distance
    e = E['tilted_planes']; assert max(e['grid']['min_b']) < 0 and (e['cloud'].min(0) < 0).all() and (e['cloud'].max(0) > 0).all() and e['n_points'] > 100
    c = CASE['holes']; d = c['depth']; e = E['holes']
    assert np.isnan(d).any() and np.isposinf(d).any() and (d == f32(0.5)).sum() == 24 and (d == f32(5.0)).sum() == 36
    used = ~ref.skipped(d, (), 0, 1, 0.5, 5.0)
    with np.errstate(invalid='ignore'): out_of_range = (d < 0.5) | (d > 5)
    assert used[d == f32(0.5)].all() and used[d == f32(5.0)].all() and not used[~np.isfinite(d)].any() and not used[out_of_range].any() and out_of_range.sum() > 40
    assert e['n_pixels_used'] == int(used.sum()) < 64 * 48 and (e['voxels'] == 0).all(1).sum() == 1               # the skipped pixels are one voxel at the origin
    c = CASE['dynamic_boxes']
    a = E['dynamic_boxes']; b = expected(variant(c, have_dynamic=0)); n = expected(variant(c, p_consider_dynamic=0))
    inside = ref.skipped(np.ones((48, 64), f32), c['boxes'], 1, 1, 0.5, 5.0)
    assert inside.sum() > 300 and not inside[8, :].any() and inside[9, 11] and not inside[9, 10] and inside[32, 42] and not inside[33, 42] and not inside[32, 43]     # strict, truncated
    assert a['n_pixels_used'] == 64 * 48 - inside.sum() and b['n_pixels_used'] == n['n_pixels_used'] == 64 * 48
    assert b['points'].tobytes() == n['points'].tobytes() and b['rgba'].tobytes() == n['rgba'].tobytes() and a['n_points'] != b['n_points']
    assert (a['voxels'] == 0).all(1).sum() == 1 and (b['voxels'] == 0).all(1).sum() == 0
    e = E['far_speck']; far = e['voxels'][:, 2] > 3
    assert far.sum() >= 4 and not e['kept'][far].any() and e['kept'][~far].sum() > 100
    e = E['long_runs']; runs = np.array([len(m) for m in e['members']]); ends = np.cumsum(runs); starts = ends - runs
    origin = int(np.nonzero((e['voxels'] == 0).all(1))[0][0])
    assert e['flags'] == 0 and (runs > 256).sum() >= 3 and runs[origin] > 512
    assert ((starts < 2048) & (ends > 2048)).any() and sum(((starts < b) & (ends > b)).any() for b in range(256, 3072, 256)) >= 8       # runs straddle workgroups and the sort's tile
    for n in ('all_invalid', 'few_points'):
        assert E[n]['flags'] == ref.FEW_POINTS and E[n]['n_points'] == 0 and 1 <= E[n]['n_voxels'] <= 8, n
    assert E['all_invalid']['n_pixels_used'] == 0 and E['few_points']['n_pixels_used'] == 4
    assert E['leaf_too_small']['flags'] == ref.LEAF_TOO_SMALL and E['leaf_too_small']['n_points'] == 0 and E['leaf_too_small']['n_voxels'] == 0
    c = CASE['world_drift']; e = E['world_drift']; g = e['grid']
    centre = ref.ros_axes(np.asarray(c['Twc'], 'f8')[None, :3, 3].astype(f32))[0]
    v = int(np.argmax([len(m) for m in e['members']]))
    assert len(e['members'][v]) == 160 * 120 - 280 and (e['cloud'][e['members'][v]] == centre).all()
    own = ref.cell_index(e['voxels'][v:v + 1], g)[0]
    assert own != e['voxel_idx'][v] and ref.cell_index(centre[None], g)[0] == e['voxel_idx'][v]                      # the centroid of the camera-centre voxel lies outside that voxel
    assert e['flags'] == 0 and e['n_points'] > 50
    assert E['world_plain']['flags'] == 0 and E['world_plain']['n_points'] > 100


def bits(x):
    return np.ascontiguousarray(x, f32).view(np.uint32)


def assert_cloud(pts, rec, e, what):
    """points (CLOUD_POINT_DTYPE) and record == the restatement, bit for bit"""
    for k in ('n_points', 'n_pixels_used', 'n_voxels', 'flags'): assert int(rec[k]) == int(e[k]), (what, k, int(rec[k]), int(e[k]))
    assert float(rec['mean']) == float(e['mean']) and float(rec['thr']) == float(e['thr']), (what, rec['mean'], e['mean'], rec['thr'], e['thr'])
    assert len(pts) == e['n_points'], what
    got = np.stack([pts['x'], pts['y'], pts['z']], 1) if len(pts) else np.zeros((0, 3), f32)
    assert (bits(got) == bits(e['points'])).all(), what                 # coordinates, order, and the sign of a zero
    assert (pts['rgba'] == e['rgba']).all(), what


def assert_taps(tap, e, what):
    vox, dist, kept = tap
    assert len(vox) == e['n_voxels'], what
    got = np.stack([vox['x'], vox['y'], vox['z']], 1) if len(vox) else np.zeros((0, 3), f32)
    assert (bits(got) == bits(e['voxels'])).all() and (vox['rgba'] == e['voxel_rgba']).all(), what
    assert (bits(dist) == bits(e['dist'])).all() and (kept == e['kept']).all(), what


def run_case(lib, c):
    """the single entry against the restatement; with a tap library also the voxel cloud, the distances and the kept flags"""
    from sg_slam_amd.pointcloudmapping import CloudBuilder
    e = expected(c)
    B = CloudBuilder(c['params'], c['W'], c['H'], c['cam'], c['mode'], max_boxes=4, lib=lib)
    pts, rec = B.build(c['depth'], c['color'], c['Twc'], c['boxes'], c['have_dynamic'])
    assert_cloud(pts, rec, e, c['name'])
    if lib.has_taps: assert_taps(B.debug_read(), e, c['name'])
    B.close()
    return rec


def batch_group():
    """the 64 x 48 LOCAL cases with the default parameters, and dynamic_boxes a second time without its flag (a batch has one parameter set)"""
    g = [c for c in CASES if (c['W'], c['H'], c['mode']) == (64, 48, LOCAL) and c['params'] == PARAMS]
    return g + [variant(CASE['dynamic_boxes'], have_dynamic=0)]


def run_batch(lib, cs, B=None):
    from sg_slam_amd.pointcloudmapping import PointCloudMappingBatch
    own = B is None
    if own: B = PointCloudMappingBatch(cs[0]['params'], cs[0]['W'], cs[0]['H'], cs[0]['cam'], len(cs), cs[0]['mode'], max_boxes=4, lib=lib)
    got = B.build(np.stack([c['depth'] for c in cs]), np.stack([c['color'] for c in cs]), np.stack([c['Twc'] for c in cs]), [c['boxes'] for c in cs], [c['have_dynamic'] for c in cs])
    if own: B.close()
    return got


def check_batch_equals_singles(lib, cs):
    """cases of one image size, mode and parameter set as ONE batch against the single entry, byte for byte (larger_window_points included)"""
    from sg_slam_amd.pointcloudmapping import CloudBuilder
    got = run_batch(lib, cs)
    S = CloudBuilder(cs[0]['params'], cs[0]['W'], cs[0]['H'], cs[0]['cam'], cs[0]['mode'], max_boxes=4, lib=lib)
    for c, (pts, rec) in zip(cs, got):
        p1, r1 = S.build(c['depth'], c['color'], c['Twc'], c['boxes'], c['have_dynamic'])
        assert pts.tobytes() == p1.tobytes() and rec.tobytes() == r1.tobytes(), c['name']
        assert_cloud(pts, rec, expected(c), c['name'])
    S.close()
    return got


def tum3_full():
    """640 x 480, TUM3's PointCloudMapping parameters and intrinsics, three keyframes, the second with a person box; the depth range keeps every keyframe between
    20 000 and 60 000 voxel points (asserted)"""
    W, H = 640, 480
    d0 = scene(41, W, H, wall=(1.9, 0.0006, 0.0003), boxes=[(250, 160, 400, 330, 1.4, 0.0003), (60, 60, 110, 120, 1.1, 0.0)], noise=0.0005, outliers=40, holes=0.02)
    d1 = scene(42, W, H, wall=(1.7, -0.0004, 0.0002), boxes=[(300, 120, 420, 440, 1.2, 0.0)], noise=0.0005, nans=0.01, far=20)
    d2 = scene(43, W, H, wall=(2.0, 0.0005, -0.0003), boxes=[(200, 150, 330, 300, 1.5, 0.0002), (400, 180, 470, 330, 1.2, 0.0)], noise=0.0005, outliers=60)
    depths = np.stack([d0, d1, d2]); cols = np.stack([colors(40 + i, W, H) for i in range(3)])
    F = dict(W=W, H=H, cam=cam_for(W, H), depths=depths, colors=cols, Twcs=np.stack([pose(), pose((-0.1, 0.2, 0.05), (1.0, 0.5, -0.2)), pose((0.03, 0.02, -0.01), (-0.5, 0.1, 0.3))]),
             boxes=[[], [(290.5, 110.25, 140.0, 340.5)], []], have_dynamic=[0, 1, 0], params=TUM3_PARAMS)
    for i in range(3):
        P, rgba, used = ref.generate(depths[i], cols[i], F['cam'], None, F['boxes'][i], F['have_dynamic'][i], 1, 0.5, 5.0, LOCAL)
        g, fin, refused = ref.grid_header(P, 0.01)
        nv = len(np.unique(ref.cell_index(P, g)))
        assert not refused and 20000 <= nv <= 60000, (i, nv)
    return F
