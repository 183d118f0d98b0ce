"""Seeded synthetic scenes for Detector3D (tests/test_obj3d_emu.py, tests/test_obj3d_gpu.py): small depth images with a slanted wall, boxes in front of it, holes,
NaN and out-of-range depth, and the expected record of every case from the restatement (tests/obj3d_ref.py), computed once and shared.

The device takes three sums in another order than the reference does (the neighbour sum of a point, and the two global sums of the outlier filter), which is the same
value only where the sums are exact in double; and a comparison against the threshold or the cluster tolerance must not sit on a rounding.  These are conditions on
the INPUTS, asserted here for every case: the restatement's sequential sums equal math.fsum and are exact in any order, no distance lies within 1e-5 (relative) of the
threshold (the device needs 1e-9; the float64 kd-tree check of the restatement needs the rest), no kept pair's d2 within 1e-6 of the squared tolerance."""
import math
import numpy as np
import obj3d_ref as ref

f32 = np.float32
PARAMS = dict(Sor_MeanK=10, Sor_StddevMulThresh=1.0, Voxel_LeafSize=0.01, EuclideanClusterTolerance=0.05, EuclideanClusterMinSize=50, EuclideanClusterMaxSize=30000,
              DetectSimilarCompareRatio=0.1, camera_valid_depth_Min=0.5, camera_valid_depth_Max=5.0)
TUM3_PARAMS = dict(Sor_MeanK=50, Sor_StddevMulThresh=1.0, Voxel_LeafSize=0.01, EuclideanClusterTolerance=0.02, EuclideanClusterMinSize=1000, EuclideanClusterMaxSize=30000,
                   DetectSimilarCompareRatio=0.1, camera_valid_depth_Min=0.5, camera_valid_depth_Max=5.0)


def cam_for(W, H):
    """TUM3's intrinsics scaled to a W x H image"""
    s = W / 640.0
    return tuple(float(f32(v)) for v in (535.4 * s, 539.2 * s, 320.1 * s, 247.6 * s))


def rot(v):
    v = np.asarray(v, 'f8'); th = np.linalg.norm(v)
    if th == 0: return np.eye(3)
    k = v / th; K = np.array([[0, -k[2], k[1]], [k[2], 0, -k[0]], [-k[1], k[0], 0]])
    return np.eye(3) + math.sin(th) * K + (1 - math.cos(th)) * K @ K


def pose(rvec=(0.05, -0.1, 0.03), t=(0.3, -0.2, 0.4)):
    T = np.eye(4); T[:3, :3] = rot(rvec); T[:3, 3] = t
    return T


def scene(seed, W, H, wall=(2.0, 0.004, 0.002), boxes=(), noise=0.001, holes=0.0, nans=0.0, far=0, outliers=0):
    """depth image: wall = (depth at the centre, slope per pixel in x, in y) or None (no wall: depth 0), boxes = [(u0, v0, u1, v1, depth, slope_x)] drawn in order,
    holes / nans = fraction of pixels set to 0 / NaN, far = number of 6 x 6 patches beyond the valid range, outliers = pixels pulled 0.2 m forward"""
    rng = np.random.RandomState(seed)
    u, v = np.meshgrid(np.arange(W), np.arange(H))
    d = np.zeros((H, W)) if wall is None else wall[0] + wall[1] * (u - W / 2) + wall[2] * (v - H / 2)
    for (u0, v0, u1, v1, dep, sl) in boxes:
        d[v0:v1, u0:u1] = dep + sl * (u[v0:v1, u0:u1] - (u0 + u1) / 2)
    d = d + (d > 0) * rng.normal(0, noise, d.shape)
    for _ in range(far):
        a, b = rng.randint(0, W - 6), rng.randint(0, H - 6); d[b:b + 6, a:a + 6] = 6.0
    for _ in range(outliers):
        a, b = rng.randint(0, W), rng.randint(0, H); d[b, a] = max(d[b, a] - 0.2, 0.0)
    d = d.astype(f32)
    d[rng.uniform(size=d.shape) < holes] = 0
    d[rng.uniform(size=d.shape) < nans] = np.nan
    return d


def _cases():
    C = []
    add = lambda name, W, H, depth, rect, Twc=None, obj=(9, 0.8), **pp: C.append(dict(name=name, W=W, H=H, cam=cam_for(W, H), depth=depth, Twc=pose() if Twc is None else Twc,
                                                                                      obj=(obj[0], obj[1], tuple(float(f32(r)) for r in rect)), params=dict(PARAMS, **pp)))
    # an object in front of a slanted wall, small blobs below min, single outliers; the wall touches the crop border; two clusters survive
    blobs = [(30, 25, 35, 30, 1.55, 0.0), (95, 60, 100, 65, 1.6, 0.0)]
    add('object_wall', 128, 96, scene(1, 128, 96, boxes=[(50, 30, 80, 62, 1.2, 0.002)] + blobs, outliers=12), (10.5, 8.25, 108.0, 80.5))
    add('holes_nan_range', 128, 96, scene(2, 128, 96, boxes=[(48, 28, 84, 66, 1.3, -0.002)], holes=0.1, nans=0.03, far=5, outliers=8), (8.0, 6.0, 112.0, 84.0), obj=(20, 0.6))
    # the wall is the largest component but above max: the smaller object wins
    add('above_max', 160, 120, scene(3, 160, 120, boxes=[(62, 44, 98, 80, 1.1, 0.0)]), (8.0, 6.0, 144.0, 108.0), EuclideanClusterMaxSize=2500)
    # two like clusters left and right of the box centre, no wall: the ratio test rejects
    add('ratio_reject', 128, 96, scene(4, 128, 96, wall=None, boxes=[(34, 34, 56, 60, 1.5, 0.0), (70, 34, 93, 60, 1.5, 0.0)]), (12.0, 10.0, 104.0, 76.0), DetectSimilarCompareRatio=0.5)
    # world z of the near object is below depth_min after Twc: the reference skips it (its quirk) and takes the wall
    add('world_z_quirk', 128, 96, scene(16, 128, 96, boxes=[(50, 30, 80, 62, 1.2, 0.0)]), (10.0, 8.0, 108.0, 80.0), Twc=pose((0.02, 0.01, -0.02), (0.1, 0.0, -0.9)))
    # 70 % holes: the first neighbour window is not enough
    add('holes70', 160, 120, scene(6, 160, 120, boxes=[(60, 40, 104, 84, 1.2, 0.001)], holes=0.7), (2.0, 2.0, 156.0, 116.0), EuclideanClusterTolerance=0.09)
    # fewer crop points than neighbours asked for
    d = scene(7, 96, 72); d[:, :] = 0; d[34:37, 46:49] = 1.5
    add('n_le_k', 96, 72, d, (30.0, 20.0, 36.0, 30.0))
    # nothing reaches min
    add('no_cluster', 96, 72, scene(8, 96, 72, boxes=[(36, 26, 60, 46, 1.2, 0.0)]), (6.0, 4.0, 84.0, 64.0), EuclideanClusterMinSize=5000)
    # two clusters of the same size (no noise, nothing filtered): ordered by their smallest point
    add('equal_size', 96, 72, scene(9, 96, 72, wall=None, boxes=[(26, 22, 40, 36, 1.5, 0.0), (50, 36, 64, 50, 1.5, 0.0)], noise=0.0), (8.0, 6.0, 80.0, 60.0), Sor_StddevMulThresh=10.0,
        DetectSimilarCompareRatio=0.0)
    # an identity pose, a box at the image corner, a non-integer rect
    add('corner_identity', 96, 72, scene(10, 96, 72, boxes=[(8, 6, 40, 34, 1.0, 0.003)], outliers=5), (0.0, 0.0, 70.7, 55.3), Twc=np.eye(4), obj=(5, 0.33))
    return C


def exact_any_order(v):
    """non-negative floats whose sum is exact in double in ANY order: every partial sum is a multiple of the smallest term's ulp and below 2^53 of them"""
    v = np.asarray(v, 'f8'); nz = v[v > 0]
    if len(nz) == 0: return True
    q = 2.0 ** (math.frexp(float(nz.min()))[1] - 1 - 23)          # ulp of the smallest float32 term
    return float(nz.sum()) / q < 2.0 ** 52


def check_input_conditions(c, e):
    """the conditions on the inputs (module docstring) for case c with restatement result e"""
    if e['crop_points'] <= c['params']['Sor_MeanK']: return
    dist, terms, thr = e['dist'], e['terms'], e['thr']
    for t in terms[::7]:
        assert ref.seq_sum(t) == math.fsum(float(x) for x in t), c['name']
    assert all(exact_any_order(t) for t in terms), c['name']
    sq = (dist * dist).astype(f32)
    assert ref.seq_sum(dist) == math.fsum(float(x) for x in dist) and ref.seq_sum(sq) == math.fsum(float(x) for x in sq), c['name']
    assert exact_any_order(dist) and exact_any_order(sq), c['name']
    assert np.abs(dist.astype('f8') - thr).min() > 1e-5 * abs(thr), c['name']            # 1e-9 would do for the device; 1e-5 lets the float64 check of the restatement ask for equal flags
    Q = e['world'][e['kept']]; t2 = float(f32(float(f32(c['params']['EuclideanClusterTolerance'])) ** 2))
    for i0 in range(0, len(Q), 512):
        assert np.abs(ref.d2_rows(Q, i0, min(len(Q), i0 + 512)).astype('f8') - t2).min() > 1e-6 * t2, c['name']


_EXPECTED = {}


def cases():
    return _cases()


CASES = _cases()
NAMES = [c['name'] for c in CASES]


def expected(c):
    """the restatement's record of a case, computed once per process; the input conditions are asserted with it"""
    if c['name'] not in _EXPECTED:
        e = ref.detect_one(c['depth'], c['cam'], c['Twc'], c['obj'], c['params'])
        check_input_conditions(c, e)
        _EXPECTED[c['name']] = e
    return _EXPECTED[c['name']]


FIELDS_INT = ('found', 'class_id', 'crop_points', 'kept_points', 'components', 'clusters', 'best_cluster_size')
FIELDS_F32 = ('prob', 'centroid', 'size', 'best_similar1', 'best_similar2', 'best_roi')


def bits(x):
    return np.atleast_1d(np.asarray(x, f32)).view(np.uint32)


def assert_record(r, e, what):
    """record r (sgx_obj3d_result as a numpy record) == restatement dict e, bit for bit"""
    for k in FIELDS_INT: assert int(r[k]) == int(e[k]), (what, k, int(r[k]), int(e[k]))
    for k in FIELDS_F32: assert (bits(r[k]) == bits(e[k])).all(), (what, k, r[k], e[k])


def assert_same_records(a, b, what):
    """two sgx_obj3d_result records are the same bytes, larger_window_points included"""
    assert a.tobytes() == b.tobytes(), (what, a, b)


def run_case(lib, c, tap=None):
    """the single entry against the restatement; with a tap library also the kept flags and the labels"""
    from sg_slam_amd.detector3d import Detector3D
    e = expected(c)
    D = Detector3D(c['params'], c['W'], c['H'], c['cam'], lib=lib)
    r = D.detect_record(c['obj'], c['depth'], c['Twc'])
    assert_record(r, e, c['name'])
    if lib.has_taps if tap is None else tap:
        kept, lab = D.debug_read()
        assert len(kept) == e['crop_points'] and (kept == e['kept']).all() and (lab == e['labels']).all(), c['name']
    D.close()
    return r


def check_batch_equals_singles(lib, cs):
    """cases of one image size as ONE batch (an image per case, and every case twice) against the single entry"""
    from sg_slam_amd.detector3d import Detector3D, Detector3DBatch
    W, H = cs[0]['W'], cs[0]['H']
    assert all(c['W'] == W and c['H'] == H and c['params'] == cs[0]['params'] for c in cs)
    B = Detector3DBatch(cs[0]['params'], W, H, cs[0]['cam'], len(cs), 2 * len(cs), lib=lib)
    jobs = [(i, c['obj']) for i, c in enumerate(cs)] + [(i, c['obj']) for i, c in reversed(list(enumerate(cs)))]
    got = B.detect(np.stack([c['depth'] for c in cs]), np.stack([c['Twc'] for c in cs]), jobs)
    D = Detector3D(cs[0]['params'], W, H, cs[0]['cam'], lib=lib)
    for (i, o), g in zip(jobs, got):
        assert_same_records(g, D.detect_record(o, cs[i]['depth'], cs[i]['Twc']), cs[i]['name'])
    B.close(); D.close()
    return B, got


def batch_group():
    """the cases that share an image size and the default parameters (a batch has one parameter set)"""
    return [c for c in CASES if (c['W'], c['H']) == (128, 96) and c['params'] == PARAMS]


def full_size_batch():
    """640 x 480, TUM3's own parameters and intrinsics, three keyframes, five boxes: a box that is the whole (dense) image, whose crop of 384 x 288 cells is the
    largest Detector2D's clamp allows, a 384 x 288 box, a typical one, one at the image corner and one without valid points"""
    W, H = 640, 480
    d0 = scene(21, W, H, wall=(2.2, 0.0006, 0.0003), boxes=[(250, 160, 400, 330, 1.4, 0.0003), (60, 60, 110, 120, 1.0, 0.0)], noise=0.0005, outliers=40, holes=0.02)
    d1 = scene(22, W, H, wall=(1.8, -0.0004, 0.0002), boxes=[(300, 200, 380, 300, 1.1, 0.0)], noise=0.0005, nans=0.01, far=20)
    d1[:140, :200] = 0
    jobs = [(0, (9, 0.9, (128.0, 96.0, 384.0, 288.0))), (0, (5, 0.5, (20.0, 30.0, 120.0, 180.0))), (1, (20, 0.7, (256.0, 192.0, 384.0, 288.0))), (1, (11, 0.4, (0.0, 0.0, 180.0, 120.0)))]
    d2 = scene(23, W, H, wall=(2.4, 0.0005, -0.0003), boxes=[(200, 150, 330, 300, 1.5, 0.0002), (400, 180, 470, 330, 1.2, 0.0)], noise=0.0005, outliers=60)
    jobs.append((2, (15, 0.95, (0.0, 0.0, 640.0, 480.0))))
    return dict(W=W, H=H, cam=cam_for(W, H), depths=np.stack([d0, d1, d2]), Twcs=np.stack([pose(), pose((-0.1, 0.2, 0.05), (1.0, 0.5, -0.2)), pose((0.03, 0.02, -0.01), (-0.5, 0.1, 0.3))]),
                jobs=jobs, params=TUM3_PARAMS)
