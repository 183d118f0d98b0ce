"""PointCloudMapping's keyframe cloud: the numpy restatement (tests/cloud_ref.py) against independent statements (voxel membership by np.unique over integer cells
with float64 means, the outlier filter by scipy's kd-tree), then the kernel-logic emulator against the restatement bit for bit (points, colours, order, the record,
and through the tap the voxel cloud, the distances and the kept flags), the batch against single calls, the argument errors, the settings reader, camera_to_map_tf
and the PointCloudMapping class."""
import ctypes as C
import os
import numpy as np
import pytest
import cloud_cases as cc
import cloud_ref as ref
from sg_slam_amd import settings
from sg_slam_amd.capi import CloudParams, CLOUD_POINT_DTYPE, CLOUD_RESULT_DTYPE, _vp
from sg_slam_amd.pointcloudmapping import CloudBuilder, PointCloudMapping, PointCloudMappingBatch, make_cloud_params, camera_to_map_tf, pose_inverse

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FIXTURES = os.path.join(ROOT, 'tests', 'golden', 'settings_mapping')
f32 = np.float32


def test_cases_contain_what_they_are_for():
    cc.check_case_contents()


@pytest.mark.parametrize('name', cc.NAMES)
def test_restatement_voxels_against_unique_cells(name):
    """membership and counts: np.unique over the integer cell triples (no linear index, no sort of pairs, no runs); means in float64.  A float running sum of n
    terms of one sign is within n * 2^-24 (relative) of the exact sum, so the float64 mean is asked to 1e-5 of the cloud's extent for voxels of up to 160 points and
    to n * 2^-24 beyond; a colour channel is the floor of the mean up to the rounding of one float division"""
    c = cc.CASE[name]; e = cc.expected(c)
    if e['flags'] == ref.LEAF_TOO_SMALL:
        P = e['cloud']; assert np.prod(((P.max(0) - P.min(0)) / f32(c['params']['leaf'])).astype('f8') + 1) > 2 ** 31
        return
    P = e['cloud']; inv = f32(1) / f32(c['params']['leaf'])
    cells = np.floor((P * inv).astype(f32)).astype(np.int64)[:, ::-1]                      # (k, j, i): np.unique sorts rows lexicographically = ascending idx
    u, inverse, counts = np.unique(cells, axis=0, return_inverse=True, return_counts=True); inverse = inverse.reshape(-1)
    assert len(u) == e['n_voxels'] and (counts == [len(m) for m in e['members']]).all()
    for v in (0, len(u) // 2, len(u) - 1): assert (np.nonzero(inverse == v)[0] == e['members'][v]).all()
    mean = np.zeros((len(u), 3)); np.add.at(mean, inverse, P.astype('f8')); mean /= counts[:, None]
    scale = np.abs(P).max()
    tol = np.maximum(1e-5, counts * 2.0 ** -24)[:, None] * scale
    assert (np.abs(e['voxels'] - mean) <= tol).all()
    ch = np.stack([(e['cloud_rgba'] >> s) & 255 for s in (16, 8, 0, 24)], 1).astype(np.int64)
    tot = np.zeros((len(u), 4), np.int64); np.add.at(tot, inverse, ch)
    got = np.stack([(e['voxel_rgba'] >> s) & 255 for s in (16, 8, 0, 24)], 1).astype(np.int64)
    assert (np.abs(got - tot // counts[:, None]) <= 1).all() and (got == tot // counts[:, None]).mean() > 0.99 and (got[:, 3] == 255).all()


@pytest.mark.parametrize('name', cc.NAMES)
def test_restatement_filter_against_kdtree(name):
    """float64 k nearest neighbours from scipy on the restatement's voxel cloud: the same distances to 2e-6 and the same kept flags (the cases keep every distance
    1e-5 away from the threshold)"""
    from scipy.spatial import cKDTree
    c = cc.CASE[name]; e = cc.expected(c); p = c['params']; k = p['mean_k']
    if e['flags']:
        assert e['n_points'] == 0 and (e['n_voxels'] <= k or e['flags'] == ref.LEAF_TOO_SMALL)
        return
    V = e['voxels'].astype('f8'); n = len(V)
    dd, _ = cKDTree(V).query(V, k + 1)
    dist = dd[:, 1:].mean(1)
    thr = dist.mean() + p['stddev_mul'] * np.sqrt(((dist ** 2).sum() - dist.sum() ** 2 / n) / (n - 1))
    assert np.allclose(dist, e['dist'], rtol=2e-6, atol=0) and abs(thr - e['thr']) < 2e-6 * thr and abs(dist.mean() - e['mean']) < 2e-6 * e['mean']
    assert ((dist <= thr) == e['kept']).all() and e['n_points'] == int(e['kept'].sum())
    Q = e['voxels'][e['kept']]
    want = ref.ros_axes(Q) if c['mode'] == ref.LOCAL else Q
    assert (cc.bits(e['points']) == cc.bits(want)).all() and not (cc.bits(e['points']) == 0x80000000).any()


@pytest.mark.parametrize('name', cc.NAMES)
def test_emulator_equals_restatement(emu, name):
    r = cc.run_case(emu, cc.CASE[name])
    if name == 'far_speck': assert r['larger_window_points'] > 0                       # the speck's neighbours are not in its first window
    if name in ('all_invalid', 'few_points', 'leaf_too_small'): assert r['larger_window_points'] == 0 and r['n_points'] == 0


def test_emulator_dynamic_branches(emu):
    """the rects with the keyframe's flag, without it (the reference's else branch) and with consider_dynamic off"""
    c = cc.CASE['dynamic_boxes']
    a = cc.run_case(emu, c); b = cc.run_case(emu, cc.variant(c, have_dynamic=0)); n = cc.run_case(emu, cc.variant(c, p_consider_dynamic=0))
    assert a['n_pixels_used'] < b['n_pixels_used'] == n['n_pixels_used'] == c['W'] * c['H'] and b.tobytes() == n.tobytes()


def test_emulator_batch_equals_singles(emu):
    group = cc.batch_group(); assert len(group) >= 4
    got = cc.check_batch_equals_singles(emu, group)
    assert len({int(r['n_points']) for _, r in got}) >= 3
    cc.check_batch_equals_singles(emu, [cc.CASE['world_plain'], cc.variant(cc.CASE['world_plain'], Twc=cc.pose((0.2, 0.1, -0.3), (-0.4, 0.2, 0.1)))])


def test_argument_errors(emu):
    c = cc.CASE['dynamic_boxes']; W, H = c['W'], c['H']
    h = C.c_void_p()
    create = lambda mode=0, boxes=4, images=1, w=W, hh=H, **pp: emu.dll.sgx_cloud_create(w, hh, images, boxes, mode, C.byref(make_cloud_params(dict(c['params'], **pp))), C.byref(h))
    for bad in (dict(mean_k=0), dict(leaf=0.0), dict(leaf=-0.01), dict(leaf=float('nan')), dict(leaf=float('inf')), dict(depth_min=float('nan')), dict(depth_max=float('inf'))):
        assert create(**bad) == -1 and not h.value, bad
        with pytest.raises(ValueError): ref.build(c['depth'], c['color'], c['cam'], c['Twc'], (), 0, dict(c['params'], **bad), ref.LOCAL)
    assert create(mode=2) == -1 and create(boxes=129) == -1 and create(boxes=-1) == -1 and create(images=0) == -1 and create(w=2048, hh=1024) == -1 and not h.value
    assert emu.dll.sgx_cloud_create(W, H, 1, 4, 0, None, C.byref(h)) == -1
    pts = np.zeros(W * H, CLOUD_POINT_DTYPE); rec = np.zeros(1, CLOUD_RESULT_DTYPE); cam = np.array(c['cam'], 'f4'); T = np.eye(4).reshape(16)
    boxes = np.zeros((5, 4), 'f4')
    B = CloudBuilder(c['params'], W, H, c['cam'], ref.WORLD, max_boxes=4, lib=emu)
    build = lambda twc, nb, cap=W * H: emu.dll.sgx_cloud_build(B.h, _vp(c['depth']), _vp(c['color']), _vp(cam), _vp(twc), _vp(boxes), nb, 1, _vp(pts), cap, _vp(rec))
    assert build(T, 4) == 0 and rec[0]['n_points'] > 0
    assert build(T, 5) == -1 and build(T, -1) == -1                                     # more rects than max_boxes
    Tn = T.copy(); Tn[6] = np.nan
    assert build(Tn, 0) == -1 and build(None, 0) == -1                                  # a NaN in Twc; WORLD mode without Twc
    with pytest.raises(ValueError): ref.build(c['depth'], c['color'], c['cam'], Tn.reshape(4, 4), (), 0, c['params'], ref.WORLD)
    assert build(T, 0, cap=3) == emu.dll.sgx_cloud_build(B.h, _vp(c['depth']), _vp(c['color']), _vp(cam), _vp(T), None, 0, 0, _vp(pts), 3, _vp(rec)) != 0 and rec[0]['n_points'] > 3      # overflow: the record is written
    res = np.zeros(2, CLOUD_RESULT_DTYPE)
    args = lambda n, dp=W, cp=3 * W: (B.h, _vp(c['depth']), dp, _vp(c['color']), cp, n, _vp(cam), _vp(T), None, None, None, _vp(pts), _vp(res), None)
    assert emu.dll.sgx_cloud_build_batch_dev(*args(1)) == 0
    assert emu.dll.sgx_cloud_build_batch_dev(*args(2)) == -1 and emu.dll.sgx_cloud_build_batch_dev(*args(0)) == -1                 # max_images is 1
    assert emu.dll.sgx_cloud_build_batch_dev(*args(1, dp=W - 1)) == -1 and emu.dll.sgx_cloud_build_batch_dev(*args(1, cp=3 * W - 1)) == -1
    B.close()
    # the device entry reads nothing back: it takes at most max_boxes rects
    L = PointCloudMappingBatch(c['params'], W, H, c['cam'], 1, ref.LOCAL, max_boxes=2, lib=emu)
    bx = np.array([list(c['boxes'][0]), list(c['boxes'][1])], 'f4')[None]
    nb = np.array([7], 'i4'); hv = np.array([1], 'i4'); d = c['depth'][None].copy(); col = c['color'][None].copy()
    L.n = 1
    assert emu.dll.sgx_cloud_build_batch_dev(L.h, _vp(d), W, _vp(col), 3 * W, 1, _vp(cam), None, _vp(bx), _vp(nb), _vp(hv), _vp(L.points), _vp(L.results), None) == 0
    (p, r), = L.read()
    cc.assert_cloud(p, r, cc.expected(c), 'n_boxes clamped')
    L.close()


def test_load_pointcloud_mapping_fixtures():
    t = settings.load_pointcloud_mapping(os.path.join(FIXTURES, 'TUM3.yaml')); f = lambda v: float(f32(v))
    assert t == dict(is_map_construction_consider_dynamic=1, is_octo_semantic_map_construction=1, is_global_pc_reconstruction=0, camera_valid_depth_Min=0.5, camera_valid_depth_Max=5.0,
                     Sor_Local_MeanK=50, Sor_Local_StddevMulThresh=3.0, Voxel_Local_LeafSize=f(0.01), Sor_Global_MeanK=50, Sor_Global_StddevMulThresh=3.0, Voxel_Global_LeafSize=f(0.01))
    b = settings.load_pointcloud_mapping(os.path.join(FIXTURES, 'Bonn.yaml'))
    assert (b['is_octo_semantic_map_construction'], b['is_global_pc_reconstruction'], b['Sor_Local_StddevMulThresh'], b['Sor_Global_StddevMulThresh']) == (0, 1, 2.0, 2.0)
    p = make_cloud_params(t); assert (p.sor_mean_k, p.sor_stddev_mul, p.consider_dynamic, p.camera_valid_depth_max) == (50, 3.0, 1, 5.0) and p.voxel_leaf_size == f32(0.01)
    g = make_cloud_params(b, ref.WORLD); assert (g.sor_mean_k, g.sor_stddev_mul) == (50, 2.0)
    assert {k: cc.TUM3_PARAMS[k] for k in ('mean_k', 'stddev_mul', 'consider_dynamic')} == dict(mean_k=p.sor_mean_k, stddev_mul=p.sor_stddev_mul, consider_dynamic=p.consider_dynamic)
    assert settings.load_mapping(os.path.join(FIXTURES, 'TUM3.yaml'))['Sor_MeanK'] == 50                                      # load_mapping is unchanged
    with pytest.raises(KeyError): settings.load_pointcloud_mapping(os.path.join(ROOT, 'tests', 'golden', 'settings', 'TUM3.yaml'))     # the tracking fixtures carry none of these keys


def test_camera_to_map_tf(emu):
    """against a float64 rotation-to-quaternion (scipy) of the same float pose, to 1e-6, over the trace branch and the three largest-diagonal branches"""
    from scipy.spatial.transform import Rotation
    rvs = [(0.05, -0.1, 0.03), (0.0, 0.0, 0.0), (3.1, 0.02, 0.01), (0.02, 3.1, -0.01), (0.01, -0.02, 3.1), (2.0, 1.5, -1.0), (-1.2, 2.2, 0.4)]
    branches = set()
    for i, rv in enumerate(rvs):
        Tcw = np.eye(4, dtype='f4'); Tcw[:3, :3] = cc.pose(rv)[:3, :3]; Tcw[:3, 3] = (0.3 * i - 1, 0.2, -0.5 + 0.1 * i)
        o, q = camera_to_map_tf(Tcw, lib=emu)
        ro, rq = ref.camera_to_map_tf(Tcw)
        assert (o == ro).all() and (q == rq).all()
        R = Tcw[:3, :3].astype('f8').T; t = -R @ Tcw[:3, 3].astype('f8')
        Q = Rotation.from_matrix(R).as_quat()                                                  # x, y, z, w
        want = np.array([Q[2], -Q[0], -Q[1], Q[3]])
        assert min(np.abs(q - want).max(), np.abs(q + want).max()) < 1e-6 and np.abs(o - [t[2], -t[0], -t[1]]).max() < 1e-6
        d = np.diag(R); branches.add('trace' if np.trace(R) > 0 else int(np.argmax(d)))
    assert branches == {'trace', 0, 1, 2}
    assert emu.dll.sgx_cloud_camera_to_map_tf(None, _vp(np.zeros(3)), _vp(np.zeros(4))) == -1


def test_pointcloudmapping_class(emu):
    """insertKeyFrame: the local cloud in ROS axes and the transform; with is_octo_semantic_map_construction and objects, Detector3D fills the object database"""
    import obj3d_cases as oc
    o = {c['name']: c for c in oc.CASES}['object_wall']; W, H = o['W'], o['H']
    mp = dict(is_map_construction_consider_dynamic=1, is_octo_semantic_map_construction=1, is_global_pc_reconstruction=1, camera_valid_depth_Min=0.5, camera_valid_depth_Max=5.0,
              Sor_Local_MeanK=8, Sor_Local_StddevMulThresh=1.0, Voxel_Local_LeafSize=0.05, Sor_Global_MeanK=8, Sor_Global_StddevMulThresh=1.5, Voxel_Global_LeafSize=0.04)
    Tcw = np.linalg.inv(o['Twc']).astype('f4'); color = cc.colors(77, W, H)
    boxes = [(70.5, 20.25, 30.0, 40.5)]
    M = PointCloudMapping(mp, W, H, o['cam'], detector3d_params=o['params'], lib=emu)
    obj = (o['obj'][0], 'chair', o['obj'][1], o['obj'][2])
    pts, (origin, rot) = M.insertKeyFrame(color, o['depth'], Tcw, [obj], boxes, True)
    Twc = pose_inverse(Tcw)
    e = ref.build(o['depth'], color, o['cam'], None, boxes, 1, dict(mean_k=8, stddev_mul=1.0, leaf=0.05, consider_dynamic=1, depth_min=0.5, depth_max=5.0), ref.LOCAL)
    cc.assert_cloud(pts, M.last_record, e, 'localMap')
    g = ref.build(o['depth'], color, o['cam'], Twc, boxes, 1, dict(mean_k=8, stddev_mul=1.5, leaf=0.04, consider_dynamic=1, depth_min=0.5, depth_max=5.0), ref.WORLD)
    cc.assert_cloud(M.temp_globalMap, M.last_world_record, g, 'temp_globalMap')
    ro, rq = ref.camera_to_map_tf(Tcw); assert (origin == ro).all() and (rot == rq).all()
    assert M.mpDetector3D.mpObjectDatabase.getDataBaseSize() == 1 and M.mpDetector3D.mpObjectDatabase.getObjectByID(1).class_id == o['obj'][0]
    M.insertKeyFrame(color, o['depth'], Tcw, [], boxes, False)
    assert M.last_record['n_pixels_used'] > e['n_pixels_used'] and M.mpDetector3D.mpObjectDatabase.getDataBaseSize() == 1
    M.close()
    M0 = PointCloudMapping(dict(mp, is_octo_semantic_map_construction=0, is_global_pc_reconstruction=0), W, H, o['cam'], detector3d_params=o['params'], lib=emu)
    assert M0.mpDetector3D is None and M0.world is None
    M0.close()
