"""Detector3D (semantic objects from detector boxes and depth): the numpy restatement (tests/obj3d_ref.py) against an independent statement with scipy's kd-tree and
connected components, then the kernel-logic emulator against the restatement bit for bit (record, diagnostics, and through the tap the kept flags and component
labels), the batch against single calls, ObjectDatabase::addObject, the settings reader and the argument errors."""
import ctypes as C
import os
import numpy as np
import pytest
import obj3d_cases as oc
import obj3d_ref as ref
from sg_slam_amd import settings
from sg_slam_amd.capi import Obj3dJob, OBJ3D_RESULT_DTYPE, SemanticObjectRecord, _vp
from sg_slam_amd.detector3d import Detector3D, Detector3DBatch, ObjectDatabase, SemanticObject, make_params, full_image_crop_points

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CASE = {c['name']: c for c in oc.CASES}


@pytest.mark.parametrize('name', oc.NAMES)
def test_restatement_against_kdtree_and_connected_components(name):
    """float64 k nearest neighbours and a radius graph from scipy on the same world points: the same kept flags and the same partition of the kept points (the
    independent distances are float64, the reference's float: they agree to 1e-6, and the cases keep every distance 1e-5 away from the threshold)"""
    from scipy.spatial import cKDTree
    from scipy.sparse import coo_matrix
    from scipy.sparse.csgraph import connected_components
    c = CASE[name]; e = oc.expected(c); p = c['params']; k = p['Sor_MeanK']
    if e['crop_points'] <= k:
        assert e['found'] == 0 and e['kept_points'] == 0
        return
    P = e['world'].astype('f8')
    dd, _ = cKDTree(P).query(P, k + 1)
    dist = dd[:, 1:].mean(1)
    n = len(P); thr = dist.mean() + p['Sor_StddevMulThresh'] * np.sqrt(((dist ** 2).sum() - dist.sum() ** 2 / n) / (n - 1))
    assert np.allclose(dist, e['dist'], rtol=2e-6, atol=0) and abs(thr - e['thr']) < 2e-6 * thr
    assert ((dist <= thr) == e['kept']).all()
    ki = np.nonzero(e['kept'])[0]; Q = P[ki]
    pairs = cKDTree(Q).query_pairs(float(np.float32(p['EuclideanClusterTolerance'])), output_type='ndarray')
    g = coo_matrix((np.ones(len(pairs)), (pairs[:, 0], pairs[:, 1])), shape=(len(Q), len(Q)))
    ncomp, lab = connected_components(g, directed=False)
    assert ncomp == e['components']
    first = np.full(ncomp, len(Q)); np.minimum.at(first, lab, np.arange(len(Q)))
    assert (ki[first[lab]] == e['labels'][ki]).all()


def test_cases_contain_what_they_are_for():
    E = {n: oc.expected(CASE[n]) for n in oc.NAMES}
    assert all(300 <= E[n]['crop_points'] <= 6000 for n in oc.NAMES if n != 'n_le_k')
    assert E['object_wall']['found'] == 1 and E['object_wall']['clusters'] >= 2 and E['object_wall']['components'] > E['object_wall']['clusters']
    assert E['object_wall']['kept_points'] < E['object_wall']['crop_points']
    d = CASE['holes_nan_range']['depth']; assert np.isnan(d).any() and (d == 0).any() and (d > 5).any()
    e = E['above_max']; sizes = np.unique(e['labels'][e['labels'] >= 0], return_counts=True)[1]
    assert e['found'] == 1 and sizes.max() > CASE['above_max']['params']['EuclideanClusterMaxSize'] > e['best_cluster_size']
    assert (sizes < 50).any()                                                           # components below min
    e = E['ratio_reject']; assert e['found'] == 0 and e['clusters'] == 2 and e['best_similar2'] > 0 and e['best_similar1'] * np.float32(0.5) < e['best_similar2']
    # the wall of object_wall touches the crop border
    c = CASE['object_wall']; x0, y0, cw, ch = ref.crop_cells(c['obj'][2], c['W'], c['H']); e = E['object_wall']
    big = e['labels'] == np.bincount(e['labels'][e['labels'] >= 0]).argmax()
    assert (e['j'][big] % c['W']).min() == x0 and (e['j'][big] // c['W']).max() == y0 + ch - 1
    # world-z quirk: two clusters survive, one is never compared (best_similar2 untouched), and it is the near object with the higher similarity in object_wall's pose
    e = E['world_z_quirk']; assert e['found'] == 1 and e['clusters'] == 2 and e['best_similar2'] == np.float32(-1)
    assert E['n_le_k']['crop_points'] <= 10 and E['n_le_k']['found'] == 0
    assert E['no_cluster']['components'] > 0 and E['no_cluster']['clusters'] == 0 and E['no_cluster']['found'] == 0
    e = E['equal_size']; sizes = np.unique(e['labels'][e['labels'] >= 0], return_counts=True)[1]
    assert list(sizes) == [196, 196] and e['clusters'] == 2
    assert (CASE['holes70']['depth'] == 0).mean() > 0.6


@pytest.mark.parametrize('name', oc.NAMES)
def test_emulator_equals_restatement(emu, name):
    r = oc.run_case(emu, CASE[name])
    if name == 'holes70': assert r['larger_window_points'] > 0                       # the first window cannot hold the neighbours
    if name == 'n_le_k': assert r['larger_window_points'] == 0


def test_emulator_batch_equals_singles(emu):
    group = oc.batch_group(); assert len(group) >= 2
    oc.check_batch_equals_singles(emu, group)


def test_object2d_tuples_of_detector2d_and_database(emu):
    """Detect() takes the (id, name, prob, rect) tuples of detector.Detector2D.detect and feeds mpObjectDatabase"""
    c = CASE['object_wall']; e = oc.expected(c)
    D = Detector3D(c['params'], c['W'], c['H'], c['cam'], lib=emu)
    o = (c['obj'][0], 'chair', c['obj'][1], c['obj'][2])
    got = D.Detect([o, o], c['depth'], c['Twc'])
    assert len(got) == 2 and isinstance(got[0], SemanticObject) and got[0].object_name == 'chair'
    assert (oc.bits(got[0].centroid) == oc.bits(e['centroid'])).all() and (oc.bits(got[0].size) == oc.bits(e['size'])).all()
    assert D.mpObjectDatabase.getDataBaseSize() == 1 and D.mpObjectDatabase.getObjectByID(1).class_id == 9      # the second one merged into the first
    assert D.DetectOne(CASE['n_le_k']['obj'], c['depth'] * 0, c['Twc']) is None
    D.close()


def test_object_database_against_restatement(emu):
    """first object, same name near (merged), same name far (appended), other name, and a seeded sequence"""
    db = ObjectDatabase(lib=emu); R = ref.ObjectDatabaseRef()
    seq = [(9, 0.8, (1.0, 0.5, 2.0), (0.5, 0.6, 0.7)), (9, 0.6, (1.3, 0.5, 2.2), (0.4, 0.5, 0.9)), (9, 0.7, (3.0, 0.5, 2.0), (0.5, 0.5, 0.5)), (5, 0.9, (1.0, 0.5, 2.0), (0.1, 0.1, 0.2)),
           (5, 0.5, (1.0, 0.65, 2.1), (0.1, 0.1, 0.2)), (5, 0.5, (1.0, 0.75, 2.2), (0.1, 0.1, 0.2)), (20, 0.5, (150.0, 0.0, 0.0), (1, 1, 1)), (20, 0.4, (150.1, 0.0, 0.0), (1, 1, 1))]
    rng = np.random.RandomState(3)
    seq += [(int(rng.choice([5, 9, 15, 20])), float(rng.uniform(0.2, 1)), tuple(rng.uniform(-1.5, 1.5, 3)), tuple(rng.uniform(0.1, 1, 3))) for _ in range(60)]
    for i, (cid, prob, cen, size) in enumerate(seq):
        s = SemanticObject(cid, prob, cen, size)
        assert db.addObject(s) == R.add(cid, prob, cen, size), i
    assert db.getDataBaseSize() == len(R.objs) > 8
    for g, o in zip(db.mvSemanticObject, R.objs):
        assert g.class_id == o['class_id'] and g.object_id == o['object_id'] and oc.bits(g.prob) == oc.bits(o['prob'])
        assert (oc.bits(g.centroid) == oc.bits(o['centroid'])).all() and (oc.bits(g.size) == oc.bits(o['size'])).all()
    assert emu.dll.sgx_objdb_add(db.h, C.byref(SemanticObjectRecord(21, 0, 0.5)), None, None) == -1      # mvSizes has 21 entries
    db.close()


def test_load_mapping_fixtures():
    t = settings.load_mapping(os.path.join(ROOT, 'tests', 'golden', 'settings_mapping', 'TUM3.yaml'))
    f = lambda v: float(np.float32(v))
    assert (t['Sor_MeanK'], t['Sor_StddevMulThresh'], t['EuclideanClusterTolerance'], t['EuclideanClusterMinSize'], t['EuclideanClusterMaxSize'], t['DetectSimilarCompareRatio'],
            t['camera_valid_depth_Min'], t['camera_valid_depth_Max']) == (50, 1.0, f(0.02), 1000, 30000, f(0.1), 0.5, 5.0)
    assert t['Voxel_LeafSize'] == f(0.01) and {k: t[k] for k in oc.TUM3_PARAMS if k not in ('EuclideanClusterTolerance', 'DetectSimilarCompareRatio', 'Voxel_LeafSize')} == \
        {k: v for k, v in oc.TUM3_PARAMS.items() if k not in ('EuclideanClusterTolerance', 'DetectSimilarCompareRatio', 'Voxel_LeafSize')}
    b = settings.load_mapping(os.path.join(ROOT, 'tests', 'golden', 'settings_mapping', 'Bonn.yaml'))
    assert b['DetectSimilarCompareRatio'] == 0.5 and b['Sor_MeanK'] == 50 and b['EuclideanClusterMinSize'] == 1000
    p = make_params(t); assert p.sor_mean_k == 50 and p.cluster_max_size == 30000 and p.sor_stddev_mul == 1.0
    # load() is unchanged and the tracking fixtures carry none of these keys
    with pytest.raises(KeyError): settings.load_mapping(os.path.join(ROOT, 'tests', 'golden', 'settings', 'TUM3.yaml'))


def test_argument_errors(emu):
    c = CASE['object_wall']
    h = C.c_void_p()
    assert emu.dll.sgx_obj3d_create(c['W'], c['H'], 1, 1, 100, C.byref(make_params(dict(c['params'], Sor_MeanK=0))), C.byref(h)) == -1      # mean_k < 1
    D = Detector3D(c['params'], c['W'], c['H'], c['cam'], lib=emu)
    out = np.zeros(1, OBJ3D_RESULT_DTYPE); T = np.ascontiguousarray(c['Twc'], 'f8'); cam = np.array(c['cam'], 'f4')
    for rect in ((-1.0, 0.0, 50.0, 50.0), (100.0, 10.0, 40.0, 40.0), (10.0, 60.0, 40.0, 40.0), (float('nan'), 0.0, 10.0, 10.0), (0.0, 0.0, -4.0, 10.0)):
        assert emu.dll.sgx_obj3d_detect(D.h, _vp(c['depth']), _vp(cam), _vp(T), C.byref(Obj3dJob(0, 9, 0.5, *rect)), _vp(out)) == -1, rect
        with pytest.raises(ValueError): ref.crop_cells(rect, c['W'], c['H'])
    assert emu.dll.sgx_obj3d_detect(D.h, _vp(c['depth']), _vp(cam), _vp(T), C.byref(Obj3dJob(1, 9, 0.5, 0.0, 0.0, 50.0, 50.0)), _vp(out)) == -1        # image index of a batch of one
    # the default capacity holds the largest crop there is: a box that is the whole image (Detector2D only clamps its boxes to the image)
    assert emu.dll.sgx_obj3d_detect(D.h, _vp(c['depth']), _vp(cam), _vp(T), C.byref(Obj3dJob(0, 9, 0.5, 0.0, 0.0, float(c['W']), float(c['H']))), _vp(out)) == 0
    x0, y0, cw, ch = ref.crop_cells((0.0, 0.0, float(c['W']), float(c['H'])), c['W'], c['H'])
    assert out[0]['crop_points'] == cw * ch == full_image_crop_points(c['W'], c['H'])
    h0 = C.c_void_p()
    assert emu.dll.sgx_obj3d_create(c['W'], c['H'], 1, 1, 0, C.byref(make_params(c['params'])), C.byref(h0)) == 0                 # 0 = that capacity, from the C ABI
    assert emu.dll.sgx_obj3d_detect(h0, _vp(c['depth']), _vp(cam), _vp(T), C.byref(Obj3dJob(0, 9, 0.5, 0.0, 0.0, float(c['W']), float(c['H']))), _vp(out)) == 0
    emu.dll.sgx_obj3d_destroy(h0)
    D.close()
    small = Detector3D(c['params'], c['W'], c['H'], c['cam'], lib=emu, max_crop_points=100)                                   # the crop does not fit
    assert emu.dll.sgx_obj3d_detect(small.h, _vp(c['depth']), _vp(cam), _vp(T), C.byref(Obj3dJob(0, 9, 0.5, *c['obj'][2])), _vp(out)) == -1
    small.close()
