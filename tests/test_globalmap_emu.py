"""The global map (sgx_globalmap_*) on the kernel-logic emulator against the restatement (tests/globalmap_ref.py) bit for bit: points, colours, order,
records and taps after every operation of every case of tests/globalmap_cases.py; the schedule of PointcloudMapping.cc:332-360 through PointCloudMapping.update_global
against the literal loop; append_batch_dev fed from a WORLD-mode PointCloudMappingBatch; the argument errors; the settings reader."""
import ctypes as C
import os
import numpy as np
import pytest
import cloud_cases as cc
import cloud_ref
import globalmap_cases as gc
import globalmap_ref as ref
from sg_slam_amd import settings
from sg_slam_amd.capi import GlobalMapParams, CLOUD_POINT_DTYPE, GMAP_APPEND_DTYPE, GMAP_RESULT_DTYPE, SGX_GMAP_MAX_POINTS, _vp
from sg_slam_amd.globalmap import GlobalMap, GlobalMapSchedule, make_globalmap_params
from sg_slam_amd.pointcloudmapping import PointCloudMapping, PointCloudMappingBatch, pose_inverse

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FIXTURES = os.path.join(ROOT, 'tests', 'golden', 'settings_mapping')
f32 = np.float32


def test_cases_contain_what_they_are_for():
    gc.check_case_contents()


@pytest.mark.parametrize('name', gc.NAMES)
def test_emulator_equals_restatement(emu, name):
    recs, tap = gc.run_case(emu, gc.CASE[name])
    assert recs is not None and tap is not None                      # the emulator has the taps: no case is left out
    gc.check_case_figures(name, recs, tap)


def test_max_radius_changes_no_result(emu):
    """the whole-cloud case with the tiers as built and with every not-proven point sent straight to the whole-cloud scan: the same bits"""
    a, ta = gc.run_case(emu, gc.CASE['specks']); b, tb = gc.run_case(emu, gc.CASE['specks_whole'])
    for k in ('n_points_in', 'n_voxels', 'n_points', 'flags', 'mean', 'thr', 'wider_window_points'): assert a[-1][k] == b[-1][k], k
    assert all(x.tobytes() == y.tobytes() for x, y in zip(ta[:3], tb[:3])) and a[-1]['whole_cloud_points'] < b[-1]['whole_cloud_points']


def _records(points):
    p = np.zeros(len(points[0]), CLOUD_POINT_DTYPE); p['x'], p['y'], p['z'] = points[0][:, 0], points[0][:, 1], points[0][:, 2]; p['rgba'] = points[1]
    return p


def test_append_batch_capacity_in_one_call(emu):
    """the capacity case as ONE batch with a stride and a count stride: the refused cloud in the middle, the later one accepted, as the single calls"""
    c = gc.CASE['capacity']; E = gc.expected(c); clouds = [_records(op[1:]) for op in c['ops'][:3]]
    stride = 700; pts = np.zeros(3 * stride, CLOUD_POINT_DTYPE); cnt = np.zeros((3, 5), 'i4')
    for i, p in enumerate(clouds): pts[i * stride:i * stride + len(p)] = p; cnt[i, 2] = len(p)
    M = GlobalMap(c['params'], c['cap'], lib=emu)
    r = M.read_records(M.append_dev(pts, stride, cnt, 20, 3, n_points_offset_bytes=8))
    assert [{k: int(x[k]) for k in x.dtype.names} for x in r] == [e[0] for e in E[:3]]
    gc.assert_map(M.points(), E[2][1], E[2][2], 'capacity as a batch')
    M.reset(); assert M.size() == 0 and len(M.points()) == 0
    neg = np.array([-5], 'i4')
    r = M.read_records(M.append_dev(pts, 0, neg, 0, 1)); assert (int(r[0]['n_in']), int(r[0]['offset']), int(r[0]['map_size']), int(r[0]['flags'])) == (0, 0, 0, 0)
    M.close()


def test_argument_errors(emu):
    h = C.c_void_p(1)
    create = lambda n=100, **pp: emu.dll.sgx_globalmap_create(n, C.byref(make_globalmap_params(dict(gc.PARAMS, **pp))), C.byref(h))
    for bad in (dict(mean_k=0), dict(leaf=0.0), dict(leaf=-0.01), dict(leaf=float('nan')), dict(leaf=float('inf')), dict(stddev_mul=float('nan'))):
        h.value = 1
        assert create(**bad) == -1 and not h.value, bad
        with pytest.raises(ValueError): ref.GlobalMap(dict(gc.PARAMS, **bad), 100)
    h.value = 1; assert create(0) == -1 and not h.value
    h.value = 1; assert create(SGX_GMAP_MAX_POINTS + 1) == -1 and not h.value
    with pytest.raises(ValueError): ref.GlobalMap(gc.PARAMS, SGX_GMAP_MAX_POINTS + 1)
    assert emu.dll.sgx_globalmap_create(100, None, C.byref(h)) == -1 and emu.dll.sgx_globalmap_create(100, C.byref(make_globalmap_params(gc.PARAMS)), None) == -1
    M = GlobalMap(gc.PARAMS, 100, lib=emu); d = emu.dll
    p = np.zeros(10, CLOUD_POINT_DTYPE); rec = np.zeros(1, GMAP_APPEND_DTYPE); res = np.zeros(1, GMAP_RESULT_DTYPE); n = np.zeros(1, 'i4')
    assert d.sgx_globalmap_append(M.h, None, 3, _vp(rec)) == -1 and d.sgx_globalmap_append(M.h, _vp(p), -1, _vp(rec)) == -1 and d.sgx_globalmap_append(M.h, _vp(p), 3, None) == -1
    assert d.sgx_globalmap_append(None, _vp(p), 3, _vp(rec)) == -1 and d.sgx_globalmap_consolidate(M.h, None) == -1 and d.sgx_globalmap_consolidate_dev(M.h, None, None) == -1
    args = lambda ps=0, ns=0, k=1: (M.h, _vp(p), ps, _vp(n), ns, k, _vp(rec), None)
    assert d.sgx_globalmap_append_batch_dev(*args()) == 0
    for bad in (dict(ps=-1), dict(ns=-4), dict(ns=6), dict(k=0), dict(k=65536)): assert d.sgx_globalmap_append_batch_dev(*args(**bad)) == -1, bad
    assert d.sgx_globalmap_size(M.h, None) == -1 and d.sgx_globalmap_read(M.h, None, 4, _vp(n)) == -1 and d.sgx_globalmap_read(M.h, _vp(p), -1, _vp(n)) == -1
    assert d.sgx_globalmap_points_dev(M.h, None, None) == -1 and d.sgx_globalmap_reset(None) == -1
    assert d.sgx_globalmap_append(M.h, _vp(p), 10, _vp(rec)) == 0 and d.sgx_globalmap_read(M.h, _vp(p), 4, _vp(n)) != 0 and n[0] == 10       # overflow: the size is written
    assert d.sgx_globalmap_debug_max_radius(M.h, 17) == -1 and d.sgx_globalmap_debug_max_radius(M.h, -1) == -1 and d.sgx_globalmap_debug_max_radius(M.h, 16) == 0
    big = np.zeros(101, CLOUD_POINT_DTYPE)
    assert d.sgx_globalmap_append(M.h, _vp(big), 101, _vp(rec)) == 0 and rec[0]['flags'] == ref.FULL and M.size() == 10          # a cloud beyond the capacity is a refusal, not an error
    M.close()


def _keyframes():
    """four 64 x 48 keyframes of one wall under four poses, and PointCloudMapping's parameters with the global cloud switched on"""
    W, H = 64, 48
    mp = dict(is_map_construction_consider_dynamic=1, is_octo_semantic_map_construction=0, is_global_pc_reconstruction=1, camera_valid_depth_Min=0.5, camera_valid_depth_Max=5.0,
              Sor_Local_MeanK=8, Sor_Local_StddevMulThresh=1.0, Voxel_Local_LeafSize=0.05, Sor_Global_MeanK=8, Sor_Global_StddevMulThresh=1.5, Voxel_Global_LeafSize=0.04)
    depths = [cc.scene(50 + i, W, H, wall=(1.4 + 0.05 * i, 0.004, 0.002), outliers=3) for i in range(4)]
    Tcws = [np.linalg.inv(cc.pose((0.02 * i, -0.05 * i, 0.01), (0.1 * i, -0.05, 0.02 * i))).astype('f4') for i in range(4)]
    return W, H, mp, depths, [cc.colors(60 + i, W, H) for i in range(4)], Tcws


def test_update_global_equals_the_literal_loop(emu):
    """insertKeyFrame + update_global over a pending pattern with threshold 2 against the loop of :332-360 on the restatement.  The pattern: two keyframes that are
    invalid throughout while none is pending (an empty cloud is published and count is NOT reset), then pending until count > 2 forces a consolidation, then not
    pending"""
    W, H, mp, depths, colors, Tcws = _keyframes(); cam = cc.cam_for(W, H)
    gp = dict(mean_k=8, stddev_mul=1.5, leaf=0.04, consider_dynamic=1, depth_min=0.5, depth_max=5.0)
    frames = [(np.zeros((H, W), f32), colors[0], Tcws[0])] * 2 + [(depths[i % 4], colors[i % 4], Tcws[i % 4]) for i in range(6)]
    pending = [False, False, True, True, True, True, True, False]
    M = PointCloudMapping(mp, W, H, cam, lib=emu, global_map=dict(mp, global_pc_update_kf_threshold=2), global_map_max_points=1 << 14)
    assert M.global_schedule.threshold == 2
    clouds = []; got = []; counts = []
    for (d, c, T), pend in zip(frames, pending):
        M.insertKeyFrame(c, d, T)
        e = cloud_ref.build(d, c, cam, pose_inverse(T), (), 0, gp, cloud_ref.WORLD)
        cc.assert_cloud(M.temp_globalMap, M.last_world_record, e, 'temp_globalMap')
        clouds.append((e['points'], e['rgba']))
        got.append(M.update_global(pend)); counts.append(M.global_schedule.count)
    want, wcounts = ref.schedule(ref.GlobalMap(dict(mean_k=8, stddev_mul=1.5, leaf=0.04), 1 << 14), clouds, pending, 2)
    assert counts == wcounts == [1, 2, 3, 1, 2, 3, 1, 1]
    assert [g is not None for g in got] == [w is not None for w in want] == [True, True, False, True, False, False, True, True]
    assert len(got[0]) == 0 and len(got[1]) == 0 and len(got[3]) > 100                          # empty publications, then a forced one
    for g, w in zip(got, want):
        if g is not None: gc.assert_map(g, w[0], w[1], 'published')
    M.close()
    M0 = PointCloudMapping(dict(mp, is_global_pc_reconstruction=0), W, H, cam, lib=emu)
    assert M0.globalMap is None and M0.update_global(False) is None
    M0.close()


def test_append_batch_dev_from_a_world_batch(emu):
    """depth image -> world cloud -> global map without a copy: the counts are read from the batch's result records"""
    W, H, mp, depths, colors, Tcws = _keyframes(); cam = cc.cam_for(W, H)
    gp = dict(mean_k=8, stddev_mul=1.5, leaf=0.04, consider_dynamic=1, depth_min=0.5, depth_max=5.0)
    B = PointCloudMappingBatch(gp, W, H, cam, 4, cloud_ref.WORLD, max_boxes=4, lib=emu)
    B.launch(np.stack(depths), np.stack(colors), np.stack([pose_inverse(T) for T in Tcws]))
    G = GlobalMap(mp, 1 << 14, lib=emu)
    r = G.read_records(G.append_batch_dev(B))
    host = B.read()
    S = GlobalMap(mp, 1 << 14, lib=emu)
    for i, (p, rec) in enumerate(host):
        a = S.append(p)
        assert a.tobytes() == r[i].tobytes() and int(a['n_in']) == int(rec['n_points']) > 100
    assert G.points().tobytes() == S.points().tobytes() and G.size() == sum(len(p) for p, _ in host)
    G.launch(); rg = G.read(); rs = S.consolidate()
    assert rg.tobytes() == rs.tobytes() and rg['flags'] == 0 and G.points().tobytes() == S.points().tobytes()
    L = PointCloudMappingBatch(gp, W, H, cam, 1, cloud_ref.LOCAL, max_boxes=4, lib=emu)
    with pytest.raises(ValueError): G.append_batch_dev(L)
    pd, nd = G.points_dev(); assert pd and nd
    for o in (B, G, S, L): o.close()


def test_load_global_map_fixtures():
    want = dict(TUM1=(2.0, 25), TUM2=(2.0, 25), TUM3=(3.0, 25), Bonn=(2.0, 25), astra_pro_camera=(2.0, 30))
    assert sorted(f[:-5] for f in os.listdir(FIXTURES)) == sorted(want)
    for name, (mul, thr) in want.items():
        g = settings.load_global_map(os.path.join(FIXTURES, name + '.yaml'))
        assert g == dict(Voxel_Global_LeafSize=float(f32(0.01)), Sor_Global_MeanK=50, Sor_Global_StddevMulThresh=mul, global_pc_update_kf_threshold=thr), name
        p = make_globalmap_params(g); assert (p.sor_mean_k, p.sor_stddev_mul) == (50, mul) and p.voxel_leaf_size == f32(0.01)
    t = settings.load_pointcloud_mapping(os.path.join(FIXTURES, 'TUM3.yaml')); assert 'global_pc_update_kf_threshold' not in t and len(t) == 11      # that dict stays as it is
    with pytest.raises(KeyError): settings.load_global_map(os.path.join(ROOT, 'tests', 'golden', 'settings', 'TUM3.yaml'))
