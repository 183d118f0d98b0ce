"""The occupancy map on the MI355X: the product library against the restatement (tests/octomap_ref.py) on every case of tests/octomap_cases.py bit for bit, a batch
against single calls, two runs byte for byte, the capacity case, the chain cloud -> map on a side stream, one full-size run (three 640 x 480 keyframes, 3 cm cells,
the launch file's z windows) against the emulator, and the C++ mirror class."""
import os
import subprocess
import numpy as np
import pytest
import octomap_cases as oc
import octomap_ref as ref
from sg_slam_amd.octomapserver import OctomapServer, sensor_to_world

pytestmark = pytest.mark.gpu
LAUNCH = dict(res=0.03, max_range=-1.0, occupancy_min_z=-1.5, occupancy_max_z=1.5, pointcloud_min_z=-5.0, pointcloud_max_z=5.0)      # the values of the reference's launch file


@pytest.mark.parametrize('name', oc.NAMES)
def test_device_equals_restatement(gpulib, name):
    oc.run_case(gpulib, oc.CASE[name])


def test_device_batch_equals_singles(gpulib):
    for name in ('generated_walk', 'out_of_key_range', 'clamps'):
        c = oc.CASE[name]; e = oc.expected(name)
        recs, S = oc.run_batch(gpulib, c)
        for i, st in enumerate(e['steps']): oc.assert_record(recs[i], st['record'], (name, i))
        oc.assert_state(S, e['steps'][-1], name); S.close()


def test_two_runs_are_byte_identical(gpulib):
    """records, cells, grid: nothing depends on the order in which the atomics of a run arrive, nor on the table's layout (the second map is larger)"""
    c = oc.CASE['generated_walk']
    ra, A = oc.run_batch(gpulib, c); a = oc.snapshot(A)
    rb, B = oc.run_batch(gpulib, c, OctomapServer(c['params'], 1 << 15, c['max_points'], lib=gpulib)); b = oc.snapshot(B)
    A.reset(); rc, _ = oc.run_batch(gpulib, c, A); cc_ = oc.snapshot(A)
    assert ra.tobytes() == rb.tobytes() == rc.tobytes() and a == b == cc_
    A.close(); B.close()


def test_capacity(gpulib):
    """max_bricks too small, and more distinct bricks than the table has slots: the flag, the map unchanged as every query sees it, the next scan applied; too many points alike"""
    for name in ('map_full', 'table_full', 'too_many_points'):
        c = oc.CASE[name]; e = oc.expected(name)
        recs, S = oc.run_batch(gpulib, c)
        for i, st in enumerate(e['steps']): oc.assert_record(recs[i], st['record'], (name, i))
        oc.assert_state(S, e['steps'][-1], name); S.close()


def _chain(lib, F, stream=None):
    from sg_slam_amd.pointcloudmapping import PointCloudMappingBatch, camera_to_map_tf
    import cloud_ref
    n = len(F['depths'])
    B = PointCloudMappingBatch(F['params'], F['W'], F['H'], F['cam'], n, cloud_ref.LOCAL, max_boxes=4, lib=lib)
    mats = []
    for i in range(n):
        o, q = camera_to_map_tf(np.linalg.inv(F['Twcs'][i]).astype('f4'), lib=lib); mats.append(sensor_to_world(o, q, lib=lib))
    S = OctomapServer(F['octo'], max_bricks=F['max_bricks'], max_points_per_scan=B.N, lib=lib)
    if stream is None:
        B.launch(F['depths'], F['colors'], None, F['boxes'], F['have_dynamic']); recs = S.insert_clouds(B, np.array(mats))
    else:
        import torch
        with torch.cuda.stream(stream):
            B.launch(F['depths'], F['colors'], None, F['boxes'], F['have_dynamic']); recs = S.insert_clouds(B, np.array(mats)); snap = oc.snapshot(S)
        stream.synchronize()
        S.close(); B.close()
        return recs, snap
    snap = oc.snapshot(S); S.close(); B.close()
    return recs, snap


def test_chain_cloud_to_map_on_a_side_stream(gpulib, emu):
    """sgx_cloud_build_batch_dev -> sgx_octomap_insert_batch_dev on a non-default stream, the map reading the cloud handle's buffers: the emulator's bytes"""
    import torch
    import cloud_cases as cc
    cs = cc.batch_group()[:3]
    F = dict(W=cs[0]['W'], H=cs[0]['H'], cam=cs[0]['cam'], params=cs[0]['params'], depths=np.stack([c['depth'] for c in cs]), colors=np.stack([c['color'] for c in cs]),
             boxes=[c['boxes'] for c in cs], have_dynamic=[c['have_dynamic'] for c in cs], Twcs=[cc.pose((0.1 * i, 0.05, -0.1 * i), (0.05 * i, -0.1 * i, 0.02)) for i in range(3)],
             octo=ref.params(res=0.05, max_range=4.0, occupancy_min_z=-1.0, occupancy_max_z=2.0), max_bricks=8192)
    want = _chain(emu, F); got = _chain(gpulib, F, torch.cuda.Stream())
    assert want[0]['n_passed'].sum() > 300 and got[0].tobytes() == want[0].tobytes() and got[1] == want[1]


def test_full_size_run_equals_emulator(gpulib, emu):
    """three 640 x 480 keyframes of about 40 000 points, 3 cm cells, three poses"""
    import cloud_cases as cc
    F = dict(cc.tum3_full()); F['octo'] = ref.params(**LAUNCH); F['max_bricks'] = 1 << 15
    want = _chain(emu, F); got = _chain(gpulib, F)
    assert (want[0]['n_passed'] > 20000).all() and (want[0]['flags'] == 0).all() and (want[0]['n_free_updates'] > 40000).all()        # the view cone to 1.1 m alone is about 1 m^3, 37 000 cells of 3 cm
    assert got[0].tobytes() == want[0].tobytes() and got[1] == want[1]


def test_cpp_mirror_class(gpulib, tmp_path):
    """sgx::OctomapServer (sg_slam_amd/host/sgx_host.hpp) through example_localmap.cpp chaining cloud -> map: the restatement's record, bounds and grid"""
    import cloud_cases as cc
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__))); host = os.path.join(root, 'sg_slam_amd', 'host')
    exe = str(tmp_path / 'example_localmap')
    subprocess.check_call(['g++', '-O1', '-std=c++17', '-Wall', os.path.join(host, 'example_localmap.cpp'), '-o', exe, '-L' + os.path.join(root, 'sg_slam_amd'), '-lsgx',
                           '-Wl,-rpath,' + os.path.join(root, 'sg_slam_amd')])
    c = cc.CASE['dynamic_boxes']; e = cc.expected(c)
    Tcw = np.linalg.inv(cc.pose((0.1, -0.2, 0.05), (0.1, 0.2, -0.1))).astype('f4')
    c['depth'].tofile(tmp_path / 'd.f32'); c['color'].tofile(tmp_path / 'c.u8'); Tcw.tofile(tmp_path / 't.f32')
    out = subprocess.check_output([exe, '--octomap', '0.1', str(tmp_path / 'd.f32'), str(tmp_path / 'c.u8'), str(c['W']), str(c['H'])] + [repr(v) for v in c['cam']] + [str(tmp_path / 't.f32'), '1'] +
                                  [repr(v) for b in c['boxes'] for v in b], text=True).splitlines()
    lines = [ln for ln in out if ln.startswith('octomap')]
    import cloud_ref
    o, q = cloud_ref.camera_to_map_tf(Tcw); m = ref.sensor_to_world(o, q)
    R = ref.Octomap(ref.params(res=0.1)); rec = R.insert(np.asarray(e['points'], 'f4').reshape(-1, 3), m); b = R.bounds(); h = R.header(b); g = R.grid_from_cells(h)
    assert lines[0] == 'octomap record: ' + ' '.join(str(rec[k]) for k in ('n_in', 'n_passed', 'n_free_updates', 'n_occupied_updates', 'n_new_cells', 'flags'))
    assert lines[1] == 'octomap bounds: %d %d %d' % (b['n_known'], b['n_occupied'], b['n_free'])
    assert lines[2] == 'octomap grid: %d %d %d %d %d' % (h['width'], h['height'], (g == 100).sum(), (g == 0).sum(), (g == -1).sum()) and rec['n_occupied_updates'] > 20
