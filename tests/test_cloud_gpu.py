"""PointCloudMapping's keyframe cloud on the MI355X: the product library against the restatement (tests/cloud_ref.py) on every case of tests/cloud_cases.py bit for
bit, the voxel cloud, distances and kept flags through the tap build, the batch against single calls, two runs of one batch, a full-size batch with TUM3's own
parameters on a side stream against the emulator, and the C++ mirror class."""
import os
import subprocess
import numpy as np
import pytest
import cloud_cases as cc
import cloud_ref as ref
from sg_slam_amd.pointcloudmapping import PointCloudMappingBatch

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize('name', cc.NAMES)
def test_device_equals_restatement(gpulib, name):
    r = cc.run_case(gpulib, cc.CASE[name])
    if name == 'far_speck': assert r['larger_window_points'] > 0


def test_device_dynamic_branches(gpulib):
    c = cc.CASE['dynamic_boxes']
    b = cc.run_case(gpulib, cc.variant(c, have_dynamic=0)); n = cc.run_case(gpulib, cc.variant(c, p_consider_dynamic=0))
    assert b['n_pixels_used'] == n['n_pixels_used'] == c['W'] * c['H'] and b.tobytes() == n.tobytes()


def test_device_taps(gpulib_taps):
    """the voxel cloud before the filter, the distances and the kept flags"""
    for name in ('lattice_wall', 'tilted_planes', 'holes', 'far_speck', 'long_runs', 'few_points', 'world_drift'):
        cc.run_case(gpulib_taps, cc.CASE[name])


def test_device_batch_equals_singles(gpulib):
    cc.check_batch_equals_singles(gpulib, cc.batch_group())
    cc.check_batch_equals_singles(gpulib, [cc.CASE['world_plain'], cc.variant(cc.CASE['world_plain'], Twc=cc.pose((0.2, 0.1, -0.3), (-0.4, 0.2, 0.1)))])


def test_two_runs_of_a_batch_are_identical(gpulib_taps):
    """points, records and taps: no result depends on the order in which the atomics of a run arrive"""
    cs = cc.batch_group()
    B = PointCloudMappingBatch(cs[0]['params'], cs[0]['W'], cs[0]['H'], cs[0]['cam'], len(cs), cs[0]['mode'], max_boxes=4, lib=gpulib_taps)
    a = cc.run_batch(gpulib_taps, cs, B); ta = [B.debug_read(i) for i in range(len(cs))]
    b = cc.run_batch(gpulib_taps, cs, B); tb = [B.debug_read(i) for i in range(len(cs))]
    for (pa, ra), (pb, rb), xa, xb, c in zip(a, b, ta, tb, cs):
        assert pa.tobytes() == pb.tobytes() and ra.tobytes() == rb.tobytes(), c['name']
        assert all(u.tobytes() == v.tobytes() for u, v in zip(xa, xb)), c['name']
        cc.assert_taps(xa, cc.expected(c), c['name'])
    B.close()


def test_full_size_batch_on_a_side_stream_equals_emulator(gpulib, emu):
    """640 x 480, TUM3's parameters (mean_k 50, leaf 1 cm), three keyframes, one with a person box, through sgx_cloud_build_batch_dev on a non-default stream"""
    import torch
    F = cc.tum3_full()
    E = PointCloudMappingBatch(F['params'], F['W'], F['H'], F['cam'], 3, ref.LOCAL, max_boxes=4, lib=emu)
    want = E.build(F['depths'], F['colors'], None, F['boxes'], F['have_dynamic']); E.close()
    assert all(20000 <= r['n_voxels'] <= 60000 and r['flags'] == 0 and 0.9 * r['n_voxels'] < r['n_points'] < r['n_voxels'] for _, r in want)
    assert want[1][1]['n_pixels_used'] < want[0][1]['n_pixels_used'] - 40000                                     # the person box
    G = PointCloudMappingBatch(F['params'], F['W'], F['H'], F['cam'], 3, ref.LOCAL, max_boxes=4, lib=gpulib)
    s = torch.cuda.Stream()
    with torch.cuda.stream(s):
        G.launch(F['depths'], F['colors'], None, F['boxes'], F['have_dynamic'])
    s.synchronize()
    got = G.read(); G.close()
    for i, ((pg, rg), (pw, rw)) in enumerate(zip(got, want)):
        assert rg.tobytes() == rw.tobytes() and pg.tobytes() == pw.tobytes(), i


def test_cpp_mirror_class(gpulib, tmp_path):
    """sgx::PointCloudMapping (sg_slam_amd/host/sgx_host.hpp) through example_localmap.cpp: the restatement's bits"""
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__))); host = os.path.join(root, 'sg_slam_amd', 'host')
    exe = str(tmp_path / 'example_localmap')
    subprocess.check_call(['g++', '-O1', '-std=c++17', '-Wall', os.path.join(host, 'example_localmap.cpp'), '-o', exe, '-L' + os.path.join(root, 'sg_slam_amd'), '-lsgx',
                           '-Wl,-rpath,' + os.path.join(root, 'sg_slam_amd')])
    c = cc.CASE['dynamic_boxes']; e = cc.expected(c)
    Tcw = np.linalg.inv(cc.pose()).astype('f4')
    c['depth'].tofile(tmp_path / 'd.f32'); c['color'].tofile(tmp_path / 'c.u8'); Tcw.tofile(tmp_path / 't.f32')
    out = subprocess.check_output([exe, str(tmp_path / 'd.f32'), str(tmp_path / 'c.u8'), str(c['W']), str(c['H'])] + [repr(v) for v in c['cam']] + [str(tmp_path / 't.f32'), '1'] +
                                  [repr(v) for b in c['boxes'] for v in b], text=True).splitlines()
    h = out[0].split()
    assert [int(h[i]) for i in (1, 3, 5, 7)] == [e['n_points'], e['n_pixels_used'], e['n_voxels'], e['flags']] and float(h[9]) == e['mean'] and float(h[11]) == e['thr']
    o, q = ref.camera_to_map_tf(Tcw)
    assert [float(v) for v in out[1].split()[1:]] == list(o) + list(q)
    rows = np.array([[float(v) for v in ln.split()] for ln in out[2:]])
    assert len(rows) == e['n_points'] and (cc.bits(rows[:, :3].astype('f4')) == cc.bits(e['points'])).all() and (rows[:, 3].astype(np.uint32) == e['rgba']).all()
