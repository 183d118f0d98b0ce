"""Detector3D on the MI355X: the product library against the restatement (tests/obj3d_ref.py) on every case of tests/obj3d_cases.py bit for bit, the kept flags and
component labels through the tap build, the batch against single calls, two runs of one batch (the union-find's atomics), and a full-size batch with TUM3's own
parameters on a side stream against the emulator."""
import numpy as np
import pytest
import obj3d_cases as oc
from sg_slam_amd.detector3d import Detector3DBatch

pytestmark = pytest.mark.gpu
CASE = {c['name']: c for c in oc.CASES}


@pytest.mark.parametrize('name', oc.NAMES)
def test_device_equals_restatement(gpulib, name):
    r = oc.run_case(gpulib, CASE[name])
    if name == 'holes70': assert r['larger_window_points'] > 0


def test_device_kept_flags_and_labels(gpulib_taps):
    for name in ('object_wall', 'holes_nan_range', 'holes70', 'equal_size'):
        oc.run_case(gpulib_taps, CASE[name])


def test_device_batch_equals_singles(gpulib):
    oc.check_batch_equals_singles(gpulib, oc.batch_group())


def test_two_runs_of_a_batch_are_identical(gpulib_taps):
    """records, kept flags and labels: the component id is the smallest point whatever order the unions ran in"""
    cs = oc.batch_group()
    B = Detector3DBatch(cs[0]['params'], cs[0]['W'], cs[0]['H'], cs[0]['cam'], len(cs), len(cs), lib=gpulib_taps)
    args = (np.stack([c['depth'] for c in cs]), np.stack([c['Twc'] for c in cs]), [(i, c['obj']) for i, c in enumerate(cs)])
    a = B.detect(*args); ta = [B.debug_read(i) for i in range(len(cs))]
    b = B.detect(*args); tb = [B.debug_read(i) for i in range(len(cs))]
    assert a.tobytes() == b.tobytes()
    for (ka, la), (kb, lb), c in zip(ta, tb, cs):
        assert (ka == kb).all() and (la == lb).all()
        assert (ka == oc.expected(c)['kept']).all() and (la == oc.expected(c)['labels']).all()
    B.close()


def test_full_size_batch_on_a_side_stream_equals_emulator(gpulib, emu):
    """640 x 480, TUM3's parameters, five boxes over three keyframes, among them a box that is the whole image (its crop of 384 x 288 cells is the largest there is),
    through sgx_obj3d_detect_batch_dev on a non-default stream"""
    import torch
    F = oc.full_size_batch()
    E = Detector3DBatch(F['params'], F['W'], F['H'], F['cam'], 3, 5, lib=emu)
    want = E.detect(F['depths'], F['Twcs'], F['jobs']); E.close()
    assert want['found'].sum() >= 2 and want['crop_points'].max() > 105000 and want['clusters'].max() >= 2          # 384 x 288 = 110 592 cells, dense
    G = Detector3DBatch(F['params'], F['W'], F['H'], F['cam'], 3, 5, lib=gpulib)
    s = torch.cuda.Stream()
    with torch.cuda.stream(s):
        G.launch(F['depths'], F['Twcs'], F['jobs'])
    s.synchronize()
    got = G.read(); G.close()
    for j in range(5): oc.assert_same_records(got[j], want[j], j)


def test_cpp_mirror_classes(gpulib, tmp_path):
    """sgx::Detector3D / sgx::ObjectDatabase (sg_slam_amd/host/sgx_host.hpp): Detect() twice on one box = one object in the database, the restatement's bits"""
    import os
    import subprocess
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__))); host = os.path.join(root, 'sg_slam_amd', 'host')
    exe = str(tmp_path / 'example_objects')
    subprocess.check_call(['g++', '-O1', '-std=c++17', '-Wall', os.path.join(host, 'example_objects.cpp'), '-o', exe, '-L' + os.path.join(root, 'sg_slam_amd'), '-lsgx',
                           '-Wl,-rpath,' + os.path.join(root, 'sg_slam_amd')])
    c = CASE['object_wall']; e = oc.expected(c)
    c['depth'].tofile(tmp_path / 'd.f32'); np.ascontiguousarray(c['Twc'], 'f8').tofile(tmp_path / 't.f64')
    cid, prob, rect = c['obj']
    out = subprocess.check_output([exe, str(tmp_path / 'd.f32'), str(c['W']), str(c['H'])] + [repr(v) for v in c['cam']] + [str(tmp_path / 't.f64'), str(cid), repr(prob)] +
                                  [repr(v) for v in rect], text=True).splitlines()
    assert out[0] == 'objects 1'
    v = out[1].split()
    assert (int(v[0]), int(v[1])) == (1, cid)
    got = np.array([float(x) for x in v[2:]], 'f4')
    assert (oc.bits(got) == oc.bits(np.concatenate([[np.float32(prob)], e['centroid'], e['size']]))).all()
