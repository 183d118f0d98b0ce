"""GPU: the C++ mirror of the essential-graph query (sgx::CovisibilityGraph::essential_graph in sg_slam_amd/host/sgx_host.hpp) through example_backend: the line it
prints for the map of a walk equals the restatement of tests/loop_ref.py."""
import os
import subprocess
import numpy as np
import pytest
import covis_cases as cc
import loop_ref as lr

pytestmark = pytest.mark.gpu


def test_cpp_essential_graph_mirror(gpulib, tmp_path):
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__))); host = os.path.join(root, 'sg_slam_amd', 'host')
    exe = str(tmp_path / 'example_backend')
    subprocess.check_call(['g++', '-O1', '-std=c++17', '-Wall', os.path.join(host, 'example_backend.cpp'), '-o', exe, '-L' + os.path.join(root, 'sg_slam_amd'), '-lsgx',
                           '-Wl,-rpath,' + os.path.join(root, 'sg_slam_amd')])
    case = cc.walk_script(8, nkf=20, npts=420, window=180, per_kf=150, cap=160, mutate=False)      # neighbours share 100 points and more
    R = lr.Map(False, cc.TH_DEPTH, 1 << 14)
    kfs = [o for o in case['ops'] if o[0] == 'kf']; obs = {o[1]: o for o in case['ops'] if o[0] == 'obs'}
    with open(tmp_path / 'map.bin', 'wb') as f:
        np.array([0, len(kfs)], 'i4').tofile(f)
        for o in kfs:
            pts = np.full(len(o[2]), -1, 'i4'); pts[obs[o[1]][2]] = obs[o[1]][3]
            np.array([o[1], len(o[2])], 'i4').tofile(f); o[2].astype('i4').tofile(f); o[3].astype('f4').tofile(f); o[4].astype('f4').tofile(f); pts.tofile(f)
            R.add_keyframe(o[1], o[2], o[3], o[4]); R.set_observations(o[1], obs[o[1]][2], obs[o[1]][3])
        ids = [o[1] for o in kfs]
        np.array([len(ids)] + ids, 'i4').tofile(f)
        np.array([1, -1], 'i4').tofile(f)
        cur = ids[len(ids) // 2]
        np.array([cur], 'i4').tofile(f)
    out = subprocess.check_output([exe, 'covis', str(tmp_path / 'map.bin')], text=True).splitlines()
    for k in ids: R.update_connections(k)
    R.KeyFrameCulling(cur)
    parent = R.tree(cur)[0]; loop = parent if parent >= 0 else cur
    w = lr.flatten_graph(lr.essential_graph(R, cur, loop, [cur], [0, 0], []))
    assert w['report']['n_kind'][1] > 5 and w['report']['n_kind'][3] > 0
    assert out[-3] == 'eg vertices %d fixed %d edges' % (len(w['vertex_id']), loop) + ''.join(' %d:%d:%d' % e for e in w['edges_by_id'])


def test_cpp_correct_loop_mirror(gpulib, tmp_path):
    """sgx::Optimizer::CorrectLoop on a map of three keyframes (example_backend loop) against CovisibilityGraph.correct_loop on the same map: the rows are equal; the poses
    and points agree to 1e-5: the C++ mirror corrects the points through sgx_correct_map_points, whose unit fuses multiply-adds, the Python one through the form
    evaluated as written; on values below 10 that is a few float32 units in the last place, 1e-6, and 1e-5 leaves room for the optimiser's own run-to-run equality."""
    from sg_slam_amd.covisibility import CovisibilityGraph
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__))); host = os.path.join(root, 'sg_slam_amd', 'host')
    exe = str(tmp_path / 'example_backend')
    subprocess.check_call(['g++', '-O1', '-std=c++17', '-Wall', os.path.join(host, 'example_backend.cpp'), '-o', exe, '-L' + os.path.join(root, 'sg_slam_amd'), '-lsgx',
                           '-Wl,-rpath,' + os.path.join(root, 'sg_slam_amd')])
    out = subprocess.check_output([exe, 'loop'], text=True).splitlines()
    G = CovisibilityGraph(max_keyframes=8, cap=32, max_points=64, max_observations=256, max_queries=2, lib=gpulib)
    for k in (1, 2, 3): G.add_keyframe(k, np.zeros(32, 'i4'), np.full(32, -1, 'f4'), np.ones(32, 'f4'))
    G.set_observations(1, range(30), range(30)); G.set_observations(2, range(16), range(16)); G.set_observations(3, range(14), range(16, 30))
    T = {}
    for k in (1, 2, 3):
        T[k] = np.eye(4, dtype='f4')[:3]; T[k][0, 3] = np.float32(-0.5) * np.float32(k); T[k][2, 3] = np.float32(0.1) * np.float32(k)
    i = np.arange(64, dtype='f4'); xw = np.stack([np.float32(0.1) * i, np.float32(1) - np.float32(0.05) * i, np.full(64, 4, 'f4')], 1)
    r = G.correct_loop(1, 3, [0, 0, 0, 1, -0.45, 0.02, 0.1, 1], T, xw)
    g = r['graph']
    assert out[0] == 'group' + ''.join(' %d' % k for k in r['begin']['group_id']) + ' lc' + ''.join(' %d' % k for k in r['connections']['lc_begin']) + ' /' + \
        ''.join(' %d' % k for k in r['connections']['lc_j']) + ' edges' + ''.join(' %d:%d:%d' % e for e in zip(g['e_i'], g['e_j'], g['e_kind'])) + ' loop edges of 1: 3'
    poses = np.array([float(x) for x in out[1].split()[1:]]).reshape(3, 3, 4); pts = np.array([float(x) for x in out[2].split()[1:]]).reshape(30, 3)
    assert np.abs(poses - np.array([r['Tcw'][k] for k in (1, 2, 3)])).max() <= 1e-5 and np.abs(pts - r['xw'][:30]).max() <= 1e-5
    assert np.abs(r['xw'][:30] - xw[:30]).max() > 1e-3
    G.close()
