"""GPU: sgx::CovisibilityGraph (sg_slam_amd/host/sgx_host.hpp) driven by `example_backend covis` prints what the restatement of tests/covis_ref.py computes: the
UpdateConnections reports and lists, the local map of a frame, the culling votes and the culling loop."""
import os
import subprocess
import numpy as np
import pytest
import covis_ref
import covis_cases as cc

pytestmark = pytest.mark.gpu


def test_cpp_covisibility_graph_mirror(gpulib, tmp_path):
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__))); host = os.path.join(root, 'sg_slam_amd', 'host')
    exe = str(tmp_path / 'example_backend')
    subprocess.check_call(['g++', '-O1', '-std=c++17', '-Wall', os.path.join(host, 'example_backend.cpp'), '-o', exe, '-L' + os.path.join(root, 'sg_slam_amd'), '-lsgx',
                           '-Wl,-rpath,' + os.path.join(root, 'sg_slam_amd')])
    case = cc.walk_script(8, nkf=30, npts=260, window=110, per_kf=56, mutate=False)
    R = covis_ref.Map(False, cc.TH_DEPTH, 1 << 14)
    kfs = [o for o in case['ops'] if o[0] == 'kf']; obs = {o[1]: o for o in case['ops'] if o[0] == 'obs'}
    with open(tmp_path / 'map.bin', 'wb') as f:
        np.array([0, len(kfs)], 'i4').tofile(f)
        for o in kfs:
            pts = np.full(len(o[2]), -1, 'i4'); pts[obs[o[1]][2]] = obs[o[1]][3]
            np.array([o[1], len(o[2])], 'i4').tofile(f); o[2].astype('i4').tofile(f); o[3].astype('f4').tofile(f); o[4].astype('f4').tofile(f); pts.tofile(f)
            R.add_keyframe(o[1], o[2], o[3], o[4]); R.set_observations(o[1], obs[o[1]][2], obs[o[1]][3])
        ids = [o[1] for o in kfs]
        np.array([len(ids)] + ids, 'i4').tofile(f)
        frame = [int(p) for p in np.random.RandomState(2).randint(60, 170, 50)] + [-1, 259]
        np.array([len(frame)] + frame, 'i4').tofile(f)
        cur = ids[len(ids) // 2]
        np.array([cur], 'i4').tofile(f)
    out = subprocess.check_output([exe, 'covis', str(tmp_path / 'map.bin')], text=True).splitlines()
    for k, line in zip(ids, out):
        rep = R.update_connections(k); o, w = R.ordered(k)
        assert line == 'uc %d: ' % k + ' '.join(str(x) for x in rep) + ' |' + ''.join(' %d:%d' % e for e in zip(o, w)) + ' |' + ''.join(' %d' % c for c in R.best_covisibles(k, 10)), (k, line)
    out = out[len(ids):]
    L = R.local_map(frame, 3, [], -1, 1 << 14)
    assert out[0] == 'local_kf %d ref %d tracked %d:' % (len(L['local_kf']), L['ref_kf'], L['ref_tracked']) + ''.join(' %d' % k for k in L['local_kf'])
    assert out[1] == 'local_points %d:' % L['n_points'] + ''.join(' %d/%d' % e for e in zip(L['points'], L['obs'])) and L['n_points'] > 100
    assert out[2] == 'votes:' + ''.join(' %d:%d/%d/%d' % v for v in R.culling_votes(cur)) and len(R.culling_votes(cur)) >= 2
    assert out[3] == 'culled:' + ''.join(' %d' % k for k in R.KeyFrameCulling(cur))
    p, _, ch = R.tree(cur)
    assert out[4] == 'parent of %d: %d, children:' % (cur, p) + ''.join(' %d' % c for c in ch)
