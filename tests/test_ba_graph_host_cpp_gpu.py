"""GPU: sgx::CovisibilityGraph::ba_graph / apply_ba_erase (sg_slam_amd/host/sgx_host.hpp) driven by `example_backend covis` print what the restatement of
tests/ba_graph_ref.py computes: the graph of the current keyframe, and the graph again after every third edge was erased as vToErase."""
import os
import subprocess
import numpy as np
import pytest
import covis_ref
import covis_cases as cc
import ba_graph_ref as br

pytestmark = pytest.mark.gpu


def line_of(w):
    return ('ba poses' + ''.join(' %d/%d' % e for e in zip(w['pose_id'], w['pose_fixed'])) + ' points' + ''.join(' %d' % p for p in w['point_id']) +
            ' edges' + ''.join(' %d:%d:%d:%d' % e for e in zip(w['edge_pose'], w['edge_point'], w['edge_kp'], w['edge_attr'])))


def test_cpp_ba_graph_mirror(gpulib, tmp_path):
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__))); host = os.path.join(root, 'sg_slam_amd', 'host')
    exe = str(tmp_path / 'example_backend')
    subprocess.check_call(['g++', '-O1', '-std=c++17', '-Wall', os.path.join(host, 'example_backend.cpp'), '-o', exe, '-L' + os.path.join(root, 'sg_slam_amd'), '-lsgx',
                           '-Wl,-rpath,' + os.path.join(root, 'sg_slam_amd')])
    case = cc.walk_script(8, nkf=30, npts=400, window=110, per_kf=56, mutate=False)      # 11 local keyframes and 19 fixed cameras around the middle keyframe
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
        np.array([1, -1], 'i4').tofile(f)
        cur = ids[len(ids) // 2]
        np.array([cur], 'i4').tofile(f)
    out = subprocess.check_output([exe, 'covis', str(tmp_path / 'map.bin')], text=True).splitlines()
    for k in ids: R.update_connections(k)
    R.KeyFrameCulling(cur)
    S = br.LocalBundleAdjustment(R, cur); w = br.flatten(S)
    assert w['report']['n_fixed_kf'] > 0 and w['report']['n_local_kf'] > 2 and w['report']['n_edges'] > 300
    assert out[-2] == line_of(w)
    br.apply_erase(R, S, [j % 3 == 0 for j in range(len(S['edges']))])
    assert out[-1] == line_of(br.flatten(br.LocalBundleAdjustment(R, cur)))
