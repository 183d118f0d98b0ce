"""GPU: the C++ mirror of the loop-closing thread (sgx::LoopClosing::DetectLoop / CorrectLoop / RunGlobalBundleAdjustment in sg_slam_amd/host/sgx_host.hpp, over
sgx::KeyFrameDatabase, sgx::CovisibilityGraph and sgx::Optimizer) through `example_backend loopclose`: it closes the ring of 40 keyframes of
loopclose_cases.ring_scene and prints what it did; the Python class sg_slam_amd.loopclosing.LoopClosing does the same on the same arrays.  Integers (the accepted
keyframe, the candidates, the groups, the group row, the states, the early exits) are equal.  Poses and points agree to 1e-4: the C++ CorrectLoop corrects the points
through sgx_correct_map_points, whose unit fuses multiply-adds, the Python one through the form evaluated as written (tests/test_loop_host_cpp_gpu.py: 1e-5 on its
outputs); that difference of a few float32 units in the last place is the solver's input here, and ten LM iterations on 40 poses carry it to the fifth decimal."""
import os
import subprocess
import numpy as np
import pytest
import kfdb_cases as kc
import voc_cases as vc
import loopclose_cases as lc

pytestmark = pytest.mark.gpu


def test_cpp_loopclosing_mirror(gpulib, tmp_path):
    from sg_slam_amd.covisibility import CovisibilityGraph
    from sg_slam_amd.keyframedatabase import KeyFrameDatabase
    from sg_slam_amd.loopclosing import LoopClosing
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__))); host = os.path.join(root, 'sg_slam_amd', 'host')
    exe = str(tmp_path / 'example_backend')
    subprocess.check_call(['g++', '-O1', '-std=c++17', '-Wall', os.path.join(host, 'example_backend.cpp'), '-o', exe, '-L' + os.path.join(root, 'sg_slam_amd'), '-lsgx',
                           '-Wl,-rpath,' + os.path.join(root, 'sg_slam_amd')])
    S = lc.ring_scene(); nkf = S['nkf']; cap = S['cap']; npts = S['npts']; kfs = S['kfs']
    voc = vc.make_vocabulary(3, k=10, L=3, early_leaf=0.0); nwords = int(voc['is_leaf'].sum()); assert npts <= nwords
    vc.write_text(voc, str(tmp_path / 'voc.txt'))
    with open(tmp_path / 'ring.bin', 'wb') as f:
        np.array([nkf, len(kfs) - nkf, cap, npts, len(S['dup']), S['cur'], S['loop']], 'i4').tofile(f)
        for k in kfs:
            np.array([k['id'], k['parent'], k['i0'], len(k['pts'])], 'i4').tofile(f)
            k['uright'].astype('f4').tofile(f); k['depth'].astype('f4').tofile(f); k['uv'].astype('f4').tofile(f); np.array(k['pts'], 'i4').tofile(f); k['T'].astype('f4').tofile(f)
            np.array([len(k['words'])] + list(k['words']), 'i4').tofile(f)
        S['xw'].astype('f4').tofile(f); S['pref'].astype('i4').tofile(f); np.array(S['dup'], 'i4').tofile(f); np.asarray(S['Scw'], 'f8').tofile(f)
        np.array([S['cam'][c] for c in ('fx', 'fy', 'cx', 'cy', 'bf')], 'f4').tofile(f); S['inv'].tofile(f)
    out = subprocess.check_output([exe, 'loopclose', str(tmp_path / 'voc.txt'), str(tmp_path / 'ring.bin')], text=True).splitlines()
    # the same through the Python class
    G = CovisibilityGraph(max_keyframes=64, cap=cap, max_points=npts, max_observations=8 * npts, max_queries=8, lib=gpulib)
    V = kc.make_voc(gpulib, nwords); db = KeyFrameDatabase(V, max_keyframes=64, lib=gpulib); L = LoopClosing(G, db, V)
    KF = {}; T = {}
    def add(k):
        G.add_keyframe(k['id'], np.zeros(cap, 'i4'), k['uright'], k['depth']); G.set_observations(k['id'], range(len(k['pts'])), k['pts'])
        if k['parent'] >= 0: G.set_observations(k['parent'], range(k['i0'], k['i0'] + len(k['pts'])), k['pts'])
        G.update_connections([k['id']]); KF[k['id']] = dict(uv=k['uv'], uright=k['uright']); T[k['id']] = k['T']
    bow = lambda k: kc.bow_of(k['words'])
    line = 'accepted'
    for k in kfs[:nkf]:
        add(k)
        if L.DetectLoop(k['id'], bow(k)): line += ' %d enough' % k['id'] + ''.join(' %d' % c for c in L.mvpEnoughConsistentCandidates)
    line += ' groups' + ''.join(' [' + ''.join(' %d' % i for i in ids) + ' ]:%d' % n for ids, n in G.consistent_groups())
    assert out[0] == line and line.startswith('accepted 39 enough'), (out[0], line)
    def fuse(graph, b, c):
        for a_, b_ in S['dup']: graph.replace_point(a_, b_)
    res = L.CorrectLoop(S['cur'], S['loop'], S['Scw'], T, S['xw'], fuse=fuse)
    assert out[1] == 'loop last %d group' % L.mLastLoopKFid + ''.join(' %d' % k for k in res['begin']['group_id']) + ' edges %d loop edges of %d:' % (len(res['graph']['e_i']), S['cur']) + \
        ''.join(' %d' % k for k in G.loop_edges(S['cur'])), out[1]
    for t in range(nkf): KF[t]['Tcw'] = np.r_[res['Tcw'][t], [[0, 0, 0, 1]]].astype('f4')
    new_T = {k['id']: k['T'] for k in kfs[nkf:]}
    def meanwhile():
        for k in kfs[nkf:]: add(k)
    u = L.RunGlobalBundleAdjustment(S['cur'], KF, res['xw'], S['inv'], S['cam'], origins=[0], point_ref=S['pref'], new_Tcw=new_T, new_xw=res['xw'], while_running=meanwhile)
    assert u['status'] == 0
    early = []
    for k in kfs[nkf:]: L.DetectLoop(k['id'], bow(k)); early.append(int(L.last['early']))
    r = u['report']
    assert out[2] == 'gba visited %d propagated %d unreached %d depth %d state' % (int(r['n_visited']), int(r['n_propagated']), int(r['n_unreached']), int(r['max_depth'])) + \
        ''.join(' %d' % s for s in u['kf_state']) + ' ids' + ''.join(' %d' % k for k in u['kf_ids']) + ' early' + ''.join(' %d' % e for e in early) + ' db %d' % db.size(), out[2]
    assert int(r['n_propagated']) == 10 and early == [1] * 9 + [0]
    poses = np.array([float(x) for x in out[3].split()[1:]]).reshape(-1, 3, 4); pts = np.array([float(x) for x in out[4].split()[1:]]).reshape(-1, 4)
    assert [int(p) for p in pts[:, 0]] == u['point_ids'] and len(poses) == 50
    assert np.abs(poses - u['Tcw_out']).max() <= 1e-4 and np.abs(pts[:, 1:] - u['xw_out']).max() <= 1e-4, (np.abs(poses - u['Tcw_out']).max(), np.abs(pts[:, 1:] - u['xw_out']).max())
    assert np.abs(u['Tcw_out'] - u['Tcw_in']).max() > 1e-3
    db.close(); G.close()
