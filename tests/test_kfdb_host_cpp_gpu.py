"""GPU: sgx::KeyFrameDatabase (sg_slam_amd/host/sgx_host.hpp) driven by example_relocalization.cpp prints the restatement's candidates and report."""
import os
import subprocess
import numpy as np
import pytest
import kfdb_ref
import kfdb_cases as kc
import voc_cases as vc
from sg_slam_amd.keyframedatabase import RELOCALIZATION, LOOP_CLOSING

pytestmark = pytest.mark.gpu


def _write_case(case, tmp_path):
    """the script's keyframes and its first query as the example's two files; returns the restatement's answer"""
    R = kfdb_ref.KeyFrameDatabase(case['nwords'])
    cov = {}
    for op in case['ops']:
        if op[0] == 'add': R.add(op[1], op[2])
        elif op[0] == 'cov': R.set_covisibility(op[1], op[2]); cov[op[1]] = op[2]
    with open(tmp_path / 'db.bin', 'wb') as f:
        np.array([len(R.kfs)], 'i4').tofile(f)
        for i, kf in R.kfs.items():
            nb = np.asarray(cov.get(i, []), 'i4')
            np.array([i, len(kf.mBowVec[0]), len(nb)], 'i4').tofile(f); kf.mBowVec[0].tofile(f); kf.mBowVec[1].tofile(f); nb.tofile(f)
    q = next(op for op in case['ops'] if op[0] in ('reloc', 'loop'))
    with open(tmp_path / 'query.bin', 'wb') as f:
        np.array([0 if q[0] == 'reloc' else 1, len(q[1][0])], 'i4').tofile(f); q[1][0].tofile(f); q[1][1].tofile(f)
        if q[0] == 'loop': np.array([len(q[2])] + list(q[2]), 'i4').tofile(f)
    if q[0] == 'reloc': return None, R.DetectRelocalizationCandidates(q[1]), R.report
    ms = R.min_score(q[1], q[2])
    return ms, R.DetectLoopCandidates(q[1], q[2], ms), R.report


def test_cpp_keyframe_database_mirror(gpulib, tmp_path):
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__))); host = os.path.join(root, 'sg_slam_amd', 'host')
    exe = str(tmp_path / 'example_relocalization')
    subprocess.check_call(['g++', '-O1', '-std=c++17', '-Wall', os.path.join(host, 'example_relocalization.cpp'), '-o', exe, '-L' + os.path.join(root, 'sg_slam_amd'), '-lsgx',
                           '-Wl,-rpath,' + os.path.join(root, 'sg_slam_amd')])
    voc = vc.make_vocabulary(3, k=10, L=3, early_leaf=0.0)                 # 1 000 words: the database takes its size and its L1 scoring from the file
    nwords = int(voc['is_leaf'].sum())
    vc.write_text(voc, str(tmp_path / 'voc.txt'))
    for mode in (RELOCALIZATION, LOOP_CLOSING):
        case = kc.places_script(5, mode, N=65, nwords=nwords, places=6, per_place=100, lo=30, hi=120)
        ms, ref, rep = _write_case(case, tmp_path)
        out = subprocess.check_output([exe, str(tmp_path / 'voc.txt'), str(tmp_path / 'db.bin'), str(tmp_path / 'query.bin')], text=True).splitlines()
        if mode == LOOP_CLOSING:
            assert kc.bits(np.float32(float(out[0].split()[1]))) == kc.bits(ms); out = out[1:]
        assert out[0] == 'candidates %d:' % len(ref) + ''.join(' %d' % c for c in ref), (mode, out, ref)
        r = out[1].split()
        assert [int(x) for x in r[1:6]] + [int(r[8])] == [rep[k] for k in ('n_sharing', 'max_common_words', 'min_common_words', 'n_scores', 'n_score_and_match', 'n_candidates')]
        assert kc.bits(np.float32(float(r[6]))) == kc.bits(rep['best_acc_score']) and kc.bits(np.float32(float(r[7]))) == kc.bits(rep['min_score_to_retain'])
        assert len(ref) >= 1
