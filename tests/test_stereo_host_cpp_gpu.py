"""GPU: sgx::StereoMatcher (sg_slam_amd/host/sgx_host.hpp) through `example_backend stereo` — two extractors on the two images, then sgx_stereo_match — prints the
restatement's mvuRight / mvDepth bit for bit."""
import os
import subprocess
import numpy as np
import pytest
import stereo_cases as sc

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_cpp_stereo_matcher_equals_restatement(gpulib, emu, tmp_path):
    exe = os.path.join(ROOT, 'sg_slam_amd', 'host', 'example_backend')
    if not os.path.exists(exe):
        import __graft_entry__
        __graft_entry__.build()
    c = sc.build(emu)['small_slant']; g = sc.GEOM['small']; e = sc.expected(c)
    c['left'].tofile(tmp_path / 'l.raw'); c['right'].tofile(tmp_path / 'r.raw')
    out = subprocess.check_output([exe, 'stereo', str(tmp_path / 'l.raw'), str(tmp_path / 'r.raw'), str(g['width']), str(g['height']), str(g['nfeatures']), repr(g['scaleFactor']),
                                   str(g['nlevels']), repr(g['fx']), repr(g['bf'])], text=True).splitlines()
    h = out[0].split()
    assert [int(h[1]), int(h[3]), int(h[5])] == [len(c['keys_left']), len(c['keys_right']), int((e['uright'] != -1).sum())]
    rows = np.array([[float(v) for v in ln.split()] for ln in out[1:]], 'f4')
    assert len(rows) == len(e['uright']) and (rows[:, 0] == c['keys_left']['x']).all() and (rows[:, 1] == c['keys_left']['y']).all()
    assert (rows[:, 2].view(np.uint32) == e['uright'].view(np.uint32)).all() and (rows[:, 3].view(np.uint32) == e['depth'].view(np.uint32)).all()
    assert (e['uright'] != -1).sum() >= 50
