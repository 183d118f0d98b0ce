"""LK tracker on the device: the geometries, criteria and batch layouts of tests/lk_track_cases.py against the oracle, bit for bit — k_lk_trackN<2> of the product library,
whose lane mapping, group sums, border paths and tile re-staging the emulator's scalar twin does not contain — and the tap build's other two lane mappings (SGX_LK_KPW)."""
import os
import subprocess
import sys
import numpy as np
import pytest
import lk_track_cases as tc

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _xp(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


@pytest.fixture(scope='module')
def geometry_refs(oracle):
    return tc.geometry_reference(oracle)


@pytest.mark.parametrize('w,h,nl', tc.GEOMETRY)
def test_geometry_gpu(gpulib, geometry_refs, w, h, nl):
    tc.check_geometry(gpulib, geometry_refs, w, h, nl)


@pytest.mark.parametrize('w,h', tc.SMALL)
def test_small_gpu(gpulib, oracle, w, h):
    tc.check_small(gpulib, oracle, _xp, w, h)


@pytest.mark.parametrize('max_level', [0, 1, 2])
def test_depth_gpu(gpulib, oracle, max_level):
    tc.check_depth(gpulib, oracle, max_level)


@pytest.mark.parametrize('max_count,epsilon,most', tc.CRITERIA)
def test_criteria_gpu(gpulib, oracle, max_count, epsilon, most):
    tc.check_criteria(gpulib, oracle, max_count, epsilon, most)


@pytest.mark.parametrize('max_level', [0, 3])
def test_restage_gpu(gpulib, oracle, max_level):
    tc.check_restage(gpulib, oracle, max_level)


def test_noise_gpu(gpulib, oracle):
    tc.check_noise(gpulib, oracle)


def test_batch_gpu(gpulib, oracle):
    tc.check_batch(gpulib, oracle, _xp)


# SGX_LK_KPW is read once per process, so each arm gets a fresh child: plain python, the tap library through SgxLib, the host entry; no torch
_CHILD = """
import sys
import numpy as np
sys.path.insert(0, sys.argv[1])
from sg_slam_amd.capi import SgxLib
from sg_slam_amd.flow import OpticalFlowLK
lib = SgxLib(sys.argv[2])
assert 'gfx950' in lib.version() and lib.has_taps
d = np.load(sys.argv[3]); out = {}
for k in ('g', 'n'):
    I, J, pts = d[k + '_I'], d[k + '_J'], d[k + '_pts']
    fl = OpticalFlowLK(width=I.shape[1], height=I.shape[0], lib=lib)
    out[k + '_xy'], out[k + '_st'] = fl(I, J, pts)
    fl.close()
np.savez(sys.argv[4], **out)
"""


def test_kpw_arms_gpu(gpulib_taps, geometry_refs, oracle, tmp_path):
    """the one- and four-keypoints-per-wave mappings of the tap build (k_lk_track, k_lk_trackN<4>) give the oracle's bits too: the A/B arms a change of the tracker is measured against"""
    I, J, pts, ref, rst, _ = geometry_refs[(97, 91)]
    a, b, npts = tc.noise_pair()
    nref, nrst = oracle.lk_pyr(a, b, npts, acc_mode=1)
    src = str(tmp_path / 'in.npz')
    np.savez(src, g_I=I, g_J=J, g_pts=pts, n_I=a, n_J=b, n_pts=npts)
    for kpw in ('1', '4'):                                      # one after the other; a failed child ends the test before the next one starts
        dst = str(tmp_path / f'out{kpw}.npz')
        r = subprocess.run([sys.executable, '-c', _CHILD, ROOT, gpulib_taps.path, src, dst], env=dict(os.environ, SGX_LK_KPW=kpw), timeout=120, capture_output=True, text=True)
        assert r.returncode == 0, f'SGX_LK_KPW={kpw}: exit {r.returncode}\n{r.stderr[-2000:]}'
        d = np.load(dst)
        tc.same(d['g_xy'], d['g_st'], ref, rst, f'SGX_LK_KPW={kpw} 97x91')
        tc.same(d['n_xy'], d['n_st'], nref, nrst, f'SGX_LK_KPW={kpw} noise')
