"""GPU: sgx::Initializer (sg_slam_amd/host/sgx_host.hpp) driven by example_initializer.cpp prints the restatement's bits."""
import os
import subprocess
import numpy as np
import pytest
import init_cases as ic

pytestmark = pytest.mark.gpu


def test_cpp_initializer_mirror(gpulib, tmp_path):
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__))); host = os.path.join(root, 'sg_slam_amd', 'host')
    exe = str(tmp_path / 'example_initializer')
    subprocess.check_call(['g++', '-O1', '-std=c++17', '-Wall', os.path.join(host, 'example_initializer.cpp'), '-o', exe, '-L' + os.path.join(root, 'sg_slam_amd'), '-lsgx',
                           '-Wl,-rpath,' + os.path.join(root, 'sg_slam_amd')])
    for name in ('general_300', 'planar_ok_300', 'rotation_257'):
        c = next(c for c in ic.CASES if c[0] == name); sc, d, want = ic.expected(name)
        sc[0].tofile(tmp_path / 'k1.f32'); sc[1].tofile(tmp_path / 'k2.f32'); sc[2].astype('i4').tofile(tmp_path / 'm.i32'); d.astype('i4').tofile(tmp_path / 'd.i32')
        out = subprocess.check_output([exe, str(tmp_path / 'k1.f32'), str(len(sc[0])), str(tmp_path / 'k2.f32'), str(len(sc[1])), str(tmp_path / 'm.i32'), str(tmp_path / 'd.i32'),
                                       str(c[2])] + [repr(float(v)) for v in ic.CAM], text=True).splitlines()
        assert out[0] == 'ok %d model %d triangulated %d' % (want[0], want[6]['model'], want[4].sum() if want[0] else 0), (name, out)
        if want[0]:
            got = np.array([float(x) for x in out[1].split()], 'f4')
            assert (ic.bits(got) == ic.bits(np.concatenate([want[1].reshape(9), want[2]]))).all(), name
