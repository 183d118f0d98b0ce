"""ORB pyramid on the device (tap build): the fused k_pyramid against the per-level k_resize path and the oracle (tests/orb_pyramid_cases.py)."""
import numpy as np
import pytest
import orb_pyramid_cases as pc

pytestmark = pytest.mark.gpu


def _dev(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


@pytest.mark.parametrize('w,h,batch', pc.GEOMETRIES)
def test_orb_pyramid_gpu(gpulib_taps, oracle, w, h, batch):
    pc.check_pyramid(gpulib_taps, oracle, _dev, w, h, batch)
