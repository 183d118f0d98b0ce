"""LK pyramid on the device (tap build: the slots are read back through include/sgx_debug.h): every byte of every level slot, padding columns included,
for batch 3 with a source pitch above the width (tests/lk_pyramid_cases.py)."""
import numpy as np
import pytest
import lk_pyramid_cases as pc

pytestmark = pytest.mark.gpu


def _xp(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


@pytest.mark.parametrize('w,h', pc.SIZES)
def test_lk_pyramid_slots_gpu(gpulib_taps, oracle, w, h):
    pc.check_slots(gpulib_taps, oracle, _xp, w, h)
