"""ORB pyramid, kernel-logic emulator: the fused k_pyramid against the per-level k_resize path and the oracle (tests/orb_pyramid_cases.py;
tests/test_orb_pyramid_gpu.py repeats it on the device)."""
import pytest
import orb_pyramid_cases as pc


@pytest.mark.parametrize('w,h,batch', pc.GEOMETRIES)
def test_orb_pyramid_emu(emu, oracle, w, h, batch):
    pc.check_pyramid(emu, oracle, lambda a: a, w, h, batch)
