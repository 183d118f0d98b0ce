"""LK pyramid, kernel-logic emulator: every byte of every level slot (padding columns included) for batch 3 with a source pitch above the width
(tests/lk_pyramid_cases.py; tests/test_lk_pyramid_gpu.py repeats it on the device)."""
import pytest
import lk_pyramid_cases as pc


@pytest.mark.parametrize('w,h', pc.SIZES)
def test_lk_pyramid_slots_emu(emu, oracle, w, h):
    pc.check_slots(emu, oracle, lambda a: a, w, h)
