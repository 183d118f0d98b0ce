"""LK tracker, kernel-logic emulator: the geometries, criteria and batch layouts of tests/lk_track_cases.py against the oracle, bit for bit
(tests/test_lk_track_gpu.py repeats them on the device, where the wave kernel runs instead of its scalar twin)."""
import pytest
import lk_track_cases as tc

_xp = lambda a: a


@pytest.fixture(scope='module')
def geometry_refs(oracle):
    return tc.geometry_reference(oracle)


@pytest.mark.parametrize('w,h,nl', tc.GEOMETRY)
def test_geometry_emu(emu, geometry_refs, w, h, nl):
    tc.check_geometry(emu, geometry_refs, w, h, nl)


@pytest.mark.parametrize('w,h', tc.SMALL)
def test_small_emu(emu, oracle, w, h):
    tc.check_small(emu, oracle, _xp, w, h)


@pytest.mark.parametrize('max_level', [0, 1, 2])
def test_depth_emu(emu, oracle, max_level):
    tc.check_depth(emu, oracle, max_level)


@pytest.mark.parametrize('max_count,epsilon,most', tc.CRITERIA)
def test_criteria_emu(emu, oracle, max_count, epsilon, most):
    tc.check_criteria(emu, oracle, max_count, epsilon, most)


@pytest.mark.parametrize('max_level', [0, 3])
def test_restage_emu(emu, oracle, max_level):
    tc.check_restage(emu, oracle, max_level)


def test_noise_emu(emu, oracle):
    tc.check_noise(emu, oracle)


def test_batch_emu(emu, oracle):
    tc.check_batch(emu, oracle, _xp)
