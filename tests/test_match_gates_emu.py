"""The tracking matchers' gates (match_gate_cases): the oracle gives the hand-written answers, the kernel logic (emulator) gives them too and equals the oracle everywhere."""
import pytest
import match_gate_cases as mg


def test_case_contents(oracle):
    mg.check_case_contents(oracle)


@pytest.mark.parametrize('name', mg.NAMES)
def test_gate_case_emu(emu, oracle, name):
    c = mg.CASE[name]
    mg.check_kat(oracle, c)
    mg.run_case(emu, oracle, c)


@pytest.mark.parametrize('ks,nlevels', [(range(9), 8), ((7, 8), 10)])
def test_level_boundary_sweep_emu(emu, oracle, ks, nlevels):
    """L3b: PredictScale on 13 consecutive floats around every level boundary 1.2f^k"""
    assert mg.sweep(lambda c: mg.run_lib(emu, c), ks, nlevels) == mg.sweep(lambda c: mg.run_oracle(oracle, c), ks, nlevels)


def test_frame_batch_emu(emu, oracle):
    mg.check_frame_batch(emu, oracle)


def test_local_batch_emu(emu, oracle):
    mg.check_local_batch(emu, oracle)
