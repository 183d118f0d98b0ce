"""The keyframe store and CreateNewMapPoints over it on the kernel-logic emulator against the restatement (newpoints_ref): integers for equality, F12, baseline, x3d,
normal, distances and descriptors bit for bit (same libm)."""
import pytest
import newpoints_cases as nc
import newpoints_ref as ref

EV = dict.fromkeys(ref.EVENTS, 0)
CASES = nc.boundary_cases()


@pytest.mark.parametrize('name', list(CASES))
def test_case_emu(emu, oracle, name):
    nc.check_case(emu, oracle, name, CASES[name], EV)


def test_batch_of_three_emu(emu, oracle):
    nc.check_batch_of_three(emu, oracle)


def test_repeat_and_prefix_emu(emu):
    nc.check_prefix_and_repeat(emu, CASES['no_node'])
    nc.check_prefix_and_repeat(emu, CASES['mono_gate'])


def test_chain_of_single_pair_entries_emu(emu, oracle):
    for name, case in CASES.items():
        nc.check_against_chain(emu, case, name)


def test_store_contract_emu(emu):
    nc.check_store_contract(emu)


def test_driver_walk_emu(emu, oracle):
    nc.check_driver_walk(emu, oracle, EV)


def test_every_branch_was_reached(emu, oracle):
    """of the restatement alone: every counter fired over the case set and the driver walk (the tests above, in file order)"""
    ref.check_events(EV)
