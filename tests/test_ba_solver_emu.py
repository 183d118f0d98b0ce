"""The bundle adjustments' three solver paths under both entries on the emulator (CPU tier): cases and checks in ba_solver_cases.py."""
import pytest
import ba_solver_cases as sc


@pytest.mark.parametrize('name', sc.GLOBAL)
def test_global_ba_matches_oracle_emu(emu, oracle, name):
    sc.check_global(emu, oracle, name)


@pytest.mark.parametrize('name', sc.LOCAL_ORACLE)
def test_local_ba_matches_oracle_emu(emu, oracle, name):
    sc.check_local(emu, oracle, name)


@pytest.mark.parametrize('name,entry', sc.INIT)
def test_initialisation_independence_emu(emu, oracle, name, entry):
    sc.check_init(emu, oracle, name, entry)


@pytest.mark.parametrize('name,entry', sc.HISTORY)
def test_history_independence_emu(emu, oracle, name, entry):
    sc.check_history(emu, oracle, name, entry)
