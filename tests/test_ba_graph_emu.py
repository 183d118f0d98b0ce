"""The bundle-adjustment graph query of the covisibility handle (sgx_covis_ba_graph*) on the kernel-logic emulator against the literal restatement of
tests/ba_graph_ref.py, and the restatement against hand-made cases with written answers.  Every comparison is equality of integers."""
import pytest
import ba_graph_cases as bc


@pytest.mark.parametrize('case', bc.hand_cases(), ids=lambda c: c['name'])
def test_hand_made_cases_have_their_written_answers(emu, case):
    bc.run_script(emu, case)


def test_generated_cases_cover_the_events():
    """conditions on the INPUTS, asserted of the restatement: a case set in which these never happen would let a wrong kernel pass"""
    ev = dict.fromkeys(bc.br.EVENTS, 0)
    for case in bc.all_generated(): bc.run_script(None, case, ev=ev)      # the restatement alone over what test_emulator_equals_restatement plays
    assert all(ev.values()), ev


@pytest.mark.parametrize('case', bc.all_generated(), ids=lambda c: c['name'])
def test_emulator_equals_restatement(emu, case):
    bc.run_script(emu, case)


def test_long_observation_lists(emu):
    """a point observed by 1, 2, 8, 9, 16, 17, 64, 65 and 257 keyframes"""
    bc.run_script(emu, bc.long_lists_script())


@pytest.mark.parametrize('Q', [1, 3, 17])
def test_batch_equals_single_calls(emu, Q):
    bc.check_batch_equals_singles(emu, Q)


def test_error_statuses(emu):
    bc.check_errors(emu)


def test_host_pointer_entry(emu):
    bc.check_host_entry(emu)


def test_chain_through_the_solver_and_the_erase(emu):
    bc.check_chain(emu)
