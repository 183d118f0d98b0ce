"""Loop closing on the covisibility handle (sgx_covis_add_loop_edge, sgx_covis_loop_begin, sgx_covis_loop_connections, sgx_covis_essential_graph) on the kernel-logic
emulator against the literal restatement of tests/loop_ref.py, and the restatement against hand-made cases with written answers.  Integers are compared for equality, Sim3
outputs, poses and corrected points for equality of bits."""
import pytest
import loop_cases as lc


@pytest.mark.parametrize('case', lc.hand_cases(), ids=lambda c: c['name'])
def test_hand_made_cases_have_their_written_answers(emu, case):
    lc.run_script(emu, case)


def test_generated_cases_cover_the_events():
    """conditions on the INPUTS, asserted of the restatement alone: a case set in which these never happen would let a wrong kernel pass"""
    ev = dict.fromkeys(lc.lr.EVENTS, 0)
    for case in lc.all_generated(): lc.run_script(None, case, ev=ev)      # the restatement alone over what test_emulator_equals_restatement plays
    assert all(ev[k] for k in lc.REQUIRED), ev


@pytest.mark.parametrize('case', lc.all_generated(), ids=lambda c: c['name'])
def test_emulator_equals_restatement(emu, case):
    lc.run_script(emu, case)


def test_two_runs_are_byte_identical(emu):
    lc.check_two_runs_identical(emu)


def test_error_statuses(emu):
    lc.check_errors(emu)


def test_sim3_glue_equals_the_scalar_restatement_bit_for_bit(emu):
    """sgx_loop_propagate_sim3, sgx_eg_flatten, sgx_eg_recover and sgx_correct_map_points[_dev] against the scalar float64 / float32 restatement: equality of bits, no
    tolerance; groups of 1, 2, 5, 65 and 257, rotations that take every branch of the matrix-to-quaternion conversion, every edge kind, a scale that is not 1"""
    lc.check_sim3_glue(emu)


def test_correct_loop_on_a_ring_of_40_keyframes(emu, oracle):
    lc.check_chain(emu, oracle)
