"""GPU: loop closing on the covisibility handle (sgx_covis_add_loop_edge, sgx_covis_loop_begin, sgx_covis_loop_connections, sgx_covis_essential_graph) of the product
library against the literal restatement of tests/loop_ref.py.  Integers are compared for equality, Sim3 outputs, poses and corrected points for equality of bits; the one
tolerance is that of the optimiser against the oracle in the chain test."""
import pytest
import loop_cases as lc

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize('case', lc.hand_cases(), ids=lambda c: c['name'])
def test_hand_made_cases_gpu(gpulib, case):
    lc.run_script(gpulib, case)


@pytest.mark.parametrize('case', lc.all_generated(), ids=lambda c: c['name'])
def test_generated_cases_gpu(gpulib, case):
    """walks with loops closed between a new and an early keyframe, the drop-reason scenario, groups of 1, 2, 63, 64, 65 and 257, maps of 1, 2 and 300 keyframes, edge
    totals of 255, 256 and 257, every capacity at the need and one short"""
    import torch
    lc.run_script(gpulib, case, stream=torch.cuda.Stream())


def test_two_runs_are_byte_identical_gpu(gpulib):
    lc.check_two_runs_identical(gpulib)


def test_error_statuses_gpu(gpulib):
    lc.check_errors(gpulib)


def test_sim3_glue_equals_the_scalar_restatement_bit_for_bit_gpu(gpulib):
    """equality of bits against the scalar float64 / float32 restatement of tests/loop_ref.py; no tolerance"""
    lc.check_sim3_glue(gpulib)


def test_correct_loop_on_a_ring_of_40_keyframes_gpu(gpulib, oracle):
    """the flattened problem equals the restatement's bit for bit; the optimised poses agree with the oracle's optimiser fed the same arrays (1e-5 with fixed scale,
    iteration count +- 1, the criteria of sim3_cases.check_eg)"""
    import torch
    lc.check_chain(gpulib, oracle, stream=torch.cuda.Stream())
