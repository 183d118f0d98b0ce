"""GPU: the device covisibility graph (sgx_covis_*) of the product library against the literal restatement of tests/covis_ref.py.  Every comparison is equality of
integers; there is no tolerance."""
import pytest
import covis_cases as cc

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize('case', cc.hand_cases(), ids=lambda c: c['name'])
def test_hand_made_cases_gpu(gpulib, case):
    cc.run_script(gpulib, case)


@pytest.mark.parametrize('case', cc.all_generated(), ids=lambda c: c['name'])
def test_generated_cases_gpu(gpulib, case):
    cc.run_script(gpulib, case, state_every=10)


def test_single_entries_gpu(gpulib):
    cc.run_script(gpulib, cc.walk_script(0), via='single', state_every=50)


@pytest.mark.parametrize('nkf', [1, 2, 63, 64, 65, 120])
def test_smallest_shapes_gpu(gpulib, nkf):
    """keyframes 1, 2, 63, 64, 65, 120 holding 0, 1, 63, 64, 65 and cap points; observation lists from 1 and 2 up to the number of keyframes that see point 0"""
    cc.run_script(gpulib, cc.shapes_script(nkf), state_every=1000)


@pytest.mark.parametrize('Q', [1, 3, 17])
def test_batch_equals_single_calls_on_a_side_stream_gpu(gpulib, Q):
    import torch
    cc.check_batch_equals_singles(gpulib, Q, stream=torch.cuda.Stream())


def test_large_case_gpu(gpulib):
    """512 keyframes x 1 000 points, Q = 64 in one batch on a side stream; most of the time is the restatement's"""
    import torch
    cc.check_large(gpulib, stream=torch.cuda.Stream())


def test_error_statuses_gpu(gpulib):
    cc.check_errors(gpulib)


def test_erased_slots_come_back_gpu(gpulib):
    cc.check_slot_reuse(gpulib)


def test_chain_into_the_database_and_the_matcher_gpu(gpulib, oracle, stream_frames):
    import torch
    cc.check_chain(gpulib, oracle, stream_frames, stream=torch.cuda.Stream())


def test_host_pointer_entries_gpu(gpulib):
    cc.check_host_entries(gpulib)
