"""GPU: the bundle-adjustment graph query of the covisibility handle (sgx_covis_ba_graph*) of the product library against the literal restatement of
tests/ba_graph_ref.py.  Every comparison is equality of integers; there is no tolerance."""
import pytest
import ba_graph_cases as bc

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize('case', bc.hand_cases(), ids=lambda c: c['name'])
def test_hand_made_cases_gpu(gpulib, case):
    bc.run_script(gpulib, case)


@pytest.mark.parametrize('case', bc.all_generated(), ids=lambda c: c['name'])
def test_generated_cases_gpu(gpulib, case):
    """the walks of covis_cases and keyframes 1, 2, 63, 64, 65, queried after their mutations: local and global mode, pcap / ecap exactly the need and one short"""
    bc.run_script(gpulib, case)


def test_long_observation_lists_gpu(gpulib):
    """a point observed by 1, 2, 8, 9, 16, 17, 64, 65 and 257 keyframes: a chunk boundary, a wave, more than a workgroup of 256"""
    bc.run_script(gpulib, bc.long_lists_script())


@pytest.mark.parametrize('Q', [1, 3, 17])
def test_batch_equals_single_calls_on_a_side_stream_gpu(gpulib, Q):
    import torch
    bc.check_batch_equals_singles(gpulib, Q, stream=torch.cuda.Stream())


def test_error_statuses_gpu(gpulib):
    bc.check_errors(gpulib)


def test_host_pointer_entry_gpu(gpulib):
    bc.check_host_entry(gpulib)


def test_chain_through_the_solver_and_the_erase_gpu(gpulib):
    """local_ba_graph -> flatten_ba_problem -> sgx_local_bundle_adjustment -> apply_ba_erase on 6 keyframes x 60 points with gross outliers"""
    import torch
    bc.check_chain(gpulib, stream=torch.cuda.Stream())
