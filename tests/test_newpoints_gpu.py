"""The keyframe store and CreateNewMapPoints over it on the MI355X.  Device libm differs from the host's in the last bit (tests/test_mappoint_gpu.py), so:
(a) the batched call equals the chain of sgx_match_search_for_triangulation + sgx_triangulate_new_map_points on the same device bit for bit, and F12, baseline and the
    centres (IEEE add / mul / div / sqrt only) equal the restatement bit for bit;
(b) on cases whose compared quantities all lie at least 1e-3 relative from their thresholds (asserted on the CPU, from the restatement's own quantities) integers are
    equal and floats are within 2e-3 relative, the bound check_triangulation_step(exact=False) uses;
(c) two runs are byte-identical and the first j neighbours' outputs equal a call with j neighbours."""
import pytest
import newpoints_cases as nc
import newpoints_ref as ref

pytestmark = pytest.mark.gpu
CASES = nc.boundary_cases()


@pytest.mark.parametrize('name', list(CASES))
def test_case_against_chain_gpu(gpulib, name):
    nc.check_against_chain(gpulib, CASES[name], name)


def test_stream_keyframes_against_chain_gpu(gpulib, oracle):
    total = 0
    for seed in (0, 1):
        total += nc.check_against_chain(gpulib, nc.stream_case(oracle, seed), 'stream %d' % seed)[0]
    assert total > 50, total


@pytest.mark.parametrize('name', list(CASES))
def test_case_against_restatement_gpu(gpulib, oracle, name):
    nc.assert_margin(oracle, name, CASES[name])
    nc.check_case(gpulib, oracle, name, CASES[name], exact=False)


def test_batch_of_three_gpu(gpulib, oracle):
    nc.check_batch_of_three(gpulib, oracle, exact=False)


def test_repeat_and_prefix_gpu(gpulib):
    nc.check_prefix_and_repeat(gpulib, CASES['no_node'])
    nc.check_prefix_and_repeat(gpulib, CASES['mono_gate'])


def test_store_contract_gpu(gpulib):
    nc.check_store_contract(gpulib)


def test_driver_walk_gpu(gpulib, oracle):
    nc.check_driver_walk(gpulib, oracle, dict.fromkeys(ref.EVENTS, 0), exact=False)
