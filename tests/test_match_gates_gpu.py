"""The tracking matchers' gates (match_gate_cases) on the device: the product library gives the hand-written answers and equals the oracle everywhere."""
import pytest
import match_gate_cases as mg

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize('name', mg.NAMES)
def test_gate_case_gpu(gpulib, oracle, name):
    mg.run_case(gpulib, oracle, mg.CASE[name])


@pytest.mark.parametrize('ks,nlevels', [(range(9), 8), ((7, 8), 10)])
def test_level_boundary_sweep_gpu(gpulib, oracle, ks, nlevels):
    """L3b: the device's PredictScale against glibc's ceilf(logf(ratio) / log_scale_factor) on 13 consecutive floats around every level boundary 1.2f^k"""
    got = mg.sweep(lambda c: mg.run_lib(gpulib, c), ks, nlevels); want = mg.sweep(lambda c: mg.run_oracle(oracle, c), ks, nlevels)
    bad = [(k, float(r), g, w) for (k, r), g, w in zip(mg.sweep_ratios(ks), got, want) if g != w]
    print('L3b nlevels %d: %d of %d ratios disagree' % (nlevels, len(bad), len(got)), bad)
    assert not bad


def test_frame_batch_gpu(gpulib, oracle):
    """F9: sgx_match_project_frame_batch_dev on a stream of its own"""
    mg.check_frame_batch(gpulib, oracle)


def test_local_batch_gpu(gpulib, oracle):
    """L6: sgx_match_project_local_batch_dev on a stream of its own"""
    mg.check_local_batch(gpulib, oracle)
