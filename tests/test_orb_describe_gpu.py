"""Describe-after-mask on the GPU: the extractor split into detect / describe around the erase step gives the bytes of the one-shot order (cases and checks:
orb_describe_cases.py), and the pipelined tracker (tap build: it carries the switch back to the old order) gives the same results in either order."""
import pytest
import orb_describe_cases as oc

pytestmark = pytest.mark.gpu


@pytest.fixture(scope='module')
def extracted(gpulib):
    E = oc.Extracted(gpulib, torch_dev=True)
    yield E
    E.close()


def test_detect_records_gpu(extracted):
    oc.check_detect(extracted)


@pytest.mark.parametrize('case', oc.CASES)
def test_describe_after_erase_gpu(extracted, case):
    oc.run_case(extracted, case)


def test_tracker_describe_order_gpu(gpulib_taps):
    oc.run_tracker_orders(gpulib_taps, pipelined=True, torch_dev=True)
