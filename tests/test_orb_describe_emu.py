"""Describe-after-mask on the kernel-logic emulator: the extractor split into detect / describe around the erase step gives the bytes of the one-shot order
(cases and checks: orb_describe_cases.py), and the tracker gives the same results in either order."""
import pytest
import orb_describe_cases as oc


@pytest.fixture(scope='module')
def extracted(emu):
    E = oc.Extracted(emu, torch_dev=False)
    yield E
    E.close()


def test_detect_records_emu(extracted):
    oc.check_detect(extracted)


@pytest.mark.parametrize('case', oc.CASES)
def test_describe_after_erase_emu(extracted, case):
    oc.run_case(extracted, case)


def test_describe_needs_a_detect_call_emu(emu):
    """describe without a detect call before it, or with another batch size, is refused: there is no pyramid or selection list to describe from"""
    import numpy as np
    from sg_slam_amd.capi import SgxError
    from sg_slam_amd.orb import ORBextractor
    ex = ORBextractor(width=oc.W, height=oc.H, max_batch=2, lib=emu)
    cap = ex.capacity
    g = np.full((2, oc.H, oc.W), 128, np.uint8)
    k, d, n, src = np.zeros(2 * cap * 28, np.uint8), np.zeros(2 * cap * 32, np.uint8), np.zeros(2, 'i4'), np.zeros(2 * cap, 'i4')
    with pytest.raises(SgxError):
        ex.describe_batch_dev(g, oc.W, 2, src, n, k, d)
    ex.detect_batch_dev(g, oc.W, 2, k, n)
    with pytest.raises(SgxError):
        ex.describe_batch_dev(g, oc.W, 1, src, n, k, d)
    ex.describe_batch_dev(g, oc.W, 2, src, n, k, d)
    ex.extract_batch_dev(g, oc.W, 2, k, d, n)               # a one-shot extraction reuses the workspace
    with pytest.raises(SgxError):
        ex.describe_batch_dev(g, oc.W, 2, src, n, k, d)
    ex.close()


def test_tracker_describe_order_emu(emu):
    oc.run_tracker_orders(emu, pipelined=False, torch_dev=False)
