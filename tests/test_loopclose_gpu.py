"""Loop closing on the covisibility handle on the device against the literal restatement of tests/loopclose_ref.py, and the restatement against hand-made
cases with written answers: DetectLoop's consistency groups and GetConnectedKeyFrames (sgx_covis_consistency*, sgx_covis_get_consistent_groups,
sgx_covis_connected_batch*), every comparison equality of integers; the map update after global BA (sgx_covis_gba_update*, sgx_gba_correct_points_dev) on the trees
of loopclose_cases, Tcw_out / TcwBef / xw_out for equality of bits; and the driver sg_slam_amd.loopclosing.LoopClosing on a ring of 40 keyframes (DetectLoop,
CorrectLoop, RunGlobalBundleAdjustment with the solver)."""
import pytest

pytestmark = pytest.mark.gpu
import loopclose_cases as lc



@pytest.mark.parametrize('case', lc.HAND, ids=lambda c: c.__name__)
def test_hand_made_cases(gpulib, case):
    case(gpulib, dict.fromkeys(lc.ref.EVENTS, 0))


@pytest.mark.parametrize('seed', lc.SEEDS)
def test_walks_equal_the_restatement(gpulib, seed):
    lc.case_walk(gpulib, dict.fromkeys(lc.ref.EVENTS, 0), seed)


def test_two_runs_are_byte_identical(gpulib):
    lc.check_two_runs_identical(gpulib)


@pytest.mark.parametrize('case', lc.GBA, ids=lambda c: c.__name__)
def test_gba_map_update_equals_the_restatement_bit_for_bit(gpulib, case):
    """Tcw_out, TcwBef and xw_out for equality of bits, no tolerance; a refused call leaves the poison pattern everywhere"""
    case(gpulib, dict.fromkeys(lc.ref.GBA_EVENTS, 0))


def test_gba_two_runs_are_byte_identical(gpulib):
    lc.check_gba_two_runs_identical(gpulib)


def test_driver_on_a_ring_of_40_keyframes(gpulib):
    lc.check_driver_chain(gpulib)
