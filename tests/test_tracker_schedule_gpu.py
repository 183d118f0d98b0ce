"""GPU (MI355X): the device build of the tracker host issues the schedule of tests/golden/tracker_sync_trace.json — the scenarios, sizes, frames and comparison of
tests/test_tracker_schedule.py, on the tap library, with torch streams as the caller's.  Five steps reach every edge: the triple buffer wraps at step 3, the detector's
double buffer at step 2, and the wait for a record pack needs the pack two steps before the slot is reused."""
import pytest
import tracker_schedule_cases as K

pytestmark = pytest.mark.gpu


def test_schedule_is_the_recorded_one_gpu(gpulib_taps):
    import torch
    s1, s2 = torch.cuda.Stream(), torch.cuda.Stream()
    expected = K.fixture()
    for name in K.SCENARIOS:
        got = K.scenario(gpulib_taps, 'torch', name, streams=(s1.cuda_stream, s2.cuda_stream))
        torch.cuda.synchronize()
        d = K.difference(got, expected[name])
        assert d is None, 'scenario %s: %s' % (name, d)
