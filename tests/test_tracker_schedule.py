"""CPU (emulator): the tracker host issues the schedule it issued before its step was split into stage functions.  tests/golden/tracker_sync_trace.json was recorded on the
emulator from that earlier host with nothing added but the trace tap and its marks; tests/tracker_schedule_cases.py has the scenarios and the comparison.  The emulator
executes nothing asynchronously, so this — not a comparison of results — is what checks the waits and records there."""
import copy
import pytest
import tracker_schedule_cases as K


@pytest.mark.parametrize('name', K.SCENARIOS)
def test_schedule_is_the_recorded_one_emu(emu, name):
    got = K.scenario(emu, 'numpy', name, streams=(0x10, 0x20))
    d = K.difference(got, K.fixture()[name])
    assert d is None, 'scenario %s: %s' % (name, d)


def _sD_and_sE(tr):
    sD = next(e[2] for e in tr if e[1] == K.MARK and e[3] == K.M_DETECTOR); sE = next(e[2] for e in tr if e[1] == K.MARK and e[3] == K.M_ORB)
    assert sD != sE
    return sD, sE


def test_comparison_sees_a_missing_detector_wait():
    """scenario B's recorded trace without one of the extraction stream's waits for "detector done" (the first record after the detector mark)"""
    exp = K.fixture()['B']; tr = copy.deepcopy(exp)
    sD, sE = _sD_and_sE(tr)
    k = next(k for k, e in enumerate(tr) if e[1] == K.MARK and e[3] == K.M_DETECTOR and e[0] == 2)
    ev_det = next(e[3] for e in tr[k:] if e[1] == K.RECORD and e[2] == sD)
    waits = [k for k, e in enumerate(tr) if e[1] == K.WAIT and e[2] == sE and e[3] == ev_det]
    assert waits and tr[waits[0] + 1][1:] == [K.MARK, sE, K.M_MASK]          # it is the wait at the head of the mask stage
    del tr[waits[0]]
    assert K.difference(exp, exp) is None
    d = K.difference(tr, exp)
    assert d is not None and 'step 2' in d, d


def test_comparison_sees_an_early_consumed_record():
    """scenario B's recorded trace with a record of ev_consumed (the second record behind the stereo mark) moved ahead of that mark: "inputs consumed" before stereo read the depth"""
    exp = K.fixture()['B']; tr = copy.deepcopy(exp)
    sD, sE = _sD_and_sE(tr)
    m = next(k for k, e in enumerate(tr) if e[1:] == [K.MARK, sE, K.M_STEREO] and e[0] == 3)
    recs = [k for k in range(m, len(tr)) if tr[k][1] == K.RECORD and tr[k][2] == sE][:2]
    assert len(recs) == 2 and tr[recs[0]][3] != tr[recs[1]][3]
    tr.insert(m, tr.pop(recs[1]))
    d = K.difference(tr, exp)
    assert d is not None and 'step 3' in d, d
