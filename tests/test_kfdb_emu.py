"""The device KeyFrameDatabase (sgx_kfdb_*) and the device BowVector (sgx_voc_bow_batch_dev) on the kernel-logic emulator, against the plain-Python restatement of
KeyFrameDatabase.cc in tests/kfdb_ref.py and against the host sgx_voc_transform.  Every comparison is of bits or integers."""
import ctypes as C
import numpy as np
import pytest
import kfdb_ref
import kfdb_cases as kc
from sg_slam_amd.keyframedatabase import RELOCALIZATION, LOOP_CLOSING


def test_restatement_score_is_the_library_score(emu, oracle):
    rng = np.random.RandomState(0)
    voc = kc.make_voc(emu, 3000)
    for _ in range(40):
        a = kc.bow_of(rng.randint(0, 3000, rng.randint(1, 400)), rng=rng); b = kc.bow_of(rng.randint(0, 3000, rng.randint(1, 400)), rng=rng)
        s = kfdb_ref.l1_score(a, b)
        assert s == voc.score(a, b) == oracle.bow_score_l1(a, b)
    voc.close()


@pytest.mark.parametrize('case', kc.hand_cases(), ids=lambda c: c['name'])
def test_hand_made_cases_have_their_written_answers(emu, case):
    R, results = kc.run_script(emu, case)
    if 'expect' in case: assert results == case['expect']
    kc.run_script(emu, case, via='single')
    # the reports of the restatement, which run_script has compared with the device's bit for bit
    if 'expect_report' in case:
        R2 = kfdb_ref.KeyFrameDatabase(case['nwords']); k = 0
        for op in case['ops']:
            if op[0] == 'add': R2.add(op[1], op[2])
            elif op[0] == 'cov': R2.set_covisibility(op[1], op[2])
            elif op[0] == 'erase': R2.erase(op[1])
            elif op[0] in ('reloc', 'loop'):
                R2.DetectRelocalizationCandidates(op[1]) if op[0] == 'reloc' else R2.DetectLoopCandidates(op[1], op[2], op[3])
                for key, v in case['expect_report'][k].items(): assert R2.report[key] == v, (case['name'], k, key, R2.report[key], v)
                k += 1
    if case.get('stale_matters'):
        assert kc.reloc_results_with_zeroed_stale(case) == [[2], [1]]


def test_generated_cases_cover_the_events():
    """conditions on the INPUTS, asserted of the restatement: a case set in which these never happen would let a wrong kernel pass"""
    two = nb = dedup = stale = empty = stale_changes = 0
    for case in kc.all_generated():
        if case['ops'][-1][0] == 'reloc':
            R, out = kc.reloc_results(case)
            stale_changes += kc.reloc_results_with_zeroed_stale(case) != out
        else:
            R = kfdb_ref.KeyFrameDatabase(case['nwords']); out = []
            for op in case['ops']:
                if op[0] == 'add': R.add(op[1], op[2])
                elif op[0] == 'cov': R.set_covisibility(op[1], op[2])
                elif op[0] == 'loop': out.append(R.DetectLoopCandidates(op[1], op[2], op[3] if op[3] is not None else R.min_score(op[1], op[2])))
        two += sum(len(o) >= 2 for o in out); empty += sum(len(o) == 0 for o in out)
        nb += R.events['best_is_neighbour']; dedup += R.events['dedup']; stale += R.events['stale_nonzero']
    assert two and nb and dedup and stale and empty and stale_changes, (two, nb, dedup, stale, empty, stale_changes)


@pytest.mark.parametrize('case', kc.all_generated(), ids=lambda c: c['name'])
def test_emulator_equals_restatement(emu, case):
    kc.run_script(emu, case)


def test_single_entries_equal_restatement(emu):
    for case in (kc.places_script(1, RELOCALIZATION), kc.places_script(1, LOOP_CLOSING)):
        kc.run_script(emu, case, via='single')


def test_container_sequences(emu):
    case = kc.container_script()
    assert sum(len(o[2][0]) for o in case['ops'] if o[0] == 'add') > 2 * case['max_bow_entries']      # more is added in total than the pool holds
    kc.run_script(emu, case)
    kc.run_script(emu, case, via='single')


@pytest.mark.parametrize('Q', [1, 3, 17])
def test_batch_equals_single_calls(emu, Q):
    kc.check_batch_equals_singles(emu, Q)


def test_min_score(emu):
    kc.check_min_score(emu)


def test_error_statuses(emu):
    kc.check_errors(emu)


def test_vocabulary_scoring_must_be_l1(emu):
    v = kc.make_voc(emu, 50, scoring=1)
    h = C.c_void_p()
    assert emu.dll.sgx_kfdb_create(v.h, 4, 100, 0, 1, C.byref(h)) == -2 and not h.value
    v.close()


def test_bow_batch_dev_equals_transform(emu):
    kc.check_bow_batch(emu, sizes=(0, 1, 63, 64, 65, 500))


def test_clear_forgets_reloc_scores(emu):
    kc.check_clear_forgets_reloc_scores(emu)


def test_chain_transform_bow_detect(emu):
    kc.check_chain(emu)


def test_smallest_shapes(emu):
    for mode in (RELOCALIZATION, LOOP_CLOSING):
        kc.run_script(emu, kc.shapes_script(65, mode), max_query_words=256)
