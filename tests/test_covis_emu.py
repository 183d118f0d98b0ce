"""The device covisibility graph (sgx_covis_*) on the kernel-logic emulator against the literal restatement of tests/covis_ref.py, and the restatement against hand-made
cases with written answers.  Every comparison is equality of integers."""
import pytest
import covis_cases as cc


@pytest.mark.parametrize('case', cc.hand_cases(), ids=lambda c: c['name'])
def test_hand_made_cases_have_their_written_answers(emu, case):
    cc.run_script(emu, case)
    cc.run_script(emu, case, via='single')


def test_generated_cases_cover_the_events():
    """conditions on the INPUTS, asserted of the restatement: a case set in which these never happen would let a wrong kernel pass"""
    import covis_ref
    ev = dict(gated=0, single=0, all_mode_low=0, empty=0, stage2=0, kept=0, overflow=0, bad_in_frame=0, vote=0, cascade=0, dead_listed=0, reparent=0)
    for case in cc.all_generated():
        R = covis_ref.Map(case.get('monocular', False), cc.TH_DEPTH, case['max_points'])
        for op in case['ops']:
            before = {k: R.tree(k)[0] for k in R.kfs} if op[0] == 'erasekf' else None
            out = cc.apply_ref(R, op)
            if op[0] == 'uc':
                for r in out: ev['gated'] += r[2] >= 15; ev['single'] += 0 < r[2] < 15; ev['empty'] += r[0] == 0 and r[1] == 0
            elif op[0] == 'lm':
                for f, r in zip(op[1], out):
                    ev['stage2'] += r['n_local_kf'] > r['n_stage1'] > 0; ev['kept'] += r['n_counter'] == 0; ev['overflow'] += r['status'] == -3
                    ev['bad_in_frame'] += sum(a != b for a, b in zip(f, r['frame']))
            elif op[0] == 'cull':
                for v in out: ev['vote'] += sum(x[3] for x in v)
            elif op[0] == 'cullloop': ev['cascade'] += len(out)
            elif op[0] == 'erasekf': ev['reparent'] += sum(before[k] == op[1] for k in R.kfs)
            for k in R.kfs:
                o, w = R.ordered(k)
                ev['all_mode_low'] += any(x < 15 for x in w) and len(w) > 1
                ev['dead_listed'] += any(x not in R.kfs for x in o)
    assert all(ev.values()), ev


@pytest.mark.parametrize('case', cc.all_generated(), ids=lambda c: c['name'])
def test_emulator_equals_restatement(emu, case):
    cc.run_script(emu, case, state_every=5)


def test_single_entries_equal_restatement(emu):
    cc.run_script(emu, cc.walk_script(0), via='single', state_every=20)


@pytest.mark.parametrize('nkf', [1, 2, 63, 64, 65, 120])
def test_smallest_shapes(emu, nkf):
    cc.run_script(emu, cc.shapes_script(nkf), state_every=1000)


@pytest.mark.parametrize('Q', [1, 3, 17])
def test_batch_equals_single_calls(emu, Q):
    cc.check_batch_equals_singles(emu, Q)


def test_error_statuses(emu):
    cc.check_errors(emu)


def test_erased_slots_come_back(emu):
    cc.check_slot_reuse(emu)


def test_chain_into_the_database_and_the_matcher(emu, oracle, stream_frames):
    cc.check_chain(emu, oracle, stream_frames)


def test_host_pointer_entries(emu):
    cc.check_host_entries(emu)
