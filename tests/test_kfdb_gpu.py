"""GPU: the device KeyFrameDatabase (sgx_kfdb_*) and the device BowVector (sgx_voc_bow_batch_dev) of the product library against the plain-Python restatement of
KeyFrameDatabase.cc (tests/kfdb_ref.py) and against the host sgx_voc_transform.  Every comparison is of bits or integers; there is no tolerance."""
import pytest
import kfdb_cases as kc
from sg_slam_amd.keyframedatabase import RELOCALIZATION, LOOP_CLOSING

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize('case', kc.hand_cases(), ids=lambda c: c['name'])
def test_hand_made_cases_gpu(gpulib, case):
    _, results = kc.run_script(gpulib, case)
    if 'expect' in case: assert results == case['expect']


@pytest.mark.parametrize('mode', [RELOCALIZATION, LOOP_CLOSING])
@pytest.mark.parametrize('seed', [0, 1, 2, 3])
def test_generated_cases_gpu(gpulib, seed, mode):
    kc.run_script(gpulib, kc.places_script(seed, mode))


@pytest.mark.parametrize('mode', [RELOCALIZATION, LOOP_CLOSING])
@pytest.mark.parametrize('N', [1, 2, 63, 64, 65, 120])
def test_smallest_shapes_gpu(gpulib, N, mode):
    """keyframe counts around the tile and wave sizes, BowVector lengths 1, 63, 64, 65, 129 and max_query_words (256) as keyframes and as queries"""
    kc.run_script(gpulib, kc.shapes_script(N, mode), max_query_words=256)


def test_single_entries_gpu(gpulib):
    for mode in (RELOCALIZATION, LOOP_CLOSING):
        kc.run_script(gpulib, kc.places_script(1, mode), via='single')
        kc.run_script(gpulib, kc.shapes_script(65, mode), via='single', max_query_words=256)


def test_container_sequences_gpu(gpulib):
    kc.run_script(gpulib, kc.container_script())
    kc.run_script(gpulib, kc.container_script(), via='single')
    kc.check_clear_forgets_reloc_scores(gpulib)


@pytest.mark.parametrize('Q', [1, 3, 17])
def test_batch_equals_single_calls_on_a_side_stream_gpu(gpulib, Q):
    import torch
    kc.check_batch_equals_singles(gpulib, Q, stream=torch.cuda.Stream())


def test_min_score_gpu(gpulib):
    kc.check_min_score(gpulib)


def test_error_statuses_gpu(gpulib):
    kc.check_errors(gpulib)


@pytest.mark.parametrize('mode', [RELOCALIZATION, LOOP_CLOSING])
def test_large_case_gpu(gpulib, mode):
    """N = 2 048 keyframes of about 600 words, 100 000 words, Q = 64 in one batch on a side stream; most of the time is the restatement's"""
    import torch
    kc.check_large(gpulib, modes=(mode,), stream=torch.cuda.Stream())


def test_bow_batch_dev_equals_transform_gpu(gpulib):
    kc.check_bow_batch(gpulib, sizes=(0, 1, 63, 64, 65, 500))


def test_bow_batch_dev_64_frames_gpu(gpulib):
    import voc_cases as vc
    sizes = tuple([1000, 1024, 0, 1, 777] + [300 + 11 * i for i in range(58)])       # 63 ragged frames and the one-word frame: B = 64, cap = 1 024
    kc.check_bow_batch(gpulib, sizes=sizes, cap=1024, vocs=[vc.make_vocabulary(9, k=10, L=4)], combos=((0, 0), (1, 2)))


def test_chain_transform_bow_detect_gpu(gpulib):
    import torch
    kc.check_chain(gpulib, stream=torch.cuda.Stream())
