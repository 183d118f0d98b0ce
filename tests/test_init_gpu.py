"""Initializer on the MI355X: the device against the restatement (tests/init_ref.py) on the emulator's cases, the batch against single device initializers, and 512
frame pairs in one batch against the emulator on a fixed sample, all bit for bit."""
import numpy as np
import pytest
import init_cases as ic
from sg_slam_amd.initializer import Initializer, InitializerBatch

pytestmark = pytest.mark.gpu


def test_device_equals_restatement(gpulib):
    """same ok, R21 / t21 / p3d bits, triangulated, inliers, scores, model, nGood, selected cosines, best hypothesis, H21 / F21: correctly rounded operations only"""
    for c in ic.CASES: ic.run_case(gpulib, c[0])


def test_device_batch_equals_single(gpulib):
    ic.check_batch_equals_single(gpulib, [c[0] for c in ic.CASES if c[2] == 200])


def test_device_batch_with_caller_draws_equals_single(gpulib):
    ic.check_batch_equals_single(gpulib, [c[0] for c in ic.CASES if c[2] == 200][:8], caller_draws=True)


def test_device_second_frame_with_more_keys_continues_the_replica(gpulib):
    ic.check_regrow_carries_replica(gpulib)


def test_device_call_longer_than_one_chunk(gpulib):
    """300 iterations: two launches of the hypothesis kernels"""
    c = next(c for c in ic.CASES if c[0] == 'general_300_its300'); assert c[2] > 256
    ic.run_case(gpulib, c[0])
    ic.check_batch_equals_single(gpulib, [c[0]])


def test_batch_512_pairs_against_emulator_sample(gpulib, emu):
    B = 512
    rng = np.random.RandomState(11); ns = rng.randint(100, 401, B)
    kw = lambda b: (dict(seed=1000 + b, n=int(ns[b]), noise=0.2, outliers=0.1, unmatched=0.1) if b % 2 == 0 else
                    dict(seed=1000 + b, n=int(ns[b]), scene='planar', noise=0.2, baseline=1.0, tseed=64, extra2=b % 7))
    scs = [ic.make_scene(**kw(b)) for b in range(B)]
    n1 = sum(len(s[0]) for s in scs); n2 = sum(len(s[1]) for s in scs)
    Bt = InitializerBatch(B, max(n1, n2), n1, 200, lib=gpulib)
    Bt.set([(s[0], s[1], s[2], ic.CAM) for s in scs])
    res = Bt.run(rand_seeds=np.arange(B))
    ok_h = sum(1 for r in res if r[0] and r[6]['model'] == 0); ok_f = sum(1 for r in res if r[0] and r[6]['model'] == 1)
    assert ok_h > B // 8 and ok_f > B // 8, (ok_h, ok_f)
    for b in np.linspace(0, B - 1, 32).astype(int):
        s = scs[b]
        S = Initializer(s[0], ic.CAM, 1.0, 200, rand_seed=int(b), lib=emu)
        ic.assert_same(res[b], S.Initialize(s[1], s[2]), int(b))
        S.close()
    Bt.close()
