"""The detector's execution plan as text, for every combination of the plan-selection taps: the regression guard of the planner (sgx_det_create).

Detector2D.op_descriptions() over fuse x legacy_kernels x block_fusion x irb x gemm x max_batch = 96 handles must equal tests/golden/detector_plans.json line by line.
The fixture holds the distinct plans once and, per handle, which of them it gets.  A planner change that is meant to change a plan updates the fixture on purpose:
    python tests/test_detector_plan.py            (records from the emulator)
max_batch 512 is left out: an unfused handle keeps every blob of every image."""
import itertools
import json
import os
import sys
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PARAM = os.path.join(ROOT, 'tests', 'golden', 'mobilenetv3_ssdlite_voc.param')
FIXTURE = os.path.join(ROOT, 'tests', 'golden', 'detector_plans.json')
AXES = (('fuse', (True, False)), ('legacy_kernels', (False, True)), ('block_fusion', (False, True)), ('irb', (None, 0, 2)), ('gemm', ('f32', 'bf16x3')), ('max_batch', (1, 2)))


def handles():
    for values in itertools.product(*(v for _, v in AXES)):
        kw = dict(zip((k for k, _ in AXES), values))
        yield ' '.join('%s=%s' % (k, kw[k]) for k, _ in AXES), kw


def plans_of(lib):
    from oracle import detector_oracle as D
    from sg_slam_amd.detector import Detector2D
    _, blob = D.synth_weights(D.parse_param(PARAM), seed=7)
    text = open(PARAM).read()
    out = {}
    for key, kw in handles():
        det = Detector2D(0.90, 0.01, param_text=text, bin_bytes=blob, lib=lib, **kw)
        out[key] = det.op_descriptions()
        assert len(out[key]) == det.num_kernels, key
        det.close()
    return out


def check(lib):
    fx = json.load(open(FIXTURE))
    got = plans_of(lib)
    assert sorted(got) == sorted(fx['handles']) and len(got) == 96
    for key, lines in got.items():
        want = fx['plans'][fx['handles'][key]]
        assert len(lines) == len(want), (key, len(lines), len(want))
        for i, (a, b) in enumerate(zip(lines, want)):
            assert a == b, (key, i, a, b)


def test_plans_equal_fixture_emu(emu):
    check(emu)


@pytest.mark.gpu
def test_plans_equal_fixture_gpu(gpulib_taps):
    check(gpulib_taps)


if __name__ == '__main__':
    sys.path.insert(0, ROOT)
    from sg_slam_amd.capi import SgxLib
    got = plans_of(SgxLib(sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, 'tests', 'emu', 'libsgx_emu.so')))
    plans, index = [], {}
    for key, lines in got.items():
        if lines not in plans: plans.append(lines)
        index[key] = plans.index(lines)
    with open(sys.argv[2] if len(sys.argv) > 2 else FIXTURE, 'w') as f:
        json.dump({'plans': plans, 'handles': index}, f, indent=0, sort_keys=True)
        f.write('\n')
    print('%d handles, %d distinct plans of %s steps' % (len(got), len(plans), sorted(set(len(p) for p in plans))))
