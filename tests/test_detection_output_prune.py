"""Two-stage DetectionOutput (first chunk of C = 64 candidates per (frame, class), per-frame cut s*, continuation of the classes that can still reach the output) against
oracle.detector_oracle.detection_output on head outputs built to hit every branch of the cut: labels and scores equal, boxes within 1e-5, as the stress test of
tests/test_detector.py compares.  The tap sgx_det_debug_continued says how many (frame, class) pairs went through the continuation, so the cases that must exercise the
second stage (and the one that must not) are asserted to have done so.  Emulator tier and GPU tier run the same cases."""
import os
import numpy as np
import pytest
import ctypes as C
from oracle import detector_oracle as D
from sg_slam_amd.detector import Detector2D
from test_detector import PARAM, model   # noqa: F401  (fixture)

FIRST = 64          # SGX_DO_FIRST (sg_slam_amd/csrc/sgx_det_kernels.h); the boundary case also plants classes at 128 / 129 candidates
SEEDS = (0, 1)


def _setup():
    layers = D.parse_param(PARAM)
    p = [L for L in layers if L['type'] == 'DetectionOutput'][0]['p']
    pri = [D.prior_box(fh, fh, 300, L['p']) for L, fh in zip([L for L in layers if L['type'] == 'PriorBox'], (19, 10, 5, 3, 2, 1))]
    return p, np.concatenate(pri, 1)


def _plant(raw, cls, count, lo, hi, rng):
    """class `cls` gets exactly `count` candidates, scores in (lo, hi); every other prior scores 0 there"""
    raw[:, cls] = 0.0
    idx = rng.permutation(len(raw))[:count]
    raw[idx, cls] = (lo + (hi - lo) * rng.rand(count)).astype('f4')


def make_case(case, seed, n, nc):
    rng = np.random.RandomState(1000 * case + seed)
    loc = (rng.randn(n, 4) * 1.0).astype('f4')
    if case == 1:       # dense: every class far above nms_top_k candidates, the top 100 sit well inside the first chunks
        raw = rng.rand(n, nc).astype('f4') ** 3
    elif case == 2:     # scores in quarters: ties across s*, across classes and across the chunk boundary
        raw = (np.round(rng.rand(n, nc) * 4) / 4).astype('f4')
    elif case == 3:     # all scores scaled down to the threshold's neighbourhood (s* near 0.02): classes from a few candidates (below the first chunk) to beyond nms_top_k
        raw = (rng.rand(n, nc) * np.r_[0.02, np.linspace(0.0101, 0.025, nc - 1)[rng.permutation(nc - 1)]]).astype('f4')
    elif case == 4:     # one class holds all of the top 100: it continues up to nms_top_k
        raw = (rng.rand(n, nc) * 0.3).astype('f4')
        raw[:, 7] = (0.5 + 0.5 * rng.rand(n)).astype('f4')
    elif case == 5:     # classes with exactly C and exactly C + 1 candidates.  Class 4 holds the only scores above 0.9, C + 1 of them: at most C first-chunk rows reach 0.9,
        #                 fewer than keep_top_k, so s* < 0.9 and its C + 1-th candidate must come back through the continuation; class 6 (C + 1 low scores) must not
        raw = rng.rand(n, nc).astype('f4') ** 3 * np.float32(0.3)
        _plant(raw, 2, FIRST, 0.5, 0.6, rng); _plant(raw, 4, FIRST + 1, 0.9, 1.0, rng); _plant(raw, 6, FIRST + 1, 0.02, 0.03, rng)
        _plant(raw, 8, 128, 0.5, 0.6, rng); _plant(raw, 10, 129, 0.8, 0.9, rng)
    elif case == 6:     # the first chunks keep fewer than keep_top_k rows: s* undefined, the truncated class continues in full
        raw = np.zeros((n, nc), 'f4')
        _plant(raw, 9, 500, 0.05, 0.9, rng); _plant(raw, 12, 30, 0.05, 0.9, rng)
    elif case == 7:     # a class without any candidate, heavy overlaps (long suppression chains, few rows per chunk)
        loc = (rng.randn(n, 4) * 0.3).astype('f4')
        raw = rng.rand(n, nc).astype('f4') ** 3
        raw[:, 3] = 0.0
    else:
        raise ValueError(case)
    return loc, np.ascontiguousarray(raw, 'f4')


_expected = {}


def expected(case, seed, n, nc, p, priors):
    key = (case, seed)
    if key not in _expected:
        loc, conf = make_case(case, seed, n, nc)
        _expected[key] = D.detection_output(loc.reshape(-1), conf.reshape(-1), priors, p)
    return _expected[key]


def run_tap(lib, det, loc, conf):
    from sg_slam_amd.capi import DetResult
    res = (DetResult * 1)()
    lib.check(lib.tap('sgx_det_debug_detection_output')(det.h, loc.ctypes.data, conf.ctypes.data, 1, res), 'detection_output')
    cont = C.c_int(-1)
    lib.check(lib.tap('sgx_det_debug_continued')(det.h, C.byref(cont)), 'continued')
    r = res[0]
    got = np.array([[d.label, d.score, d.xmin, d.ymin, d.xmax, d.ymax] for d in r.raw[:r.n_raw]], np.float32).reshape(-1, 6)
    return got, cont.value


def run_prune_cases(lib, model):
    layers, W, blob = model
    p, priors = _setup()
    det = Detector2D(0.90, 0.01, param_text=open(PARAM).read(), bin_bytes=blob, max_batch=2, lib=lib)
    n, nc = det.num_priors, det.num_class
    nms_top_k, keep_top_k, conf_th = p[2], p[3], np.float32(p[4])
    assert priors.shape[1] == 4 * n and nms_top_k > FIRST
    for case in range(1, 8):
        for seed in SEEDS:
            loc, conf = make_case(case, seed, n, nc)
            ncand = (conf[:, 1:] > conf_th).sum(0)
            exp = expected(case, seed, n, nc, p, priors)
            got, continued = run_tap(lib, det, loc, conf)
            print('case %d seed %d: candidates per class %d..%d, rows %d, continued %d of %d classes' % (case, seed, ncand.min(), ncand.max(), len(exp), continued, nc - 1))
            assert got.shape == exp.shape, (case, seed, got.shape, exp.shape)
            assert (got[:, :2] == exp[:, :2]).all(), (case, seed)
            assert len(exp) == 0 or np.abs(got[:, 2:] - exp[:, 2:]).max() < 1e-5, (case, seed)
            # the inputs are what the case says they are, and the stage the case is about really ran
            if case == 1:
                assert ncand.min() > 4 * nms_top_k and len(exp) == keep_top_k and continued == 0, (case, seed, continued)
            if case == 2:
                assert continued >= 1, (case, seed, continued)
            if case == 3:
                assert ncand.min() <= FIRST and ncand.max() > nms_top_k and len(exp) == keep_top_k and exp[-1, 1] < 0.03, (case, seed, ncand.min(), ncand.max())
            if case == 4:
                assert continued >= 1 and (exp[:, 0] == 7).all(), (case, seed, continued)
            if case == 5:
                assert [int(ncand[c - 1]) for c in (2, 4, 6, 8, 10)] == [FIRST, FIRST + 1, FIRST + 1, 128, 129] and continued >= 1, (case, seed, continued)
            if case == 6:
                assert FIRST + ncand[11] < keep_top_k and continued == 1, (case, seed, continued)      # at most FIRST + 30 first-chunk rows; only class 9 is truncated
            if case == 7:
                assert ncand[2] == 0 and not (exp[:, 0] == 3).any()
    det.close()


def run_single_stage_arm(lib, model):
    """SGX_DET_OUT_SINGLE (tap builds): the single-stage path returns the same rows, bit for bit, and continues nothing"""
    layers, W, blob = model
    outs = []
    for single in (False, True):
        if single: os.environ['SGX_DET_OUT_SINGLE'] = '1'
        try:
            det = Detector2D(0.90, 0.01, param_text=open(PARAM).read(), bin_bytes=blob, max_batch=2, lib=lib)
        finally:
            os.environ.pop('SGX_DET_OUT_SINGLE', None)
        row = []
        for case in (2, 4, 7):
            loc, conf = make_case(case, 0, det.num_priors, det.num_class)
            rows, continued = run_tap(lib, det, loc, conf)
            assert (continued == 0) if single else (case == 7 or continued >= 1), (single, case, continued)
            row.append(rows.tobytes())
        outs.append(row)
        det.close()
    assert outs[0] == outs[1]


def test_prune_cases_emu(emu, model):
    run_prune_cases(emu, model)


def test_single_stage_arm_emu(emu, model):
    run_single_stage_arm(emu, model)


@pytest.mark.gpu
def test_prune_cases_gpu(gpulib_taps, model):
    run_prune_cases(gpulib_taps, model)


@pytest.mark.gpu
def test_single_stage_arm_gpu(gpulib_taps, model):
    run_single_stage_arm(gpulib_taps, model)
