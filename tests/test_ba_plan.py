"""The bundle adjustment's solver plan (sgx_ba_debug_last_plan: envelope solver or dense, first branch, second branch, separator) for a matrix of problem sizes x
solver mode x SGX_BA_TWIST: the regression guard of the planner (plan_solver, sgx_ba_plan.h).

Optimizer.BundleAdjustment(..., nIterations=0) plans and allocates but runs no LM iteration.  The four integers must equal tests/golden/ba_plans.json.  A planner change
that is meant to change a plan updates the fixture on purpose:
    python tests/test_ba_plan.py            (records from the emulator)"""
import ctypes as C
import json
import os
import sys
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FIXTURE = os.path.join(ROOT, 'tests', 'golden', 'ba_plans.json')
SIZES = ((60, 1500, False), (150, 3600, False), (171, 4000, True), (400, 10000, False), (600, 15000, False), (2000, 50000, False))      # keyframes, landmarks, open_trajectory
SOLVERS = (-1, 1, 2)          # sgx_ba_debug_set_solver: automatic, dense, envelope solver forced
TWISTS = ('1', '0')           # SGX_BA_TWIST: two-branch ordering allowed / one branch


def plans_of(lib):
    from scenes import make_big_ba_problem, CAM
    from test_localba import open_trajectory
    from sg_slam_amd.optimizer import Optimizer
    out = {}
    twist_before = os.environ.get('SGX_BA_TWIST')
    try:
        for nkf, npt, open_ends in SIZES:
            prob, _, _ = make_big_ba_problem(nkf, npt)
            if open_ends: prob = open_trajectory(prob, nkf)
            for solver in SOLVERS:
                for twist in TWISTS:
                    os.environ['SGX_BA_TWIST'] = twist
                    lib.tap('sgx_ba_debug_set_solver')(solver)
                    Optimizer.BundleAdjustment(dict(prob), CAM, nIterations=0, lib=lib)
                    pl = (C.c_int32 * 4)(); lib.check(lib.tap('sgx_ba_debug_last_plan')(pl))
                    out['nkf=%d npt=%d%s solver=%d twist=%s' % (nkf, npt, ' open' if open_ends else '', solver, twist)] = [int(v) for v in pl]
    finally:
        lib.tap('sgx_ba_debug_set_solver')(-1)
        if twist_before is None: os.environ.pop('SGX_BA_TWIST', None)
        else: os.environ['SGX_BA_TWIST'] = twist_before
    return out


def check(lib):
    fx = json.load(open(FIXTURE))
    got = plans_of(lib)
    assert sorted(got) == sorted(fx) and len(got) == len(SIZES) * len(SOLVERS) * len(TWISTS)
    for key, plan in got.items():
        assert plan == fx[key], (key, plan, fx[key])


def test_plans_equal_fixture_emu(emu):
    check(emu)


@pytest.mark.gpu
def test_plans_equal_fixture_gpu(gpulib_taps):
    check(gpulib_taps)


if __name__ == '__main__':
    sys.path.insert(0, ROOT)
    from sg_slam_amd.capi import SgxLib
    got = plans_of(SgxLib(sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, 'tests', 'emu', 'libsgx_emu.so')))
    with open(sys.argv[2] if len(sys.argv) > 2 else FIXTURE, 'w') as f:
        f.write('{\n' + ',\n'.join('%s: %s' % (json.dumps(k), json.dumps(v)) for k, v in sorted(got.items())) + '\n}\n')
    print('%d cases, %d with the envelope solver, %d with two branches' % (len(got), sum(p[0] for p in got.values()), sum(p[2] > 0 for p in got.values())))
