"""PnPsolver on the MI355X: the device against the float64 restatement (tests/pnp_ref.py) on the emulator's cases, the batch against single device solvers, and
512 x 16 solvers in one batch against the emulator on a fixed sample, all bit for bit."""
import numpy as np
import pytest
import pnp_cases as pc
import pnp_ref as ref
from sg_slam_amd.pnpsolver import PnPsolver, PnPsolverBatch, RELOCALIZATION_RANSAC

pytestmark = pytest.mark.gpu


def test_device_equals_restatement(gpulib):
    """same found, bNoMore, iterations run, inlier flags, nInliers and Tcw bits: the kernels use correctly rounded fp64 operations only (sgx_pnp_hypot)"""
    for c in pc.CASES: pc.run_case(gpulib, c, exact=True)


def test_device_batch_equals_single(gpulib):
    cases = [c for c in pc.CASES if c[1] >= 15][:10]
    pc.check_batch_equals_single(gpulib, cases)


def test_batch_8192_solvers_against_emulator_sample(gpulib, emu):
    B = 512 * 16
    rng = np.random.RandomState(5)
    ns = rng.randint(15, 301, B)
    data = [pc.make_case(10000 + b, int(ns[b]), 0.3)[:3] for b in range(B)]
    Bt = PnPsolverBatch(B, int(ns.sum()), lib=gpulib)
    Bt.set([(d[0], d[1], d[2], pc.CAM) for d in data], RELOCALIZATION_RANSAC, rand_seeds=np.arange(B))
    res, T, inl = Bt.iterate(5)
    assert res[:, 0].sum() > 0.5 * B
    for b in np.linspace(0, B - 1, 64).astype(int):
        d = data[b]
        S = PnPsolver(d[0], d[1], d[2], pc.CAM, rand_seed=int(b), lib=emu); S.SetRansacParameters(*RELOCALIZATION_RANSAC)
        gT, gnm, ginl, gni, grun = S.iterate(5)
        assert res[b, 0] == (gT is not None) and res[b, 1] == gnm and res[b, 2] == gni and res[b, 3] == grun, (b, res[b], gnm, gni, grun)
        assert (inl[b] == ginl).all()
        if gT is not None: assert (T[b].view('u4') == gT.view('u4')).all(), b
        S.close()
    Bt.close()


def test_device_defined_undefined_behaviour(gpulib_taps):
    """the two defined undefined behaviours of the device EPnP (no update on a singular qr_solve, IEEE division by a zero beta), through the test tap"""
    pc.check_defined_ub(gpulib_taps)


def test_device_batch_with_caller_draws_equals_single(gpulib):
    cases = [c for c in pc.CASES if c[1] >= 15][:6]
    pc.check_batch_equals_single(gpulib, cases, caller_draws=True)


def test_device_call_longer_than_one_chunk(gpulib):
    """1000 hypotheses in one call: two launches of the kernels, against the restatement"""
    p2d, s2, p3, R, t, bad = pc.make_case(4000, 400, 0.95)
    S = PnPsolver(p2d, s2, p3, pc.CAM, lib=gpulib); O = ref.PnPsolverRef(p2d, s2, p3, pc.CAM)
    ransac = (0.99, 30, 1000, 4, 0.02, 5.991)
    S.SetRansacParameters(*ransac); O.set_ransac_parameters(*ransac)
    d = pc.glibc_rand(9, 4 * 1100)
    g = S.iterate(5, d); e = O.iterate(5, d)
    assert g[4] == e[4] == 1000 and g[1] == e[1] and (g[0] is None) == (e[0] is None) and g[3] == e[3] and (g[2] == e[2]).all()
    if e[0] is not None: assert (g[0].view('u4') == e[0].view('u4')).all()
