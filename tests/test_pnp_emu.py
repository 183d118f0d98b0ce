"""PnPsolver (Tracking::Relocalization's EPnP RANSAC): the float64 restatement (tests/pnp_ref.py) against numpy.linalg, EPnP on noiseless data, then the kernel-logic
emulator against the restatement bit for bit, the quirks of PnPsolver::iterate, the two defined undefined behaviours, and the batch against single solvers."""
import numpy as np
import pytest
import pnp_cases as pc
import pnp_ref as ref
from sg_slam_amd.pnpsolver import PnPsolver, PnPsolverBatch, DEFAULT_RANSAC, RELOCALIZATION_RANSAC

CAM = tuple(float(c) for c in pc.CAM)


def test_restated_svd_solve_invert_against_numpy():
    rng = np.random.RandomState(0)
    for m, n in ((12, 12), (6, 4), (6, 3), (6, 5), (3, 3)):
        A = rng.normal(size=(20, m, n))
        U, W, Vt = ref.svd(A)
        assert np.allclose(W, np.linalg.svd(A, compute_uv=False), rtol=1e-12, atol=1e-12)
        assert np.allclose(U * W[:, None, :] @ Vt, A, atol=1e-12)
        b = rng.normal(size=(20, m))
        x = ref.solve_svd(A, b)
        assert np.allclose(x, np.stack([np.linalg.lstsq(A[h], b[h], rcond=None)[0] for h in range(20)]), atol=1e-10)
    C = rng.normal(size=(20, 3, 3))
    assert np.allclose(ref.invert_svd(C), np.linalg.pinv(C), atol=1e-9)
    # MtM of rank 8 (four points): the null-space projector of the four smallest singular directions
    p2d, s2, p3, R, t, _ = pc.make_case(3, 4, 0.0)
    M = rng.normal(size=(1, 8, 12)); MtM = ref.mul_transposed(M)
    assert np.allclose(MtM[0], M[0].T @ M[0], atol=1e-12)
    U, W, Vt = ref.svd(MtM)
    Pn = Vt[0, 8:].T @ Vt[0, 8:]; w, V = np.linalg.eigh(MtM[0]); Pe = V[:, :4] @ V[:, :4].T
    assert np.allclose(Pn, Pe, atol=1e-9)


@pytest.mark.parametrize('n,planar', [(4, False), (50, False), (50, True)])     # four coplanar points: the reference's EPnP has no planar case
def test_epnp_recovers_noiseless_pose(n, planar):
    rng = np.random.RandomState(n + planar)
    R = pc.rot(rng.normal(0, 0.3, 3)); t = rng.normal(0, 0.3, 3)
    Xc = np.c_[rng.uniform(-1.5, 1.5, n), rng.uniform(-1.0, 1.0, n), rng.uniform(2.0, 6.0, n)]
    if planar: Xc[:, 2] = 3.0 + 0.3 * Xc[:, 0] - 0.2 * Xc[:, 1]
    Xw = (R.T @ (Xc - t).T).T
    fu, fv, uc, vc = CAM
    uv = np.c_[fu * Xc[:, 0] / Xc[:, 2] + uc, fv * Xc[:, 1] / Xc[:, 2] + vc]
    Rr, tr = ref.epnp(Xw[None], uv[None], CAM)
    # four points: the reference's five Gauss-Newton steps stop short of exact (observed 3e-5 / 5e-4 on one case); 50 points: exact to 1e-9
    tol = 1e-3 if n == 4 else 1e-9
    assert np.abs(Rr[0] - R).max() < tol and np.abs(tr[0] - t).max() < tol, (np.abs(Rr[0] - R).max(), np.abs(tr[0] - t).max())


def test_glibc_rand_replica(emu):
    """find() with the solver's own replica == the restatement fed with this machine's libc rand() after srand(seed)"""
    for seed in (0, 1, 12345):
        p2d, s2, p3, R, t, bad = pc.make_case(50 + seed, 120, 0.5)
        S = PnPsolver(p2d, s2, p3, pc.CAM, rand_seed=seed, lib=emu); O = ref.PnPsolverRef(p2d, s2, p3, pc.CAM)
        S.SetRansacParameters(*RELOCALIZATION_RANSAC); O.set_ransac_parameters(*RELOCALIZATION_RANSAC)
        g = S.find(); e = O.iterate(O.max_its, pc.glibc_rand(seed, 4 * O.max_its))
        assert (g[0] is None) == (e[0] is None) and g[1:2] + g[3:] == e[1:2] + e[3:] and (g[2] == e[2]).all()
        if e[0] is not None: assert (g[0] == e[0]).all()
        # draws of hypotheses that did not run are handed back: the next call continues the libc sequence after 4 x iterations run
        d = pc.glibc_rand(seed, 4 * (e[4] + 400))[4 * e[4]:]
        g2 = S.iterate(5); e2 = O.iterate(5, d)
        assert g2[4] == e2[4] and g2[3] == e2[3] and (g2[2] == e2[2]).all()
        S.close()


@pytest.mark.parametrize('k', range(0, 28, 4))
def test_emulator_equals_restatement(emu, k):
    """28 seeded cases (N 4 .. 400, 0 .. 70 % outliers, both parameter sets) x iterate(5) until a model or bNoMore: Tcw bits, found, bNoMore, iterations, inliers"""
    for c in pc.CASES[k:k + 4]: pc.run_case(emu, c)


def test_emulator_equals_restatement_more_cases(emu):
    """24 more cases with other seeds, find() style calls, and iterate(1) / iterate(50) calls"""
    n_found = 0
    for i in range(24):
        n = [15, 30, 60, 120, 250, 400][i % 6]; out = [0.1, 0.3, 0.5, 0.6][i % 4]
        calls, O = pc.run_case(emu, (900 + i, n, out, RELOCALIZATION_RANSAC if i % 2 else DEFAULT_RANSAC, [1, 5, 50][i % 3], 300 + i))
        n_found += O.best > 0
    assert n_found >= 12


def _solver_pair(lib, seed, n, out, ransac):
    p2d, s2, p3, R, t, bad = pc.make_case(seed, n, out)
    S = PnPsolver(p2d, s2, p3, pc.CAM, lib=lib); O = ref.PnPsolverRef(p2d, s2, p3, pc.CAM)
    S.SetRansacParameters(*ransac); O.set_ransac_parameters(*ransac)
    return S, O


def test_quirk_or_loop_runs_max_iterations_on_first_call(emu):
    """`mnIterations < mRansacMaxIts || nCurrent < nIterations`: iterate(5) runs mRansacMaxIts hypotheses when nothing succeeds, then iterate(5) runs 5 more"""
    S, O = _solver_pair(emu, 7, 40, 0.9, RELOCALIZATION_RANSAC)
    d = pc.glibc_rand(3, 4 * 2000)
    g = S.iterate(5, d); e = O.iterate(5, d)
    assert g[4] == e[4] == O.max_its > 5 and g[1] and e[1]
    g = S.iterate(5, d); e = O.iterate(5, d)
    assert g[4] == e[4] == 5 and S.state()['iterations'] == O.its == O.max_its + 5


def test_quirk_n_below_min_inliers_and_n_equal(emu):
    S, O = _solver_pair(emu, 8, 9, 0.0, RELOCALIZATION_RANSAC)           # N = 9 < minInliers 10: bNoMore at once, nothing consumed
    g = S.iterate(5, np.zeros(40, 'i4'))
    assert g[0] is None and g[1] and g[4] == 0 and S.state()['iterations'] == 0
    S, O = _solver_pair(emu, 8, 10, 0.0, RELOCALIZATION_RANSAC)          # N == minInliers: nIterations = 1
    assert S.state()['max_iterations'] == O.max_its == 1
    d = pc.glibc_rand(5, 400)
    g = S.iterate(5, d); e = O.iterate(5, d)
    assert g[4] == e[4] and g[1] == e[1] and (g[0] is None) == (e[0] is None)


def test_quirk_refine_uses_best_so_far_and_strict_comparisons(emu):
    """Refine runs on the best-so-far set, not the hypothesis': a case where a later hypothesis has >= minInliers inliers, not more than the best, and a different inlier set
    (the restatement counts it), and the emulator agrees bit for bit"""
    p2d, s2, p3, R, t, bad = pc.make_case(3020, 40, 0.5, noise=1.5)
    ransac = (0.99, int((~bad).sum()) - 4, 300, 4, 0.1, 5.991)
    S = PnPsolver(p2d, s2, p3, pc.CAM, lib=emu); O = ref.PnPsolverRef(p2d, s2, p3, pc.CAM)
    S.SetRansacParameters(*ransac); O.set_ransac_parameters(*ransac)
    d = pc.glibc_rand(20, 4 * 2000); used = 0
    for call in range(20):
        k = O.call_hypotheses(5)
        g = S.iterate(5, d[used:used + 4 * max(k, 1)]); e = O.iterate(5, d[used:used + 4 * max(k, 1)])
        assert (g[0] is None) == (e[0] is None) and g[1] == e[1] and g[3] == e[3] and g[4] == e[4] and (g[2] == e[2]).all()
        if e[0] is not None: assert (g[0].view('u4') == e[0].view('u4')).all()
        used += 4 * e[4]
        if e[0] is not None or e[1]: break
    assert O.refines_on_other_set >= 1


def test_set_ransac_parameters_reruns_a_failed_refine(emu):
    """a Refine that failed can succeed after SetRansacParameters lowers minInliers: the reference reruns it on the same best set, and so must the solver"""
    p2d, s2, p3, R, t, bad = pc.make_case(3020, 40, 0.5, noise=1.5)
    n_in = int((~bad).sum())
    S = PnPsolver(p2d, s2, p3, pc.CAM, lib=emu); O = ref.PnPsolverRef(p2d, s2, p3, pc.CAM)
    ransac = (0.99, n_in - 4, 8, 4, 0.1, 5.991)                          # eight hypotheses, then bNoMore
    S.SetRansacParameters(*ransac); O.set_ransac_parameters(*ransac)
    d = pc.glibc_rand(20, 4 * 4000)
    g = S.iterate(5, d); e = O.iterate(5, d)
    assert g[4] == e[4] and g[1] == e[1] and g[3] == e[3]
    failed = O.refines                                                       # Refines done so far, none succeeded when the call found nothing by Refine
    lowered = (0.99, 4, 300, 4, 0.1, 5.991)
    S.SetRansacParameters(*lowered); O.set_ransac_parameters(*lowered)
    used = 4 * e[4]
    g = S.iterate(5, d[used:]); e = O.iterate(5, d[used:])
    assert (g[0] is None) == (e[0] is None) and g[1] == e[1] and g[3] == e[3] and g[4] == e[4] and (g[2] == e[2]).all()
    if e[0] is not None: assert (g[0].view('u4') == e[0].view('u4')).all()


def test_defined_undefined_behaviour_on_the_kernel(emu):
    pc.check_defined_ub(emu)


def test_call_longer_than_one_chunk(emu):
    """a call of 1000 hypotheses runs in two launches of the kernels (draws, the replica and the iteration count carried across them): caller draws and the replica"""
    p2d, s2, p3, R, t, bad = pc.make_case(4000, 400, 0.95)
    for seed in (None, 5):
        S = PnPsolver(p2d, s2, p3, pc.CAM, rand_seed=seed or 0, lib=emu); O = ref.PnPsolverRef(p2d, s2, p3, pc.CAM)
        ransac = (0.99, 30, 1000, 4, 0.02, 5.991)
        S.SetRansacParameters(*ransac); O.set_ransac_parameters(*ransac)
        assert O.max_its == 1000
        d = pc.glibc_rand(seed or 9, 4 * 1700)
        g = S.iterate(5, None if seed else d); e = O.iterate(5, d)
        assert g[4] == e[4] == 1000 and g[1] == e[1] and (g[0] is None) == (e[0] is None) and g[3] == e[3] and (g[2] == e[2]).all()
        g = S.iterate(600, None if seed else d[4000:]); e = O.iterate(600, d[4000:])
        assert g[4] == e[4] == 600 and S.state()['iterations'] == O.its == 1600


def test_batch_with_caller_draws_equals_single_solvers(emu):
    cases = [c for c in pc.CASES if c[1] >= 15][:6]
    pc.check_batch_equals_single(emu, cases, caller_draws=True)


def test_degenerate_draws_defined_behaviour(emu):
    """all correspondences identical: every hypothesis hits the singular qr_solve (approx 2: betas 0, no update) and approx 3's 0 / 0; emulator == restatement"""
    p3 = np.tile(np.array([[0.1, -0.2, 3.0]], 'f4'), (12, 1)); p2d = np.tile(np.array([[300.0, 200.0]], 'f4'), (12, 1)); s2 = np.ones(12, 'f4')
    cam = tuple(float(c) for c in pc.CAM)
    L_rho = None
    with np.errstate(all='ignore'):
        R, t = ref.epnp(p3[:4][None].astype('f8'), p2d[:4][None].astype('f8'), cam)
        pws = p3[:4][None].astype('f8')
        # the approximations themselves: approx 2 ends at exactly 0 (no Gauss-Newton update on the singular A), approx 3 is NaN (0 / 0)
        b2 = ref.gauss_newton(np.zeros((1, 6, 10)), np.zeros((1, 6)), np.zeros((1, 4)))
        assert (b2 == 0).all()
        b3 = ref.find_betas(np.zeros((1, 6, 10)), np.zeros((1, 6)), 3)
        assert np.isnan(b3[0, 2])
    S = PnPsolver(p2d, s2, p3, pc.CAM, lib=emu); O = ref.PnPsolverRef(p2d, s2, p3, pc.CAM)
    d = pc.glibc_rand(1, 4 * 400)
    g = S.iterate(5, d); e = O.iterate(5, d)
    assert (g[0] is None) == (e[0] is None) and g[1] == e[1] and g[3] == e[3] and g[4] == e[4] and (g[2] == e[2]).all()
    if e[0] is not None: assert (g[0].view('u4') == e[0].view('u4')).all()


def test_batch_equals_single_solvers(emu):
    cases = [c for c in pc.CASES if c[1] >= 15][:10]
    pc.check_batch_equals_single(emu, cases)
