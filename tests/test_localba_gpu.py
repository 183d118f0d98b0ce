"""GPU parity (MI355X) for LocalBundleAdjustment vs the oracle: identical iteration counts and erase flags,
poses / points / final chi2 within 1e-5 relative."""
import numpy as np
import pytest
from scenes import make_ba_problem, CAM
from sg_slam_amd.optimizer import Optimizer
from test_localba import close, points_close

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize('seed,n_free,n_fixed,n_points', [(11, 8, 5, 400), (12, 3, 0, 120), (13, 16, 10, 900), (14, 20, 40, 2000), (15, 30, 8, 1500), (16, 70, 30, 5000), (17, 56, 10, 2500), (18, 130, 20, 7000)])
def test_gpu_matches_oracle(gpulib, oracle, seed, n_free, n_fixed, n_points):
    prob, _, _ = make_ba_problem(oracle, n_free=n_free, n_fixed=n_fixed, n_points=n_points, seed=seed)
    eposes, epoints, eerase, etrace, eiters = oracle.local_ba(prob, CAM)
    p2 = {k: (v.copy() if hasattr(v, 'copy') else v) for k, v in prob.items()}
    erase, stats = Optimizer.LocalBundleAdjustment(p2, CAM, lib=gpulib)
    assert stats['iterations'] == tuple(eiters)
    assert (erase == eerase).all()
    assert close(p2['poses'], eposes) and points_close(p2['points'], epoints)
    ref = etrace[1, eiters[1] - 1, 0]
    assert abs(stats['chi2'][1] - ref) <= 1e-5 * max(1.0, ref)


def test_envelope_solver_equals_dense_gpu(gpulib_taps):
    gpulib = gpulib_taps          # forces the solver plan (sgx_ba_debug_set_solver)
    from test_localba import run_envelope_solver_equals_dense
    run_envelope_solver_equals_dense(gpulib, 60, 1500, 2)        # forced on a small system (partial last tile, cyclic corner)
    run_envelope_solver_equals_dense(gpulib, 600, 15000, 0)      # automatic choice: 3 594 unknowns, narrow covisibility band


def test_two_branch_solver_matches_oracle_gpu(gpulib_taps, oracle):
    gpulib = gpulib_taps
    from test_localba import run_two_branch_matches_oracle
    run_two_branch_matches_oracle(gpulib, oracle, 400, 10000, -1)    # 2 394 unknowns = 75 tiles, automatic solver choice; the oracle's dense solve takes ~20 s


def test_gpu_stop_flag(gpulib, oracle):
    prob, _, _ = make_ba_problem(oracle, seed=5)
    p2 = {k: (v.copy() if hasattr(v, 'copy') else v) for k, v in prob.items()}
    erase, stats = Optimizer.LocalBundleAdjustment(p2, CAM, stop_flag=np.array([1], 'i4'), lib=gpulib)
    assert (p2['poses'] == prob['poses']).all() and (p2['points'] == prob['points']).all() and erase.sum() == 0


def test_ba_config4_matches_oracle_fixture(gpulib, oracle):
    """BASELINE config 4 size (2 000 keyframes / 50 000 landmarks, ~397 k edges) against the ORACLE — live (its envelope LDL^T takes seconds) and through the committed
    fixture tests/golden/ba_2000kf_50klm.npz (tools/make_golden.py): identical LM iteration counts and erase flags, chi2 of every accepted iteration, every pose and
    point within 1e-5 relative (VERDICT r3 'next round' #5: this size used to be property-checked only).  Plus the run-to-run bit-reproducibility of the device."""
    import os
    from scenes import make_big_ba_problem
    prob, Ttrue, T0 = make_big_ba_problem(2000, 50000)
    eposes, epoints, eerase, etrace, eiters = oracle.local_ba(prob, CAM)
    g = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'ba_2000kf_50klm.npz'))
    assert (eiters == g['iters']).all() and (np.packbits(eerase) == g['erase_bits']).all() and (eposes.astype('f4') == g['poses']).all()      # the live oracle IS the fixture
    runs = []
    for _ in range(2):
        p2 = {k: (v.copy() if hasattr(v, 'copy') else v) for k, v in prob.items()}
        erase, stats = Optimizer.LocalBundleAdjustment(p2, CAM, lib=gpulib)
        runs.append((p2['poses'].copy(), p2['points'].copy(), erase.copy(), stats))
    poses, points, erase, stats = runs[0]
    assert stats['free_poses'] == 1999 and stats['iterations'] == tuple(eiters)
    assert (erase == eerase).all() and 0.02 < erase.mean() < 0.12                       # 5 % gross outliers were planted
    assert close(poses, eposes) and points_close(points, epoints)
    for ps in range(2):
        ref = etrace[ps, eiters[ps] - 1, 0]
        assert abs(stats['chi2'][ps] - ref) <= 1e-5 * max(1.0, ref), (ps, stats['chi2'][ps], ref)
    # the mnId==0 keyframe is a fixed vertex that the reference still rewrites through SE3Quat (Optimizer.cc:762-768): equal up to that fp32 round trip
    assert np.abs(poses[0] - prob['poses'][0]).max() <= 2e-6 * np.abs(prob['poses'][0]).max()
    e0 = np.abs(T0[:, :3, 3] - Ttrue[:, :3, 3]); e1 = np.abs(poses.astype('f8')[:, :3, 3] - Ttrue[:, :3, 3])
    assert e1.mean() < 0.5 * e0.mean() and e1.max() < e0.max()
    # run-to-run: bit-identical (the Schur complement is summed per destination block in landmark order, no atomics)
    assert (runs[1][0] == poses).all() and (runs[1][1] == points).all() and (runs[1][2] == erase).all() and runs[1][3]['iterations'] == stats['iterations']


@pytest.mark.parametrize('case', ['small', 'fixed_poses', 'band', 'wide_landmark'])
def test_device_job_list_equals_host_built_gpu(gpulib_taps, oracle, case):
    """Round 6: the Schur job list (which pairs of edges feed which 6 x 6 block of the reduced camera system, in the reference's subtraction order) is built by kernels
    (k_ba_jobs_row / k_ba_jobs_scan) instead of a host pass + 25 MB upload.  Same list -> same sums in the same order -> the whole bundle adjustment must come out with the
    SAME BITS as with the host builder (sgx_ba_debug_set_jobs), including the second build after the classification pass switched edges off."""
    from scenes import make_big_ba_problem
    lib = gpulib_taps
    if case == 'band': prob, _, _ = make_big_ba_problem(600, 15000)
    elif case == 'wide_landmark':
        # one landmark seen by 150 keyframes (the fill pass walks a landmark's edges 64 at a time) and twice by one of them (two jobs of one landmark in the same block: the
        # in-tile rank), spliced into the middle of the edge list; the copied observations are inconsistent with the landmark, so these edges also exercise the classification pass
        prob, _, _ = make_big_ba_problem(300, 6000)
        ep, el, eo, ei = (np.asarray(prob[k]) for k in ('edge_pose', 'edge_point', 'edge_obs', 'edge_info'))
        src = [int(np.flatnonzero(ep == q)[0]) for q in list(range(40, 190)) + [77]]
        at = len(ep) // 2
        prob['edge_pose'] = np.concatenate([ep[:at], ep[src], ep[at:]]).astype('i4'); prob['edge_point'] = np.concatenate([el[:at], np.full(len(src), 5, 'i4'), el[at:]]).astype('i4')
        prob['edge_obs'] = np.concatenate([eo[:at], eo[src], eo[at:]]).astype('f4'); prob['edge_info'] = np.concatenate([ei[:at], ei[src], ei[at:]]).astype('f4')
    else: prob, _, _ = make_ba_problem(oracle, n_free=30 if case == 'small' else 20, n_fixed=0 if case == 'small' else 40, n_points=1500 if case == 'small' else 2000, seed=21)
    out = []
    try:
        for host in (1, 0):
            lib.tap('sgx_ba_debug_set_jobs')(host)
            p = {k: (v.copy() if hasattr(v, 'copy') else v) for k, v in prob.items()}
            er, st = Optimizer.LocalBundleAdjustment(p, CAM, lib=lib)
            out.append((np.ascontiguousarray(p['poses']).copy(), np.ascontiguousarray(p['points']).copy(), er.copy(), st))
    finally:
        lib.tap('sgx_ba_debug_set_jobs')(0)
    a, b = out
    assert a[3]['iterations'] == b[3]['iterations'] and a[3]['chi2'] == b[3]['chi2']
    assert (a[2] == b[2]).all() and a[2].sum() > 0          # edges were switched off, so the second list differs from the first
    assert a[0].tobytes() == b[0].tobytes() and a[1].tobytes() == b[1].tobytes()


def test_envelope_tiles_only_initialisation_gpu(gpulib_taps):
    """Round 6: with the envelope solver only the tiles of its column steps are initialised per LM trial (k_ba_schur_init_env: 16 MB instead of the 1.15 GB dense matrix at 2 000
    keyframes).  Same bits as the full initialisation — also when the whole matrix is NaN before the tiles are written (mode 2): nothing outside the tiles is ever read —
    and when every double / float scratch array of the arena is NaN before the first kernel as well (mode 3; the smaller shapes and the global entry: test_ba_solver_gpu.py)."""
    from scenes import make_big_ba_problem
    lib = gpulib_taps
    prob, _, _ = make_big_ba_problem(600, 15000)
    out = {}
    try:
        for mode in (1, 0, 2, 3):
            lib.tap('sgx_ba_debug_set_init')(mode)
            p = {k: (v.copy() if hasattr(v, 'copy') else v) for k, v in prob.items()}
            er, st = Optimizer.LocalBundleAdjustment(p, CAM, lib=lib)
            import ctypes as C
            pl = (C.c_int32 * 4)(); lib.check(lib.tap('sgx_ba_debug_last_plan')(pl)); assert pl[0] == 1, 'the envelope solver must have run'
            out[mode] = (np.ascontiguousarray(p['poses']).tobytes(), np.ascontiguousarray(p['points']).tobytes(), er.tobytes(), st['iterations'], st['chi2'])
    finally:
        lib.tap('sgx_ba_debug_set_init')(0)
    assert np.isfinite(out[1][4]).all()
    assert out[0] == out[1] and out[2] == out[1] and out[3] == out[1]
