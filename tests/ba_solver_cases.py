"""Shared cases and checks for the three solvers of the reduced camera system (sgx_ba.cpp: k_chol_small_reg, the dense blocked Cholesky, the envelope solver with one
or two branches) under BOTH entries, sgx_local_bundle_adjustment and sgx_bundle_adjustment — emulator (CPU tier, test_ba_solver_emu.py) and device (-m gpu,
test_ba_solver_gpu.py).

Every shape is the smallest at which its path exists.  A case names the plan it is there for and every run asserts it (sgx_ba_debug_last_plan): an envelope that is
forced on a problem with more than SGX_ENV_MAXM row tiles in a step falls back to the dense solver without a word, and the case would test nothing.

The checks:
  (a) check_global          BundleAdjustment against oracle.bundle_adjustment, the criteria of ba_global_cases.check_gba
  (b) check_local           LocalBundleAdjustment against oracle.local_ba, the criteria of test_localba_gpu.test_gpu_matches_oracle
  (c) check_init            the same bits whatever the solver's memory held before: sgx_ba_debug_set_init 1 (whole matrix initialised) = 0 (the envelope's tiles only)
                            = 2 (matrix NaN, then the tiles) = 3 (2 + every double / float scratch array of the arena NaN before the first kernel)
  (d) check_history         the same bits whatever ran before in the process: the arena is grow-only, shared and never cleared; needs no tap

For the global entry pose_fixed is (index == 0) and five unobserved points are appended, as ba_global_cases.gba_problem does.  That frees the fixed cameras of the two
make_ba_problem cases: `reg` then has 156 unknowns and `dense-partial` 228, both on the blocked dense path with a partial last tile (the register kernel under the
global entry is what test_ba_global's 6- and 12-keyframe cases run); and it makes `env-fixed-inside` the same problem as `env2-150`, so that case is local only."""
import contextlib
import ctypes as C
import os
import numpy as np
import ba_global_cases as bc
from scenes import make_ba_problem, make_big_ba_problem, CAM
from sg_slam_amd.optimizer import Optimizer
from test_localba import close, points_close, open_trajectory


def _big(nkf, npt, open_ends=False, fix_every7=False):
    def make(oracle):
        prob = make_big_ba_problem(nkf, npt)[0]
        if open_ends: prob = open_trajectory(prob, nkf)
        if fix_every7:
            fixed = np.array(prob['pose_fixed'], np.uint8); fixed[3::7] = 1      # fixed cameras inside the band: their rows are compacted away (hidx), couplings skip them
            prob = dict(prob, pose_fixed=fixed)
        return prob
    return make


def _small(n_free, n_fixed, n_points, seed):
    return lambda oracle: make_ba_problem(oracle, n_free=n_free, n_fixed=n_fixed, n_points=n_points, seed=seed)[0]


DENSE = (0, 0, 0, 0)


def _case(make, solver, plan, twist=None, local_only=False):
    return dict(make=make, solver=solver, twist=twist, plan={'local': plan} if local_only else {'local': plan, 'global': plan})


# make, solver (sgx_ba_debug_set_solver: -1 automatic, 2 envelope forced), plan (sgx_ba_debug_last_plan: envelope?, column steps of the first branch — all of them when there
# is one —, of the second, separator unknowns; recorded from the emulator: the planner is host code and does not depend on the build), SGX_BA_TWIST (None = left alone).
# The two entries of a case have the same free poses, hence the same plan.
CASES = {
    'reg':              _case(_small(16, 10, 900, 13), -1, DENSE),                        # local: 96 unknowns, k_chol_small_reg
    'dense-partial':    _case(_small(30, 8, 1500, 15), -1, DENSE),                        # local: 180 unknowns, blocked dense, partial last tile
    'env1-60':          _case(_big(60, 1500), 2, (1, 12, 0, 0)),                          # 354 unknowns, 12 tiles, one branch, cyclic corner, partial last tile of 2
    'env2-150':         _case(_big(150, 3600), 2, (1, 12, 15, 30)),                       # 894 unknowns, 28 tiles, the separator is a partial tile
    'env1-150-notwist': _case(_big(150, 3600), 2, (1, 28, 0, 0), twist='0'),              # the same problem as one branch over 28 tiles
    'env2-161':         _case(_big(161, 3900), 2, (1, 15, 12, 96)),                       # 960 unknowns, exactly 30 tiles: no partial tile anywhere
    'env2-open171':     _case(_big(171, 4000, open_ends=True), 2, (1, 15, 15, 60)),       # 1020 unknowns, free poses no multiple of 16, no cyclic corner
    'auto-171':         _case(_big(171, 4000), -1, DENSE),                                # 1020 unknowns: NP <= 1024 stays dense ...
    'auto-172':         _case(_big(172, 4000), -1, (1, 15, 15, 66)),                      # ... 1026 unknowns: the planner takes the envelope by itself
    'env-fixed-inside': _case(_big(150, 3600, fix_every7=True), 2, (1, 12, 9, 96), local_only=True),      # 128 free poses of 150: 768 unknowns, 24 tiles
}
ALL = tuple(CASES)
GLOBAL = tuple(n for n in ALL if 'global' in CASES[n]['plan'])
LOCAL_ORACLE = ('env-fixed-inside', 'env2-161', 'env1-150-notwist')          # (b): the other shapes have such a test already
INIT = tuple((n, e) for n in ALL for e in CASES[n]['plan'])                   # (c)
HISTORY = (('env2-150', 'global'), ('env1-60', 'local'), ('dense-partial', 'local'), ('auto-172', 'global'))      # (d); auto-172: the one X whose envelope the product library, which has no tap to force it, chooses itself
HISTORY_BIG = (300, 7000)                                                       # local BA between the runs of X: another layout, a larger arena

_problems, _refs = {}, {}


def problem(oracle, name, entry):
    """a fresh copy of the case's problem for the entry"""
    if name not in _problems: _problems[name] = CASES[name]['make'](oracle)
    prob = {k: np.array(v) for k, v in _problems[name].items()}
    if entry == 'global':
        fixed = np.zeros(len(prob['poses']), np.uint8); fixed[0] = 1
        prob['pose_fixed'] = fixed
        prob['points'] = np.concatenate([prob['points'], np.full((5, 3), 7.5, 'f4')])
    return prob


def reference(oracle, name, entry, *args):
    """the oracle's result, computed once per (case, entry, arguments) and never written to"""
    key = (name, entry) + args
    if key not in _refs:
        prob = problem(oracle, name, entry)
        _refs[key] = oracle.local_ba(prob, CAM) if entry == 'local' else oracle.bundle_adjustment(prob, CAM, *args)
    return _refs[key]


def last_plan(lib):
    pl = (C.c_int32 * 4)(); lib.check(lib.tap('sgx_ba_debug_last_plan')(pl))
    return tuple(int(v) for v in pl)


@contextlib.contextmanager
def switches(lib, name, init=None):
    """the case's solver choice and SGX_BA_TWIST, and the initialisation tap, for the calls inside; all put back afterwards.  The product library has no taps: it plans by itself."""
    case = CASES[name]
    twist_before = os.environ.get('SGX_BA_TWIST')
    try:
        if case['twist'] is not None: os.environ['SGX_BA_TWIST'] = case['twist']
        if lib.has_taps:
            lib.tap('sgx_ba_debug_set_solver')(case['solver'])
            if init is not None: lib.tap('sgx_ba_debug_set_init')(init)
        yield
    finally:
        if lib.has_taps:
            lib.tap('sgx_ba_debug_set_solver')(-1); lib.tap('sgx_ba_debug_set_init')(0)
        if twist_before is None: os.environ.pop('SGX_BA_TWIST', None)
        else: os.environ['SGX_BA_TWIST'] = twist_before


def assert_plan(lib, name, entry):
    """the call that just ran took the path the case is named for"""
    if lib.has_taps:
        got = last_plan(lib)
        assert got == CASES[name]['plan'][entry], (name, entry, got)


def run(lib, oracle, name, entry, init=None, n_iter=10, robust=True):
    """one bundle adjustment of the case; everything it returns, as bytes and exact numbers"""
    prob = problem(oracle, name, entry)
    with switches(lib, name, init):
        if entry == 'local': erase, st = Optimizer.LocalBundleAdjustment(prob, CAM, lib=lib)
        else: erase, st = np.zeros(0, np.uint8), Optimizer.BundleAdjustment(prob, CAM, nIterations=n_iter, bRobust=robust, lib=lib)
        assert_plan(lib, name, entry)
    return (np.ascontiguousarray(prob['poses']).tobytes(), np.ascontiguousarray(prob['points']).tobytes(), erase.tobytes(), st['iterations'], st['chi2'])


def differences(a, b):
    """which parts of two run() results differ (for the assertion message)"""
    return [what for what, x, y in zip(('poses', 'points', 'erase', 'iterations', 'chi2'), a, b) if x != y]


def assert_oracle_run(oracle, name, entry, res):
    """A run() result is the oracle's optimisation: its iteration counts, its erase flags, its final chi2 (1e-5 relative, as in (a) and (b)).  For the checks that compare
    runs with each other: a run's scratch is what earlier calls left, the NaN of an earlier mode 3 included, and runs that all went wrong in the same way would still agree."""
    if entry == 'local':
        _, _, eerase, etrace, eiters = reference(oracle, name, 'local')
        assert res[3] == tuple(eiters) and res[2] == eerase.tobytes()
        chi, ref = res[4][1], etrace[1, eiters[1] - 1, 0]
    else:
        _, _, etrace, eit = reference(oracle, name, 'global', 10, True)
        assert res[3] == eit
        chi, ref = res[4], etrace[eit - 1, 0]
    assert abs(chi - ref) <= 1e-5 * max(1.0, ref), (chi, ref)


def check_global(lib, oracle, name):
    """(a) BundleAdjustment against the oracle, robust with 10 iterations and plain with 5"""
    for n_iter, robust in ((10, True), (5, False)):
        with switches(lib, name):
            bc.check_gba_problem(lib, oracle, problem(oracle, name, 'global'), n_iter, robust, ref=reference(oracle, name, 'global', n_iter, robust))
            assert_plan(lib, name, 'global')


def check_local(lib, oracle, name):
    """(b) LocalBundleAdjustment against the oracle"""
    eposes, epoints, eerase, etrace, eiters = reference(oracle, name, 'local')
    prob = problem(oracle, name, 'local')
    with switches(lib, name):
        erase, stats = Optimizer.LocalBundleAdjustment(prob, CAM, lib=lib)
        assert_plan(lib, name, 'local')
    assert stats['iterations'] == tuple(eiters)
    assert (erase == eerase).all()
    assert close(prob['poses'], eposes) and points_close(prob['points'], epoints)
    ref = etrace[1, eiters[1] - 1, 0]
    assert abs(stats['chi2'][1] - ref) <= 1e-5 * max(1.0, ref), (stats['chi2'][1], ref)


def check_init(lib, oracle, name, entry):
    """(c) initialisation independence.  With an envelope plan mode 1 is the baseline; the dense solvers initialise the whole matrix in every mode (2 is a no-op there), so
    their baseline is mode 0 against the arena poison of mode 3."""
    modes = (1, 0, 2, 3) if CASES[name]['plan'][entry][0] else (0, 3)
    out = {mode: run(lib, oracle, name, entry, init=mode) for mode in modes}
    base = out[modes[0]]
    assert np.isfinite(base[4]).all(), base[4]
    for mode in modes[1:]:
        assert out[mode] == base, (name, entry, mode, differences(out[mode], base))
    assert_oracle_run(oracle, name, entry, base)


def check_history(lib, oracle, name, entry):
    """(d) history independence: X, a larger problem (another layout, the arena grows), X, a smaller one (another layout over the same memory), X"""
    first = run(lib, oracle, name, entry)
    assert np.isfinite(first[4]).all(), first[4]
    if 'history-big' not in _problems: _problems['history-big'] = make_big_ba_problem(*HISTORY_BIG)[0]
    big = {k: np.array(v) for k, v in _problems['history-big'].items()}
    _, st = Optimizer.LocalBundleAdjustment(big, CAM, lib=lib)
    assert st['free_poses'] == HISTORY_BIG[0] - 1 and np.isfinite(st['chi2']).all()
    second = run(lib, oracle, name, entry)
    run(lib, oracle, 'reg', 'local')
    third = run(lib, oracle, name, entry)
    assert second == first, (name, entry, differences(second, first))
    assert third == first, (name, entry, differences(third, first))
    assert_oracle_run(oracle, name, entry, first)
