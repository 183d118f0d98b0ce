"""Same bits from two builds of the library on the bundle adjustments and the essential-graph optimisation (a host refactor must not move a single one): poses, points,
erase flags, iteration counts, chi2 and the solver plan of every case, each library in a process of its own.
usage: python tools/ab_ba_libs.py LIB_A LIB_B [--gpu]      (--gpu adds config 4, 2000 keyframes / 50000 landmarks, and both Schur job builders)"""
import ctypes as C, os, subprocess, sys, tempfile
import numpy as np
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, 'tests')]


def outputs(lib, gpu):
    from oracle import oracle as orc
    from scenes import make_ba_problem, make_big_ba_problem, CAM
    from ba_global_cases import gba_problem
    from sim3_cases import make_graph
    from sg_slam_amd.optimizer import Optimizer
    out = {}
    def ba(key, prob, solver=-1, twist='1', jobs=0, gba=None):
        if lib.has_taps: os.environ['SGX_BA_TWIST'] = twist; lib.tap('sgx_ba_debug_set_solver')(solver); lib.tap('sgx_ba_debug_set_jobs')(jobs)
        elif jobs: return          # the product library has no switches: automatic solver, device job builder
        p = {k: (v.copy() if hasattr(v, 'copy') else v) for k, v in prob.items()}
        if gba is None: er, st = Optimizer.LocalBundleAdjustment(p, CAM, lib=lib)
        else: er, st = np.zeros(0, np.uint8), Optimizer.BundleAdjustment(p, CAM, nIterations=10, bRobust=gba, lib=lib)
        pl = (C.c_int32 * 4)()
        if lib.has_taps: lib.check(lib.tap('sgx_ba_debug_last_plan')(pl))
        for name, v in (('poses', p['poses']), ('points', p['points']), ('erase', er), ('iters', np.array(st['iterations'])), ('chi2', np.array(st['chi2'], 'f8')), ('plan', np.array(pl))): out[key + ' ' + name] = v
    for seed, nfree, nfix, npt in ((11, 8, 5, 400), (12, 3, 0, 120), (13, 16, 10, 900), (15, 30, 8, 1500), (17, 56, 10, 2500)):
        ba('localba seed=%d' % seed, make_ba_problem(orc, n_free=nfree, n_fixed=nfix, n_points=npt, seed=seed)[0])
    for nkf, npt in ((150, 3600), (400, 10000), (600, 15000)) + (((2000, 50000),) if gpu else ()):
        for twist in '10':
            for jobs in (0, 1) if gpu else (0,): ba('band nkf=%d env twist=%s jobs=%d' % (nkf, twist, jobs), make_big_ba_problem(nkf, npt)[0], 2, twist, jobs)
    ba('band nkf=150 dense', make_big_ba_problem(150, 3600)[0], 1)
    for robust in (True, False): ba('gba robust=%d' % robust, gba_problem(orc, 12, 600, 21, 0.05), gba=robust)
    for seed, nv in enumerate((20, 60, 150, 400)):
        g = make_graph(50 + seed, nv, noise=[0.02, 0.01, 0.03, 0.005][seed], scale_drift=[0.0, 0.1, 0.0, 0.05][seed])
        for fix in (True, False): out['eg nv=%d fix=%d S' % (nv, fix)], out['eg nv=%d fix=%d stats' % (nv, fix)] = Optimizer.OptimizeEssentialGraph(g['S0'], g['fixed'], g['ei'], g['ej'], g['meas'], fix, 20, lib=lib)
    return out


if __name__ == '__main__':
    gpu = '--gpu' in sys.argv
    if sys.argv[1] == '--child':
        from sg_slam_amd.capi import SgxLib
        np.savez(sys.argv[3], **outputs(SgxLib(sys.argv[2]), gpu)); sys.exit(0)
    with tempfile.TemporaryDirectory() as tmp:
        res = []
        for i, so in enumerate(sys.argv[1:3]):
            subprocess.check_call([sys.executable, os.path.abspath(__file__), '--child', so, os.path.join(tmp, '%d.npz' % i)] + ['--gpu'] * gpu, timeout=900)
            res.append(dict(np.load(os.path.join(tmp, '%d.npz' % i))))
    bad = [k for k in res[0] if res[0][k].dtype != res[1][k].dtype or res[0][k].shape != res[1][k].shape or res[0][k].tobytes() != res[1][k].tobytes()]
    print('%d arrays compared, %d differ%s' % (len(res[0]), len(bad), ': ' + ', '.join(bad) if bad else ''))
    sys.exit(1 if bad or sorted(res[0]) != sorted(res[1]) else 0)
