"""Shared cases for PnPsolver (Tracking::Relocalization's EPnP RANSAC): synthetic correspondences, the restatement tests/pnp_ref.py against a library (device or emulator)."""
import ctypes
import numpy as np
import pnp_ref as ref
from sg_slam_amd.capi import _vp
from sg_slam_amd.pnpsolver import PnPsolver, PnPsolverBatch, DEFAULT_RANSAC, RELOCALIZATION_RANSAC

CAM = np.array([535.4, 539.2, 320.1, 247.6], 'f4')
SIGMA2 = (1.2 ** (2 * np.arange(8))).astype('f4')          # mvLevelSigma2 for scale factor 1.2


def rot(w):
    th = np.linalg.norm(w)
    if th == 0: return np.eye(3)
    k = w / th; K = np.array([[0, -k[2], k[1]], [k[2], 0, -k[0]], [-k[1], k[0], 0]])
    return np.eye(3) + np.sin(th) * K + (1 - np.cos(th)) * K @ K


def make_case(seed, n, outliers=0.3, noise=0.5, planar=False):
    """n world points seen from a camera (R, t) with keypoint noise (pixels) and gross outliers; -> p2d, sigma2, p3dw (float32), R, t, outlier mask"""
    rng = np.random.RandomState(seed)
    R = rot(rng.normal(0, 0.3, 3)); t = rng.normal(0, 0.3, 3)
    Xc = np.c_[rng.uniform(-1.5, 1.5, n), rng.uniform(-1.0, 1.0, n), rng.uniform(2.0, 6.0, n)]
    if planar: Xc[:, 2] = 3.0 + 0.3 * Xc[:, 0]
    Xw = (R.T @ (Xc - t).T).T
    fx, fy, cx, cy = CAM.astype('f8')
    uv = np.c_[fx * Xc[:, 0] / Xc[:, 2] + cx, fy * Xc[:, 1] / Xc[:, 2] + cy]
    oct_ = rng.randint(0, 4, n)
    uv += rng.normal(0, noise, (n, 2)) * np.sqrt(SIGMA2[oct_])[:, None]
    bad = rng.rand(n) < outliers
    uv[bad] = np.c_[rng.uniform(0, 640, bad.sum()), rng.uniform(0, 480, bad.sum())]
    return uv.astype('f4'), SIGMA2[oct_].copy(), Xw.astype('f4'), R, t, bad


class HostBatch(PnPsolverBatch):
    """PnPsolverBatch on the kernel-logic emulator, whose "device" memory is host memory"""
    def _dev(self, a): return np.ascontiguousarray(a)
    def _stream(self): return None
    def _host(self, x): return x.copy()


def batch_for(lib, B, n):
    return HostBatch(B, n, lib=lib) if 'EMULATOR' in lib.version() else PnPsolverBatch(B, n, lib=lib)


def glibc_rand(seed, count):
    libc = ctypes.CDLL(None)
    libc.srand(seed)
    return np.array([libc.rand() for _ in range(count)], 'i8')


CASES = []          # (seed, n, outliers, ransac, n_iterations per call, draw seed)
for i, n in enumerate([4, 9, 10, 15, 30, 120, 400]):
    for j, out in enumerate([0.0, 0.3, 0.5, 0.7]):
        CASES.append((100 + 10 * i + j, n, out, RELOCALIZATION_RANSAC if (i + j) % 2 == 0 else DEFAULT_RANSAC, 5, 7 * i + j))


def run_case(lib, case, exact=True, max_calls=80):
    """iterate(5) until a model or bNoMore on the library and the restatement with the same draws; returns the number of calls that agreed"""
    seed, n, out, ransac, nit, dseed = case
    p2d, s2, p3, R, t, bad = make_case(seed, n, out)
    S = PnPsolver(p2d, s2, p3, CAM, lib=lib); O = ref.PnPsolverRef(p2d, s2, p3, CAM)
    S.SetRansacParameters(*ransac); O.set_ransac_parameters(*ransac)
    st = S.state()
    assert (st['max_iterations'], st['min_inliers']) == (O.max_its, O.min_inliers), (case, st, O.max_its, O.min_inliers)
    draws = glibc_rand(dseed, 4 * 4000)
    used = 0; calls = 0
    for call in range(max_calls):
        k = O.call_hypotheses(nit)
        assert S.call_hypotheses(nit) == k
        d = draws[used:used + 4 * max(k, 1)]
        gT, gnm, ginl, gni, grun = S.iterate(nit, d)
        eT, enm, einl, eni, erun = O.iterate(nit, d)
        calls += 1
        assert (gT is None) == (eT is None) and gnm == enm and grun == erun and gni == eni, (case, call, gT is None, eT is None, gnm, enm, grun, erun, gni, eni)
        assert (ginl == einl).all(), (case, call)
        if eT is not None:
            if exact: assert (gT.view('u4') == eT.view('u4')).all(), (case, call, gT, eT)
            else: assert np.abs(gT - eT).max() <= 1e-6 * max(1.0, np.abs(eT).max()), (case, call, gT, eT)
        used += 4 * erun
        if eT is not None or enm: break
    S.close()
    return calls, O


def check_batch_equals_single(lib, cases, nit=5, calls=3, caller_draws=False):
    """B solvers in one batch == B single solvers, call by call, with their own glibc replicas (or, caller_draws, each solver's own libc rand() values passed in)"""
    data = [make_case(c[0], c[1], c[2])[:3] for c in cases]
    Bt = batch_for(lib, len(cases), sum(len(d[1]) for d in data))
    Bt.set([(d[0], d[1], d[2], CAM) for d in data], RELOCALIZATION_RANSAC, rand_seeds=[c[5] for c in cases])
    singles = []
    for c, d in zip(cases, data):
        S = PnPsolver(d[0], d[1], d[2], CAM, rand_seed=c[5], lib=lib); S.SetRansacParameters(*RELOCALIZATION_RANSAC); singles.append(S)
    streams = [glibc_rand(c[5], 4 * 3000) for c in cases]; used = [0] * len(cases)
    for call in range(calls):
        if caller_draws:
            k = 4 * max(max(S.call_hypotheses(nit) for S in singles), 1)
            D = np.stack([st[u:u + k] for st, u in zip(streams, used)])
            res, T, inl = Bt.iterate(nit, D)
        else: res, T, inl = Bt.iterate(nit)
        for b, S in enumerate(singles):
            gT, gnm, ginl, gni, grun = S.iterate(nit, streams[b][used[b]:] if caller_draws else None)
            used[b] += 4 * grun
            assert res[b, 0] == (gT is not None) and res[b, 1] == gnm and res[b, 2] == gni and res[b, 3] == grun, (b, call, res[b], gT is None, gnm, gni, grun)
            assert (inl[b] == ginl).all(), (b, call)
            if gT is not None: assert (T[b].view('u4') == gT.view('u4')).all(), (b, call)
    for S in singles: S.close()
    Bt.close()


def check_defined_ub(lib):
    """the kernel's two defined undefined behaviours, through the test tap sgx_pnp_debug_betas (device or emulator), against the restatement bit for bit:
    a Gauss-Newton step whose qr_solve meets a singular A makes no update; a zero betas[0] divides in IEEE arithmetic"""
    tap = lib.tap('sgx_pnp_debug_betas')
    rng = np.random.RandomState(3)
    def run(which, L, rho, betas):
        b = np.ascontiguousarray(betas, 'f8').copy(); Lc = np.ascontiguousarray(L, 'f8'); rc = np.ascontiguousarray(rho, 'f8')
        lib.check(tap(which, _vp(Lc), _vp(rc), _vp(b)), 'sgx_pnp_debug_betas'); return b
    # (a) A = 0 in every step (L = 0, or betas = 0): five singular qr_solves, betas unchanged
    for L, betas in ((np.zeros((6, 10)), np.array([0.3, -0.2, 0.1, 0.05])), (rng.normal(size=(6, 10)), np.zeros(4))):
        rho = rng.normal(size=6)
        got = run(0, L, rho, betas)
        assert (got.view('u8') == betas.view('u8')).all(), got
        assert (ref.gauss_newton(L[None], rho[None], betas[None])[0].view('u8') == got.view('u8')).all()
    # a regular A moves the betas (so the check above is not vacuous)
    L = rng.normal(size=(6, 10)); rho = rng.normal(size=6); betas = np.array([0.3, -0.2, 0.1, 0.05])
    got = run(0, L, rho, betas)
    assert (got != betas).any() and (ref.gauss_newton(L[None], rho[None], betas[None])[0].view('u8') == got.view('u8')).all()
    # (b) L's first column zero: the solved b[0] is exactly 0, betas[0] = 0, and approximations 1 and 3 divide by it (inf / NaN)
    L = rng.normal(size=(6, 10)); L[:, 0] = 0; rho = rng.normal(size=6)
    with np.errstate(all='ignore'):
        for which in (1, 3):
            got = run(which, L, rho, np.zeros(4))
            want = ref.find_betas(L[None], rho[None], which)[0]
            assert got[0] == 0 and not np.isfinite(got[2]), (which, got)
            assert (got.view('u8') == want.view('u8')).all(), (which, got, want)
