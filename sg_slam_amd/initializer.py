"""Initializer — Python mirror of src/sg-slam/src/Initializer.cc over the C ABI (the two-view initialisation of Tracking::MonocularInitialization,
Tracking.cc:605-671), and InitializerBatch: B independent frame pairs in one launch sequence."""
import ctypes as C
import math
import numpy as np
import torch
from . import load
from .capi import _vp, InitReport

KEY_DTYPE = np.dtype([('x', 'f4'), ('y', 'f4'), ('size', 'f4'), ('angle', 'f4'), ('response', 'f4'), ('octave', 'i4'), ('class_id', 'i4')])      # sgx_keypoint
REPORT_DTYPE = np.dtype([('SH', 'f4'), ('SF', 'f4'), ('RH', 'f4'), ('model', 'i4'), ('n_matches', 'i4'), ('n_inliers_h', 'i4'), ('n_inliers_f', 'i4'), ('n_hyp', 'i4'),
                         ('best_hyp', 'i4'), ('n_good', 'i4', 8), ('cos_parallax', 'f4', 8), ('parallax', 'f4', 8), ('H21', 'f4', 9), ('F21', 'f4', 9)])  # sgx_init_report


def as_keys(k):
    """sgx_keypoint records from records or from an (n, 2) array of undistorted points (the other fields are not read by the Initializer)"""
    k = np.asarray(k)
    if k.dtype == KEY_DTYPE: return np.ascontiguousarray(k)
    out = np.zeros(len(k), KEY_DTYPE)
    if len(k): p = np.asarray(k, 'f4').reshape(-1, 2); out['x'] = p[:, 0]; out['y'] = p[:, 1]
    out['class_id'] = -1
    return out


def parallax_of(cos):
    """CheckRT's parallax (:901) of a selected cosine, as the C entry evaluates it on the host"""
    c = float(np.float32(cos))
    return np.float32(math.acos(c) * 180 / math.pi) if -1.0 <= c <= 1.0 else np.float32(np.nan)


def report_dict(r):
    """one REPORT_DTYPE record (or InitReport) as a dict of numpy values"""
    if isinstance(r, InitReport): r = np.frombuffer(bytes(r), REPORT_DTYPE)[0]
    return {n: (r[n].copy() if r[n].ndim else r[n].item()) for n in REPORT_DTYPE.names}


class Initializer:
    def __init__(self, keys1_un, cam, sigma=1.0, iterations=200, rand_seed=0, lib=None):
        """keys1_un = ReferenceFrame.mvKeysUn (sgx_keypoint records or (n, 2) points), cam = (fx, fy, cx, cy)"""
        self.lib = lib or load()
        self.k1 = as_keys(keys1_un); self.n1 = len(self.k1); self.iterations = int(iterations)
        cam = np.ascontiguousarray(cam, 'f4').reshape(4)
        self.h = C.c_void_p()
        self.lib.check(self.lib.dll.sgx_initializer_create(self.n1, _vp(self.k1), _vp(cam), float(sigma), self.iterations, int(rand_seed), C.byref(self.h)), 'sgx_initializer_create')

    def Initialize(self, keys2_un, matches12, rand_draws=None):
        """(ok, R21 (3, 3), t21 (3), vP3D (n1, 3), vbTriangulated (n1), inliers (n1), report); rand_draws = the 8 x iterations raw rand() values of mvSets, optional"""
        k2 = as_keys(keys2_un); m = np.ascontiguousarray(matches12, 'i4').reshape(-1)
        assert len(m) == self.n1, 'matches12: one entry per key of frame 1'
        d = None
        if rand_draws is not None:
            d = np.ascontiguousarray(rand_draws, 'i4').reshape(-1)
            assert len(d) >= 8 * self.iterations, 'rand_draws: 8 values per iteration'
        n = max(self.n1, 1)
        R = np.zeros(9, 'f4'); t = np.zeros(3, 'f4'); P = np.zeros((n, 3), 'f4'); tri = np.zeros(n, 'u1'); inl = np.zeros(n, 'u1'); ok = C.c_int32(); rep = InitReport()
        self.lib.check(self.lib.dll.sgx_initializer_initialize(self.h, len(k2), _vp(k2), _vp(m), _vp(d), _vp(R), _vp(t), _vp(P), _vp(tri), _vp(inl), C.byref(ok), C.byref(rep)),
                       'sgx_initializer_initialize')
        return bool(ok.value), R.reshape(3, 3), t, P[:self.n1], tri[:self.n1].astype(bool), inl[:self.n1].astype(bool), report_dict(rep)

    def close(self):
        if self.h: self.lib.dll.sgx_initializer_destroy(self.h); self.h = C.c_void_p()

    def __del__(self):
        try: self.close()
        except Exception: pass


class InitializerBatch:
    """B Initializers; run() is Initialize of all of them in one launch sequence on the current torch stream."""

    def __init__(self, max_pairs, max_keys, max_matches, iterations=200, lib=None):
        self.lib = lib or load(); self.h = C.c_void_p(); self.iterations = int(iterations)
        self.lib.check(self.lib.dll.sgx_init_batch_create(int(max_pairs), int(max_keys), int(max_matches), self.iterations, C.byref(self.h)), 'sgx_init_batch_create')
        self.B = 0

    def _dev(self, a):
        return torch.from_numpy(np.ascontiguousarray(a).view('u1').reshape(-1)).cuda().contiguous()

    def _stream(self):
        return C.c_void_p(torch.cuda.current_stream().cuda_stream)

    def _host(self, x, dtype):
        return x.cpu().numpy().view(dtype)

    def set(self, pairs, sigma=1.0):
        """pairs = [(keys1_un, keys2_un, matches12, cam (fx, fy, cx, cy)), ...]; sigma = one value for all or one per pair"""
        B = len(pairs)
        k1 = [as_keys(p[0]) for p in pairs]; k2 = [as_keys(p[1]) for p in pairs]
        self.off1 = np.zeros(B + 1, 'i4'); self.off1[1:] = np.cumsum([len(k) for k in k1])
        self.off2 = np.zeros(B + 1, 'i4'); self.off2[1:] = np.cumsum([len(k) for k in k2])
        pad = np.zeros(1, KEY_DTYPE)
        self._k1 = self._dev(np.concatenate(k1 + [pad])); self._k2 = self._dev(np.concatenate(k2 + [pad]))
        m = [np.asarray(p[2], 'i4').reshape(-1) for p in pairs]
        assert all(len(a) == len(k) for a, k in zip(m, k1)), 'matches12: one entry per key of frame 1'
        self._m = self._dev(np.concatenate(m + [np.zeros(1, 'i4')]))
        self.cam = np.ascontiguousarray(np.array([np.asarray(p[3], 'f4').reshape(4) for p in pairs], 'f4'))
        self.sigma = np.ascontiguousarray(np.broadcast_to(np.asarray(sigma, 'f4'), (B,)), 'f4')
        self.B = B; n = int(self.off1[-1]) + 1
        self.R21 = self._dev(np.zeros((B, 9), 'f4')); self.t21 = self._dev(np.zeros((B, 3), 'f4')); self.p3d = self._dev(np.zeros((n, 3), 'f4'))
        self.tri = self._dev(np.zeros(n, 'u1')); self.inl = self._dev(np.zeros(n, 'u1')); self.ok = self._dev(np.zeros(B, 'i4')); self.report = self._dev(np.zeros(B, REPORT_DTYPE))

    def launch(self, rand_seeds=None, rand_draws=None):
        """Initialize of every pair, asynchronous on the current stream; the results stay in self.ok / R21 / t21 / p3d / tri / inl / report.  rand_seeds (B) re-seeds the
        pairs' rand() replicas (None: they continue); rand_draws (B x k int32, k >= 8 x iterations): each pair's raw rand() values instead"""
        seeds = np.ascontiguousarray(rand_seeds, 'u4') if rand_seeds is not None else None
        d = None; stride = 0
        if rand_draws is not None:
            a = np.ascontiguousarray(rand_draws, 'i4'); assert a.shape[0] == self.B and a.shape[1] >= 8 * self.iterations
            stride = a.shape[1]; d = self._dev(a)
        self._draws = d                                           # alive until the launch sequence has read it
        self.lib.check(self.lib.dll.sgx_init_batch_run_dev(self.h, self.B, _vp(self.off1), _vp(self._k1), _vp(self._m), _vp(self.off2), _vp(self._k2), _vp(self.cam),
                                                           _vp(self.sigma), _vp(seeds), _vp(d), int(stride), _vp(self.R21), _vp(self.t21), _vp(self.p3d), _vp(self.tri),
                                                           _vp(self.inl), _vp(self.ok), _vp(self.report), self._stream()), 'sgx_init_batch_run_dev')

    def run(self, rand_seeds=None, rand_draws=None):
        """launch() and read back: a list of B tuples as Initializer.Initialize returns them"""
        self.launch(rand_seeds, rand_draws)
        ok = self._host(self.ok, 'i4'); R = self._host(self.R21, 'f4').reshape(-1, 3, 3); t = self._host(self.t21, 'f4').reshape(-1, 3)
        P = self._host(self.p3d, 'f4').reshape(-1, 3); tri = self._host(self.tri, 'u1').astype(bool); inl = self._host(self.inl, 'u1').astype(bool)
        rep = self._host(self.report, REPORT_DTYPE)
        out = []
        for b in range(self.B):
            r = report_dict(rep[b])
            for k in range(r['n_hyp']): r['parallax'][k] = parallax_of(r['cos_parallax'][k]) if r['n_good'][k] > 0 else 0.0
            s = slice(int(self.off1[b]), int(self.off1[b + 1]))
            out.append((bool(ok[b]), R[b].copy(), t[b].copy(), P[s].copy(), tri[s].copy(), inl[s].copy(), r))
        return out

    def close(self):
        if self.h: self.lib.dll.sgx_init_batch_destroy(self.h); self.h = C.c_void_p()

    def __del__(self):
        try: self.close()
        except Exception: pass
