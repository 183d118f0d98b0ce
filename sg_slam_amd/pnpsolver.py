"""PnPsolver — Python mirror of src/sg-slam/src/PnPsolver.cc over the C ABI (the EPnP RANSAC of Tracking::Relocalization, Tracking.cc:1504-1530), and PnPsolverBatch:
B independent solvers iterated in one launch sequence, their state kept on the device."""
import ctypes as C
import numpy as np
import torch
from . import load
from .capi import _vp

DEFAULT_RANSAC = (0.99, 8, 300, 4, 0.4, 5.991)          # PnPsolver.h:67-68
RELOCALIZATION_RANSAC = (0.99, 10, 300, 4, 0.5, 5.991)  # Tracking.cc:1510


class PnPsolver:
    def __init__(self, p2d, sigma2, p3dw, cam, rand_seed=0, lib=None):
        """the n correspondences as the constructor flattens them (PnPsolver.cc:67-110): mvKeysUn points (n x 2), mvLevelSigma2[octave] (n), map point positions (n x 3);
        cam = (fx, fy, cx, cy)"""
        self.lib = lib or load()
        a = np.ascontiguousarray(p2d, 'f4').reshape(-1, 2); s = np.ascontiguousarray(sigma2, 'f4').reshape(-1); w = np.ascontiguousarray(p3dw, 'f4').reshape(-1, 3)
        k = np.ascontiguousarray(cam, 'f4').reshape(4)
        assert len(a) == len(s) == len(w)
        self.N = len(a); self.h = C.c_void_p()
        self.lib.check(self.lib.dll.sgx_pnp_solver_create(self.N, _vp(a), _vp(s), _vp(w), _vp(k), int(rand_seed), C.byref(self.h)), 'sgx_pnp_solver_create')

    def SetRansacParameters(self, probability=0.99, minInliers=8, maxIterations=300, minSet=4, epsilon=0.4, th2=5.991):
        self.lib.check(self.lib.dll.sgx_pnp_solver_set_ransac_parameters(self.h, float(probability), int(minInliers), int(maxIterations), int(minSet), float(epsilon),
                                                                          float(th2)), 'sgx_pnp_solver_set_ransac_parameters')

    def call_hypotheses(self, nIterations):
        """hypotheses the next iterate(nIterations) runs unless it succeeds first: max(nIterations, mRansacMaxIts - mnIterations), 0 when N < mRansacMinInliers"""
        st = self.state()
        if self.N < st['min_inliers']: return 0
        return max(0, nIterations, st['max_iterations'] - st['iterations'])

    def iterate(self, nIterations, rand_draws=None):
        """(Tcw or None, bNoMore, vbInliers[n], nInliers, iterations_run); rand_draws = 4 raw rand() values per hypothesis of the call (call_hypotheses)"""
        T = np.zeros(16, 'f4'); nm = C.c_int32(); inl = np.zeros(max(self.N, 1), np.uint8); ni = C.c_int32(); fnd = C.c_int32(); run = C.c_int32()
        d = None
        if rand_draws is not None:
            d = np.ascontiguousarray(rand_draws, 'i4')
            assert len(d) >= 4 * self.call_hypotheses(nIterations), 'rand_draws: 4 values per hypothesis of the call'
        self.lib.check(self.lib.dll.sgx_pnp_solver_iterate(self.h, int(nIterations), _vp(d) if d is not None else None, _vp(T), C.byref(nm), _vp(inl), C.byref(ni),
                                                           C.byref(fnd), C.byref(run)), 'sgx_pnp_solver_iterate')
        return (T.reshape(4, 4) if fnd.value else None), bool(nm.value), inl[:self.N].astype(bool), int(ni.value), int(run.value)

    def find(self, rand_draws=None):
        """find(vbInliers, nInliers) (:159-163) = iterate(mRansacMaxIts)"""
        return self.iterate(self.state()['max_iterations'], rand_draws)

    def state(self):
        T = np.zeros(16, 'f4'); m = C.c_int32(); mi = C.c_int32(); it = C.c_int32(); bi = C.c_int32()
        self.lib.check(self.lib.dll.sgx_pnp_solver_get_estimate(self.h, _vp(T), C.byref(m), C.byref(mi), C.byref(it), C.byref(bi)), 'sgx_pnp_solver_get_estimate')
        return dict(best_tcw=T.reshape(4, 4), max_iterations=int(m.value), min_inliers=int(mi.value), iterations=int(it.value), best_inliers=int(bi.value))

    def close(self):
        if self.h: self.lib.dll.sgx_pnp_solver_destroy(self.h); self.h = C.c_void_p()

    def __del__(self):
        try: self.close()
        except Exception: pass


class PnPsolverBatch:
    """B PnPsolvers with device-resident state; iterate() runs iterate(nIterations) of all of them in one launch sequence on the current torch stream."""

    def __init__(self, max_solvers, max_correspondences, lib=None):
        self.lib = lib or load(); self.h = C.c_void_p()
        self.lib.check(self.lib.dll.sgx_pnp_batch_create(int(max_solvers), int(max_correspondences), C.byref(self.h)), 'sgx_pnp_batch_create')
        self.B = 0; self.offsets = None

    def _dev(self, a):
        return torch.from_numpy(np.ascontiguousarray(a)).cuda().contiguous()

    def _stream(self):
        return C.c_void_p(torch.cuda.current_stream().cuda_stream)

    def _host(self, x):
        return x.cpu().numpy()

    def set(self, solvers, ransac=RELOCALIZATION_RANSAC, rand_seeds=None):
        """solvers = [(p2d (n x 2), sigma2 (n), p3dw (n x 3), cam (fx, fy, cx, cy)), ...]; ransac = one tuple for all or one per solver"""
        B = len(solvers)
        n = np.array([len(np.asarray(s[1]).reshape(-1)) for s in solvers], 'i8')
        self.offsets = np.zeros(B + 1, 'i4'); self.offsets[1:] = np.cumsum(n)
        cat = lambda i, w: self._dev(np.concatenate([np.asarray(s[i], 'f4').reshape(-1, w) for s in solvers] + [np.zeros((1, w), 'f4')]))
        self._p2d, self._sig, self._p3 = cat(0, 2), cat(1, 1), cat(2, 3)
        cam = np.ascontiguousarray(np.array([np.asarray(s[3], 'f4').reshape(4) for s in solvers], 'f4'))
        r = np.asarray(ransac, 'f8')
        r = np.ascontiguousarray(np.broadcast_to(r, (B, 6)) if r.ndim == 1 else r, 'f8')
        seeds = np.ascontiguousarray(rand_seeds if rand_seeds is not None else np.zeros(B), 'u4')
        self.lib.check(self.lib.dll.sgx_pnp_batch_set_dev(self.h, B, _vp(self.offsets), _vp(self._p2d), _vp(self._sig), _vp(self._p3), _vp(cam), _vp(r), _vp(seeds),
                                                          self._stream()), 'sgx_pnp_batch_set_dev')
        self.B = B
        self.result = self._dev(np.zeros((B, 4), 'i4')); self.tcw = self._dev(np.zeros((B, 16), 'f4')); self.inliers = self._dev(np.zeros(max(int(self.offsets[-1]), 1), 'u1'))

    def launch(self, nIterations, rand_draws=None):
        """iterate(nIterations) of every solver, asynchronous on the current stream; the results stay in self.result (B x 4: found, bNoMore, nInliers, iterations
        run), self.tcw (B x 16), self.inliers (offsets[B] flags).  rand_draws (B x k int32, optional): 4 raw rand() values per hypothesis of each solver's call"""
        d = None; stride = 0
        if rand_draws is not None:
            d = self._dev(np.asarray(rand_draws, 'i4')); stride = d.shape[1]
        self._draws = d                                           # alive until the launch sequence has read it
        self.lib.check(self.lib.dll.sgx_pnp_batch_iterate_dev(self.h, int(nIterations), _vp(d), int(stride), _vp(self.result), _vp(self.tcw), _vp(self.inliers),
                                                              self._stream()), 'sgx_pnp_batch_iterate_dev')

    def iterate(self, nIterations, rand_draws=None):
        """launch() and read back: (B x 4 int array, Tcw (B x 4 x 4), list of per-solver inlier flags)"""
        self.launch(nIterations, rand_draws)
        res = self._host(self.result); T = self._host(self.tcw).reshape(-1, 4, 4); inl = self._host(self.inliers).astype(bool)
        return res, T, [inl[self.offsets[b]:self.offsets[b + 1]] for b in range(self.B)]

    def close(self):
        if self.h: self.lib.dll.sgx_pnp_batch_destroy(self.h); self.h = C.c_void_p()

    def __del__(self):
        try: self.close()
        except Exception: pass
