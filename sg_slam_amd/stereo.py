"""Stereo — Frame::ComputeStereoMatches (src/sg-slam/src/Frame.cc:716-890) and the stereo Frame constructor up to it (:70-99) over the C ABI.

StereoMatcher is the handle (sgx_stereo_*): device pointers in (torch CUDA tensors in the product, numpy arrays under the kernel-logic emulator of the tests), mvuRight /
mvDepth out.  StereoFrameBatch does what the constructor does for B rectified pairs in one launch sequence: optional cvtColor on both images, ONE extraction of the 2B
images (left ones first), UndistortKeyPoints of the left keys, the stereo match; StereoFrame is the batch of one.  The results are ready for frame.unproject_batch, the
matchers and the solvers, which take a uright / depth pair per keypoint whatever sensor it came from.

As in the reference, mvuRight is computed from the RAW keypoints (mvKeys, mvKeysRight), not from the undistorted ones: ComputeStereoMatches assumes a rectified pair,
for which the distortion coefficients are zero and mvKeysUn is a copy of mvKeys."""
import ctypes as C
import numpy as np
from . import load
from .capi import _vp, KP_DTYPE
from .matcher import camera_struct


class StereoMatcher:
    """extractor: an ORBextractor whose geometry (image size, levels, scale factor, nfeatures) every extractor passed to the match calls must share"""

    def __init__(self, extractor, max_batch=1, lib=None):
        self.lib = lib if lib is not None else extractor.lib
        self.cap = extractor.capacity; self.max_batch = int(max_batch); self.h = C.c_void_p()
        self.lib.check(self.lib.dll.sgx_stereo_create(extractor.h, self.max_batch, C.byref(self.h)), 'sgx_stereo_create')

    def close(self):
        if getattr(self, 'h', None):
            self.lib.dll.sgx_stereo_destroy(self.h); self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def match_batch_dev(self, batch, orb_left, left_first_frame, d_gray_left, pitch_left, orb_right, right_first_frame, d_gray_right, pitch_right,
                        d_keys_left, d_desc_left, d_n_left, d_keys_right, d_desc_right, d_n_right, fx, bf, d_uright, d_zdepth, d_nmatched=None, stream=None, cap=None):
        """sgx_stereo_match_batch_dev: asynchronous on `stream`, after the extraction(s) that built the pyramids on the same stream"""
        self.lib.check(self.lib.dll.sgx_stereo_match_batch_dev(self.h, int(batch), orb_left.h, int(left_first_frame), _vp(d_gray_left), int(pitch_left),
                                                               orb_right.h, int(right_first_frame), _vp(d_gray_right), int(pitch_right),
                                                               self.cap if cap is None else int(cap), _vp(d_keys_left), _vp(d_desc_left), _vp(d_n_left),
                                                               _vp(d_keys_right), _vp(d_desc_right), _vp(d_n_right), float(fx), float(bf),
                                                               _vp(d_uright), _vp(d_zdepth), _vp(d_nmatched), _vp(stream)), 'sgx_stereo_match_batch_dev')

    def match(self, orb_left, orb_right, keys_left, desc_left, keys_right, desc_right, fx, bf):
        """one host pair (sgx_stereo_match) after orb_left(image_left) and orb_right(image_right): (mvuRight, mvDepth, matches kept)"""
        kl = np.ascontiguousarray(keys_left, KP_DTYPE); kr = np.ascontiguousarray(keys_right, KP_DTYPE)
        dl = np.ascontiguousarray(desc_left, np.uint8); dr = np.ascontiguousarray(desc_right, np.uint8)
        ur = np.full(max(len(kl), 1), -1, 'f4'); z = np.full(max(len(kl), 1), -1, 'f4'); n = C.c_int(0)
        self.lib.check(self.lib.dll.sgx_stereo_match(self.h, orb_left.h, orb_right.h, _vp(kl) if len(kl) else None, _vp(dl) if len(kl) else None, len(kl),
                                                     _vp(kr) if len(kr) else None, _vp(dr) if len(kr) else None, len(kr), float(fx), float(bf), _vp(ur), _vp(z), C.byref(n)),
                       'sgx_stereo_match')
        return ur[:len(kl)], z[:len(kl)], n.value

    def debug_read(self, frame=0):
        """test tap: dict(best_idx, best_dist, code, best_inc, sads) of every keypoint slot of left frame `frame` of the last batch"""
        c = self.cap
        out = dict(best_idx=np.zeros(c, 'i4'), best_dist=np.zeros(c, 'i4'), code=np.zeros(c, 'i4'), best_inc=np.zeros(c, 'i4'), sads=np.zeros((c, 11), 'i4'))
        self.lib.check(self.lib.tap('sgx_stereo_debug_read')(self.h, int(frame), _vp(out['best_idx']), _vp(out['best_dist']), _vp(out['code']), _vp(out['best_inc']),
                                                             _vp(out['sads'])), 'sgx_stereo_debug_read')
        return out


class StereoFrameBatch:
    """Frame::Frame(imLeft, imRight, ...) (Frame.cc:70-99) for `batch` rectified pairs on the device.  cam: dict(fx, fy, cx, cy, bf); dist: mDistCoef (4, 5 or 8
    coefficients; None or k1 == 0: mvKeysUn is a byte copy of mvKeys).  Images are torch CUDA uint8 tensors: batch x height x width (gray) or batch x height x width x
    channels (3 or 4; rgb: Camera.RGB).  Returns dict(n, keys, keys_un, desc, uright, depth, nmatched, n_right, keys_right, desc_right): torch tensors of batch x cap
    slots; mvuRight comes from the raw keys, as in the reference."""

    def __init__(self, width, height, cam, dist=None, batch=1, nfeatures=1000, scaleFactor=1.2, nlevels=8, iniThFAST=20, minThFAST=7, lib=None):
        import torch
        from .orb import ORBextractor
        self.lib = lib if lib is not None else load()
        self.width, self.height, self.batch = int(width), int(height), int(batch)
        self.cam = dict(cam); self.dist = np.zeros(4, 'f4') if dist is None else np.ascontiguousarray(dist, 'f4').reshape(-1)
        self.extractor = ORBextractor(nfeatures, scaleFactor, nlevels, iniThFAST, minThFAST, width, height, max_batch=2 * self.batch, lib=self.lib)
        self.matcher = StereoMatcher(self.extractor, max_batch=self.batch, lib=self.lib)
        B, cap = self.batch, self.extractor.capacity
        self.cap = cap; self.pitch = (self.width + 3) & ~3
        dev = torch.device('cuda')
        self.gray = torch.zeros((2 * B, self.height, self.pitch), dtype=torch.uint8, device=dev)
        self.keys = torch.zeros((2 * B, cap, 7), dtype=torch.float32, device=dev)           # sgx_keypoint records, 28 bytes
        self.desc = torch.zeros((2 * B, cap, 32), dtype=torch.uint8, device=dev)
        self.n = torch.zeros(2 * B, dtype=torch.int32, device=dev)
        self.keys_un = torch.zeros((B, cap, 7), dtype=torch.float32, device=dev)
        self.uright = torch.zeros((B, cap), dtype=torch.float32, device=dev); self.depth = torch.zeros((B, cap), dtype=torch.float32, device=dev)
        self.nmatched = torch.zeros(B, dtype=torch.int32, device=dev)
        self.no_depth = torch.zeros((B, self.height, self.width), dtype=torch.int16, device=dev)      # the undistort entry is fused with ComputeStereoFromRGBD: no depth image here

    def close(self):
        self.matcher.close(); self.extractor.close()

    def __call__(self, left, right, rgb=False):
        import torch
        from . import frame
        B, W, H = self.batch, self.width, self.height
        assert left.shape == right.shape and left.shape[0] == B and tuple(left.shape[1:3]) == (H, W) and left.dtype == torch.uint8 and left.is_cuda and right.is_cuda
        stream = torch.cuda.current_stream().cuda_stream
        if left.dim() == 4:                                                                  # cvtColor on both images (Tracking.cc:175-200)
            ch = int(left.shape[3])
            for half, img in enumerate((left, right)):
                src = img.contiguous()
                frame.gray_from_color_batch(self.lib, B, W, H, src, W * ch, ch, not rgb, self.gray[half * B:], self.pitch, stream=stream)
        else:
            self.gray[:B, :, :W] = left; self.gray[B:, :, :W] = right
        ex = self.extractor
        ex.extract_batch_dev(self.gray, self.pitch, 2 * B, self.keys, self.desc, self.n, stream=stream)      # ExtractORB(0, imLeft), ExtractORB(1, imRight)
        cam = dict(self.cam); cam.setdefault('depth_factor', 1.0)
        frame.undistort_stereo_rgbd_batch_dev(self.lib, B, self.cap, self.keys, self.n, self.dist, cam, self.no_depth, W, H, self.keys_un, self.uright, self.depth, stream=stream)
        self.matcher.match_batch_dev(B, ex, 0, self.gray, self.pitch, ex, B, self.gray, self.pitch, self.keys, self.desc, self.n, self.keys[B:], self.desc[B:], self.n[B:],
                                     self.cam['fx'], self.cam['bf'], self.uright, self.depth, self.nmatched, stream=stream)
        return dict(n=self.n[:B], keys=self.keys[:B], keys_un=self.keys_un, desc=self.desc[:B], uright=self.uright, depth=self.depth, nmatched=self.nmatched,
                    n_right=self.n[B:], keys_right=self.keys[B:], desc_right=self.desc[B:])


class StereoFrame(StereoFrameBatch):
    """one pair: images height x width (gray) or height x width x channels; the result's tensors keep the leading batch dimension of 1"""

    def __init__(self, width, height, cam, dist=None, **kw):
        super().__init__(width, height, cam, dist=dist, batch=1, **kw)

    def __call__(self, left, right, rgb=False):
        return super().__call__(left[None], right[None], rgb=rgb)
