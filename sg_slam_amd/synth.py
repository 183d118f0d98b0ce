"""Deterministic synthetic 640x480 RGB-D streams (SURVEY.md §8(d) input 1).

Integer-only image synthesis (Mersenne-Twister integers + fixed-point bilinear warps) so the
same seed gives byte-identical frames on every machine.  The scene is a textured
fronto-parallel plane at depth Z0 seen by a camera that translates parallel to the plane and
rolls about its optical axis, so consecutive frames are related by an exact similarity in the
image and the ground-truth pose Tcw(t) is known (used for ATE on synthetic streams).

Camera intrinsics default to the reference's TUM3.yaml (src/sg-slam/Examples/TUM3.yaml:8-34).
"""
import math
import numpy as np

TUM3 = dict(fx=535.4, fy=539.2, cx=320.1, cy=247.6, bf=40.0, depth_factor=5000.0, th_depth=40.0)


def world_texture(seed=1234, size=1536, n_rect=2400):
    """u8 texture: 4 octaves of value noise + high-contrast rectangles (corners at all scales)."""
    rng = np.random.RandomState(seed)
    acc = np.zeros((size, size), np.int64)
    for cell, amp in ((64, 8), (32, 4), (16, 2), (8, 2)):       # amplitudes sum to 16
        n = size // cell + 2
        lat = rng.randint(0, 256, (n, n)).astype(np.int64)
        idx = np.arange(size)
        i0 = idx // cell
        f = (idx % cell) * (256 // cell)                         # Q8 fraction
        a = lat[i0][:, i0]; b = lat[i0][:, i0 + 1]
        c = lat[i0 + 1][:, i0]; d = lat[i0 + 1][:, i0 + 1]
        fx = f[None, :]; fy = f[:, None]
        top = a * (256 - fx) + b * fx
        bot = c * (256 - fx) + d * fx
        acc += amp * ((top * (256 - fy) + bot * fy) >> 16)
    img = (acc >> 4)
    img = 48 + (img * 160 >> 8)                                  # keep head-room for rectangles
    for _ in range(n_rect):
        w = int(rng.randint(4, 64)); h = int(rng.randint(4, 64))
        x = int(rng.randint(0, size - w)); y = int(rng.randint(0, size - h))
        g = int(rng.randint(0, 256))
        img[y:y + h, x:x + w] = g
    return img.astype(np.uint8)


class PlaneStream:
    """Frame t of a synthetic RGB-D stream; frame(t) -> (gray u8 HxW, depth u16 HxW, Tcw 4x4 f64)."""

    def __init__(self, seed=1234, width=640, height=480, z0=2.0, cam=TUM3, noise=2, tex_size=1536):
        self.seed, self.w, self.h, self.z0, self.cam, self.noise = seed, width, height, z0, dict(cam), noise
        self.tex = world_texture(seed, tex_size)
        self.ts = tex_size

    def pose(self, t):
        """Camera centre (metres) and roll (rad): <= ~8 px and <= ~1.5 deg change per frame."""
        z0, fx = self.z0, self.cam['fx']
        px = z0 / fx                                             # metres per pixel on the plane
        cxm = 180.0 * px * math.sin(2 * math.pi * t / 140.0)
        cym = 120.0 * px * math.sin(2 * math.pi * t / 95.0 + 0.7)
        th = math.radians(12.0) * math.sin(2 * math.pi * t / 60.0)
        return cxm, cym, th

    def Tcw(self, t):
        cxm, cym, th = self.pose(t)
        c, s = math.cos(th), math.sin(th)
        R = np.array([[c, -s, 0.0], [s, c, 0.0], [0.0, 0.0, 1.0]])
        C = np.array([cxm, cym, 0.0])
        T = np.eye(4)
        T[:3, :3] = R
        T[:3, 3] = -R @ C
        return T

    def _warp_coords(self, t, z):
        """Q16 texel coordinates of every pixel for the plane at depth z (texels are pixels at depth z0): texel = (z/z0) * S(u - cx, v - cy) + centre"""
        cam, z0, ts = self.cam, self.z0, self.ts
        fx, fy, cx, cy = cam['fx'], cam['fy'], cam['cx'], cam['cy']
        cxm, cym, th = self.pose(t)
        c, s = math.cos(th), math.sin(th)
        Q = 1 << 16
        k = z / z0
        # texel = A * (u,v) + b   (Q16), derived from Pw = R^T Pc + C on the plane at depth z
        a00 = int(round(k * c * Q)); a01 = int(round(k * s * (fx / fy) * Q))
        a10 = int(round(-k * s * (fy / fx) * Q)); a11 = int(round(k * c * Q))
        b0 = int(round((ts / 2 + fx / z0 * cxm - k * (c * cx + s * (fx / fy) * cy)) * Q))
        b1 = int(round((ts / 2 + fy / z0 * cym + k * (s * (fy / fx) * cx - c * cy)) * Q))
        u = np.arange(self.w, dtype=np.int64)[None, :]
        v = np.arange(self.h, dtype=np.int64)[:, None]
        return a00 * u + a01 * v + b0, a10 * u + a11 * v + b1

    def _warp(self, tex, t, z):
        """bilinear (Q8 fractions, integer arithmetic) sample of `tex` under the warp of the plane at depth z"""
        ts = self.ts
        X, Y = self._warp_coords(t, z)
        xi = X >> 16; yi = Y >> 16
        xf = (X & 0xFFFF) >> 8; yf = (Y & 0xFFFF) >> 8             # Q8 fractions
        xi = np.clip(xi, 0, ts - 2); yi = np.clip(yi, 0, ts - 2)
        T = tex.astype(np.int64)
        p00 = T[yi, xi]; p01 = T[yi, xi + 1]; p10 = T[yi + 1, xi]; p11 = T[yi + 1, xi + 1]
        top = p00 * (256 - xf) + p01 * xf
        bot = p10 * (256 - xf) + p11 * xf
        return (top * (256 - yf) + bot * yf + 32768) >> 16

    def _noise(self, img, t):
        if self.noise:
            rng = np.random.RandomState((self.seed * 100003 + t) & 0x7FFFFFFF)
            img = img + rng.randint(-self.noise, self.noise + 1, img.shape)
        return np.clip(img, 0, 255).astype(np.uint8)

    def frame(self, t):
        gray = self._noise(self._warp(self.tex, t, self.z0), t)
        depth = np.full((self.h, self.w), int(round(self.z0 * self.cam['depth_factor'])), np.uint16)
        return gray, depth, self.Tcw(t)


class LayeredStream(PlaneStream):
    """PlaneStream plus a second fronto-parallel layer in front of it: textured rectangles at depth z1 < z0 occlude the background plane, so the scene
    has parallax (the epipolar geometry between frames is well determined — a single plane leaves cv::findFundamentalMat degenerate), depth
    discontinuities and occlusion boundaries.  Same camera motion and ground-truth poses as PlaneStream; the depth image holds z1 / z0 per pixel."""

    def __init__(self, seed=1234, z1=1.3, coverage=0.35, **kw):
        super().__init__(seed=seed, **kw)
        self.z1 = z1
        self.tex_fg = world_texture(seed + 7919, self.ts, n_rect=2400)
        rng = np.random.RandomState(seed + 104729)
        m = np.zeros((self.ts, self.ts), np.uint8)
        while m.mean() < coverage:
            w = int(rng.randint(90, 260)); h = int(rng.randint(90, 260))
            x = int(rng.randint(0, self.ts - w)); y = int(rng.randint(0, self.ts - h))
            m[y:y + h, x:x + w] = 1
        self.fg_mask = m

    def frame(self, t):
        X, Y = self._warp_coords(t, self.z1)
        xi = np.clip((X + 32768) >> 16, 0, self.ts - 1); yi = np.clip((Y + 32768) >> 16, 0, self.ts - 1)
        fg = self.fg_mask[yi, xi].astype(bool)                      # nearest texel of the foreground layer's footprint
        img = np.where(fg, self._warp(self.tex_fg, t, self.z1), self._warp(self.tex, t, self.z0))
        gray = self._noise(img, t)
        f = self.cam['depth_factor']
        depth = np.where(fg, int(round(self.z1 * f)), int(round(self.z0 * f))).astype(np.uint16)
        return gray, depth, self.Tcw(t)


class DynamicStream(LayeredStream):
    """LayeredStream plus an independently moving "walker": a textured 110 x 230 rectangle at depth 1.0 m that crosses the image back and forth (3 - 6 px per frame against the
    static scene, integer positions so frames stay byte-exact) — the dynamic content SG-SLAM's mask exists for (TUM fr3/walking_xyz: a person walking through the view).  Its
    keypoints violate the epipolar geometry of the static scene, so LK + RANSAC + the 1.0 px / 0.2 px test have points to erase; poses and depth of the static scene are unchanged."""

    def __init__(self, seed=1234, z_obj=1.0, **kw):
        super().__init__(seed=seed, **kw)
        self.z_obj = z_obj
        self.obj_w, self.obj_h = 110, 230
        self.obj_tex = world_texture(seed + 31337, 512, n_rect=500)[120:120 + self.obj_h, 80:80 + self.obj_w].copy()

    def walker_box(self, t):
        """(x, y, w, h) of the walker in frame t"""
        x = 265 + int(round(230 * math.sin(2 * math.pi * t / 97.0 + 0.3)))          # |dx/dt| <= 15 px, typically 3 - 12
        y = 120 + int(round(60 * math.sin(2 * math.pi * t / 41.0)))
        return max(0, min(self.w - self.obj_w, x)), max(0, min(self.h - self.obj_h, y)), self.obj_w, self.obj_h

    def frame(self, t):
        gray, depth, T = super().frame(t)
        x, y, w, h = self.walker_box(t)
        gray = gray.copy(); depth = depth.copy()
        gray[y:y + h, x:x + w] = self.obj_tex
        depth[y:y + h, x:x + w] = int(round(self.z_obj * self.cam['depth_factor']))
        return gray, depth, T


def distort_normalized(x, y, dist):
    """OpenCV's forward lens model on normalised coordinates (float64): k1, k2, p1, p2 [, k3 [, k4, k5, k6]]"""
    k = np.zeros(8); d = np.asarray(dist, 'f8').reshape(-1); k[:len(d)] = d
    r2 = x * x + y * y
    radial = (1 + ((k[4] * r2 + k[1]) * r2 + k[0]) * r2) / (1 + ((k[7] * r2 + k[6]) * r2 + k[5]) * r2)
    return (x * radial + 2 * k[2] * x * y + k[3] * (r2 + 2 * x * x), y * radial + k[2] * (r2 + 2 * y * y) + 2 * k[3] * x * y)


class _DistortedRender:
    """Renders a stream through a lens: the distorted pixel (u, v) shows what the pinhole camera sees at its undistorted position.  The inverse of the
    lens model is computed once per pixel in float64 by fixed-point iteration run to convergence (not OpenCV's five steps); poses and scene are the
    base stream's."""

    def _init_lens(self, dist):
        self.dist = np.asarray(dist, 'f4').reshape(-1)
        cam = self.cam
        fx, fy, cx, cy = (float(np.float32(cam[c])) for c in ('fx', 'fy', 'cx', 'cy'))
        u = np.arange(self.w, dtype='f8')[None, :].repeat(self.h, 0); v = np.arange(self.h, dtype='f8')[:, None].repeat(self.w, 1)
        xd = (u - cx) / fx; yd = (v - cy) / fy
        x, y = xd.copy(), yd.copy()
        for _ in range(500):
            px, py = distort_normalized(x, y, self.dist)
            ex, ey = px - xd, py - yd
            x, y = x - ex, y - ey
            if max(np.abs(ex).max(), np.abs(ey).max()) < 1e-14:
                break
        px, py = distort_normalized(x, y, self.dist)
        self.lens_residual_px = float(max(np.abs(px - xd).max() * fx, np.abs(py - yd).max() * fy))
        assert self.lens_residual_px < 1e-6, 'lens inverse did not converge'
        self._uu = x * fx + cx; self._vu = y * fy + cy                 # undistorted pixel of every distorted pixel

    def _warp_coords(self, t, z):
        """Q16 texel coordinates of the base stream's warp (PlaneStream._warp_coords) evaluated at the undistorted position of every pixel"""
        cam, z0, ts = self.cam, self.z0, self.ts
        fx, fy, cx, cy = cam['fx'], cam['fy'], cam['cx'], cam['cy']
        cxm, cym, th = self.pose(t)
        c, s = math.cos(th), math.sin(th)
        Q = 1 << 16
        k = z / z0
        a00 = int(round(k * c * Q)); a01 = int(round(k * s * (fx / fy) * Q))
        a10 = int(round(-k * s * (fy / fx) * Q)); a11 = int(round(k * c * Q))
        b0 = int(round((ts / 2 + fx / z0 * cxm - k * (c * cx + s * (fx / fy) * cy)) * Q))
        b1 = int(round((ts / 2 + fy / z0 * cym + k * (s * (fy / fx) * cx - c * cy)) * Q))
        u, v = self._uu, self._vu
        return np.floor(a00 * u + a01 * v + b0 + 0.5).astype(np.int64), np.floor(a10 * u + a11 * v + b1 + 0.5).astype(np.int64)


class DistortedPlaneStream(_DistortedRender, PlaneStream):
    """PlaneStream seen through a lens with distortion coefficients `dist` (e.g. TUM1.yaml's); same ground-truth poses."""

    def __init__(self, dist, seed=1234, **kw):
        PlaneStream.__init__(self, seed=seed, **kw)
        self._init_lens(dist)


class DistortedLayeredStream(_DistortedRender, LayeredStream):
    """LayeredStream seen through a lens with distortion coefficients `dist`; the depth image is registered to the distorted colour image."""

    def __init__(self, dist, seed=1234, **kw):
        LayeredStream.__init__(self, seed=seed, **kw)
        self._init_lens(dist)


def _texel_map(stream, t):
    """3x3 homogeneous map pixel (u, v) of frame t -> texel of the world texture (the float form of PlaneStream.frame's Q16 warp)."""
    cam, z0, ts = stream.cam, stream.z0, stream.ts
    fx, fy, cx, cy = cam['fx'], cam['fy'], cam['cx'], cam['cy']
    cxm, cym, th = stream.pose(t)
    c, s = math.cos(th), math.sin(th)
    return np.array([[c, s * (fx / fy), ts / 2 + fx / z0 * cxm - c * cx - s * (fx / fy) * cy],
                     [-s * (fy / fx), c, ts / 2 + fy / z0 * cym + s * (fy / fx) * cx - c * cy],
                     [0.0, 0.0, 1.0]])


def flow_affine(stream, t_cur, t_prev):
    """2x3 affine map: pixel of frame t_cur -> pixel of the same scene point in frame t_prev.  Stands in for cv::calcOpticalFlowPyrLK
    (Frame.cc:445, SURVEY.md §8(f) N1: not built) when the dynamic-feature mask is exercised on synthetic streams."""
    M = np.linalg.inv(_texel_map(stream, t_prev)) @ _texel_map(stream, t_cur)
    return M[:2, :]


def fundamental(stream, t_cur, t_prev):
    """3x3 F with x_prev^T F x_cur = 0 from the ground-truth poses (stands in for cv::findFundamentalMat, Frame.cc:469-472)."""
    cam = stream.cam
    K = np.array([[cam['fx'], 0, cam['cx']], [0, cam['fy'], cam['cy']], [0, 0, 1.0]])
    T = stream.Tcw(t_prev) @ np.linalg.inv(stream.Tcw(t_cur))              # X_prev = R X_cur + t
    R, t = T[:3, :3], T[:3, 3]
    tx = np.array([[0, -t[2], t[1]], [t[2], 0, -t[0]], [-t[1], t[0], 0]])
    F = np.linalg.inv(K).T @ tx @ R @ np.linalg.inv(K)
    nrm = np.abs(F).max()
    return F / nrm if nrm > 0 else F


def constant_image(value=128, width=640, height=480):
    """Degenerate case: no corners anywhere -> 0 keypoints (ORBextractor.cc:1065-1066)."""
    return np.full((height, width), value, np.uint8)


def low_contrast_image(seed=5, width=640, height=480):
    """Low-contrast texture: FAST at iniThFAST=20 finds nothing, so every cell takes the
    minThFAST=7 fallback branch (ORBextractor.cc:813-817)."""
    tex = world_texture(seed, 1024, n_rect=600).astype(np.int64)
    img = 118 + ((tex[:height, :width] - 128) * 22 >> 7)
    return np.clip(img, 0, 255).astype(np.uint8)


class MovingObject:
    """An independently moving textured rectangle composited over a stream's frames — the "person" of the dynamic-feature mask tests.  Integer
    positions, so frames stay byte-exact; box(t) is the rectangle (x, y, w, h) a detector would report for frame t."""

    def __init__(self, seed=77, w=120, h=200, x0=250, y0=140, vx=5, vy=-3):
        self.w, self.h, self.x0, self.y0, self.vx, self.vy = w, h, x0, y0, vx, vy
        self.tex = world_texture(seed, 512, n_rect=400)[100:100 + h, 60:60 + w].copy()

    def box(self, t):
        return (float(self.x0 + self.vx * t), float(self.y0 + self.vy * t), float(self.w), float(self.h))

    def paste(self, gray, t):
        out = gray.copy()
        x, y = self.x0 + self.vx * t, self.y0 + self.vy * t
        out[y:y + self.h, x:x + self.w] = self.tex
        return out


# ---- detector weights: the reference's mobilenetv3_ssdlite_voc.bin is not in its tree, so harness and tests synthesise a blob in ncnn .bin order
def parse_ncnn_param(path):
    """ncnn .param text -> list of layers (type, name, ins, outs, params) — the graph the reference loads at Detector2D.cc:24 (layer_count / blob_count
    header, `id=value` and `-233xx=n,v,...` array parameters)."""
    lines = [l.split() for l in open(path).read().strip().split('\n')]
    assert lines[0][0] == '7767517'
    layers = []
    for tok in lines[2:]:
        typ, name, nin, nout = tok[0], tok[1], int(tok[2]), int(tok[3])
        ins = tok[4:4 + nin]; outs = tok[4 + nin:4 + nin + nout]
        params = {}
        for kv in tok[4 + nin + nout:]:
            k, v = kv.split('=')
            k = int(k)
            if k <= -23300:
                vals = v.split(','); params[-k - 23300] = [float(x) for x in vals[1:]]
            else:
                params[k] = float(v) if ('.' in v or 'e' in v) else int(v)
        layers.append(dict(type=typ, name=name, ins=ins, outs=outs, p=params))
    return layers


def _calibration_inputs(seed):
    """three 3 x 300 x 300 float64 network inputs (u8 pixels minus the channel means of Detector2D.cc:40): uniform noise, a smooth texture replicated to the three
    channels (what the bench streams look like) and their average — the statistics the synthetic "batch-norm fold" below is computed on"""
    rng = np.random.RandomState(seed + 1000)
    mean = np.array([123.675, 116.28, 103.53])[:, None, None]
    a = rng.randint(0, 256, (3, 300, 300)).astype(np.float64)
    t = world_texture(seed + 1, 512, n_rect=300)[100:400, 60:360].astype(np.float64)
    b = np.repeat(t[None], 3, 0)
    return np.stack([a - mean, b - mean, np.floor((a + b) / 2) - mean])


def _quantise(v, bits=12):
    """round to `bits` mantissa bits: the calibration constants do not depend on the last bits of the float64 statistics (which may differ between CPUs)"""
    v = np.asarray(v, np.float64)
    m, e = np.frexp(v)
    return np.ldexp(np.round(m * (1 << bits)) / (1 << bits), e)


def _calibrate(layers, W, seed, person_logit, conf_gain=2.0, background_logit=2.0):
    """Fold a synthetic batch-norm into every convolution, in graph order: with the He draw the activations grow to 1e4 and every clip / gate saturates, the network
    amplifies an input perturbation ~1e8 and any two fp32 evaluation orders disagree by 10 % at the heads — unusable as a parity input (VERDICT r4 "weak" #1).  A trained
    network has batch-norm folded into each convolution; this does the same with the statistics of three calibration inputs: output channel c of every convolution is
    rescaled to unit variance and a small random mean (w_c *= s_c, b_c = beta_c + (b_c - mu_c) * s_c), per channel where the map has >= 32 samples, per layer otherwise.
    The confidence heads get `conf_gain` x unit logits, +background_logit on class 0 and +person_logit on class 15, so that DetectionOutput sees separated scores.
    float64 torch operators on the CPU; nothing of oracle/ is used (this generates INPUT data for the harness, the tests and the oracle alike)."""
    import torch
    import torch.nn.functional as F
    rng = np.random.RandomState(seed + 2000)
    producer = {o: L for L in layers for o in L['outs']}
    head_of = {}
    for nm, kind in (('mbox_conf', 'conf'), ('mbox_loc', 'loc')):
        for blob_name in next(L for L in layers if L['name'] == nm)['ins']:
            L = producer[blob_name]
            while L['type'] in ('Flatten', 'Permute'):
                L = producer[L['ins'][0]]
            head_of[L['name']] = kind
    blobs = {'input': torch.from_numpy(_calibration_inputs(seed))}
    nthreads = torch.get_num_threads()
    torch.set_num_threads(1)          # one thread: a few seconds, and no OpenMP oversubscription when several test workers calibrate at once (measured: 4 s alone, 700 s with 6 workers x 8 threads)
    try:
      with torch.no_grad():
          for L in layers:
              t, p, ins, outs = L['type'], L['p'], L['ins'], L['outs']
              if t == 'Input': continue
              if t == 'MemoryData': blobs[outs[0]] = torch.tensor(float(W[L['name']][0]), dtype=torch.float64); continue
              if t == 'Split':
                  for o in outs: blobs[o] = blobs[ins[0]]
                  continue
              if ins[0] not in blobs: continue                          # behind the heads (Permute .. DetectionOutput): nothing to calibrate
              a = blobs[ins[0]]
              if t in ('Convolution', 'ConvolutionDepthWise'):
                  w, b = W[L['name']]
                  outc, k, group = p[0], p[1], p.get(7, 1)
                  wt = torch.from_numpy(w.astype(np.float64).reshape(outc, -1, k, k))
                  y = F.conv2d(a, wt, torch.from_numpy(b.astype(np.float64)), stride=p.get(3, 1), padding=p.get(4, 0), groups=group)
                  kind = head_of.get(L['name'])
                  n = y.shape[0] * y.shape[2] * y.shape[3]
                  if n >= 32 and kind is None:
                      mu = y.mean((0, 2, 3)).numpy(); sd = y.std((0, 2, 3), unbiased=False).numpy()
                  else:
                      mu = np.full(outc, float(y.mean())); sd = np.full(outc, float(y.std(unbiased=False)))
                  sd = np.maximum(sd, 1e-3 * max(float(sd.max()), 1e-30))
                  if kind == 'conf':
                      gain = np.full(outc, conf_gain); beta = np.zeros(outc); beta[0::21] += background_logit; beta[15::21] += person_logit
                  elif kind == 'loc':
                      gain = np.ones(outc); beta = np.zeros(outc)
                  else:
                      gain = rng.uniform(0.8, 1.25, outc); beta = rng.randn(outc) * 0.3
                  s = _quantise(gain / sd)
                  b2 = _quantise(beta + (b.astype(np.float64) - mu) * s)
                  w2 = (w.astype(np.float64).reshape(outc, -1) * s[:, None]).astype(np.float32).reshape(-1)
                  W[L['name']] = (w2, b2.astype(np.float32))
                  y = F.conv2d(a, torch.from_numpy(w2.astype(np.float64).reshape(outc, -1, k, k)), torch.from_numpy(b2.astype(np.float32).astype(np.float64)), stride=p.get(3, 1), padding=p.get(4, 0), groups=group)
              elif t == 'BinaryOp':
                  b = blobs[ins[1]]; op = p.get(0, 0)
                  y = a + b if op == 0 else a * b if op == 2 else a / b
              elif t == 'Clip': y = torch.clamp(a, float(p[0]), float(p[1]))
              elif t == 'ReLU': y = torch.relu(a)
              else: continue
              blobs[outs[0]] = y
    finally:
        torch.set_num_threads(nthreads)
    return W


_WEIGHT_CACHE = {}


def synth_ncnn_weights(layers, seed=7, person_logit=0.0, calibrate=True):
    """dict layer-name -> arrays, and the ncnn .bin byte string (flag word 0 + raw fp32 per conv weight, raw bias, raw MemoryData).
    The draw is N(0, 2/fan_in) per convolution, then (calibrate=True, the default since round 5) a synthetic batch-norm fold per layer (_calibrate): unit-variance
    blobs, active gates, separated class scores — a network as well conditioned as a trained one.  calibrate=False is the raw draw of rounds 1-4 (chaotic: kept for the
    stress comparisons only).
    person_logit: added to the bias of every class-15 ("person") channel of the six confidence heads, so that a handful of person boxes per frame reach the
    dynamic-feature mask downstream."""
    key = (tuple((L['type'], L['name'], tuple(sorted((k, str(v)) for k, v in L['p'].items()))) for L in layers if L['type'] in ('Convolution', 'ConvolutionDepthWise')), seed, float(person_logit), bool(calibrate))
    if key in _WEIGHT_CACHE:
        W, blob = _WEIGHT_CACHE[key]
        return dict(W), blob
    rng = np.random.RandomState(seed)
    W = {}; blob = []
    for L in layers:
        p = L['p']
        if L['type'] == 'MemoryData':
            n = p.get(0, 0) * max(p.get(1, 1), 1) * max(p.get(2, 1), 1)
            # scalars of the h-swish / h-sigmoid chains: +3 and /6 in the original network; keep those semantics
            W[L['name']] = None
        elif L['type'] in ('Convolution', 'ConvolutionDepthWise'):
            outc, k = p[0], p[1]; wsize = p[6]; group = p.get(7, 1)
            inc = wsize // (outc * k * k) * group
            fan_in = (inc // group) * k * k
            w = (rng.randn(wsize) * np.sqrt(2.0 / fan_in)).astype(np.float32)
            b = (rng.randn(outc) * 0.05).astype(np.float32) if p.get(5, 0) else np.zeros(outc, np.float32)
            W[L['name']] = (w, b)
    # MemoryData constants: consumers tell whether it is the "+3" or the "/6" (BinaryOp add vs div)
    use = {}
    for L in layers:
        if L['type'] == 'BinaryOp':
            for i in L['ins']:
                if i in W and W[i] is None:
                    use[i] = L['p'].get(0, 0)
    for L in layers:
        if L['type'] == 'MemoryData':
            W[L['name']] = np.array([3.0 if use.get(L['name'], 0) == 0 else 6.0], np.float32)
    if calibrate:
        assert all(L['p'].get(5, 0) for L in layers if L['type'] in ('Convolution', 'ConvolutionDepthWise')), 'the fold needs a bias term on every convolution'
        _calibrate(layers, W, seed, person_logit)
    elif person_logit:
        producer = {o: L for L in layers for o in L['outs']}
        conf_in = next(L for L in layers if L['name'] == 'mbox_conf')['ins']
        for blob_name in conf_in:                                # F{i}_conf <- Flatten <- Permute <- Convolution
            L = producer[blob_name]
            while L['type'] in ('Flatten', 'Permute'):
                L = producer[L['ins'][0]]
            w, b = W[L['name']]
            b = b.copy(); b[15::21] += np.float32(person_logit); W[L['name']] = (w, b)
    for L in layers:     # .bin order = layer order
        if L['type'] == 'MemoryData':
            blob.append(W[L['name']].tobytes())
        elif L['type'] in ('Convolution', 'ConvolutionDepthWise'):
            w, b = W[L['name']]
            blob.append(np.zeros(1, np.uint32).tobytes()); blob.append(w.tobytes())
            if L['p'].get(5, 0): blob.append(b.tobytes())
    blob = b''.join(blob)
    _WEIGHT_CACHE[key] = (dict(W), blob)
    return W, blob


# ---- parallel synthesis of many streams (bench harness): one generator per worker process
_POOL_GEN = None


def _pool_init(cls_name, seed):
    global _POOL_GEN
    _POOL_GEN = globals()[cls_name](seed=seed)


def _pool_frame(t):
    g, d, _ = _POOL_GEN.frame(t)
    return g, d


def synth_streams(cls_name, seed, offsets, T, workers=None):
    """(gray[T, S, H, W] u8, depth[T, S, H, W] u16) of the streams starting at time offsets `offsets`, synthesised by a process pool"""
    import os
    from concurrent.futures import ProcessPoolExecutor
    S = len(offsets)
    ts = [o + t for o in offsets for t in range(T)]
    workers = workers or max(1, min(32, (os.cpu_count() or 2) // 2))
    gray = None; depth = None
    with ProcessPoolExecutor(workers, initializer=_pool_init, initargs=(cls_name, seed)) as ex:
        for i, (g, d) in enumerate(ex.map(_pool_frame, ts, chunksize=8)):
            if gray is None:
                gray = np.empty((T, S) + g.shape, np.uint8); depth = np.empty((T, S) + d.shape, np.uint16)
            gray[i % T, i // T] = g; depth[i % T, i // T] = d
    return gray, depth
