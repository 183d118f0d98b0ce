"""Cases for the two tracking matchers (sgx_match_project_frame, sgx_match_project_local): one hand-made scene per gate that the synthetic streams never reach (level
windows under bForward / bBackward, projection and frustum rejections, grid edges, the radius and stereo equalities, TH_HIGH, scan-order ties, the rotation histogram,
long lock chains, the 4.0 search radius, PredictScale and its level boundaries, the ratio test), the sizes at which the kernels take another path, and the batch entries.

Inputs are exact in float: identity rotations, fx = fy = 512 and z = 2 (so u = 256 * x with no rounding; cx = cy = 0 keeps even "one float outside a bound"
reachable), bf = 32 (mb = 1/16), coordinates that are multiples of 1/64, np.nextafter for "just outside".  A descriptor is BASE with its first n bits flipped: the Hamming
distance between desc(n) and desc(m) is |n - m| by construction.

A case marked KAT carries its answer (match array, nmatches, in_view) written out by hand from the reference's text (ORBmatcher.cc:45-137, 1332-1472, 1603-1644,
Frame.cc:296-418, MapPoint.cc:372-417); no code computes it.  expected() is the oracle's answer, run_case() a library against both, check_case_contents() shows that each
case contains the gate it is for."""
import ctypes as C
import numpy as np
from oracle.oracle import KP_DTYPE
from sg_slam_amd.capi import _vp
from sg_slam_amd.matcher import ORBmatcher, camera_struct

f32 = np.float32
CAM = dict(fx=512.0, fy=512.0, cx=0.0, cy=0.0, bf=32.0, min_x=-12.5, max_x=655.25, min_y=-9.75, max_y=490.5)      # bounds like an undistorted frame's: cells are not 10 px
MB = f32(32.0) / f32(512.0)                            # Frame::mb, 0.0625 exactly
INVW = f32(64) / (f32(CAM['max_x']) - f32(CAM['min_x'])); INVH = f32(48) / (f32(CAM['max_y']) - f32(CAM['min_y']))
I4 = np.eye(4, dtype='f4')


def scales(n):
    s = [f32(1.0)]
    for _ in range(n - 1): s.append(f32(s[-1] * f32(1.2)))
    return np.array(s, 'f4')


SF = scales(8)
BASE = np.array([(37 * i + 11) & 255 for i in range(32)], np.uint8)


def desc(n):
    b = np.unpackbits(BASE); b[:n] ^= 1
    return np.packbits(b)


def cell(x, y):
    """Frame::PosInGrid (Frame.cc:409-418) under CAM"""
    return int(np.round(np.float64((f32(x) - f32(CAM['min_x'])) * INVW))), int(np.round(np.float64((f32(y) - f32(CAM['min_y'])) * INVH)))


def below(x): return np.nextafter(f32(x), f32(-np.inf))
def above(x): return np.nextafter(f32(x), f32(np.inf))
def inward(x): return np.nextafter(f32(x), f32(0))


def cur_of(rows, Tcw=I4):
    """current frame from rows (x, y, octave, flipped bits[, uright[, angle[, mp_obs]]])"""
    n = len(rows); k = np.zeros(n, KP_DTYPE); k['size'] = 31; k['class_id'] = -1
    d = np.zeros((n, 32), np.uint8); ur = np.full(n, -1, 'f4'); ob = np.full(n, -1, 'i4')
    for i, r in enumerate(rows):
        k['x'][i], k['y'][i], k['octave'][i] = r[0], r[1], r[2]; d[i] = desc(r[3])
        if len(r) > 4: ur[i] = r[4]
        if len(r) > 5: k['angle'][i] = r[5]
        if len(r) > 6: ob[i] = r[6]
    return dict(keys=k, desc=d, uright=ur, Tcw=np.array(Tcw, 'f4'), mp_obs=ob)


def mp(u=0.0, v=0.0, octave=0, n=0, obs=1, has=1, out=0, ang=0.0, xyz=None):
    """a last-frame map point that projects to (u, v) from z = 2 under the identity pose (or sits at xyz)"""
    return dict(xyz=(f32(u) / f32(256), f32(v) / f32(256), f32(2)) if xyz is None else xyz, octave=octave, n=n, obs=obs, has=has, out=out, ang=ang)


def last_of(pts, Tcw=I4):
    n = len(pts); k = np.zeros(n, KP_DTYPE); k['size'] = 31; k['class_id'] = -1
    k['octave'] = [p['octave'] for p in pts]; k['angle'] = [p['ang'] for p in pts]
    return dict(keys=k, has_mp=np.array([p['has'] for p in pts], np.uint8), outlier=np.array([p['out'] for p in pts], np.uint8),
                xw=np.array([p['xyz'] for p in pts], 'f4').reshape(n, 3), obs=np.array([p['obs'] for p in pts], 'i4'),
                mpdesc=np.array([desc(p['n']) for p in pts], np.uint8).reshape(n, 32), Tcw=np.array(Tcw, 'f4'))


def frame_case(name, cur, last, kat=None, th=15.0, mono=0, ori=1, **extra):
    return dict(name=name, kind='frame', cur=cur, last=last, th=th, mono=mono, ori=ori, kat=kat, **extra)


def lp(xyz, normal=(0, 0, 1), min_dist=0.1, max_dist=None, n=0, obs=1, skip=0, ratio=0.9):
    """a local map point; without max_dist the ratio max_dist / dist is `ratio` (0.9: predicted level 0)"""
    xyz = np.array(xyz, 'f4')
    return dict(xyz=xyz, normal=normal, min_dist=min_dist, max_dist=f32(ratio) * norm3(xyz) if max_dist is None else max_dist, n=n, obs=obs, skip=skip)


def at(u, v): return (f32(u) / f32(256), f32(v) / f32(256), f32(2))


def norm3(p):
    """cv::norm of a float 3-vector as isInFrustum uses it (camera centre at the origin): accumulated in double, returned as float"""
    return f32(np.sqrt(float(p[0]) * float(p[0]) + float(p[1]) * float(p[1]) + float(p[2]) * float(p[2])))


def local_of(pts):
    n = len(pts)
    return dict(xw=np.array([p['xyz'] for p in pts], 'f4').reshape(n, 3), normal=np.array([p['normal'] for p in pts], 'f4').reshape(n, 3),
                min_dist=np.array([p['min_dist'] for p in pts], 'f4'), max_dist=np.array([p['max_dist'] for p in pts], 'f4'),
                desc=np.array([desc(p['n']) for p in pts], np.uint8).reshape(n, 32), obs=np.array([p['obs'] for p in pts], 'i4'), skip=np.array([p['skip'] for p in pts], np.uint8))


def local_case(name, cur, lm, kat=None, th=3.0, nnratio=0.8, sf=SF, **extra):
    return dict(name=name, kind='local', cur=cur, lm=lm, th=th, nnratio=nnratio, sf=sf, kat=kat, **extra)


# ------------------------------------------------------------------------------------------------------------------ F1: level windows
TZ = [f32(0), MB, above(MB), f32(0.2), -MB, below(-MB), f32(-0.2)]           # tlc.z: neither, neither (strict >), forward, forward, neither, backward, backward
# scene 1: one map point of octave 3 at (320, 240), radius 15 * 1.728; keypoint k has octave k.  Distances: octave 0 -> 5, 7 -> 10, 2 -> 15, 4 -> 20, 3 -> 25, 1 -> 30,
# 5 -> 35, 6 -> 40.  Neither flag: levels 2..4, the smallest is octave 2.  Forward: levels >= 3, octave 7.  Backward: levels 0..3, octave 0.
S1_BITS = [5, 30, 15, 25, 20, 35, 40, 10]
S1_WIN = [2, 2, 7, 7, 2, 0, 0]
# scene 2: the map point has octave 0.  Keypoints: 0 octave 0 distance 30, 1 octave 1 distance 20, 2 octave 5 distance 10, 3 octave 2 distance 15.  Forward is
# GetFeaturesInArea(u, v, r, 0) with maxLevel -1: no level check at all, keypoint 2.  Neither: levels -1..1, keypoint 1.  Backward: level 0 only, keypoint 0.
S2_ROWS = [(320, 240, 0, 30), (322, 240, 1, 20), (324, 240, 5, 10), (326, 240, 2, 15)]
S2_WIN = [1, 1, 2, 2, 1, 0, 0]


def _one(n, k):
    m = [-1] * n; m[k] = 0
    return (m, 1)


def _f1():
    out = []
    s1 = [(320 + k, 240, k, S1_BITS[k]) for k in range(8)]
    for i, tz in enumerate(TZ):
        Tl = I4.copy(); Tl[2, 3] = tz                      # cur at the identity: tlc = tlw
        for mono in (0, 1):
            out.append(frame_case('F1_oct3_tz%d_mono%d' % (i, mono), cur_of(s1), last_of([mp(320, 240, octave=3)], Tl), _one(8, 2 if mono else S1_WIN[i]), mono=mono, f1=('oct3', i)))
            out.append(frame_case('F1_oct0_tz%d_mono%d' % (i, mono), cur_of(S2_ROWS), last_of([mp(320, 240, octave=0)], Tl), _one(4, 1 if mono else S2_WIN[i]), mono=mono, f1=('oct0', i)))
    # rotated last frame (yaw 0.5 rad about y): tlc.z = Rlw row 2 . twc + tlw.z = -sin(0.5) * 0.5 + 0.25 = 0.0103 < mb, while the translations alone (0.25) would say
    # forward.  Compared with the oracle only.
    c, s = np.cos(0.5), np.sin(0.5)
    Tl = np.array([[c, 0, s, 0], [0, 1, 0, 0], [-s, 0, c, 0.25], [0, 0, 0, 1]], 'f4'); Tc = I4.copy(); Tc[0, 3] = -0.5
    for mono in (0, 1):
        out.append(frame_case('F1_rotated_mono%d' % mono, cur_of(s1, Tc), last_of([mp(octave=3, xyz=(f32(1.75), f32(0.9375), f32(2)))], Tl), None, mono=mono))
    return out


# ------------------------------------------------------------------------------------------------------------------ F2: projection gates
def _f2():
    X0, X1, Y0, Y1 = (f32(CAM[k]) for k in ('min_x', 'max_x', 'min_y', 'max_y'))
    pts = [mp(xyz=(f32(-0.5), f32(-0.5), f32(-2))),       # 0  z_c < 0 (would land on keypoint 0 if the sign were ignored)
           mp(xyz=(f32(0.5), f32(0.5), f32(0))),          # 1  z_c == 0: u = v = +inf
           mp(xyz=(f32(-0.5), f32(0.5), f32(0))),         # 2  z_c == 0: u = -inf
           mp(X0, 100), mp(below(X0), 140),               # 3  u == minX kept, 4 one float outside
           mp(X1, 100), mp(above(X1), 140),               # 5, 6
           mp(200, Y0), mp(240, below(Y0)),               # 7, 8
           mp(200, Y1), mp(240, above(Y1)),               # 9, 10
           mp(320, 240, has=0), mp(400, 240, out=1),      # 11 no map point, 12 outlier
           mp(480, 240)]                                  # 13 control
    kp = [(128, 128), (-9.5, 100), (-9.5, 140), (645, 100), (645, 140), (200, -6), (240, -6), (200, 480), (240, 480), (320, 240), (400, 240), (480, 240)]
    kat = ([-1, 3, -1, 5, -1, 7, -1, 9, -1, -1, -1, 13], 5)
    return [frame_case('F2_projection_gates', cur_of([(x, y, 0, 0) for x, y in kp]), last_of(pts), kat, pairs=[(1, 2), (3, 4), (5, 6), (7, 8)])]


# ------------------------------------------------------------------------------------------------------------------ F3: grid edges
# keypoints: 0 rounds to column 64 (absent), 1 column 63, 2 rounds to row 48 (absent), 3 row 47, 4 x < minX and column -1 (absent), 5 x < minX but column 0 (present)
F3_KP = [(651, 200, 0, 0), (645, 200, 0, 10), (300, 486, 0, 0), (300, 480, 0, 12), (-20, 300, 0, 0), (-14, 300, 0, 14)]


def _f3():
    cur = cur_of(F3_KP)
    a = frame_case('F3_grid_edges', cur, last_of([mp(648, 200), mp(300, 483), mp(-10, 300)]), ([-1, 0, -1, 1, -1, 2], 3))
    # radius 700 around (320, 240): the cell window is clamped on all four sides.  Map point 0 (distance 0 to the absent keypoints) takes column 63 (distance 10, then 12, 14);
    # map point 1 = desc(20) sees 10 / 8 / 6 and takes the keypoint in column 0.
    b = frame_case('F3_window_clamped', cur, last_of([mp(320, 240), mp(320, 240, n=20)]), ([-1, 0, -1, -1, -1, 1], 2), th=700.0)
    return [a, b]


# ------------------------------------------------------------------------------------------------------------------ F4: radius and stereo gate (radius 15, ur = u - 16)
def _f4():
    rows = [(115, 100, 0, 0), (inward(115), 160, 0, 0), (200, 115, 0, 0), (260, inward(115), 0, 0),          # |dx| == r out, one float inside in; the same for y
            (100, 300, 0, 0, 99), (160, 300, 0, 0, above(159)),                                              # ur - kur == -15 kept, one float more rejected
            (220, 300, 0, 0, 189), (280, 300, 0, 0, inward(249)),                                            # ur - kur == +15 kept, one float more rejected
            (340, 300, 0, 0, 0), (400, 300, 0, 0, -1)]                                                       # kur == 0 and kur == -1: no stereo gate (|ur - kur| is 324 and 385)
    pts = [mp(100, 100), mp(100, 160), mp(200, 100), mp(260, 100), mp(100, 300), mp(160, 300), mp(220, 300), mp(280, 300), mp(340, 300), mp(400, 300)]
    return [frame_case('F4_radius_stereo', cur_of(rows), last_of(pts), ([-1, 1, -1, 3, 4, -1, 6, -1, 8, 9], 6), pairs=[(0, 1), (2, 3), (4, 5), (6, 7)])]


# ------------------------------------------------------------------------------------------------------------------ F5: distance and scan-order ties
def _f5():
    rows = [(50, 50, 0, 100), (50, 120, 0, 101),          # 0: best distance TH_HIGH matches, 1: 101 does not
            (206, 200, 0, 7), (198, 206, 0, 7),           # 2 (column 21, row 20) and 3 (column 20, row 21) tie: the lower column is scanned first
            (300, 206, 0, 7), (300, 200, 0, 7),           # 4 (column 30, row 21) and 5 (column 30, row 20) tie: the lower row
            (402, 301, 0, 7), (400, 299, 0, 7)]           # 6 and 7 in cell (40, 30): the lower index
    pts = [mp(50, 50), mp(50, 120), mp(202, 203), mp(300, 203), mp(401, 300)]
    return [frame_case('F5_distance_ties', cur_of(rows), last_of(pts), ([0, -1, -1, 2, -1, 3, 4, -1], 4), cells={2: (21, 20), 3: (20, 21), 4: (30, 21), 5: (30, 20), 6: (40, 30), 7: (40, 30)})]


# ------------------------------------------------------------------------------------------------------------------ F6: rotation histogram
def _slot(j): return (60 + 40 * (j % 6), 60 + 40 * (j // 6))


def _f6():
    # keypoints 0-3 -> bin 29 (rot 350 three times, and 10 - 20 = -10 wrapped), 4-6 -> bin 0 (rot 0, 354.5 and 359.9 through bin 30), 7-9 -> bin 7 (rot 84),
    # 10-11 -> bin 12 (rot 144).  Keypoint 7 is taken by map point 7 (unobserved, rot 144, bin 12) and again by map point 10 (rot 84, bin 7).
    # ComputeThreeMaxima: bins 0, 7, 12 hold 3 each and are seen in that order, bin 29 holds 4 and pushes bin 12 out of third place.  Bin 12 is rejected: keypoints
    # 7, 10, 11 are cleared and nmatches = 13 - 3.
    kang = [0, 0, 0, 20] + [0] * 8
    cur = cur_of([_slot(j) + (0, 0, -1, kang[j]) for j in range(12)])
    tgt = [0, 1, 2, 3, 4, 5, 6, 7, 10, 11, 7, 8, 9]
    ang = [350, 350, 350, 10, 0, 354.5, 359.9, 144, 144, 144, 84, 84, 84]
    last = last_of([mp(*_slot(tgt[i]), ang=ang[i], obs=0 if i == 7 else 1) for i in range(13)])
    out = [frame_case('F6_histogram_ori1', cur, last, ([0, 1, 2, 3, 4, 5, 6, -1, 11, 12, -1, -1], 10)),
           frame_case('F6_histogram_ori0', cur, last, ([0, 1, 2, 3, 4, 5, 6, 10, 11, 12, 8, 9], 13), ori=0)]
    # m2 == 0.1f * m1: ten assignments in bin 5 (rot 60), one in bin 9 (rot 108): 1 < 1.0f is false, the bin stays.  Eleven and one: 1 < 1.1f, it goes.
    for m1 in (10, 11):
        cur = cur_of([_slot(j) + (0, 0) for j in range(m1 + 1)])
        last = last_of([mp(*_slot(j), ang=60 if j < m1 else 108) for j in range(m1 + 1)])
        out.append(frame_case('F6_tenth_%d_and_1' % m1, cur, last, (list(range(m1)) + [m1 if m1 == 10 else -1], m1 + 1 if m1 == 10 else m1)))
    return out


# ------------------------------------------------------------------------------------------------------------------ F7: long lock chain
F7_THIRDS = [0, 1, 3, 4, 6, 7, 9, 10, 12, 13, 15, 16, 18, 19, 21, 22, 24, 25, 27, 28, 30, 31, 33, 34, 36, 37, 39, 40, 42, 43, 45, 46, 47] + [-1] * 15


def _f7(pad_to=0):
    # 48 keypoints within 6 px of (320, 240), keypoint k at distance k from BASE; 48 map points with BASE at (320, 240).  All observed: map point i finds 0..i-1 locked and
    # takes keypoint i.  Every third one (i % 3 == 2) unobserved: it takes the best free keypoint without locking it and the next map point takes the same one, so keypoint 2g
    # ends with map point 3g, keypoint 2g + 1 with 3g + 1, keypoint 32 with the last (unobserved) point 47, and every one of the 48 assignments counts.
    rows = [(314 + 2 * (k % 7), 234 + 2 * (k // 7), 0, k) for k in range(48)]
    out = [frame_case('F7_chain', cur_of(rows), last_of([mp(320, 240) for _ in range(48)]), (list(range(48)), 48)),
           frame_case('F7_chain_thirds', cur_of(rows), last_of([mp(320, 240, obs=0 if i % 3 == 2 else 1) for i in range(48)]), (F7_THIRDS, 48))]
    # the chain inside a frame of exactly 256 keypoints and map points (for the batch entry's clamp): the others are far away and hold no map point
    far = [(600 - 3 * (j % 60), 400 + 3 * (j // 60), 0, 200) for j in range(208)]
    out.append(frame_case('F7_chain_256', cur_of(rows + far), last_of([mp(320, 240) for _ in range(48)] + [mp(20, 20, has=0) for _ in range(208)]), (list(range(48)) + [-1] * 208, 48)))
    return out


# ------------------------------------------------------------------------------------------------------------------ F8: sizes
def _rand_desc(rng, n): return rng.integers(0, 256, (n, 32)).astype(np.uint8)


def _flip(rng, d, kmax):
    out = d.copy()
    for i in range(len(d)):
        b = np.unpackbits(out[i]); b[rng.choice(256, rng.integers(0, kmax + 1), replace=False)] ^= 1; out[i] = np.packbits(b)
    return out


def _lattice(rng, n):
    c = np.concatenate([rng.permutation(1200), rng.integers(0, 1200, max(n - 1200, 0))])[:n]
    return 20 + (c % 40) * 15.0 + rng.uniform(-4, 4, n), 20 + (c // 40) * 14.5 + rng.uniform(-4, 4, n)


def _f8(n=1280, seed=8):
    rng = np.random.default_rng(seed)
    x, y = _lattice(rng, n); z = rng.uniform(2, 5, n)
    lk = np.zeros(n, KP_DTYPE); lk['x'] = x; lk['y'] = y; lk['octave'] = rng.integers(0, 6, n); lk['angle'] = rng.uniform(0, 360, n); lk['size'] = 31; lk['class_id'] = -1
    xw = np.stack([x * z / 512, y * z / 512, z], 1).astype('f4'); ld = _rand_desc(rng, n)
    last = dict(keys=lk, has_mp=(rng.random(n) < 0.9).astype(np.uint8), outlier=(rng.random(n) < 0.05).astype(np.uint8), xw=xw, obs=(rng.random(n) < 0.6).astype('i4') * 3,
                mpdesc=ld, Tcw=I4.copy())
    Tc = I4.copy(); Tc[2, 3] = -0.2                       # the camera moved forward by 0.2 m: tlc.z = 0.2 > mb
    zc = z - 0.2; p = rng.permutation(n)
    ck = np.zeros(n, KP_DTYPE); ck['x'] = (512 * xw[:, 0] / zc + rng.normal(0, 0.5, n))[p]; ck['y'] = (512 * xw[:, 1] / zc + rng.normal(0, 0.5, n))[p]
    ck['octave'] = (lk['octave'] + rng.integers(-1, 2, n))[p].clip(0, 7); ck['angle'] = ((lk['angle'] + rng.normal(0, 3, n)) % 360)[p]; ck['size'] = 31; ck['class_id'] = -1
    ur = np.where(rng.random(n) < 0.5, ck['x'] - (32 / zc)[p] + rng.normal(0, 0.3, n), -1).astype('f4')
    cur = dict(keys=ck, desc=_flip(rng, ld, 30)[p], uright=ur, Tcw=Tc, mp_obs=np.full(n, -1, 'i4'))
    return cur, last


def _sub_frame(cur, last, nc, nl):
    return {k: (v if k == 'Tcw' else v[:nc]) for k, v in cur.items()}, {k: (v if k == 'Tcw' else v[:nl]) for k, v in last.items()}


def _f8_cases():
    cur, last = _f8()
    c64, l64 = _f8(64, seed=9); Tc = cur['Tcw']
    return [frame_case('F8_1280', cur, last, None),
            frame_case('F8_1x1', cur_of([(333.5, 222.25, 0, 3)], Tc), last_of([mp(300, 200)]), None),          # (300, 200) seen from 0.2 m nearer: (333.3, 222.2)
            frame_case('F8_no_keypoints', *_sub_frame(c64, l64, 0, 64), None), frame_case('F8_no_map_points', *_sub_frame(c64, l64, 64, 0), None)]


# ------------------------------------------------------------------------------------------------------------------ L1: frustum
def _step_to(p, axis, target, up):
    """move one coordinate of p float by float until norm3(p) is `target`"""
    p = np.array(p, 'f4')
    for _ in range(8):
        if norm3(p) == target: return p
        p[axis] = above(p[axis]) if up else below(p[axis])
    raise AssertionError('no float with that norm nearby')


def _l1():
    X0, X1, Y0, Y1 = (f32(CAM[k]) for k in ('min_x', 'max_x', 'min_y', 'max_y'))
    # 0.8f = 13421773 * 2^-24 and 13421773 = 53 * 253241, 53^2 = 28^2 + 45^2: with min_dist = 4 the product 0.8f * 4 is exact, and (0, 28, 45) * 253241 * 2^-22 has that norm
    # exactly.  1.2f = 5033165 * 2^-22 and 5033165 = 5 * 1006633, 5^2 = 3^2 + 4^2: with max_dist = 2 the product 1.2f * 2 is exact and (3, 0, 4) * 1006633 * 2^-21 has that norm.
    dmin = f32(0.8) * f32(4.0); dmax = f32(1.2) * f32(2.0)
    on_min = np.array([0, 28 * 253241, 45 * 253241], 'f4') * f32(2.0 ** -22); on_max = np.array([3 * 1006633, 0, 4 * 1006633], 'f4') * f32(2.0 ** -21)
    under_min = _step_to(on_min[[1, 0, 2]], 2, inward(dmin), False); over_max = _step_to(on_max[[1, 0, 2]], 2, above(dmax), True)
    pts = [lp(at(100, 100), skip=1),                                            # 0  skip
           lp((-0.5, -0.5, -2), normal=(0, 0, -1)),                             # 1  z_c < 0
           lp(at(X0, 100)), lp(at(below(X0), 140)),                             # 2  u == minX kept, 3 one float outside
           lp(at(X1, 100)), lp(at(above(X1), 140)),                             # 4, 5
           lp(at(200, Y0)), lp(at(240, below(Y0))),                             # 6, 7
           lp(at(200, Y1)), lp(at(240, above(Y1))),                             # 8, 9
           lp(on_min, min_dist=4.0, max_dist=3.0), lp(under_min, min_dist=4.0, max_dist=3.0),      # 10 dist == 0.8f * min_dist kept, 11 one float below
           lp(on_max, max_dist=2.0), lp(over_max, max_dist=2.0),                # 12 dist == 1.2f * max_dist kept, 13 one float above
           lp((0, 0, 2), normal=(0, 0, 0.5)),                                   # 14 viewCos == 0.5 kept; it is observed and locks keypoint 14
           lp((0, 0, 2), normal=(0, 0, inward(0.5)), n=30),                     # 15 one float below: out of view; in view it would take keypoint 15 (distance 0)
           lp(at(300, 200))]                                                    # 16 control
    kp = [(100, 100), (128, 128), (-9.5, 100), (-9.5, 140), (649, 100), (649, 140), (200, -6), (240, -6), (200, 484), (240, 484), (0, 318.5), (318.5, 0), (384, 0), (0, 384),
          (0, 0), (0, 0), (300, 200)]
    cur = cur_of([(x, y, 0, 30 if i == 15 else 0) for i, (x, y) in enumerate(kp)])
    kat = ([-1, -1, 2, -1, 4, -1, 6, -1, 8, -1, 10, -1, 12, -1, 14, -1, 16], 8, [0, 0, 1, 0, 1, 0, 1, 0, 1, 0, 1, 0, 1, 0, 1, 0, 1])
    return [local_case('L1_frustum', cur, local_of(pts), kat, pairs=[(2, 3), (4, 5), (6, 7), (8, 9), (10, 11), (12, 13), (14, 15)], dist_targets={10: dmin, 11: inward(dmin), 12: dmax, 13: above(dmax)})]


# ------------------------------------------------------------------------------------------------------------------ L2: search radius
def _l2():
    # one point at (0, 0, 2) seen at level 0; keypoint 0 at 3 px (distance 20), keypoint 1 at 9 px (distance 0).  viewCos = 2 * nz / 2 = nz exactly.
    # RadiusByViewingCos compares in double with the literal 0.998.  0.998f is 0.99800002575: ABOVE the literal, so viewCos == 0.998f takes the 2.5 radius (a comparison
    # in float, viewCos > 0.998f, would take 4.0), and the float below it, 0.99799996614, is the largest that takes 4.0.
    # 4.0, th 1: r = 4, keypoint 0 alone.  th 3: r = 12, both, keypoint 1 wins (0 against 20 passes the ratio test).
    # 2.5, th 1: r = 2.5, nothing.  th 3: r = 7.5, keypoint 0 alone.
    cur = cur_of([(3, 0, 0, 20), (9, 0, 0, 0)]); c = f32(0.998)
    mk = lambda nz: local_of([lp((0, 0, 2), normal=(0, 0, nz))])
    return [local_case('L2_r4.0_th1', cur, mk(below(c)), ([0, -1], 1, [1]), th=1.0), local_case('L2_r2.5_th1', cur, mk(c), ([-1, -1], 0, [1]), th=1.0),
            local_case('L2_r4.0_th3', cur, mk(below(c)), ([-1, 0], 1, [1]), th=3.0), local_case('L2_r2.5_th3', cur, mk(c), ([0, -1], 1, [1]), th=3.0)]


# ------------------------------------------------------------------------------------------------------------------ L3: predicted level
def _l3a():
    # th 1.  a: ratio 1 -> level 0, which admits octave 0 only.  b: ratio 0.9 -> ceil(-0.58) -> 0 (a level below 0 needs ratio <= 1 / 1.2, which is where dist > 1.2 * max_dist
    # begins: the lower clamp can only act on the equality that L1 has).  c: ratio 10 -> ceil(12.6) clamped to 7: octaves 6, 7.  d1, d2: ratio 1.6 -> level 3: octaves 2 and 3,
    # not 1 and 4 (the refused ones have the smallest distances).
    pts = [lp((0, 0, 2), max_dist=2.0), lp((3, 0, 4), max_dist=4.5), lp((0, 3, 4), max_dist=50.0), lp((4, 1, 8), max_dist=f32(14.4)), lp((1, 4, 8), max_dist=f32(14.4))]
    rows = [(0, 0, 0, 10), (0, 0, 1, 0), (384, 0, 0, 10), (384, 0, 1, 0), (0, 384, 7, 10), (0, 384, 5, 0),
            (256, 64, 1, 0), (256, 64, 4, 2), (256, 64, 3, 10), (256, 64, 2, 20), (64, 256, 1, 0), (64, 256, 4, 2), (64, 256, 2, 10)]
    return [local_case('L3a_levels', cur_of(rows), local_of(pts), ([0, -1, 1, -1, 2, -1, -1, -1, 3, -1, -1, -1, 4], 5, [1] * 5), th=1.0)]


def sweep_ratios(ks):
    """13 consecutive floats around float(1.2f^k)"""
    s = scales(10); out = []
    for k in ks:
        r = s[k]
        for _ in range(6): r = below(r)
        for _ in range(13): out.append((k, r)); r = above(r)
    return out


def sweep_case(ratio, nlevels):
    """dist = 1 exactly, max_dist = ratio; one keypoint per octave at the projection, the higher octave the nearer: of the two admitted octaves (level - 1, level) the level's
    own wins, so the matched keypoint's index is the predicted level"""
    cur = cur_of([(0, 0, o, 10 * (nlevels - 1 - o)) for o in range(nlevels)])
    return local_case('L3b_%r_%d' % (float(ratio), nlevels), cur, local_of([lp((0, 0, 1), max_dist=ratio)]), None, th=1.0, sf=scales(nlevels))


# ------------------------------------------------------------------------------------------------------------------ L4: ratio test (level 3: octaves 2, 3; nnratio 0.8f)
def _l4():
    px = [100, 160, 220, 280, 340, 400, 400, 460, 520]
    pts = [lp(at(x, 200), ratio=1.6, n=50 if i == 5 else 0) for i, x in enumerate(px)]
    rows = [(100, 200, 3, 41), (100, 200, 3, 50),                     # 0: 41 > 0.8f * 50 on one level: rejected
            (160, 200, 3, 40), (160, 200, 3, 50),                     # 1: 40 > 40.0000006 is false: accepted
            (220, 200, 3, 41), (220, 200, 2, 50),                     # 2: different levels: accepted
            (280, 200, 3, 90),                                        # 3: one candidate, the second distance stays 256
            (340, 200, 3, 41), (340, 200, 3, 50, -1, 0, 1), (340, 200, 3, 60),        # 4: the 50 holds an observed map point from the start, the second is 60: accepted
            (400, 200, 3, 41), (400, 200, 3, 50), (400, 200, 3, 60),  # 5 = desc(50) takes the 50 (0 against 9) and locks it; 6 then sees 41 and 60: accepted
            (460, 200, 3, 100), (520, 200, 3, 101)]                   # 7: TH_HIGH accepted, 8: 101 not
    kat = ([-1, -1, 1, -1, 2, -1, 3, 4, -1, -1, 6, 5, -1, 7, -1], 7, [1] * 9)
    return [local_case('L4_ratio_test', cur_of(rows), local_of(pts), kat)]


# ------------------------------------------------------------------------------------------------------------------ L5: sizes
L5_GATES = ('behind', 'bounds', 'near', 'far', 'cos')


def _l5(nm=4096, nc=1280, seed=5):
    rng = np.random.default_rng(seed)
    a, b = 0.05, -0.03
    R = np.array([[np.cos(a), 0, np.sin(a)], [0, 1, 0], [-np.sin(a), 0, np.cos(a)]]) @ np.array([[1, 0, 0], [0, np.cos(b), -np.sin(b)], [0, np.sin(b), np.cos(b)]])
    t = np.array([0.1, -0.05, 0.2]); Tc = I4.copy(); Tc[:3, :3] = R; Tc[:3, 3] = t; Ow = -R.T @ t
    x, y = _lattice(rng, nc); z = rng.uniform(2, 6, nc)
    ck = np.zeros(nc, KP_DTYPE); ck['x'] = x; ck['y'] = y; ck['octave'] = rng.integers(0, 8, nc); ck['size'] = 31; ck['class_id'] = -1
    cd = _rand_desc(rng, nc)
    cur = dict(keys=ck, desc=cd, uright=np.where(rng.random(nc) < 0.5, x - 32 / z + rng.normal(0, 0.3, nc), -1).astype('f4'), Tcw=Tc,
               mp_obs=rng.choice([-1, 0, 2], nc, p=[0.8, 0.1, 0.1]).astype('i4'))
    k = np.concatenate([rng.permutation(nc), rng.integers(0, nc, nm - nc)])[:nm]          # every keypoint is wanted by one of the first nc points and by later ones
    gate = rng.choice(len(L5_GATES) + 1, nm, p=[0.025] * 5 + [0.875]); gate[0] = 5
    pc = np.stack([x[k] * z[k] / 512, y[k] * z[k] / 512, z[k]], 1) + rng.normal(0, 0.002, (nm, 3))
    pc[gate == 0] *= -1; pc[gate == 1, 0] *= 3
    P = (pc - t) @ R; PO = P - Ow; dist = np.linalg.norm(PO, axis=1)
    nrm = PO / dist[:, None]
    tilt = (rng.random(nm) < 0.2) | (gate == 4); c = np.where(gate == 4, 0.3, 0.95)
    perp = np.cross(nrm, [0, 1, 0]); perp /= np.linalg.norm(perp, axis=1, keepdims=True)
    nrm[tilt] = (c[:, None] * nrm + np.sqrt(1 - c * c)[:, None] * perp)[tilt]
    mx = dist * 1.2 ** (ck['octave'][k] - 0.5); mn = mx / 1.2 ** 7
    mn[gate == 2] = dist[gate == 2] * 1.5; mx[gate == 3] = dist[gate == 3] * 0.7
    lm = dict(xw=P.astype('f4'), normal=nrm.astype('f4'), min_dist=mn.astype('f4'), max_dist=mx.astype('f4'), desc=_flip(rng, cd[k], 25), obs=(rng.random(nm) < 0.7).astype('i4') * 2,
              skip=(rng.random(nm) < 0.03).astype(np.uint8))
    lm['skip'][0] = 0
    return cur, lm, gate


def _l5_cases():
    cur, lm, gate = _l5()
    sub = lambda n: {k: v[:n] for k, v in lm.items()}
    return [local_case('L5_4096', cur, lm, None, gate=gate), local_case('L5_1025', cur, sub(1025), None), local_case('L5_1', cur, sub(1), None)]


def _build():
    return _f1() + _f2() + _f3() + _f4() + _f5() + _f6() + _f7() + _f8_cases() + _l1() + _l2() + _l3a() + _l4() + _l5_cases()


CASES = _build()
CASE = {c['name']: c for c in CASES}
NAMES = [c['name'] for c in CASES]
assert len(CASE) == len(CASES)
# at most 64 keypoints and 64 map points everywhere but in the size cases (F8, L5) and the 256-keypoint frame of the batch entry
assert all(len(c['cur']['keys']) <= 64 and len(c.get('last', c.get('lm'))['xw']) <= 64 for c in CASES if not c['name'].startswith(('F8_', 'L5_', 'F7_chain_256')))


# ------------------------------------------------------------------------------------------------------------------ running
def run_oracle(oracle, c, **kw):
    """(match, nmatches) or (match, nmatches, in_view) of the oracle; kw overrides th / mono / ori / last / lm"""
    c = dict(c, **kw)
    if c['kind'] == 'frame':
        m, n = oracle.search_by_projection_frame(c['cur'], c['last'], CAM, SF, th=c['th'], mono=bool(c['mono']), check_ori=bool(c['ori']))
        return m.copy(), n
    m, n, v = oracle.search_by_projection_local(c['cur'], c['lm'], CAM, c['sf'], th=c['th'], nnratio=c['nnratio'])
    return m.copy(), n, v.copy()


def run_lib(lib, c):
    if c['kind'] == 'frame':
        cur = dict(c['cur']); n = ORBmatcher(0.9, bool(c['ori']), lib=lib).SearchByProjection(cur, c['last'], c['th'], bool(c['mono']), CAM, SF)
        return cur['match'], n
    cur = dict(c['cur']); lm = dict(c['lm']); n = ORBmatcher(c['nnratio'], True, lib=lib).SearchByProjectionLocal(cur, lm, c['th'], CAM, c['sf'])
    return cur['match_local'], n, lm['in_view']


_EXPECTED = {}


def expected(oracle, name):
    if name not in _EXPECTED: _EXPECTED[name] = run_oracle(oracle, CASE[name])
    return _EXPECTED[name]


def same(got, want, what):
    assert len(got) == len(want), what
    assert np.array_equal(np.asarray(got[0]), np.asarray(want[0], 'i4')), (what, 'match', list(np.asarray(got[0])[:64]), list(np.asarray(want[0])[:64]))
    assert int(got[1]) == int(want[1]), (what, 'nmatches', got[1], want[1])
    if len(want) == 3: assert np.array_equal(np.asarray(got[2]), np.asarray(want[2], np.uint8)), (what, 'in_view', list(np.asarray(got[2])[:64]), list(np.asarray(want[2])[:64]))


def check_kat(oracle, c):
    """the oracle gives the hand-written answer"""
    if c['kat'] is not None: same(expected(oracle, c['name']), c['kat'], (c['name'], 'oracle against the known answer'))


def run_case(lib, oracle, c):
    got = run_lib(lib, c)
    if c['kat'] is not None: same(got, c['kat'], (c['name'], 'library against the known answer'))
    same(got, expected(oracle, c['name']), (c['name'], 'library against the oracle'))
    return got


def sweep(run, ks, nlevels):
    """the matched keypoint (= predicted level) for every ratio of sweep_ratios(ks); run(case) -> (match, n, in_view)"""
    out = []
    for k, r in sweep_ratios(ks):
        m, n, v = run(sweep_case(r, nlevels))
        assert n == 1 and v[0] == 1 and (np.asarray(m) >= 0).sum() == 1, (k, float(r), list(m), n)
        out.append(int(np.flatnonzero(np.asarray(m) >= 0)[0]))
    return out


# ------------------------------------------------------------------------------------------------------------------ batch entries
class Dev:
    """device arrays for a batch entry: torch tensors filled on a stream of their own, or numpy arrays with the emulator"""
    def __init__(self, lib):
        self.host = 'EMULATOR' in lib.version()
        if not self.host:
            import torch
            self.torch = torch; self.s = torch.cuda.Stream(); assert self.s.cuda_stream != torch.cuda.default_stream().cuda_stream

    def up(self, a):
        a = np.ascontiguousarray(a); a = a.view(np.uint8) if a.dtype.fields else a
        if self.host: return a.copy()
        with self.torch.cuda.stream(self.s): return self.torch.from_numpy(a).cuda()

    def stream(self): return None if self.host else C.c_void_p(self.s.cuda_stream)

    def down(self, a):
        if self.host: return a
        self.s.synchronize(); return a.cpu().numpy()


def _rows(B, cap, arrs, tail=(), dtype=None):
    out = np.zeros((B, cap) + tail, dtype or arrs[0].dtype)
    for f, a in enumerate(arrs): out[f, :len(a)] = a
    return out


def frame_batch(lib, cases, cap, counts=None, fill=-7):
    """sgx_match_project_frame_batch_dev on `cases` as one launch (same th, mono, ori); counts[f] = (cn, ln) overrides what the entry is told.  Returns (cur_match[B, cap], nmatches[B])"""
    B = len(cases); D = Dev(lib); c0 = cases[0]; cu = [c['cur'] for c in cases]; la = [c['last'] for c in cases]
    assert all((c['th'], c['mono'], c['ori']) == (c0['th'], c0['mono'], c0['ori']) for c in cases)
    n = np.array(counts if counts is not None else [(len(c['keys']), len(l['keys'])) for c, l in zip(cu, la)], 'i4')
    args = [_rows(B, cap, [c['keys'] for c in cu]), _rows(B, cap, [c['desc'] for c in cu], (32,)), _rows(B, cap, [c['uright'] for c in cu]), n[:, 0].copy(),
            np.stack([c['Tcw'].reshape(16) for c in cu]), _rows(B, cap, [l['keys'] for l in la]), n[:, 1].copy(), _rows(B, cap, [l['has_mp'] for l in la]),
            _rows(B, cap, [l['outlier'] for l in la]), _rows(B, cap, [l['xw'] for l in la], (3,)), _rows(B, cap, [l['obs'] for l in la]), _rows(B, cap, [l['mpdesc'] for l in la], (32,)),
            np.stack([l['Tcw'].reshape(16) for l in la])]
    dev = [D.up(a) for a in args]; match = D.up(np.full((B, cap), fill, 'i4')); nm = D.up(np.full(B, fill, 'i4')); cs = camera_struct(CAM)
    lib.check(lib.dll.sgx_match_project_frame_batch_dev(B, cap, *[_vp(a) for a in dev], C.byref(cs), _vp(SF), len(SF), float(c0['th']), int(c0['mono']), int(c0['ori']),
                                                        _vp(match), _vp(nm), D.stream()), 'sgx_match_project_frame_batch_dev')
    return D.down(match), D.down(nm)


def local_batch(lib, cases, cap, mcap, fill=-7, view_fill=0xA5):
    """sgx_match_project_local_batch_dev on `cases` as one launch (same th, nnratio).  Returns (cur_match[B, cap], nmatches[B], in_view[B, mcap])"""
    B = len(cases); D = Dev(lib); c0 = cases[0]; cu = [c['cur'] for c in cases]; lm = [c['lm'] for c in cases]
    assert all((c['th'], c['nnratio']) == (c0['th'], c0['nnratio']) for c in cases)
    args = [_rows(B, cap, [c['keys'] for c in cu]), _rows(B, cap, [c['desc'] for c in cu], (32,)), _rows(B, cap, [c['uright'] for c in cu]), np.array([len(c['keys']) for c in cu], 'i4'),
            np.stack([c['Tcw'].reshape(16) for c in cu]), _rows(B, cap, [c['mp_obs'] for c in cu])]
    margs = [np.array([len(m['xw']) for m in lm], 'i4'), _rows(B, mcap, [m['xw'] for m in lm], (3,), 'f4'), _rows(B, mcap, [m['normal'] for m in lm], (3,), 'f4'),
             _rows(B, mcap, [m['min_dist'] for m in lm], (), 'f4'), _rows(B, mcap, [m['max_dist'] for m in lm], (), 'f4'), _rows(B, mcap, [m['desc'] for m in lm], (32,), np.uint8),
             _rows(B, mcap, [m['obs'] for m in lm], (), 'i4'), _rows(B, mcap, [m['skip'] for m in lm], (), np.uint8)]
    dev = [D.up(a) for a in args]; mdev = [D.up(a) for a in margs]
    match = D.up(np.full((B, cap), fill, 'i4')); nm = D.up(np.full(B, fill, 'i4')); view = D.up(np.full((B, mcap), view_fill, np.uint8)); cs = camera_struct(CAM)
    lib.check(lib.dll.sgx_match_project_local_batch_dev(B, cap, *[_vp(a) for a in dev], mcap, *[_vp(a) for a in mdev], C.byref(cs), _vp(SF), len(SF), float(np.log(np.float32(SF[1]))),
                                                        float(c0['th']), float(c0['nnratio']), 0.5, _vp(match), _vp(nm), _vp(view), D.stream()), 'sgx_match_project_local_batch_dev')
    return D.down(match), D.down(nm), D.down(view)


def empty_frame():
    return frame_case('empty', cur_of([]), last_of([]), ([], 0))


def check_frame_batch(lib, oracle):
    """F9: four frames in one launch, cap 256: F1 (tlc.z 0.2), F2, F7 inside 256 keypoints and told 261 (the clamp to cap), an empty frame; cur_match prefilled with -7"""
    cap = 256; cs = [CASE['F1_oct3_tz3_mono0'], CASE['F2_projection_gates'], CASE['F7_chain_256'], empty_frame()]
    m, nm = frame_batch(lib, cs, cap, counts=[(8, 1), (12, 14), (cap + 5, cap + 5), (0, 0)])
    for f, c in enumerate(cs):
        n = len(c['cur']['keys']); single = run_lib(lib, c) if n else ([], 0)
        assert np.array_equal(m[f, :n], np.asarray(single[0], 'i4')) and np.array_equal(m[f, :n], np.asarray(c['kat'][0], 'i4')), (c['name'], list(m[f, :n]))
        assert (m[f, n:] == -1).all(), (c['name'], 'rows beyond n')
        assert nm[f] == single[1] == c['kat'][1], (c['name'], nm[f], single[1])


def check_local_batch(lib, oracle):
    """L6: L1, L4 and an empty local map in one launch, cap 128, mcap 256.  include/sgx.h: in_view rows [mn, mcap) are not written, so nothing is asserted about them"""
    cap, mcap = 128, 256; l4 = CASE['L4_ratio_test']
    cs = [CASE['L1_frustum'], l4, local_case('L6_empty_map', l4['cur'], local_of([]), ([-1] * 15, 0, []))]
    m, nm, view = local_batch(lib, cs, cap, mcap)
    for f, c in enumerate(cs):
        n = len(c['cur']['keys']); mn = len(c['lm']['xw']); single = run_lib(lib, c)
        same((m[f, :n], nm[f], view[f, :mn]), single, (c['name'], 'batch against the single call')); same((m[f, :n], nm[f], view[f, :mn]), c['kat'], (c['name'], 'batch against the known answer'))
        assert (m[f, n:] == -1).all(), (c['name'], 'rows beyond n')


# ------------------------------------------------------------------------------------------------------------------ what each case is for
def _frustum_first_fail(cur, lm):
    """first isInFrustum gate each local map point fails (index into L5_GATES, 5 = in view, -1 = skipped), in double"""
    T = cur['Tcw'].astype('f8'); R, t = T[:3, :3], T[:3, 3]; Ow = -R.T @ t; P = lm['xw'].astype('f8'); pc = P @ R.T + t
    with np.errstate(all='ignore'):
        u = 512 * pc[:, 0] / pc[:, 2]; v = 512 * pc[:, 1] / pc[:, 2]
        PO = P - Ow; d = np.linalg.norm(PO, axis=1); cos = (PO * lm['normal']).sum(1) / d
    fails = [pc[:, 2] < 0, (u < CAM['min_x']) | (u > CAM['max_x']) | (v < CAM['min_y']) | (v > CAM['max_y']), d < 0.8 * lm['min_dist'], d > 1.2 * lm['max_dist'], cos < 0.5]
    out = np.full(len(P), 5)
    for g in reversed(range(5)): out[fails[g]] = g
    out[lm['skip'] > 0] = -1
    return out


def check_case_contents(oracle):
    """each case contains what it is for"""
    E = lambda n: expected(oracle, n)
    assert np.array_equal(SF, oracle.orb_params()['scale'])
    for n in range(0, 120, 7): assert oracle.descriptor_distance(desc(n), BASE) == n and oracle.descriptor_distance(desc(n), desc(33)) == abs(n - 33)
    # F1: bMono changes the answer exactly where |tlc.z| > mb
    for scene in ('oct3', 'oct0'):
        for i, tz in enumerate(TZ):
            a, b = E('F1_%s_tz%d_mono0' % (scene, i)), E('F1_%s_tz%d_mono1' % (scene, i))
            assert (abs(float(tz)) > float(MB)) == (not np.array_equal(a[0], b[0])), (scene, i)
            assert CASE['F1_%s_tz%d_mono0' % (scene, i)]['last']['Tcw'][2, 3] == tz
    assert float(TZ[1]) == 0.0625 and TZ[2] > MB and TZ[5] < -MB and len({tuple(E('F1_oct0_tz%d_mono0' % i)[0]) for i in (0, 3, 6)}) == 3
    c = CASE['F1_rotated_mono0']; Tl = c['last']['Tcw'].astype('f8'); twc = -c['cur']['Tcw'][:3, 3].astype('f8')
    tlc = Tl[:3, :3] @ twc + Tl[:3, 3]
    assert np.linalg.norm(tlc) > MB and abs(tlc[2]) < MB < twc[2] + Tl[2, 3]            # the neither-flag path, which only Rlw's third row shows
    assert np.array_equal(E('F1_rotated_mono0')[0], E('F1_rotated_mono1')[0]) and E('F1_rotated_mono0')[1] == 1 and E('F1_rotated_mono0')[0][2] == 0
    # F2, F4: the members of each kept / dropped pair answer differently (a pair names the two keypoints)
    m = E('F2_projection_gates')[0]
    for a, b in CASE['F2_projection_gates']['pairs']: assert m[a] >= 0 and m[b] == -1, (a, b)
    with np.errstate(divide='ignore'): assert np.isinf(CASE['F2_projection_gates']['last']['xw'][1:3, :2] / CASE['F2_projection_gates']['last']['xw'][1:3, 2:]).all()
    m = E('F4_radius_stereo')[0]
    for a, b in CASE['F4_radius_stereo']['pairs']: assert {m[a] >= 0, m[b] >= 0} == {True, False}, (a, b)
    k = CASE['F4_radius_stereo']['cur']['keys']
    assert k['x'][0] - f32(100) == f32(15) and k['x'][1] - f32(100) < f32(15) and k['y'][2] - f32(100) == f32(15) and k['y'][3] - f32(100) < f32(15)
    # F3: the column-64 keypoint lies within the radius of a map point whose descriptor equals its own; the others sit where the case says
    assert cell(*F3_KP[0][:2])[0] == 64 and cell(*F3_KP[1][:2])[0] == 63 and cell(*F3_KP[2][:2])[1] == 48 and cell(*F3_KP[3][:2])[1] == 47 and cell(*F3_KP[4][:2])[0] == -1 and \
        cell(*F3_KP[5][:2])[0] == 0 and F3_KP[4][0] < CAM['min_x'] and F3_KP[5][0] < CAM['min_x']
    c = CASE['F3_grid_edges']; u = c['last']['xw'][0, 0] * 256; v = c['last']['xw'][0, 1] * 256
    assert abs(F3_KP[0][0] - u) < 15 and abs(F3_KP[0][1] - v) < 15 and np.array_equal(c['last']['mpdesc'][0], c['cur']['desc'][0])
    for lo, hi, inv, c0, n in ((320 - 700, 320 + 700, INVW, CAM['min_x'], 64), (240 - 700, 240 + 700, INVH, CAM['min_y'], 48)):
        assert np.floor((lo - c0) * inv) < 0 and np.ceil((hi - c0) * inv) > n - 1
    # F5: the tied candidates have equal distance and lie in the cells the case names
    c = CASE['F5_distance_ties']; kk = c['cur']['keys']
    for i, want in c['cells'].items(): assert cell(kk['x'][i], kk['y'][i]) == want, (i, cell(kk['x'][i], kk['y'][i]))
    for (a, b), mpi in (((2, 3), 2), ((4, 5), 3), ((6, 7), 4)):
        assert oracle.descriptor_distance(c['cur']['desc'][a], c['last']['mpdesc'][mpi]) == oracle.descriptor_distance(c['cur']['desc'][b], c['last']['mpdesc'][mpi]) == 7
    # F6
    assert not np.array_equal(E('F6_histogram_ori1')[0], E('F6_histogram_ori0')[0]) and E('F6_histogram_ori1')[1] != E('F6_histogram_ori0')[1]
    # F7: the identity chain, and it hangs on map point 0
    assert np.array_equal(E('F7_chain')[0], np.arange(48))
    c = CASE['F7_chain']; l = {k: (v if k == 'Tcw' else v[1:]) for k, v in c['last'].items()}
    assert not np.array_equal(run_oracle(oracle, c, last=l)[0], np.arange(48))
    # F8
    c = CASE['F8_1280']; assert len(c['cur']['keys']) == 1280 and len(c['last']['keys']) == 1280 and E('F8_1280')[1] >= 300
    assert -c['cur']['Tcw'][2, 3] > MB and not np.array_equal(E('F8_1280')[0], run_oracle(oracle, c, mono=1)[0]) and (E('F8_1280')[0] >= 1024).sum() >= 20
    assert E('F8_1x1')[1] == 1
    # L1, L2
    m, _, v = E('L1_frustum'); c = CASE['L1_frustum']
    for a, b in c['pairs']: assert (v[a], v[b], m[a], m[b]) == (1, 0, a, -1), (a, b)
    for i, d in c['dist_targets'].items(): assert norm3(c['lm']['xw'][i]) == d, i
    assert f32(0.8) * f32(4.0) == c['dist_targets'][10] and float(f32(0.8)) * 4.0 == float(c['dist_targets'][10]) and float(f32(1.2)) * 2.0 == float(c['dist_targets'][12])
    assert float(below(f32(0.998))) < 0.998 < float(f32(0.998)) and CASE['L2_r2.5_th1']['lm']['normal'][0, 2] == f32(0.998)
    for th in (1, 3): assert not np.array_equal(E('L2_r4.0_th%d' % th)[0], E('L2_r2.5_th%d' % th)[0])
    assert not np.array_equal(E('L2_r4.0_th1')[0], E('L2_r4.0_th3')[0])
    # L3b: both ceil outcomes around every k (8 levels show them up to k = 6, 10 levels for k = 7, 8)
    for ks, nl in ((range(0, 7), 8), ((7, 8), 10)):
        lv = sweep(lambda cc: run_oracle(oracle, cc), ks, nl)
        for j, k in enumerate(ks): assert set(lv[13 * j:13 * j + 13]) == {k, k + 1}, (k, lv[13 * j:13 * j + 13])
    # L5
    c = CASE['L5_4096']; m, n, v = E('L5_4096'); g = _frustum_first_fail(c['cur'], c['lm'])
    assert len(c['lm']['xw']) == 4096 and len(c['cur']['keys']) == 1280 and n >= 300 and (m >= 1024).sum() >= 50
    for i, name in enumerate(L5_GATES): assert (g == i).sum() >= 20 and (v[g == i] == 0).mean() > 0.9, (name, (g == i).sum())
    assert 0.6 < (c['lm']['obs'] > 0).mean() < 0.8 and len(CASE['L5_1025']['lm']['xw']) == 1025 and E('L5_1')[1] == 1
