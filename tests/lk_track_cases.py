"""Shared cases of the LK tracker tests (tests/test_lk_track_emu.py, tests/test_lk_track_gpu.py): the tracker against the oracle away from the 640 x 480 defaults.

The device body of k_lk_trackN<2> (two keypoints per wave, DPP group sums, sgx_lk_stage_row, the `direct` / `whole` border paths, the tile re-staging rule) is not compiled into
the kernel-logic emulator, which runs the scalar twin sgx_lk_track_point; so the GPU tier is what covers it, and these cases take it through the geometries, criteria and batch
layouts that sgx_flow_create accepts.  Every comparison is exact: status equal and positions equal as uint32 bit patterns against oracle.lk_pyr(..., acc_mode=1) called with the
same max_level, max_count and epsilon.  No tolerance anywhere.

Inputs (one recipe for all cases)
  texture   RandomState(seed).randint(0, 256) on an (h + 40, w + 40) float plane, `passes` rounds of the separable [1 4 6 4 1] / 16 filter with wrap-around, rescaled to 0..255;
            I = crop at (20, 20), J = crop at (20 + dy, 20 + dx), both cast to uint8
  points    64 per image, uniform(-25, w + 25) x uniform(-25, h + 25), float32, from the same RandomState after the texture: about a third start outside the image
  order     even slots hold points at least 25 px inside the image as far as there are any, odd slots the rest: with two keypoints per wave an interior window (the `direct`
            path) shares its wave with a border, outside or skipped one

Every case asserts GUARDS on the oracle's output (how many points are tracked, how many iterations run, how far the windows move) before it compares, so that a change of
the recipe cannot leave a case comparing nothing.  The figures beside the guards are what the oracle gives with the seeds below.

Not covered: the double-precision convergence band of k_lk_trackN (`fabsf(f2 - e2f) <= 1e-5f * e2f`) is reached only by chance; no input here is built to reach it.
"""
import ctypes as C
import numpy as np
from sg_slam_amd.flow import OpticalFlowLK
from sg_slam_amd.capi import KP_DTYPE, _vp

NPTS = 64
K5 = np.array([1, 4, 6, 4, 1], np.float64) / 16


def texture(rs, w, h, passes):
    t = rs.randint(0, 256, (h + 40, w + 40)).astype(np.float64)
    for _ in range(passes):
        for ax in (0, 1):
            t = sum(K5[i] * np.roll(t, i - 2, ax) for i in range(5))
    t -= t.min()
    return t * (255.0 / t.max())


def crop(t, w, h, dy=0, dx=0):
    return np.ascontiguousarray(t[20 + dy:20 + dy + h, 20 + dx:20 + dx + w].astype(np.uint8))


def points(rs, w, h, n=NPTS):
    p = np.c_[rs.uniform(-25, w + 25, n), rs.uniform(-25, h + 25, n)].astype('f4')
    inner = (p[:, 0] >= 25) & (p[:, 0] <= w - 25) & (p[:, 1] >= 25) & (p[:, 1] <= h - 25)
    a, b = list(p[inner]), list(p[~inner])
    out = []
    for i in range(n):                                          # even slot: an interior point while there is one (and once the others are used up)
        out.append(a.pop(0) if a and (i % 2 == 0 or not b) else b.pop(0))
    return np.array(out, 'f4')


def pair(seed, w, h, passes=2, shift=(1, -2)):
    """(I, J, pts) of the recipe"""
    rs = np.random.RandomState(seed)
    t = texture(rs, w, h, passes)
    return crop(t, w, h), crop(t, w, h, *shift), points(rs, w, h)


def outside(pts, w, h):
    return (pts[:, 0] < 0) | (pts[:, 0] > w - 1) | (pts[:, 1] < 0) | (pts[:, 1] > h - 1)


def same(got, st, ref, rst, what):
    assert st.dtype == rst.dtype == np.uint8 and got.dtype == ref.dtype == np.float32
    bad = (st != rst) | (got.view(np.uint32) != ref.view(np.uint32)).any(1)
    assert not bad.any(), f'{what}: {int(bad.sum())} of {len(bad)} points differ from the oracle, first {int(np.argmax(bad))}: got {got[bad][0]} status {st[bad][0]}, oracle {ref[bad][0]} status {rst[bad][0]}'


def host_track(lib, I, J, pts, **cfg):
    h, w = I.shape
    fl = OpticalFlowLK(width=w, height=h, lib=lib, **cfg)
    try:
        got, st = fl(I, J, pts)
        return got, st, fl.levels
    finally:
        fl.close()


# ---- 1. geometry: (width, height, levels).  Four, three, two and one levels; a 22 x 22 top level (173 x 170) and a 22 x 22 image, the smallest the library tracks; level-1
#         widths 27, 25, 23 (3 mod 4 and 1 mod 4).  42 x 19, a one-level size the library tracked before it refused sides below 22, is with the refused sizes of case 2
GEOMETRY = [(173, 170, 4), (173, 131, 3), (97, 91, 3), (53, 50, 2), (49, 44, 2), (45, 46, 2), (30, 25, 1), (22, 22, 1)]
GEOMETRY_SEED = 100


def geometry_reference(orc):
    """the oracle's answers for the whole list, with the guards that span the list; computed once per session (the callers cache it)"""
    out = {}
    for i, (w, h, nl) in enumerate(GEOMETRY):
        I, J, pts = pair(GEOMETRY_SEED + i, w, h)
        ref, rst, it = orc.lk_pyr(I, J, pts, acc_mode=1, want_iters=True)
        assert it.shape[1] == nl
        ok = rst > 0
        # tracked points, and tracked points that started outside the image.  The oracle gives 38/6, 45/7, 35/11, 24/13, 26/15, 24/14, 14/8, 13/12 for the sizes in order
        assert ok.sum() >= 8 and (ok & outside(pts, w, h)).sum() >= 3, (w, h, int(ok.sum()), int((ok & outside(pts, w, h)).sum()))
        out[(w, h)] = (I, J, pts, ref, rst, it)
    assert max(v[5].max() for v in out.values()) == 30          # some point runs all 30 iterations at some level (173 x 170 and 53 x 50 have one)
    lvl0 = np.concatenate([v[5][:, 0][v[4] > 0] for v in out.values()])
    assert 0 < lvl0[lvl0 > 0].min() < 10                        # some tracked point stops at level 0 in under 10 iterations (the quickest after 1)
    return out


def check_geometry(lib, refs, w, h, nl):
    I, J, pts, ref, rst, _ = refs[(w, h)]
    got, st, levels = host_track(lib, I, J, pts)
    assert levels == nl
    same(got, st, ref, rst, f'{w}x{h}')


# ---- 2. level-0 sides below 22.  A window reads indices -21 .. len + 20 of a side; one fold of REFLECT_101, which is what the device stages with (sgx_reflect1), covers that only
#         for len >= 22.  Measured on an MI355X before the library refused these sizes (product library, host entry, this recipe and these seeds; points that differ from the
#         oracle, of 64):  21 x 21: 0   20 x 33: 0   12 x 9: 0   5 x 40: 4   2 x 2: 0   42 x 19: 0.  The emulator, which reflects fully, equalled the oracle everywhere.
#         The reference never tracks images this small, so both builds refuse to: SGX_ERR_UNSUPPORTED from sgx_flow_lk and from a sgx_flow_lk_batch_dev call that would
#         track; the pyramid alone is still built at any size (tests/lk_pyramid_cases.py has 42 x 19).
SMALL = [(21, 21), (20, 33), (12, 9), (5, 40), (2, 2), (42, 19)]
SMALL_SEED = {(21, 21): 200, (20, 33): 201, (12, 9): 202, (5, 40): 203, (2, 2): 204, (42, 19): 106}
SGX_ERR_UNSUPPORTED = -2


def check_small(lib, orc, xp, w, h):
    I, J, pts = pair(SMALL_SEED[(w, h)], w, h)
    _, rst = orc.lk_pyr(I, J, pts, acc_mode=1)                   # what is refused is not an empty case: the oracle tracks 14, 14, 14, 8, 0 and 22 points
    if (w, h) == (2, 2): assert (rst == 0).all()                # nothing to track in four pixels
    else: assert (rst > 0).sum() >= 8, (w, h, int((rst > 0).sum()))
    fl = OpticalFlowLK(width=w, height=h, lib=lib)
    assert fl.levels == 1
    out = np.full((NPTS, 2), -777, 'f4'); st = np.full(NPTS, 9, np.uint8)
    rc = lib.dll.sgx_flow_lk(fl.h, _vp(I), _vp(J), w, _vp(pts), NPTS, _vp(out), _vp(st))
    assert rc == SGX_ERR_UNSUPPORTED and (out == -777).all() and (st == 9).all()
    # streaming entry: the first call builds the pyramid as before; the call that would track is refused and leaves the outputs and the handle as they were
    pitch = (w + 3) & ~3
    fr = np.zeros((2, h, pitch), np.uint8); fr[0, :, :w] = J; fr[1, :, :w] = I
    keys = np.zeros(NPTS, KP_DTYPE); keys['x'] = pts[:, 0]; keys['y'] = pts[:, 1]
    d_k, d_n = xp(keys.view(np.uint8).reshape(1, NPTS, 28)), xp(np.array([NPTS], 'i4'))
    d_out, d_st = xp(out.reshape(1, NPTS, 2)), xp(st.reshape(1, NPTS))
    assert fl.lk_batch_dev(xp(fr[0:1]), pitch, 1, d_k, d_n, NPTS, d_out, d_st) is False
    d_fr = xp(fr[1:2])
    for _ in range(2):
        have = C.c_int32(7)
        rc = lib.dll.sgx_flow_lk_batch_dev(fl.h, _vp(d_fr), pitch, 1, _vp(d_k), _vp(d_n), NPTS, _vp(d_out), _vp(d_st), C.byref(have), None)
        assert rc == SGX_ERR_UNSUPPORTED and have.value == 7
    host = lambda a: np.asarray(a.cpu() if hasattr(a, 'cpu') else a)
    assert (host(d_out) == -777).all() and (host(d_st) == 9).all()
    fl.reset()
    assert fl.lk_batch_dev(d_fr, pitch, 1, None, None, 0, None) is False      # pyramid alone: still fine
    fl.close()


# ---- 3. pyramid depth: the first-level initialisation when the top level is level 0, 1 or 2
def check_depth(lib, orc, max_level):
    w, h = 173, 170
    I, J, pts = pair(300, w, h)
    ref, rst = orc.lk_pyr(I, J, pts, max_level=max_level, acc_mode=1)
    assert (rst > 0).sum() >= 8                                 # 42 at each depth
    got, st, levels = host_track(lib, I, J, pts, max_level=max_level)
    assert levels == max_level + 1
    same(got, st, ref, rst, f'max_level {max_level}')


# ---- 4. criteria: (max_count, epsilon, the largest iteration count the oracle reports).  track() clamps to 100 and 10 as OpenCV's wrapper does; the oracle gets the clamped values
CRITERIA = [(0, 0.01, 0), (1, 0.01, 1), (5, 0.01, 5), (30, 0.0, 30), (30, 0.3, 30), (100, 0.001, 100), (200, 20.0, 1)]
CRITERIA_SEED = 405


def check_criteria(lib, orc, max_count, epsilon, most):
    w, h = 97, 91
    I, J, pts = pair(CRITERIA_SEED, w, h)
    ref, rst, it = orc.lk_pyr(I, J, pts, max_count=min(max_count, 100), epsilon=min(epsilon, 10.0), acc_mode=1, want_iters=True)
    assert it.max() == most, (max_count, epsilon, int(it.max()))      # measured with this seed: 0, 1, 5, 30, 30, 100, 1
    got, st, _ = host_track(lib, I, J, pts, max_count=max_count, epsilon=epsilon)
    same(got, st, ref, rst, f'criteria ({max_count}, {epsilon})')


# ---- 5. the window leaves its tile: a staged tile leaves 3 to 6 px of room horizontally and 7 vertically, so a window that ends further away was staged again
def check_restage(lib, orc, max_level):
    w, h = 173, 170
    I, J, pts = pair(500, w, h, passes=20, shift=(8, 9))
    ref, rst = orc.lk_pyr(I, J, pts, max_level=max_level, acc_mode=1)
    far = (rst > 0) & ((np.abs(ref[:, 0] - pts[:, 0]) > 7) | (np.abs(ref[:, 1] - pts[:, 1]) > 8))
    assert far.sum() >= 20, int(far.sum())                      # 42 of 43 tracked points at max_level 0, 42 of 42 at max_level 3
    got, st, _ = host_track(lib, I, J, pts, max_level=max_level)
    same(got, st, ref, rst, f'restage max_level {max_level}')
    return int(far.sum())


def noise_pair():
    w, h = 97, 91
    rs = np.random.RandomState(7)
    a = rs.randint(0, 256, (h, w)).astype(np.uint8)
    return a, np.roll(a, (3, -5), (0, 1)), points(rs, w, h)


def check_noise(lib, orc):
    """pure noise against shifted noise: many iterations, oscillation exits, out-of-image exits (the small version of test_flow_gpu.py::test_lk_noise_gpu)"""
    a, b, pts = noise_pair()
    ref, rst, it = orc.lk_pyr(a, b, pts, acc_mode=1, want_iters=True)
    assert it.max() >= 10 and (rst > 0).sum() >= 8 and (rst == 0).sum() >= 8      # up to 30 iterations; 36 points tracked, 28 lost
    got, st, _ = host_track(lib, a, b, pts)
    same(got, st, ref, rst, 'noise')


# ---- 6. batch layout of the streaming entry: a full group of eight frames plus a remainder (sgx_lk_decode_block), a source pitch above the width, a capacity that is no multiple
#         of 8, keypoint counts of 0, 1, odd, and above the capacity
BATCH_N = [37, 0, 1, 42, 36, 7, 8, 9, 33, 2, 37]
BATCH_CAP = 37
BATCH_SEED = 600


def check_batch(lib, orc, xp):
    w, h, B, cap = 97, 91, len(BATCH_N), BATCH_CAP
    pitch = ((w + 3) & ~3) + 8
    host = lambda a: np.asarray(a.cpu() if hasattr(a, 'cpu') else a)
    rs = np.random.RandomState(BATCH_SEED)
    tex = [texture(np.random.RandomState(BATCH_SEED + 1 + f), w, h, 2) for f in range(B)]
    n = np.array(BATCH_N, 'i4')
    fl = OpticalFlowLK(width=w, height=h, max_batch=B, lib=lib)
    assert fl.levels == 3

    def frames_of(call):                                        # the shift between two calls grows with the call index: (1, -2), then (2, -4)
        s = call * (call + 1) // 2
        fr = rs.randint(0, 256, (B, h, pitch)).astype(np.uint8)      # the bytes past the width are random: nothing may read them
        for f in range(B): fr[f, :, :w] = crop(tex[f], w, h, s, -2 * s)
        return fr

    def keys_of():
        keys = np.zeros((B, cap), KP_DTYPE)
        for f in range(B):
            p = points(rs, w, h)[:cap]
            keys[f]['x'] = p[:, 0]; keys[f]['y'] = p[:, 1]
        return keys

    def run(fr, keys, with_status=True):
        d_fr, d_k, d_n = xp(fr), xp(keys.view(np.uint8).reshape(B, cap, 28)), xp(n)
        d_out = xp(np.full((B, cap, 2), -777, 'f4')); d_st = xp(np.full((B, cap), 9, np.uint8)) if with_status else None
        have = fl.lk_batch_dev(d_fr, pitch, B, d_k, d_n, cap, d_out, d_st)
        return have, host(d_out), (host(d_st) if with_status else None)

    prev = frames_of(0)
    assert run(prev, keys_of())[0] is False                     # the first call only builds the pyramid
    tracked = 0
    for call in (1, 2):                                         # two tracked calls: each slot is the tracked-from one once
        fr, keys = frames_of(call), keys_of()
        have, out, st = run(fr, keys)
        assert have is True
        for f in range(B):
            m = min(n[f], cap)
            pts = np.stack([keys[f, :m]['x'], keys[f, :m]['y']], 1)
            ref, rst = orc.lk_pyr(fr[f, :, :w], prev[f, :, :w], pts, acc_mode=1)
            same(out[f, :m], st[f, :m], ref, rst, f'call {call} frame {f}')
            assert (out[f, m:] == -777).all() and (st[f, m:] == 9).all(), f'call {call} frame {f}: rows from {m} on were written'
            tracked += int((rst > 0).sum())
        last = (prev, fr, keys, out)
        prev = fr
    assert tracked >= 150, tracked                              # the oracle tracks 266 of the 414 compared points
    # the last call once more without a status array: the same positions
    fl.reset()
    assert run(last[0], last[2])[0] is False
    have, out, _ = run(last[1], last[2], with_status=False)
    assert have is True and (out.view(np.uint32) == last[3].view(np.uint32)).all()
    fl.close()
    return tracked
