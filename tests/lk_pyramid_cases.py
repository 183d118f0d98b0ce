"""Shared case of the LK pyramid tests (tests/test_lk_pyramid_emu.py, tests/test_lk_pyramid_gpu.py): every byte of every level slot, padding columns included.

What a slot holds (sgx_flow.cpp: sgx_flow_create / build_pyramid):
  * level l is stored with a row pitch of (w_l + 3) & ~3 bytes; levels are halved ((n + 1) / 2) while both sides stay above the 21-pixel window, at most max_level times
  * level 0 is the frame; the padding columns of its last dword group are 0
  * level l >= 1 is cv::pyrDown of the VALID part of level l-1: dst(x, y) = (sum_ij k_i k_j src(R(2x-2+i, w), R(2y-2+j, h)) + 128) >> 8, k = [1 4 6 4 1], R = BORDER_REFLECT_101,
    and its padding columns x = w_l .. pitch_l-1 are the SAME formula evaluated at those x (a reflected index never leaves the valid source columns)
The valid part is checked against the oracle's pyrDown (oracle/flow_oracle.c) as well.
"""
import numpy as np
from sg_slam_amd.flow import OpticalFlowLK

WIN, MAX_LEVEL = 21, 3

# (width, height).  Level-1 widths 24, 25, 26, 27 (= 0, 1, 2, 3 mod 4) with odd and even heights: the smallest sizes that still have a level 1 (a side of 42 or less is
# never halved: 21 is not above the window).  42 x 19 therefore is a one-level pyramid (the copy alone), and a level 3 cannot be 3 pixels high: 173 x 170 is the
# smallest geometry with four levels (level 3 = 22 x 22, the minimum the library builds).  640 x 480 is the product geometry.
SIZES = [(48, 47), (49, 44), (51, 45), (53, 50), (42, 19), (173, 170), (640, 480)]


def _reflect101(p, n):
    if n == 1:
        return 0
    while p < 0 or p >= n:
        p = -p if p < 0 else 2 * n - 2 - p
    return p


def _pyr_down_slot(src):
    """the stored rows of the next level (pitch columns) from the valid pixels of this one"""
    sh, sw = src.shape
    dw, dh = (sw + 1) // 2, (sh + 1) // 2
    pitch = (dw + 3) & ~3
    k = np.array([1, 4, 6, 4, 1], np.int64)
    cols = np.array([[_reflect101(2 * x - 2 + i, sw) for i in range(5)] for x in range(pitch)])
    rows = np.array([[_reflect101(2 * y - 2 + j, sh) for j in range(5)] for y in range(dh)])
    s = src.astype(np.int64)
    hor = (s[:, cols] * k).sum(2)                                # (sh, pitch)
    out = (hor[rows, :] * k[None, :, None]).sum(1)               # (dh, pitch)
    return ((out + 128) >> 8).astype(np.uint8), dw


def reference_slots(img):
    """[(slot bytes (h, pitch), valid width)] per level"""
    h, w = img.shape
    lvl0 = np.zeros((h, (w + 3) & ~3), np.uint8); lvl0[:, :w] = img
    out = [(lvl0, w)]
    for _ in range(MAX_LEVEL):
        if (w + 1) // 2 <= WIN or (h + 1) // 2 <= WIN:
            break
        slot, w = _pyr_down_slot(out[-1][0][:, :out[-1][1]])
        h = slot.shape[0]
        out.append((slot, w))
    return out


def check_slots(lib, orc, xp, w, h, batch=3):
    rng = np.random.RandomState(1000 * w + h)
    pitch = ((w + 3) & ~3) + 8                                   # source rows are longer than the image
    fl = OpticalFlowLK(width=w, height=h, max_batch=batch, lib=lib)
    for slot in (0, 1):                                          # two calls: the second one fills the other slot
        frames = rng.randint(0, 256, (batch, h, pitch)).astype(np.uint8)      # the bytes past the width are random too: nothing may read them
        keep = xp(frames)
        fl.reset()
        assert fl.lk_batch_dev(keep, pitch, batch, None, None, 0, None) is False
        for f in range(batch):
            ref = reference_slots(frames[f, :, :w])
            assert fl.levels == len(ref), (w, h, fl.levels, len(ref))
            valid = frames[f, :, :w]
            for l, (exp, vw) in enumerate(ref):
                got = fl.debug_slot(slot, f, l)
                assert got.shape == exp.shape, (w, h, l, got.shape, exp.shape)
                bad = np.argwhere(got != exp)
                assert len(bad) == 0, f'{w}x{h} slot {slot} frame {f} level {l}: {len(bad)} bytes differ, first at (y, x) = {tuple(bad[0])} (valid width {vw}, pitch {exp.shape[1]})'
                assert (got[:, :vw] == valid).all(), f'{w}x{h} level {l} differs from the oracle pyrDown'
                valid = orc.pyr_down(valid)
    fl.close()
