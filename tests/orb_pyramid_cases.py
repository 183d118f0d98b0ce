"""Shared case of the ORB pyramid tests (tests/test_orb_pyramid_emu.py, tests/test_orb_pyramid_gpu.py): the fused k_pyramid (one launch, tiles chained through LDS, the x
coefficients of a dword group held in registers) against the library's per-level k_resize launches and against the oracle's cv::resize chain, byte for byte.  The tile and
group tables are built per geometry, so the product geometry runs with batch 2 and two small geometries have level widths that are no multiples of 4: 322 x 242, and
298 x 226, about the smallest eight-level geometry sgx_orb_create accepts (203 x 151 is refused: its coarsest level has no room for a FAST cell grid)."""
import numpy as np
from sg_slam_amd.orb import ORBextractor

GEOMETRIES = [(640, 480, 2), (322, 242, 1), (298, 226, 1)]      # width, height, batch


def check_pyramid(lib, orc, to_dev, w, h, batch, nl=8, sf=1.2):
    sizes = orc.level_sizes(w, h, sf, nl)
    if (w, h) != (640, 480):
        assert any(lw % 4 for lw, _ in sizes[1:]), sizes
    rng = np.random.RandomState(w * 7 + h)
    pitch = (w + 3) & ~3
    rows = rng.randint(0, 256, (batch, h, pitch)).astype(np.uint8)      # the row pitch is a multiple of 4; the bytes past the width are random too
    imgs = rows[:, :, :w]
    e = ORBextractor(lib=lib, width=w, height=h, nlevels=nl, scaleFactor=sf, max_batch=batch)
    cap = e.capacity
    kps = to_dev(np.zeros((batch, cap * 28), np.uint8)); desc = to_dev(np.zeros((batch, cap, 32), np.uint8)); cnt = to_dev(np.zeros(batch, 'i4')); dimg = to_dev(rows)
    got = []
    try:
        for unfused in (1, 0):
            lib.tap('sgx_orb_debug_set_unfused_pyramid')(unfused)
            e.extract_batch_dev(dimg, pitch, batch, kps, desc, cnt)
            e.last_status()
            got.append([[e.debug_level(f, l) for l in range(1, nl)] for f in range(batch)])
    finally:
        lib.tap('sgx_orb_debug_set_unfused_pyramid')(0)
        e.close()
    for f in range(batch):
        ref = imgs[f]
        for l in range(1, nl):
            ref = orc.resize_linear(ref, *sizes[l])
            per_level, fused = got[0][f][l - 1], got[1][f][l - 1]
            assert fused.shape == ref.shape == per_level.shape, (w, h, l)
            assert (per_level == ref).all(), f'{w}x{h} frame {f} level {l}: k_resize differs from the oracle'
            bad = np.argwhere(fused != ref)
            assert len(bad) == 0, f'{w}x{h} frame {f} level {l}: k_pyramid differs from the oracle in {len(bad)} bytes, first at (y, x) = {tuple(bad[0])}'
