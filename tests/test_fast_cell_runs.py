"""k_fast_cells at the places where sharing a tile between neighbouring cells can change results (ORBextractor.cc:790-830): a corner beside a stronger one across a
cell edge, the per-cell 20 -> 7 fallback beside cells that stay at 20, runs shorter than the rest, narrow last cells, list capacities on pure noise, several frames per
launch.  Every case compares ORBextractor.debug_candidates(frame, level) with oracle.level_candidates(level image) as sorted (x, y, score) lists, exactly.
The emulator cases run in the CPU tier; the same functions run on the device with the tap library."""
import numpy as np
import pytest
from sg_slam_amd.orb import ORBextractor

W0, H0 = 200, 136           # level 0: 5 x 3 cells of 34 x 35; interiors start at 19 + j * 34, 19 + i * 35


def boundary_dots():
    img = np.full((H0, W0), 128, np.uint8)
    for (x, y, v) in ((52, 40, 118), (53, 40, 28), (63, 45, 118), (60, 53, 118), (61, 54, 28), (30, 62, 120), (30, 74, 122)):
        img[y, x] = v
    return img


def noise(seed, w=W0, h=H0):
    return np.random.RandomState(1000 + seed).randint(0, 256, (h, w)).astype(np.uint8)


def checkerboard(seed):
    """noise everywhere; the interior of every level-0 cell with (i + j) odd is 128 +- 9 noise: no corner at 20 there, some at 7"""
    rng = np.random.RandomState(2000 + seed)
    img = noise(seed)
    for i in range(3):
        for j in range(5):
            if (i + j) & 1:
                y0, x0 = 19 + i * 35, 19 + j * 34
                sub = img[y0:y0 + 35, x0:x0 + 34]
                sub[...] = rng.randint(119, 138, sub.shape)
    return img


def _triples(x, y, s):
    return sorted(zip((int(v) for v in x), (int(v) for v in y), (int(v) for v in s)))


def _levels_match(ex, oracle, frame, img):
    """every level of one frame of the last call on `ex`; returns the level-0 list in image coordinates (candidates are relative to the (16, 16) border origin)"""
    first = None
    for l in range(ex.nlevels):
        lvl = img if l == 0 else ex.debug_level(frame, l)
        got = _triples(*ex.debug_candidates(frame, l))
        want = _triples(*oracle.level_candidates(lvl))
        assert got == want, (frame, l, len(got), len(want))
        if l == 0: first = [(x + 16, y + 16, v) for (x, y, v) in got]
    return first


def _single(lib, oracle, img, nlevels):
    h, w = img.shape
    ex = ORBextractor(lib=lib, width=w, height=h, nlevels=nlevels)
    try:
        ex(img)
        return _levels_match(ex, oracle, 0, img)
    finally:
        ex.close()


def _cell_of(x, y, wcell=34, hcell=35):
    return (y - 19) // hcell, (x - 19) // wcell


def _cross_cell_adjacent_pairs(c):
    n = 0
    for a in range(len(c)):
        for b in range(a + 1, len(c)):
            if abs(c[a][0] - c[b][0]) <= 1 and abs(c[a][1] - c[b][1]) <= 1 and _cell_of(*c[a][:2]) != _cell_of(*c[b][:2]): n += 1
    return n


def run_boundary_dots(lib, oracle):
    got = _single(lib, oracle, boundary_dots(), 1)
    # (52, 40) is the last interior column of cell (0, 0) and scores 9 beside the 99 of (53, 40) in cell (0, 1); cell (1, 1) has the corner (61, 54) at 20, so its weak dots
    # (63, 45) and (60, 53) are not reported; (30, 62) scores 7 and is the only corner of cell (1, 0); (30, 74) scores 5
    assert got == [(30, 62, 7), (52, 40, 9), (53, 40, 99), (61, 54, 99)]


def run_checkerboard(lib, oracle, seed):
    got = _single(lib, oracle, checkerboard(seed), 3)
    low = set(_cell_of(x, y) for (x, y, s) in got if s < 20)
    # the low threshold was used in all 7 flattened cells and in no other; 946-976 candidates is what the oracle finds on these seeded images
    assert low == set((i, j) for i in range(3) for j in range(5) if (i + j) & 1) and 940 <= len(got) <= 980


def run_noise(lib, oracle, seed):
    got = _single(lib, oracle, noise(seed), 3)
    # the oracle finds 1615-1652 candidates on these seeded images, 34-53 pairs of them 8-adjacent across a cell edge
    assert 1600 <= len(got) <= 1660 and 34 <= _cross_cell_adjacent_pairs(got) <= 53
    _single(lib, oracle, noise(seed, 131, 101), 2)                            # level 1 is 2 x 1 cells: one short run


def run_batch(lib, oracle, to_dev=lambda a: a):
    imgs = np.stack([boundary_dots(), checkerboard(1), noise(2)])
    ex = ORBextractor(lib=lib, width=W0, height=H0, nlevels=3, max_batch=3)
    try:
        cap = ex.capacity
        kps, desc, cnt = to_dev(np.zeros((3, cap * 28), np.uint8)), to_dev(np.zeros((3, cap, 32), np.uint8)), to_dev(np.zeros(3, 'i4'))
        ex.extract_batch_dev(to_dev(imgs), W0, 3, kps, desc, cnt)
        ex.last_status()
        firsts = [_levels_match(ex, oracle, f, imgs[f]) for f in range(3)]
        assert len(firsts[0]) == 4 and len(firsts[1]) == 946 and len(firsts[2]) == 1615
    finally:
        ex.close()


# (260, 150): 7 cells of 33 per row over 228 px, the last one 30 wide; (333, 140): 10 cells of 31 over 301 px, the last one 22 wide; (236, 120): 6 cells of 34, one cell row
GEOMETRIES = ((260, 150), (333, 140), (236, 120))


def run_geometry(lib, oracle, w, h):
    got = _single(lib, oracle, noise(w, w, h), 2)
    assert len(got) > 500


def test_boundary_dots_emu(emu, oracle):
    run_boundary_dots(emu, oracle)


@pytest.mark.parametrize('seed', range(3))
def test_checkerboard_emu(emu, oracle, seed):
    run_checkerboard(emu, oracle, seed)


@pytest.mark.parametrize('seed', range(3))
def test_noise_emu(emu, oracle, seed):
    run_noise(emu, oracle, seed)


def test_batch_emu(emu, oracle):
    run_batch(emu, oracle)


@pytest.mark.parametrize('w,h', GEOMETRIES)
def test_geometry_emu(emu, oracle, w, h):
    run_geometry(emu, oracle, w, h)


@pytest.mark.gpu
def test_boundary_dots_gpu(gpulib_taps, oracle):
    run_boundary_dots(gpulib_taps, oracle)


@pytest.mark.gpu
@pytest.mark.parametrize('seed', range(3))
def test_checkerboard_gpu(gpulib_taps, oracle, seed):
    run_checkerboard(gpulib_taps, oracle, seed)


@pytest.mark.gpu
@pytest.mark.parametrize('seed', range(3))
def test_noise_gpu(gpulib_taps, oracle, seed):
    run_noise(gpulib_taps, oracle, seed)


@pytest.mark.gpu
def test_batch_gpu(gpulib_taps, oracle):
    import torch
    run_batch(gpulib_taps, oracle, to_dev=lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda())


@pytest.mark.gpu
@pytest.mark.parametrize('w,h', GEOMETRIES)
def test_geometry_gpu(gpulib_taps, oracle, w, h):
    run_geometry(gpulib_taps, oracle, w, h)
