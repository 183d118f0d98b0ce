"""Frame::ComputeStereoMatches on the MI355X: the product library against the numpy restatement (tests/stereo_ref.py) bit for bit on every case of
tests/stereo_cases.py, the taps through the tap build, the batch against single pairs, two runs of one batch, a 640 x 480 batch of 8 on a side stream against the
emulator, and StereoFrame -> frame.unproject on the two-layer scene."""
import numpy as np
import pytest
import stereo_cases as sc
import stereo_ref as ref

pytestmark = pytest.mark.gpu
F = np.float32
SMALL = [n for n in sc.NAMES if not n.startswith('wide')]
WIDE = [n for n in sc.NAMES if n.startswith('wide')]


def _dev():
    import torch
    return dict(to_dev=lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda(), to_host=lambda t: t.cpu().numpy(), sync=torch.cuda.synchronize)


@pytest.fixture(scope='module')
def cases(emu):
    return sc.build(emu)


def _all(lib, cases):
    out = {}
    for names in (SMALL, WIDE):
        for n, r in zip(names, sc.run(lib, [cases[n] for n in names], **_dev())): out[n] = r
    return out


@pytest.fixture(scope='module')
def batches(gpulib, cases):
    return _all(gpulib, cases)


@pytest.mark.parametrize('name', sc.NAMES)
def test_device_equals_restatement(cases, batches, name):
    assert 'code' not in batches[name]                      # the product library has no taps
    sc.assert_equal(batches[name], cases[name])


def test_device_taps_equal_restatement(gpulib_taps, cases):
    got = _all(gpulib_taps, cases)
    for n in sc.NAMES:
        assert 'sads' in got[n]
        sc.assert_equal(got[n], cases[n])


def test_batch_equals_singles_and_repeats(gpulib, cases, batches):
    for n in ('small_slant', 'hand_rows', 'hand_empty_right', 'wide_const'):
        sc.assert_same(sc.run(gpulib, [cases[n]], **_dev())[0], batches[n], n)
    again = _all(gpulib, cases)
    for n in sc.NAMES: sc.assert_same(again[n], batches[n], n)


def test_vga_batch_on_a_side_stream_equals_emulator(gpulib, emu):
    import torch
    pairs = sc.vga_batch(8)
    want = sc.run(emu, pairs)
    s = torch.cuda.Stream()
    with torch.cuda.stream(s):
        got = sc.run(gpulib, pairs, stream=s.cuda_stream, **_dev())
    assert sum(w['nmatched'] for w in want) >= 8 * 100
    for w, g_ in zip(want, got):
        for k in ('uright', 'depth', 'n', 'nmatched'): assert np.asarray(w[k]).tobytes() == np.asarray(g_[k]).tobytes(), k


def test_stereo_frame_unprojects_onto_the_two_layers(gpulib, cases):
    """StereoFrame (conversion to gray, one extraction of both images, UndistortKeyPoints, the match) -> frame.unproject with the identity pose: the z of every
    matched octave-0 keypoint lies on one of the scene's two depths bf / d within dz <= z^2 * 0.5 / bf, what a disparity error of 0.5 px implies to first order (the
    layers are whole-pixel shifts, so the SAD is 0 at the true offset and the parabola moves the match by at most 0.5 px at scale 1)"""
    import torch
    from sg_slam_amd import frame
    from sg_slam_amd.stereo import StereoFrame
    c = cases['small_layers']; g = sc.GEOM['small']; bf = g['bf']
    cam = dict(fx=g['fx'], fy=g['fx'], cx=g['width'] / 2, cy=g['height'] / 2, bf=bf)
    sf = StereoFrame(g['width'], g['height'], cam, nfeatures=g['nfeatures'], scaleFactor=g['scaleFactor'], nlevels=g['nlevels'], lib=gpulib)
    bgr = [torch.from_numpy(np.repeat(im[:, :, None], 3, 2).copy()).cuda() for im in (c['left'], c['right'])]      # equal channels: the gray value is the channel value
    r = sf(bgr[0], bgr[1])
    cap = sf.cap
    Tcw = torch.eye(4, dtype=torch.float32, device='cuda').reshape(1, 16).contiguous()
    xw = torch.zeros((1, cap, 3), dtype=torch.float32, device='cuda'); has = torch.zeros((1, cap), dtype=torch.uint8, device='cuda')
    frame.unproject_batch(gpulib, 1, cap, r['keys_un'], r['n'], r['depth'], Tcw, cam, xw, has, stream=torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    n = int(r['n'][0]); e = sc.expected(c)
    keys = r['keys'][0].cpu().numpy().view(np.uint8).reshape(cap, 28)[:n].copy().view(sc.KP_DTYPE).reshape(n)
    assert n == len(c['keys_left']) and (keys == c['keys_left']).all() and (r['keys_un'][0].cpu().numpy().tobytes() == r['keys'][0].cpu().numpy().tobytes())
    assert (r['uright'][0, :n].cpu().numpy().view(np.uint32) == e['uright'].view(np.uint32)).all() and int(r['nmatched'][0]) == (e['uright'] != -1).sum()
    sel = (e['uright'] != -1) & (keys['octave'] == 0)
    assert sel.sum() >= 50 and (has[0, :n].cpu().numpy().astype(bool) == (e['depth'] > 0)).all()
    z = xw[0, :n, 2].cpu().numpy().astype('f8')[sel]
    layers = np.array([bf / sc.LAYERS['d_back'], bf / sc.LAYERS['d_front']])
    dz = np.abs(z[:, None] - layers[None, :]); j = dz.argmin(1)
    assert (dz.min(1) <= layers[j] ** 2 * 0.5 / bf).all() and (j == 0).any() and (j == 1).any()
    sf.close()
