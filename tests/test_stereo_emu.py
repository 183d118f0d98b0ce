"""Frame::ComputeStereoMatches on the kernel-logic emulator (CPU): the numpy restatement (tests/stereo_ref.py) against statements that do not go through the code
under test, then the emulator against the restatement bit for bit on every case of tests/stereo_cases.py (the uright and depth float bits, and through the taps
bestIdxR, the Hamming distance, the exit code, bestincR and the 11 SADs), the batch against single pairs, one extractor handle with 2B frames against two handles,
the host entry, and the argument errors."""
import ctypes as C
import numpy as np
import pytest
import stereo_cases as sc
import stereo_ref as ref
from sg_slam_amd.capi import KP_DTYPE, _vp
from sg_slam_amd.stereo import StereoMatcher

F = np.float32
SMALL = [n for n in sc.NAMES if not n.startswith('wide')]
WIDE = [n for n in sc.NAMES if n.startswith('wide')]


@pytest.fixture(scope='module')
def cases(emu):
    return sc.build(emu)


@pytest.fixture(scope='module')
def batches(emu, cases):
    """every case once, as two batches (one per geometry) through one extractor handle"""
    out = {}
    for names in (SMALL, WIDE):
        for n, r in zip(names, sc.run(emu, [cases[n] for n in names])): out[n] = r
    return out


def test_cases_contain_what_they_are_for(cases):
    sc.check_case_contents(cases)


@pytest.mark.parametrize('name', ['small_const', 'hand_rows', 'wide_slant'])
def test_restatement_row_table_against_the_interval_predicate(cases, name):
    """the candidate list of every row equals { iR : floor(y - r) <= yi <= ceil(y + r) } evaluated row by row (the hand-made rows case has keys off the image, a
    NaN, infinities and octaves that are no level)"""
    c = cases[name]; g = sc.GEOM[c['geom']]; k = c['keys_right']; H = g['height']
    table = ref.row_table(k, g['scale'], H)
    y = k['y'].astype(F); ok = (k['octave'] >= 0) & (k['octave'] < g['nlevels']) & np.isfinite(y)
    r = F(2) * g['scale'][np.clip(k['octave'], 0, g['nlevels'] - 1)]
    with np.errstate(all='ignore'):
        lo = np.floor((y - r).astype(F)); hi = np.ceil((y + r).astype(F))
    for yi in range(H):
        assert table[yi] == list(np.nonzero(ok & (lo <= yi) & (yi <= hi))[0]), yi
    assert any(table)


@pytest.mark.parametrize('name', sc.SYNTH + ('hand_sadtie',))
def test_restatement_median_cut_against_sort(cases, name):
    """the cut is SAD >= 1.5f * 1.4f * sorted[n // 2] over the accepted matches, whatever order they are visited in"""
    e = sc.expected(cases[name])
    acc = e['code'] >= ref.ACCEPTED
    sad = e['sads'][np.arange(len(acc)), 5 + e['best_inc']][acc]
    th = F(1.5) * F(1.4) * F(np.sort(sad)[len(sad) // 2])
    assert ((e['code'][acc] == ref.CUT) == (sad.astype(F) >= th)).all() and (e['code'][acc] == ref.CUT).any()
    assert ((e['uright'] == -1) == ~np.isin(e['code'], (ref.ACCEPTED, ref.ACCEPTED_CLAMPED))).all() and ((e['depth'] == -1) == (e['uright'] == -1)).all()


@pytest.mark.parametrize('name', ['small_const'])          # the exact shift; wide_const carries +-1 of noise (stereo_cases.images)
def test_restatement_constant_disparity_within_half_a_pixel(cases, name):
    """derived, not measured: the right image is the left one shifted by d whole pixels, so at level 0 the SAD is 0 at the true offset; with dist2 = 0 the parabola
    gives |deltaR| = |d1 - d3| / (2 (d1 + d3)) <= 0.5, and the scale of octave 0 is 1"""
    c = cases[name]; e = sc.expected(c); d = sc.CONST_D[name]
    sel = np.isin(e['code'], (ref.ACCEPTED, ref.ACCEPTED_CLAMPED)) & (c['keys_left']['octave'] == 0)
    assert sel.sum() >= 10
    assert (np.abs(c['keys_left']['x'][sel].astype('f8') - e['uright'][sel].astype('f8') - d) < 0.5).all()
    assert (np.abs(e['depth'][sel].astype('f8') - c['bf'] / (c['keys_left']['x'][sel].astype('f8') - e['uright'][sel].astype('f8'))) < 1e-4 * e['depth'][sel]).all()


@pytest.mark.parametrize('name', sc.NAMES)
def test_emulator_equals_restatement(cases, batches, name):
    sc.assert_equal(batches[name], cases[name])


def test_batch_equals_singles(emu, cases, batches):
    for n in ('small_slant', 'hand_rows', 'hand_empty_right', 'wide_const'):
        one = sc.run(emu, [cases[n]])[0]
        sc.assert_same(one, batches[n], n)


def test_two_handles_equal_one_handle(emu, cases, batches):
    names = ['small_layers', 'small_zero', 'hand_ties']
    for n, r in zip(names, sc.run(emu, [cases[n] for n in names], two_handles=True)):
        sc.assert_same(r, batches[n], n)


def test_host_entry(emu, cases):
    """sgx_stereo_match after two sgx_orb_extract calls == the restatement; and it refuses one handle for both sides or a handle whose last call was a batch"""
    c = cases['small_slant']; g = sc.GEOM['small']
    exl, exr = sc.extractor(emu, 'small', 1), sc.extractor(emu, 'small', 1)
    kl, dl = exl(c['left']); kr, dr = exr(c['right'])
    assert np.array_equal(kl, c['keys_left']) and np.array_equal(dr, c['desc_right'])
    sm = StereoMatcher(exl, lib=emu)
    ur, z, nm = sm.match(exl, exr, kl, dl, kr, dr, g['fx'], g['bf'])
    e = sc.expected(c)
    assert (ur.view(np.uint32) == e['uright'].view(np.uint32)).all() and (z.view(np.uint32) == e['depth'].view(np.uint32)).all() and nm == (e['uright'] != -1).sum()
    with pytest.raises(Exception, match='invalid'): sm.match(exl, exl, kl, dl, kr, dr, g['fx'], g['bf'])
    P = 320; gray = np.zeros((1, 240, P), np.uint8); gray[0] = c['right']
    keys = np.zeros((1, exr.capacity), KP_DTYPE); desc = np.zeros((1, exr.capacity, 32), np.uint8); n = np.zeros(1, np.int32)
    exr.extract_batch_dev(gray, P, 1, keys, desc, n)
    with pytest.raises(Exception, match='invalid'): sm.match(exl, exr, kl, dl, kr, dr, g['fx'], g['bf'])
    sm.close(); exl.close(); exr.close()


def test_argument_errors(emu, cases):
    g = sc.GEOM['small']; W, H = g['width'], g['height']; B = 2; P = W
    ex = sc.extractor(emu, 'small', 2 * B); other = sc.extractor(emu, 'wide', 2); more = sc.ORBextractor(g['nfeatures'] + 300, g['scaleFactor'], g['nlevels'], 20, 7, W, H, max_batch=2, lib=emu)
    cap = ex.capacity
    h = C.c_void_p(1)
    assert emu.dll.sgx_stereo_create(None, 1, C.byref(h)) != 0 and not h.value
    assert emu.dll.sgx_stereo_create(ex.h, 0, C.byref(h)) != 0 and emu.dll.sgx_stereo_create(ex.h, 1, None) != 0
    sm = StereoMatcher(ex, max_batch=B, lib=emu)
    gray = np.zeros((2 * B, H, P), np.uint8); gray[:] = cases['small_const']['left']
    keys = np.zeros((2 * B, cap), KP_DTYPE); desc = np.zeros((2 * B, cap, 32), np.uint8); n = np.zeros(2 * B, np.int32)
    ur = np.zeros((B, cap), F); z = np.zeros((B, cap), F)

    def call(batch=B, ol=ex, lf=0, gl=gray, pl=P, orr=ex, rf=B, gr=gray, pr=P, cap_=cap, kl=keys, ur_=ur):
        return emu.dll.sgx_stereo_match_batch_dev(sm.h, batch, ol.h, lf, _vp(gl), pl, orr.h, rf, _vp(gr), pr, cap_, _vp(kl), _vp(desc), _vp(n), _vp(keys[B:]), _vp(desc[B:]), _vp(n[B:]),
                                                  g['fx'], g['bf'], _vp(ur_), _vp(z), None, None)
    INVALID = -1
    assert emu.dll.sgx_status_string(INVALID) == b'invalid argument'
    assert call() == INVALID                                              # no pyramid yet
    ex.extract_batch_dev(gray, P, B, keys, desc, n)
    assert call() == INVALID                                              # a pyramid for B frames, the right ones start at B
    ex.extract_batch_dev(gray, P, 2 * B, keys, desc, n)
    assert call() == 0
    assert call(batch=B + 1) == INVALID and call(batch=0) == INVALID      # batch > max_batch
    assert call(cap_=cap - 1) == INVALID and call(cap_=cap + 1) == INVALID
    assert call(kl=None) == INVALID and call(ur_=None) == INVALID and call(gl=None) == INVALID
    assert call(lf=-1) == INVALID and call(rf=B + 1) == INVALID
    assert call(gl=gray[1:]) == INVALID and call(pr=P + 4) == INVALID     # not the image the pyramid was built from
    g2 = np.zeros((2, 484, 644), np.uint8); k2 = np.zeros((2, other.capacity), KP_DTYPE); d2 = np.zeros((2, other.capacity, 32), np.uint8); n2 = np.zeros(2, np.int32)
    other.extract_batch_dev(g2, 644, 2, k2, d2, n2)
    assert call(orr=other, rf=0, gr=g2, pr=644) == INVALID                # another geometry
    g3 = np.zeros((2, H, P), np.uint8); k3 = np.zeros((2, more.capacity), KP_DTYPE); d3 = np.zeros((2, more.capacity, 32), np.uint8)
    more.extract_batch_dev(g3, P, 2, k3, d3, n2)
    assert call(orr=more, rf=0, gr=g3) == INVALID                         # the same image size with another capacity
    ex.detect_batch_dev(gray, P, 2 * B, keys, n)
    assert call() == 0                                                    # a detection leaves a pyramid as well
    assert emu.tap('sgx_stereo_debug_read')(sm.h, B, None, None, None, None, None) == INVALID
    sm.close(); ex.close(); other.close(); more.close()
