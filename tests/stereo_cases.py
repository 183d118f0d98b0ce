"""Stereo cases for tests/test_stereo_emu.py and tests/test_stereo_gpu.py: rectified pairs of smoothed random texture at 320 x 240 (8 levels / 1.2) and at 644 x 484
(4 levels / 1.5, so that the +-1 octave filter and the level scaling differ), and hand-made key sets over real pyramids for the exits that extractor keys cannot reach.

A case is dict(name, geom, left, right, keys_left, desc_left, keys_right, desc_right, fx, bf, hand): hand = False means the keys are the extractor's own (the runner
leaves what the extraction wrote), hand = True that the runner overwrites them.  Keys, descriptors and pyramids come from the kernel-logic emulator (a `lib` argument:
the conftest's `emu`), whose extractor the extractor tests hold to the oracle.  expected(case) is the restatement's result (tests/stereo_ref.py), computed once.
check_case_contents() asserts on the restatement alone that every exit of the function occurs somewhere and that every synthetic-image case keeps enough matches."""
import numpy as np
import stereo_ref as ref
from sg_slam_amd.capi import KP_DTYPE
from sg_slam_amd.orb import ORBextractor

F = np.float32
GEOM = {
    'small': dict(width=320, height=240, nlevels=8, scaleFactor=1.2, nfeatures=500, fx=260.0, bf=26.0),
    'wide': dict(width=644, height=484, nlevels=4, scaleFactor=1.5, nfeatures=600, fx=520.0, bf=52.0),
    'vga': dict(width=640, height=480, nlevels=8, scaleFactor=1.2, nfeatures=1000, fx=520.0, bf=40.0),      # vga_batch() only: device against emulator, no restatement
}
SYNTH = ('small_const', 'small_slant', 'small_layers', 'small_zero', 'wide_const', 'wide_slant')      # pairs of one scene: each must keep >= 50 matches
LAYERS = dict(d_back=2, d_front=9)                                                                    # small_layers: disparities of its two depth layers
CONST_D = {'small_const': 3, 'wide_const': 5}
SADTIE = dict(median=10, sads=(2, 4, 6, 8, 10, 10, 20, 21, 21, 22, 30))      # F(1.5) * F(1.4) * F(10) == 21.0 exactly: 20 stays, 21 goes

_cache = {}


def texture(h, w, seed):
    """smoothed random texture, full contrast"""
    rng = np.random.default_rng(seed)
    a = rng.random((h + 4, w + 4))
    for _ in range(2):
        a = (a[:-2] + a[1:-1] + a[2:]) / 3.0
        a = (a[:, :-2] + a[:, 1:-1] + a[:, 2:]) / 3.0
    a = (a - a.min()) / (a.max() - a.min())
    return np.clip(np.rint(20 + 215 * a), 0, 255).astype(np.uint8)


def _sample(T, xs):
    """row-wise linear interpolation of T at the float columns xs (h x w)"""
    x0 = np.floor(xs).astype(np.int64); a = xs - x0
    x0 = np.clip(x0, 0, T.shape[1] - 2)
    rows = np.arange(T.shape[0])[:, None]
    v = (1 - a) * T[rows, x0] + a * T[rows, x0 + 1]
    return np.clip(np.rint(v), 0, 255).astype(np.uint8)


def images(name):
    """(left, right) of a synthetic pair: a scene point at left column x stands at right column x - d"""
    g = GEOM[name.split('_')[0]]; W, H = g['width'], g['height']
    seed = 11 if name.startswith('small') else 23
    T = texture(H, W + 96, seed)
    left = T[:, :W].copy()
    kind = name.split('_')[1]
    if kind == 'const':
        d = CONST_D[name]; right = T[:, d:d + W].copy()
        if name == 'wide_const':                            # with 4 levels most matches are octave-0 ones whose SAD is 0 on an exact shift: the median is 0 and the cut takes
            right = np.clip(right.astype(np.int32) + np.random.default_rng(6).integers(-1, 2, (H, W)), 0, 255).astype(np.uint8)      # every match.  +-1 of noise keeps it above 0
    elif kind == 'slant':                                   # d(xl, y) = 2 + 0.02 xl + 0.01 y: xl = (xr + 2 + 0.01 y) / 0.98
        xr = np.arange(W)[None, :].astype(np.float64); y = np.arange(H)[:, None].astype(np.float64)
        right = _sample(T, (xr + 2.0 + 0.01 * y) / 0.98)
    elif kind == 'layers':                                  # a fronto-parallel rectangle in front of a fronto-parallel background: an occlusion edge on its left side
        db, df = LAYERS['d_back'], LAYERS['d_front']
        x0, x1, y0, y1 = int(W * 0.35), int(W * 0.7), int(H * 0.3), int(H * 0.75)
        right = T[:, db:db + W].copy(); right[y0:y1, x0 - df:x1 - df] = left[y0:y1, x0:x1]
    elif kind == 'noise':
        right = texture(H, W, seed + 100)
    elif kind == 'zero':                                    # the upper third at zero disparity; below it disparity 7 with +-1 of noise, so that the median SAD is > 0.
        rng = np.random.default_rng(5)                      # disparity == 0 exactly needs deltaR == 0, i.e. d1 == d3: the upper third is mirror-symmetric about the
        h0 = int(H * 0.35); xc = W // 2                     # column xc, so that a key ON that column sees mirrored windows at +1 and -1 (hand_clamp)
        left[:h0, xc + 1:] = left[:h0, xc - 1:2 * xc - W:-1]
        right = np.clip(T[:, 7:7 + W].astype(np.int32) + rng.integers(-1, 2, (H, W)), 0, 255).astype(np.uint8)
        right[:h0] = left[:h0]
    elif kind == 'sadtie':                                  # disparity 3; one pixel of each hand-made key's window is off by the SAD that key shall have
        right = T[:, 3:3 + W].copy()
        for (x, y), s in zip(_sadtie_points(), SADTIE['sads']):
            v = int(right[y + 3, x - 3 + 3]); right[y + 3, x - 3 + 3] = v + s if v + s <= 255 else v - s
    else:
        raise KeyError(name)
    return left, right


def vga_batch(B):
    """B pairs at 640 x 480 (slanted planes of different slopes, +-1 of noise), keys left to the extractor: for runs that compare two libraries"""
    g = GEOM['vga']; W, H = g['width'], g['height']; out = []
    for i in range(B):
        T = texture(H, W + 96, 300 + i); rng = np.random.default_rng(400 + i)
        xr = np.arange(W)[None, :].astype(np.float64); y = np.arange(H)[:, None].astype(np.float64)
        right = _sample(T, (xr + 1.0 + i + 0.004 * (i + 1) * y) / (1.0 - 0.005 * (i + 1)))
        right = np.clip(right.astype(np.int32) + rng.integers(-1, 2, (H, W)), 0, 255).astype(np.uint8)
        out.append(dict(name='vga_%d' % i, geom='vga', left=T[:, :W].copy(), right=right, hand=False))
    return out


def _sadtie_points():
    return [(40 + 24 * (i % 10), 40 + 14 * i) for i in range(len(SADTIE['sads']))]      # left positions, rows 14 apart: no window sees another key's pixel


def extractor(lib, geom, max_batch):
    g = GEOM[geom]
    return ORBextractor(g['nfeatures'], g['scaleFactor'], g['nlevels'], 20, 7, g['width'], g['height'], max_batch=max_batch, lib=lib)


def extract(lib, geom, imgs):
    """emulator extraction of a list of images: [(keys, desc, pyramid)]"""
    g = GEOM[geom]; W, H = g['width'], g['height']; n = len(imgs); P = (W + 3) & ~3
    ex = extractor(lib, geom, n); cap = ex.capacity
    gray = np.zeros((n, H, P), np.uint8)
    for i, im in enumerate(imgs): gray[i, :, :W] = im
    keys = np.zeros((n, cap), KP_DTYPE); desc = np.zeros((n, cap, 32), np.uint8); cnt = np.zeros(n, np.int32)
    ex.extract_batch_dev(gray, P, n, keys, desc, cnt)
    out = []
    for i in range(n):
        pyr = [np.ascontiguousarray(imgs[i])] + [ex.debug_level(i, l) for l in range(1, g['nlevels'])]
        out.append((keys[i, :cnt[i]].copy(), desc[i, :cnt[i]].copy(), pyr))
    tables = (ex.mvScaleFactor.copy(), ex.mvInvScaleFactor.copy(), cap)
    ex.close()
    return out, tables


def _key(x, y, octave=0):
    k = np.zeros(1, KP_DTYPE); k['x'] = x; k['y'] = y; k['octave'] = octave; k['size'] = 31; k['angle'] = 0
    return k


def _hand(pairs, rng):
    """[(left (x, y, octave), right (x, y, octave))] -> key sets whose pair i shares one random descriptor"""
    kl = np.concatenate([_key(*a) for a, _ in pairs]); kr = np.concatenate([_key(*b) for _, b in pairs])
    d = rng.integers(0, 256, (len(pairs), 32), dtype=np.uint8)
    return kl, d.copy(), kr, d.copy()


def build(lib):
    """every case, keyed by name (cached per library path)"""
    if lib.path in _cache:
        return _cache[lib.path]
    C = {}
    pyrs = {}
    for geom in GEOM:
        names = [n for n in SYNTH + ('small_noise', 'small_sadtie') if n.startswith(geom)]
        if not names: continue
        imgs = []
        for n in names: imgs += list(images(n))
        ext, tables = extract(lib, geom, imgs)
        GEOM[geom]['scale'], GEOM[geom]['inv_scale'], GEOM[geom]['cap'] = tables
        for i, n in enumerate(names):
            (kl, dl, pl), (kr, dr, pr) = ext[2 * i], ext[2 * i + 1]
            C[n] = dict(name=n, geom=geom, left=imgs[2 * i], right=imgs[2 * i + 1], keys_left=kl, desc_left=dl, keys_right=kr, desc_right=dr, hand=False)
            pyrs[n] = (pl, pr)
    g = GEOM['small']; W, H = g['width'], g['height']
    base = C['small_const']; rng = np.random.default_rng(77)

    def hand(name, kl, dl, kr, dr, of='small_const', swap=False):
        b = C[of]; pl, pr = pyrs[of]
        C[name] = dict(name=name, geom='small', left=b['right'] if swap else b['left'], right=b['left'] if swap else b['right'], keys_left=kl, desc_left=dl,
                       keys_right=kr, desc_right=dr, hand=True)
        pyrs[name] = (pr, pl) if swap else (pl, pr)

    # borders: the reference's test (endu >= cols, iniu < 0) and the windows it does not cover (a right key within 10 px of the border, left windows and rows outside)
    hand('hand_borders', *_hand([((W - 6, 100, 0), (W - 8, 100, 0)), ((60, 120, 0), (7, 120, 0)), ((60, 140, 0), (-3, 140, 0)), ((3, 160, 0), (1, 160, 0)),
                                 ((100, H - 3, 0), (90, H - 3, 0)), ((150, 6, 3), (140, 6, 3)), ((200, 3, 0), (190, 3, 0)), ((120, 180, 0), (117, 180, 0))], rng))
    # rows: left keys on rows without candidates, rows outside the image, keys that are no keys; one left key left of the image on a row that has a candidate
    kl, dl, kr, dr = base['keys_left'], base['desc_left'], base['keys_right'], base['desc_right']
    lo = kr['y'] < 100; hi = kl['y'] > 150; few = np.nonzero(kl['y'] < 100)[0][:40]
    sk = [_key(10, -100), _key(20, H + 1), _key(30, 1e9), _key(40, np.nan), _key(50, np.inf), _key(60, -np.inf), _key(70, 200, -1), _key(80, 200, 99), _key(30, 50)]
    sl = [_key(50, -5), _key(50, H + 10), _key(50, np.nan), _key(50, -0.5), _key(50, 170, 99), _key(50, 170, -1), _key(-4, 50), _key(50, H - 0.5), _key(np.nan, 50)]
    hand('hand_rows', np.concatenate([kl[hi], kl[few]] + sl), np.concatenate([dl[hi], dl[few], rng.integers(0, 256, (len(sl), 32), dtype=np.uint8)]),
         np.concatenate([kr[lo]] + sk), np.concatenate([dr[lo], rng.integers(0, 256, (len(sk), 32), dtype=np.uint8)]))
    # ties: every matched right key once more at the END of the list, two columns further right, with the same descriptor: the smaller index must win
    e = ref.compute_stereo_matches(kl, dl, kr, dr, *pyrs['small_const'], g['scale'], g['inv_scale'], g['fx'], g['bf'])
    acc = np.nonzero(e['code'] == ref.ACCEPTED)[0][:30]; dup = kr[e['best_idx'][acc]].copy(); dup['x'] += 2
    bi = e['best_idx'][acc]
    hand('hand_ties', kl[acc], dl[acc], np.concatenate([kr[bi], dup]), np.concatenate([dr[bi], dr[bi]]))
    hand('hand_empty_left', kl[:0], dl[:0], kr, dr)
    hand('hand_empty_right', kl, dl, kr[:0], dr[:0])
    # the pair swapped: every true disparity is -3.  A right key at the left key's own position passes the range filter; the window search then finds +3 (disparity
    # < 0), or +5, the end of its range, when the right key stands two columns further left
    o0 = np.nonzero(kr['octave'] == 0)[0][:30]; sk = kr[o0].copy(); sk['x'][15:] -= 2
    hand('hand_swapped', kr[o0], dr[o0], sk, dr[o0], swap=True)
    # the disparity == 0 clamp: three keys on the symmetry column of small_zero's upper third, the same in both images, among real matches of its lower part whose SADs
    # keep the median above 0
    z = C['small_zero']; low = z['keys_left']['y'] > 110; ax = [((W // 2, y, 0), (W // 2, y, 0)) for y in (20, 40, 60)]
    akl, adl, akr, adr = _hand(ax, rng)
    lowr = z['keys_right']['y'] > 100
    hand('hand_clamp', np.concatenate([akl, z['keys_left'][low]]), np.concatenate([adl, z['desc_left'][low]]), np.concatenate([akr, z['keys_right'][lowr]]),
         np.concatenate([adr, z['desc_right'][lowr]]), of='small_zero')
    # SAD ties at exactly thDist: octave-0 keys over the small_sadtie pair, whose SADs are the listed ones
    pts = _sadtie_points()
    C['small_sadtie'].update(dict(zip(('keys_left', 'desc_left', 'keys_right', 'desc_right'), _hand([((x, y, 0), (x - 3, y, 0)) for x, y in pts], rng))), hand=True, name='hand_sadtie')
    C['hand_sadtie'] = C.pop('small_sadtie'); pyrs['hand_sadtie'] = pyrs.pop('small_sadtie')
    for c in C.values():
        c['pyr'] = pyrs[c['name']]; c['fx'] = GEOM[c['geom']]['fx']; c['bf'] = GEOM[c['geom']]['bf']
    _cache[lib.path] = C
    return C


NAMES = SYNTH + ('small_noise', 'hand_clamp', 'hand_borders', 'hand_rows', 'hand_ties', 'hand_empty_left', 'hand_empty_right', 'hand_swapped', 'hand_sadtie')


def expected(c):
    if 'expected' not in c:
        g = GEOM[c['geom']]
        c['expected'] = ref.compute_stereo_matches(c['keys_left'], c['desc_left'], c['keys_right'], c['desc_right'], c['pyr'][0], c['pyr'][1], g['scale'], g['inv_scale'], c['fx'], c['bf'])
    return c['expected']


def check_case_contents(C):
    seen = set()
    for n in NAMES:
        e = expected(C[n]); seen |= set(int(v) for v in e['code'])
        if n in SYNTH:
            kept = int(np.isin(e['code'], (ref.ACCEPTED, ref.ACCEPTED_CLAMPED)).sum())
            assert kept >= 50, (n, kept)
    # DELTA cannot be taken (stereo_ref's docstring has the argument); every other exit must occur
    assert seen >= set(range(11)) - {ref.DELTA}, sorted(set(range(11)) - seen)
    e = expected(C['hand_clamp']); assert (e['code'][:3] == ref.ACCEPTED_CLAMPED).all() and (e['depth'][:3] == F(26.0) / F(0.01)).all(), (e['code'][:3], e['sads'][:3])
    assert (expected(C['small_noise'])['code'] >= ref.ACCEPTED).sum() < 50
    e = expected(C['hand_borders'])['code']; assert (e[:8] == [ref.BORDER, ref.WINDOW_OUTSIDE, ref.BORDER, ref.WINDOW_OUTSIDE, ref.WINDOW_OUTSIDE, ref.WINDOW_OUTSIDE,
                                                              ref.WINDOW_OUTSIDE, ref.CUT]).all(), e      # the one match has SAD 0 = the median: thDist = 0 cuts it, as in the reference
    e = expected(C['hand_ties']); assert (e['best_idx'] < len(e['code'])).all() and (e['best_dist'] < 75).all()      # never one of the copies in the second half
    e = expected(C['hand_swapped'])['code']; assert (e[:15] == ref.DISPARITY).all() and (e[15:] == ref.EDGE_OFFSET).all(), e
    e = expected(C['hand_sadtie']); s = np.array(SADTIE['sads'])
    assert (e['sads'][np.arange(len(s)), 5 + e['best_inc']] == s).all() and (e['code'] == np.where(s >= 21, ref.CUT, ref.ACCEPTED)).all(), (e['code'], e['sads'])
    e = expected(C['hand_rows'])['code']; assert (e[-9:] == [0, 0, 0, 0, 0, 0, ref.LEFT_OF_IMAGE, ref.NO_DESCRIPTOR, ref.NO_DESCRIPTOR]).all(), e[-9:]


def run(lib, cases, to_dev=lambda a: a, to_host=lambda a: a, stream=None, two_handles=False, sync=lambda: None):
    """the cases (one geometry) as ONE batch through sgx_stereo_match_batch_dev: an extraction of the 2B images, the hand-made key sets written over its output, the
    match.  Returns [dict(uright, depth, n, taps...)] per case; taps when the library has them.  two_handles: a left and a right extractor instead of one."""
    from sg_slam_amd.stereo import StereoMatcher
    geom = cases[0]['geom']; g = GEOM[geom]; W, H = g['width'], g['height']; B = len(cases); P = (W + 3) & ~3
    assert all(c['geom'] == geom for c in cases)
    exs = [extractor(lib, geom, B), extractor(lib, geom, B)] if two_handles else [extractor(lib, geom, 2 * B)]
    cap = exs[0].capacity
    gray = np.zeros((2 * B, H, P), np.uint8)
    for i, c in enumerate(cases): gray[i, :, :W] = c['left']; gray[B + i, :, :W] = c['right']
    d_gray = to_dev(gray)
    d_keys = to_dev(np.zeros((2 * B, cap), KP_DTYPE).view(np.uint8).reshape(2 * B, cap * 28)); d_desc = to_dev(np.zeros((2 * B, cap * 32), np.uint8)); d_n = to_dev(np.zeros(2 * B, np.int32))
    if two_handles:
        exs[0].extract_batch_dev(d_gray[:B], P, B, d_keys[:B], d_desc[:B], d_n[:B], stream=stream)
        exs[1].extract_batch_dev(d_gray[B:], P, B, d_keys[B:], d_desc[B:], d_n[B:], stream=stream)
    else:
        exs[0].extract_batch_dev(d_gray, P, 2 * B, d_keys, d_desc, d_n, stream=stream)
    if any(c['hand'] for c in cases):
        sync()
        keys = to_host(d_keys).copy(); desc = to_host(d_desc).copy(); n = to_host(d_n).copy()
        for i, c in enumerate(cases):
            if not c['hand']: continue
            for j, (k, d) in ((i, (c['keys_left'], c['desc_left'])), (B + i, (c['keys_right'], c['desc_right']))):
                assert len(k) <= cap
                keys[j] = 0; desc[j] = 0; n[j] = len(k)
                keys[j, :len(k) * 28] = np.ascontiguousarray(k).view(np.uint8); desc[j, :len(k) * 32] = np.ascontiguousarray(d).reshape(-1)
        d_keys = to_dev(keys); d_desc = to_dev(desc); d_n = to_dev(n)
    d_ur = to_dev(np.full((B, cap), 7, F)); d_z = to_dev(np.full((B, cap), 7, F)); d_nm = to_dev(np.full(B, -7, np.int32))
    sm = StereoMatcher(exs[0], max_batch=B, lib=lib)
    left = (exs[0], 0, d_gray[:B] if two_handles else d_gray, P); right = (exs[1], 0, d_gray[B:], P) if two_handles else (exs[0], B, d_gray, P)
    sm.match_batch_dev(B, *left, *right, d_keys[:B], d_desc[:B], d_n[:B], d_keys[B:], d_desc[B:], d_n[B:], g['fx'], g['bf'], d_ur, d_z, d_nm, stream=stream)
    sync()
    ur = to_host(d_ur); z = to_host(d_z); nm = to_host(d_nm); nn = to_host(d_n)
    out = []
    for i in range(B):
        r = dict(uright=ur[i].copy(), depth=z[i].copy(), nmatched=int(nm[i]), n=int(nn[i]))
        if lib.has_taps: r.update(sm.debug_read(i))
        out.append(r)
    sm.close()
    for e in exs: e.close()
    return out


def assert_same(a, b, what=''):
    """two run() results byte for byte"""
    assert a.keys() == b.keys()
    for k in a: assert np.asarray(a[k]).tobytes() == np.asarray(b[k]).tobytes(), (what, k)


def assert_equal(got, c):
    """one run() result against the restatement, bit for bit; the taps when they were read"""
    e = expected(c); n = len(c['keys_left'])
    assert got['n'] == n, (c['name'], got['n'], n)
    for k in ('uright', 'depth'):
        assert (got[k][:n].view(np.uint32) == e[k].view(np.uint32)).all(), (c['name'], k, np.nonzero(got[k][:n].view(np.uint32) != e[k].view(np.uint32))[0][:5])
        assert (got[k][n:] == -1).all(), (c['name'], k, 'slots beyond n_left')
    assert got['nmatched'] == int((e['uright'] != -1).sum()), c['name']
    if 'code' in got:
        for k in ('best_idx', 'best_dist', 'code', 'best_inc', 'sads'):
            assert (got[k][:n] == e[k]).all(), (c['name'], k, np.argwhere(got[k][:n] != e[k])[:5].tolist())
        assert (got['code'][n:] == -1).all()
