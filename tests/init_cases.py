"""Shared cases for the Initializer (Tracking::MonocularInitialization's two-view initialisation): synthetic frame pairs with ground truth, the restatement
tests/init_ref.py against a library (device or emulator)."""
import ctypes
import functools
import numpy as np
import init_ref as ref
from sg_slam_amd.initializer import Initializer, InitializerBatch

CAM = np.array([535.4, 539.2, 320.1, 247.6], 'f4')          # TUM3


def rot(w):
    th = np.linalg.norm(w)
    if th == 0: return np.eye(3)
    k = w / th; K = np.array([[0, -k[2], k[1]], [k[2], 0, -k[0]], [-k[1], k[0], 0]])
    return np.eye(3) + np.sin(th) * K + (1 - np.cos(th)) * K @ K


def make_scene(seed, n, scene='general', noise=0.0, outliers=0.0, extra1=0, extra2=0, unmatched=0.0, baseline=None, tilt=0.25, far=0, tseed=None):
    """n matched points seen from two cameras.  scene: 'general' (depth 2-6 m, baseline 0.2-0.5 m), 'planar', 'rotation' (no baseline); tilt = the plane's slope along x; far = the
    first `far` points are 60 times as deep (cosParallax >= 0.99998); tseed = seed of the motion alone (default: drawn from `seed` before the points).  noise = keypoint noise in pixels, outliers = share of matches whose second point is anywhere, extra1 / extra2 = unmatched keys appended to the frames (n1 != n2), unmatched = share of
    -1 entries interleaved with the matches.  -> keys1 (n1, 2), keys2 (n2, 2), matches12 (n1), R21, t21 (ground truth), X (n, 3) in camera 1, row of each point in keys1"""
    rng = np.random.RandomState(seed); mrng = rng if tseed is None else np.random.RandomState(tseed)
    R = rot(mrng.normal(0, 0.05, 3))
    b = mrng.uniform(0.2, 0.5) if baseline is None else baseline
    d = mrng.normal(0, 1, 3); d[2] *= 0.3; t = b * d / np.linalg.norm(d)
    if scene == 'rotation': t = np.zeros(3)
    X = np.c_[rng.uniform(-1.5, 1.5, n), rng.uniform(-1.0, 1.0, n), rng.uniform(2.0, 6.0, n)]
    if scene == 'planar': X[:, 2] = 3.5 + tilt * X[:, 0] - 0.15 * X[:, 1]
    X[:far] *= 60
    fx, fy, cx, cy = CAM.astype('f8')
    proj = lambda P: np.c_[fx * P[:, 0] / P[:, 2] + cx, fy * P[:, 1] / P[:, 2] + cy]
    p1 = proj(X) + rng.normal(0, 1, (n, 2)) * noise; p2 = proj((R @ X.T).T + t) + rng.normal(0, 1, (n, 2)) * noise
    bad = rng.rand(n) < outliers
    p2[bad] = np.c_[rng.uniform(0, 640, bad.sum()), rng.uniform(0, 480, bad.sum())]
    n_un = int(round(unmatched * n))
    n1 = n + n_un + extra1; n2 = n + extra2
    rows1 = np.sort(rng.permutation(n + n_un)[:n])                 # matched keys interleaved with unmatched ones
    keys1 = np.c_[rng.uniform(0, 640, n1), rng.uniform(0, 480, n1)]; keys1[rows1] = p1
    perm2 = rng.permutation(n2)
    keys2 = np.c_[rng.uniform(0, 640, n2), rng.uniform(0, 480, n2)]; keys2[perm2[:n]] = p2
    m = np.full(n1, -1, 'i4'); m[rows1] = perm2[:n]
    return keys1.astype('f4'), keys2.astype('f4'), m, R, t, X, rows1


def glibc_rand(seed, count):
    libc = ctypes.CDLL(None)
    libc.srand(seed)
    return np.array([libc.rand() for _ in range(count)], 'i8')


class HostBatch(InitializerBatch):
    """InitializerBatch on the kernel-logic emulator, whose "device" memory is host memory"""
    def _dev(self, a): return np.ascontiguousarray(a).view('u1').reshape(-1).copy()
    def _stream(self): return None
    def _host(self, x, dtype): return x.copy().view(dtype)


def batch_for(lib, B, keys, matches, iterations):
    return (HostBatch if 'EMULATOR' in lib.version() else InitializerBatch)(B, keys, matches, iterations, lib=lib)


# (name, scene arguments, iterations, draw seed, sigma).  N covers 8, 9, 65, 257, 300; iterations 1, 65, 200 and one above the chunk of 256 hypotheses.
CASES = [
    ('general_300', dict(seed=1, n=300, noise=0.3, outliers=0.1, extra1=7, extra2=3, unmatched=0.1), 200, 1, 1.0),
    ('general_257', dict(seed=2, n=257, noise=0.2, outliers=0.2, extra2=11), 200, 2, 1.0),
    ('general_65_its65', dict(seed=3, n=65, noise=0.1, unmatched=0.2), 65, 3, 1.0),
    ('general_300_its300', dict(seed=4, n=300, noise=0.3, outliers=0.3, extra1=2), 300, 4, 1.0),
    ('planar_300', dict(seed=5, n=300, scene='planar', noise=0.3, outliers=0.1, extra1=5), 200, 5, 1.0),
    ('planar_257', dict(seed=6, n=257, scene='planar', noise=0.2, unmatched=0.1), 200, 6, 1.0),
    ('planar_65', dict(seed=7, n=65, scene='planar', noise=0.2), 65, 7, 1.0),
    ('rotation_300', dict(seed=8, n=300, scene='rotation', noise=0.3), 200, 8, 1.0),
    ('rotation_257', dict(seed=9, n=257, scene='rotation', noise=0.0), 200, 9, 1.0),
    ('small_baseline_300', dict(seed=10, n=300, noise=0.2, baseline=0.01), 200, 10, 1.0),
    ('small_baseline_257', dict(seed=11, n=257, noise=0.2, baseline=0.02, extra2=4), 200, 11, 1.0),
    ('planar_ok_300', dict(seed=64, n=300, scene='planar', noise=0.2, baseline=1.0), 200, 12, 1.0),
    ('planar_ok_257', dict(seed=64, n=257, scene='planar', noise=0.2, baseline=0.5, tilt=1.0, extra1=5, unmatched=0.1), 200, 21, 1.0),
    ('planar_low_parallax_300', dict(seed=64, n=300, scene='planar', noise=0.05, baseline=0.03), 200, 22, 1.0),
    ('planar_low_parallax_257', dict(seed=64, n=257, scene='planar', noise=0.05, baseline=0.04, tilt=1.0), 200, 23, 1.0),
    ('general_low_parallax_300', dict(seed=51, n=300, noise=0.1, baseline=0.05), 200, 1, 1.0),
    ('general_low_parallax_257', dict(seed=52, n=257, noise=0.1, baseline=0.05, extra2=9), 200, 1, 1.0),
    ('rh_above_300', dict(seed=50, n=300, noise=0.1, baseline=0.03), 200, 1, 1.0),
    ('rh_below_300', dict(seed=50, n=300, noise=0.1, baseline=0.05), 200, 1, 1.0),
    ('far_points_300', dict(seed=21, n=300, noise=0.1, far=12, unmatched=0.1), 200, 24, 1.0),
    ('outliers_300', dict(seed=13, n=300, noise=0.5, outliers=0.8), 200, 13, 1.0),
    ('outliers_257_its1', dict(seed=14, n=257, noise=0.5, outliers=0.5), 1, 14, 1.0),
    ('n8', dict(seed=15, n=8, noise=0.1, extra1=3, extra2=2), 65, 15, 1.0),
    ('n9', dict(seed=16, n=9, noise=0.1, unmatched=0.5), 200, 16, 1.0),
    ('n9_planar_its1', dict(seed=17, n=9, scene='planar'), 1, 17, 1.0),
    ('general_65_sigma2', dict(seed=18, n=65, noise=1.0, outliers=0.1), 200, 18, 2.0),
    ('rotation_noiseless_300', dict(seed=19, n=300, scene='rotation'), 65, 19, 1.0),
    ('rotation_noiseless_65', dict(seed=20, n=65, scene='rotation', extra1=4), 200, 20, 1.0),
]


@functools.lru_cache(maxsize=None)
def expected(name):
    """the restatement's result of a case, computed once: (scene, draws, result tuple)"""
    _, kw, its, dseed, sigma = next(c for c in CASES if c[0] == name)
    sc = make_scene(**kw)
    draws = glibc_rand(dseed, 8 * its)
    res = ref.InitializerRef(sc[0], CAM, sigma, its).initialize(sc[1], sc[2], draws)
    return sc, draws, res


def bits(a):
    """bit patterns of float32 values; every NaN maps to one pattern (the sign and payload of an invalid operation's NaN differ between processors)"""
    a = np.ascontiguousarray(a, 'f4')
    return np.where(np.isnan(a), np.uint32(0x7fc00000), a.view('u4'))


def assert_same(got, want, what=''):
    """every compared value of Initialize, bit for bit: ok, R21 / t21, p3d, triangulated, inliers, SH / SF / RH, model, n_good, cos_parallax, best_hyp, H21 / F21"""
    gok, gR, gt, gP, gtri, ginl, grep = got; eok, eR, et, eP, etri, einl, erep = want
    assert gok == eok, (what, gok, eok, grep, erep)
    assert (bits(gR) == bits(eR)).all() and (bits(gt) == bits(et)).all(), (what, gR, eR, gt, et)
    assert (gtri == etri).all() and (ginl == einl).all(), what
    assert (bits(gP) == bits(eP)).all(), what
    for k in ('SH', 'SF', 'RH', 'H21', 'F21', 'cos_parallax', 'parallax'):
        assert (bits(grep[k]) == bits(erep[k])).all(), (what, k, grep[k], erep[k])
    for k in ('model', 'n_matches', 'n_inliers_h', 'n_inliers_f', 'n_hyp', 'best_hyp'):
        assert grep[k] == erep[k], (what, k, grep[k], erep[k])
    assert (np.asarray(grep['n_good']) == np.asarray(erep['n_good'])).all(), (what, grep['n_good'], erep['n_good'])


def run_case(lib, name):
    """one case on the library (caller draws) against the restatement"""
    _, kw, its, dseed, sigma = next(c for c in CASES if c[0] == name)
    sc, draws, want = expected(name)
    S = Initializer(sc[0], CAM, sigma, its, lib=lib)
    got = S.Initialize(sc[1], sc[2], draws)
    S.close()
    assert_same(got, want, name)
    return got


def check_regrow_carries_replica(lib):
    """one Initializer (12 keys in frame 1, 8 iterations, srand(5)) under its own rand() replica: a second frame of 12 keys, then one of 40, for which the batch of one
    behind it is rebuilt.  The replica's state moves into the new batch, so the second call draws glibc's values 8 x its .. 16 x its - 1"""
    its = 8
    a = make_scene(seed=31, n=12, noise=0.2); b = make_scene(seed=31, n=12, noise=0.2, extra2=28)
    assert len(a[1]) == 12 and len(b[1]) == 40 and (a[0] == b[0]).all()
    d = glibc_rand(5, 16 * its)
    R = ref.InitializerRef(a[0], CAM, 1.0, its)
    S = Initializer(a[0], CAM, 1.0, its, rand_seed=5, lib=lib)
    assert_same(S.Initialize(a[1], a[2]), R.initialize(a[1], a[2], d[:8 * its]), 'regrow: 12 keys')
    assert_same(S.Initialize(b[1], b[2]), R.initialize(b[1], b[2], d[8 * its:]), 'regrow: 40 keys')
    S.close()


def check_batch_equals_single(lib, names, caller_draws=False):
    """the cases `names` (same iterations) in one batch == one Initializer each, with their own rand() replicas or with each pair's libc values passed in"""
    cs = [next(c for c in CASES if c[0] == n) for n in names]
    its = cs[0][2]; assert all(c[2] == its for c in cs)
    scs = [make_scene(**c[1]) for c in cs]
    n1 = sum(len(s[0]) for s in scs); n2 = sum(len(s[1]) for s in scs)
    Bt = batch_for(lib, len(cs), max(n1, n2), n1, its)
    Bt.set([(s[0], s[1], s[2], CAM) for s in scs], sigma=[c[4] for c in cs])
    seeds = [c[3] for c in cs]
    if caller_draws: res = Bt.run(rand_draws=np.stack([glibc_rand(sd, 8 * its + 5) for sd in seeds]))
    else: res = Bt.run(rand_seeds=seeds)
    for c, s, r in zip(cs, scs, res):
        S = Initializer(s[0], CAM, c[4], its, rand_seed=c[3], lib=lib)
        assert_same(r, S.Initialize(s[1], s[2], glibc_rand(c[3], 8 * its) if caller_draws else None), c[0])
        S.close()
    Bt.close()
    return res
