"""Initializer on the CPU tier: the restated OpenCV float SVD against numpy.linalg, the restatement (tests/init_ref.py) against ground truth, the rand() replica
against this machine's libc, the kernel-logic emulator against the restatement bit for bit on every case, the reference's quirks and the defined cases one test each,
the batch against single initializers."""
import numpy as np
import pytest
import init_cases as ic
import init_ref as ref
from sg_slam_amd.initializer import Initializer

OUTCOMES = ('ok_h', 'ok_f', 'parallax', 'ambiguous', 'd_ratio_exit')


def test_case_list_covers_every_outcome():
    """at least two cases each: H path ok, F path ok, rejected by parallax, rejected by nsimilar > 1 / maxGood < nMinGood (or ReconstructH's counterpart), the d1/d2 exit;
    and the shapes at which indexing can go wrong: N in {8, 9, 65, 257, 300}, 1 / 65 / 200 iterations and one count above the chunk of 256"""
    got = {}
    for c in ic.CASES: got.setdefault(ic.expected(c[0])[2][6]['outcome'], []).append(c[0])
    for o in OUTCOMES: assert len(got.get(o, [])) >= 2, (o, got)
    assert {ic.expected(c[0])[2][6]['n_matches'] for c in ic.CASES} >= {8, 9, 65, 257, 300}
    assert {c[2] for c in ic.CASES} >= {1, 65, 200} and max(c[2] for c in ic.CASES) > 256


# ---------------------------------------------------------------------------------------------------------------------------------------------------- the float SVD
# float one-sided Jacobi against double LAPACK: the bounds are 10 x the largest deviation seen over the seeds below (relative to the largest singular value)
SVD_TOL = {'w': 2.6e-6, 'Av': 2.0e-6, 'unit': 3.0e-6, 'orth': 7.0e-7}         # seen: 2.53e-7, 1.97e-7, 2.91e-7, 6.70e-8


def _svd_dev(seed):
    rng = np.random.RandomState(seed); dev = dict(w=0.0, Av=0.0, unit=0.0, orth=0.0)
    upd = lambda k, v: dev.__setitem__(k, max(dev[k], float(v)))
    for m, n in ((16, 9), (3, 3), (4, 4)):
        A = rng.normal(size=(5, m, n)).astype('f4')
        At, W, Vt = ref.jacobi(np.swapaxes(A, 1, 2), m, n, 0)
        sv = np.linalg.svd(A.astype('f8'), compute_uv=False)
        upd('w', (np.abs(W - sv) / sv[:, :1]).max())
        last = Vt[:, n - 1, :].astype('f8')
        upd('Av', (np.abs(np.linalg.norm(np.einsum('hmn,hn->hm', A.astype('f8'), last), axis=1) - sv[:, -1]) / sv[:, 0]).max())
        upd('unit', np.abs(np.linalg.norm(last, axis=1) - 1).max())
    A = rng.normal(size=(5, 8, 9)).astype('f4')                   # m < n, FULL_UV: the rows of A are rotated, the ninth row is completed
    At, W, Vt = ref.jacobi(np.concatenate([A, np.zeros((5, 1, 9), 'f4')], 1), 9, 8, 9, want_vt=False)
    sv = np.linalg.svd(A.astype('f8'), compute_uv=False)
    upd('w', (np.abs(W - sv) / sv[:, :1]).max())
    row = At[:, 8, :].astype('f8')
    upd('unit', np.abs(np.linalg.norm(row, axis=1) - 1).max())
    upd('orth', np.abs(np.einsum('hrk,hk->hr', At[:, :8, :].astype('f8'), row)).max())
    upd('Av', (np.linalg.norm(np.einsum('hmn,hn->hm', A.astype('f8'), row), axis=1) / sv[:, 0]).max())
    return dev


@pytest.mark.parametrize('seed', range(4))
def test_restated_float_svd_against_lapack(seed):
    dev = _svd_dev(seed)
    print('svd deviations', seed, dev)
    for k, v in dev.items(): assert v <= SVD_TOL[k], (k, v)


# ---------------------------------------------------------------------------------------------------------------------------------------------------- ground truth
# noiseless scenes, restatement against the true motion: 10 x the largest deviation over the listed seeds; the cap is 1e-2 rad / 1e-2 relative
GT_SEEDS = (101, 102, 103, 104)
GT_TOL = {'rot': 3.0e-3, 'dir': 3.1e-3, 'pts': 8.3e-4}                      # seen: 2.94e-4 rad, 3.06e-4 rad, 8.25e-5


def _gt_dev(seed):
    k1, k2, m, R, t, X, rows = ic.make_scene(seed, 200)
    ok, R21, t21, P, tri, inl, rep = ref.InitializerRef(k1, ic.CAM, 1.0, 200).initialize(k2, m, ic.glibc_rand(seed, 1600))
    assert ok, rep
    dR = R21.astype('f8') @ R.T
    rot_err = np.arccos(np.clip((np.trace(dR) - 1) / 2, -1, 1))
    dir_err = np.arccos(np.clip(t21.astype('f8') @ (t / np.linalg.norm(t)), -1, 1))
    g = tri[rows]
    pts_err = (np.linalg.norm(P[rows][g].astype('f8') * np.linalg.norm(t) - X[g], axis=1) / np.linalg.norm(X[g], axis=1)).max()
    assert g.sum() > 150
    return dict(rot=float(rot_err), dir=float(dir_err), pts=float(pts_err))


@pytest.mark.parametrize('seed', GT_SEEDS)
def test_restatement_recovers_ground_truth(seed):
    dev = _gt_dev(seed)
    print('ground truth deviations', seed, dev)
    for k, v in dev.items(): assert v <= GT_TOL[k] <= 1e-2, (k, v)


# ---------------------------------------------------------------------------------------------------------------------------------------------------- random numbers
def test_replica_draws_equal_libc_rand(emu):
    """mvSets from the object's glibc replica (srand(seed) at creation, continuing across calls) = this machine's srand / rand"""
    name = 'general_65_its65'; c = next(c for c in ic.CASES if c[0] == name); sc = ic.make_scene(**c[1]); its = c[2]
    for seed in (0, 1, 77):
        d = ic.glibc_rand(seed if seed else 1, 16 * its)           # srand(0) = srand(1) in glibc
        S = Initializer(sc[0], ic.CAM, 1.0, its, rand_seed=seed, lib=emu); T = Initializer(sc[0], ic.CAM, 1.0, its, lib=emu)
        for call in range(2):
            ic.assert_same(S.Initialize(sc[1], sc[2]), T.Initialize(sc[1], sc[2], d[8 * its * call:8 * its * (call + 1)]), (seed, call))
        S.close(); T.close()
    assert (ic.glibc_rand(0, 8) == ic.glibc_rand(1, 8)).all()


def test_second_frame_with_more_keys_continues_the_replica(emu):
    ic.check_regrow_carries_replica(emu)


def test_draw_sets_are_the_swap_and_pop_of_the_reference():
    """RandomInt(0, size - 1) over the shrinking vAvailableIndices with swap-with-back removal, against a literal list implementation"""
    d = ic.glibc_rand(5, 8 * 50).reshape(50, 8)
    for N in (8, 9, 65):
        got = ref.draw_sets(N, d)
        for h in range(50):
            avail = list(range(N)); want = []
            for k in range(8):
                r = int((float(d[h, k]) / (2147483647.0 + 1.0)) * len(avail)); want.append(avail[r]); avail[r] = avail[-1]; avail.pop()
            assert list(got[h]) == want
            assert len(set(want)) == 8


# ---------------------------------------------------------------------------------------------------------------------------------------------------- bit for bit
@pytest.mark.parametrize('name', [c[0] for c in ic.CASES])
def test_emulator_equals_restatement(emu, name):
    ic.run_case(emu, name)


def test_call_longer_than_one_chunk(emu):
    """300 iterations: two launches of the hypothesis kernels (256 + 44).  In this case the H winner comes from the second launch and the F winner from the first, so the
    best model has to be both replaced and carried across the chunk boundary"""
    c = next(c for c in ic.CASES if c[0] == 'general_300_its300'); assert c[2] > 256
    got = ic.run_case(emu, c[0])
    sc, d, want = ic.expected(c[0])
    M = ref.InitializerRef(sc[0], ic.CAM, 1.0, c[2]).models(sc[1], sc[2], d)
    assert M['win_h'] >= 256 > M['win_f'] >= 0
    S = Initializer(sc[0], ic.CAM, 1.0, 256, lib=emu); short = S.Initialize(sc[1], sc[2], d[:8 * 256]); S.close()
    assert short[6]['SH'] < got[6]['SH'] and short[6]['SF'] == got[6]['SF']


def test_batch_equals_single(emu):
    names = [c[0] for c in ic.CASES if c[2] == 200]
    ic.check_batch_equals_single(emu, names)
    ic.check_batch_equals_single(emu, names[:6], caller_draws=True)
    ic.check_batch_equals_single(emu, ['general_300_its300'])


# ---------------------------------------------------------------------------------------------------------------------------------------------------- quirks
def _draws_for_positions(N, positions):
    """raw rand() values that make one iteration pick the positions given of the shrinking index list"""
    return [int((p + 0.5) * 2147483648.0 / (N - k)) for k, p in enumerate(positions)]


def test_strict_first_maximum():
    """`currentScore > score` from 0: ties keep the earlier iteration, a zero or NaN score never wins"""
    assert ref.first_strict_max(np.array([1, 3, 3, 2], 'f4')) == (1, np.float32(3))
    assert ref.first_strict_max(np.array([0, 0], 'f4'))[0] == -1
    assert ref.first_strict_max(np.array([np.nan, 2, np.nan], 'f4')) == (1, np.float32(2))


def test_strict_first_maximum_on_repeated_iterations(emu):
    """iterations that repeat iteration 0's draws score the same: the result is the one of iteration 0 alone when it is the best (also checks the per-iteration draw layout)"""
    c = next(c for c in ic.CASES if c[0] == 'general_65_its65'); sc = ic.make_scene(**c[1])
    d = ic.glibc_rand(3, 8)
    one = Initializer(sc[0], ic.CAM, 1.0, 1, lib=emu).Initialize(sc[1], sc[2], d)
    many = Initializer(sc[0], ic.CAM, 1.0, 5, lib=emu).Initialize(sc[1], sc[2], np.tile(d, 5))
    ic.assert_same(many, one)


def test_fundamental_gate_3_841_score_5_991(emu):
    """a match with 3.841 < chiSquare <= 5.991 is no inlier and adds nothing, one below 3.841 adds 5.991 - chiSquare"""
    sc = ic.make_scene(34, 200, noise=1.2); its = 50; d = ic.glibc_rand(4, 8 * its)
    O = ref.InitializerRef(sc[0], ic.CAM, 1.0, its); M = O.models(sc[1], sc[2], d)
    F21 = M['F21'][None]
    s_ref, inl = ref.check_fundamental(F21, M['xy'], 1.0)
    # the same matrix scored with one threshold for both: more inliers and another score, so this scene can tell the two rules apart
    import unittest.mock as mock
    with mock.patch.object(ref, '_score', lambda c1, c2, th, ths, f=ref._score: f(c1, c2, ths, ths)):
        s_one, inl_one = ref.check_fundamental(F21, M['xy'], 1.0)
    assert inl_one.sum() > inl.sum() and s_one[0] != s_ref[0]
    got = Initializer(sc[0], ic.CAM, 1.0, its, lib=emu).Initialize(sc[1], sc[2], d)
    ic.assert_same(got, O.initialize(sc[1], sc[2], d))
    assert np.float32(got[6]['SF']) == s_ref[0] == M['SF'] and got[6]['n_inliers_f'] == inl.sum()


def test_low_parallax_point_is_counted_and_written_but_not_triangulated(emu):
    got = ic.run_case(emu, 'far_points_300')
    ok, R, t, P, tri, inl, rep = got
    sc = ic.expected('far_points_300')[0]; rows = sc[6]
    assert ok
    far = rows[:12]
    written = (P != 0).any(1)
    assert written[far].all() and not tri[far].any()              # cosParallax >= 0.99998: vP3D written, vbGood false
    assert rep['n_good'][rep['best_hyp']] == written.sum() > tri.sum() > 200


def test_points_are_indexed_by_the_keypoint_of_frame_1(emu):
    ok, R, t, P, tri, inl, rep = ic.run_case(emu, 'general_300')
    k1, k2, m, Rt, tt, X, rows = ic.expected('general_300')[0]
    assert ok and len(k1) > 300 and (rows != np.arange(300)).any()
    unmatched = np.setdiff1d(np.arange(len(k1)), rows)
    assert not (P[unmatched] != 0).any() and not tri[unmatched].any() and not inl[unmatched].any()
    w = (P != 0).any(1); fx, fy, cx, cy = ic.CAM.astype('f8'); Q = P[w].astype('f8')
    uv = np.c_[fx * Q[:, 0] / Q[:, 2] + cx, fy * Q[:, 1] / Q[:, 2] + cy]
    assert w.sum() > 200 and (np.linalg.norm(uv - k1[w], axis=1) <= 2.001).all()      # CheckRT's gate: every written point reprojects within 2 sigma of ITS key


def test_parallax_index_with_fewer_than_51_good_points(emu):
    """vCosParallax[min(50, size - 1)]: with 9 good points the largest cosine; always ok = 0"""
    ok, R, t, P, tri, inl, rep = ic.run_case(emu, 'n9')
    sc, d, want = ic.expected('n9')
    M = ref.InitializerRef(sc[0], ic.CAM, 1.0, 200).models(sc[1], sc[2], d)
    Rs, ts = ref.decompose_e(M['F21'], ic.CAM)
    state, cosp, X = ref.check_rt(Rs, ts, M['xy'], M['inl_f'], ic.CAM, np.float32(4.0))
    q = int(np.argmax(rep['n_good']))
    assert not ok and 0 < rep['n_good'][q] < 51
    assert np.float32(rep['cos_parallax'][q]) == cosp[q][state[q] > 0].max()


def test_reconstruct_f_tests_the_first_best_hypothesis_only(emu):
    """the else-if chain of ReconstructF looks at the parallax of the first hypothesis whose nGood equals maxGood; a tie has nsimilar >= 2 and was rejected before, so
    through Initialize the rule shows as: ok = clear winner and that hypothesis' parallax > 1"""
    seen = set()
    for c in ic.CASES:
        r = ic.expected(c[0])[2]; rep = r[6]
        if rep['model'] != 1 or rep['n_hyp'] != 4: continue
        ng = rep['n_good'][:4]; best = int(np.nonzero(ng == ng.max())[0][0])
        assert rep['best_hyp'] == best
        clear = ng.max() >= max(int(0.9 * rep['n_inliers_f']), 50) and (ng > 0.7 * ng.max()).sum() <= 1
        assert r[0] == bool(clear and rep['parallax'][best] > 1.0)
        seen.add((bool(clear), bool(r[0])))
        ic.run_case(emu, c[0]) if (bool(clear), bool(r[0])) == (True, False) else None
    assert seen >= {(True, True), (True, False), (False, False)}


def test_rh_on_both_sides_of_0_40(emu):
    a = ic.run_case(emu, 'rh_above_300')[6]; b = ic.run_case(emu, 'rh_below_300')[6]
    assert 0.40 < a['RH'] < 0.45 and a['model'] == 0 and a['n_hyp'] == 8
    assert 0.35 < b['RH'] <= 0.40 and b['model'] == 1 and b['n_hyp'] == 4


# ---------------------------------------------------------------------------------------------------------------------------------------------------- defined cases
def test_fewer_than_8_matches_consumes_nothing(emu):
    sc = ic.make_scene(31, 60, noise=0.1)
    m7 = sc[2].copy(); m7[np.nonzero(m7 >= 0)[0][7:]] = -1
    S = Initializer(sc[0], ic.CAM, 1.0, 65, rand_seed=9, lib=emu)
    ok, R, t, P, tri, inl, rep = S.Initialize(sc[1], m7)
    assert not ok and rep['n_matches'] == 7 and rep['n_hyp'] == 0 and not inl.any() and not P.any()
    ic.assert_same((ok, R, t, P, tri, inl, rep), ref.InitializerRef(sc[0], ic.CAM, 1.0, 65).initialize(sc[1], m7, None))
    T = Initializer(sc[0], ic.CAM, 1.0, 65, rand_seed=9, lib=emu)
    ic.assert_same(S.Initialize(sc[1], sc[2]), T.Initialize(sc[1], sc[2]))          # the first call drew nothing
    S.close(); T.close()


def test_all_scores_zero_is_not_ok(emu):
    """every match fails both gates of every hypothesis (gross outliers, sigma = 1e-5: even the eight sampled points miss): SH = SF = 0, RH = 0 / 0, no matrix to decompose"""
    sc = ic.make_scene(32, 40, outliers=1.0)
    got = Initializer(sc[0], ic.CAM, 1e-5, 20, lib=emu).Initialize(sc[1], sc[2], ic.glibc_rand(1, 160))
    want = ref.InitializerRef(sc[0], ic.CAM, 1e-5, 20).initialize(sc[1], sc[2], ic.glibc_rand(1, 160))
    ic.assert_same(got, want)
    assert not got[0] and got[6]['SH'] == 0 and got[6]['SF'] == 0 and np.isnan(got[6]['RH']) and want[6]['outcome'] == 'no_model' and not got[5].any()


def test_nan_hypothesis_never_wins(emu):
    """frame 2 has one key, so Normalize divides by a zero deviation and every hypothesis of both models scores NaN: `currentScore > score` is false for each of them"""
    k1, k2, m, R, t, X, rows = ic.make_scene(33, 80, noise=0.1)
    m1 = np.where(m >= 0, 0, -1).astype('i4'); its = 10; d = ic.glibc_rand(2, 8 * its)
    O = ref.InitializerRef(k1, ic.CAM, 1.0, its)
    M = O.models(k2[:1], m1, d)
    assert M['N'] == 80 and np.isnan(M['scores_h']).all() and np.isnan(M['scores_f']).all()
    got = Initializer(k1, ic.CAM, 1.0, its, lib=emu).Initialize(k2[:1], m1, d)
    ic.assert_same(got, O.initialize(k2[:1], m1, d))
    assert not got[0] and got[6]['SH'] == 0 and got[6]['SF'] == 0 and not got[6]['H21'].any() and not got[6]['F21'].any()


def test_degenerate_sample_of_one_point_eight_times(emu):
    """iteration 0 samples eight coincident matches (a rank-deficient system for both models): the same bits as the restatement, and the later iterations decide"""
    k1, k2, m, R, t, X, rows = ic.make_scene(33, 80, noise=0.1)
    k1[rows[:8]] = k1[rows[0]]; k2[m[rows[:8]]] = k2[m[rows[0]]]
    its = 30
    d = np.concatenate([_draws_for_positions(80, range(8)), ic.glibc_rand(2, 8 * (its - 1))])
    O = ref.InitializerRef(k1, ic.CAM, 1.0, its)
    M = O.models(k2, m, d)
    assert list(M['sets'][0]) == list(range(8)) and M['win_h'] > 0 and M['win_f'] > 0
    one = Initializer(k1, ic.CAM, 1.0, 1, lib=emu).Initialize(k2, m, d[:8])
    ic.assert_same(one, ref.InitializerRef(k1, ic.CAM, 1.0, 1).initialize(k2, m, d[:8]))
    ic.assert_same(Initializer(k1, ic.CAM, 1.0, its, lib=emu).Initialize(k2, m, d), O.initialize(k2, m, d))
