"""Shared cases for the device KeyFrameDatabase (sgx_kfdb_*): a "places" generator, hand-made cases (one per rule of KeyFrameDatabase.cc) and the runner that plays a
script of database operations on the device (or the emulator) and on the restatement of tests/kfdb_ref.py and compares them bit for bit.  A script is a list of
  ('add', id, bow) ('cov', id, ids) ('erase', id) ('clear',) ('reloc', bow) ('loop', bow, connected, minScore) ('min', bow, ids)
with bow = (ids ascending int32, weights float64)."""
import numpy as np
import kfdb_ref
from sg_slam_amd.vocabulary import ORBVocabulary
from sg_slam_amd.keyframedatabase import KeyFrameDatabase, RELOCALIZATION, LOOP_CLOSING

F = np.float32


def make_voc(lib, nwords, scoring=0):
    """a vocabulary of nwords words: a root with nwords leaves (the database takes only its size and its scoring type)"""
    n = nwords + 1
    parent = np.zeros(n, 'i4'); leaf = np.ones(n, np.uint8); leaf[0] = 0
    return ORBVocabulary(lib).create(10, 1, parent, np.zeros((n, 32), np.uint8), np.ones(n, 'f8'), leaf, scoring, 0)


def bow_of(words, weights=None, rng=None):
    words = np.array(sorted(set(int(w) for w in words)), 'i4')
    if weights is None:
        weights = rng.uniform(0.1, 1.0, len(words)) if rng is not None else np.ones(len(words))
    weights = np.asarray(weights, 'f8')
    return words, weights / np.abs(weights).sum()


# ---- the generator -----------------------------------------------------------------------------------------------------------------------------------------------
def places_script(seed, mode, N=120, nwords=4000, places=12, per_place=150, nq=8, lo=30, hi=200):
    """N keyframes walk through `places` places in time order; a keyframe draws lo..hi entries, 70 % of them from its place's words; weights uniform, L1-normalised;
    covisibility = up to 10 shuffled ids of the +-7 temporal neighbours.  nq queries from random places, then one from words no keyframe can hold (an empty result)."""
    rng = np.random.RandomState(seed)
    usable = nwords - 20                                                   # the top 20 words stay unused: the last query lives there
    pw = [rng.choice(usable, per_place, replace=False) for _ in range(places)]
    def draw(p):
        n = rng.randint(lo, hi + 1); k = min(int(round(0.7 * n)), per_place)
        return bow_of(np.concatenate([rng.choice(pw[p], k, replace=False), rng.randint(0, usable, n - k)]), rng=rng)
    place = lambda i: i * places // N
    ops = []
    for i in range(N):
        ops.append(('add', 10 + 3 * i, draw(place(i))))
    for i in range(N):
        nb = [10 + 3 * j for j in range(max(0, i - 7), min(N, i + 8)) if j != i]
        rng.shuffle(nb)
        ops.append(('cov', 10 + 3 * i, nb[:10]))
    for q in range(nq):
        j = rng.randint(0, N); b = draw(place(j))
        if mode == RELOCALIZATION: ops.append(('reloc', b))
        else:
            conn = [10 + 3 * t for t in range(max(0, j - 5), min(N, j + 6))]
            ops.append(('loop', b, conn, None))                           # None: minScore = min_score over the connected keyframes, as LoopClosing::DetectLoop
    far = bow_of(np.arange(usable, nwords), rng=rng)
    ops.append(('reloc', far) if mode == RELOCALIZATION else ('loop', far, [], 0.01))
    return dict(name=f'places-{seed}-{mode}', nwords=nwords, ops=ops)


# ---- hand-made cases: each carries its written-down answer as `expect` = list of candidate lists, one per query ---------------------------------------------------
def hand_cases():
    C = []
    # the inverted-file order: keyframe 2's first common word (2) precedes keyframe 1's (5) though 1 was added first; two keyframes whose first common word is the same (7)
    # come in add() order, whichever id was added first
    ops = [('add', 1, bow_of([5, 6, 100])), ('add', 2, bow_of([2, 6, 101])), ('reloc', bow_of([2, 5, 6]))]
    C.append(dict(name='order-first-word', nwords=200, ops=ops, expect=[[2, 1]]))
    ops = [('add', 9, bow_of([7, 8, 100])), ('add', 4, bow_of([7, 8, 101])), ('reloc', bow_of([7, 8]))]
    C.append(dict(name='order-add-sequence', nwords=200, ops=ops, expect=[[9, 4]]))
    ops = [('add', 4, bow_of([7, 8, 101])), ('add', 9, bow_of([7, 8, 100])), ('reloc', bow_of([7, 8]))]
    C.append(dict(name='order-add-sequence-swapped', nwords=200, ops=ops, expect=[[4, 9]]))
    # maxCommonWords in {4, 5, 6, 10}: (int)(m * 0.8f) = 3, 4, 4, 8 (5 * 0.8f is exactly 4.0f in float, 4.000000059... before rounding); a keyframe with exactly that
    # many common words fails the gate (n_scores 1), one with one more passes (n_scores 2) and, scoring (minw + 1) / (minw + 3) against keyframe 1's m / (m + 1), is retained
    for m, minw in ((4, 3), (5, 4), (6, 4), (10, 8)):
        for extra in (0, 1):
            q = list(range(m))
            ops = [('add', 1, bow_of(q + [150])), ('add', 2, bow_of(list(range(minw + extra)) + [151, 152])), ('reloc', bow_of(q))]
            C.append(dict(name=f'gate-{m}-{extra}', nwords=200, ops=ops, expect=[[1, 2][:1 + extra]], expect_report=[dict(max_common_words=m, min_common_words=minw, n_scores=1 + extra)]))
    # a stale score that changes the candidate list.  Query 1 scores keyframe 2 (10 / 11).  Query 2 matches keyframe 1 fully (1.0), keyframe 3 in 9 of 15 words (0.6),
    # and shares one word with 2, which fails the gate but is 3's neighbour: 3's entry accumulates 2's stale 10 / 11, names 2 as its pBestKF (10 / 11 > 0.6) and reaches
    # 1.509; keyframe 1 (acc 1.0) falls below 0.75 of that.  The answer is the keyframe this query never scored.  With the stale score zeroed it would be [1].
    k1 = bow_of(range(0, 10)); k2 = bow_of(list(range(20, 30)) + [9]); k3 = bow_of(list(range(0, 9)) + [40, 41, 42, 43, 44, 45])
    ops = [('add', 1, k1), ('add', 2, k2), ('add', 3, k3), ('cov', 3, [2]), ('reloc', bow_of(range(20, 30))), ('reloc', bow_of(range(0, 10)))]
    C.append(dict(name='stale-changes-result', nwords=200, ops=ops, expect=[[2], [2]], stale_matters=True))
    # the same with the neighbour erased before the second query: nothing stale to add; 1 stands, 3 (0.6) is below 0.75
    ops = ops[:5] + [('erase', 2), ('reloc', bow_of(range(0, 10)))]
    C.append(dict(name='erased-neighbour', nwords=200, ops=ops, expect=[[2], [1]]))
    # loop: the connected keyframe 1 shares all 10 words; the maximum comes from 2 (5 words): min 4, so 3 (5 words) is scored too; with 1 counted the gate would be 8
    ops = [('add', 1, bow_of(range(0, 10))), ('add', 2, bow_of(list(range(0, 5)) + [50])), ('add', 3, bow_of(list(range(5, 10)) + [51])),
           ('loop', bow_of(range(0, 10)), [1], 0.0)]
    C.append(dict(name='loop-connected-max', nwords=200, ops=ops, expect=[[2, 3]], expect_report=[dict(n_sharing=2, max_common_words=5, min_common_words=4, n_scores=2)]))
    # si == minScore is kept: the score of identical vectors of 4 equal weights is exactly 1; accScore == 0.75f * best is dropped: scores 1 and 0.75
    same = bow_of(range(0, 4))
    ops = [('add', 1, same), ('loop', same, [], 1.0)]
    C.append(dict(name='loop-si-equals-min', nwords=200, ops=ops, expect=[[1]], expect_report=[dict(n_score_and_match=1)]))
    # keyframe 2 holds the query's four words at 0.1875 and a fifth at 0.25: it passes the word gate and scores 4 * 0.1875 = 0.75 exactly, which is not > 0.75f * 1
    ops = [('add', 1, same), ('add', 2, (np.array([0, 1, 2, 3, 60], 'i4'), np.array([0.1875] * 4 + [0.25]))), ('reloc', same)]
    C.append(dict(name='acc-equals-retain', nwords=200, ops=ops, expect=[[1]], expect_report=[dict(n_score_and_match=2, best_acc_score=F(1), min_score_to_retain=F(0.75))]))
    # the three empty returns: nothing shares a word (both modes); every scored keyframe falls below minScore (loop)
    ops = [('add', 1, bow_of([1, 2, 3])), ('reloc', bow_of([10, 11])), ('loop', bow_of([10, 11]), [], 0.0), ('loop', bow_of([1, 2, 50, 51, 52]), [], 0.9),
           ('loop', bow_of([1, 2, 3]), [1], 0.0)]
    C.append(dict(name='empty-returns', nwords=200, ops=ops, expect=[[], [], [], []],
                  expect_report=[dict(n_sharing=0), dict(n_sharing=0), dict(n_sharing=1, n_scores=1, n_score_and_match=0), dict(n_sharing=0)]))
    # a sparse vocabulary: most keyframes share nothing with the query
    rng = np.random.RandomState(5)
    ops = [('add', i, bow_of(rng.randint(0, 200000, 40), rng=rng)) for i in range(60)]
    ops += [('add', 100, bow_of([7, 70000, 150000, 199999], rng=rng)), ('add', 101, bow_of([7, 70000, 199999, 5], rng=rng)), ('cov', 100, [101, 3]),
            ('reloc', bow_of([7, 70000, 150000, 199999], rng=rng)), ('loop', bow_of([7, 70000, 150000, 199999], rng=rng), [101], 0.0)]
    C.append(dict(name='sparse-vocabulary', nwords=200000, ops=ops))
    return C


def container_script(seed=11, nwords=500):
    """interleaved add / erase / clear / queries with a pool far smaller than the total of what is ever added: erase must give entries back"""
    rng = np.random.RandomState(seed)
    ops = []; live = []; nid = 0
    draw = lambda: bow_of(rng.randint(0, nwords, rng.randint(5, 40)), rng=rng)
    for step in range(160):
        r = rng.rand()
        if step == 90: ops.append(('clear',)); live = []; continue
        if r < 0.5 and len(live) < 12:
            ops.append(('add', nid, draw())); live.append(nid); nid += 1
            if len(live) > 1: ops.append(('cov', live[-1], [int(x) for x in rng.choice(live, min(len(live), 4), replace=False)] + [9999]))
        elif r < 0.75 and live:
            ops.append(('erase', live.pop(rng.randint(len(live)))))
        elif r < 0.9: ops.append(('reloc', draw()))
        else: ops.append(('loop', draw(), [int(x) for x in live[:3]], 0.0))
    return dict(name='container', nwords=nwords, ops=ops, max_keyframes=12, max_bow_entries=12 * 40)


# ---- the runner --------------------------------------------------------------------------------------------------------------------------------------------------
def bits(x):
    return np.asarray(x, 'f4').view('u4')


def check_report(got, ref, what):
    for k in ('n_sharing', 'max_common_words', 'min_common_words', 'n_scores', 'n_score_and_match', 'n_candidates'):
        assert int(got[k]) == int(ref[k]), (what, k, int(got[k]), int(ref[k]))
    for k in ('best_acc_score', 'min_score_to_retain'):
        assert bits(got[k]) == bits(ref[k]), (what, k, float(got[k]), float(ref[k]))


def run_script(lib, case, via='batch', max_query_words=0):
    """plays the script on the device database and on the restatement; every query is compared: candidates in order, the report with its floats as bits and, through the
    batch entry, mnRelocWords / mnLoopWords and the score of every keyframe.  Returns (restatement, list of candidate lists)."""
    voc = make_voc(lib, case['nwords'])
    ops = case['ops']
    max_kf = case.get('max_keyframes') or max(1, sum(1 for o in ops if o[0] == 'add'))
    max_ent = case.get('max_bow_entries') or max(1, sum(len(o[2][0]) for o in ops if o[0] == 'add'))
    D = KeyFrameDatabase(voc, max_keyframes=max_kf, max_bow_entries=max_ent, max_query_words=max_query_words, max_queries=4)
    R = kfdb_ref.KeyFrameDatabase(case['nwords'])
    results = []
    for k, op in enumerate(ops):
        what = (case['name'], k, op[0])
        if op[0] == 'add': D.add(op[1], op[2]); R.add(op[1], op[2])
        elif op[0] == 'cov': D.set_covisibility(op[1], op[2]); R.set_covisibility(op[1], op[2])
        elif op[0] == 'erase': D.erase(op[1]); R.erase(op[1])
        elif op[0] == 'clear': D.clear(); R.clear()
        elif op[0] == 'min':
            assert bits(D.min_score(op[1], op[2])) == bits(R.min_score(op[1], op[2])), what
        else:
            mode = RELOCALIZATION if op[0] == 'reloc' else LOOP_CLOSING
            bow = op[1]; conn = ms = None
            if mode == LOOP_CLOSING:
                conn = op[2]; ms = op[3]
                if ms is None:
                    ms = R.min_score(bow, conn)
                    assert bits(D.min_score(bow, conn)) == bits(ms), what
            ref = R.DetectRelocalizationCandidates(bow) if mode == RELOCALIZATION else R.DetectLoopCandidates(bow, conn, ms)
            if via == 'single':
                got = D.DetectRelocalizationCandidates(bow) if mode == RELOCALIZATION else D.DetectLoopCandidates(bow, conn, ms)
                rep = D.last_report
            else:
                res, reps, words, scores = D.detect_batch([bow], mode, [conn] if conn is not None else None, [ms] if ms is not None else None, want_members=True)
                got = res[0]; rep = reps[0]
                assert int(rep['status']) == 0
                slot_ids = D.slots()
                rw, rs = R.members(mode, [int(i) for i in slot_ids], R.report['min_common_words'])
                assert (words[0] == rw).all(), (what, 'words', words[0], rw)
                assert (bits(scores[0]) == bits(rs)).all(), (what, 'scores', scores[0], rs)
            assert list(map(int, got)) == ref, (what, list(map(int, got)), ref)
            check_report(rep, R.report, what)
            results.append(ref)
        assert D.size() == len(R.kfs), what
    D.close(); voc.close()
    return R, results


def all_generated():
    return [places_script(seed, mode) for seed in range(4) for mode in (RELOCALIZATION, LOOP_CLOSING)]


def reloc_results_with_zeroed_stale(case):
    """the restatement alone, with every mRelocScore zeroed before each query: what the candidates would be if the stale score did not exist"""
    R = kfdb_ref.KeyFrameDatabase(case['nwords']); out = []
    for op in case['ops']:
        if op[0] == 'add': R.add(op[1], op[2])
        elif op[0] == 'cov': R.set_covisibility(op[1], op[2])
        elif op[0] == 'erase': R.erase(op[1])
        elif op[0] == 'clear': R.clear()
        elif op[0] == 'reloc':
            for kf in R.kfs.values(): kf.mRelocScore = F(0)
            out.append(R.DetectRelocalizationCandidates(op[1]))
    return out


def reloc_results(case):
    R = kfdb_ref.KeyFrameDatabase(case['nwords']); out = []
    for op in case['ops']:
        if op[0] == 'add': R.add(op[1], op[2])
        elif op[0] == 'cov': R.set_covisibility(op[1], op[2])
        elif op[0] == 'erase': R.erase(op[1])
        elif op[0] == 'clear': R.clear()
        elif op[0] == 'reloc': out.append(R.DetectRelocalizationCandidates(op[1]))
    return R, out


# ---- batches, min_score, statuses, the device BowVector ------------------------------------------------------------------------------------------------------------
def _load(lib, case, **kw):
    voc = make_voc(lib, case['nwords'])
    adds = [o for o in case['ops'] if o[0] == 'add']
    D = KeyFrameDatabase(voc, max_keyframes=kw.pop('max_keyframes', len(adds)), max_bow_entries=sum(len(o[2][0]) for o in adds), **kw)
    R = kfdb_ref.KeyFrameDatabase(case['nwords'])
    for op in case['ops']:
        if op[0] == 'add': D.add(op[1], op[2]); R.add(op[1], op[2])
        elif op[0] == 'cov': D.set_covisibility(op[1], op[2]); R.set_covisibility(op[1], op[2])
    return voc, D, R


def check_batch_equals_singles(lib, Q, N=65, stream=None):
    """a batch of Q = Q single calls, bit for bit, including the mRelocScore the calls leave behind (read through the members of one more query)"""
    for mode in (RELOCALIZATION, LOOP_CLOSING):
        case = places_script(20 + Q, mode, N=N, nq=Q)
        queries = [o for o in case['ops'] if o[0] in ('reloc', 'loop')][:Q]
        voc1, A, R = _load(lib, case, max_queries=max(Q, 1)); voc2, B, _ = _load(lib, case, max_queries=max(Q, 1))
        bows = [o[1] for o in queries]
        conn = [o[2] for o in queries] if mode == LOOP_CLOSING else None
        ms = [R.min_score(o[1], o[2]) for o in queries] if mode == LOOP_CLOSING else None
        singles = []; reports = []; refs = []
        for q, o in enumerate(queries):
            if mode == RELOCALIZATION: singles.append(A.DetectRelocalizationCandidates(o[1])); refs.append(R.DetectRelocalizationCandidates(o[1]))
            else: singles.append(A.DetectLoopCandidates(o[1], conn[q], ms[q])); refs.append(R.DetectLoopCandidates(o[1], conn[q], ms[q]))
            reports.append(A.last_report); check_report(A.last_report, R.report, (mode, Q, q))
        res, reps = B.detect_batch(bows, mode, conn, ms, stream=stream)
        for q in range(Q):
            assert list(map(int, res[q])) == list(map(int, singles[q])) == refs[q], (mode, Q, q)
            check_report(reps[q], reports[q], (mode, Q, q, 'batch'))
        probe = [bow_of(np.arange(0, case['nwords'] - 20, 7))]              # touches most keyframes: the members it returns are the mRelocScore left behind
        ra = A.detect_batch(probe, RELOCALIZATION, want_members=True); rb = B.detect_batch(probe, RELOCALIZATION, want_members=True, stream=stream)
        R.DetectRelocalizationCandidates(probe[0])
        rw, rs = R.members(RELOCALIZATION, [int(i) for i in A.slots()])
        assert (ra[2] == rb[2]).all() and (ra[2][0] == rw).all()
        assert (bits(ra[3]) == bits(rb[3])).all() and (bits(ra[3][0]) == bits(rs)).all()
        assert list(map(int, ra[0][0])) == list(map(int, rb[0][0]))
        for x in (A, B, voc1, voc2): x.close()


def check_min_score(lib):
    case = places_script(7, RELOCALIZATION, N=40, nq=3)
    voc, D, R = _load(lib, case)
    ids = sorted(R.kfs); rng = np.random.RandomState(3)
    queries = [o[1] for o in case['ops'] if o[0] == 'reloc']
    D.DetectRelocalizationCandidates(queries[0]); R.DetectRelocalizationCandidates(queries[0])
    for b in queries:
        for lst in ([], ids[:1], ids, [int(x) for x in rng.choice(ids, 9)] + [5, 100000], [100000]):
            assert bits(D.min_score(b, lst)) == bits(R.min_score(b, lst)), lst
    assert bits(D.min_score(queries[0], [100000])) == bits(F(1))
    # it is not a query: mRelocScore is as the one relocalisation query left it
    res = D.detect_batch([queries[1]], RELOCALIZATION, want_members=True); R.DetectRelocalizationCandidates(queries[1])
    rw, rs = R.members(RELOCALIZATION, [int(i) for i in D.slots()])
    assert (res[2][0] == rw).all() and (bits(res[3][0]) == bits(rs)).all()
    D.close(); voc.close()


def check_errors(lib):
    import ctypes as C
    from sg_slam_amd.capi import KfdbReport, _vp
    INVALID, UNSUPPORTED, NOMEM = -1, -2, -3
    d = lib.dll
    voc = make_voc(lib, 100)
    h = C.c_void_p()
    assert d.sgx_kfdb_create(voc.h, 4, 100, 4097, 1, C.byref(h)) == UNSUPPORTED
    assert d.sgx_kfdb_create(voc.h, 0, 100, 0, 1, C.byref(h)) == INVALID
    D = KeyFrameDatabase(voc, max_keyframes=3, max_bow_entries=10, max_query_words=8, max_queries=2)
    def add(i, ids, w=None):
        ids = np.asarray(ids, 'i4'); w = np.ones(len(ids)) / max(len(ids), 1) if w is None else np.asarray(w, 'f8')
        return d.sgx_kfdb_add(D.h, i, len(ids), _vp(ids), _vp(w))
    assert add(1, [1, 2, 3]) == 0
    assert add(1, [4, 5]) == INVALID                                       # present
    assert add(2, [3, 2]) == INVALID and add(2, [2, 2]) == INVALID         # not strictly ascending
    assert add(2, [1, 100]) == INVALID and add(2, [-1, 5]) == INVALID      # word id outside the vocabulary
    assert add(2, [1, 2], [0.5, np.inf]) == INVALID and add(2, [1, 2], [np.nan, 0.5]) == INVALID
    assert add(-5, [1, 2]) == INVALID
    assert d.sgx_kfdb_erase(D.h, 7) == INVALID
    assert add(2, [1, 2, 3, 4, 5, 6, 7, 8]) == NOMEM                       # 3 + 8 entries > 10
    assert add(2, [1, 2, 3, 4]) == 0 and add(3, [5, 6, 7]) == 0
    assert add(4, []) == NOMEM                                             # no slot left
    assert D.size() == 3
    assert d.sgx_kfdb_erase(D.h, 2) == 0 and add(4, [1, 2, 3, 4]) == 0     # the erased entries and slot are back
    nb = np.arange(11, dtype='i4')
    assert d.sgx_kfdb_set_covisibility(D.h, 1, 11, _vp(nb)) == INVALID and d.sgx_kfdb_set_covisibility(D.h, 9, 2, _vp(nb)) == INVALID
    assert d.sgx_kfdb_set_covisibility(D.h, 1, 10, _vp(nb)) == 0
    cand = np.zeros(8, 'i4'); n = C.c_int32(); rep = KfdbReport()
    def reloc(ids, w=None):
        ids = np.asarray(ids, 'i4'); w = np.ones(len(ids)) if w is None else np.asarray(w, 'f8')
        return d.sgx_kfdb_detect_relocalization_candidates(D.h, len(ids), _vp(ids), _vp(w), _vp(cand), C.byref(n), C.byref(rep))
    assert reloc(list(range(9))) == INVALID                                # longer than max_query_words
    assert reloc([3, 1]) == INVALID and reloc([1, 200]) == INVALID and reloc([1, 2], [1.0, -np.inf]) == INVALID
    m = C.c_float()
    assert d.sgx_kfdb_min_score(D.h, 9, _vp(np.arange(9, dtype='i4')), _vp(np.ones(9)), 1, _vp(nb), C.byref(m)) == INVALID
    assert reloc(list(range(8))) == 0 and n.value > 0
    assert reloc([]) == 0 and n.value == 0 and bytes(rep) == bytes(36)     # an empty query: no candidates, a zero report
    # in a batch a query that is too long is reported in its own record and leaves the others alone
    with_long = [bow_of(range(8)), bow_of(range(20)), bow_of([1, 2, 3])]
    try:
        D.detect_batch(with_long); assert False, 'a batch larger than max_queries must be refused'
    except Exception as e:
        assert 'invalid' in str(e).lower() or '-1' in str(e)
    res, reps = D.detect_batch(with_long[:2])
    assert reps[0]['status'] == 0 and len(res[0]) > 0 and reps[1]['status'] == INVALID and len(res[1]) == 0 and reps[1]['n_sharing'] == 0
    D.clear()
    assert D.size() == 0 and reloc([1, 2, 3]) == 0 and n.value == 0 and bytes(rep) == bytes(36)      # an empty database
    res, reps = D.detect_batch([bow_of([1, 2, 3])], LOOP_CLOSING, [[1]], [0.0])
    assert len(res[0]) == 0 and reps[0].tobytes() == bytes(36)
    D.close(); voc.close()


def check_clear_forgets_reloc_scores(lib):
    case = [c for c in hand_cases() if c['name'] == 'stale-changes-result'][0]
    ops = case['ops']
    replay = dict(name='clear-forgets', nwords=200, ops=ops[:5] + [('clear',)] + ops[:4] + [ops[5]])
    _, results = run_script(lib, replay)
    assert results == [[2], [1]]                                           # after clear() the stale score of keyframe 2 is gone


def check_bow_batch(lib, sizes=(0, 1, 63, 64, 65, 500), cap=None, vocs=None,
                    combos=((0, 0), (0, 1), (0, 2), (0, 3), (1, 0), (1, 2), (3, 1), (5, 0), (5, 3))):
    """sgx_voc_transform_batch_dev -> sgx_voc_bow_batch_dev against sgx_voc_transform frame by frame, bit for bit"""
    import voc_cases as vc
    on_host = 'EMULATOR' in lib.version()
    if on_host: dev = lambda a: np.ascontiguousarray(a).copy(); host = lambda a: a
    else:
        import torch
        dev = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda(); host = lambda a: a.cpu().numpy()
    cap = cap or max(max(sizes), 1)
    B = len(sizes) + 1
    vocs = vocs or [vc.make_vocabulary(100, k=10, L=3), vc.make_vocabulary(101, k=6, L=4)]
    merged = 0
    for vi, voc in enumerate(vocs + [vc.make_vocabulary(102, k=5, L=2, stop=1.0)]):            # the last one: every word stopped
        for scoring, weighting in combos:                                  # (scoring, weighting): L1 / L2 / KL normalise, DOT_PRODUCT divides by nd; TF_IDF, TF, IDF, BINARY
            V = ORBVocabulary(lib).create(voc['k'], voc['L'], voc['parent'], voc['desc'], voc['weight'], voc['is_leaf'], scoring, weighting)
            desc = np.zeros((B, cap, 32), np.uint8); n = np.zeros(B, 'i4')
            for b, sz in enumerate(sizes):
                desc[b, :sz] = vc.make_features(voc, 31 * vi + b, max(sz, 1))[:sz]; n[b] = sz
            one = vc.make_features(voc, 99, 1)[0]                          # the last frame: every feature the same descriptor, so all land in one word
            n[B - 1] = min(cap, 37); desc[B - 1, :n[B - 1]] = one
            d_n = dev(n); d_word = dev(np.zeros((B, cap), 'i4')); d_w = dev(np.zeros((B, cap), 'f8')); d_node = dev(np.zeros((B, cap), 'i4'))
            V.transform_batch_dev(dev(desc), cap * 32, d_n, B, cap, d_word, d_w, d_node)
            d_ids = dev(np.full((B, cap), -7, 'i4')); d_bw = dev(np.zeros((B, cap), 'f8')); d_nb = dev(np.full(B, -7, 'i4'))
            V.bow_batch_dev(d_n, B, cap, d_word, d_w, d_ids, d_bw, d_nb)
            ids, bw, nb = host(d_ids), host(d_bw), host(d_nb)
            for b in range(B):
                ei, ew, _, eword = V.transform(desc[b, :n[b]])
                what = (vi, scoring, weighting, b, int(n[b]))
                assert nb[b] == len(ei), what
                assert (ids[b, :nb[b]] == ei).all(), what
                assert (bw[b, :nb[b]].view('u8') == ew.view('u8')).all(), what
                merged += int(n[b]) - len(ei)
            if vi == len(vocs): assert (nb == 0).all()
            elif n[B - 1] > 0: assert nb[B - 1] <= 1
            V.close()
    assert merged > 0                                                      # words with several features occurred


def check_chain(lib, n_kf=24, Q=5, stream=None):
    """device transform -> bow_batch_dev -> detect_batch_dev (nothing leaves the device between them) equals host transform -> single queries"""
    import voc_cases as vc
    on_host = 'EMULATOR' in lib.version()
    if on_host: dev = lambda a: np.ascontiguousarray(a).copy()
    else:
        import torch
        dev = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()
    voc = vc.make_vocabulary(100, k=10, L=3)
    V = ORBVocabulary(lib).create(voc['k'], voc['L'], voc['parent'], voc['desc'], voc['weight'], voc['is_leaf'])
    A = KeyFrameDatabase(V, max_keyframes=n_kf, max_bow_entries=n_kf * 400, max_queries=Q); B = KeyFrameDatabase(V, max_keyframes=n_kf, max_bow_entries=n_kf * 400, max_queries=Q)
    R = kfdb_ref.KeyFrameDatabase(V.nwords)
    rng = np.random.RandomState(4)
    frames = [vc.make_features(voc, 200 + i // 3, 300)[rng.permutation(300)[:rng.randint(150, 300)]] for i in range(n_kf)]      # three keyframes per "place"
    for i, f in enumerate(frames):
        b = V.transform(f)[:2]
        A.add(i, b); B.add(i, b); R.add(i, b)
    for i in range(n_kf):
        nb = [j for j in range(max(0, i - 3), min(n_kf, i + 4)) if j != i]
        A.set_covisibility(i, nb); B.set_covisibility(i, nb); R.set_covisibility(i, nb)
    cap = 300
    qf = [vc.make_features(voc, 200 + q, 300)[rng.permutation(300)[:rng.randint(100, 300)]] for q in range(Q)]
    desc = np.zeros((Q, cap, 32), np.uint8); n = np.zeros(Q, 'i4')
    for q, f in enumerate(qf): desc[q, :len(f)] = f; n[q] = len(f)
    d_n = dev(n); d_word = dev(np.zeros((Q, cap), 'i4')); d_w = dev(np.zeros((Q, cap), 'f8')); d_node = dev(np.zeros((Q, cap), 'i4'))
    d_ids = dev(np.zeros((Q, cap), 'i4')); d_bw = dev(np.zeros((Q, cap), 'f8')); d_nb = dev(np.zeros(Q, 'i4'))
    s = None
    if stream is not None: s = stream.cuda_stream
    V.transform_batch_dev(dev(desc), cap * 32, d_n, Q, cap, d_word, d_w, d_node, stream=s)
    V.bow_batch_dev(d_n, Q, cap, d_word, d_w, d_ids, d_bw, d_nb, stream=s)
    cand, ncand, rep, _, _ = A.detect_batch_dev(RELOCALIZATION, Q, d_ids, d_bw, cap, d_nb, stream=stream)
    if stream is not None: stream.synchronize()
    elif not on_host:
        import torch
        torch.cuda.current_stream().synchronize()
    cand, ncand, rep = A._host(cand), A._host(ncand), A._host(rep).view(A_REPORT)
    total = 0
    for q in range(Q):
        b = V.transform(qf[q])[:2]
        got = B.DetectRelocalizationCandidates(b); ref = R.DetectRelocalizationCandidates(b)
        assert list(map(int, cand[q, :ncand[q]])) == list(map(int, got)) == ref, q
        check_report(rep[q], B.last_report, q); check_report(rep[q], R.report, q)
        total += len(ref)
    assert total >= Q
    for x in (A, B, V): x.close()


from sg_slam_amd.capi import KFDB_REPORT_DTYPE as A_REPORT


def shapes_script(N, mode, lengths=(1, 63, 64, 65, 129), max_len=256, nwords=700, seed=0):
    """the smallest shapes at which the kernels can go wrong: N keyframes around the tile (16) and wave (64) sizes, BowVector lengths around the 64-entry chunk, and one
    vector of max_query_words words as a keyframe and as a query; the words are few, so that most pairs share some"""
    rng = np.random.RandomState(1000 * N + seed)
    L = list(lengths) + [max_len]
    draw = lambda n: bow_of(rng.choice(nwords, n, replace=False), rng=rng)
    ops = [('add', 2 * i + 1, draw(L[i % len(L)])) for i in range(N)]
    for i in range(N):
        nb = [2 * j + 1 for j in range(max(0, i - 6), min(N, i + 7)) if j != i]; rng.shuffle(nb)
        ops.append(('cov', 2 * i + 1, nb[:10]))
    for n in L:
        b = draw(n)
        ops.append(('reloc', b) if mode == RELOCALIZATION else ('loop', b, [2 * j + 1 for j in range(0, N, 5)], None))
    return dict(name=f'shapes-{N}-{mode}', nwords=nwords, ops=ops)


def check_large(lib, N=2048, Q=64, nwords=100000, modes=(RELOCALIZATION, LOOP_CLOSING), stream=None):
    """one larger case: N keyframes of about 600 words, Q queries in one batch; the expected values come from the restatement, query after query"""
    for mode in modes:
        case = places_script(77, mode, N=N, nwords=nwords, places=64, per_place=1500, nq=Q - 1, lo=550, hi=650)
        voc, D, R = _load(lib, case, max_queries=Q, max_query_words=1024)
        queries = [o for o in case['ops'] if o[0] in ('reloc', 'loop')]
        assert len(queries) == Q
        bows = [o[1] for o in queries]
        conn = [o[2] for o in queries] if mode == LOOP_CLOSING else None
        ms = [o[3] if o[3] is not None else R.min_score(o[1], o[2]) for o in queries] if mode == LOOP_CLOSING else None
        res, reps, words, scores = D.detect_batch(bows, mode, conn, ms, want_members=True, stream=stream)
        ids = [int(i) for i in D.slots()]
        total = 0
        for q in range(Q):
            ref = R.DetectRelocalizationCandidates(bows[q]) if mode == RELOCALIZATION else R.DetectLoopCandidates(bows[q], conn[q], ms[q])
            assert list(map(int, res[q])) == ref, (mode, q)
            check_report(reps[q], R.report, (mode, q))
            rw, rs = R.members(mode, ids, R.report['min_common_words'])
            assert (words[q] == rw).all() and (bits(scores[q]) == bits(rs)).all(), (mode, q)
            total += len(ref)
        assert total >= Q - 1
        D.close(); voc.close()
