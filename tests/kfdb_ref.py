"""KeyFrameDatabase.cc restated in plain Python, as written: a real inverted file of per-word lists, keyframe objects with their mutable query fields, the same loops
in the same order, np.float32 wherever the reference has a float.  The scoring is the merge loop of L1Scoring::score (ScoringObject.cpp:23-67).  This is the yardstick
of the device database; it deliberately knows nothing of the (first common word, add sequence) formulation the kernels use."""
import numpy as np

F = np.float32


def l1_score(v1, v2):
    """L1Scoring::score on two BowVectors (ids ascending, weights), the merge loop with its lower_bound skips"""
    i1, w1 = v1; i2, w2 = v2
    a = b = 0; n1 = len(i1); n2 = len(i2)
    score = 0.0
    while a < n1 and b < n2:
        if i1[a] == i2[b]:
            vi = float(w1[a]); wi = float(w2[b])
            score += abs(vi - wi) - abs(vi) - abs(wi)
            a += 1; b += 1
        elif i1[a] < i2[b]:
            a = int(np.searchsorted(i1, i2[b], 'left'))
        else:
            b = int(np.searchsorted(i2, i1[a], 'left'))
    return -score / 2.0


class KeyFrame:
    def __init__(self, mnId, bow):
        self.mnId = mnId
        self.mBowVec = (np.asarray(bow[0], 'i4'), np.asarray(bow[1], 'f8'))
        self.neighbours = []                    # GetBestCovisibilityKeyFrames(10), ids
        self.mnLoopQuery = 0; self.mnLoopWords = 0; self.mLoopScore = F(0)
        self.mnRelocQuery = 0; self.mnRelocWords = 0
        self.mRelocScore = F(0)                 # defined: 0 until a query scores the keyframe (the reference leaves it uninitialised)


class Report(dict):
    __getattr__ = dict.__getitem__


def _report():
    return Report(n_sharing=0, max_common_words=0, min_common_words=0, n_scores=0, n_score_and_match=0, best_acc_score=F(0), min_score_to_retain=F(0), n_candidates=0)


class KeyFrameDatabase:
    def __init__(self, nwords):
        self.nwords = nwords
        self.mvInvertedFile = {}                # word -> list of keyframes in add() order (a dict of the non-empty lists of the reference's vector)
        self.kfs = {}                           # the map's keyframes by id (the reference holds pointers)
        self.next_query = 1                     # a query's mnId: fresh and nonzero
        self.events = dict(best_is_neighbour=0, dedup=0, stale_nonzero=0)

    def add(self, mnId, bow):
        kf = KeyFrame(mnId, bow)
        self.kfs[mnId] = kf
        for w in kf.mBowVec[0]:
            self.mvInvertedFile.setdefault(int(w), []).append(kf)
        return kf

    def erase(self, mnId):
        kf = self.kfs.pop(mnId)
        for w in kf.mBowVec[0]:
            lKFs = self.mvInvertedFile[int(w)]
            for k, x in enumerate(lKFs):
                if x is kf:
                    del lKFs[k]
                    break

    def clear(self):
        self.mvInvertedFile = {}; self.kfs = {}

    def set_covisibility(self, mnId, ids):
        self.kfs[mnId].neighbours = list(ids)

    def _neighbours(self, kf):
        return [self.kfs[i] for i in kf.neighbours if i in self.kfs]      # a keyframe that is not in the database is never touched by the query

    def DetectLoopCandidates(self, bow, connected, minScore):
        minScore = F(minScore)
        qid = self.next_query; self.next_query += 1
        R = _report(); self.report = R
        spConnected = set(connected)
        lKFsSharingWords = []
        for w in bow[0]:
            for pKFi in self.mvInvertedFile.get(int(w), []):
                if pKFi.mnLoopQuery != qid:
                    pKFi.mnLoopWords = 0
                    if pKFi.mnId not in spConnected:
                        pKFi.mnLoopQuery = qid
                        lKFsSharingWords.append(pKFi)
                pKFi.mnLoopWords += 1
                pKFi.loop_touch = qid           # instrument (not in the reference): which query last wrote mnLoopWords
        R['n_sharing'] = len(lKFsSharingWords)
        if not lKFsSharingWords:
            return []
        maxCommonWords = 0
        for kf in lKFsSharingWords:
            if kf.mnLoopWords > maxCommonWords: maxCommonWords = kf.mnLoopWords
        minCommonWords = int(F(maxCommonWords) * F(0.8))
        R['max_common_words'] = maxCommonWords; R['min_common_words'] = minCommonWords
        lScoreAndMatch = []; nscores = 0
        for pKFi in lKFsSharingWords:
            if pKFi.mnLoopWords > minCommonWords:
                nscores += 1
                si = F(l1_score(bow, pKFi.mBowVec))
                pKFi.mLoopScore = si
                if si >= minScore: lScoreAndMatch.append((si, pKFi))
        R['n_scores'] = nscores; R['n_score_and_match'] = len(lScoreAndMatch)
        if not lScoreAndMatch:
            return []
        lAcc = []; bestAccScore = minScore
        for si, pKFi in lScoreAndMatch:
            bestScore = si; accScore = si; pBestKF = pKFi
            for pKF2 in self._neighbours(pKFi):
                if pKF2.mnLoopQuery == qid and pKF2.mnLoopWords > minCommonWords:
                    accScore = F(accScore + pKF2.mLoopScore)
                    if pKF2.mLoopScore > bestScore:
                        pBestKF = pKF2; bestScore = pKF2.mLoopScore
            lAcc.append((accScore, pBestKF))
            if pBestKF is not pKFi: self.events['best_is_neighbour'] += 1
            if accScore > bestAccScore: bestAccScore = accScore
        return self._retain(lAcc, bestAccScore, R)

    def DetectRelocalizationCandidates(self, bow):
        qid = self.next_query; self.next_query += 1
        R = _report(); self.report = R
        lKFsSharingWords = []
        for w in bow[0]:
            for pKFi in self.mvInvertedFile.get(int(w), []):
                if pKFi.mnRelocQuery != qid:
                    pKFi.mnRelocWords = 0
                    pKFi.mnRelocQuery = qid
                    lKFsSharingWords.append(pKFi)
                pKFi.mnRelocWords += 1
        R['n_sharing'] = len(lKFsSharingWords)
        if not lKFsSharingWords:
            return []
        maxCommonWords = 0
        for kf in lKFsSharingWords:
            if kf.mnRelocWords > maxCommonWords: maxCommonWords = kf.mnRelocWords
        minCommonWords = int(F(maxCommonWords) * F(0.8))
        R['max_common_words'] = maxCommonWords; R['min_common_words'] = minCommonWords
        lScoreAndMatch = []; nscores = 0
        for pKFi in lKFsSharingWords:
            if pKFi.mnRelocWords > minCommonWords:
                nscores += 1
                si = F(l1_score(bow, pKFi.mBowVec))
                pKFi.mRelocScore = si
                pKFi.scored_by = qid
                lScoreAndMatch.append((si, pKFi))
        R['n_scores'] = nscores; R['n_score_and_match'] = len(lScoreAndMatch)
        if not lScoreAndMatch:
            return []
        lAcc = []; bestAccScore = F(0)
        for si, pKFi in lScoreAndMatch:
            bestScore = si; accScore = bestScore; pBestKF = pKFi
            for pKF2 in self._neighbours(pKFi):
                if pKF2.mnRelocQuery != qid:
                    continue
                if getattr(pKF2, 'scored_by', 0) != qid and pKF2.mRelocScore != 0: self.events['stale_nonzero'] += 1
                accScore = F(accScore + pKF2.mRelocScore)
                if pKF2.mRelocScore > bestScore:
                    pBestKF = pKF2; bestScore = pKF2.mRelocScore
            lAcc.append((accScore, pBestKF))
            if pBestKF is not pKFi: self.events['best_is_neighbour'] += 1
            if accScore > bestAccScore: bestAccScore = accScore
        return self._retain(lAcc, bestAccScore, R)

    def _retain(self, lAcc, bestAccScore, R):
        minScoreToRetain = F(F(0.75) * bestAccScore)
        R['best_acc_score'] = bestAccScore; R['min_score_to_retain'] = minScoreToRetain
        added = set(); out = []
        for acc, pKFi in lAcc:
            if acc > minScoreToRetain:
                if pKFi.mnId not in added:
                    out.append(pKFi.mnId); added.add(pKFi.mnId)
                else:
                    self.events['dedup'] += 1
        R['n_candidates'] = len(out)
        return out

    def min_score(self, bow, kf_ids):
        """LoopClosing.cc:126-138 over the listed keyframes that are in the database"""
        m = F(1)
        for i in kf_ids:
            if i not in self.kfs: continue
            s = F(l1_score(bow, self.kfs[i].mBowVec))
            if s < m: m = s
        return m

    # what the reference leaves in the keyframes' public members, as the device reports it for a query (by keyframe id)
    def members(self, mode, ids, minCommonWords=None):
        qid = self.next_query - 1
        words = []; scores = []
        for i in ids:
            kf = self.kfs.get(i)
            if kf is None: words.append(0); scores.append(F(0)); continue
            if mode == 0:
                words.append(kf.mnRelocWords if kf.mnRelocQuery == qid else 0); scores.append(kf.mRelocScore)
            else:
                touched = kf.mnLoopQuery == qid or getattr(kf, 'loop_touch', 0) == qid
                words.append(kf.mnLoopWords if touched else 0)
                scores.append(kf.mLoopScore if (kf.mnLoopQuery == qid and kf.mnLoopWords > minCommonWords) else F(0))
        return np.array(words, 'i4'), np.array(scores, 'f4')
