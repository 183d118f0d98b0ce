"""Literal restatement of the covisibility graph of the reference, in plain Python objects, dicts and lists: KeyFrame.cc:124-158 (AddConnection, UpdateBestCovisibles),
:251-276 (TrackedMapPoints), :290-380 (UpdateConnections), :454-568 (SetBadFlag, EraseConnection), MapPoint.cc:98-215 (AddObservation, EraseObservation, SetBadFlag,
Replace), Tracking.cc:1324-1458 (UpdateLocalPoints, UpdateLocalKeyFrames) and LocalMapping.cc:632-696 (KeyFrameCulling).

Where the reference's order is that of pointers (map<KeyFrame*, ...>, set<KeyFrame*>, sort of pair<int, KeyFrame*>) the order here is that of mnId.  A point exists while
it has an observation: Map.point() makes a fresh object for an id that has none."""
import numpy as np

F = np.float32


def by_id(d):
    """a map<KeyFrame*, T> or set<KeyFrame*> in iteration order"""
    if isinstance(d, dict):
        return sorted(d.items(), key=lambda kv: kv[0].mnId)
    return sorted(d, key=lambda k: k.mnId)


class KeyFrame:
    def __init__(self, mnId, octave, uright, depth, thDepth):
        self.mnId = mnId; self.N = len(octave)
        self.octave = [int(o) for o in octave]; self.mvuRight = [F(u) for u in uright]; self.mvDepth = [F(d) for d in depth]; self.mThDepth = F(thDepth)
        self.mvpMapPoints = [None] * self.N
        self.mConnectedKeyFrameWeights = {}
        self.mvpOrderedConnectedKeyFrames = []; self.mvOrderedWeights = []
        self.mbFirstConnection = True; self.mpParent = None; self.mspChildrens = set()
        self.mbBad = False; self.mnTrackReferenceForFrame = 0

    def isBad(self):
        return self.mbBad

    def AddConnection(self, pKF, weight):
        if pKF not in self.mConnectedKeyFrameWeights: self.mConnectedKeyFrameWeights[pKF] = weight
        elif self.mConnectedKeyFrameWeights[pKF] != weight: self.mConnectedKeyFrameWeights[pKF] = weight
        else: return
        self.UpdateBestCovisibles()

    def UpdateBestCovisibles(self):
        vPairs = [(w, k) for k, w in by_id(self.mConnectedKeyFrameWeights)]
        vPairs.sort(key=lambda p: (p[0], p[1].mnId))
        lKFs = []; lWs = []
        for w, k in vPairs:
            lKFs.insert(0, k); lWs.insert(0, w)
        self.mvpOrderedConnectedKeyFrames = lKFs; self.mvOrderedWeights = lWs

    def GetBestCovisibilityKeyFrames(self, N):
        return list(self.mvpOrderedConnectedKeyFrames[:N])

    def GetWeight(self, pKF):
        return self.mConnectedKeyFrameWeights.get(pKF, 0)

    def TrackedMapPoints(self, minObs):
        nPoints = 0; bCheckObs = minObs > 0
        for i in range(self.N):
            pMP = self.mvpMapPoints[i]
            if pMP:
                if not pMP.isBad():
                    if bCheckObs:
                        if pMP.Observations() >= minObs: nPoints += 1
                    else: nPoints += 1
        return nPoints

    def UpdateConnections(self):
        """returns the report of the call: (KFcounter.size(), nmax, pKFmax id, ordered size)"""
        KFcounter = {}
        for pMP in list(self.mvpMapPoints):
            if not pMP: continue
            if pMP.isBad(): continue
            for k, _ in by_id(pMP.mObservations):
                if k.mnId == self.mnId: continue
                KFcounter[k] = KFcounter.get(k, 0) + 1
        if not KFcounter:
            return (0, 0, -1, 0)
        nmax = 0; pKFmax = None; th = 15
        vPairs = []
        for k, c in by_id(KFcounter):
            if c > nmax: nmax = c; pKFmax = k
            if c >= th:
                vPairs.append((c, k)); k.AddConnection(self, c)
        if not vPairs:
            vPairs.append((nmax, pKFmax)); pKFmax.AddConnection(self, nmax)
        vPairs.sort(key=lambda p: (p[0], p[1].mnId))
        lKFs = []; lWs = []
        for w, k in vPairs:
            lKFs.insert(0, k); lWs.insert(0, w)
        self.mConnectedKeyFrameWeights = dict(KFcounter)
        self.mvpOrderedConnectedKeyFrames = lKFs; self.mvOrderedWeights = lWs
        if self.mbFirstConnection and self.mnId != 0:
            self.mpParent = self.mvpOrderedConnectedKeyFrames[0]
            self.mpParent.mspChildrens.add(self)
            self.mbFirstConnection = False
        return (len(KFcounter), nmax, pKFmax.mnId, len(lKFs))

    def ChangeParent(self, pKF):
        self.mpParent = pKF
        if pKF is not None: pKF.mspChildrens.add(self)

    def EraseConnection(self, pKF):
        if pKF in self.mConnectedKeyFrameWeights:
            del self.mConnectedKeyFrameWeights[pKF]
            self.UpdateBestCovisibles()

    def SetBadFlag(self):
        """past the mbNotErase gate (:467-541)"""
        if self.mnId == 0: return
        for k, _ in by_id(self.mConnectedKeyFrameWeights): k.EraseConnection(self)
        for i in range(len(self.mvpMapPoints)):
            if self.mvpMapPoints[i]: self.mvpMapPoints[i].EraseObservation(self)
        self.mConnectedKeyFrameWeights = {}; self.mvpOrderedConnectedKeyFrames = []; self.mvOrderedWeights = []
        sParentCandidates = {self.mpParent}
        while self.mspChildrens:
            bContinue = False; mx = -1; pC = pP = None
            for pKF in by_id(self.mspChildrens):
                if pKF.isBad(): continue
                for vc in pKF.mvpOrderedConnectedKeyFrames:
                    for cand in sParentCandidates:
                        if cand is not None and vc.mnId == cand.mnId:
                            w = pKF.GetWeight(vc)
                            if w > mx: pC = pKF; pP = vc; mx = w; bContinue = True
            if bContinue:
                pC.ChangeParent(pP); sParentCandidates.add(pC); self.mspChildrens.discard(pC)
            else: break
        for pKF in by_id(self.mspChildrens): pKF.ChangeParent(self.mpParent)      # without a parent (the reference would dereference NULL) they are left without one
        self.mspChildrens = set()
        if self.mpParent is not None: self.mpParent.mspChildrens.discard(self)
        self.mbBad = True
        self.mvpMapPoints = [None] * self.N                                        # deviation 4: an erased keyframe contributes nothing


class MapPoint:
    def __init__(self, mnId, mp):
        self.mnId = mnId; self.map = mp; self.mObservations = {}; self.nObs = 0; self.mbBad = False; self.mnTrackReferenceForFrame = 0

    def isBad(self): return self.mbBad
    def Observations(self): return self.nObs
    def IsInKeyFrame(self, pKF): return pKF in self.mObservations

    def AddObservation(self, pKF, idx):
        if pKF in self.mObservations: return
        self.mObservations[pKF] = idx
        if pKF.mvuRight[idx] >= 0: self.nObs += 2
        else: self.nObs += 1

    def EraseObservation(self, pKF):
        bBad = False
        if pKF in self.mObservations:
            idx = self.mObservations[pKF]
            if pKF.mvuRight[idx] >= 0: self.nObs -= 2
            else: self.nObs -= 1
            del self.mObservations[pKF]
            if self.nObs <= 2: bBad = True
        if bBad: self.SetBadFlag()

    def SetBadFlag(self):
        self.mbBad = True
        obs = self.mObservations; self.mObservations = {}
        for k, idx in by_id(obs): k.mvpMapPoints[idx] = None
        self.map.points.pop(self.mnId, None)

    def Replace(self, pMP):
        if pMP.mnId == self.mnId: return
        obs = self.mObservations; self.mObservations = {}; self.mbBad = True
        for k, idx in by_id(obs):
            if not pMP.IsInKeyFrame(k):
                k.mvpMapPoints[idx] = pMP; pMP.AddObservation(k, idx)
            else:
                k.mvpMapPoints[idx] = None
        self.map.points.pop(self.mnId, None)


class Invalid(Exception):
    pass


class Map:
    """the mutations and queries of the handle, on the objects above; ids as the handle takes them"""
    def __init__(self, monocular=False, th_depth=40.0, max_points=1 << 30):
        self.kfs = {}; self.all_kfs = {}; self.points = {}; self.mbMonocular = bool(monocular); self.th_depth = th_depth; self.max_points = max_points; self.frame_id = 0

    def point(self, pid):
        if pid not in self.points: self.points[pid] = MapPoint(pid, self)
        return self.points[pid]

    def add_keyframe(self, kf_id, octave, uright, depth):
        if kf_id < 0 or kf_id in self.all_kfs: raise Invalid()
        self.kfs[kf_id] = self.all_kfs[kf_id] = KeyFrame(kf_id, octave, uright, depth, self.th_depth)

    def _check(self, kf_id, idx, pts):
        """deviation 2: one relation.  Played on a copy of what the call touches, so that a refused call changes nothing."""
        if kf_id not in self.kfs: raise Invalid()
        k = self.kfs[kf_id]
        for i, p in zip(idx, pts):
            if i < 0 or i >= k.N or p < -1 or p >= self.max_points: raise Invalid()

    def set_observations(self, kf_id, idx, pts, may_fail=False):
        """may_fail: keep a copy of the map to go back to (the scripts that feed refused calls set it; copying the map for every call of a long script is slow)"""
        import copy
        self._check(kf_id, idx, pts)
        saved = copy.deepcopy((self.kfs, self.all_kfs, self.points)) if may_fail else None
        try:
            k = self.kfs[kf_id]
            for i, p in zip(idx, pts):
                cur = k.mvpMapPoints[i]
                if p < 0:
                    if cur is not None:
                        k.mvpMapPoints[i] = None; cur.EraseObservation(k)
                elif cur is None or cur.mnId != p:
                    if cur is not None or (p in self.points and self.points[p].IsInKeyFrame(k)): raise Invalid()
                    pMP = self.point(p); k.mvpMapPoints[i] = pMP; pMP.AddObservation(k, i)
        except Invalid:
            assert saved is not None, 'a refused call in a script that did not announce one'
            self.kfs, self.all_kfs, self.points = saved
            for pm in self.points.values(): pm.map = self
            raise

    def set_points_bad(self, ids):
        for p in ids:
            if p < 0 or p >= self.max_points: raise Invalid()
        for p in ids:
            if p in self.points: self.points[p].SetBadFlag()

    def replace_point(self, old, new):
        if old == new or old not in self.points: return
        self.points[old].Replace(self.point(new))
        if not self.points[new].mObservations: del self.points[new]

    def erase_keyframe(self, kf_id):
        if kf_id not in self.kfs: raise Invalid()
        if kf_id == 0: return
        self.kfs[kf_id].SetBadFlag(); del self.kfs[kf_id]

    # ---- state as the getters give it
    def weights(self, kf_id):
        kv = by_id(self.kfs[kf_id].mConnectedKeyFrameWeights)
        return [k.mnId for k, _ in kv], [w for _, w in kv]

    def ordered(self, kf_id):
        k = self.kfs[kf_id]
        return [x.mnId for x in k.mvpOrderedConnectedKeyFrames], list(k.mvOrderedWeights)

    def best_covisibles(self, kf_id, N=10):
        return [x.mnId for x in self.kfs[kf_id].GetBestCovisibilityKeyFrames(N)]

    def tree(self, kf_id):
        k = self.kfs[kf_id]
        return (k.mpParent.mnId if k.mpParent is not None else -1), k.mbFirstConnection, [c.mnId for c in by_id(k.mspChildrens)]

    def observations(self, pid):
        if pid not in self.points: return [], 0
        p = self.points[pid]
        return [(k.mnId, i) for k, i in by_id(p.mObservations)], p.nObs

    def keyframe_points(self, kf_id):
        return [p.mnId if p is not None else -1 for p in self.kfs[kf_id].mvpMapPoints]

    # ---- the queries
    def update_connections(self, kf_id):
        """(status, n_counter, max_weight, max_kf, n_ordered, parent)"""
        if kf_id not in self.kfs: return (-1, 0, 0, -1, 0, -1)
        k = self.kfs[kf_id]
        n, nmax, idmax, nord = k.UpdateConnections()
        return (0, n, nmax, idmax, nord, k.mpParent.mnId if k.mpParent is not None else -1)

    def local_map(self, frame, min_obs, local_kf, ref_kf, mcap):
        """Tracking::UpdateLocalMap.  frame: point ids (-1 none); local_kf: ids of mvpLocalKeyFrames going in; ref_kf: id of mpReferenceKF or -1.  Returns a dict as
        CovisibilityGraph.local_map does, or None for a malformed frame."""
        for p in frame:
            if p < -1 or p >= self.max_points: return None
        self.frame_id += 1; fid = self.frame_id                                  # deviation 3: a fresh nonzero mnId
        mvpMapPoints = [self.points.get(p) if p >= 0 else None for p in frame]   # an id without observations is a bad point
        bad = object()
        mvpMapPoints = [bad if (p >= 0 and m is None) else m for p, m in zip(frame, mvpMapPoints)]
        mvpLocalKeyFrames = [self.all_kfs.get(i) for i in local_kf]              # None: an id that never was a keyframe (contributes nothing)
        mpReferenceKF = self.all_kfs.get(ref_kf)
        # UpdateLocalKeyFrames
        keyframeCounter = {}
        for i in range(len(mvpMapPoints)):
            if mvpMapPoints[i] is not None:
                pMP = mvpMapPoints[i]
                if pMP is not bad and not pMP.isBad():
                    for k, _ in by_id(pMP.mObservations): keyframeCounter[k] = keyframeCounter.get(k, 0) + 1
                else:
                    mvpMapPoints[i] = None
        n_stage1 = 0; mx = 0; pKFmax = None
        if keyframeCounter:
            mvpLocalKeyFrames = []
            for pKF, c in by_id(keyframeCounter):
                if pKF.isBad(): continue
                if c > mx: mx = c; pKFmax = pKF
                mvpLocalKeyFrames.append(pKF); pKF.mnTrackReferenceForFrame = fid
            n_stage1 = len(mvpLocalKeyFrames)
            for pKF in list(mvpLocalKeyFrames):
                if len(mvpLocalKeyFrames) > 80: break
                for pNeighKF in pKF.GetBestCovisibilityKeyFrames(10):
                    if not pNeighKF.isBad():
                        if pNeighKF.mnTrackReferenceForFrame != fid:
                            mvpLocalKeyFrames.append(pNeighKF); pNeighKF.mnTrackReferenceForFrame = fid
                            break
                for pChildKF in by_id(pKF.mspChildrens):
                    if not pChildKF.isBad():
                        if pChildKF.mnTrackReferenceForFrame != fid:
                            mvpLocalKeyFrames.append(pChildKF); pChildKF.mnTrackReferenceForFrame = fid
                            break
                pParent = pKF.mpParent
                if pParent:
                    if pParent.mnTrackReferenceForFrame != fid:
                        mvpLocalKeyFrames.append(pParent); pParent.mnTrackReferenceForFrame = fid
                        break
            if pKFmax: mpReferenceKF = pKFmax
        # UpdateLocalPoints
        mvpLocalMapPoints = []
        for pKF in mvpLocalKeyFrames:
            if pKF is None or pKF.isBad(): continue                              # deviation 4
            for pMP in pKF.mvpMapPoints:
                if not pMP: continue
                if pMP.mnTrackReferenceForFrame == fid: continue
                if not pMP.isBad():
                    mvpLocalMapPoints.append(pMP); pMP.mnTrackReferenceForFrame = fid
        tracked = mpReferenceKF.TrackedMapPoints(min_obs) if (mpReferenceKF is not None and not mpReferenceKF.isBad()) else 0
        n = len(mvpLocalMapPoints)
        return dict(frame=[m.mnId if m is not None else -1 for m in mvpMapPoints],
                    local_kf=[k.mnId for k in mvpLocalKeyFrames] if keyframeCounter else list(local_kf),
                    ref_kf=mpReferenceKF.mnId if (keyframeCounter and pKFmax) else ref_kf, ref_tracked=tracked,
                    points=[m.mnId for m in mvpLocalMapPoints[:mcap]], obs=[m.nObs for m in mvpLocalMapPoints[:mcap]], n_points=n,
                    status=-3 if n > mcap else 0, n_counter=len(keyframeCounter), max_weight=mx, max_kf=pKFmax.mnId if pKFmax else -1, n_stage1=n_stage1,
                    n_local_kf=len(mvpLocalKeyFrames))

    def _candidate_counts(self, pKF):
        nObs = 3; thObs = nObs; nRedundantObservations = 0; nMPs = 0
        for i in range(len(pKF.mvpMapPoints)):
            pMP = pKF.mvpMapPoints[i]
            if pMP:
                if not pMP.isBad():
                    if not self.mbMonocular:
                        if pKF.mvDepth[i] > pKF.mThDepth or pKF.mvDepth[i] < 0: continue
                    nMPs += 1
                    if pMP.Observations() > thObs:
                        scaleLevel = pKF.octave[i]
                        nObs = 0
                        for pKFi, idx in by_id(pMP.mObservations):
                            if pKFi is pKF: continue
                            if pKFi.octave[idx] <= scaleLevel + 1:
                                nObs += 1
                                if nObs >= thObs: break
                        if nObs >= thObs: nRedundantObservations += 1
        return nRedundantObservations, nMPs

    def KeyFrameCulling(self, cur_id):
        """the literal loop, SetBadFlag between the candidates included; returns the ids it erased"""
        erased = []
        for pKF in list(self.kfs[cur_id].mvpOrderedConnectedKeyFrames):
            if pKF.mnId == 0: continue
            nRedundantObservations, nMPs = self._candidate_counts(pKF)
            if nRedundantObservations > 0.9 * nMPs:
                if pKF.mnId in self.kfs:
                    pKF.SetBadFlag(); del self.kfs[pKF.mnId]; erased.append(pKF.mnId)
        return erased

    def culling_votes(self, cur_id):
        """deviation 5: the votes against the map as it stands: [(candidate id, nRedundantObservations, nMPs, vote)]"""
        if cur_id not in self.kfs: return None
        out = []
        for pKF in self.kfs[cur_id].mvpOrderedConnectedKeyFrames:
            if pKF.mnId == 0 or pKF.isBad(): out.append((pKF.mnId, 0, 0, 0)); continue
            r, m = self._candidate_counts(pKF)
            out.append((pKF.mnId, r, m, int(r > 0.9 * m)))
        return out
