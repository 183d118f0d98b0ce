"""Literal restatement of LoopClosing::DetectLoop's covisibility consistency (src/sg-slam/src/LoopClosing.cc:152-225) with Python sets over the objects of
tests/loop_ref.py / tests/covis_ref.py, and of KeyFrame::GetConnectedKeyFrames as the CSR sgx_covis_connected_batch returns.

Defined where the reference is not (include/sgx.h rules 12, 13): the members of a set<KeyFrame*> are keyframe ids; a dead entry of a weight row is no member of a
candidate's group; a stored group keeps the id of a keyframe erased since and never matches through it; a candidate the map does not hold, a candidate twice, or more
than max_groups resulting groups refuse the call and leave everything as it was.

EVENTS counts the branches a case set has to reach; tests/loopclose_cases.py asserts that each fired."""

EVENTS = dict(pushed_twice=0, pushed_nothing=0, enough_but_marked=0, cleared=0, stale_slot=0, pushed_zero=0, dead_in_row=0, weak_member=0)


class Detector:
    """mvConsistentGroups and mvpEnoughConsistentCandidates over a Map"""
    def __init__(self, M, max_groups=64):
        self.M = M; self.max_groups = max_groups
        self.mvConsistentGroups = []                                         # [(set of ids, counter)]

    def clear(self):
        self.mvConsistentGroups = []

    def groups(self):
        return [(sorted(s), n) for s, n in self.mvConsistentGroups]

    def candidate_group(self, pCandidateKF, ev=EVENTS):
        spCandidateGroup = set()
        for k, w in pCandidateKF.mConnectedKeyFrameWeights.items():          # GetConnectedKeyFrames(): every key of the map
            if k.isBad(): ev['dead_in_row'] += 1; continue                   # rule 12
            if w < 15: ev['weak_member'] += 1
            spCandidateGroup.add(k.mnId)
        spCandidateGroup.add(pCandidateKF.mnId)
        return spCandidateGroup

    def consistency(self, cand_ids, th=3, ev=EVENTS):
        """dict(status, enough = mvpEnoughConsistentCandidates as ids, report)"""
        M = self.M; before = len(self.mvConsistentGroups)
        refused = dict(status=-1, enough=None, report=dict(status=-1, n_before=before, n_after=before))
        if len(set(cand_ids)) != len(cand_ids) or any(c not in M.kfs for c in cand_ids): return refused      # rule 13
        if not cand_ids:                                                     # :144-150
            self.mvConsistentGroups = []; ev['cleared'] += 1
            return dict(status=0, enough=[], report=dict(status=0, n_before=before, n_after=0, n_consistent=0, n_pushed_zero=0, n_pushed_nothing=0, n_enough=0, n_cand=0))
        vpCandidateKFs = [M.kfs[c] for c in cand_ids]
        mvpEnoughConsistentCandidates = []
        vCurrentConsistentGroups = []
        vbConsistentGroup = [False] * len(self.mvConsistentGroups)
        n_consistent = n_zero = n_nothing = 0
        live = set(M.kfs)
        for pCandidateKF in vpCandidateKFs:
            spCandidateGroup = self.candidate_group(pCandidateKF, ev)
            bEnoughConsistent = False
            bConsistentForSomeGroup = False
            pushed = 0
            for iG in range(len(self.mvConsistentGroups)):
                sPreviousGroup = self.mvConsistentGroups[iG][0]
                if sPreviousGroup - live: ev['stale_slot'] += 1              # a stored member erased since: it matches nothing (rule 12)
                bConsistent = False
                for sit in sorted(spCandidateGroup):
                    if sit in sPreviousGroup:
                        bConsistent = True
                        bConsistentForSomeGroup = True
                        break
                if bConsistent:
                    nPreviousConsistency = self.mvConsistentGroups[iG][1]
                    nCurrentConsistency = nPreviousConsistency + 1
                    if not vbConsistentGroup[iG]:
                        vCurrentConsistentGroups.append((set(spCandidateGroup), nCurrentConsistency))
                        vbConsistentGroup[iG] = True
                        pushed += 1
                    elif nCurrentConsistency >= th and not bEnoughConsistent: ev['enough_but_marked'] += 1
                    if nCurrentConsistency >= th and not bEnoughConsistent:
                        mvpEnoughConsistentCandidates.append(pCandidateKF.mnId)
                        bEnoughConsistent = True
            if not bConsistentForSomeGroup:
                vCurrentConsistentGroups.append((set(spCandidateGroup), 0))
                n_zero += 1; ev['pushed_zero'] += 1
            else:
                n_consistent += 1
                if pushed >= 2: ev['pushed_twice'] += 1
                if pushed == 0: n_nothing += 1; ev['pushed_nothing'] += 1
        if len(vCurrentConsistentGroups) > self.max_groups:                  # rule 13
            return dict(status=-3, enough=None, report=dict(status=-3, n_before=before, n_after=before))
        self.mvConsistentGroups = vCurrentConsistentGroups
        return dict(status=0, enough=mvpEnoughConsistentCandidates,
                    report=dict(status=0, n_before=before, n_after=len(vCurrentConsistentGroups), n_consistent=n_consistent, n_pushed_zero=n_zero,
                                n_pushed_nothing=n_nothing, n_enough=len(mvpEnoughConsistentCandidates), n_cand=len(cand_ids)))


def connected_batch(M, kf_ids, cap=1 << 30):
    """dict(off, rows (None where the query's status is not 0), status, n)"""
    off = [0]; rows = []; status = []; n = []
    for i in kf_ids:
        if i not in M.kfs:
            rows.append(None); status.append(-1); n.append(0); off.append(off[-1]); continue
        row = sorted(k.mnId for k in M.kfs[i].mConnectedKeyFrameWeights if not k.isBad())
        off.append(off[-1] + len(row)); n.append(len(row))
        if off[-1] > cap: rows.append(None); status.append(-3)
        else: rows.append(row); status.append(0)
    return dict(off=off, rows=rows, status=status, n=n)


# ---- LoopClosing::RunGlobalBundleAdjustment :676-737 --------------------------------------------------------------------------------------------------------------------
# numpy float32 scalars; KeyFrame::SetPose and the cv::Mat product in the form of loop_ref.propagate_sim3 (:276-297): float32 products summed left to right, alpha applied
# in double.  Rules 14 and 15 of include/sgx.h.  OpenCV is not pinned: this file is the yardstick.
import numpy as np
from collections import deque

F32 = np.float32
GBA_EVENTS = dict(chain_depth3=0, unreached=0, point_skipped=0, reparented=0, two_origins=0)
ORIGIN_NOT_IN_GBA = 1


def pose_inverse(T):
    """KeyFrame::SetPose: Twc as 4 x 4 float32"""
    Twc = np.zeros((4, 4), 'f4'); Twc[3, 3] = 1
    for r in range(3):
        for c in range(3): Twc[r, c] = T[c, r]
        d = T[0, r] * T[0, 3] + T[1, r] * T[1, 3] + T[2, r] * T[2, 3]
        Twc[r, 3] = F32(float(d) * -1.0)
    return Twc


def mul44(A, B):
    """rows 0..2 of the product of two 4 x 4 poses (A given as 3 x 4 or 4 x 4, B as 4 x 4)"""
    C = np.zeros((4, 4), 'f4'); C[3, 3] = 1
    for r in range(3):
        for c in range(4):
            d = A[r, 0] * B[0, c] + A[r, 1] * B[1, c] + A[r, 2] * B[2, c] + A[r, 3] * B[3, c]
            C[r, c] = F32(float(d) * 1.0)
    return C


def map_point(T, x):
    """R * x + t as one gemm"""
    y = np.zeros(3, 'f4')
    for r in range(3):
        d = T[r, 0] * x[0] + T[r, 1] * x[1] + T[r, 2] * x[2]
        y[r] = F32(float(d) * 1.0 + float(T[r, 3]) * 1.0)
    return y


def as44(T):
    P = np.zeros((4, 4), 'f4'); P[3, 3] = 1; P[:3, :] = np.asarray(T, 'f4').reshape(-1, 4)[:3]
    return P


def gba_update(M, origins, kf_ids, in_gba, Tcw, TcwGBA, ev=GBA_EVENTS):
    """dict(status, Tcw_out (nk x 3 x 4), TcwBef {row: 3 x 4} of the visited rows, kf_state, report)"""
    nk = len(kf_ids)
    if nk != len(M.kfs) or len(set(kf_ids)) != nk or any(k not in M.kfs for k in kf_ids) or any(o not in M.kfs for o in origins): return dict(status=-1)
    row = {k: r for r, k in enumerate(kf_ids)}
    if any(not in_gba[row[o]] for o in origins): return dict(status=ORIGIN_NOT_IN_GBA)                      # rule 14
    pose = {k: as44(Tcw[row[k]]) for k in kf_ids}                                                           # GetPose()
    mTcwGBA = {k: as44(TcwGBA[row[k]]) for k in kf_ids if in_gba[row[k]]}
    mnBAGlobalForKF = {k: bool(in_gba[row[k]]) for k in kf_ids}
    mTcwBefGBA = {}; visited = set(); depth = {}
    if len(set(origins)) >= 2: ev['two_origins'] += 1
    lpKFtoCheck = deque(M.kfs[o] for o in origins)
    old = dict(pose)
    while lpKFtoCheck:
        pKF = lpKFtoCheck[0]
        Twc = pose_inverse(old[pKF.mnId])                                    # :683, the pose before :698
        for pChild in sorted(pKF.mspChildrens, key=lambda k: k.mnId):
            if pChild.isBad(): continue
            if not mnBAGlobalForKF[pChild.mnId]:
                Tchildc = mul44(old[pChild.mnId], Twc)
                mTcwGBA[pChild.mnId] = mul44(Tchildc, mTcwGBA[pKF.mnId])
                mnBAGlobalForKF[pChild.mnId] = True
                depth[pChild.mnId] = depth.get(pKF.mnId, 0) + 1
                if depth[pChild.mnId] >= 3: ev['chain_depth3'] += 1
            lpKFtoCheck.append(pChild)
        mTcwBefGBA[pKF.mnId] = old[pKF.mnId]
        pose[pKF.mnId] = mTcwGBA[pKF.mnId]                                   # SetPose(mTcwGBA)
        visited.add(pKF.mnId)
        lpKFtoCheck.popleft()
    un = [k for k in kf_ids if k not in visited]
    ev['unreached'] += len(un)                                               # rule 15
    state = [(1 if k in visited else 0) | (2 if mnBAGlobalForKF[k] else 0) for k in kf_ids]
    return dict(status=0, Tcw_out=np.array([pose[k][:3] for k in kf_ids], 'f4'), TcwBef={row[k]: mTcwBefGBA[k][:3] for k in visited}, kf_state=state,
                report=dict(status=0, n_visited=len(visited), n_propagated=len(depth), n_unreached=len(un), max_depth=max(depth.values(), default=0)))


def gba_correct_points(xw, in_gba, xw_gba, ref, S, ev=GBA_EVENTS):
    """:705-736 on the result S of gba_update"""
    out = np.array(xw, 'f4').reshape(-1, 3).copy()
    for i in range(len(out)):
        if in_gba[i]: out[i] = np.asarray(xw_gba[i], 'f4'); continue
        r = int(ref[i])
        if r < 0 or S['kf_state'][r] != 3: ev['point_skipped'] += 1; continue      # pRefKF->mnBAGlobalForKF != nLoopKF; rule 15 for a keyframe that was not visited
        Xc = map_point(as44(S['TcwBef'][r]), out[i])
        out[i] = map_point(pose_inverse(as44(S['Tcw_out'][r])), Xc)
    return out
