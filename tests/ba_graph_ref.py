"""Literal restatement of the graph construction of the reference's bundle adjustments on the objects of tests/covis_ref.py: the set selection of
Optimizer::LocalBundleAdjustment (Optimizer.cc:453-504) with mnBALocalForKF / mnBAFixedForKF as written, its edge loop (:572-653), the vertex and edge loops of
Optimizer::BundleAdjustment (:49-150) over Map::GetAllKeyFrames / GetAllMapPoints, and the vToErase loops (:711-757).  flatten() turns the lists into the arrays
sgx_covis_ba_graph returns.

Defined where the reference is not: the marks start as no keyframe's id before a query (the reference initialises them to 0 and never runs for keyframe 0, whose query
is one like any other here); the points of the global graph run in ascending id (a set<MapPoint*> there)."""
import numpy as np
from covis_ref import by_id

ATTR_RIGHT = 32; ATTR_CLOSE = 64
EVENTS = dict(dead_skipped=0, fixed=0, pose_fixed_2=0, first_kept=0, bad_by_erase=0, nomem=0)


def attr_of(pKF, idx):
    """the handle's attribute byte (sgx_covis_add_keyframe): octave | RIGHT | CLOSE, close = !(depth > th_depth || depth < 0) in float"""
    close = not (pKF.mvDepth[idx] > pKF.mThDepth or pKF.mvDepth[idx] < 0)
    return pKF.octave[idx] | (ATTR_RIGHT if pKF.mvuRight[idx] >= 0 else 0) | (ATTR_CLOSE if close else 0)


def LocalBundleAdjustment(M, kf_id, ev=EVENTS):
    """the lists of :453-504 and the edges of :572-653: dict(local, points, fixed, edges = [(pKFi, pMP, idx, stereo)] in insertion order), None for no keyframe"""
    if kf_id not in M.kfs: return None
    for k in M.all_kfs.values(): k.mnBALocalForKF = -1; k.mnBAFixedForKF = -1
    for p in M.points.values(): p.mnBALocalForKF = -1
    pKF = M.kfs[kf_id]
    lLocalKeyFrames = [pKF]
    pKF.mnBALocalForKF = pKF.mnId
    vNeighKFs = list(pKF.mvpOrderedConnectedKeyFrames)                        # GetVectorCovisibleKeyFrames()
    for pKFi in vNeighKFs:
        pKFi.mnBALocalForKF = pKF.mnId
        if not pKFi.isBad(): lLocalKeyFrames.append(pKFi)
        else: ev['dead_skipped'] += 1
    lLocalMapPoints = []
    for lit in lLocalKeyFrames:
        for pMP in lit.mvpMapPoints:
            if pMP:
                if not pMP.isBad():
                    if pMP.mnBALocalForKF != pKF.mnId:
                        lLocalMapPoints.append(pMP); pMP.mnBALocalForKF = pKF.mnId
                    else: ev['first_kept'] += 1
    lFixedCameras = []
    for pMP in lLocalMapPoints:
        for pKFi, _ in by_id(pMP.mObservations):
            if pKFi.mnBALocalForKF != pKF.mnId and pKFi.mnBAFixedForKF != pKF.mnId:
                pKFi.mnBAFixedForKF = pKF.mnId
                if not pKFi.isBad(): lFixedCameras.append(pKFi)
    ev['fixed'] += len(lFixedCameras)
    edges = []
    for pMP in lLocalMapPoints:
        for pKFi, idx in by_id(pMP.mObservations):
            if not pKFi.isBad():
                if pKFi.mvuRight[idx] < 0: edges.append((pKFi, pMP, idx, False))      # vpEdgesMono / vpEdgeKFMono / vpMapPointEdgeMono
                else: edges.append((pKFi, pMP, idx, True))                            # vpEdgesStereo / ...
    return dict(local=lLocalKeyFrames, points=lLocalMapPoints, fixed=lFixedCameras, edges=edges)


def BundleAdjustment(M):
    """:49-150 on GetAllKeyFrames() / GetAllMapPoints()"""
    vpKFs = [k for _, k in sorted(M.kfs.items())]
    vpMP = [p for _, p in sorted(M.points.items())]
    local = []; maxKFid = 0
    for pKF in vpKFs:
        if pKF.isBad(): continue
        local.append(pKF)
        if pKF.mnId > maxKFid: maxKFid = pKF.mnId
    points = []; edges = []
    for pMP in vpMP:
        if pMP.isBad(): continue
        points.append(pMP)
        for pKF, idx in by_id(pMP.mObservations):
            if pKF.isBad() or pKF.mnId > maxKFid: continue
            edges.append((pKF, pMP, idx, not pKF.mvuRight[idx] < 0))
    return dict(local=local, points=points, fixed=[], edges=edges)


def flatten(S, pcap=1 << 30, ecap=1 << 30, ev=EVENTS):
    """the arrays of sgx_covis_ba_graph from the lists; beyond pcap / ecap: status -3, the first pcap points and the edges of the points that fit wholly"""
    if S is None or pcap < 0 or ecap < 0: return dict(status=-1)
    poses = sorted(S['local'] + S['fixed'], key=lambda k: k.mnId)
    fixed = set(id(k) for k in S['fixed'])
    pose_fixed = [1 if id(k) in fixed else (2 if k.mnId == 0 else 0) for k in poses]      # setFixed(pKFi->mnId==0) (:529), setFixed(true) (:542)
    ev['pose_fixed_2'] += pose_fixed.count(2)
    pidx = {id(k): j for j, k in enumerate(poses)}; qidx = {id(p): j for j, p in enumerate(S['points'])}
    begin = [0] * (len(S['points']) + 1)
    for _, pMP, _, _ in S['edges']: begin[qidx[id(pMP)] + 1] += 1
    begin = list(np.cumsum(begin))
    assert [qidx[id(e[1])] for e in S['edges']] == sorted(qidx[id(e[1])] for e in S['edges'])      # the outer loop is the points'
    n_points = len(S['points']); n_edges = len(S['edges']); n_stereo = sum(e[3] for e in S['edges'])
    status = -3 if n_points > pcap or n_edges > ecap else 0
    ev['nomem'] += status == -3
    npt = min(n_points, pcap); begin = begin[:npt + 1]
    ne = max(b for b in begin if b <= ecap)
    E = S['edges'][:ne]
    return dict(status=status, pose_id=[k.mnId for k in poses], pose_fixed=pose_fixed, point_id=[p.mnId for p in S['points'][:npt]], point_edge_begin=[int(b) for b in begin],
                edge_pose=[pidx[id(e[0])] for e in E], edge_point=[qidx[id(e[1])] for e in E], edge_kp=[e[2] for e in E], edge_attr=[attr_of(e[0], e[2]) for e in E],
                report=dict(status=status, n_local_kf=len(S['local']), n_fixed_kf=len(S['fixed']), n_poses=len(poses), n_points=n_points, n_edges=n_edges,
                            n_mono_edges=n_edges - n_stereo, n_stereo_edges=n_stereo))


def apply_erase(M, S, erase, ev=EVENTS):
    """:711-757: vToErase from the flagged monocular edges and then the flagged stereo ones, and the erase loop.  erase: a flag per edge of S['edges'].  Returns the
    (keyframe id, point id) pairs of vToErase."""
    assert len(erase) == len(S['edges'])
    vToErase = []
    for stereo in (False, True):
        for flag, (pKFi, pMP, _, st) in zip(erase, S['edges']):
            if st != stereo: continue
            if pMP.isBad(): continue
            if flag: vToErase.append((pKFi, pMP))
    for pKFi, pMPi in vToErase:
        idx = pMPi.mObservations.get(pKFi, -1)                                 # KeyFrame::EraseMapPointMatch(MapPoint*): GetIndexInKeyFrame
        if idx >= 0: pKFi.mvpMapPoints[idx] = None
        was = pMPi.isBad()
        pMPi.EraseObservation(pKFi)
        ev['bad_by_erase'] += pMPi.isBad() and not was
    return [(k.mnId, p.mnId) for k, p in vToErase]
