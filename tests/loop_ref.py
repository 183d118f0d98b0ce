"""Literal restatement of the map bookkeeping of loop closing on the objects of tests/covis_ref.py: KeyFrame::AddLoopEdge (KeyFrame.cc:419-430),
KeyFrame::GetCovisiblesByWeight with its upper_bound as written (:185-200), the three phases of LoopClosing::CorrectLoop that touch the graph (LoopClosing.cc:432-436 with
the marks of :472-516, and :546-564), and the vertex and edge loops of Optimizer::OptimizeEssentialGraph with sInsertedEdges (Optimizer.cc:797-983).  flatten_*() turn the
lists into the arrays the sgx_covis_loop_* / sgx_covis_essential_graph entries return.

Defined where the reference is not (include/sgx.h rules 10, 11): a keyframe with a loop edge is not erased; a dead list entry is no group member, no loop connection and
no edge end.  The mark mnCorrectedByKF behaves as fresh for every call."""
import covis_ref
from covis_ref import by_id, Invalid

MINFEAT = 100
EVENTS = dict(kind0=0, kind1=0, kind2=0, kind3=0, drop_parent=0, drop_child=0, drop_loop_edge=0, drop_larger_id=0, drop_dead=0, drop_inserted=0, tree_inserted=0,
              quirk_fired=0, quirk_not_fired=0, lc_row=0, asymmetric=0, curloop_weak=0, dropped_99=0, ref_later_in_list=0, dead_in_group_list=0, dead_in_row=0, prev_rebuilt=0,
              nomem_points=0, nomem_lc=0, nomem_edges=0)


class NoMem(Exception):
    pass


def loop_set(k):
    return k.__dict__.setdefault('mspLoopEdges', set())


class Map(covis_ref.Map):
    """covis_ref.Map with mspLoopEdges (capacity = the handle's max_keyframes pairs) and rule 10"""
    def __init__(self, monocular=False, th_depth=40.0, max_points=1 << 30, max_keyframes=1 << 30):
        covis_ref.Map.__init__(self, monocular, th_depth, max_points)
        self.max_keyframes = max_keyframes

    def n_loop_edges(self):
        return sum(len(loop_set(k)) for k in self.kfs.values()) // 2

    def add_loop_edge(self, a, b):
        if a == b or a not in self.kfs or b not in self.kfs: raise Invalid()
        A, B = self.kfs[a], self.kfs[b]
        if B in loop_set(A): return
        if self.n_loop_edges() >= self.max_keyframes: raise NoMem()
        loop_set(A).add(B); loop_set(B).add(A)                               # mpMatchedKF->AddLoopEdge(mpCurrentKF); mpCurrentKF->AddLoopEdge(mpMatchedKF)

    def loop_edges(self, kf_id):
        if kf_id not in self.kfs: raise Invalid()
        return [k.mnId for k in by_id(loop_set(self.kfs[kf_id]))]

    def erase_keyframe(self, kf_id):
        if kf_id in self.kfs and kf_id != 0 and loop_set(self.kfs[kf_id]): raise Invalid()      # mbNotErase: SetBadFlag only records mbToBeErased
        covis_ref.Map.erase_keyframe(self, kf_id)


def GetCovisiblesByWeight(k, w):
    if not k.mvpOrderedConnectedKeyFrames: return []
    # upper_bound(mvOrderedWeights.begin(), end(), w, weightComp) with weightComp(a, b) = a > b: the first element e with w > e
    it = next((i for i, e in enumerate(k.mvOrderedWeights) if w > e), None)
    if it is None: return []
    return list(k.mvpOrderedConnectedKeyFrames[:it])


def vertex_index(M):
    return {i: j for j, i in enumerate(sorted(M.kfs))}


# ---- CorrectLoop :432-436, :472-516
def loop_begin(M, cur, ev=EVENTS):
    """dict(group = mvpCurrentConnectedKFs, points = [(pMP, pKFi = its mnCorrectedReference)] in the order they are corrected), None for no keyframe"""
    if cur not in M.kfs: return None
    pCur = M.kfs[cur]
    pCur.UpdateConnections()
    group = []
    for k in pCur.mvpOrderedConnectedKeyFrames:                              # GetVectorCovisibleKeyFrames()
        if k.isBad(): ev['dead_in_group_list'] += 1; continue                # rule 11
        group.append(k)
    group.append(pCur)
    mark = object(); points = []
    place = {k: j for j, k in enumerate(group)}
    for pKFi in by_id(group):                                                # CorrectedSim3, a map<KeyFrame*, g2o::Sim3>
        for pMPi in pKFi.mvpMapPoints:
            if not pMPi: continue
            if pMPi.isBad(): continue
            if getattr(pMPi, 'mnCorrectedByKF', None) is mark: continue
            pMPi.mnCorrectedByKF = mark; pMPi.mnCorrectedReference = pKFi.mnId
            points.append((pMPi, pKFi))
            if any(place[o] < place[pKFi] for o in pMPi.mObservations if o in place): ev['ref_later_in_list'] += 1
        pKFi.UpdateConnections()
    return dict(group=group, points=points)


def flatten_begin(M, S, pcap=1 << 30, ev=EVENTS):
    vi = vertex_index(M); gi = {k: j for j, k in enumerate(S['group'])}
    n = len(S['points']); status = -3 if n > pcap else 0
    ev['nomem_points'] += status == -3
    P = S['points'][:max(pcap, 0)]
    return dict(status=status, group_id=[k.mnId for k in S['group']], group_vertex=[vi[k.mnId] for k in S['group']], point_id=[p.mnId for p, _ in P],
                point_ref=[gi[k] for _, k in P], report=dict(status=status, n_group=len(S['group']), n_points=n))


# ---- CorrectLoop :546-564
def group_of(M, cur, group_ids):
    """the group row as the entries validate it: live, distinct, cur last"""
    if len(set(group_ids)) != len(group_ids) or not group_ids or group_ids[-1] != cur or any(i not in M.kfs for i in group_ids): return None
    return [M.kfs[i] for i in group_ids]


def loop_connections(M, cur, group_ids, ev=EVENTS):
    """LoopConnections as {pKFi: set}, None for a refused group row (nothing changes)"""
    group = group_of(M, cur, group_ids)
    if group is None: return None
    LoopConnections = {}
    before = {k: list(k.mvpOrderedConnectedKeyFrames) for k in group}
    for pKFi in group:
        vpPreviousNeighbors = list(pKFi.mvpOrderedConnectedKeyFrames)
        if vpPreviousNeighbors != before[pKFi]: ev['prev_rebuilt'] += 1
        pKFi.UpdateConnections()
        s = set(pKFi.mConnectedKeyFrameWeights.keys())                       # GetConnectedKeyFrames()
        for p in vpPreviousNeighbors: s.discard(p)
        for g in group: s.discard(g)
        for k in list(s):
            if k.isBad(): s.discard(k); ev['dead_in_row'] += 1               # rule 11
        LoopConnections[pKFi] = s
        ev['lc_row'] += bool(s)
    return LoopConnections


def flatten_connections(LC, lcap=1 << 30, ev=EVENTS):
    if LC is None: return dict(status=-1)
    begin = [0]; rows = []
    for k, s in by_id(LC):
        rows.append([x.mnId for x in by_id(s)]); begin.append(begin[-1] + len(rows[-1]))
    status = -3 if begin[-1] > lcap else 0
    ev['nomem_lc'] += status == -3
    lc_j = []
    for r, row in enumerate(rows):
        if begin[r + 1] <= lcap: lc_j += row
    return dict(status=status, lc_begin=begin, lc_j=lc_j, full=[x for row in rows for x in row], report=dict(status=status, n_group=len(rows), n_connections=begin[-1]))


# ---- OptimizeEssentialGraph :797-983
def essential_graph(M, cur, loop, group_ids, lc_begin, lc_j, ev=EVENTS):
    """dict(vertices = [KeyFrame], edges = [(pKF of vertex 0, pKF of vertex 1, kind)]) in insertion order; None where the entry refuses its input"""
    group = group_of(M, cur, group_ids)
    if group is None or cur not in M.kfs or loop not in M.kfs: return None
    if len(lc_begin) != len(group) + 1 or lc_begin[0] != 0 or any(b < a for a, b in zip(lc_begin, lc_begin[1:])) or lc_begin[-1] > len(lc_j): return None
    LoopConnections = {}
    for r, (_, k) in enumerate(sorted((k.mnId, k) for k in group)):
        row = [int(x) for x in lc_j[lc_begin[r]:lc_begin[r + 1]]]
        if any(x not in M.kfs for x in row) or any(b <= a for a, b in zip(row, row[1:])): return None
        LoopConnections[k] = set(M.kfs[x] for x in row)
    pCurKF, pLoopKF = M.kfs[cur], M.kfs[loop]
    vpKFs = [k for _, k in sorted(M.kfs.items())]                            # GetAllKeyFrames(), none of them isBad()
    edges = []
    sInsertedEdges = set()
    for pKF, spConnections in by_id(LoopConnections):
        nIDi = pKF.mnId
        for pKFj in by_id(spConnections):
            nIDj = pKFj.mnId
            if (nIDi != pCurKF.mnId or nIDj != pLoopKF.mnId) and pKF.GetWeight(pKFj) < MINFEAT:
                ev['dropped_99'] += pKF.GetWeight(pKFj) == MINFEAT - 1
                ev['asymmetric'] += pKFj.GetWeight(pKF) >= MINFEAT
                continue
            ev['curloop_weak'] += pKF.GetWeight(pKFj) < MINFEAT
            ev['asymmetric'] += pKFj.GetWeight(pKF) < MINFEAT <= pKF.GetWeight(pKFj)
            edges.append((pKF, pKFj, 0)); ev['kind0'] += 1
            sInsertedEdges.add((min(nIDi, nIDj), max(nIDi, nIDj)))
    for pKF in vpKFs:
        pParentKF = pKF.mpParent
        if pParentKF:
            edges.append((pKF, pParentKF, 1)); ev['kind1'] += 1
            ev['tree_inserted'] += (min(pKF.mnId, pParentKF.mnId), max(pKF.mnId, pParentKF.mnId)) in sInsertedEdges
        sLoopEdges = loop_set(pKF)
        for pLKF in by_id(sLoopEdges):
            if pLKF.mnId < pKF.mnId:
                edges.append((pKF, pLKF, 2)); ev['kind2'] += 1
        vpConnectedKFs = GetCovisiblesByWeight(pKF, MINFEAT)
        if pKF.mvOrderedWeights and min(pKF.mvOrderedWeights) >= MINFEAT: ev['quirk_fired'] += 1
        if vpConnectedKFs: ev['quirk_not_fired'] += 1
        for pKFn in vpConnectedKFs:
            if pKFn is pParentKF: ev['drop_parent'] += 1; continue
            if pKFn in pKF.mspChildrens: ev['drop_child'] += 1; continue
            if pKFn in sLoopEdges: ev['drop_loop_edge'] += 1; continue
            if pKFn.isBad(): ev['drop_dead'] += 1; continue
            if not pKFn.mnId < pKF.mnId: ev['drop_larger_id'] += 1; continue
            if (min(pKF.mnId, pKFn.mnId), max(pKF.mnId, pKFn.mnId)) in sInsertedEdges: ev['drop_inserted'] += 1; continue
            edges.append((pKF, pKFn, 3)); ev['kind3'] += 1
    return dict(vertices=vpKFs, edges=edges, group=group, loop=pLoopKF, n_connections=lc_begin[-1])


def flatten_graph(S, ecap=1 << 30, ev=EVENTS):
    if S is None or ecap < 0: return dict(status=-1)
    vi = {k: j for j, k in enumerate(S['vertices'])}; gi = {k: j for j, k in enumerate(S['group'])}
    n = len(S['edges']); status = -3 if n > ecap else 0
    ev['nomem_edges'] += status == -3
    E = S['edges'][:ecap]
    return dict(status=status, vertex_id=[k.mnId for k in S['vertices']], vertex_fixed=[int(k is S['loop']) for k in S['vertices']],
                vertex_group=[gi.get(k, -1) for k in S['vertices']], e_i=[vi[e[0]] for e in E], e_j=[vi[e[1]] for e in E], e_kind=[e[2] for e in E],
                edges_by_id=[(e[0].mnId, e[1].mnId, e[2]) for e in E],
                report=dict(status=status, n_group=len(S['group']), n_connections=S['n_connections'], n_vertices=len(S['vertices']), n_edges=n,
                            n_kind=[sum(e[2] == k for e in S['edges']) for k in range(4)]))


# ---- the Sim3 glue: scalar float64 (Python floats) in the operation order of sgx_se3.h / sgx_sim3.h, float32 where the reference is float (cv::gemm's small-matrix path
# as tests/init_ref.py::mul3 / mulv3 state it, extended to four terms).  A Sim3 is [qx, qy, qz, qw, tx, ty, tz, s], a pose 3 x 4 float32.
import math
import numpy as np

F32 = np.float32


def quat_from_R(R):
    """Eigen Quaterniond(Matrix3d) as sgx_quat_from_R writes it"""
    q = [0.0] * 4
    t = R[0][0] + R[1][1] + R[2][2]
    if t > 0:
        t = math.sqrt(t + 1.0); q[3] = 0.5 * t; t = 0.5 / t
        q[0] = (R[2][1] - R[1][2]) * t; q[1] = (R[0][2] - R[2][0]) * t; q[2] = (R[1][0] - R[0][1]) * t
    else:
        i = 0
        if R[1][1] > R[0][0]: i = 1
        if R[2][2] > R[i][i]: i = 2
        if i == 0:
            t = math.sqrt(R[0][0] - R[1][1] - R[2][2] + 1.0); q[0] = 0.5 * t; t = 0.5 / t
            q[3] = (R[2][1] - R[1][2]) * t; q[1] = (R[1][0] + R[0][1]) * t; q[2] = (R[2][0] + R[0][2]) * t
        elif i == 1:
            t = math.sqrt(R[1][1] - R[2][2] - R[0][0] + 1.0); q[1] = 0.5 * t; t = 0.5 / t
            q[3] = (R[0][2] - R[2][0]) * t; q[2] = (R[2][1] + R[1][2]) * t; q[0] = (R[0][1] + R[1][0]) * t
        else:
            t = math.sqrt(R[2][2] - R[0][0] - R[1][1] + 1.0); q[2] = 0.5 * t; t = 0.5 / t
            q[3] = (R[1][0] - R[0][1]) * t; q[0] = (R[0][2] + R[2][0]) * t; q[1] = (R[1][2] + R[2][1]) * t
    return q


def quat_rotate(q, v):
    ux = q[1] * v[2] - q[2] * v[1]; uy = q[2] * v[0] - q[0] * v[2]; uz = q[0] * v[1] - q[1] * v[0]
    ux += ux; uy += uy; uz += uz
    return [v[0] + q[3] * ux + (q[1] * uz - q[2] * uy), v[1] + q[3] * uy + (q[2] * ux - q[0] * uz), v[2] + q[3] * uz + (q[0] * uy - q[1] * ux)]


def quat_mul(a, b):
    return [a[3] * b[0] + a[0] * b[3] + a[1] * b[2] - a[2] * b[1], a[3] * b[1] + a[1] * b[3] + a[2] * b[0] - a[0] * b[2],
            a[3] * b[2] + a[2] * b[3] + a[0] * b[1] - a[1] * b[0], a[3] * b[3] - a[0] * b[0] - a[1] * b[1] - a[2] * b[2]]


def quat_to_R(q):
    tx = 2 * q[0]; ty = 2 * q[1]; tz = 2 * q[2]
    twx = tx * q[3]; twy = ty * q[3]; twz = tz * q[3]
    txx = tx * q[0]; txy = ty * q[0]; txz = tz * q[0]; tyy = ty * q[1]; tyz = tz * q[1]; tzz = tz * q[2]
    return [[1 - (tyy + tzz), txy - twz, txz + twy], [txy + twz, 1 - (txx + tzz), tyz - twx], [txz - twy, tyz + twx, 1 - (txx + tyy)]]


def sim3_mul(a, b):
    rt = quat_rotate(a[:4], b[4:7])
    return quat_mul(a[:4], b[:4]) + [a[7] * rt[0] + a[4], a[7] * rt[1] + a[5], a[7] * rt[2] + a[6], a[7] * b[7]]


def sim3_inverse(a):
    q = [-a[0], -a[1], -a[2], a[3]]
    f = -1. / a[7]
    return q + quat_rotate(q, [f * a[4], f * a[5], f * a[6]]) + [1. / a[7]]


def sim3_map(S, x):
    r = quat_rotate(S[:4], x)
    return [S[7] * r[0] + S[4], S[7] * r[1] + S[5], S[7] * r[2] + S[6]]


def sim3_of_pose(T):
    """g2o::Sim3(Converter::toMatrix3d(R), Converter::toVector3d(t), 1.0)"""
    R = [[float(T[r][c]) for c in range(3)] for r in range(3)]
    return quat_from_R(R) + [float(T[0][3]), float(T[1][3]), float(T[2][3]), 1.0]


def pose_of_sim3(S):
    """Converter::toCvSE3(rotation().toRotationMatrix(), translation() * (1. / scale()))"""
    R = quat_to_R(S[:4]); inv = 1. / S[7]
    return np.array([[F32(R[r][0]), F32(R[r][1]), F32(R[r][2]), F32(S[4 + r] * inv)] for r in range(3)], 'f4')


def propagate_sim3(Tcw, Scw):
    """CorrectLoop :440-469, :503-512 over the group (cur last): (NonCorrectedSim3, CorrectedSim3, the corrected poses)"""
    Tcw = [np.asarray(T, 'f4')[:3, :4] for T in Tcw]; Scw = [float(x) for x in Scw]
    Tc = Tcw[-1]
    Twc = np.zeros((4, 4), 'f4'); Twc[3, 3] = 1                                  # KeyFrame::SetPose
    for r in range(3):
        for c in range(3): Twc[r, c] = Tc[c, r]
        d = Tc[0, r] * Tc[0, 3] + Tc[1, r] * Tc[1, 3] + Tc[2, r] * Tc[2, 3]       # float32, left to right
        Twc[r, 3] = F32(float(d) * -1.0)                                         # Ow = -Rwc * tcw: alpha = -1
    non, cor, out = [], [], []
    for g, Ti in enumerate(Tcw):
        non.append(sim3_of_pose(Ti))
        if g != len(Tcw) - 1:
            Tic = np.zeros((3, 4), 'f4')
            for r in range(3):
                for c in range(4):
                    d = Ti[r, 0] * Twc[0, c] + Ti[r, 1] * Twc[1, c] + Ti[r, 2] * Twc[2, c] + Ti[r, 3] * Twc[3, c]
                    Tic[r, c] = F32(float(d) * 1.0)
            cor.append(sim3_mul(sim3_of_pose(Tic), Scw))
        else: cor.append(list(Scw))
        out.append(pose_of_sim3(cor[-1]))
    return np.array(non), np.array(cor), np.array(out, 'f4')


def flatten_sim3(vertex_group, Tcw, corrected, noncorrected, e_i, e_j, e_kind):
    """vScw and the measurements Sji = Sjw * Swi of Optimizer.cc:818-832, :857-867, :889-972"""
    cor = [[float(x) for x in s] for s in corrected]; non = [[float(x) for x in s] for s in noncorrected]
    S_in = [cor[g] if g >= 0 else sim3_of_pose(np.asarray(Tcw[v], 'f4')) for v, g in enumerate(vertex_group)]
    meas = []
    for i, j, k in zip(e_i, e_j, e_kind):
        gi = vertex_group[i] if k else -1; gj = vertex_group[j] if k else -1
        Siw = non[gi] if gi >= 0 else S_in[i]; Sjw = non[gj] if gj >= 0 else S_in[j]
        meas.append(sim3_mul(Sjw, sim3_inverse(Siw)))
    return np.array(S_in, 'f8').reshape(-1, 8), np.array(meas, 'f8').reshape(-1, 8)


def recover_sim3(S_out):
    S = [[float(x) for x in s] for s in S_out]
    return np.array([pose_of_sim3(s) for s in S], 'f4').reshape(-1, 3, 4), np.array([sim3_inverse(s) for s in S], 'f8').reshape(-1, 8)


def correct_points(xw, ref, Srw, cSwr):
    out = np.zeros((len(xw), 3), 'f4')
    for n, (p, r) in enumerate(zip(np.asarray(xw, 'f4'), ref)):
        o = sim3_map([float(x) for x in cSwr[r]], sim3_map([float(x) for x in Srw[r]], [float(p[0]), float(p[1]), float(p[2])]))
        out[n] = [F32(o[0]), F32(o[1]), F32(o[2])]
    return out
