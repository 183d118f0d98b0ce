"""Cases for the ten LocalMapping / LoopClosing / initialiser matcher entries and the new-map-point step (sgx_match2_kernels.h): one hand-made scene per gate that the
synthetic keyframe pairs of match2_cases never reach, in the manner of match_gate_cases (whose descriptors, scale tables and exact-in-float camera are imported).

Groups: T SearchForTriangulation, B SearchByBoW (both overloads), P the projection body (fuse_search, fuse_search_sim3, project_sim3, search_by_sim3, project_keyframe:
one table of cases, every case run through every entry that has the gate, with the expected DIFFERENCE between entries written out), S SearchBySim3's own rules and the
Scw decomposition, I SearchForInitialization, N the per-pair body of CreateNewMapPoints, Z the sizes at which a kernel's loop takes another turn (oracle only).

A case's `want` is written out by hand from the reference's text (ORBmatcher.cc:140-157, 159-290, 292-405, 407-522, 524-657, 659-827, 829-1101, 1106-1330, 1474-1644,
KeyFrame.cc:570-609, MapPoint.cc PredictScale, LocalMapping.cc:283-421); no code computes it.  Comparisons made in double against a decimal literal, with the floats on
either side (asserted in check_case_contents):
    3.84   float(3.84f) = 3.83999991 is BELOW the literal.  The epipolar cases put dsqr = 4 against 3.84 * sigma2 with sigma2 = 1.04166663 (product 3.99999985: rejected)
           and the next float 1.04166675 (product 4.00000031: accepted).
    5.99   float(5.99f) = 5.98999977 is BELOW the literal: e2 * invSigma2 = 5.99f is not `> 5.99` (kept), the next float 5.99000025 is (rejected).
    7.8    float(7.8f) = 7.80000019 is ABOVE the literal: 7.8f is rejected, the float below it, 7.79999971, is kept.
    0.5    exact: dot == 0.5 * dist is kept (`<` rejects), the float below 0.5 as the normal's length is rejected.
    0.7f = 0.69999999 and 0.9f = 0.89999998 are below their literals, but 0.7f * 10.0f and 0.9f * 10.0f round to 7.0f and 9.0f in float: 7 < 7.0f and 9 < 9.0f are false.
    100 * 1.2f = 120.000008 in float; 100 * 1.0f = 100: a squared distance of exactly 100 to the epipole is not `< 100`."""
import numpy as np
import match_gate_cases as mg
from match_gate_cases import desc, scales, below, above, inward, CAM, SF, I4, f32, at, lp, local_of, cur_of, norm3
from oracle.oracle import KP_DTYPE
from sg_slam_amd import mappoint
from sg_slam_amd.matcher import ORBmatcher

X0, X1, Y0, Y1 = (f32(CAM[k]) for k in ('min_x', 'max_x', 'min_y', 'max_y'))
S_OUT = f32(4 / 3.84); S_IN = above(S_OUT)                 # 3.84 * S_OUT < 4 < 3.84 * S_IN
M_IN = f32(5.99); M_OUT = above(M_IN)                      # M_IN < 5.99 < M_OUT
C_OUT = f32(7.8); C_IN = below(C_OUT)                      # C_IN < 7.8 < C_OUT
SG = np.array([1, S_IN, S_OUT, 4, 4, 4, 4, 4], 'f4')       # level sigma^2 of the T cases
IS2_OFF = np.full(12, 2.0 ** -20, 'f4')                    # inverse sigma^2 that lets Fuse's chi^2 gate pass everything
IS2_CHI = np.array([1, M_IN, M_OUT, C_IN, C_OUT, 1, 1, 1], 'f4')
RZ = np.array([[0, -1, 0], [1, 0, 0], [0, 0, 1]], 'f4')    # +90 degrees about z: exact, and RZ != RZ.T
CLAMP0_Z = f32(1.2) * f32(1.75)                            # 2.1000001: the far edge of the distance band of max_dist = 1.75


def keys_of(rows):
    """keypoints from rows (x, y, octave, flipped bits[, uright[, angle]])"""
    return cur_of(rows)


# ===================================================================================================================== T: SearchForTriangulation
# F12 = [[0, 0, 0], [0, 0, -1], [0, 1, 0]]: the epipolar line of keypoint 1 is (a, b, c) = (0, 1, -y1), so den = 1 and dsqr = (y2 - y1)^2 exactly.
# Camera centre 1 = (0.5, 0.25, 2), Tcw2 = identity: the epipole is (128, 64).  scale2 = 1.2f^k, sigma2 = SG.
F_Y = np.array([[0, 0, 0], [0, 0, -1], [0, 1, 0]], 'f4')


def tri_side(rows, Tcw=I4):
    """rows (x, y, octave, bits, uright, has_mp, node[, angle])"""
    k = cur_of([(r[0], r[1], r[2], r[3], r[4], r[7] if len(r) > 7 else 0.0) for r in rows])
    return dict(keys=k['keys'], desc=k['desc'], uright=k['uright'], has_mp=np.array([r[5] for r in rows], np.uint8), feat_node=np.array([r[6] for r in rows], 'i4'),
                Tcw=np.array(Tcw, 'f4'), cam_center=np.array([0.5, 0.25, 2], 'f4'))


def G(g): return 900 - 10 * g                              # node ids fall while keypoint indices rise: node order is not index order


Y72 = below(72)
T_K1 = [(300, 100, 0, 0, -1, 1, G(0)), (300, 100, 0, 10, -1, 0, G(0)),          # 0, 1   g0 has_mp on side 1: 0 holds a point, 1 takes keypoint 0 of side 2
        (300, 110, 0, 0, -1, 0, G(1)),                                          # 2      g1 has_mp on side 2
        (300, 120, 0, 0, -1, 0, G(2)), (300, 120, 0, 0, -1, 0, G(2)),            # 3, 4   g2 TH_LOW: 50 accepted, 51 not
        (300, 130, 0, 0, -1, 0, G(3)),                                          # 5      g3 equal distances: the last wins
        (300, 140, 0, 0, -1, 0, G(4)),                                          # 6      g4 a closer candidate off the epipolar line does not lower bestDist
        (300, 72, 0, 0, -1, 0, G(5)), (300, 72, 0, 0, -1, 0, G(6)), (300, 72, 0, 0, -1, 0, G(7)), (300, 72, 0, 0, -1, 0, G(8)),          # 7-10  g5-g8 epipole
        (300, 72, 0, 0, 280, 0, G(9)),                                          # 11     g9 stereo on side 1: no epipole gate
        (300, 200, 0, 0, -1, 0, G(10)), (300, 200, 0, 0, -1, 0, G(10)),          # 12, 13 g10 octave 0: dsqr 1 in, 4 out
        (300, 220, 0, 0, -1, 0, G(11)), (300, 240, 0, 0, -1, 0, G(12)),          # 14, 15 g11 octave 1 (S_IN): 4 in; g12 octave 2 (S_OUT): 4 out
        (300, 260, 0, 10, -1, 0, G(14)), (300, 260, 0, 0, -1, 0, G(14)),         # 16, 17 g14 the lock: the lower idx1 takes it although the higher is closer
        (300, 270, 0, 0, -1, 0, G(15)), (300, 280, 0, 40, -1, 0, G(16)),         # 18, 19 g15, g16: the twin of each sits in the other node
        (300, 290, 0, 0, -1, 0, -1),                                            # 20     node -1
        (300, 300, 0, 0, 280, 0, G(17)), (300, 300, 0, 1, -1, 0, G(17))]         # 21, 22 g17 only_stereo
T_K2 = [(320, 100, 0, 0, -1, 0, G(0)),                                          # 0
        (320, 110, 0, 0, -1, 1, G(1)), (320, 110, 0, 10, -1, 0, G(1)),           # 1 holds a point, 2
        (320, 120, 0, 50, -1, 0, G(2)), (320, 120, 0, 51, -1, 0, G(2)),          # 3, 4
        (320, 130, 0, 7, -1, 0, G(3)), (320, 130, 0, 7, -1, 0, G(3)), (320, 130, 0, 8, -1, 0, G(3)),          # 5, 6, 7
        (320, 143, 0, 5, -1, 0, G(4)), (320, 140, 0, 20, -1, 0, G(4)),           # 8 (dsqr 9), 9
        (134, 72, 0, 0, -1, 0, G(5)),                                           # 10     36 + 64 = 100 from the epipole: not < 100
        (134, Y72, 0, 0, -1, 0, G(6)), (334, 72, 0, 30, -1, 0, G(6)),            # 11 one float nearer: skipped, 12
        (134, 72, 1, 0, -1, 0, G(7)), (334, 72, 0, 30, -1, 0, G(7)),             # 13 octave 1: 100 < 120.000008, 14
        (134, Y72, 0, 0, 100, 0, G(8)), (334, 72, 0, 30, -1, 0, G(8)),           # 15 stereo: no epipole gate, 16
        (134, Y72, 0, 0, -1, 0, G(9)), (334, 72, 0, 30, -1, 0, G(9)),            # 17, 18
        (320, 201, 0, 0, -1, 0, G(10)), (320, 202, 0, 0, -1, 0, G(10)),          # 19, 20
        (320, 222, 1, 0, -1, 0, G(11)),                                         # 21
        (320, 242, 2, 0, -1, 0, G(12)), (320, 240, 0, 30, -1, 0, G(12)),         # 22, 23
        (320, 260, 0, 0, -1, 0, G(14)),                                         # 24
        (320, 270, 0, 40, -1, 0, G(15)), (320, 280, 0, 0, -1, 0, G(16)),         # 25, 26
        (320, 290, 0, 0, -1, 0, -1),                                            # 27
        (320, 300, 0, 0, -1, 0, G(17)), (320, 300, 0, 9, 300, 0, G(17))]         # 28 mono, 29 stereo
T_PAIRS = [(1, 0), (2, 2), (3, 3), (5, 6), (6, 9), (7, 10), (8, 12), (9, 14), (10, 15), (11, 17), (12, 19), (14, 21), (15, 23), (16, 24), (18, 25), (19, 26), (21, 28), (22, 29)]
T_PAIRS_STEREO = [(21, 29)]                                # only_stereo: keypoint 21 may not take the monocular 28, 22 is monocular itself

HIST_ANG = [350, 350, 350, 10, 0, 354.5, 359.9, 84, 84, 84, 144, 144, 144]      # rot of pair i; pair 3 is 10 - 20 = -10, wrapped to 350
# bins: 29 four times (350 x 3 and the wrapped one), 0 three times (0, and 354.5, 359.9 through bin 30), 7 and 12 three times each.  ComputeThreeMaxima sees bins 0, 7, 12
# in that order with 3 each, then 29 with 4 pushes 12 out of third place: pairs 10-12 go, and nmatches is 13 - 3.


def hist_rows(counts):
    """counts[j] pairs with rot 60 (bin 5), 108 (bin 9), 144 (bin 12)"""
    return [a for a, c in zip((60, 108, 144), counts) for _ in range(c)]


def tri_case(name, k1, k2, want, F=F_Y, stereo=0, ori=0, sg=SG):
    return dict(name=name, kind='tri', kf1=tri_side(k1), kf2=tri_side(k2), F12=F, stereo=stereo, ori=ori, sf=SF, sg=sg, want=(len(want), np.array(want, 'i4').reshape(-1, 2)))


def _own_nodes(angles, x, second):
    """pair i in a node of its own, at y = 100 + 10 i (on each other's epipolar line), the first side carrying the angle"""
    return [(x, 100 + 10 * i, 0, 0, -1, 0, 100 + i, (20.0 if i == 3 and a == 10 else 0.0) if second else a) for i, a in enumerate(angles)]


# Two keypoints of side 1 that stay unmatched, both with rot 144 (bin 12): 13 is refused by TH_LOW (its only candidate is 51 away), 14 by the epipolar gate (dsqr 9).  Were
# either counted, bin 12 would hold 4, come first, and bin 7 (pairs 7-9) would go instead of bin 12.
H_K1 = _own_nodes(HIST_ANG, 300, 0) + [(300, 230, 0, 0, -1, 0, 113, 144.0), (300, 240, 0, 0, -1, 0, 114, 144.0)]
H_K2 = _own_nodes(HIST_ANG, 320, 1) + [(320, 230, 0, 51, -1, 0, 113, 0.0), (320, 243, 0, 0, -1, 0, 114, 0.0)]


def _t():
    out = [tri_case('T_gates', T_K1, T_K2, T_PAIRS), tri_case('T_gates_only_stereo', T_K1, T_K2, T_PAIRS_STEREO, stereo=1),
           tri_case('T_hist_ori1', H_K1, H_K2, [(i, i) for i in range(10)], ori=1),
           tri_case('T_hist_ori0', H_K1, H_K2, [(i, i) for i in range(13)], ori=0),
           # den == 0: F12 with only its corner entry set gives the line (0, 0, x1); nothing passes (ORBmatcher.cc:148-149)
           tri_case('T_den0', [(300, 100, 0, 0, -1, 0, 5)], [(320, 100, 0, 0, -1, 0, 5)], [], F=np.array([[0, 0, 1], [0, 0, 0], [0, 0, 0]], 'f4'))]
    # dsqr == 3.84 * sigma2 exactly: F12 = [[0, 0, -1], [0, 0, -1], [1, 1, 0]] gives the line (1, 1, -(x1 + y1)), den = 2; keypoint 2 at (+12, +12) has num = 24 and
    # dsqr = 576 / 2 = 288, and 3.84 * 75.0 rounds to 288.0 in double: 288 < 288 is false.  The control at (+11, +12) has 264.5.
    out.append(tri_case('T_epipolar_equal', [(300, 100, 0, 0, -1, 0, 5), (300, 200, 0, 0, -1, 0, 6)], [(312, 112, 0, 0, -1, 0, 5), (311, 212, 0, 0, -1, 0, 6)], [(1, 1)],
                        F=np.array([[0, 0, -1], [0, 0, -1], [1, 1, 0]], 'f4'), sg=np.full(8, 75, 'f4')))
    # the 0.1 rules: (10, 1): 1 < 1.0f is false, bin 9 stays; (11, 1): 1 < 1.1f, it goes; (10, 2, 1): third 1 < 1.0f false, all stay; (11, 2, 1): second stays, third goes
    for counts, keep in (((10, 1, 0), 11), ((11, 1, 0), 11), ((10, 2, 1), 13), ((11, 2, 1), 13)):
        a = hist_rows(counts)
        out.append(tri_case('T_tenth_%d_%d_%d' % counts, _own_nodes(a, 300, 0), _own_nodes(a, 320, 1), [(i, i) for i in range(keep)], ori=1))
    return out


# ===================================================================================================================== B: SearchByBoW
def N(g): return 50 + g


#        bits, good, node
B_KK = [(0, 0, N(0)), (10, 1, N(0)),                       # 0, 1   N0 good_k: 0 holds no good point, 1 takes the frame keypoint
        (0, 1, N(1)),                                      # 2      N1 good_f (KeyFrame overload only)
        (0, 1, N(2)), (0, 1, N(2)),                        # 3, 4   N2 a frame keypoint taken earlier is skipped and not counted for bestDist2
        (0, 1, N(3)), (0, 1, N(4)), (0, 1, N(5)),          # 5-7    N3 50, N4 49, N5 51
        (0, 1, N(6)), (0, 1, N(7)), (0, 1, N(8)), (0, 1, N(9)),          # 8-11   ratio test: 7 / 10, 6 / 10, 15 / 20, 14 / 20
        (0, 1, N(10)), (0, 1, N(11))]                      # 12, 13 N10 a lone candidate at 45, N11 45 with a second at 50
B_FF = [(0, 1, 999),                                       # 0      a node the keyframe does not have: the two sides index differently from here on
        (0, 1, N(0)),                                      # 1
        (0, 0, N(1)), (10, 1, N(1)),                       # 2 holds no good point (KeyFrame overload), 3
        (0, 1, N(2)), (30, 1, N(2)),                       # 4, 5
        (50, 1, N(3)), (49, 1, N(4)), (51, 1, N(5)),       # 6, 7, 8
        (7, 1, N(6)), (10, 1, N(6)), (6, 1, N(7)), (10, 1, N(7)), (15, 1, N(8)), (20, 1, N(8)), (14, 1, N(9)), (20, 1, N(9)),          # 9-16
        (45, 1, N(10)), (45, 1, N(11)), (50, 1, N(11))]    # 17, 18, 19
# KeyFrame-Frame overload: the answer is indexed by the FRAME's keypoints and holds keyframe indices; 50 is accepted; good_f does not exist (frame keypoint 2 is taken)
B_F_070 = (8, [-1, 1, 2, -1, 3, 4, 5, 6, -1, -1, -1, 9, -1, -1, -1, -1, -1, 12, -1, -1])
B_F_075 = (10, [-1, 1, 2, -1, 3, 4, 5, 6, -1, 8, -1, 9, -1, -1, -1, 11, -1, 12, -1, -1])      # 7 < 7.5 and 14 < 15 pass now; 15 < 15 does not
# KeyFrame-KeyFrame overload: indexed by keyframe 1's keypoints, holds keyframe 2 indices; 50 is refused (`< TH_LOW`); keypoint 2 of side 2 is skipped, so 2 takes 3
B_K_070 = (7, [-1, 1, 3, 4, 5, -1, 7, -1, -1, 11, -1, -1, 17, -1])
B_K_075 = (9, [-1, 1, 3, 4, 5, -1, 7, -1, 9, 11, -1, 15, 17, -1])


def bow_side(rows, angles=None):
    k = cur_of([(100 + 7 * i, 100, 0, r[0], -1, 0.0 if angles is None else angles[i]) for i, r in enumerate(rows)])
    return dict(keys=k['keys'], desc=k['desc'], good_mp=np.array([r[1] for r in rows], np.uint8), feat_node=np.array([r[2] for r in rows], 'i4'))


def bow_case(name, kind, kk, ff, ratio, ori, want):
    return dict(name=name, kind=kind, kf=kk, F=ff, ratio=ratio, ori=ori, want=want)


def _b():
    kk, ff = bow_side(B_KK), bow_side(B_FF)
    out = [bow_case('B_frame_0.7', 'bow', kk, ff, 0.7, 0, B_F_070), bow_case('B_frame_0.75', 'bow', kk, ff, 0.75, 0, B_F_075),
           bow_case('B_keyframe_0.7', 'bowkf', kk, ff, 0.7, 0, B_K_070), bow_case('B_keyframe_0.75', 'bowkf', kk, ff, 0.75, 0, B_K_075)]
    own = [(0, 1, 100 + i) for i in range(13)]
    hk = bow_side(own, HIST_ANG); hf = bow_side(own, [20.0 if i == 3 else 0.0 for i in range(13)])
    for kind in ('bow', 'bowkf'):
        out.append(bow_case('B_hist_ori1_' + kind, kind, hk, hf, 0.7, 1, (10, list(range(10)) + [-1] * 3)))
        out.append(bow_case('B_hist_ori0_' + kind, kind, hk, hf, 0.7, 0, (13, list(range(13)))))
    return out


# ===================================================================================================================== P: the projection body
# A case: keypoints, points, th (an integer: project_sim3 takes an int), and per entry the keypoint each point ends with, written by hand:
#   want['A']   fuse_search, fuse_search_sim3 and project_sim3 (unless the case names one of them: 'fuse', 'fs3', 'ps3'), want['pkf'] project_keyframe,
#   want['bys'] search_by_sim3 (identity Sim3; side 1 carries the points, side 2 the keypoints; see bys_sides).
# An entry missing from want is not run on the case.  dist: the Hamming distance of every fused pair, for the two Fuse entries.
ENTRIES = ('fuse', 'fs3', 'ps3', 'pkf', 'bys')


def p_case(name, rows, pts, want, th=15, dist=None, sf=SF, is2=IS2_OFF, od=50, taken=None, Scw=I4, **extra):
    K = keys_of(rows); n = len(rows)
    return dict(name=name, kind='proj', K=K, P=local_of(pts), th=th, sf=sf, is2=is2[:len(sf)], od=od, taken=np.zeros(n, np.uint8) if taken is None else np.array(taken, np.uint8),
                Scw=np.array(Scw, 'f4'), want=want, dist=dist, **extra)


def want_for(c, e):
    w = c['want']
    return w.get(e, w.get('A') if e in ('fuse', 'fs3', 'ps3') else None)


GRID_SIDES_KP = [(-10, 200, 0, 0), (645, 300, 0, 0), (300, -8, 0, 0), (400, 480, 0, 0)]
F7_ROWS = [(314 + 2 * (k % 7), 234 + 2 * (k // 7), 0, k) for k in range(48)]


def _p():
    L1 = mg.CASE['L1_frustum']['lm']
    band = [lp(L1['xw'][i], min_dist=L1['min_dist'][i], max_dist=L1['max_dist'][i]) for i in (10, 11, 12, 13)]
    lv3 = lp((4, 1, 8), max_dist=f32(14.4))               # dist 9, ratio 1.6: level 3, projects to (256, 64)
    out = [
        # depth: z < 0 (would land on keypoint 0 were the sign ignored), z = 0 (u = +inf), z = -0.0 (not `< 0`: u = -inf, refused by the bounds).  The relocalisation
        # matcher has no depth test at all (ORBmatcher.cc:1499-1512): it projects the point behind the camera and matches it.
        p_case('P_depth', [(128, 128, 0, 0), (320, 240, 0, 0)], [lp((-0.5, -0.5, -2)), lp((0.5, 0.5, 0.0)), lp((0.5, 0.5, -0.0)), lp(at(320, 240))],
               dict(A=[-1, -1, -1, 1], pkf=[0, -1, -1, 1], bys=[-1, -1, -1, 1]), dist=[0]),
        # image bounds: KeyFrame::IsInImage is half-open (u == maxX and v == maxY are outside), the relocalisation matcher's test is closed
        p_case('P_bounds', [(-9.5, 100, 0, 0), (-9.5, 140, 0, 0), (645, 100, 0, 0), (645, 140, 0, 0), (645, 180, 0, 0), (200, -6, 0, 0), (240, -6, 0, 0), (200, 480, 0, 0), (240, 480, 0, 0),
                            (280, 480, 0, 0)],
               [lp(at(X0, 100)), lp(at(below(X0), 140)), lp(at(X1, 100)), lp(at(below(X1), 140)), lp(at(above(X1), 180)), lp(at(200, Y0)), lp(at(240, below(Y0))), lp(at(200, Y1)),
                lp(at(240, below(Y1))), lp(at(280, above(Y1)))],
               dict(A=[0, -1, -1, 3, -1, 5, -1, -1, 8, -1], pkf=[0, -1, 2, 3, -1, 5, -1, 7, 8, -1], bys=[0, -1, -1, 3, -1, 5, -1, -1, 8, -1]), dist=[0] * 4),
        # distance band: dist == 0.8f * min_dist and == 1.2f * max_dist are kept, one float beyond is not (the points of match_gate_cases' L1)
        p_case('P_band', [(0, 318.5, 0, 0), (318.5, 0, 0, 0), (384, 0, 0, 0), (0, 384, 0, 0)], band, dict(A=[0, -1, 2, -1], pkf=[0, -1, 2, -1], bys=[0, -1, 2, -1]), dist=[0, 0]),
        # viewing angle: dot == 0.5 * dist is kept, the float below is not; SearchBySim3 and the relocalisation matcher have no such gate
        p_case('P_angle', [(0, 0, 0, 0), (0, 0, 0, 30)], [lp((0, 0, 2), normal=(0, 0, 0.5)), lp((0, 0, 2), normal=(0, 0, inward(0.5)), n=30)],
               dict(A=[0, -1], pkf=[0, 1], bys=[0, 1]), dist=[0]),
        # level clamp at nlevels - 1: ratio 10 predicts level 13; 8 levels admit octaves 6, 7 (7, 8 for the relocalisation matcher), 12 levels 10, 11
        p_case('P_clamp_8', [(0, 0, 5, 0), (0, 0, 6, 10), (0, 0, 7, 20)], [lp((0, 0, 2), max_dist=20.0)], dict(A=[1], pkf=[1], bys=[1]), th=1, dist=[10]),
        p_case('P_clamp_12', [(0, 0, 9, 0), (0, 0, 10, 10), (0, 0, 11, 20)], [lp((0, 0, 2), max_dist=20.0)], dict(A=[1], pkf=[1], bys=[1]), th=1, dist=[10], sf=scales(12)),
        # level clamp at 0: at the band's equality dist = 1.2f * max_dist the ratio can fall one float short of fl(1 / 1.2f) = 0.8333333.  max_dist = 1.75 gives dist = 2.1000001,
        # ratio 0.83333325 and logf(ratio) / logf(1.2f) = -1.0000002: ceilf says -1, clamped to 0.  The radius is th * scale[0] and the window [-1, 0] ([-1, 1] for the
        # relocalisation matcher, which takes the nearer keypoint at octave 1).  Unclamped, the radius would come from scale[-1] and the window [-2, -1] holds no keypoint.
        p_case('P_clamp0_8', [(0, 0, 1, 0), (0, 0, 0, 10)], [lp((0, 0, CLAMP0_Z), max_dist=1.75)], dict(A=[1], pkf=[0], bys=[1]), th=1, dist=[10]),
        p_case('P_clamp0_12', [(0, 0, 1, 0), (0, 0, 0, 10)], [lp((0, 0, CLAMP0_Z), max_dist=1.75)], dict(A=[1], pkf=[0], bys=[1]), th=1, dist=[10], sf=scales(12)),
        # level window: [l - 1, l] everywhere but in the relocalisation matcher, which takes [l - 1, l + 1]
        p_case('P_window', [(256, 64, 1, 0), (256, 64, 2, 10), (256, 64, 3, 20), (256, 64, 4, 5), (256, 64, 5, 1)], [lv3], dict(A=[1], pkf=[3], bys=[1]), th=1, dist=[10]),
        # radius: |dx| == r and |dy| == r are outside, one float nearer is inside; (14, 14) is inside a square window of 15
        p_case('P_radius', [(115, 100, 0, 0), (inward(115), 160, 0, 0), (200, 115, 0, 0), (260, inward(115), 0, 0), (414, 114, 0, 0)],
               [lp(at(100, 100)), lp(at(100, 160)), lp(at(200, 100)), lp(at(260, 100)), lp(at(400, 100))], dict(A=[-1, 1, -1, 3, 4], pkf=[-1, 1, -1, 3, 4], bys=[-1, 1, -1, 3, 4]), dist=[0] * 3),
        # grid: keypoints 0, 2, 4 round into column 64, row 48, column -1 and belong to no cell, although each has the smallest distance in its window
        p_case('P_grid', mg.F3_KP, [lp(at(648, 200)), lp(at(300, 483)), lp(at(-10, 300))], dict(A=[1, 3, 5], pkf=[1, 3, 5], bys=[1, 3, 5]), dist=[10, 12, 14]),
        # a radius of 700: the cell window is clipped on all four sides
        p_case('P_grid_clipped', mg.F3_KP, [lp(at(320, 240)), lp(at(320, 240), n=20)], dict(A=[1, 5], pkf=[1, 5], bys=[1, 5]), th=700, dist=[10, 6]),
        # one side at a time (radius 15): the window of point 0 reaches past column 0, of point 1 past column 63, of point 2 past row 0, of point 3 past row 47, and the
        # only keypoint of each sits in that last column or row
        p_case('P_grid_sides', GRID_SIDES_KP, [lp(at(-5, 200)), lp(at(648, 300)), lp(at(300, -3)), lp(at(400, 484))], dict(A=[0, 1, 2, 3], pkf=[0, 1, 2, 3], bys=[0, 1, 2, 3]),
               dist=[0] * 4, cells={0: (0, None), 1: (63, None), 2: (None, 0), 3: (None, 47)}),
        # Fuse's chi^2 with the KEYPOINT's level: point 0 (level 2) sees octave 1 (e2 * M_IN kept) and octave 2 (e2 * M_OUT refused); point 1 (level 4) the stereo limit with
        # octaves 3 (C_IN) and 4 (C_OUT); point 2: er = -2 gives 6 (over 5.99, under 7.8: kept as stereo), er = -2.5 gives 8.25, a monocular 6.25 is refused; point 3: uright == 0
        # is stereo (er = 32), the monocular neighbour is taken
        p_case('P_chi2', [(101, 100, 1, 10), (101, 100, 2, 0), (201, 100, 3, 10, 184), (201, 100, 4, 0, 184), (301, 101, 0, 10, 286), (301, 101, 0, 0, 286.5), (302, 101.5, 0, 0),
                          (48, 100, 0, 0, 0), (49, 100, 0, 10)],
               [lp(at(100, 100), ratio=1.3), lp(at(200, 100), ratio=1.9), lp(at(300, 100)), lp(at(48, 100))], dict(fuse=[0, 2, 4, 8]), th=3, dist=[10] * 4, is2=IS2_CHI),
        # acceptance: TH_LOW = 50 in the Fuse entries and project_sim3, ORBdist (64 here) in the relocalisation matcher, TH_HIGH = 100 in SearchBySim3
        p_case('P_accept', [(100, 300, 0, 50), (200, 300, 0, 51), (300, 300, 0, 64), (400, 300, 0, 65), (100, 400, 0, 100), (200, 400, 0, 101)],
               [lp(at(100, 300)), lp(at(200, 300)), lp(at(300, 300)), lp(at(400, 300)), lp(at(100, 400)), lp(at(200, 400))],
               dict(A=[0, -1, -1, -1, -1, -1], pkf=[0, 1, 2, -1, -1, -1], bys=[0, 1, 2, 3, 4, -1]), od=64, dist=[50]),
        # scan-order ties at distance 7: the lower grid column, then the lower row, then the lower index (cells as in match_gate_cases' F5)
        p_case('P_ties', [(206, 200, 0, 7), (198, 206, 0, 7), (300, 206, 0, 7), (300, 200, 0, 7), (402, 301, 0, 7), (400, 299, 0, 7)], [lp(at(202, 203)), lp(at(300, 203)), lp(at(401, 300))],
               dict(A=[1, 3, 4], pkf=[1, 3, 4], bys=[1, 3, 4]), dist=[7] * 3, cells={0: (21, 20), 1: (20, 21), 2: (30, 21), 3: (30, 20), 4: (40, 30), 5: (40, 30)}),
        # locks on entry: keypoint 0 is taken (vpMatched / a map point of the frame); the Fuse entries know no such thing
        p_case('P_taken', [(100, 100, 0, 0), (100, 100, 0, 10)], [lp(at(100, 100))], dict(fuse=[0], fs3=[0], ps3=[1], pkf=[1]), taken=[1, 0], dist=[0]),
        # a chain: 48 identical points; point i finds keypoints 0..i-1 taken and takes keypoint i (48 sweeps).  The Fuse entries give all of them keypoint 0.
        p_case('P_chain', F7_ROWS, [lp(at(320, 240)) for _ in range(48)], dict(fuse=[0] * 48, fs3=[0] * 48, ps3=list(range(48)), pkf=list(range(48))), dist=[0] * 48),
    ]
    # Scw = s [R | t]: the scale is the norm of ROW 0 of the rotation block.  Rows 1 and 2 carry twice that norm here: divided by row 0's 2, R = diag(1, 2, 2), t = (1, 0, 0),
    # Ow = (-1, 0, 0), the point lands on (128, 64) with dist 1.1319 >= 0.8f * 1.35.  Divided by 4, Ow = (-0.25, 0, 0) and dist 1.0383 falls below the band.
    out.append(p_case('P_scw_row0', [(128, 64, 0, 0)], [lp((-0.5, 0.125, 1), min_dist=1.35, max_dist=1.0)], dict(fs3=[0], ps3=[0]), dist=[0],
                      Scw=[[2, 0, 0, 2], [0, 4, 0, 0], [0, 0, 4, 0], [0, 0, 0, 1]]))
    # s = 2 and 0.5 with R = RZ, t = (0.25, 0, 0): (0.25, -0.25, 2) goes to (0.5, 0.25, 2) = (128, 64); through RZ' it would go to (0, -0.25, 2), outside the image.  With the scale
    # left in, Ow = (0, 1, 0) or (0, 0.0625, 0) instead of (0, 0.25, 0), and the distance 2.0767 becomes 2.3717 (beyond 1.2f * 1.87) or 2.0396 (below 0.8f * 2.575)
    for s in (2.0, 0.5):
        S = np.eye(4, dtype='f4'); S[:3, :3] = RZ * f32(s); S[0, 3] = 0.25 * s
        out.append(p_case('P_scw_rot_%g' % s, [(128, 64, 0, 0)], [lp((0.25, -0.25, 2), min_dist=2.575, max_dist=1.87)], dict(fs3=[0], ps3=[0]), dist=[0], Scw=S))
    return out


def bys_sides(c):
    """search_by_sim3 on a P case under the identity Sim3 (both poses the identity, s12 = 1): side 1's keypoint i carries point i, side 2 is the case's keypoints.  For the
    agreement, the side-2 keypoint that want['bys'] gives to point i carries the same point, and side 1's keypoint i is a copy of it (same place and octave, a descriptor of
    its own that side 2's point repeats); unmatched side-1 keypoints sit in a corner of their own."""
    w = c['want']['bys']; P = c['P']; K = c['K']; n1 = len(w); n2 = len(K['keys'])
    k1 = np.zeros(n1, KP_DTYPE); k1['size'] = 31; k1['class_id'] = -1; d1 = np.zeros((n1, 32), np.uint8)
    ok2 = np.zeros(n2, np.uint8); xw2 = np.zeros((n2, 3), 'f4'); mn2 = np.ones(n2, 'f4'); mx2 = np.ones(n2, 'f4'); md2 = np.zeros((n2, 32), np.uint8)
    for i, k in enumerate(w):
        d1[i] = desc(120 + i)
        if k < 0: k1['x'][i], k1['y'][i] = 600 + i, 450; continue
        k1[i] = K['keys'][k]; ok2[k] = 1; xw2[k] = P['xw'][i]; mn2[k] = P['min_dist'][i]; mx2[k] = P['max_dist'][i]; md2[k] = d1[i]
    kf1 = dict(keys=k1, desc=d1, Tcw=I4, mp_ok=(1 - P['skip']).astype(np.uint8), xw=P['xw'], min_dist=P['min_dist'], max_dist=P['max_dist'], mp_desc=P['desc'])
    kf2 = dict(keys=K['keys'], desc=K['desc'], Tcw=I4, mp_ok=ok2, xw=xw2, min_dist=mn2, max_dist=mx2, mp_desc=md2)
    return kf1, kf2


# ===================================================================================================================== S: SearchBySim3's own rules
def sim_side(rows, pts):
    """rows: keypoints (x, y, octave, bits); pts[i]: None or (xyz, min_dist, max_dist, bits of the map point's descriptor)"""
    k = cur_of(rows); n = len(rows)
    return dict(keys=k['keys'], desc=k['desc'], Tcw=I4, mp_ok=np.array([p is not None for p in pts], np.uint8), xw=np.array([(0, 0, 1) if p is None else p[0] for p in pts], 'f4').reshape(n, 3),
                min_dist=np.array([1 if p is None else p[1] for p in pts], 'f4'), max_dist=np.array([1 if p is None else p[2] for p in pts], 'f4'),
                mp_desc=np.array([desc(0 if p is None else p[3]) for p in pts], np.uint8).reshape(n, 32))


def sim_case(name, kf1, kf2, m0, want, s12=1.0, R12=np.eye(3, dtype='f4'), t12=(0, 0, 0), th=15):
    return dict(name=name, kind='sim', kf1=kf1, kf2=kf2, m0=np.array(m0, 'i4'), s12=s12, R12=np.array(R12, 'f4'), t12=np.array(t12, 'f4'), th=th, want=want)


def _s():
    xs = [100, 160, 220, 280, 340, 400]
    p = lambda x: (at(x, 100), 0.1, f32(0.9) * norm3(at(x, 100)), 0)          # level 0
    k1 = sim_side([(x, 100, 0, 0) for x in xs[:5]] + [(400, 100, 0, 10), (402, 100, 0, 0)], [p(x) for x in xs[:5]] + [p(400)[:3] + (20,), None])
    k2 = sim_side([(x, 100, 0, 0) for x in xs[:5]] + [(400, 100, 0, 20)], [p(x) for x in xs])
    # 0 free and mutual: found.  1 came in as -2 (matched to a point side 2 does not observe): left alone.  2 came in matched to keypoint 2: left alone.  3 is free and finds
    # keypoint 3, but that one is occupied by 4's earlier match, so its point is not projected back: dropped.  5 finds keypoint 5 (descriptor 20), whose point (descriptor 0)
    # prefers side 1's keypoint 6 over 5 (descriptor 10): one-sided, dropped.
    out = [sim_case('S_prior', k1, k2, [-1, -2, 2, -1, 3, -1, -1], (1, [0, -2, 2, -1, 3, -1, -1]))]
    # R12 = RZ, t12 = (0.5, 0.25, 0), s12 = 1: side 1's point (0.25, 1, 2) is RZ' ((0.25, 1, 2) - t12) = (0.75, 0.25, 2) in camera 2: (192, 64); back, RZ (0.75, 0.25, 2) + t12 lands
    # on (64, 256).  RZ for RZ', or t12 for t21 = -RZ' t12, put it outside the image.
    out.append(sim_case('S_rot', sim_side([(64, 256, 0, 0)], [((0.25, 1.0, 2), 0.1, 1.94, 0)]), sim_side([(192, 64, 0, 0)], [((0.75, 0.25, 2), 0.1, 2.03, 0)]), [-1], (1, [0]),
                        R12=RZ, t12=(0.5, 0.25, 0)))
    # the distance is |p3Dc| in the TARGET camera: s12 = 2 halves side 1's point (0, 1, 4) to (0.5, 0, 2), 2.06 away, inside [0.8f * 0.1, 1.2f * 1.86]; its distance from the
    # camera centre, 4.12, is not.  Back: (0.5, 0, 2) doubles to (0, 1, 4), 4.12 inside [0.8f * 3, 1.2f * 3.72]; 2.06 is not.  s12 = 0.5 likewise.
    out.append(sim_case('S_scale_2', sim_side([(0, 128, 0, 0)], [((0, 1, 4), 0.1, 1.86, 0)]), sim_side([(128, 0, 0, 0)], [((0.5, 0, 2), 3.0, 3.72, 0)]), [-1], (1, [0]), s12=2.0, R12=RZ))
    out.append(sim_case('S_scale_0.5', sim_side([(0, 128, 0, 0)], [((0, 0.25, 1), 2.0, 2.0, 0)]), sim_side([(128, 0, 0, 0)], [((0.5, 0, 2), 0.1, 0.93, 0)]), [-1], (1, [0]), s12=0.5, R12=RZ))
    return out


# ===================================================================================================================== I: SearchForInitialization
def init_case(name, r1, r2, want_m, want_pm, pm=None, window=10, ratio=0.9, ori=0):
    """rows (x, y, octave, bits[, angle]); pm: {index: (x, y)} where vbPrevMatched is not the keypoint's own place; want_pm: {index: (x, y)} of the entries that change"""
    a = cur_of([(r[0], r[1], r[2], r[3], -1, r[4] if len(r) > 4 else 0.0) for r in r1]); b = cur_of([(r[0], r[1], r[2], r[3], -1, r[4] if len(r) > 4 else 0.0) for r in r2])
    pm0 = np.stack([a['keys']['x'], a['keys']['y']], 1).astype('f4')
    for i, xy in (pm or {}).items(): pm0[i] = xy
    wpm = pm0.copy()
    for i, xy in want_pm.items(): wpm[i] = xy
    return dict(name=name, kind='init', F1=dict(keys=a['keys'], desc=a['desc']), F2=dict(keys=b['keys'], desc=b['desc']), pm=pm0, window=window, ratio=ratio, ori=ori,
                want=(sum(m >= 0 for m in want_m), want_m, wpm))


I_1 = [(50, 50, 1, 0),                                     # 0   octave 1: not searched, though keypoint 0 of frame 2 is its twin
       (100, 50, 0, 0),                                    # 1   takes 2 (octave 0, distance 20), not 1 (octave 1, distance 0)
       (150, 50, 0, 0), (200, 50, 0, 0),                   # 2, 3  the window is strict: |dx| == 10 and |dy| == 10 are outside
       (250, 50, 0, 10), (250, 50, 0, 10),                 # 4, 5  an equal distance does not steal
       (300, 50, 0, 30), (300, 50, 0, 20), (300, 50, 0, 10),          # 6, 7, 8  a steal chain: 30, then 20, then 10
       (350, 50, 0, 0), (400, 50, 0, 0),                   # 9, 10  TH_LOW: 50 accepted, 51 not
       (450, 50, 0, 0), (500, 50, 0, 0),                   # 11, 12  ratio 0.9f: 9 < 9.0f is false, 8 < 9.0f
       (550, 50, 0, 0), (600, 50, 0, 0)]                   # 13, 14  windows off the grid, right and left
I_2 = [(50, 50, 0, 0), (100, 50, 1, 0), (102, 50, 0, 20), (160, 50, 0, 0), (inward(160), 50, 0, 20), (200, 60, 0, 0), (200, inward(60), 0, 20),          # 0-6
       (250, 50, 0, 0), (300, 50, 0, 0), (350, 50, 0, 50), (400, 50, 0, 51), (450, 50, 0, 9), (450, 50, 0, 10), (500, 50, 0, 8), (500, 50, 0, 10),       # 7-14
       (550, 50, 0, 0), (600, 50, 0, 0)]                   # 15, 16: the twins of 13 and 14, which look elsewhere
I_WANT = [-1, 2, 4, 6, 7, -1, -1, -1, 8, 9, -1, -1, 13, -1, -1]
I_PM = {1: (102, 50), 2: (inward(160), 50), 3: (200, inward(60)), 8: (300, 50)}      # 4, 9 and 12 are matched to keypoints at their own place
# stale histogram counts: keypoints 0, 1 (rot 240, bin 20) are matched first and then robbed by 2, 3 (rot 60, bin 5).  rotHist keeps them: bin 20 counts 2 stale + 2 live = 4,
# bin 5 has 3, bin 9 two, bin 12 two.  The maxima are 20, 5, 9 and bin 12 (keypoints 7, 8) goes.  Counting live matches only, bins 5, 9, 12 would stay and bin 20 (9, 10) go.
I_H1 = [(100, 100, 0, 30, 240), (160, 100, 0, 30, 240), (100, 100, 0, 10, 60), (160, 100, 0, 10, 60), (220, 100, 0, 0, 60), (280, 100, 0, 0, 108), (340, 100, 0, 0, 108),
        (400, 100, 0, 0, 144), (460, 100, 0, 0, 144), (520, 100, 0, 0, 240), (580, 100, 0, 0, 240)]
I_H2 = [(x, 100, 0, 0, 0) for x in (100, 160, 220, 280, 340, 400, 460, 520, 580)]
I_HWANT = [-1, -1, 0, 1, 2, 3, 4, -1, -1, 7, 8]


def _i():
    # keypoint 6 looks from (301, 50): it is matched to (300, 50), robbed, and keeps (301, 50): vbPrevMatched moves for survivors only
    return [init_case('I_gates', I_1, I_2, I_WANT, I_PM, pm={6: (301, 50), 13: (5000, 50), 14: (-500, 50)}),
            init_case('I_stale_hist', I_H1, I_H2, I_HWANT, {}, ori=1),
            init_case('I_stale_hist_ori0', I_H1, I_H2, [-1, -1, 0, 1, 2, 3, 4, 5, 6, 7, 8], {}, ori=0)]


# ===================================================================================================================== N: new map points
# fx = fy = 512, cx = cy = 0, bf = 32 (mb = 1/16), ratioFactor = 1.5f * 1.2f = 1.8, sigma2 = 1.44^k.  Keyframe 1 at the identity, keyframe 2 at Ow2 = (b, 0, 0).
# The point (0.5, 0.25, 2) is (128, 64) in keyframe 1 and (128 - 256 b, 64) in keyframe 2.  A stereo keypoint with depth 2 has cosParallaxStereo = cos(2 atan2(1/32, 2)) = 0.99951.
#   b = 0.5:  rays (0.25, 0.125, 1) and (0, 0.125, 1), cosParallaxRays = 0.9706: below 0.99951 and 0.9998, the SVD branch whether stereo or not.
#   b = 1/64: cosParallaxRays = 0.99997: above both, so a stereo side is unprojected and a monocular pair is dropped.
# keys (mvKeys) differ from keys_un (mvKeysUn) by whole pixels: UnprojectStereo reads mvKeys (KeyFrame.cc:635-636), every other line reads mvKeysUn.
def np_side(rows, ow, shift=(0, 0)):
    """rows (x, y, octave, uright, depth) of keys_un; keys = keys_un + shift; the camera centre is (ow[0], 0, ow[1]), the rotation the identity"""
    k = cur_of([(r[0], r[1], r[2], 0) for r in rows])['keys']; kd = k.copy(); kd['x'] += shift[0]; kd['y'] += shift[1]
    T = I4.copy(); T[0, 3] = -ow[0]; T[2, 3] = -ow[1]
    return dict(keys_un=k, keys=kd, uright=np.array([r[3] for r in rows], 'f4'), depth=np.array([r[4] for r in rows], 'f4'), Tcw=T)


def np_case(name, r1, r2, ow2, want_ok, want_x=None, shift1=(0, 0), shift2=(0, 0), ow1=(0.0, 0.0), branch=None, relax=None):
    """relax[q]: what to replace in the refused pair q (1 / 2: the row of that side; 'ow1' / 'ow2': that camera centre) so that the gate it is for lets it pass"""
    n = len(r1)
    return dict(name=name, kind='newpts', pairs=np.stack([np.arange(n), np.arange(n)], 1).astype('i4'), kf1=np_side(r1, ow1, shift1), kf2=np_side(r2, ow2, shift2), want_ok=want_ok,
                want_x=want_x or {}, branch=branch or {}, relax=relax or {}, made=dict(r1=r1, r2=r2, ow1=ow1, ow2=ow2, shift1=shift1, shift2=shift2))


def np_relaxed(c, q):
    """the case with the refused pair q relaxed as c['relax'][q] says"""
    m = dict(c['made']); m['r1'] = list(m['r1']); m['r2'] = list(m['r2'])
    for what, v in c['relax'][q].items():
        if what in (1, 2): m['r%d' % what][q] = v
        else: m[what] = v
    return np_case(c['name'] + '_relaxed_%d' % q, m['r1'], m['r2'], m['ow2'], None, shift1=m['shift1'], shift2=m['shift2'], ow1=m['ow1'])


def _n():
    M = (-1, -1)                                           # monocular: uright, depth
    a = np_case('N_wide',
                [(128, 64, 0) + M, (128, 64, 0, 112, 2), (1024, 0, 0) + M, (-128, 0, 0) + M],
                [(0, 64, 0) + M, (0, 64, 0) + M, (-512, 0, 0) + M, (128, 0, 0) + M], (0.5, 0),
                # 0 SVD, two monocular keypoints.  1 SVD chosen over stereo.  2 rays (2, 0, 1) and (-1, 0, 1): cosParallaxRays = -0.32 <= 0, although they meet at (1/3, 0, 1/6), in
                # front of both cameras and with no reprojection error: only the parallax test refuses it.  With keypoint 2 at (896, 0) the rays meet at (4, 0, 2), cos 0.9985.
                # 3 rays (-0.25, 0, 1) from the origin and (0.25, 0, 1) from (0.5, 0, 0) meet at (0.25, 0, -1): behind both cameras (either depth test refuses it; N_behind_1
                # and N_behind_2 have one each).  With the keypoints exchanged they meet at (0.25, 0, 1).
                [1, 1, 0, 0], branch={0: 'svd', 1: 'svd'}, relax={2: {2: (896, 0, 0) + M}, 3: {1: (128, 0, 0) + M, 2: (-128, 0, 0) + M}})
    # keyframe 1's mvKeys are 3 px right of mvKeysUn, keyframe 2's 2 px below
    b_r1 = [(128, 64, 4, 112, 2),                          # 0  side 1 unprojected from mvKeys (131, 64): (0.51171875, 0.25, 2); errors 9 + 9 (u1_r 115 against 112) < 7.8 * 4.3
            (128, 64, 4) + M,                              # 1  side 2 unprojected from mvKeys (124, 66): (0.484375, 0.2578125, 2) + Ow2 = (0.5, 0.2578125, 2)
            (128, 64, 0) + M]                              # 2  monocular pair, cosParallaxRays 0.99997 >= 0.9998: neither.  At a disparity of 16 px (depth 0.5) cos is 0.9996
    b_r2 = [(124, 64, 4) + M, (124, 64, 4, 108, 2), (124, 64, 0) + M]
    b = np_case('N_narrow_shifted', b_r1, b_r2, (1 / 64, 0), [1, 1, 0], {0: (0.51171875, 0.25, 2.0), 1: (0.5, 0.2578125, 2.0)}, shift1=(3, 0), shift2=(0, 2),
                branch={0: 'unproject1', 1: 'unproject2'}, relax={2: {2: (112, 64, 0) + M}})
    # chi^2, keys == keys_un, b = 1/64, the unprojected point is (0.5, 0.25, 2) = (128, 64) / (124, 64) exactly.  Each limit with the judged side at octave 0 (sigma2 1: refused)
    # and at octave 1 (1.44: kept); the OTHER side, whose error is 0, has the other octave of the two, so the sigma2 of the wrong side gives the opposite answer.
    c_r1 = [(128, 64, 0, 109, 2), (128, 64, 1, 109, 2),    # 0, 1  stereo side 1: errX1_r = 112 - 109 = 3, 9 > 7.8, 9 < 11.23
            (128, 64, 1, 112, 2), (128, 64, 0, 112, 2),    # 2, 3  monocular side 2 at (126, 65.5): 4 + 2.25 = 6.25 > 5.991, < 8.63
            (130, 65.5, 0) + M, (130, 65.5, 1) + M,        # 4, 5  monocular side 1 at (130, 65.5), the point comes from side 2
            (128, 64, 1) + M, (128, 64, 0) + M]            # 6, 7  stereo side 2: errX2_r = 108 - 105 = 3
    c_r2 = [(124, 64, 1) + M, (124, 64, 0) + M, (126, 65.5, 0) + M, (126, 65.5, 1) + M, (124, 64, 1, 108, 2), (124, 64, 0, 108, 2), (124, 64, 0, 105, 2), (124, 64, 1, 105, 2)]
    c = np_case('N_narrow_gates', c_r1, c_r2, (1 / 64, 0), [0, 1, 0, 1, 0, 1, 0, 1], {1: (0.5, 0.25, 2.0), 3: (0.5, 0.25, 2.0), 5: (0.5, 0.25, 2.0), 7: (0.5, 0.25, 2.0)},
                branch={1: 'unproject1', 3: 'unproject1', 5: 'unproject2', 7: 'unproject2'},
                relax={0: {1: (128, 64, 0, 112, 2)}, 2: {2: (124, 64, 0) + M}, 4: {1: (128, 64, 0) + M}, 6: {2: (124, 64, 0, 108, 2)}})     # the error taken away, the octaves kept
    # the scale ratio: keyframe 2 sits on keypoint 1's ray at a quarter of the way to the point (0.5, 0, 2), which it sees at (128, 0) too: cosParallaxRays = 1, side 1 is
    # unprojected, no reprojection error, ratioDist = dist2 / dist1 = 0.75 and ratioFactor = 1.8.  ratioOctave = scale[octave 1] / scale[octave 2]:
    #   0  octaves 2, 0: 0.75 * 1.8 = 1.35 < 1.44: refused by the first bound      1  octaves 1, 0: 1.35 > 1.2: kept
    #   2  octaves 0, 5: 0.75 > 0.4019 * 1.8 = 0.7234: refused by the second bound  3  octaves 0, 4: 0.75 < 0.4823 * 1.8 = 0.868: kept
    # With the ratio inverted (1 / 1.44 and 2.488) pairs 0 and 2 would change bounds: 0 passes both, 2 fails the first.
    s_r1 = [(128, 0, 2, 112, 2), (128, 0, 1, 112, 2), (128, 0, 0, 112, 2), (128, 0, 0, 112, 2)]
    s_r2 = [(128, 0, 0) + M, (128, 0, 0) + M, (128, 0, 5) + M, (128, 0, 4) + M]
    s = np_case('N_scale', s_r1, s_r2, (0.125, 0.5), [0, 1, 0, 1], {1: (0.5, 0.0, 2.0), 3: (0.5, 0.0, 2.0)}, branch={1: 'unproject1', 3: 'unproject1'},
                relax={0: {1: (128, 0, 1, 112, 2)}, 2: {2: (128, 0, 4) + M}})
    # z2 <= 0 alone: keyframe 2 sits on keypoint 1's ray BEYOND the point, at 1.5 (0.5, 0, 2) = (0.75, 0, 3), looking the same way.  Side 1 is unprojected (cosParallaxRays = 1)
    # to (0.5, 0, 2): z1 = 2, z2 = -1, and the point projects to (-0.25 / -1, 0) = (128, 0), on keypoint 2, so chi^2 has nothing to refuse; ratioDist = 0.5 against
    # ratioOctave 1 / 1.728 passes both bounds.  Mirrored to 0.5 (0.5, 0, 2) the camera sees the same keypoint at the same distance with z2 = +1.
    d = np_case('N_behind_2', [(128, 0, 0, 112, 2)], [(128, 0, 3) + M], (0.75, 3), [0], relax={0: {'ow2': (0.25, 1)}})
    # z1 <= 0 alone: the same with the sides exchanged; side 2 (at the origin) is unprojected, z1 = -1, ratioDist = 2 against ratioOctave 1.728
    e = np_case('N_behind_1', [(128, 0, 3) + M], [(128, 0, 0, 112, 2)], (0, 0), [0], ow1=(0.75, 3), relax={0: {'ow1': (0.25, 1)}})
    return [a, b, c, s, d, e]


# ===================================================================================================================== Z: sizes (oracle only)
def _flip_rows(rng, d, kmax): return mg._flip(rng, d, kmax)


def z_nodes(nn, seed):
    """nn common vocabulary nodes, 1 or 2 keypoints of each keyframe in every node, keypoint order shuffled.  (The ORB vocabulary at levelsup = 4 gives about 100 nodes per
    keyframe: this is the entry's contract, not the workload.)"""
    rng = np.random.default_rng(seed); sides = []
    base = mg._rand_desc(rng, nn)
    for s in (0, 1):
        node = np.concatenate([np.arange(nn), np.arange(nn)[(np.arange(nn) >> s) % 2 == 1]]); p = rng.permutation(len(node)); node = node[p]; n = len(node)
        k = np.zeros(n, KP_DTYPE); k['x'] = 20 + (node % 30) * 20 + rng.uniform(-3, 3, n); k['y'] = 20 + (node // 30) * 20 + rng.normal(0, 0.6, n); k['octave'] = rng.integers(0, 4, n)
        k['angle'] = np.array([0, 0, 0, 90, 90, 180, 270], 'f4')[node % 7] if s else 0; k['size'] = 31; k['class_id'] = -1          # rot 0, 270, 180, 90: four bins, 180 and 90 tie for third place
        d = _flip_rows(rng, base[node], 22); ur = np.where(rng.random(n) < 0.5, k['x'] - 10, -1).astype('f4'); has = (rng.random(n) < 0.1).astype(np.uint8); good = (rng.random(n) < 0.9).astype(np.uint8)
        last = np.flatnonzero(node == nn - 1)              # the last node matches for sure: on one line, stereo, free, descriptors 0 and 30 bits from the node's
        k['y'][last] = 20 + ((nn - 1) // 30) * 20; ur[last] = k['x'][last] - 10; has[last] = 0; good[last] = 1
        for j, i in enumerate(last): b = np.unpackbits(base[nn - 1]); b[:30 * j * s] ^= 1; d[i] = np.packbits(b)
        sides.append(dict(keys=k, desc=d, uright=ur, has_mp=has, good_mp=good, feat_node=(node * 3 + 5).astype('i4'), Tcw=I4.copy(), cam_center=np.array([0.5, 0.25, 2], 'f4')))
    return sides


def z_proj(nk, nm, seed):
    """nk keypoints on a lattice, nm points each projecting within 2 px of one of them with a descriptor at most 25 bits away, at the level of the keypoint's octave"""
    rng = np.random.default_rng(seed)
    x, y = mg._lattice(rng, nk); k = np.zeros(nk, KP_DTYPE); k['x'] = x; k['y'] = y; k['octave'] = rng.integers(0, 3, nk); k['size'] = 31; k['class_id'] = -1; k['angle'] = rng.uniform(0, 360, nk)
    kd = mg._rand_desc(rng, nk)
    t = np.concatenate([rng.permutation(nk), rng.integers(0, nk, max(nm - nk, 0))])[:nm]; t[t == nk - 1] = 0; t[-1] = nk - 1          # the last point alone looks at the last keypoint
    xw = np.stack([(k['x'][t] + rng.uniform(-2, 2, nm)) / 256, (k['y'][t] + rng.uniform(-2, 2, nm)) / 256, np.full(nm, 2.0)], 1).astype('f4')
    xw[-1, :2] = k['x'][t[-1]] / f32(256), k['y'][t[-1]] / f32(256)                       # the last point sits on its keypoint, with its descriptor, and is not skipped
    dist = np.linalg.norm(xw.astype('f8'), axis=1)
    pd = _flip_rows(rng, kd[t], 25); pd[-1] = kd[t[-1]]; skip = (rng.random(nm) < 0.05).astype(np.uint8); skip[-1] = 0
    P = dict(xw=xw, normal=np.tile(np.array([0, 0, 1], 'f4'), (nm, 1)), min_dist=np.full(nm, 0.1, 'f4'), max_dist=(dist * 1.2 ** (k['octave'][t] - 0.5)).astype('f4'),
             desc=pd, skip=skip)
    K = dict(keys=k, desc=kd, uright=np.where(rng.random(nk) < 0.5, k['x'] - 16, -1).astype('f4'))
    taken = (rng.random(nk) < 0.1).astype(np.uint8); taken[-1] = 0
    return K, P, taken


def z_init(seed=3):
    """300 keypoints of frame 2 in grid column 11 (x in [100, 104]), all octaves; frame 1's level-0 keypoints look at (102, 230) with a window of 250.  Frame-2 keypoints 3 and
    297 (octave 0) tie at distance 5 from frame-1 keypoint 0; keypoint 1 of frame 1 is one bit nearer and steals"""
    rng = np.random.default_rng(seed); n = 300
    k2 = np.zeros(n, KP_DTYPE); k2['x'] = 100 + 4 * rng.random(n); k2['y'] = 20 + 1.4 * np.arange(n); k2['octave'] = np.arange(n) % 3; k2['size'] = 31; k2['class_id'] = -1
    d2 = np.array([desc(60 + j % 100) for j in range(n)], np.uint8); d2[3] = desc(5); d2[297] = desc(5)
    k1 = cur_of([(102, 230, 0, 0), (102, 230, 0, 1), (102, 230, 1, 0), (102, 230, 0, 118)])
    return dict(keys=k1['keys'], desc=k1['desc']), dict(keys=k2, desc=d2)


# ===================================================================================================================== the table
def _build():
    return _t() + _b() + _p() + _s() + _i() + _n()


CASES = _build()
CASE = {c['name']: c for c in CASES}
NAMES = [c['name'] for c in CASES]
assert len(CASE) == len(CASES)
assert all(len(c['K']['keys']) <= 48 and len(c['P']['xw']) <= 48 for c in CASES if c['kind'] == 'proj')


# ===================================================================================================================== running
def _invert(w, nk):
    """per-keypoint answer of the locked entries from the per-point one (a keypoint is given to one point)"""
    out = [-1] * nk
    for i, k in enumerate(w):
        if k >= 0: assert out[k] == -1; out[k] = i
    return out


def proj_runs(c):
    """(entry, expected answer, run(lib or oracle module)) for every entry the P case names"""
    K, P, th, sf = c['K'], c['P'], c['th'], c['sf']; nk = len(K['keys']); nm = len(P['xw']); out = []
    is_orc = lambda f: not hasattr(f, 'dll')
    for e in ENTRIES:
        w = want_for(c, e)
        if w is None: continue
        if e in ('fuse', 'fs3'):
            wd = iter(c['dist']); exp = (sum(k >= 0 for k in w), list(w), [next(wd) if k >= 0 else 256 for k in w])
        elif e == 'bys': exp = (sum(k >= 0 for k in w), list(w))
        else: exp = (sum(k >= 0 for k in w), _invert(w, nk))
        if e == 'fuse':
            kf = dict(keys=K['keys'], desc=K['desc'], uright=K['uright'], Tcw=I4)
            run = lambda f, kf=kf: f.fuse_search(kf, P, CAM, sf, c['is2'], th) if is_orc(f) else ORBmatcher(lib=f).FuseSearch(kf, P, th, CAM, sf, c['is2'])
        elif e == 'fs3':
            kf = dict(keys=K['keys'], desc=K['desc'])
            run = lambda f, kf=kf: f.fuse_search_sim3(kf, c['Scw'], P, CAM, sf, th) if is_orc(f) else ORBmatcher(lib=f).FuseSearchSim3(kf, c['Scw'], P, th, CAM, sf)
        elif e == 'ps3':
            kf = dict(keys=K['keys'], desc=K['desc'], matched=c['taken'])
            run = lambda f, kf=kf: f.search_by_projection_sim3(kf, c['Scw'], P, CAM, sf, th) if is_orc(f) else ORBmatcher(lib=f).SearchByProjectionSim3(kf, c['Scw'], P, th, CAM, sf)
        elif e == 'pkf':
            F = dict(keys=K['keys'], desc=K['desc'], has_mp=c['taken'], Tcw=I4); kk = np.zeros(nm, KP_DTYPE)
            kf = dict(keys=kk, ok=(1 - P['skip']).astype(np.uint8), xw=P['xw'], min_dist=P['min_dist'], max_dist=P['max_dist'], desc=P['desc'])
            run = lambda f, F=F, kf=kf: f.search_by_projection_kf(F, kf, CAM, sf, float(th), c['od'], False) if is_orc(f) else ORBmatcher(0.9, False, lib=f).SearchByProjectionKF(F, kf, float(th), c['od'], CAM, sf)
        else:
            k1, k2 = bys_sides(c); m0 = np.full(nm, -1, 'i4')
            run = lambda f, k1=k1, k2=k2, m0=m0: f.search_by_sim3(k1, k2, m0, 1.0, np.eye(3), np.zeros(3), float(th), CAM, sf) if is_orc(f) else ORBmatcher(lib=f).SearchBySim3(k1, k2, m0, 1.0, np.eye(3), np.zeros(3), float(th), CAM, sf)
        out.append((e, exp, run))
    return out


def runs(c):
    """[(label, hand-written answer or None, run(lib or oracle module))]"""
    is_orc = lambda f: not hasattr(f, 'dll'); k = c['kind']
    if k == 'proj': return proj_runs(c)
    if k == 'tri':
        return [('tri', c['want'], lambda f: f.search_for_triangulation(c['kf1'], c['kf2'], c['F12'], c['stereo'], CAM, c['sf'], c['sg'], check_ori=bool(c['ori'])) if is_orc(f)
                 else ORBmatcher(0.6, bool(c['ori']), lib=f).SearchForTriangulation(c['kf1'], c['kf2'], c['F12'], c['stereo'], CAM, c['sf'], c['sg']))]
    if k == 'bow':
        F = {x: c['F'][x] for x in ('keys', 'desc', 'feat_node')}
        return [('bow', c['want'], lambda f: f.search_by_bow(c['kf'], F, c['ratio'], bool(c['ori'])) if is_orc(f) else ORBmatcher(c['ratio'], bool(c['ori']), lib=f).SearchByBoW(c['kf'], F))]
    if k == 'bowkf':
        return [('bowkf', c['want'], lambda f: f.search_by_bow_kf(c['kf'], c['F'], c['ratio'], bool(c['ori'])) if is_orc(f) else ORBmatcher(c['ratio'], bool(c['ori']), lib=f).SearchByBoWKF(c['kf'], c['F']))]
    if k == 'sim':
        a = (c['kf1'], c['kf2'], c['m0'], c['s12'], c['R12'], c['t12'], float(c['th']), CAM, SF)
        return [('bys', c['want'], lambda f: f.search_by_sim3(*a) if is_orc(f) else ORBmatcher(lib=f).SearchBySim3(*a))]
    if k == 'init':
        return [('init', c['want'], lambda f: f.search_for_initialization(c['F1'], c['F2'], c['pm'], c['window'], CAM, c['ratio'], bool(c['ori'])) if is_orc(f)
                 else ORBmatcher(c['ratio'], bool(c['ori']), lib=f).SearchForInitialization(c['F1'], c['F2'], c['pm'], c['window'], CAM))]
    raise KeyError(k)


def same(got, want, what):
    assert len(got) == len(want), what
    for g, w in zip(got, want):
        g = np.asarray(g); w = np.asarray(w, g.dtype if g.dtype.kind == 'f' else 'i8')
        assert g.shape == w.shape and np.array_equal(g, w), (what, np.atleast_1d(g).tolist()[:64], np.atleast_1d(w).tolist()[:64])


_EXPECTED = {}


def expected(oracle, name):
    """the oracle's answers of a case, once"""
    if name not in _EXPECTED: _EXPECTED[name] = [run(oracle) for _, _, run in runs(CASE[name])]
    return _EXPECTED[name]


SG2 = np.array([f32(s) * f32(s) for s in SF], 'f4')       # mvLevelSigma2 of the N cases


def run_newpts(f, c):
    if not hasattr(f, 'dll'): return f.triangulate_pairs(c['pairs'], c['kf1'], c['kf2'], CAM, SF, SG2)
    return mappoint.TriangulateNewMapPoints(c['pairs'], c['kf1'], c['kf2'], CAM, SF, SG2, lib=f)


def check_newpts(c, got, who):
    n, ok, x = got
    assert n == sum(c['want_ok']) and ok.astype(int).tolist() == c['want_ok'], (c['name'], who, ok.astype(int).tolist())
    for q, xyz in c['want_x'].items(): assert x[q].tolist() == list(xyz), (c['name'], who, q, x[q].tolist())
    assert (x[~ok] == 0).all()


def check_kat(oracle, c):
    """the oracle gives the hand-written answer"""
    if c['kind'] == 'newpts': return check_newpts(c, expected_newpts(oracle, c), 'oracle')
    for (label, want, _), got in zip(runs(c), expected(oracle, c['name'])): same(got, want, (c['name'], label, 'oracle against the known answer'))


def expected_newpts(oracle, c):
    if c['name'] not in _EXPECTED: _EXPECTED[c['name']] = run_newpts(oracle, c)
    return _EXPECTED[c['name']]


def run_case(lib, oracle, c, exact=True):
    """the library gives the hand-written answer and the oracle's.  newpts: flags equal; positions bit-equal on the emulator (exact) and in the unprojection branches, within
    2e-3 relative in the SVD branch on the device.  Returns {branch: largest position difference} for newpts."""
    if c['kind'] == 'newpts':
        got = run_newpts(lib, c); ref = expected_newpts(oracle, c); check_newpts(c, got, 'library')
        assert got[0] == ref[0] and np.array_equal(got[1], ref[1]), (c['name'], 'flags against the oracle')
        diff = {}
        for q, b in c['branch'].items():
            d = float(np.abs(got[2][q] - ref[2][q]).max()); diff[b] = max(diff.get(b, 0.0), d)
            if exact or b != 'svd': assert d == 0.0, (c['name'], q, b, got[2][q].tolist(), ref[2][q].tolist())
            else: assert d <= 2e-3 * max(1.0, float(np.abs(ref[2][q]).max())), (c['name'], q, b, d)
        return diff
    for (label, want, run), ref in zip(runs(c), expected(oracle, c['name'])):
        got = run(lib)
        same(got, want, (c['name'], label, 'library against the known answer')); same(got, ref, (c['name'], label, 'library against the oracle'))


# ------------------------------------------------------------------------------------------------------------------ PredictScale sweep through fuse_search_sim3
def sweep_fs3(f, ks, nlevels):
    """the level that sgx_match_fuse_search_sim3 predicts for the 13 floats around every 1.2f^k (mg.sweep_ratios), in ONE call: the point sits at (0, 0, 1), dist = 1,
    max_dist = ratio; one keypoint per octave at the projection, the higher octave the nearer (4 bits a level: all within TH_LOW), so the level's own octave wins over level - 1"""
    r = [x for _, x in mg.sweep_ratios(ks)]; sf = scales(nlevels)
    K = cur_of([(0, 0, o, 4 * (nlevels - 1 - o)) for o in range(nlevels)]); P = local_of([lp((0, 0, 1), max_dist=x) for x in r]); kf = dict(keys=K['keys'], desc=K['desc'])
    n, bi, bd = f.fuse_search_sim3(kf, I4, P, CAM, sf, 1) if not hasattr(f, 'dll') else ORBmatcher(lib=f).FuseSearchSim3(kf, I4, P, 1, CAM, sf)
    assert n == len(r) and (bi >= 0).all()
    return bi.tolist()


# ------------------------------------------------------------------------------------------------------------------ sizes
def check_sizes_nodes(lib, oracle, nn):
    k1, k2 = z_nodes(nn, 100 + nn)
    common = len(set(k1['feat_node'].tolist()) & set(k2['feat_node'].tolist()))
    assert common == nn and len(k1['keys']) > 256 and len(k2['keys']) > 256                # the node loop takes a second (and, at 600, a third) turn
    sg = SG2
    for stereo, ori in ((0, 1), (1, 0)):
        en, ep = oracle.search_for_triangulation(k1, k2, F_Y, stereo, CAM, SF, sg, check_ori=bool(ori)); gn, gp = ORBmatcher(0.6, bool(ori), lib=lib).SearchForTriangulation(k1, k2, F_Y, stereo, CAM, SF, sg)
        assert gn == en and np.array_equal(gp, ep), (nn, stereo, ori, gn, en)
        late = (k1['feat_node'][ep[:, 0]] - 5) // 3 >= 256
        assert en >= nn // 16 and late.sum() >= 1, (nn, en, int(late.sum()))                 # pairs from nodes beyond the first turn
    F = {x: k2[x] for x in ('keys', 'desc', 'feat_node')}
    for ori in (1, 0):
        en, em = oracle.search_by_bow(k1, F, 0.7, bool(ori)); gn, gm = ORBmatcher(0.7, bool(ori), lib=lib).SearchByBoW(k1, F)
        assert gn == en and np.array_equal(gm, em) and en >= nn // 4 and ((k2['feat_node'][em >= 0] - 5) // 3 >= 256).any(), (nn, ori, gn, en)
        en, em = oracle.search_by_bow_kf(k1, k2, 0.75, bool(ori)); gn, gm = ORBmatcher(0.75, bool(ori), lib=lib).SearchByBoWKF(k1, k2)
        assert gn == en and np.array_equal(gm, em) and en >= nn // 4 and ((k1['feat_node'][em >= 0] - 5) // 3 >= 256).any(), (nn, ori, gn, en)


def check_sizes_points(lib, oracle, nm):
    """k_fuse_search and k_sim3_search around one workgroup of 256 candidates"""
    K, P, _ = z_proj(400, nm, 200 + nm); is2 = (1 / SG2).astype('f4'); assert len(P['xw']) == nm
    kf = dict(keys=K['keys'], desc=K['desc'], uright=K['uright'], Tcw=I4)
    e = oracle.fuse_search(kf, P, CAM, SF, is2, 3.0); g = ORBmatcher(lib=lib).FuseSearch(kf, P, 3.0, CAM, SF, is2)
    same(g, e, ('fuse_search', nm)); assert e[0] >= nm // 4 and e[1][-1] >= 0, (nm, e[0])
    e = oracle.fuse_search_sim3(kf, I4, P, CAM, SF, 4.0); g = ORBmatcher(lib=lib).FuseSearchSim3(kf, I4, P, 4.0, CAM, SF)
    same(g, e, ('fuse_search_sim3', nm)); assert e[0] >= nm // 2 and e[1][-1] >= 0, (nm, e[0])


def check_sizes_workgroup(lib, oracle, nk, nm):
    """k_match_project_kf and k_sim3_search_locked (one workgroup of 1024 threads) with more than 1024 keypoints and / or candidates"""
    K, P, taken = z_proj(nk, nm, 300 + nk + nm); assert len(K['keys']) == nk and len(P['xw']) == nm and max(nk, nm) > 1024
    kf = dict(keys=K['keys'], desc=K['desc'], matched=taken)
    e = oracle.search_by_projection_sim3(kf, I4, P, CAM, SF, 4); g = ORBmatcher(lib=lib).SearchByProjectionSim3(kf, I4, P, 4, CAM, SF)
    same(g, e, ('project_sim3', nk, nm)); assert e[0] >= min(nk, nm) // 3 and e[1][-1] == nm - 1, (nk, nm, e[0], e[1][-1])          # the last candidate and the last keypoint, both beyond the first 1024
    F = dict(keys=K['keys'], desc=K['desc'], has_mp=taken, Tcw=I4); kk = np.zeros(nm, KP_DTYPE); kk['angle'] = (np.arange(nm) * 37) % 360
    kfm = dict(keys=kk, ok=(1 - P['skip']).astype(np.uint8), xw=P['xw'], min_dist=P['min_dist'], max_dist=P['max_dist'], desc=P['desc'])
    for ori in (True, False):
        e = oracle.search_by_projection_kf(F, kfm, CAM, SF, 4.0, 64, ori); g = ORBmatcher(0.9, ori, lib=lib).SearchByProjectionKF(F, kfm, 4.0, 64, CAM, SF)
        same(g, e, ('project_keyframe', nk, nm, ori)); assert ori or (e[0] >= min(nk, nm) // 3 and e[1][-1] == nm - 1), (nk, nm, e[0], e[1][-1])


def grid_span(keys, x, y, r):
    """per grid column of the window around (x, y): how many keypoints the cells [y0, y1] of that column hold (Frame::PosInGrid, every octave)"""
    cx = np.round(((keys['x'] - X0) * mg.INVW).astype('f8')).astype(int); cy = np.round(((keys['y'] - Y0) * mg.INVH).astype('f8')).astype(int)
    x0 = max(int(np.floor((x - X0 - r) * mg.INVW)), 0); x1 = min(int(np.ceil((x - X0 + r) * mg.INVW)), 63); y0 = max(int(np.floor((y - Y0 - r) * mg.INVH)), 0); y1 = min(int(np.ceil((y - Y0 + r) * mg.INVH)), 47)
    return {c: int(((cx == c) & (cy >= y0) & (cy <= y1)).sum()) for c in range(x0, x1 + 1)}


def check_sizes_init(lib, oracle):
    F1, F2 = z_init(); pm = np.stack([F1['keys']['x'], F1['keys']['y']], 1).astype('f4')
    span = grid_span(F2['keys'], 102, 230, 250)
    assert max(span.values()) > 256 and span[11] == 300 and (F2['keys']['octave'] > 0).sum() >= 150          # the column span exceeds 256 only with every octave counted
    for ratio, ori in ((2.0, False), (2.0, True), (0.9, False)):
        e = oracle.search_for_initialization(F1, F2, pm, 250, CAM, ratio, ori); g = ORBmatcher(ratio, ori, lib=lib).SearchForInitialization(F1, F2, pm, 250, CAM)
        same(g, e, ('search_for_initialization', ratio, ori))
    e = oracle.search_for_initialization(F1, F2, pm, 250, CAM, 2.0, False)
    # keypoint 0 took frame-2 keypoint 3 (the first of the tie at distance 5, ordinal 3; the other, 297, has ordinal 297 > 256) and lost it to keypoint 1 (distance 4);
    # keypoint 3 (descriptor 118) has its twin at ordinal 258
    assert e[1].tolist()[:3] == [-1, 3, -1] and e[1][3] > 256, e[1].tolist()
    F1b = dict(keys=F1['keys'][:1], desc=F1['desc'][:1])
    e = oracle.search_for_initialization(F1b, F2, pm[:1], 250, CAM, 2.0, False); g = ORBmatcher(2.0, False, lib=lib).SearchForInitialization(F1b, F2, pm[:1], 250, CAM)
    same(g, e, ('search_for_initialization', 'tie')); assert e[1].tolist() == [3]


# ------------------------------------------------------------------------------------------------------------------ what each case is for
def _variant(oracle, c, **kw):
    """the oracle's answers on the case with some fields replaced"""
    return [run(oracle) for _, _, run in runs(dict(c, **kw))]


def check_case_contents(oracle):
    """each case contains the gate it is for: the competing candidate exists and wins once the gate's input is taken away"""
    E = lambda n: expected(oracle, n)
    for n in range(0, 130, 7): assert oracle.descriptor_distance(desc(n), desc(0)) == n
    # the decimal literals and the floats beside them
    assert float(f32(3.84)) < 3.84 and 3.84 * float(S_OUT) < 4.0 < 3.84 * float(S_IN) and S_IN == above(S_OUT)
    assert 3.84 * 75.0 == 288.0 and _variant(oracle, CASE['T_epipolar_equal'], sg=np.full(8, above(75), 'f4'))[0][0] == 2
    assert float(M_IN) < 5.99 < float(M_OUT) and float(C_IN) < 7.8 < float(C_OUT)
    assert f32(0.7) * f32(10) == f32(7) and f32(0.9) * f32(10) == f32(9) and f32(0.7) * f32(20) == f32(14) and f32(0.75) * f32(20) == f32(15) and f32(100) * SF[1] > f32(120)
    assert float(Y72) < 72 and (f32(128) - f32(134)) ** 2 + (f32(64) - Y72) ** 2 < f32(100)
    # T: without has_mp keypoint 0 of side 1 takes the match that 1 gets; a monocular world changes the epipole answers; the sigma2 neighbours swap the two octave answers
    c = CASE['T_gates']; k1 = dict(c['kf1'], has_mp=np.zeros(23, np.uint8)); p = _variant(oracle, c, kf1=k1)[0][1]
    assert [0, 0] in p.tolist() and [1, 0] not in p.tolist()
    k2 = dict(c['kf2'], has_mp=np.zeros(30, np.uint8)); assert [2, 1] in _variant(oracle, c, kf2=k2)[0][1].tolist()
    p = _variant(oracle, c, sg=np.array([1, S_OUT, S_IN, 4, 4, 4, 4, 4], 'f4'))[0][1].tolist(); assert [14, 21] not in p and [15, 22] in p
    k2 = dict(c['kf2'], uright=np.full(30, -1, 'f4')); p = _variant(oracle, c, kf2=k2)[0][1].tolist(); assert [10, 16] in p and [10, 15] not in p           # g8 without its stereo flag
    k2 = dict(c['kf2']); kk = k2['keys'].copy(); kk['octave'][13] = 0; k2['keys'] = kk; assert [9, 13] in _variant(oracle, c, kf2=k2)[0][1].tolist()       # g7 at octave 0
    assert (np.diff(E('T_gates')[0][1][:, 0]) > 0).all() and (np.diff(c['kf1']['feat_node'][E('T_gates')[0][1][:, 0]]) < 0).any()                      # ascending idx1, not node order
    assert E('T_hist_ori1')[0][0] == 10 and E('T_hist_ori0')[0][0] == 13
    # the two unmatched keypoints of the histogram case: once either is matched (50 bits instead of 51; on the epipolar line), bin 12 stays and bin 7 goes
    c = CASE['T_hist_ori1']; late = [[i, i] for i in (0, 1, 2, 3, 4, 5, 6, 10, 11, 12)]
    d = c['kf2']['desc'].copy(); d[13] = desc(50); assert _variant(oracle, c, kf2=dict(c['kf2'], desc=d))[0][1].tolist() == late + [[13, 13]]
    kk = c['kf2']['keys'].copy(); kk['y'][14] = 240; assert _variant(oracle, c, kf2=dict(c['kf2'], keys=kk))[0][1].tolist() == late + [[14, 14]]
    # B: the two overloads differ on node N1 (good_f) and N3 (50); the ratio changes N6 and N9 only
    assert E('B_frame_0.7')[0][1][2] == 2 and E('B_keyframe_0.7')[0][1][2] == 3 and E('B_frame_0.7')[0][1][6] == 5 and E('B_keyframe_0.7')[0][1][5] == -1
    assert np.flatnonzero(E('B_frame_0.7')[0][1] != E('B_frame_0.75')[0][1]).tolist() == [9, 15]
    assert len(CASE['B_frame_0.7']['kf']['keys']) != len(CASE['B_frame_0.7']['F']['keys'])
    # P: every case that gives entries different answers really does, and the rival of every refused keypoint is nearer in descriptor distance
    for name in ('P_depth', 'P_bounds', 'P_angle', 'P_clamp0_8', 'P_clamp0_12', 'P_window', 'P_accept', 'P_taken', 'P_chain'):
        ans = {e: tuple(np.asarray(g[1]).tolist()) for (e, _, _), g in zip(runs(CASE[name]), E(name))}
        assert len(set(ans.values())) >= 2, name
    for name in ('P_bounds', 'P_radius', 'P_accept'):                                         # every refused point has its keypoint (same index) inside a window of 15, or on its edge
        c = CASE[name]; k = c['K']['keys']; u = c['P']['xw'][:, 0] * 256; v = c['P']['xw'][:, 1] * 256
        assert (np.abs(k['x'][:len(u)] - u) <= 15).all() and (np.abs(k['y'][:len(u)] - v) <= 15).all() and (c['K']['keys']['octave'] == 0).all(), name
    for name, lo in (('P_window', 3), ('P_clamp_8', 0), ('P_clamp_12', 0), ('P_clamp0_8', 0), ('P_clamp0_12', 0)):          # the keypoint outside the level window is the nearest in descriptor distance
        c = CASE[name]; d = [oracle.descriptor_distance(x, c['P']['desc'][0]) for x in c['K']['desc']]; assert d[lo] < d[c['want']['A'][0]], name
    # the level below 0: the point sits ON the far edge of its band, its ratio is the float below fl(1 / 1.2f), and the true quotient lies more than a float's spacing under -1
    r = f32(1.75) / CLAMP0_Z; lsf = f32(np.log(f32(SF[1])))
    for name in ('P_clamp0_8', 'P_clamp0_12'):
        P = CASE[name]['P']; assert P['xw'][0].tolist() == [0, 0, float(CLAMP0_Z)] and P['max_dist'][0] == f32(1.75) and norm3(P['xw'][0]) == f32(1.2) * P['max_dist'][0]
    assert r == below(f32(1) / f32(1.2)) and np.log(float(r)) / np.log(float(SF[1])) < -1 - 2e-7 and np.ceil(f32(np.log(r)) / lsf) == -1
    c = CASE['P_grid_sides']; u = c['P']['xw'][:, 0] * 256; v = c['P']['xw'][:, 1] * 256                          # each window is cut at one side only, and its keypoint lies in the cut cell
    for i, (col, row) in c['cells'].items():
        kc = mg.cell(c['K']['keys']['x'][i], c['K']['keys']['y'][i]); assert (col is None or kc[0] == col) and (row is None or kc[1] == row), (i, kc)
    lo_x = np.floor((u - X0 - 15) * mg.INVW); hi_x = np.ceil((u - X0 + 15) * mg.INVW); lo_y = np.floor((v - Y0 - 15) * mg.INVH); hi_y = np.ceil((v - Y0 + 15) * mg.INVH)
    assert [bool(a) for a in lo_x < 0] == [True, False, False, False] and [bool(a) for a in hi_x > 63] == [False, True, False, False]
    assert [bool(a) for a in lo_y < 0] == [False, False, True, False] and [bool(a) for a in hi_y > 47] == [False, False, False, True]
    c = CASE['P_grid']; assert [mg.cell(*r[:2]) for r in mg.F3_KP][0][0] == 64 and mg.cell(*mg.F3_KP[2][:2])[1] == 48 and mg.cell(*mg.F3_KP[4][:2])[0] == -1
    c = CASE['P_ties']
    for i, want in c['cells'].items(): assert mg.cell(c['K']['keys']['x'][i], c['K']['keys']['y'][i]) == want, i
    c = CASE['P_band']; L1 = mg.CASE['L1_frustum']
    for j, i in enumerate((10, 11, 12, 13)): assert norm3(c['P']['xw'][j]) == L1['dist_targets'][i]
    c = CASE['P_chi2']; off = _variant(oracle, c, is2=IS2_OFF[:8])[0]; assert off[1].tolist() == [1, 3, 5, 7] and E('P_chi2')[0][1].tolist() == [0, 2, 4, 8]      # without the gate the refused twins win
    c = CASE['P_radius']; k = c['K']['keys']; assert k['x'][0] - f32(100) == f32(15) and k['x'][1] - f32(100) < f32(15) and k['y'][2] - f32(100) == f32(15) and k['y'][3] - f32(100) < f32(15)
    for name in ('P_scw_row0', 'P_scw_rot_2', 'P_scw_rot_0.5'):
        S = CASE[name]['Scw']; assert abs(np.linalg.norm(S[0, :3]) - 1) > 0.4
    # S: with nothing matched on entry every pair but the one-sided one is found
    c = CASE['S_prior']; assert _variant(oracle, c, m0=np.full(7, -1, 'i4'))[0][1].tolist() == [0, 1, 2, 3, 4, -1, -1]
    for name in ('S_rot', 'S_scale_2', 'S_scale_0.5'):
        c = CASE[name]; assert not np.array_equal(c['R12'], c['R12'].T) and _variant(oracle, c, R12=c['R12'].T.copy())[0][0] == 0
    c = CASE['S_rot']; t21 = -(c['R12'].T @ c['t12'])                                          # t12 is neither t21 nor -t12
    assert not np.array_equal(t21, c['t12']) and not np.array_equal(t21, -c['t12']) and _variant(oracle, c, t12=t21)[0][0] == 0 and _variant(oracle, c, t12=-c['t12'])[0][0] == 0
    for name, s in (('S_scale_2', 2.0), ('S_scale_0.5', 0.5)):
        c = CASE[name]; assert _variant(oracle, c, s12=1.0)[0][0] == 0
        d = norm3(c['kf1']['xw'][0]); assert d > f32(1.2) * c['kf1']['max_dist'][0] or d < f32(0.8) * c['kf1']['min_dist'][0]             # the distance from the camera centre fails the band
    # I: live counts alone would keep another set of bins
    assert E('I_stale_hist')[0][1].tolist() != E('I_stale_hist_ori0')[0][1].tolist() and E('I_gates')[0][0] == 7
    # N: the two key arrays differ, and every branch is named by a pair that is kept
    c = CASE['N_narrow_shifted']; assert (c['kf1']['keys']['x'] - c['kf1']['keys_un']['x'] == 3).all() and (c['kf2']['keys']['y'] - c['kf2']['keys_un']['y'] == 2).all()
    assert {b for n in NAMES if CASE[n]['kind'] == 'newpts' for b in CASE[n]['branch'].values()} == {'svd', 'unproject1', 'unproject2'}
    import mappoint_cases as mpc
    for n in NAMES:
        c = CASE[n]
        if c['kind'] != 'newpts': continue
        br = mpc.triangulation_branches(c['pairs'], c['kf1'], c['kf2'], CAM)                  # the float64 restatement of LocalMapping.cc:311-349 names the same branches
        for q, b in c['branch'].items(): assert br[q] == b, (n, q, br[q], b)
    assert mpc.triangulation_branches(CASE['N_wide']['pairs'], CASE['N_wide']['kf1'], CASE['N_wide']['kf2'], CAM).tolist() == ['svd', 'svd', 'none', 'svd']
    c = CASE['N_narrow_shifted']; assert mpc.triangulation_branches(c['pairs'], c['kf1'], c['kf2'], CAM)[2] == 'none'
    c = CASE['N_narrow_gates']; assert 'svd' not in mpc.triangulation_branches(c['pairs'], c['kf1'], c['kf2'], CAM).tolist()
    x = expected_newpts(oracle, CASE['N_wide'])[2]; assert np.abs(x[:2] - np.array([0.5, 0.25, 2])).max() < 1e-4
    # N: every refused pair is kept once the input of its gate is relaxed, and nothing else changes
    for n in NAMES:
        c = CASE[n]
        if c['kind'] != 'newpts': continue
        assert sorted(c['relax']) == [q for q, k in enumerate(c['want_ok']) if not k], n
        for q in c['relax']:
            ok = run_newpts(oracle, np_relaxed(c, q))[1].astype(int).tolist()
            assert ok[q] == 1 and (len(ok) == 1 or ok[:q] + ok[q + 1:] == c['want_ok'][:q] + c['want_ok'][q + 1:]), (n, q, ok)
    c = CASE['N_narrow_gates']; o1 = c['kf1']['keys_un']['octave']; o2 = c['kf2']['keys_un']['octave']; assert (o1 + o2 == 1).all()          # the two sides never share an octave
    assert o1[[0, 4]].tolist() == [0, 0] and o2[[2, 6]].tolist() == [0, 0]                                       # the refused pairs have the JUDGED side at octave 0
    for n, ow in (('N_scale', (0.125, 0, 0.5)), ('N_behind_2', (0.75, 0, 3))):                                   # camera 2 on the ray of keypoint 1: ratioDist is 0.75 and 0.5
        c = CASE[n]; assert (-c['kf2']['Tcw'][:3, 3]).tolist() == list(ow) and np.allclose(np.cross(ow, (0.5, 0, 2)), 0)
    c = CASE['N_behind_1']; assert (-c['kf1']['Tcw'][:3, 3]).tolist() == [0.75, 0, 3]
    rd = 0.75; rf = 1.8; so = lambda a, b: float(SF[a]) / float(SF[b])
    assert rd * rf < so(2, 0) and not rd > so(2, 0) * rf and rd > so(0, 5) * rf and not rd * rf < so(0, 5)       # pair 0 fails the first bound alone, pair 2 the second alone
    assert not (rd * rf < so(0, 2) or rd > so(0, 2) * rf) and rd * rf < so(5, 0)                                 # inverted, pair 0 passes and pair 2 fails the OTHER bound
