"""Optimizer — host-side mirror of ORB_SLAM2::Optimizer (reference: src/sg-slam/include/Optimizer.h:40-58)
over the C-ABI.  Implemented on the device so far:
  PoseOptimization(pFrame)     src/sg-slam/src/Optimizer.cc:239-451
The Frame is a flattened dict: keys (mvKeysUn, KP_DTYPE), uright, has_mp, xw (map-point world
positions per keypoint), Tcw (4x4 f32).  PoseOptimization updates frame['Tcw'] and frame['outlier']
in place and returns the inlier count, like the reference mutates pFrame."""
import ctypes as C
import numpy as np
from .capi import _vp, BaProblem, BaStats
from .matcher import camera_struct
from ._lib import load


class Optimizer:
    @staticmethod
    def PoseOptimization(frame, cam, inv_level_sigma2, lib=None):
        lib = lib if lib is not None else load()
        k = np.ascontiguousarray(frame['keys']); ur = np.ascontiguousarray(frame['uright'], 'f4')
        has = np.ascontiguousarray(frame['has_mp'], np.uint8); xw = np.ascontiguousarray(frame['xw'], 'f4')
        T = np.ascontiguousarray(frame['Tcw'], 'f4').reshape(16).copy()
        is2 = np.ascontiguousarray(inv_level_sigma2, 'f4')
        n = len(k)
        out = np.zeros(max(n, 1), np.uint8); ninl = np.zeros(1, 'i4')
        cs = camera_struct(cam)
        lib.check(lib.dll.sgx_pose_optimization(n, _vp(k), _vp(ur), _vp(has), _vp(xw), _vp(is2), len(is2), C.byref(cs), _vp(T), _vp(out), _vp(ninl)),
                  'sgx_pose_optimization')
        frame['Tcw'] = T.reshape(4, 4)
        frame['outlier'] = out[:n]
        return int(ninl[0])

    @staticmethod
    def LocalBundleAdjustment(problem, cam, stop_flag=None, lib=None):
        """Optimizer::LocalBundleAdjustment on a flattened local graph (see include/sgx.h sgx_ba_problem).
        problem: dict(poses[np,4,4] f32, pose_fixed[np] u8, points[nl,3] f32, edge_pose, edge_point [ne] i4,
        edge_obs[ne,3] f32, edge_info[ne] f32).  Updates problem['poses'] / ['points'] in place (like the reference
        mutates KeyFrames / MapPoints) and returns (erase[ne] u8, stats)."""
        lib = lib if lib is not None else load()
        poses = np.ascontiguousarray(problem['poses'], 'f4').reshape(-1, 16).copy(); fixed = np.ascontiguousarray(problem['pose_fixed'], np.uint8)
        pts = np.ascontiguousarray(problem['points'], 'f4').copy()
        ep = np.ascontiguousarray(problem['edge_pose'], 'i4'); el = np.ascontiguousarray(problem['edge_point'], 'i4')
        eo = np.ascontiguousarray(problem['edge_obs'], 'f4'); ei = np.ascontiguousarray(problem['edge_info'], 'f4')
        P = BaProblem(len(poses), len(pts), len(ep), poses.ctypes.data, fixed.ctypes.data, pts.ctypes.data, ep.ctypes.data, el.ctypes.data,
                      eo.ctypes.data, ei.ctypes.data)
        erase = np.zeros(len(ep), np.uint8); st = BaStats()
        cs = camera_struct(cam)
        stop = None if stop_flag is None else _vp(stop_flag)
        lib.check(lib.dll.sgx_local_bundle_adjustment(C.byref(P), C.byref(cs), stop, _vp(erase), C.byref(st)), 'sgx_local_bundle_adjustment')
        problem['poses'] = poses.reshape(-1, 4, 4); problem['points'] = pts
        return erase, dict(iterations=(st.iterations_first, st.iterations_second), chi2=(st.chi2_first, st.chi2_second), free_poses=st.free_poses)

    @staticmethod
    def flatten_ba_problem(graph, keyframes, points, inv_level_sigma2):
        """The dict LocalBundleAdjustment / BundleAdjustment take, from a graph of CovisibilityGraph.local_ba_graph / global_ba_graph (status 0) and the caller's arrays:
        keyframes[id] = dict(Tcw [4,4], uv [n,2] = mvKeysUn[i].pt, uright [n] = mvuRight), points [P,3] = GetWorldPos() by point id, inv_level_sigma2 = mvInvLevelSigma2.
        edge_obs = (u, v, uR) with uR = -1 for a monocular edge (Optimizer.cc:594), edge_info = mvInvLevelSigma2[octave] (:604, :632).  A numpy gather: the solver takes
        host pointers."""
        assert graph['status'] == 0, 'a graph that did not fit its rows'
        ids = [int(k) for k in graph['pose_id']]; ne = len(graph['edge_pose'])
        poses = np.stack([np.asarray(keyframes[k]['Tcw'], 'f4').reshape(4, 4) for k in ids]) if ids else np.zeros((0, 4, 4), 'f4')
        pts = np.ascontiguousarray(np.asarray(points, 'f4').reshape(-1, 3)[graph['point_id']])
        ep = np.ascontiguousarray(graph['edge_pose'], 'i4'); kp = np.asarray(graph['edge_kp']); attr = np.asarray(graph['edge_attr'])
        obs = np.zeros((ne, 3), 'f4')
        for j, k in enumerate(ids):
            m = ep == j
            if not m.any(): continue
            obs[m, :2] = np.asarray(keyframes[k]['uv'], 'f4').reshape(-1, 2)[kp[m]]; obs[m, 2] = np.asarray(keyframes[k]['uright'], 'f4').reshape(-1)[kp[m]]
        obs[(attr & 32) == 0, 2] = -1.0
        info = np.ascontiguousarray(np.asarray(inv_level_sigma2, 'f4')[attr & 31])
        return dict(poses=poses, pose_fixed=np.ascontiguousarray(graph['pose_fixed'], np.uint8), points=pts, edge_pose=ep,
                    edge_point=np.ascontiguousarray(graph['edge_point'], 'i4'), edge_obs=obs, edge_info=info)

    @staticmethod
    def BundleAdjustment(problem, cam, nIterations=5, stop_flag=None, nLoopKF=0, bRobust=True, lib=None):
        """Optimizer::BundleAdjustment(vpKFs, vpMP, nIterations, pbStopFlag, nLoopKF, bRobust) on the flattened graph (pose_fixed != 0 exactly for the keyframe
        with mnId == 0).  nLoopKF == 0: problem['poses'] / ['points'] are updated in place (SetPose / SetWorldPos); otherwise the results are returned under
        'poses_gba' / 'points_gba' (mTcwGBA / mPosGBA, mnBAGlobalForKF = nLoopKF) and the problem is left untouched.  Returns stats."""
        lib = lib if lib is not None else load()
        poses = np.ascontiguousarray(problem['poses'], 'f4').reshape(-1, 16).copy(); fixed = np.ascontiguousarray(problem['pose_fixed'], np.uint8)
        pts = np.ascontiguousarray(problem['points'], 'f4').copy()
        ep = np.ascontiguousarray(problem['edge_pose'], 'i4'); el = np.ascontiguousarray(problem['edge_point'], 'i4')
        eo = np.ascontiguousarray(problem['edge_obs'], 'f4'); ei = np.ascontiguousarray(problem['edge_info'], 'f4')
        P = BaProblem(len(poses), len(pts), len(ep), poses.ctypes.data, fixed.ctypes.data, pts.ctypes.data, ep.ctypes.data, el.ctypes.data,
                      eo.ctypes.data, ei.ctypes.data)
        st = BaStats(); cs = camera_struct(cam)
        stop = None if stop_flag is None else _vp(stop_flag)
        lib.check(lib.dll.sgx_bundle_adjustment(C.byref(P), C.byref(cs), int(nIterations), stop, int(bool(bRobust)), C.byref(st)), 'sgx_bundle_adjustment')
        if nLoopKF == 0:
            problem['poses'] = poses.reshape(-1, 4, 4); problem['points'] = pts
        else:
            problem['poses_gba'] = poses.reshape(-1, 4, 4); problem['points_gba'] = pts; problem['mnBAGlobalForKF'] = nLoopKF
        return dict(iterations=st.iterations_first, chi2=st.chi2_first, free_poses=st.free_poses)

    @staticmethod
    def ApplyGlobalBundleAdjustment(problem, graph, covis, origins, point_ref, Tcw=None, xw=None, stream=None):
        """The map update of LoopClosing::RunGlobalBundleAdjustment (LoopClosing.cc:676-737) from what BundleAdjustment(nLoopKF != 0) left in `problem` ('poses_gba',
        'points_gba') for the keyframes and points of `graph` (global_ba_graph when the solver started).  The map of `covis` as it stands now may hold more: Tcw (by
        keyframe id) and xw (by point id) give their poses and positions.  origins = mvpKeyFrameOrigins as ids; point_ref = GetReferenceKeyFrame()->mnId by point id
        (a dict or an array; missing or -1: none).  Returns Tcw {id: 3 x 4}, xw {point id: position}, kf_state {id: bits}, and the rows of covis.gba_update."""
        assert 'poses_gba' in problem, 'BundleAdjustment was not run with nLoopKF != 0'
        now = covis.global_ba_graph(stream=stream)
        assert now['status'] == 0
        ids = [int(k) for k in now['pose_id']]; pids = [int(p) for p in now['point_id']]
        in_kf = {int(k): j for j, k in enumerate(graph['pose_id'])}; in_pt = {int(p): j for j, p in enumerate(graph['point_id'])}
        T = np.zeros((len(ids), 3, 4), 'f4'); G = np.zeros((len(ids), 3, 4), 'f4'); g = np.zeros(len(ids), 'u1')
        for r, k in enumerate(ids):
            if k in in_kf:
                j = in_kf[k]; g[r] = 1; T[r] = np.asarray(problem['poses'], 'f4').reshape(-1, 4, 4)[j, :3]; G[r] = np.asarray(problem['poses_gba'], 'f4').reshape(-1, 4, 4)[j, :3]
            else: T[r] = np.asarray(Tcw[k], 'f4').reshape(-1, 4)[:3]
        row = {k: r for r, k in enumerate(ids)}
        X = np.zeros((len(pids), 3), 'f4'); XG = np.zeros((len(pids), 3), 'f4'); pg = np.zeros(len(pids), 'u1'); ref = np.full(len(pids), -1, 'i4')
        for i, p in enumerate(pids):
            if p in in_pt: pg[i] = 1; X[i] = problem['points'][in_pt[p]]; XG[i] = problem['points_gba'][in_pt[p]]
            else: X[i] = np.asarray(xw[p], 'f4')
            k = -1 if point_ref is None else (point_ref.get(p, -1) if isinstance(point_ref, dict) else int(point_ref[p]))
            ref[i] = row.get(int(k), -1)
        out = covis.gba_update(origins, ids, g, T, G, points=dict(xw=X, in_gba=pg, xw_gba=XG, ref=ref), stream=stream)
        if out['status'] == 0:
            out['Tcw'] = {k: out['Tcw_out'][r] for r, k in enumerate(ids)}; out['xw'] = {p: out['xw_out'][i] for i, p in enumerate(pids)}
            out['kf_state_by_id'] = {k: int(out['kf_state'][r]) for r, k in enumerate(ids)}
        out['kf_ids'] = ids; out['point_ids'] = pids; out['in_gba'] = g; out['Tcw_in'] = T; out['TcwGBA'] = G; out['points_in'] = dict(xw=X, in_gba=pg, xw_gba=XG, ref=ref)
        return out

    @staticmethod
    def OptimizeSim3(p1c, p2c, obs1, obs2, info1, info2, K1, K2, S12, th2=10.0, bFixScale=False, lib=None):
        """Optimizer::OptimizeSim3(pKF1, pKF2, vpMatches1, g2oS12, th2, bFixScale) (Optimizer.cc:1046-1257) on the flattened correspondences (see include/sgx.h):
        returns (nIn, S12[8] = (qx, qy, qz, qw, tx, ty, tz, s), inlier[n], iterations[2])."""
        lib = lib if lib is not None else load()
        p1c = np.ascontiguousarray(p1c, 'f4').reshape(-1, 3); p2c = np.ascontiguousarray(p2c, 'f4').reshape(-1, 3); n = len(p1c)
        o1 = np.ascontiguousarray(obs1, 'f4').reshape(-1, 2); o2 = np.ascontiguousarray(obs2, 'f4').reshape(-1, 2)
        i1 = np.ascontiguousarray(info1, 'f4'); i2 = np.ascontiguousarray(info2, 'f4')
        k1 = np.ascontiguousarray(K1, 'f4'); k2 = np.ascontiguousarray(K2, 'f4')
        S = np.ascontiguousarray(S12, 'f8').copy(); inl = np.zeros(max(n, 1), np.uint8); it = np.zeros(2, 'i4'); nin = np.zeros(1, 'i4')
        lib.check(lib.dll.sgx_optimize_sim3(n, _vp(p1c), _vp(p2c), _vp(o1), _vp(o2), _vp(i1), _vp(i2), _vp(k1), _vp(k2), _vp(S), float(th2), int(bool(bFixScale)), _vp(inl), _vp(it), _vp(nin)),
                  'sgx_optimize_sim3')
        return int(nin[0]), S, inl[:n].copy(), it

    @staticmethod
    def OptimizeEssentialGraph(S, fixed, e_i, e_j, e_meas, bFixScale=True, iterations=20, lib=None):
        """the optimisation of Optimizer::OptimizeEssentialGraph (Optimizer.cc:781-1042) on a flattened pose graph (see include/sgx.h): (S_out[nv, 8], stats[iterations, chi2 before, after])"""
        lib = lib if lib is not None else load()
        S = np.ascontiguousarray(S, 'f8').reshape(-1, 8); fx = np.ascontiguousarray(fixed, np.uint8)
        ei = np.ascontiguousarray(e_i, 'i4'); ej = np.ascontiguousarray(e_j, 'i4'); em = np.ascontiguousarray(e_meas, 'f8').reshape(-1, 8)
        out = np.zeros_like(S); st = np.zeros(3, 'f8')
        lib.check(lib.dll.sgx_optimize_essential_graph(len(S), _vp(S), _vp(fx), len(ei), _vp(ei), _vp(ej), _vp(em), int(bool(bFixScale)), int(iterations), _vp(out), _vp(st)), 'sgx_optimize_essential_graph')
        return out, st

    @staticmethod
    def CorrectMapPoints(xw, ref, Srw, corrected_Swr, lib=None):
        """Optimizer.cc:1004-1041: P' = correctedSwr.map(Srw.map(P)) for every map point (ref = its reference keyframe's vertex index)"""
        lib = lib if lib is not None else load()
        xw = np.ascontiguousarray(xw, 'f4').reshape(-1, 3); ref = np.ascontiguousarray(ref, 'i4')
        a = np.ascontiguousarray(Srw, 'f8').reshape(-1, 8); c = np.ascontiguousarray(corrected_Swr, 'f8').reshape(-1, 8)
        out = np.zeros_like(xw)
        lib.check(lib.dll.sgx_correct_map_points(len(xw), _vp(xw), _vp(ref), len(a), _vp(a), _vp(c), _vp(out)), 'sgx_correct_map_points')
        return out

    # ---- the Sim3 glue of loop closing (see include/sgx.h): a Sim3 is (qx, qy, qz, qw, tx, ty, tz, s), a pose the rows of [R | t]
    @staticmethod
    def _poses(T):
        T = np.asarray(T, 'f4')
        return np.ascontiguousarray(T.reshape(-1, T.shape[-2], 4)[:, :3, :], 'f4')

    @staticmethod
    def PropagateLoopSim3(Tcw_group, Scw, lib=None):
        """LoopClosing::CorrectLoop :440-469, :503-512: the poses of the group in group order (the current keyframe last) and its Scw ->
        (NonCorrectedSim3[ng, 8], CorrectedSim3[ng, 8], the corrected poses [ng, 3, 4] float32)"""
        lib = lib if lib is not None else load()
        T = Optimizer._poses(Tcw_group); S = np.ascontiguousarray(Scw, 'f8').reshape(8); n = len(T)
        non = np.zeros((n, 8)); cor = np.zeros((n, 8)); out = np.zeros((n, 3, 4), 'f4')
        lib.check(lib.dll.sgx_loop_propagate_sim3(n, _vp(T), _vp(S), _vp(non), _vp(cor), _vp(out)), 'sgx_loop_propagate_sim3')
        return non, cor, out

    @staticmethod
    def FlattenEssentialGraph(graph, Tcw_vertices, corrected, noncorrected, lib=None):
        """Optimizer.cc:818-832, :857-867, :889-972 for a graph of CovisibilityGraph.essential_graph and the poses in vertex order (a group vertex's is not read):
        (S_in[nv, 8], e_meas[ne, 8]), what OptimizeEssentialGraph takes with graph['vertex_fixed'], graph['e_i'], graph['e_j']"""
        lib = lib if lib is not None else load()
        vg = np.ascontiguousarray(graph['vertex_group'], 'i4'); T = Optimizer._poses(Tcw_vertices); nv = len(vg)
        assert len(T) == nv
        cor = np.ascontiguousarray(corrected, 'f8').reshape(-1, 8); non = np.ascontiguousarray(noncorrected, 'f8').reshape(-1, 8)
        ei = np.ascontiguousarray(graph['e_i'], 'i4'); ej = np.ascontiguousarray(graph['e_j'], 'i4'); ek = np.ascontiguousarray(graph['e_kind'], 'u1')
        S = np.zeros((nv, 8)); m = np.zeros((len(ei), 8))
        lib.check(lib.dll.sgx_eg_flatten(nv, _vp(vg), _vp(T), len(cor), _vp(cor), _vp(non), len(ei), _vp(ei), _vp(ej), _vp(ek), _vp(S), _vp(m)), 'sgx_eg_flatten')
        return S, m

    @staticmethod
    def RecoverEssentialGraph(S_out, lib=None):
        """Optimizer.cc:991-1010: (Tcw[nv, 3, 4] float32, vCorrectedSwc[nv, 8])"""
        lib = lib if lib is not None else load()
        S = np.ascontiguousarray(S_out, 'f8').reshape(-1, 8); n = len(S)
        T = np.zeros((n, 3, 4), 'f4'); inv = np.zeros((n, 8))
        lib.check(lib.dll.sgx_eg_recover(n, _vp(S), _vp(T), _vp(inv)), 'sgx_eg_recover')
        return T, inv
