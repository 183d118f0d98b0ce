"""CovisibilityGraph — Python mirror of the covisibility graph over the C ABI (sgx_covis_*).

The relation "keyframe k observes map point p at keypoint index i" lives on the device with what the reference derives from it (mConnectedKeyFrameWeights, the ordered
lists, the spanning tree, every point's observations and nObs).  Mutations take host arrays and are synchronous; the three walks — KeyFrame::UpdateConnections
(KeyFrame.cc:290-380), Tracking::UpdateLocalMap (Tracking.cc:1314-1458) and the votes of LocalMapping::KeyFrameCulling (LocalMapping.cc:632-696) — are batched launch
sequences on a stream, and so is the graph of Optimizer::LocalBundleAdjustment / BundleAdjustment (Optimizer.cc:453-504, :572-653, :49-150): local_ba_graph,
global_ba_graph, ba_graph_batch, with apply_ba_erase for the vToErase loop (:745-757), and the map bookkeeping of LoopClosing::CorrectLoop (LoopClosing.cc:432-573)
with the vertices and edges of Optimizer::OptimizeEssentialGraph (Optimizer.cc:797-983): add_loop_edge, loop_begin, loop_connections, essential_graph.  Keyframes are named by the caller's mnId, points by dense handles in [0, max_points)."""
import ctypes as C
import numpy as np
from .capi import _vp, COVIS_REPORT_DTYPE, COVIS_BA_REPORT_DTYPE, COVIS_LOOP_REPORT_DTYPE, COVIS_CONSISTENCY_REPORT_DTYPE, COVIS_GBA_REPORT_DTYPE


def _i4(v):
    return np.ascontiguousarray(v, 'i4').reshape(-1)


class CovisibilityGraph:
    def __init__(self, max_keyframes=1024, cap=2048, max_points=1 << 17, max_observations=1 << 20, max_queries=64, monocular=False, th_depth=40.0, lib=None):
        if lib is None:
            import sg_slam_amd
            lib = sg_slam_amd.load()
        self.lib = lib
        self.max_keyframes = int(max_keyframes); self.cap = int(cap); self.max_points = int(max_points); self.max_queries = int(max_queries)
        self.h = C.c_void_p()
        lib.check(lib.dll.sgx_covis_create(self.max_keyframes, self.cap, self.max_points, int(max_observations), self.max_queries, int(bool(monocular)), float(th_depth),
                                           C.byref(self.h)), 'sgx_covis_create')
        self._on_host = 'EMULATOR' in lib.version()               # the emulator's "device" memory is host memory

    # ---- mutations (host arrays, synchronous)
    def add_keyframe(self, kf_id, octave, uright, depth):
        o = _i4(octave); u = np.ascontiguousarray(uright, 'f4').reshape(-1); d = np.ascontiguousarray(depth, 'f4').reshape(-1)
        assert len(o) == len(u) == len(d)
        self.lib.check(self.lib.dll.sgx_covis_add_keyframe(self.h, int(kf_id), len(o), _vp(o), _vp(u), _vp(d)), 'sgx_covis_add_keyframe')

    def set_observations(self, kf_id, idx, point_ids):
        """pairs in order: point >= 0 = AddMapPoint + AddObservation, -1 = EraseMapPointMatch + EraseObservation"""
        i = _i4(idx); p = _i4(point_ids)
        assert len(i) == len(p)
        self.lib.check(self.lib.dll.sgx_covis_set_observations(self.h, int(kf_id), len(i), _vp(i), _vp(p)), 'sgx_covis_set_observations')

    def erase_observation(self, kf_id, idx):
        self.set_observations(kf_id, [idx], [-1])

    def set_points_bad(self, ids):
        p = _i4(ids)
        self.lib.check(self.lib.dll.sgx_covis_set_points_bad(self.h, len(p), _vp(p)), 'sgx_covis_set_points_bad')

    def replace_point(self, old, new):
        self.lib.check(self.lib.dll.sgx_covis_replace_point(self.h, int(old), int(new)), 'sgx_covis_replace_point')

    def erase_keyframe(self, kf_id):
        self.lib.check(self.lib.dll.sgx_covis_erase_keyframe(self.h, int(kf_id)), 'sgx_covis_erase_keyframe')

    def clear(self):
        self.lib.check(self.lib.dll.sgx_covis_clear(self.h), 'sgx_covis_clear')

    def size(self):
        return int(self.lib.dll.sgx_covis_size(self.h))

    def info(self):
        """(device bytes, of which workspace bytes, live observations)"""
        a = C.c_int64(); b = C.c_int64(); n = C.c_int32()
        self.lib.check(self.lib.dll.sgx_covis_info(self.h, C.byref(a), C.byref(b), C.byref(n)), 'sgx_covis_info')
        return a.value, b.value, n.value

    # ---- getters (synchronous)
    def _pairs(self, fn, kf_id):
        a = np.zeros(self.max_keyframes, 'i4'); b = np.zeros(self.max_keyframes, 'i4'); n = C.c_int32()
        self.lib.check(getattr(self.lib.dll, fn)(self.h, int(kf_id), _vp(a), _vp(b), C.byref(n)), fn)
        return [int(x) for x in a[:n.value]], [int(x) for x in b[:n.value]]

    def weights(self, kf_id):
        """mConnectedKeyFrameWeights as (ids ascending, weights)"""
        return self._pairs('sgx_covis_get_weights', kf_id)

    def ordered(self, kf_id):
        """(mvpOrderedConnectedKeyFrames as ids, mvOrderedWeights)"""
        return self._pairs('sgx_covis_get_ordered', kf_id)

    def best_covisibles(self, kf_id, N=10):
        """GetBestCovisibilityKeyFrames(N) as ids: what KeyFrameDatabase.set_covisibility takes"""
        a = np.zeros(max(int(N), 1), 'i4'); n = C.c_int32()
        self.lib.check(self.lib.dll.sgx_covis_best_covisibles(self.h, int(kf_id), int(N), _vp(a), C.byref(n)), 'sgx_covis_best_covisibles')
        return [int(x) for x in a[:n.value]]

    def tree(self, kf_id):
        """(parent id or -1, mbFirstConnection, children ids ascending)"""
        p = C.c_int32(); f = C.c_int32(); c = np.zeros(self.max_keyframes, 'i4'); n = C.c_int32()
        self.lib.check(self.lib.dll.sgx_covis_get_tree(self.h, int(kf_id), C.byref(p), C.byref(f), _vp(c), C.byref(n)), 'sgx_covis_get_tree')
        return p.value, bool(f.value), [int(x) for x in c[:n.value]]

    def observations(self, point_id):
        """(mObservations as [(keyframe id, index)] in keyframe order, nObs)"""
        k, i = np.zeros(self.max_keyframes, 'i4'), np.zeros(self.max_keyframes, 'i4'); n = C.c_int32(); no = C.c_int32()
        self.lib.check(self.lib.dll.sgx_covis_get_observations(self.h, int(point_id), _vp(k), _vp(i), C.byref(n), C.byref(no)), 'sgx_covis_get_observations')
        return [(int(a), int(b)) for a, b in zip(k[:n.value], i[:n.value])], no.value

    def keyframe_points(self, kf_id):
        p = np.zeros(self.cap, 'i4'); n = C.c_int32()
        self.lib.check(self.lib.dll.sgx_covis_get_keyframe_points(self.h, int(kf_id), _vp(p), C.byref(n)), 'sgx_covis_get_keyframe_points')
        return p[:n.value].copy()

    # ---- device plumbing
    def _dev(self, a):
        a = np.ascontiguousarray(a)
        if self._on_host: return a.copy()
        import torch
        return torch.from_numpy(a).cuda()

    def _host(self, x):
        return x if self._on_host else x.cpu().numpy()

    def _stream(self, stream):
        if self._on_host: return None
        import torch
        s = stream if stream is not None else torch.cuda.current_stream()
        return C.c_void_p(s.cuda_stream)

    def _sync(self, stream):
        if self._on_host: return
        import torch
        (stream if stream is not None else torch.cuda.current_stream()).synchronize()

    # ---- the queries
    def update_connections_batch_dev(self, Q, kf_ids_dev, report_dev, stream=None):
        self._keep = (kf_ids_dev, report_dev)
        self.lib.check(self.lib.dll.sgx_covis_update_connections_batch_dev(self.h, int(Q), _vp(kf_ids_dev), _vp(report_dev), self._stream(stream)),
                       'sgx_covis_update_connections_batch_dev')

    def update_connections(self, kf_ids, stream=None):
        """KeyFrame::UpdateConnections of the listed keyframes, in order, as one batch; the report records"""
        k = _i4(kf_ids); Q = len(k)
        rep = self._dev(np.zeros(Q * COVIS_REPORT_DTYPE.itemsize, 'u1'))
        self.update_connections_batch_dev(Q, self._dev(k), rep, stream)
        self._sync(stream)
        return self._host(rep).view(COVIS_REPORT_DTYPE).copy()

    def local_map_batch_dev(self, Q, cap, frame_mp_dev, n_dev, min_obs_dev, local_kf_dev, n_local_kf_dev, ref_kf_dev, ref_tracked_dev, mcap, local_points_dev, local_obs_dev,
                            n_local_points_dev, report_dev, stream=None):
        self._keep = (frame_mp_dev, n_dev, min_obs_dev, local_kf_dev, n_local_kf_dev, ref_kf_dev, ref_tracked_dev, local_points_dev, local_obs_dev, n_local_points_dev, report_dev)
        self.lib.check(self.lib.dll.sgx_covis_local_map_batch_dev(self.h, int(Q), int(cap), _vp(frame_mp_dev), _vp(n_dev), _vp(min_obs_dev), _vp(local_kf_dev), _vp(n_local_kf_dev),
                                                                  _vp(ref_kf_dev), _vp(ref_tracked_dev), int(mcap), _vp(local_points_dev), _vp(local_obs_dev),
                                                                  _vp(n_local_points_dev), _vp(report_dev), self._stream(stream)), 'sgx_covis_local_map_batch_dev')

    def local_map(self, frames, min_obs, local_kfs=None, ref_kfs=None, mcap=4096, stream=None):
        """Tracking::UpdateLocalMap for Q frames (lists of point ids, -1 = none) from the host, read back.  local_kfs / ref_kfs: mvpLocalKeyFrames (id lists) and
        mpReferenceKF (-1 none) going in.  Returns one dict per frame: frame (mvpMapPoints after), local_kf, ref_kf, ref_tracked, points, obs, n_points, report."""
        Q = len(frames); cap = max([len(f) for f in frames] + [1]); N = self.max_keyframes
        fm = np.full((Q, cap), -1, 'i4'); n = np.zeros(Q, 'i4'); lk = np.full((Q, N), -1, 'i4'); nlk = np.zeros(Q, 'i4'); ref = np.full(Q, -1, 'i4')
        for q, f in enumerate(frames):
            fm[q, :len(f)] = f; n[q] = len(f)
            if local_kfs is not None: lk[q, :len(local_kfs[q])] = local_kfs[q]; nlk[q] = len(local_kfs[q])
            if ref_kfs is not None: ref[q] = ref_kfs[q]
        mo = np.broadcast_to(np.asarray(min_obs, 'i4'), (Q,)).copy()
        d = [self._dev(x) for x in (fm, n, mo, lk, nlk, ref, np.zeros(Q, 'i4'), np.full((Q, mcap), -1, 'i4'), np.full((Q, mcap), -1, 'i4'), np.zeros(Q, 'i4'),
                                    np.zeros(Q * COVIS_REPORT_DTYPE.itemsize, 'u1'))]
        self.local_map_batch_dev(Q, cap, d[0], d[1], d[2], d[3], d[4], d[5], d[6], mcap, d[7], d[8], d[9], d[10], stream)
        self._sync(stream)
        fm, _, _, lk, nlk, ref, rt, pts, obs, npts, rep = [self._host(x) for x in d]
        rep = rep.view(COVIS_REPORT_DTYPE)
        out = []
        for q in range(Q):
            m = min(int(npts[q]), mcap)
            out.append(dict(frame=fm[q, :n[q]].copy(), local_kf=[int(x) for x in lk[q, :nlk[q]]], ref_kf=int(ref[q]), ref_tracked=int(rt[q]), points=pts[q, :m].copy(),
                            obs=obs[q, :m].copy(), n_points=int(npts[q]), report=rep[q].copy()))
        return out

    def keyframe_culling_batch_dev(self, Q, kf_ids_dev, max_cand, cand_dev, n_cand_dev, n_redundant_dev, n_mps_dev, cull_dev, stream=None):
        self._keep = (kf_ids_dev, cand_dev, n_cand_dev, n_redundant_dev, n_mps_dev, cull_dev)
        self.lib.check(self.lib.dll.sgx_covis_keyframe_culling_batch_dev(self.h, int(Q), _vp(kf_ids_dev), int(max_cand), _vp(cand_dev), _vp(n_cand_dev), _vp(n_redundant_dev),
                                                                         _vp(n_mps_dev), _vp(cull_dev), self._stream(stream)), 'sgx_covis_keyframe_culling_batch_dev')

    def keyframe_culling(self, kf_ids, max_cand=None, stream=None):
        """the votes of LocalMapping::KeyFrameCulling for the listed current keyframes, against the map as it stands: per keyframe a list of
        (candidate id, nRedundantObservations, nMPs, vote), or None for an unknown keyframe"""
        k = _i4(kf_ids); Q = len(k); M = int(max_cand or self.max_keyframes)
        d = [self._dev(x) for x in (k, np.full((Q, M), -1, 'i4'), np.zeros(Q, 'i4'), np.zeros((Q, M), 'i4'), np.zeros((Q, M), 'i4'), np.zeros((Q, M), 'i4'))]
        self.keyframe_culling_batch_dev(Q, d[0], M, d[1], d[2], d[3], d[4], d[5], stream)
        self._sync(stream)
        _, cand, nc, red, mps, cull = [self._host(x) for x in d]
        return [None if nc[q] < 0 else [(int(cand[q, r]), int(red[q, r]), int(mps[q, r]), int(cull[q, r])) for r in range(min(int(nc[q]), M))] for q in range(Q)]

    # ---- the bundle-adjustment graph
    BA_LOCAL = 0; BA_GLOBAL = 1; ATTR_OCTAVE = 31; ATTR_RIGHT = 32; ATTR_CLOSE = 64

    def ba_graph_batch_dev(self, Q, mode, kf_ids_dev, pose_id_dev, pose_fixed_dev, pcap, point_id_dev, point_edge_begin_dev, ecap, edge_pose_dev, edge_point_dev, edge_kp_dev,
                           edge_attr_dev, report_dev, stream=None):
        self._keep = (kf_ids_dev, pose_id_dev, pose_fixed_dev, point_id_dev, point_edge_begin_dev, edge_pose_dev, edge_point_dev, edge_kp_dev, edge_attr_dev, report_dev)
        self.lib.check(self.lib.dll.sgx_covis_ba_graph_batch_dev(self.h, int(Q), int(mode), _vp(kf_ids_dev), _vp(pose_id_dev), _vp(pose_fixed_dev), int(pcap), _vp(point_id_dev),
                                                                 _vp(point_edge_begin_dev), int(ecap), _vp(edge_pose_dev), _vp(edge_point_dev), _vp(edge_kp_dev),
                                                                 _vp(edge_attr_dev), _vp(report_dev), self._stream(stream)), 'sgx_covis_ba_graph_batch_dev')

    def ba_graph_batch(self, kf_ids, mode=0, pcap=None, ecap=None, stream=None):
        """The graph of Optimizer::LocalBundleAdjustment (Optimizer.cc:453-504, :572-653) for each listed keyframe as one batch, or with mode = BA_GLOBAL that of
        Optimizer::BundleAdjustment (:49-150) for the whole map (one query; kf_ids is not read).  pcap / ecap: capacities of the point and edge rows; by default what the
        map as it stands can need.  One dict per query, the rows trimmed to what was written: status, pose_id, pose_fixed, point_id, point_edge_begin, edge_pose,
        edge_point, edge_kp, edge_attr and the report (the true counts)."""
        k = _i4(kf_ids) if mode == self.BA_LOCAL else np.zeros(1, 'i4'); Q = len(k); N = self.max_keyframes
        nobs = self.info()[2]
        pcap = int(min(self.max_points, nobs) if pcap is None else pcap); ecap = int(nobs if ecap is None else ecap)
        pc, ec = max(pcap, 0), max(ecap, 0)
        d = [self._dev(x) for x in (k, np.full((Q, N), -1, 'i4'), np.full((Q, N), 255, 'u1'), np.full((Q, max(pc, 1)), -1, 'i4'), np.full((Q, pc + 1), -1, 'i4'),
                                    np.full((Q, max(ec, 1)), -1, 'i4'), np.full((Q, max(ec, 1)), -1, 'i4'), np.full((Q, max(ec, 1)), -1, 'i4'), np.full((Q, max(ec, 1)), 255, 'u1'),
                                    np.zeros(Q * COVIS_BA_REPORT_DTYPE.itemsize, 'u1'))]
        self.ba_graph_batch_dev(Q, mode, d[0], d[1], d[2], pcap, d[3], d[4], ecap, d[5], d[6], d[7], d[8], d[9], stream)
        self._sync(stream)
        _, pid, pfx, pts, beg, ep, el, ek, ea, rep = [self._host(x) for x in d]
        rep = rep.view(COVIS_BA_REPORT_DTYPE)
        out = []
        for q in range(Q):
            r = rep[q].copy(); st = int(r['status'])
            if st == -1:
                out.append(dict(status=st, report=r)); continue
            npo = int(r['n_poses']); npt = min(int(r['n_points']), pc); b = beg[q, :npt + 1]
            ne = int(b[np.searchsorted(b, ec, side='right') - 1])                       # the edges of the leading points that fit wholly
            out.append(dict(status=st, pose_id=pid[q, :npo].copy(), pose_fixed=pfx[q, :npo].copy(), point_id=pts[q, :npt].copy(), point_edge_begin=b.copy(),
                            edge_pose=ep[q, :ne].copy(), edge_point=el[q, :ne].copy(), edge_kp=ek[q, :ne].copy(), edge_attr=ea[q, :ne].copy(), report=r))
        return out

    def local_ba_graph(self, kf_id, pcap=None, ecap=None, stream=None):
        return self.ba_graph_batch([kf_id], self.BA_LOCAL, pcap, ecap, stream)[0]

    def global_ba_graph(self, pcap=None, ecap=None, stream=None):
        return self.ba_graph_batch([], self.BA_GLOBAL, pcap, ecap, stream)[0]

    def apply_ba_erase(self, graph, erase):
        """vToErase of Optimizer::LocalBundleAdjustment (Optimizer.cc:711-757) into the relation: every flagged monocular edge in edge order, then every flagged stereo
        edge, each EraseMapPointMatch + EraseObservation with its SetBadFlag at nObs <= 2 (an edge whose point went that way before its turn finds nothing to erase).
        Returns the (keyframe id, point id) pairs in the order applied."""
        e = np.asarray(erase).reshape(-1) != 0
        assert len(e) == len(graph['edge_pose'])
        stereo = (graph['edge_attr'] & self.ATTR_RIGHT) != 0
        done = []
        for j in list(np.flatnonzero(e & ~stereo)) + list(np.flatnonzero(e & stereo)):
            kf = int(graph['pose_id'][graph['edge_pose'][j]])
            self.set_observations(kf, [int(graph['edge_kp'][j])], [-1])
            done.append((kf, int(graph['point_id'][graph['edge_point'][j]])))
        return done

    # ---- loop closing: mspLoopEdges, CorrectLoop's group / LoopConnections and the graph of OptimizeEssentialGraph
    def add_loop_edge(self, kf_a, kf_b):
        """KeyFrame::AddLoopEdge both ways (LoopClosing.cc:572-573); a set: the same edge again changes nothing"""
        self.lib.check(self.lib.dll.sgx_covis_add_loop_edge(self.h, int(kf_a), int(kf_b)), 'sgx_covis_add_loop_edge')

    def loop_edges(self, kf_id):
        """mspLoopEdges of the keyframe as ids ascending"""
        a = np.zeros(self.max_keyframes, 'i4'); n = C.c_int32()
        self.lib.check(self.lib.dll.sgx_covis_get_loop_edges(self.h, int(kf_id), _vp(a), C.byref(n)), 'sgx_covis_get_loop_edges')
        return [int(x) for x in a[:n.value]]

    def loop_info(self):
        """(device bytes the loop calls allocated beyond create's: 0 before the first of them, loop edges)"""
        a = C.c_int64(); n = C.c_int32()
        self.lib.check(self.lib.dll.sgx_covis_loop_info(self.h, C.byref(a), C.byref(n)), 'sgx_covis_loop_info')
        return a.value, n.value

    def loop_begin_dev(self, cur, group_id_dev, group_vertex_dev, pcap, point_id_dev, point_ref_dev, report_dev, stream=None):
        self._keep = (group_id_dev, group_vertex_dev, point_id_dev, point_ref_dev, report_dev)
        self.lib.check(self.lib.dll.sgx_covis_loop_begin_dev(self.h, int(cur), _vp(group_id_dev), _vp(group_vertex_dev), int(pcap), _vp(point_id_dev), _vp(point_ref_dev),
                                                             _vp(report_dev), self._stream(stream)), 'sgx_covis_loop_begin_dev')

    def loop_begin(self, cur, pcap=None, stream=None):
        """LoopClosing::CorrectLoop :432-436 and the marks of :472-516: UpdateConnections(cur), the group (the listed neighbours without dead entries, then cur), the
        UpdateConnections of every member in ascending id, and the group's existing points with mnCorrectedReference.  Returns status, group_id, group_vertex, point_id,
        point_ref (an index into the group row) trimmed to what was written, and the report (the true counts)."""
        N = self.max_keyframes
        pcap = int(min(self.max_points, self.info()[2]) if pcap is None else pcap); pc = max(pcap, 0)
        d = [self._dev(x) for x in (np.full(N, -1, 'i4'), np.full(N, -1, 'i4'), np.full(max(pc, 1), -1, 'i4'), np.full(max(pc, 1), -1, 'i4'),
                                    np.zeros(COVIS_LOOP_REPORT_DTYPE.itemsize, 'u1'))]
        self.loop_begin_dev(cur, d[0], d[1], pcap, d[2], d[3], d[4], stream)
        self._sync(stream)
        gid, gv, pid, pref, rep = [self._host(x) for x in d]
        r = rep.view(COVIS_LOOP_REPORT_DTYPE)[0].copy(); ng = int(r['n_group']); npt = min(int(r['n_points']), pc)
        return dict(status=int(r['status']), group_id=gid[:ng].copy(), group_vertex=gv[:ng].copy(), point_id=pid[:npt].copy(), point_ref=pref[:npt].copy(), report=r)

    def loop_connections_dev(self, cur, n_group, group_id_dev, lcap, lc_begin_dev, lc_j_dev, report_dev, stream=None):
        self._keep = (group_id_dev, lc_begin_dev, lc_j_dev, report_dev)
        self.lib.check(self.lib.dll.sgx_covis_loop_connections_dev(self.h, int(cur), int(n_group), _vp(group_id_dev), int(lcap), _vp(lc_begin_dev), _vp(lc_j_dev),
                                                                   _vp(report_dev), self._stream(stream)), 'sgx_covis_loop_connections_dev')

    def loop_connections(self, cur, group_id, lcap=None, stream=None):
        """CorrectLoop :546-564 after the caller's fusion: per member in list order its previous list, UpdateConnections, LoopConnections = the keys of its row minus
        the previous list minus the group.  Returns status, lc_begin (CSR over the members in ascending id; None for a refused group row), lc_j (ids ascending per row,
        the rows that fit wholly) and the report."""
        g = _i4(group_id); ng = len(g)
        lcap = int(ng * self.max_keyframes if lcap is None else lcap); lc = max(lcap, 0)
        d = [self._dev(x) for x in (g, np.full(ng + 1, -1, 'i4'), np.full(max(lc, 1), -1, 'i4'), np.zeros(COVIS_LOOP_REPORT_DTYPE.itemsize, 'u1'))]
        self.loop_connections_dev(cur, ng, d[0], lcap, d[1], d[2], d[3], stream)
        self._sync(stream)
        _, beg, lj, rep = [self._host(x) for x in d]
        r = rep.view(COVIS_LOOP_REPORT_DTYPE)[0].copy()
        if int(r['status']) == -1: return dict(status=-1, lc_begin=None, lc_j=None, report=r, raw=(beg, lj))
        nw = int(beg[np.searchsorted(beg, lc, side='right') - 1])
        return dict(status=int(r['status']), lc_begin=beg.copy(), lc_j=lj[:nw].copy(), report=r, raw=(beg, lj))

    def essential_graph_dev(self, cur, loop, n_group, group_id_dev, lcap, lc_begin_dev, lc_j_dev, vertex_id_dev, vertex_fixed_dev, vertex_group_dev, ecap, e_i_dev, e_j_dev,
                            e_kind_dev, report_dev, stream=None):
        self._keep = (group_id_dev, lc_begin_dev, lc_j_dev, vertex_id_dev, vertex_fixed_dev, vertex_group_dev, e_i_dev, e_j_dev, e_kind_dev, report_dev)
        self.lib.check(self.lib.dll.sgx_covis_essential_graph_dev(self.h, int(cur), int(loop), int(n_group), _vp(group_id_dev), int(lcap), _vp(lc_begin_dev), _vp(lc_j_dev),
                                                                  _vp(vertex_id_dev), _vp(vertex_fixed_dev), _vp(vertex_group_dev), int(ecap), _vp(e_i_dev), _vp(e_j_dev),
                                                                  _vp(e_kind_dev), _vp(report_dev), self._stream(stream)), 'sgx_covis_essential_graph_dev')

    def essential_graph(self, cur, loop, group_id, lc_begin, lc_j, ecap=None, stream=None):
        """The vertices and edges of Optimizer::OptimizeEssentialGraph (Optimizer.cc:797-983) for the group row of loop_begin and the CSR of loop_connections.  Returns
        status, vertex_id, vertex_fixed, vertex_group, e_i, e_j, e_kind (0 loop connection, 1 spanning tree, 2 loop edge, 3 covisibility) and the report."""
        g = _i4(group_id); b = _i4(lc_begin); j = _i4(lc_j); ng = len(g); N = self.max_keyframes
        assert len(b) == ng + 1
        n = self.size()
        ecap = int(len(j) + n * (n + 1) // 2 + n + self.loop_info()[1] if ecap is None else ecap); ec = max(ecap, 0)
        d = [self._dev(x) for x in (g, b, j if len(j) else np.zeros(1, 'i4'), np.full(N, -1, 'i4'), np.full(N, 255, 'u1'), np.full(N, -9, 'i4'), np.full(max(ec, 1), -1, 'i4'),
                                    np.full(max(ec, 1), -1, 'i4'), np.full(max(ec, 1), 255, 'u1'), np.zeros(COVIS_LOOP_REPORT_DTYPE.itemsize, 'u1'))]
        self.essential_graph_dev(cur, loop, ng, d[0], len(j), d[1], d[2], d[3], d[4], d[5], ecap, d[6], d[7], d[8], d[9], stream)
        self._sync(stream)
        _, _, _, vid, vfx, vgr, ei, ej, ek, rep = [self._host(x) for x in d]
        r = rep.view(COVIS_LOOP_REPORT_DTYPE)[0].copy(); st = int(r['status'])
        raw = (vid, vfx, vgr, ei, ej, ek)
        if st == -1: return dict(status=st, report=r, raw=raw)
        nv = int(r['n_vertices']); ne = min(int(r['n_edges']), ec)
        return dict(status=st, vertex_id=vid[:nv].copy(), vertex_fixed=vfx[:nv].copy(), vertex_group=vgr[:nv].copy(), e_i=ei[:ne].copy(), e_j=ej[:ne].copy(),
                    e_kind=ek[:ne].copy(), report=r, raw=raw)

    def correct_map_points(self, xw, ref, Srw, corrected_Swr, stream=None):
        """P' = correctedSwr.map(Srw.map(P)) through sgx_correct_map_points_dev, the form evaluated as written (bit-equal to the scalar restatement)"""
        x = np.ascontiguousarray(xw, 'f4').reshape(-1, 3); n = len(x)
        if n == 0: return x.copy()
        d = [self._dev(v) for v in (x, _i4(ref), np.ascontiguousarray(Srw, 'f8').reshape(-1, 8), np.ascontiguousarray(corrected_Swr, 'f8').reshape(-1, 8), np.zeros((n, 3), 'f4'))]
        self._keep = d
        self.lib.check(self.lib.dll.sgx_correct_map_points_dev(n, _vp(d[0]), _vp(d[1]), _vp(d[2]), _vp(d[3]), _vp(d[4]), self._stream(stream)), 'sgx_correct_map_points_dev')
        self._sync(stream)
        return np.array(self._host(d[4]), 'f4')

    def correct_loop(self, cur, loop, Scw, Tcw, xw, fuse=None, fix_scale=True, point_ref_kf=None, iterations=20, stream=None):
        """LoopClosing::CorrectLoop (LoopClosing.cc:432-573) with Optimizer::OptimizeEssentialGraph, in the reference's order: loop_begin, the Sim3 propagation and the
        first point correction (:440-512), the caller's fusion fuse(self, begin, corrected) through replace_point / set_observations (:519-545, SearchAndFuse),
        loop_connections, essential_graph, the flattening, the optimisation, the pose recovery and the second point correction (Optimizer.cc:1013-1041), add_loop_edge.
        Tcw: the pose of every live keyframe by id (a dict, or an array indexed by id; 4 x 4 or 3 x 4); xw: the world positions by point id.  point_ref_kf (optional):
        GetReferenceKeyFrame()->mnId by point id, for the points outside the group; without it the second correction covers the group's points only.
        Returns the new poses by id (3 x 4 float32), the new points, and every intermediate row."""
        from .optimizer import Optimizer
        lib = self.lib
        pose = lambda k: np.asarray(Tcw[int(k)], 'f4')[:3, :4]
        xw = np.array(xw, 'f4').reshape(-1, 3)
        b = self.loop_begin(cur, stream=stream)
        assert b['status'] == 0
        non, cor, cTiw = Optimizer.PropagateLoopSim3([pose(k) for k in b['group_id']], Scw, lib=lib)
        cSwi = Optimizer.RecoverEssentialGraph(cor, lib=lib)[1]
        if len(b['point_id']): xw[b['point_id']] = self.correct_map_points(xw[b['point_id']], b['point_ref'], non, cSwi, stream)
        if fuse is not None: fuse(self, b, cor)
        c = self.loop_connections(cur, b['group_id'], stream=stream)
        assert c['status'] == 0
        g = self.essential_graph(cur, loop, b['group_id'], c['lc_begin'], c['lc_j'], stream=stream)
        assert g['status'] == 0
        S_in, e_meas = Optimizer.FlattenEssentialGraph(g, [pose(k) for k in g['vertex_id']], cor, non, lib=lib)
        S_out, stats = Optimizer.OptimizeEssentialGraph(S_in, g['vertex_fixed'], g['e_i'], g['e_j'], e_meas, fix_scale, iterations, lib=lib)
        Tnew, cSwc = Optimizer.RecoverEssentialGraph(S_out, lib=lib)
        ids = b['point_id']; ref = b['group_vertex'][b['point_ref']] if len(ids) else np.zeros(0, 'i4')
        if point_ref_kf is not None:                                               # every existing point: mnCorrectedReference inside the group, the reference keyframe outside
            vi = {int(k): j for j, k in enumerate(g['vertex_id'])}; mine = dict(zip([int(p) for p in ids], [int(r) for r in ref]))
            ids = self.global_ba_graph(stream=stream)['point_id']
            ref = np.array([mine[int(p)] if int(p) in mine else vi[int(point_ref_kf[int(p)])] for p in ids], 'i4')
        if len(ids): xw[ids] = self.correct_map_points(xw[ids], ref, S_in, cSwc, stream)
        if cur != loop: self.add_loop_edge(loop, cur)
        return dict(Tcw={int(k): Tnew[j] for j, k in enumerate(g['vertex_id'])}, xw=xw, begin=b, connections=c, graph=g, noncorrected=non, corrected=cor, corrected_Tiw=cTiw,
                    S_in=S_in, e_meas=e_meas, S_out=S_out, stats=stats, corrected_Swc=cSwc)

    # ---- DetectLoop: GetConnectedKeyFrames of a batch, and mvConsistentGroups as state of the handle
    def connected_batch_dev(self, Q, kf_ids_dev, off_dev, ids_dev, cap, report_dev, stream=None):
        self._keep = (kf_ids_dev, off_dev, ids_dev, report_dev)
        self.lib.check(self.lib.dll.sgx_covis_connected_batch_dev(self.h, int(Q), _vp(kf_ids_dev), _vp(off_dev), _vp(ids_dev), int(cap), _vp(report_dev),
                                                                  self._stream(stream)), 'sgx_covis_connected_batch_dev')

    def connected_batch(self, kf_ids, cap=None, stream=None):
        """GetConnectedKeyFrames() of the listed keyframes as a CSR of ascending ids (dead entries left out): the conn_offsets / conn_ids of
        KeyFrameDatabase.DetectLoopCandidates.  Returns off (whole), ids (the leading rows that were written), status per query, n per query, and the raw id row."""
        k = _i4(kf_ids); Q = len(k)
        cap = int(Q * self.max_keyframes if cap is None else cap); c = max(cap, 0)
        d = [self._dev(x) for x in (k, np.full(Q + 1, -1, 'i4'), np.full(max(c, 1), -1, 'i4'), np.zeros(Q * COVIS_REPORT_DTYPE.itemsize, 'u1'))]
        self.connected_batch_dev(Q, d[0], d[1], d[2], cap, d[3], stream)
        self._sync(stream)
        _, off, ids, rep = [self._host(x) for x in d]
        rep = rep.view(COVIS_REPORT_DTYPE)
        rows = [ids[off[q]:off[q + 1]].copy() if int(rep[q]['status']) == 0 else None for q in range(Q)]
        return dict(off=off.copy(), rows=rows, status=[int(r['status']) for r in rep], n=[int(r['n_counter']) for r in rep], raw=ids)

    def consistency_reserve(self, max_groups):
        self.lib.check(self.lib.dll.sgx_covis_consistency_reserve(self.h, int(max_groups)), 'sgx_covis_consistency_reserve')

    def consistency_clear(self):
        self.lib.check(self.lib.dll.sgx_covis_consistency_clear(self.h), 'sgx_covis_consistency_clear')

    def consistency_info(self):
        """(device bytes of the groups: 0 before they are reserved, groups stored, max_groups: 0 before)"""
        a = C.c_int64(); n = C.c_int32(); g = C.c_int32()
        self.lib.check(self.lib.dll.sgx_covis_consistency_info(self.h, C.byref(a), C.byref(n), C.byref(g)), 'sgx_covis_consistency_info')
        return a.value, n.value, g.value

    def consistent_groups(self):
        """mvConsistentGroups as [(members as ascending ids, counter)] in stored order"""
        G = self.consistency_info()[2]
        n = C.c_int32(); cnt = np.zeros(max(G, 1), 'i4'); off = np.zeros(G + 1, 'i4'); ids = np.zeros(max(G * self.max_keyframes, 1), 'i4')
        self.lib.check(self.lib.dll.sgx_covis_get_consistent_groups(self.h, C.byref(n), _vp(cnt), _vp(off), len(ids), _vp(ids)), 'sgx_covis_get_consistent_groups')
        return [([int(x) for x in ids[off[g]:off[g + 1]]], int(cnt[g])) for g in range(n.value)]

    def consistency_dev(self, cand_dev, n_cand_dev, th, enough_dev, n_enough_dev, report_dev, stream=None):
        self._keep = (cand_dev, n_cand_dev, enough_dev, n_enough_dev, report_dev)
        self.lib.check(self.lib.dll.sgx_covis_consistency_dev(self.h, _vp(cand_dev), _vp(n_cand_dev), int(th), _vp(enough_dev), _vp(n_enough_dev), _vp(report_dev),
                                                              self._stream(stream)), 'sgx_covis_consistency_dev')

    def consistency(self, candidates, th=3, max_groups=None, stream=None):
        """LoopClosing::DetectLoop :152-211 for vpCandidateKFs as ids: the groups of the handle are replaced, and mvpEnoughConsistentCandidates comes back as ids.
        max_groups: the capacity, if this is the call that reserves the groups.  Returns status, enough (None unless status is 0), the report, and the raw rows."""
        c = _i4(candidates)
        if max_groups is not None: self.consistency_reserve(max_groups)
        d = [self._dev(x) for x in (c if len(c) else np.zeros(1, 'i4'), np.array([len(c)], 'i4'), np.full(self.max_keyframes, -7, 'i4'), np.full(1, -7, 'i4'),
                                    np.zeros(COVIS_CONSISTENCY_REPORT_DTYPE.itemsize, 'u1'))]
        self.consistency_dev(d[0], d[1], th, d[2], d[3], d[4], stream)
        self._sync(stream)
        _, _, en, nen, rep = [self._host(x) for x in d]
        r = rep.view(COVIS_CONSISTENCY_REPORT_DTYPE)[0].copy(); st = int(r['status'])
        return dict(status=st, enough=[int(x) for x in en[:int(nen[0])]] if st == 0 else None, report=r, raw=(en, nen))

    # ---- RunGlobalBundleAdjustment's map update
    GBA_ORIGIN_NOT_IN_GBA = 1

    def gba_update_dev(self, n_origins, origins_dev, nk, kf_ids_dev, in_gba_dev, Tcw_dev, TcwGBA_dev, Tcw_out_dev, TcwBef_dev, kf_state_dev, report_dev, stream=None):
        self._keep = (origins_dev, kf_ids_dev, in_gba_dev, Tcw_dev, TcwGBA_dev, Tcw_out_dev, TcwBef_dev, kf_state_dev, report_dev)
        self.lib.check(self.lib.dll.sgx_covis_gba_update_dev(self.h, int(n_origins), _vp(origins_dev), int(nk), _vp(kf_ids_dev), _vp(in_gba_dev), _vp(Tcw_dev), _vp(TcwGBA_dev),
                                                             _vp(Tcw_out_dev), _vp(TcwBef_dev), _vp(kf_state_dev), _vp(report_dev), self._stream(stream)), 'sgx_covis_gba_update_dev')

    def correct_points_gba_dev(self, n, xw_dev, in_gba_dev, xw_gba_dev, ref_dev, kf_state_dev, TcwBef_dev, Tcw_out_dev, xw_out_dev, stream=None):
        self._keep2 = (xw_dev, in_gba_dev, xw_gba_dev, ref_dev, kf_state_dev, TcwBef_dev, Tcw_out_dev, xw_out_dev)
        self.lib.check(self.lib.dll.sgx_gba_correct_points_dev(int(n), _vp(xw_dev), _vp(in_gba_dev), _vp(xw_gba_dev), _vp(ref_dev), _vp(kf_state_dev), _vp(TcwBef_dev),
                                                               _vp(Tcw_out_dev), _vp(xw_out_dev), self._stream(stream)), 'sgx_gba_correct_points_dev')

    def gba_update(self, origins, kf_ids, in_gba, Tcw, TcwGBA, points=None, poison=None, stream=None):
        """LoopClosing::RunGlobalBundleAdjustment :676-737 after global BA.  kf_ids lists every live keyframe once; in_gba = mnBAGlobalForKF == nLoopKF; Tcw / TcwGBA
        3 x 4 (or 4 x 4) per row; origins = mvpKeyFrameOrigins as ids.  points (optional) = dict(xw, in_gba, xw_gba, ref = row of the reference keyframe or -1).
        Returns status, Tcw_out, TcwBef, kf_state, report and with points xw_out; the outputs start from the 32-bit pattern `poison` (default 0), so what a call did not write shows."""
        o = _i4(origins); k = _i4(kf_ids); nk = len(k)
        g = np.ascontiguousarray(np.asarray(in_gba).reshape(-1) != 0, 'u1'); assert len(g) == nk
        T = np.ascontiguousarray(np.asarray(Tcw, 'f4').reshape(nk, -1, 4)[:, :3, :]); Tg = np.ascontiguousarray(np.asarray(TcwGBA, 'f4').reshape(nk, -1, 4)[:, :3, :])
        fill = lambda shape: np.full(shape, 0 if poison is None else int(poison), 'u4').view('f4')      # poison: a 32-bit pattern
        d = [self._dev(x) for x in (o, k, g, T, Tg, fill((nk, 3, 4)), fill((nk, 3, 4)), np.full(nk, 0x55, 'u1'), np.zeros(COVIS_GBA_REPORT_DTYPE.itemsize, 'u1'))]
        self.gba_update_dev(len(o), d[0], nk, d[1], d[2], d[3], d[4], d[5], d[6], d[7], d[8], stream)
        out = {}
        if points is not None:
            x = np.ascontiguousarray(points['xw'], 'f4').reshape(-1, 3); n = len(x)
            pg = np.ascontiguousarray(np.asarray(points['in_gba']).reshape(-1) != 0, 'u1'); xg = np.ascontiguousarray(points['xw_gba'], 'f4').reshape(-1, 3); ref = _i4(points['ref'])
            assert len(pg) == len(xg) == len(ref) == n and (ref >= -1).all() and (ref < nk).all()
            self._sync(stream)
            if int(self._host(d[8]).view(COVIS_GBA_REPORT_DTYPE)[0]['status']) == 0 and n:
                e = [self._dev(v) for v in (x, pg, xg, ref, fill((n, 3)))]
                self.correct_points_gba_dev(n, e[0], e[1], e[2], e[3], d[7], d[6], d[5], e[4], stream)
                self._sync(stream)
                out['xw_out'] = np.array(self._host(e[4]), 'f4')
            else: out['xw_out'] = None if n else x.copy()
        self._sync(stream)
        r = self._host(d[8]).view(COVIS_GBA_REPORT_DTYPE)[0].copy()
        out.update(status=int(r['status']), Tcw_out=np.array(self._host(d[5]), 'f4'), TcwBef=np.array(self._host(d[6]), 'f4'), kf_state=np.array(self._host(d[7]), 'u1'), report=r)
        return out

    def close(self):
        if self.h: self.lib.dll.sgx_covis_destroy(self.h); self.h = C.c_void_p()

    def __del__(self):
        try: self.close()
        except Exception: pass
