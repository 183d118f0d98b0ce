"""KeyFrameStore — what LocalMapping reads of a keyframe, on the device, over the C ABI (sgx_kfstore_*), and LocalMapping::CreateNewMapPoints over it.

A keyframe is stored once: mvKeysUn, mvKeys, descriptors, mvuRight, mvDepth, the pose and its features grouped by vocabulary node (the FeatureVector).  Mutations take
host arrays and are synchronous.  create_new_map_points walks the neighbours of a keyframe in one launch (LocalMapping.cc:207-452: the baseline gate, ComputeF12,
SearchForTriangulation, the triangulation of every pair, the commit and the two MapPoint post-steps); create_new_map_points_batch_dev takes Q such queries as device
arrays on a stream.  The relation keyframe x map point stays in CovisibilityGraph: the queries take its keyframe_points rows."""
import ctypes as C
import numpy as np
from .capi import _vp, NEWPOINTS_REPORT_DTYPE
from .matcher import camera_struct


def _i4(v):
    return np.ascontiguousarray(v, 'i4').reshape(-1)


class KeyFrameStore:
    def __init__(self, cam, scale_factors, level_sigma2, max_keyframes=1024, cap=2048, lib=None):
        if lib is None:
            import sg_slam_amd
            lib = sg_slam_amd.load()
        self.lib = lib
        self.max_keyframes = int(max_keyframes); self.cap = int(cap)
        sf = np.ascontiguousarray(scale_factors, 'f4'); sg = np.ascontiguousarray(level_sigma2, 'f4')
        assert len(sf) == len(sg)
        self.scale_factors = sf.copy(); self.level_sigma2 = sg.copy()
        self.h = C.c_void_p()
        cs = camera_struct(cam)
        lib.check(lib.dll.sgx_kfstore_create(self.max_keyframes, self.cap, C.byref(cs), _vp(sf), _vp(sg), len(sf), C.byref(self.h)), 'sgx_kfstore_create')
        self._on_host = 'EMULATOR' in lib.version()               # the emulator's "device" memory is host memory
        self._n = {}                                              # keypoints per keyframe id

    def close(self):
        if self.h:
            self.lib.dll.sgx_kfstore_destroy(self.h); self.h = C.c_void_p()

    # ---- mutations (host arrays, synchronous)
    def add(self, kf_id, keys_un, desc, uright, depth, feat_node, Tcw, keys=None):
        """keys (mvKeys) defaults to keys_un; Tcw is 3 x 4 or 4 x 4"""
        ku = np.ascontiguousarray(keys_un); n = len(ku)
        kd = None if keys is None else np.ascontiguousarray(keys)
        d = np.ascontiguousarray(desc, np.uint8).reshape(-1, 32); u = np.ascontiguousarray(uright, 'f4').reshape(-1); z = np.ascontiguousarray(depth, 'f4').reshape(-1)
        f = _i4(feat_node); T = np.ascontiguousarray(np.asarray(Tcw, 'f4')[:3, :4])
        assert len(d) == len(u) == len(z) == len(f) == n and (kd is None or len(kd) == n)
        self.lib.check(self.lib.dll.sgx_kfstore_add(self.h, int(kf_id), n, _vp(ku), _vp(kd), _vp(d), _vp(u), _vp(z), _vp(f), _vp(T)), 'sgx_kfstore_add')
        self._n[int(kf_id)] = n

    def set_pose(self, kf_id, Tcw):
        T = np.ascontiguousarray(np.asarray(Tcw, 'f4')[:3, :4])
        self.lib.check(self.lib.dll.sgx_kfstore_set_pose(self.h, int(kf_id), _vp(T)), 'sgx_kfstore_set_pose')

    def erase(self, kf_id):
        self.lib.check(self.lib.dll.sgx_kfstore_erase(self.h, int(kf_id)), 'sgx_kfstore_erase')
        self._n.pop(int(kf_id), None)

    def clear(self):
        self.lib.check(self.lib.dll.sgx_kfstore_clear(self.h), 'sgx_kfstore_clear')
        self._n.clear()

    def size(self):
        return int(self.lib.dll.sgx_kfstore_size(self.h))

    def info(self):
        """(device bytes, of which workspace bytes)"""
        a = C.c_int64(); b = C.c_int64()
        self.lib.check(self.lib.dll.sgx_kfstore_info(self.h, C.byref(a), C.byref(b)), 'sgx_kfstore_info')
        return a.value, b.value

    # ---- device plumbing (as CovisibilityGraph)
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

    # ---- the query
    def create_new_map_points_batch_dev(self, Q, cur_ids_dev, nb_offsets_dev, nb_ids_dev, first_new_id_dev, median_depth_dev, mp_rows_dev, n_new_dev, new_kf2_dev, new_idx1_dev,
                                        new_idx2_dev, new_x3d_dev, new_desc_dev, new_normal_dev, new_min_dist_dev, new_max_dist_dev, report_dev,
                                        pair_idx1_dev=None, pair_idx2_dev=None, pair_ok_dev=None, stream=None):
        self._keep = (cur_ids_dev, nb_offsets_dev, nb_ids_dev, first_new_id_dev, median_depth_dev, mp_rows_dev, n_new_dev, new_kf2_dev, new_idx1_dev, new_idx2_dev, new_x3d_dev,
                      new_desc_dev, new_normal_dev, new_min_dist_dev, new_max_dist_dev, report_dev, pair_idx1_dev, pair_idx2_dev, pair_ok_dev)
        self.lib.check(self.lib.dll.sgx_create_new_map_points_batch_dev(self.h, int(Q), *[_vp(x) for x in self._keep], self._stream(stream)), 'sgx_create_new_map_points_batch_dev')

    def batch_buffers(self, queries, poison=None, pairs=True):
        """the host arrays of a batch, in the order of create_new_map_points_batch_dev: queries = [(cur, neighbours, rows, first_new_id, median_depth or None)], rows =
        1 + len(neighbours) lists of point ids.  Every byte of an output is `poison` (default 0)."""
        Q = len(queries); cap = self.cap
        off = np.zeros(Q + 1, 'i4'); off[1:] = np.cumsum([len(q[1]) for q in queries]); M = int(off[Q])
        nb = np.zeros(max(M, 1), 'i4'); rows = np.full((Q + M, cap), -1, 'i4')
        mono = Q > 0 and queries[0][4] is not None
        med = np.ones(max(M, 1), 'f4') if mono else None
        for q, (cur, nbs, rws, first, md) in enumerate(queries):
            assert (md is not None) == mono and len(rws) == len(nbs) + 1
            nb[off[q]:off[q + 1]] = nbs
            if mono: med[off[q]:off[q + 1]] = md
            for r, row in enumerate(rws): rows[q + off[q] + r, :len(row)] = row
        def f(shape, dt):                                          # every byte of an output starts as `poison`
            a = np.zeros(shape, dt)
            if poison is not None: a.view('u1').reshape(-1)[:] = poison
            return a
        return [_i4([q[0] for q in queries]) if Q else np.zeros(1, 'i4'), off, nb, _i4([q[3] for q in queries]) if Q else np.zeros(1, 'i4'), med, rows,
                f(max(Q, 1), 'i4'), f((max(Q, 1), cap), 'i4'), f((max(Q, 1), cap), 'i4'), f((max(Q, 1), cap), 'i4'), f((max(Q, 1), cap, 3), 'f4'), f((max(Q, 1), cap, 32), 'u1'),
                f((max(Q, 1), cap, 3), 'f4'), f((max(Q, 1), cap), 'f4'), f((max(Q, 1), cap), 'f4'), f(max(M, 1) * NEWPOINTS_REPORT_DTYPE.itemsize, 'u1'),
                f((max(M, 1), cap), 'i4') if pairs else None, f((max(M, 1), cap), 'i4') if pairs else None, f((max(M, 1), cap), 'u1') if pairs else None]

    def create_new_map_points_batch(self, queries, poison=None, pairs=True, stream=None, raw=False):
        """Q queries as one launch, read back.  One dict per query: rows (after), n_new, new_kf2 / new_idx1 / new_idx2 / x3d / desc / normal / min_dist / max_dist (trimmed
        to n_new), report (one record per neighbour) and pairs: per neighbour (idx1, idx2, ok) trimmed to n_pairs.  raw=True adds the untrimmed host arrays as 'raw'."""
        Q = len(queries)
        h = self.batch_buffers(queries, poison, pairs)
        d = [None if x is None else self._dev(x) for x in h]
        self.create_new_map_points_batch_dev(Q, *d, stream=stream)
        self._sync(stream)
        o = [None if x is None else self._host(x) for x in d]
        off = h[1]; rep = o[15].view(NEWPOINTS_REPORT_DTYPE)
        out = []
        for q, (cur, nbs, rws, first, md) in enumerate(queries):
            k = int(o[6][q]); a, b = int(off[q]), int(off[q + 1])
            r = dict(rows=[o[5][q + a + i, :len(row)].copy() for i, row in enumerate(rws)], n_new=k, new_kf2=o[7][q, :k].copy(), new_idx1=o[8][q, :k].copy(), new_idx2=o[9][q, :k].copy(),
                     x3d=o[10][q, :k].copy(), desc=o[11][q, :k].copy(), normal=o[12][q, :k].copy(), min_dist=o[13][q, :k].copy(), max_dist=o[14][q, :k].copy(), report=rep[a:b].copy())
            if pairs:
                r['pairs'] = [(o[16][j, :rep[j]['n_pairs']].copy(), o[17][j, :rep[j]['n_pairs']].copy(), o[18][j, :rep[j]['n_pairs']].copy()) for j in range(a, b)]
            out.append(r)
        if raw:
            for r in out: r['raw'] = o
        return out

    def create_new_map_points(self, cur, neighbours, rows, first_new_id, median_depth=None):
        """LocalMapping::CreateNewMapPoints of keyframe cur against `neighbours` (GetBestCovisibilityKeyFrames(nn), in order) through the synchronous batch-of-one entry.
        rows: mvpMapPoints of cur and of each neighbour as point ids, -1 none (CovisibilityGraph.keyframe_points).  median_depth (one per neighbour) selects the monocular
        gate.  Returns the dict of create_new_map_points_batch."""
        nbs = _i4(neighbours); M = len(nbs); cap = self.cap
        assert len(rows) == M + 1
        R = np.full((M + 1, cap), -1, 'i4')
        for r, row in enumerate(rows): R[r, :len(row)] = row
        med = None if median_depth is None else np.ascontiguousarray(median_depth, 'f4').reshape(-1)
        assert med is None or len(med) == M
        n = C.c_int32(); kf2 = np.zeros(cap, 'i4'); i1 = np.zeros(cap, 'i4'); i2 = np.zeros(cap, 'i4'); x = np.zeros((cap, 3), 'f4'); dd = np.zeros((cap, 32), 'u1')
        nr = np.zeros((cap, 3), 'f4'); mn = np.zeros(cap, 'f4'); mx = np.zeros(cap, 'f4'); rep = np.zeros(max(M, 1), NEWPOINTS_REPORT_DTYPE)
        p1 = np.zeros((max(M, 1), cap), 'i4'); p2 = np.zeros((max(M, 1), cap), 'i4'); pk = np.zeros((max(M, 1), cap), 'u1')
        self.lib.check(self.lib.dll.sgx_create_new_map_points(self.h, int(cur), M, _vp(nbs) if M else None, int(first_new_id), _vp(med), _vp(R), C.byref(n), _vp(kf2), _vp(i1), _vp(i2),
                                                              _vp(x), _vp(dd), _vp(nr), _vp(mn), _vp(mx), _vp(rep), _vp(p1), _vp(p2), _vp(pk)), 'sgx_create_new_map_points')
        k = n.value
        return dict(rows=[R[r, :len(row)].copy() for r, row in enumerate(rows)], n_new=k, new_kf2=kf2[:k].copy(), new_idx1=i1[:k].copy(), new_idx2=i2[:k].copy(), x3d=x[:k].copy(),
                    desc=dd[:k].copy(), normal=nr[:k].copy(), min_dist=mn[:k].copy(), max_dist=mx[:k].copy(), report=rep[:M].copy(),
                    pairs=[(p1[j, :rep[j]['n_pairs']].copy(), p2[j, :rep[j]['n_pairs']].copy(), pk[j, :rep[j]['n_pairs']].copy()) for j in range(M)])
