"""GlobalMap — MapViewer's accumulating dense cloud (src/sg-slam/src/PointcloudMapping.cc:332-360, /SG_SLAM/Global_Point_Clouds) over the C ABI (sgx_globalmap_*): the
filtered temp_globalMap of every keyframe is appended to a device-resident map, and voxel_global + sor_global run over the whole map when the schedule says so.
GlobalMapSchedule is that schedule (count, pending, global_pc_update_kf_threshold) as host code.  DESIGN.md 9j."""
import ctypes as C
import numpy as np
from . import load
from .capi import (_vp, GlobalMapParams, GMAP_APPEND_DTYPE, GMAP_RESULT_DTYPE, CLOUD_POINT_DTYPE, CLOUD_RESULT_DTYPE, SGX_CLOUD_WORLD, SGX_GMAP_FEW_POINTS,
                   SGX_GMAP_LEAF_TOO_SMALL, SGX_GMAP_FULL, SGX_GMAP_MAX_POINTS, SGX_GMAP_MAX_RADIUS)


def make_globalmap_params(p):
    """GlobalMapParams from a dict with the keys of settings.load_global_map or settings.load_pointcloud_mapping (Sor_Global_*, Voxel_Global_LeafSize), from a dict
    with the short keys mean_k, stddev_mul, leaf, or a GlobalMapParams"""
    if isinstance(p, GlobalMapParams):
        return p
    if 'mean_k' in p:
        return GlobalMapParams(float(p['stddev_mul']), int(p['mean_k']), float(p['leaf']))
    return GlobalMapParams(float(p['Sor_Global_StddevMulThresh']), int(p['Sor_Global_MeanK']), float(p['Voxel_Global_LeafSize']))


def _as_points(points):
    a = np.asarray(points)
    if a.dtype == CLOUD_POINT_DTYPE: return np.ascontiguousarray(a)
    a = np.asarray(a, 'f4').reshape(-1, 3); p = np.zeros(len(a), CLOUD_POINT_DTYPE)
    p['x'], p['y'], p['z'] = a[:, 0], a[:, 1], a[:, 2]; p['rgba'] = 0xff000000
    return p


class GlobalMap:
    """One map of at most max_points points.  append / consolidate / points: host memory, synchronous.  append_batch_dev / launch: clouds that are on the device
    already, asynchronous on the current torch stream with nothing read back; with the kernel-logic emulator the "device" arrays are numpy arrays."""

    def __init__(self, params, max_points=1 << 20, lib=None):
        self.lib = lib or load(); self.params = make_globalmap_params(params); self.max_points = int(max_points)
        self.host = 'EMULATOR' in self.lib.version(); self.h = C.c_void_p()
        self.lib.check(self.lib.dll.sgx_globalmap_create(self.max_points, C.byref(self.params), C.byref(self.h)), 'sgx_globalmap_create')
        self.result = self._dev(np.zeros(GMAP_RESULT_DTYPE.itemsize, 'u1'))

    def _dev(self, a):
        if self.host: return np.ascontiguousarray(a)
        import torch
        return torch.from_numpy(np.ascontiguousarray(a)).cuda().contiguous()

    def _np(self, a):
        return a if self.host else a.cpu().numpy()

    def _stream(self):
        if self.host: return None
        import torch
        return C.c_void_p(torch.cuda.current_stream().cuda_stream)

    def reset(self):
        self.lib.check(self.lib.dll.sgx_globalmap_reset(self.h), 'sgx_globalmap_reset')

    def append(self, points):
        """`*globalMap += cloud` for one cloud from host memory (CLOUD_POINT_DTYPE records or an n x 3 float array); returns its record"""
        p = _as_points(points); rec = np.zeros(1, GMAP_APPEND_DTYPE)
        self.lib.check(self.lib.dll.sgx_globalmap_append(self.h, _vp(p) if len(p) else None, len(p), _vp(rec)), 'sgx_globalmap_append')
        return rec[0]

    def append_dev(self, points_dev, point_stride, n_points_dev, n_points_stride_bytes, n_clouds, records_dev=None, n_points_offset_bytes=0):
        """sgx_globalmap_append_batch_dev on raw device arrays; returns the device array of records (bytes)"""
        if records_dev is None: records_dev = self._dev(np.zeros(int(n_clouds) * GMAP_APPEND_DTYPE.itemsize, 'u1'))
        npd = C.c_void_p(_vp(n_points_dev).value + int(n_points_offset_bytes))
        self._inputs = (points_dev, n_points_dev, records_dev)                                # alive until the launch sequence has read them
        self.lib.check(self.lib.dll.sgx_globalmap_append_batch_dev(self.h, _vp(points_dev), int(point_stride), npd, int(n_points_stride_bytes), int(n_clouds), _vp(records_dev),
                                                                   self._stream()), 'sgx_globalmap_append_batch_dev')
        return records_dev

    def append_batch_dev(self, cloud_batch):
        """the clouds of the last launch of a PointCloudMappingBatch in WORLD mode, straight from its device buffers (the counts are its result records); nothing is
        read back: returns the device array of records, for read_records"""
        if cloud_batch.mode != SGX_CLOUD_WORLD: raise ValueError('the global map takes temp_globalMap: a PointCloudMappingBatch in SGX_CLOUD_WORLD mode')
        return self.append_dev(cloud_batch.points, cloud_batch.N, cloud_batch.results, CLOUD_RESULT_DTYPE.itemsize, cloud_batch.n,
                               n_points_offset_bytes=CLOUD_RESULT_DTYPE.fields['n_points'][1])

    def read_records(self, records_dev):
        if not self.host:
            import torch
            torch.cuda.current_stream().synchronize()
        return self._np(records_dev).view(GMAP_APPEND_DTYPE).copy()

    def launch(self):
        """the consolidation on the current torch stream; the record stays in self.result (device) until read()"""
        self.lib.check(self.lib.dll.sgx_globalmap_consolidate_dev(self.h, _vp(self.result), self._stream()), 'sgx_globalmap_consolidate_dev')

    def read(self):
        """the record of the last launch (waits for the current stream)"""
        if not self.host:
            import torch
            torch.cuda.current_stream().synchronize()
        return self._np(self.result).view(GMAP_RESULT_DTYPE)[0].copy()

    def consolidate(self):
        """voxel_global + sor_global over the whole map, synchronous; returns the record"""
        rec = np.zeros(1, GMAP_RESULT_DTYPE)
        self.lib.check(self.lib.dll.sgx_globalmap_consolidate(self.h, _vp(rec)), 'sgx_globalmap_consolidate')
        return rec[0]

    def size(self):
        n = C.c_int32(0)
        self.lib.check(self.lib.dll.sgx_globalmap_size(self.h, C.byref(n)), 'sgx_globalmap_size')
        return int(n.value)

    def points(self):
        """the map as CLOUD_POINT_DTYPE records (host copy)"""
        n = self.size(); p = np.zeros(n, CLOUD_POINT_DTYPE); m = C.c_int32(0)
        self.lib.check(self.lib.dll.sgx_globalmap_read(self.h, _vp(p) if n else None, n, C.byref(m)), 'sgx_globalmap_read')
        return p[:int(m.value)]

    def points_dev(self):
        """(address of the map's points, address of its int32 size) on the device, for a consumer on the same stream"""
        p = C.c_void_p(); n = C.c_void_p()
        self.lib.check(self.lib.dll.sgx_globalmap_points_dev(self.h, C.byref(p), C.byref(n)), 'sgx_globalmap_points_dev')
        return p.value, n.value

    def debug_read(self):
        """test tap: (voxel points, dist, kept flags, window tier) of the last consolidation, before the outlier filter"""
        n = C.c_int(0); N = self.max_points
        vox = np.zeros(N, CLOUD_POINT_DTYPE); dist = np.zeros(N, 'f4'); kept = np.zeros(N, 'u1'); tier = np.zeros(N, 'u1')
        self.lib.check(self.lib.tap('sgx_globalmap_debug_read')(self.h, _vp(vox), _vp(dist), _vp(kept), _vp(tier), N, C.byref(n)), 'sgx_globalmap_debug_read')
        return vox[:n.value].copy(), dist[:n.value].copy(), kept[:n.value].astype(bool), tier[:n.value].copy()

    def debug_max_radius(self, r):
        self.lib.check(self.lib.tap('sgx_globalmap_debug_max_radius')(self.h, int(r)), 'sgx_globalmap_debug_max_radius')

    def close(self):
        if self.h: self.lib.dll.sgx_globalmap_destroy(self.h); self.h = C.c_void_p()

    def __del__(self):
        try: self.close()
        except Exception: pass


class GlobalMapSchedule:
    """PointcloudMapping.cc:332-360 around a GlobalMap: after every appended keyframe `if (!pending || count > threshold)` consolidate and publish, count = 0 only
    when the published cloud is not empty, then count++ in every case.  `pending` (CheckNewKeyFrames()) is the caller's."""

    def __init__(self, gmap, threshold):
        self.map = gmap; self.threshold = int(threshold); self.count = 0; self.last_record = None

    def update(self, pending):
        """call after the keyframe's temp_globalMap was appended; returns the published cloud (CLOUD_POINT_DTYPE records, possibly empty) or None"""
        out = None
        if not pending or self.count > self.threshold:
            self.last_record = self.map.consolidate()
            out = self.map.points()
            if len(out): self.count = 0
        self.count += 1
        return out
