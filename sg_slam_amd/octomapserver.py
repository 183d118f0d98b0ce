"""OctomapServer — Python mirror of src/octomap_server/src/OctomapServer.cpp over the C ABI (sgx_octomap_*): the occupancy map that consumes the keyframe clouds of
PointCloudMapping.  insertCloudCallback's transform and PassThrough filters, insertScan's rays and updates, and the queries of publishAll that do not depend on ROS: the
occupied / free cell centres in the order of octomap's leaf iterator and the projected 2-D occupancy grid.  Occupancy only (no colour), no ground filter; DESIGN.md 9i."""
import ctypes as C
import numpy as np
from . import load
from .capi import (_vp, OctomapParams, OctomapGridHeader, OCTOMAP_RECORD_DTYPE, OCTOMAP_CELL_DTYPE, OCTOMAP_BOUNDS_DTYPE, CLOUD_POINT_DTYPE, CLOUD_RESULT_DTYPE,
                   SGX_OCTOMAP_ORIGIN_OUT_OF_RANGE, SGX_OCTOMAP_RAY_LEFT_KEYSPACE, SGX_OCTOMAP_MAP_FULL, SGX_OCTOMAP_TOO_MANY_POINTS, SGX_OCTOMAP_GRID_EMPTY,
                   SGX_OCTOMAP_GRID_KEY_OUT_OF_RANGE)

DBL_MAX = float(np.finfo('f8').max)
# octomap_server's defaults (OctomapServer.cpp:44-70)
DEFAULTS = dict(res=0.05, prob_hit=0.7, prob_miss=0.4, thres_min=0.12, thres_max=0.97, max_range=-1.0, pointcloud_min_x=-DBL_MAX, pointcloud_max_x=DBL_MAX,
                pointcloud_min_y=-DBL_MAX, pointcloud_max_y=DBL_MAX, pointcloud_min_z=-DBL_MAX, pointcloud_max_z=DBL_MAX, occupancy_min_z=-DBL_MAX, occupancy_max_z=DBL_MAX,
                min_size_x=0.0, min_size_y=0.0)


def make_octomap_params(p=None, **kw):
    """OctomapParams from octomap_server's defaults, a dict of the launch file's names (resolution / sensor_model/hit, /miss, /min, /max, sensor_model/max_range are
    accepted beside the field names) and keywords"""
    if isinstance(p, OctomapParams):
        return p
    alias = {'resolution': 'res', 'sensor_model/hit': 'prob_hit', 'sensor_model/miss': 'prob_miss', 'sensor_model/min': 'thres_min', 'sensor_model/max': 'thres_max',
             'sensor_model/max_range': 'max_range'}
    v = dict(DEFAULTS)
    for k, x in list((p or {}).items()) + list(kw.items()):
        k = alias.get(k, k)
        if k not in v: raise KeyError(k)
        v[k] = float(x)
    return OctomapParams(*[v[k] for k, _ in OctomapParams._fields_])


def sensor_to_world(origin, rotation, lib=None):
    """the 4 x 4 float sensorToWorld of insertCloudCallback (:275-288) from camera_to_map_tf's (origin, rotation = x, y, z, w)"""
    lib = lib or load()
    o = np.ascontiguousarray(origin, 'f8').reshape(3); q = np.ascontiguousarray(rotation, 'f8').reshape(4); out = np.zeros(16, 'f4')
    lib.check(lib.dll.sgx_octomap_sensor_to_world(_vp(o), _vp(q), _vp(out)), 'sgx_octomap_sensor_to_world')
    return out.reshape(4, 4)


class OctomapServer:
    """One map.  insert: one scan from host memory, synchronous.  insert_batch_dev: scans that are on the device already (the output of PointCloudMappingBatch), one
    asynchronous launch sequence on the current torch stream with nothing read back; with the kernel-logic emulator the "device" arrays are numpy arrays."""

    def __init__(self, params=None, max_bricks=1 << 14, max_points_per_scan=1 << 16, lib=None, **kw):
        self.lib = lib or load(); self.params = make_octomap_params(params, **kw); self.max_bricks = int(max_bricks); self.max_points = int(max_points_per_scan)
        self.host = 'EMULATOR' in self.lib.version(); self.h = C.c_void_p()
        self.lib.check(self.lib.dll.sgx_octomap_create(C.byref(self.params), self.max_bricks, self.max_points, C.byref(self.h)), 'sgx_octomap_create')

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

    def insert(self, points, sensor_to_world):
        """insertCloudCallback for one cloud: points as CLOUD_POINT_DTYPE records or an n x 3 float array; returns the scan's record"""
        p = _as_points(points); m = np.ascontiguousarray(sensor_to_world, 'f4').reshape(16); rec = np.zeros(1, OCTOMAP_RECORD_DTYPE)
        self.lib.check(self.lib.dll.sgx_octomap_insert(self.h, _vp(p) if len(p) else None, len(p), _vp(m), _vp(rec)), 'sgx_octomap_insert')
        return rec[0]

    def insertCloud(self, points, origin, rotation):
        """a cloud with the (origin, rotation) that camera_to_map_tf gave for its keyframe"""
        return self.insert(points, sensor_to_world(origin, rotation, lib=self.lib))

    def insert_batch_dev(self, points_dev, point_stride, n_points_dev, n_points_stride_bytes, sensor_to_world_dev, n_scans, records_dev=None, n_points_offset_bytes=0):
        """sgx_octomap_insert_batch_dev; returns the device array of records (bytes).  n_points_offset_bytes: where the first count stands in n_points_dev"""
        if records_dev is None: records_dev = self._dev(np.zeros(int(n_scans) * OCTOMAP_RECORD_DTYPE.itemsize, 'u1'))
        npd = _vp(n_points_dev); npd = C.c_void_p(npd.value + int(n_points_offset_bytes))
        self._inputs = (points_dev, n_points_dev, sensor_to_world_dev, records_dev)
        self.lib.check(self.lib.dll.sgx_octomap_insert_batch_dev(self.h, _vp(points_dev), int(point_stride), npd, int(n_points_stride_bytes), _vp(sensor_to_world_dev),
                                                                 int(n_scans), _vp(records_dev), self._stream()), 'sgx_octomap_insert_batch_dev')
        return records_dev

    def insert_clouds(self, cloud_batch, sensor_to_worlds):
        """the clouds of the last launch of a PointCloudMappingBatch, straight from its device buffers; returns the records"""
        n = cloud_batch.n; m = self._dev(np.ascontiguousarray(sensor_to_worlds, 'f4').reshape(n, 16))
        r = self.insert_batch_dev(cloud_batch.points, cloud_batch.N, cloud_batch.results, CLOUD_RESULT_DTYPE.itemsize, m, n,
                                  n_points_offset_bytes=CLOUD_RESULT_DTYPE.fields['n_points'][1])
        return self.read_records(r)

    def read_records(self, records_dev):
        if not self.host:
            import torch
            torch.cuda.current_stream().synchronize()
        return self._np(records_dev).view(OCTOMAP_RECORD_DTYPE).copy()

    def bounds(self):
        b = np.zeros(1, OCTOMAP_BOUNDS_DTYPE)
        self.lib.check(self.lib.dll.sgx_octomap_bounds(self.h, _vp(b)), 'sgx_octomap_bounds')
        return b[0]

    def cells(self, occupied=True):
        """the occupied or free cells inside the z window, in ascending Morton code (publishAll's traversal order)"""
        b = self.bounds(); cap = int(b['n_occupied'] if occupied else b['n_free']); out = np.zeros(cap, OCTOMAP_CELL_DTYPE); n = C.c_int32(0)
        self.lib.check(self.lib.dll.sgx_octomap_cells(self.h, int(bool(occupied)), _vp(out) if cap else None, cap, C.byref(n)), 'sgx_octomap_cells')
        return out[:n.value].copy()

    def search(self, keys=None, points=None):
        """log-odds of keys (m x 3 uint16) or points (m x 3 float); NaN where unknown"""
        assert (keys is None) != (points is None)
        a = np.ascontiguousarray(keys, 'u2').reshape(-1, 3) if keys is not None else np.ascontiguousarray(points, 'f4').reshape(-1, 3)
        m = len(a)
        if m == 0: return np.zeros(0, 'f4')
        d = self._dev(a); out = self._dev(np.zeros(m, 'f4'))
        self.lib.check(self.lib.dll.sgx_octomap_search_dev(self.h, _vp(d) if keys is not None else None, _vp(d) if keys is None else None, m, _vp(out), self._stream()),
                       'sgx_octomap_search_dev')
        if not self.host:
            import torch
            torch.cuda.current_stream().synchronize()
        return self._np(out).copy()

    def grid_header(self, bounds=None):
        b = np.array([self.bounds() if bounds is None else bounds], OCTOMAP_BOUNDS_DTYPE); hd = OctomapGridHeader()
        self.lib.check(self.lib.dll.sgx_octomap_grid_header(self.h, _vp(b), C.byref(hd)), 'sgx_octomap_grid_header')
        return hd

    def project(self):
        """(header, grid): nav_msgs::OccupancyGrid's info and data as a height x width int8 array"""
        hd = self.grid_header(); n = hd.width * hd.height; g = np.zeros(n, 'i1')
        if n:
            d = self._dev(g)
            self.lib.check(self.lib.dll.sgx_octomap_project_dev(self.h, C.byref(hd), _vp(d), self._stream()), 'sgx_octomap_project_dev')
            if not self.host:
                import torch
                torch.cuda.current_stream().synchronize()
            g = self._np(d).copy()
        return hd, g.reshape(hd.height, hd.width)

    def reset(self):
        self.lib.check(self.lib.dll.sgx_octomap_reset(self.h), 'sgx_octomap_reset')

    def close(self):
        if self.h: self.lib.dll.sgx_octomap_destroy(self.h); self.h = C.c_void_p()

    def __del__(self):
        try: self.close()
        except Exception: pass


def _as_points(points):
    a = np.asarray(points)
    if a.dtype == CLOUD_POINT_DTYPE: return np.ascontiguousarray(a)
    a = np.asarray(a, 'f4').reshape(-1, 3); p = np.zeros(len(a), CLOUD_POINT_DTYPE)
    p['x'], p['y'], p['z'] = a[:, 0], a[:, 1], a[:, 2]
    return p
