"""PointCloudMapping — Python mirror of src/sg-slam/src/PointcloudMapping.cc over the C ABI: the filtered cloud of a keyframe (generatePointCloud /
generatePointCloudForDyamic, MapViewer's voxel and outlier filters, slam_to_ros_mode_transform) and camera_to_map_tf, as octomap_server consumes them; the semantic
objects of the keyframe through the existing Detector3D; and PointCloudMappingBatch: the clouds of many keyframes in one launch sequence."""
import ctypes as C
import numpy as np
from . import load
from .capi import (_vp, CloudParams, CLOUD_POINT_DTYPE, CLOUD_RESULT_DTYPE, SGX_CLOUD_LOCAL, SGX_CLOUD_WORLD, SGX_CLOUD_FEW_POINTS, SGX_CLOUD_LEAF_TOO_SMALL,
                   SGX_CLOUD_MAX_BOXES)


def make_cloud_params(p, mode=SGX_CLOUD_LOCAL):
    """CloudParams from a dict with the keys of settings.load_pointcloud_mapping (Sor_Local_* / Voxel_Local_* in LOCAL mode, *_Global_* in WORLD mode), from a dict
    with the short keys mean_k, stddev_mul, leaf, consider_dynamic, depth_min, depth_max, or a CloudParams"""
    if isinstance(p, CloudParams):
        return p
    if 'mean_k' in p:
        return CloudParams(float(p['stddev_mul']), int(p['mean_k']), int(bool(p['consider_dynamic'])), float(p['leaf']), float(p['depth_min']), float(p['depth_max']), 0)
    w = 'Local' if mode == SGX_CLOUD_LOCAL else 'Global'
    return CloudParams(float(p['Sor_%s_StddevMulThresh' % w]), int(p['Sor_%s_MeanK' % w]), int(bool(p['is_map_construction_consider_dynamic'])),
                       float(p['Voxel_%s_LeafSize' % w]), float(p['camera_valid_depth_Min']), float(p['camera_valid_depth_Max']), 0)


def camera_to_map_tf(Tcw, lib=None):
    """(origin, rotation = x, y, z, w) of MapViewer's camera_to_map_tf (:254-265) from the keyframe's float pose Tcw"""
    lib = lib or load()
    T = np.ascontiguousarray(Tcw, 'f4').reshape(16); o = np.zeros(3, 'f8'); q = np.zeros(4, 'f8')
    lib.check(lib.dll.sgx_cloud_camera_to_map_tf(_vp(T), _vp(o), _vp(q)), 'sgx_cloud_camera_to_map_tf')
    return o, q


def pose_inverse(Tcw):
    """KeyFrame::GetPoseInverse as KeyFrame::SetPose forms it, in float: Rwc = Rcw^T, Ow = -Rwc * tcw; as the double 4 x 4 that transformPointCloud takes"""
    T = np.asarray(Tcw, 'f4').reshape(4, 4)
    Rwc = T[:3, :3].T
    Ow = (-(Rwc.astype('f8') @ T[:3, 3].astype('f8'))).astype('f4')
    Twc = np.eye(4, dtype='f8'); Twc[:3, :3] = Rwc; Twc[:3, 3] = Ow
    return Twc


def _boxes(map_boxes):
    """n x (x, y, w, h) float from rect tuples or Object2D-like tuples (id, prob, rect) / (id, name, prob, rect)"""
    out = []
    for b in map_boxes or ():
        r = b[-1] if len(b) in (3, 4) and hasattr(b[-1], '__len__') else b
        out.append([float(v) for v in r])
    return np.array(out, 'f4').reshape(-1, 4)


class _CloudHandle:
    def __init__(self, params, width, height, cam, mode, max_images, max_boxes, lib):
        self.lib = lib or load(); self.mode = int(mode); self.params = make_cloud_params(params, self.mode)
        self.width = int(width); self.height = int(height); self.N = self.width * self.height
        self.cam = np.ascontiguousarray(cam, 'f4').reshape(4); self.max_images = int(max_images); self.max_boxes = int(max_boxes); self.h = C.c_void_p()
        self.lib.check(self.lib.dll.sgx_cloud_create(self.width, self.height, self.max_images, self.max_boxes, self.mode, C.byref(self.params), C.byref(self.h)), 'sgx_cloud_create')

    def debug_read(self, image=0):
        """test tap: (voxel points CLOUD_POINT_DTYPE, dist, kept flags) of a keyframe of the last call, before the outlier filter"""
        n = C.c_int(0); vox = np.zeros(self.N, CLOUD_POINT_DTYPE); dist = np.zeros(self.N, 'f4'); kept = np.zeros(self.N, 'u1')
        self.lib.check(self.lib.tap('sgx_cloud_debug_read')(self.h, int(image), _vp(vox), _vp(dist), _vp(kept), self.N, C.byref(n)), 'sgx_cloud_debug_read')
        return vox[:n.value].copy(), dist[:n.value].copy(), kept[:n.value].astype(bool)

    def close(self):
        if self.h: self.lib.dll.sgx_cloud_destroy(self.h); self.h = C.c_void_p()

    def __del__(self):
        try: self.close()
        except Exception: pass


class CloudBuilder(_CloudHandle):
    """one keyframe per call from host memory (sgx_cloud_build)"""

    def __init__(self, params, width, height, cam, mode=SGX_CLOUD_LOCAL, max_boxes=SGX_CLOUD_MAX_BOXES, lib=None):
        super().__init__(params, width, height, cam, mode, 1, max_boxes, lib)

    def build(self, depth, color, Twc=None, map_boxes=(), have_dynamic=False):
        """(points CLOUD_POINT_DTYPE[n_points], the sgx_cloud_result record)"""
        d = np.ascontiguousarray(depth, 'f4'); c = np.ascontiguousarray(color, 'u1'); assert d.shape == (self.height, self.width) and c.shape == (self.height, self.width, 3)
        T = None if Twc is None else np.ascontiguousarray(Twc, 'f8').reshape(16)
        b = _boxes(map_boxes); pts = np.zeros(self.N, CLOUD_POINT_DTYPE); rec = np.zeros(1, CLOUD_RESULT_DTYPE)
        self.lib.check(self.lib.dll.sgx_cloud_build(self.h, _vp(d), _vp(c), _vp(self.cam), _vp(T), _vp(b) if len(b) else None, len(b), int(bool(have_dynamic)), _vp(pts), self.N,
                                                    _vp(rec)), 'sgx_cloud_build')
        return pts[:int(rec[0]['n_points'])].copy(), rec[0]


class PointCloudMapping:
    """The reference class for one keyframe at a time: insertKeyFrame returns what MapViewer publishes for it.  params: settings.load_pointcloud_mapping;
    detector3d_params: settings.load_mapping (needed when is_octo_semantic_map_construction is set and objects are passed)"""

    def __init__(self, params, width, height, cam, detector3d_params=None, lib=None, max_boxes=SGX_CLOUD_MAX_BOXES, global_map=None, global_map_max_points=1 << 20):
        """global_map: settings.load_global_map's dict (default: the *_Global_* keys of params and a global_pc_update_kf_threshold of 25, the value of the reference's
        example settings); global_map_max_points: the capacity of self.globalMap"""
        self.lib = lib or load(); self.params = dict(params); self.width = int(width); self.height = int(height); self.cam = np.ascontiguousarray(cam, 'f4').reshape(4)
        self.is_octo_semantic_map_construction = bool(params.get('is_octo_semantic_map_construction', 1))
        self.is_global_pc_reconstruction = bool(params.get('is_global_pc_reconstruction', 0))
        self.is_map_construction_consider_dynamic = bool(params.get('is_map_construction_consider_dynamic', 0))
        self.local = CloudBuilder(params, width, height, cam, SGX_CLOUD_LOCAL, max_boxes, lib=self.lib)
        self.world = CloudBuilder(params, width, height, cam, SGX_CLOUD_WORLD, max_boxes, lib=self.lib) if self.is_global_pc_reconstruction else None
        self.mpDetector3D = None
        if self.is_octo_semantic_map_construction and detector3d_params is not None:
            from .detector3d import Detector3D
            self.mpDetector3D = Detector3D(detector3d_params, width, height, cam, lib=self.lib)
        self.last_record = None; self.temp_globalMap = None; self.globalMap = None; self.global_schedule = None; self.last_append_record = None
        if self.is_global_pc_reconstruction:
            from .globalmap import GlobalMap, GlobalMapSchedule
            g = dict(global_map) if global_map is not None else dict(params)
            self.globalMap = GlobalMap(g, global_map_max_points, lib=self.lib)
            self.global_schedule = GlobalMapSchedule(self.globalMap, g.get('global_pc_update_kf_threshold', 25))

    def insertKeyFrame(self, color, depth, Tcw, objects2d=(), map_boxes=(), have_dynamic=False):
        """color: height x width x 3 bytes as mImRGB, depth: float metres, Tcw: the keyframe's float pose, objects2d: mvObjects2D (the tuples of
        detector.Detector2D.detect), map_boxes / have_dynamic: mvPotentialDynamicBorderForMapping / mbHaveDynamicObjectForMapping.  Returns (localMap as
        CLOUD_POINT_DTYPE records in ROS axes, (origin, rotation) of camera_to_map_tf).  Objects found go into mpDetector3D.mpObjectDatabase (:145-151, :189-190); with
        is_global_pc_reconstruction the keyframe's filtered temp_globalMap is left in self.temp_globalMap and appended to self.globalMap (:339; its record in
        self.last_append_record); update_global runs the rest of :332-360."""
        Twc = pose_inverse(Tcw)
        if self.mpDetector3D is not None and len(objects2d) > 0:
            self.mpDetector3D.Detect(list(objects2d), depth, Twc)
        pts, rec = self.local.build(depth, color, None, map_boxes, have_dynamic)
        self.last_record = rec
        if self.world is not None:
            self.temp_globalMap, self.last_world_record = self.world.build(depth, color, Twc, map_boxes, have_dynamic)
            self.last_append_record = self.globalMap.append(self.temp_globalMap)
        return pts, camera_to_map_tf(Tcw, lib=self.lib)

    def update_global(self, pending):
        """the schedule of :340-359 after insertKeyFrame: pending = CheckNewKeyFrames().  When no keyframe is waiting or more than global_pc_update_kf_threshold
        keyframes went by since the last publication, voxel_global + sor_global run over the whole of self.globalMap and the map is returned (CLOUD_POINT_DTYPE
        records in ROS axes, what /SG_SLAM/Global_Point_Clouds carries); otherwise None"""
        if self.global_schedule is None: return None
        return self.global_schedule.update(pending)

    def close(self):
        for o in (self.local, self.world, self.mpDetector3D, self.globalMap):
            if o is not None: o.close()

    def __del__(self):
        try: self.close()
        except Exception: pass


class PointCloudMappingBatch(_CloudHandle):
    """The clouds of many keyframes in one launch sequence (sgx_cloud_build_batch_dev), asynchronous on the current torch stream; with the kernel-logic emulator
    the "device" arrays are numpy arrays."""

    def __init__(self, params, width, height, cam, max_images, mode=SGX_CLOUD_LOCAL, max_boxes=SGX_CLOUD_MAX_BOXES, lib=None):
        super().__init__(params, width, height, cam, mode, max_images, max_boxes, lib)
        self.host = 'EMULATOR' in self.lib.version(); self.n = 0
        self.points = self._dev(np.zeros(self.max_images * self.N, CLOUD_POINT_DTYPE).view('u1'))
        self.results = self._dev(np.zeros(self.max_images * CLOUD_RESULT_DTYPE.itemsize, 'u1'))

    def _dev(self, a):
        if self.host: return np.ascontiguousarray(a)
        import torch
        return torch.from_numpy(np.ascontiguousarray(a)).cuda().contiguous()

    def _stream(self):
        if self.host: return None
        import torch
        return C.c_void_p(torch.cuda.current_stream().cuda_stream)

    def launch(self, depths, colors, Twcs=None, boxes=None, have_dynamic=None):
        """depths: n x height x width float, colors: n x height x width x 3 bytes (numpy, or device tensors already), Twcs: n x 4 x 4 double (WORLD mode),
        boxes: a list of n rect lists, have_dynamic: n flags; the clouds stay in self.points / self.results (device) until read()"""
        d = depths if hasattr(depths, 'data_ptr') else self._dev(np.asarray(depths, 'f4'))
        c = colors if hasattr(colors, 'data_ptr') else self._dev(np.asarray(colors, 'u1'))
        n = int(d.shape[0]); assert tuple(d.shape[1:]) == (self.height, self.width) and tuple(c.shape) == (n, self.height, self.width, 3)
        T = None if Twcs is None else (Twcs if hasattr(Twcs, 'data_ptr') else self._dev(np.asarray(Twcs, 'f8').reshape(n, 16)))
        B = nb = hv = None
        if boxes is not None:
            bh = np.zeros((n, max(self.max_boxes, 1), 4), 'f4'); cnt = np.zeros(n, 'i4')
            for i, bl in enumerate(boxes):
                b = _boxes(bl)
                if len(b) > self.max_boxes: raise ValueError('more rects than max_boxes')
                bh[i, :len(b)] = b; cnt[i] = len(b)
            hd = np.zeros(n, 'i4') if have_dynamic is None else np.asarray(have_dynamic).astype('i4')
            B, nb, hv = self._dev(bh[:, :self.max_boxes] if self.max_boxes else bh), self._dev(cnt), self._dev(hd)
        self.n = n; self._inputs = (d, c, T, B, nb, hv)                 # alive until the launch sequence has read them
        self.lib.check(self.lib.dll.sgx_cloud_build_batch_dev(self.h, _vp(d), self.width, _vp(c), 3 * self.width, n, _vp(self.cam), _vp(T), _vp(B), _vp(nb), _vp(hv),
                                                              _vp(self.points), _vp(self.results), self._stream()), 'sgx_cloud_build_batch_dev')

    def read(self):
        """[(points, record)] of the last launch"""
        r = (self.results if self.host else self.results.cpu().numpy()).view(CLOUD_RESULT_DTYPE)[:self.n].copy()
        p = (self.points if self.host else self.points.cpu().numpy()).view(CLOUD_POINT_DTYPE)
        return [(p[i * self.N:i * self.N + int(r[i]['n_points'])].copy(), r[i]) for i in range(self.n)]

    def build(self, depths, colors, Twcs=None, boxes=None, have_dynamic=None):
        self.launch(depths, colors, Twcs, boxes, have_dynamic)
        return self.read()
