"""Detector3D / ObjectDatabase — Python mirror of src/sg-slam/src/Detector3D.cc and ObjectDatabase.cc over the C ABI: the semantic objects of a keyframe from the
boxes of Detector2D (mvObjects2D), its depth image and its pose (PointCloudMapping::generatePointCloud, PointcloudMapping.cc:145-151, :189-190), and
Detector3DBatch: the jobs of many keyframes in one launch sequence."""
import ctypes as C
import numpy as np
from . import load
from .capi import _vp, Obj3dParams, Obj3dJob, OBJ3D_RESULT_DTYPE, SemanticObjectRecord
from .detector import CLASS_NAMES


def full_image_crop_points(width, height):
    """cells of the largest crop: Detector2D only clamps its boxes to the image (Detector2D.cc:63-71), so a box can be the whole image and its crop the central 60 %
    of it (384 x 288 cells of a 640 x 480 image)"""
    return max(1, (int(int(width) * 0.8) - int(int(width) * 0.2)) * (int(int(height) * 0.8) - int(int(height) * 0.2)))


def make_params(p):
    """Obj3dParams from a dict with the keys of settings.load_mapping (or an Obj3dParams)"""
    if isinstance(p, Obj3dParams):
        return p
    return Obj3dParams(float(p['Sor_StddevMulThresh']), int(p['Sor_MeanK']), int(p['EuclideanClusterMinSize']), int(p['EuclideanClusterMaxSize']),
                       float(p.get('Voxel_LeafSize', 0.01)), float(p['EuclideanClusterTolerance']), float(p['DetectSimilarCompareRatio']),
                       float(p['camera_valid_depth_Min']), float(p['camera_valid_depth_Max']))


def _object2d(o):
    """(class id, prob, (x, y, w, h)) of an Object2D: the (id, name, prob, rect) tuples of detector.Detector2D.detect, or (id, prob, rect)"""
    if len(o) == 4:
        return int(o[0]), float(o[2]), tuple(float(v) for v in o[3])
    return int(o[0]), float(o[1]), tuple(float(v) for v in o[2])


class SemanticObject:
    """ObjectDatabase.h:12-24"""

    def __init__(self, class_id, prob, centroid, size, object_id=0, record=None):
        self.class_id = int(class_id); self.object_name = CLASS_NAMES[self.class_id] if 0 <= self.class_id < len(CLASS_NAMES) else str(self.class_id)
        self.prob = np.float32(prob); self.centroid = np.array(centroid, 'f4'); self.size = np.array(size, 'f4'); self.object_id = int(object_id)
        self.record = record          # the whole sgx_obj3d_result (diagnostics included) when the object comes from DetectOne

    def __repr__(self):
        return f'SemanticObject({self.object_id}, {self.object_name}, prob={self.prob:.3f}, centroid={self.centroid}, size={self.size})'


class ObjectDatabase:
    def __init__(self, lib=None):
        self.lib = lib or load(); self.h = C.c_void_p()
        self.lib.check(self.lib.dll.sgx_objdb_create(C.byref(self.h)), 'sgx_objdb_create')

    def addObject(self, cluster):
        """ObjectDatabase::addObject; returns (object_id, merged) and sets cluster.object_id when the object is appended, as the reference does"""
        r = SemanticObjectRecord(cluster.class_id, 0, float(cluster.prob), (C.c_float * 3)(*cluster.centroid), (C.c_float * 3)(*cluster.size))
        oid = C.c_int32(); merged = C.c_int32()
        self.lib.check(self.lib.dll.sgx_objdb_add(self.h, C.byref(r), C.byref(oid), C.byref(merged)), 'sgx_objdb_add')
        if not merged.value: cluster.object_id = oid.value
        return oid.value, bool(merged.value)

    def getDataBaseSize(self):
        return int(self.lib.dll.sgx_objdb_size(self.h))

    def getObject(self, index):
        r = SemanticObjectRecord()
        self.lib.check(self.lib.dll.sgx_objdb_get(self.h, int(index), C.byref(r)), 'sgx_objdb_get')
        return SemanticObject(r.class_id, r.prob, list(r.centroid), list(r.size), r.object_id)

    def getObjectByID(self, object_id):
        return self.getObject(object_id - 1)

    @property
    def mvSemanticObject(self):
        return [self.getObject(i) for i in range(self.getDataBaseSize())]

    def close(self):
        if self.h: self.lib.dll.sgx_objdb_destroy(self.h); self.h = C.c_void_p()

    def __del__(self):
        try: self.close()
        except Exception: pass


class Detector3D:
    def __init__(self, params, width, height, cam, lib=None, max_crop_points=None):
        """params: the Detector3D.* / camera_valid_depth_* values (settings.load_mapping); cam = (fx, fy, cx, cy)"""
        self.lib = lib or load(); self.params = make_params(params); self.width = int(width); self.height = int(height)
        self.cam = np.ascontiguousarray(cam, 'f4').reshape(4); self.h = C.c_void_p()
        cap = int(max_crop_points or full_image_crop_points(self.width, self.height))
        self.lib.check(self.lib.dll.sgx_obj3d_create(self.width, self.height, 1, 1, cap, C.byref(self.params), C.byref(self.h)), 'sgx_obj3d_create')
        self.mpObjectDatabase = ObjectDatabase(lib=self.lib)

    def detect_record(self, object2d, depth, Twc):
        """the sgx_obj3d_result record (numpy, OBJ3D_RESULT_DTYPE) of one Object2D"""
        cid, prob, (x, y, w, h) = _object2d(object2d)
        d = np.ascontiguousarray(depth, 'f4'); T = np.ascontiguousarray(Twc, 'f8').reshape(16)
        assert d.shape == (self.height, self.width)
        job = Obj3dJob(0, cid, prob, x, y, w, h); out = np.zeros(1, OBJ3D_RESULT_DTYPE)
        self.lib.check(self.lib.dll.sgx_obj3d_detect(self.h, _vp(d), _vp(self.cam), _vp(T), C.byref(job), _vp(out)), 'sgx_obj3d_detect')
        return out[0]

    def DetectOne(self, object2d, depth, Twc):
        """bool DetectOne(object2d, semantic_object, depth, cloud): the SemanticObject, or None where the reference returns false"""
        r = self.detect_record(object2d, depth, Twc)
        return SemanticObject(r['class_id'], r['prob'], r['centroid'], r['size'], record=r) if r['found'] else None

    def Detect(self, mvObjects2D, depth, Twc):
        """Detector3D::Detect (:26-39): every object found goes into mpObjectDatabase; returns them"""
        out = []
        for o in mvObjects2D:
            s = self.DetectOne(o, depth, Twc)
            if s is not None:
                self.mpObjectDatabase.addObject(s); out.append(s)
        return out

    def debug_read(self, job=0):
        """test tap: (kept flags, component labels) of the crop points of the last call"""
        n = C.c_int(0); cap = self.width * self.height
        kept = np.zeros(cap, 'u1'); lab = np.zeros(cap, 'i4')
        self.lib.check(self.lib.tap('sgx_obj3d_debug_read')(self.h, int(job), _vp(kept), _vp(lab), cap, C.byref(n)), 'sgx_obj3d_debug_read')
        return kept[:n.value].astype(bool), lab[:n.value].copy()

    def close(self):
        if self.h: self.lib.dll.sgx_obj3d_destroy(self.h); self.h = C.c_void_p()
        if getattr(self, 'mpObjectDatabase', None): self.mpObjectDatabase.close()

    def __del__(self):
        try: self.close()
        except Exception: pass


class Detector3DBatch:
    """The Object2D boxes of many keyframes in one launch sequence (sgx_obj3d_detect_batch_dev), asynchronous on the current torch stream; with the kernel-logic
    emulator the "device" arrays are numpy arrays."""

    def __init__(self, params, width, height, cam, max_images, max_jobs, lib=None, max_crop_points=None):
        self.lib = lib or load(); self.params = make_params(params); self.width = int(width); self.height = int(height)
        self.cam = np.ascontiguousarray(cam, 'f4').reshape(4); self.h = C.c_void_p(); self.host = 'EMULATOR' in self.lib.version()
        cap = int(max_crop_points or full_image_crop_points(self.width, self.height))
        self.lib.check(self.lib.dll.sgx_obj3d_create(self.width, self.height, int(max_images), int(max_jobs), cap, C.byref(self.params), C.byref(self.h)), 'sgx_obj3d_create')
        self.n_jobs = 0

    def _dev(self, a):
        if self.host: return np.ascontiguousarray(a)
        import torch
        return torch.from_numpy(np.ascontiguousarray(a)).cuda().contiguous()

    def _stream(self):
        if self.host: return None
        import torch
        return C.c_void_p(torch.cuda.current_stream().cuda_stream)

    def launch(self, depths, Twcs, jobs):
        """depths: n x height x width float (numpy, or a device tensor already), Twcs: n x 4 x 4 double, jobs: [(image index, Object2D), ...]; the records stay in
        self.results (device) until read()"""
        d = depths if hasattr(depths, 'data_ptr') else self._dev(np.asarray(depths, 'f4'))
        n = int(d.shape[0]); assert tuple(d.shape[1:]) == (self.height, self.width)
        T = Twcs if hasattr(Twcs, 'data_ptr') else self._dev(np.asarray(Twcs, 'f8').reshape(n, 16))
        arr = (Obj3dJob * max(len(jobs), 1))()
        for i, (img, o) in enumerate(jobs):
            cid, prob, (x, y, w, h) = _object2d(o)
            arr[i] = Obj3dJob(int(img), cid, prob, x, y, w, h)
        self.n_jobs = len(jobs)
        self.results = self._dev(np.zeros(max(self.n_jobs, 1) * OBJ3D_RESULT_DTYPE.itemsize, 'u1'))
        self._inputs = (d, T)                                      # alive until the launch sequence has read them
        self.lib.check(self.lib.dll.sgx_obj3d_detect_batch_dev(self.h, _vp(d), self.width, n, _vp(self.cam), _vp(T), arr, self.n_jobs, _vp(self.results), self._stream()),
                       'sgx_obj3d_detect_batch_dev')

    def read(self):
        r = self.results if self.host else self.results.cpu().numpy()
        return r.view(OBJ3D_RESULT_DTYPE)[:self.n_jobs].copy()

    def detect(self, depths, Twcs, jobs):
        self.launch(depths, Twcs, jobs)
        return self.read()

    def debug_read(self, job):
        n = C.c_int(0); cap = self.width * self.height
        kept = np.zeros(cap, 'u1'); lab = np.zeros(cap, 'i4')
        self.lib.check(self.lib.tap('sgx_obj3d_debug_read')(self.h, int(job), _vp(kept), _vp(lab), cap, C.byref(n)), 'sgx_obj3d_debug_read')
        return kept[:n.value].astype(bool), lab[:n.value].copy()

    def close(self):
        if self.h: self.lib.dll.sgx_obj3d_destroy(self.h); self.h = C.c_void_p()

    def __del__(self):
        try: self.close()
        except Exception: pass
