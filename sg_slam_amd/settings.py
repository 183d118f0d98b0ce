"""Reader of the reference's OpenCV-FileStorage settings files (src/sg-slam/Examples/*.yaml, read by Tracking::Tracking, src/sg-slam/src/Tracking.cc:56-150).

A line parser for the flat `Key: value` entries those files hold (no PyYAML): the camera (Camera.fx..cy, bf, RGB), the distortion vector mDistCoef
(k1, k2, p1, p2, plus k3 only when it is nonzero: Tracking.cc:66-77), ThDepth, DepthMapFactor and the ORBextractor.* parameters.  Values are read as
doubles and stored as float32 where the reference keeps them in a float (`float fx = fSettings["Camera.fx"]`)."""
import numpy as np


def parse(path):
    """{key: str value} of every `Key: value` line (comments and the %YAML header skipped)"""
    out = {}
    with open(path) as f:
        for line in f:
            line = line.split('#', 1)[0].strip()
            if not line or line.startswith('%') or ':' not in line:
                continue
            k, v = line.split(':', 1)
            v = v.strip()
            if v:
                out[k.strip()] = v
    return out


def _f32(kv, key, default=0.0):
    return float(np.float32(float(kv.get(key, default))))


def load(path):
    """dict(cam, dist, rgb, orb, width, height): `cam` is the CAM dict the package uses (fx, fy, cx, cy, bf, depth_factor, th_depth), `dist` the float32
    mDistCoef (4 or 5 entries), `orb` the ORBextractor parameters (nfeatures, scale_factor, nlevels, ini_th_fast, min_th_fast)."""
    kv = parse(path)
    cam = dict(fx=_f32(kv, 'Camera.fx'), fy=_f32(kv, 'Camera.fy'), cx=_f32(kv, 'Camera.cx'), cy=_f32(kv, 'Camera.cy'), bf=_f32(kv, 'Camera.bf'),
               depth_factor=_f32(kv, 'DepthMapFactor', 1.0), th_depth=_f32(kv, 'ThDepth'))
    dist = [_f32(kv, 'Camera.' + k) for k in ('k1', 'k2', 'p1', 'p2')]
    k3 = _f32(kv, 'Camera.k3')
    if k3 != 0:
        dist.append(k3)
    orb = dict(nfeatures=int(kv.get('ORBextractor.nFeatures', 1000)), scale_factor=_f32(kv, 'ORBextractor.scaleFactor', 1.2),
               nlevels=int(kv.get('ORBextractor.nLevels', 8)), ini_th_fast=int(kv.get('ORBextractor.iniThFAST', 20)), min_th_fast=int(kv.get('ORBextractor.minThFAST', 7)))
    return dict(cam=cam, dist=np.array(dist, 'f4'), rgb=int(float(kv.get('Camera.RGB', 1))), orb=orb,
                width=int(float(kv.get('Camera.width', 640))), height=int(float(kv.get('Camera.height', 480))))


def load_mapping(path):
    """The semantic-mapping parameters System::System reads (System.cc:92 ff.): Detector3D.* as the Detector3D constructor takes them (Sor_MeanK,
    Sor_StddevMulThresh (double), Voxel_LeafSize, EuclideanClusterTolerance, EuclideanClusterMinSize, EuclideanClusterMaxSize, DetectSimilarCompareRatio) and
    PointCloudMapping.camera_valid_depth_Min / Max.  A missing key raises KeyError: the reference has no defaults for them."""
    kv = parse(path)
    d = lambda k: float(kv['Detector3D.' + k])
    return dict(Sor_MeanK=int(d('Sor_MeanK')), Sor_StddevMulThresh=d('Sor_StddevMulThresh'), Voxel_LeafSize=_f32(kv, 'Detector3D.Voxel_LeafSize'),
                EuclideanClusterTolerance=float(np.float32(d('EuclideanClusterTolerance'))), EuclideanClusterMinSize=int(d('EuclideanClusterMinSize')),
                EuclideanClusterMaxSize=int(d('EuclideanClusterMaxSize')), DetectSimilarCompareRatio=float(np.float32(d('DetectSimilarCompareRatio'))),
                camera_valid_depth_Min=float(np.float32(float(kv['PointCloudMapping.camera_valid_depth_Min']))),
                camera_valid_depth_Max=float(np.float32(float(kv['PointCloudMapping.camera_valid_depth_Max']))))


def load_pointcloud_mapping(path):
    """The PointCloudMapping.* parameters System::System reads for the map cloud (src/sg-slam/src/PointcloudMapping.cc): the three switches
    (is_map_construction_consider_dynamic, is_octo_semantic_map_construction, is_global_pc_reconstruction), the valid depth range, and mean_k, stddev_mul (double) and
    the voxel leaf (float) of the local and of the global filter.  A missing key raises KeyError: the reference has no defaults for them."""
    kv = parse(path)
    d = lambda k: float(kv['PointCloudMapping.' + k])
    out = {k: int(d(k)) for k in ('is_map_construction_consider_dynamic', 'is_octo_semantic_map_construction', 'is_global_pc_reconstruction')}
    for k in ('camera_valid_depth_Min', 'camera_valid_depth_Max'):
        out[k] = float(np.float32(d(k)))
    for w in ('Local', 'Global'):
        out['Sor_%s_MeanK' % w] = int(d('Sor_%s_MeanK' % w)); out['Sor_%s_StddevMulThresh' % w] = d('Sor_%s_StddevMulThresh' % w)
        out['Voxel_%s_LeafSize' % w] = float(np.float32(d('Voxel_%s_LeafSize' % w)))
    return out


def load_global_map(path):
    """The parameters of MapViewer's global cloud (src/sg-slam/src/PointcloudMapping.cc:332-360): Voxel_Global_LeafSize (float), Sor_Global_MeanK,
    Sor_Global_StddevMulThresh (double) of PointCloudMapping.*, and global_pc_update_kf_threshold, which the reference reads as
    Detector3D.global_pc_update_kf_threshold (System.cc:114).  A missing key raises KeyError: the reference has no defaults for them."""
    kv = parse(path)
    d = lambda k: float(kv['PointCloudMapping.' + k])
    return dict(Voxel_Global_LeafSize=float(np.float32(d('Voxel_Global_LeafSize'))), Sor_Global_MeanK=int(d('Sor_Global_MeanK')),
                Sor_Global_StddevMulThresh=d('Sor_Global_StddevMulThresh'), global_pc_update_kf_threshold=int(float(kv['Detector3D.global_pc_update_kf_threshold'])))
