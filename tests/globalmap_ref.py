"""Restatement of MapViewer's accumulating global cloud (src/sg-slam/src/PointcloudMapping.cc:332-360) in numpy, brute force: the yardstick of
sg_slam_amd/csrc/sgx_globalmap_kernels.h and of the emulator.  `*globalMap += *temp_globalMap` is a concatenation; voxel_global + sor_global over the whole map are
tests/cloud_ref.voxel_grid and tests/obj3d_ref.sor (PCL restated, UNPINNED: DESIGN.md §2, §9f, §9j) with the defined cases of include/sgx.h: a consolidation that is
refused (LEAF_TOO_SMALL, or <= mean_k voxel points: FEW_POINTS) leaves the map as it was; a cloud that does not fit is refused whole (FULL).  schedule() is the literal
loop of :332-360."""
import numpy as np
import cloud_ref
import obj3d_ref

f32 = np.float32
FEW_POINTS, LEAF_TOO_SMALL, FULL = 1, 2, 4


def check_params(p, max_points):
    leaf = f32(p['leaf'])
    if int(p['mean_k']) < 1 or not (np.isfinite(leaf) and leaf > 0) or float(p['stddev_mul']) != float(p['stddev_mul']) or max_points < 1 or max_points > 1 << 22:
        raise ValueError('invalid parameters')


class GlobalMap:
    """xyz float[n][3] and rgba uint32[n] in ROS axes"""

    def __init__(self, p, max_points):
        check_params(p, max_points)
        self.p = dict(p); self.cap = int(max_points)
        self.xyz = np.zeros((0, 3), f32); self.rgba = np.zeros(0, np.uint32)

    def append(self, xyz, rgba):
        """dict(n_in, offset, map_size, flags): points that are not finite are stored (operator+=)"""
        xyz = np.asarray(xyz, f32).reshape(-1, 3); rgba = np.asarray(rgba, np.uint32).reshape(-1); n = len(xyz)
        if len(self.xyz) + n > self.cap:
            return dict(n_in=n, offset=-1, map_size=len(self.xyz), flags=FULL)
        off = len(self.xyz)
        self.xyz = np.concatenate([self.xyz, xyz]); self.rgba = np.concatenate([self.rgba, rgba])
        return dict(n_in=n, offset=off, map_size=len(self.xyz), flags=0)

    def consolidate(self):
        """the fields of sgx_globalmap_result (except the two window counts, which the implementation defines) and, for the taps, voxels / voxel_rgba / dist / terms /
        kept / members"""
        mean_k = int(self.p['mean_k']); n_in = len(self.xyz)
        V = cloud_ref.voxel_grid(self.xyz, self.rgba, f32(self.p['leaf']))
        nv = len(V['xyz'])
        out = dict(n_points_in=n_in, n_voxels=nv, n_points=n_in, flags=0, mean=0.0, thr=0.0, voxels=V['xyz'], voxel_rgba=V['rgba'], voxel_idx=V['idx'], members=V['members'],
                   grid=V['grid'], dist=np.zeros(nv, f32), kept=np.zeros(nv, bool), terms=None)
        if V['refused']:
            out['flags'] = LEAF_TOO_SMALL
            return out
        if nv <= mean_k:
            out['flags'] = FEW_POINTS
            return out
        dist, terms, thr, kept = obj3d_ref.sor(V['xyz'], mean_k, self.p['stddev_mul'])
        self.xyz = V['xyz'][kept]; self.rgba = V['rgba'][kept]
        out.update(dist=dist, terms=terms, thr=thr, mean=obj3d_ref.seq_sum(dist) / nv, kept=kept, n_points=int(kept.sum()))
        return out


def schedule(gmap, clouds, pending, threshold):
    """the literal loop of :332-360 over keyframes whose filtered temp_globalMap is clouds[i] = (xyz, rgba) and whose CheckNewKeyFrames() answer is pending[i]:
    [None or (published xyz, rgba)] per keyframe, and the counts after every keyframe"""
    count = 0; out = []; counts = []
    for (xyz, rgba), pend in zip(clouds, pending):
        gmap.append(xyz, rgba)                                       # *globalMap += *temp_globalMap
        pub = None
        if not pend or count > threshold:
            gmap.consolidate()                                       # voxel_global, sor_global
            pub = (gmap.xyz.copy(), gmap.rgba.copy())
            if len(gmap.xyz):                                        # globalMap_pcl_to_publish.data.size()
                count = 0
        count += 1
        out.append(pub); counts.append(count)
    return out, counts
