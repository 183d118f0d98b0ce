"""The global map (sgx_globalmap_*) on the MI355X: the product library against the restatement (tests/globalmap_ref.py) on every case of
tests/globalmap_cases.py bit for bit, the taps on the tap build, two runs of one sequence, the chain depth image -> world cloud -> global map on a side stream, the
C++ mirror class, three full-size TUM3 keyframes against the emulator, and lattice_big: the one test that crosses 2^20 voxel points."""
import math
import os
import subprocess
import numpy as np
import pytest
import cloud_cases as cc
import cloud_ref
import obj3d_ref
import globalmap_cases as gc
import globalmap_ref as ref
from sg_slam_amd.capi import CLOUD_POINT_DTYPE
from sg_slam_amd.globalmap import GlobalMap
from sg_slam_amd.pointcloudmapping import PointCloudMappingBatch

pytestmark = pytest.mark.gpu
f32 = np.float32


@pytest.mark.parametrize('name', [n for n in gc.NAMES if n != 'specks_whole'])
def test_device_equals_restatement(gpulib, name):
    recs, _ = gc.run_case(gpulib, gc.CASE[name])
    gc.check_case_figures(name, recs, None)


@pytest.mark.parametrize('name', gc.NAMES)
def test_device_taps(gpulib_taps, name):
    """the voxel cloud before the filter, the distances, the kept flags and the tiers; specks_whole forces the whole-cloud path through debug_max_radius"""
    recs, tap = gc.run_case(gpulib_taps, gc.CASE[name])
    gc.check_case_figures(name, recs, tap)


def _sequence(lib):
    c = gc.CASE['two_views']; M = GlobalMap(c['params'], c['cap'], lib=lib); out = []
    for op in c['ops']:
        if op[0] == 'append':
            p = np.zeros(len(op[1]), CLOUD_POINT_DTYPE); p['x'], p['y'], p['z'] = op[1][:, 0], op[1][:, 1], op[1][:, 2]; p['rgba'] = op[2]
            out.append(M.append(p).tobytes())
        else:
            out.append(M.consolidate().tobytes()); out += [t.tobytes() for t in M.debug_read()]
        out.append(M.points().tobytes())
    M.close()
    return out


def test_two_runs_of_a_sequence_are_identical(gpulib_taps):
    """records, maps and taps (the window counts and tiers included): no result depends on the order in which the atomics of a run arrive"""
    assert _sequence(gpulib_taps) == _sequence(gpulib_taps)


def test_cloud_handle_chain_on_a_side_stream(gpulib, emu):
    """depth image -> world cloud -> global map -> consolidation, one launch sequence on a non-default stream with nothing read back; the caller synchronises that
    stream before the synchronous reads.  Against the same chain on the emulator"""
    import torch
    W, H = 64, 48; cam = cc.cam_for(W, H)
    gp = dict(mean_k=8, stddev_mul=1.5, leaf=0.04, consider_dynamic=1, depth_min=0.5, depth_max=5.0)
    depths = np.stack([cc.scene(50 + i, W, H, wall=(1.4 + 0.05 * i, 0.004, 0.002), outliers=3) for i in range(4)]); cols = np.stack([cc.colors(60 + i, W, H) for i in range(4)])
    Twcs = np.stack([cc.pose((0.02 * i, -0.05 * i, 0.01), (0.1 * i, -0.05, 0.02 * i)) for i in range(4)])
    got = {}
    for lib in (emu, gpulib):
        B = PointCloudMappingBatch(gp, W, H, cam, 4, cloud_ref.WORLD, max_boxes=4, lib=lib); G = GlobalMap(gp, 1 << 14, lib=lib)
        if lib is gpulib:
            s = torch.cuda.Stream()
            with torch.cuda.stream(s):
                B.launch(depths, cols, Twcs); r = G.append_batch_dev(B); G.launch()
            s.synchronize()
        else:
            B.launch(depths, cols, Twcs); r = G.append_batch_dev(B); G.launch()
        got[lib is gpulib] = (G.read_records(r).tobytes(), G.read().tobytes(), G.points().tobytes(), G.size())
        B.close(); G.close()
    assert got[True] == got[False] and got[True][3] > 300


def test_cpp_mirror_class(gpulib, tmp_path):
    """sgx::GlobalMap (sg_slam_amd/host/sgx_host.hpp) through example_globalmap.cpp: the literal loop's schedule and the restatement's bits"""
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__))); host = os.path.join(root, 'sg_slam_amd', 'host')
    exe = str(tmp_path / 'example_globalmap')
    subprocess.check_call(['g++', '-O1', '-std=c++17', '-Wall', os.path.join(host, 'example_globalmap.cpp'), '-o', exe, '-L' + os.path.join(root, 'sg_slam_amd'), '-lsgx',
                           '-Wl,-rpath,' + os.path.join(root, 'sg_slam_amd')])
    clouds = [gc.wall(70 + i, 40, 30, y0=-1.0 + 0.3 * i) for i in range(5)]; pending = [True, True, True, True, False]; args = []
    for i, (xyz, rgba) in enumerate(clouds):
        p = np.zeros(len(xyz), CLOUD_POINT_DTYPE); p['x'], p['y'], p['z'] = xyz[:, 0], xyz[:, 1], xyz[:, 2]; p['rgba'] = rgba
        p.tofile(tmp_path / ('c%d.bin' % i)); args += [str(tmp_path / ('c%d.bin' % i)), str(int(pending[i]))]
    out = subprocess.check_output([exe, '0.05', '8', '1.0', '1', '8192'] + args, text=True).splitlines()
    M = ref.GlobalMap(gc.PARAMS, 8192); want, counts = ref.schedule(M, clouds, pending, 1)
    kf = [ln.split() for ln in out if ln.startswith('keyframe')]
    assert [int(k[-1]) for k in kf] == counts == [1, 2, 1, 2, 1] and [int(k[-3]) for k in kf] == [int(w is not None) for w in want] == [0, 0, 1, 0, 1]
    at = out.index([ln for ln in out if ln.startswith('map ')][0]); rows = np.array([[float(v) for v in ln.split()] for ln in out[at + 1:]])
    assert int(out[at].split()[1]) == len(M.xyz) == len(rows) > 200
    assert (cc.bits(rows[:, :3].astype('f4')) == cc.bits(M.xyz)).all() and (rows[:, 3].astype(np.uint32) == M.rgba).all()


def test_full_size_keyframes_equal_emulator(gpulib, emu):
    """three 640 x 480 TUM3 keyframes (mean_k 50, leaf 1 cm) in WORLD mode appended and consolidated, against the emulator"""
    F = cc.tum3_full(); got = {}
    for lib in (emu, gpulib):
        B = PointCloudMappingBatch(F['params'], F['W'], F['H'], F['cam'], 3, cloud_ref.WORLD, max_boxes=4, lib=lib); G = GlobalMap(F['params'], 1 << 18, lib=lib)
        B.launch(F['depths'], F['colors'], F['Twcs'], F['boxes'], F['have_dynamic'])
        a = G.read_records(G.append_batch_dev(B)); G.launch(); r = G.read()
        got[lib is gpulib] = (a.tobytes(), r.tobytes(), G.points().tobytes()); B.close(); G.close()
        assert (a['flags'] == 0).all() and r['flags'] == 0 and 60000 < r['n_points_in'] < 1 << 18 and 0.5 * r['n_voxels'] < r['n_points'] < r['n_voxels']
    assert got[True] == got[False]


def test_lattice_big(gpulib_taps):
    """130 x 130 x 64 = 1 081 600 points, one per voxel at (i + 1/2) * 2^-6, leaf 2^-6, mean_k 8, stddev_mul 1: more than 2^20 voxel points.  Every coordinate and every
    d2 is exact, so a point's nine nearest neighbours depend only on how close it is to each face, clipped at 3 cells (the K-th neighbour is at most 2 cells away):
    the expected dist of every point is a look-up into the restatement's answer on the 8 x 8 x 8 lattice.  The statistics are taken in double over the expected
    distances; both sums are exact in double, so their order is free (asserted), and the nearest distance is about 1.4 % from the threshold (asserted > 1 %)."""
    L = 2.0 ** -6; dims = (130, 130, 64); K8 = 8
    P8, _ = gc.lattice(K8, K8, K8, L)
    V8 = cloud_ref.voxel_grid(P8, np.full(len(P8), 0xff000000, np.uint32), f32(L))
    assert (cc.bits(V8['xyz']) == cc.bits(P8[np.lexsort((P8[:, 0], P8[:, 1], P8[:, 2]))])).all()                 # the voxel step is the identity (in idx order: x fastest)
    d8, _, _, _ = obj3d_ref.sor(P8, 8, 1.0)
    d8 = d8.reshape(K8, K8, K8)                                       # lattice() orders i, j, k with k fastest
    cls = lambda n: np.minimum(np.minimum(np.arange(n), n - 1 - np.arange(n)), 3)
    fold = lambda n: np.where(np.arange(n) < n - 1 - np.arange(n), cls(n), K8 - 1 - cls(n))      # the 8-lattice position with the same distance to the faces, clipped at 3
    ix, iy, iz = (fold(n) for n in dims)
    want = d8[ix[:, None, None], iy[None, :, None], iz[None, None, :]]                           # [i][j][k]
    want_idx = np.ascontiguousarray(want.transpose(2, 1, 0)).reshape(-1)                         # voxel order: idx = i + j * 130 + k * 130 * 130
    assert sorted(round(float(v), 6) for v in np.unique(want)) == [0.017243, 0.018052, 0.018861, 0.021435]
    n = want_idx.size; w8 = want_idx.astype('f8'); sq = (want_idx * want_idx).astype(f32).astype('f8')
    s, q = float(np.add.accumulate(w8)[-1]), float(np.add.accumulate(sq)[-1])
    assert s == math.fsum(w8) and q == math.fsum(sq) and cc.exact_any_order(want_idx) and cc.exact_any_order(sq.astype(f32))      # both sums are exact in double
    mean = s / n; thr = mean + 1.0 * np.sqrt((q - s * s / n) / (n - 1))
    assert abs(thr - 0.0174926) < 1e-7 and np.abs(w8 - thr).min() > 0.01 * thr
    keep = ~(w8 > thr); assert int(keep.sum()) == 128 * 128 * 62
    i, j, k = np.meshgrid(np.arange(dims[0]), np.arange(dims[1]), np.arange(dims[2]), indexing='ij')
    pts = np.zeros(n, CLOUD_POINT_DTYPE)                              # appended in i, j, k order with k fastest: NOT the voxel order, the sort has work to do
    pts['x'] = ((i.reshape(-1) + 0.5) * L).astype(f32); pts['y'] = ((j.reshape(-1) + 0.5) * L).astype(f32); pts['z'] = ((k.reshape(-1) + 0.5) * L).astype(f32)
    pts['rgba'] = (0xff000000 + (np.arange(n) % 0xffffff)).astype(np.uint32)
    M = GlobalMap(dict(mean_k=8, stddev_mul=1.0, leaf=L), 1 << 21, lib=gpulib_taps)
    assert n > 1 << 20 and int(M.append(pts)['map_size']) == n
    r = M.consolidate()
    assert (int(r['n_points_in']), int(r['n_voxels']), int(r['n_points']), int(r['flags'])) == (n, n, 128 * 128 * 62, 0)
    assert float(r['mean']) == mean and float(r['thr']) == thr
    assert r['wider_window_points'] == 8 and r['whole_cloud_points'] == 0                        # the eight corners: their ninth neighbour is two cells away
    vox, dist, kept, tier = M.debug_read()
    order = np.lexsort((pts['x'], pts['y'], pts['z']))                                           # voxel order
    assert vox.tobytes() == pts[order].tobytes()                                                 # the voxel step is the identity, colours included
    assert (cc.bits(dist) == cc.bits(want_idx)).all() and (kept == keep).all() and set(tier.tolist()) == {2, 4}
    assert M.points().tobytes() == pts[order][keep].tobytes()
    M.close()
