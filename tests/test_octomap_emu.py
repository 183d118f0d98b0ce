"""CPU: the occupancy map (sgx_octomap_*).  The restatement (tests/octomap_ref.py) against independent statements: rays are 6-connected paths whose cells the segment
meets, a dense dictionary of cells equals the tree's expanded leaves after every scan (the equivalence the device design rests on), the grid from pruned leaves equals
the grid from cells.  Then the kernel-logic emulator against the restatement bit for bit on every case, a batch against single calls, the argument errors, the chain
cloud -> map without a host copy, sensor_to_world, and the Python class."""
import ctypes as C
import numpy as np
import pytest
import octomap_cases as oc
import octomap_ref as ref
from sg_slam_amd.capi import OctomapParams, OctomapGridHeader, OCTOMAP_RECORD_DTYPE, OCTOMAP_BOUNDS_DTYPE, CLOUD_POINT_DTYPE, CLOUD_RESULT_DTYPE, _vp
from sg_slam_amd.octomapserver import OctomapServer, make_octomap_params, sensor_to_world

MARGIN = 1e-4        # of res: how far outside a cell the float64 segment may pass and still count as meeting it


def test_cases_contain_what_they_are_for():
    oc.check_case_contents()


def _segment_meets_box(o, e, lo, hi):
    t0, t1 = 0.0, 1.0
    for a in range(3):
        d = e[a] - o[a]
        if d == 0.0:
            if o[a] < lo[a] or o[a] > hi[a]: return False
            continue
        ta, tb = (lo[a] - o[a]) / d, (hi[a] - o[a]) / d
        t0, t1 = max(t0, min(ta, tb)), min(t1, max(ta, tb))
    return t0 <= t1


@pytest.mark.parametrize('name', [n for n in oc.NAMES if n not in ('empty', 'clamps')])
def test_rays_are_connected_paths_along_the_segment(name):
    c = oc.CASE[name]; p = c['params']; res = p['res']; n = 0
    for pts, m in c['scans']:
        o = [float(m[i, 3]) for i in range(3)]
        for q in ref.transform_and_filter(p, pts, m):
            ok, keys, info = ref.compute_ray_keys(res, [m[0, 3], m[1, 3], m[2, 3]], q)
            if not ok or not keys: continue
            e = [float(v) for v in q]; ke = ref.key3(res, q)[1]
            assert keys[0] == ref.key3(res, o)[1] and ke not in keys and len(set(keys)) == len(keys)
            for a, b in zip(keys, keys[1:]): assert sum(abs(a[i] - b[i]) for i in range(3)) == 1
            if name not in oc.BOUNDARY:                   # the condition on the inputs that gives the margin its meaning: no tested cell's corner within it of the segment
                cs = np.unique(np.array([[k[0] + a, k[1] + b, k[2] + c] for k in keys for a in (0, 1) for b in (0, 1) for c in (0, 1)]), axis=0)
                P = (cs - 32768.0) * res; O = np.array(o); D = np.array(e) - O
                tt = np.clip((P - O) @ D / (D @ D), 0.0, 1.0)
                assert np.linalg.norm(P - (O + tt[:, None] * D), axis=1).min() > MARGIN * res, name
            for k in keys:
                lo = [ref.coord(res, k[i]) - res / 2 - MARGIN * res for i in range(3)]; hi = [ref.coord(res, k[i]) + res / 2 + MARGIN * res for i in range(3)]
                assert _segment_meets_box(o, e, lo, hi), (name, k)
            n += 1
    assert n > 0 or name in ('same_cell',)


@pytest.mark.parametrize('name', oc.NAMES)
def test_dictionary_of_cells_equals_the_tree(name):
    """cells only, no tree, no early return, free-minus-occupied then occupied: the same log-odds bits in the same order after every scan; the tree stays maximally
    pruned; the grid from pruned leaves is the grid from cells"""
    c = oc.CASE[name]; e = oc.expected(name); D = ref.DictMap(c['params']); R = ref.Octomap(c['params'], c['max_bricks'], c['max_points'])
    for (pts, m), step in zip(c['scans'], e['steps']):
        rec = R.insert(pts, m)
        if not rec['flags'] & (ref.MAP_FULL | ref.TOO_MANY_POINTS): D.apply(*R.last_sets)
        got = D.expanded(); want = step['expanded']
        assert [k for k, _ in got] == [k for k, _ in want] and [oc.bits(v) for _, v in got] == [oc.bits(v) for _, v in want]
        assert np.array_equal(step['grid'], step['grid_leaves'])
        if R.tree.root is not None: assert all(R.tree._prune_recurs(R.tree.root, 0, d) == 0 for d in range(15, 0, -1))       # nothing left to prune


def test_pruned_nodes_occur_and_expand():
    """a block of 2 x 2 x 2 equal cells collapses; an update inside it expands it again with the block's value"""
    p = ref.params(res=0.1); T = ref.OcTree(p)
    ks = [(40000 + x, 40000 + y, 40000 + z) for x in (0, 1) for y in (0, 1) for z in (0, 1)]
    for k in ks: T.update_node(k, True)
    assert [d for _, d, _ in T.leaves()] == [15] and len(T.expanded()) == 8
    T.update_node(ks[3], False)
    assert sorted(d for _, d, _ in T.leaves()) == [16] * 8 and T.search(ks[3]).value == np.float32(T.hit + T.miss) and T.search(ks[0]).value == T.hit


@pytest.mark.parametrize('name', oc.NAMES)
def test_emulator_equals_restatement(emu, name):
    oc.run_case(emu, oc.CASE[name])


def test_batch_equals_singles(emu):
    for name in ('generated_walk', 'map_full', 'table_full', 'too_many_points', 'out_of_key_range', 'clamps'):
        c = oc.CASE[name]; e = oc.expected(name)
        recs, S = oc.run_batch(emu, c)
        for i, st in enumerate(e['steps']): oc.assert_record(recs[i], st['record'], (name, i))
        oc.assert_state(S, e['steps'][-1], name)
        S.reset(); b = S.bounds(); assert b['n_known'] == 0 and b['n_bricks'] == 0
        recs2, _ = oc.run_batch(emu, c, S)
        assert recs2.tobytes() == recs.tobytes(); oc.assert_state(S, e['steps'][-1], name); S.close()


def test_argument_errors(emu):
    d = emu.dll; h = C.c_void_p()
    def create(**kw): return d.sgx_octomap_create(C.byref(make_octomap_params(**kw)), 16, 16, C.byref(h))
    for bad in (dict(res=0.0), dict(res=-1.0), dict(res=float('nan')), dict(res=float('inf')), dict(prob_hit=1.0), dict(prob_miss=0.0), dict(thres_min=0.0), dict(thres_max=1.0),
                dict(thres_min=0.5, thres_max=0.5), dict(thres_min=0.9, thres_max=0.2), dict(max_range=float('nan')), dict(pointcloud_min_x=float('nan')),
                dict(occupancy_max_z=float('nan')), dict(min_size_y=float('nan'))):
        assert create(**bad) == -1 and not h.value, bad
    P = make_octomap_params()
    assert d.sgx_octomap_create(C.byref(P), 0, 16, C.byref(h)) == -1 and d.sgx_octomap_create(C.byref(P), 16, 0, C.byref(h)) == -1 and d.sgx_octomap_create(None, 16, 16, C.byref(h)) == -1
    assert d.sgx_octomap_create(C.byref(P), 16, 16, None) == -1
    assert create() == 0 and h.value
    pts = np.zeros(4, CLOUD_POINT_DTYPE); m = np.eye(4, dtype='f4'); rec = np.zeros(1, OCTOMAP_RECORD_DTYPE); n = np.zeros(1, 'i4'); b = np.zeros(1, OCTOMAP_BOUNDS_DTYPE)
    assert d.sgx_octomap_insert(h, None, 4, _vp(m), _vp(rec)) == -1 and d.sgx_octomap_insert(h, _vp(pts), -1, _vp(m), _vp(rec)) == -1
    bad = m.copy(); bad[1, 2] = np.nan
    assert d.sgx_octomap_insert(h, _vp(pts), 4, _vp(bad), _vp(rec)) == -1 and d.sgx_octomap_insert(h, _vp(pts), 4, None, _vp(rec)) == -1
    assert d.sgx_octomap_insert_batch_dev(h, _vp(pts), 4, _vp(n), 4, _vp(m), 0, _vp(rec), None) == -1 and d.sgx_octomap_insert_batch_dev(h, _vp(pts), 4, _vp(n), 2, _vp(m), 1, _vp(rec), None) == -1
    assert d.sgx_octomap_insert_batch_dev(h, None, 4, _vp(n), 4, _vp(m), 1, _vp(rec), None) == -1
    assert d.sgx_octomap_bounds(h, None) == -1 and d.sgx_octomap_bounds(None, _vp(b)) == -1
    assert d.sgx_octomap_cells(h, 1, None, 4, _vp(n)) == -1 and d.sgx_octomap_cells(h, 1, None, 0, None) == -1
    out = np.zeros(4, 'f4'); keys = np.zeros((4, 3), 'u2')
    assert d.sgx_octomap_search_dev(h, _vp(keys), _vp(out), 4, _vp(out), None) == -1 and d.sgx_octomap_search_dev(h, None, None, 4, _vp(out), None) == -1
    hd = OctomapGridHeader()
    assert d.sgx_octomap_grid_header(h, None, C.byref(hd)) == -1 and d.sgx_octomap_project(h, None, None, 0) == -1 and d.sgx_octomap_reset(None) == -1
    q = np.array([0, 0, 0, 0], 'f8'); o = np.zeros(3); o16 = np.zeros(16, 'f4')
    assert d.sgx_octomap_sensor_to_world(_vp(o), _vp(q), _vp(o16)) == -1 and d.sgx_octomap_sensor_to_world(None, _vp(q), _vp(o16)) == -1
    assert d.sgx_octomap_insert(h, _vp(pts), 4, _vp(m), _vp(rec)) == 0 and rec[0]['n_in'] == 4          # the handle still works
    d.sgx_octomap_destroy(h)


def test_cells_overflow_reports_the_count(emu):
    c = oc.CASE['brick_borders']; e = oc.expected(c['name']); S = OctomapServer(c['params'], lib=emu)
    S.insert(*c['scans'][0]); want = e['steps'][0]['free']
    from sg_slam_amd.capi import OCTOMAP_CELL_DTYPE
    out = np.zeros(10, OCTOMAP_CELL_DTYPE); n = C.c_int32(0)
    assert emu.dll.sgx_octomap_cells(S.h, 0, _vp(out), 10, C.byref(n)) == -5 and n.value == len(want) > 10
    assert np.array_equal(out['key'], np.array([k for k, _, _ in want[:10]], 'u2'))
    hd = OctomapGridHeader(); g = np.zeros(4, 'i1')
    assert emu.dll.sgx_octomap_project(S.h, C.byref(hd), _vp(g), 4) == -5 and hd.width * hd.height > 4
    S.close()


def test_sensor_to_world(emu):
    rng = np.random.default_rng(5)
    for _ in range(20):
        q = rng.normal(size=4); o = rng.normal(size=3) * 3; qn = q / np.linalg.norm(q); x, y, z, w = qn
        Rm = np.array([[1 - 2 * (y * y + z * z), 2 * (x * y - z * w), 2 * (x * z + y * w)], [2 * (x * y + z * w), 1 - 2 * (x * x + z * z), 2 * (y * z - x * w)],
                       [2 * (x * z - y * w), 2 * (y * z + x * w), 1 - 2 * (x * x + y * y)]])
        m = sensor_to_world(o, q, lib=emu)
        assert np.abs(m[:3, :3] - Rm).max() <= 1e-7 and np.array_equal(m[:3, 3], o.astype('f4')) and list(m[3]) == [0, 0, 0, 1]
        assert np.array_equal(oc.bits(m), oc.bits(ref.sensor_to_world(o, q)))


def test_chain_cloud_to_map_without_a_host_copy(emu):
    """cloud_ref -> octomap_ref against sgx_cloud_build_batch_dev -> sgx_octomap_insert_batch_dev reading the cloud handle's own output and result records"""
    import cloud_cases as cc
    import cloud_ref
    from sg_slam_amd.pointcloudmapping import PointCloudMappingBatch, camera_to_map_tf
    cs = cc.batch_group()[:2]
    B = PointCloudMappingBatch(cs[0]['params'], cs[0]['W'], cs[0]['H'], cs[0]['cam'], len(cs), cs[0]['mode'], max_boxes=4, lib=emu)
    cc.run_batch(emu, cs, B)
    p = ref.params(res=0.1, max_range=4.0, occupancy_min_z=-1.0, occupancy_max_z=2.0)
    mats = []
    for i in range(len(cs)):
        Tcw = np.linalg.inv(cc.pose((0.1 * i, 0.05, -0.1 * i), (0.05 * i, -0.1 * i, 0.02))).astype('f4'); o, q = camera_to_map_tf(Tcw, lib=emu)
        mats.append(sensor_to_world(o, q, lib=emu))
    S = OctomapServer(p, max_bricks=4096, max_points_per_scan=B.N, lib=emu)
    recs = S.insert_clouds(B, np.array(mats))
    R = ref.Octomap(p, 4096, B.N)
    for i, c in enumerate(cs):
        e = cc.expected(c); pts = np.asarray(e['points'], 'f4').reshape(-1, 3)
        assert len(pts) > 50
        oc.assert_record(recs[i], R.insert(pts, mats[i]), i)
    cells = R.tree.expanded(); b = R.bounds(cells); h = R.header(b)
    oc.assert_state(S, dict(bounds=b, occupied=R.cells(True, cells), free=R.cells(False, cells), header=h, grid=R.grid_from_cells(h, cells)), 'chain')
    S.close(); B.close()


def test_python_class(emu):
    S = OctomapServer({'resolution': 0.1, 'sensor_model/max_range': 2.0}, occupancy_min_z=-1.0, lib=emu)
    assert S.params.res == 0.1 and S.params.max_range == 2.0 and S.params.prob_hit == 0.7 and S.params.occupancy_min_z == -1.0
    rec = S.insertCloud(np.array([[1.0, 0.0, 0.0], [0.0, 5.0, 0.0]], 'f4'), (0.05, 0.05, 0.05), (0, 0, 0, 1))
    assert rec['n_passed'] == 2 and rec['n_truncated'] == 1 and rec['n_occupied_updates'] == 1
    occ = S.cells(True); assert len(occ) == 1 and list(occ[0]['key']) == [32778, 32768, 32768] and occ[0]['logodds'] == ref.logodds(0.7)
    assert np.isnan(S.search(points=[[9, 9, 9]])[0]) and S.search(keys=[[32770, 32768, 32768]])[0] == ref.logodds(0.4)
    hd, g = S.project(); assert g.shape == (hd.height, hd.width) and (g == 100).sum() == 1 and (g == 0).sum() > 20
    S.reset(); assert S.bounds()['n_known'] == 0 and S.project()[0].flags == 1
    with pytest.raises(KeyError): make_octomap_params(nonsense=1)
    S.close()
