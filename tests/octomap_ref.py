"""Literal restatement of what sgx_octomap_* computes, in plain Python and numpy scalars: octomap's pointer octree (search, expandNode, pruneNode / isNodeCollapsible,
updateNode with its early return, updateNodeRecurs with the prune on the way up, prune, the leaf iterator), octomap_server's insertCloudCallback (non-ground branch) and
insertScan with two Python sets (src/octomap_server/src/OctomapServer.cpp:261-480), computeRayKeys, the cell lists, the projected 2-D grid built from the tree's leaves
at their own depths (update2DMap's square fill, :1078-1107) and its header (:934-990).  octomap is restated from its published algorithm, unpinned.
DictMap is the independent model the device design rests on: cells only, no tree, no early return."""
import math
import numpy as np

f32, f64 = np.float32, np.float64
DBL_MAX = float(np.finfo('f8').max)
ORIGIN_OUT_OF_RANGE, RAY_LEFT_KEYSPACE, MAP_FULL, TOO_MANY_POINTS = 1, 2, 4, 8
GRID_EMPTY, GRID_KEY_OUT_OF_RANGE = 1, 2
DEFAULTS = dict(res=0.05, prob_hit=0.7, prob_miss=0.4, thres_min=0.12, thres_max=0.97, max_range=-1.0, pointcloud_min_x=-DBL_MAX, pointcloud_max_x=DBL_MAX,
                pointcloud_min_y=-DBL_MAX, pointcloud_max_y=DBL_MAX, pointcloud_min_z=-DBL_MAX, pointcloud_max_z=DBL_MAX, occupancy_min_z=-DBL_MAX, occupancy_max_z=DBL_MAX,
                min_size_x=0.0, min_size_y=0.0)
RECORD_FIELDS = ('n_in', 'n_passed', 'n_truncated', 'n_bad_end_key', 'n_invalid_rays', 'n_free_updates', 'n_occupied_updates', 'n_new_cells', 'bbx_min', 'bbx_max', 'flags')


def params(**kw):
    p = dict(DEFAULTS); p.update(kw); return p


def logodds(p):
    return f32(math.log(p / (1.0 - p)))


def to_f32(v):
    """a double limit taken as float: +-DBL_MAX become +-inf"""
    with np.errstate(over='ignore'):
        return f32(v)


def key1(res, c):
    """coordToKeyChecked of one coordinate -> (valid, key)"""
    c = float(f32(c))
    if not math.isfinite(c): return False, 0
    s = math.floor((1.0 / res) * c)
    if not (-32768 <= s < 32768): return False, 0
    return True, int(s) + 32768


def key3(res, p):
    ks = [key1(res, c) for c in p]
    return all(k[0] for k in ks), tuple(k[1] for k in ks)


def coord(res, k):
    """keyToCoord at depth 16, a double"""
    return (float(k - 32768) + 0.5) * res


def coord_at(res, k, depth):
    """keyToCoord(key, depth) of octomap for an inner node"""
    if depth == 16: return coord(res, k)
    return (math.floor((float(k) - 32768.0) / float(1 << (16 - depth))) + 0.5) * (res * float(1 << (16 - depth)))


def morton(k):
    m = 0
    for i in range(16):
        m |= ((k[0] >> i) & 1) << (3 * i) | ((k[1] >> i) & 1) << (3 * i + 1) | ((k[2] >> i) & 1) << (3 * i + 2)
    return m


def brick(k):
    return (k[0] >> 3, k[1] >> 3, k[2] >> 3)


# ---- the tree -----------------------------------------------------------------------------------------------------------------------------------------------------
class Node:
    __slots__ = ('value', 'children')

    def __init__(self, value=f32(0.0)):
        self.value = value; self.children = None


def _child_idx(key, i):
    return ((key[0] >> i) & 1) | (((key[1] >> i) & 1) << 1) | (((key[2] >> i) & 1) << 2)


class OcTree:
    def __init__(self, p):
        self.res = p['res']; self.root = None
        self.hit, self.miss = logodds(p['prob_hit']), logodds(p['prob_miss'])
        self.clamp_min, self.clamp_max = logodds(p['thres_min']), logodds(p['thres_max'])

    def clear(self):
        self.root = None

    @staticmethod
    def has_children(n):
        return n.children is not None and any(c is not None for c in n.children)

    def search(self, key):
        if self.root is None: return None
        cur = self.root
        for i in range(15, -1, -1):
            pos = _child_idx(key, i)
            if cur.children is not None and cur.children[pos] is not None: cur = cur.children[pos]
            elif not self.has_children(cur): return cur            # a pruned node stands for all its cells
            else: return None
        return cur

    def expand_node(self, n):
        n.children = [Node(n.value) for _ in range(8)]

    def is_collapsible(self, n):
        if n.children is None or any(c is None for c in n.children): return False
        first = n.children[0]
        if self.has_children(first): return False
        for c in n.children[1:]:
            if self.has_children(c) or not (c.value == first.value): return False
        return True

    def prune_node(self, n):
        if not self.is_collapsible(n): return False
        n.value = n.children[0].value; n.children = None
        return True

    def update_node(self, key, occupied):
        upd = self.hit if occupied else self.miss
        leaf = self.search(key)
        if leaf is not None and ((upd >= 0 and leaf.value >= self.clamp_max) or (upd <= 0 and leaf.value <= self.clamp_min)): return leaf
        created = False
        if self.root is None: self.root = Node(); created = True
        return self._update_recurs(self.root, created, key, 0, upd)

    def _update_recurs(self, node, just_created, key, depth, upd):
        if depth < 16:
            pos = _child_idx(key, 15 - depth); created = False
            if node.children is None or node.children[pos] is None:
                if not self.has_children(node) and not just_created: self.expand_node(node)
                else:
                    if node.children is None: node.children = [None] * 8
                    node.children[pos] = Node(); created = True
            ret = self._update_recurs(node.children[pos], created, key, depth + 1, upd)
            if self.prune_node(node): ret = node
            else: node.value = max(c.value for c in node.children if c is not None)
            return ret
        v = f32(node.value + upd)
        node.value = self.clamp_min if v < self.clamp_min else (self.clamp_max if v > self.clamp_max else v)
        return node

    def prune(self):
        if self.root is None: return
        for depth in range(15, 0, -1):
            if self._prune_recurs(self.root, 0, depth) == 0: break

    def _prune_recurs(self, node, depth, max_depth):
        n = 0
        if depth < max_depth:
            for c in (node.children or ()):
                if c is not None: n += self._prune_recurs(c, depth + 1, max_depth)
        elif self.prune_node(node): n += 1
        return n

    def leaves(self):
        """the leaf iterator: (min-corner key, depth, value) depth first in child order"""
        if self.root is None: return
        stack = [(self.root, (0, 0, 0), 0)]
        while stack:
            n, k, d = stack.pop()
            if not self.has_children(n): yield k, d, n.value; continue
            h = 1 << (15 - d)
            for pos in range(7, -1, -1):
                c = n.children[pos]
                if c is not None: stack.append((c, (k[0] + (pos & 1) * h, k[1] + ((pos >> 1) & 1) * h, k[2] + ((pos >> 2) & 1) * h), d + 1))

    def expanded(self):
        """every depth-16 cell a leaf stands for, in the iterator's order (ascending Morton code): [(key, value)]"""
        out = []
        for k, d, v in self.leaves():
            if d == 16: out.append((k, v)); continue
            s = 1 << (16 - d); cells = [(k[0] + x, k[1] + y, k[2] + z) for z in range(s) for y in range(s) for x in range(s)]
            out.extend((c, v) for c in sorted(cells, key=morton))
        return out


class DictMap:
    """cells only: v = clamp(v + u), an unknown cell starts at 0"""

    def __init__(self, p):
        self.cells = {}; self.hit, self.miss = logodds(p['prob_hit']), logodds(p['prob_miss']); self.lo, self.hi = logodds(p['thres_min']), logodds(p['thres_max'])

    def update(self, key, occupied):
        v = f32(self.cells.get(key, f32(0.0)) + (self.hit if occupied else self.miss))
        self.cells[key] = self.lo if v < self.lo else (self.hi if v > self.hi else v)

    def apply(self, free, occ):
        for k in free:
            if k not in occ: self.update(k, False)
        for k in occ: self.update(k, True)

    def expanded(self):
        return [(k, self.cells[k]) for k in sorted(self.cells, key=morton)]


# ---- insertScan ----------------------------------------------------------------------------------------------------------------------------------------------------
def compute_ray_keys(res, o, e):
    """octomap's computeRayKeys(origin, end) -> (valid, keys, info); info: exit ('empty', 'end', 'length', 'left'), ties, len"""
    info = dict(exit='empty', ties=0)
    vo, ko = key3(res, o); ve, ke = key3(res, e)
    if not (vo and ve): return False, [], info
    if ko == ke: return True, [], info
    keys = [ko]
    d = [f32(e[i]) - f32(o[i]) for i in range(3)]
    length = f32(math.sqrt(float(f32(f32(f32(d[0] * d[0]) + f32(d[1] * d[1])) + f32(d[2] * d[2])))))
    d = [f32(d[i] / length) for i in range(3)]
    step = [0] * 3; tmax = [DBL_MAX] * 3; tdelta = [DBL_MAX] * 3
    for i in range(3):
        step[i] = 1 if d[i] > 0 else (-1 if d[i] < 0 else 0)
        if step[i] != 0:
            border = coord(res, ko[i]) + float(f32(step[i] * res * 0.5))
            tmax[i] = (border - float(f32(o[i]))) / float(d[i])
            tdelta[i] = res / abs(float(d[i]))
    cur = list(ko)
    while True:
        if tmax[0] < tmax[1]: dim = 0 if tmax[0] < tmax[2] else 2
        else: dim = 1 if tmax[1] < tmax[2] else 2
        srt = sorted(tmax)
        if srt[0] == srt[1]: info['ties'] += 1
        nk = cur[dim] + step[dim]
        if nk < 0 or nk > 65535: info['exit'] = 'left'; break
        cur[dim] = nk; tmax[dim] += tdelta[dim]
        if tuple(cur) == ke: info['exit'] = 'end'; break
        if min(tmax) > float(length): info['exit'] = 'length'; break
        keys.append(tuple(cur))
    return True, keys, info


def transform_and_filter(p, pts, m):
    """pcl::transformPointCloud and the PassThrough filters x, y, z; the survivors in order"""
    m = np.asarray(m, 'f4').reshape(4, 4); out = []
    lo = [to_f32(p['pointcloud_min_' + a]) for a in 'xyz']; hi = [to_f32(p['pointcloud_max_' + a]) for a in 'xyz']
    with np.errstate(all='ignore'):
        for q in np.asarray(pts, 'f4').reshape(-1, 3):
            t = [f32(f32(f32(f32(m[r, 0] * q[0]) + f32(m[r, 1] * q[1])) + f32(m[r, 2] * q[2])) + m[r, 3]) for r in range(3)]
            if all(np.isfinite(v) and not (v < lo[i] or v > hi[i]) for i, v in enumerate(t)): out.append(t)
    return out


def scan_sets(p, pts, m, trace=None):
    """insertScan up to the two sets -> (free, occupied, record)"""
    res = p['res']; mr = p['max_range']
    rec = dict(n_in=len(pts), n_passed=0, n_truncated=0, n_bad_end_key=0, n_invalid_rays=0, n_free_updates=0, n_occupied_updates=0, n_new_cells=0,
               bbx_min=[65535] * 3, bbx_max=[0] * 3, flags=0)
    m = np.asarray(m, 'f4').reshape(4, 4); o = [m[0, 3], m[1, 3], m[2, 3]]
    free, occ = set(), set()

    def box(k):
        for i in range(3): rec['bbx_min'][i] = min(rec['bbx_min'][i], k[i]); rec['bbx_max'][i] = max(rec['bbx_max'][i], k[i])
    vo, ko = key3(res, o)
    if vo: box(ko)
    else: rec['flags'] |= ORIGIN_OUT_OF_RANGE
    kept = transform_and_filter(p, pts, m); rec['n_passed'] = len(kept)
    with np.errstate(all='ignore'):
        for q in kept:
            d = [f32(q[i] - o[i]) for i in range(3)]
            norm = math.sqrt(float(f32(f32(f32(d[0] * d[0]) + f32(d[1] * d[1])) + f32(d[2] * d[2]))))
            if mr < 0 or norm <= mr:
                ok, keys, info = compute_ray_keys(res, o, q)
                if ok: free.update(keys)
                else: rec['n_invalid_rays'] += 1
                ve, ke = key3(res, q)
                if ve: occ.add(ke); box(ke)
                else: rec['n_bad_end_key'] += 1
            else:
                rec['n_truncated'] += 1
                ln = f32(norm); e = [f32(o[i] + f32(f32(d[i] / ln) * f32(mr))) for i in range(3)]
                ok, keys, info = compute_ray_keys(res, o, e)
                if ok:
                    free.update(keys)
                    ve, ke = key3(res, e)
                    if ve: free.add(ke); box(ke)
                else: rec['n_invalid_rays'] += 1
            if info['exit'] == 'left': rec['flags'] |= RAY_LEFT_KEYSPACE
            if trace is not None: trace.append(info)
    return free, occ, rec


class Octomap:
    """the tree with octomap_server's insertScan and queries; max_bricks / max_points as sgx_octomap_create"""

    def __init__(self, p, max_bricks=1 << 20, max_points=1 << 24):
        self.p = dict(p); self.tree = OcTree(p); self.max_bricks = max_bricks; self.max_points = max_points; self.bricks = set()

    def reset(self):
        self.tree.clear(); self.bricks = set()

    def insert(self, pts, m, trace=None):
        pts = np.asarray(pts, 'f4').reshape(-1, 3)
        if len(pts) > self.max_points:
            return dict(n_in=len(pts), n_passed=0, n_truncated=0, n_bad_end_key=0, n_invalid_rays=0, n_free_updates=0, n_occupied_updates=0, n_new_cells=0,
                        bbx_min=[65535] * 3, bbx_max=[0] * 3, flags=TOO_MANY_POINTS | (0 if key3(self.p['res'], np.asarray(m, 'f4').reshape(4, 4)[:3, 3])[0] else ORIGIN_OUT_OF_RANGE))
        free, occ, rec = scan_sets(self.p, pts, m, trace)
        need = self.bricks | {brick(k) for k in free} | {brick(k) for k in occ}
        if len(need) > self.max_bricks:
            rec['flags'] = (rec['flags'] & ~RAY_LEFT_KEYSPACE) | MAP_FULL; return rec      # a refused scan does not report RAY_LEFT_KEYSPACE
        self.bricks = need
        rec['n_new_cells'] = sum(1 for k in free | occ if self.tree.search(k) is None)
        for k in free:                                                   # :434-444, in the sets' own iteration order
            if k not in occ: self.tree.update_node(k, False); rec['n_free_updates'] += 1
        for k in occ: self.tree.update_node(k, True); rec['n_occupied_updates'] += 1
        self.tree.prune()
        self.last_sets = (free, occ)
        return rec

    def search(self, key):
        n = self.tree.search(tuple(int(v) for v in key))
        return f32(np.nan) if n is None else n.value

    def search_point(self, pt):
        ok, k = key3(self.p['res'], pt)
        return self.search(k) if ok else f32(np.nan)

    def bounds(self, cells=None):
        cells = self.tree.expanded() if cells is None else cells
        b = dict(n_known=len(cells), n_occupied=sum(1 for _, v in cells if v >= 0), n_free=sum(1 for _, v in cells if not v >= 0), key_min=[65535] * 3, key_max=[0] * 3)
        for k, _ in cells:
            for i in range(3): b['key_min'][i] = min(b['key_min'][i], k[i]); b['key_max'][i] = max(b['key_max'][i], k[i])
        return b

    def in_window(self, z, half):
        return z + half > self.p['occupancy_min_z'] and z - half < self.p['occupancy_max_z']

    def cells(self, occupied, cells=None):
        """[(key, centre floats, logodds)] of the occupied or free depth-16 cells inside the z window, in the iterator's order"""
        res = self.p['res']; out = []
        for k, v in (self.tree.expanded() if cells is None else cells):
            if bool(v >= 0) == bool(occupied) and self.in_window(coord(res, k[2]), res / 2.0): out.append((k, tuple(f32(coord(res, c)) for c in k), v))
        return out

    def header(self, b=None):
        b = self.bounds() if b is None else b; res = self.p['res']
        h = dict(width=0, height=0, flags=0, pad_min_key=[0, 0], pad_max_key=[0, 0], key_min_z=0, key_max_z=0, resolution=res, origin_x=0.0, origin_y=0.0)
        if b['n_known'] == 0: h['flags'] = GRID_EMPTY; return h
        lo = [coord(res, b['key_min'][i]) - res / 2.0 for i in range(3)]; hi = [coord(res, b['key_max'][i]) - res / 2.0 + res for i in range(3)]
        hp = [0.5 * self.p['min_size_x'], 0.5 * self.p['min_size_y']]
        for i in range(2): lo[i] = min(lo[i], -hp[i]); hi[i] = max(hi[i], hp[i])
        vmin, kmin = key3(res, [f32(v) for v in lo]); vmax, kmax = key3(res, [f32(v) for v in hi])
        if not (vmin and vmax) or kmax[0] < kmin[0] or kmax[1] < kmin[1]: h['flags'] = GRID_KEY_OUT_OF_RANGE; return h
        h.update(width=kmax[0] - kmin[0] + 1, height=kmax[1] - kmin[1] + 1, pad_min_key=list(kmin[:2]), pad_max_key=list(kmax[:2]), key_min_z=b['key_min'][2],
                 key_max_z=b['key_max'][2], origin_x=float(f32(coord(res, kmin[0]))) - res * 0.5, origin_y=float(f32(coord(res, kmin[1]))) - res * 0.5)
        return h

    def _fill(self, g, h, k, size, occupied):
        for dx in range(size):
            for dy in range(size):
                x = k[0] + dx - h['pad_min_key'][0]; y = k[1] + dy - h['pad_min_key'][1]
                if not (0 <= x < h['width'] and 0 <= y < h['height']): continue      # defined case: the reference would index outside its vector
                if occupied: g[y, x] = 100
                elif g[y, x] == -1: g[y, x] = 0

    def grid_from_leaves(self, h=None):
        """publishAll's traversal: leaves at their own depth, the z window at the node's size, update2DMap's square fill"""
        h = self.header() if h is None else h; res = self.p['res']; g = np.full((h['height'], h['width']), -1, 'i1')
        for k, d, v in self.tree.leaves():
            size = 1 << (16 - d)
            if self.in_window(coord_at(res, k[2], d), res * size / 2.0): self._fill(g, h, k, size, bool(v >= 0))
        return g

    def grid_from_cells(self, h=None, cells=None):
        h = self.header() if h is None else h; res = self.p['res']; g = np.full((h['height'], h['width']), -1, 'i1')
        for k, v in (self.tree.expanded() if cells is None else cells):
            if self.in_window(coord(res, k[2]), res / 2.0): self._fill(g, h, k, 1, bool(v >= 0))
        return g


def sensor_to_world(origin, q):
    """tf::Matrix3x3::setRotation in double, entries and origin cast to float"""
    x, y, z, w = [float(v) for v in q]; s = 2.0 / (x * x + y * y + z * z + w * w)
    xs, ys, zs = x * s, y * s, z * s; wx, wy, wz = w * xs, w * ys, w * zs; xx, xy, xz = x * xs, x * ys, x * zs; yy, yz, zz = y * ys, y * zs, z * zs
    m = np.eye(4, dtype='f4')
    m[:3, :3] = np.array([[1.0 - (yy + zz), xy - wz, xz + wy], [xy + wz, 1.0 - (xx + zz), yz - wx], [xz - wy, yz + wx, 1.0 - (xx + yy)]], 'f8').astype('f4')
    m[:3, 3] = np.asarray(origin, 'f8').astype('f4')
    return m
