"""Restatement of Detector3D::DetectOne (src/sg-slam/src/Detector3D.cc:41-168) with the PCL calls it makes, in numpy, brute force: the yardstick of the device kernels
(sg_slam_amd/csrc/sgx_obj3d_kernels.h) and of the emulator.  PCL and FLANN are not part of the tree: StatisticalOutlierRemoval::applyFilterIndices,
extractEuclideanClusters, compute3DCentroid and getMinMax3D are restated from their published sources (PCL 1.8 .. 1.12 agree on them), UNPINNED, like every
third-party primitive here.  An exact k nearest neighbour search and an exact radius search stand for the kd-tree.

Number formats as the reference has them: depth, camera point and world point float; Twc double; d2 float in x, y, z order; the neighbour sum, the two global sums,
mean, variance and threshold double; centroid a float running sum; the similarity float."""
import numpy as np

f32 = np.float32


def crop_cells(rect, width, height):
    """(x0, y0, cw, ch) of the crop grid (:47-58): `(size_t)rect2d.height*0.2` casts first, multiplies in double, truncates"""
    x, y, w, h = (f32(v) for v in rect)
    if not (x >= 0 and y >= 0 and w >= 0 and h >= 0 and f32(x + w) <= f32(width) and f32(y + h) <= f32(height)):
        raise ValueError('rect not inside the image')
    rb, re = int(float(int(h)) * 0.2), int(float(int(h)) * 0.8)
    cb, ce = int(float(int(w)) * 0.2), int(float(int(w)) * 0.8)
    return int(x) + cb, int(y) + rb, ce - cb, re - rb


def crop_points(depth, rect, dmin, dmax):
    """flat indices j (ascending) of the crop's valid depths"""
    H, W = depth.shape
    x0, y0, cw, ch = crop_cells(rect, W, H)
    rows, cols = np.meshgrid(np.arange(y0, y0 + ch), np.arange(x0, x0 + cw), indexing='ij')
    j = (rows * W + cols).reshape(-1)
    d = depth.reshape(-1)[j]
    with np.errstate(invalid='ignore'):
        ok = ~((d < f32(dmin)) | (d > f32(dmax)) | np.isnan(d))
    return j[ok]


def world_points(depth, cam, Twc, j):
    W = depth.shape[1]
    fx, fy, cx, cy = (f32(v) for v in cam)
    n = (j % W).astype(f32); m = (j // W).astype(f32)
    d = depth.reshape(-1)[j].astype(f32)
    x = ((n - cx) * d / fx).astype(f32); y = ((m - cy) * d / fy).astype(f32); z = d
    T = np.asarray(Twc, 'f8').reshape(4, 4)
    xd, yd, zd = x.astype('f8'), y.astype('f8'), z.astype('f8')
    return np.stack([((T[r, 0] * xd + T[r, 1] * yd) + T[r, 2] * zd) + T[r, 3] for r in range(3)], 1).astype(f32)


def d2_rows(P, i0, i1):
    """float d2 of points i0..i1 against all: (dx * dx + dy * dy) + dz * dz"""
    dx = P[i0:i1, None, 0] - P[None, :, 0]; dy = P[i0:i1, None, 1] - P[None, :, 1]; dz = P[i0:i1, None, 2] - P[None, :, 2]
    return (dx * dx + dy * dy) + dz * dz


def seq_sum(v):
    """sum of doubles one after the other, as a C loop does (numpy's add.accumulate is sequential; np.sum is pairwise)"""
    v = np.asarray(v, 'f8')
    return float(np.add.accumulate(v)[-1]) if len(v) else 0.0


def sor(P, mean_k, mul):
    """(dist float[n], terms: the n x mean_k float sqrt terms in ascending order, thr, kept)"""
    n = len(P); K = mean_k + 1
    terms = np.zeros((n, mean_k), f32)
    for i0 in range(0, n, 512):
        d2 = d2_rows(P, i0, min(n, i0 + 512))
        small = np.sort(np.partition(d2, K - 1, axis=1)[:, :K], axis=1)          # the K smallest, ascending; the first is the point itself
        terms[i0:i0 + 512] = np.sqrt(small[:, 1:])                               # sqrtf, correctly rounded
    dist = np.array([f32(seq_sum(t) / mean_k) for t in terms], f32)
    s = seq_sum(dist); sq = seq_sum((dist * dist).astype(f32))
    mean = s / n; var = (sq - s * s / n) / (n - 1)
    thr = mean + float(mul) * np.sqrt(var)
    kept = ~(dist.astype('f8') > thr)
    return dist, terms, thr, kept


def components(P, tol):
    """labels[i] = smallest index of i's component of the graph d2 < (float)((double)tol * (double)tol)"""
    n = len(P); t2 = f32(float(f32(tol)) * float(f32(tol)))
    adj = np.zeros((n, n), bool)
    for i0 in range(0, n, 512):
        adj[i0:i0 + 512] = d2_rows(P, i0, min(n, i0 + 512)) < t2
    lab = np.full(n, -1, np.int64)
    for s in range(n):
        if lab[s] >= 0: continue
        seen = np.zeros(n, bool); seen[s] = True; front = np.array([s])
        while len(front):
            new = adj[front].any(0) & ~seen
            seen |= new; front = np.nonzero(new)[0]
        lab[seen] = s
    return lab, adj


def similarity(r1, r2, points):
    """Detector3D::GetSimilarity (:204-218), float; powf(x, 2) taken as x * x"""
    x1, y1, w1, h1 = (f32(v) for v in r1); x2, y2, w2, h2 = (f32(v) for v in r2)
    two = f32(2)
    c1x, c1y, c2x, c2y = x1 + w1 / two, y1 + h1 / two, x2 + w2 / two, y2 + h2 / two
    a1, a2 = w1 * h1, w2 * h2
    ix, iy = max(x1, x2), max(y1, y2)
    iw, ih = min(x1 + w1, x2 + w2) - ix, min(y1 + h1, y2 + h2) - iy
    if iw <= 0 or ih <= 0: iw = ih = f32(0)
    a0 = iw * ih
    with np.errstate(all='ignore'):
        overlap = a0 / (a1 + a2 - a0)
        dx, dy = c1x - c2x, c1y - c2y
        deviate = dx * dx + dy * dy
        score = f32(float(f32(points)) / 10.0)
        return f32(f32(overlap * score) / deviate)


def detect_one(depth, cam, Twc, obj, p):
    """obj = (class id, prob, (x, y, w, h)); p = dict with the keys of settings.load_mapping.  Returns a dict: found, class_id, prob, centroid, size, the diagnostics
    of sgx_obj3d_result (except larger_window_points, which the implementation defines) and, for the tap, j, kept, labels (-1 for removed points), dist, terms, thr"""
    depth = np.asarray(depth, f32); H, W = depth.shape
    cid, prob, rect = obj
    mean_k = int(p['Sor_MeanK'])
    if mean_k < 1: raise ValueError('mean_k < 1')
    dmin, dmax = f32(p['camera_valid_depth_Min']), f32(p['camera_valid_depth_Max'])
    j = crop_points(depth, rect, dmin, dmax)
    n = len(j)
    out = dict(found=0, class_id=int(cid), prob=f32(prob), centroid=np.zeros(3, f32), size=np.zeros(3, f32), crop_points=n, kept_points=0, components=0, clusters=0,
               best_cluster_size=0, best_similar1=f32(-1), best_similar2=f32(-1), best_roi=np.zeros(4, f32), j=j, kept=np.zeros(n, bool), labels=np.full(n, -1, np.int64))
    if n <= mean_k:                                                   # defined case: the reference reads past the neighbour list
        return out
    P = world_points(depth, cam, Twc, j)
    dist, terms, thr, kept = sor(P, mean_k, p['Sor_StddevMulThresh'])
    out.update(dist=dist, terms=terms, thr=thr, kept=kept, kept_points=int(kept.sum()), world=P)
    ki = np.nonzero(kept)[0]
    Q = P[ki]
    lab_k, adj = components(Q, p['EuclideanClusterTolerance'])
    labels = np.full(n, -1, np.int64); labels[ki] = ki[lab_k]
    roots, sizes = np.unique(lab_k, return_counts=True)
    out.update(labels=labels, components=len(roots), adj=adj)
    keep = (sizes >= int(p['EuclideanClusterMinSize'])) & (sizes <= int(p['EuclideanClusterMaxSize']))
    roots, sizes = roots[keep], sizes[keep]
    order = np.lexsort((roots, -sizes))                               # size descending; equal sizes by smallest point (defined case: PCL's sort is unstable)
    out['clusters'] = len(roots)
    best1, best2, best = f32(-1), f32(-1), None
    for o in order:
        idx = ki[lab_k == roots[o]]                                   # ascending
        C = P[idx]
        cen = np.add.accumulate(C, axis=0)[-1] / f32(len(idx))        # float running sum, / (float)n
        if cen[2] < dmin: continue                                    # the reference's quirk: WORLD z against the camera's minimum depth
        px = (j[idx] % W).astype(np.uint32); py = (j[idx] // W).astype(np.uint32)
        rx, ry = f32(px.min()), f32(py.min())
        roi = (rx, ry, f32(px.max()) - rx, f32(py.max()) - ry)
        s = similarity(rect, roi, len(idx))
        if s > best1:
            best, best1 = (cen, C, roi, len(idx)), s
        elif s > best2:
            best2 = s
    out.update(best_similar1=best1, best_similar2=best2)
    if best is None:                                                  # defined case: no cluster chosen
        return out
    out.update(best_cluster_size=best[3], best_roi=np.array(best[2], f32))
    if best1 * f32(p['DetectSimilarCompareRatio']) < best2 and best2 > 0:
        return out
    out.update(found=1, centroid=best[0].astype(f32), size=(best[1].max(0) - best[1].min(0)).astype(f32))
    return out


class ObjectDatabaseRef:
    """ObjectDatabase::addObject (ObjectDatabase.cc:44-112)"""

    def __init__(self):
        self.sizes = [f32(0.6)] * 21; self.sizes[5] = f32(0.2); self.sizes[9] = f32(1.0); self.sizes[20] = f32(0.5)
        self.objs = []; self.n = 0

    def add(self, class_id, prob, centroid, size):
        c = dict(class_id=int(class_id), prob=f32(prob), centroid=np.array(centroid, f32), size=np.array(size, f32))
        best, center_distance = None, f32(100)
        for o in self.objs:
            if o['class_id'] != c['class_id']: continue
            d = c['centroid'] - o['centroid']
            dist = np.sqrt(f32(f32(d[0] * d[0] + d[1] * d[1]) + d[2] * d[2]))
            if dist < center_distance: center_distance, best = dist, o
        if best is not None and center_distance < self.sizes[c['class_id']]:
            best['prob'] = f32(float(best['prob'] + c['prob']) / 2.0)
            best['centroid'] = (best['centroid'] + c['centroid']) / f32(2); best['size'] = (best['size'] + c['size']) / f32(2)
            return best['object_id'], True
        self.n += 1; c['object_id'] = self.n; self.objs.append(c)
        return self.n, False
