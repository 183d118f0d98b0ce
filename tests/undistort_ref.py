"""numpy float64 restatement of the lens-distortion stages (tests only), written from OpenCV 3.4.15's cvUndistortPointsInternal on the 32F point path as
cv::undistortPoints(src, dst, K, D, noArray(), K) reaches it with its default TermCriteria(MAX_ITER, 5, 0.01), and from the reference's Frame helpers
(src/sg-slam/src/Frame.cc:654-714, :893-914).  Every expression is evaluated in the order it is written there, so the results are the library's bits."""
import numpy as np

KP_DTYPE = np.dtype([('x', 'f4'), ('y', 'f4'), ('size', 'f4'), ('angle', 'f4'), ('response', 'f4'), ('octave', 'i4'), ('class_id', 'i4')])


def padded(dist):
    d = np.asarray(dist, 'f4').reshape(-1)
    assert len(d) in (4, 5, 8)
    k = np.zeros(12, 'f8'); k[:len(d)] = d.astype('f8')
    return k


def undistort_points(pts, cam, dist):
    """(n, 2) float32 -> (n, 2) float32"""
    p = np.asarray(pts, 'f4').reshape(-1, 2)
    k = padded(dist)
    fx, fy, cx, cy = (np.float64(np.float32(cam[c])) for c in ('fx', 'fy', 'cx', 'cy'))
    u = p[:, 0].astype('f8'); v = p[:, 1].astype('f8')
    ifx = 1. / fx; ify = 1. / fy
    x = (u - cx) * ifx; y = (v - cy) * ify
    x0 = x.copy(); y0 = y.copy()
    done = np.zeros(len(p), bool)
    with np.errstate(all='ignore'):
        for _ in range(5):
            r2 = x * x + y * y
            icdist = (1 + ((k[7] * r2 + k[6]) * r2 + k[5]) * r2) / (1 + ((k[4] * r2 + k[1]) * r2 + k[0]) * r2)
            neg = (~done) & (icdist < 0)                       # regression_14583 guard: back to the normalised input, stop
            x = np.where(neg, (u - cx) * ifx, x); y = np.where(neg, (v - cy) * ify, y)
            done |= neg
            deltaX = 2 * k[2] * x * y + k[3] * (r2 + 2 * x * x) + k[8] * r2 + k[9] * r2 * r2
            deltaY = k[2] * (r2 + 2 * y * y) + 2 * k[3] * x * y + k[10] * r2 + k[11] * r2 * r2
            x = np.where(done, x, (x0 - deltaX) * icdist)
            y = np.where(done, y, (y0 - deltaY) * icdist)
        out = np.stack([(fx * x + cx).astype('f4'), (fy * y + cy).astype('f4')], 1)
    return out


def image_bounds(width, height, cam, dist):
    """Frame::ComputeImageBounds (Frame.cc:686-714) -> (min_x, max_x, min_y, max_y) float32"""
    if np.float32(np.asarray(dist, 'f4').reshape(-1)[0]) == 0:
        return np.float32(0), np.float32(width), np.float32(0), np.float32(height)
    m = undistort_points(np.array([[0, 0], [width, 0], [0, height], [width, height]], 'f4'), cam, dist)
    mn = lambda a, b: b if b < a else a                      # std::min / std::max
    mx = lambda a, b: b if a < b else a
    return mn(m[0, 0], m[2, 0]), mx(m[1, 0], m[3, 0]), mn(m[0, 1], m[1, 1]), mx(m[2, 1], m[3, 1])


def undistort_keypoints(keys, cam, dist):
    """Frame::UndistortKeyPoints (Frame.cc:654-684): mvKeysUn, keypoint records with pt replaced (a copy when k1 == 0)"""
    keys = np.asarray(keys).view(KP_DTYPE)
    out = keys.copy()
    if np.float32(np.asarray(dist, 'f4').reshape(-1)[0]) == 0 or len(keys) == 0:
        return out
    un = undistort_points(np.stack([keys['x'], keys['y']], 1), cam, dist)
    out['x'] = un[:, 0]; out['y'] = un[:, 1]
    return out


def cam_with_bounds(cam, dist, width=640, height=480):
    c = dict(cam)
    c['min_x'], c['max_x'], c['min_y'], c['max_y'] = (float(v) for v in image_bounds(width, height, cam, dist))
    return c
