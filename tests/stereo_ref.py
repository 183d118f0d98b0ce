"""Frame::ComputeStereoMatches (src/sg-slam/src/Frame.cc:716-890) restated in numpy, literally: a row table, the candidate loop, the 11 x 11 window at 11 offsets,
the parabola and the median cut, every float operation an np.float32 operation in the reference's order.  The parity target of the emulator and of the device
(tests/test_stereo_emu.py, tests/test_stereo_gpu.py); test code.

Defined where the reference is not:
  * mb is read at Frame.cc:99 before :123 assigns it: mb = bf / fx and maxD = bf / mb, both in float
  * rows of the row table outside [0, nRows) are dropped, a left keypoint whose row is outside it has no candidates; a non-finite y, or an octave that is no level
    of the pyramid, takes no part
  * after the reference's own border test (:823-826, kept as it is), a window of which any pixel lies outside its level gives no match
  * no accepted match: nothing to cut

compute_stereo_matches also returns which exit every left keypoint took (the codes below).  DELTA is listed for completeness: bestincR is the FIRST minimum of the
11 values and not an end of the range, so d1 > d2 <= d3 and |d1 - d3| <= d1 + d3 - 2 d2, hence |deltaR| <= 0.5 or deltaR is NaN (0 / 0 cannot occur with d1 > d2):
the exit at :854 cannot be taken."""
import math
import numpy as np

F = np.float32
TH_HIGH, TH_LOW = 100, 50
NO_CANDIDATES, LEFT_OF_IMAGE, NO_DESCRIPTOR, BORDER, WINDOW_OUTSIDE, EDGE_OFFSET, DELTA, DISPARITY, ACCEPTED, ACCEPTED_CLAMPED, CUT = range(11)
CODE_NAMES = ('no candidates', 'maxU < 0', 'bestDist >= thOrbDist', 'border test', 'window outside its level', 'bestincR at the end of the range', 'deltaR outside [-1, 1]',
              'disparity outside [0, maxD)', 'accepted', 'accepted, disparity == 0 clamp', 'accepted, reset by the median cut')
_POP = np.array([bin(i).count('1') for i in range(256)], np.int32)


def cround(x):
    """round() of a float: half away from zero (exact in double for a float argument)"""
    x = float(x)
    return F(math.copysign(math.floor(abs(x) + 0.5), x)) if math.isfinite(x) else F(x)


def row_table(keys_right, scale, n_rows):
    """vRowIndices (:725-743): the list of right keypoints of every image row, in ascending iR"""
    rows = [[] for _ in range(n_rows)]
    for iR in range(len(keys_right)):
        y = F(keys_right['y'][iR]); octave = int(keys_right['octave'][iR])
        if not (0 <= octave < len(scale)) or not math.isfinite(float(y)):
            continue
        r = F(2.0) * F(scale[octave])
        maxr = math.ceil(float(F(y + r))); minr = math.floor(float(F(y - r)))
        for yi in range(max(minr, 0), min(maxr, n_rows - 1) + 1):
            rows[yi].append(iR)
    return rows


def descriptor_distance(a, b):
    return int(_POP[np.bitwise_xor(a, b)].sum())


def compute_stereo_matches(keys_left, desc_left, keys_right, desc_right, pyr_left, pyr_right, scale, inv_scale, fx, bf):
    """keys: KP_DTYPE records, desc: n x 32 bytes, pyr: one 2-D uint8 array per level, scale / inv_scale: mvScaleFactors / mvInvScaleFactors (float32).
    Returns dict(uright, depth, best_idx, best_dist, code, best_inc, sads): one entry per left keypoint"""
    N = len(keys_left)
    uright = np.full(N, -1, F); depth = np.full(N, -1, F)
    best_idx = np.zeros(N, np.int32); best_dist = np.full(N, TH_HIGH, np.int32); code = np.full(N, NO_CANDIDATES, np.int32)
    best_inc = np.zeros(N, np.int32); sads = np.full((N, 11), -1, np.int32)
    thOrbDist = (TH_HIGH + TH_LOW) // 2
    nRows = pyr_left[0].shape[0]; nlev = len(pyr_left)
    vRowIndices = row_table(keys_right, scale, nRows)
    bf = F(bf); mb = bf / F(fx)
    minD = F(0); maxD = bf / mb
    vDistIdx = []
    for iL in range(N):
        levelL = int(keys_left['octave'][iL]); vL = F(keys_left['y'][iL]); uL = F(keys_left['x'][iL])
        if not (vL > F(-1) and vL < F(nRows)) or not (0 <= levelL < nlev):
            continue
        vCandidates = vRowIndices[int(vL)]
        if not vCandidates:
            continue
        minU = uL - maxD; maxU = uL - minD
        if maxU < 0:
            code[iL] = LEFT_OF_IMAGE; continue
        bestDist = TH_HIGH; bestIdxR = 0
        for iR in vCandidates:
            octR = int(keys_right['octave'][iR])
            if octR < levelL - 1 or octR > levelL + 1:
                continue
            uR = F(keys_right['x'][iR])
            if uR >= minU and uR <= maxU:
                dist = descriptor_distance(desc_left[iL], desc_right[iR])
                if dist < bestDist:
                    bestDist = dist; bestIdxR = iR
        best_idx[iL] = bestIdxR; best_dist[iL] = bestDist
        if not bestDist < thOrbDist:
            code[iL] = NO_DESCRIPTOR; continue
        uR0 = F(keys_right['x'][bestIdxR]); scaleFactor = F(inv_scale[levelL])
        scaleduL = cround(uL * scaleFactor); scaledvL = cround(vL * scaleFactor); scaleduR0 = cround(uR0 * scaleFactor)
        w = 5; L = 5
        IL_img = pyr_left[levelL]; IR_img = pyr_right[levelL]
        iniu = scaleduR0 + F(L) - F(w); endu = scaleduR0 + F(L) + F(w) + F(1)
        if iniu < 0 or endu >= IR_img.shape[1]:
            code[iL] = BORDER; continue
        rows_, cols_ = IL_img.shape
        if not (scaleduL >= 5 and scaleduL <= cols_ - 6 and scaledvL >= 5 and scaledvL <= rows_ - 6 and scaleduR0 >= 10 and scaleduR0 <= cols_ - 11):
            code[iL] = WINDOW_OUTSIDE; continue
        su, sv, sr = int(scaleduL), int(scaledvL), int(scaleduR0)
        IL = IL_img[sv - w:sv + w + 1, su - w:su + w + 1].astype(np.int32); IL = IL - IL[w, w]
        bestSad = 2 ** 31 - 1; bestincR = 0
        for incR in range(-L, L + 1):
            IR = IR_img[sv - w:sv + w + 1, sr + incR - w:sr + incR + w + 1].astype(np.int32); IR = IR - IR[w, w]
            dist = int(np.abs(IL - IR).sum())
            if dist < bestSad:
                bestSad = dist; bestincR = incR
            sads[iL, L + incR] = dist
        best_inc[iL] = bestincR
        if bestincR == -L or bestincR == L:
            code[iL] = EDGE_OFFSET; continue
        dist1 = F(sads[iL, L + bestincR - 1]); dist2 = F(sads[iL, L + bestincR]); dist3 = F(sads[iL, L + bestincR + 1])
        with np.errstate(all='ignore'):
            deltaR = (dist1 - dist3) / (F(2.0) * (dist1 + dist3 - F(2.0) * dist2))
        if deltaR < -1 or deltaR > 1:
            code[iL] = DELTA; continue
        bestuR = F(scale[levelL]) * (scaleduR0 + F(bestincR) + deltaR)
        disparity = uL - bestuR
        if disparity >= minD and disparity < maxD:
            code[iL] = ACCEPTED
            if disparity <= 0:
                disparity = F(0.01); bestuR = F(np.float64(uL) - 0.01); code[iL] = ACCEPTED_CLAMPED
            depth[iL] = bf / disparity; uright[iL] = bestuR
            vDistIdx.append((bestSad, iL))
        else:
            code[iL] = DISPARITY
    if vDistIdx:
        vDistIdx.sort()
        median = F(vDistIdx[len(vDistIdx) // 2][0])
        thDist = F(1.5) * F(1.4) * median
        for i in range(len(vDistIdx) - 1, -1, -1):
            if F(vDistIdx[i][0]) < thDist:
                break
            uright[vDistIdx[i][1]] = -1; depth[vDistIdx[i][1]] = -1; code[vDistIdx[i][1]] = CUT
    return dict(uright=uright, depth=depth, best_idx=best_idx, best_dist=best_dist, code=code, best_inc=best_inc, sads=sads)
