"""Restatement of the front half of LocalMapping::Run over a small pointer-style map: ProcessNewKeyFrame (src/sg-slam/src/LocalMapping.cc:128-168), MapPointCulling
(:170-205), CreateNewMapPoints (:207-452) and ComputeF12 (:536-553), in plain Python / numpy float32 scalars.  It is the yardstick of the sgx_kfstore entries and of
sg_slam_amd.localmapping.  The two bodies the project already judges are not restated again: SearchForTriangulation and the per-pair body :286-431 are the oracle's
(oracle.search_for_triangulation, oracle.triangulate_pairs), and so are the two MapPoint post-steps (oracle.distinctive_descriptors, oracle.update_normal_and_depth).

Arithmetic, chosen here because OpenCV is not pinned; every cv::Mat is CV_32F:
  * a product without a transposed operand is cv::gemm's small-matrix path: float products summed left to right, then (float)(double(dot) * alpha + beta * double(c));
    A * B + C is one gemm (beta = 1), -A * B one gemm (alpha = -1).
  * a product with a transposed operand (R1w * R2w.t()) takes the generic path: products and sums in double, alpha applied to the double sum, one rounding to float.
    That is how camera_centre() of sgx_match2.cpp and the oracle evaluate -Rcw.t() * tcw.
  * GetCameraCenter() is KeyFrame::SetPose's Ow = -Rwc * tcw with Rwc = Rcw.t() STORED first (KeyFrame.cc:77-78): no transposed operand, so the float path with
    alpha = -1.  These centres serve vBaseline, the epipole and UpdateNormalAndDepth.  The per-pair body is the oracle's and forms its own centres from Tcw (the double
    path), as sgx_triangulate_new_map_points does.
  * cv::norm(vBaseline) accumulates the squares in double, takes the double square root and is stored in a float; baseline < mb compares floats, mb = mbf / fx in float;
    baseline / medianDepthKF2 is a float quotient compared with 0.01 in double.
  * ComputeF12: R12 = R1w * R2w.t() (double path); -R1w * R2w.t() is evaluated as its own gemm (alpha = -1, double path) because a product stands to its right;
    t12 = (that) * t2w + t1w is one gemm without flags, beta = 1; t12x holds exact negations; K1.t().inv() * t12x * R12 * K2.inv() is evaluated left to right, each
    product materialised (float path).  inv() of a 3 x 3 matrix is OpenCV's closed form: determinant and cofactors in double, d = 1 / det, one rounding per element;
    inv() * M is the inverse times M (not the solve() some versions substitute).
  * the epipole (ORBmatcher.cc:666-674): C2 = R2w * Cw + t2w one gemm (beta = 1), invz = 1.0f / C2.z, ex = fx * C2.x * invz + cx in float: the oracle does it from
    cam_center.
  * containers keyed by KeyFrame* run in ascending keyframe id (rule 1 of the covisibility section of include/sgx.h): the two observations of a new point.
Every branch of the restatement counts an event (EVENTS); check_events() asserts that a set of counters has all of them."""
import math
import numpy as np
import covis_ref

F32 = np.float32
PROCESSED, SKIPPED, UNKNOWN = 0, 1, -1
EVENTS = ('gate_skip_stereo', 'gate_skip_mono', 'gate_pass', 'unknown_keyframe', 'no_common_node', 'idx1_carried_filled', 'idx1_rejected_then_matched', 'pair_accepted',
          'pair_rejected', 'cull_bad', 'cull_found_ratio', 'cull_few_observations', 'cull_old', 'cull_kept', 'process_add_observation', 'process_recent')


def check_events(ev):
    missing = [k for k in EVENTS if not ev.get(k)]
    assert not missing, ('branches the case set never reached', missing)


def centre(T):
    """GetCameraCenter(): Ow = -Rwc * tcw, Rwc stored"""
    T = np.asarray(T, 'f4'); Ow = np.zeros(3, 'f4')
    for i in range(3):
        d = T[0, i] * T[0, 3] + T[1, i] * T[1, 3] + T[2, i] * T[2, 3]          # float32, left to right
        Ow[i] = F32(float(d) * -1.0)
    return Ow


def baseline(Ow1, Ow2):
    b = [Ow2[i] - Ow1[i] for i in range(3)]                                    # float32
    return F32(math.sqrt(float(b[0]) * float(b[0]) + float(b[1]) * float(b[1]) + float(b[2]) * float(b[2])))


def invert33(S):
    """cv::invert, 3 x 3 CV_32F, the closed form"""
    S = [float(x) for x in np.asarray(S, 'f4').reshape(9)]
    d = S[0] * (S[4] * S[8] - S[5] * S[7]) - S[1] * (S[3] * S[8] - S[5] * S[6]) + S[2] * (S[3] * S[7] - S[4] * S[6])
    assert d != 0.
    d = 1. / d
    t = [(S[4] * S[8] - S[5] * S[7]) * d, (S[2] * S[7] - S[1] * S[8]) * d, (S[1] * S[5] - S[2] * S[4]) * d,
         (S[5] * S[6] - S[3] * S[8]) * d, (S[0] * S[8] - S[2] * S[6]) * d, (S[2] * S[3] - S[0] * S[5]) * d,
         (S[3] * S[7] - S[4] * S[6]) * d, (S[1] * S[6] - S[0] * S[7]) * d, (S[0] * S[4] - S[1] * S[3]) * d]
    return np.array(t, 'f8').astype('f4').reshape(3, 3)


def mul33(A, B):
    C = np.zeros((3, 3), 'f4')
    for r in range(3):
        for c in range(3):
            d = A[r, 0] * B[0, c] + A[r, 1] * B[1, c] + A[r, 2] * B[2, c]      # float32, left to right
            C[r, c] = F32(float(d) * 1.0)
    return C


def compute_f12(T1, T2, cam):
    T1 = np.asarray(T1, 'f4'); T2 = np.asarray(T2, 'f4')
    K = np.array([[cam['fx'], 0, cam['cx']], [0, cam['fy'], cam['cy']], [0, 0, 1]], 'f4')
    R12 = np.zeros((3, 3), 'f4'); nR12 = np.zeros((3, 3), 'f4'); t12 = np.zeros(3, 'f4')
    for r in range(3):
        for c in range(3):
            s = 0.0
            for k in range(3): s += float(T1[r, k]) * float(T2[c, k])
            R12[r, c] = F32(s * 1.0); nR12[r, c] = F32(s * -1.0)
    for r in range(3):
        d = nR12[r, 0] * T2[0, 3] + nR12[r, 1] * T2[1, 3] + nR12[r, 2] * T2[2, 3]
        t12[r] = F32(float(d) * 1.0 + 1.0 * float(T1[r, 3]))
    tx = np.array([[0, -t12[2], t12[1]], [t12[2], 0, -t12[0]], [-t12[1], t12[0], 0]], 'f4')
    return mul33(mul33(mul33(invert33(K.T), tx), R12), invert33(K))


def _T44(T):
    out = np.zeros((4, 4), 'f4'); out[:3, :4] = np.asarray(T, 'f4')[:3, :4]; out[3, 3] = 1
    return out


def create_new_map_points(orc, kfs, cur, neighbours, rows, first_new_id, cam, sf, sg, median_depth=None, ev=None):
    """:207-452 for keyframe `cur` against `neighbours` in order.  kfs: id -> dict(keys_un, keys, desc, uright, depth, feat_node, Tcw); rows: mvpMapPoints of cur and of
    each neighbour as point ids (-1 none), updated in place as lists.  Returns the dict KeyFrameStore.create_new_map_points returns."""
    ev = ev if ev is not None else dict.fromkeys(EVENTS, 0)
    rows = [np.array(r, 'i4') for r in rows]
    rep = np.zeros(len(neighbours), [('status', 'i4'), ('kf2', 'i4'), ('n_pairs', 'i4'), ('n_new', 'i4'), ('baseline', 'f4'), ('F12', 'f4', (9,)), ('Ow1', 'f4', (3,)), ('Ow2', 'f4', (3,))])
    out = dict(new_kf2=[], new_idx1=[], new_idx2=[], x3d=[], desc=[], normal=[], min_dist=[], max_dist=[], pairs=[])
    filled_here = set(); rejected = set(); nnew = 0
    mb = F32(cam['bf']) / F32(cam['fx'])
    for j, kf2 in enumerate(neighbours):
        rep[j]['kf2'] = kf2; out['pairs'].append((np.zeros(0, 'i4'), np.zeros(0, 'i4'), np.zeros(0, 'u1')))
        if cur not in kfs or kf2 not in kfs or kf2 == cur or kf2 < 0:
            rep[j]['status'] = UNKNOWN; ev['unknown_keyframe'] += 1; continue
        a, b = kfs[cur], kfs[kf2]
        Ow1, Ow2 = centre(a['Tcw']), centre(b['Tcw'])
        bl = baseline(Ow1, Ow2)
        rep[j]['baseline'] = bl; rep[j]['Ow1'] = Ow1; rep[j]['Ow2'] = Ow2
        if median_depth is None:
            if bl < mb:                                                        # :249-253
                rep[j]['status'] = SKIPPED; ev['gate_skip_stereo'] += 1; continue
        else:
            ratio = bl / F32(median_depth[j])                                  # :254-261
            if float(ratio) < 0.01:
                rep[j]['status'] = SKIPPED; ev['gate_skip_mono'] += 1; continue
        ev['gate_pass'] += 1
        F12 = compute_f12(a['Tcw'], b['Tcw'], cam); rep[j]['F12'] = F12.reshape(9)
        n1, n2 = len(a['keys_un']), len(b['keys_un'])
        nodes2 = set(int(x) for x in b['feat_node'] if x >= 0)
        common = [i for i in range(n1) if a['feat_node'][i] >= 0 and int(a['feat_node'][i]) in nodes2]
        if not common: ev['no_common_node'] += 1
        if any(i in filled_here for i in common): ev['idx1_carried_filled'] += 1           # ORBmatcher.cc:704-705 skips what an earlier neighbour filled
        pairs = np.zeros((0, 2), 'i4')
        if n1 and n2:
            k1 = dict(keys=a['keys_un'], desc=a['desc'], uright=a['uright'], has_mp=(rows[0][:n1] >= 0).astype(np.uint8), feat_node=a['feat_node'], cam_center=Ow1)
            k2 = dict(keys=b['keys_un'], desc=b['desc'], uright=b['uright'], has_mp=(rows[j + 1][:n2] >= 0).astype(np.uint8), feat_node=b['feat_node'], Tcw=_T44(b['Tcw']))
            _, pairs = orc.search_for_triangulation(k1, k2, F12, False, cam, sf, sg, check_ori=False)
        ok = np.zeros(len(pairs), bool); x3d = np.zeros((len(pairs), 3), 'f4')
        if len(pairs):
            A = dict(keys_un=a['keys_un'], keys=a['keys'], uright=a['uright'], depth=a['depth'], Tcw=_T44(a['Tcw']))
            B = dict(keys_un=b['keys_un'], keys=b['keys'], uright=b['uright'], depth=b['depth'], Tcw=_T44(b['Tcw']))
            _, ok, x3d = orc.triangulate_pairs(pairs, A, B, cam, sf, sg)
        out['pairs'][-1] = (pairs[:, 0].copy(), pairs[:, 1].copy(), ok.astype('u1'))
        rep[j]['n_pairs'] = len(pairs); rep[j]['status'] = PROCESSED
        for (i1, i2), good, X in zip(pairs, ok, x3d):                          # the commit :433-447 in pair order
            i1 = int(i1); i2 = int(i2)
            if not good:
                ev['pair_rejected'] += 1; rejected.add(i1); continue
            ev['pair_accepted'] += 1
            if i1 in rejected: ev['idx1_rejected_then_matched'] += 1; rejected.discard(i1)
            pid = first_new_id + nnew
            rows[0][i1] = pid; rows[j + 1][i2] = pid; filled_here.add(i1)
            obs = sorted([(cur, a['desc'][i1], Ow1), (kf2, b['desc'][i2], Ow2)], key=lambda o: o[0])     # mObservations in ascending keyframe id
            best = orc.distinctive_descriptors([0, 2], np.stack([obs[0][1], obs[1][1]]))[0]
            nr, mn, mx = orc.update_normal_and_depth(X.reshape(1, 3), [0, 2], np.stack([obs[0][2], obs[1][2]]), Ow1.reshape(1, 3), [int(a['keys_un']['octave'][i1])], sf,
                                                     np.zeros((1, 3), 'f4'), np.zeros(1, 'f4'), np.zeros(1, 'f4'))
            out['new_kf2'].append(kf2); out['new_idx1'].append(i1); out['new_idx2'].append(i2); out['x3d'].append(X); out['desc'].append(obs[best][1])
            out['normal'].append(nr[0]); out['min_dist'].append(mn[0]); out['max_dist'].append(mx[0])
            nnew += 1; rep[j]['n_new'] += 1
    res = dict(rows=rows, n_new=nnew, report=rep, pairs=out['pairs'])
    for k, dt, shape in (('new_kf2', 'i4', (0,)), ('new_idx1', 'i4', (0,)), ('new_idx2', 'i4', (0,)), ('x3d', 'f4', (0, 3)), ('desc', 'u1', (0, 32)), ('normal', 'f4', (0, 3)),
                         ('min_dist', 'f4', (0,)), ('max_dist', 'f4', (0,))):
        res[k] = np.array(out[k], dt) if out[k] else np.zeros(shape, dt)
    return res


class LocalMappingRef:
    """the map as objects: the relation is covis_ref.Map, the keyframes' data and the points' attributes live here"""
    def __init__(self, orc, cam, sf, sg, monocular=False, th_depth=40.0):
        self.orc = orc; self.cam = cam; self.sf = np.asarray(sf, 'f4'); self.sg = np.asarray(sg, 'f4'); self.mbMonocular = bool(monocular)
        self.R = covis_ref.Map(monocular, th_depth)
        self.kf = {}; self.pt = {}; self.recent = []; self.ev = dict.fromkeys(EVENTS, 0)

    def isBad(self, pid):
        return pid not in self.R.points

    def _post_steps(self, pid):
        """UpdateNormalAndDepth + ComputeDistinctiveDescriptors of one point over its observations (MapPoint.cc:330-371, :242-307)"""
        obs, _ = self.R.observations(pid); p = self.pt[pid]
        oc = np.stack([centre(self.kf[k]['Tcw']) for k, _ in obs]); dd = np.stack([self.kf[k]['desc'][i] for k, i in obs])
        ref = p['ref_kf']; lvl = int(self.kf[ref]['keys_un']['octave'][dict(obs)[ref]])
        nr, mn, mx = self.orc.update_normal_and_depth(p['xw'].reshape(1, 3), [0, len(obs)], oc, centre(self.kf[ref]['Tcw']).reshape(1, 3), [lvl], self.sf,
                                                      p['normal'].reshape(1, 3), [p['min_dist']], [p['max_dist']])
        p['normal'] = nr[0]; p['min_dist'] = mn[0]; p['max_dist'] = mx[0]
        p['desc'] = dd[self.orc.distinctive_descriptors([0, len(obs)], dd)[0]].copy()

    def new_point(self, pid, xw, ref_kf, found=1, visible=1):
        self.pt[pid] = dict(xw=np.asarray(xw, 'f4').copy(), desc=np.zeros(32, 'u1'), normal=np.zeros(3, 'f4'), min_dist=F32(0), max_dist=F32(0), ref_kf=int(ref_kf), first_kf=int(ref_kf),
                            visible=int(visible), found=int(found))

    def ProcessNewKeyFrame(self, kf_id, data, matches, new_stereo=None):
        """:128-168.  matches: the keyframe's mvpMapPoints from Tracking as point ids (-1 none); new_stereo: {idx: (point id, xw)}, the points Tracking created with
        the keyframe (Tracking.cc:1196-1245), which observe it already"""
        self.kf[kf_id] = data
        self.R.add_keyframe(kf_id, data['keys_un']['octave'].astype('i4'), data['uright'], data['depth'])
        for i, (pid, xw) in sorted((new_stereo or {}).items()):                # Tracking::CreateNewKeyFrame: AddObservation, AddMapPoint, the two post-steps
            self.new_point(pid, xw, kf_id); self.R.set_observations(kf_id, [i], [pid]); self._post_steps(pid)
        for i, pid in enumerate(matches):
            if pid < 0: continue
            if self.isBad(pid): continue
            if (kf_id, i) not in self.R.observations(pid)[0]:                  # !IsInKeyFrame
                self.R.set_observations(kf_id, [i], [pid]); self._post_steps(pid); self.ev['process_add_observation'] += 1
            else:
                self.recent.append(pid); self.ev['process_recent'] += 1
        self.R.update_connections(kf_id)

    def MapPointCulling(self, kf_id):
        """:170-205"""
        th = 2 if self.mbMonocular else 3
        keep = []
        for pid in self.recent:
            p = self.pt[pid]
            if self.isBad(pid): self.ev['cull_bad'] += 1
            elif F32(p['found']) / F32(p['visible']) < F32(0.25):
                self.R.set_points_bad([pid]); self.ev['cull_found_ratio'] += 1
            elif (int(kf_id) - int(p['first_kf'])) >= 2 and self.R.observations(pid)[1] <= th:
                self.R.set_points_bad([pid]); self.ev['cull_few_observations'] += 1
            elif (int(kf_id) - int(p['first_kf'])) >= 3: self.ev['cull_old'] += 1
            else:
                keep.append(pid); self.ev['cull_kept'] += 1
        self.recent = keep

    def CreateNewMapPoints(self, kf_id, first_new_id, stop_after=None, median_depth=None):
        nbs = self.R.best_covisibles(kf_id, 20 if self.mbMonocular else 10)
        if stop_after is not None: nbs = nbs[:max(int(stop_after), 1)] if nbs else nbs          # CheckNewKeyFrames() is only asked for i > 0 (:239)
        rows = [self.R.keyframe_points(kf_id)] + [self.R.keyframe_points(k) for k in nbs]
        res = create_new_map_points(self.orc, self.kf, kf_id, nbs, rows, first_new_id, self.cam, self.sf, self.sg, None if median_depth is None else median_depth[:len(nbs)], self.ev)
        for k in range(res['n_new']):
            pid = first_new_id + k; kf2 = int(res['new_kf2'][k])
            self.R.set_observations(kf_id, [int(res['new_idx1'][k])], [pid]); self.R.set_observations(kf2, [int(res['new_idx2'][k])], [pid])
            self.new_point(pid, res['x3d'][k], kf_id)
            p = self.pt[pid]; p['desc'] = res['desc'][k].copy(); p['normal'] = res['normal'][k].copy(); p['min_dist'] = res['min_dist'][k]; p['max_dist'] = res['max_dist'][k]
            self.recent.append(pid)
        return res
