"""LocalMapping — the front half of the local-mapping thread of the reference (src/sg-slam/src/LocalMapping.cc:47-112) over a CovisibilityGraph and a KeyFrameStore:
ProcessNewKeyFrame (:128-168), MapPointCulling (:170-205) and CreateNewMapPoints (:207-452).  The relation keyframe x map point lives in the covisibility handle, the
keyframes' features in the store; this class owns what neither holds: a host table of map-point attributes by id and mlpRecentAddedMapPoints.  SearchInNeighbors,
LocalBundleAdjustment and KeyFrameCulling are the caller's next steps (CovisibilityGraph.local_ba_graph, Optimizer, CovisibilityGraph.keyframe_culling); ComputeBoW and
ComputeSceneMedianDepth stay with the caller."""
import numpy as np
from . import mappoint


def camera_centre(Tcw):
    """KeyFrame::GetCameraCenter(): Ow = -Rwc * tcw with Rwc = Rcw.t() stored (KeyFrame.cc:77-78): float products left to right, alpha = -1 last"""
    T = np.asarray(Tcw, 'f4'); Ow = np.zeros(3, 'f4')
    for i in range(3):
        d = T[0, i] * T[0, 3] + T[1, i] * T[1, 3] + T[2, i] * T[2, 3]
        Ow[i] = np.float32(float(d) * -1.0)
    return Ow


class LocalMapping:
    ATTRS = ('xw', 'desc', 'normal', 'min_dist', 'max_dist', 'ref_kf', 'first_kf', 'visible', 'found')

    def __init__(self, covis, store, monocular=False):
        self.covis = covis; self.store = store; self.mbMonocular = bool(monocular); self.lib = covis.lib
        self.points = {}                                  # point id -> dict of ATTRS
        self.kf = {}                                      # keyframe id -> what the MapPoint post-steps read of it on the host: desc, octave (mvKeysUn), Ow
        self.mlpRecentAddedMapPoints = []
        self.next_point_id = 0

    # ---- the attribute table
    def add_point(self, pid, xw, ref_kf, found=1, visible=1):
        """a MapPoint as its constructor leaves it (MapPoint.cc:32-44): mnFound = mnVisible = 1, mnFirstKFid = pRefKF->mnId"""
        self.points[int(pid)] = dict(xw=np.asarray(xw, 'f4').reshape(3).copy(), desc=np.zeros(32, 'u1'), normal=np.zeros(3, 'f4'), min_dist=np.float32(0), max_dist=np.float32(0),
                                     ref_kf=int(ref_kf), first_kf=int(ref_kf), visible=int(visible), found=int(found))
        self.next_point_id = max(self.next_point_id, int(pid) + 1)

    def increase_found(self, pid, n=1):
        self.points[int(pid)]['found'] += int(n)

    def increase_visible(self, pid, n=1):
        self.points[int(pid)]['visible'] += int(n)

    def isBad(self, pid):
        return not self.covis.observations(pid)[0]        # a point exists exactly while it has an observation

    def set_pose(self, kf_id, Tcw):
        """after a bundle adjustment"""
        self.store.set_pose(kf_id, Tcw); self.kf[int(kf_id)]['Ow'] = camera_centre(Tcw)

    def _post_steps(self, pids):
        """UpdateNormalAndDepth + ComputeDistinctiveDescriptors (MapPoint.cc:330-371, :242-307) of the listed points over covis.observations, one batch each"""
        if not pids: return
        st = [0]; oc = []; dd = []; rc = []; rl = []
        for pid in pids:
            obs, _ = self.covis.observations(pid); p = self.points[pid]
            for k, i in obs: oc.append(self.kf[k]['Ow']); dd.append(self.kf[k]['desc'][i])
            st.append(len(oc)); ref = p['ref_kf']
            rc.append(self.kf[ref]['Ow']); rl.append(int(self.kf[ref]['octave'][dict(obs)[ref]]))
        P = [self.points[p] for p in pids]
        nr, mn, mx = mappoint.UpdateNormalAndDepth(np.stack([p['xw'] for p in P]), st, np.stack(oc), np.stack(rc), rl, self.store.scale_factors, np.stack([p['normal'] for p in P]),
                                                   [p['min_dist'] for p in P], [p['max_dist'] for p in P], lib=self.lib)
        best, desc = mappoint.ComputeDistinctiveDescriptors(st, np.stack(dd), lib=self.lib)
        for n, p in enumerate(P):
            p['normal'] = nr[n].copy(); p['min_dist'] = mn[n]; p['max_dist'] = mx[n]; p['desc'] = desc[n].copy()

    # ---- the three steps
    def ProcessNewKeyFrame(self, kf, matches, new_stereo=None):
        """:128-168 for the keyframe kf = dict(id, keys_un, desc, uright, depth, feat_node, Tcw[, keys]).  matches: its mvpMapPoints from Tracking as point ids (-1 none).
        new_stereo: {keypoint index: (point id, xw)}, the points Tracking created together with the keyframe (Tracking.cc:1196-1245): they observe it already and go to
        the recent list when they stand in `matches`."""
        kid = int(kf['id']); ku = np.ascontiguousarray(kf['keys_un'])
        self.covis.add_keyframe(kid, ku['octave'].astype('i4'), kf['uright'], kf['depth'])
        self.store.add(kid, ku, kf['desc'], kf['uright'], kf['depth'], kf['feat_node'], kf['Tcw'], keys=kf.get('keys'))
        self.kf[kid] = dict(desc=np.ascontiguousarray(kf['desc'], np.uint8).reshape(-1, 32).copy(), octave=ku['octave'].astype('i4'), Ow=camera_centre(kf['Tcw']))
        created = sorted((new_stereo or {}).items())
        if created:
            for i, (pid, xw) in created: self.add_point(pid, xw, kid)
            self.covis.set_observations(kid, [i for i, _ in created], [pid for _, (pid, _) in created])
            self._post_steps([int(pid) for _, (pid, _) in created])
        idx = []; pts = []
        for i, pid in enumerate(matches):
            pid = int(pid)
            if pid < 0 or self.isBad(pid): continue
            if (kid, i) not in self.covis.observations(pid)[0]: idx.append(i); pts.append(pid)                   # !IsInKeyFrame: AddObservation and the two updates
            else: self.mlpRecentAddedMapPoints.append(pid)                                                       # only Tracking's new stereo points
        if idx:
            self.covis.set_observations(kid, idx, pts)
            self._post_steps(pts)
        self.covis.update_connections([kid])

    def MapPointCulling(self, kf_id):
        """:170-205"""
        th = 2 if self.mbMonocular else 3
        keep = []; bad = []
        for pid in self.mlpRecentAddedMapPoints:
            p = self.points[pid]; obs, nobs = self.covis.observations(pid)
            if not obs: continue                                                                                 # isBad()
            if np.float32(p['found']) / np.float32(p['visible']) < np.float32(0.25): bad.append(pid)               # GetFoundRatio() < 0.25f
            elif (int(kf_id) - int(p['first_kf'])) >= 2 and nobs <= th: bad.append(pid)
            elif (int(kf_id) - int(p['first_kf'])) >= 3: pass
            else: keep.append(pid)
        if bad: self.covis.set_points_bad(bad)                                                                   # SetBadFlag; the points are independent
        self.mlpRecentAddedMapPoints = keep
        return bad

    def CreateNewMapPoints(self, kf_id, stop_after=None, median_depth=None, first_new_id=None):
        """:207-452 through KeyFrameStore.create_new_map_points.  stop_after = j is the CheckNewKeyFrames() exit before neighbour j (:239-240; it is asked for j > 0
        only): the results of the first j neighbours, which later ones cannot influence.  median_depth: ComputeSceneMedianDepth(2) of each neighbour (monocular)."""
        kid = int(kf_id)
        nbs = self.covis.best_covisibles(kid, 20 if self.mbMonocular else 10)
        if stop_after is not None and nbs: nbs = nbs[:max(int(stop_after), 1)]
        rows = [self.covis.keyframe_points(kid)] + [self.covis.keyframe_points(k) for k in nbs]
        first = self.next_point_id if first_new_id is None else int(first_new_id)
        res = self.store.create_new_map_points(kid, nbs, rows, first, None if median_depth is None else np.asarray(median_depth, 'f4')[:len(nbs)])
        n = res['n_new']
        if n:
            self.covis.set_observations(kid, res['new_idx1'], np.arange(first, first + n))
            for kf2 in nbs:
                sel = np.nonzero(res['new_kf2'] == kf2)[0]
                if len(sel): self.covis.set_observations(kf2, res['new_idx2'][sel], first + sel)
            for k in range(n):
                self.add_point(first + k, res['x3d'][k], kid)
                p = self.points[first + k]
                p['desc'] = res['desc'][k].copy(); p['normal'] = res['normal'][k].copy(); p['min_dist'] = res['min_dist'][k]; p['max_dist'] = res['max_dist'][k]
                self.mlpRecentAddedMapPoints.append(first + k)
        return res
