"""LoopClosing — the loop-closing thread of the reference (src/sg-slam/src/LoopClosing.cc) over a CovisibilityGraph, a KeyFrameDatabase and a vocabulary:
DetectLoop (:103-229), CorrectLoop (:402-585, through CovisibilityGraph.correct_loop) and RunGlobalBundleAdjustment (:645-749).  ComputeSim3's orchestration (:231-400)
stays the caller's: its steps are SearchByBoW, Sim3Solver, SearchBySim3, OptimizeSim3 and SearchByProjection of this package.  SetNotErase / SetErase and
InformNewBigChange are the caller's bookkeeping."""
import numpy as np
from .optimizer import Optimizer


class LoopClosing:
    def __init__(self, covis, kfdb, voc=None, bFixScale=True, consistency_th=3, max_groups=None):
        self.covis = covis; self.kfdb = kfdb; self.voc = voc; self.mbFixScale = bool(bFixScale)
        self.mnCovisibilityConsistencyTh = int(consistency_th)
        self.mLastLoopKFid = 0
        self.mvpEnoughConsistentCandidates = []
        self.last = None                                                      # what the last DetectLoop saw: minScore, candidates, the consistency report
        if max_groups is not None: covis.consistency_reserve(max_groups)

    def DetectLoop(self, kf_id, bow):
        """:103-229 for mpCurrentKF = kf_id with its BowVector.  True when mvpEnoughConsistentCandidates is not empty.  The keyframe enters the database on every exit."""
        kf_id = int(kf_id)
        try:
            self.mvpEnoughConsistentCandidates = []
            if kf_id < self.mLastLoopKFid + 10:                               # :114
                self.last = dict(early=True); return False
            listed = [k for k in self.covis.ordered(kf_id)[0]]                # GetVectorCovisibleKeyFrames(); min_score passes over what the database does not hold
            minScore = self.kfdb.min_score(bow, listed)                       # :126-138, the one synchronous hop
            conn = self.covis.connected_batch([kf_id])
            assert conn['status'][0] == 0
            cands = [int(c) for c in self.kfdb.DetectLoopCandidates(bow, conn['rows'][0], minScore)]      # :141
            c = self.covis.consistency(cands, self.mnCovisibilityConsistencyTh)      # :144-211; no candidate clears the groups (:147)
            assert c['status'] == 0, c['status']
            self.last = dict(early=False, minScore=float(minScore), candidates=cands, report=c['report'])
            self.mvpEnoughConsistentCandidates = list(c['enough'])
            return bool(self.mvpEnoughConsistentCandidates)
        finally:
            self.kfdb.add(kf_id, bow)                                         # :116, :146, :215

    def CorrectLoop(self, cur, loop, Scw, Tcw, xw, **kw):
        """:402-585 through CovisibilityGraph.correct_loop; mLastLoopKFid = the current keyframe (:584)"""
        out = self.covis.correct_loop(cur, loop, Scw, Tcw, xw, fix_scale=self.mbFixScale, **kw)
        self.mLastLoopKFid = int(cur)
        return out

    def RunGlobalBundleAdjustment(self, nLoopKF, keyframes, points, inv_level_sigma2, cam, origins=(0,), point_ref=None, nIterations=10, new_Tcw=None, new_xw=None, while_running=None):
        """:645-749: global_ba_graph -> flatten_ba_problem -> the solver with nLoopKF -> ApplyGlobalBundleAdjustment.  keyframes / points as flatten_ba_problem takes
        them.  new_Tcw / new_xw (optional): poses by id and positions by point id as they stand when the update runs, for what was created while the solver ran.
        while_running (optional): called once the solver has returned and before the update, where LocalMapping's work during the BA shows (it may add keyframes and fill
        new_Tcw / new_xw / point_ref)."""
        graph = self.covis.global_ba_graph()
        problem = Optimizer.flatten_ba_problem(graph, keyframes, points, inv_level_sigma2)
        stats = Optimizer.BundleAdjustment(problem, cam, nIterations, None, int(nLoopKF), False, lib=self.covis.lib)
        if while_running is not None: while_running()
        out = Optimizer.ApplyGlobalBundleAdjustment(problem, graph, self.covis, list(origins), point_ref, Tcw=new_Tcw, xw=new_xw)
        out['stats'] = stats; out['problem'] = problem; out['graph'] = graph
        return out
