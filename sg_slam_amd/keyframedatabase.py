"""KeyFrameDatabase — Python mirror of src/sg-slam/src/KeyFrameDatabase.cc over the C ABI (sgx_kfdb_*).

The database lives on the device: every keyframe's BowVector, its add() order, its best-covisibility list and its mRelocScore.  DetectRelocalizationCandidates
(:199-309, Tracking::Relocalization) and DetectLoopCandidates (:76-197, LoopClosing::DetectLoop) return keyframe ids in the reference's order; detect_batch runs Q
queries as one launch sequence, for one lost frame or for hundreds.  A BowVector is the pair (ids ascending, weights) ORBVocabulary.transform returns."""
import ctypes as C
import numpy as np
from .capi import _vp, KfdbReport, KFDB_REPORT_DTYPE

RELOCALIZATION, LOOP_CLOSING = 0, 1


def _bow(v):
    return np.ascontiguousarray(v[0], 'i4').reshape(-1), np.ascontiguousarray(v[1], 'f8').reshape(-1)


def _report(r):
    return {k: getattr(r, k) for k, _ in KfdbReport._fields_}


class KeyFrameDatabase:
    def __init__(self, voc, max_keyframes=4096, max_bow_entries=None, max_query_words=0, max_queries=64, lib=None):
        self.lib = lib or voc.lib
        self.max_keyframes = int(max_keyframes); self.max_queries = int(max_queries)
        self.max_query_words = int(max_query_words) or 2048
        self.h = C.c_void_p()
        self.lib.check(self.lib.dll.sgx_kfdb_create(voc.h, self.max_keyframes, int(max_bow_entries or 1024 * self.max_keyframes), int(max_query_words), self.max_queries,
                                                    C.byref(self.h)), 'sgx_kfdb_create')
        self._on_host = 'EMULATOR' in self.lib.version()          # the emulator's "device" memory is host memory
        self.last_report = None

    # ---- the container (:40-73)
    def add(self, kf_id, bow):
        i, w = _bow(bow)
        self.lib.check(self.lib.dll.sgx_kfdb_add(self.h, int(kf_id), len(i), _vp(i), _vp(w)), 'sgx_kfdb_add')

    def erase(self, kf_id):
        self.lib.check(self.lib.dll.sgx_kfdb_erase(self.h, int(kf_id)), 'sgx_kfdb_erase')

    def clear(self):
        self.lib.check(self.lib.dll.sgx_kfdb_clear(self.h), 'sgx_kfdb_clear')

    def size(self):
        return int(self.lib.dll.sgx_kfdb_size(self.h))

    def set_covisibility(self, kf_id, neighbour_ids):
        """what pKF->GetBestCovisibilityKeyFrames(10) returns for keyframe kf_id, in its order"""
        n = np.ascontiguousarray(neighbour_ids, 'i4').reshape(-1)
        self.lib.check(self.lib.dll.sgx_kfdb_set_covisibility(self.h, int(kf_id), len(n), _vp(n)), 'sgx_kfdb_set_covisibility')

    def slots(self):
        """keyframe id per slot (-1 = free): the order of the words / scores arrays of detect_batch"""
        ids = np.full(self.max_keyframes, -1, 'i4'); n = C.c_int32()
        self.lib.check(self.lib.dll.sgx_kfdb_slots(self.h, _vp(ids), C.byref(n)), 'sgx_kfdb_slots')
        return ids[:n.value].copy()

    # ---- the queries
    def DetectRelocalizationCandidates(self, bow):
        """vpRelocCandidates as keyframe ids; the report of the call is left in self.last_report"""
        i, w = _bow(bow)
        cand = np.zeros(max(self.size(), 1), 'i4'); n = C.c_int32(); rep = KfdbReport()
        self.lib.check(self.lib.dll.sgx_kfdb_detect_relocalization_candidates(self.h, len(i), _vp(i), _vp(w), _vp(cand), C.byref(n), C.byref(rep)),
                       'sgx_kfdb_detect_relocalization_candidates')
        self.last_report = _report(rep)
        return cand[:n.value].copy()

    def DetectLoopCandidates(self, bow, connected, minScore):
        """vpLoopCandidates as keyframe ids; connected = pKF->GetConnectedKeyFrames() as ids"""
        i, w = _bow(bow); c = np.ascontiguousarray(list(connected), 'i4').reshape(-1)
        cand = np.zeros(max(self.size(), 1), 'i4'); n = C.c_int32(); rep = KfdbReport()
        self.lib.check(self.lib.dll.sgx_kfdb_detect_loop_candidates(self.h, len(i), _vp(i), _vp(w), len(c), _vp(c), float(minScore), _vp(cand), C.byref(n), C.byref(rep)),
                       'sgx_kfdb_detect_loop_candidates')
        self.last_report = _report(rep)
        return cand[:n.value].copy()

    def min_score(self, bow, kf_ids):
        """the minScore of LoopClosing::DetectLoop (LoopClosing.cc:126-138) over the listed keyframes (those that are not isBad())"""
        i, w = _bow(bow); k = np.ascontiguousarray(list(kf_ids), 'i4').reshape(-1)
        m = C.c_float()
        self.lib.check(self.lib.dll.sgx_kfdb_min_score(self.h, len(i), _vp(i), _vp(w), len(k), _vp(k), C.byref(m)), 'sgx_kfdb_min_score')
        return np.float32(m.value)

    # ---- batches
    def _dev(self, a):
        a = np.ascontiguousarray(a)
        if self._on_host: return a.copy()
        import torch
        return torch.from_numpy(a).cuda()

    def _host(self, x):
        return x if self._on_host else x.cpu().numpy()

    def _stream(self, stream):
        if self._on_host: return None
        import torch
        s = stream if stream is not None else torch.cuda.current_stream()
        return C.c_void_p(s.cuda_stream)

    def detect_batch_dev(self, mode, Q, ids_dev, weights_dev, pitch, counts_dev, connected=None, minScore=None, want_members=False, stream=None):
        """Q queries resident on the device (rows of pitch `pitch` and a count per row: what ORBVocabulary.bow_batch_dev writes), asynchronous on `stream` (default: the
        current torch stream).  connected = one id list per query, minScore = one per query (loop closing).  Returns device arrays (cand Q x max_keyframes, n_cand, report
        records, words, scores); synchronise the stream before reading them."""
        conn_off = conn_ids = ms = None
        if mode == LOOP_CLOSING:
            off = np.zeros(Q + 1, 'i4'); off[1:] = np.cumsum([len(c) for c in connected])
            conn_off = self._dev(off); conn_ids = self._dev(np.concatenate([np.asarray(list(c), 'i4').reshape(-1) for c in connected] + [np.zeros(1, 'i4')]))
            ms = self._dev(np.asarray(minScore, 'f4').reshape(Q))
        N = self.max_keyframes
        cand = self._dev(np.zeros((Q, N), 'i4')); ncand = self._dev(np.zeros(Q, 'i4')); rep = self._dev(np.zeros(Q * KFDB_REPORT_DTYPE.itemsize, 'u1'))
        words = self._dev(np.zeros((Q, N), 'i4')) if want_members else None
        scores = self._dev(np.zeros((Q, N), 'f4')) if want_members else None
        self._keep = (ids_dev, weights_dev, counts_dev, conn_off, conn_ids, ms)      # alive until the launch sequence has read them
        self.lib.check(self.lib.dll.sgx_kfdb_detect_batch_dev(self.h, int(mode), int(Q), _vp(ids_dev), _vp(weights_dev), int(pitch), _vp(counts_dev), _vp(conn_off), _vp(conn_ids),
                                                              _vp(ms), _vp(cand), _vp(ncand), _vp(rep), _vp(words), _vp(scores), self._stream(stream)),
                       'sgx_kfdb_detect_batch_dev')
        return cand, ncand, rep, words, scores

    def detect_batch(self, bows, mode=RELOCALIZATION, connected=None, minScore=None, want_members=False, stream=None):
        """Q BowVectors from the host through detect_batch_dev, read back: (list of candidate id arrays, report records[, words Q x slots, scores Q x slots])"""
        Q = len(bows)
        pitch = max([len(b[0]) for b in bows] + [1])
        ids = np.zeros((Q, pitch), 'i4'); w = np.zeros((Q, pitch), 'f8'); cnt = np.zeros(Q, 'i4')
        for q, b in enumerate(bows):
            i, ww = _bow(b); ids[q, :len(i)] = i; w[q, :len(i)] = ww; cnt[q] = len(i)
        out = self.detect_batch_dev(mode, Q, self._dev(ids), self._dev(w), pitch, self._dev(cnt), connected, minScore, want_members, stream)
        if not self._on_host:
            import torch
            (stream if stream is not None else torch.cuda.current_stream()).synchronize()
        cand, ncand, rep = self._host(out[0]), self._host(out[1]), self._host(out[2]).view(KFDB_REPORT_DTYPE)
        res = [cand[q, :ncand[q]].copy() for q in range(Q)]
        if not want_members: return res, rep
        ns = len(self.slots())
        return res, rep, self._host(out[3])[:, :ns].copy(), self._host(out[4])[:, :ns].copy()

    def close(self):
        if self.h: self.lib.dll.sgx_kfdb_destroy(self.h); self.h = C.c_void_p()

    def __del__(self):
        try: self.close()
        except Exception: pass
