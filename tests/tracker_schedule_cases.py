"""The schedule the tracker host issues (sg_slam_amd/csrc/sgx_tracker.cpp), read back through sgx_tracker_debug_sync_trace: six scenarios that between them reach every
stream / event edge of the host, and the comparison of two traces.  Shared by tests/test_tracker_schedule.py (emulator) and tests/test_tracker_schedule_gpu.py (device
build); tests/golden/tracker_sync_trace.json holds what the scenarios gave on the host as it was before its stages were split into functions.

A trace is a list of [step, op, stream, event]: `step` counts the step calls issued so far (1 = issued during or after the first step), the rest is the tap's triple.
Streams and events are numbered in order of first appearance, the host is stream -1; for a mark the last field is the mark's id."""
import ctypes as C
import json
import os
import numpy as np
from scenes import CAM
from sg_slam_amd import synth
from sg_slam_amd.tracker_native import TrackerNative

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FIXTURE = os.path.join(ROOT, 'tests', 'golden', 'tracker_sync_trace.json')
RECORD, WAIT, EV_SYNC, ST_SYNC, DEV_SYNC, MARK = range(6)
OPS = ('record', 'wait', 'event-sync', 'stream-sync', 'device-sync', 'mark')
M_DETECTOR, M_ORB, M_MASK, M_STEREO, M_MOTION, M_UNPROJECT, M_UPLOAD, M_GRAY, M_PACK = range(1, 10)
SCENARIOS = ('A', 'B', 'C', 'D', 'E', 'F')
W, H = 640, 480


class Run:
    """one tracker of one stream (S = 1) over synth.LayeredStream frames; every call is followed by a read of the trace"""

    def __init__(self, lib, xp, streams=(None, None), **kw):
        self.lib, self.xp, self.trace, self.steps = lib, xp, [], 0
        self.gen = synth.LayeredStream(seed=1234)
        self.tr = TrackerNative(lib, 1, CAM, **kw)
        self.tr.set_initial_pose(self.gen.Tcw(3)[None])
        self.s1, self.s2 = streams                  # caller streams: raw handles (the emulator takes any token)
        self.held = []
        self.drain()

    def drain(self):
        tap = self.lib.tap('sgx_tracker_debug_sync_trace'); n = C.c_int()
        self.lib.check(tap(self.tr.h, None, 0, C.byref(n)))
        buf = np.zeros(max(1, n.value), 'i4')
        self.lib.check(tap(self.tr.h, buf.ctypes.data_as(C.c_void_p), n.value, C.byref(n)))
        self.trace += [[self.steps] + [int(v) for v in buf[3 * k:3 * k + 3]] for k in range(n.value // 3)]

    def quiesce(self):
        """device build: nothing is in flight when the next call is issued (uploads run on torch's stream, the tracker's and the caller's streams are non-blocking, and
        scenario E changes the caller's stream between steps); the trace is what the host issues and does not depend on it"""
        if self.xp == 'torch':
            import torch
            torch.cuda.synchronize()

    def dev(self, a):
        if self.xp != 'torch':
            return a
        import torch
        d = torch.from_numpy(a.view(np.int16) if a.dtype == np.uint16 else a).cuda()
        self.quiesce()
        return d

    def frame(self):
        gray, depth = self.gen.frame(3 + self.steps)[:2]
        return gray[None], depth[None], np.repeat(gray[None, ..., None], 3, 3)

    def zeros(self, shape, dt):
        return self.dev(np.zeros(shape, dt))

    def step(self, with_bgr=False, stream=None):
        gray, depth, bgr = self.frame()
        args = (self.dev(gray), self.dev(depth), self.dev(bgr) if with_bgr else None)
        self.held.append(args)
        self.steps += 1
        self.tr.step(args[0], args[1], d_bgr=args[2], stream=stream if stream is not None else self.s1); self.drain()

    def step_host(self):
        slot = self.steps & 1
        hb, hd = self.tr.host_buffers(slot); self.drain()
        gray, depth, bgr = self.frame()
        hb[:, :, :W * 3] = bgr.reshape(1, H, W * 3); hd[...] = depth
        self.steps += 1; self.quiesce()
        self.tr.step_host(slot); self.drain()

    def pack(self, stream=None):
        rec = self.zeros((1, self.tr.rec_bytes), np.uint8); self.held.append(rec)
        self.tr.pack_records(rec, stream=stream if stream is not None else self.s1); self.drain()

    def snapshot_boxes(self):
        bx, bn = self.zeros((self.tr.max_boxes, 4), 'f4'), self.zeros(1, 'i4'); self.held.append((bx, bn))
        self.tr.snapshot_boxes(0, bx, bn); self.drain()

    def call(self, f, *a):
        r = f(*a); self.drain()
        return r

    def close(self):
        self.tr.synchronize(); self.tr.close()
        return self.trace


def _detector(lib):
    from test_tracker_native_gpu import _detector as make
    return make(lib, 1)


def _device_input(lib, xp, streams, detector, steps=5, **kw):
    """A, B: pack after steps 2 and 4 (the slot of step 2 is reused by step 5, which must wait for the pack), wait_inputs(1) after step 3, read at the end"""
    r = Run(lib, xp, streams, detector=_detector(lib) if detector else None, **kw)
    for t in range(1, steps + 1):
        r.step(with_bgr=detector)
        if detector: r.snapshot_boxes()
        if t in (2, 4): r.pack()
        if t == 3: r.call(r.tr.wait_inputs, 1)
    r.call(r.tr.read)
    return r.close()


def scenario(lib, xp, name, streams=(None, None)):
    """the trace of scenario `name` on `lib`; streams: two distinct caller-stream handles (only E uses the second)"""
    if name == 'A':
        return _device_input(lib, xp, streams, False)
    if name == 'B':
        return _device_input(lib, xp, streams, True)
    if name == 'C':                                 # host input with a detector: the upload stream waits for both readers of the staging slot
        r = Run(lib, xp, streams, detector=_detector(lib))
        for _ in range(5): r.step_host()
        r.call(r.tr.host_buffers, 0); r.call(r.tr.synchronize)
        return r.close()
    if name == 'D':                                 # ev_det_read without the mask's detector wait
        r = Run(lib, xp, streams, detector=_detector(lib), dynamic_mask=False)
        for _ in range(4): r.step(with_bgr=True)
        return r.close()
    if name == 'E':                                 # non-pipelined: the pack on another stream waits for ev_step
        r = Run(lib, xp, streams, pipelined=False)
        for _ in range(3): r.step()
        r.pack(stream=r.s2)
        for _ in range(3): r.step_host()
        return r.close()
    if name == 'F':
        from test_undistort_emu import load
        r = Run(lib, xp, streams, dist=load('TUM1')['dist'])
        for _ in range(3): r.step()
        return r.close()
    raise KeyError(name)


def fixture():
    with open(FIXTURE) as f:
        return json.load(f)['scenarios']


def _show(e):
    if e is None:
        return 'nothing (the trace ends)'
    step, op, st, ev = e
    what = 'mark %d' % ev if op == MARK else OPS[op] + ('' if ev < 0 else ' event %d' % ev)
    return 'step %d: %s on %s' % (step, what, 'the host' if st < 0 else 'stream %d' % st)


def _first_difference(a, b, what):
    for k in range(max(len(a), len(b))):
        x = a[k] if k < len(a) else None; y = b[k] if k < len(b) else None
        if x is None or y is None or x[1:] != y[1:]:
            return '%s, entry %d: got %s, expected %s' % (what, k, _show(x), _show(y))
    return None


def difference(got, exp):
    """None when the two traces issue the same schedule, else a description of the first entry that differs.  Judged on the two projections HIP's semantics make
    meaningful: the subsequence of every stream (the host included: the three kinds of synchronisation), and for every event the global order of the records, waits
    and synchronisations that name it (a wait binds to the latest record at the time of the call)."""
    def of_stream(tr, s):
        return [e for e in tr if (e[2] == s if s >= 0 else e[1] in (EV_SYNC, ST_SYNC, DEV_SYNC))]
    def of_event(tr, v):
        return [e for e in tr if e[1] in (RECORD, WAIT, EV_SYNC) and e[3] == v]
    streams = sorted({e[2] for e in got + exp})
    events = sorted({e[3] for e in got + exp if e[1] in (RECORD, WAIT, EV_SYNC)})
    for s in streams:
        d = _first_difference(of_stream(got, s), of_stream(exp, s), 'the host' if s < 0 else 'stream %d' % s)
        if d: return d
    for v in events:
        d = _first_difference(of_event(got, v), of_event(exp, v), 'event %d' % v)
        if d: return d
    return None
