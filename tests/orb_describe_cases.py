"""Shared by test_orb_describe_emu.py / test_orb_describe_gpu.py: orientation and descriptors computed AFTER the erase step of the dynamic mask
(sgx_orb_detect_batch_dev -> sgx_frame_compact_keys_src_batch_dev -> sgx_orb_describe_batch_dev) against the order the reference has
(sgx_orb_extract_batch_dev -> sgx_frame_compact_keys_batch_dev): same count, same keypoint bytes (angle included), same descriptor rows, nothing written past the count."""
import numpy as np
from scenes import CAM
from sg_slam_amd import frame as fr, synth
from sg_slam_amd.capi import KP_DTYPE
from sg_slam_amd.orb import ORBextractor

B, W, H, NFEAT = 8, 640, 480, 1000
FLAT = 5                      # index of the flat frame (no corner anywhere: no raw keypoint)
FILL = 0xA5                   # what the output buffers hold before a call: bytes that stay prove "not written"
CASES = ('all', 'none', 'half', 'rect', 'one_coarsest', 'mod4', 'restore')


def frames():
    """eight 640 x 480 frames of the stream fixtures (two-layer parallax stream), one of them replaced by a flat image"""
    gen = synth.LayeredStream(seed=1234)
    g = np.stack([gen.frame(3 + 7 * i)[0] for i in range(B)]).astype(np.uint8)
    g[FLAT] = 128
    return np.ascontiguousarray(g)


class Backend:
    """numpy arrays under the emulator, torch CUDA tensors on the GPU"""
    def __init__(self, torch_dev):
        self.t = torch_dev

    def dev(self, a):
        if not self.t: return np.ascontiguousarray(a).copy()
        import torch
        return torch.from_numpy(np.ascontiguousarray(a).view(np.uint8).reshape(-1)).cuda()

    def host(self, a, dtype, shape):
        if self.t:
            import torch
            torch.cuda.synchronize()
            a = a.cpu().numpy()
        return np.asarray(a).reshape(-1).view(np.uint8).view(dtype).reshape(shape).copy()

    def filled(self, nbytes):
        return self.dev(np.full(nbytes, FILL, np.uint8))


class Extracted:
    """the reference side, computed once per library: one-shot extraction of the batch, and the detect call that every case then describes from"""
    def __init__(self, lib, torch_dev):
        self.lib, self.be = lib, Backend(torch_dev)
        be = self.be
        self.ex = ORBextractor(nfeatures=NFEAT, width=W, height=H, max_batch=B, lib=lib)
        self.cap = cap = self.ex.capacity
        self.gray = be.dev(frames())
        self.d_rkeys, self.d_rdesc, self.d_rn = be.filled(B * cap * 28), be.filled(B * cap * 32), be.dev(np.zeros(B, 'i4'))
        self.ex.extract_batch_dev(self.gray, W, B, self.d_rkeys, self.d_rdesc, self.d_rn)
        self.ex.last_status()
        self.rkeys = be.host(self.d_rkeys, np.uint8, (B, cap, 28)).view(KP_DTYPE).reshape(B, cap)
        self.rn = be.host(self.d_rn, 'i4', (B,))
        self.d_dkeys, self.d_dn = be.filled(B * cap * 28), be.dev(np.zeros(B, 'i4'))
        self.ex.detect_batch_dev(self.gray, W, B, self.d_dkeys, self.d_dn)          # last extraction on the handle: its pyramid and selection lists serve every describe below
        self.ex.last_status()
        self.dkeys = be.host(self.d_dkeys, np.uint8, (B, cap, 28)).view(KP_DTYPE).reshape(B, cap)
        self.dn = be.host(self.d_dn, 'i4', (B,))

    def close(self):
        self.ex.close()


def check_detect(E):
    """detect = the one-shot records with the angle left open (-1), same counts; rows past the count untouched"""
    assert (E.dn == E.rn).all() and E.rn[FLAT] == 0 and (np.delete(E.rn, FLAT) > 500).all()
    for f in range(B):
        n = E.rn[f]
        for k in ('x', 'y', 'size', 'response', 'octave', 'class_id'):
            assert (E.dkeys[f, :n][k].view(np.uint32) == E.rkeys[f, :n][k].view(np.uint32)).all(), (f, k)
        assert (E.dkeys[f, :n]['angle'] == -1.0).all()
        assert (E.dkeys[f, n:].view(np.uint8) == FILL).all()


def keep_mask(E, case):
    """keep flags (B, cap) u8 and have-dynamic flags (B,) of one case"""
    cap, rn, k = E.cap, E.rn, E.rkeys
    rng = np.random.RandomState(7)
    keep = np.zeros((B, cap), np.uint8); have = np.zeros(B, 'i4')
    for f in range(B):
        n = rn[f]
        if case == 'all': keep[f, :n] = 1
        elif case == 'none': pass                                                           # no dynamic object: nothing is restored, n = 0
        elif case == 'half': keep[f, :n] = rng.randint(0, 2, n); have[f] = 1
        elif case == 'rect': keep[f, :n] = ~((k[f, :n]['x'] > 213) & (k[f, :n]['x'] < 427)); have[f] = 1      # an erased rectangle over the middle third of the image
        elif case == 'one_coarsest':
            top = np.nonzero(k[f, :n]['octave'] == k[f, :n]['octave'].max())[0] if n else []
            if len(top): keep[f, top[len(top) // 2]] = 1
        elif case == 'mod4':                                                                # 1, 2, 3 (mod 4) survivors, few and many
            m = min(n, [1, 2, 3, 101, 202, 303, 5, 6][f])
            if m: keep[f, rng.permutation(n)[:m]] = 1
        elif case == 'restore':                                                             # fewer than 0.1 * nFeatures survive beside a dynamic object: everything comes back
            keep[f, :n] = rng.rand(n) < 0.05; have[f] = 1
    return keep, have


def run_case(E, case):
    be, cap, lib = E.be, E.cap, E.lib
    keep, have = keep_mask(E, case)
    d_keep, d_have = be.dev(keep), be.dev(have)
    # the order the reference has: everything described, the erase step moves keypoints and descriptor rows
    ko, do, no = be.filled(B * cap * 28), be.filled(B * cap * 32), be.dev(np.zeros(B, 'i4'))
    fr.compact_keys_batch(lib, B, cap, E.d_rkeys, E.d_rdesc, E.d_rn, d_keep, d_have, NFEAT, ko, do, no)
    # describe after the erase step
    kn, dn, nn, src = be.filled(B * cap * 28), be.filled(B * cap * 32), be.dev(np.zeros(B, 'i4')), be.filled(B * cap * 4)
    fr.compact_keys_src_batch(lib, B, cap, E.d_dkeys, E.d_dn, d_keep, d_have, NFEAT, kn, src, nn)
    E.ex.describe_batch_dev(E.gray, W, B, src, nn, kn, dn)
    E.ex.last_status()
    ko, kn = be.host(ko, np.uint8, (B, cap, 28)), be.host(kn, np.uint8, (B, cap, 28))
    do, dn = be.host(do, np.uint8, (B, cap, 32)), be.host(dn, np.uint8, (B, cap, 32))
    no, nn, src = be.host(no, 'i4', (B,)), be.host(nn, 'i4', (B,)), be.host(src, 'i4', (B, cap))
    assert (nn == no).all(), (case, nn, no)
    surv = keep.sum(1)
    if case == 'restore': assert (nn == E.rn).all() and (surv[np.arange(B) != FLAT] > 0).all() and (surv < 100).all()
    elif case == 'none': assert (nn == 0).all()
    elif case == 'one_coarsest': assert (np.delete(nn, FLAT) == 1).all() and E.rkeys[0, src[0, 0]]['octave'] == 7
    elif case == 'mod4': assert sorted(set(int(v) % 4 for v in np.delete(nn, FLAT))) == [1, 2, 3]
    else: assert (nn == surv).all()
    if case in ('half', 'rect'): assert (np.delete(nn, FLAT) >= 100).all() and (np.delete(E.rn - nn, FLAT) > 100).all()      # a real erasure, above the restore rule
    assert nn[FLAT] == 0
    for f in range(B):
        n = nn[f]
        want = np.arange(n) if case == 'restore' else np.nonzero(keep[f])[0]
        assert (src[f, :n] == want).all(), (case, f)
        assert (kn[f, :n] == ko[f, :n]).all(), (case, f)                  # every byte of every keypoint record, angle included
        assert (dn[f, :n] == do[f, :n]).all(), (case, f)                  # every descriptor row
        assert (kn[f, n:] == FILL).all() and (dn[f, n:] == FILL).all(), (case, f)      # nothing written past the count
        if n: assert (kn[f, :n].copy().view(KP_DTYPE)['angle'] >= 0).all()


def boxes_for(S, MB):
    """synthetic person rectangles: one box over the middle third of the image in every stream, plus a small second one in stream 0"""
    boxes = np.zeros((S, MB, 4), 'f4'); nb = np.ones(S, 'i4'); have = np.ones(S, 'i4')
    boxes[:, 0] = (213, 60, 214, 360)
    boxes[0, 1] = (20, 300, 120, 150); nb[0] = 2
    return boxes, nb, have


def run_tracker_orders(lib, pipelined, torch_dev, S=2, steps=4):
    """four steps with synthetic person boxes, once describing after the mask and once before it (tap switch): read() and the packed frame records are identical"""
    from sg_slam_amd.tracker_native import TrackerNative
    be = Backend(torch_dev)
    gen = synth.LayeredStream(seed=1234); offs = [3, 57][:S]
    T0 = np.stack([gen.Tcw(o) for o in offs])
    trk = [TrackerNative(lib, S, CAM, dynamic_mask=True, pipelined=pipelined, describe_early=e) for e in (False, True)]
    erased = 0
    for t in trk:
        t.set_initial_pose(T0)
        t.debug_set_boxes(*boxes_for(S, t.max_boxes))
    held = []
    for s in range(steps):
        f = [gen.frame(o + s) for o in offs]
        gray, depth = be.dev(np.stack([x[0] for x in f])), be.dev(np.stack([x[1] for x in f]))
        held.append((gray, depth))
        out = []
        for t in trk:
            t.step(gray, depth)
            r = t.read()
            rec = be.dev(np.zeros((S, t.rec_bytes), np.uint8))
            if torch_dev:
                import torch
                t.pack_records(rec, stream=torch.cuda.current_stream().cuda_stream)
            else:
                t.pack_records(rec)
            t.last_status()
            out.append((r, be.host(rec, np.uint8, (S, t.rec_bytes))))
        (ra, reca), (rb, recb) = out
        for k in ra:
            assert (ra[k].view(np.uint32) == rb[k].view(np.uint32)).all(), (s, k)
        assert (reca == recb).all(), s
        if s > 0: erased += int((ra['nkeys_raw'] - ra['nkeys']).sum())
    assert erased > 50 * (steps - 1)          # the boxes did erase keypoints: the two orders did different work
    for t in trk: t.close()
