"""Lens distortion (Frame::UndistortKeyPoints, Frame::ComputeImageBounds, src/sg-slam/src/Frame.cc:654-714) on the kernel-logic emulator: the point
undistortion, the bounds and the fused undistort + stereo-from-RGBD kernel against the float64 restatement (tests/undistort_ref.py), bit for bit; the
settings loader on the reference's five settings files; the tracking chain with a distorted camera stage by stage against the oracle, and the C++ host
against the Python orchestration.

Fixtures: tests/golden/settings/*.yaml are the camera and ORB sections of the reference's five settings files (src/sg-slam/Examples/TUM1.yaml, TUM2.yaml,
TUM3.yaml, Bonn.yaml, astra_pro_camera.yaml; viewer / mapping keys and comments dropped).  Settings only; only TUM3 has k1 = 0."""
import ctypes as C
import os
import numpy as np
import pytest
import undistort_ref as R
from scenes import CAM
from sg_slam_amd import frame, settings, synth
from sg_slam_amd.capi import KP_DTYPE
from sg_slam_amd.tracker import TrackerBatch
from sg_slam_amd.tracker_native import TrackerNative

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SETTINGS = ('TUM1', 'TUM2', 'TUM3', 'Bonn', 'astra_pro_camera')
DISTORTED = ('TUM1', 'TUM2', 'Bonn', 'astra_pro_camera')


def load(name):
    return settings.load(os.path.join(ROOT, 'tests', 'golden', 'settings', name + '.yaml'))


def coeffs(name, ndist):
    """the settings file's coefficients as an ndist-vector (8: k4..k6 made up so the rational terms are exercised)"""
    d = np.zeros(ndist, 'f4'); s = load(name)['dist']; m = min(ndist, len(s)); d[:m] = s[:m]
    if ndist == 8:
        d[5:] = (0.012, -0.031, 0.007)
    return d


def random_points(seed, n=20000):
    rng = np.random.RandomState(seed)
    return np.stack([rng.uniform(-160, 800, n), rng.uniform(-120, 600, n)], 1).astype('f4')     # across and beyond the 640 x 480 image


def check_undistort_points(lib):
    for si, name in enumerate(DISTORTED):
        cam = load(name)['cam']
        for ndist in (4, 5, 8):
            pts = random_points(100 * si + ndist)
            pts[:4] = ((0, 0), (640, 0), (0, 480), (640, 480))
            got = frame.undistort_points(lib, pts, cam, coeffs(name, ndist))
            exp = R.undistort_points(pts, cam, coeffs(name, ndist))
            assert (got.view(np.uint32) == exp.view(np.uint32)).all(), (name, ndist, int((got != exp).sum()))


def check_image_bounds(lib):
    for name in SETTINGS:
        s = load(name)
        got = frame.image_bounds(lib, 640, 480, s['cam'], s['dist'])
        exp = R.image_bounds(640, 480, s['cam'], s['dist'])
        assert [np.float32(got[k]) for k in ('min_x', 'max_x', 'min_y', 'max_y')] == list(exp), name
        if name == 'TUM3':
            assert (got['min_x'], got['max_x'], got['min_y'], got['max_y']) == (0.0, 640.0, 0.0, 480.0)


def random_keys(rng, S, cap, n):
    keys = np.zeros((S, cap), KP_DTYPE)
    keys['x'] = rng.uniform(0, 639.99, (S, cap)); keys['y'] = rng.uniform(0, 479.99, (S, cap))
    keys['size'] = rng.randint(31, 130, (S, cap)); keys['angle'] = rng.uniform(0, 360, (S, cap)); keys['response'] = rng.uniform(0, 90, (S, cap))
    keys['octave'] = rng.randint(0, 8, (S, cap)); keys['class_id'] = -1
    return keys


def check_undistort_stereo_kernel(lib, oracle, to_dev=lambda a: a, to_host=lambda a: a):
    """k_undistort_stereo_rgbd: keys_un, uright, zdepth (padding rows too) against the restatement + the oracle's ComputeStereoFromRGBD, and the existing kernel"""
    rng = np.random.RandomState(3)
    S, cap = 3, 700
    n = np.array([650, 0, 700], 'i4')
    keys = random_keys(rng, S, cap, n)
    gen = synth.LayeredStream(seed=1234)
    depth = np.stack([gen.frame(t)[1] for t in range(S)])
    depth[0, 100:140, 200:260] = 0                                              # holes: zdepth / uright = -1
    keys[0, :40]['x'] = rng.uniform(200, 259, 40); keys[0, :40]['y'] = rng.uniform(100, 139, 40)
    for name in DISTORTED + ('TUM3',):
        s = load(name); cam = dict(s['cam'])
        out = [to_dev(np.zeros((S, cap, 28), np.uint8)), to_dev(np.zeros((S, cap), 'f4')), to_dev(np.zeros((S, cap), 'f4'))]
        ref = [to_dev(np.zeros((S, cap), 'f4')), to_dev(np.zeros((S, cap), 'f4'))]
        dk, dn, dd = to_dev(keys.view(np.uint8).reshape(S, cap, 28)), to_dev(n), to_dev(depth)
        frame.undistort_stereo_rgbd_batch_dev(lib, S, cap, dk, dn, s['dist'], cam, dd, 640, 480, *out)
        frame.stereo_from_rgbd_batch(lib, S, cap, dk, dn, dd, 640, 480, cam['depth_factor'], cam['bf'], *ref)
        kun, ur, z = (to_host(a) for a in out); rur, rz = (to_host(a) for a in ref)
        kun = kun.reshape(S, cap * 28).view(KP_DTYPE)
        assert (z.view(np.uint32) == rz.view(np.uint32)).all(), name                # depth at the distorted pixel, padding -1
        for f in range(S):
            m = n[f]
            exp = R.undistort_keypoints(keys[f, :m], cam, s['dist'])
            assert (kun[f, :m].view(np.uint8) == exp.view(np.uint8)).all(), (name, f)
            assert (kun[f, m:].view(np.uint8) == keys[f, m:].view(np.uint8)).all(), (name, f)      # rows n..cap-1: copies
            for fld in ('size', 'angle', 'response', 'octave', 'class_id'):
                assert (kun[f][fld].view(np.uint32) == keys[f][fld].view(np.uint32)).all()
            eur, ez = oracle.compute_stereo_from_rgbd(keys[f, :m], depth[f], cam['bf'], cam['depth_factor'])
            assert (z[f, :m].view(np.uint32) == ez.view(np.uint32)).all(), (name, f)
            with np.errstate(divide='ignore'):
                exp_ur = np.where(ez > 0, (exp['x'] - np.float32(cam['bf']) / ez).astype('f4'), np.float32(-1))
            assert (ur[f, :m].view(np.uint32) == exp_ur.view(np.uint32)).all(), (name, f)
            assert (ur[f, m:] == -1).all() and (z[f, m:] == -1).all()
            if name == 'TUM3':
                assert (ur.view(np.uint32) == rur.view(np.uint32)).all()
        assert (z > 0).sum() > 500 and (z[0, :40] == -1).any()


# ---------------------------------------------------------------------------------------------------------- CPU tier
def test_settings_loader():
    counts = {name: len(load(name)['dist']) for name in SETTINGS}
    assert counts == dict(TUM1=5, TUM2=5, TUM3=4, Bonn=4, astra_pro_camera=4)
    t3 = load('TUM3')
    assert (t3['dist'] == 0).all() and t3['cam']['fx'] == np.float32(535.4) and t3['cam']['depth_factor'] == 5000.0
    t1 = load('TUM1')
    assert t1['dist'][0] == np.float32(0.262383) and t1['dist'][4] == np.float32(1.163314) and t1['cam']['cy'] == np.float32(255.313989)
    assert load('TUM2')['cam']['depth_factor'] == 5208.0 and load('astra_pro_camera')['cam']['depth_factor'] == 1.0
    assert t1['orb'] == dict(nfeatures=1000, scale_factor=np.float32(1.2), nlevels=8, ini_th_fast=20, min_th_fast=7) and t1['rgb'] == 1


def test_undistort_points_bit_exact_emu(emu):
    check_undistort_points(emu)


def test_undistort_points_edge_cases_emu(emu):
    cam = load('TUM1')['cam']
    # the icdist < 0 guard: a denominator that turns negative far from the centre returns the normalised input unchanged (u, v in, u, v out)
    d = np.array([-0.9, 0.0, 0.0, 0.0], 'f4')
    pts = np.array([[1500, 1300], [-900, -700], [320, 240], [639, 479]], 'f4')
    got = frame.undistort_points(emu, pts, cam, d); exp = R.undistort_points(pts, cam, d)
    assert (got.view(np.uint32) == exp.view(np.uint32)).all()
    fx, fy, cx, cy = (np.float64(np.float32(cam[c])) for c in ('fx', 'fy', 'cx', 'cy'))
    back = np.stack([(fx * ((pts[:2, 0].astype('f8') - cx) * (1. / fx)) + cx), (fy * ((pts[:2, 1].astype('f8') - cy) * (1. / fy)) + cy)], 1).astype('f4')
    assert (got[:2] == back).all() and np.abs(got[:2] - pts[:2]).max() < 1e-3
    # k1 == 0 with p1 / p2 / k3 != 0: cv::undistortPoints iterates ...
    d0 = np.array([0.0, 0.0, 0.004, -0.003, 0.2], 'f4')
    pts = random_points(7, 1000)
    got = frame.undistort_points(emu, pts, cam, d0)
    assert (got.view(np.uint32) == R.undistort_points(pts, cam, d0).view(np.uint32)).all() and (got != pts).any()
    # ... but Frame::UndistortKeyPoints / ComputeImageBounds stop at k1 == 0 (Frame.cc:656-660, :707-713): keys_un is a byte copy, bounds are the image
    rng = np.random.RandomState(1)
    keys = random_keys(rng, 1, 300, None); n = np.array([300], 'i4')
    depth = np.full((1, 480, 640), 10000, np.uint16)
    kun = np.zeros((1, 300, 28), np.uint8); ur = np.zeros((1, 300), 'f4'); z = np.zeros((1, 300), 'f4')
    frame.undistort_stereo_rgbd_batch_dev(emu, 1, 300, keys.view(np.uint8).reshape(1, 300, 28), n, d0, cam, depth, 640, 480, kun, ur, z)
    assert (kun.reshape(-1) == keys.view(np.uint8).reshape(-1)).all()
    assert frame.image_bounds(emu, 640, 480, cam, d0) == dict(min_x=0.0, max_x=640.0, min_y=0.0, max_y=480.0)
    # n == 0, invalid ndist
    assert frame.undistort_points(emu, np.zeros((0, 2), 'f4'), cam, d0).shape == (0, 2)
    from sg_slam_amd.capi import _vp
    K4 = np.array([cam['fx'], cam['fy'], cam['cx'], cam['cy']], 'f4'); p = np.zeros((4, 2), 'f4'); o = np.zeros_like(p)
    for nd in (0, 3, 6, 7, 12):
        dd = np.full(12, 0.1, 'f4')
        assert emu.dll.sgx_undistort_points(4, _vp(p), _vp(K4), _vp(dd), nd, _vp(o)) == -1, nd
        assert emu.dll.sgx_frame_image_bounds(640, 480, _vp(K4), _vp(dd), nd, C.byref(frame.camera_struct(cam))) == -1, nd


def test_image_bounds_emu(emu):
    check_image_bounds(emu)


def test_undistort_stereo_kernel_emu(emu, oracle):
    check_undistort_stereo_kernel(emu, oracle)


def test_tracker_set_distortion_rules_emu(emu):
    from sg_slam_amd.capi import _vp, Camera
    d = load('TUM1')['dist']
    gen = synth.PlaneStream(seed=1234)
    tr = TrackerNative(emu, 1, CAM, pipelined=False, dynamic_mask=False, dist=d)
    assert tr.bounds == {k: float(v) for k, v in zip(('min_x', 'max_x', 'min_y', 'max_y'), R.image_bounds(640, 480, CAM, d))}
    tr.set_initial_pose(gen.Tcw(0)[None])
    g, dep, _ = gen.frame(0)
    tr.step(g[None], dep[None])
    cam = Camera()
    assert emu.dll.sgx_tracker_set_distortion(tr.h, _vp(d), len(d), C.byref(cam)) == -1          # only before the first step
    assert tr.frame_keys_un_dev() != tr.frame_dev()['keys']
    tr.close()
    plain = TrackerNative(emu, 1, CAM, pipelined=False, dynamic_mask=False, dist=np.zeros(4, 'f4'))
    assert plain.bounds == dict(min_x=0.0, max_x=640.0, min_y=0.0, max_y=480.0)
    assert emu.dll.sgx_tracker_set_distortion(plain.h, _vp(d), 6, None) == -1
    plain.set_initial_pose(gen.Tcw(0)[None]); plain.step(g[None], dep[None])
    assert plain.frame_keys_un_dev() == plain.frame_dev()['keys']
    plain.close()


# ---------------------------------------------------------------------------------------------------------- the chain
def run_tracker_distorted(lib, oracle, dist, nframes=5, offs=(0, 41)):
    """TrackerBatch(dist) stage by stage against the oracle fed the restated keys_un, bounds and uright (the way tests/test_tracker_emu.py chains it)"""
    from test_tracker_emu import make_map_points, ring_concat
    gen = synth.DistortedLayeredStream(dist, seed=1234)
    offs = list(offs)
    tr = TrackerBatch(lib, 2, CAM, xp='numpy', debug_taps=True, dist=dist)
    cam = R.cam_with_bounds(CAM, dist)
    assert all(np.float32(tr.cam[k]) == np.float32(cam[k]) for k in ('min_x', 'max_x', 'min_y', 'max_y'))
    cap = tr.cap
    rings = [[None, None], [None, None]]
    tr.set_initial_pose(np.stack([gen.Tcw(o) for o in offs]))
    sf = oracle.orb_params()['scale']; is2 = oracle.orb_params()['inv_sigma2']
    last = [None, None]; Tl = [gen.Tcw(o).astype('f4') for o in offs]; Tll = [t.copy() for t in Tl]
    for t in range(nframes):
        fr = [gen.frame(o + t) for o in offs]
        tr.step(np.stack([f[0] for f in fr]), np.stack([f[1] for f in fr]))
        n, nm, ninl = tr.last_counts(); nml, ninl2 = tr.last_local_counts()
        Tg = tr.last_pose(); Tmm = tr.Tcw_mm.reshape(2, 4, 4)
        c = tr.cur
        for s in range(2):
            k, d = oracle.orb_extract(fr[s][0])
            assert n[s] == len(k)
            ku = R.undistort_keypoints(k, CAM, dist)
            assert (tr.keys[c][s, :len(k)].reshape(-1) == k.view(np.uint8).reshape(-1)).all()
            assert (tr.keys_un[c][s, :len(k)].reshape(-1) == ku.view(np.uint8).reshape(-1)).all()
            _, z = oracle.compute_stereo_from_rgbd(k, fr[s][1], CAM['bf'], CAM['depth_factor'])
            with np.errstate(divide='ignore'):
                ur = np.where(z > 0, (ku['x'] - np.float32(CAM['bf']) / z).astype('f4'), np.float32(-1)).astype('f4')
            assert (tr.uright[c][s, :len(k)].view(np.uint32) == ur.view(np.uint32)).all()
            if t == 0:
                Tc = Tl[s].copy()
            else:
                A = Tl[s]; P = Tll[s]
                if t == 1:
                    Tpred = A.copy()
                else:
                    Twc = np.eye(4, dtype='f4'); Twc[:3, :3] = P[:3, :3].T
                    Twc[:3, 3] = (-(P[:3, :3].T.astype('f8') @ P[:3, 3].astype('f8'))).astype('f4')
                    def mm(X, Y):
                        Z = np.zeros((4, 4), 'f4')
                        for i in range(4):
                            for j in range(4):
                                acc = np.float32(X[i, 0] * Y[0, j])
                                for kk in range(1, 4):
                                    acc = np.float32(acc + np.float32(X[i, kk] * Y[kk, j]))
                                Z[i, j] = acc
                        return Z
                    Tpred = mm(mm(A, Twc), A)
                cur = dict(keys=ku, desc=d, uright=ur, Tcw=Tpred)
                exp_match, exp_n = oracle.search_by_projection_frame(cur, last[s], cam, sf, th=15, mono=False, check_ori=True)
                assert nm[s] == exp_n and (tr.match[s, :len(k)] == exp_match).all(), (t, s)
                fr2 = dict(keys=ku, uright=ur, has_mp=(exp_match >= 0).astype(np.uint8), Tcw=Tpred,
                           xw=np.where((exp_match >= 0)[:, None], last[s]['xw'][np.maximum(exp_match, 0)], 0).astype('f4'))
                en, eT, eout = oracle.pose_optimization(fr2, cam, is2)
                assert ninl[s] == en and (tr.outlier[s, :len(k)] == eout).all(), (t, s)
                assert np.abs(Tmm[s] - eT).max() <= 1e-5 * max(1.0, np.abs(eT).max())
                keep = (exp_match >= 0) & (eout == 0)
                lm = ring_concat(rings[s], cap)
                cur2 = dict(keys=ku, desc=d, uright=ur, Tcw=Tmm[s], mp_obs=np.where(keep, 0, -1).astype('i4'))
                eml, enl, einview = oracle.search_by_projection_local(cur2, lm, cam, sf, th=3.0, nnratio=0.8, viewing_cos_limit=0.5)
                assert nml[s] == enl and (tr.match_local[s, :len(k)] == eml).all() and (tr.in_view[s] == einview).all(), (t, s)
                merged = np.where(eml >= 0, cap + eml, np.where(keep, exp_match, -1))
                xw_all = np.concatenate([np.pad(last[s]['xw'], ((0, cap - len(last[s]['xw'])), (0, 0))), lm['xw']]).astype('f4')
                fr3 = dict(keys=ku, uright=ur, has_mp=(merged >= 0).astype(np.uint8), Tcw=Tmm[s],
                           xw=np.where((merged >= 0)[:, None], xw_all[np.maximum(merged, 0)], 0).astype('f4'))
                en2, eT2, eout2 = oracle.pose_optimization(fr3, cam, is2)
                assert ninl2[s] == en2 and (tr.outlier2[s, :len(k)] == eout2).all(), (t, s)
                assert np.abs(Tg[s] - eT2).max() <= 1e-5 * max(1.0, np.abs(eT2).max())
                Tc = Tg[s].copy()
                assert np.abs(Tc - gen.Tcw(offs[s] + t)).max() < 0.03 and en > 100, (t, s)
            if t > 0:
                rings[s][(t - 1) % 2] = make_map_points(last[s]['keys'], last[s]['xw'], last[s]['has_mp'], last[s]['desc'], Tl[s], np.asarray(sf, 'f4'))
            xw, has = oracle.unproject_stereo(ku, z, Tc, cam)
            last[s] = dict(keys=ku, desc=d, uright=ur, Tcw=Tc, has_mp=has, outlier=np.zeros(len(k), np.uint8), xw=xw, obs=np.zeros(len(k), 'i4'), mpdesc=d)
            Tll[s] = Tl[s]; Tl[s] = Tc


def test_tracker_distorted_chain_emu(emu, oracle):
    run_tracker_distorted(emu, oracle, load('TUM1')['dist'])


def run_native_equals_python_distorted(lib, xp, dynamic_mask, dist, nframes=4, S=2, gen=None, compare_plain=False):
    """TrackerNative(dist) == TrackerBatch(dist), bit for bit (poses, counts, RANSAC statistics, records, mvKeysUn).  compare_plain: a third tracker built
    WITHOUT dist must give the same bits too (for coefficient vectors with k1 == 0)."""
    gen = gen or synth.DistortedLayeredStream(load('TUM1')['dist'], seed=1234)
    offs = [3, 57][:S]
    def D(a):
        if xp != 'torch':
            return a
        import torch
        return torch.from_numpy(a.view(np.int16) if a.dtype == np.uint16 else a).cuda()
    H = (lambda a: a.cpu().numpy()) if xp == 'torch' else (lambda a: np.asarray(a))
    py = TrackerBatch(lib, S, CAM, xp=xp, lk=dynamic_mask, dist=dist)
    nat = TrackerNative(lib, S, CAM, dynamic_mask=dynamic_mask, pipelined=(xp == 'torch'), dist=dist)
    ref = TrackerNative(lib, S, CAM, dynamic_mask=dynamic_mask, pipelined=(xp == 'torch')) if compare_plain else None
    assert nat.bounds == {k: float(py.cs.__getattribute__(k)) for k in ('min_x', 'max_x', 'min_y', 'max_y')}
    T0 = np.stack([gen.Tcw(o) for o in offs])
    py.set_initial_pose(T0); nat.set_initial_pose(T0)
    if ref: ref.set_initial_pose(T0)
    held = []
    for t in range(nframes):
        fr = [gen.frame(o + t) for o in offs]
        gray = D(np.stack([f[0] for f in fr])); depth = D(np.stack([f[1] for f in fr]))
        held.append((gray, depth))
        py.step(gray, depth); nat.step(gray, depth)
        if ref: ref.step(gray, depth)
        r = nat.read()
        n, nm, ninl = py.last_counts(); nml, ninl2 = py.last_local_counts()
        assert (r['nkeys'] == n).all(), t
        assert (r['Tcw'].view(np.uint32) == py.last_pose().reshape(S, 16).view(np.uint32)).all(), t
        if t > 0:
            assert (r['nmatch'] == nm).all() and (r['ninl'] == ninl).all() and (r['nmatch_local'] == nml).all() and (r['ninl2'] == ninl2).all(), t
            if dynamic_mask:
                assert (r['nkeys_raw'] == H(py.rn)).all() and (r['f_ok'] == H(py.f_ok)).all() and (r['f_stats'] == H(py.f_stats)).all(), t
        if ref:
            rr = ref.read()
            for k in r:
                assert (r[k].view(np.uint32) == rr[k].view(np.uint32)).all(), (t, k)
        cap = nat.cap; c = py.cur
        if xp == 'torch':
            import torch
            rec = torch.zeros((S, nat.rec_bytes), dtype=torch.uint8, device='cuda')
            nat.pack_records(rec, stream=torch.cuda.current_stream().cuda_stream); torch.cuda.synchronize()
            rec = rec.cpu().numpy()
            kun_host = np.empty((S, cap * 28), np.uint8); dev_to_host(nat.frame_keys_un_dev(), kun_host)
        else:
            rec = np.zeros((S, nat.rec_bytes), np.uint8); nat.pack_records(rec)
            kun_host = np.frombuffer((C.c_uint8 * (S * cap * 28)).from_address(nat.frame_keys_un_dev()), np.uint8).reshape(S, cap * 28).copy()
        assert (rec[:, 0:4].copy().view(np.int32)[:, 0] == n).all() and (rec[:, 4:16] == 0).all()
        assert (rec[:, 16:16 + cap * 28] == H(py.keys[c]).reshape(S, cap * 28)).all()          # the records keep mvKeys
        assert (rec[:, 16 + cap * 28:16 + cap * 60] == H(py.desc[c]).reshape(S, cap * 32)).all()
        assert (rec[:, 16 + cap * 60:].copy().view(np.float32) == r['Tcw']).all()
        assert (kun_host == H(py.keys_un[c]).reshape(S, cap * 28)).all()
        if ref:                                                                                 # and so do the records of a tracker without the call
            if xp == 'torch':
                rec2 = torch.zeros((S, nat.rec_bytes), dtype=torch.uint8, device='cuda')
                ref.pack_records(rec2, stream=torch.cuda.current_stream().cuda_stream); torch.cuda.synchronize(); rec2 = rec2.cpu().numpy()
            else:
                rec2 = np.zeros((S, nat.rec_bytes), np.uint8); ref.pack_records(rec2)
            assert (rec2 == rec).all(), t
    nat.close()
    if ref: ref.close()
    return r, gen, offs


def dev_to_host(ptr, out):
    """synchronous device -> host copy of out.nbytes bytes at device address `ptr` (GPU runs; the HIP runtime torch has loaded)"""
    hip = C.CDLL('libamdhip64.so')
    hip.hipMemcpy.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int]
    assert hip.hipMemcpy(out.ctypes.data_as(C.c_void_p), C.c_void_p(ptr), out.nbytes, 2) == 0


def test_native_equals_python_distorted_emu(emu):
    run_native_equals_python_distorted(emu, 'numpy', dynamic_mask=False, dist=load('TUM1')['dist'], nframes=5)


def test_native_equals_python_distorted_mask_emu(emu):
    run_native_equals_python_distorted(emu, 'numpy', dynamic_mask=True, dist=load('TUM1')['dist'], nframes=3)
