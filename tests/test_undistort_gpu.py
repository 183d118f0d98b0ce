"""GPU (MI355X): lens distortion on the device — sgx_undistort_points, Frame::ComputeImageBounds and k_undistort_stereo_rgbd bit for bit against the
float64 restatement (tests/undistort_ref.py, hence the emulator), the C++ tracker with a distorted camera against the Python orchestration (with the
detector's bf16 matrix products on their own stream beside the fp64 kernel), zero-k1 coefficient vectors that must change nothing, and the accuracy the
feature exists for."""
import numpy as np
import pytest
from scenes import CAM
from test_undistort_emu import (load, check_undistort_points, check_image_bounds, check_undistort_stereo_kernel, run_native_equals_python_distorted)

pytestmark = pytest.mark.gpu


def _dev(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a.view(np.int16) if a.dtype == np.uint16 else a)).cuda()


def _host(t):
    return t.cpu().numpy()


def test_undistort_points_device_bit_exact(gpulib):
    check_undistort_points(gpulib)


def test_image_bounds_device(gpulib):
    check_image_bounds(gpulib)


def test_undistort_stereo_kernel_device(gpulib, oracle):
    check_undistort_stereo_kernel(gpulib, oracle, to_dev=_dev, to_host=_host)


@pytest.mark.parametrize('dynamic_mask', [False, True])
def test_native_equals_python_distorted_gpu(gpulib, dynamic_mask):
    run_native_equals_python_distorted(gpulib, 'torch', dynamic_mask=dynamic_mask, dist=load('TUM1')['dist'], nframes=5)


@pytest.mark.parametrize('dist', [np.zeros(4, 'f4'), np.array([0.0, 0.0, 0.004, -0.003, 0.2], 'f4')], ids=['tum3_zero', 'k1_zero_p1_nonzero'])
@pytest.mark.parametrize('dynamic_mask', [False, True])
def test_zero_k1_changes_nothing_gpu(gpulib, dist, dynamic_mask):
    """k1 == 0 (TUM3, or k1 = 0 with p1 / p2 / k3 != 0): poses, counts and records bit-identical to a tracker that never heard of distortion"""
    from sg_slam_amd import synth
    run_native_equals_python_distorted(gpulib, 'torch', dynamic_mask=dynamic_mask, dist=dist, nframes=5, gen=synth.LayeredStream(seed=1234), compare_plain=True)


def test_native_tracker_distorted_with_detector_gpu(gpulib):
    """the detector on its own stream (bf16 matrix products beside k_undistort_stereo_rgbd), its boxes feeding the mask: library-side event chain == Python-side"""
    import ctypes as C
    import torch
    from sg_slam_amd import synth
    from sg_slam_amd.capi import DetResult
    from sg_slam_amd.tracker import TrackerBatch
    from sg_slam_amd.tracker_native import TrackerNative
    from test_tracker_native_gpu import _detector
    S, MB, NF = 2, 100, 5
    dist = load('TUM1')['dist']
    gen = synth.DistortedPlaneStream(dist, seed=1234); offs = [3, 57]
    T0 = np.stack([gen.Tcw(o) for o in offs])
    det_py, det_nat = _detector(gpulib, S), _detector(gpulib, S)
    py = TrackerBatch(gpulib, S, CAM, xp='torch', lk=True, max_boxes=MB, dist=dist); py.set_initial_pose(T0)
    nat = TrackerNative(gpulib, S, CAM, dynamic_mask=True, max_boxes=MB, detector=det_nat, dist=dist); nat.set_initial_pose(T0)
    sD = torch.cuda.Stream()
    res = [torch.zeros((S, C.sizeof(DetResult)), dtype=torch.uint8, device='cuda') for _ in range(2)]
    boxes = [torch.zeros((S, MB, 4), dtype=torch.float32, device='cuda') for _ in range(2)]
    nb = [torch.zeros(S, dtype=torch.int32, device='cuda') for _ in range(2)]; have = [torch.zeros(S, dtype=torch.int32, device='cuda') for _ in range(2)]
    ev = [torch.cuda.Event() for _ in range(2)]
    held = []; total = 0
    for t in range(NF):
        fr = [gen.frame(o + t) for o in offs]
        d_gray = torch.from_numpy(np.stack([f[0] for f in fr])).cuda(); d_depth = torch.from_numpy(np.stack([f[1] for f in fr]).view(np.int16)).cuda()
        d_bgr = d_gray.unsqueeze(-1).expand(S, 480, 640, 3).contiguous()
        held.append((d_gray, d_depth, d_bgr))
        b = t & 1
        sD.wait_stream(torch.cuda.current_stream())
        if t >= 2: sD.wait_event(py.ev_extract[(t - 2) % 3])
        det_py.detect_batch_dev(d_bgr, 640 * 3, S, res[b], boxes[b], nb[b], MB, have[b], stream=sD.cuda_stream)
        ev[b].record(sD)
        py.step(d_gray, d_depth, mask=dict(boxes=boxes[b], nboxes=nb[b], have_dynamic=have[b], event=ev[b]))
        nat.step(d_gray, d_depth, d_bgr=d_bgr, stream=torch.cuda.current_stream().cuda_stream)
        r = nat.read(); py.synchronize(); sD.synchronize(); torch.cuda.synchronize()
        total += int(nb[b].sum().item())
        n, nm, ninl = py.last_counts(); nml, ninl2 = py.last_local_counts()
        assert (r['nkeys'] == n).all() and (r['Tcw'].view(np.uint32) == py.last_pose().reshape(S, 16).view(np.uint32)).all(), t
        if t > 0:
            assert (r['nkeys_raw'] == py.rn.cpu().numpy()).all() and (r['f_stats'] == py.f_stats.cpu().numpy()).all(), t
            assert (r['nmatch'] == nm).all() and (r['ninl'] == ninl).all() and (r['nmatch_local'] == nml).all() and (r['ninl2'] == ninl2).all(), t
    assert total > 0
    assert np.abs(r['Tcw'].reshape(S, 4, 4) - np.stack([gen.Tcw(o + NF - 1) for o in offs])).max() < 0.03
    nat.close()


def test_distorted_camera_tracks_ground_truth_gpu(gpulib):
    """the point of the feature: on a lens with TUM1's coefficients the tracker that undistorts follows the ground truth over 24 frames"""
    import torch
    from sg_slam_amd import synth
    from sg_slam_amd.tracker_native import TrackerNative
    S, NF = 2, 24
    dist = load('TUM1')['dist']
    gen = synth.DistortedPlaneStream(dist, seed=1234); offs = [0, 50]
    T0 = np.stack([gen.Tcw(o) for o in offs])
    err = {}
    for name, d in (('undistorted', dist), ('raw', None)):
        tr = TrackerNative(gpulib, S, CAM, dynamic_mask=True, dist=d); tr.set_initial_pose(T0)
        worst, held = 0.0, []
        for t in range(NF):
            fr = [gen.frame(o + t) for o in offs]
            g = torch.from_numpy(np.stack([f[0] for f in fr])).cuda(); dp = torch.from_numpy(np.stack([f[1] for f in fr]).view(np.int16)).cuda()
            held.append((g, dp)); held = held[-4:]
            tr.step(g, dp)
            T = tr.last_pose()
            worst = max(worst, float(np.abs(T - np.stack([gen.Tcw(o + t) for o in offs])).max()))
        tr.close(); err[name] = worst
    print(f'max |Tcw - ground truth| over {NF} frames, TUM1 lens: with undistortion {err["undistorted"]:.4f}, without {err["raw"]:.4f}')
    assert err['undistorted'] < 0.03
