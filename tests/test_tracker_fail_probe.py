"""CPU: tests/host/tracker_fail_probe.cpp walks the failure exits of the tracker host with sgx_tracker_debug_fail_after — every acquisition of sgx_tracker_create, of the
first sgx_tracker_host_buffers and of sgx_tracker_set_distortion, and every checked call of a step — and checks what include/sgx.h promises for them: *out cleared and the
status that occurred, all-or-nothing set-up calls that a retry completes, a failed step that poisons the tracker.  It and the emulator units it needs are built with
AddressSanitizer (LeakSanitizer included) and UBSan, so a failed call that leaves a buffer behind, or a later call that touches a half-built tracker, ends the program.
A stand-alone program: nothing is loaded into Python."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
UNITS = ('sgx_orb', 'sgx_prof', 'sgx_tracker', 'sgx_flow', 'sgx_det', 'sgx_match', 'sgx_poseopt', 'sgx_undistort')


def test_tracker_fail_probe_under_sanitizers(tmp_path):
    csrc = os.path.join(ROOT, 'sg_slam_amd', 'csrc')
    flags = ['-O2', '-g', '-std=c++17', '-ffp-contract=off', '-DSGX_EMU', '-DSGX_DEBUG_TAPS', '-fsanitize=address,undefined', '-fno-sanitize-recover=all',
             '-Wno-unused-function', '-Wno-unused-variable', '-Wno-unknown-pragmas']          # -O2 as the emulator build (csrc/Makefile)
    objs = []
    jobs = []
    for u in UNITS:
        # the kernel units only: sgx_i64_to_f32 (sgx_flow_kernels.h) shifts a negative 64-bit value left, which every compiler in use defines (and C++20 too) but C++17's
        # UBSan reports; the host under test and the probe itself keep every check
        kernels_only = [] if u == 'sgx_tracker' else ['-fno-sanitize=shift-base']
        objs.append(str(tmp_path / (u + '.o')))
        jobs.append(subprocess.Popen(['g++'] + flags + kernels_only + ['-x', 'c++', '-c', os.path.join(csrc, u + '.cpp'), '-o', objs[-1]]))
    assert [j.wait() for j in jobs] == [0] * len(jobs)
    exe = str(tmp_path / 'tracker_fail_probe')
    subprocess.check_call(['g++'] + flags + [os.path.join(ROOT, 'tests', 'host', 'tracker_fail_probe.cpp')] + objs + ['-o', exe, '-lm'])
    r = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    print(r.stdout[-4000:])
    assert r.returncode == 0, r.stdout[-4000:]
    assert 'tracker_fail_probe: ok' in r.stdout
