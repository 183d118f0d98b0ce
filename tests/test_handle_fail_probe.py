"""CPU: tests/host/handle_fail_probe.cpp walks the failure exits of the handles whose device buffers one owner holds (sg_slam_amd/csrc/sgx_devmem.h) with
sgx_debug_devmem_fail_after — every allocation and upload copy of the PnP, Initializer, Sim3Solver, Detector3D, vocabulary, keyframe database and ORB extractor creates,
of the Initializer's regrow and of the PnP batch's hypothesis buffers — and checks what include/sgx.h promises for them: *out cleared and the status that occurred, a
failed Initialize that leaves the initializer as it was, an all-or-nothing reserve that a retry completes.  It and the emulator units it needs are built with
AddressSanitizer (LeakSanitizer included) and UBSan, so a failed call that leaves a buffer behind, or a later call that touches a half-built handle, ends the program.
A stand-alone program: nothing is loaded into Python."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
UNITS = ('sgx_pnp', 'sgx_init', 'sgx_sim3solver', 'sgx_obj3d', 'sgx_kfdb', 'sgx_voc', 'sgx_orb', 'sgx_prof', 'sgx_devmem')


def test_handle_fail_probe_under_sanitizers(tmp_path):
    csrc = os.path.join(ROOT, 'sg_slam_amd', 'csrc')
    flags = ['-O2', '-g', '-std=c++17', '-ffp-contract=off', '-DSGX_EMU', '-DSGX_DEBUG_TAPS', '-fsanitize=address,undefined', '-fno-sanitize-recover=all',
             '-Wno-unused-function', '-Wno-unused-variable', '-Wno-unknown-pragmas']          # -O2 as the emulator build (csrc/Makefile)
    objs = []
    jobs = []
    for u in UNITS:
        # the kernel units only, as in test_tracker_fail_probe.py: sgx_i64_to_f32 shifts a negative 64-bit value left, which every compiler in use defines (and C++20
        # too) but C++17's UBSan reports; the owner's unit and the probe itself keep every check
        kernels_only = [] if u == 'sgx_devmem' else ['-fno-sanitize=shift-base']
        objs.append(str(tmp_path / (u + '.o')))
        jobs.append(subprocess.Popen(['g++'] + flags + kernels_only + ['-x', 'c++', '-c', os.path.join(csrc, u + '.cpp'), '-o', objs[-1]]))
    assert [j.wait() for j in jobs] == [0] * len(jobs)
    exe = str(tmp_path / 'handle_fail_probe')
    subprocess.check_call(['g++'] + flags + [os.path.join(ROOT, 'tests', 'host', 'handle_fail_probe.cpp')] + objs + ['-o', exe, '-lm'])
    r = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    print(r.stdout[-4000:])
    assert r.returncode == 0, r.stdout[-4000:]
    assert 'handle_fail_probe: ok' in r.stdout
