"""CPU: tests/host/match2_stage_probe.cpp calls every host-pointer matcher entry once on heap buffers of exactly the documented sizes; it and the emulator units it needs are
built with AddressSanitizer and UBSan, so an upload or read-back that leaves the caller's buffer or the staging slot ends the program.  A stand-alone program: nothing is
loaded into Python."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
UNITS = ('sgx_match2', 'sgx_match', 'sgx_sim3', 'sgx_poseopt', 'sgx_prof', 'sgx_orb')          # sgx_orb.cpp defines the emulator's blockIdx / blockDim / gridDim


def test_match2_stage_probe_under_sanitizers(tmp_path):
    csrc = os.path.join(ROOT, 'sg_slam_amd', 'csrc')
    # -O2 as the emulator build (csrc/Makefile).  Below it g++ 11 miscompiles `(c ? p : q)[i]` (sgx_sim3_kernels.h) once both the pointer-overflow and the alignment checks of
    # UBSan instrument it: a three-line program with that expression and nothing else segfaults at -O0
    flags = ['-O2', '-g', '-std=c++17', '-ffp-contract=off', '-DSGX_EMU', '-DSGX_DEBUG_TAPS', '-fsanitize=address,undefined', '-fno-sanitize-recover=all',
             '-Wno-unused-function', '-Wno-unused-variable', '-Wno-unknown-pragmas']
    objs = []
    jobs = []
    for u in UNITS:
        objs.append(str(tmp_path / (u + '.o')))
        jobs.append(subprocess.Popen(['g++'] + flags + ['-x', 'c++', '-c', os.path.join(csrc, u + '.cpp'), '-o', objs[-1]]))
    assert [j.wait() for j in jobs] == [0] * len(jobs)
    exe = str(tmp_path / 'match2_stage_probe')
    subprocess.check_call(['g++'] + flags + [os.path.join(ROOT, 'tests', 'host', 'match2_stage_probe.cpp')] + objs + ['-o', exe, '-lm'])
    r = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert r.returncode == 0, r.stdout[-4000:]
