"""CPU: tests/host/orb_plan_probe.cpp creates and destroys an ORB extractor handle for every geometry of test_orb_plan.py, the refused ones included; it and the emulator
units it needs are built with AddressSanitizer (LeakSanitizer included) and UBSan, so a planner that leaves its tables, or a refused geometry that leaves the handle or a
buffer behind, ends the program.  A stand-alone program: nothing is loaded into Python.  The SGX_ERR_DEVICE exits of sgx_orb_create cannot be reached in the emulator: they
rest on the create function's single failure exit and the handle's owning destructor."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
UNITS = ('sgx_orb', 'sgx_prof')


def test_orb_plan_probe_under_sanitizers(tmp_path):
    csrc = os.path.join(ROOT, 'sg_slam_amd', 'csrc')
    flags = ['-O2', '-g', '-std=c++17', '-ffp-contract=off', '-DSGX_EMU', '-DSGX_DEBUG_TAPS', '-fsanitize=address,undefined', '-fno-sanitize-recover=all',
             '-Wno-unused-function', '-Wno-unused-variable', '-Wno-unknown-pragmas']          # -O2 as the emulator build (csrc/Makefile)
    objs = []
    jobs = []
    for u in UNITS:
        objs.append(str(tmp_path / (u + '.o')))
        jobs.append(subprocess.Popen(['g++'] + flags + ['-x', 'c++', '-c', os.path.join(csrc, u + '.cpp'), '-o', objs[-1]]))
    assert [j.wait() for j in jobs] == [0] * len(jobs)
    exe = str(tmp_path / 'orb_plan_probe')
    subprocess.check_call(['g++'] + flags + [os.path.join(ROOT, 'tests', 'host', 'orb_plan_probe.cpp')] + objs + ['-o', exe, '-lm'])
    r = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert r.returncode == 0, r.stdout[-4000:]
