"""CPU: tests/host/globalmap_probe.cpp feeds the sgx_globalmap_* entries a refused create, a full map, strided batches, a read buffer smaller than the map, a reset
between sequences and a destroy after a failed call, and checks the statuses, the unchanged map after a refused call and a clean exit.  It and the emulator unit it
needs are built with AddressSanitizer (LeakSanitizer included) and UBSan, and its buffers have exactly the documented sizes, so a point, a count or a workspace entry
read or written outside its array ends the program.  A stand-alone program: nothing is loaded into Python."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
UNITS = ('sgx_globalmap',)


def test_globalmap_probe_under_sanitizers(tmp_path):
    csrc = os.path.join(ROOT, 'sg_slam_amd', 'csrc')
    flags = ['-O2', '-g', '-std=c++17', '-ffp-contract=off', '-DSGX_EMU', '-DSGX_DEBUG_TAPS', '-fsanitize=address,undefined', '-fno-sanitize-recover=all',
             '-Wno-unused-function', '-Wno-unused-variable', '-Wno-unknown-pragmas']          # -O2 as the emulator build (csrc/Makefile)
    objs = []
    for u in UNITS:
        objs.append(str(tmp_path / (u + '.o')))
        subprocess.check_call(['g++'] + flags + ['-x', 'c++', '-c', os.path.join(csrc, u + '.cpp'), '-o', objs[-1]])
    exe = str(tmp_path / 'globalmap_probe')
    subprocess.check_call(['g++'] + flags + [os.path.join(ROOT, 'tests', 'host', 'globalmap_probe.cpp')] + objs + ['-o', exe, '-lm'])
    r = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert r.returncode == 0, r.stdout[-4000:]
    assert 'globalmap_probe: ok' in r.stdout
