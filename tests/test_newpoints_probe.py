"""CPU: tests/host/newpoints_probe.cpp feeds sgx_kfstore_* and sgx_create_new_map_points* buffers of exactly the documented sizes, refused adds (a known id, a full store,
a bad octave), NULL optional outputs, Q = 0, missing arrays, an erased keyframe named as neighbour and every allocation or upload refused in turn, and checks the statuses, the untouched outputs of every refused call
and a clean exit.  It and the emulator unit it needs are built with AddressSanitizer (LeakSanitizer included) and UBSan, so a row or a workspace entry read or written
outside its array ends the program.  A stand-alone program: nothing is loaded into Python."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
UNITS = ('sgx_newpoints', 'sgx_devmem')


def test_newpoints_probe_under_sanitizers(tmp_path):
    csrc = os.path.join(ROOT, 'sg_slam_amd', 'csrc')
    flags = ['-O2', '-g', '-std=c++17', '-ffp-contract=off', '-DSGX_EMU', '-DSGX_DEBUG_TAPS', '-fsanitize=address,undefined', '-fno-sanitize-recover=all',
             '-Wno-unused-function', '-Wno-unused-variable', '-Wno-unknown-pragmas']          # -O2 as the emulator build (csrc/Makefile)
    objs = []
    for u in UNITS:
        objs.append(str(tmp_path / (u + '.o')))
        subprocess.check_call(['g++'] + flags + ['-x', 'c++', '-c', os.path.join(csrc, u + '.cpp'), '-o', objs[-1]])
    exe = str(tmp_path / 'newpoints_probe')
    subprocess.check_call(['g++'] + flags + [os.path.join(ROOT, 'tests', 'host', 'newpoints_probe.cpp')] + objs + ['-o', exe, '-lm'])
    r = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert r.returncode == 0, r.stdout[-4000:]
    assert 'newpoints_probe: ok' in r.stdout
