"""CPU: tests/host/loopclose_probe.cpp feeds sgx_covis_consistency_reserve / _clear / _info, sgx_covis_consistency*, sgx_covis_get_consistent_groups,
sgx_covis_connected_batch*, sgx_covis_gba_update*, sgx_gba_correct_points_dev and sgx_gba_correct_points capacities of 0 and one short of the need, candidate ids out of range and twice, counts out of range, a full group table, malformed keyframe tables, origins outside the GBA, reference rows out of range and missing arrays,
and checks the statuses, the untouched outputs of every refused call and a clean exit.  It and the emulator unit it needs are built with AddressSanitizer
(LeakSanitizer included) and UBSan, and its buffers have exactly the documented sizes, so a row or a workspace entry read or written outside its array ends the program.
A stand-alone program: nothing is loaded into Python."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
UNITS = ('sgx_covis',)


def test_loopclose_probe_under_sanitizers(tmp_path):
    csrc = os.path.join(ROOT, 'sg_slam_amd', 'csrc')
    flags = ['-O2', '-g', '-std=c++17', '-ffp-contract=off', '-DSGX_EMU', '-DSGX_DEBUG_TAPS', '-fsanitize=address,undefined', '-fno-sanitize-recover=all',
             '-Wno-unused-function', '-Wno-unused-variable', '-Wno-unknown-pragmas']          # -O2 as the emulator build (csrc/Makefile)
    objs = []
    for u in UNITS:
        objs.append(str(tmp_path / (u + '.o')))
        subprocess.check_call(['g++'] + flags + ['-x', 'c++', '-c', os.path.join(csrc, u + '.cpp'), '-o', objs[-1]])
    exe = str(tmp_path / 'loopclose_probe')
    subprocess.check_call(['g++'] + flags + [os.path.join(ROOT, 'tests', 'host', 'loopclose_probe.cpp')] + objs + ['-o', exe, '-lm'])
    r = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert r.returncode == 0, r.stdout[-4000:]
    assert 'loopclose_probe: ok' in r.stdout
