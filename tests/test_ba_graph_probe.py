"""CPU: tests/host/ba_graph_probe.cpp feeds sgx_covis_ba_graph_batch_dev / sgx_covis_ba_graph ids out of range, capacities of 0 and one short of the need, a full
max_queries and a query for a keyframe erased while lists still name it, and checks the statuses, the untouched remainder of every row and a clean exit.  It and the
emulator unit it needs are built with AddressSanitizer (LeakSanitizer included) and UBSan, and its buffers have exactly the documented sizes, so a row or a workspace
entry read or written outside its array ends the program.  A stand-alone program: nothing is loaded into Python."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
UNITS = ('sgx_covis',)


def test_ba_graph_probe_under_sanitizers(tmp_path):
    csrc = os.path.join(ROOT, 'sg_slam_amd', 'csrc')
    flags = ['-O2', '-g', '-std=c++17', '-ffp-contract=off', '-DSGX_EMU', '-DSGX_DEBUG_TAPS', '-fsanitize=address,undefined', '-fno-sanitize-recover=all',
             '-Wno-unused-function', '-Wno-unused-variable', '-Wno-unknown-pragmas']          # -O2 as the emulator build (csrc/Makefile)
    objs = []
    for u in UNITS:
        objs.append(str(tmp_path / (u + '.o')))
        subprocess.check_call(['g++'] + flags + ['-x', 'c++', '-c', os.path.join(csrc, u + '.cpp'), '-o', objs[-1]])
    exe = str(tmp_path / 'ba_graph_probe')
    subprocess.check_call(['g++'] + flags + [os.path.join(ROOT, 'tests', 'host', 'ba_graph_probe.cpp')] + objs + ['-o', exe, '-lm'])
    r = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert r.returncode == 0, r.stdout[-4000:]
    assert 'ba_graph_probe: ok' in r.stdout
