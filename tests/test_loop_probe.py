"""CPU: tests/host/loop_probe.cpp feeds sgx_covis_add_loop_edge, sgx_covis_loop_begin*, sgx_covis_loop_connections*, sgx_covis_essential_graph* and the Sim3 glue entries
(sgx_loop_propagate_sim3, sgx_eg_flatten, sgx_eg_recover, sgx_correct_map_points_dev; their unit is sgx_loop_sim3.cpp) ids out of range,
capacities of 0 and one short of the need, malformed group rows and CSRs and a full loop-edge table, and checks the statuses, the untouched remainder of every row and a
clean exit.  It and the emulator unit it needs are built with AddressSanitizer (LeakSanitizer included) and UBSan, and its buffers have exactly the documented sizes, so
a row or a workspace entry read or written outside its array ends the program.  A stand-alone program: nothing is loaded into Python."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
UNITS = ('sgx_covis', 'sgx_loop_sim3')


def test_loop_probe_under_sanitizers(tmp_path):
    csrc = os.path.join(ROOT, 'sg_slam_amd', 'csrc')
    flags = ['-O2', '-g', '-std=c++17', '-ffp-contract=off', '-DSGX_EMU', '-DSGX_DEBUG_TAPS', '-fsanitize=address,undefined', '-fno-sanitize-recover=all',
             '-Wno-unused-function', '-Wno-unused-variable', '-Wno-unknown-pragmas']          # -O2 as the emulator build (csrc/Makefile)
    objs = []
    for u in UNITS:
        objs.append(str(tmp_path / (u + '.o')))
        subprocess.check_call(['g++'] + flags + ['-x', 'c++', '-c', os.path.join(csrc, u + '.cpp'), '-o', objs[-1]])
    exe = str(tmp_path / 'loop_probe')
    subprocess.check_call(['g++'] + flags + [os.path.join(ROOT, 'tests', 'host', 'loop_probe.cpp')] + objs + ['-o', exe, '-lm'])
    r = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert r.returncode == 0, r.stdout[-4000:]
    assert 'loop_probe: ok' in r.stdout
