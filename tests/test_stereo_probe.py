"""CPU: tests/host/stereo_probe.cpp runs sgx_stereo_match_batch_dev over key sets off the image, on its borders, with NaN, infinities and octaves that are no level of
the pyramid, and over empty frames.  It and the emulator units it needs are built with AddressSanitizer (LeakSanitizer included) and UBSan, and its buffers have exactly
the documented sizes, so a window or a table row read outside its image, or a float converted to an integer it does not fit, ends the program: this is where the defined
cases of DESIGN 9g are shown to read nothing out of bounds.  A stand-alone program: nothing is loaded into Python."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
UNITS = ('sgx_orb', 'sgx_prof', 'sgx_stereo')


def test_stereo_probe_under_sanitizers(tmp_path):
    csrc = os.path.join(ROOT, 'sg_slam_amd', 'csrc')
    flags = ['-O2', '-g', '-std=c++17', '-ffp-contract=off', '-DSGX_EMU', '-DSGX_DEBUG_TAPS', '-fsanitize=address,undefined', '-fno-sanitize-recover=all',
             '-Wno-unused-function', '-Wno-unused-variable', '-Wno-unknown-pragmas']          # -O2 as the emulator build (csrc/Makefile)
    objs = []
    jobs = []
    for u in UNITS:
        objs.append(str(tmp_path / (u + '.o')))
        jobs.append(subprocess.Popen(['g++'] + flags + ['-x', 'c++', '-c', os.path.join(csrc, u + '.cpp'), '-o', objs[-1]]))
    assert [j.wait() for j in jobs] == [0] * len(jobs)
    exe = str(tmp_path / 'stereo_probe')
    subprocess.check_call(['g++'] + flags + [os.path.join(ROOT, 'tests', 'host', 'stereo_probe.cpp')] + objs + ['-o', exe, '-lm'])
    r = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert r.returncode == 0, r.stdout[-4000:]
    assert 'stereo_probe: ok' in r.stdout
