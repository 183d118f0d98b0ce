"""Everything sgx_orb_create decides (sgx_orb_plan.h: geometry, FAST runs, blur tiles, resize tables, the fused-pyramid plan), read back through sgx_orb_debug_read_plan
for a matrix of geometries: the regression guard of the extractor's planner and of its uploads.

Handles are created and destroyed; no kernel is launched.  For every case the create status, a SHA-256 per section and a few readable integers must equal
tests/golden/orb_plans.json.  A planner change that is meant to change a plan updates the fixture on purpose:
    python tests/test_orb_plan.py            (records from the emulator)"""
import ctypes as C
import hashlib
import json
import os
import struct
import sys
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FIXTURE = os.path.join(ROOT, 'tests', 'golden', 'orb_plans.json')
SGX_ERR_UNSUPPORTED = -2
# width, height, nlevels, nfeatures, scaleFactor
CASES = ((640, 480, 8, 1000, 1.2),         # product geometry
         (1241, 376, 8, 2000, 1.2),        # width not a multiple of 4; the wide octree kernels
         (322, 242, 8, 1000, 1.2), (298, 226, 8, 1000, 1.2),      # orb_pyramid_cases.py
         (200, 136, 1, 1000, 1.2),         # one level, oct_maxlim above 256
         (64, 64, 1, 100, 1.2),            # smallest accepted
         (640, 480, 3, 1000, 1.5),
         (1280, 960, 2, 1000, 2.5),        # fused plan abandoned with more than one level: per-level k_resize launches
         (752, 480, 8, 1200, 1.2),         # a single-cell run above the LDS budget
         (203, 151, 8, 1000, 1.2), (100, 300, 1, 500, 1.2), (640, 480, 2, 3000, 1.2), (4000, 100, 2, 500, 1.2), (640, 480, 4, 1000, 2.0))      # refused
SECTIONS = ('geom', 'runs', 'blur_tiles', 'xtabs', 'ytabs', 'xgroups', 'yt_all', 'rects', 'pyr')      # section numbers of sgx_orb_debug_read_plan
GEOM_INTS = {'ncells': 4, 'nruns': 5, 'kp_cap': 6, 'fast_lds_bytes': 11, 'cand_pitch': 12, 'nblur_tiles': 14}      # int index in SgxOrbGeom
MAX_LEVELS = 12                 # SGX_MAX_LEVELS
PYR_INTS = {'pyr_tiles': 2 * MAX_LEVELS + 2, 'pyr_lds': 2 * MAX_LEVELS + 3, 'oct_maxlim': 2 * MAX_LEVELS + 4}      # after SgxPyrTabs { xoff[], yoff[], lds_a, lds_b }


def key_of(case):
    return '%dx%d levels=%d features=%d scale=%g' % case


def read_section(lib, h, section):
    read = lib.tap('sgx_orb_debug_read_plan')
    n = C.c_size_t(0)
    lib.check(read(h, section, None, 0, C.byref(n)))
    buf = (C.c_uint8 * max(1, n.value))()
    lib.check(read(h, section, buf, n.value, C.byref(n)))
    return bytes(buf[:n.value])


def plans_of(lib):
    from sg_slam_amd.capi import OrbConfig
    out = {}
    for case in CASES:
        w, hgt, nl, nf, sf = case
        cfg = OrbConfig(nfeatures=nf, scale_factor=sf, nlevels=nl, ini_th_fast=20, min_th_fast=7, width=w, height=hgt, max_batch=1)
        h = C.c_void_p(0xdead)          # must come back NULL when creation fails
        rec = {'status': int(lib.dll.sgx_orb_create(C.byref(cfg), C.byref(h)))}
        if rec['status'] == 0:
            try:
                blobs = [read_section(lib, h, s) for s in range(len(SECTIONS))]
            finally:
                lib.dll.sgx_orb_destroy(h)
            rec['sha256'] = {name: hashlib.sha256(b).hexdigest() for name, b in zip(SECTIONS, blobs)}
            assert len(blobs[8]) == (2 * MAX_LEVELS + 6) * 4 + 8
            for name, i in GEOM_INTS.items(): rec[name] = struct.unpack_from('<i', blobs[0], 4 * i)[0]
            for name, i in PYR_INTS.items(): rec[name] = struct.unpack_from('<i', blobs[8], 4 * i)[0]
        else:
            rec['out_is_null'] = not h.value
        out[key_of(case)] = rec
    return out


def check(lib):
    """one fixture for both builds: at the commit it was recorded from, the emulator and the device build gave the same bytes in every section"""
    fx = json.load(open(FIXTURE))
    got = plans_of(lib)
    assert sorted(got) == sorted(fx) and len(got) == len(CASES)
    for key, rec in got.items():
        if rec['status'] != 0:
            assert rec['status'] == SGX_ERR_UNSUPPORTED and rec.pop('out_is_null'), (key, rec)
        assert rec == fx[key], (key, {k: (v, fx[key].get(k)) for k, v in rec.items() if v != fx[key].get(k)})


def test_plans_equal_fixture_emu(emu):
    check(emu)


@pytest.mark.gpu
def test_plans_equal_fixture_gpu(gpulib_taps):
    check(gpulib_taps)


if __name__ == '__main__':
    sys.path.insert(0, ROOT)
    from sg_slam_amd.capi import SgxLib
    got = plans_of(SgxLib(sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, 'tests', 'emu', 'libsgx_emu.so')))
    for rec in got.values(): rec.pop('out_is_null', None)
    with open(sys.argv[2] if len(sys.argv) > 2 else FIXTURE, 'w') as f:
        f.write('{\n' + ',\n'.join('%s: %s' % (json.dumps(k), json.dumps(v, sort_keys=True)) for k, v in got.items()) + '\n}\n')
    print('%d cases, %d accepted' % (len(got), sum(r['status'] == 0 for r in got.values())))
