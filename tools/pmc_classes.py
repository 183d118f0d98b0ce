"""Kernel name -> bench.py per-kernel class (the sgx_profile_* classes of sgx_prof.h), shared by the PMC post-processing tools."""
CLASS = [('k_pyramid', 'pyramid_resize'), ('k_resize', 'pyramid_resize'), ('k_gray_from_color', 'pyramid_resize'), ('k_fast_cells', 'fast_cells'), ('k_octree_keys', 'octree'), ('k_octree', 'octree'),
         ('k_blur_levels', 'orient_desc'), ('k_orient_desc', 'orient_desc'),
         ('k_stereo_from_rgbd', 'stereo_from_rgbd'), ('k_motion_model', 'motion_model'), ('k_match_project_frame', 'match_project_frame'),
         ('k_match_project_local', 'match_project_local'), ('k_pose_opt', 'pose_opt'), ('k_unproject', 'unproject'),
         ('k_make_map_points', 'map_point_glue'), ('k_merge_matches', 'map_point_glue'), ('k_gather_xw', 'map_point_glue'),
         ('k_dynamic_mask', 'dynamic_mask'), ('k_compact_keys', 'dynamic_mask'),
         ('k_lk_copy', 'lk_pyramid'), ('k_lk_pyr', 'lk_pyramid'), ('k_lk_track', 'lk_track'), ('k_fm_ransac', 'fm_ransac'),
         ('k_det_preprocess', 'det_forward'), ('k_stem_pre', 'det_forward'), ('k_conv_pw', 'det_forward'), ('k_conv_kxk', 'det_forward'), ('k_conv_dw', 'det_forward'), ('k_conv_stem', 'det_forward'), ('k_binary', 'det_forward'), ('k_unary', 'det_forward'),
         ('k_copy_into', 'det_forward'), ('k_permute_hwc_into', 'det_forward'), ('k_softmax_rows', 'det_forward'), ('k_fused_block', 'det_forward'),
         ('k_irb', 'det_forward'), ('k_se_gate', 'det_forward'),
         ('k_det_class_nms', 'det_output'), ('k_det_cut', 'det_output'), ('k_det_merge', 'det_output')]

# Membership rule behind the prefix table (VERDICT r3 weak #3a: k_irb / k_se_gate were added to the plan and fell into class None): every kernel DEFINED in one of the
# detector's kernel headers (sg_slam_amd/csrc/sgx_det*.h) that the table above does not name belongs to det_forward — a new plan kernel is classified by where it lives,
# not by somebody remembering this file.  tests/test_campaign_tools.py checks that every SGX_KERNEL of csrc/ gets a class.
import os as _os
import re as _re
_CSRC = _os.path.join(_os.path.dirname(_os.path.dirname(_os.path.abspath(__file__))), 'sg_slam_amd', 'csrc')


def source_kernels():
    """{kernel name: header file} of every SGX_KERNEL / SGX_KERNEL_OCC definition under sg_slam_amd/csrc"""
    out = {}
    try:
        for fn in sorted(_os.listdir(_CSRC)):
            if not fn.endswith(('.h', '.cpp')) or fn == 'sgx_rt.h': continue
            src = open(_os.path.join(_CSRC, fn)).read()
            for m in _re.finditer(r'SGX_KERNEL(?:_OCC)?\s*\((?:[^()]|\([^()]*\))*\)\s*(\w+)\s*\(', src):
                out[m.group(1)] = fn
            for m in _re.finditer(r'__global__\s+void(?:\s+__launch_bounds__\s*\([^)]*\))?(?:\s+__attribute__\s*\(\([^;{]*?\)\))?\s+(\w+)\s*\(', src):
                out[m.group(1)] = fn
    except OSError:
        pass
    return out


_DET_MEMBERS = sorted((k for k, f in source_kernels().items() if f.startswith('sgx_det')), key=len, reverse=True)
# kernels that are not part of the per-frame chain (runtime copies / fills, torch's own elementwise kernels in bench.py's set-up): never counted as "unclassified"
FOREIGN_PREFIXES = ('__amd_rocclr_', 'at::native::', 'void at::native::', 'ncclDevKernel', 'void rccl', 'rccl')


def classify(kernel_name):
    base = kernel_name.split('(')[0]
    if base.startswith('void '): base = base[5:]
    base = base.split('<')[0].strip()
    for pre, cls in CLASS:
        if base.startswith(pre):
            return cls
    for k in _DET_MEMBERS:
        if base.startswith(k):
            return 'det_forward'
    return None


def is_foreign(kernel_name):
    return kernel_name.startswith(FOREIGN_PREFIXES)


def unclassified_share(rows, name_key='Name', dur_key='TotalDurationNs'):
    """rows of a rocprofv3 kernel_stats table -> (share of the chain's kernel time in kernels without a class, their names); bench.py and the PMC tools refuse tables
    where this exceeds 1 % (a new kernel nobody told the classifier about silently corrupts every per-class figure)"""
    tot = 0.0; bad = 0.0; names = []
    for r in rows:
        if is_foreign(r[name_key]): continue
        d = float(r[dur_key]); tot += d
        if classify(r[name_key]) is None:
            bad += d; names.append(base_name(r[name_key]))
    return (bad / tot if tot else 0.0), sorted(set(names))


# dispatches per bench step of the kernels that run more than once per step (everything else: once); used to find out in how many of the profiled steps a class
# ran at all — the first step of a run has no previous frame, so the tracking-stage kernels (LK, RANSAC, matchers, pose optimisation ...) run in one step fewer
DISPATCHES_PER_STEP = {'k_pose_opt': 2, 'k_merge_matches': 2, 'k_resize': 7}


def steps_ran(dispatch_counts):
    """dispatch_counts: {kernel base name: dispatches} of ONE class -> number of steps in which the class ran"""
    best = 0.0
    for name, n in dispatch_counts.items():
        per = 1
        for pre, k in DISPATCHES_PER_STEP.items():
            if name.startswith(pre): per = k
        best = max(best, n / per)
    return max(1, int(round(best)))


def base_name(kernel_name):
    base = kernel_name.split('(')[0]
    if base.startswith('void '): base = base[5:]
    return base.split('<')[0].strip()
