// sgx_poseopt.cpp — host side of the PoseOptimization C-ABI (include/sgx.h).
// Reference behaviour: src/sg-slam/src/Optimizer.cc:239-451.
// fp64 solver arithmetic: multiply-adds may fuse here.  The reference does NOT fuse them — g2o and sg-slam are built plain -O3 (Thirdparty/g2o/CMakeLists.txt:57,
// src/sg-slam/CMakeLists.txt:11-12; only DBoW2 has -march=native) — a deliberate divergence inside the stated tolerance (1e-5 relative on the pose, identical
// outlier flags), see sgx_ba.cpp.  -DSGX_FP_CONTRACT_OFF keeps the reference's rounding.  The bit-exact integer / fp32 feature kernels keep -ffp-contract=off.
#ifndef SGX_FP_CONTRACT_OFF
#pragma clang fp contract(fast)
#endif
#include "sgx_poseopt_kernels.h"
#include "sgx_host_args.h"
#include "sgx_prof.h"
#include "sgx_stage.h"
#include "../../include/sgx.h"
#ifdef SGX_DEBUG_TAPS
#include "../../include/sgx_debug.h"      // test / tuning taps: compiled into tests/taps/libsgx_taps.so and the emulator only
#endif
#include <stdio.h>
#include <string.h>
#include <vector>


static thread_local int g_po_threads = 0;      // tuning / test tap: 0 = default (256), 64 or 256 = force
SGX_TAP int sgx_pose_opt_debug_set_threads(int t) { if (t != 0 && t != 64 && t != 256) return SGX_ERR_INVALID; g_po_threads = t; return SGX_OK; }

extern "C" int sgx_pose_optimization_batch_dev(int batch, int cap, const sgx_keypoint *d_keys_un, const float *d_uright, const int32_t *d_n,
                                                const int32_t *d_mp_index, const uint8_t *d_has_mp, const float *d_mp_xw, int xw_pitch,
                                                const float *inv_level_sigma2, int nlevels, const sgx_camera *cam,
                                                float *d_Tcw, uint8_t *d_outlier, int32_t *d_n_inliers, void *stream)
{
    if (batch < 1 || cap < 1 || cap > SGX_PO_CAP || !d_keys_un || !d_uright || !d_n || (!d_mp_index && !d_has_mp) || !d_mp_xw || xw_pitch < 1 ||
        !inv_level_sigma2 || nlevels < 1 || nlevels > 12 || !cam || !d_Tcw || !d_outlier || !d_n_inliers) return SGX_ERR_INVALID;
    const SgxScales is2 = to_scales(inv_level_sigma2, nlevels);
    sgx_prof_begin(SGX_K_POSEOPT, (sgx_stream_t)stream);
    // threads per frame: four waves.  The one-wave variant (tap below) is kept for tuning: measured on MI355X it is 2x slower per launch at every
    // batch size (0.67 vs 0.35 ms at 64-256 frames, tools/bench_poseopt.py) because its 85 KB of LDS still limits a CU to one frame at a time.
    const int wide = g_po_threads ? (g_po_threads == 256) : 1;
    if (wide) { auto kfn = k_pose_opt<256>; SGX_LAUNCH(kfn, dim3(batch), dim3(256), (sgx_stream_t)stream, cap, (const uint8_t *)d_keys_un, d_uright, d_n,
                                                       d_mp_index, d_has_mp, d_mp_xw, xw_pitch, is2, to_cam(cam), d_Tcw, d_outlier, d_n_inliers); }
    else { auto kfn = k_pose_opt<64>; SGX_LAUNCH(kfn, dim3(batch), dim3(64), (sgx_stream_t)stream, cap, (const uint8_t *)d_keys_un, d_uright, d_n,
                                                 d_mp_index, d_has_mp, d_mp_xw, xw_pitch, is2, to_cam(cam), d_Tcw, d_outlier, d_n_inliers); }
    sgx_prof_end(SGX_K_POSEOPT, (sgx_stream_t)stream);
    SGX_CHECK_HIP(hipGetLastError());
    return SGX_OK;
}

// Host pointers, one frame: the drop-in for `int Optimizer::PoseOptimization(Frame *pFrame)`.
extern "C" int sgx_pose_optimization(int n, const sgx_keypoint *keys_un, const float *uright, const uint8_t *has_mp, const float *mp_xw,
                                      const float *inv_level_sigma2, int nlevels, const sgx_camera *cam,
                                      float *Tcw, uint8_t *outlier, int32_t *n_inliers)
{
    if (n < 0 || n > SGX_PO_CAP || !Tcw || !outlier || !n_inliers || !cam || !inv_level_sigma2 || nlevels < 1) return SGX_ERR_INVALID;
    if (n > 0 && (!keys_un || !uright || !has_mp || !mp_xw)) return SGX_ERR_INVALID;      // a NULL source would leave the staging slot's previous contents in place
    const int cap = n > 0 ? n : 1;
    SgxStaging st(SGX_STAGE_POSE_OPT);                     // with n == 0 the frame's arrays are empty slots: the kernel's loops end at *d_n
    const sgx_keypoint *d_keys = st.in(keys_un, n); const float *d_uright = st.in(uright, n); const int32_t *d_n = st.in(&n, 1);
    const uint8_t *d_has = st.in(has_mp, n); const float *d_xw = st.in(mp_xw, (size_t)n * 3);
    float *d_Tcw = st.inout(Tcw, 16); uint8_t *d_outlier = st.out<uint8_t>(n); int32_t *d_nin = st.out<int32_t>(1);
    if (st.rc == SGX_OK) st.hip(hipStreamSynchronize(0));     // &n is a stack variable
    if (st.rc != SGX_OK) return st.rc;
    const int rc = sgx_pose_optimization_batch_dev(1, cap, d_keys, d_uright, d_n, nullptr, d_has, d_xw, cap, inv_level_sigma2, nlevels, cam, d_Tcw, d_outlier, d_nin, nullptr);
    if (rc != SGX_OK) return rc;
    st.back(Tcw, d_Tcw, 16); st.back(outlier, d_outlier, n); st.back(n_inliers, d_nin, 1);
    return st.rc;
}

