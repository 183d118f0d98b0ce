// sgx_match.cpp — host side of the matcher / frame-glue C-ABI (include/sgx.h).
// Reference behaviour: src/sg-slam/src/ORBmatcher.cc:1332-1472, src/sg-slam/src/Frame.cc:893-932.
#include "sgx_match_kernels.h"
#include "sgx_host_args.h"
#include "sgx_prof.h"
#include "sgx_stage.h"
#include "../../include/sgx.h"
#ifdef SGX_DEBUG_TAPS
#include "../../include/sgx_debug.h"      // test / tuning taps: compiled into tests/taps/libsgx_taps.so and the emulator only
#endif
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <vector>


extern "C" int sgx_match_project_frame_batch_dev(
    int batch, int cap,
    const sgx_keypoint *d_ckeys, const uint8_t *d_cdesc, const float *d_curight, const int32_t *d_cn, const float *d_cTcw,
    const sgx_keypoint *d_lkeys, const int32_t *d_ln, const uint8_t *d_l_has_mp, const uint8_t *d_l_outlier, const float *d_l_xw,
    const int32_t *d_l_obs, const uint8_t *d_l_mpdesc, const float *d_lTcw,
    const sgx_camera *cam, const float *scale_factors, int nlevels, float th, int b_mono, int check_orientation,
    int32_t *d_cur_match, int32_t *d_nmatches, void *stream)
{
    if (batch < 1 || cap < 1 || cap > SGX_MATCH_CAP || !cam || !scale_factors || nlevels < 1 || nlevels > 12) return SGX_ERR_INVALID;
    if (!d_ckeys || !d_cdesc || !d_curight || !d_cn || !d_cTcw || !d_lkeys || !d_ln || !d_l_has_mp || !d_l_outlier || !d_l_xw ||
        !d_l_obs || !d_l_mpdesc || !d_lTcw || !d_cur_match || !d_nmatches) return SGX_ERR_INVALID;
    const SgxScales sc = to_scales(scale_factors, nlevels);
    sgx_prof_begin(SGX_K_MATCH, (sgx_stream_t)stream);
    static const int mthreads = sgx_getenv("SGX_TUNE_MATCH_THREADS") ? atoi(sgx_getenv("SGX_TUNE_MATCH_THREADS")) : SGX_MATCH_THREADS;   // env = tuning tap (64..1024)
    SGX_LAUNCH(k_match_project_frame, dim3(batch), dim3(mthreads), (sgx_stream_t)stream, cap,
               (const uint8_t *)d_ckeys, d_cdesc, d_curight, d_cn, d_cTcw, (const uint8_t *)d_lkeys, d_ln, d_l_has_mp, d_l_outlier,
               d_l_xw, d_l_obs, d_l_mpdesc, d_lTcw, to_cam(cam), sc, th, b_mono, check_orientation, d_cur_match, d_nmatches);
    sgx_prof_end(SGX_K_MATCH, (sgx_stream_t)stream);
    SGX_CHECK_HIP(hipGetLastError());
    return SGX_OK;
}

extern "C" int sgx_frame_stereo_from_rgbd_batch_dev(int batch, int cap, const sgx_keypoint *d_keys, const int32_t *d_n,
                                                     const uint16_t *d_depth, int width, int height, float depth_map_factor,
                                                     float bf, float *d_uright, float *d_zdepth, void *stream)
{
    if (batch < 1 || cap < 1 || !d_keys || !d_n || !d_depth || !d_uright || !d_zdepth || !(depth_map_factor > 0)) return SGX_ERR_INVALID;
    const float inv = 1.0f / depth_map_factor;           // mDepthMapFactor = 1.0f/mDepthMapFactor, Tracking.cc:139-142
    sgx_prof_begin(SGX_K_STEREO, (sgx_stream_t)stream);
    SGX_LAUNCH(k_stereo_from_rgbd, dim3((cap + 255) / 256, batch), dim3(256), (sgx_stream_t)stream, cap, (const uint8_t *)d_keys, d_n,
               d_depth, width, height, inv, bf, d_uright, d_zdepth);
    sgx_prof_end(SGX_K_STEREO, (sgx_stream_t)stream);
    SGX_CHECK_HIP(hipGetLastError());
    return SGX_OK;
}

extern "C" int sgx_frame_unproject_batch_dev(int batch, int cap, const sgx_keypoint *d_keys, const int32_t *d_n, const float *d_zdepth,
                                              const float *d_Tcw, const sgx_camera *cam, float *d_xw, uint8_t *d_has, void *stream)
{
    if (batch < 1 || cap < 1 || !d_keys || !d_n || !d_zdepth || !d_Tcw || !cam || !d_xw || !d_has) return SGX_ERR_INVALID;
    sgx_prof_begin(SGX_K_UNPROJECT, (sgx_stream_t)stream);
    SGX_LAUNCH(k_unproject, dim3((cap + 255) / 256, batch), dim3(256), (sgx_stream_t)stream, cap, (const uint8_t *)d_keys, d_n, d_zdepth,
               d_Tcw, to_cam(cam), d_xw, d_has);
    sgx_prof_end(SGX_K_UNPROJECT, (sgx_stream_t)stream);
    SGX_CHECK_HIP(hipGetLastError());
    return SGX_OK;
}

extern "C" int sgx_match_project_local_batch_dev(
    int batch, int cap, const sgx_keypoint *d_ckeys, const uint8_t *d_cdesc, const float *d_curight, const int32_t *d_cn, const float *d_cTcw, const int32_t *d_cur_mp_obs,
    int mcap, const int32_t *d_mn, const float *d_m_xw, const float *d_m_normal, const float *d_m_min_dist, const float *d_m_max_dist, const uint8_t *d_m_desc,
    const int32_t *d_m_obs, const uint8_t *d_m_skip,
    const sgx_camera *cam, const float *scale_factors, int nlevels, float log_scale_factor, float th, float nnratio, float viewing_cos_limit,
    int32_t *d_cur_match, int32_t *d_nmatches, uint8_t *d_in_view, void *stream)
{
    if (batch < 1 || cap < 1 || cap > SGX_MATCH_CAP || mcap < 1 || mcap > SGX_LOCAL_CAP || !cam || !scale_factors || nlevels < 1 || nlevels > 12) return SGX_ERR_INVALID;
    if (!d_ckeys || !d_cdesc || !d_curight || !d_cn || !d_cTcw || !d_mn || !d_m_xw || !d_m_normal || !d_m_min_dist || !d_m_max_dist || !d_m_desc || !d_m_obs ||
        !d_m_skip || !d_cur_match || !d_nmatches || !d_in_view) return SGX_ERR_INVALID;
    const SgxScales sc = to_scales(scale_factors, nlevels);
    sgx_prof_begin(SGX_K_MATCH_LOCAL, (sgx_stream_t)stream);
    SGX_LAUNCH(k_match_project_local, dim3(batch), dim3(SGX_MATCH_THREADS), (sgx_stream_t)stream, cap, (const uint8_t *)d_ckeys, d_cdesc, d_curight, d_cn, d_cTcw,
               d_cur_mp_obs, mcap, d_mn, d_m_xw, d_m_normal, d_m_min_dist, d_m_max_dist, d_m_desc, d_m_obs, d_m_skip, to_cam(cam), sc, nlevels, log_scale_factor,
               th, nnratio, viewing_cos_limit, d_cur_match, d_nmatches, d_in_view);
    sgx_prof_end(SGX_K_MATCH_LOCAL, (sgx_stream_t)stream);
    SGX_CHECK_HIP(hipGetLastError());
    return SGX_OK;
}

extern "C" int sgx_frame_make_map_points_batch_dev(int batch, int cap, int half, const sgx_keypoint *d_keys, const int32_t *d_n, const float *d_xw, const uint8_t *d_has,
                                                    const uint8_t *d_desc, const float *d_Tcw, const float *scale_factors, int nlevels,
                                                    float *d_m_xw, float *d_m_normal, float *d_m_min_dist, float *d_m_max_dist, uint8_t *d_m_desc, uint8_t *d_m_skip, void *stream)
{
    if (batch < 1 || cap < 1 || half < 0 || half > 1 || !d_keys || !d_n || !d_xw || !d_has || !d_desc || !d_Tcw || !scale_factors || nlevels < 1 || nlevels > 12 ||
        !d_m_xw || !d_m_normal || !d_m_min_dist || !d_m_max_dist || !d_m_desc || !d_m_skip) return SGX_ERR_INVALID;
    const SgxScales sc = to_scales(scale_factors, nlevels);
    sgx_prof_begin(SGX_K_MAPGLUE, (sgx_stream_t)stream);
    SGX_LAUNCH(k_make_map_points, dim3((cap + 255) / 256, batch), dim3(256), (sgx_stream_t)stream, cap, half, (const uint8_t *)d_keys, d_n, d_xw, d_has, d_desc, d_Tcw, sc, nlevels,
               d_m_xw, d_m_normal, d_m_min_dist, d_m_max_dist, d_m_desc, d_m_skip);
    sgx_prof_end(SGX_K_MAPGLUE, (sgx_stream_t)stream);
    SGX_CHECK_HIP(hipGetLastError());
    return SGX_OK;
}

extern "C" int sgx_frame_merge_matches_batch_dev(int batch, int cap, const int32_t *d_n, const int32_t *d_match_last, const uint8_t *d_outlier_last, const int32_t *d_match_local,
                                                  const float *d_xw_last, const float *d_m_xw, int32_t *d_merged, int32_t *d_cur_mp_obs, float *d_xw_all, void *stream)
{
    if (batch < 1 || cap < 1 || !d_n || !d_match_last || !d_outlier_last) return SGX_ERR_INVALID;
    sgx_prof_begin(SGX_K_MAPGLUE, (sgx_stream_t)stream);
    SGX_LAUNCH(k_merge_matches, dim3((cap + 255) / 256, batch), dim3(256), (sgx_stream_t)stream, cap, d_n, d_match_last, d_outlier_last, d_match_local, d_merged, d_cur_mp_obs);
    if (d_xw_all && d_xw_last && d_m_xw)
        SGX_LAUNCH(k_gather_xw, dim3((3 * cap + 255) / 256, batch), dim3(256), (sgx_stream_t)stream, cap, d_xw_last, d_m_xw, d_xw_all);
    sgx_prof_end(SGX_K_MAPGLUE, (sgx_stream_t)stream);
    SGX_CHECK_HIP(hipGetLastError());
    return SGX_OK;
}

extern "C" int sgx_frame_motion_model_batch_dev(int batch, const float *d_Tcw_cur, const float *d_Tcw_prev, const uint8_t *d_valid, float *d_Tcw_pred, void *stream)
{
    if (batch < 1 || !d_Tcw_cur || !d_Tcw_prev || !d_Tcw_pred) return SGX_ERR_INVALID;
    sgx_prof_begin(SGX_K_MOTION, (sgx_stream_t)stream);
    SGX_LAUNCH(k_motion_model, dim3((batch + 63) / 64), dim3(64), (sgx_stream_t)stream, batch, d_Tcw_cur, d_Tcw_prev, d_valid, d_Tcw_pred);
    sgx_prof_end(SGX_K_MOTION, (sgx_stream_t)stream);
    SGX_CHECK_HIP(hipGetLastError());
    return SGX_OK;
}

// Host-pointer, single pair: the drop-in for ORBmatcher::SearchByProjection(Frame&, const Frame&, th, bMono).
// Device staging of the host-pointer entries: per-thread slots that persist from call to call; this entry, sgx_match_project_local and sgx_pose_optimization
// each have a slot range of their own (SGX_STAGE_*, sgx_stage.h).
extern "C" int sgx_match_project_frame(
    int nc, const sgx_keypoint *ckeys, const uint8_t *cdesc, const float *curight, const float *cTcw,
    int nl, const sgx_keypoint *lkeys, const uint8_t *l_has_mp, const uint8_t *l_outlier, const float *l_xw,
    const int32_t *l_obs, const uint8_t *l_mpdesc, const float *lTcw,
    const sgx_camera *cam, const float *scale_factors, int nlevels, float th, int b_mono, int check_orientation,
    int32_t *cur_match, int32_t *nmatches)
{
    if (nc < 0 || nl < 0 || nc > SGX_MATCH_CAP || nl > SGX_MATCH_CAP || !cur_match || !nmatches || !cTcw || !lTcw || !cam || !scale_factors || nlevels < 1) return SGX_ERR_INVALID;
    if (nc > 0 && (!ckeys || !cdesc || !curight)) return SGX_ERR_INVALID;
    if (nl > 0 && (!lkeys || !l_has_mp || !l_outlier || !l_xw || !l_obs || !l_mpdesc)) return SGX_ERR_INVALID;
    int cap = nc > nl ? nc : nl; if (cap < 1) cap = 1;
    SgxStaging st(SGX_STAGE_FRAME_MATCH);
    // the kernel reads `cap` elements of every array: each is zero-padded to cap through one host vector, so every upload has to finish before the next overwrites it
    std::vector<uint8_t> pad;
    auto padded = [&](auto *src, int per, int n) {
        const size_t elem = (size_t)per * sizeof *src;
        pad.assign((size_t)cap * elem, 0);
        if (n > 0 && src) memcpy(pad.data(), src, (size_t)n * elem);
        const uint8_t *d = st.in(pad.data(), pad.size());
        if (st.rc == SGX_OK) st.hip(hipStreamSynchronize(0));
        return (decltype(src))d;
    };
    const sgx_keypoint *d_ckeys = padded(ckeys, 1, nc); const uint8_t *d_cdesc = padded(cdesc, 32, nc); const float *d_curight = padded(curight, 1, nc);
    const sgx_keypoint *d_lkeys = padded(lkeys, 1, nl); const uint8_t *d_has = padded(l_has_mp, 1, nl), *d_outlier = padded(l_outlier, 1, nl);
    const float *d_lxw = padded(l_xw, 3, nl); const int32_t *d_lobs = padded(l_obs, 1, nl); const uint8_t *d_mpdesc = padded(l_mpdesc, 32, nl);
    const int32_t *d_nc = st.in(&nc, 1), *d_nl = st.in(&nl, 1);
    const float *d_cTcw = st.in(cTcw, 16), *d_lTcw = st.in(lTcw, 16);
    int32_t *d_match = st.out<int32_t>(cap), *d_nmatches = st.out<int32_t>(1);
    if (st.rc != SGX_OK) return st.rc;
    SGX_CHECK_HIP(hipStreamSynchronize(0));
    const int rc = sgx_match_project_frame_batch_dev(1, cap, d_ckeys, d_cdesc, d_curight, d_nc, d_cTcw, d_lkeys, d_nl, d_has, d_outlier, d_lxw, d_lobs, d_mpdesc, d_lTcw,
                                                     cam, scale_factors, nlevels, th, b_mono, check_orientation, d_match, d_nmatches, nullptr);
    if (rc != SGX_OK) return rc;
    st.back(cur_match, d_match, nc); st.back(nmatches, d_nmatches, 1);
    return st.rc;
}

// Host pointers, one frame: the drop-in for Tracking::SearchLocalPoints' isInFrustum loop + ORBmatcher::SearchByProjection(Frame &F, vpMapPoints, th).
extern "C" int sgx_match_project_local(
    int nc, const sgx_keypoint *ckeys, const uint8_t *cdesc, const float *curight, const float *cTcw, const int32_t *cur_mp_obs,
    int nm, const float *m_xw, const float *m_normal, const float *m_min_dist, const float *m_max_dist, const uint8_t *m_desc, const int32_t *m_obs, const uint8_t *m_skip,
    const sgx_camera *cam, const float *scale_factors, int nlevels, float log_scale_factor, float th, float nnratio, float viewing_cos_limit,
    int32_t *cur_match, int32_t *nmatches, uint8_t *in_view)
{
    if (nc < 0 || nm < 0 || nc > SGX_MATCH_CAP || nm > SGX_LOCAL_CAP || !cur_match || !nmatches || !cTcw || !cam || !scale_factors) return SGX_ERR_INVALID;
    for (int i = 0; i < nc; i++) cur_match[i] = -1;
    if (in_view) memset(in_view, 0, (size_t)nm);
    *nmatches = 0;
    if (nc == 0 || nm == 0) return SGX_OK;                       // the reference's loops do not execute (ORBmatcher.cc:52-127)
    std::vector<int32_t> no_obs;
    if (!cur_mp_obs) { no_obs.assign((size_t)nc, -1); cur_mp_obs = no_obs.data(); }
    SgxStaging st(SGX_STAGE_LOCAL_MATCH);
    const sgx_keypoint *d_ckeys = st.in(ckeys, nc); const uint8_t *d_cdesc = st.in(cdesc, (size_t)nc * 32); const float *d_curight = st.in(curight, nc);
    const int32_t *d_nc = st.in(&nc, 1); const float *d_cTcw = st.in(cTcw, 16); const int32_t *d_obs = st.in(cur_mp_obs, nc);
    const int32_t *d_nm = st.in(&nm, 1); const float *d_xw = st.in(m_xw, (size_t)nm * 3), *d_normal = st.in(m_normal, (size_t)nm * 3);
    const float *d_min = st.in(m_min_dist, nm), *d_max = st.in(m_max_dist, nm);
    const uint8_t *d_mdesc = st.in(m_desc, (size_t)nm * 32); const int32_t *d_mobs = st.in(m_obs, nm); const uint8_t *d_skip = st.in(m_skip, nm);
    int32_t *d_match = st.out<int32_t>(nc), *d_nmatches = st.out<int32_t>(1); uint8_t *d_in_view = st.out<uint8_t>(nm);
    if (st.rc != SGX_OK) return st.rc;
    SGX_CHECK_HIP(hipStreamSynchronize(0));
    const int rc = sgx_match_project_local_batch_dev(1, nc, d_ckeys, d_cdesc, d_curight, d_nc, d_cTcw, d_obs, nm, d_nm, d_xw, d_normal, d_min, d_max, d_mdesc, d_mobs, d_skip,
                                                     cam, scale_factors, nlevels, log_scale_factor, th, nnratio, viewing_cos_limit, d_match, d_nmatches, d_in_view, nullptr);
    if (rc != SGX_OK) return rc;
    st.back(cur_match, d_match, nc); st.back(nmatches, d_nmatches, 1);
    if (in_view) st.back(in_view, d_in_view, nm);
    return st.rc;
}

extern "C" int sgx_frame_gray_from_color_batch_dev(int batch, int width, int height, const uint8_t *d_src, int src_pitch, int channels, int blue_first,
                                                   uint8_t *d_gray, int gray_pitch, void *stream)
{
    if (batch < 1 || width < 1 || height < 1 || !d_src || !d_gray || (channels != 3 && channels != 4) || src_pitch < width * channels || gray_pitch < width ||
        (src_pitch & 3) || (gray_pitch & 3) || ((uintptr_t)d_src & 3) || ((uintptr_t)d_gray & 3)) return SGX_ERR_INVALID;
    SGX_LAUNCH(k_gray_from_color, dim3((width + 255) / 256, height, batch), dim3(64), (sgx_stream_t)stream, width, height, d_src, src_pitch, channels, blue_first ? 1 : 0, d_gray, gray_pitch);
    SGX_CHECK_HIP(hipGetLastError());
    return SGX_OK;
}

SGX_TAP int sgx_debug_flow_affine_batch_dev(int batch, int cap, const sgx_keypoint *d_keys, const int32_t *d_n, const float *d_A, const float *d_shift, const float *d_boxes,
                                               int max_boxes, float *d_prev_xy, void *stream)
{
    if (batch < 1 || cap < 1 || !d_keys || !d_n || !d_A || !d_prev_xy) return SGX_ERR_INVALID;
    SGX_LAUNCH(k_flow_affine, dim3((cap + 255) / 256, batch), dim3(256), (sgx_stream_t)stream, cap, (const uint8_t *)d_keys, d_n, d_A, d_shift, d_boxes, max_boxes, d_prev_xy);
    SGX_CHECK_HIP(hipGetLastError());
    return SGX_OK;
}
