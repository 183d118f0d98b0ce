// sgx_undistort.cpp — host side of the lens-distortion entries (include/sgx.h): cv::undistortPoints as Frame::UndistortKeyPoints calls it,
// the fused undistort + stereo-from-RGBD stage, and Frame::ComputeImageBounds.
// Reference behaviour: src/sg-slam/src/Frame.cc:654-714, :893-914; the coefficient hand-over Tracking.cc:66-77.
#include "sgx_undistort.h"
#include "sgx_prof.h"
#include "../../include/sgx.h"
#include <stdio.h>
#include <string.h>


static int make_undist(const float *K4, const float *dist, int ndist, int on, SgxUndist *ud)
{
    memset(ud, 0, sizeof *ud);
    if (!sgx_undistort_coeffs(dist, ndist, ud->k)) return SGX_ERR_INVALID;
    ud->fx = K4[0]; ud->fy = K4[1]; ud->cx = K4[2]; ud->cy = K4[3]; ud->on = on;
    return SGX_OK;
}

// cv::undistortPoints(src, dst, K, D, noArray(), K) on host points, computed on the device.  No k1 == 0 shortcut here: OpenCV itself always iterates.
extern "C" int sgx_undistort_points(int n, const float *pts, const float *K4, const float *dist, int ndist, float *out)
{
    if (n < 0 || !K4 || !dist) return SGX_ERR_INVALID;
    SgxUndist ud;
    if (make_undist(K4, dist, ndist, 1, &ud) != SGX_OK) return SGX_ERR_INVALID;
    if (n == 0) return SGX_OK;
    if (!pts || !out) return SGX_ERR_INVALID;
    void *d_in = nullptr, *d_out = nullptr;
    const size_t bytes = (size_t)n * 8;
    int rc = SGX_OK;
    if (hipMalloc(&d_in, bytes) != hipSuccess || hipMalloc(&d_out, bytes) != hipSuccess) rc = SGX_ERR_NOMEM;
    else if (hipMemcpy(d_in, pts, bytes, hipMemcpyHostToDevice) != hipSuccess) rc = SGX_ERR_DEVICE;
    else {
        SGX_LAUNCH(k_undistort_points, dim3((unsigned)((n + 255) / 256)), dim3(256), (sgx_stream_t)0, n, (const float *)d_in, ud, (float *)d_out);
        if (hipGetLastError() != hipSuccess || hipMemcpy(out, d_out, bytes, hipMemcpyDeviceToHost) != hipSuccess) rc = SGX_ERR_DEVICE;
    }
    if (d_in) (void)hipFree(d_in);
    if (d_out) (void)hipFree(d_out);
    return rc;
}

// Frame::UndistortKeyPoints + Frame::ComputeStereoFromRGBD for a batch of frames on the device (one launch).  dist[0] == 0 is the reference's early-out
// (Frame.cc:656-660): keys_un is a byte copy of keys, whatever the other coefficients are.
extern "C" int sgx_frame_undistort_stereo_rgbd_batch_dev(int batch, int cap, const sgx_keypoint *d_keys, const int32_t *d_n, const float *dist, int ndist,
                                                          const sgx_camera *cam, const uint16_t *d_depth, int width, int height, float depth_map_factor,
                                                          sgx_keypoint *d_keys_un, float *d_uright, float *d_zdepth, void *stream)
{
    if (batch < 1 || cap < 1 || !d_keys || !d_n || !dist || !cam || !d_depth || !d_keys_un || !d_uright || !d_zdepth || !(depth_map_factor > 0)) return SGX_ERR_INVALID;
    const float K4[4] = { cam->fx, cam->fy, cam->cx, cam->cy };
    SgxUndist ud;
    if (make_undist(K4, dist, ndist, dist[0] != 0.0f, &ud) != SGX_OK) return SGX_ERR_INVALID;
    const float inv = 1.0f / depth_map_factor;           // mDepthMapFactor = 1.0f/mDepthMapFactor, Tracking.cc:139-142
    sgx_prof_begin(SGX_K_STEREO, (sgx_stream_t)stream);
    SGX_LAUNCH(k_undistort_stereo_rgbd, dim3((cap + 255) / 256, batch), dim3(256), (sgx_stream_t)stream, cap, (const uint8_t *)d_keys, d_n,
               d_depth, width, height, inv, cam->bf, ud, (uint8_t *)d_keys_un, d_uright, d_zdepth);
    sgx_prof_end(SGX_K_STEREO, (sgx_stream_t)stream);
    SGX_CHECK_HIP(hipGetLastError());
    return SGX_OK;
}

// Frame::ComputeImageBounds (Frame.cc:686-714): min_x..max_y from the undistorted corners (0,0), (cols,0), (0,rows), (cols,rows); 0, cols, 0, rows when
// dist[0] == 0.  The other fields of *cam are left as they are.
extern "C" int sgx_frame_image_bounds(int width, int height, const float *K4, const float *dist, int ndist, sgx_camera *cam)
{
    if (width < 1 || height < 1 || !K4 || !dist || !cam || (ndist != 4 && ndist != 5 && ndist != 8)) return SGX_ERR_INVALID;
    if (dist[0] == 0.0f) {
        cam->min_x = 0.0f; cam->max_x = (float)width; cam->min_y = 0.0f; cam->max_y = (float)height;
        return SGX_OK;
    }
    const float W = (float)width, H = (float)height;
    const float corners[8] = { 0.0f, 0.0f, W, 0.0f, 0.0f, H, W, H };
    float m[8];
    const int rc = sgx_undistort_points(4, corners, K4, dist, ndist, m);
    if (rc != SGX_OK) return rc;
    cam->min_x = m[4] < m[0] ? m[4] : m[0];            // std::min(mat(0,0), mat(2,0)) = b < a ? b : a
    cam->max_x = m[2] < m[6] ? m[6] : m[2];            // std::max(mat(1,0), mat(3,0)) = a < b ? b : a
    cam->min_y = m[3] < m[1] ? m[3] : m[1];            // min(mat(0,1), mat(1,1))
    cam->max_y = m[5] < m[7] ? m[7] : m[5];            // max(mat(2,1), mat(3,1))
    return SGX_OK;
}
