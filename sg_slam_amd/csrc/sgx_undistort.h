// sgx_undistort.h — Frame::UndistortKeyPoints (src/sg-slam/src/Frame.cc:654-684) fused with Frame::ComputeStereoFromRGBD (:893-914), and the
// point undistortion they share with Frame::ComputeImageBounds (:686-714).
//
// sgx_undistort_point restates OpenCV 3.4.15's cvUndistortPointsInternal on the 32F point path as the reference reaches it,
// cv::undistortPoints(src, dst, K, D, noArray(), K) with the default TermCriteria(MAX_ITER, 5, 0.01): exactly five iterations, no EPS test,
// the icdist < 0 guard of OpenCV 3.4 (test undistortPoints.regression_14583).  R = I and P = K, so the RR / ww products reduce to fx * x + cx.
// Everything is fp64 with the float inputs promoted; the translation units are built with -ffp-contract=off and fp64 division is correctly rounded,
// so the device, the -DSGX_EMU emulator and a float64 numpy restatement give the same bits.
#pragma once
#include "sgx_rt.h"

#ifndef SGX_EMU
#define SGX_HD __host__ __device__ inline
#else
#define SGX_HD static inline
#endif

// k[0..11] = k1, k2, p1, p2, k3, k4, k5, k6, s1..s4 (the 4-, 5- or 8-coefficient vector padded with zeros); fx..cy: the float K of the settings file
struct SgxUndist {
    double k[12];
    float fx, fy, cx, cy;
    int on;                 // 0: mvKeysUn = mvKeys (the reference's k1 == 0 early-out, Frame.cc:656-660)
};

SGX_HD void sgx_undistort_point(float u_f, float v_f, float fx_f, float fy_f, float cx_f, float cy_f, const double *k, float *out_u, float *out_v)
{
    const double u = u_f, v = v_f, fx = fx_f, fy = fy_f, cx = cx_f, cy = cy_f;
    const double ifx = 1. / fx, ify = 1. / fy;
    double x = (u - cx) * ifx, y = (v - cy) * ify;
    const double x0 = x, y0 = y;
    for (int j = 0; j < 5; j++) {
        const double r2 = x * x + y * y;
        const double icdist = (1 + ((k[7] * r2 + k[6]) * r2 + k[5]) * r2) / (1 + ((k[4] * r2 + k[1]) * r2 + k[0]) * r2);
        if (icdist < 0) { x = (u - cx) * ifx; y = (v - cy) * ify; break; }
        const double deltaX = 2 * k[2] * x * y + k[3] * (r2 + 2 * x * x) + k[8] * r2 + k[9] * r2 * r2;
        const double deltaY = k[2] * (r2 + 2 * y * y) + 2 * k[3] * x * y + k[10] * r2 + k[11] * r2 * r2;
        x = (x0 - deltaX) * icdist;
        y = (y0 - deltaY) * icdist;
    }
    *out_u = (float)(fx * x + cx);
    *out_v = (float)(fy * y + cy);
}

// the padded coefficient vector of a 4-, 5- or 8-entry distortion vector (returns 0 for any other length)
SGX_HD int sgx_undistort_coeffs(const float *dist, int ndist, double *k)
{
    if (ndist != 4 && ndist != 5 && ndist != 8) return 0;
    for (int i = 0; i < 12; i++) k[i] = i < ndist ? (double)dist[i] : 0.0;
    return 1;
}

// ---------------------------------------------------------------------------------------------
// k_undistort_points: cv::undistortPoints(src, dst, K, D, noArray(), K) on n points (x, y float pairs), one thread per point
// ---------------------------------------------------------------------------------------------
SGX_KERNEL(256) k_undistort_points(int n, const float *pts, SgxUndist ud, float *out)
{
    SGX_THREADS_BEGIN(tid)
    const int i = (int)blockIdx.x * 256 + tid;
    if (i < n) sgx_undistort_point(pts[2 * i], pts[2 * i + 1], ud.fx, ud.fy, ud.cx, ud.cy, ud.k, &out[2 * i], &out[2 * i + 1]);
    SGX_THREADS_END
}

// ---------------------------------------------------------------------------------------------
// k_undistort_stereo_rgbd: Frame::UndistortKeyPoints + Frame::ComputeStereoFromRGBD, grid = (ceil(cap/256), batch), the layout of k_stereo_from_rgbd.
// keys_un[i] = keys[i] with pt replaced by the undistorted point (angle, octave, response, size keep their bits; rows >= n[f] are plain copies);
// the depth is read at the DISTORTED pixel ((int)kp.x, (int)kp.y) and uright = kpUn.x - bf / d (Frame.cc:899-912).  With ud.on == 0 keys_un is a
// byte copy of keys and uright / zdepth are those of k_stereo_from_rgbd.
// ---------------------------------------------------------------------------------------------
SGX_KERNEL(256) k_undistort_stereo_rgbd(int cap, const uint8_t *keys_raw, const int *n, const uint16_t *depth, int W, int H,
                                        float depth_factor_inv, float bf, SgxUndist ud, uint8_t *keys_un_raw, float *uright, float *zdepth)
{
    SGX_THREADS_BEGIN(tid)
    const int f = (int)blockIdx.y, i = (int)blockIdx.x * 256 + tid;
    if (i < cap) {
        const size_t o = (size_t)f * cap + i;
        const uint32_t *src = (const uint32_t *)(keys_raw + o * 28);
        uint32_t *dst = (uint32_t *)(keys_un_raw + o * 28);
        for (int j = 0; j < 7; j++) dst[j] = src[j];
        float ur = -1.f, z = -1.f;
        if (i < n[f]) {
            const float *kp = (const float *)src;
            float xu = kp[0], yu = kp[1];
            if (ud.on) {
                sgx_undistort_point(kp[0], kp[1], ud.fx, ud.fy, ud.cx, ud.cy, ud.k, &xu, &yu);
                float *dk = (float *)dst;
                dk[0] = xu; dk[1] = yu;
            }
            const int u = (int)kp[0], v = (int)kp[1];                    // cv::Mat::at<float>(float,float) truncates; the distorted pixel (Frame.cc:899-901)
            const float d = (float)depth[((size_t)f * H + v) * W + u] * depth_factor_inv;
            if (d > 0) { z = d; ur = xu - bf / d; }
        }
        uright[o] = ur; zdepth[o] = z;
    }
    SGX_THREADS_END
}
