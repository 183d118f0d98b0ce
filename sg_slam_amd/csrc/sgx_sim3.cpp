// sgx_sim3.cpp — host side of Optimizer::OptimizeSim3 (include/sgx.h: sgx_optimize_sim3).  Reference: src/sg-slam/src/Optimizer.cc:1046-1257.
#include "sgx_sim3_kernels.h"
#include "sgx_stage.h"
#include "../../include/sgx.h"
#ifdef SGX_DEBUG_TAPS
#include "../../include/sgx_debug.h"      // test / tuning taps: compiled into tests/taps/libsgx_taps.so and the emulator only
#endif
#include <stdio.h>
#include <string.h>


extern "C" int sgx_optimize_sim3(int n, const float *p1c, const float *p2c, const float *obs1, const float *obs2, const float *info1, const float *info2,
                                 const float *K1, const float *K2, double *S12, float th2, int fix_scale, uint8_t *inlier, int32_t *iterations, int32_t *n_inliers)
{
    if (n < 0 || !K1 || !K2 || !S12 || !n_inliers || (n > 0 && (!p1c || !p2c || !obs1 || !obs2 || !info1 || !info2 || !inlier))) return SGX_ERR_INVALID;
    *n_inliers = 0;
    if (iterations) { iterations[0] = 0; iterations[1] = 0; }
    if (n < 10) {                                          // with fewer than 10 correspondences the reference optimises 5 iterations and then returns 0 without reading the estimate back:
        for (int i = 0; i < n; i++) inlier[i] = 1;          // nothing observable changes except vpMatches1 entries NULLed by the first check — run the kernel only when n >= 1 to get those flags
        if (n == 0) return SGX_OK;
    }
    SgxSim3Args A; memset(&A, 0, sizeof A);
    A.n = n; A.fix_scale = fix_scale ? 1 : 0; A.th2 = th2;
    for (int i = 0; i < 4; i++) { A.K1[i] = K1[i]; A.K2[i] = K2[i]; }
    SgxStaging st(SGX_STAGE_SHARED);
    A.p1c = st.in(p1c, (size_t)n * 3); A.p2c = st.in(p2c, (size_t)n * 3); A.obs1 = st.in(obs1, (size_t)n * 2); A.obs2 = st.in(obs2, (size_t)n * 2); A.info1 = st.in(info1, n); A.info2 = st.in(info2, n);
    A.S12 = st.inout(S12, 8); A.err = st.out<double>((size_t)n * 4); A.inlier = st.out<uint8_t>(n); A.iters = st.out<int>(2); A.nin = st.out<int>(1);
    if (st.rc != SGX_OK) return st.rc;
    SGX_LAUNCH(k_optimize_sim3, dim3(1), dim3(256), (sgx_stream_t)0, A);
    SGX_CHECK_HIP(hipGetLastError());
    int nin = 0, its[2] = { 0, 0 };
    st.back(&nin, A.nin, 1); st.back(its, A.iters, 2); st.back(inlier, A.inlier, n);
    if (st.rc == SGX_OK && (nin > 0 || its[1] > 0)) st.back(S12, A.S12, 8);     // the "fewer than 10 survivors" exit leaves g2oS12 untouched
    if (st.rc != SGX_OK) return st.rc;
    *n_inliers = nin;
    if (iterations) { iterations[0] = its[0]; iterations[1] = its[1]; }
    return SGX_OK;
}
