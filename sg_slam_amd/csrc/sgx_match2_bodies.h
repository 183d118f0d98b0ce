// sgx_match2_bodies.h — the device bodies and argument structs that more than one translation unit runs: SearchForTriangulation's node loop, the per-pair body of
// LocalMapping::CreateNewMapPoints and the two MapPoint post-steps.  sgx_match2_kernels.h wraps them in the kernels of the host-pointer entries (sgx_match2.cpp),
// sgx_newpoints_kernels.h in k_create_new_map_points (sgx_newpoints.cpp).  No kernel is defined here: a kernel has one home, so the units link.
#pragma once
#include "sgx_match_common.h"
#include <float.h>

#define SGX_TH_LOW 50             /* ORBmatcher::TH_LOW, ORBmatcher.cc:38 */

struct SgxTriArgs {
    int n1, n2, nnodes;                      /* keypoints of KF1 / KF2, common vocabulary nodes */
    const uint8_t *keys1, *keys2;            /* mvKeysUn (28-byte cv::KeyPoint) */
    const uint32_t *desc1, *desc2;
    const float *uright1, *uright2;
    const uint8_t *has_mp1, *has_mp2;        /* GetMapPoint(idx) != NULL */
    const int *items1, *items2;              /* feature indices grouped by node (FeatureVector order) */
    const int *job;                          /* per common node: start1, end1, start2, end2 into items1 / items2 */
    float F12[9];                            /* row-major */
    float ex, ey;                            /* epipole of KF1's centre in KF2 */
    SgxScales scale2, sigma2_2;              /* pKF2->mvScaleFactors, pKF2->mvLevelSigma2 */
    int only_stereo, check_ori;
    int *match12;                            /* out: n1 entries, index in KF2 or -1 */
    uint8_t *matched2;                       /* work: n2 flags */
    int *nmatches;
};

// GetMapPoint(idx) != NULL, from a flag array (the host-pointer entry) or from a mvpMapPoints row of point ids, -1 none (sgx_create_new_map_points_batch_dev)
SGX_DEV bool sgx_has_mp(const uint8_t *flag, int i) { return flag[i] != 0; }
SGX_DEV bool sgx_has_mp(const int *row, int i) { return row[i] >= 0; }

// One common vocabulary node of SearchForTriangulation (:696-773), exactly as written: features [s1, e1) of items1 against [s2, e2) of items2.  One thread runs it;
// the caller's phase has initialised match12 / matched2.  Shared by k_search_triangulation and k_create_new_map_points (sgx_newpoints_kernels.h).
template <class P> SGX_DEV void sgx_tri_search_node(const SgxTriArgs &A, P has1, P has2, int s1, int e1, int s2, int e2, int *s_total, int *hist)
{
    for (int q1 = s1; q1 < e1; q1++) {
        const int idx1 = A.items1[q1];
        if (sgx_has_mp(has1, idx1)) continue;                                       // :704-705
        const bool stereo1 = A.uright1[idx1] >= 0;
        if (A.only_stereo && !stereo1) continue;
        const float *kp1 = (const float *)(A.keys1 + (size_t)idx1 * 28);
        const uint32_t *d1 = A.desc1 + (size_t)idx1 * 8;
        // CheckDistEpipolarLine: l = x1' F12 (ORBmatcher.cc:140-143), float arithmetic left to right
        const float a = kp1[0] * A.F12[0] + kp1[1] * A.F12[3] + A.F12[6];
        const float b = kp1[0] * A.F12[1] + kp1[1] * A.F12[4] + A.F12[7];
        const float c = kp1[0] * A.F12[2] + kp1[1] * A.F12[5] + A.F12[8];
        const float den = a * a + b * b;
        int bestDist = SGX_TH_LOW, bestIdx2 = -1;
        for (int q2 = s2; q2 < e2; q2++) {
            const int idx2 = A.items2[q2];
            if (A.matched2[idx2] || sgx_has_mp(has2, idx2)) continue;               // :728-729
            const bool stereo2 = A.uright2[idx2] >= 0;
            if (A.only_stereo && !stereo2) continue;
            const int dist = sgx_hamming256(d1, A.desc2 + (size_t)idx2 * 8);
            if (dist > SGX_TH_LOW || dist > bestDist) continue;
            const float *kp2 = (const float *)(A.keys2 + (size_t)idx2 * 28);
            const int oct2 = ((const int *)kp2)[5];
            if (!stereo1 && !stereo2) {                                      // too close to the epipole: :746-752
                const float dx = A.ex - kp2[0], dy = A.ey - kp2[1];
                if (dx * dx + dy * dy < 100 * A.scale2.s[oct2]) continue;
            }
            const float num = a * kp2[0] + b * kp2[1] + c;
            if (den == 0) continue;
            const float dsqr = num * num / den;
            if ((double)dsqr < 3.84 * (double)A.sigma2_2.s[oct2]) { bestIdx2 = idx2; bestDist = dist; }      // :157 compares in double (3.84 is a double literal)
        }
        if (bestIdx2 >= 0) {
            A.match12[idx1] = bestIdx2; A.matched2[bestIdx2] = 1;
            sgx_atomic_add(s_total, 1);
            if (A.check_ori) {
                const float *kp2 = (const float *)(A.keys2 + (size_t)bestIdx2 * 28);
                float rot = kp1[3] - kp2[3];
                if (rot < 0.0f) rot += 360.0f;
                int bin = (int)round((double)(rot * (SGX_HISTO / 360.0f)));
                if (bin == SGX_HISTO) bin = 0;
                sgx_atomic_add(&hist[bin], 1);
            }
        }
    }
}

// MapPoint::UpdateNormalAndDepth of one point P with nobs > 0 observations (camera centres oc, mObservations order), reference centre rc, mvScaleFactors[level] and
// mvScaleFactors[nLevels - 1].  Shared by k_mappoint_normal_depth and k_create_new_map_points (sgx_newpoints_kernels.h).
SGX_DEV void sgx_mp_normal_depth(const float *P, const float *oc, int nobs, const float *rc, float scale_level, float scale_last, float *normal, float *min_dist, float *max_dist)
{
    float n0 = 0.f, n1 = 0.f, n2 = 0.f;
    for (int q = 0; q < nobs; q++) {
        const float d0 = P[0] - oc[3 * (size_t)q], d1 = P[1] - oc[3 * (size_t)q + 1], d2 = P[2] - oc[3 * (size_t)q + 2];
        const double len = sqrt((double)d0 * d0 + (double)d1 * d1 + (double)d2 * d2);
        const float inv = (float)(1.0 / len);
        n0 = n0 + d0 * inv; n1 = n1 + d1 * inv; n2 = n2 + d2 * inv;
    }
    const float c0 = P[0] - rc[0], c1 = P[1] - rc[1], c2 = P[2] - rc[2];
    const float dist = (float)sqrt((double)c0 * c0 + (double)c1 * c1 + (double)c2 * c2);
    const float mx = dist * scale_level;
    *max_dist = mx; *min_dist = mx / scale_last;
    const float invn = (float)(1.0 / (double)nobs);
    normal[0] = n0 * invn; normal[1] = n1 * invn; normal[2] = n2 * invn;
}

// the median of row i of the N x N distance matrix of the descriptors d (see below): element k = (int)(0.5 * (N - 1)) of the sorted row.  Shared by
// k_mappoint_distinctive and k_create_new_map_points (sgx_newpoints_kernels.h).
SGX_DEV int sgx_mp_row_median(const uint32_t *d, int N, int i, int k)
{
    uint32_t di[8];
#pragma unroll
    for (int w = 0; w < 8; w++) di[w] = d[(size_t)i * 8 + w];
    int lo = 0, hi = 256;                                          // smallest v in [0, 256] with count(d <= v) >= k + 1
    while (lo < hi) {
        const int mid = (lo + hi) >> 1;
        int cnt = 0;
        for (int j = 0; j < N; j++) cnt += (i == j ? 0 : sgx_hamming256(di, d + (size_t)j * 8)) <= mid ? 1 : 0;
        if (cnt >= k + 1) hi = mid; else lo = mid + 1;
    }
    return lo;
}

struct SgxNewPointArgs {
    int npairs;
    const int *pairs;
    const uint8_t *keys1_un, *keys1, *keys2_un, *keys2; const float *ur1, *dp1, *ur2, *dp2;
    float Tcw1[16], Tcw2[16], Ow1[3], Ow2[3];
    float fx, fy, cx, cy, mbf, ratio_factor;
    SgxScales scale, sigma2;
    uint8_t *ok; float *x3d;
};

SGX_DEV void sgx_jacobi_svd4_vt3(const float *A, float *v)
{
    const int n = 4, m = 4; const float eps = FLT_EPSILON * 2;
    float At[16], Vt[16]; double W[4];
    for (int i = 0; i < 4; i++) for (int k = 0; k < 4; k++) At[4 * i + k] = A[4 * k + i];
    for (int i = 0; i < n; i++) { double sd = 0; for (int k = 0; k < m; k++) { const float t = At[4 * i + k]; sd += (double)t * t; } W[i] = sd; for (int k = 0; k < n; k++) Vt[4 * i + k] = i == k ? 1.f : 0.f; }
    for (int iter = 0; iter < 30; iter++) {
        bool changed = false;
        for (int i = 0; i < n - 1; i++)
            for (int j = i + 1; j < n; j++) {
                float *Ai = At + 4 * i, *Aj = At + 4 * j;
                double a = W[i], p = 0, b = W[j];
                for (int k = 0; k < m; k++) p += (double)Ai[k] * Aj[k];
                if (fabs(p) <= (double)eps * sqrt(a * b)) continue;
                p *= 2;
                const double beta = a - b, gamma = hypot(p, beta);
                float c, s;
                if (beta < 0) { const double delta = (gamma - beta) * 0.5; s = (float)sqrt(delta / gamma); c = (float)(p / (gamma * (double)s * 2)); }
                else { c = (float)sqrt((gamma + beta) / (gamma * 2)); s = (float)(p / (gamma * (double)c * 2)); }
                a = b = 0;
                for (int k = 0; k < m; k++) { const float t0 = c * Ai[k] + s * Aj[k], t1 = -s * Ai[k] + c * Aj[k]; Ai[k] = t0; Aj[k] = t1; a += (double)t0 * t0; b += (double)t1 * t1; }
                W[i] = a; W[j] = b; changed = true;
                float *Vi = Vt + 4 * i, *Vj = Vt + 4 * j;
                for (int k = 0; k < n; k++) { const float t0 = c * Vi[k] + s * Vj[k], t1 = -s * Vi[k] + c * Vj[k]; Vi[k] = t0; Vj[k] = t1; }
            }
        if (!changed) break;
    }
    for (int i = 0; i < n; i++) { double sd = 0; for (int k = 0; k < m; k++) { const float t = At[4 * i + k]; sd += (double)t * t; } W[i] = sqrt(sd); }
    for (int i = 0; i < n - 1; i++) {
        int j = i;
        for (int k = i + 1; k < n; k++) if (W[j] < W[k]) j = k;
        if (i != j) { const double tw = W[i]; W[i] = W[j]; W[j] = tw; for (int k = 0; k < 4; k++) { float t = At[4 * i + k]; At[4 * i + k] = At[4 * j + k]; At[4 * j + k] = t; t = Vt[4 * i + k]; Vt[4 * i + k] = Vt[4 * j + k]; Vt[4 * j + k] = t; } }
    }
    for (int k = 0; k < 4; k++) v[k] = Vt[12 + k];
}

SGX_DEV double sgx_dot3d(const float *a, const float *b) { double r = 0; for (int i = 0; i < 3; i++) r += (double)a[i] * (double)b[i]; return r; }
SGX_DEV float sgx_gemm3_t(const float *T, int col, const float *b, float c, double beta)      // row `col` of the TRANSPOSE of the 3 x 3 block of T (4-float rows) times b, + beta * c
{
    const float t = T[col] * b[0] + T[4 + col] * b[1] + T[8 + col] * b[2];
    return (float)((double)t * 1.0 + beta * (double)c);
}

// the per-pair body of LocalMapping::CreateNewMapPoints (:286-431) for the pair (idx1, idx2): 1 and the point in X when the triangulation is accepted, else 0 (X is then
// unspecified).  Shared by k_triangulate_pairs and k_create_new_map_points (sgx_newpoints_kernels.h).
SGX_DEV uint8_t sgx_triangulate_pair(const SgxNewPointArgs &A, int idx1, int idx2, float *X)
{
    const float *kp1 = (const float *)(A.keys1_un + (size_t)idx1 * 28), *kp2 = (const float *)(A.keys2_un + (size_t)idx2 * 28);
    const int oct1 = ((const int *)kp1)[5], oct2 = ((const int *)kp2)[5];
    const float invfx = 1.0f / A.fx, invfy = 1.0f / A.fy, mb = A.mbf / A.fx;
    const float kp1_ur = A.ur1[idx1], kp2_ur = A.ur2[idx2];
    const bool bStereo1 = kp1_ur >= 0, bStereo2 = kp2_ur >= 0;
    const float xn1[3] = { (kp1[0] - A.cx) * invfx, (kp1[1] - A.cy) * invfy, 1.0f }, xn2[3] = { (kp2[0] - A.cx) * invfx, (kp2[1] - A.cy) * invfy, 1.0f };
    const float ray1[3] = { sgx_gemm3_t(A.Tcw1, 0, xn1, 0.f, 0.0), sgx_gemm3_t(A.Tcw1, 1, xn1, 0.f, 0.0), sgx_gemm3_t(A.Tcw1, 2, xn1, 0.f, 0.0) };
    const float ray2[3] = { sgx_gemm3_t(A.Tcw2, 0, xn2, 0.f, 0.0), sgx_gemm3_t(A.Tcw2, 1, xn2, 0.f, 0.0), sgx_gemm3_t(A.Tcw2, 2, xn2, 0.f, 0.0) };
    const float cosParallaxRays = (float)(sgx_dot3d(ray1, ray2) / (sqrt(sgx_dot3d(ray1, ray1)) * sqrt(sgx_dot3d(ray2, ray2))));
    float cosParallaxStereo = cosParallaxRays + 1, cs1 = cosParallaxStereo, cs2 = cosParallaxStereo;
    if (bStereo1) cs1 = cosf(2 * atan2f(mb / 2, A.dp1[idx1]));
    else if (bStereo2) cs2 = cosf(2 * atan2f(mb / 2, A.dp2[idx2]));
    cosParallaxStereo = cs1 < cs2 ? cs1 : cs2;
    if (cosParallaxRays < cosParallaxStereo && cosParallaxRays > 0 && (bStereo1 || bStereo2 || (double)cosParallaxRays < 0.9998)) {
        float M[16], v[4];
        for (int k = 0; k < 4; k++) {
            M[k] = xn1[0] * A.Tcw1[8 + k] - A.Tcw1[k]; M[4 + k] = xn1[1] * A.Tcw1[8 + k] - A.Tcw1[4 + k];
            M[8 + k] = xn2[0] * A.Tcw2[8 + k] - A.Tcw2[k]; M[12 + k] = xn2[1] * A.Tcw2[8 + k] - A.Tcw2[4 + k];
        }
        sgx_jacobi_svd4_vt3(M, v);
        if (v[3] == 0) return 0;
        const float inv = (float)(1.0 / (double)v[3]);
        X[0] = v[0] * inv; X[1] = v[1] * inv; X[2] = v[2] * inv;
    } else if (bStereo1 && cs1 < cs2) {
        const float z = A.dp1[idx1];
        if (!(z > 0)) return 0;
        const float *kd = (const float *)(A.keys1 + (size_t)idx1 * 28);
        const float xc[3] = { (kd[0] - A.cx) * z * invfx, (kd[1] - A.cy) * z * invfy, z };
        for (int i = 0; i < 3; i++) X[i] = sgx_gemm3_t(A.Tcw1, i, xc, A.Ow1[i], 1.0);
    } else if (bStereo2 && cs2 < cs1) {
        const float z = A.dp2[idx2];
        if (!(z > 0)) return 0;
        const float *kd = (const float *)(A.keys2 + (size_t)idx2 * 28);
        const float xc[3] = { (kd[0] - A.cx) * z * invfx, (kd[1] - A.cy) * z * invfy, z };
        for (int i = 0; i < 3; i++) X[i] = sgx_gemm3_t(A.Tcw2, i, xc, A.Ow2[i], 1.0);
    } else return 0;
    const float z1 = (float)(sgx_dot3d(A.Tcw1 + 8, X) + (double)A.Tcw1[11]);
    if (z1 <= 0) return 0;
    const float z2 = (float)(sgx_dot3d(A.Tcw2 + 8, X) + (double)A.Tcw2[11]);
    if (z2 <= 0) return 0;
    const float s1 = A.sigma2.s[oct1];
    const float x1 = (float)(sgx_dot3d(A.Tcw1, X) + (double)A.Tcw1[3]), y1 = (float)(sgx_dot3d(A.Tcw1 + 4, X) + (double)A.Tcw1[7]);
    const float invz1 = (float)(1.0 / (double)z1);
    {
        const float u1 = A.fx * x1 * invz1 + A.cx, v1 = A.fy * y1 * invz1 + A.cy, eX = u1 - kp1[0], eY = v1 - kp1[1];
        if (!bStereo1) { if ((double)(eX * eX + eY * eY) > 5.991 * (double)s1) return 0; }
        else { const float u1r = u1 - A.mbf * invz1, eR = u1r - kp1_ur; if ((double)(eX * eX + eY * eY + eR * eR) > 7.8 * (double)s1) return 0; }
    }
    const float s2 = A.sigma2.s[oct2];
    const float x2 = (float)(sgx_dot3d(A.Tcw2, X) + (double)A.Tcw2[3]), y2 = (float)(sgx_dot3d(A.Tcw2 + 4, X) + (double)A.Tcw2[7]);
    const float invz2 = (float)(1.0 / (double)z2);
    {
        const float u2 = A.fx * x2 * invz2 + A.cx, v2 = A.fy * y2 * invz2 + A.cy, eX = u2 - kp2[0], eY = v2 - kp2[1];
        if (!bStereo2) { if ((double)(eX * eX + eY * eY) > 5.991 * (double)s2) return 0; }
        else { const float u2r = u2 - A.mbf * invz2, eR = u2r - kp2_ur; if ((double)(eX * eX + eY * eY + eR * eR) > 7.8 * (double)s2) return 0; }
    }
    const float n1[3] = { X[0] - A.Ow1[0], X[1] - A.Ow1[1], X[2] - A.Ow1[2] }, n2[3] = { X[0] - A.Ow2[0], X[1] - A.Ow2[1], X[2] - A.Ow2[2] };
    const float dist1 = (float)sqrt(sgx_dot3d(n1, n1)), dist2 = (float)sqrt(sgx_dot3d(n2, n2));
    if (dist1 == 0 || dist2 == 0) return 0;
    const float ratioDist = dist2 / dist1, ratioOctave = A.scale.s[oct1] / A.scale.s[oct2];
    if (ratioDist * A.ratio_factor < ratioOctave || ratioDist > ratioOctave * A.ratio_factor) return 0;
    return 1;
}
