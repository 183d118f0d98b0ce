// sgx_init_kernels.h — Initializer (src/sg-slam/src/Initializer.cc), the two-view initialisation of Tracking::MonocularInitialization (Tracking.cc:605-671):
//   Initialize :44-121, FindHomography / FindFundamental :124-223, ComputeH21 / ComputeF21 :226-303, CheckHomography / CheckFundamental :305-468, ReconstructF :470-570,
//   ReconstructH :572-732, Triangulate :734-747, Normalize :749-795, CheckRT :798-907, DecomposeE :909-929.
// Every expression is evaluated in the order written there (-ffp-contract=off, correctly rounded operations only), so the device, the emulator and tests/init_ref.py
// agree bit for bit.  The OpenCV calls are restated from OpenCV 3.4's published algorithm; each rests on one assumption, stated once here:
//   - cv::SVDecomp / cv::SVD::compute on CV_32F = JacobiSVDImpl_<float> on the rows of A^T (m >= n) or of A itself (m < n): minval = FLT_MIN, eps = 2 FLT_EPSILON,
//     max(m, 30) sweeps, column norms and the inner product p in double, c, s and the rotated entries in float, descending sort, then the rows are normalised and rows
//     with a zero singular value (and, with FULL_UV, rows n .. n1 - 1) are completed from cv::RNG(0x12345678) by two Gram-Schmidt passes.  std::hypot of the rotation is
//     written as sgx_init_hypot (correctly rounded operations only; libm's hypot differs in the last bit between hosts and the device).
//     8 x 9 (ComputeF21, m < n, FULL_UV): the eight rows of A are rotated, vt = the 9 x 9 buffer whose ninth row is that completion, so vt.row(8) is the completed row.
//     16 x 9 (ComputeH21): vt = the accumulated rotations; the completion touches only U rows nobody reads and is skipped.  4 x 4 (Triangulate): likewise, vt.row(3).
//   - 3 x 3 float products without a transpose = cv::gemm's small-matrix path: float dot product left to right, then (float)(dot * alpha [+ beta * c]) in double;
//     `s * U * Rp * Vt` folds s into alpha.  Products with a transposed operand (K.t() * F21, -R.t() * t) take the generic path: double accumulation.
//   - Mat::inv() and cv::determinant on 3 x 3 float = the closed form with a double determinant (inv of a singular matrix is the zero matrix).
//   - cv::norm and Mat::dot accumulate in double; `m / x` and `m *= x` multiply by the float of 1. / x (of x).
//   - `a * row - row` (Triangulate) is evaluated in float.
// Defined where the reference is undefined: fewer than 8 matches -> ok = 0 and no random number is consumed; no hypothesis of the chosen model scored above 0 (the
// reference would decompose an empty matrix) -> ok = 0; a NaN score never wins (IEEE comparison, as written); matches12[i] >= n2 counts as unmatched.
// acos is not evaluated on the device: parallax = (float)(acos((double)c) * 180 / CV_PI) is monotone in c, so the host turns the two gates (`> minParallax` in
// ReconstructF, `>= minParallax` in ReconstructH) into the largest cosine that passes (cos_gt, cos_ge) and the kernels compare cosines.
// Layout: k_init_setup = one lane per pair (the match list in index order, the rand() replica's draws); k_init_normalize = one lane per (pair, frame), sequential float
// sums; k_init_hyp = one lane per (pair, model, iteration) with the Jacobi working set in LDS, lane index minor; k_init_score = one lane per hypothesis, the matches
// staged in LDS and read as broadcasts, the float score summed in match order; k_init_best = the first strict maximum per (pair, model); k_init_inliers = the two
// winners' flags, one lane per match; k_init_decide = one lane per pair (RH, DecomposeE or Faugeras); k_init_check_rt = one lane per (pair, hypothesis, match);
// k_init_finish = one workgroup per pair (counts, the min(50, nGood - 1)-th smallest cosine by rank, the selection rule, the outputs).
#pragma once
#include "sgx_rt.h"
#include "sgx_grand.h"
#include <math.h>
#include <float.h>

#define SGX_INIT_MAXIT 256           /* hypotheses per (pair, model) and launch */
#define SGX_INIT_HYP 18              /* floats per hypothesis: H21 9 | H12 9, or F21 9 | unused */
#define SGX_INIT_TILE 512            /* matches staged per LDS tile of k_init_score */

struct SgxInitReport {               // = sgx_init_report (include/sgx.h)
    float SH, SF, RH; int32_t model, n_matches, n_inliers_h, n_inliers_f, n_hyp, best_hyp;
    int32_t n_good[8]; float cos_parallax[8], parallax[8]; float H21[9], F21[9];
};

struct SgxInitArgs {
    int B, iterations, chunk0, chunk_n, cap, ntot;  // this launch covers iterations [chunk0, chunk0 + chunk_n); cap = hypotheses per (pair, model) in hyp / scores; ntot = off1[B]
    const int *off1, *off2;                         // B + 1: keys of pair b = [off[b], off[b + 1]) of keys1 / keys2; matches12 and everything per match follow off1
    const float *keys1, *keys2;                     // sgx_keypoint = 7 words, pt first
    const int *matches12;
    const float *cam, *sigma;                       // B x 4 (fx, fy, cx, cy), B
    const int *draws; int draw_stride;              // raw rand() values: pair b, iteration h, draw k -> draws[b * draw_stride + 8 * h + k]
    float cos_gt, cos_ge;                           // the largest cosine whose parallax is > / >= 1 degree
    int *nmatch;                                    // B: N = mvMatches12.size()
    int *mi;                                        // 2 per match: keypoint index in frame 1, in frame 2
    float *mxy;                                     // 4 per match: u1, v1, u2, v2
    float *norm;                                    // B x 2 x 4: meanX, meanY, sX, sY of Normalize
    float *hyp, *scores;                            // B x 2 x cap x SGX_INIT_HYP, B x 2 x cap
    float *best;                                    // B x 2 x 10: best score so far, its H21 / F21
    uint8_t *inl;                                   // 2 x ntot: vbMatchesInliers of the H / F winner
    int *ninl;                                      // B x 2
    int *dec;                                       // B x 2: model, number of motion hypotheses (0: none to check)
    float *rt;                                      // B x 8 x 12: R 9 | t 3
    uint8_t *good; float *cosp, *pts;               // 8 x ntot (x 3): per hypothesis and match 0 / 1 counted in nGood / 2 also vbGood, cosParallax, the point
    float *R21, *t21, *p3d; uint8_t *tri, *inl_out; int *ok; SgxInitReport *report;       // outputs: B x 9, B x 3, ntot x 3, ntot, ntot, B, B
};

// ---------------------------------------------------------------------------------------------------------------------------------------------------- OpenCV algebra
SGX_DEV double sgx_init_hypot(double x, double y)
{
    double a = fabs(x), b = fabs(y);
    if (a < b) { const double t = a; a = b; b = t; }
    if (a == 0 || b == 0) return a + b;
    const double r = b / a;
    return a * sqrt(1.0 + r * r);
}

// JacobiSVDImpl_<float>(At, W, Vt, m, n, n1, FLT_MIN, FLT_EPSILON * 2): At = n1 rows of m (the first n are rotated), Vt n x n or NULL (rotations not accumulated), W n
// doubles (descending on return).  Element e of an array sits at [e * es]: es = 1 for a private array, es = the workgroup size for the lane-minor LDS layout.
SGX_DEV void sgx_init_jacobi(float *At, double *W, float *Vt, int es, int m, int n, int n1)
{
#define SGX_AT(i, k) At[((i) * m + (k)) * es]
#define SGX_VT(i, k) Vt[((i) * n + (k)) * es]
#define SGX_W(i) W[(i) * es]
    const double minval = FLT_MIN; const float eps = FLT_EPSILON * 2;
    const int max_iter = m > 30 ? m : 30;
    for (int i = 0; i < n; i++) {
        double sd = 0;
        for (int k = 0; k < m; k++) { const float t = SGX_AT(i, k); sd += (double)t * t; }
        SGX_W(i) = sd;
        if (Vt) for (int k = 0; k < n; k++) SGX_VT(i, k) = i == k ? 1.f : 0.f;
    }
    for (int iter = 0; iter < max_iter; iter++) {
        bool changed = false;
        for (int i = 0; i < n - 1; i++)
            for (int j = i + 1; j < n; j++) {
                double a = SGX_W(i), p = 0, b = SGX_W(j);
                for (int k = 0; k < m; k++) p += (double)SGX_AT(i, k) * SGX_AT(j, k);
                if (fabs(p) <= eps * sqrt(a * b)) continue;
                p *= 2;
                const double beta = a - b, gamma = sgx_init_hypot(p, beta);
                float c, s;
                if (beta < 0) { const double delta = (gamma - beta) * 0.5; s = (float)sqrt(delta / gamma); c = (float)(p / (gamma * s * 2)); }
                else { c = (float)sqrt((gamma + beta) / (gamma * 2)); s = (float)(p / (gamma * c * 2)); }
                a = b = 0;
                for (int k = 0; k < m; k++) {
                    const float ai = SGX_AT(i, k), aj = SGX_AT(j, k);
                    const float t0 = c * ai + s * aj, t1 = -s * ai + c * aj;
                    SGX_AT(i, k) = t0; SGX_AT(j, k) = t1;
                    a += (double)t0 * t0; b += (double)t1 * t1;
                }
                SGX_W(i) = a; SGX_W(j) = b;
                changed = true;
                if (Vt) for (int k = 0; k < n; k++) { const float vi = SGX_VT(i, k), vj = SGX_VT(j, k); SGX_VT(i, k) = c * vi + s * vj; SGX_VT(j, k) = -s * vi + c * vj; }
            }
        if (!changed) break;
    }
    for (int i = 0; i < n; i++) {
        double sd = 0;
        for (int k = 0; k < m; k++) { const float t = SGX_AT(i, k); sd += (double)t * t; }
        SGX_W(i) = sqrt(sd);
    }
    for (int i = 0; i < n - 1; i++) {
        int j = i;
        for (int k = i + 1; k < n; k++) if (SGX_W(j) < SGX_W(k)) j = k;
        if (i != j) {
            const double tw = SGX_W(i); SGX_W(i) = SGX_W(j); SGX_W(j) = tw;
            for (int k = 0; k < m; k++) { const float t = SGX_AT(i, k); SGX_AT(i, k) = SGX_AT(j, k); SGX_AT(j, k) = t; }
            if (Vt) for (int k = 0; k < n; k++) { const float t = SGX_VT(i, k); SGX_VT(i, k) = SGX_VT(j, k); SGX_VT(j, k) = t; }
        }
    }
    uint64_t rng = 0x12345678u;                                  // cv::RNG(0x12345678), advanced only by the completions
    for (int i = 0; i < n1; i++) {
        double sd = i < n ? SGX_W(i) : 0;
        for (int ii = 0; ii < 100 && sd <= minval; ii++) {
            const float val0 = (float)(1. / m);
            for (int k = 0; k < m; k++) {
                rng = (uint64_t)(unsigned)rng * 4164903690u + (unsigned)(rng >> 32);
                SGX_AT(i, k) = ((unsigned)rng & 256) != 0 ? val0 : -val0;
            }
            for (int it = 0; it < 2; it++)
                for (int j = 0; j < i; j++) {
                    sd = 0;
                    for (int k = 0; k < m; k++) sd += (double)(SGX_AT(i, k) * SGX_AT(j, k));
                    float asum = 0;
                    for (int k = 0; k < m; k++) { const float t = (float)((double)SGX_AT(i, k) - sd * (double)SGX_AT(j, k)); SGX_AT(i, k) = t; asum += fabsf(t); }
                    asum = asum > eps * 100 ? 1 / asum : 0;
                    for (int k = 0; k < m; k++) SGX_AT(i, k) *= asum;
                }
            sd = 0;
            for (int k = 0; k < m; k++) { const float t = SGX_AT(i, k); sd += (double)t * t; }
            sd = sqrt(sd);
        }
        const float s = (float)(sd > minval ? 1 / sd : 0.);
        for (int k = 0; k < m; k++) SGX_AT(i, k) *= s;
    }
#undef SGX_AT
#undef SGX_VT
#undef SGX_W
}

// cv::SVD::compute(A 3 x 3, w, U, Vt) (FULL_UV or not: the same for a square matrix) in a lane-minor workspace ws (18 floats) / wd (3 doubles)
SGX_DEV void sgx_init_svd3(const float *A, float *ws, double *wd, int es, float *U, float *w, float *Vt)
{
    for (int i = 0; i < 3; i++) for (int k = 0; k < 3; k++) ws[(3 * i + k) * es] = A[3 * k + i];
    sgx_init_jacobi(ws, wd, ws + 9 * es, es, 3, 3, 3);
    for (int i = 0; i < 3; i++) {
        w[i] = (float)wd[i * es];
        for (int k = 0; k < 3; k++) { U[3 * k + i] = ws[(3 * i + k) * es]; Vt[3 * i + k] = ws[(9 + 3 * i + k) * es]; }
    }
}

// D = alpha * A * B on cv::gemm's small-matrix path (3 x 3 row-major; D may not alias A or B)
SGX_DEV void sgx_init_mul3(const float *A, const float *B, double alpha, float *D)
{
    for (int i = 0; i < 3; i++)
        for (int j = 0; j < 3; j++) { const float t = A[3 * i] * B[j] + A[3 * i + 1] * B[3 + j] + A[3 * i + 2] * B[6 + j]; D[3 * i + j] = (float)((double)t * alpha); }
}

// D = A^T * B on the generic path (transpose flag): double accumulation
SGX_DEV void sgx_init_mul3_tn(const float *A, const float *B, float *D)
{
    for (int i = 0; i < 3; i++)
        for (int j = 0; j < 3; j++) { double s = 0; for (int k = 0; k < 3; k++) s += (double)A[3 * k + i] * (double)B[3 * k + j]; D[3 * i + j] = (float)(s * 1.0); }
}

SGX_DEV void sgx_init_mulv3(const float *A, const float *b, float *d)      // 3 x 3 times 3 x 1, small path
{
    for (int i = 0; i < 3; i++) { const float t = A[3 * i] * b[0] + A[3 * i + 1] * b[1] + A[3 * i + 2] * b[2]; d[i] = (float)((double)t * 1.0); }
}

SGX_DEV double sgx_init_det3(const float *m)
{
    return m[0] * ((double)m[4] * m[8] - (double)m[5] * m[7]) - m[1] * ((double)m[3] * m[8] - (double)m[5] * m[6]) + m[2] * ((double)m[3] * m[7] - (double)m[4] * m[6]);
}

SGX_DEV void sgx_init_inv3(const float *S, float *D)
{
    double d = sgx_init_det3(S);
    if (d == 0.) { for (int i = 0; i < 9; i++) D[i] = 0.f; return; }
    d = 1. / d;
    D[0] = (float)(((double)S[4] * S[8] - (double)S[5] * S[7]) * d);
    D[1] = (float)(((double)S[2] * S[7] - (double)S[1] * S[8]) * d);
    D[2] = (float)(((double)S[1] * S[5] - (double)S[2] * S[4]) * d);
    D[3] = (float)(((double)S[5] * S[6] - (double)S[3] * S[8]) * d);
    D[4] = (float)(((double)S[0] * S[8] - (double)S[2] * S[6]) * d);
    D[5] = (float)(((double)S[2] * S[3] - (double)S[0] * S[5]) * d);
    D[6] = (float)(((double)S[3] * S[7] - (double)S[4] * S[6]) * d);
    D[7] = (float)(((double)S[1] * S[6] - (double)S[0] * S[7]) * d);
    D[8] = (float)(((double)S[0] * S[4] - (double)S[1] * S[3]) * d);
}

SGX_DEV double sgx_init_dot3d(const float *a, const float *b) { double r = 0; for (int i = 0; i < 3; i++) r += (double)a[i] * (double)b[i]; return r; }

// t / cv::norm(t)
SGX_DEV void sgx_init_unit3(float *t)
{
    const float inv = (float)(1. / sqrt(sgx_init_dot3d(t, t)));
    for (int i = 0; i < 3; i++) t[i] = t[i] * inv;
}

SGX_DEV void sgx_init_T(const float *nm, float *T)               // the T of Normalize (:790-794)
{
    T[0] = nm[2]; T[1] = 0.f; T[2] = -nm[0] * nm[2]; T[3] = 0.f; T[4] = nm[3]; T[5] = -nm[1] * nm[3]; T[6] = 0.f; T[7] = 0.f; T[8] = 1.f;
}

// ---------------------------------------------------------------------------------------------------------------------------------------------------- scoring
// one match of CheckHomography (:337-385): adds to score, returns bIn
SGX_DEV bool sgx_init_check_h(const float *h, const float *hi, float u1, float v1, float u2, float v2, float invSigmaSquare, float &score)
{
    const float th = 5.991f;
    bool bIn = true;
    const float w2in1inv = (float)(1.0 / (double)(hi[6] * u2 + hi[7] * v2 + hi[8]));
    const float u2in1 = (hi[0] * u2 + hi[1] * v2 + hi[2]) * w2in1inv;
    const float v2in1 = (hi[3] * u2 + hi[4] * v2 + hi[5]) * w2in1inv;
    const float squareDist1 = (u1 - u2in1) * (u1 - u2in1) + (v1 - v2in1) * (v1 - v2in1);
    const float chiSquare1 = squareDist1 * invSigmaSquare;
    if (chiSquare1 > th) bIn = false; else score += th - chiSquare1;
    const float w1in2inv = (float)(1.0 / (double)(h[6] * u1 + h[7] * v1 + h[8]));
    const float u1in2 = (h[0] * u1 + h[1] * v1 + h[2]) * w1in2inv;
    const float v1in2 = (h[3] * u1 + h[4] * v1 + h[5]) * w1in2inv;
    const float squareDist2 = (u2 - u1in2) * (u2 - u1in2) + (v2 - v1in2) * (v2 - v1in2);
    const float chiSquare2 = squareDist2 * invSigmaSquare;
    if (chiSquare2 > th) bIn = false; else score += th - chiSquare2;
    return bIn;
}

// one match of CheckFundamental (:413-465): the gate is 3.841, the score counts from 5.991
SGX_DEV bool sgx_init_check_f(const float *f, float u1, float v1, float u2, float v2, float invSigmaSquare, float &score)
{
    const float th = 3.841f, thScore = 5.991f;
    bool bIn = true;
    const float a2 = f[0] * u1 + f[1] * v1 + f[2], b2 = f[3] * u1 + f[4] * v1 + f[5], c2 = f[6] * u1 + f[7] * v1 + f[8];
    const float num2 = a2 * u2 + b2 * v2 + c2;
    const float squareDist1 = num2 * num2 / (a2 * a2 + b2 * b2);
    const float chiSquare1 = squareDist1 * invSigmaSquare;
    if (chiSquare1 > th) bIn = false; else score += thScore - chiSquare1;
    const float a1 = f[0] * u2 + f[3] * v2 + f[6], b1 = f[1] * u2 + f[4] * v2 + f[7], c1 = f[2] * u2 + f[5] * v2 + f[8];
    const float num1 = a1 * u1 + b1 * v1 + c1;
    const float squareDist2 = num1 * num1 / (a1 * a1 + b1 * b1);
    const float chiSquare2 = squareDist2 * invSigmaSquare;
    if (chiSquare2 > th) bIn = false; else score += thScore - chiSquare2;
    return bIn;
}

SGX_DEV float sgx_init_inv_sigma2(float sigma) { return (float)(1.0 / (double)(sigma * sigma)); }

// ---------------------------------------------------------------------------------------------------------------------------------------------------- kernels
// one lane per pair: mvMatches12 (:51-63) in index order and, without caller draws, the 8 x iterations values its rand() replica hands out (none when N < 8)
SGX_KERNEL(64) k_init_setup(SgxInitArgs A, int32_t *rng, int32_t *own_draws)
{
    SGX_THREADS_BEGIN(tid)
    const int b = (int)blockIdx.x * 64 + tid;
    if (b < A.B) {
        const int o1 = A.off1[b], n1 = A.off1[b + 1] - o1, o2 = A.off2[b], n2 = A.off2[b + 1] - o2;
        int N = 0;
        for (int i = 0; i < n1; i++) {
            const int m = A.matches12[o1 + i];
            if (m >= 0 && m < n2) {
                A.mi[2 * (size_t)(o1 + N)] = i; A.mi[2 * (size_t)(o1 + N) + 1] = m;
                float *xy = A.mxy + 4 * (size_t)(o1 + N);
                xy[0] = A.keys1[7 * (size_t)(o1 + i)]; xy[1] = A.keys1[7 * (size_t)(o1 + i) + 1];
                xy[2] = A.keys2[7 * (size_t)(o2 + m)]; xy[3] = A.keys2[7 * (size_t)(o2 + m) + 1];
                N++;
            }
        }
        A.nmatch[b] = N;
        for (int q = 0; q < 2; q++) { A.best[10 * (2 * b + q)] = 0.f; A.ninl[2 * b + q] = 0; }       // score = 0.0 (:137, :188)
        if (own_draws && N >= 8) { int32_t *g = rng + SGX_GRAND_WORDS * b; for (int i = 0; i < 8 * A.iterations; i++) own_draws[(size_t)b * 8 * A.iterations + i] = sgx_grand(g); }
    }
    SGX_THREADS_END
}

// one lane per (pair, frame): Normalize (:749-795) over all keys of the frame, the float sums in key order
SGX_KERNEL(64) k_init_normalize(SgxInitArgs A)
{
    SGX_THREADS_BEGIN(tid)
    const int q = (int)blockIdx.x * 64 + tid;
    if (q < 2 * A.B) {
        const int b = q >> 1, fr = q & 1;
        const int o = fr ? A.off2[b] : A.off1[b], n = (fr ? A.off2[b + 1] : A.off1[b + 1]) - o;
        const float *keys = (fr ? A.keys2 : A.keys1) + 7 * (size_t)o;
        float meanX = 0, meanY = 0;
        for (int i = 0; i < n; i++) { meanX += keys[7 * (size_t)i]; meanY += keys[7 * (size_t)i + 1]; }
        meanX = meanX / n; meanY = meanY / n;
        float meanDevX = 0, meanDevY = 0;
        for (int i = 0; i < n; i++) { meanDevX += fabsf(keys[7 * (size_t)i] - meanX); meanDevY += fabsf(keys[7 * (size_t)i + 1] - meanY); }
        meanDevX = meanDevX / n; meanDevY = meanDevY / n;
        float *nm = A.norm + 4 * q;
        nm[0] = meanX; nm[1] = meanY; nm[2] = (float)(1.0 / (double)meanDevX); nm[3] = (float)(1.0 / (double)meanDevY);
    }
    SGX_THREADS_END
}

// one lane per (pair, model, iteration): the eight draws (:82-97), ComputeH21 + H21i / H12i (:159-161) or ComputeF21 + F21i (:210-212).  The Jacobi working set
// (9 x 16 + 9 x 9 floats, 9 doubles per lane) lives in LDS with the lane index minor: 62208 bytes per workgroup of 64.
SGX_KERNEL(64) k_init_hyp(SgxInitArgs A)
{
    SGX_LDS float s_at[144 * 64], s_vt[81 * 64];
    SGX_LDS double s_w[9 * 64];
    SGX_THREADS_BEGIN(tid)
    const int b = (int)blockIdx.y, model = (int)blockIdx.z, hl = (int)blockIdx.x * 64 + tid, h = A.chunk0 + hl;
    const int N = A.nmatch[b];
    if (hl < A.chunk_n && h < A.iterations && N >= 8) {
        const int o1 = A.off1[b];
        int pos[8], val[8], idx[8];
        const double R1 = (double)2147483647 + 1.0;
        for (int k = 0; k < 8; k++) {
            const int size = N - k;
            int r = (int)(((double)A.draws[(size_t)b * A.draw_stride + 8 * (size_t)h + k] / R1) * size);
            r = r < 0 ? 0 : r >= size ? size - 1 : r;                // rand() is in [0, RAND_MAX]; a caller's value outside it cannot index out of bounds
            int v = r, back = size - 1;                              // vAvailableIndices[p] = the latest value written to position p, else p
            for (int q = 0; q < k; q++) { if (pos[q] == r) v = val[q]; if (pos[q] == size - 1) back = val[q]; }
            idx[k] = v; pos[k] = r; val[k] = back;
        }
        const float *nm1 = A.norm + 8 * b, *nm2 = nm1 + 4;
        float T1[9], T2[9];
        sgx_init_T(nm1, T1); sgx_init_T(nm2, T2);
        float *at = s_at + tid, *vt = s_vt + tid; double *w = s_w + tid;
        float *out = A.hyp + ((size_t)(2 * b + model) * A.cap + hl) * SGX_INIT_HYP;
        if (model == 0) {
            for (int i = 0; i < 8; i++) {
                const float *xy = A.mxy + 4 * (size_t)(o1 + idx[i]);
                const float u1 = (xy[0] - nm1[0]) * nm1[2], v1 = (xy[1] - nm1[1]) * nm1[3], u2 = (xy[2] - nm2[0]) * nm2[2], v2 = (xy[3] - nm2[1]) * nm2[3];
                const float r0[9] = { 0.f, 0.f, 0.f, -u1, -v1, -1.f, v2 * u1, v2 * v1, v2 }, r1[9] = { u1, v1, 1.f, 0.f, 0.f, 0.f, -u2 * u1, -u2 * v1, -u2 };
                for (int c = 0; c < 9; c++) { at[(16 * c + 2 * i) * 64] = r0[c]; at[(16 * c + 2 * i + 1) * 64] = r1[c]; }
            }
            sgx_init_jacobi(at, w, vt, 64, 16, 9, 0);
            float Hn[9], T2inv[9], tmp[9], H21[9], H12[9];
            for (int k = 0; k < 9; k++) Hn[k] = vt[(72 + k) * 64];
            sgx_init_inv3(T2, T2inv);
            sgx_init_mul3(T2inv, Hn, 1.0, tmp); sgx_init_mul3(tmp, T1, 1.0, H21);
            sgx_init_inv3(H21, H12);
            for (int k = 0; k < 9; k++) { out[k] = H21[k]; out[9 + k] = H12[k]; }
        } else {
            for (int i = 0; i < 8; i++) {
                const float *xy = A.mxy + 4 * (size_t)(o1 + idx[i]);
                const float u1 = (xy[0] - nm1[0]) * nm1[2], v1 = (xy[1] - nm1[1]) * nm1[3], u2 = (xy[2] - nm2[0]) * nm2[2], v2 = (xy[3] - nm2[1]) * nm2[3];
                const float r[9] = { u2 * u1, u2 * v1, u2, v2 * u1, v2 * v1, v2, u1, v1, 1.f };
                for (int c = 0; c < 9; c++) at[(9 * i + c) * 64] = r[c];
            }
            for (int c = 0; c < 9; c++) at[(72 + c) * 64] = 0.f;
            sgx_init_jacobi(at, w, (float *)0, 64, 9, 8, 9);
            float Fpre[9], U[9], sw[3], Vt[9], ud[9], Fn[9], T2t[9], tmp[9], F21[9];
            for (int k = 0; k < 9; k++) Fpre[k] = at[(72 + k) * 64];
            sgx_init_svd3(Fpre, vt, w, 64, U, sw, Vt);
            sw[2] = 0.f;
            const float D[9] = { sw[0], 0.f, 0.f, 0.f, sw[1], 0.f, 0.f, 0.f, sw[2] };
            sgx_init_mul3(U, D, 1.0, ud); sgx_init_mul3(ud, Vt, 1.0, Fn);
            for (int i = 0; i < 3; i++) for (int k = 0; k < 3; k++) T2t[3 * i + k] = T2[3 * k + i];
            sgx_init_mul3(T2t, Fn, 1.0, tmp); sgx_init_mul3(tmp, T1, 1.0, F21);
            for (int k = 0; k < 9; k++) { out[k] = F21[k]; out[9 + k] = 0.f; }
        }
    }
    SGX_THREADS_END
}

// one lane per hypothesis of one (pair, model): CheckHomography / CheckFundamental over all matches in order; the matches are staged tile by tile in LDS
SGX_KERNEL(256) k_init_score(SgxInitArgs A)
{
    SGX_LDS float s_xy[4 * SGX_INIT_TILE];
    SGX_PRIV_DECL(float, score, 1, 256);
    const int b = (int)blockIdx.y, model = (int)blockIdx.z;
    const int N = A.nmatch[b], o1 = A.off1[b];
    if (N < 8) return;
    const float invSigmaSquare = sgx_init_inv_sigma2(A.sigma[b]);
    SGX_THREADS_BEGIN(tid)
    SGX_PRIV_BIND(score, tid);
    score[0] = 0.f;
    SGX_THREADS_END
    for (int t0 = 0; t0 < N; t0 += SGX_INIT_TILE) {
        const int nt = N - t0 < SGX_INIT_TILE ? N - t0 : SGX_INIT_TILE;
        SGX_SYNC();
        SGX_THREADS_BEGIN(tid)
        for (int q = tid; q < 4 * nt; q += 256) s_xy[q] = A.mxy[4 * (size_t)(o1 + t0) + q];
        SGX_THREADS_END
        SGX_SYNC();
        SGX_THREADS_BEGIN(tid)
        SGX_PRIV_BIND(score, tid);
        const int hl = (int)blockIdx.x * 256 + tid;
        if (hl < A.chunk_n && A.chunk0 + hl < A.iterations) {
            const float *hp = A.hyp + ((size_t)(2 * b + model) * A.cap + hl) * SGX_INIT_HYP;
            float m[18];
            for (int k = 0; k < 18; k++) m[k] = hp[k];
            float sc = score[0];
            if (model == 0) for (int i = 0; i < nt; i++) (void)sgx_init_check_h(m, m + 9, s_xy[4 * i], s_xy[4 * i + 1], s_xy[4 * i + 2], s_xy[4 * i + 3], invSigmaSquare, sc);
            else for (int i = 0; i < nt; i++) (void)sgx_init_check_f(m, s_xy[4 * i], s_xy[4 * i + 1], s_xy[4 * i + 2], s_xy[4 * i + 3], invSigmaSquare, sc);
            score[0] = sc;
        }
        SGX_THREADS_END
    }
    SGX_THREADS_BEGIN(tid)
    SGX_PRIV_BIND(score, tid);
    const int hl = (int)blockIdx.x * 256 + tid;
    if (hl < A.chunk_n && A.chunk0 + hl < A.iterations) A.scores[(size_t)(2 * b + model) * A.cap + hl] = score[0];
    SGX_THREADS_END
}

// one lane per (pair, model): `if(currentScore>score)` in iteration order (:165, :216) over this chunk; a NaN score never wins
SGX_KERNEL(64) k_init_best(SgxInitArgs A)
{
    SGX_THREADS_BEGIN(tid)
    const int q = (int)blockIdx.x * 64 + tid;
    if (q < 2 * A.B && A.nmatch[q >> 1] >= 8) {
        float *best = A.best + 10 * q;
        int nh = A.iterations - A.chunk0; if (nh > A.chunk_n) nh = A.chunk_n;
        int win = -1;
        for (int h = 0; h < nh; h++) { const float s = A.scores[(size_t)q * A.cap + h]; if (s > best[0]) { best[0] = s; win = h; } }
        if (win >= 0) for (int k = 0; k < 9; k++) best[1 + k] = A.hyp[((size_t)q * A.cap + win) * SGX_INIT_HYP + k];
    }
    SGX_THREADS_END
}

// one lane per match: vbMatchesInliers of the H and of the F winner
SGX_KERNEL(256) k_init_inliers(SgxInitArgs A)
{
    SGX_THREADS_BEGIN(tid)
    const int b = (int)blockIdx.y, model = (int)blockIdx.z, i = (int)blockIdx.x * 256 + tid;
    const int N = A.nmatch[b], o1 = A.off1[b];
    if (i < N) {
        const float *best = A.best + 10 * (2 * b + model);
        bool in = false;
        if (N >= 8 && best[0] > 0.f) {
            const float *xy = A.mxy + 4 * (size_t)(o1 + i);
            const float invSigmaSquare = sgx_init_inv_sigma2(A.sigma[b]);
            float sc = 0.f;
            if (model == 0) { float Hi[9]; sgx_init_inv3(best + 1, Hi); in = sgx_init_check_h(best + 1, Hi, xy[0], xy[1], xy[2], xy[3], invSigmaSquare, sc); }
            else in = sgx_init_check_f(best + 1, xy[0], xy[1], xy[2], xy[3], invSigmaSquare, sc);
        }
        A.inl[(size_t)model * A.ntot + o1 + i] = in ? 1 : 0;
        if (in) sgx_atomic_add(&A.ninl[2 * b + model], 1);
    }
    SGX_THREADS_END
}

// one lane per pair: RH (:112-118) and the motion hypotheses: the eight of Faugeras (:584-686) or the four of DecomposeE (:479-487, :909-929)
SGX_KERNEL(64) k_init_decide(SgxInitArgs A)
{
    SGX_THREADS_BEGIN(tid)
    const int b = (int)blockIdx.x * 64 + tid;
    if (b < A.B) {
        SgxInitReport *rep = A.report + b;
        const float *bh = A.best + 20 * b, *bf = bh + 10;
        const int N = A.nmatch[b];
        const float SH = N >= 8 ? bh[0] : 0.f, SF = N >= 8 ? bf[0] : 0.f;
        const float RH = SH / (SH + SF);
        const int model = (double)RH > 0.40 ? 0 : 1;
        rep->SH = SH; rep->SF = SF; rep->RH = RH; rep->model = model; rep->n_matches = N; rep->n_inliers_h = A.ninl[2 * b]; rep->n_inliers_f = A.ninl[2 * b + 1];
        rep->best_hyp = -1;
        for (int k = 0; k < 8; k++) { rep->n_good[k] = 0; rep->cos_parallax[k] = 0.f; rep->parallax[k] = 0.f; }
        for (int k = 0; k < 9; k++) { rep->H21[k] = SH > 0.f ? bh[1 + k] : 0.f; rep->F21[k] = SF > 0.f ? bf[1 + k] : 0.f; }
        int nhyp = 0;
        float *rt = A.rt + 96 * (size_t)b;
        const float *c = A.cam + 4 * b;
        const float K[9] = { c[0], 0.f, c[2], 0.f, c[1], c[3], 0.f, 0.f, 1.f };
        float ws[18]; double wd[3];
        float U[9], w[3], Vt[9], tmp[9];
        if (model == 0 && SH > 0.f) {
            float invK[9], Am[9];
            sgx_init_inv3(K, invK);
            sgx_init_mul3(invK, bh + 1, 1.0, tmp); sgx_init_mul3(tmp, K, 1.0, Am);
            sgx_init_svd3(Am, ws, wd, 1, U, w, Vt);
            const float s = (float)(sgx_init_det3(U) * sgx_init_det3(Vt));
            const float d1 = w[0], d2 = w[1], d3 = w[2];
            if (!((double)(d1 / d2) < 1.00001 || (double)(d2 / d3) < 1.00001)) {
                nhyp = 8;
                const float aux1 = sqrtf((d1 * d1 - d2 * d2) / (d1 * d1 - d3 * d3)), aux3 = sqrtf((d2 * d2 - d3 * d3) / (d1 * d1 - d3 * d3));
                const float x1[4] = { aux1, aux1, -aux1, -aux1 }, x3[4] = { aux3, -aux3, aux3, -aux3 };
                const float aux_stheta = sqrtf((d1 * d1 - d2 * d2) * (d2 * d2 - d3 * d3)) / ((d1 + d3) * d2);
                const float ctheta = (d2 * d2 + d1 * d3) / ((d1 + d3) * d2);
                const float stheta[4] = { aux_stheta, -aux_stheta, -aux_stheta, aux_stheta };
                const float aux_sphi = sqrtf((d1 * d1 - d2 * d2) * (d2 * d2 - d3 * d3)) / ((d1 - d3) * d2);
                const float cphi = (d1 * d3 - d2 * d2) / ((d1 - d3) * d2);
                const float sphi[4] = { aux_sphi, -aux_sphi, -aux_sphi, aux_sphi };
                for (int i = 0; i < 8; i++) {
                    const int q = i & 3;
                    float Rp[9], tp[3];
                    if (i < 4) {
                        const float r[9] = { ctheta, 0.f, -stheta[q], 0.f, 1.f, 0.f, stheta[q], 0.f, ctheta };
                        for (int k = 0; k < 9; k++) Rp[k] = r[k];
                        tp[0] = x1[q] * (d1 - d3); tp[1] = 0.f * (d1 - d3); tp[2] = -x3[q] * (d1 - d3);
                    } else {
                        const float r[9] = { cphi, 0.f, sphi[q], 0.f, -1.f, 0.f, sphi[q], 0.f, -cphi };
                        for (int k = 0; k < 9; k++) Rp[k] = r[k];
                        tp[0] = x1[q] * (d1 + d3); tp[1] = 0.f * (d1 + d3); tp[2] = x3[q] * (d1 + d3);
                    }
                    float *R = rt + 12 * i, *t = R + 9;
                    sgx_init_mul3(U, Rp, (double)s, tmp); sgx_init_mul3(tmp, Vt, 1.0, R);
                    sgx_init_mulv3(U, tp, t);
                    sgx_init_unit3(t);
                }
            }
        } else if (model == 1 && SF > 0.f) {
            nhyp = 4;
            float E[9];
            sgx_init_mul3_tn(K, bf + 1, tmp); sgx_init_mul3(tmp, K, 1.0, E);
            sgx_init_svd3(E, ws, wd, 1, U, w, Vt);
            float t[3] = { U[2], U[5], U[8] };
            sgx_init_unit3(t);
            const float W[9] = { 0.f, -1.f, 0.f, 1.f, 0.f, 0.f, 0.f, 0.f, 1.f }, Wt[9] = { 0.f, 1.f, 0.f, -1.f, 0.f, 0.f, 0.f, 0.f, 1.f };
            float R1[9], R2[9];
            sgx_init_mul3(U, W, 1.0, tmp); sgx_init_mul3(tmp, Vt, 1.0, R1);
            if (sgx_init_det3(R1) < 0) for (int k = 0; k < 9; k++) R1[k] = -R1[k];
            sgx_init_mul3(U, Wt, 1.0, tmp); sgx_init_mul3(tmp, Vt, 1.0, R2);
            if (sgx_init_det3(R2) < 0) for (int k = 0; k < 9; k++) R2[k] = -R2[k];
            for (int i = 0; i < 4; i++) {
                float *R = rt + 12 * i;
                for (int k = 0; k < 9; k++) R[k] = (i & 1) ? R2[k] : R1[k];
                for (int k = 0; k < 3; k++) R[9 + k] = i < 2 ? t[k] : -t[k];
            }
        }
        rep->n_hyp = nhyp;
        A.dec[2 * b] = model; A.dec[2 * b + 1] = nhyp;
    }
    SGX_THREADS_END
}

// one lane per (pair, hypothesis, match): the body of CheckRT's loop (:830-894) with Triangulate (:734-747)
SGX_KERNEL(256) k_init_check_rt(SgxInitArgs A)
{
    SGX_THREADS_BEGIN(tid)
    const int b = (int)blockIdx.y, hy = (int)blockIdx.z, i = (int)blockIdx.x * 256 + tid;
    const int N = A.nmatch[b], o1 = A.off1[b], model = A.dec[2 * b];
    if (i < N && hy < A.dec[2 * b + 1]) {
        const size_t slot = (size_t)hy * A.ntot + o1 + i;
        uint8_t g = 0; float cosParallax = 0.f, X[3] = { 0.f, 0.f, 0.f };
        do {
            if (!A.inl[(size_t)model * A.ntot + o1 + i]) break;
            const float *c = A.cam + 4 * b;
            const float fx = c[0], fy = c[1], cx = c[2], cy = c[3];
            const float *R = A.rt + 96 * (size_t)b + 12 * hy, *t = R + 9;
            const float sigma = A.sigma[b];
            const float th2 = (float)(4.0 * (double)(sigma * sigma));
            const float K[9] = { fx, 0.f, cx, 0.f, fy, cy, 0.f, 0.f, 1.f };
            const float P1[12] = { fx, 0.f, cx, 0.f, 0.f, fy, cy, 0.f, 0.f, 0.f, 1.f, 0.f };
            float P2[12];
            for (int r = 0; r < 3; r++)
                for (int q = 0; q < 4; q++) {
                    const float b0 = q < 3 ? R[q] : t[0], b1 = q < 3 ? R[3 + q] : t[1], b2 = q < 3 ? R[6 + q] : t[2];
                    const float d = K[3 * r] * b0 + K[3 * r + 1] * b1 + K[3 * r + 2] * b2;
                    P2[4 * r + q] = (float)((double)d * 1.0);
                }
            float O2[3];
            for (int r = 0; r < 3; r++) { double s = 0; for (int k = 0; k < 3; k++) s += (double)R[3 * k + r] * (double)t[k]; O2[r] = (float)(s * -1.0); }
            const float *xy = A.mxy + 4 * (size_t)(o1 + i);
            float M[16], At[16], Vt[16]; double W[4];
            for (int k = 0; k < 4; k++) {
                M[k] = xy[0] * P1[8 + k] - P1[k]; M[4 + k] = xy[1] * P1[8 + k] - P1[4 + k];
                M[8 + k] = xy[2] * P2[8 + k] - P2[k]; M[12 + k] = xy[3] * P2[8 + k] - P2[4 + k];
            }
            for (int r = 0; r < 4; r++) for (int k = 0; k < 4; k++) At[4 * r + k] = M[4 * k + r];
            sgx_init_jacobi(At, W, Vt, 1, 4, 4, 0);
            const float inv = (float)(1.0 / (double)Vt[15]);
            X[0] = Vt[12] * inv; X[1] = Vt[13] * inv; X[2] = Vt[14] * inv;
            if (!isfinite(X[0]) || !isfinite(X[1]) || !isfinite(X[2])) break;
            const float n2[3] = { X[0] - O2[0], X[1] - O2[1], X[2] - O2[2] };
            const float dist1 = (float)sqrt(sgx_init_dot3d(X, X)), dist2 = (float)sqrt(sgx_init_dot3d(n2, n2));
            cosParallax = (float)(sgx_init_dot3d(X, n2) / (double)(dist1 * dist2));
            if (X[2] <= 0 && (double)cosParallax < 0.99998) break;
            float X2[3];
            for (int r = 0; r < 3; r++) { const float d = R[3 * r] * X[0] + R[3 * r + 1] * X[1] + R[3 * r + 2] * X[2]; X2[r] = (float)((double)d * 1.0 + (double)t[r] * 1.0); }
            if (X2[2] <= 0 && (double)cosParallax < 0.99998) break;
            const float invZ1 = (float)(1.0 / (double)X[2]);
            const float im1x = fx * X[0] * invZ1 + cx, im1y = fy * X[1] * invZ1 + cy;
            const float squareError1 = (im1x - xy[0]) * (im1x - xy[0]) + (im1y - xy[1]) * (im1y - xy[1]);
            if (squareError1 > th2) break;
            const float invZ2 = (float)(1.0 / (double)X2[2]);
            const float im2x = fx * X2[0] * invZ2 + cx, im2y = fy * X2[1] * invZ2 + cy;
            const float squareError2 = (im2x - xy[2]) * (im2x - xy[2]) + (im2y - xy[3]) * (im2y - xy[3]);
            if (squareError2 > th2) break;
            g = (double)cosParallax < 0.99998 ? 2 : 1;
        } while (0);
        A.good[slot] = g; A.cosp[slot] = cosParallax;
        A.pts[3 * slot] = X[0]; A.pts[3 * slot + 1] = X[1]; A.pts[3 * slot + 2] = X[2];
    }
    SGX_THREADS_END
}

// one workgroup per pair: nGood and the sorted vCosParallax[min(50, nGood - 1)] of every hypothesis (:896-904, the element found by its rank), then the selection rule of
// ReconstructH (:689-731) or ReconstructF (:499-569) and the outputs
SGX_KERNEL(256) k_init_finish(SgxInitArgs A)
{
    SGX_LDS int s_ngood[8], s_win;
    SGX_LDS float s_cos[8];
    const int b = (int)blockIdx.x;
    const int N = A.nmatch[b], o1 = A.off1[b], n1 = A.off1[b + 1] - o1, model = A.dec[2 * b], nhyp = A.dec[2 * b + 1];
    SGX_THREADS_BEGIN(tid)
    if (tid < 8) { s_ngood[tid] = 0; s_cos[tid] = 0.f; }
    for (int i = tid; i < n1; i += 256) { A.tri[o1 + i] = 0; A.inl_out[o1 + i] = 0; A.p3d[3 * (size_t)(o1 + i)] = 0.f; A.p3d[3 * (size_t)(o1 + i) + 1] = 0.f; A.p3d[3 * (size_t)(o1 + i) + 2] = 0.f; }
    SGX_THREADS_END
    SGX_SYNC();
    SGX_THREADS_BEGIN(tid)
    for (int q = tid; q < nhyp * N; q += 256) { const int hy = q / N, i = q - hy * N; if (A.good[(size_t)hy * A.ntot + o1 + i]) sgx_atomic_add(&s_ngood[hy], 1); }
    SGX_THREADS_END
    SGX_SYNC();
    SGX_THREADS_BEGIN(tid)
    for (int q = tid; q < nhyp * N; q += 256) {
        const int hy = q / N, i = q - hy * N;
        const uint8_t *g = A.good + (size_t)hy * A.ntot + o1; const float *cp = A.cosp + (size_t)hy * A.ntot + o1;
        if (g[i]) {
            const int want = s_ngood[hy] - 1 < 50 ? s_ngood[hy] - 1 : 50;
            const float ci = cp[i];
            int rank = 0;
            for (int j = 0; j < N; j++) if (g[j] && (cp[j] < ci || (cp[j] == ci && j < i))) rank++;
            if (rank == want) s_cos[hy] = ci;                       // one element has this rank (none if a cosine is NaN: the gate then fails)
        }
    }
    SGX_THREADS_END
    SGX_SYNC();
    SGX_THREADS_BEGIN(tid)
    if (tid == 0) {
        SgxInitReport *rep = A.report + b;
        const int Nin = A.ninl[2 * b + model];
        int win = -1, best = -1;
        bool pass[8];
        for (int k = 0; k < 8; k++) {
            rep->n_good[k] = k < nhyp ? s_ngood[k] : 0; rep->cos_parallax[k] = k < nhyp ? s_cos[k] : 0.f;
            const float cg = model == 0 ? A.cos_ge : A.cos_gt;
            pass[k] = k < nhyp && s_ngood[k] > 0 && s_cos[k] >= -1.f && s_cos[k] <= cg;          // parallax >= (H) / > (F) minParallax; parallax = 0 when nGood = 0
        }
        if (nhyp == 8) {
            int bestGood = 0, secondBestGood = 0;
            for (int k = 0; k < 8; k++) {
                const int nGood = s_ngood[k];
                if (nGood > bestGood) { secondBestGood = bestGood; bestGood = nGood; best = k; }
                else if (nGood > secondBestGood) secondBestGood = nGood;
            }
            if (best >= 0 && (double)secondBestGood < 0.75 * bestGood && pass[best] && bestGood > 50 && (double)bestGood > 0.9 * Nin) win = best;
        } else if (nhyp == 4) {
            int maxGood = 0;
            for (int k = 0; k < 4; k++) if (s_ngood[k] > maxGood) maxGood = s_ngood[k];
            const int nMinGood = (int)(0.9 * Nin) > 50 ? (int)(0.9 * Nin) : 50;
            int nsimilar = 0;
            for (int k = 0; k < 4; k++) if ((double)s_ngood[k] > 0.7 * maxGood) nsimilar++;
            for (int k = 3; k >= 0; k--) if (s_ngood[k] == maxGood) best = k;         // the else-if chain tests the parallax of the first hypothesis equal to maxGood only
            if (!(maxGood < nMinGood || nsimilar > 1) && pass[best]) win = best;
        }
        rep->best_hyp = best;
        A.ok[b] = win >= 0 ? 1 : 0;
        for (int k = 0; k < 9; k++) A.R21[9 * b + k] = win >= 0 ? A.rt[96 * (size_t)b + 12 * win + k] : 0.f;
        for (int k = 0; k < 3; k++) A.t21[3 * b + k] = win >= 0 ? A.rt[96 * (size_t)b + 12 * win + 9 + k] : 0.f;
        s_win = win;
    }
    SGX_THREADS_END
    SGX_SYNC();
    SGX_THREADS_BEGIN(tid)
    const bool have = N >= 8 && A.best[10 * (2 * b + model)] > 0.f;
    for (int i = tid; i < N; i += 256) {
        const int i1 = A.mi[2 * (size_t)(o1 + i)];
        if (have) A.inl_out[o1 + i1] = A.inl[(size_t)model * A.ntot + o1 + i];
        if (s_win >= 0) {
            const size_t slot = (size_t)s_win * A.ntot + o1 + i;
            const uint8_t g = A.good[slot];
            if (g) { A.p3d[3 * (size_t)(o1 + i1)] = A.pts[3 * slot]; A.p3d[3 * (size_t)(o1 + i1) + 1] = A.pts[3 * slot + 1]; A.p3d[3 * (size_t)(o1 + i1) + 2] = A.pts[3 * slot + 2]; }
            A.tri[o1 + i1] = g == 2 ? 1 : 0;
        }
    }
    SGX_THREADS_END
}
