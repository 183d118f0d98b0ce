// sgx_pnp_kernels.h — PnPsolver (src/sg-slam/src/PnPsolver.cc), the EPnP RANSAC of Tracking::Relocalization (Tracking.cc:1504-1530):
//   iterate :165-257, Refine :260-306, CheckInliers :308-340, compute_pose :477-525 and everything it calls (EPnP, Lepetit et al. 2009).
// The OpenCV C calls of the reference are restated from OpenCV 3.4's published algorithm (lapack.cpp / matmul.cpp, no LAPACK):
//   cvSVD / cv::SVD::compute = JacobiSVDImpl_<double> (one-sided Jacobi on A^T, hypot as sgx_pnp_hypot below, max(m, 30) sweeps, descending sort, normalised U rows, zero singular values completed
//   from RNG(0x12345678)); cvSolve / cvInvert with CV_SVD = SVBkSb (singular values <= 2 DBL_EPSILON * sum(w) dropped); cvMulTransposed = MulTransposedR (each entry one
//   sequential sum over the rows).  Every expression is evaluated in the order written there (-ffp-contract=off), so the emulator equals tests/pnp_ref.py bit for bit.
// Two places where the reference's behaviour is undefined get one defined behaviour here:
//   - qr_solve on a singular A (:887-890) returns without writing X, and gauss_newton adds the uninitialised x: here that Gauss-Newton step makes no update.
//   - find_betas_approx_3 (:756) and _1 divide by betas[0], which can be 0: plain IEEE arithmetic (inf / NaN propagate; a NaN pose has no inliers).
// Layout: k_pnp_hyp = one lane per hypothesis (four draws with the swap-and-pop of vAvailableIndices, EPnP on four points in fp64); k_pnp_count = one workgroup per
// solver counts the inliers of all its hypotheses over all its correspondences; k_pnp_replay = one workgroup per solver replays the accept rule in iteration order and
// runs Refine once per distinct best-so-far set (a failed Refine on the same set fails again), with MtM accumulated one lane per entry.
#pragma once
#include "sgx_rt.h"
#include <math.h>
#include <float.h>

#define SGX_PNP_MAXIT 512            /* hypotheses per solver and launch, at most (the batch sizes its buffers to max(nIterations, mRansacMaxIts) up to this) */
#define SGX_PNP_HYP 12               /* doubles per hypothesis: R 9 | t 3 */
#define SGX_PNP_ST 8                 /* ints of persistent solver state */
enum { SGX_PNP_N = 0, SGX_PNP_MININ = 1, SGX_PNP_MAXITS = 2, SGX_PNP_ITS = 3, SGX_PNP_BEST = 4, SGX_PNP_BEST_FAILED = 5 };
#define SGX_PNP_CS 4                 /* ints of per-call state: found iteration (-1), iterations run, hypotheses of the call, refined inliers */

struct SgxPnpArgs {
    int B, n_iterations, chunk0, chunk_n, cap;      // this launch covers call iterations [chunk0, chunk0 + chunk_n) of every solver; cap = hypotheses per solver in hyp / counts
    const int *offsets;                             // B + 1: correspondences of solver b = [offsets[b], offsets[b + 1])
    const float *p2d, *p3dw, *sigma2;               // concatenated mvP2D (x, y), mvP3Dw (x, y, z), mvSigma2
    const float *cam;                               // B x 4: fu, fv, uc, vc
    const float *th2;                               // B: mvMaxError = sigma2 * th2
    const int *draws; int draw_stride, draw_base;   // raw rand() values: solver b, call iteration h -> draws[b * draw_stride + 4 * (h - draw_base) + k]
    int *state;                                     // B x SGX_PNP_ST (persistent)
    float *best_tcw;                                // B x 16 (persistent mBestTcw)
    uint8_t *best_mask;                             // concatenated mvbBestInliers (persistent)
    int *call;                                      // B x SGX_PNP_CS
    double *hyp;                                    // B x cap x SGX_PNP_HYP
    int *counts;                                    // B x cap
    double *ws;                                     // concatenated Refine workspace: 3 (pws) + 2 (us) + 4 (alphas) + 3 (pcs) + 24 (M) doubles per correspondence
    float *tcw_out;                                 // B x 16: the returned model
    uint8_t *inl_out;                               // concatenated vbInliers of the returned model
};

// the call's hypothesis count: while(mnIterations < mRansacMaxIts || nCurrentIterations < nIterations) (:182) runs max(nIterations, mRansacMaxIts - mnIterations)
SGX_DEV int sgx_pnp_call_total(const int *st, int n_iterations)
{
    if (st[SGX_PNP_N] < st[SGX_PNP_MININ]) return 0;
    const int a = n_iterations, b = st[SGX_PNP_MAXITS] - st[SGX_PNP_ITS];
    const int m = a > b ? a : b;
    return m > 0 ? m : 0;
}

// ---------------------------------------------------------------------------------------------------------------------------------------------------- OpenCV algebra
// hypot of the Jacobi rotation.  OpenCV calls std::hypot, whose last bit differs between glibc and the device library; EPnP on four points amplifies such a bit
// through the four-dimensional null space of MtM (the approximations use subsets of a basis that rounding alone decides), so a libm hypot would make the device's
// hypotheses differ from the CPU's.  This form uses only correctly rounded operations, so the device, the emulator and tests/pnp_ref.py agree bit for bit.
SGX_DEV double sgx_pnp_hypot(double x, double y)
{
    double a = fabs(x), b = fabs(y);
    if (a < b) { const double t = a; a = b; b = t; }
    if (a == 0 || b == 0) return a + b;
    const double r = b / a;
    return a * sqrt(1.0 + r * r);
}

// JacobiSVDImpl_<double>(At, W, Vt, m, n, n1 = n, DBL_MIN, DBL_EPSILON * 10): At is n x m (row stride m), Vt n x n.  On return W is descending, the rows of At are the
// normalised left singular vectors (U^T) and Vt the right ones.
SGX_DEV void sgx_pnp_jacobi(double *At, double *W, double *Vt, int m, int n)
{
    const double minval = DBL_MIN, eps = DBL_EPSILON * 10;
    const int max_iter = m > 30 ? m : 30;
    for (int i = 0; i < n; i++) {
        double sd = 0;
        for (int k = 0; k < m; k++) { const double t = At[i * m + k]; sd += t * t; }
        W[i] = sd;
        for (int k = 0; k < n; k++) Vt[i * n + k] = 0;
        Vt[i * n + i] = 1;
    }
    for (int iter = 0; iter < max_iter; iter++) {
        bool changed = false;
        for (int i = 0; i < n - 1; i++)
            for (int j = i + 1; j < n; j++) {
                double *Ai = At + i * m, *Aj = At + j * m;
                double a = W[i], p = 0, b = W[j];
                for (int k = 0; k < m; k++) p += Ai[k] * Aj[k];
                if (fabs(p) <= eps * sqrt(a * b)) continue;
                p *= 2;
                const double beta = a - b, gamma = sgx_pnp_hypot(p, beta);
                double c, s;
                if (beta < 0) { const double delta = (gamma - beta) * 0.5; s = sqrt(delta / gamma); c = p / (gamma * s * 2); }
                else { c = sqrt((gamma + beta) / (gamma * 2)); s = p / (gamma * c * 2); }
                a = b = 0;
                for (int k = 0; k < m; k++) {
                    const double t0 = c * Ai[k] + s * Aj[k], t1 = -s * Ai[k] + c * Aj[k];
                    Ai[k] = t0; Aj[k] = t1;
                    a += t0 * t0; b += t1 * t1;
                }
                W[i] = a; W[j] = b;
                changed = true;
                double *Vi = Vt + i * n, *Vj = Vt + j * n;
                for (int k = 0; k < n; k++) { const double t0 = c * Vi[k] + s * Vj[k], t1 = -s * Vi[k] + c * Vj[k]; Vi[k] = t0; Vj[k] = t1; }
            }
        if (!changed) break;
    }
    for (int i = 0; i < n; i++) {
        double sd = 0;
        for (int k = 0; k < m; k++) { const double t = At[i * m + k]; sd += t * t; }
        W[i] = sqrt(sd);
    }
    for (int i = 0; i < n - 1; i++) {
        int j = i;
        for (int k = i + 1; k < n; k++) if (W[j] < W[k]) j = k;
        if (i != j) {
            const double tw = W[i]; W[i] = W[j]; W[j] = tw;
            for (int k = 0; k < m; k++) { const double t = At[i * m + k]; At[i * m + k] = At[j * m + k]; At[j * m + k] = t; }
            for (int k = 0; k < n; k++) { const double t = Vt[i * n + k]; Vt[i * n + k] = Vt[j * n + k]; Vt[j * n + k] = t; }
        }
    }
    uint64_t rng = 0x12345678u;                                  // cv::RNG(0x12345678), advanced only by the completion of zero singular values
    for (int i = 0; i < n; i++) {
        double sd = W[i];
        for (int ii = 0; ii < 100 && sd <= minval; ii++) {
            const double val0 = 1. / m;
            for (int k = 0; k < m; k++) {
                rng = (uint64_t)(unsigned)rng * 4164903690u + (unsigned)(rng >> 32);
                At[i * m + k] = ((unsigned)rng & 256) != 0 ? val0 : -val0;
            }
            for (int it = 0; it < 2; it++)
                for (int j = 0; j < i; j++) {
                    sd = 0;
                    for (int k = 0; k < m; k++) sd += At[i * m + k] * At[j * m + k];
                    double asum = 0;
                    for (int k = 0; k < m; k++) { const double t = At[i * m + k] - sd * At[j * m + k]; At[i * m + k] = t; asum += fabs(t); }
                    asum = asum > eps * 100 ? 1 / asum : 0;
                    for (int k = 0; k < m; k++) At[i * m + k] *= asum;
                }
            sd = 0;
            for (int k = 0; k < m; k++) { const double t = At[i * m + k]; sd += t * t; }
            sd = sqrt(sd);
        }
        const double s = sd > minval ? 1 / sd : 0.;
        for (int k = 0; k < m; k++) At[i * m + k] *= s;
    }
}

// cvSolve(A, b, x, CV_SVD) for an m x n A (m = 6 >= n): At = A^T, JacobiSVD, SVBkSb with nb = 1
SGX_DEV void sgx_pnp_solve_svd(const double *A, int m, int n, const double *b, double *x)
{
    double At[5 * 6], W[5], Vt[5 * 5];
    for (int i = 0; i < n; i++) for (int k = 0; k < m; k++) At[i * m + k] = A[k * n + i];
    sgx_pnp_jacobi(At, W, Vt, m, n);
    double threshold = 0;
    for (int i = 0; i < n; i++) x[i] = 0;
    for (int i = 0; i < n; i++) threshold += W[i];
    threshold *= DBL_EPSILON * 2;
    for (int i = 0; i < n; i++) {
        double wi = W[i];
        if (fabs(wi) <= threshold) continue;
        wi = 1 / wi;
        double s = 0;
        for (int j = 0; j < m; j++) s += At[i * m + j] * b[j];
        s *= wi;
        for (int j = 0; j < n; j++) x[j] = x[j] + s * Vt[i * n + j];
    }
}

// cvInvert(CC, CC_inv, CV_SVD) on a 3 x 3 matrix: SVD::compute + SVD::backSubst(w, u, vt, noArray())
SGX_DEV void sgx_pnp_invert3(const double *A, double *X)
{
    double At[9], W[3], Vt[9], buf[3];
    for (int i = 0; i < 3; i++) for (int k = 0; k < 3; k++) At[i * 3 + k] = A[k * 3 + i];
    sgx_pnp_jacobi(At, W, Vt, 3, 3);
    double threshold = 0;
    for (int i = 0; i < 9; i++) X[i] = 0;
    for (int i = 0; i < 3; i++) threshold += W[i];
    threshold *= DBL_EPSILON * 2;
    for (int i = 0; i < 3; i++) {
        double wi = W[i];
        if (fabs(wi) <= threshold) continue;
        wi = 1 / wi;
        for (int j = 0; j < 3; j++) buf[j] = At[i * 3 + j] * wi;
        for (int r = 0; r < 3; r++) { const double s = Vt[i * 3 + r]; for (int j = 0; j < 3; j++) X[r * 3 + j] = X[r * 3 + j] + s * buf[j]; }
    }
}

// ---------------------------------------------------------------------------------------------------------------------------------------------------- EPnP
struct SgxEpnpCam { double fu, fv, uc, vc; };

SGX_DEV double sgx_pnp_dot(const double *a, const double *b) { return a[0] * b[0] + a[1] * b[1] + a[2] * b[2]; }
SGX_DEV double sgx_pnp_dist2(const double *a, const double *b) { return (a[0] - b[0]) * (a[0] - b[0]) + (a[1] - b[1]) * (a[1] - b[1]) + (a[2] - b[2]) * (a[2] - b[2]); }

// choose_control_points (:375-409) + the inverse of compute_barycentric_coordinates (:411-421)
SGX_DEV void sgx_epnp_control_points(const double *pws, int n, double *cws /* 4 x 3 */, double *ccinv /* 3 x 3 */)
{
    cws[0] = cws[1] = cws[2] = 0;
    for (int i = 0; i < n; i++) for (int j = 0; j < 3; j++) cws[j] += pws[3 * i + j];
    for (int j = 0; j < 3; j++) cws[j] /= n;
    double pp[9], dc[3], Vt[9];
    for (int a = 0; a < 3; a++)
        for (int b = a; b < 3; b++) {                           // cvMulTransposed(PW0, PW0tPW0, 1)
            double s = 0;
            for (int k = 0; k < n; k++) s += (pws[3 * k + a] - cws[a]) * (pws[3 * k + b] - cws[b]);
            pp[3 * a + b] = s; pp[3 * b + a] = s;
        }
    sgx_pnp_jacobi(pp, dc, Vt, 3, 3);                            // cvSVD(MODIFY_A | U_T) of a symmetric matrix: uct = the rotated rows
    for (int i = 1; i < 4; i++) {
        const double k = sqrt(dc[i - 1] / n);
        for (int j = 0; j < 3; j++) cws[3 * i + j] = cws[j] + k * pp[3 * (i - 1) + j];
    }
    double cc[9];
    for (int i = 0; i < 3; i++) for (int j = 1; j < 4; j++) cc[3 * i + j - 1] = cws[3 * j + i] - cws[i];
    sgx_pnp_invert3(cc, ccinv);
}

// compute_barycentric_coordinates' per-point part (:423-433) and fill_M (:436-451) of one correspondence
SGX_DEV void sgx_epnp_alphas_M(const double *pi, const double *ui, const double *cws, const double *ci, const SgxEpnpCam &cam, double *a, double *M /* 2 x 12 */)
{
    for (int j = 0; j < 3; j++) a[1 + j] = ci[3 * j] * (pi[0] - cws[0]) + ci[3 * j + 1] * (pi[1] - cws[1]) + ci[3 * j + 2] * (pi[2] - cws[2]);
    a[0] = 1.0 - a[1] - a[2] - a[3];
    for (int i = 0; i < 4; i++) {
        M[3 * i] = a[i] * cam.fu; M[3 * i + 1] = 0.0; M[3 * i + 2] = a[i] * (cam.uc - ui[0]);
        M[12 + 3 * i] = 0.0; M[12 + 3 * i + 1] = a[i] * cam.fv; M[12 + 3 * i + 2] = a[i] * (cam.vc - ui[1]);
    }
}

// qr_solve (:860-950) on A 6 x 4; false on a singular A (X not written)
SGX_DEV bool sgx_epnp_qr_solve(double *A, double *b, double *X)
{
    const int nr = 6, nc = 4;
    double A1[4], A2[4];
    for (int k = 0; k < nc; k++) {
        double eta = fabs(A[k * nc + k]);                         // the reference reads ppAik before advancing it (:880-885): rows k .. nr - 2, the last row is not scanned
        for (int i = k + 1; i < nr; i++) { const double elt = fabs(A[(i - 1) * nc + k]); if (eta < elt) eta = elt; }
        if (eta == 0) return false;
        double sum = 0.0; const double inv_eta = 1. / eta;
        for (int i = k; i < nr; i++) { A[i * nc + k] *= inv_eta; sum += A[i * nc + k] * A[i * nc + k]; }
        double sigma = sqrt(sum);
        if (A[k * nc + k] < 0) sigma = -sigma;
        A[k * nc + k] += sigma;
        A1[k] = sigma * A[k * nc + k];
        A2[k] = -eta * sigma;
        for (int j = k + 1; j < nc; j++) {
            double s = 0;
            for (int i = k; i < nr; i++) s += A[i * nc + k] * A[i * nc + j];
            const double tau = s / A1[k];
            for (int i = k; i < nr; i++) A[i * nc + j] -= tau * A[i * nc + k];
        }
    }
    for (int j = 0; j < nc; j++) {
        double tau = 0;
        for (int i = j; i < nr; i++) tau += A[i * nc + j] * b[i];
        tau /= A1[j];
        for (int i = j; i < nr; i++) b[i] -= tau * A[i * nc + j];
    }
    X[nc - 1] = b[nc - 1] / A2[nc - 1];
    for (int i = nc - 2; i >= 0; i--) {
        double s = 0;
        for (int j = i + 1; j < nc; j++) s += A[i * nc + j] * X[j];
        X[i] = (b[i] - s) / A2[i];
    }
    return true;
}

// gauss_newton (:840-858) with compute_A_and_b_gauss_newton (:812-838)
SGX_DEV void sgx_epnp_gauss_newton(const double *L, const double *rho, double *betas)
{
    for (int it = 0; it < 5; it++) {
        double A[24], b[6], x[4];
        for (int i = 0; i < 6; i++) {
            const double *r = L + 10 * i;
            A[4 * i] = 2 * r[0] * betas[0] + r[1] * betas[1] + r[3] * betas[2] + r[6] * betas[3];
            A[4 * i + 1] = r[1] * betas[0] + 2 * r[2] * betas[1] + r[4] * betas[2] + r[7] * betas[3];
            A[4 * i + 2] = r[3] * betas[0] + r[4] * betas[1] + 2 * r[5] * betas[2] + r[8] * betas[3];
            A[4 * i + 3] = r[6] * betas[0] + r[7] * betas[1] + r[8] * betas[2] + 2 * r[9] * betas[3];
            b[i] = rho[i] - (r[0] * betas[0] * betas[0] + r[1] * betas[0] * betas[1] + r[2] * betas[1] * betas[1] + r[3] * betas[0] * betas[2] +
                             r[4] * betas[1] * betas[2] + r[5] * betas[2] * betas[2] + r[6] * betas[0] * betas[3] + r[7] * betas[1] * betas[3] +
                             r[8] * betas[2] * betas[3] + r[9] * betas[3] * betas[3]);
        }
        if (!sgx_epnp_qr_solve(A, b, x)) continue;              // singular A: no update (the reference adds an uninitialised x)
        for (int i = 0; i < 4; i++) betas[i] += x[i];
    }
}

// the three beta approximations (:667-758)
SGX_DEV void sgx_epnp_betas(const double *L, const double *rho, int which, double *betas)
{
    double A[6 * 5], b[5];
    const int cols1[4] = { 0, 1, 3, 6 };
    const int nc = which == 1 ? 4 : which == 2 ? 3 : 5;
    for (int i = 0; i < 6; i++) for (int c = 0; c < nc; c++) A[i * nc + c] = L[10 * i + (which == 1 ? cols1[c] : c)];
    sgx_pnp_solve_svd(A, 6, nc, rho, b);
    if (which == 1) {
        if (b[0] < 0) { betas[0] = sqrt(-b[0]); betas[1] = -b[1] / betas[0]; betas[2] = -b[2] / betas[0]; betas[3] = -b[3] / betas[0]; }
        else { betas[0] = sqrt(b[0]); betas[1] = b[1] / betas[0]; betas[2] = b[2] / betas[0]; betas[3] = b[3] / betas[0]; }
        return;
    }
    if (b[0] < 0) { betas[0] = sqrt(-b[0]); betas[1] = (b[2] < 0) ? sqrt(-b[2]) : 0.0; }
    else { betas[0] = sqrt(b[0]); betas[1] = (b[2] > 0) ? sqrt(b[2]) : 0.0; }
    if (b[1] < 0) betas[0] = -betas[0];
    betas[2] = which == 2 ? 0.0 : b[3] / betas[0];             // approx 3 divides by betas[0] (may be 0: IEEE)
    betas[3] = 0.0;
}

// compute_R_and_t (:651-662): compute_ccs, compute_pcs, solve_for_sign, estimate_R_and_t (cvSVD of ABt, det < 0 row flip), reprojection_error
SGX_DEV double sgx_epnp_R_and_t(const double *pws, const double *us, const double *alphas, double *pcs, int n, const double *ut, const double *betas,
                                const SgxEpnpCam &cam, double *R /* 3 x 3 */, double *t)
{
    double ccs[12];
    for (int i = 0; i < 12; i++) ccs[i] = 0.0;
    for (int i = 0; i < 4; i++) { const double *v = ut + 12 * (11 - i); for (int j = 0; j < 4; j++) for (int k = 0; k < 3; k++) ccs[3 * j + k] += betas[i] * v[3 * j + k]; }
    for (int i = 0; i < n; i++) {
        const double *a = alphas + 4 * i; double *pc = pcs + 3 * i;
        for (int j = 0; j < 3; j++) pc[j] = a[0] * ccs[j] + a[1] * ccs[3 + j] + a[2] * ccs[6 + j] + a[3] * ccs[9 + j];
    }
    if (pcs[2] < 0.0) {
        for (int i = 0; i < 12; i++) ccs[i] = -ccs[i];
        for (int i = 0; i < 3 * n; i++) pcs[i] = -pcs[i];
    }
    double pc0[3] = { 0.0, 0.0, 0.0 }, pw0[3] = { 0.0, 0.0, 0.0 };
    for (int i = 0; i < n; i++) for (int j = 0; j < 3; j++) { pc0[j] += pcs[3 * i + j]; pw0[j] += pws[3 * i + j]; }
    for (int j = 0; j < 3; j++) { pc0[j] /= n; pw0[j] /= n; }
    double abt[9];
    for (int i = 0; i < 9; i++) abt[i] = 0;
    for (int i = 0; i < n; i++) {
        const double *pc = pcs + 3 * i, *pw = pws + 3 * i;
        for (int j = 0; j < 3; j++) {
            abt[3 * j] += (pc[j] - pc0[j]) * (pw[0] - pw0[0]);
            abt[3 * j + 1] += (pc[j] - pc0[j]) * (pw[1] - pw0[1]);
            abt[3 * j + 2] += (pc[j] - pc0[j]) * (pw[2] - pw0[2]);
        }
    }
    double At[9], W[3], Vt[9];                                   // cvSVD(ABt, D, U, V, MODIFY_A): U = At^T, V = Vt^T
    for (int i = 0; i < 3; i++) for (int k = 0; k < 3; k++) At[3 * i + k] = abt[3 * k + i];
    sgx_pnp_jacobi(At, W, Vt, 3, 3);
    for (int i = 0; i < 3; i++)
        for (int j = 0; j < 3; j++) R[3 * i + j] = At[i] * Vt[j] + At[3 + i] * Vt[3 + j] + At[6 + i] * Vt[6 + j];
    const double det = R[0] * R[4] * R[8] + R[1] * R[5] * R[6] + R[2] * R[3] * R[7] - R[2] * R[4] * R[6] - R[1] * R[3] * R[8] - R[0] * R[5] * R[7];
    if (det < 0) { R[6] = -R[6]; R[7] = -R[7]; R[8] = -R[8]; }
    for (int i = 0; i < 3; i++) t[i] = pc0[i] - sgx_pnp_dot(R + 3 * i, pw0);
    double sum2 = 0.0;
    for (int i = 0; i < n; i++) {
        const double *pw = pws + 3 * i;
        const double Xc = sgx_pnp_dot(R, pw) + t[0], Yc = sgx_pnp_dot(R + 3, pw) + t[1], inv_Zc = 1.0 / (sgx_pnp_dot(R + 6, pw) + t[2]);
        const double ue = cam.uc + cam.fu * Xc * inv_Zc, ve = cam.vc + cam.fv * Yc * inv_Zc;
        const double u = us[2 * i], v = us[2 * i + 1];
        sum2 += sqrt((u - ue) * (u - ue) + (v - ve) * (v - ve));
    }
    return sum2 / n;
}

// compute_pose (:477-525) after MtM: its SVD, L_6x10, rho, the three approximations + Gauss-Newton, the smallest reprojection error wins (<).  mtm is destroyed.
SGX_DEV void sgx_epnp_finish(const double *pws, const double *us, const double *alphas, double *pcs, int n, const double *cws, double *mtm, const SgxEpnpCam &cam,
                             double *R, double *t)
{
    double d[12], Vt[144];
    sgx_pnp_jacobi(mtm, d, Vt, 12, 12);                          // cvSVD(MtM, D, Ut, 0, MODIFY_A | U_T): ut = the rotated rows
    const double *ut = mtm;
    double L[60], rho[6];
    {
        double dv[4][6][3];
        for (int i = 0; i < 4; i++) {
            const double *v = ut + 12 * (11 - i);
            int a = 0, b = 1;
            for (int j = 0; j < 6; j++) {
                for (int k = 0; k < 3; k++) dv[i][j][k] = v[3 * a + k] - v[3 * b + k];
                b++;
                if (b > 3) { a++; b = a + 1; }
            }
        }
        for (int i = 0; i < 6; i++) {
            double *row = L + 10 * i;
            row[0] = sgx_pnp_dot(dv[0][i], dv[0][i]);
            row[1] = 2.0 * sgx_pnp_dot(dv[0][i], dv[1][i]);
            row[2] = sgx_pnp_dot(dv[1][i], dv[1][i]);
            row[3] = 2.0 * sgx_pnp_dot(dv[0][i], dv[2][i]);
            row[4] = 2.0 * sgx_pnp_dot(dv[1][i], dv[2][i]);
            row[5] = sgx_pnp_dot(dv[2][i], dv[2][i]);
            row[6] = 2.0 * sgx_pnp_dot(dv[0][i], dv[3][i]);
            row[7] = 2.0 * sgx_pnp_dot(dv[1][i], dv[3][i]);
            row[8] = 2.0 * sgx_pnp_dot(dv[2][i], dv[3][i]);
            row[9] = sgx_pnp_dot(dv[3][i], dv[3][i]);
        }
        rho[0] = sgx_pnp_dist2(cws, cws + 3); rho[1] = sgx_pnp_dist2(cws, cws + 6); rho[2] = sgx_pnp_dist2(cws, cws + 9);
        rho[3] = sgx_pnp_dist2(cws + 3, cws + 6); rho[4] = sgx_pnp_dist2(cws + 3, cws + 9); rho[5] = sgx_pnp_dist2(cws + 6, cws + 9);
    }
    double bestR[9] = { 0 }, bestt[3] = { 0 }, best_err = 0;
    for (int which = 1; which <= 3; which++) {
        double betas[4], Rk[9], tk[3];
        sgx_epnp_betas(L, rho, which, betas);
        sgx_epnp_gauss_newton(L, rho, betas);
        const double err = sgx_epnp_R_and_t(pws, us, alphas, pcs, n, ut, betas, cam, Rk, tk);
        if (which == 1 || err < best_err) { best_err = err; for (int i = 0; i < 9; i++) bestR[i] = Rk[i]; for (int i = 0; i < 3; i++) bestt[i] = tk[i]; }
    }
    for (int i = 0; i < 9; i++) R[i] = bestR[i];
    for (int i = 0; i < 3; i++) t[i] = bestt[i];
}

// CheckInliers (:308-340) for one correspondence: float Xc / Yc / invZc from the double pose, double ue / ve, float distances and error
SGX_DEV bool sgx_pnp_inlier(const double *R, const double *t, const float *P3, const float *P2, const SgxEpnpCam &cam, float max_err)
{
    const float Xc = R[0] * P3[0] + R[1] * P3[1] + R[2] * P3[2] + t[0];
    const float Yc = R[3] * P3[0] + R[4] * P3[1] + R[5] * P3[2] + t[1];
    const float invZc = 1 / (R[6] * P3[0] + R[7] * P3[1] + R[8] * P3[2] + t[2]);
    const double ue = cam.uc + cam.fu * Xc * invZc, ve = cam.vc + cam.fv * Yc * invZc;
    const float distX = P2[0] - ue, distY = P2[1] - ve;
    const float error2 = distX * distX + distY * distY;
    return error2 < max_err;
}

SGX_DEV SgxEpnpCam sgx_pnp_cam(const float *c) { SgxEpnpCam k; k.fu = c[0]; k.fv = c[1]; k.uc = c[2]; k.vc = c[3]; return k; }

// ---------------------------------------------------------------------------------------------------------------------------------------------------- kernels
// one lane per hypothesis: RandomInt(0, size - 1) four times with the swap-and-pop of vAvailableIndices (:191-201), then compute_pose on the four points
SGX_KERNEL(64) k_pnp_hyp(SgxPnpArgs A)
{
    SGX_THREADS_BEGIN(tid)
    const int b = (int)blockIdx.y, hl = (int)blockIdx.x * 64 + tid;
    const int *st = A.state + SGX_PNP_ST * b;
    const int total = sgx_pnp_call_total(st, A.n_iterations);
    const int h = A.chunk0 + hl;
    if (hl < A.chunk_n && h < total && A.call[SGX_PNP_CS * b] < 0) {
        const int N = st[SGX_PNP_N], o = A.offsets[b];
        int pos[4], val[4], nov = 0, idx[4];
        const double R1 = (double)2147483647 + 1.0;
        for (int k = 0; k < 4; k++) {
            const int size = N - k;
            int r = (int)(((double)A.draws[(size_t)b * A.draw_stride + 4 * (h - A.draw_base) + k] / R1) * size);
            r = r < 0 ? 0 : r >= size ? size - 1 : r;                // rand() is in [0, RAND_MAX]; a caller's value outside it cannot index out of bounds
            int v = r, back = size - 1;                              // vAvailableIndices[p] = the latest value written to position p, else p
            for (int q = 0; q < nov; q++) { if (pos[q] == r) v = val[q]; if (pos[q] == size - 1) back = val[q]; }
            idx[k] = v;
            pos[nov] = r; val[nov] = back; nov++;                 // vAvailableIndices[randi] = back(); pop_back()
        }
        double pws[12], us[8], alphas[16], pcs[12], M[96], mtm[144], cws[12], ci[9];
        for (int k = 0; k < 4; k++) {
            for (int j = 0; j < 3; j++) pws[3 * k + j] = A.p3dw[3 * (size_t)(o + idx[k]) + j];
            for (int j = 0; j < 2; j++) us[2 * k + j] = A.p2d[2 * (size_t)(o + idx[k]) + j];
        }
        const SgxEpnpCam cam = sgx_pnp_cam(A.cam + 4 * b);
        sgx_epnp_control_points(pws, 4, cws, ci);
        for (int k = 0; k < 4; k++) sgx_epnp_alphas_M(pws + 3 * k, us + 2 * k, cws, ci, cam, alphas + 4 * k, M + 24 * k);
        for (int a = 0; a < 12; a++)
            for (int c = a; c < 12; c++) { double s = 0; for (int r = 0; r < 8; r++) s += M[12 * r + a] * M[12 * r + c]; mtm[12 * a + c] = s; mtm[12 * c + a] = s; }
        double *out = A.hyp + ((size_t)b * A.cap + hl) * SGX_PNP_HYP;
        sgx_epnp_finish(pws, us, alphas, pcs, 4, cws, mtm, cam, out, out + 9);
    }
    SGX_THREADS_END
}

// one workgroup per solver: the inliers of every hypothesis of the chunk over all correspondences ((hypothesis, point) pairs dealt flat)
SGX_KERNEL(256) k_pnp_count(SgxPnpArgs A)
{
    SGX_LDS int cnt[SGX_PNP_MAXIT];
    const int b = (int)blockIdx.x;
    SGX_THREADS_BEGIN(tid)
    for (int h = tid; h < A.cap; h += 256) cnt[h] = 0;
    SGX_THREADS_END
    SGX_SYNC();
    SGX_THREADS_BEGIN(tid)
    const int *st = A.state + SGX_PNP_ST * b;
    const int total = sgx_pnp_call_total(st, A.n_iterations);
    int nh = total - A.chunk0; if (nh > A.chunk_n) nh = A.chunk_n; if (nh < 0 || A.call[SGX_PNP_CS * b] >= 0) nh = 0;
    const int N = st[SGX_PNP_N], o = A.offsets[b];
    const SgxEpnpCam cam = sgx_pnp_cam(A.cam + 4 * b);
    const float th2 = A.th2[b];
    for (int q = tid; q < nh * N; q += 256) {
        const int h = q / N, i = q - h * N;
        const double *hp = A.hyp + ((size_t)b * A.cap + h) * SGX_PNP_HYP;
        if (sgx_pnp_inlier(hp, hp + 9, A.p3dw + 3 * (size_t)(o + i), A.p2d + 2 * (size_t)(o + i), cam, A.sigma2[o + i] * th2)) sgx_atomic_add(&cnt[h], 1);
    }
    SGX_THREADS_END
    SGX_SYNC();
    SGX_THREADS_BEGIN(tid)
    for (int h = tid; h < A.cap; h += 256) A.counts[(size_t)b * A.cap + h] = cnt[h];
    SGX_THREADS_END
}

// one workgroup per solver: the accept rule (:209-237) in iteration order; Refine (:260-306) on the best-so-far set whenever that set has not failed before
SGX_KERNEL(256) k_pnp_replay(SgxPnpArgs A)
{
    SGX_LDS int s_h, s_new, s_nh, s_pos, s_nsel, s_cnt;
    SGX_LDS double s_cws[12], s_ci[9], s_mtm[144], s_R[12];
    const int b = (int)blockIdx.x;
    int *st = A.state + SGX_PNP_ST * b, *cs = A.call + SGX_PNP_CS * b;
    const int N = st[SGX_PNP_N], o = A.offsets[b];
    double *ws = A.ws + 36 * (size_t)o, *pws = ws, *us = ws + 3 * (size_t)N, *alphas = ws + 5 * (size_t)N, *pcs = ws + 9 * (size_t)N, *M = ws + 12 * (size_t)N;
    const SgxEpnpCam cam = sgx_pnp_cam(A.cam + 4 * b);
    const float th2 = A.th2[b];
    SGX_THREADS_BEGIN(tid)
    if (tid == 0) {
        const int total = sgx_pnp_call_total(st, A.n_iterations);
        int nh = total - A.chunk0; if (nh > A.chunk_n) nh = A.chunk_n; if (nh < 0 || cs[0] >= 0) nh = 0;
        s_nh = nh; s_pos = 0;
    }
    SGX_THREADS_END
    SGX_SYNC();
    for (;;) {
        SGX_THREADS_BEGIN(tid)
        if (tid == 0) {
            s_h = -1; s_new = 0;
            for (int h = s_pos; h < s_nh; h++) {
                const int c = A.counts[(size_t)b * A.cap + h];
                if (c < st[SGX_PNP_MININ]) continue;
                if (c > st[SGX_PNP_BEST]) { st[SGX_PNP_BEST] = c; st[SGX_PNP_BEST_FAILED] = 0; s_new = 1; }
                if (!st[SGX_PNP_BEST_FAILED]) { s_h = h; s_pos = h + 1; break; }
            }
            if (s_h < 0) cs[1] += s_nh;                          // no success in this chunk: all its hypotheses ran
        }
        SGX_THREADS_END
        SGX_SYNC();
        if (s_h < 0) break;
        if (s_new) {                                             // mvbBestInliers = mvbInliersi, mBestTcw = the hypothesis' pose in float
            SGX_THREADS_BEGIN(tid)
            const double *hp = A.hyp + ((size_t)b * A.cap + s_h) * SGX_PNP_HYP;
            for (int i = tid; i < N; i += 256)
                A.best_mask[o + i] = sgx_pnp_inlier(hp, hp + 9, A.p3dw + 3 * (size_t)(o + i), A.p2d + 2 * (size_t)(o + i), cam, A.sigma2[o + i] * th2) ? 1 : 0;
            if (tid < 16) { const int r = tid >> 2, c = tid & 3; A.best_tcw[16 * b + tid] = r == 3 ? (c == 3 ? 1.f : 0.f) : (float)(c < 3 ? hp[3 * r + c] : hp[9 + r]); }
            SGX_THREADS_END
            SGX_SYNC();
        }
        // Refine: gather the best inliers in index order
        SGX_THREADS_BEGIN(tid)
        if (tid == 0) {
            int n = 0;
            for (int i = 0; i < N; i++)
                if (A.best_mask[o + i]) {
                    for (int j = 0; j < 3; j++) pws[3 * n + j] = A.p3dw[3 * (size_t)(o + i) + j];
                    for (int j = 0; j < 2; j++) us[2 * n + j] = A.p2d[2 * (size_t)(o + i) + j];
                    n++;
                }
            s_nsel = n; s_cnt = 0;
            sgx_epnp_control_points(pws, n, s_cws, s_ci);
        }
        SGX_THREADS_END
        SGX_SYNC();
        SGX_THREADS_BEGIN(tid)
        for (int i = tid; i < s_nsel; i += 256) sgx_epnp_alphas_M(pws + 3 * i, us + 2 * i, s_cws, s_ci, cam, alphas + 4 * i, M + 24 * (size_t)i);
        SGX_THREADS_END
        SGX_SYNC();
        SGX_THREADS_BEGIN(tid)
        if (tid < 144) {                                         // cvMulTransposed(M, MtM, 1): one lane per entry, rows in order
            const int a = tid / 12, c = tid % 12;
            if (c >= a) {
                double s = 0;
                for (int r = 0; r < 2 * s_nsel; r++) s += M[12 * (size_t)r + a] * M[12 * (size_t)r + c];
                s_mtm[12 * a + c] = s; s_mtm[12 * c + a] = s;
            }
        }
        SGX_THREADS_END
        SGX_SYNC();
        SGX_THREADS_BEGIN(tid)
        if (tid == 0) sgx_epnp_finish(pws, us, alphas, pcs, s_nsel, s_cws, s_mtm, cam, s_R, s_R + 9);
        SGX_THREADS_END
        SGX_SYNC();
        SGX_THREADS_BEGIN(tid)
        for (int i = tid; i < N; i += 256) {
            const bool in = sgx_pnp_inlier(s_R, s_R + 9, A.p3dw + 3 * (size_t)(o + i), A.p2d + 2 * (size_t)(o + i), cam, A.sigma2[o + i] * th2);
            A.inl_out[o + i] = in ? 1 : 0;
            if (in) sgx_atomic_add(&s_cnt, 1);
        }
        SGX_THREADS_END
        SGX_SYNC();
        SGX_THREADS_BEGIN(tid)
        if (tid == 0) {
            if (s_cnt > st[SGX_PNP_MININ]) {                     // mnInliersi > mRansacMinInliers (:292)
                cs[0] = A.chunk0 + s_h; cs[1] += s_h + 1; cs[3] = s_cnt;
                for (int q = 0; q < 16; q++) { const int r = q >> 2, c = q & 3; A.tcw_out[16 * b + q] = r == 3 ? (c == 3 ? 1.f : 0.f) : (float)(c < 3 ? s_R[3 * r + c] : s_R[9 + r]); }
            } else st[SGX_PNP_BEST_FAILED] = 1;
        }
        SGX_THREADS_END
        SGX_SYNC();
        if (cs[0] >= 0) break;
    }
}

// per solver, after the last chunk of the call: mnIterations, bNoMore and the best model when the call found nothing (:241-255)
SGX_KERNEL(64) k_pnp_finish(SgxPnpArgs A, int *out /* B x 4: found, no_more, n_inliers, iterations_run */)
{
    SGX_THREADS_BEGIN(tid)
    const int b = (int)blockIdx.x * 64 + tid;
    if (b < A.B) {
        int *st = A.state + SGX_PNP_ST * b, *cs = A.call + SGX_PNP_CS * b, *ob = out + 4 * b;
        const int N = st[SGX_PNP_N], o = A.offsets[b];
        ob[0] = 0; ob[1] = 0; ob[2] = 0; ob[3] = 0;
        if (N < st[SGX_PNP_MININ]) ob[1] = 1;                    // :173-177
        else {
            st[SGX_PNP_ITS] += cs[1]; ob[3] = cs[1];
            if (cs[0] >= 0) { ob[0] = 1; ob[2] = cs[3]; }
            else if (st[SGX_PNP_ITS] >= st[SGX_PNP_MAXITS]) {
                ob[1] = 1;
                if (st[SGX_PNP_BEST] >= st[SGX_PNP_MININ]) {
                    ob[0] = 1; ob[2] = st[SGX_PNP_BEST];
                    for (int q = 0; q < 16; q++) A.tcw_out[16 * b + q] = A.best_tcw[16 * b + q];
                    for (int i = 0; i < N; i++) A.inl_out[o + i] = A.best_mask[o + i];
                }
            }
        }
        if (!ob[0]) for (int i = 0; i < N; i++) A.inl_out[o + i] = 0;
    }
    SGX_THREADS_END
}
