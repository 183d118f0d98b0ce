// sgx_loop_sim3_kernels.h — the Sim3 arithmetic of loop closing between the index rows of the covisibility handle and the essential-graph optimiser.  Its translation
// unit (sgx_loop_sim3.cpp) is built like the feature kernels, -ffp-contract=off: every expression is evaluated as written, so the device, the emulator and the scalar
// restatement of tests/loop_ref.py agree in every bit.  (sgx_ba.cpp, where the optimiser's kernels live, lets multiply-adds fuse; these kernels must not be compiled there.)
#pragma once
#include "sgx_sim3.h"

#define SGX_EG_THREADS 256
SGX_DEV void sgx_eg_load(const double *p, SgxSim3 &s) { s.q[0] = p[0]; s.q[1] = p[1]; s.q[2] = p[2]; s.q[3] = p[3]; s.t[0] = p[4]; s.t[1] = p[5]; s.t[2] = p[6]; s.s = p[7]; }
// ------------------------------------------------------------------------------------------------------------------------------------------ the Sim3 glue of loop closing
// Between the index rows of sgx_covis_loop_begin / sgx_covis_essential_graph and the optimiser: LoopClosing::CorrectLoop :440-469, :503-512, the estimates and
// measurements of Optimizer::OptimizeEssentialGraph (Optimizer.cc:818-832, :857-867, :889-972) and its pose recovery (:991-1010).  Double except where the reference is
// float: the cv::Mat products of KeyFrame::SetPose and of Tic = Tiw * Twc are cv::gemm's small-matrix path, a float dot product left to right whose result goes through
// double with alpha.  A pose is 12 floats, the rows of [R | t].
SGX_DEV void sgx_eg_store(double *p, const SgxSim3 &s) { p[0] = s.q[0]; p[1] = s.q[1]; p[2] = s.q[2]; p[3] = s.q[3]; p[4] = s.t[0]; p[5] = s.t[1]; p[6] = s.t[2]; p[7] = s.s; }
SGX_DEV void sgx_eg_sim3_of_pose(const float *T, SgxSim3 &o)              // g2o::Sim3(Converter::toMatrix3d(R), Converter::toVector3d(t), 1.0)
{
    double R[3][3];
    for (int r = 0; r < 3; r++) { for (int c = 0; c < 3; c++) R[r][c] = (double)T[4 * r + c]; o.t[r] = (double)T[4 * r + 3]; }
    sgx_quat_from_R(R, o.q); o.s = 1.0;
}
SGX_DEV void sgx_eg_pose_of_sim3(const SgxSim3 &S, float *T)              // Converter::toCvSE3(rotation().toRotationMatrix(), translation() * (1. / scale()))
{
    double R[3][3]; sgx_quat_to_R(S.q, R);
    const double is = 1. / S.s;
    for (int r = 0; r < 3; r++) { for (int c = 0; c < 3; c++) T[4 * r + c] = (float)R[r][c]; T[4 * r + 3] = (float)(S.t[r] * is); }
}

// one lane per group member (cur is the last): NonCorrectedSim3, CorrectedSim3 = Sim3(Ric, tic, 1) * Scw with Tic = Tiw * Twc (Scw itself for cur), and the corrected pose
SGX_KERNEL(SGX_EG_THREADS) k_loop_propagate(int ng, const float *Tcw, const double *Scw, double *noncorrected, double *corrected, float *corrected_Tiw)
{
    SGX_THREADS_BEGIN(tid)
    const int g = (int)blockIdx.x * SGX_EG_THREADS + tid;
    if (g < ng) {
        const float *Ti = Tcw + 12 * (size_t)g, *Tc = Tcw + 12 * (size_t)(ng - 1);
        SgxSim3 non, cor, scw; sgx_eg_load(Scw, scw);
        sgx_eg_sim3_of_pose(Ti, non);
        if (g != ng - 1) {
            float Twc[4][4], Tic[12];                                     // KeyFrame::SetPose: Rwc = Rcw.t(), Ow = -Rwc * tcw
            for (int r = 0; r < 3; r++) {
                for (int c = 0; c < 3; c++) Twc[r][c] = Tc[4 * c + r];
                const float d = Tc[4 * 0 + r] * Tc[3] + Tc[4 * 1 + r] * Tc[7] + Tc[4 * 2 + r] * Tc[11];
                Twc[r][3] = (float)((double)d * -1.0);
            }
            Twc[3][0] = 0.f; Twc[3][1] = 0.f; Twc[3][2] = 0.f; Twc[3][3] = 1.f;
            for (int r = 0; r < 3; r++)
                for (int c = 0; c < 4; c++) {                             // the fourth row of Tiw is (0, 0, 0, 1) and is not needed
                    const float d = Ti[4 * r] * Twc[0][c] + Ti[4 * r + 1] * Twc[1][c] + Ti[4 * r + 2] * Twc[2][c] + Ti[4 * r + 3] * Twc[3][c];
                    Tic[4 * r + c] = (float)((double)d * 1.0);
                }
            SgxSim3 sic; sgx_eg_sim3_of_pose(Tic, sic);
            sgx_sim3_mul(sic, scw, cor);
        } else cor = scw;
        sgx_eg_store(noncorrected + 8 * (size_t)g, non); sgx_eg_store(corrected + 8 * (size_t)g, cor);
        sgx_eg_pose_of_sim3(cor, corrected_Tiw + 12 * (size_t)g);
    }
    SGX_THREADS_END
}

// vScw: CorrectedSim3 for a vertex of the group, Sim3(Rcw, tcw, 1) otherwise
SGX_KERNEL(SGX_EG_THREADS) k_loop_flatten_vertices(int nv, const int *vertex_group, const float *Tcw, const double *corrected, double *S_in)
{
    SGX_THREADS_BEGIN(tid)
    const int v = (int)blockIdx.x * SGX_EG_THREADS + tid;
    if (v < nv) {
        SgxSim3 s;
        if (vertex_group[v] >= 0) sgx_eg_load(corrected + 8 * (size_t)vertex_group[v], s); else sgx_eg_sim3_of_pose(Tcw + 12 * (size_t)v, s);
        sgx_eg_store(S_in + 8 * (size_t)v, s);
    }
    SGX_THREADS_END
}

// Sji = Sjw * Swi: both operands from vScw for a loop-connection edge (kind 0), NonCorrectedSim3 for a group vertex of the other kinds
SGX_KERNEL(SGX_EG_THREADS) k_loop_flatten_edges(int ne, const int *e_i, const int *e_j, const unsigned char *e_kind, const int *vertex_group, const double *S_in,
                                              const double *noncorrected, double *e_meas)
{
    SGX_THREADS_BEGIN(tid)
    const int k = (int)blockIdx.x * SGX_EG_THREADS + tid;
    if (k < ne) {
        const int i = e_i[k], j = e_j[k], gi = e_kind[k] ? vertex_group[i] : -1, gj = e_kind[k] ? vertex_group[j] : -1;
        SgxSim3 siw, sjw, swi, sji;
        sgx_eg_load(gi >= 0 ? noncorrected + 8 * (size_t)gi : S_in + 8 * (size_t)i, siw);
        sgx_eg_load(gj >= 0 ? noncorrected + 8 * (size_t)gj : S_in + 8 * (size_t)j, sjw);
        sgx_sim3_inverse(siw, swi); sgx_sim3_mul(sjw, swi, sji);
        sgx_eg_store(e_meas + 8 * (size_t)k, sji);
    }
    SGX_THREADS_END
}

// the pose recovery: Sim3 [sR t; 0 1] -> SE3 [R t/s; 0 1], and vCorrectedSwc
SGX_KERNEL(SGX_EG_THREADS) k_loop_recover(int nv, const double *S_out, float *Tcw, double *corrected_Swc)
{
    SGX_THREADS_BEGIN(tid)
    const int v = (int)blockIdx.x * SGX_EG_THREADS + tid;
    if (v < nv) {
        SgxSim3 s, inv; sgx_eg_load(S_out + 8 * (size_t)v, s);
        sgx_sim3_inverse(s, inv); sgx_eg_store(corrected_Swc + 8 * (size_t)v, inv);
        sgx_eg_pose_of_sim3(s, Tcw + 12 * (size_t)v);
    }
    SGX_THREADS_END
}

// P' = correctedSwr.map(Srw.map(P)), r = the point's reference (LoopClosing.cc:491-497, Optimizer.cc:1032-1040): k_eg_correct_points evaluated as written
SGX_KERNEL(SGX_EG_THREADS) k_loop_correct_points(int n, const float *xw, const int *ref, const double *Srw, const double *cSwr, float *out)
{
    SGX_THREADS_BEGIN(tid)
    const int i = (int)blockIdx.x * SGX_EG_THREADS + tid;
    if (i < n) {
        SgxSim3 a, c; sgx_eg_load(Srw + 8 * (size_t)ref[i], a); sgx_eg_load(cSwr + 8 * (size_t)ref[i], c);
        const double p[3] = { (double)xw[3 * (size_t)i], (double)xw[3 * (size_t)i + 1], (double)xw[3 * (size_t)i + 2] };
        double m[3], o[3]; sgx_sim3_map(a, p, m); sgx_sim3_map(c, m, o);
        out[3 * (size_t)i] = (float)o[0]; out[3 * (size_t)i + 1] = (float)o[1]; out[3 * (size_t)i + 2] = (float)o[2];
    }
    SGX_THREADS_END
}
