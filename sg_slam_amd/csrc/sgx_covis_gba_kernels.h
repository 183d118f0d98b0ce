// sgx_covis_gba_kernels.h — the map update of LoopClosing::RunGlobalBundleAdjustment (src/sg-slam/src/LoopClosing.cc:676-737) over the spanning tree the covisibility
// handle keeps: the correction propagated from mvpKeyFrameOrigins down to the keyframes global BA did not optimise (:676-700), and the point loop (:705-736).
//
// The float arithmetic is cv::Mat's as tests/loop_ref.py:276-297 states it: a product entry is a float dot product summed left to right whose result goes through
// double with alpha; KeyFrame::SetPose builds Twc from Rcw.t() and Ow = -Rwc * tcw (alpha = -1); A * x + b is one gemm, the double of the dot product plus the double
// of b, rounded to float once.  The unit is built with -ffp-contract=off like every feature unit, so no multiply-add is fused.  OpenCV itself is not pinned.
//
// The BFS of the reference becomes levels: a keyframe's level is its distance to its nearest ancestor-or-self that was in the GBA, counted on the way up to the first
// origin; level 0 takes its own mTcwGBA, level L needs level L - 1 of its parent.  No result depends on which wave finishes first: every row is written by one lane.
#pragma once
#include "sgx_covis_kernels.h"

enum { GS_VALID = 0, GS_FIELDS = 8 };
enum { SGX_GBA_ORIGIN_NOT_IN_GBA = 1 };                                      // sgx.h: SGX_COVIS_GBA_ORIGIN_NOT_IN_GBA

struct SgxCovisGbaReport {                // sgx_covis_gba_report
    int status, n_visited, n_propagated, n_unreached, max_depth, pad[3];
};

struct SgxCovisGbaArgs {
    int n_origins, nk;
    const int *origins, *kf_ids;
    const unsigned char *in_gba;
    const float *Tcw, *TcwGBA;
    float *Tcw_out, *TcwBef;
    unsigned char *kf_state;
    SgxCovisGbaReport *report;
    int *row_of, *orig, *level, *prow, *gs;      // slot -> row (-1 none), slot -> is an origin, row -> level (-1 unreached), row -> row of the parent, GS_*
};

// KeyFrame::SetPose: Twc (3 x 4) of the pose T (3 x 4)
SGX_DEV void sgx_gba_inverse(const float *T, float Twc[12])
{
    for (int r = 0; r < 3; r++) {
        for (int c = 0; c < 3; c++) Twc[4 * r + c] = T[4 * c + r];
        const float d = T[4 * 0 + r] * T[3] + T[4 * 1 + r] * T[7] + T[4 * 2 + r] * T[11];
        Twc[4 * r + 3] = (float)((double)d * -1.0);
    }
}

// the 4 x 4 product A * B of two poses whose fourth rows are (0, 0, 0, 1), rows 0..2
SGX_DEV void sgx_gba_mul(const float *A, const float *B, float *C)
{
    const float b3[4] = { 0.f, 0.f, 0.f, 1.f };
    for (int r = 0; r < 3; r++)
        for (int c = 0; c < 4; c++) {
            const float d = A[4 * r] * B[c] + A[4 * r + 1] * B[4 + c] + A[4 * r + 2] * B[8 + c] + A[4 * r + 3] * b3[c];
            C[4 * r + c] = (float)((double)d * 1.0);
        }
}

// R * x + t of the pose T (gemm with the addend)
SGX_DEV void sgx_gba_map(const float *T, const float *x, float *y)
{
    for (int r = 0; r < 3; r++) {
        const float d = T[4 * r] * x[0] + T[4 * r + 1] * x[1] + T[4 * r + 2] * x[2];
        y[r] = (float)((double)d * 1.0 + (double)T[4 * r + 3] * 1.0);
    }
}

// The table checked by one workgroup: every live keyframe exactly once, every origin a live keyframe that was in the GBA (rule 14).  Leaves slot -> row, the origin
// marks and GS_VALID; a refused call writes its report here and nothing else is written by the kernels behind it.
SGX_KERNEL(256) k_covis_gba_begin(SgxCovisArgs A, SgxCovisGbaArgs B)
{
    SGX_LDS int s_bad, s_nogba;
    SGX_THREADS_BEGIN(tid)
    for (int t = tid; t < A.nslots; t += 256) { B.row_of[t] = -1; B.orig[t] = 0; }
    if (tid == 0) { s_bad = B.nk != A.nlive; s_nogba = 0; }
    SGX_THREADS_END
    SGX_SYNC();
    SGX_THREADS_BEGIN(tid)
    int bad = 0;
    for (int r = tid; r < B.nk; r += 256) { const int s = sgx_covis_lookup(A, B.kf_ids[r]); if (s < 0) bad = 1; else B.row_of[s] = r; }
    if (bad) sgx_atomic_or(&s_bad, 1);
    SGX_THREADS_END
    SGX_SYNC();
    SGX_THREADS_BEGIN(tid)
    int bad = 0, nogba = 0;
    for (int j = tid; j < A.nlive; j += 256) bad |= B.row_of[A.sorted_slot[j]] < 0;          // nk == nlive: an id twice leaves another one out
    for (int o = tid; o < B.n_origins; o += 256) {
        const int s = sgx_covis_lookup(A, B.origins[o]);
        if (s < 0) { bad = 1; continue; }
        B.orig[s] = 1;
        const int r = B.row_of[s];
        if (r >= 0 && !B.in_gba[r]) nogba = 1;
    }
    if (bad) sgx_atomic_or(&s_bad, 1);
    if (nogba) sgx_atomic_or(&s_nogba, 1);
    SGX_THREADS_END
    SGX_SYNC();
    SGX_THREADS_BEGIN(tid)
    if (tid == 0) {
        B.gs[GS_VALID] = !s_bad && !s_nogba;
        if (s_bad || s_nogba) { SgxCovisGbaReport R = {}; R.status = s_bad ? -1 : SGX_GBA_ORIGIN_NOT_IN_GBA; *B.report = R; }
    }
    SGX_THREADS_END
}

// One lane per row: the walk up the tree to the first origin, at most nslots steps, noting the distance to the first keyframe that was in the GBA.
SGX_KERNEL(256) k_covis_gba_depth(SgxCovisArgs A, SgxCovisGbaArgs B)
{
    if (!B.gs[GS_VALID]) return;
    SGX_THREADS_BEGIN(tid)
    const int r = (int)blockIdx.x * 256 + tid;
    if (r < B.nk) {
        int cur = sgx_covis_lookup(A, B.kf_ids[r]), dist = -1, reached = 0;
        const int p0 = A.kf[cur * CV_FIELDS + CV_PARENT];
        for (int d = 0; d < A.nslots; d++) {
            if (dist < 0 && B.in_gba[B.row_of[cur]]) dist = d;
            if (B.orig[cur]) { reached = 1; break; }
            const int p = A.kf[cur * CV_FIELDS + CV_PARENT];
            if (p < 0 || p >= A.nslots || A.kf[p * CV_FIELDS + CV_STATE] != SGX_COVIS_LIVE || B.row_of[p] < 0) break;
            cur = p;
        }
        B.level[r] = reached ? dist : -1;
        B.prow[r] = reached && dist > 0 ? B.row_of[p0] : -1;
    }
    SGX_THREADS_END
}

// One workgroup advances the levels: level 0 and the unreached rows first, then level L from level L - 1 of the parent, a barrier between levels.  Both factors of
// Tchildc = Tcw_child * Twc_parent are the OLD poses (:683 and :689 read before :698 writes).  Bounded by rows x levels / 256 passes over the level array.
SGX_KERNEL(256) k_covis_gba_levels(SgxCovisArgs A, SgxCovisGbaArgs B)
{
    SGX_LDS int s_max, s_vis, s_prop, s_un;
    if (!B.gs[GS_VALID]) return;
    SGX_THREADS_BEGIN(tid)
    if (tid == 0) { s_max = 0; s_vis = 0; s_prop = 0; s_un = 0; }
    SGX_THREADS_END
    SGX_SYNC();
    SGX_THREADS_BEGIN(tid)
    int mx = 0, vis = 0, prop = 0, un = 0;
    for (int r = tid; r < B.nk; r += 256) {
        const int L = B.level[r];
        if (L > mx) mx = L;
        if (L < 0) {                                                         // rule 15: not visited, the pose copied through, the mark kept
            for (int e = 0; e < 12; e++) B.Tcw_out[12 * (size_t)r + e] = B.Tcw[12 * (size_t)r + e];
            B.kf_state[r] = B.in_gba[r] ? 2 : 0; un++;
        } else {
            vis++; prop += L > 0;
            if (L == 0) for (int e = 0; e < 12; e++) { B.TcwBef[12 * (size_t)r + e] = B.Tcw[12 * (size_t)r + e]; B.Tcw_out[12 * (size_t)r + e] = B.TcwGBA[12 * (size_t)r + e]; }
            B.kf_state[r] = 3;
        }
    }
    sgx_atomic_max(&s_max, mx); sgx_atomic_add(&s_vis, vis); sgx_atomic_add(&s_prop, prop); sgx_atomic_add(&s_un, un);
    SGX_THREADS_END
    SGX_SYNC();
    const int maxL = s_max;
    for (int L = 1; L <= maxL; L++) {
        SGX_THREADS_BEGIN(tid)
        for (int r = tid; r < B.nk; r += 256) {
            if (B.level[r] != L) continue;
            const int p = B.prow[r];
            float Twc[12], Tcc[12], out[12];
            sgx_gba_inverse(B.Tcw + 12 * (size_t)p, Twc);
            sgx_gba_mul(B.Tcw + 12 * (size_t)r, Twc, Tcc);
            sgx_gba_mul(Tcc, B.Tcw_out + 12 * (size_t)p, out);
            for (int e = 0; e < 12; e++) { B.TcwBef[12 * (size_t)r + e] = B.Tcw[12 * (size_t)r + e]; B.Tcw_out[12 * (size_t)r + e] = out[e]; }
        }
        SGX_THREADS_END
        SGX_SYNC();
    }
    SGX_THREADS_BEGIN(tid)
    if (tid == 0) { SgxCovisGbaReport R = {}; R.n_visited = s_vis; R.n_propagated = s_prop; R.n_unreached = s_un; R.max_depth = maxL; *B.report = R; }
    SGX_THREADS_END
}

// :705-736, one lane per point: memory-bound (a point, its flags, two poses of its reference keyframe), not tuned.
SGX_KERNEL(256) k_gba_correct_points(int n, const float *xw, const unsigned char *in_gba, const float *xw_gba, const int *ref, const unsigned char *kf_state,
                                     const float *TcwBef, const float *Tcw_out, float *xw_out)
{
    SGX_THREADS_BEGIN(tid)
    const int i = (int)blockIdx.x * 256 + tid;
    if (i < n) {
        float y[3] = { xw[3 * (size_t)i], xw[3 * (size_t)i + 1], xw[3 * (size_t)i + 2] };
        if (in_gba[i]) { y[0] = xw_gba[3 * (size_t)i]; y[1] = xw_gba[3 * (size_t)i + 1]; y[2] = xw_gba[3 * (size_t)i + 2]; }
        else {
            const int r = ref[i];
            if (r >= 0 && kf_state[r] == 3) {                                // mnBAGlobalForKF == nLoopKF, and visited (rule 15: mTcwBefGBA is stale otherwise)
                float xc[3], Twc[12];
                sgx_gba_map(TcwBef + 12 * (size_t)r, y, xc);
                sgx_gba_inverse(Tcw_out + 12 * (size_t)r, Twc);
                sgx_gba_map(Twc, xc, y);
            }
        }
        xw_out[3 * (size_t)i] = y[0]; xw_out[3 * (size_t)i + 1] = y[1]; xw_out[3 * (size_t)i + 2] = y[2];
    }
    SGX_THREADS_END
}
