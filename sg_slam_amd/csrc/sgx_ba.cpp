// sgx_ba.cpp — host side of the LocalBundleAdjustment / BundleAdjustment / OptimizeEssentialGraph C-ABI: the device arena, the Schur job list, the solver launches and
// the drivers.  The planning that needs no device (index structures, solver plan, switches) is in sgx_ba_plan.h, the Levenberg-Marquardt control loop in sgx_lm.h.
// Reference: src/sg-slam/src/Optimizer.cc:453-778.
// fp64 solver arithmetic: multiply-adds may fuse here.  The reference does NOT fuse them — g2o and sg-slam are built plain -O3 (Thirdparty/g2o/CMakeLists.txt:57,
// src/sg-slam/CMakeLists.txt:11-12; only DBoW2 has -march=native), so on x86-64 every product is rounded before it is added — which makes this a deliberate
// divergence inside the stated tolerance: the parity bar for poses / landmarks is 1e-5 relative, not bit equality, and the fused form saves a quarter of the fp64
// instructions.  Building with -DSGX_FP_CONTRACT_OFF keeps the reference's rounding (tests/test_poseopt_gpu.py runs one parity case on that build
// when it is present).  The bit-exact integer / fp32 feature kernels keep -ffp-contract=off.
#ifndef SGX_FP_CONTRACT_OFF
#pragma clang fp contract(fast)
#endif
#include "sgx_ba_kernels.h"
#include "sgx_eg_kernels.h"
#include "sgx_prof.h"
#include "../../include/sgx.h"
#ifdef SGX_DEBUG_TAPS
#include "../../include/sgx_debug.h"      // test / tuning taps: compiled into tests/taps/libsgx_taps.so and the emulator only
#endif
#include <math.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <algorithm>
#include <chrono>
#include <mutex>
#include <thread>
#include <type_traits>
#include <utility>
#include <vector>
#include "sgx_ba_plan.h"
#include "sgx_lm.h"

namespace {
// One grow-only device arena per process (LocalBundleAdjustment runs on the single LocalMapping thread, LocalMapping.cc:81): avoids ~30 hipMalloc/hipFree pairs per
// call.  With it a grow-only pinned staging buffer of the packed host->device inputs: no 17 MB zero-fill + pageable copy per call at 2 000 keyframes.
// layout(f) runs the list of arrays f twice: the first pass sizes (no pointers handed out), the second assigns and packs the inputs, which then go up with one copy.
struct Arena {
    char *base = nullptr, *stage = nullptr; size_t cap = 0, stage_cap = 0, off = 0, in_bytes = 0; int device = -1; bool sizing = false, taking_input = false;      // taking_input: take() on behalf of input()
    int reserve(size_t bytes) {
#ifndef SGX_EMU
        int cur = 0;
        if (hipGetDevice(&cur) != hipSuccess) return SGX_ERR_DEVICE;
        if (base && cur != device) {                      // the arena lives on the device that was current when it was allocated: a caller on another device gets a fresh one
            const int keep = cur; (void)hipSetDevice(device); (void)hipFree(base); (void)hipSetDevice(keep);
            base = nullptr; cap = 0;
        }
        device = cur;
#endif
        if (bytes <= cap) return SGX_OK;
        if (base) (void)hipFree(base);
        base = nullptr; cap = 0;
        const size_t want = bytes + bytes / 4;
        if (hipMalloc((void **)&base, want) != hipSuccess) return SGX_ERR_NOMEM;
        cap = want; return SGX_OK;
    }
    int stage_reserve(size_t bytes) {
        if (bytes <= stage_cap) return SGX_OK;
        const size_t want = bytes + bytes / 4;
#ifndef SGX_EMU
        if (stage) (void)hipHostFree(stage);
        stage = nullptr; stage_cap = 0;
        if (hipHostMalloc((void **)&stage, want, hipHostMallocPortable) != hipSuccess) { stage = nullptr; return SGX_ERR_NOMEM; }
#else
        free(stage); stage = (char *)malloc(want); if (!stage) { stage_cap = 0; return SGX_ERR_NOMEM; }
#endif
        stage_cap = want; return SGX_OK;
    }
    template <class T> void take(T **p, size_t n)
    {
        off = (off + 255) & ~(size_t)255; if (!sizing) *p = (T *)(base + off);
#ifdef SGX_DEBUG_TAPS
        if (!sizing && !taking_input && std::is_floating_point<T>::value) scratch_fp.push_back({ off, (n ? n : 1) * sizeof(T) });
#endif
        off += (n ? n : 1) * sizeof(T);
    }
    // one allocation handed out as adjacent parts: *p0 is the whole, *p1 starts n0 elements in, *p2 n1 further
    template <class T> void take_parts(T **p0, size_t n0, T **p1, size_t n1, T **p2 = nullptr, size_t n2 = 0) { take(p0, n0 + n1 + n2); if (!sizing) { *p1 = *p0 + n0; if (p2) *p2 = *p1 + n1; } }
    // a host->device input (they come first): taken like any array and packed into the staging buffer from src (nullptr: zeros); the alignment gaps between them are never read
    template <class T> void input(T **p, const T *src, size_t n) {
        taking_input = true; take(p, n); taking_input = false; in_bytes = off;
        if (!sizing && n) { char *dst = stage + ((const char *)*p - base); if (src) memcpy(dst, src, n * sizeof(T)); else memset(dst, 0, n * sizeof(T)); }
    }
    template <class F> int layout(F &&arrays) {
        sizing = true; off = in_bytes = 0; arrays(*this);
        int rc = reserve(off); if (rc != SGX_OK) return rc;
        if ((rc = stage_reserve(in_bytes)) != SGX_OK) return rc;
        sizing = false; off = in_bytes = 0;
#ifdef SGX_DEBUG_TAPS
        scratch_fp.clear();
#endif
        arrays(*this);
        SGX_CHECK_HIP(hipMemcpy(base, stage, in_bytes, hipMemcpyHostToDevice));
        return SGX_OK;
    }
#ifdef SGX_DEBUG_TAPS
    // (test tap, sgx_ba_debug_set_init(3)) the double / float arrays of the last layout that are no inputs, as (offset, bytes), and their fill with 0xFF bytes: every value
    // a NaN, where the product build has whatever the previous call left.  The integer arrays keep their content: a stale index must not become an address.
    std::vector<std::pair<size_t, size_t>> scratch_fp;
    int poison_scratch() { for (const auto &r : scratch_fp) SGX_CHECK_HIP(hipMemsetAsync(base + r.first, 0xFF, r.second, 0)); return SGX_OK; }
#endif
};
static Arena g_arena;
static std::mutex g_arena_mutex;      // one arena per process: calls from several threads (the reference has one LocalMapping thread, plus GlobalBundleAdjustment from LoopClosing) take turns

// test / tuning taps (include/sgx_debug.h): values for the following calls of this thread, read by ba_switches() only
static thread_local int g_ba_init_mode = 0, g_ba_jobs_host = 0, g_ba_solver = -1, g_ba_last_plan[4] = { 0, 0, 0, 0 };

static BaSwitches ba_switches()
{
    auto env = [](const char *name, int &v) { if (const char *e = sgx_getenv(name)) v = atoi(e); };
    BaSwitches s;
    s.init_mode = g_ba_init_mode; s.jobs_host = g_ba_jobs_host;
#ifdef SGX_EMU
    s.jobs_host = 1;                                       // the device builder's kernels are wave-level code: not in the emulator
#endif
    if (const char *e = sgx_getenv("SGX_BA_SOLVER")) s.solver = strcmp(e, "dense") == 0 ? 1 : (strcmp(e, "env") == 0 ? 2 : 0);
    if (g_ba_solver >= 0) s.solver = g_ba_solver;
    env("SGX_BA_TWIST", s.twist); env("SGX_ENV_DBG", s.env_dbg); env("SGX_TUNE_CHOL_WIDE_MIN", s.wide_min); s.timing = sgx_getenv("SGX_BA_TIMING") != nullptr;
    return s;
}

// wall-clock of the host phases on stderr (BaSwitches::timing)
struct PhaseClock {
    bool on; double mark = now();
    static double now() { return std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now().time_since_epoch()).count(); }
    void lap(const char *what) { if (on) { (void)hipDeviceSynchronize(); const double t = now(); fprintf(stderr, "[sgx_ba] %-22s %8.3f ms\n", what, t - mark); mark = t; } }
};

static double sum_of(const double *v, int n) { double s = 0; for (int i = 0; i < n; i++) s += v[i]; return s; }
// n partial results of a kernel, and their sum in the order of the blocks
static int read_back(std::vector<double> &host, const double *dev, size_t n, double *sum = nullptr)
{
    host.resize(n); SGX_CHECK_HIP(hipMemcpy(host.data(), dev, sizeof(double) * n, hipMemcpyDeviceToHost));
    if (sum) *sum = sum_of(host.data(), (int)n);
    return SGX_OK;
}

// Dense symmetric positive definite solve  S x = bp - coef  on the device (in place: S is overwritten by its factor): a register kernel for small systems, the blocked
// right-looking Cholesky with the fp64-MFMA trailing update above SGX_CHOL_SMALL unknowns, or — with an envelope plan — the persistent-workgroup solver.  *ok (device) is
// cleared when a pivot is not positive; x then keeps its previous content.  *xout = where the solution was left (xp or xsol).  Shared by the bundle adjustments
// (reduced camera system) and the essential-graph optimisation.
struct Chol {
    int NP = 0; double *S = nullptr, *Linv = nullptr, *bp = nullptr, *coef = nullptr, *xp = nullptr, *xsol = nullptr; int *ok = nullptr;
    int *env_rstart = nullptr, *env_rows = nullptr; int env_nA = 0, env_nB = 0;      // EnvPlan on the device (NULL = dense)
    double *env_S2 = nullptr, *env_x2 = nullptr;         // the second branch's contributions to the separator (nsep x nsep, then nsep): ONE allocation, cleared with one memset
};
static int chol_factor_solve(const Chol &C, const BaSwitches &sw, const double **xout)
{
    *xout = C.xp;
    if (C.NP <= 0) return SGX_OK;
    const int nt = (C.NP + SGX_NB - 1) / SGX_NB;
    if (C.env_rstart) {                                  // sparse covisibility: the whole factorisation + forward substitution as one persistent workgroup, then the backward pass
        const int nA = C.env_nB > 0 ? C.env_nA : nt, nB = C.env_nB > 0 ? C.env_nB : 0;
        if (nB > 0) {                                    // the second branch's separator contributions start from zero
            const size_t ns = (size_t)(C.NP - (nA + nB) * SGX_NB);
            SGX_CHECK_HIP(hipMemsetAsync(C.env_S2, 0, sizeof(double) * (ns * ns + ns), 0));
        }
        SGX_LAUNCH(k_chol_env_factor, dim3(nB > 0 ? 2 : 1), dim3(SGX_ENV_THREADS), (sgx_stream_t)0, C.NP, nt, C.env_rstart, C.env_rows, C.S, C.Linv, C.ok, C.bp, C.coef, C.xp, sw.env_dbg, 0, nA, nB, C.env_S2, C.env_x2);
        if (nA + nB < nt) {
            SGX_LAUNCH(k_chol_env_factor, dim3(1), dim3(SGX_ENV_THREADS), (sgx_stream_t)0, C.NP, nt, C.env_rstart, C.env_rows, C.S, C.Linv, C.ok, C.bp, C.coef, C.xp, sw.env_dbg, 1, nA, nB, C.env_S2, C.env_x2);
            SGX_LAUNCH(k_chol_env_back, dim3(1), dim3(1024), (sgx_stream_t)0, C.NP, nt, C.env_rstart, C.env_rows, C.S, C.Linv, C.xp, C.xsol, C.ok, 0, nA, nB);
        }
        SGX_LAUNCH(k_chol_env_back, dim3(nB > 0 ? 2 : 1), dim3(1024), (sgx_stream_t)0, C.NP, nt, C.env_rstart, C.env_rows, C.S, C.Linv, C.xp, C.xsol, C.ok, 1, nA, nB);
        *xout = C.xsol;
        return SGX_OK;
    }
    if (C.NP <= SGX_CHOL_SMALL) {
        SGX_LAUNCH(k_chol_small_reg, dim3(1), dim3(256), (sgx_stream_t)0, C.NP, C.S, C.bp, C.coef, C.xp, C.ok);
        return SGX_OK;
    }
    // blocked Cholesky.  Tiles per outer panel; small systems keep one level (a rank-256 launch on the critical path costs them more than its eight rank-32 shares)
    const int OT = C.NP > sw.wide_min ? SGX_OB / SGX_NB : (1 << 24);
    for (int kb = 0; kb < nt; kb++) {
        const int k0 = kb * SGX_NB, rem = nt - kb - 1;
        const int in_panel = OT - 1 - kb % OT;           // column tiles right of this one that still belong to the outer panel
#ifndef SGX_EMU
        SGX_LAUNCH(k_chol_diag_wave, dim3(1), dim3(64), (sgx_stream_t)0, C.NP, k0, C.S, C.Linv, C.ok, C.bp, C.coef, C.xp);
#else
        SGX_LAUNCH(k_chol_diag, dim3(1), dim3(256), (sgx_stream_t)0, C.NP, k0, C.S, C.Linv, C.ok, C.bp, C.coef, C.xp);      // the workgroup / LDS version: the emulator's diagonal-tile kernel
#endif
        if (rem > 0) {
            SGX_LAUNCH(k_chol_panel, dim3(rem), dim3(256), (sgx_stream_t)0, C.NP, k0, C.S, C.Linv, C.ok, C.xp);
            const int pc = in_panel < rem ? in_panel : rem;
            if (pc > 0) SGX_LAUNCH(k_chol_update, dim3(rem, pc), dim3(256), (sgx_stream_t)0, C.NP, k0, C.S, C.ok);
            if (in_panel == 0) {                         // panel finished: one rank-256 update of the rest on the matrix cores
                const int p0 = (kb / OT) * SGX_OB, q0 = p0 + SGX_OB;
                const int wt = (C.NP - q0 + SGX_WT - 1) / SGX_WT;
                if (wt > 0) SGX_LAUNCH(k_chol_update_wide, dim3(wt, wt), dim3(256), (sgx_stream_t)0, C.NP, p0, SGX_OB, C.S, C.ok);
            }
        }
    }
    // backward pass: one launch per diagonal block, all CUs on the row panel (measured against one workgroup for the whole pass: the per-block launches win at every
    // blocked size — 360 unknowns: 9.9 -> 9.5 ms per LocalBA, 12 000: 2.5 -> 1.1 s)
    for (int kb = nt - 1; kb >= 0; kb--) {
        const int k0 = kb * SGX_NB;
        SGX_LAUNCH(k_chol_back_step, dim3(k0 > 0 ? (k0 + 255) / 256 : 1), dim3(256), (sgx_stream_t)0, C.NP, k0, C.S, C.Linv, C.xp, C.xsol, C.ok);
    }
    *xout = C.xsol;
    return SGX_OK;
}

// One bundle adjustment on the device; value-initialise it (BA B{}).  It is the problem object of sgx_lm_solve: the hooks below are one LM step's device work.
struct BA {
    int np, nl, ne, nf;
    SgxCam cam; double dMono, dStereo;
    const volatile int32_t *stop;
    BaSwitches sw;
    Chol C;                                  // the reduced camera system (6 nf unknowns) and its solver plan
    int env_nrows;                           // entries of C.env_rows
    // device
    SgxBaEdge *E; SgxSE3 *T, *Tb; double *X, *Xb, *err, *Hll, *bl, *Hpl, *W, *Hpp, *xl, *Dinv, *dwork, *partial;
    int *pt_start, *pt_edges, *pose_start, *pose_edges, *hidx, *free_pose; uint8_t *pt_active;
    SgxBaJob *jobs; int *blk_start; long long njobs, nblk; size_t jobs_cap;
    int *pose_edges_l, *row_jobs, *row_blks, *job_off, *blk_off, *jtot;      // device-side job list build (k_ba_jobs_*): a pose's edges in ascending landmark order; per-row counts and their exclusive sums; { jobs, blocks }
    double *trial_out, *part_scale, *part_chi;      // what a trial reports, ONE allocation read back with one copy: [ok (C.ok, in the first slot) | part_scale[nblk_v] | part_chi[nblk_e]]
    int nblk_e, nblk_v;
    float *Tcw; uint8_t *fixed, *erase;      // the caller's poses (in and out) and fixed flags; the erase flags of the classification passes
    std::vector<double> hpart;
    // host copy of the sorted Schur job list of THIS problem (build_jobs_host): the classification pass filters it in place instead of rebuilding it.  Owned by the problem, so the
    // cache can neither be applied to another problem that happens to have the same job count nor outlive the call (it used to be thread_local and never released)
    std::vector<SgxBaJob> h_jobs; std::vector<int> h_blk_start;

    bool stopped() const { return stop && *stop; }
    int chi2(double *chi)
    {
        SGX_LAUNCH(k_ba_errors, dim3(nblk_e), dim3(SGX_BA_THREADS), (sgx_stream_t)0, ne, E, T, X, cam, dMono, dStereo, err, part_chi);
        return read_back(hpart, part_chi, nblk_e, chi);
    }
    int linearize()      // buildSystem: J^T J / J^T r block accumulation
    {
        sgx_prof_begin(SGX_K_BA_LINEARIZE, (sgx_stream_t)0);
        SGX_LAUNCH(k_ba_linearize_points, dim3((nl + SGX_BA_THREADS - 1) / SGX_BA_THREADS), dim3(SGX_BA_THREADS), (sgx_stream_t)0, nl, pt_start, pt_edges,
                   E, T, X, hidx, err, cam, dMono, dStereo, Hll, bl, Hpl, pt_active);
        if (nf > 0)
            SGX_LAUNCH(k_ba_linearize_poses, dim3(nf), dim3(SGX_BA_THREADS), (sgx_stream_t)0, np, free_pose, pose_start, pose_edges, E, T, X, err,
                       cam, dMono, dStereo, Hpp, C.bp);
        sgx_prof_end(SGX_K_BA_LINEARIZE, (sgx_stream_t)0);
        return SGX_OK;
    }
    int initial_lambda(double *lambda)      // computeLambdaInit: 1e-5 * the largest diagonal entry
    {
        SGX_LAUNCH(k_ba_maxdiag, dim3(nblk_v), dim3(SGX_BA_THREADS), (sgx_stream_t)0, nf, nl, Hpp, Hll, pt_active, partial);
        const int rc = read_back(hpart, partial, nblk_v);
        double maxd = 0; for (int i = 0; i < nblk_v; i++) maxd = fmax(maxd, hpart[i]);
        *lambda = 1e-5 * maxd;
        return rc;
    }
    int trial(double lambda, LmTrial *t)
    {
        const int NP = C.NP; int rc;
        const double *xsol = C.xp;                               // where the solver leaves the pose increments
        { const int one = 1; SGX_CHECK_HIP(hipMemcpyAsync(C.ok, &one, 4, hipMemcpyHostToDevice, 0)); }
        sgx_prof_begin(SGX_K_BA_SCHUR, (sgx_stream_t)0);
        if (NP > 0) {
            const int g = (int)(((size_t)NP * NP + SGX_BA_THREADS - 1) / SGX_BA_THREADS);
            if (C.env_rstart && sw.init_mode != 1) {             // envelope solver: only the tiles it reads
                if (sw.init_mode >= 2) SGX_CHECK_HIP(hipMemsetAsync(C.S, 0xFF, sizeof(double) * (size_t)NP * NP, 0));      // (test tap) all ones = NaN everywhere first
                const int nt = (NP + SGX_NB - 1) / SGX_NB;
                SGX_LAUNCH(k_ba_schur_init_env, dim3((unsigned)(nt + env_nrows)), dim3(SGX_BA_THREADS), (sgx_stream_t)0, nf, Hpp, lambda, C.S, C.coef, nt, C.env_rstart, C.env_rows);
            } else
            SGX_LAUNCH(k_ba_schur_init, dim3(g > 4096 ? 4096 : g), dim3(SGX_BA_THREADS), (sgx_stream_t)0, nf, Hpp, lambda, C.S, C.coef);
        }
        SGX_LAUNCH(k_ba_dinv, dim3((nl + SGX_BA_THREADS - 1) / SGX_BA_THREADS), dim3(SGX_BA_THREADS), (sgx_stream_t)0, nl, pt_active, Hll, lambda, Dinv);
        if (njobs > 0) {
            const long long n36 = nblk * 36, n6 = (long long)ne * 6;
            SGX_LAUNCH(k_ba_hpl_dinv, dim3((unsigned)((n6 + SGX_BA_THREADS - 1) / SGX_BA_THREADS)), dim3(SGX_BA_THREADS), (sgx_stream_t)0, n6, E, hidx, Hpl, Dinv, W);
            SGX_LAUNCH(k_ba_schur_pairs, dim3((unsigned)((n36 + SGX_BA_THREADS - 1) / SGX_BA_THREADS)), dim3(SGX_BA_THREADS), (sgx_stream_t)0, n36, nf, blk_start, jobs, E,
                       hidx, bl, Hpl, W, C.S, C.coef);
        }
        sgx_prof_end(SGX_K_BA_SCHUR, (sgx_stream_t)0);
        sgx_prof_begin(SGX_K_BA_SOLVE, (sgx_stream_t)0);
        if ((rc = chol_factor_solve(C, sw, &xsol)) != SGX_OK) return rc;
        sgx_prof_end(SGX_K_BA_SOLVE, (sgx_stream_t)0);
        sgx_prof_begin(SGX_K_BA_UPDATE, (sgx_stream_t)0);
        // when the factorisation failed, xp/xl keep the previous solution (as g2o's _x does) and the step is rejected by the driver
        SGX_LAUNCH(k_ba_backsub, dim3((nl + SGX_BA_THREADS - 1) / SGX_BA_THREADS), dim3(SGX_BA_THREADS), (sgx_stream_t)0, nl, pt_start, pt_edges, E, hidx,
                   pt_active, bl, Hpl, Dinv, xsol, xl, C.ok);
        // push + update + computeScale
        SGX_LAUNCH(k_ba_update, dim3(nblk_v), dim3(SGX_BA_THREADS), (sgx_stream_t)0, np, nl, hidx, pt_active, xsol, xl, C.bp, bl, lambda, T, X, Tb, Xb, part_scale);
        SGX_LAUNCH(k_ba_errors, dim3(nblk_e), dim3(SGX_BA_THREADS), (sgx_stream_t)0, ne, E, T, X, cam, dMono, dStereo, err, part_chi);
        sgx_prof_end(SGX_K_BA_UPDATE, (sgx_stream_t)0);
        // ok flag, computeScale partials and the new chi2 partials in one device->host copy
        rc = read_back(hpart, trial_out, 1 + (size_t)nblk_v + nblk_e);
        memcpy(&t->ok, &hpart[0], 4);
        t->scale = sum_of(&hpart[1], nblk_v); t->chi = sum_of(&hpart[1 + nblk_v], nblk_e);
        return rc;
    }
    int reject()      // pop
    { SGX_CHECK_HIP(hipMemcpy(T, Tb, sizeof(SgxSE3) * np, hipMemcpyDeviceToDevice)); SGX_CHECK_HIP(hipMemcpy(X, Xb, sizeof(double) * 3 * (size_t)nl, hipMemcpyDeviceToDevice)); return SGX_OK; }
};

// Schur job list for the current active edge set: all ordered pairs (k1, k2) of active free-pose edges of one landmark, grouped by destination block (i1, i2) of the reduced
// system; inside a block the jobs are in landmark order, the order in which the reference subtracts them (block_solver.hpp:380-433); k_ba_schur_pairs then sums every block
// sequentially, without atomics.  Built block row by block row: the jobs of row i1 come from the edges of that pose (pose_edges_l: ascending landmark) x the active edges of
// their landmarks, and are dealt to their i2 with a counting sort over the few poses the row touches — everything a row needs sits in L1 / L2 (a sort of the whole list by
// the nf^2 keys was 30 ms per call at 2 000 keyframes: a third of the bundle adjustment).
// level1 == nullptr: build from scratch (every edge of a free pose is active).  level1 != nullptr: the list of the SAME problem after the classification pass — the previous list
// with the jobs of the newly switched-off edges taken out (a stable filter of the sorted list: a few ms instead of a rebuild).
static int build_jobs_host(BA &B, const BaIndex &ix, const std::vector<uint8_t> *level1)
{
    const std::vector<int> &pt_start = ix.pt_start, &pt_edges = ix.pt_edges, &pose_start = ix.pose_start, &pose_edges_l = ix.pose_edges_l, &free_pose = ix.free_pose;
    const std::vector<SgxBaEdge> &E = ix.E;
    std::vector<SgxBaJob> &sorted = B.h_jobs;
    std::vector<int> &blk_start = B.h_blk_start;
    if (level1 && !sorted.empty() && (long long)sorted.size() == B.njobs) {
        const std::vector<uint8_t> &lv = *level1;
        size_t w = 0, nb = 0;
        const size_t nblk = blk_start.size() - 1;
        for (size_t b = 0; b < nblk; b++) {
            const size_t beg = (size_t)blk_start[b], end = (size_t)blk_start[b + 1], w0 = w;
            for (size_t i = beg; i < end; i++) { const SgxBaJob j = sorted[i]; if (!lv[(size_t)j.k1] && !lv[(size_t)j.k2]) sorted[w++] = j; }
            if (w > w0) blk_start[nb++] = (int)w0;
        }
        sorted.resize(w); blk_start.resize(nb + 1); blk_start[nb] = (int)w;
    } else {
        const int nthreads = std::max(1, std::min(8, B.nf / 64));
        std::vector<int> eh(B.ne);
        for (int k = 0; k < B.ne; k++) eh[k] = (level1 && (*level1)[k]) ? -1 : ix.row_of_edge(k);      // destination row / column of an active edge, -1 = not in the system
        // block rows dealt to the threads in contiguous ranges of about equal edge counts
        std::vector<int> cut(nthreads + 1, B.nf); cut[0] = 0;
        { long long tot = 0; for (int h = 0; h < B.nf; h++) tot += pose_start[free_pose[h] + 1] - pose_start[free_pose[h]];
          long long run = 0; int t = 1; for (int h = 0; h < B.nf && t < nthreads; h++) { run += pose_start[free_pose[h] + 1] - pose_start[free_pose[h]]; if (run * nthreads >= tot * t) cut[t++] = h + 1; } }
        std::vector<std::vector<SgxBaJob>> part((size_t)nthreads); std::vector<std::vector<int>> pblk((size_t)nthreads);
        auto work = [&](int t) {
            std::vector<SgxBaJob> &out = part[(size_t)t], grp; std::vector<int> &ob = pblk[(size_t)t], grp_h2, touched, cnt((size_t)(B.nf > 0 ? B.nf : 1), 0);
            for (int h1 = cut[t]; h1 < cut[t + 1]; h1++) {
                const int p = free_pose[h1];
                grp.clear(); grp_h2.clear(); touched.clear();
                for (int q = pose_start[p]; q < pose_start[p + 1]; q++) {
                    const int k1 = pose_edges_l[q]; if (eh[k1] < 0) continue;
                    const int l = E[k1].point;
                    for (int q2 = pt_start[l]; q2 < pt_start[l + 1]; q2++) {
                        const int k2 = pt_edges[q2], h2 = eh[k2]; if (h2 < 0) continue;
                        if (cnt[h2]++ == 0) touched.push_back(h2);
                        grp.push_back(SgxBaJob{k1, k2}); grp_h2.push_back(h2);
                    }
                }
                if (grp.empty()) continue;
                std::sort(touched.begin(), touched.end());
                const size_t base = out.size();
                { int run = 0; for (int h2 : touched) { const int c = cnt[h2]; cnt[h2] = run; ob.push_back((int)base + run); run += c; } }
                out.resize(base + grp.size());
                for (size_t i = 0; i < grp.size(); i++) out[base + (size_t)cnt[grp_h2[i]]++] = grp[i];
                for (int h2 : touched) cnt[h2] = 0;
            }
        };
        if (nthreads == 1) work(0);
        else { std::vector<std::thread> th; for (int t = 0; t < nthreads; t++) th.emplace_back(work, t); for (auto &x : th) x.join(); }
        size_t total = 0; for (auto &v : part) total += v.size();
        if (total > B.jobs_cap) return SGX_ERR_NOMEM;
        sorted.resize(total); blk_start.clear();
        size_t off = 0;
        for (int t = 0; t < nthreads; t++) {
            if (!part[(size_t)t].empty()) memcpy(sorted.data() + off, part[(size_t)t].data(), sizeof(SgxBaJob) * part[(size_t)t].size());
            for (int b : pblk[(size_t)t]) blk_start.push_back((int)off + b);
            off += part[(size_t)t].size();
        }
        blk_start.push_back((int)total);
    }
    B.njobs = (long long)sorted.size(); B.nblk = 0;
    if (sorted.empty()) return SGX_OK;
    B.nblk = (long long)blk_start.size() - 1;
    SGX_CHECK_HIP(hipMemcpy(B.jobs, sorted.data(), sizeof(SgxBaJob) * sorted.size(), hipMemcpyHostToDevice));
    SGX_CHECK_HIP(hipMemcpy(B.blk_start, blk_start.data(), sizeof(int) * blk_start.size(), hipMemcpyHostToDevice));
    return SGX_OK;
}

// The same list built on the device (k_ba_jobs_row / k_ba_jobs_scan, sgx_ba_kernels.h): no host pass over the edges, no 25 MB upload at 2 000 keyframes, and after the
// classification pass no download of the edge records either — the kernels read the levels where k_ba_classify wrote them.  One 8-byte read-back (jobs, blocks) per build.
static int build_jobs_dev(BA &B)
{
#ifndef SGX_EMU
    B.njobs = 0; B.nblk = 0;
    if (B.nf < 1) return SGX_OK;
    const size_t lds = sizeof(int) * (size_t)B.nf;      // at most 16 KB (static_assert beside SGX_BA_MAX_DENSE): always inside the default dynamic LDS limit, so there is no fallback
    hipLaunchKernelGGL((k_ba_jobs_row<0>), dim3((unsigned)B.nf), dim3(64), lds, (sgx_stream_t)0, B.nf, B.free_pose, B.pose_start, B.pose_edges_l, B.pt_start, B.pt_edges, B.E, B.hidx,
                       B.row_jobs, B.row_blks, (const int *)nullptr, (const int *)nullptr, (SgxBaJob *)nullptr, (int *)nullptr);
    SGX_CHECK_HIP(hipGetLastError());
    SGX_LAUNCH(k_ba_jobs_scan, dim3(1), dim3(256), (sgx_stream_t)0, B.nf, B.row_jobs, B.row_blks, B.job_off, B.blk_off, B.jtot, B.blk_start);
    int tot[2] = { 0, 0 };                                // int like the kernels' sums: build_index refused every problem whose list could pass INT_MAX
    SGX_CHECK_HIP(hipMemcpy(tot, B.jtot, sizeof tot, hipMemcpyDeviceToHost));
    if ((size_t)tot[0] > B.jobs_cap) return SGX_ERR_NOMEM;
    B.njobs = tot[0]; B.nblk = tot[1];
    if (tot[0] == 0) return SGX_OK;
    hipLaunchKernelGGL((k_ba_jobs_row<1>), dim3((unsigned)B.nf), dim3(64), lds, (sgx_stream_t)0, B.nf, B.free_pose, B.pose_start, B.pose_edges_l, B.pt_start, B.pt_edges, B.E, B.hidx,
                       B.row_jobs, B.row_blks, B.job_off, B.blk_off, B.jobs, B.blk_start);
    SGX_CHECK_HIP(hipGetLastError());
    return SGX_OK;
#else
    (void)B; return SGX_ERR_UNSUPPORTED;
#endif
}

// the job list of the current active edge set, by the builder this call uses; reclassified: k_ba_classify has just changed the edges' levels
static int job_list(BA &B, const BaIndex &ix, bool reclassified)
{
    if (!B.sw.jobs_host) return build_jobs_dev(B);       // the kernels read the new levels in place
    if (!reclassified) return build_jobs_host(B, ix, nullptr);
    std::vector<SgxBaEdge> Eh(B.ne);                     // mirror the new levels on the host
    SGX_CHECK_HIP(hipMemcpy(Eh.data(), B.E, sizeof(SgxBaEdge) * B.ne, hipMemcpyDeviceToHost));
    std::vector<uint8_t> level1(B.ne);
    for (int k = 0; k < B.ne; k++) level1[k] = (Eh[k].flags & 2) ? 1 : 0;
    return build_jobs_host(B, ix, &level1);
}

// device state: one arena; the host->device inputs are packed contiguously and uploaded with one copy
static int upload(BA &B, const BaIndex &ix, const EnvPlan &plan, const sgx_ba_problem &P, int mode)
{
    Chol &C = B.C;
    B.np = ix.np; B.nl = ix.nl; B.ne = ix.ne; B.nf = ix.nf; C.NP = ix.NP; B.jobs_cap = ix.jobs_cap;
    const size_t np = ix.np, nl = ix.nl, ne = ix.ne, nf = ix.nf, NP = ix.NP;
    B.nblk_e = (B.ne + SGX_BA_THREADS - 1) / SGX_BA_THREADS; B.nblk_v = (std::max(B.np, B.nl) + SGX_BA_THREADS - 1) / SGX_BA_THREADS;
    const int rc = g_arena.layout([&](Arena &A) {
        A.input(&B.E, ix.E.data(), ne); A.input(&B.X, ix.Xd.data(), 3 * nl); A.input(&B.pt_start, ix.pt_start.data(), nl + 1); A.input(&B.pt_edges, ix.pt_edges.data(), ne);
        A.input(&B.pose_start, ix.pose_start.data(), np + 1); A.input(&B.pose_edges, ix.pose_edges.data(), ne); A.input(&B.hidx, ix.hidx.data(), np); A.input(&B.free_pose, ix.free_pose.data(), nf);
        A.input(&B.Tcw, P.poses, 16 * np);
        A.input(&B.fixed, mode == 0 ? P.pose_fixed : nullptr, np);      // mode 1: every keyframe is rewritten from its vertex (Optimizer.cc:200-214) -> flags stay 0
        A.input(&C.env_rstart, plan.rstart.data(), plan.rstart.size()); A.input(&C.env_rows, plan.rows.data(), plan.rows.size()); A.input(&B.pose_edges_l, ix.pose_edges_l.data(), ne);
        A.take(&B.row_jobs, nf); A.take(&B.row_blks, nf); A.take(&B.job_off, nf + 1); A.take(&B.blk_off, nf + 1); A.take(&B.jtot, 2);
        A.take(&B.T, np); A.take(&B.Tb, np); A.take(&B.Xb, 3 * nl); A.take(&B.err, 3 * ne);
        A.take(&B.Hll, 9 * nl); A.take(&B.bl, 3 * nl); A.take(&B.Hpl, 18 * ne); A.take(&B.W, 18 * ne); A.take(&B.Hpp, 36 * nf);
        A.take(&C.bp, NP); A.take(&C.S, NP * NP); A.take(&C.coef, NP); A.take(&C.xp, NP); A.take(&C.xsol, NP); A.take(&B.xl, 3 * nl);
        A.take(&B.Dinv, 9 * nl); A.take(&B.dwork, NP); A.take(&B.partial, B.nblk_v);
        A.take_parts(&B.trial_out, 1, &B.part_scale, B.nblk_v, &B.part_chi, B.nblk_e);
        A.take(&B.pt_active, nl); A.take(&B.erase, ne);
        A.take_parts(&C.env_S2, plan.nsep * plan.nsep, &C.env_x2, plan.nsep + 1);
        A.take(&B.jobs, ix.jobs_cap); A.take(&B.blk_start, ix.jobs_cap + 1); A.take(&C.Linv, (size_t)((ix.NP + SGX_NB - 1) / SGX_NB) * SGX_NB * SGX_NB);
    });
    if (rc != SGX_OK) return rc;
#ifdef SGX_DEBUG_TAPS
    if (B.sw.init_mode == 3) { const int prc = g_arena.poison_scratch(); if (prc != SGX_OK) return prc; }      // before the clears below and the first kernel
#endif
    C.ok = (int *)B.trial_out;
    if (plan.empty()) { C.env_rstart = nullptr; C.env_rows = nullptr; }
    B.env_nrows = plan.nrows(); C.env_nA = plan.nA; C.env_nB = plan.nB;
    SGX_CHECK_HIP(hipMemsetAsync(C.xp, 0, sizeof(double) * (NP ? NP : 1), 0));
    SGX_CHECK_HIP(hipMemsetAsync(C.xsol, 0, sizeof(double) * (NP ? NP : 1), 0));
    SGX_CHECK_HIP(hipMemsetAsync(B.xl, 0, sizeof(double) * 3 * nl, 0));
    SGX_CHECK_HIP(hipMemsetAsync(B.err, 0, sizeof(double) * 3 * ne, 0));
    SGX_CHECK_HIP(hipMemsetAsync(B.Hpl, 0, sizeof(double) * 18 * ne, 0));
    SGX_LAUNCH(k_ba_poses_in, dim3((B.np + SGX_BA_THREADS - 1) / SGX_BA_THREADS), dim3(SGX_BA_THREADS), (sgx_stream_t)0, B.np, B.Tcw, B.T);
    return SGX_OK;
}

// one optimizer.optimize(iterations) call; a failed launch is reported by the phase that made it
static int optimize(BA &B, int iterations, LmResult *res)
{
    const int rc = sgx_lm_solve(B, iterations, res);
    if (rc == SGX_OK) SGX_CHECK_HIP(hipGetLastError());
    return rc;
}

// level 1 for the edges over the chi2 / depth thresholds (final == 0, Optimizer.cc:662-707), or their erase flags (final == 1, :709-742)
static void classify(BA &B, int final) { SGX_LAUNCH(k_ba_classify, dim3(B.nblk_e), dim3(SGX_BA_THREADS), (sgx_stream_t)0, B.ne, B.E, B.T, B.X, B.err, final, B.erase); }

// results back to the caller: erase flags (mode 0), every pose that is not fixed, the landmarks through Converter::toCvMat(Vector3d) (Optimizer.cc:771-777 / :216-236)
static int download(BA &B, const BaIndex &ix, const sgx_ba_problem &P, int mode, uint8_t *edge_erase)
{
    if (mode == 0) classify(B, 1);
    SGX_LAUNCH(k_ba_poses_out, dim3((B.np + SGX_BA_THREADS - 1) / SGX_BA_THREADS), dim3(SGX_BA_THREADS), (sgx_stream_t)0, B.np, B.fixed, B.T, B.Tcw);
    SGX_CHECK_HIP(hipGetLastError());
    if (mode == 0) SGX_CHECK_HIP(hipMemcpy(edge_erase, B.erase, B.ne, hipMemcpyDeviceToHost));
    SGX_CHECK_HIP(hipMemcpy(P.poses, B.Tcw, 64 * (size_t)B.np, hipMemcpyDeviceToHost));
    std::vector<double> Xd(3 * (size_t)B.nl);
    SGX_CHECK_HIP(hipMemcpy(Xd.data(), B.X, sizeof(double) * Xd.size(), hipMemcpyDeviceToHost));
    for (int l = 0; l < B.nl; l++)
        if (mode == 0 || ix.pt_start[l + 1] > ix.pt_start[l])                                // BundleAdjustment: points without edges were removed from the graph (vbNotIncludedMP)
            for (int c = 0; c < 3; c++) P.points[3 * (size_t)l + c] = (float)Xd[3 * (size_t)l + c];
    return SGX_OK;
}
}  // namespace

SGX_TAP int sgx_ba_debug_last_plan(int32_t plan[4]) { if (!plan) return SGX_ERR_INVALID; for (int i = 0; i < 4; i++) plan[i] = g_ba_last_plan[i]; return SGX_OK; }
SGX_TAP int sgx_ba_debug_set_init(int mode) { g_ba_init_mode = mode < 0 ? 0 : (mode > 3 ? 3 : mode); return SGX_OK; }
SGX_TAP int sgx_ba_debug_set_jobs(int host) { g_ba_jobs_host = host ? 1 : 0; return SGX_OK; }
SGX_TAP int sgx_ba_debug_set_solver(int mode) { g_ba_solver = mode < 0 ? -1 : (mode > 2 ? 2 : mode); return SGX_OK; }

// mode 0: Optimizer::LocalBundleAdjustment (Optimizer.cc:453-778); mode 1: Optimizer::BundleAdjustment (Optimizer.cc:49-237): one optimize(n_iterations) over
// all edges, Huber deltas sqrt(5.99) / sqrt(7.815) only when `robust`, no classification, every pose rewritten
static int ba_run(const sgx_ba_problem *P, const sgx_camera *cam, const volatile int32_t *stop_flag, uint8_t *edge_erase, sgx_ba_stats *stats, int mode, int n_iterations, int robust)
{
    if (!P || !cam || (mode == 0 && !edge_erase) || P->n_poses < 1 || P->n_points < 1 || P->n_edges < 1 || !P->poses || !P->pose_fixed || !P->points ||
        !P->edge_pose || !P->edge_point || !P->edge_obs || !P->edge_info) return SGX_ERR_INVALID;
    std::lock_guard<std::mutex> arena_lock(g_arena_mutex);
    const BaSwitches sw = ba_switches();
    PhaseClock phases{sw.timing != 0};
    if (stats) memset(stats, 0, sizeof *stats);
    if (edge_erase) memset(edge_erase, 0, P->n_edges);
    if (mode == 0 && stop_flag && *stop_flag) return SGX_OK;                                 // Optimizer.cc:655-657
    BaIndex ix;
    int rc = build_index(*P, &ix); if (rc != SGX_OK) return rc;
    const EnvPlan plan = plan_solver(ix, sw);
    phases.lap("index + solver plan");
    BA B{};
    B.sw = sw; B.stop = stop_flag;
    B.cam.fx = cam->fx; B.cam.fy = cam->fy; B.cam.cx = cam->cx; B.cam.cy = cam->cy; B.cam.bf = cam->bf;
    B.dMono = (double)(float)sqrt(5.991); B.dStereo = (double)(float)sqrt(7.815);          // Optimizer.cc:569-570 (float)
    if (mode == 1) { B.dMono = robust ? (double)(float)sqrt(5.99) : 1e150; B.dStereo = robust ? (double)(float)sqrt(7.815) : 1e150; }   // :83-84; no kernel = Huber that never leaves its quadratic zone
    if ((rc = upload(B, ix, plan, *P, mode)) != SGX_OK) return rc;
    plan.describe(ix.NP, g_ba_last_plan);
    phases.lap("arena + upload");
    LmResult first, second;
    if ((rc = job_list(B, ix, false)) != SGX_OK) return rc;
    phases.lap("schur job list 1");
    if ((rc = optimize(B, mode == 1 ? n_iterations : 5, &first)) != SGX_OK) return rc;       // Optimizer.cc:659-660 / :187-188
    phases.lap("optimize 1");
    if (mode == 0 && !B.stopped()) {                                                         // :662-707
        classify(B, 0);
        if ((rc = job_list(B, ix, true)) != SGX_OK) return rc;
        phases.lap("classify + job list 2");
        if ((rc = optimize(B, 10, &second)) != SGX_OK) return rc;
        phases.lap("optimize 2");
    }
    if ((rc = download(B, ix, *P, mode, edge_erase)) != SGX_OK) return rc;
    if (stats) { stats->iterations_first = first.iterations; stats->iterations_second = second.iterations; stats->chi2_first = first.chi_last; stats->chi2_second = second.chi_last; stats->free_poses = B.nf; }
    phases.lap("classify + download");
    return SGX_OK;
}

extern "C" int sgx_local_bundle_adjustment(const sgx_ba_problem *P, const sgx_camera *cam, const volatile int32_t *stop_flag,
                                           uint8_t *edge_erase, sgx_ba_stats *stats)
{
    return ba_run(P, cam, stop_flag, edge_erase, stats, 0, 0, 1);
}

extern "C" int sgx_bundle_adjustment(const sgx_ba_problem *P, const sgx_camera *cam, int n_iterations, const volatile int32_t *stop_flag, int robust, sgx_ba_stats *stats)
{
    if (n_iterations < 0) return SGX_ERR_INVALID;
    return ba_run(P, cam, stop_flag, nullptr, stats, 1, n_iterations, robust);
}


// ---------------------------------------------------------------------------------------------------------------------------------------------------------
// Optimizer::OptimizeEssentialGraph: the optimisation (Optimizer.cc:794, :961-962) on a flattened pose graph; kernels in sgx_eg_kernels.h
// ---------------------------------------------------------------------------------------------------------------------------------------------------------
namespace {
struct DevBufs {                                       // plain hipMalloc'ed buffers of one call (loop closing is rare: no arena)
    std::vector<void *> p; int rc = SGX_OK;            // rc: the first failure; requests after it do nothing, so the caller checks once after the last
    ~DevBufs() { for (void *q : p) (void)hipFree(q); }
    template <class T> void get(T **out, size_t n) { void *q = nullptr; *out = nullptr; if (rc != SGX_OK) return; if (hipMalloc(&q, (n ? n : 1) * sizeof(T)) != hipSuccess) { rc = SGX_ERR_NOMEM; return; } p.push_back(q); *out = (T *)q; }
    template <class T> void put(T **out, const T *src, size_t n) { get(out, n); if (rc == SGX_OK && n && hipMemcpy(*out, src, n * sizeof(T), hipMemcpyHostToDevice) != hipSuccess) rc = SGX_ERR_DEVICE; }
};

// incidence lists of the free vertices and the groups of edges that share an unordered vertex pair, both in edge order
struct EgIndex { std::vector<int> inc_start, inc_edge, pair_start, pair_lo, pair_hi, pair_edge; std::vector<uint8_t> inc_side, pair_flip; int npair = 0; };
static EgIndex build_eg_index(int nf, int ne, const int32_t *e_i, const int32_t *e_j, const std::vector<int> &hidx)
{
    EgIndex x;
    x.inc_start.assign((size_t)nf + 1, 0);
    for (int k = 0; k < ne; k++) { if (hidx[(size_t)e_i[k]] >= 0) x.inc_start[(size_t)hidx[(size_t)e_i[k]] + 1]++; if (hidx[(size_t)e_j[k]] >= 0) x.inc_start[(size_t)hidx[(size_t)e_j[k]] + 1]++; }
    for (int h = 0; h < nf; h++) x.inc_start[(size_t)h + 1] += x.inc_start[(size_t)h];
    x.inc_edge.resize((size_t)x.inc_start[(size_t)nf] > 0 ? (size_t)x.inc_start[(size_t)nf] : 1); x.inc_side.resize(x.inc_edge.size());
    { std::vector<int> fill((size_t)nf, 0);
      for (int k = 0; k < ne; k++) for (int side = 0; side < 2; side++) { const int h = hidx[(size_t)(side ? e_j[k] : e_i[k])]; if (h < 0) continue;
          const size_t q = (size_t)x.inc_start[(size_t)h] + (size_t)fill[(size_t)h]++; x.inc_edge[q] = k; x.inc_side[q] = (uint8_t)side; } }
    std::vector<int> order; order.reserve((size_t)ne);
    for (int k = 0; k < ne; k++) if (hidx[(size_t)e_i[k]] >= 0 && hidx[(size_t)e_j[k]] >= 0) order.push_back(k);
    auto lo_of = [&](int k) { return std::min(hidx[(size_t)e_i[k]], hidx[(size_t)e_j[k]]); };
    auto hi_of = [&](int k) { return std::max(hidx[(size_t)e_i[k]], hidx[(size_t)e_j[k]]); };
    std::stable_sort(order.begin(), order.end(), [&](int a, int b) { return lo_of(a) != lo_of(b) ? lo_of(a) < lo_of(b) : hi_of(a) < hi_of(b); });
    for (size_t q = 0; q < order.size(); q++) {
        const int k = order[q];
        if (q == 0 || lo_of(k) != lo_of(order[q - 1]) || hi_of(k) != hi_of(order[q - 1])) { x.pair_start.push_back((int)q); x.pair_lo.push_back(lo_of(k)); x.pair_hi.push_back(hi_of(k)); }
        x.pair_edge.push_back(k); x.pair_flip.push_back((uint8_t)(hidx[(size_t)e_i[k]] > hidx[(size_t)e_j[k]]));
    }
    x.pair_start.push_back((int)order.size());
    x.npair = (int)x.pair_lo.size();
    if (x.pair_edge.empty()) { x.pair_edge.push_back(0); x.pair_flip.push_back(0); }
    if (x.pair_lo.empty()) { x.pair_lo.push_back(0); x.pair_hi.push_back(0); }
    return x;
}

// One essential-graph optimisation on the device: the problem object of sgx_lm_solve (computeLambdaInit with setUserLambdaInit(1e-16), no stop flag)
struct EG {
    int nv = 0, ne = 0, nf = 0, npair = 0, fix_scale = 0, nblk_e = 0, nblk_v = 0;
    BaSwitches sw; Chol C; DevBufs D;
    double *V, *Vb, *M, *err, *blk, *H, *b, *part; int *ei, *ej, *hidx, *is, *ie, *ps, *pl, *ph, *pe; uint8_t *side, *flip;
    std::vector<double> hp;

    int alloc(const double *S_in, const int32_t *e_i, const int32_t *e_j, const double *e_meas, const std::vector<int> &h, const EgIndex &x)
    {
        const size_t NP = (size_t)C.NP;
        D.put(&V, S_in, 8 * (size_t)nv); D.get(&Vb, 8 * (size_t)nv); D.put(&M, e_meas, 8 * (size_t)ne); D.put(&ei, e_i, (size_t)ne); D.put(&ej, e_j, (size_t)ne);
        D.put(&hidx, h.data(), (size_t)nv); D.get(&err, 7 * (size_t)ne); D.get(&blk, (size_t)SGX_EG_BLK * ne);
        D.get(&H, NP * NP); D.get(&C.S, NP * NP); D.get(&b, NP); D.get(&C.bp, NP); D.get(&C.coef, NP); D.get(&C.xp, NP); D.get(&C.xsol, NP);
        D.get(&C.Linv, (size_t)((C.NP + SGX_NB - 1) / SGX_NB) * SGX_NB * SGX_NB); D.get(&C.ok, 4); D.get(&part, (size_t)std::max(nblk_e, nblk_v));
        D.put(&is, x.inc_start.data(), x.inc_start.size()); D.put(&ie, x.inc_edge.data(), x.inc_edge.size()); D.put(&side, x.inc_side.data(), x.inc_side.size());
        D.put(&ps, x.pair_start.data(), x.pair_start.size()); D.put(&pl, x.pair_lo.data(), x.pair_lo.size()); D.put(&ph, x.pair_hi.data(), x.pair_hi.size());
        D.put(&pe, x.pair_edge.data(), x.pair_edge.size()); D.put(&flip, x.pair_flip.data(), x.pair_flip.size());
        if (D.rc != SGX_OK) return D.rc;
        SGX_CHECK_HIP(hipMemset(C.xp, 0, sizeof(double) * NP)); SGX_CHECK_HIP(hipMemset(C.xsol, 0, sizeof(double) * NP));
        return SGX_OK;
    }
    bool stopped() const { return false; }
    int chi2(double *chi)
    {
        SGX_LAUNCH(k_eg_errors, dim3(nblk_e), dim3(SGX_EG_THREADS), (sgx_stream_t)0, ne, ei, ej, M, V, err, part);
        return read_back(hp, part, (size_t)nblk_e, chi);
    }
    int linearize()
    {
        SGX_LAUNCH(k_eg_linearize, dim3(nblk_e), dim3(SGX_EG_THREADS), (sgx_stream_t)0, ne, ei, ej, M, V, hidx, fix_scale, err, blk);
        SGX_CHECK_HIP(hipMemsetAsync(H, 0, sizeof(double) * (size_t)C.NP * C.NP, 0));
        SGX_LAUNCH(k_eg_assemble_diag, dim3(nf), dim3(64), (sgx_stream_t)0, C.NP, is, ie, side, blk, H, b);
        if (npair > 0) SGX_LAUNCH(k_eg_assemble_pairs, dim3(npair), dim3(64), (sgx_stream_t)0, C.NP, ps, pl, ph, pe, flip, blk, H);
        return SGX_OK;
    }
    int initial_lambda(double *lambda) { *lambda = 1e-16; return SGX_OK; }
    int trial(double lambda, LmTrial *t)
    {
        int rc;
        SGX_CHECK_HIP(hipMemcpyAsync(Vb, V, sizeof(double) * 8 * (size_t)nv, hipMemcpyDeviceToDevice, 0));       // push
        { const int one = 1; SGX_CHECK_HIP(hipMemcpyAsync(C.ok, &one, 4, hipMemcpyHostToDevice, 0)); }
        const size_t n2 = (size_t)C.NP * C.NP; const int g = (int)std::min<size_t>((n2 + SGX_EG_THREADS - 1) / SGX_EG_THREADS, 8192);
        SGX_LAUNCH(k_eg_damp, dim3(g), dim3(SGX_EG_THREADS), (sgx_stream_t)0, C.NP, H, b, lambda, C.S, C.bp, C.coef);
        const double *xsol = C.xp;
        if ((rc = chol_factor_solve(C, sw, &xsol)) != SGX_OK) return rc;
        SGX_LAUNCH(k_eg_update, dim3(nblk_v), dim3(SGX_EG_THREADS), (sgx_stream_t)0, nv, hidx, xsol, b, lambda, fix_scale, C.ok, Vb, V, part);
        if ((rc = read_back(hp, part, (size_t)nblk_v, &t->scale)) != SGX_OK) return rc;
        SGX_CHECK_HIP(hipMemcpy(&t->ok, C.ok, 4, hipMemcpyDeviceToHost));
        return chi2(&t->chi);
    }
    int reject() { SGX_CHECK_HIP(hipMemcpyAsync(V, Vb, sizeof(double) * 8 * (size_t)nv, hipMemcpyDeviceToDevice, 0)); return SGX_OK; }      // pop
};
}

extern "C" int sgx_optimize_essential_graph(int nv, const double *S_in, const uint8_t *fixed, int ne, const int32_t *e_i, const int32_t *e_j, const double *e_meas,
                                            int fix_scale, int iterations, double *S_out, double *stats)
{
    if (nv < 0 || ne < 0 || iterations < 0 || (nv > 0 && (!S_in || !fixed || !S_out)) || (ne > 0 && (!e_i || !e_j || !e_meas))) return SGX_ERR_INVALID;
    if (stats) { stats[0] = 0; stats[1] = 0; stats[2] = 0; }
    for (int k = 0; k < ne; k++) if (e_i[k] < 0 || e_i[k] >= nv || e_j[k] < 0 || e_j[k] >= nv || e_i[k] == e_j[k]) return SGX_ERR_INVALID;
    if (nv > 0 && S_out != S_in) memcpy(S_out, S_in, sizeof(double) * 8 * (size_t)nv);
    std::vector<int> hidx((size_t)(nv > 0 ? nv : 1), -1);
    int nf = 0;
    for (int v = 0; v < nv; v++) hidx[(size_t)v] = fixed[v] ? -1 : nf++;
    const int NP = 7 * nf;
    if (NP == 0 || ne == 0 || iterations == 0) return SGX_OK;
    if (NP > SGX_BA_MAX_DENSE) return SGX_ERR_UNSUPPORTED;
    const EgIndex x = build_eg_index(nf, ne, e_i, e_j, hidx);
    EG G;
    G.nv = nv; G.ne = ne; G.nf = nf; G.npair = x.npair; G.fix_scale = fix_scale; G.C.NP = NP; G.sw = ba_switches();
    G.nblk_e = (ne + SGX_EG_THREADS - 1) / SGX_EG_THREADS; G.nblk_v = (nv + SGX_EG_THREADS - 1) / SGX_EG_THREADS;
    int rc = G.alloc(S_in, e_i, e_j, e_meas, hidx, x); if (rc != SGX_OK) return rc;
    LmResult res;
    if ((rc = sgx_lm_solve(G, iterations, &res)) != SGX_OK) return rc;
    SGX_CHECK_HIP(hipMemcpy(S_out, G.V, sizeof(double) * 8 * (size_t)nv, hipMemcpyDeviceToHost));
    if (stats) { stats[0] = res.iterations; stats[1] = res.chi_first; stats[2] = res.chi_last; }
    return SGX_OK;
}

extern "C" int sgx_correct_map_points(int n, const float *xw, const int32_t *ref, int nv, const double *Srw, const double *corrected_Swr, float *xw_out)
{
    if (n < 0 || nv < 0 || (n > 0 && (!xw || !ref || !Srw || !corrected_Swr || !xw_out))) return SGX_ERR_INVALID;
    if (n == 0) return SGX_OK;
    for (int i = 0; i < n; i++) if (ref[i] < 0 || ref[i] >= nv) return SGX_ERR_INVALID;
    DevBufs D; float *dx, *dout; int *dref; double *da, *dc;
    D.put(&dx, xw, 3 * (size_t)n); D.put(&dref, ref, (size_t)n); D.put(&da, Srw, 8 * (size_t)nv); D.put(&dc, corrected_Swr, 8 * (size_t)nv); D.get(&dout, 3 * (size_t)n);
    if (D.rc != SGX_OK) return D.rc;
    SGX_LAUNCH(k_eg_correct_points, dim3((n + SGX_EG_THREADS - 1) / SGX_EG_THREADS), dim3(SGX_EG_THREADS), (sgx_stream_t)0, n, dx, dref, da, dc, dout);
    SGX_CHECK_HIP(hipGetLastError());
    SGX_CHECK_HIP(hipMemcpy(xw_out, dout, sizeof(float) * 3 * (size_t)n, hipMemcpyDeviceToHost));
    return SGX_OK;
}
