// sgx_pnp.cpp — host side of PnPsolver (src/sg-slam/src/PnPsolver.cc) behind the C ABI: B solvers with their correspondences, RANSAC parameters, glibc rand()
// replicas and persistent state (mnIterations, the best model) on the device; iterate() runs the kernels of sgx_pnp_kernels.h in chunks of SGX_PNP_MAXIT hypotheses.
// The single solver (sgx_pnp_solver_*) is a batch of one fed from host memory.
#include "sgx_pnp_kernels.h"
#include "sgx_grand.h"
#include "sgx_devmem.h"
#include "../../include/sgx.h"
#include <limits.h>
#include <math.h>
#include <stdio.h>
#include <string.h>
#include <vector>
#ifdef SGX_DEBUG_TAPS
#include "../../include/sgx_debug.h"      // test taps: compiled into tests/taps/libsgx_taps.so and the emulator only
#endif

// replica draws of one chunk (one lane per solver): the state at the start of the call is kept in saved; the draws of a chunk continue from the live state
SGX_KERNEL(64) k_pnp_rng(SgxPnpArgs A, int32_t *rng, int32_t *saved, int32_t *draws, int save)
{
    SGX_THREADS_BEGIN(tid)
    const int b = (int)blockIdx.x * 64 + tid;
    if (b < A.B) {
        int32_t *g = rng + SGX_GRAND_WORDS * b, *sv = saved + SGX_GRAND_WORDS * b;
        if (save) for (int i = 0; i < SGX_GRAND_WORDS; i++) sv[i] = g[i];
        const int total = sgx_pnp_call_total(A.state + SGX_PNP_ST * b, A.n_iterations);
        int nh = total - A.chunk0; if (nh > A.chunk_n) nh = A.chunk_n; if (nh < 0 || A.call[SGX_PNP_CS * b] >= 0) nh = 0;
        for (int i = 0; i < 4 * nh; i++) draws[(size_t)b * 4 * A.cap + i] = sgx_grand(g);
    }
    SGX_THREADS_END
}

// after the call: the replica gives back the draws of the iterations that did not run (the state = the saved one advanced by 4 x iterations run)
SGX_KERNEL(64) k_pnp_rng_commit(SgxPnpArgs A, int32_t *rng, const int32_t *saved)
{
    SGX_THREADS_BEGIN(tid)
    const int b = (int)blockIdx.x * 64 + tid;
    if (b < A.B) {
        int32_t *g = rng + SGX_GRAND_WORDS * b; const int32_t *sv = saved + SGX_GRAND_WORDS * b;
        for (int i = 0; i < SGX_GRAND_WORDS; i++) g[i] = sv[i];
        for (int i = 0; i < 4 * A.call[SGX_PNP_CS * b + 1]; i++) (void)sgx_grand(g);
    }
    SGX_THREADS_END
}

SGX_KERNEL(64) k_pnp_call_reset(SgxPnpArgs A)
{
    SGX_THREADS_BEGIN(tid)
    const int b = (int)blockIdx.x * 64 + tid;
    if (b < A.B) { int *cs = A.call + SGX_PNP_CS * b; cs[0] = -1; cs[1] = 0; cs[2] = 0; cs[3] = 0; }
    SGX_THREADS_END
}

struct sgx_pnp_batch {
    int maxB = 0, maxN = 0, B = 0, ntot = 0, max_its = 1, cap = 0;       // cap: hypotheses per solver that hyp / counts / draws hold
    std::vector<int> offsets_h;
    int *offsets = nullptr, *state = nullptr, *call = nullptr, *counts = nullptr, *draws = nullptr, *rng = nullptr, *rng_saved = nullptr;
    float *p2d = nullptr, *p3dw = nullptr, *sigma2 = nullptr, *cam = nullptr, *th2 = nullptr, *best_tcw = nullptr, *tcw_out = nullptr;
    uint8_t *best_mask = nullptr, *inl_out = nullptr;
    double *hyp = nullptr, *ws = nullptr;
    SgxDevMem mem;
};

extern "C" int sgx_pnp_batch_create(int max_solvers, int max_correspondences, sgx_pnp_batch **out)
{
    if (out) *out = nullptr;
    if (!out || max_solvers < 1 || max_correspondences < 0) return SGX_ERR_INVALID;
    sgx_pnp_batch *t = new sgx_pnp_batch;
    const size_t B = (size_t)max_solvers, N = (size_t)(max_correspondences > 0 ? max_correspondences : 1);
    t->maxB = max_solvers; t->maxN = max_correspondences;
    SgxDevMem &m = t->mem;
    int rc;
    if ((rc = m.alloc(&t->offsets, B + 1)) || (rc = m.alloc(&t->state, SGX_PNP_ST * B)) || (rc = m.alloc(&t->call, SGX_PNP_CS * B)) ||
        (rc = m.alloc(&t->rng, SGX_GRAND_WORDS * B)) || (rc = m.alloc(&t->rng_saved, SGX_GRAND_WORDS * B)) || (rc = m.alloc(&t->p2d, 2 * N)) || (rc = m.alloc(&t->p3dw, 3 * N)) ||
        (rc = m.alloc(&t->sigma2, N)) || (rc = m.alloc(&t->cam, 4 * B)) || (rc = m.alloc(&t->th2, B)) || (rc = m.alloc(&t->best_tcw, 16 * B)) ||
        (rc = m.alloc(&t->tcw_out, 16 * B)) || (rc = m.alloc(&t->best_mask, N)) || (rc = m.alloc(&t->inl_out, N)) || (rc = m.alloc(&t->ws, 36 * N))) { delete t; return rc; }
    *out = t;
    return SGX_OK;
}

extern "C" void sgx_pnp_batch_destroy(sgx_pnp_batch *t) { delete t; }

// hypothesis buffers for `need` hypotheses per solver (a relocalisation call runs about 35; at most SGX_PNP_MAXIT per launch).  All or nothing: after a failure the
// batch holds none of the three and cap is 0
static int pnp_reserve(sgx_pnp_batch *t, int need)
{
    if (need <= t->cap) return SGX_OK;
    const auto drop = [t] { t->mem.release(t->hyp); t->mem.release(t->counts); t->mem.release(t->draws); t->hyp = nullptr; t->counts = nullptr; t->draws = nullptr; t->cap = 0; };
    drop();
    const size_t B = (size_t)t->maxB, c = (size_t)need;
    int rc;
    if ((rc = t->mem.alloc(&t->hyp, SGX_PNP_HYP * c * B)) || (rc = t->mem.alloc(&t->counts, c * B)) || (rc = t->mem.alloc(&t->draws, 4 * c * B))) { drop(); return rc; }
    t->cap = need;
    return SGX_OK;
}

// SetRansacParameters (:121-157) for n correspondences: the adjusted mRansacMinInliers and mRansacMaxIts
static int pnp_ransac(int N, const double *p, int *min_inliers, int *max_its)
{
    const double prob = p[0]; int minIn = (int)p[1], maxIts = (int)p[2]; const int minSet = (int)p[3]; float eps = (float)p[4];
    if (minSet != 4 || !(prob > 0 && prob < 1) || maxIts < 1 || minIn < 0) return SGX_ERR_INVALID;       // the hypothesis kernel solves EPnP on four points
    int nMinInliers = (int)((float)N * eps);
    if (nMinInliers < minIn) nMinInliers = minIn;
    if (nMinInliers < minSet) nMinInliers = minSet;
    minIn = nMinInliers;
    if (eps < (float)minIn / (float)N) eps = (float)minIn / (float)N;
    int nIterations;
    if (minIn == N) nIterations = 1;
    else {
        const double v = ceil(log(1 - prob) / log(1 - pow((double)eps, 3.0)));
        nIterations = (v == v && v < 2147483648.0 && v >= -2147483648.0) ? (int)v : INT_MIN;   // x86's conversion of NaN / out of range (N = 0 or minInliers > N)
    }
    const int m = nIterations < maxIts ? nIterations : maxIts;
    *min_inliers = minIn; *max_its = m > 1 ? m : 1;
    return SGX_OK;
}

static SgxPnpArgs pnp_args(sgx_pnp_batch *t, int n_iterations)
{
    SgxPnpArgs A; memset(&A, 0, sizeof A);
    A.B = t->B; A.n_iterations = n_iterations; A.offsets = t->offsets; A.p2d = t->p2d; A.p3dw = t->p3dw; A.sigma2 = t->sigma2; A.cam = t->cam; A.th2 = t->th2;
    A.state = t->state; A.best_tcw = t->best_tcw; A.best_mask = t->best_mask; A.call = t->call; A.hyp = t->hyp; A.counts = t->counts; A.ws = t->ws;
    A.tcw_out = t->tcw_out; A.inl_out = t->inl_out;
    return A;
}

extern "C" int sgx_pnp_batch_set_dev(sgx_pnp_batch *t, int B, const int32_t *offsets, const float *p2d_dev, const float *sigma2_dev, const float *p3dw_dev,
                                     const float *cam, const double *ransac, const uint32_t *rand_seeds, void *stream)
{
    if (!t || B < 1 || B > t->maxB || !offsets || !cam || !ransac || offsets[0] != 0) return SGX_ERR_INVALID;
    for (int b = 0; b < B; b++) if (offsets[b + 1] < offsets[b]) return SGX_ERR_INVALID;
    const int n = offsets[B];
    if (n > t->maxN || (n > 0 && (!p2d_dev || !sigma2_dev || !p3dw_dev))) return SGX_ERR_INVALID;
    std::vector<int> st((size_t)SGX_PNP_ST * B, 0), rng((size_t)SGX_GRAND_WORDS * B);
    std::vector<float> th2(B), tcw((size_t)16 * B, 0.f);
    int max_its = 1;
    for (int b = 0; b < B; b++) {
        const int N = offsets[b + 1] - offsets[b]; int minIn, maxIts;
        const int r = pnp_ransac(N, ransac + 6 * b, &minIn, &maxIts);
        if (r != SGX_OK) return r;
        int *s = st.data() + SGX_PNP_ST * b;
        s[SGX_PNP_N] = N; s[SGX_PNP_MININ] = minIn; s[SGX_PNP_MAXITS] = maxIts;
        th2[b] = (float)ransac[6 * b + 5];
        if (maxIts > max_its) max_its = maxIts;
        sgx_gsrand(rand_seeds ? rand_seeds[b] : 0u, rng.data() + SGX_GRAND_WORDS * b);
    }
    const sgx_stream_t s = (sgx_stream_t)stream;
    t->B = 0;                                                    // not set until every copy below has arrived: iterate_dev refuses a batch that a failed copy left half written
    SGX_CHECK_HIP(hipMemcpyAsync(t->offsets, offsets, 4 * (size_t)(B + 1), hipMemcpyHostToDevice, s));
    SGX_CHECK_HIP(hipMemcpyAsync(t->state, st.data(), 4 * st.size(), hipMemcpyHostToDevice, s));
    SGX_CHECK_HIP(hipMemcpyAsync(t->rng, rng.data(), 4 * rng.size(), hipMemcpyHostToDevice, s));
    SGX_CHECK_HIP(hipMemcpyAsync(t->th2, th2.data(), 4 * (size_t)B, hipMemcpyHostToDevice, s));
    SGX_CHECK_HIP(hipMemcpyAsync(t->cam, cam, 16 * (size_t)B, hipMemcpyHostToDevice, s));
    SGX_CHECK_HIP(hipMemcpyAsync(t->best_tcw, tcw.data(), 64 * (size_t)B, hipMemcpyHostToDevice, s));
    if (n > 0) {
        SGX_CHECK_HIP(hipMemcpyAsync(t->p2d, p2d_dev, 8 * (size_t)n, hipMemcpyDeviceToDevice, s));
        SGX_CHECK_HIP(hipMemcpyAsync(t->p3dw, p3dw_dev, 12 * (size_t)n, hipMemcpyDeviceToDevice, s));
        SGX_CHECK_HIP(hipMemcpyAsync(t->sigma2, sigma2_dev, 4 * (size_t)n, hipMemcpyDeviceToDevice, s));
        SGX_CHECK_HIP(hipMemsetAsync(t->best_mask, 0, (size_t)n, s));
    }
    // host inputs are staged: the caller may reuse them when this returns
    SGX_CHECK_HIP(hipStreamSynchronize(s));
    t->offsets_h.assign(offsets, offsets + B + 1);
    t->B = B; t->ntot = n; t->max_its = max_its;
    return SGX_OK;
}

extern "C" int sgx_pnp_batch_iterate_dev(sgx_pnp_batch *t, int n_iterations, const int32_t *rand_draws_dev, int draw_stride, int32_t *result_dev, float *tcw_dev,
                                         uint8_t *inliers_dev, void *stream)
{
    if (!t || t->B < 1 || n_iterations < 0 || !result_dev || !tcw_dev || (t->ntot > 0 && !inliers_dev) || (rand_draws_dev && draw_stride < 0)) return SGX_ERR_INVALID;
    const sgx_stream_t s = (sgx_stream_t)stream;
    SgxPnpArgs A = pnp_args(t, n_iterations);
    A.tcw_out = tcw_dev; A.inl_out = inliers_dev;
    const int nb = (t->B + 63) / 64;
    SGX_LAUNCH(k_pnp_call_reset, dim3(nb), dim3(64), s, A);
    // a call runs at most max(nIterations, mRansacMaxIts) hypotheses; solvers that are done skip the later chunks
    const int most = n_iterations > t->max_its ? n_iterations : t->max_its;
    const int chunk = most < SGX_PNP_MAXIT ? (most > 1 ? most : 1) : SGX_PNP_MAXIT;
    const int rr = pnp_reserve(t, chunk);
    if (rr != SGX_OK) return rr;
    A.cap = t->cap; A.hyp = t->hyp; A.counts = t->counts;         // (re)allocated by pnp_reserve
    for (int c0 = 0; c0 < most; c0 += chunk) {
        A.chunk0 = c0; A.chunk_n = most - c0 < chunk ? most - c0 : chunk;
        if (rand_draws_dev) { A.draws = rand_draws_dev; A.draw_stride = draw_stride; A.draw_base = 0; }
        else {                                                       // the replica's draws of this chunk, solver b at b * 4 * cap
            SGX_LAUNCH(k_pnp_rng, dim3(nb), dim3(64), s, A, t->rng, t->rng_saved, t->draws, c0 == 0 ? 1 : 0);
            A.draws = t->draws; A.draw_stride = 4 * A.cap; A.draw_base = c0;
        }
        SGX_LAUNCH(k_pnp_hyp, dim3((unsigned)((A.chunk_n + 63) / 64), (unsigned)t->B), dim3(64), s, A);
        SGX_LAUNCH(k_pnp_count, dim3((unsigned)t->B), dim3(256), s, A);
        SGX_LAUNCH(k_pnp_replay, dim3((unsigned)t->B), dim3(256), s, A);
    }
    if (!rand_draws_dev) SGX_LAUNCH(k_pnp_rng_commit, dim3(nb), dim3(64), s, A, t->rng, t->rng_saved);
    SGX_LAUNCH(k_pnp_finish, dim3(nb), dim3(64), s, A, result_dev);
    SGX_CHECK_HIP(hipGetLastError());
    return SGX_OK;
}

// ------------------------------------------------------------------------------------------------------------------------------------------------ single solver
struct sgx_pnp_solver {
    sgx_pnp_batch *t = nullptr;
    int N = 0, minIn = 0, maxIts = 1;
    int32_t *res = nullptr, *dd = nullptr; float *tcw = nullptr; uint8_t *inl = nullptr;
    size_t dd_cap = 0;                                           // int32 values dd holds: the caller's draws of the longest call so far
    SgxDevMem mem;
    ~sgx_pnp_solver() { delete t; }
};

extern "C" int sgx_pnp_solver_create(int n, const float *p2d, const float *sigma2, const float *p3dw, const float *cam4, unsigned rand_seed, sgx_pnp_solver **out)
{
    if (out) *out = nullptr;
    if (!out || n < 0 || !cam4 || (n > 0 && (!p2d || !sigma2 || !p3dw))) return SGX_ERR_INVALID;
    sgx_pnp_solver *s = new sgx_pnp_solver;
    s->N = n;
    const size_t m = (size_t)n;
    const int32_t off[2] = { 0, n };
    const double defaults[6] = { 0.99, 8, 300, 4, 0.4f, 5.991f };                // SetRansacParameters() defaults (PnPsolver.h:67-68)
    const uint32_t seed = rand_seed;
    SgxDevMem staged;                                            // the correspondences on their way into the batch of one
    float *d2 = nullptr, *ds = nullptr, *d3 = nullptr;
    int rc;
    if ((rc = sgx_pnp_batch_create(1, n, &s->t)) || (rc = s->mem.alloc(&s->res, 4)) || (rc = s->mem.alloc(&s->tcw, 16)) || (rc = s->mem.alloc(&s->inl, m)) ||
        (rc = staged.upload(&d2, p2d, 2 * m)) || (rc = staged.upload(&ds, sigma2, m)) || (rc = staged.upload(&d3, p3dw, 3 * m)) ||
        (rc = sgx_pnp_batch_set_dev(s->t, 1, off, d2, ds, d3, cam4, defaults, &seed, nullptr))) { delete s; return rc; }
    pnp_ransac(n, defaults, &s->minIn, &s->maxIts);
    *out = s;
    return SGX_OK;
}

extern "C" void sgx_pnp_solver_destroy(sgx_pnp_solver *s) { delete s; }

extern "C" int sgx_pnp_solver_set_ransac_parameters(sgx_pnp_solver *s, double probability, int min_inliers, int max_iterations, int min_set, float epsilon, float th2)
{
    if (!s) return SGX_ERR_INVALID;
    const double p[6] = { probability, (double)min_inliers, (double)max_iterations, (double)min_set, (double)epsilon, (double)th2 };
    int minIn, maxIts;
    const int r = pnp_ransac(s->N, p, &minIn, &maxIts);
    if (r != SGX_OK) return r;
    // mnIterations and the best model are kept, as in the reference
    int st[SGX_PNP_ST];
    SGX_CHECK_HIP(hipMemcpy(st, s->t->state, sizeof st, hipMemcpyDeviceToHost));
    st[SGX_PNP_MININ] = minIn; st[SGX_PNP_MAXITS] = maxIts;
    st[SGX_PNP_BEST_FAILED] = 0;                                  // Refine's outcome on the best set depends on minInliers and th2: the reference reruns it
    SGX_CHECK_HIP(hipMemcpy(s->t->state, st, sizeof st, hipMemcpyHostToDevice));
    SGX_CHECK_HIP(hipMemcpy(s->t->th2, &th2, 4, hipMemcpyHostToDevice));
    s->minIn = minIn; s->maxIts = maxIts; s->t->max_its = maxIts;
    return SGX_OK;
}

extern "C" int sgx_pnp_solver_get_estimate(const sgx_pnp_solver *s, float *best_tcw, int32_t *max_iterations, int32_t *min_inliers, int32_t *iterations, int32_t *best_inliers)
{
    if (!s) return SGX_ERR_INVALID;
    int st[SGX_PNP_ST];
    SGX_CHECK_HIP(hipMemcpy(st, s->t->state, sizeof st, hipMemcpyDeviceToHost));
    if (best_tcw) SGX_CHECK_HIP(hipMemcpy(best_tcw, s->t->best_tcw, 64, hipMemcpyDeviceToHost));
    if (max_iterations) *max_iterations = st[SGX_PNP_MAXITS];
    if (min_inliers) *min_inliers = st[SGX_PNP_MININ];
    if (iterations) *iterations = st[SGX_PNP_ITS];
    if (best_inliers) *best_inliers = st[SGX_PNP_BEST];
    return SGX_OK;
}

extern "C" int sgx_pnp_solver_iterate(sgx_pnp_solver *s, int n_iterations, const int32_t *rand_draws, float *Tcw, int32_t *no_more, uint8_t *inliers, int32_t *n_inliers,
                                      int32_t *found, int32_t *iterations_run)
{
    if (!s || !Tcw || !no_more || !n_inliers || !found || (s->N > 0 && !inliers) || n_iterations < 0) return SGX_ERR_INVALID;
    int st[SGX_PNP_ST];
    SGX_CHECK_HIP(hipMemcpy(st, s->t->state, sizeof st, hipMemcpyDeviceToHost));
    int total = n_iterations > st[SGX_PNP_MAXITS] - st[SGX_PNP_ITS] ? n_iterations : st[SGX_PNP_MAXITS] - st[SGX_PNP_ITS];
    if (total < 0 || s->N < st[SGX_PNP_MININ]) total = 0;
    if (rand_draws && total > 0) {
        if (4 * (size_t)total > s->dd_cap) {
            s->mem.release(s->dd); s->dd = nullptr; s->dd_cap = 0;
            const int rc = s->mem.alloc(&s->dd, 4 * (size_t)total);
            if (rc != SGX_OK) return rc;
            s->dd_cap = 4 * (size_t)total;
        }
        SGX_CHECK_HIP(hipMemcpy(s->dd, rand_draws, 16 * (size_t)total, hipMemcpyHostToDevice));
    }
    const int r = sgx_pnp_batch_iterate_dev(s->t, n_iterations, rand_draws && total > 0 ? s->dd : nullptr, 0, s->res, s->tcw, s->inl, nullptr);
    if (r != SGX_OK) return r;
    int32_t res[4];
    SGX_CHECK_HIP(hipMemcpy(res, s->res, 16, hipMemcpyDeviceToHost));
    *found = res[0]; *no_more = res[1]; *n_inliers = res[2]; if (iterations_run) *iterations_run = res[3];
    if (res[0]) SGX_CHECK_HIP(hipMemcpy(Tcw, s->tcw, 64, hipMemcpyDeviceToHost));
    if (s->N > 0) SGX_CHECK_HIP(hipMemcpy(inliers, s->inl, (size_t)s->N, hipMemcpyDeviceToHost));
    return SGX_OK;
}

#ifdef SGX_DEBUG_TAPS
// test tap: the kernel's Gauss-Newton refinement (which = 0) or beta approximation `which` (1..3) on one lane, so that the tests can see the two defined undefined behaviours
SGX_KERNEL(64) k_pnp_debug_betas(const double *L, const double *rho, double *betas, int which)
{
    SGX_THREADS_BEGIN(tid)
    if (tid == 0) { if (which == 0) sgx_epnp_gauss_newton(L, rho, betas); else sgx_epnp_betas(L, rho, which, betas); }
    SGX_THREADS_END
}

SGX_TAP int sgx_pnp_debug_betas(int which, const double *L, const double *rho, double *betas)
{
    if (which < 0 || which > 3 || !L || !rho || !betas) return SGX_ERR_INVALID;
    double *d = nullptr;
    if (hipMalloc((void **)&d, 8 * 70) != hipSuccess) return SGX_ERR_NOMEM;
    bool ok = hipMemcpy(d, L, 8 * 60, hipMemcpyHostToDevice) == hipSuccess && hipMemcpy(d + 60, rho, 8 * 6, hipMemcpyHostToDevice) == hipSuccess &&
              hipMemcpy(d + 66, betas, 8 * 4, hipMemcpyHostToDevice) == hipSuccess;
    if (ok) { SGX_LAUNCH(k_pnp_debug_betas, dim3(1), dim3(64), (sgx_stream_t)0, (const double *)d, (const double *)(d + 60), d + 66, which);
              ok = hipGetLastError() == hipSuccess && hipMemcpy(betas, d + 66, 8 * 4, hipMemcpyDeviceToHost) == hipSuccess; }
    (void)hipFree(d);
    return ok ? SGX_OK : SGX_ERR_DEVICE;
}
#endif
