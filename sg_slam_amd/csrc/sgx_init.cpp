// sgx_init.cpp — host side of Initializer (src/sg-slam/src/Initializer.cc) behind the C ABI: B frame pairs with their keys, matches, intrinsics and glibc rand()
// replicas; run() is one launch sequence of the kernels of sgx_init_kernels.h for all pairs, the RANSAC iterations in chunks of SGX_INIT_MAXIT.
// The single initializer (sgx_initializer_*) is a batch of one fed from host memory.
#include "sgx_init_kernels.h"
#include "sgx_prof.h"
#include "sgx_devmem.h"
#include "../../include/sgx.h"
#include <math.h>
#include <stdio.h>
#include <string.h>
#include <vector>

static_assert(sizeof(SgxInitReport) == sizeof(sgx_init_report), "SgxInitReport mirrors sgx_init_report");
static_assert(sizeof(sgx_keypoint) == 28, "the kernels read a key as 7 words");

// parallax of CheckRT (:901) from the selected cosine, on the host: the one libm call of the path
static float init_parallax(float c) { return (float)(acos((double)c) * 180 / 3.1415926535897932384626433832795); }

// the largest cosine whose parallax passes `> 1` (strict) or `>= 1`: parallax is monotone in the cosine, so a bisection over the float bit patterns finds it
static float init_cos_threshold(bool strict)
{
    auto pass = [&](uint32_t bits) { float c; memcpy(&c, &bits, 4); const float p = init_parallax(c); return strict ? p > 1.0f : p >= 1.0f; };
    uint32_t lo, hi; const float a = 0.9f, b = 1.0f;
    memcpy(&lo, &a, 4); memcpy(&hi, &b, 4);
    while (hi - lo > 1) { const uint32_t mid = lo + (hi - lo) / 2; if (pass(mid)) lo = mid; else hi = mid; }
    float c; memcpy(&c, &lo, 4);
    return c;
}

struct sgx_init_batch {
    int maxB = 0, maxK = 0, maxM = 0, iterations = 0, cap = 0;
    float cos_gt = 0, cos_ge = 0;
    std::vector<int32_t> off1_h, off2_h, rng_h; std::vector<float> cam_h, sigma_h;
    int *off1 = nullptr, *off2 = nullptr, *nmatch = nullptr, *mi = nullptr, *ninl = nullptr, *dec = nullptr, *rng = nullptr, *draws = nullptr;
    float *cam = nullptr, *sigma = nullptr, *mxy = nullptr, *norm = nullptr, *hyp = nullptr, *scores = nullptr, *best = nullptr, *rt = nullptr, *cosp = nullptr, *pts = nullptr;
    uint8_t *inl = nullptr, *good = nullptr;
    SgxDevMem mem;
};

extern "C" int sgx_init_batch_create(int max_pairs, int max_keys, int max_matches, int iterations, sgx_init_batch **out)
{
    if (out) *out = nullptr;
    if (!out || max_pairs < 1 || max_keys < 0 || max_matches < 0 || iterations < 1) return SGX_ERR_INVALID;
    sgx_init_batch *t = new sgx_init_batch;
    t->maxB = max_pairs; t->maxK = max_keys; t->maxM = max_matches; t->iterations = iterations;
    t->cap = iterations < SGX_INIT_MAXIT ? iterations : SGX_INIT_MAXIT;
    t->cos_gt = init_cos_threshold(true); t->cos_ge = init_cos_threshold(false);
    const size_t B = (size_t)max_pairs, M = (size_t)(max_matches > 0 ? max_matches : 1), c = (size_t)t->cap;
    t->rng_h.resize(SGX_GRAND_WORDS * B);                        // every replica starts as srand(0)
    for (size_t b = 0; b < B; b++) sgx_gsrand(0u, t->rng_h.data() + SGX_GRAND_WORDS * b);
    SgxDevMem &m = t->mem;
    int rc;
    if ((rc = m.alloc(&t->off1, B + 1)) || (rc = m.alloc(&t->off2, B + 1)) || (rc = m.alloc(&t->nmatch, B)) || (rc = m.alloc(&t->mi, 2 * M)) || (rc = m.alloc(&t->ninl, 2 * B)) ||
        (rc = m.alloc(&t->dec, 2 * B)) || (rc = m.upload(&t->rng, t->rng_h)) || (rc = m.alloc(&t->draws, 8 * (size_t)iterations * B)) || (rc = m.alloc(&t->cam, 4 * B)) ||
        (rc = m.alloc(&t->sigma, B)) || (rc = m.alloc(&t->mxy, 4 * M)) || (rc = m.alloc(&t->norm, 8 * B)) || (rc = m.alloc(&t->hyp, SGX_INIT_HYP * 2 * c * B)) ||
        (rc = m.alloc(&t->scores, 2 * c * B)) || (rc = m.alloc(&t->best, 20 * B)) || (rc = m.alloc(&t->rt, 96 * B)) || (rc = m.alloc(&t->cosp, 8 * M)) ||
        (rc = m.alloc(&t->pts, 24 * M)) || (rc = m.alloc(&t->inl, 2 * M)) || (rc = m.alloc(&t->good, 8 * M))) { delete t; return rc; }
    *out = t;
    return SGX_OK;
}

extern "C" void sgx_init_batch_destroy(sgx_init_batch *t) { delete t; }

extern "C" int sgx_init_batch_run_dev(sgx_init_batch *t, int B, const int32_t *offsets1, const sgx_keypoint *keys1_dev, const int32_t *matches12_dev, const int32_t *offsets2,
                                      const sgx_keypoint *keys2_dev, const float *cam, const float *sigma, const uint32_t *rand_seeds, const int32_t *rand_draws_dev,
                                      int draw_stride, float *R21_dev, float *t21_dev, float *p3d_dev, uint8_t *triangulated_dev, uint8_t *inliers_dev, int32_t *ok_dev,
                                      sgx_init_report *report_dev, void *stream)
{
    if (!t || B < 1 || B > t->maxB || !offsets1 || !offsets2 || !cam || !sigma || offsets1[0] != 0 || offsets2[0] != 0 || !R21_dev || !t21_dev || !ok_dev || !report_dev)
        return SGX_ERR_INVALID;
    int widest = 0;
    for (int b = 0; b < B; b++) {
        if (offsets1[b + 1] < offsets1[b] || offsets2[b + 1] < offsets2[b]) return SGX_ERR_INVALID;
        if (offsets1[b + 1] - offsets1[b] > widest) widest = offsets1[b + 1] - offsets1[b];
    }
    const int n1 = offsets1[B], n2 = offsets2[B];
    if (n1 > t->maxK || n2 > t->maxK || n1 > t->maxM || (n1 > 0 && (!keys1_dev || !matches12_dev || !p3d_dev || !triangulated_dev || !inliers_dev)) || (n2 > 0 && !keys2_dev))
        return SGX_ERR_INVALID;
    if (rand_draws_dev && draw_stride < 8 * t->iterations && B > 1) return SGX_ERR_INVALID;
    const sgx_stream_t s = (sgx_stream_t)stream;
    // host inputs are staged in the batch: the caller may reuse them when this returns
    t->off1_h.assign(offsets1, offsets1 + B + 1); t->off2_h.assign(offsets2, offsets2 + B + 1); t->cam_h.assign(cam, cam + 4 * (size_t)B); t->sigma_h.assign(sigma, sigma + B);
    SGX_CHECK_HIP(hipMemcpyAsync(t->off1, t->off1_h.data(), 4 * (size_t)(B + 1), hipMemcpyHostToDevice, s));
    SGX_CHECK_HIP(hipMemcpyAsync(t->off2, t->off2_h.data(), 4 * (size_t)(B + 1), hipMemcpyHostToDevice, s));
    SGX_CHECK_HIP(hipMemcpyAsync(t->cam, t->cam_h.data(), 16 * (size_t)B, hipMemcpyHostToDevice, s));
    SGX_CHECK_HIP(hipMemcpyAsync(t->sigma, t->sigma_h.data(), 4 * (size_t)B, hipMemcpyHostToDevice, s));
    if (rand_seeds) {
        for (int b = 0; b < B; b++) sgx_gsrand(rand_seeds[b], t->rng_h.data() + SGX_GRAND_WORDS * (size_t)b);
        SGX_CHECK_HIP(hipMemcpyAsync(t->rng, t->rng_h.data(), 4 * SGX_GRAND_WORDS * (size_t)B, hipMemcpyHostToDevice, s));
    }
    SgxInitArgs A; memset(&A, 0, sizeof A);
    A.B = B; A.iterations = t->iterations; A.cap = t->cap; A.ntot = n1; A.off1 = t->off1; A.off2 = t->off2; A.keys1 = (const float *)keys1_dev; A.keys2 = (const float *)keys2_dev;
    A.matches12 = matches12_dev; A.cam = t->cam; A.sigma = t->sigma; A.cos_gt = t->cos_gt; A.cos_ge = t->cos_ge; A.nmatch = t->nmatch; A.mi = t->mi; A.mxy = t->mxy; A.norm = t->norm;
    A.hyp = t->hyp; A.scores = t->scores; A.best = t->best; A.inl = t->inl; A.ninl = t->ninl; A.dec = t->dec; A.rt = t->rt; A.good = t->good; A.cosp = t->cosp; A.pts = t->pts;
    A.R21 = R21_dev; A.t21 = t21_dev; A.p3d = p3d_dev; A.tri = triangulated_dev; A.inl_out = inliers_dev; A.ok = ok_dev; A.report = (SgxInitReport *)report_dev;
    if (rand_draws_dev) { A.draws = rand_draws_dev; A.draw_stride = draw_stride; }
    else { A.draws = t->draws; A.draw_stride = 8 * t->iterations; }
    const unsigned nb = (unsigned)((B + 63) / 64), nb2 = (unsigned)((2 * B + 63) / 64), gx = (unsigned)((widest + 255) / 256 > 0 ? (widest + 255) / 256 : 1);
    sgx_prof_begin(SGX_K_INIT_SETUP, s);
    SGX_LAUNCH(k_init_setup, dim3(nb), dim3(64), s, A, t->rng, rand_draws_dev ? (int32_t *)nullptr : t->draws);
    SGX_LAUNCH(k_init_normalize, dim3(nb2), dim3(64), s, A);
    sgx_prof_end(SGX_K_INIT_SETUP, s);
    for (int c0 = 0; c0 < t->iterations; c0 += t->cap) {
        A.chunk0 = c0; A.chunk_n = t->iterations - c0 < t->cap ? t->iterations - c0 : t->cap;
        sgx_prof_begin(SGX_K_INIT_HYP, s);
        SGX_LAUNCH(k_init_hyp, dim3((unsigned)((A.chunk_n + 63) / 64), (unsigned)B, 2), dim3(64), s, A);
        sgx_prof_end(SGX_K_INIT_HYP, s);
        sgx_prof_begin(SGX_K_INIT_SCORE, s);
        SGX_LAUNCH(k_init_score, dim3((unsigned)((A.chunk_n + 255) / 256), (unsigned)B, 2), dim3(256), s, A);
        SGX_LAUNCH(k_init_best, dim3(nb2), dim3(64), s, A);
        sgx_prof_end(SGX_K_INIT_SCORE, s);
    }
    sgx_prof_begin(SGX_K_INIT_DECIDE, s);
    SGX_LAUNCH(k_init_inliers, dim3(gx, (unsigned)B, 2), dim3(256), s, A);
    SGX_LAUNCH(k_init_decide, dim3(nb), dim3(64), s, A);
    sgx_prof_end(SGX_K_INIT_DECIDE, s);
    sgx_prof_begin(SGX_K_INIT_CHECK_RT, s);
    SGX_LAUNCH(k_init_check_rt, dim3(gx, (unsigned)B, 8), dim3(256), s, A);
    sgx_prof_end(SGX_K_INIT_CHECK_RT, s);
    sgx_prof_begin(SGX_K_INIT_FINISH, s);
    SGX_LAUNCH(k_init_finish, dim3((unsigned)B), dim3(256), s, A);
    sgx_prof_end(SGX_K_INIT_FINISH, s);
    SGX_CHECK_HIP(hipGetLastError());
    return SGX_OK;
}

// ------------------------------------------------------------------------------------------------------------------------------------------------ single initializer
struct sgx_initializer {
    sgx_init_batch *t = nullptr;
    int n1 = 0, iterations = 0;
    unsigned seed = 0;                                           // srand(seed) of the replica, applied when the batch of one is first sized
    float cam[4] = { 0, 0, 0, 0 }, sigma = 1.f;
    sgx_keypoint *k1 = nullptr, *k2 = nullptr; int32_t *m12 = nullptr, *dd = nullptr, *ok = nullptr;
    float *R = nullptr, *tt = nullptr, *p3d = nullptr; uint8_t *tri = nullptr, *inl = nullptr; sgx_init_report *rep = nullptr;
    SgxDevMem mem;
    ~sgx_initializer() { delete t; }
};

extern "C" int sgx_initializer_create(int n1, const sgx_keypoint *keys1_un, const float *cam4, float sigma, int iterations, unsigned rand_seed, sgx_initializer **out)
{
    if (out) *out = nullptr;
    if (!out || n1 < 0 || !cam4 || iterations < 1 || (n1 > 0 && !keys1_un)) return SGX_ERR_INVALID;
    sgx_initializer *s = new sgx_initializer;
    s->n1 = n1; s->iterations = iterations; s->sigma = sigma;
    for (int i = 0; i < 4; i++) s->cam[i] = cam4[i];
    const size_t m = (size_t)(n1 > 0 ? n1 : 1);
    SgxDevMem &d = s->mem;
    int rc;
    if ((rc = d.upload(&s->k1, keys1_un, (size_t)n1)) || (rc = d.alloc(&s->m12, m)) || (rc = d.alloc(&s->dd, 8 * (size_t)iterations)) || (rc = d.alloc(&s->ok, 1)) || (rc = d.alloc(&s->R, 9)) ||
        (rc = d.alloc(&s->tt, 3)) || (rc = d.alloc(&s->p3d, 3 * m)) || (rc = d.alloc(&s->tri, m)) || (rc = d.alloc(&s->inl, m)) || (rc = d.alloc(&s->rep, 1))) { delete s; return rc; }
    s->seed = rand_seed;                                        // the batch of one is sized at the first Initialize (n2 is not known before)
    *out = s;
    return SGX_OK;
}

extern "C" void sgx_initializer_destroy(sgx_initializer *s) { delete s; }

extern "C" int sgx_initializer_initialize(sgx_initializer *s, int n2, const sgx_keypoint *keys2_un, const int32_t *matches12, const int32_t *rand_draws, float *R21, float *t21,
                                          float *p3d, uint8_t *triangulated, uint8_t *inliers, int32_t *ok, sgx_init_report *report)
{
    if (!s || n2 < 0 || (n2 > 0 && !keys2_un) || !R21 || !t21 || !ok || (s->n1 > 0 && (!matches12 || !p3d || !triangulated || !inliers))) return SGX_ERR_INVALID;
    const int most = s->n1 > n2 ? s->n1 : n2;
    if (!s->t || s->t->maxK < most) {
        // (re)size for this frame 2 as a transaction: the new batch and the new k2 are built and the replica's state carried over before anything of the handle
        // changes, so a failure leaves the initializer as it was (usable at its old size, the replica unmoved)
        sgx_init_batch *nt = nullptr; sgx_keypoint *nk2 = nullptr;
        const auto carry_replica = [&]() -> int {
            if (s->t) SGX_CHECK_HIP(hipMemcpy(nt->rng, s->t->rng, 4 * SGX_GRAND_WORDS, hipMemcpyDeviceToDevice));
            else { int32_t g[SGX_GRAND_WORDS]; sgx_gsrand(s->seed, g); SGX_CHECK_HIP(hipMemcpy(nt->rng, g, sizeof g, hipMemcpyHostToDevice)); }
            return SGX_OK;
        };
        int r;
        if ((r = sgx_init_batch_create(1, most, s->n1, s->iterations, &nt)) || (r = s->mem.alloc(&nk2, (size_t)most)) || (r = carry_replica())) {
            delete nt; s->mem.release(nk2);
            return r;
        }
        delete s->t; s->t = nt;
        s->mem.release(s->k2); s->k2 = nk2;
    }
    if (n2 > 0) SGX_CHECK_HIP(hipMemcpy(s->k2, keys2_un, 28 * (size_t)n2, hipMemcpyHostToDevice));
    if (s->n1 > 0) SGX_CHECK_HIP(hipMemcpy(s->m12, matches12, 4 * (size_t)s->n1, hipMemcpyHostToDevice));
    if (rand_draws) SGX_CHECK_HIP(hipMemcpy(s->dd, rand_draws, 32 * (size_t)s->iterations, hipMemcpyHostToDevice));
    const int32_t off1[2] = { 0, s->n1 }, off2[2] = { 0, n2 };
    const int r = sgx_init_batch_run_dev(s->t, 1, off1, s->k1, s->m12, off2, s->k2, s->cam, &s->sigma, nullptr, rand_draws ? s->dd : nullptr, 8 * s->iterations, s->R, s->tt, s->p3d,
                                         s->tri, s->inl, s->ok, s->rep, nullptr);
    if (r != SGX_OK) return r;
    SGX_CHECK_HIP(hipMemcpy(ok, s->ok, 4, hipMemcpyDeviceToHost));
    SGX_CHECK_HIP(hipMemcpy(R21, s->R, 36, hipMemcpyDeviceToHost));
    SGX_CHECK_HIP(hipMemcpy(t21, s->tt, 12, hipMemcpyDeviceToHost));
    if (s->n1 > 0) {
        SGX_CHECK_HIP(hipMemcpy(p3d, s->p3d, 12 * (size_t)s->n1, hipMemcpyDeviceToHost));
        SGX_CHECK_HIP(hipMemcpy(triangulated, s->tri, (size_t)s->n1, hipMemcpyDeviceToHost));
        SGX_CHECK_HIP(hipMemcpy(inliers, s->inl, (size_t)s->n1, hipMemcpyDeviceToHost));
    }
    if (report) {
        SGX_CHECK_HIP(hipMemcpy(report, s->rep, sizeof(sgx_init_report), hipMemcpyDeviceToHost));
        for (int k = 0; k < report->n_hyp; k++) report->parallax[k] = report->n_good[k] > 0 ? init_parallax(report->cos_parallax[k]) : 0.f;
    }
    return SGX_OK;
}
