// sgx_orb.cpp — host side of the ORB extractor C-ABI (include/sgx.h): the handle and its device memory, the launches.  What creation decides (tables, level geometry, FAST
// runs, blur tiles, resize tables, the fused-pyramid plan) is planned in sgx_orb_plan.h before anything is allocated.  Compiled as HIP for gfx950 (product) or as plain C++
// with -DSGX_EMU (kernel-logic emulator, tests only).  Reference behaviour: src/sg-slam/src/ORBextractor.cc (cited inline).
#include "sgx_orb_kernels.h"
#include "sgx_prof.h"
#include "sgx_devmem.h"
#include "../../include/sgx.h"
#ifdef SGX_DEBUG_TAPS
#include "../../include/sgx_debug.h"      // test / tuning taps: compiled into tests/taps/libsgx_taps.so and the emulator only
#endif
#include "../../include/sgx_orb_pattern.h"
#include <math.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <new>
#include <vector>
#include "sgx_orb_plan.h"
#include "sgx_orb_view.h"

#ifdef SGX_EMU
thread_local sgx_dim3 blockIdx, blockDim, gridDim;
#endif


struct sgx_orb {
    sgx_orb_config cfg;
    OrbPlan p;                     // what creation decided; the launches read p.g, the pyramid plan, oct_maxlim and the packed umax
    SgxDevMem mem;                 // every device allocation of the handle
    // device tables: the plan's vectors
    SgxRun *d_runs = nullptr; SgxBlurTile *d_blur_tiles = nullptr; signed char *d_pattern = nullptr;
    SgxXTab *d_xt[SGX_MAX_LEVELS] = {}; SgxYTab *d_yt[SGX_MAX_LEVELS] = {};        // k_resize; d_yt[l] is level l's slice of d_yt_all
    SgxXGroup *d_xg_all = nullptr; SgxYTab *d_yt_all = nullptr; SgxPyrRect *d_pyr_rects = nullptr;      // fused pyramid (k_pyramid): concatenated tables, per (tile, level) rects
    // device workspace (sized for cfg.max_batch): pyramid levels 1.., blurred copy of every level (k_blur_levels), FAST candidates, octree scratch and sel lists, status bits
    uint8_t *d_pyr = nullptr, *d_blur = nullptr;
    uint32_t *d_cand = nullptr, *d_sel = nullptr, *d_status = nullptr; int *d_cand_count = nullptr, *d_sel_count = nullptr; uint16_t *d_node_scratch = nullptr;
    // single-frame staging for sgx_orb_extract
    uint8_t *d_gray1 = nullptr; uint8_t *d_kps1 = nullptr; uint8_t *d_desc1 = nullptr; int *d_count1 = nullptr;
    int detected_batch = 0;        // batch of the last sgx_orb_detect_batch_dev whose pyramid and sel lists are still in the workspace (0: none; any other extraction clears it)
    // the pyramid in the workspace: frames of the last extraction or detection (0: none), the level-0 image it was built from, 1 when that image is d_gray1 (sgx_orb_extract)
    int pyr_batch = 0; const uint8_t *pyr_gray = nullptr; int pyr_gray_pitch = 0, pyr_staged = 0;
};

static thread_local int g_orb_unfused_pyramid = 0;      // test tap: 1 = one k_resize launch per level instead of the fused k_pyramid
SGX_TAP int sgx_orb_debug_set_unfused_pyramid(int on) { g_orb_unfused_pyramid = on ? 1 : 0; return SGX_OK; }

// Every tuning switch of the extractor's launches, filled at the top of a C entry (orb_switches()) from the environment.  The product build has no environment switches
// (sgx_rt.h: sgx_getenv() is a constant NULL): every member folds to its default there.
struct OrbSwitches {
    int oct_threads = SGX_OCT_THREADS;      // SGX_TUNE_OCT_THREADS: k_octree workgroup size (64..SGX_OCT_THREADS)
    // SGX_TUNE_OCT_FRAME_FAST: (frames, levels) dispatch order of k_octree — all level-0 workgroups first, small levels in the tail — instead of (levels, frames).  It runs the
    // kernel itself 30 % faster at 256 frames (0.33 -> 0.22 ms) but the two-stream pipeline 1.5 % slower (A/B on one box: 112.5 k vs 114.1 k frames/s), so it is not the default
    bool oct_frame_fast = false;
    int pyr_threads = 512;                  // SGX_TUNE_PYR_THREADS: k_pyramid workgroup size (64..1024; measured: 0.130 / 0.086 / 0.073 ms per 64 frames at 128 / 256 / 512)
    int fast_threads = SGX_FAST_THREADS;    // SGX_TUNE_FAST_THREADS: k_fast_cells workgroup size (64..SGX_FAST_THREADS, whole waves)
    int e_extra_lds = 0;                    // SGX_TUNE_E_EXTRA_LDS: pad the extraction kernels' LDS to cap their occupancy
    int blur_threads = 256;                 // SGX_TUNE_BLUR_THREADS: k_blur_levels workgroup size (256..512)
    int blur_grid = 4096;                   // SGX_TUNE_ORB_BLUR_GRID: target grid size of k_blur_levels (measured at 512 frames with the round-3 walk: 0.59 / 0.48 / 0.46 ms at 1 024 / 2 048 / 4 096)
    bool patch_blur = false;                // SGX_TUNE_ORB_PATCH_BLUR: the first design, blur of a 37x37 window per keypoint inside k_orient_desc (tap build only)
    bool one_per_wave = false;              // SGX_TUNE_ORB_DESC_ONE_PER_WAVE: k_orient_desc2, one keypoint per wave (tap build only)
};

static OrbSwitches orb_switches()
{
    auto env = [](const char *name, int &v) { if (const char *e = sgx_getenv(name)) v = atoi(e); };
    OrbSwitches s;
    env("SGX_TUNE_OCT_THREADS", s.oct_threads); env("SGX_TUNE_PYR_THREADS", s.pyr_threads); env("SGX_TUNE_E_EXTRA_LDS", s.e_extra_lds); env("SGX_TUNE_ORB_BLUR_GRID", s.blur_grid);
    env("SGX_TUNE_FAST_THREADS", s.fast_threads); s.fast_threads = std::min(SGX_FAST_THREADS, std::max(64, s.fast_threads & ~63));
    env("SGX_TUNE_BLUR_THREADS", s.blur_threads); s.blur_threads = std::min(512, std::max(256, s.blur_threads));
    s.oct_frame_fast = sgx_getenv("SGX_TUNE_OCT_FRAME_FAST") != nullptr;
    s.patch_blur = sgx_getenv("SGX_TUNE_ORB_PATCH_BLUR") != nullptr; s.one_per_wave = sgx_getenv("SGX_TUNE_ORB_DESC_ONE_PER_WAVE") != nullptr;
    return s;
}

extern "C" const char *sgx_version(void) {
#ifdef SGX_EMU
    return "sgx 0.1 (EMULATOR - tests only)";
#else
    return "sgx 0.1 (gfx950)";
#endif
}

extern "C" const char *sgx_status_string(int s)
{
    switch (s) {
    case SGX_OK: return "ok";
    case SGX_ERR_INVALID: return "invalid argument";
    case SGX_ERR_UNSUPPORTED: return "unsupported geometry";
    case SGX_ERR_NOMEM: return "out of memory";
    case SGX_ERR_DEVICE: return "HIP runtime error";
    case SGX_ERR_OVERFLOW: return "device buffer overflow";
    default: return "unknown";
    }
}

extern "C" void sgx_orb_destroy(sgx_orb *h) { delete h; }

// the plan's tables and the workspace as device allocations of the handle
static int orb_allocate(sgx_orb *h)
{
    const OrbPlan &p = h->p; const SgxOrbGeom &g = p.g;
    const size_t B = (size_t)h->cfg.max_batch, nl = (size_t)g.nlevels;
    SgxDevMem &m = h->mem;
    int rc;
    if ((rc = m.upload(&h->d_runs, p.runs)) || (rc = m.upload(&h->d_blur_tiles, p.blur_tiles)) || (rc = m.upload(&h->d_pattern, sgx_orb_pattern_xy, 1024)) ||
        (rc = m.upload(&h->d_yt_all, p.yt_all)) || (rc = m.upload(&h->d_xg_all, p.xgroups)) || (rc = m.upload(&h->d_pyr_rects, p.rects))) return rc;
    for (size_t l = 1; l < nl; l++) {
        if ((rc = m.upload(&h->d_xt[l], p.xt[l]))) return rc;
        h->d_yt[l] = h->d_yt_all + p.pyr_tabs.yoff[l];
    }
    if (m.alloc(&h->d_pyr, B * g.pyr_pitch + 256) || m.alloc(&h->d_blur, B * g.blur_pitch + 256) || m.alloc(&h->d_cand, B * g.cand_pitch) ||
        m.alloc(&h->d_node_scratch, B * g.cand_pitch) || m.alloc(&h->d_cand_count, B * nl) || m.alloc(&h->d_sel, B * nl * SGX_OCT_MAXN) ||
        m.alloc(&h->d_sel_count, B * nl) || m.alloc(&h->d_status, 1) ||
        m.alloc(&h->d_gray1, (size_t)((g.W + 3) & ~3) * g.H) ||          // staging copy of a host frame, rows padded to dwords (the kernels stage aligned dwords)
        m.alloc(&h->d_kps1, (size_t)g.kp_cap * 28) || m.alloc(&h->d_desc1, (size_t)g.kp_cap * 32) || m.alloc(&h->d_count1, 1)) return SGX_ERR_NOMEM;
    SGX_CHECK_HIP(hipMemsetAsync(h->d_status, 0, 4, 0));
    SGX_CHECK_HIP(hipStreamSynchronize(0));
    return SGX_OK;
}

extern "C" int sgx_orb_create(const sgx_orb_config *cfg, sgx_orb **out)
{
    if (!cfg || !out) return SGX_ERR_INVALID;
    *out = nullptr;
    if (cfg->nlevels < 1 || cfg->nlevels > SGX_MAX_LEVELS || cfg->nfeatures < 1 || cfg->width < 64 || cfg->height < 64 ||
        cfg->width > 4000 || cfg->height > 4000 || cfg->max_batch < 1 || !(cfg->scale_factor > 1.0f)) return SGX_ERR_INVALID;
    sgx_orb *h = new (std::nothrow) sgx_orb();
    if (!h) return SGX_ERR_NOMEM;
    h->cfg = *cfg;
    int rc;
    try { rc = orb_plan(*cfg, &h->p); if (!rc) rc = orb_allocate(h); } catch (const std::bad_alloc &) { rc = SGX_ERR_NOMEM; }
    if (rc) { delete h; return rc; }          // the single failure exit: the handle owns whatever was allocated so far
    *out = h;
    return SGX_OK;
}

extern "C" int sgx_orb_keypoint_capacity(const sgx_orb *h) { return h ? h->p.g.kp_cap : SGX_ERR_INVALID; }

extern "C" int sgx_orb_get_tables(const sgx_orb *h, float *scale, float *inv_scale, float *sigma2, float *inv_sigma2, int32_t *per_level)
{
    if (!h) return SGX_ERR_INVALID;
    for (int l = 0; l < h->p.g.nlevels; l++) {
        if (scale) scale[l] = h->p.scale[l];
        if (inv_scale) inv_scale[l] = h->p.inv_scale[l];
        if (sigma2) sigma2[l] = h->p.sigma2[l];
        if (inv_sigma2) inv_sigma2[l] = h->p.inv_sigma2[l];
        if (per_level) per_level[l] = h->p.g.lv[l].quota;
    }
    return SGX_OK;
}

// k_octree launches.  Candidate-count classes: small LDS footprints let several (frame, level) workgroups share a CU; each block runs in exactly one launch.
static void launch_octree(sgx_orb *h, const OrbSwitches &sw, int batch, sgx_stream_t stream)
{
    const SgxOrbGeom &g = h->p.g; const int nl = g.nlevels;
    const dim3 ogrid = sw.oct_frame_fast ? dim3(batch, nl) : dim3(nl, batch);
    // nk_lo: the class takes the (frame, level) lists with more candidates than that
    const auto launch = [&](auto kern, int nk_lo) { SGX_LAUNCH(kern, ogrid, dim3(sw.oct_threads), stream, g, h->d_cand, h->d_cand_count, h->d_node_scratch, h->d_sel, h->d_sel_count, h->d_status, nk_lo); };
    if (h->p.oct_maxlim <= 256) {
        launch(k_octree<true, 256, 2048>, -1); launch(k_octree<true, 256, SGX_CAND_LDS>, 2048); launch(k_octree<false, 256, 1>, SGX_CAND_LDS);
    } else {
        launch(k_octree<true, SGX_OCT_MAXN, SGX_CAND_LDS>, -1); launch(k_octree<false, SGX_OCT_MAXN, 1>, SGX_CAND_LDS);
    }
}

// ComputePyramid, ComputeKeyPointsOctTree (ORBextractor.cc:1045-1084): pyramid, FAST cells, octree -> the per-(frame, level) sel lists in the handle;
// with d_kps, also the keypoint records without orientation (sgx_orb_detect_batch_dev)
static int launch_detect(sgx_orb *h, const OrbSwitches &sw, const uint8_t *d_gray, int pitch, int batch, sgx_stream_t stream, sgx_keypoint *d_kps = nullptr, int32_t *d_count = nullptr, int cap = 0)
{
    const OrbPlan &p = h->p; const SgxOrbGeom &g = p.g;
    const int nl = g.nlevels;
    SGX_CHECK_HIP(hipMemsetAsync(h->d_cand_count, 0, (size_t)batch * nl * 4, stream));
    sgx_prof_begin(SGX_K_RESIZE, stream);
    if (p.pyr_tiles > 0 && !g_orb_unfused_pyramid)
        SGX_LAUNCH_DYN(k_pyramid, dim3(p.pyr_tiles, batch), dim3(sw.pyr_threads), p.pyr_lds, stream, g, p.pyr_tabs, d_gray, pitch, h->d_pyr, h->d_xg_all, h->d_yt_all, h->d_pyr_rects);
    else
        for (int l = 1; l < nl; l++) {
            dim3 grid((g.lv[l].w + 255) / 256, (g.lv[l].h + 3) / 4, batch);
            SGX_LAUNCH(k_resize, grid, dim3(256), stream, g, l, d_gray, pitch, h->d_pyr, h->d_xt[l], h->d_yt[l]);
        }
    sgx_prof_end(SGX_K_RESIZE, stream);
    sgx_prof_begin(SGX_K_FAST, stream);
    SGX_LAUNCH_DYN(k_fast_cells, dim3(g.nruns * batch), dim3(sw.fast_threads), g.fast_lds_bytes + sw.e_extra_lds, stream, g, h->d_runs, d_gray, pitch, h->d_pyr, batch,
               h->d_cand, h->d_cand_count, h->d_status);
    sgx_prof_end(SGX_K_FAST, stream);
    sgx_prof_begin(SGX_K_OCTREE, stream);
    launch_octree(h, sw, batch, stream);
    if (d_kps) SGX_LAUNCH(k_octree_keys, dim3((g.kp_cap + 255) / 256, batch), dim3(256), stream, g, h->d_sel, h->d_sel_count, (uint8_t *)d_kps, d_count, cap, h->d_status);
    sgx_prof_end(SGX_K_OCTREE, stream);
    return SGX_OK;
}

// GaussianBlur of every level (ORBextractor.cc:1086-1087) into h->d_blur, then orientation and descriptor (:78-148) of every keypoint of the sel lists (count to d_count), or
// with d_src / d_n_kept of the survivors of an erase step alone
static int launch_describe(sgx_orb *h, const OrbSwitches &sw, const uint8_t *d_gray, int pitch, int batch, sgx_stream_t stream,
                           sgx_keypoint *d_kps, uint8_t *d_desc, int32_t *d_count, int cap, const int32_t *d_src = nullptr, const int32_t *d_n_kept = nullptr)
{
    const SgxOrbGeom &g = h->p.g;
    sgx_prof_begin(SGX_K_ORIENT_DESC, stream);
    // default: blur whole levels once (k_blur_levels), then a light per-keypoint kernel; SGX_TUNE_ORB_PATCH_BLUR=1 selects the first design (blur of a
    // 37x37 window per keypoint inside k_orient_desc) — identical bytes (tests), ~45 vs ~20+ VALU operations per pixel-equivalent
#ifdef SGX_DEBUG_TAPS      // the superseded descriptor kernels (k_orient_desc: blur per keypoint window; k_orient_desc2: one keypoint per wave) exist in the tap build only, for every keypoint
    if (sw.patch_blur && !d_src) {
        SGX_LAUNCH_DYN(k_orient_desc, dim3(g.kp_cap * batch), dim3(64), sw.e_extra_lds / 2, stream, g, d_gray, pitch, h->d_pyr, h->d_sel, h->d_sel_count,
                       h->p.umax_packed, h->d_pattern, (uint8_t *)d_kps, d_desc, d_count, cap, batch, h->d_status);
    } else
#endif
    {
        // persistent workgroups: `parts` per frame, each walks a contiguous range of the frame's tiles (see k_blur_levels); about 4 096 workgroups = 16 per CU
        const int parts = std::min(g.nblur_tiles, std::max(1, sw.blur_grid / batch));
        SGX_LAUNCH(k_blur_levels, dim3(parts * batch), dim3(sw.blur_threads), stream, g, h->d_blur_tiles, d_gray, pitch, h->d_pyr, h->d_blur, batch);
        const auto desc4 = [&](auto kern) { SGX_LAUNCH(kern, dim3(((g.kp_cap + 3) / 4) * batch), dim3(64), stream, g, d_gray, pitch, h->d_pyr, h->d_blur, h->d_sel, h->d_sel_count,
                                                       h->p.umax_packed, h->d_pattern, (uint8_t *)d_kps, d_desc, d_count, cap, batch, h->d_status, d_src, d_n_kept); };
#ifdef SGX_DEBUG_TAPS
        if (sw.one_per_wave && !d_src)
            SGX_LAUNCH(k_orient_desc2, dim3(g.kp_cap * batch), dim3(64), stream, g, d_gray, pitch, h->d_pyr, h->d_blur, h->d_sel, h->d_sel_count,
                       h->p.umax_packed, h->d_pattern, (uint8_t *)d_kps, d_desc, d_count, cap, batch, h->d_status);
        else
#endif
        if (d_src) desc4(k_orient_desc4<true>); else desc4(k_orient_desc4<false>);
    }
    sgx_prof_end(SGX_K_ORIENT_DESC, stream);
    SGX_CHECK_HIP(hipGetLastError());
    return SGX_OK;
}

// the frame arguments of the three batch entries; each adds its own rule for `batch`
static bool frames_ok(const sgx_orb *h, const uint8_t *d_gray, int pitch, int batch, int cap)
{
    return batch >= 1 && pitch >= h->p.g.W && !(pitch & 3) && !((uintptr_t)d_gray & 3) && cap >= h->p.g.kp_cap;
}

extern "C" int sgx_orb_extract_batch_dev(sgx_orb *h, const uint8_t *d_gray, int pitch, int batch,
                                         sgx_keypoint *d_kps, uint8_t *d_desc, int32_t *d_count, int cap, void *stream_)
{
    if (!h || !d_gray || !d_kps || !d_desc || !d_count) return SGX_ERR_INVALID;
    if (!frames_ok(h, d_gray, pitch, batch, cap) || batch > h->cfg.max_batch) return SGX_ERR_INVALID;
    const OrbSwitches sw = orb_switches();
    h->detected_batch = 0; h->pyr_batch = 0;
    { const int rc = launch_detect(h, sw, d_gray, pitch, batch, (sgx_stream_t)stream_); if (rc != SGX_OK) return rc; }
    { const int rc = launch_describe(h, sw, d_gray, pitch, batch, (sgx_stream_t)stream_, d_kps, d_desc, d_count, cap); if (rc != SGX_OK) return rc; }
    h->pyr_batch = batch; h->pyr_gray = d_gray; h->pyr_gray_pitch = pitch; h->pyr_staged = 0;
    return SGX_OK;
}

// The extractor in two calls, for callers that erase keypoints between detection and description (the dynamic-feature mask): see include/sgx.h
extern "C" int sgx_orb_detect_batch_dev(sgx_orb *h, const uint8_t *d_gray, int pitch, int batch, sgx_keypoint *d_kps, int32_t *d_count, int cap, void *stream_)
{
    if (!h || !d_gray || !d_kps || !d_count) return SGX_ERR_INVALID;
    if (!frames_ok(h, d_gray, pitch, batch, cap) || batch > h->cfg.max_batch) return SGX_ERR_INVALID;
    h->detected_batch = 0; h->pyr_batch = 0;
    { const int rc = launch_detect(h, orb_switches(), d_gray, pitch, batch, (sgx_stream_t)stream_, d_kps, d_count, cap); if (rc != SGX_OK) return rc; }
    SGX_CHECK_HIP(hipGetLastError());
    h->detected_batch = batch;
    h->pyr_batch = batch; h->pyr_gray = d_gray; h->pyr_gray_pitch = pitch; h->pyr_staged = 0;
    return SGX_OK;
}

extern "C" int sgx_orb_describe_batch_dev(sgx_orb *h, const uint8_t *d_gray, int pitch, int batch, const int32_t *d_src, const int32_t *d_n_kept,
                                          sgx_keypoint *d_kps, uint8_t *d_desc, int cap, void *stream_)
{
    if (!h || !d_gray || !d_src || !d_n_kept || !d_kps || !d_desc) return SGX_ERR_INVALID;
    if (!frames_ok(h, d_gray, pitch, batch, cap) || batch != h->detected_batch) return SGX_ERR_INVALID;
    return launch_describe(h, orb_switches(), d_gray, pitch, batch, (sgx_stream_t)stream_, d_kps, d_desc, nullptr, cap, d_src, d_n_kept);
}

extern "C" int sgx_orb_last_status(sgx_orb *h, void *stream_)
{
    if (!h) return SGX_ERR_INVALID;
    uint32_t st = 0;
    SGX_CHECK_HIP(hipMemcpyAsync(&st, h->d_status, 4, hipMemcpyDeviceToHost, (sgx_stream_t)stream_));
    SGX_CHECK_HIP(hipStreamSynchronize((sgx_stream_t)stream_));
    if (st) { SGX_CHECK_HIP(hipMemsetAsync(h->d_status, 0, 4, (sgx_stream_t)stream_)); return SGX_ERR_OVERFLOW; }
    return SGX_OK;
}

extern "C" int sgx_orb_extract(sgx_orb *h, const uint8_t *gray, int stride, sgx_keypoint *kps, uint8_t *desc, int cap, int *n)
{
    if (!h || !gray || !kps || !desc || !n || stride < h->p.g.W || cap < 0) return SGX_ERR_INVALID;
    const int W = h->p.g.W, H = h->p.g.H, kc = h->p.g.kp_cap, P = (W + 3) & ~3;      // any image width (KITTI: 1241): the device copy is pitched to dwords
    if (stride == P) SGX_CHECK_HIP(hipMemcpyAsync(h->d_gray1, gray, (size_t)P * (H - 1) + W, hipMemcpyHostToDevice, 0));
    else for (int y = 0; y < H; y++)
        SGX_CHECK_HIP(hipMemcpyAsync(h->d_gray1 + (size_t)y * P, gray + (size_t)y * stride, W, hipMemcpyHostToDevice, 0));
    int rc = sgx_orb_extract_batch_dev(h, h->d_gray1, P, 1, (sgx_keypoint *)h->d_kps1, h->d_desc1, h->d_count1, kc, 0);
    if (rc != SGX_OK) return rc;
    h->pyr_staged = 1;
    int cnt = 0;
    SGX_CHECK_HIP(hipMemcpyAsync(&cnt, h->d_count1, 4, hipMemcpyDeviceToHost, 0));
    SGX_CHECK_HIP(hipStreamSynchronize(0));
    rc = sgx_orb_last_status(h, 0);
    if (rc != SGX_OK) return rc;
    if (cnt > cap) return SGX_ERR_OVERFLOW;
    SGX_CHECK_HIP(hipMemcpyAsync(kps, h->d_kps1, (size_t)cnt * 28, hipMemcpyDeviceToHost, 0));
    SGX_CHECK_HIP(hipMemcpyAsync(desc, h->d_desc1, (size_t)cnt * 32, hipMemcpyDeviceToHost, 0));
    SGX_CHECK_HIP(hipStreamSynchronize(0));
    *n = cnt;
    return SGX_OK;
}

// the handle as another unit of the library may see it (sgx_orb_view.h)
static_assert(SGX_VIEW_LEVELS == SGX_MAX_LEVELS, "sgx_orb_view.h mirrors the level tables");
int sgx_orb_view(const sgx_orb *h, SgxOrbView *v)
{
    if (!h || !v) return SGX_ERR_INVALID;
    memset(v, 0, sizeof *v);
    const SgxOrbGeom &g = h->p.g;
    v->lv.nlevels = g.nlevels; v->lv.W = g.W; v->lv.H = g.H; v->lv.kp_cap = g.kp_cap; v->lv.pyr_pitch = g.pyr_pitch;
    for (int l = 0; l < g.nlevels; l++) {
        v->lv.w[l] = g.lv[l].w; v->lv.h[l] = g.lv[l].h; v->lv.stride[l] = g.lv[l].stride; v->lv.off[l] = g.lv[l].off;
        v->lv.scale[l] = h->p.scale[l]; v->lv.inv_scale[l] = h->p.inv_scale[l];
    }
    v->lv.stride[0] = 0; v->lv.off[0] = 0;          // level 0 is the caller's image: its pitch is an argument of every call
    v->d_pyr = h->d_pyr; v->d_gray = h->pyr_gray; v->gray_pitch = h->pyr_gray_pitch; v->pyr_batch = h->pyr_batch; v->staged = h->pyr_staged;
    return SGX_OK;
}

SGX_TAP int sgx_orb_debug_level_geometry(const sgx_orb *h, int level, int32_t *w, int32_t *hgt, int32_t *stride)
{
    if (!h || level < 0 || level >= h->p.g.nlevels) return SGX_ERR_INVALID;
    if (w) *w = h->p.g.lv[level].w; if (hgt) *hgt = h->p.g.lv[level].h; if (stride) *stride = h->p.g.lv[level].stride;
    return SGX_OK;
}

SGX_TAP int sgx_orb_debug_read_level(sgx_orb *h, int frame, int level, uint8_t *dst)
{
    if (!h || !dst || level < 1 || level >= h->p.g.nlevels || frame < 0 || frame >= h->cfg.max_batch) return SGX_ERR_INVALID;
    const SgxLevel &L = h->p.g.lv[level];
    for (int y = 0; y < L.h; y++)
        SGX_CHECK_HIP(hipMemcpyAsync(dst + (size_t)y * L.w, h->d_pyr + (size_t)frame * h->p.g.pyr_pitch + L.off + (size_t)y * L.stride, L.w, hipMemcpyDeviceToHost, 0));
    SGX_CHECK_HIP(hipStreamSynchronize(0));
    return SGX_OK;
}

SGX_TAP int sgx_orb_debug_read_candidates(sgx_orb *h, int frame, int level, int32_t *x, int32_t *y, int32_t *score, int cap, int *n)
{
    if (!h || !n || level < 0 || level >= h->p.g.nlevels || frame < 0 || frame >= h->cfg.max_batch) return SGX_ERR_INVALID;
    const SgxOrbGeom &g = h->p.g;
    int cnt = 0;
    SGX_CHECK_HIP(hipMemcpyAsync(&cnt, h->d_cand_count + frame * g.nlevels + level, 4, hipMemcpyDeviceToHost, 0));
    SGX_CHECK_HIP(hipStreamSynchronize(0));
    if (cnt > g.lv[level].cand_cap) cnt = g.lv[level].cand_cap;
    std::vector<uint32_t> buf(cnt > 0 ? cnt : 1);
    SGX_CHECK_HIP(hipMemcpyAsync(buf.data(), h->d_cand + (size_t)frame * g.cand_pitch + g.lv[level].cand_off, (size_t)cnt * 4, hipMemcpyDeviceToHost, 0));
    SGX_CHECK_HIP(hipStreamSynchronize(0));
    for (int i = 0; i < cnt && i < cap; i++) { x[i] = buf[i] & 0xFFF; y[i] = (buf[i] >> 12) & 0xFFF; score[i] = buf[i] >> 24; }
    *n = cnt;
    return SGX_OK;
}

// test tap: run k_octree alone on a caller-supplied candidate list for `level` (frame slot 0)
SGX_TAP int sgx_orb_debug_run_octree(sgx_orb *h, int level, const uint32_t *packed, int n, uint32_t *out_sel, int cap, int *nsel)
{
    if (!h || !packed || !out_sel || !nsel || level < 0 || level >= h->p.g.nlevels || n < 0 || n > h->p.g.lv[level].cand_cap) return SGX_ERR_INVALID;
    const int nl = h->p.g.nlevels;
    std::vector<int> cnt(nl, 0); cnt[level] = n;
    SGX_CHECK_HIP(hipMemcpyAsync(h->d_cand_count, cnt.data(), nl * 4, hipMemcpyHostToDevice, 0));
    SGX_CHECK_HIP(hipMemcpyAsync(h->d_cand + h->p.g.lv[level].cand_off, packed, (size_t)n * 4, hipMemcpyHostToDevice, 0));
    launch_octree(h, orb_switches(), 1, (sgx_stream_t)0);
    int ns = 0;
    SGX_CHECK_HIP(hipMemcpyAsync(&ns, h->d_sel_count + level, 4, hipMemcpyDeviceToHost, 0));
    SGX_CHECK_HIP(hipStreamSynchronize(0));
    if (ns > cap) return SGX_ERR_OVERFLOW;
    SGX_CHECK_HIP(hipMemcpyAsync(out_sel, h->d_sel + (size_t)level * SGX_OCT_MAXN, (size_t)ns * 4, hipMemcpyDeviceToHost, 0));
    SGX_CHECK_HIP(hipStreamSynchronize(0));
    *nsel = ns;
    return sgx_orb_last_status(h, 0);
}

// test tap: what creation decided, one section per call (include/sgx_debug.h); the tables are read back from their device copies
SGX_TAP int sgx_orb_debug_read_plan(const sgx_orb *h, int section, void *dst, size_t cap, size_t *bytes)
{
    if (!h || !bytes || section < 0 || section > 8) return SGX_ERR_INVALID;
    const OrbPlan &p = h->p; const int nl = p.g.nlevels;
    struct { SgxPyrTabs tabs; int pyr_tiles, pyr_lds, oct_maxlim, pad; unsigned long long umax_packed; } misc;
    struct Part { const void *p; size_t n; bool dev; };
    std::vector<Part> parts;
    switch (section) {
    case 0: parts.push_back({&p.g, sizeof p.g, false}); break;
    case 1: parts.push_back({h->d_runs, p.runs.size() * sizeof(SgxRun), true}); break;
    case 2: parts.push_back({h->d_blur_tiles, p.blur_tiles.size() * sizeof(SgxBlurTile), true}); break;
    case 3: for (int l = 1; l < nl; l++) parts.push_back({h->d_xt[l], p.g.lv[l].w * sizeof(SgxXTab), true}); break;
    case 4: for (int l = 1; l < nl; l++) parts.push_back({h->d_yt[l], p.g.lv[l].h * sizeof(SgxYTab), true}); break;      // through the pointers k_resize is given
    case 5: parts.push_back({h->d_xg_all, p.xgroups.size() * sizeof(SgxXGroup), true}); break;
    case 6: parts.push_back({h->d_yt_all, p.yt_all.size() * sizeof(SgxYTab), true}); break;
    case 7: parts.push_back({h->d_pyr_rects, p.rects.size() * sizeof(SgxPyrRect), true}); break;
    default:
        memset(&misc, 0, sizeof misc);
        misc.tabs = p.pyr_tabs; misc.pyr_tiles = p.pyr_tiles; misc.pyr_lds = p.pyr_lds; misc.oct_maxlim = p.oct_maxlim; misc.umax_packed = p.umax_packed;
        parts.push_back({&misc, sizeof misc, false});
    }
    size_t total = 0;
    for (const Part &q : parts) total += q.n;
    *bytes = total;
    if (!dst) return SGX_OK;
    if (cap < total) return SGX_ERR_OVERFLOW;
    char *o = (char *)dst;
    for (const Part &q : parts) {
        if (!q.n) continue;
        if (q.dev) SGX_CHECK_HIP(hipMemcpy(o, q.p, q.n, hipMemcpyDeviceToHost)); else memcpy(o, q.p, q.n);
        o += q.n;
    }
    return SGX_OK;
}
