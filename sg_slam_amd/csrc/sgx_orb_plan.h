// sgx_orb_plan.h — host-only planning of an ORB extractor handle, before anything touches the device: everything sgx_orb_create decides (OrbPlan), one function per
// job, orb_plan() calls them in order and refuses unsupported geometries.  Included by sgx_orb.cpp only, after sgx_orb_kernels.h (the Sgx* table structs and limits).
// Guarded by tests/test_orb_plan.py (fixture of every table, emulator and device) and tests/test_orb_plan_probe.py (sanitizers).
#pragma once
#include <algorithm>
#include <vector>

struct OrbPlan {
    SgxOrbGeom g = {};
    float scale[SGX_MAX_LEVELS] = {}, inv_scale[SGX_MAX_LEVELS] = {}, sigma2[SGX_MAX_LEVELS] = {}, inv_sigma2[SGX_MAX_LEVELS] = {};
    int umax[16] = {}; unsigned long long umax_packed = 0;      // umax_packed: 4 bits per entry, the form the descriptor kernels take
    int oct_maxlim = 0;                                         // largest octree list capacity over the levels (quota + 3 or 4*nIni)
    std::vector<SgxRun> runs;                                   // k_fast_cells: one workgroup per run
    std::vector<SgxBlurTile> blur_tiles;                        // k_blur_levels
    std::vector<SgxXTab> xt[SGX_MAX_LEVELS];                    // cv::resize tables of level l from level l - 1 (k_resize, and the source of the fused plan)
    std::vector<SgxYTab> yt_all;                                // the levels' y tables back to back: level l starts at pyr_tabs.yoff[l]
    // fused pyramid (k_pyramid): x coefficients per dword group, per (tile, level) rects, LDS carve; pyr_tiles == 0: per-level k_resize launches instead
    std::vector<SgxXGroup> xgroups; std::vector<SgxPyrRect> rects; SgxPyrTabs pyr_tabs = {}; int pyr_tiles = 0, pyr_lds = 0;
};

static inline int cvround_f(float v) { return (int)lrintf(v); }
static inline int cvround_d(double v) { return (int)lrint(v); }

// ORBextractor::ORBextractor, ORBextractor.cc:411-471 (scale tables, per-level quotas, umax)
static int plan_tables(const sgx_orb_config &c, OrbPlan *p)
{
    const double sf = (double)c.scale_factor;           // member `double scaleFactor` (ORBextractor.h:99) set from a float
    const int nl = c.nlevels;
    p->scale[0] = 1.0f; p->sigma2[0] = 1.0f;
    for (int i = 1; i < nl; i++) { p->scale[i] = (float)((double)p->scale[i - 1] * sf); p->sigma2[i] = p->scale[i] * p->scale[i]; }
    for (int i = 0; i < nl; i++) { p->inv_scale[i] = 1.0f / p->scale[i]; p->inv_sigma2[i] = 1.0f / p->sigma2[i]; }
    const float factor = (float)(1.0f / sf);
    float want = c.nfeatures * (1 - factor) / (1 - (float)pow((double)factor, (double)nl));
    int sum = 0;
    for (int l = 0; l < nl - 1; l++) { p->g.lv[l].quota = cvround_f(want); sum += p->g.lv[l].quota; want *= factor; }
    p->g.lv[nl - 1].quota = c.nfeatures - sum > 0 ? c.nfeatures - sum : 0;
    // umax (:455-470)
    int umax[17] = {0};
    const int HP = 15;
    const int vmax = (int)floor(HP * sqrtf(2.f) / 2 + 1), vmin = (int)ceil(HP * sqrtf(2.f) / 2);
    for (int v = 0; v <= vmax; ++v) umax[v] = cvround_d(sqrt((double)HP * HP - v * v));
    for (int v = HP, v0 = 0; v >= vmin; --v) { while (umax[v0] == umax[v0 + 1]) ++v0; umax[v] = v0; ++v0; }
    for (int i = 0; i < 16; i++) { p->umax[i] = umax[i]; p->umax_packed |= (unsigned long long)(umax[i] & 15) << (4 * i); }
    return SGX_OK;
}

// one FAST cell (ORBextractor.cc:790-808): tile rect in level coords incl. the 3-px aprons; col = j, ox = j*wCell, oy = i*hCell
struct SgxCell { short level, x0, y0, cw, ch, ox, oy, col; };

// Level geometry (ORBextractor.cc:1112-1113), the FAST cell grid of every level (:774-808) and the octree capacities; the cells go to plan_fast_runs
static int plan_levels(const sgx_orb_config &cfg, OrbPlan *p, std::vector<SgxCell> *cells)
{
    SgxOrbGeom &g = p->g;
    int off = 0, cand_off = 0;
    for (int l = 0; l < g.nlevels; l++) {
        SgxLevel &L = g.lv[l];
        L.w = cvround_f((float)cfg.width * p->inv_scale[l]);       // ORBextractor.cc:1112-1113
        L.h = cvround_f((float)cfg.height * p->inv_scale[l]);
        L.stride = (L.w + 63) & ~63;
        L.scale = p->scale[l];
        L.patch_size = (int)(31 * p->scale[l]);                     // :838
        if (l > 0) { L.off = off; off += L.stride * L.h; }
        if (L.w < 2 * SGX_EDGE + 8 || L.h < 2 * SGX_EDGE + 8) return SGX_ERR_UNSUPPORTED;
        // FAST cell grid, ORBextractor.cc:774-808
        const float W = 30;
        const int minBX = SGX_BORDER, minBY = SGX_BORDER, maxBX = L.w - SGX_EDGE + 3, maxBY = L.h - SGX_EDGE + 3;
        const float width = (float)(maxBX - minBX), height = (float)(maxBY - minBY);
        L.ncols = (int)(width / W); L.nrows = (int)(height / W);
        if (L.ncols < 1 || L.nrows < 1) return SGX_ERR_UNSUPPORTED;
        L.wcell = (int)ceilf(width / L.ncols); L.hcell = (int)ceilf(height / L.nrows);
        L.cell0 = (int)cells->size();
        L.cand_off = cand_off; L.cand_cap = 0;
        if (L.wcell + 6 > SGX_TILE_MAX || L.hcell + 6 > SGX_TILE_MAX || L.ncols > 1023 || L.nrows > 1023 || L.wcell > 1023 || L.hcell > 1023) return SGX_ERR_UNSUPPORTED;
        for (int i = 0; i < L.nrows; i++) {
            const float iniY = (float)(minBY + i * L.hcell);
            float maxY = iniY + L.hcell + 6;
            if (iniY >= maxBY - 3) continue;
            if (maxY > maxBY) maxY = (float)maxBY;
            for (int j = 0; j < L.ncols; j++) {
                const float iniX = (float)(minBX + j * L.wcell);
                float maxX = iniX + L.wcell + 6;
                if (iniX >= maxBX - 6) continue;
                if (maxX > maxBX) maxX = (float)maxBX;
                SgxCell c; c.level = (short)l; c.x0 = (short)iniX; c.y0 = (short)iniY;
                c.cw = (short)((int)maxX - (int)iniX); c.ch = (short)((int)maxY - (int)iniY);
                c.ox = (short)(j * L.wcell); c.oy = (short)(i * L.hcell);
                c.col = (short)j;
                if (c.cw >= 7 && c.ch >= 7) {                        // cv::FAST yields nothing on tiles < 7 px
                    cells->push_back(c);
                    L.cand_cap += ((c.cw - 6 + 1) / 2) * ((c.ch - 6 + 1) / 2);   // strict-'>' NMS: no two survivors are 8-adjacent
                }
            }
        }
        const int nIni = (int)roundf((float)(maxBX - minBX) / (float)(maxBY - minBY));
        // a level whose bordered area is more than twice as tall as wide has nIni = 0 root nodes: the reference divides by it and indexes an empty vector
        // (ORBextractor.cc:544-566, undefined behaviour) — refuse such geometries instead of returning a level without keypoints
        if (nIni < 1 || nIni > 64) return SGX_ERR_UNSUPPORTED;
        int lim = L.quota + 3; if (lim < 4 * nIni) lim = 4 * nIni;
        if (lim > SGX_OCT_MAXN) return SGX_ERR_UNSUPPORTED;
        g.kp_cap += lim;
        if (lim > p->oct_maxlim) p->oct_maxlim = lim;
        L.cand_cap = (L.cand_cap + 63) & ~63;
        cand_off += L.cand_cap;
    }
    g.cand_pitch = cand_off;
    g.pyr_pitch = (off + 255) & ~255;
    g.ncells = (int)cells->size();
    return SGX_OK;
}

// k_fast_cells LDS carve of a run of ncell cells, tile rw x ch: bytes of the staged tile (the score map is as large), of the quick-test list (the corner list is as large:
// every interior pixel can pass both tests) and of the output list (strict-'>' NMS inside a cell: no two survivors of a cell are 8-adjacent)
#ifndef SGX_FAST_LDS_BUDGET
#define SGX_FAST_LDS_BUDGET 24576
#endif
struct FastCarve { int tile, q, out; int total() const { return 2 * tile + 2 * q + out; } };
static FastCarve fast_carve(int rw, int ch, int ncell, int wcell)
{
    const int last = rw - 6 - (ncell - 1) * wcell;                     // interior width of the run's last cell
    return { ch * ((15 + rw + 5 + 15) & ~15), ((rw - 6) * (ch - 6) * 2 + 15) & ~15, ((((ncell - 1) * ((wcell + 1) / 2) + (last + 1) / 2) * ((ch - 5) / 2)) * 4 + 15) & ~15 };
}

// k_fast_cells works on runs of adjacent cells of one cell row.  Cells per run: as many as keep the LDS carve of a run within SGX_FAST_LDS_BUDGET (6 workgroups of
// 4 waves per CU: 24 resident waves, the single-cell kernel had 16; at 640x480 that is 3 cells on levels 1-3 and 2 on the others), at most SGX_FAST_MAXG; a row's cells are spread evenly
// over its runs.  Measured per 512 frames by budget (profiles/fast_cell_runs_ab.txt): 0.903 ms at 24 KB, 0.954 at 17 KB, 0.970 at 32 KB, 0.924 at 40 KB (256 threads); 0.961 / 1.082 at 24 KB and 192 / 128 threads.
static int plan_fast_runs(OrbPlan *p, const std::vector<SgxCell> &cells)
{
    SgxOrbGeom &g = p->g;
    FastCarve lds = {0, 0, 0};                                      // the largest of every part over the runs
    for (size_t i = 0; i < cells.size();) {
        const SgxLevel &L = g.lv[cells[i].level];
        size_t e = i + 1;                                           // [i, e): the cells of one cell row (adjacent columns)
        while (e < cells.size() && cells[e].level == cells[i].level && cells[e].y0 == cells[i].y0 && cells[e].col == cells[e - 1].col + 1) e++;
        const int n = (int)(e - i), ch = cells[i].ch;
        int G = 1;
        for (int t = 2; t <= SGX_FAST_MAXG && t <= n; t++) {
            const int rw = t * L.wcell + 6;
            if (rw > SGX_FAST_MAXRW) break;
            if (fast_carve(rw, ch, t, L.wcell).total() > SGX_FAST_LDS_BUDGET) break;
            G = t;
        }
        const int nr = (n + G - 1) / G;
        for (int r = 0, k = 0; r < nr; r++) {
            const int m = n / nr + (r < n % nr ? 1 : 0);
            const SgxCell &a = cells[i + k], &z = cells[i + k + m - 1];
            SgxRun u; memset(&u, 0, sizeof u);
            u.level = a.level; u.x0 = a.x0; u.y0 = a.y0; u.rw = (short)(z.x0 + z.cw - a.x0); u.ch = a.ch; u.ox = a.ox; u.oy = a.oy; u.ncell = (short)m; u.wcell = (short)L.wcell;
            const int lead = u.x0 & 15;
            u.ts = (short)((lead + u.rw + 5 + 15) & ~15);           // room for the dword two groups right of the last quick-test task
            while ((1 << u.sh) < (u.ts >> 4)) u.sh++;
            u.wc_m16 = (unsigned short)((65536 + L.wcell - 1) / L.wcell);
            const FastCarve c = fast_carve(u.rw, u.ch, m, L.wcell);
            lds.tile = std::max(lds.tile, c.tile); lds.q = std::max(lds.q, c.q); lds.out = std::max(lds.out, c.out);
            if (u.rw > SGX_FAST_MAXRW || (u.ts >> 2) > SGX_FAST_MAXGROUPS) return SGX_ERR_UNSUPPORTED;
            p->runs.push_back(u);
            k += m;
        }
        i = e;
    }
    g.fast_off_score = lds.tile; g.fast_off_qlist = 2 * lds.tile; g.fast_off_clist = 2 * lds.tile + lds.q; g.fast_off_out = 2 * lds.tile + 2 * lds.q; g.fast_lds_bytes = lds.total();
    g.nruns = (int)p->runs.size();
    return SGX_OK;
}

// the blurred copy of every level, level 0 included, and its partition into SGX_BT_W x SGX_BT_H tiles in row-major order inside a level (the walk of k_blur_levels)
static int plan_blur_tiles(OrbPlan *p)
{
    SgxOrbGeom &g = p->g;
    int boff = 0;
    for (int l = 0; l < g.nlevels; l++) {
        SgxLevel &L = g.lv[l];
        L.bstride = (L.w + 63) & ~63; L.boff = boff; boff += L.bstride * L.h;
        for (int y0 = 0; y0 < L.h; y0 += SGX_BT_H) for (int x0 = 0; x0 < L.w; x0 += SGX_BT_W) {
            SgxBlurTile t; memset(&t, 0, sizeof t);
            t.level = (short)l; t.x0 = (short)x0; t.y0 = (short)y0; t.w = (short)std::min(SGX_BT_W, L.w - x0); t.h = (short)std::min(SGX_BT_H, L.h - y0);
            p->blur_tiles.push_back(t);
        }
    }
    g.blur_pitch = (boff + 255) & ~255; g.nblur_tiles = (int)p->blur_tiles.size();
    return SGX_OK;
}

// cv::resize coefficient tables (OpenCV 3.4 imgproc/resize.cpp, INTER_LINEAR, 8U fixed point) of every level from the one below it, built once: k_resize reads them
// as they are, plan_pyramid derives the fused kernel's tables from them
static int plan_resize_tables(OrbPlan *p)
{
    const SgxOrbGeom &g = p->g;
    for (int l = 1; l < g.nlevels; l++) {
        const int sw = g.lv[l - 1].w, sh = g.lv[l - 1].h, dw = g.lv[l].w, dh = g.lv[l].h;
        const double scale_x = 1. / ((double)dw / sw), scale_y = 1. / ((double)dh / sh);
        p->pyr_tabs.yoff[l] = (int)p->yt_all.size();
        p->xt[l].resize(dw); p->yt_all.resize(p->yt_all.size() + dh);
        SgxXTab *xt = p->xt[l].data(); SgxYTab *yt = p->yt_all.data() + p->pyr_tabs.yoff[l];
        for (int dx = 0; dx < dw; dx++) {
            float fx = (float)((dx + 0.5) * scale_x - 0.5);
            int sx = (int)floorf(fx);
            fx -= sx;
            if (sx < 0) { fx = 0; sx = 0; }
            if (sx >= sw - 1) { fx = 0; sx = sw - 1; }
            xt[dx].sx = (short)sx; xt[dx].sx1 = (short)(sx + 1 < sw ? sx + 1 : sx);
            xt[dx].a0 = (short)cvround_f((1.f - fx) * 2048); xt[dx].a1 = (short)cvround_f(fx * 2048);
        }
        for (int dy = 0; dy < dh; dy++) {
            float fy = (float)((dy + 0.5) * scale_y - 0.5);
            int sy = (int)floorf(fy);
            fy -= sy;
            int r0 = sy, r1 = sy + 1;
            if (r0 < 0) r0 = 0; if (r0 > sh - 1) r0 = sh - 1;
            if (r1 < 0) r1 = 0; if (r1 > sh - 1) r1 = sh - 1;
            yt[dy].sy0 = (short)r0; yt[dy].sy1 = (short)r1;
            yt[dy].b0 = (short)cvround_f((1.f - fy) * 2048); yt[dy].b1 = (short)cvround_f(fy * 2048);
        }
    }
    return SGX_OK;
}

// the x coefficients per dword group, in the form k_pyramid keeps in registers; false: a group does not find its source bytes within SGX_PYR_SPAN of its first one
static bool pyr_xgroups(OrbPlan *p)
{
    const SgxOrbGeom &g = p->g;
    bool span_ok = true;
    for (int l = 1; l < g.nlevels; l++) {
        p->pyr_tabs.xoff[l] = (int)p->xgroups.size();
        for (int x4 = 0; x4 < g.lv[l].w; x4 += 4) {
            SgxXGroup G; memset(&G, 0, sizeof G);
            G.sx0 = p->xt[l][x4].sx;
            for (int i = 0; i < 4; i++) {
                G.sel[i] = 0x0c0c0c0cu;
                if (x4 + i >= g.lv[l].w) continue;
                const SgxXTab &t = p->xt[l][x4 + i];
                const int o0 = t.sx - G.sx0, o1 = t.sx1 - G.sx0;
                if (o0 < 0 || o1 < 0 || o0 >= SGX_PYR_SPAN || o1 >= SGX_PYR_SPAN || t.a0 < 0 || t.a1 < 0) { span_ok = false; continue; }
                G.sel[i] = (uint32_t)o0 | 0x0c00u | ((uint32_t)o1 << 16) | 0x0c000000u;
                G.a01[i] = (uint32_t)t.a0 | ((uint32_t)t.a1 << 16);
            }
            p->xgroups.push_back(G);
        }
    }
    return span_ok;
}

// k_pyramid plan: tiles are a fixed partition of every level; needed regions are propagated from the coarsest level up.  A geometry too large for the LDS (or a scale
// factor too steep for the groups' span) keeps its tables but gets pyr_tiles = 0: per-level k_resize launches
static int plan_pyramid(OrbPlan *p)
{
    const SgxOrbGeom &g = p->g; const int nl = g.nlevels;
    if (nl < 2) return SGX_OK;
    const bool span_ok = pyr_xgroups(p);
    const int T = 32, ntx = (g.lv[nl - 1].w + T - 1) / T, nty = (g.lv[nl - 1].h + T - 1) / T;
    p->rects.resize((size_t)ntx * nty * nl);
    int max_a = 0, max_b = 0, max_y = 0;
    for (int j = 0; j < nty; j++) for (int i = 0; i < ntx; i++) {
        SgxPyrRect *R = &p->rects[((size_t)j * ntx + i) * nl];
        int nx0 = 0, nx1 = 0, ny0 = 0, ny1 = 0;                 // needed region of level l+1 (exclusive ends)
        for (int l = nl - 1; l >= 0; l--) {
            const int Wl = g.lv[l].w, Hl = g.lv[l].h;
            int ax0 = Wl, ax1 = 0, ay0 = Hl, ay1 = 0;
            if (l >= 1) {                                        // owned part of this level
                ax0 = i == 0 ? 0 : (int)(((long)i * Wl / ntx) & ~3L); ax1 = i == ntx - 1 ? Wl : (int)(((long)(i + 1) * Wl / ntx) & ~3L);
                ay0 = (int)((long)j * Hl / nty); ay1 = j == nty - 1 ? Hl : (int)((long)(j + 1) * Hl / nty);
            }
            SgxPyrRect &r = R[l];
            r.ox0 = (short)ax0; r.ox1 = (short)ax1; r.oy0 = (short)ay0; r.oy1 = (short)ay1;
            if (l < nl - 1) {                                    // sources of the next level's needed region
                const SgxXTab *xt = p->xt[l + 1].data(); const SgxYTab *yt = p->yt_all.data() + p->pyr_tabs.yoff[l + 1];
                for (int x = nx0; x < std::min(nx1, g.lv[l + 1].w); x++) { ax0 = std::min(ax0, (int)xt[x].sx); ax1 = std::max(ax1, (int)xt[x].sx1 + 1); }
                for (int y = ny0; y < ny1; y++) { ay0 = std::min(ay0, (int)yt[y].sy0); ay1 = std::max(ay1, (int)yt[y].sy1 + 1); }
            }
            ax0 &= ~3; ax1 = (ax1 + 3) & ~3;                     // dword groups; groups past the image width are computed as zeros / read inside the row pitch
            r.nx0 = (short)ax0; r.ny0 = (short)ay0; r.nw = (short)(ax1 - ax0); r.nh = (short)(ay1 - ay0);
            const int q = r.nw / 4; r.qmagic = q <= 1 ? 0u : (unsigned)((0x100000000ull + (unsigned)q - 1) / (unsigned)q); r.pad0 = r.pad1 = 0;
            const int bytes = (int)r.nw * r.nh;
            if (l & 1) max_b = std::max(max_b, bytes); else max_a = std::max(max_a, bytes);
            nx0 = ax0; nx1 = ax1; ny0 = ay0; ny1 = ay1;
        }
        int yo = 0;
        for (int l = 1; l < nl; l++) { R[l].yo = yo; yo += R[l].nh; }
        R[0].yo = 0;
        max_y = std::max(max_y, yo);
    }
    p->pyr_tabs.lds_a = (max_a + SGX_PYR_SPAN + 15) & ~15; p->pyr_tabs.lds_b = (max_b + SGX_PYR_SPAN + 15) & ~15;      // + the reach of the last row's 8-byte reads
    p->pyr_lds = p->pyr_tabs.lds_a + p->pyr_tabs.lds_b + max_y * (int)sizeof(SgxYTab);
    p->pyr_tiles = p->pyr_lds > 64 * 1024 || !span_ok ? 0 : ntx * nty;
    return SGX_OK;
}

// cfg has passed the argument checks of sgx_orb_create; *p is a fresh OrbPlan.  SGX_ERR_UNSUPPORTED: a geometry outside the compiled limits, nothing to undo
static int orb_plan(const sgx_orb_config &cfg, OrbPlan *p)
{
    memset(&p->g, 0, sizeof p->g); memset(&p->pyr_tabs, 0, sizeof p->pyr_tabs);
    p->g.nlevels = cfg.nlevels; p->g.W = cfg.width; p->g.H = cfg.height; p->g.ini_th = cfg.ini_th_fast; p->g.min_th = cfg.min_th_fast;
    std::vector<SgxCell> cells;
    int rc;
    if ((rc = plan_tables(cfg, p)) || (rc = plan_levels(cfg, p, &cells)) || (rc = plan_fast_runs(p, cells)) || (rc = plan_blur_tiles(p)) || (rc = plan_resize_tables(p))) return rc;
    return plan_pyramid(p);
}
