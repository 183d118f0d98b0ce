// sgx_stereo_kernels.h — HIP kernels of Frame::ComputeStereoMatches (src/sg-slam/src/Frame.cc:716-890) for gfx950, phase style (sgx_rt.h).  A batch of B rectified
// stereo pairs per launch sequence, nothing read back:
//   k_stereo_best    grid (ceil(cap / 32), B)  the row-table search (:725-799): per left keypoint the right keypoint of smallest descriptor distance among those
//                                              whose row interval holds the left row, within one octave and the disparity range; first index wins a tie
//   k_stereo_sad     grid (ceil(cap / 4), B)   the sliding 11 x 11 window at the left keypoint's level (:801-873): 11 SAD values, parabola, disparity, depth
//   k_stereo_median  grid (B)                  the median cut (:876-889): matches with SAD >= 1.5 * 1.4 * median are reset
// Every value the reference holds in a float is formed by the same float operations in the same order (-ffp-contract=off, IEEE division); the SAD values are exact
// integers (<= 121 * 510).  Defined where the reference is not: mb = bf / fx; rows of the row table outside the image are dropped; a window that leaves
// its level gives no match; no accepted match means nothing to cut; a keypoint whose octave is no level of the pyramid takes no part.
#pragma once
#include "sgx_rt.h"
#include "sgx_orb_view.h"

#define SGX_ST_TILE 2048          /* right-keypoint records staged in LDS per pass (12 bytes each) */
#define SGX_ST_KPB 32             /* left keypoints per k_stereo_best workgroup: 4 waves x 8 */
#define SGX_ST_TH_HIGH 100        /* ORBmatcher::TH_HIGH */
#define SGX_ST_TH_ORB 75          /* (TH_HIGH + TH_LOW) / 2 */
#define SGX_ST_W 5                /* window half-size w and search half-range L (:812, :819) */
#define SGX_ST_TAPS 12            /* tap record per left keypoint: bestincR, 11 SAD values */

// which exit of the function a left keypoint took (the tap build reads them back; k_stereo_sad and k_stereo_median read them in every build)
enum {
    SGX_ST_NOT_A_KEY = -1,        // slot >= n_left
    SGX_ST_NO_CANDIDATES = 0,     // :763 (and the defined cases: row outside the image, octave outside the pyramid)
    SGX_ST_LEFT_OF_IMAGE = 1,     // :769 maxU < 0
    SGX_ST_NO_DESCRIPTOR = 2,     // :802 bestDist >= thOrbDist
    SGX_ST_BORDER = 3,            // :825 iniu < 0 || endu >= cols
    SGX_ST_WINDOW_OUTSIDE = 4,    // defined here: a pixel of either window lies outside its level
    SGX_ST_EDGE_OFFSET = 5,       // :844 bestincR == -L || bestincR == L
    SGX_ST_DELTA = 6,             // :854 deltaR outside [-1, 1]
    SGX_ST_DISPARITY = 7,         // :862 disparity outside [minD, maxD) (NaN included)
    SGX_ST_ACCEPTED = 8,
    SGX_ST_ACCEPTED_CLAMPED = 9,  // :864 disparity == 0 -> 0.01
    SGX_ST_CUT = 10,              // accepted, then reset by the median cut (:880-888)
    SGX_ST_PENDING = 11           // between k_stereo_best and k_stereo_sad only
};

struct SgxStereoSide {
    const uint8_t *gray, *pyr;    // level 0 (pitch bytes per row, H rows per frame) and levels 1.. of the extractor's frames
    int pitch, first;             // first: index of the pair's first frame in gray / pyr
    const uint8_t *keys, *desc;   // batch x cap x 28 / x 32
    const int *n;                 // batch
};

struct SgxStereoArgs {
    SgxOrbLevels lv;
    SgxStereoSide L, R;
    int cap;
    float bf, maxD;
    float *uright, *zdepth;       // batch x cap
    int *best, *code, *sad;       // batch x cap workspace: (bestDist << 16) | bestIdxR, exit code, SAD of an accepted match (-1: none)
    int *tap;                     // batch x cap x SGX_ST_TAPS in the tap build, NULL in the product
    int *nmatched;                // batch, or NULL
};

SGX_DEV const uint8_t *sgx_stereo_level(const SgxOrbLevels &lv, const SgxStereoSide &s, int f, int level, int *stride)
{
    if (level == 0) { *stride = s.pitch; return s.gray + (size_t)(s.first + f) * (size_t)s.pitch * (size_t)lv.H; }
    *stride = lv.stride[level];
    return s.pyr + (size_t)(s.first + f) * (size_t)lv.pyr_pitch + (size_t)lv.off[level];
}

SGX_DEV int sgx_stereo_count(const int *n, int f, int cap) { const int v = n[f]; return v < 0 ? 0 : (v > cap ? cap : v); }

// ---------------------------------------------------------------------------------------------
// k_stereo_best (:725-799).  vRowIndices is not materialised: right keypoint iR stands in the list of row yi iff floor(y - r) <= yi <= ceil(y + r), r = 2 * scale[octave]
// (:737-742), so a staged record carries that interval, clipped to 16 bits each (rows < 4000), beside x and the octave.  The left keypoint reads row (size_t)vL (:761).
// One wave walks the records of a pass 64 at a time for each of its 8 left keypoints and fetches a descriptor only for a record that passed the row, octave and range
// tests.  The reference keeps the first candidate in ascending iR whose distance is strictly smaller (:793): the minimum of (dist << 16) | iR, taken per lane and
// then with an LDS atomic minimum — the result does not depend on the order of arrival.
// ---------------------------------------------------------------------------------------------
SGX_KERNEL(256) k_stereo_best(SgxStereoArgs A)
{
    SGX_LDS uint32_t r_rows[SGX_ST_TILE];      // lo | (hi + 1) << 16: the record is a candidate of rows lo <= yi < hi + 1
    SGX_LDS float r_x[SGX_ST_TILE];
    SGX_LDS int r_oct[SGX_ST_TILE];
    SGX_LDS int s_best[SGX_ST_KPB], s_any[SGX_ST_KPB];

    const int f = (int)blockIdx.y, k0 = (int)blockIdx.x * SGX_ST_KPB, cap = A.cap;
    const int nL = sgx_stereo_count(A.L.n, f, cap), nR = sgx_stereo_count(A.R.n, f, cap);
    const uint8_t *lkeys = A.L.keys + (size_t)f * cap * 28, *rkeys = A.R.keys + (size_t)f * cap * 28;
    const uint8_t *ldesc = A.L.desc + (size_t)f * cap * 32, *rdesc = A.R.desc + (size_t)f * cap * 32;
    const int NONE = SGX_ST_TH_HIGH << 16;      // bestDist = TH_HIGH, bestIdxR = 0 (:772-773)

    SGX_THREADS_BEGIN(tid)
    if (tid < SGX_ST_KPB) {
        s_best[tid] = NONE; s_any[tid] = 0;
        const int iL = k0 + tid;
        if (iL < cap) {                          // mvuRight / mvDepth start at -1 (:718-719)
            const size_t o = (size_t)f * cap + iL;
            A.uright[o] = -1.0f; A.zdepth[o] = -1.0f; A.sad[o] = -1;
            if (A.tap) { A.tap[o * SGX_ST_TAPS] = 0; for (int j = 1; j < SGX_ST_TAPS; j++) A.tap[o * SGX_ST_TAPS + j] = -1; }
        }
    }
    SGX_THREADS_END
    SGX_SYNC();

    for (int t0 = 0; t0 < nR; t0 += SGX_ST_TILE) {
        const int tn = min(SGX_ST_TILE, nR - t0);
        SGX_THREADS_BEGIN(tid)
        for (int i = tid; i < tn; i += (int)blockDim.x) {
            const float *kp = (const float *)(rkeys + (size_t)(t0 + i) * 28);
            const float y = kp[1];
            const int oct = ((const int *)kp)[5];
            uint32_t rows = 0;                   // empty interval
            if (oct >= 0 && oct < A.lv.nlevels && y == y) {
                const float r = 2.0f * A.lv.scale[oct];
                const float fl = floorf(y - r), ce = ceilf(y + r);          // minr, maxr (:738-739)
                const uint32_t lo = fl <= 0.0f ? 0u : (fl >= 65535.0f ? 65535u : (uint32_t)(int)fl);
                const uint32_t hi1 = ce < 0.0f ? 0u : (ce >= 65534.0f ? 65535u : (uint32_t)((int)ce + 1));
                rows = lo | (hi1 << 16);
            }
            r_rows[i] = rows; r_x[i] = kp[0]; r_oct[i] = oct;
        }
        SGX_THREADS_END
        SGX_SYNC();
        SGX_THREADS_BEGIN(tid)
        const int w = tid >> 6, lane = tid & 63;
        for (int kk = 0; kk < SGX_ST_KPB / 4; kk++) {
            const int slot = w * (SGX_ST_KPB / 4) + kk, iL = k0 + slot;
            if (iL >= nL) continue;
            const float *kp = (const float *)(lkeys + (size_t)iL * 28);
            const float uL = kp[0], vL = kp[1];
            const int octL = ((const int *)kp)[5];
            if (!(vL > -1.0f && vL < (float)A.lv.H) || octL < 0 || octL >= A.lv.nlevels) continue;      // no row of the table
            const uint32_t yi = (uint32_t)(int)vL;                                                       // (size_t)vL truncates
            const float minU = uL - A.maxD, maxU = uL;                                                   // minD = 0
            const uint32_t *dl = (const uint32_t *)(ldesc + (size_t)iL * 32);
            uint32_t d[8];
#pragma unroll
            for (int j = 0; j < 8; j++) d[j] = dl[j];
            int best = NONE, any = 0;
            for (int i = lane; i < tn; i += 64) {
                const uint32_t rows = r_rows[i];
                if (yi < (rows & 0xFFFFu) || yi >= (rows >> 16)) continue;
                any = 1;
                const int oct = r_oct[i];
                if (oct < octL - 1 || oct > octL + 1) continue;
                const float uR = r_x[i];
                if (!(uR >= minU && uR <= maxU)) continue;
                const uint32_t *dr = (const uint32_t *)(rdesc + (size_t)(t0 + i) * 32);
                int dist = 0;
#pragma unroll
                for (int j = 0; j < 8; j++) dist += __builtin_popcount(d[j] ^ dr[j]);
                if (dist < SGX_ST_TH_HIGH) best = min(best, (dist << 16) | (t0 + i));
            }
            if (best < NONE) sgx_atomic_min_i32(&s_best[slot], best);
            if (any) sgx_atomic_or(&s_any[slot], 1);
        }
        SGX_THREADS_END
        SGX_SYNC();
    }

    SGX_THREADS_BEGIN(tid)
    if (tid < SGX_ST_KPB && k0 + tid < cap) {
        const int iL = k0 + tid;
        const size_t o = (size_t)f * cap + iL;
        int code = SGX_ST_NOT_A_KEY, best = NONE;
        if (iL < nL) {
            const float uL = ((const float *)(lkeys + (size_t)iL * 28))[0];
            if (!s_any[tid]) code = SGX_ST_NO_CANDIDATES;
            else if (uL < 0.0f) code = SGX_ST_LEFT_OF_IMAGE;
            else { best = s_best[tid]; code = (best >> 16) < SGX_ST_TH_ORB ? SGX_ST_PENDING : SGX_ST_NO_DESCRIPTOR; }
        }
        A.best[o] = best; A.code[o] = code;
    }
    SGX_THREADS_END
}

// ---------------------------------------------------------------------------------------------
// k_stereo_sad (:801-873), one wave per left keypoint, four per workgroup.  Lane 0 places the windows: scaled coordinates round half away from zero (:807-809), the
// reference's own border test (:823-826) and then the defined one over every pixel either window reads.  The 11 x 11 left patch and the 11 x 21 right strip are staged
// once; the 121 (row, offset) sums of |(IL - IL(w,w)) - (IR - IR(w,w))| are spread over the lanes as integers (each <= 11 * 510), summed per offset, and lane 0 does the
// float tail in the reference's order.
// ---------------------------------------------------------------------------------------------
SGX_KERNEL(256) k_stereo_sad(SgxStereoArgs A)
{
    SGX_LDS int s_l[4][121], s_r[4][231], s_part[4][121], s_sad[4][11];
    SGX_LDS int s_go[4], s_su[4], s_sv[4], s_sr[4], s_oct[4];
    SGX_LDS float s_srf[4];

    const int f = (int)blockIdx.y, cap = A.cap;
    const int nL = sgx_stereo_count(A.L.n, f, cap);
    const uint8_t *lkeys = A.L.keys + (size_t)f * cap * 28, *rkeys = A.R.keys + (size_t)f * cap * 28;

    SGX_THREADS_BEGIN(tid)
    const int w = tid >> 6, lane = tid & 63, iL = (int)blockIdx.x * 4 + w;
    if (lane == 0) {
        int go = 0;
        const size_t o = (size_t)f * cap + (size_t)iL;
        if (iL < nL && A.code[o] == SGX_ST_PENDING) {
            const float *kl = (const float *)(lkeys + (size_t)iL * 28);
            const int oct = ((const int *)kl)[5];
            const int iR = A.best[o] & 0xFFFF;
            const float uR0 = ((const float *)(rkeys + (size_t)iR * 28))[0];
            const float sf = A.lv.inv_scale[oct];
            const float su = roundf(kl[0] * sf), sv = roundf(kl[1] * sf), sr = roundf(uR0 * sf);
            const float iniu = sr + (float)SGX_ST_W - (float)SGX_ST_W, endu = sr + (float)SGX_ST_W + (float)SGX_ST_W + 1.0f;
            const float cols = (float)A.lv.w[oct], rows = (float)A.lv.h[oct];
            if (iniu < 0.0f || endu >= cols) A.code[o] = SGX_ST_BORDER;
            else if (!(su >= 5.0f && su <= cols - 6.0f && sv >= 5.0f && sv <= rows - 6.0f && sr >= 10.0f && sr <= cols - 11.0f)) A.code[o] = SGX_ST_WINDOW_OUTSIDE;
            else { go = 1; s_su[w] = (int)su; s_sv[w] = (int)sv; s_sr[w] = (int)sr; s_srf[w] = sr; s_oct[w] = oct; }
        }
        s_go[w] = go;
    }
    SGX_THREADS_END
    SGX_SYNC();
    if (!(s_go[0] | s_go[1] | s_go[2] | s_go[3])) return;

    SGX_THREADS_BEGIN(tid)
    const int w = tid >> 6, lane = tid & 63;
    if (s_go[w]) {
        int sl, sr;
        const uint8_t *il = sgx_stereo_level(A.lv, A.L, f, s_oct[w], &sl), *ir = sgx_stereo_level(A.lv, A.R, f, s_oct[w], &sr);
        const int y0 = s_sv[w] - SGX_ST_W, xl = s_su[w] - SGX_ST_W, xr = s_sr[w] - 2 * SGX_ST_W;
        for (int p = lane; p < 121 + 231; p += 64) {
            if (p < 121) { const int r = p / 11, c = p - 11 * r; s_l[w][p] = (int)il[(size_t)(y0 + r) * sl + (xl + c)]; }
            else { const int q = p - 121, r = q / 21, c = q - 21 * r; s_r[w][q] = (int)ir[(size_t)(y0 + r) * sr + (xr + c)]; }
        }
    }
    SGX_THREADS_END
    SGX_SYNC();
    SGX_THREADS_BEGIN(tid)
    const int w = tid >> 6, lane = tid & 63;
    if (s_go[w]) {
        const int cl = s_l[w][5 * 11 + 5];
        for (int p = lane; p < 121; p += 64) {
            const int r = p / 11, off = p - 11 * r;          // off = incR + L
            const int cr = s_r[w][5 * 21 + off + 5];
            int sum = 0;
#pragma unroll
            for (int c = 0; c < 11; c++) { const int v = (s_l[w][r * 11 + c] - cl) - (s_r[w][r * 21 + off + c] - cr); sum += v < 0 ? -v : v; }
            s_part[w][p] = sum;
        }
    }
    SGX_THREADS_END
    SGX_SYNC();
    SGX_THREADS_BEGIN(tid)
    const int w = tid >> 6, lane = tid & 63;
    if (s_go[w] && lane < 11) {
        int sum = 0;
        for (int r = 0; r < 11; r++) sum += s_part[w][r * 11 + lane];
        s_sad[w][lane] = sum;
    }
    SGX_THREADS_END
    SGX_SYNC();
    SGX_THREADS_BEGIN(tid)
    const int w = tid >> 6, lane = tid & 63, iL = (int)blockIdx.x * 4 + w;
    if (s_go[w] && lane == 0) {
        const size_t o = (size_t)f * cap + (size_t)iL;
        int bestDist = 0x7FFFFFFF, bestinc = 0;
        for (int j = 0; j < 11; j++) if (s_sad[w][j] < bestDist) { bestDist = s_sad[w][j]; bestinc = j - SGX_ST_W; }      // strict: the first minimum (:835)
        if (A.tap) { A.tap[o * SGX_ST_TAPS] = bestinc; for (int j = 0; j < 11; j++) A.tap[o * SGX_ST_TAPS + 1 + j] = s_sad[w][j]; }
        int code;
        if (bestinc == -SGX_ST_W || bestinc == SGX_ST_W) code = SGX_ST_EDGE_OFFSET;
        else {
            const float d1 = (float)s_sad[w][SGX_ST_W + bestinc - 1], d2 = (float)s_sad[w][SGX_ST_W + bestinc], d3 = (float)s_sad[w][SGX_ST_W + bestinc + 1];
            const float deltaR = (d1 - d3) / (2.0f * (d1 + d3 - 2.0f * d2));
            if (deltaR < -1.0f || deltaR > 1.0f) code = SGX_ST_DELTA;          // NaN passes, as in the reference
            else {
                const float uL = ((const float *)(lkeys + (size_t)iL * 28))[0];
                float bestuR = A.lv.scale[s_oct[w]] * (s_srf[w] + (float)bestinc + deltaR);
                float disparity = uL - bestuR;
                if (disparity >= 0.0f && disparity < A.maxD) {
                    code = SGX_ST_ACCEPTED;
                    if (disparity <= 0.0f) { disparity = 0.01f; bestuR = (float)((double)uL - 0.01); code = SGX_ST_ACCEPTED_CLAMPED; }
                    A.zdepth[o] = A.bf / disparity; A.uright[o] = bestuR; A.sad[o] = bestDist;
                } else code = SGX_ST_DISPARITY;
            }
        }
        A.code[o] = code;
    }
    SGX_THREADS_END
}

// ---------------------------------------------------------------------------------------------
// k_stereo_median (:876-889), one workgroup per frame.  The reference sorts (SAD, iL) and takes the SAD of element size / 2; the k-th smallest of values below 2^16 is
// found by counting: a histogram of the high bytes, then of the low bytes inside the bin that holds rank k.  Counts are integer sums, so the order in which the atomic
// adds arrive does not matter.  thDist = 1.5f * 1.4f * median; every match with (float)SAD >= thDist is reset (the reference walks the sorted list from its end to
// the first smaller one: the same set).  No accepted match: nothing to cut (the reference indexes an empty vector).
// ---------------------------------------------------------------------------------------------
SGX_KERNEL(256) k_stereo_median(SgxStereoArgs A)
{
    SGX_LDS int h_hi[256], h_lo[256];
    SGX_LDS int s_n, s_bin, s_rank, s_med, s_kept;
    const int f = (int)blockIdx.x, cap = A.cap, NT = (int)blockDim.x;
    const int nL = sgx_stereo_count(A.L.n, f, cap);
    const size_t o = (size_t)f * cap;

    SGX_THREADS_BEGIN(tid)
    for (int i = tid; i < 256; i += NT) { h_hi[i] = 0; h_lo[i] = 0; }
    if (tid == 0) s_kept = 0;
    SGX_THREADS_END
    SGX_SYNC();
    SGX_THREADS_BEGIN(tid)
    for (int i = tid; i < nL; i += NT) { const int s = A.sad[o + i]; if (s >= 0) sgx_atomic_add(&h_hi[(s >> 8) & 255], 1); }
    SGX_THREADS_END
    SGX_SYNC();
    SGX_THREADS_BEGIN(tid)
    if (tid == 0) {
        int n = 0;
        for (int b = 0; b < 256; b++) n += h_hi[b];
        s_n = n; s_bin = 0; s_rank = 0;
        if (n > 0) {
            int k = n / 2, b = 0;                    // vDistIdx[vDistIdx.size() / 2]
            while (k >= h_hi[b]) { k -= h_hi[b]; b++; }
            s_bin = b; s_rank = k;
        }
    }
    SGX_THREADS_END
    SGX_SYNC();
    if (s_n == 0) {
        SGX_THREADS_BEGIN(tid)
        if (tid == 0 && A.nmatched) A.nmatched[f] = 0;
        SGX_THREADS_END
        return;
    }
    SGX_THREADS_BEGIN(tid)
    for (int i = tid; i < nL; i += NT) { const int s = A.sad[o + i]; if (s >= 0 && ((s >> 8) & 255) == s_bin) sgx_atomic_add(&h_lo[s & 255], 1); }
    SGX_THREADS_END
    SGX_SYNC();
    SGX_THREADS_BEGIN(tid)
    if (tid == 0) {
        int k = s_rank, b = 0;
        while (k >= h_lo[b]) { k -= h_lo[b]; b++; }
        s_med = (s_bin << 8) | b;
    }
    SGX_THREADS_END
    SGX_SYNC();
    SGX_THREADS_BEGIN(tid)
    const float median = (float)s_med;
    const float thDist = 1.5f * 1.4f * median;
    int kept = 0;
    for (int i = tid; i < nL; i += NT) {
        const int s = A.sad[o + i];
        if (s < 0) continue;
        if ((float)s >= thDist) { A.uright[o + i] = -1.0f; A.zdepth[o + i] = -1.0f; A.code[o + i] = SGX_ST_CUT; }
        else kept++;
    }
    if (kept) sgx_atomic_add(&s_kept, kept);
    SGX_THREADS_END
    SGX_SYNC();
    SGX_THREADS_BEGIN(tid)
    if (tid == 0 && A.nmatched) A.nmatched[f] = s_kept;
    SGX_THREADS_END
}
