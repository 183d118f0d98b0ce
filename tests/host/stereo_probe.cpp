// stereo_probe.cpp — stand-alone host program: sgx_stereo_match_batch_dev over key sets that do not come from an extractor — coordinates off the image, on its borders,
// NaN and infinities, octaves that are no level of the pyramid — and over empty frames, on real pyramids of the emulator's extractor.  tests/test_stereo_probe.py builds
// this file and the emulator units with AddressSanitizer / UBSan.  Every buffer is a heap allocation of exactly the size the entry is documented to use and the
// emulator's device memory is the heap too, so a window, a row-table index, a key or a tap record read or written outside its array ends the program.  Every left
// keypoint and its right twin share one descriptor, so the search reaches the window stage wherever the reference would.
#include "../../include/sgx.h"
#include "../../include/sgx_debug.h"
#include <limits.h>
#include <math.h>
#include <stdio.h>
#include <string.h>
#include <vector>

static const int W = 320, H = 240, B = 2;
static int g_matches = 0;

static std::vector<sgx_keypoint> grid_keys(const int *octaves, int noct)
{
    const float inf = INFINITY, nan = NAN;
    const float xs[] = { -1e9f, -11.f, -1.f, 0.f, 4.f, 5.f, 9.f, 10.f, W - 11.f, W - 10.f, W - 6.f, W - 5.f, W - 1.f, (float)W, W + 9.f, 1e9f, nan, inf };
    const float ys[] = { -1e9f, -3.f, -1.f, -0.5f, 0.f, 4.f, 5.f, H - 6.f, H - 5.f, H - 1.f, H - 0.5f, (float)H, H + 2.f, 1e9f, nan, inf, -inf };
    std::vector<sgx_keypoint> k;
    for (int o = 0; o < noct; o++) for (float y : ys) for (float x : xs) {
        sgx_keypoint p; memset(&p, 0, sizeof p);
        p.x = x; p.y = y; p.size = 31.f; p.octave = octaves[o];
        k.push_back(p);
    }
    return k;
}

// one call over B pairs; side = per-pair key sets (left, right); checks the outputs' shape
static int run(sgx_stereo *st, sgx_orb *orb, const uint8_t *gray, int pitch, int cap, const std::vector<sgx_keypoint> (&left)[B], const std::vector<sgx_keypoint> (&right)[B], const char *what)
{
    std::vector<sgx_keypoint> kl((size_t)B * cap), kr((size_t)B * cap);
    std::vector<uint8_t> dl((size_t)B * cap * 32, 0x5a), dr((size_t)B * cap * 32, 0x5a);
    std::vector<int32_t> nl(B), nr(B), nm(B, -7);
    std::vector<float> ur((size_t)B * cap, 7.f), z((size_t)B * cap, 7.f);
    memset(kl.data(), 0, kl.size() * sizeof(sgx_keypoint)); memset(kr.data(), 0, kr.size() * sizeof(sgx_keypoint));
    for (size_t i = 0; i < dl.size(); i++) { const unsigned slot = (unsigned)((i / 32) % (size_t)cap); dl[i] = dr[i] = (uint8_t)((slot * 2654435761u + (unsigned)(i % 32) * 40503u) >> 13); }      // key i and its twin share descriptor i
    for (int f = 0; f < B; f++) {
        if ((int)left[f].size() > cap || (int)right[f].size() > cap) { fprintf(stderr, "%s: key set larger than the capacity %d\n", what, cap); return 1; }
        nl[f] = (int)left[f].size(); nr[f] = (int)right[f].size();
        if (nl[f]) memcpy(&kl[(size_t)f * cap], left[f].data(), left[f].size() * sizeof(sgx_keypoint));
        if (nr[f]) memcpy(&kr[(size_t)f * cap], right[f].data(), right[f].size() * sizeof(sgx_keypoint));
    }
    const int rc = sgx_stereo_match_batch_dev(st, B, orb, 0, gray, pitch, orb, B, gray, pitch, cap, kl.data(), dl.data(), nl.data(), kr.data(), dr.data(), nr.data(),
                                              260.f, 26.f, ur.data(), z.data(), nm.data(), NULL);
    if (rc != SGX_OK) { fprintf(stderr, "%s: status %d\n", what, rc); return 1; }
    int bad = 0;
    std::vector<int32_t> code(cap), inc(cap), sads((size_t)cap * 11), bi(cap), bd(cap);
    for (int f = 0; f < B; f++) {
        if (sgx_stereo_debug_read(st, f, bi.data(), bd.data(), code.data(), inc.data(), sads.data()) != SGX_OK) { fprintf(stderr, "%s: tap read failed\n", what); return 1; }
        int kept = 0;
        for (int i = 0; i < cap; i++) {
            const float u = ur[(size_t)f * cap + i], d = z[(size_t)f * cap + i];
            const bool none = u == -1.f && d == -1.f, match = d > 0.f && u == u;
            if (!(none || match) || (i >= nl[f] && (!none || code[i] != -1)) || (i < nl[f] && (code[i] < 0 || code[i] > 10)) || (match != (code[i] == 8 || code[i] == 9)))
                { fprintf(stderr, "%s: pair %d key %d: uright %g depth %g exit %d\n", what, f, i, u, d, code[i]); bad++; }
            // a key whose windows would leave the level never matches: the defined case
            if (i < nl[f] && match) {
                const sgx_keypoint &p = left[f][i];
                if (!(p.x >= 5.f && p.x <= W - 6.f && p.y >= 5.f && p.y <= H - 6.f) && p.octave == 0) { fprintf(stderr, "%s: pair %d key %d matched from outside the image\n", what, f, i); bad++; }
            }
            kept += match;
        }
        g_matches += kept;
        if (kept != nm[f]) { fprintf(stderr, "%s: pair %d: %d matches, nmatched %d\n", what, f, kept, nm[f]); bad++; }
    }
    return bad;
}

int main()
{
    sgx_orb_config cfg = {1000, 1.2f, 8, 20, 7, W, H, 2 * B};
    sgx_orb *orb = NULL; sgx_stereo *st = NULL;
    if (sgx_orb_create(&cfg, &orb) != SGX_OK || sgx_stereo_create(orb, B, &st) != SGX_OK) { fprintf(stderr, "create failed\n"); return 1; }
    const int cap = sgx_orb_keypoint_capacity(orb), pitch = W;
    // 2B frames of smoothed noise, the right ones the left ones three columns on (values <= 254 before the offset below); exactly 2B * H * pitch bytes
    std::vector<uint8_t> gray((size_t)2 * B * H * pitch);
    {
        std::vector<int> t((size_t)H * (W + 8));
        unsigned s = 12345u;
        for (int &v : t) { s = s * 1664525u + 1013904223u; v = (int)(s >> 24); }
        for (int f = 0; f < 2 * B; f++) for (int y = 0; y < H; y++) for (int x = 0; x < W; x++) {
            const int xo = x + (f >= B ? 3 : 0), y0 = y > 0 ? y - 1 : y, y1 = y < H - 1 ? y + 1 : y;
            int a = 0;
            for (int yy : { y0, y, y1 }) for (int dx = 0; dx < 3; dx++) a += t[(size_t)yy * (W + 8) + xo + dx];
            // an exact shift would give every match the SAD 0, a median of 0 and a cut that takes them all: every fifth pixel of the right frames is one level up
            gray[((size_t)f * H + y) * pitch + x] = (uint8_t)(a / 9 + (f >= B && (x * 7 + y * 13) % 5 == 0 ? 1 : 0));
        }
    }
    std::vector<sgx_keypoint> k((size_t)2 * B * cap); std::vector<uint8_t> d((size_t)2 * B * cap * 32); std::vector<int32_t> n(2 * B);
    if (sgx_orb_extract_batch_dev(orb, gray.data(), pitch, 2 * B, k.data(), d.data(), n.data(), cap, NULL) != SGX_OK) { fprintf(stderr, "extraction failed\n"); return 1; }
    const int o07[] = { 0, 7 }, o3[] = { 3 }, obad[] = { -1, 8 }, omax[] = { INT_MAX, INT_MIN };
    const std::vector<sgx_keypoint> g07 = grid_keys(o07, 2), g3 = grid_keys(o3, 1), gbad = grid_keys(obad, 2), gmax = grid_keys(omax, 2), none;
    std::vector<sgx_keypoint> inside;          // ordinary keys: the run must also find matches, or the checks above see nothing
    for (int y = 30; y < H - 30; y += 12) for (int x = 40; x < W - 30; x += 28) { sgx_keypoint p; memset(&p, 0, sizeof p); p.x = (float)x; p.y = (float)y; p.size = 31.f; inside.push_back(p); }
    std::vector<sgx_keypoint> inside_r = inside; for (sgx_keypoint &p : inside_r) p.x -= 3.f;
    int bad = 0;
    { const std::vector<sgx_keypoint> l[B] = { g07, none }, r[B] = { g07, g07 }; bad += run(st, orb, gray.data(), pitch, cap, l, r, "grid keys / no left keys"); }
    { const std::vector<sgx_keypoint> l[B] = { g3, gbad }, r[B] = { none, gbad }; bad += run(st, orb, gray.data(), pitch, cap, l, r, "no right keys / octaves outside the pyramid"); }
    { const std::vector<sgx_keypoint> l[B] = { inside, g3 }, r[B] = { inside_r, g07 }; bad += run(st, orb, gray.data(), pitch, cap, l, r, "ordinary keys / grids of different octaves"); }
    { const std::vector<sgx_keypoint> l[B] = { gmax, g07 }, r[B] = { gmax, gbad }; bad += run(st, orb, gray.data(), pitch, cap, l, r, "octaves at the ends of int / right octaves outside"); }
    { const std::vector<sgx_keypoint> l[B] = { none, none }, r[B] = { none, none }; bad += run(st, orb, gray.data(), pitch, cap, l, r, "nothing at all"); }
    sgx_stereo_destroy(st); sgx_orb_destroy(orb);
    if (g_matches < 20) { fprintf(stderr, "only %d matches over all runs: the window stage was hardly reached\n", g_matches); bad++; }
    if (!bad) printf("stereo_probe: ok, %d matches\n", g_matches);
    return bad ? 1 : 0;
}
