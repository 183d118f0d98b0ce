// sgx_grand.h — the glibc rand() replica of the RANSAC solvers (PnPsolver, Initializer, Sim3Solver draw from the process-global rand()): random_r TYPE_3,
// r[i] = r[i - 3] + r[i - 31].  srand(seed) on the host; the draws on the device, or on the host where the solver's loop is host code.
#pragma once
#include "sgx_rt.h"

#define SGX_GRAND_WORDS 36           /* ints per replica: r[31], f, b, pad */

#ifdef SGX_EMU
#define SGX_GRAND_FN SGX_DEV
#else
#define SGX_GRAND_FN __host__ SGX_DEV
#endif

static inline void sgx_gsrand(unsigned seed, int32_t *g)
{
    int32_t word = seed ? (int32_t)seed : 1; g[0] = word;
    for (int i = 1; i < 31; i++) { const long hi = word / 127773, lo = word % 127773; long w = 16807 * lo - 2836 * hi; if (w < 0) w += 2147483647; word = (int32_t)w; g[i] = word; }
    int f = 3, b = 0;
    for (int i = 0; i < 310; i++) { g[f] = (int32_t)((uint32_t)g[f] + (uint32_t)g[b]); f = (f + 1) % 31; b = (b + 1) % 31; }
    g[31] = f; g[32] = b; g[33] = 0; g[34] = 0; g[35] = 0;
}

SGX_GRAND_FN int32_t sgx_grand(int32_t *g)
{
    int f = g[31], b = g[32];
    g[f] = (int32_t)((uint32_t)g[f] + (uint32_t)g[b]);
    const int32_t o = (int32_t)(((uint32_t)g[f]) >> 1);
    g[31] = (f + 1) % 31; g[32] = (b + 1) % 31;
    return o;
}
