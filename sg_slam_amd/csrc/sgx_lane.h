// sgx_lane.h — lane-level integer helpers shared by the kernels: one instruction on the device, a scalar twin with identical semantics in the emulator
#pragma once
#include "sgx_rt.h"

// ((hi:lo) >> 8*sh) as 32 bits (v_alignbyte_b32)
SGX_DEV uint32_t sgx_alignbyte(uint32_t hi, uint32_t lo, int sh)
{
#ifndef SGX_EMU
    return __builtin_amdgcn_alignbyte(hi, lo, (uint32_t)sh);
#else
    return (uint32_t)((((unsigned long long)hi << 32) | lo) >> (8 * sh));
#endif
}

// exact integer dot products of packed operands: 4 x u8 (v_dot4_u32_u8) and 2 x u16 (v_dot2_u32_u16), 32-bit accumulate, no clamp
SGX_DEV uint32_t sgx_udot4(uint32_t a, uint32_t b, uint32_t c)
{
#ifndef SGX_EMU
    return __builtin_amdgcn_udot4(a, b, c, false);
#else
    for (int i = 0; i < 4; i++) c += ((a >> (8 * i)) & 255u) * ((b >> (8 * i)) & 255u);
    return c;
#endif
}
SGX_DEV uint32_t sgx_udot2(uint32_t a, uint32_t b, uint32_t c)
{
#ifndef SGX_EMU
    typedef unsigned short sgx_us2 __attribute__((ext_vector_type(2)));
    return __builtin_amdgcn_udot2(__builtin_bit_cast(sgx_us2, a), __builtin_bit_cast(sgx_us2, b), c, false);
#else
    return c + (a & 0xFFFFu) * (b & 0xFFFFu) + (a >> 16) * (b >> 16);
#endif
}

// byte i of the result = byte sel_i of the eight bytes (hi:lo) (0..3 = lo, 4..7 = hi), sel_i = 0x0c gives 0: v_perm_b32 (only these selector values are used)
SGX_DEV uint32_t sgx_perm(uint32_t hi, uint32_t lo, uint32_t sel)
{
#ifndef SGX_EMU
    return __builtin_amdgcn_perm(hi, lo, sel);
#else
    const unsigned long long v = ((unsigned long long)hi << 32) | lo;
    uint32_t r = 0;
    for (int i = 0; i < 4; i++) { const uint32_t s = (sel >> (8 * i)) & 255u; if (s < 8u) r |= (uint32_t)((v >> (8 * s)) & 255u) << (8 * i); }
    return r;
#endif
}

// a * b for operands below 2^24 whose product fits 32 bits (v_mul_u32_u24: full rate, where the 32-bit multiply takes four passes)
SGX_DEV uint32_t sgx_umul24(uint32_t a, uint32_t b)
{
#ifndef SGX_EMU
    return __umul24(a, b);
#else
    return a * b;
#endif
}
