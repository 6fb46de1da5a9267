// What the exact reductions share (sph_ledger.hip, sph_wall_load.hip): 128-bit two's-complement sums added per thread, per wave and on
// the host, the 64-bit keys that carry a particle's id, and the rules of include/sph_ledger.h for exponents and the resolved value.
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

#include <cmath>

#include "sph_ledger.h"

struct U128 {
    unsigned long long lo;
    long long hi;
};
__host__ __device__ inline void add128(U128& a, unsigned long long lo, long long hi)
{
    const unsigned long long s = a.lo + lo;
    a.hi += hi + (long long)(s < lo);
    a.lo = s;
}

__device__ __forceinline__ uint32_t ord_f32(float a)
{
    const uint32_t b = __float_as_uint(a);
    return (b & 0x80000000u) ? ~b : (b ^ 0x80000000u);
}
__device__ __forceinline__ void key_max(unsigned long long& w, float a, uint32_t id)
{
    const unsigned long long k = ((unsigned long long)ord_f32(a) << 32) | (unsigned long long)(0xffffffffu - id);
    w = k > w ? k : w;
}
__device__ __forceinline__ void key_min(unsigned long long& w, float a, uint32_t id)
{
    const unsigned long long k = ((unsigned long long)ord_f32(a) << 32) | (unsigned long long)id;
    w = k < w ? k : w;
}
__device__ __forceinline__ bool finite_f32(float a) { return fabsf(a) < INFINITY; }

__device__ __forceinline__ unsigned long long shfl_xor_u64(unsigned long long v, int o)
{
    const uint32_t lo = (uint32_t)__shfl_xor((int)(uint32_t)v, o, 64), hi = (uint32_t)__shfl_xor((int)(uint32_t)(v >> 32), o, 64);
    return ((unsigned long long)hi << 32) | lo;
}
__device__ __forceinline__ U128 wave_add128(U128 v)
{
    for (int o = 32; o > 0; o >>= 1) {
        const unsigned long long lo = shfl_xor_u64(v.lo, o);
        const long long hi = (long long)shfl_xor_u64((unsigned long long)v.hi, o);
        add128(v, lo, hi);
    }
    return v;
}

// e with m < 2^e <= 2 m for m > 0 (frexp: m = f 2^e, 0.5 <= f < 1), 0 for m = 0
inline int exponent_of_bits(uint64_t bits)
{
    const double m = __builtin_bit_cast(double, bits);
    if (!(m > 0.0)) return 0;
    int e = 0;
    (void)std::frexp(m, &e);
    return e;
}

// the value and the id of a maximum key (ord(a) << 32 | 0xffffffff - id); {0, SPH_LEDGER_NO_ID} for the empty key 0
inline sph_ledger_extreme unpack_max_key(uint64_t key)
{
    if (key == 0) return sph_ledger_extreme{0.f, SPH_LEDGER_NO_ID};
    const uint32_t o = (uint32_t)(key >> 32);
    return sph_ledger_extreme{__builtin_bit_cast(float, (o & 0x80000000u) ? (o ^ 0x80000000u) : ~o), 0xffffffffu - (uint32_t)key};
}

// the 128-bit integer -> the nearest f64, ties to even, times 2^shift
inline double resolve128(const sph_ledger_sum& q, int shift)
{
    const bool neg = q.hi < 0;
    unsigned __int128 mag = ((unsigned __int128)(uint64_t)q.hi << 64) | q.lo;
    if (neg) mag = (unsigned __int128)0 - mag;
    if (mag == 0) return 0.0;
    int top = 127;
    while (!((mag >> top) & 1)) top--;
    double v;
    if (top <= 52) v = (double)(uint64_t)mag;
    else {
        const int sh = top - 52;
        uint64_t mant = (uint64_t)(mag >> sh);                                   // 53 bits
        const unsigned __int128 rem = mag & (((unsigned __int128)1 << sh) - 1), half = (unsigned __int128)1 << (sh - 1);
        if (rem > half || (rem == half && (mant & 1u))) mant++;                  // (2^53 after the carry is still exact)
        v = std::ldexp((double)mant, sh);
    }
    v = std::ldexp(v, shift);
    return neg ? -v : v;
}
