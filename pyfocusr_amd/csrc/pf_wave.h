// Device helpers that belong to no one search: the order-preserving integer encoding of a double, the bit spread of the
// 30-bit Morton keys, and the reductions across the 64 lanes of a wave.  Every one is a fixed butterfly: the same order of
// operations on every run, the result in every lane - but for wave_sum_down, the sum of the solve's vector kernels
// (pf_sums.h), whose result is lane 0's alone.
#pragma once
#include "pf_internal.h"

// unsigned integers that compare like the doubles they encode (min / max by 64-bit atomics), and back
__device__ __forceinline__ unsigned long long enc_f64(double d) {
    const unsigned long long u = (unsigned long long)__double_as_longlong(d);
    return (u >> 63) ? ~u : (u | (1ull << 63));
}
__device__ __forceinline__ double dec_f64(unsigned long long u) {
    return __longlong_as_double((long long)((u >> 63) ? (u & ~(1ull << 63)) : ~u));
}

__device__ __forceinline__ unsigned spread10(unsigned v) {  // 10 bits -> every third bit: bit i -> bit 3 i
    v &= 0x3ffu;
    v = (v | (v << 16)) & 0x030000ffu;
    v = (v | (v << 8)) & 0x0300f00fu;
    v = (v | (v << 4)) & 0x030c30c3u;
    v = (v | (v << 2)) & 0x09249249u;
    return v;
}

__device__ __forceinline__ double wave_min(double v) {
    for (int off = PF_WAVE / 2; off > 0; off >>= 1) v = fmin(v, __shfl_xor(v, off, PF_WAVE));
    return v;
}

__device__ __forceinline__ double wave_max(double v) {
    for (int off = PF_WAVE / 2; off > 0; off >>= 1) v = fmax(v, __shfl_xor(v, off, PF_WAVE));
    return v;
}

__device__ __forceinline__ double wave_sum(double v) {
    for (int off = PF_WAVE / 2; off > 0; off >>= 1) v += __shfl_xor(v, off, PF_WAVE);
    return v;
}

// The other sum of a wave, and not interchangeable with wave_sum (other pairings: other bits): lane l adds lane l + off for
// off = 32, 16, 8, 4, 2, 1.  The result is in lane 0 only.
__device__ __forceinline__ double wave_sum_down(double v) {
#pragma unroll
    for (int off = PF_WAVE / 2; off > 0; off >>= 1) v += __shfl_down(v, off, PF_WAVE);
    return v;
}

// the tie rule of every search; a NaN d2 compares false: never wins
__device__ __forceinline__ bool better(double d2, int32_t orig, double bd2, int32_t borig) {
    return d2 < bd2 || (d2 == bd2 && orig < borig);
}

// the least distance of the wave and its index, in every lane; lowest index on ties.  Two overloads with the bodies their
// users were compiled with: 32-bit reference indices (the point searches), 64-bit chunk numbers (the triangle hierarchy).
__device__ __forceinline__ void wave_argmin(double& s, int32_t& o) {
#pragma unroll
    for (int off = PF_WAVE / 2; off > 0; off >>= 1) {
        const double s2 = __shfl_xor(s, off, PF_WAVE);
        const int32_t o2 = __shfl_xor(o, off, PF_WAVE);
        const bool take = s2 < s || (s2 == s && o2 < o);
        s = take ? s2 : s;
        o = take ? o2 : o;
    }
}
__device__ __forceinline__ void wave_argmin(double& d, int64_t& i) {
    for (int off = PF_WAVE / 2; off > 0; off >>= 1) {
        const double od = __shfl_xor(d, off, PF_WAVE);
        const int64_t oi = __shfl_xor(i, off, PF_WAVE);
        if (od < d || (od == d && oi < i)) d = od, i = oi;
    }
}
