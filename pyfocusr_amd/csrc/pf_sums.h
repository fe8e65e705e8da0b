// The fixed-order sums of the solve's vector kernels (pf_reduce.hip, pf_orth.hip), each stated once.  A reduction over a
// workspace vector is always
//   1. a block's sum over a chunk of PF_DOT_CHUNK rows, every thread adding its products in row order (chunk_dot,
//      chunk_dot_regs, chunk_resid2),
//   2. the sum of the block (block_sum_put, a barrier, block_sum_get), and
//   3. one wave's sum of the per-chunk partials of a column (column_sum),
// so two kernels that call the same helpers give the same bits.  axpy_sub is the one subtraction of every projection.
#pragma once
#include "pf_wave.h"

// pairs of rows per thread in a whole chunk
constexpr int PF_CHUNK_PAIRS = PF_DOT_CHUNK / (2 * PF_BLOCK);

// Sum of a block of PF_BLOCK threads, in two halves around the caller's __syncthreads(): every wave's wave_sum_down goes
// into red[wave]; then (red[0] + red[1]) + (red[2] + red[3]).
__device__ __forceinline__ void block_sum_put(double s, double* red) {
    s = wave_sum_down(s);
    if ((threadIdx.x & (PF_WAVE - 1)) == 0) red[threadIdx.x / PF_WAVE] = s;
}
__device__ __forceinline__ double block_sum_get(const double* red) {
    static_assert(PF_BLOCK / PF_WAVE == 4, "the combine is written for four waves");
    return (red[0] + red[1]) + (red[2] + red[3]);
}

// This thread's share of <v, w> over rows [chunk PF_DOT_CHUNK, the chunk's end or n_pad): its pairs of rows 2 threadIdx.x,
// + 2 PF_BLOCK, ... in ascending order, of each pair the x product and then the y product.
__device__ __forceinline__ double chunk_dot(const double* v, const double* w, int64_t chunk, int64_t n_pad) {
    const int64_t lo = chunk * PF_DOT_CHUNK;
    const int64_t hi = lo + PF_DOT_CHUNK < n_pad ? lo + PF_DOT_CHUNK : n_pad;
    double s = 0.0;
    for (int64_t i = lo + 2 * threadIdx.x; i < hi; i += 2 * PF_BLOCK) {
        const double2 a = *reinterpret_cast<const double2*>(v + i);
        const double2 c = *reinterpret_cast<const double2*>(w + i);
        s += a.x * c.x;
        s += a.y * c.y;
    }
    return s;
}

// The same share of a WHOLE chunk (n_pad is a multiple of the chunk) from registers: chunk_load issues the thread's
// PF_CHUNK_PAIRS loads - a caller issues all of them, of every vector, before the first product waits for one -
// and chunk_dot_regs adds the products in chunk_dot's order.
__device__ __forceinline__ void chunk_load(double2 (&x)[PF_CHUNK_PAIRS], const double* v, int64_t chunk) {
#pragma unroll
    for (int it = 0; it < PF_CHUNK_PAIRS; ++it)
        x[it] = *reinterpret_cast<const double2*>(v + chunk * PF_DOT_CHUNK + 2 * threadIdx.x + (int64_t)it * (2 * PF_BLOCK));
}
__device__ __forceinline__ double chunk_dot_regs(const double2 (&x)[PF_CHUNK_PAIRS], const double2 (&c)[PF_CHUNK_PAIRS]) {
    double s = 0.0;
#pragma unroll
    for (int it = 0; it < PF_CHUNK_PAIRS; ++it) {
        s += x[it].x * c[it].x;
        s += x[it].y * c[it].y;
    }
    return s;
}

// This thread's share of |ax - lam x|^2 over the chunk: rows threadIdx.x, + PF_BLOCK, ... in ascending order.
__device__ __forceinline__ double chunk_resid2(const double* ax, const double* x, double lam, int64_t chunk, int64_t n_pad) {
    const int64_t lo = chunk * PF_DOT_CHUNK;
    const int64_t hi = lo + PF_DOT_CHUNK < n_pad ? lo + PF_DOT_CHUNK : n_pad;
    double s = 0.0;
    for (int64_t i = lo + threadIdx.x; i < hi; i += PF_BLOCK) {
        const double r = ax[i] - lam * x[i];
        s += r * r;
    }
    return s;
}

// Sum of column b of partial[..][n_chunks] by ONE wave: lane l adds the column's entries l, l + 64, ... in ascending order,
// then wave_sum_down.  The result is in lane 0 only.
__device__ __forceinline__ double column_sum(const double* partial, int b, int64_t n_chunks, int lane) {
    double s = 0.0;
    for (int64_t k = lane; k < n_chunks; k += PF_WAVE) s += partial[(int64_t)b * n_chunks + k];
    return wave_sum_down(s);
}
// hs[b] = column_sum of column b of partial[count][n_chunks], the columns dealt out to the waves of the block (the
// caller's __syncthreads() follows)
__device__ __forceinline__ void column_sums(const double* partial, int64_t n_chunks, int count, double* hs) {
    const int lane = threadIdx.x & (PF_WAVE - 1);
    for (int b = threadIdx.x / PF_WAVE; b < count; b += PF_BLOCK / PF_WAVE) {
        const double s = column_sum(partial, b, n_chunks, lane);
        if (lane == 0) hs[b] = s;
    }
}

// acc -= h v for a pair of rows: x, then y.  A projection applies it for b = 0, 1, ... in ascending order.
__device__ __forceinline__ void axpy_sub(double2& acc, double h, double2 v) {
    acc.x -= h * v.x;
    acc.y -= h * v.y;
}
// rows i, i + 1 of slot wslot -= sum_b h[b] (rows i, i + 1 of slot first + b), b = 0 .. count - 1 in ascending order
__device__ __forceinline__ void axpy_rows(double* ws, int64_t n_pad, int32_t first, int32_t count, int32_t wslot, const double* h, int64_t i) {
    double2 acc = *reinterpret_cast<double2*>(ws + (int64_t)wslot * n_pad + i);
    for (int b = 0; b < count; ++b) axpy_sub(acc, h[b], *reinterpret_cast<const double2*>(ws + (int64_t)(first + b) * n_pad + i));
    *reinterpret_cast<double2*>(ws + (int64_t)wslot * n_pad + i) = acc;
}
