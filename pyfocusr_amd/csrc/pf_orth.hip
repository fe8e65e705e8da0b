// The Gram-Schmidt step of the Krylov-Schur driver, in two halves (pf_orth_begin / pf_orth_end): w is projected against a
// basis of workspace slots, and the coefficients, the norm of what is left and a verdict on a second pass land in a
// pinned block of the graph's own, behind a ticket the host polls for.  Three shapes: two fused launches (k_orth_dots +
// k_orth_project, one graph or both graphs of a pair), the whole local step of Lanczos with partial
// reorthogonalisation in one launch with a grid-wide wait (k_orth_local), and - bases of PF_ORTH_MAX vectors and more -
// the plain dot products (pf_reduce.hip) and k_multi_axpy twice.
// The shapes give the same bits because they call the same statements of each rule: the sums of pf_sums.h (chunk, block,
// column; axpy_sub / axpy_rows in ascending order of b) and, here, orth_slot / orth_vec (where basis vector b lives),
// orth_verdict (Pythagoras, the threshold, the second pass's verdict) and orth_report (block 0's report, the ticket
// last).  On the host orth_fused queues the fused step for one graph or two and orth_coef names the regions of g->coef.
#include <math.h>
#include <stdlib.h>

#include <algorithm>
#include <atomic>
#include <map>
#include <mutex>

#include "pf_internal.h"
#include "pf_sums.h"

namespace {

// w -= sum_b h[b] V_b
__global__ __launch_bounds__(PF_BLOCK) void k_multi_axpy(double* __restrict__ ws, int64_t n_pad, int32_t first,
                                                         int32_t count, int32_t wslot, const double* __restrict__ h) {
    const int64_t i = 2 * ((int64_t)blockIdx.x * PF_BLOCK + threadIdx.x);
    if (i < n_pad) axpy_rows(ws, n_pad, first, count, wslot, h, i);
}

// Fused forms for pf_orth_begin (one Gram-Schmidt pass = k_dot_partial + one of these; no separate finish launch):
// every block finishes the per-chunk partial sums itself - column_sum, as k_dot_finish does, so all blocks (and the
// host) see the same bits - then subtracts.  Block 0 also publishes the coefficients.
constexpr int PF_ORTH_MAX = 256;
// k_axpy_finishing: a plain pass, hsum[b] (+)= h[b] (the second pass of the rare case below).
__global__ __launch_bounds__(PF_BLOCK) void k_axpy_finishing(double* __restrict__ ws, int64_t n_pad, int32_t first, int32_t count,
                                                             int32_t wslot, const double* __restrict__ partial, int64_t n_chunks,
                                                             double* __restrict__ hsum, int accumulate) {
    __shared__ double hs[PF_ORTH_MAX];
    column_sums(partial, n_chunks, count, hs);
    __syncthreads();
    if (blockIdx.x == 0)
        for (int b = threadIdx.x; b < count; b += PF_BLOCK) hsum[b] = accumulate ? hsum[b] + hs[b] : hs[b];
    const int64_t i = 2 * ((int64_t)blockIdx.x * PF_BLOCK + threadIdx.x);
    if (i < n_pad) axpy_rows(ws, n_pad, first, count, wslot, hs, i);
}
// The orthogonalisation step of one graph - or of the two graphs of a pair in the same two launches (blockIdx.z) - is
// k_orth_dots + k_orth_project:
//   h = V^T w and |w|^2 (partial sums per chunk);   w' = w - V h;   |w'|^2 = |w|^2 - sum h^2  (Pythagoras);
//   w' /= |w'| if `normalize`
// and h, |w'|^2 and a verdict go straight to the host's pinned buffer: host_out = [h (count), |w'|^2, redo].
// If |w'| < 0.3 |w| (0.71 |w| in strict mode, pf_orth_strict) the projection cancelled digits - the second Gram-Schmidt
// pass is due ("twice is enough", Daniel, Gragg, Kaufman, Stewart; ARPACK's criterion, by default with a looser constant) and Pythagoras is no longer a fair norm: redo = 1,
// w' stays un-normalised and pf_orth_end runs the second pass itself.  Otherwise the basis stays orthogonal to ~eps / 0.3
// and |w'| carries a relative error <= ~eps / 0.09: far inside what Lanczos needs (semi-orthogonality sqrt(eps) already
// preserves the Ritz values; the eigenvalues handed out come from a Rayleigh-Ritz step on the operator itself).
// Measured on the 250k blobs: the ratio is 0.35-0.78 in all steps but one or two per solve, and a step costs 2 launches
// where it took 6 (the two gated passes and the separate norm were ~4.4 us of launch floor each).
struct OrthArgs {
    double* ws;
    int64_t n_pad, n_chunks;
    int32_t first, count, wslot, normalize;
    // basis vector b < count lives in slot first + b for b < split and in slot first2 + (b - split) from there on: one range
    // (split = count), or - the local steps of Lanczos with partial reorthogonalisation, pf_orth_split - the locked null
    // vectors and the last two basis vectors
    int32_t split, first2;
    double* partial;   // [count + 1][n_chunks]
    double* hsum;      // device copy of h
    double* nrm2;      // device copy of |w'|^2
    double* host_out;  // pinned: h, |w'|^2, redo, then the ticket (written last: the host polls it)
    double thresh;     // second pass when |w'|^2 < thresh |w|^2
    double ticket;     // this step's number (> 0)
    // The second pass ON THE DEVICE (pf_orth_device_passes): the two kernels are queued twice; pass 1 leaves its verdict in
    // device memory and reports to the host only if it was fine, pass 2 returns at once unless the verdict asks for it and
    // reports h1 + h2 and the norm itself.  Whatever is queued behind (the next filter application of a pipelined driver)
    // then always reads the final vector - no pf_orth_redone, no repeated application.
    int32_t pass;      // 0: one pass, a raised verdict is the host's business (pf_orth_end); 1 / 2: first / second of two; -1: not this graph
    double* verdict;   // device copy of pass 1's verdict
    // k_orth_local (the whole step in one launch): arrivals at its grid-wide wait, the count that ends the wait, where a
    // wait that ran out is reported (the resident filter kernel's abort words)
    unsigned long long* counter;
    unsigned long long target;
    uint32_t* abort_flag;
    int32_t* host_abort;
};
struct OrthArgs2 {
    OrthArgs g[2];
};
__device__ __forceinline__ int32_t orth_slot(const OrthArgs& a, int b) { return b < a.split ? a.first + b : a.first2 + (b - a.split); }
__device__ __forceinline__ const double* orth_vec(const OrthArgs& a, int b) { return a.ws + (int64_t)orth_slot(a, b) * a.n_pad; }

// The verdict on a pass from hs = [h (count), |w|^2], by one thread (the same sequence in every block: the same bits):
// sum = h_0^2 + h_1^2 + ... in ascending order, |w'|^2 = |w|^2 - sum (Pythagoras).  `pass` as in OrthArgs; a kernel that
// only ever runs one pass hands in the constant 0.
struct OrthVerdict {
    double redo;   // 0: fine; 1: the second pass is due; 2: it was, and ran
    double after;  // |w'|^2
    double scale;  // what w' is multiplied by: 1 / |w'| if it is to be normalised and the pass was fine
};
__device__ __forceinline__ OrthVerdict orth_verdict(const double* hs, int32_t count, double thresh, int32_t normalize, int32_t pass) {
    double sum = 0.0;
    for (int b = 0; b < count; ++b) sum += hs[b] * hs[b];
    const double before = hs[count], after = before - sum;
    // (false for NaN and for a vanished vector: take the second pass.  The second pass itself is final - "twice is
    // enough" - unless it produced no number at all: verdict 1 then hands the step to pf_orth_end's own passes.
    // The flag goes through a vector register on purpose: this compiler turned `fine ? 0.0 : 1.0` into an s_cselect on
    // SCC behind a v_cmp that sets VCC - the verdict then was whatever the last scalar compare had left)
    int fine = (pass == 2 ? (after == after) : after >= thresh * before) ? 1 : 0;
    asm volatile("" : "+v"(fine));
    return {fine ? (pass == 2 ? 2.0 : 0.0) : 1.0, after, (fine && normalize && after > 1e-280) ? 1.0 / sqrt(after) : 1.0};
}

// Block 0's report of a pass, by the whole block: h into a.hsum (h1 + h2 after a second pass), |w'|^2 into a.nrm2, a first
// pass's verdict into a.verdict, and - unless a first pass asks for the second and leaves the report to it - all of it
// into the pinned a.host_out.  The ticket goes out behind everything else (system-scope fences + the block's barrier):
// the host polls it instead of waiting for an event behind the kernel - the coefficients are known long before the
// projection has finished, and an event record would cost ~5 us of device time per step.
__device__ __forceinline__ void orth_report(const OrthArgs& a, const double* hs, const OrthVerdict& v, int32_t pass) {
    const int32_t count = a.count;
    const bool report = !(pass == 1 && v.redo != 0.0);
    for (int b = threadIdx.x; b < count; b += PF_BLOCK) {
        const double hb = pass == 2 ? a.hsum[b] + hs[b] : hs[b];
        a.hsum[b] = hb;
        if (report) a.host_out[b] = hb;
    }
    if (threadIdx.x == 0) {
        if (pass == 1) *a.verdict = v.redo;
        *a.nrm2 = v.after;
        if (report) {
            a.host_out[count] = v.after;
            a.host_out[count + 1] = v.redo;
        }
    }
    __threadfence_system();
    __syncthreads();
    if (threadIdx.x == 0 && report) __hip_atomic_store(a.host_out + count + 2, a.ticket, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_SYSTEM);
}

// partial[b][chunk] = <slot first+b, slot wslot> over the chunk, b < count; partial[count][chunk] = |w|^2 over the chunk
// VB: basis vectors per block.  1: the shape tuned for bases that live in the Infinity Cache (250k pairs: 6 TB/s).  4 (bases
// beyond it: 1M rows x 50 vectors = 400 MB): the chunk of w is loaded ONCE for four vectors - with one vector per block it
// came back from HBM once per vector, half of the kernel's traffic - and four vectors' 32 KB pieces are in flight per block.
// Per (vector, chunk) the sums are formed by the same threads in the same order either way: the same bits.
template <int VB>
__global__ __launch_bounds__(PF_BLOCK) void k_orth_dots(OrthArgs2 a2) {
    __shared__ double red[VB][PF_BLOCK / PF_WAVE];
    const OrthArgs& a = a2.g[blockIdx.z];
    const int b0 = blockIdx.y * VB;
    const int64_t chunk = blockIdx.x;
    if (a.pass < 0 || b0 > a.count || chunk >= a.n_chunks) return;  // (block-uniform: the grid is sized for the larger graph of a pair)
    if (a.pass == 2 && *a.verdict == 0.0) return;                   // (the first pass was fine)
    // n_pad is a multiple of the chunk: every chunk is whole, every thread has 8 pairs, all of whose loads are issued
    // before the first product waits for one (the sums keep their order)
    double2 cs[PF_CHUNK_PAIRS], xs[VB][PF_CHUNK_PAIRS];
    chunk_load(cs, a.ws + (int64_t)a.wslot * a.n_pad, chunk);
#pragma unroll
    for (int u = 0; u < VB; ++u) {
        const int b = b0 + u;
        if (b > a.count) continue;
        chunk_load(xs[u], a.ws + (int64_t)(b == a.count ? a.wslot : orth_slot(a, b)) * a.n_pad, chunk);
    }
#pragma unroll
    for (int u = 0; u < VB; ++u) {
        if (b0 + u > a.count) continue;
        block_sum_put(chunk_dot_regs(xs[u], cs), red[u]);
    }
    __syncthreads();
    if (threadIdx.x < VB && b0 + (int)threadIdx.x <= a.count)
        a.partial[(int64_t)(b0 + threadIdx.x) * a.n_chunks + chunk] = block_sum_get(red[threadIdx.x]);
}

// P: pairs of rows per thread.  1: a block owns 512 rows (many blocks: what fills the chip at 250k rows).  8 (bases beyond the
// Infinity Cache): a block owns a whole 4096-row chunk, so that it reads 32 KB of every basis vector in one piece instead of
// 4 KB pieces of fifty streams (DRAM pages), and the sums of the partial dot products are redone by an eighth of the blocks.
// Per row the subtractions are the same, in the same order.
template <int P>
__global__ __launch_bounds__(PF_BLOCK) void k_orth_project(OrthArgs2 a2) {
    __shared__ double hs[PF_ORTH_MAX + 1];
    __shared__ OrthVerdict s_v;
    const OrthArgs& a = a2.g[blockIdx.z];
    if (a.pass < 0 || 2 * (int64_t)blockIdx.x * PF_BLOCK * P >= a.n_pad) return;  // (block-uniform)
    if (a.pass == 2 && *a.verdict == 0.0) return;
    const int32_t count = a.count;
    column_sums(a.partial, a.n_chunks, count + 1, hs);
    __syncthreads();
    if (threadIdx.x == 0) s_v = orth_verdict(hs, count, a.thresh, a.normalize, a.pass);
    __syncthreads();
    if (blockIdx.x == 0) orth_report(a, hs, s_v, a.pass);
    const double sc = s_v.scale;
    if constexpr (P == 1) {
        const int64_t i = 2 * ((int64_t)blockIdx.x * PF_BLOCK + threadIdx.x);
        if (i >= a.n_pad) return;
        double2 acc = *reinterpret_cast<double2*>(a.ws + (int64_t)a.wslot * a.n_pad + i);
        // eight basis vectors' loads in flight per thread (the subtractions keep their order: the same bits)
        int b = 0;
        for (; b + 8 <= count; b += 8) {
            double2 vv[8];
#pragma unroll
            for (int u = 0; u < 8; ++u) vv[u] = *reinterpret_cast<const double2*>(orth_vec(a, b + u) + i);
#pragma unroll
            for (int u = 0; u < 8; ++u) axpy_sub(acc, hs[b + u], vv[u]);
        }
        if (b < count) {
            // the last 1-7 vectors (a local step of Lanczos with partial reorthogonalisation has 3-4 in all): their loads in
            // flight together as well - one round trip instead of one per vector; a vector past the end is the last one
            // again with coefficient 0 (x - 0 v = x exactly)
            double2 vv[7];
            double hh[7];
#pragma unroll
            for (int u = 0; u < 7; ++u) {
                const int bu = b + u < count ? b + u : count - 1;
                vv[u] = *reinterpret_cast<const double2*>(orth_vec(a, bu) + i);
                hh[u] = b + u < count ? hs[bu] : 0.0;
            }
#pragma unroll
            for (int u = 0; u < 7; ++u) axpy_sub(acc, hh[u], vv[u]);
        }
        acc.x *= sc;
        acc.y *= sc;
        *reinterpret_cast<double2*>(a.ws + (int64_t)a.wslot * a.n_pad + i) = acc;
    } else {
        const int64_t i0 = (int64_t)blockIdx.x * (2 * PF_BLOCK * P) + 2 * threadIdx.x;  // (n_pad is a multiple of 4096: whole blocks)
        double2 acc[P];
#pragma unroll
        for (int it = 0; it < P; ++it) acc[it] = *reinterpret_cast<double2*>(a.ws + (int64_t)a.wslot * a.n_pad + i0 + (int64_t)it * (2 * PF_BLOCK));
        // (one block per CU at this shape: two vectors' pieces - 2 x 8 x 16 bytes per thread - are requested before the
        // first is used; the subtractions keep the order b, b + 1)
        int b = 0;
        for (; b + 2 <= count; b += 2) {
            const double h0 = hs[b], h1 = hs[b + 1];
            const double* v0 = orth_vec(a, b) + i0;
            const double* v1 = orth_vec(a, b + 1) + i0;
            double2 x0[P], x1[P];
#pragma unroll
            for (int it = 0; it < P; ++it) x0[it] = *reinterpret_cast<const double2*>(v0 + (int64_t)it * (2 * PF_BLOCK));
#pragma unroll
            for (int it = 0; it < P; ++it) x1[it] = *reinterpret_cast<const double2*>(v1 + (int64_t)it * (2 * PF_BLOCK));
#pragma unroll
            for (int it = 0; it < P; ++it) {
                axpy_sub(acc[it], h0, x0[it]);
                axpy_sub(acc[it], h1, x1[it]);
            }
        }
        for (; b < count; ++b) {
            const double hb = hs[b];
            const double* vb = orth_vec(a, b) + i0;
            double2 vv[P];
#pragma unroll
            for (int it = 0; it < P; ++it) vv[it] = *reinterpret_cast<const double2*>(vb + (int64_t)it * (2 * PF_BLOCK));
#pragma unroll
            for (int it = 0; it < P; ++it) axpy_sub(acc[it], hb, vv[it]);
        }
#pragma unroll
        for (int it = 0; it < P; ++it) {
            acc[it].x *= sc;
            acc[it].y *= sc;
            *reinterpret_cast<double2*>(a.ws + (int64_t)a.wslot * a.n_pad + i0 + (int64_t)it * (2 * PF_BLOCK)) = acc[it];
        }
    }
}
// One lane per block: arrival at the meeting of the blocks of a graph inside a launch, then a bounded wait until the counter
// has reached `want`.  What the blocks exchange travels in 8-byte agent-scope atomic stores and loads (the partial sums):
// performed at the memory side, the stores waited for before the arrival, the loads issued behind the poll that matched -
// no release in front and no acquire behind (an L2 write-back and an invalidation: ~3 us of a 14 us step), and the poll
// itself is a relaxed load.  0: the wait ran out (abort words raised).
__device__ __forceinline__ int orth_meet(const OrthArgs& a, unsigned long long want) {
    __hip_atomic_fetch_add(a.counter, 1ull, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    const unsigned long long t0 = __builtin_amdgcn_s_memrealtime();
    while (__hip_atomic_load(a.counter, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) < want) {
        if (__builtin_amdgcn_s_memrealtime() - t0 > 20000000ull ||  // 0.2 s of the 100 MHz clock
            __hip_atomic_load(a.abort_flag, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) != 0u) {
            __hip_atomic_store(a.abort_flag, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            *a.host_abort = 1;
            return 0;
        }
        __builtin_amdgcn_s_sleep(2);
    }
    return 1;
}

// A LOCAL Gram-Schmidt step (Lanczos with partial reorthogonalisation: the null vectors and the last two basis vectors, 4
// at most) in ONE launch.  A block owns a 4096-row chunk: it loads w and the basis vectors' pieces once, forms the chunk's
// partial sums with k_orth_dots' calls, publishes them, waits until every chunk of the graph has (a counter, bounded),
// sums the partials in column_sum's order, takes k_orth_project's verdict and report (as one pass: pass = 0, a constant
// here) and projects the rows it still holds in registers - the same operations in the same order on every number: the
// same bits as the two launches, one kernel boundary less (~5 us of a ~16 us step).  The grid is one block per chunk and
// graph (122 at 250k, 490 at 1M rows): all resident.
constexpr int PF_ORTH_LOCAL_MAX = 4;
__global__ __launch_bounds__(PF_BLOCK) void k_orth_local(OrthArgs2 a2) {
    __shared__ double red[PF_ORTH_LOCAL_MAX + 1][PF_BLOCK / PF_WAVE];
    __shared__ double hs[PF_ORTH_LOCAL_MAX + 1];
    __shared__ OrthVerdict s_v;
    __shared__ int s_ok;
    const OrthArgs& a = a2.g[blockIdx.z];
    const int64_t chunk = blockIdx.x;
    if (a.pass < 0 || chunk >= a.n_chunks) return;  // (block-uniform: the grid is sized for the larger graph of a pair)
    const int32_t count = a.count;
    const int lane = threadIdx.x & (PF_WAVE - 1);
    double* w = a.ws + (int64_t)a.wslot * a.n_pad;
    double2 cs[PF_CHUNK_PAIRS], xs[PF_ORTH_LOCAL_MAX][PF_CHUNK_PAIRS];
    chunk_load(cs, w, chunk);
#pragma unroll
    for (int u = 0; u < PF_ORTH_LOCAL_MAX; ++u) chunk_load(xs[u], orth_vec(a, u < count ? u : count - 1), chunk);  // (past the end: the last again)
    // ---- the chunk's partial sums: k_orth_dots' calls (column `count`: |w|^2)
#pragma unroll
    for (int u = 0; u <= PF_ORTH_LOCAL_MAX; ++u) {
        if (u > count) continue;
        double2 x[PF_CHUNK_PAIRS];
#pragma unroll
        for (int it = 0; it < PF_CHUNK_PAIRS; ++it) x[it] = u == count ? cs[it] : xs[u < PF_ORTH_LOCAL_MAX ? u : 0][it];
        block_sum_put(chunk_dot_regs(x, cs), red[u]);
    }
    __syncthreads();
    if ((int)threadIdx.x <= count) {
        __hip_atomic_store(reinterpret_cast<unsigned long long*>(a.partial) + (int64_t)threadIdx.x * a.n_chunks + chunk,
                           (unsigned long long)__double_as_longlong(block_sum_get(red[threadIdx.x])), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");  // in memory before the block says it has arrived
    }
    __syncthreads();
    // ---- every chunk of this graph has published: one arrival per block, a bounded wait
    if (threadIdx.x == 0) s_ok = orth_meet(a, a.target);
    __syncthreads();
    if (!s_ok) return;
    // ---- the sums of the partials, read from where the other XCDs wrote them: column_sum's additions in its order, of the
    // two columns of a wave - b and b + 4 - at once so that their loads are in flight together
    {
        const int b0 = threadIdx.x / PF_WAVE, b1 = b0 + PF_BLOCK / PF_WAVE;
        auto part = [&](int b, int64_t k) {
            return b < count + 1 ? __longlong_as_double((long long)__hip_atomic_load(reinterpret_cast<unsigned long long*>(a.partial) + (int64_t)b * a.n_chunks + k,
                                                                                     __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT))
                                 : 0.0;
        };
        double s0 = 0.0, s1 = 0.0;
        for (int64_t k = lane; k < a.n_chunks; k += PF_WAVE) {
            const double x0 = part(b0, k), x1 = part(b1, k);
            s0 += x0;
            s1 += x1;
        }
        s0 = wave_sum_down(s0);
        s1 = wave_sum_down(s1);
        if (lane == 0 && b0 < count + 1) hs[b0] = s0;
        if (lane == 0 && b1 < count + 1) hs[b1] = s1;
    }
    __syncthreads();
    if (threadIdx.x == 0) s_v = orth_verdict(hs, count, a.thresh, a.normalize, 0);  // (one pass: a raised verdict is pf_orth_end's business)
    __syncthreads();
    if (chunk == 0) orth_report(a, hs, s_v, 0);
    const double sc = s_v.scale;
#pragma unroll
    for (int it = 0; it < PF_CHUNK_PAIRS; ++it) {
        double2 acc = cs[it];
#pragma unroll
        for (int u = 0; u < PF_ORTH_LOCAL_MAX; ++u)
            if (u < count) axpy_sub(acc, hs[u], xs[u][it]);
        acc.x *= sc;
        acc.y *= sc;
        *reinterpret_cast<double2*>(w + chunk * PF_DOT_CHUNK + 2 * threadIdx.x + (int64_t)it * (2 * PF_BLOCK)) = acc;
    }
}
__global__ __launch_bounds__(PF_BLOCK) void k_scale_finishing(double* __restrict__ x, int64_t n_pad, const double* __restrict__ partial,
                                                              int64_t n_chunks, int normalize, const double* __restrict__ hsum,
                                                              int32_t count, double* __restrict__ nrm2, double* __restrict__ host_out) {
    __shared__ double s_v;
    if (threadIdx.x < PF_WAVE) {
        const double s = column_sum(partial, 0, n_chunks, threadIdx.x);
        if (threadIdx.x == 0) s_v = s;
    }
    __syncthreads();
    const double v = s_v;
    if (blockIdx.x == 0) {
        for (int b = threadIdx.x; b < count; b += PF_BLOCK) host_out[b] = hsum[b];
        if (threadIdx.x == 0) {
            *nrm2 = v;
            host_out[count] = v;
            host_out[count + 1] = 0.0;  // (the verdict slot of k_orth_project: nothing left to redo)
        }
    }
    const int64_t i = (int64_t)blockIdx.x * PF_BLOCK + threadIdx.x;
    if (normalize && i < n_pad && v > 1e-280) x[i] *= 1.0 / sqrt(v);
}

}  // namespace

extern "C" {

// One outer step of a pipelined pair driver in ONE library call: the Gram-Schmidt step of both graphs (pf_orth_begin2) and,
// queued right behind it, the next filter application of both (pf_cheb2) - the device then never waits for the host
// between the two (two calls from Python leave it idle for ~15-25 us per step, a tenth of the filter application).
//   orth[8]   = {w, first, count, normalize} of graph a, then of graph b
//   cheb_i[8] = {op, src, dst, degree} of graph a, then of graph b;   cheb_d[6] = {c, e, rho} of a, then of b
int pf_orth_cheb2(pf_graph* ga, pf_graph* gb, const int32_t* orth, const int32_t* cheb_i, const double* cheb_d) {
    PF_CHECK(ga && gb && orth && cheb_i && cheb_d, PF_E_ARG, "pf_orth_cheb2: NULL argument");
    PF_TRY(pf_orth_begin2(ga, orth[0], orth[1], orth[2], orth[3], gb, orth[4], orth[5], orth[6], orth[7]));
    return pf_cheb2(ga, cheb_i[0], cheb_i[1], cheb_i[2], cheb_i[3], cheb_d[0], cheb_d[1], cheb_d[2], gb, cheb_i[4], cheb_i[5], cheb_i[6],
                    cheb_i[7], cheb_d[3], cheb_d[4], cheb_d[5]);
}

// pf_orth_one_launch: -1 as the environment says (PF_ORTH_LOCAL; on by default), 0 the separate launches, 1 on
static std::atomic<int> g_orth_one_launch{-1};

// blocks of k_orth_local the device holds at once (0: the one-launch step is switched off - PF_ORTH_LOCAL=0 - or unknown)
static int64_t orth_local_capacity(int device) {
    static std::mutex m;
    static std::map<int, int64_t> cap;
    std::lock_guard<std::mutex> lk(m);
    auto it = cap.find(device);
    if (it != cap.end()) return it->second;
    int64_t c = 0;
    const char* e = getenv("PF_ORTH_LOCAL");
    if (!(e && e[0] == '0')) {
        int per_cu = 0;
        hipDeviceProp_t prop;
        if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, reinterpret_cast<const void*>(k_orth_local), PF_BLOCK, 0) == hipSuccess &&
            hipGetDeviceProperties(&prop, device) == hipSuccess)
            c = (int64_t)per_cu * prop.multiProcessorCount;
        else
            (void)hipGetLastError();
    }
    cap[device] = c;
    return c;
}

// the counter of the meeting inside k_orth_local: `arrivals` more per launch
static int orth_meetings_prepare(pf_graph* g, OrthArgs& a, unsigned long long arrivals, hipStream_t st) {
    pf_ctx* ctx = g->ctx;
    const uint64_t epoch = pf_persist_abort_epoch();
    if (!g->orth_counter) PF_HIP(pf_malloc(st, (void**)&g->orth_counter, sizeof(unsigned long long)));
    if (g->orth_epoch != epoch) {  // new, or a bounded wait ran out since: whatever had arrived then is void
        PF_HIP(hipMemsetAsync(g->orth_counter, 0, sizeof(unsigned long long), st));
        g->orth_arrivals = 0;
        g->orth_epoch = epoch;
    }
    g->orth_arrivals += arrivals;
    a.counter = g->orth_counter;
    a.target = g->orth_arrivals;
    a.abort_flag = ctx->persist_sync;
    a.host_abort = ctx->persist_abort;
    return PF_OK;
}

// the two launches of one Gram-Schmidt pass (of one graph, or of both graphs of a pair: ng = 2); bases beyond the Infinity
// Cache (>= 400k rows: 1M x 50 vectors = 400 MB) take the shapes with several vectors / a whole chunk per block
static int orth_launch_pass(OrthArgs2& a2, int ng, int64_t n_chunks, int64_t n_pad, int32_t count, hipStream_t st, pf_graph* const* gs = nullptr) {
    // a local step (4 vectors at most, one pass) of every graph in the launch: the whole step in ONE kernel
    bool local = gs != nullptr && count <= PF_ORTH_LOCAL_MAX && count >= 1;
    for (int q = 0; q < ng && local; ++q) local = a2.g[q].pass == 0 && a2.g[q].count <= PF_ORTH_LOCAL_MAX && a2.g[q].count >= 1;
    if (local && g_orth_one_launch.load() != 0 && pf_persist_trusted() && n_chunks * ng <= orth_local_capacity(gs[0]->ctx->device)) {
        PF_TRY(pf_persist_sync_ensure(gs[0]->ctx));
        for (int q = 0; q < ng; ++q) PF_TRY(orth_meetings_prepare(gs[q], a2.g[q], (unsigned long long)gs[q]->n_chunks, st));
        k_orth_local<<<dim3((unsigned)n_chunks, 1u, (unsigned)ng), PF_BLOCK, 0, st>>>(a2);
        PF_HIP(hipGetLastError());
        return PF_OK;
    }
    if (n_pad >= 400000) {
        k_orth_dots<4><<<dim3((unsigned)n_chunks, (unsigned)((count + 1 + 3) / 4), (unsigned)ng), PF_BLOCK, 0, st>>>(a2);
        PF_HIP(hipGetLastError());
        k_orth_project<8><<<dim3((unsigned)(n_pad / (2 * PF_BLOCK * 8)), 1u, (unsigned)ng), PF_BLOCK, 0, st>>>(a2);
    } else {
        k_orth_dots<1><<<dim3((unsigned)n_chunks, (unsigned)(count + 1), (unsigned)ng), PF_BLOCK, 0, st>>>(a2);
        PF_HIP(hipGetLastError());
        k_orth_project<1><<<dim3(pf_blocks(n_pad / 2), 1u, (unsigned)ng), PF_BLOCK, 0, st>>>(a2);
    }
    PF_HIP(hipGetLastError());
    return PF_OK;
}

// checks, pinned result buffer, event: everything of pf_orth_begin that comes before the launches
static int orth_prepare(pf_graph* g, int32_t w, int32_t first, int32_t count, int32_t normalize) {
    // pf_orth_split (this step only, whatever becomes of it): the basis is slots [first, first + split) and
    // [first2, first2 + count - split)
    const int32_t split_req = g->orth_split, first2_req = g->orth_first2;
    g->orth_split = -1;
    PF_TRY(pf_check_slots(g, w, 1, "pf_orth_begin"));
    if (split_req < 0) PF_TRY(pf_check_slots(g, first, count, "pf_orth_begin"));
    PF_CHECK(g->orth_pending < 0, PF_E_STATE, "pf_orth_begin: a previous pf_orth_begin has not been collected");
    g->orth_split_now = -1;
    if (split_req >= 0) {
        const int32_t split = split_req, first2 = first2_req;
        PF_CHECK(split <= count && count > 0 && count < PF_ORTH_MAX, PF_E_ARG, "pf_orth_split: %d of %d vectors in the first range", split, count);
        PF_TRY(pf_check_slots(g, first, split, "pf_orth_begin"));
        PF_TRY(pf_check_slots(g, first2, count - split, "pf_orth_begin"));
        PF_CHECK((w < first || w >= first + split) && (w < first2 || w >= first2 + count - split), PF_E_ARG, "pf_orth_begin: w inside the basis ranges");
        PF_CHECK(first + split <= first2 || first2 + count - split <= first, PF_E_ARG, "pf_orth_split: overlapping ranges");
        g->orth_split_now = split;
        g->orth_first2_now = first2;
    } else {
        PF_CHECK(w < first || w >= first + count, PF_E_ARG, "pf_orth_begin: w inside the basis range");
    }
    hipStream_t st = g->ctx->stream;
    PF_TRY(pf_reduce_ensure(g, count + 1));  // (+ the |w|^2 column)
    // (h, |w'|^2, verdict, ticket: count + 3 doubles of cap + 2; an outgrown block may still be written to by a kernel in
    // flight: the stream is drained before it goes back to the pool)
    PF_HIP(g->orth_land.ensure(g->ctx->pools, count + 1, 64, st));
    g->orth_land.host[count + 1] = 0.0;  // the verdict slot; only k_orth_project ever raises it
    g->orth_land.host[count + 2] = 0.0;  // the ticket slot
    g->orth_ticket = 0.0;              // (set by the launch paths whose kernel writes a ticket)
    g->orth_w = w, g->orth_first = first, g->orth_normalize = normalize ? 1 : 0;
    return PF_OK;
}

// g->coef (pf_reduce_ensure: 8 x coef_cap doubles) as the Gram-Schmidt step uses it
struct OrthCoef {
    double *hpass, *hsum, *nrm2, *verdict;  // coefficients of the current pass; h1 + h2; |w'|^2; a first device pass's verdict
};
static OrthCoef orth_coef(const pf_graph* g) {
    const int32_t cap = g->coef_cap;
    return {g->coef, g->coef + cap, g->coef + 2 * cap, g->coef + 3 * cap};
}

static OrthArgs orth_args(pf_graph* g, int32_t w, int32_t first, int32_t count, int32_t normalize) {
    const OrthCoef c = orth_coef(g);
    OrthArgs a{};
    a.ws = g->ws;
    a.n_pad = g->n_pad;
    a.n_chunks = g->n_chunks;
    a.first = first, a.count = count, a.wslot = w, a.normalize = normalize ? 1 : 0;
    a.split = g->orth_split_now >= 0 ? g->orth_split_now : count;
    a.first2 = g->orth_first2_now;
    a.partial = g->partials;
    a.hsum = c.hsum;
    a.nrm2 = c.nrm2;
    a.host_out = g->orth_land.host;
    a.thresh = g->orth_thresh;
    g->orth_serial += 1.0;
    a.ticket = g->orth_serial;
    g->orth_ticket = a.ticket;  // pf_orth_end polls for it
    a.pass = g->orth_device_passes ? 1 : 0;
    a.verdict = c.verdict;
    return a;
}

// The fused step of ng graphs of one ctx (one, or the two of a pair), each with 0 < count < PF_ORTH_MAX, behind the same
// launches: 2 launches (or k_orth_local's one) and no copies - the projection, its norm (Pythagoras) and the normalisation
// ride behind one batch of dot products; the second Gram-Schmidt pass is queued as well with pf_orth_device_passes, and is
// pf_orth_end's business otherwise in the rare step that needs it.  No event: the results carry tickets, pf_orth_end
// polls for them.
struct OrthStep {
    pf_graph* g;
    int32_t w, first, count, normalize;
};
static int orth_fused(const OrthStep* s, int ng) {
    for (int q = 0; q < ng; ++q) PF_TRY(orth_prepare(s[q].g, s[q].w, s[q].first, s[q].count, s[q].normalize));
    hipStream_t st = s[0].g->ctx->stream;
    OrthArgs2 a2{};
    pf_graph* gs[2] = {};
    int64_t chunks = 0, pad = 0;  // (the grids are sized for the larger graph)
    int32_t count = 0;
    bool second = false;
    for (int q = 0; q < ng; ++q) {
        gs[q] = s[q].g;
        a2.g[q] = orth_args(s[q].g, s[q].w, s[q].first, s[q].count, s[q].normalize);
        chunks = std::max(chunks, gs[q]->n_chunks), pad = std::max(pad, gs[q]->n_pad), count = std::max(count, s[q].count);
        second = second || a2.g[q].pass == 1;
    }
    PF_TRY(orth_launch_pass(a2, ng, chunks, pad, count, st, gs));
    if (second) {  // the second pass of the graph(s) that asked for it, on the device's own verdict
        for (int q = 0; q < ng; ++q) a2.g[q].pass = a2.g[q].pass == 1 ? 2 : -1;
        PF_TRY(orth_launch_pass(a2, ng, chunks, pad, count, st));
    }
    for (int q = 0; q < ng; ++q) {
        gs[q]->orth_wait = gs[q]->orth_land.ev;
        gs[q]->orth_pending = s[q].count;
    }
    return PF_OK;
}

int pf_orth_begin(pf_graph* g, int32_t w, int32_t first, int32_t count, int32_t normalize) {
    if (count > 0 && count < PF_ORTH_MAX) {
        const OrthStep one = {g, w, first, count, normalize};
        return orth_fused(&one, 1);
    }
    PF_TRY(orth_prepare(g, w, first, count, normalize));
    hipStream_t st = g->ctx->stream;
    const OrthCoef c = orth_coef(g);
    if (count == 0) {
        PF_TRY(pf_dot_partials(g, w, w, 1, g->partials));
        k_scale_finishing<<<pf_blocks(g->n_pad), PF_BLOCK, 0, st>>>(pf_slot(g, w), g->n_pad, g->partials, g->n_chunks, normalize ? 1 : 0,
                                                              c.hsum, count, c.nrm2, g->orth_land.host);
        PF_HIP(hipGetLastError());
    } else {
        for (int pass = 0; pass < 2; ++pass) {
            PF_TRY(pf_dots_device(g, w, first, count, c.hpass, c.hsum, pass));
            PF_TRY(pf_multi_axpy(g, w, first, count, c.hpass));
        }
        PF_TRY(pf_dots_device(g, w, w, 1, c.nrm2, nullptr, 0));
        if (normalize) PF_TRY(pf_scale_rsqrt(g, pf_slot(g, w), c.nrm2));
        PF_HIP(hipMemcpyAsync(g->orth_land.host, c.hsum, sizeof(double) * count, hipMemcpyDeviceToHost, st));
        PF_HIP(hipMemcpyAsync(g->orth_land.host + count, c.nrm2, sizeof(double), hipMemcpyDeviceToHost, st));
    }
    PF_HIP(hipEventRecord(g->orth_land.ev, st));  // (no ticket from these kernels: pf_orth_end waits for the event)
    g->orth_wait = g->orth_land.ev;
    g->orth_pending = count;
    return PF_OK;
}

// pf_orth_begin for the two graphs of a pair (one ctx) behind the same two launches; each graph's result is collected
// with its own pf_orth_end.  Shapes the fused kernels do not cover take one pf_orth_begin each.
int pf_orth_begin2(pf_graph* ga, int32_t w_a, int32_t first_a, int32_t count_a, int32_t normalize_a, pf_graph* gb, int32_t w_b,
                   int32_t first_b, int32_t count_b, int32_t normalize_b) {
    PF_CHECK(ga != nullptr && gb != nullptr && ga != gb, PF_E_ARG, "pf_orth_begin2: two different graphs are needed");
    if (ga->ctx != gb->ctx || count_a <= 0 || count_b <= 0 || count_a >= PF_ORTH_MAX || count_b >= PF_ORTH_MAX) {
        PF_TRY(pf_orth_begin(ga, w_a, first_a, count_a, normalize_a));
        return pf_orth_begin(gb, w_b, first_b, count_b, normalize_b);
    }
    const OrthStep two[2] = {{ga, w_a, first_a, count_a, normalize_a}, {gb, w_b, first_b, count_b, normalize_b}};
    return orth_fused(two, 2);
}

int pf_orth_end(pf_graph* g, double* h, double* nrm) {
    PF_CHECK(g != nullptr && nrm != nullptr, PF_E_ARG, "pf_orth_end: NULL argument");
    PF_CHECK(g->orth_pending >= 0, PF_E_STATE, "pf_orth_end: no pf_orth_begin in flight");
    const int32_t count = g->orth_pending;
    PF_CHECK(h != nullptr || count == 0, PF_E_ARG, "pf_orth_end: h is NULL");
    PF_HIP(hipSetDevice(g->ctx->device));
    if (g->orth_ticket != 0.0) {
        // the kernel's block 0 writes the results and then the ticket into the pinned buffer: poll for it (the stream is asked
        // now and then whether it has run dry without a ticket - a failed launch must not hang the host)
        volatile double* ticket = g->orth_land.host + count + 2;
        bool got = false;
        for (uint64_t spin = 0;; ++spin) {
            if (__atomic_load_n(reinterpret_cast<volatile uint64_t*>(ticket), __ATOMIC_ACQUIRE) ==
                *reinterpret_cast<const uint64_t*>(&g->orth_ticket)) {
                got = true;
                break;
            }
            if ((spin & 0xfff) == 0xfff) {
                const hipError_t q = hipStreamQuery(g->ctx->stream);
                if (q == hipSuccess) {  // everything queued has completed: the ticket is there, or never will be
                    got = __atomic_load_n(reinterpret_cast<volatile uint64_t*>(ticket), __ATOMIC_ACQUIRE) ==
                          *reinterpret_cast<const uint64_t*>(&g->orth_ticket);
                    break;
                }
                if (q != hipErrorNotReady) {
                    g->orth_pending = -1;
                    PF_HIP(q);
                }
            }
            __builtin_ia32_pause();
        }
        if (!got) {
            g->orth_pending = -1;
            PF_TRY(pf_persist_check(g->ctx));
            PF_CHECK(false, PF_E_HIP, "pf_orth_end: the Gram-Schmidt step never reported (launch failure?)");
        }
    } else {
        PF_HIP(hipEventSynchronize(g->orth_wait));
    }
    g->orth_pending = -1;
    g->orth_redone = 0;
    PF_TRY(pf_persist_check(g->ctx));
    g->orth_twice = g->orth_land.host[count + 1] == 2.0 ? 1 : 0;  // (both passes ran on the device: nothing behind them read a stale w)
    if (g->orth_land.host[count + 1] == 1.0) {
        // the first pass cancelled digits (or w vanished): second pass, exact norm, normalisation - synchronously.
        // Whatever was queued behind pf_orth_begin read a w that is only now final: pf_orth_redone tells the caller.
        hipStream_t st = g->ctx->stream;
        const OrthCoef c = orth_coef(g);
        const int32_t w = g->orth_w;
        const int32_t split = g->orth_split_now >= 0 ? g->orth_split_now : count;
        // one range of the basis, or two: columns [at[r], at[r + 1]) are slots from[r] .. (all dot products first, as in one)
        const int32_t from[2] = {g->orth_first, g->orth_first2_now}, at[3] = {0, split, count};
        for (int r = 0; r < 2; ++r)
            if (at[r + 1] > at[r]) PF_TRY(pf_dot_partials(g, w, from[r], at[r + 1] - at[r], g->partials + (size_t)at[r] * g->n_chunks));
        for (int r = 0; r < 2; ++r) {
            if (at[r + 1] == at[r]) continue;
            k_axpy_finishing<<<pf_blocks(g->n_pad / 2), PF_BLOCK, 0, st>>>(g->ws, g->n_pad, from[r], at[r + 1] - at[r], w,
                                                                      g->partials + (size_t)at[r] * g->n_chunks, g->n_chunks, c.hsum + at[r], 1);
            PF_HIP(hipGetLastError());
        }
        PF_TRY(pf_dot_partials(g, w, w, 1, g->partials));
        k_scale_finishing<<<pf_blocks(g->n_pad), PF_BLOCK, 0, st>>>(pf_slot(g, w), g->n_pad, g->partials, g->n_chunks, g->orth_normalize,
                                                              c.hsum, count, c.nrm2, g->orth_land.host);
        PF_HIP(hipGetLastError());
        PF_HIP(hipStreamSynchronize(st));
        PF_TRY(pf_persist_check(g->ctx));
        g->orth_redone = 1;
    }
    for (int32_t b = 0; b < count; ++b) h[b] = g->orth_land.host[b];
    const double v = g->orth_land.host[count];
    *nrm = sqrt(v > 0.0 ? v : 0.0);
    return PF_OK;
}

// The criterion for the second Gram-Schmidt pass: |w'| < 0.3 |w| by default; strict: |w'| < 0.71 |w| (the classical
// "twice is enough" constant).  The loose one is measured safe where it matters for speed - the filtered iteration of a
// large graph: ~35 steps, ratios 0.35-0.78 - and is NOT safe for an unfiltered iteration that comes close to exhausting a
// small space (a 120-vertex mesh, 47 steps: ratios around 0.3-0.5 step after step, orthogonality lost, Ritz values
// above the spectrum), where the second pass costs nothing that matters.  Drivers switch to strict there.
int pf_orth_strict(pf_graph* g, int32_t on) {
    PF_CHECK(g != nullptr, PF_E_ARG, "pf_orth_strict: NULL graph");
    g->orth_thresh = on >= 2 ? 4.0 : (on ? 0.5 : 0.09);  // (2: |w'|^2 < 4 |w|^2 holds always - every step takes its second pass)
    return PF_OK;
}

int pf_orth_device_passes(pf_graph* g, int32_t on) {
    PF_CHECK(g != nullptr, PF_E_ARG, "pf_orth_device_passes: NULL graph");
    g->orth_device_passes = on ? 1 : 0;
    return PF_OK;
}

int pf_orth_one_launch(int32_t on) {
    g_orth_one_launch.store(on < 0 ? -1 : (on ? 1 : 0));
    return PF_OK;
}

// The NEXT pf_orth_begin / _begin2 / pf_orth_cheb2 step of this graph (and only that one) takes its basis from two ranges
// of slots: [first, first + split) and [first2, first2 + count - split), first / count as passed to that call.
int pf_orth_split(pf_graph* g, int32_t first2, int32_t split) {
    PF_CHECK(g != nullptr && split >= 0 && first2 >= 0, PF_E_ARG, "pf_orth_split: bad argument");
    g->orth_split = split;
    g->orth_first2 = first2;
    return PF_OK;
}

int pf_orth_redone(pf_graph* g) {
    PF_CHECK(g != nullptr, PF_E_ARG, "pf_orth_redone: NULL graph");
    return g->orth_redone ? 1 : (g->orth_twice ? 2 : 0);
}

int pf_orth(pf_graph* g, int32_t w, int32_t first, int32_t count, double* h, double* nrm) {
    PF_CHECK(nrm != nullptr && (h != nullptr || count == 0), PF_E_ARG, "pf_orth: NULL output");
    PF_TRY(pf_orth_begin(g, w, first, count, 0));
    return pf_orth_end(g, h, nrm);
}

}  // extern "C"

int pf_multi_axpy(pf_graph* g, int32_t w, int32_t first, int32_t count, const double* d_h) {
    k_multi_axpy<<<pf_blocks(g->n_pad / 2), PF_BLOCK, 0, g->ctx->stream>>>(g->ws, g->n_pad, first, count, w, d_h);
    PF_HIP(hipGetLastError());
    return PF_OK;
}
