// The small reductions of the solve over workspace slots, and their way to the host: dot products, Gram matrices and
// residual norms (two-stage and atomic-free: per-chunk partial sums in g->partials, finished in a fixed order into
// g->coef, so results are bitwise reproducible run to run), the basis rotation pf_combine and pf_scale.  The order of
// every sum is pf_sums.h's: a first-stage kernel here is a chunk sum and the block sum, the one second stage (k_dot_finish,
// finish_queue) is the column sum; pf_resnorm is pf_resnorms with a count of one.  The few
// doubles of a result reach the host either at once (small_to_host: pinned scratch, a copy kernel, a wait) or in two
// halves (small_begin / pf_small_end: the graph's own pinned landing and an event).
#include <math.h>
#include <string.h>

#include <algorithm>

#include "pf_internal.h"
#include "pf_launch.h"
#include "pf_sums.h"

namespace {

// partial[b][chunk] = <slot first+b, slot wslot> over the chunk (pf_sums.h: fixed order -> deterministic); with
// self_col >= 0 column b == self_col is w itself (|w|^2 rides along)
// (d_*: the body of k_* - the kernel itself, and the form pf_launch.h records when a pair's driver queues the heads of its
// two solves in shared launches, f_*)
__device__ __forceinline__ void d_dot_partial(const double* __restrict__ ws, int64_t n_pad, int32_t first,
                                              int32_t wslot, int64_t n_chunks, double* __restrict__ partial,
                                              int32_t self_col) {
    __shared__ double red[PF_BLOCK / PF_WAVE];
    const int b = blockIdx.y;
    const int64_t chunk = blockIdx.x;
    const double* v = ws + (int64_t)(b == self_col ? wslot : first + b) * n_pad;
    const double* w = ws + (int64_t)wslot * n_pad;
    block_sum_put(chunk_dot(v, w, chunk, n_pad), red);
    __syncthreads();
    if (threadIdx.x == 0) partial[(int64_t)b * n_chunks + chunk] = block_sum_get(red);
}
__global__ __launch_bounds__(PF_BLOCK) void k_dot_partial(const double* __restrict__ ws, int64_t n_pad, int32_t first,
                                                          int32_t wslot, int64_t n_chunks, double* __restrict__ partial,
                                                          int32_t self_col = -1) {
    d_dot_partial(ws, n_pad, first, wslot, n_chunks, partial, self_col);
}
struct f_dot_partial {
    static constexpr int BOUNDS = PF_BLOCK;
    static __device__ __forceinline__ void run(const double* ws, int64_t n_pad, int32_t first, int32_t wslot, int64_t n_chunks, double* partial,
                                               int32_t self_col) {
        d_dot_partial(ws, n_pad, first, wslot, n_chunks, partial, self_col);
    }
};

// out[b] = sum_chunks partial[b][chunk];  acc[b] (+)= out[b]
__device__ __forceinline__ void d_dot_finish(const double* __restrict__ partial, int64_t n_chunks,
                                             double* __restrict__ out, double* __restrict__ acc, int accumulate) {
    const int b = blockIdx.x;
    const double s = column_sum(partial, b, n_chunks, threadIdx.x);
    if (threadIdx.x == 0) {
        out[b] = s;
        if (acc) acc[b] = accumulate ? acc[b] + s : s;
    }
}
__global__ __launch_bounds__(PF_WAVE) void k_dot_finish(const double* __restrict__ partial, int64_t n_chunks,
                                                        double* __restrict__ out, double* __restrict__ acc, int accumulate) {
    d_dot_finish(partial, n_chunks, out, acc, accumulate);
}
struct f_dot_finish {
    static constexpr int BOUNDS = PF_WAVE;
    static __device__ __forceinline__ void run(const double* partial, int64_t n_chunks, double* out, double* acc, int accumulate) {
        d_dot_finish(partial, n_chunks, out, acc, accumulate);
    }
};

__global__ __launch_bounds__(PF_BLOCK) void k_scale(double* __restrict__ x, int64_t n_pad, double alpha) {
    const int64_t i = (int64_t)blockIdx.x * PF_BLOCK + threadIdx.x;
    if (i < n_pad) x[i] *= alpha;
}

// x *= 1/sqrt(*nrm2) with the norm still on the device (no host round trip between a Lanczos step and the next
// filter application); left alone when the norm is ~0 (invariant subspace: the host stops the iteration)
__device__ __forceinline__ void d_scale_rsqrt(double* __restrict__ x, int64_t n_pad, const double* __restrict__ nrm2) {
    const int64_t i = (int64_t)blockIdx.x * PF_BLOCK + threadIdx.x;
    const double v = *nrm2;
    if (i < n_pad && v > 1e-280) x[i] *= 1.0 / sqrt(v);
}
__global__ __launch_bounds__(PF_BLOCK) void k_scale_rsqrt(double* __restrict__ x, int64_t n_pad, const double* __restrict__ nrm2) {
    d_scale_rsqrt(x, n_pad, nrm2);
}
struct f_scale_rsqrt {
    static constexpr int BOUNDS = PF_BLOCK;
    static __device__ __forceinline__ void run(double* x, int64_t n_pad, const double* nrm2) { d_scale_rsqrt(x, n_pad, nrm2); }
};

// dst_c = sum_b src_b Y[b][c] for up to 8 output columns per launch (Y row-major m x k, in device memory)
constexpr int COMBINE_COLS = 8;
// (blockIdx.y = 1: the same rotation of a second block of vectors, src_first2 -> dst_first2)
__global__ __launch_bounds__(PF_BLOCK) void k_combine(double* __restrict__ ws, int64_t n_pad, int32_t src_first, int32_t m,
                                                      const double* __restrict__ Y, int32_t k, int32_t c0, int32_t ncols,
                                                      int32_t dst_first, int32_t src_first2, int32_t dst_first2) {
    const int64_t i = (int64_t)blockIdx.x * PF_BLOCK + threadIdx.x;
    if (i >= n_pad) return;
    if (blockIdx.y) src_first = src_first2, dst_first = dst_first2;
    double acc[COMBINE_COLS];
#pragma unroll
    for (int c = 0; c < COMBINE_COLS; ++c) acc[c] = 0.0;
    for (int b = 0; b < m; ++b) {
        const double v = ws[(int64_t)(src_first + b) * n_pad + i];
        const double* yr = Y + (int64_t)b * k + c0;
#pragma unroll
        for (int c = 0; c < COMBINE_COLS; ++c)
            if (c < ncols) acc[c] += v * yr[c];
    }
#pragma unroll
    for (int c = 0; c < COMBINE_COLS; ++c)
        if (c < ncols) ws[(int64_t)(dst_first + c0 + c) * n_pad + i] = acc[c];
}

// the batched forms (pf_gram, pf_resnorms): one launch for all pairs / all vectors
__global__ __launch_bounds__(PF_BLOCK) void k_gram_partial(const double* __restrict__ ws, int64_t n_pad, int32_t first_a, int32_t first_b,
                                                           int32_t count_b, int64_t n_chunks, double* __restrict__ partial) {
    __shared__ double red[PF_BLOCK / PF_WAVE];
    const int p = blockIdx.y;  // pair (i, j): row i of the first block against row j of the second
    const int i = p / count_b, j = p - i * count_b;
    const double* v = ws + (int64_t)(first_b + j) * n_pad;
    const double* w = ws + (int64_t)(first_a + i) * n_pad;
    block_sum_put(chunk_dot(v, w, blockIdx.x, n_pad), red);
    __syncthreads();
    if (threadIdx.x == 0) partial[(int64_t)p * n_chunks + blockIdx.x] = block_sum_get(red);
}

// partial[b][chunk] = |slot ax_first+b - lam[b] slot x_first+b|^2 over the chunk
constexpr int PF_RESNORMS_MAX = 64;
struct LamArgs {
    double lam[PF_RESNORMS_MAX];
};
__global__ __launch_bounds__(PF_BLOCK) void k_resnorms_partial(const double* __restrict__ ws, int64_t n_pad, int32_t ax_first,
                                                               int32_t x_first, LamArgs la, int64_t n_chunks,
                                                               double* __restrict__ partial) {
    __shared__ double red[PF_BLOCK / PF_WAVE];
    const int b = blockIdx.y;
    const double* ax = ws + (int64_t)(ax_first + b) * n_pad;
    const double* x = ws + (int64_t)(x_first + b) * n_pad;
    block_sum_put(chunk_resid2(ax, x, la.lam[b], blockIdx.x, n_pad), red);
    __syncthreads();
    if (threadIdx.x == 0) partial[(int64_t)b * n_chunks + blockIdx.x] = block_sum_get(red);
}

// `count` doubles of device memory to the host behind whatever is queued on the ctx stream, and wait for them: through
// pinned memory and a copy kernel (pf_copy_by_kernel) - a copy COMMAND may queue behind the partner graph's eigenvector
// download on a DMA engine
int small_to_host(pf_graph* g, const double* d_src, double* out, size_t count) {
    pf_ctx* c = g->ctx;
    hipStream_t st = c->stream;
    const size_t bytes = sizeof(double) * count;
    void* pin = nullptr;
    if (bytes <= ((size_t)1 << 16) && pf_pinned_scratch(c, bytes, &pin) == PF_OK) {
        PF_TRY(pf_copy_by_kernel(st, d_src, pin, bytes));
        PF_HIP(hipStreamSynchronize(st));
        memcpy(out, pin, bytes);
        return PF_OK;
    }
    PF_HIP(hipMemcpyAsync(out, d_src, bytes, hipMemcpyDeviceToHost, st));
    PF_HIP(hipStreamSynchronize(st));
    return PF_OK;
}

// the second stage of every reduction here: columns [0, count) of g->partials summed into out[0 .. count), acc[b] (+)= out[b]
int finish_queue(pf_graph* g, int32_t count, double* out, double* acc = nullptr, int accumulate = 0) {
    k_dot_finish<<<(unsigned)count, PF_WAVE, 0, g->ctx->stream>>>(g->partials, g->n_chunks, out, acc, accumulate);
    PF_HIP(hipGetLastError());
    return PF_OK;
}

}  // namespace

int pf_dots_device(pf_graph* g, int32_t w, int32_t first, int32_t count, double* d_out, double* d_acc, int accumulate) {
    hipStream_t st = g->ctx->stream;
    PF_TRY(pf_reduce_ensure(g, count));
    if (pfl::tl_rec) {  // the head of a pair's solve is being recorded: the partner's dot products share the launches
        const dim3 grid((unsigned)g->n_chunks, (unsigned)count);
        pfl::launch<f_dot_partial>(grid, dim3(PF_BLOCK), 0, st, g->ws, g->n_pad, first, w, g->n_chunks, g->partials, -1);
        pfl::launch<f_dot_finish>(dim3((unsigned)count), dim3(PF_WAVE), 0, st, g->partials, g->n_chunks, d_out, d_acc, accumulate);
        return PF_OK;
    }
    PF_TRY(pf_dot_partials(g, w, first, count, g->partials));
    return finish_queue(g, count, d_out, d_acc, accumulate);
}

int pf_dot_partials(pf_graph* g, int32_t w, int32_t first, int32_t count, double* partial) {
    k_dot_partial<<<dim3((unsigned)g->n_chunks, (unsigned)count), PF_BLOCK, 0, g->ctx->stream>>>(g->ws, g->n_pad, first, w, g->n_chunks, partial);
    PF_HIP(hipGetLastError());
    return PF_OK;
}

int pf_scale_rsqrt(pf_graph* g, double* x, const double* nrm2) {
    hipStream_t st = g->ctx->stream;
    if (pfl::tl_rec) pfl::launch<f_scale_rsqrt>(dim3(pf_blocks(g->n_pad)), dim3(PF_BLOCK), 0, st, x, g->n_pad, nrm2);
    else k_scale_rsqrt<<<pf_blocks(g->n_pad), PF_BLOCK, 0, st>>>(x, g->n_pad, nrm2);
    PF_HIP(hipGetLastError());
    return PF_OK;
}

int pf_reduce_ensure(pf_graph* g, int32_t count) {
    if (count > g->partial_cap) {
        pf_free(g->ctx->stream, g->partials);
        g->partials = nullptr;
        const int32_t cap = std::max(count, 64);
        // sized for VecStats partials (48 B) as well as plain doubles
        PF_HIP(pf_malloc(g->ctx->stream, (void**)&g->partials, PF_PARTIAL_BYTES * (size_t)cap * (size_t)(g->n_chunks + 1)));
        g->partial_cap = cap;
    }
    if (count > g->coef_cap) {
        pf_free(g->ctx->stream, g->coef);
        g->coef = nullptr;
        const int32_t cap = std::max(count, 64);
        PF_HIP(pf_malloc(g->ctx->stream, (void**)&g->coef, sizeof(double) * 8 * (size_t)cap));
        g->coef_cap = cap;
    }
    return PF_OK;
}

extern "C" {

int pf_dots(pf_graph* g, int32_t w, int32_t first, int32_t count, double* out) {
    PF_TRY(pf_check_slots(g, w, 1, "pf_dots"));
    PF_TRY(pf_check_slots(g, first, count, "pf_dots"));
    PF_CHECK(out != nullptr, PF_E_ARG, "pf_dots: out is NULL");
    if (count == 0) return PF_OK;
    PF_TRY(pf_reduce_ensure(g, count));  // g->coef must exist before its address is taken
    PF_TRY(pf_dots_device(g, w, first, count, g->coef, nullptr, 0));
    return small_to_host(g, g->coef, out, (size_t)count);
}

int pf_scale(pf_graph* g, int32_t slot, double alpha) {
    PF_TRY(pf_check_slots(g, slot, 1, "pf_scale"));
    k_scale<<<pf_blocks(g->n_pad), PF_BLOCK, 0, g->ctx->stream>>>(pf_slot(g, slot), g->n_pad, alpha);
    PF_HIP(hipGetLastError());
    return PF_OK;
}

int pf_combine(pf_graph* g, int32_t src_first, int32_t m, const double* Y, int32_t k, int32_t dst_first) {
    return pf_combine2(g, src_first, m, Y, k, dst_first, -1, -1);
}

}  // extern "C"

// dst = src Y and, when src_first2 >= 0, dst2 = src2 Y in the same launches (one upload of Y)
int pf_combine2(pf_graph* g, int32_t src_first, int32_t m, const double* Y, int32_t k, int32_t dst_first, int32_t src_first2,
                int32_t dst_first2) {
    PF_TRY(pf_check_slots(g, src_first, m, "pf_combine"));
    PF_TRY(pf_check_slots(g, dst_first, k, "pf_combine"));
    PF_CHECK(Y != nullptr && m > 0 && k > 0, PF_E_ARG, "pf_combine: bad argument");
    PF_CHECK(src_first + m <= dst_first || dst_first + k <= src_first, PF_E_ARG, "pf_combine: overlapping ranges");
    const bool two = src_first2 >= 0;
    if (two) {
        PF_TRY(pf_check_slots(g, src_first2, m, "pf_combine"));
        PF_TRY(pf_check_slots(g, dst_first2, k, "pf_combine"));
        PF_CHECK((src_first2 + m <= dst_first2 || dst_first2 + k <= src_first2) && (dst_first + k <= dst_first2 || dst_first2 + k <= dst_first) &&
                     (src_first + m <= dst_first2 || dst_first2 + k <= src_first) && (src_first2 + m <= dst_first || dst_first + k <= src_first2),
                 PF_E_ARG, "pf_combine: overlapping ranges");
    }
    pf_ctx* ctx = g->ctx;
    hipStream_t st = ctx->stream;
    Scratch sc(st);
    double* dY = sc.get<double>((size_t)m * k);
    PF_HIP(sc.err);
    // Y goes through one of a few pinned staging slots, so that the call need not wait for the copy (a synchronisation costs
    // 30-50 us of idle device, and the tail of a solve has three of these calls); a slot is reused only after the copy
    // that read it last has completed
    const size_t bytes = sizeof(double) * (size_t)m * k;
    const void* src = Y;
    bool staged = false;
    if (bytes <= PF_STAGE_BYTES) {
        if (!ctx->stage_ring) {
            if (hipHostMalloc(&ctx->stage_ring, (size_t)PF_STAGE_SLOTS * PF_STAGE_BYTES, hipHostMallocDefault) != hipSuccess) {
                (void)hipGetLastError();
                ctx->stage_ring = nullptr;
            } else {
                for (int i = 0; i < PF_STAGE_SLOTS; ++i) ctx->stage_ev[i] = nullptr;
            }
        }
        if (ctx->stage_ring) {
            const int slot = ctx->stage_next;
            ctx->stage_next = (slot + 1) % PF_STAGE_SLOTS;
            bool ok = true;
            if (!ctx->stage_ev[slot]) ok = hipEventCreateWithFlags(&ctx->stage_ev[slot], hipEventDisableTiming) == hipSuccess;
            else ok = hipEventSynchronize(ctx->stage_ev[slot]) == hipSuccess;
            if (ok) {
                void* dst = static_cast<unsigned char*>(ctx->stage_ring) + (size_t)slot * PF_STAGE_BYTES;
                memcpy(dst, Y, bytes);
                src = dst;
                staged = true;
                hipError_t es = hipMemcpyAsync(dY, src, bytes, hipMemcpyHostToDevice, st);
                if (es == hipSuccess) es = hipEventRecord(ctx->stage_ev[slot], st);
                PF_HIP(es);
            } else {
                (void)hipGetLastError();
            }
        }
    }
    if (!staged) sc.upload(dY, Y, (size_t)m * k);
    for (int32_t c0 = 0; c0 < k && sc.ok(); c0 += COMBINE_COLS) {
        const int32_t nc = std::min(COMBINE_COLS, k - c0);
        k_combine<<<dim3(pf_blocks(g->n_pad), two ? 2u : 1u), PF_BLOCK, 0, st>>>(g->ws, g->n_pad, src_first, m, dY, k, c0, nc, dst_first, src_first2,
                                                                          dst_first2);
        sc.launched();
    }
    const hipError_t e2 = staged ? hipSuccess : hipStreamSynchronize(st);  // (not staged: Y is the caller's host buffer)
    PF_HIP(sc.err);
    PF_HIP(e2);
    return PF_OK;
}

// The queueing half of pf_gram / pf_gram_begin and of pf_resnorms / pf_resnorms_begin: the checks (args_ok: what the caller
// found of the arguments that are its own), the partial sums and their finish into g->coef.
static int gram_queue(pf_graph* g, int32_t first_a, int32_t count_a, int32_t first_b, int32_t count_b, bool args_ok) {
    PF_TRY(pf_check_slots(g, first_a, count_a, "pf_gram"));
    PF_TRY(pf_check_slots(g, first_b, count_b, "pf_gram"));
    PF_CHECK(args_ok && count_a > 0 && count_b > 0, PF_E_ARG, "pf_gram: bad argument");
    PF_TRY(pf_reduce_ensure(g, count_a * count_b));  // partials: one column per pair
    k_gram_partial<<<dim3((unsigned)g->n_chunks, (unsigned)(count_a * count_b)), PF_BLOCK, 0, g->ctx->stream>>>(
        g->ws, g->n_pad, first_a, first_b, count_b, g->n_chunks, g->partials);
    PF_HIP(hipGetLastError());
    return finish_queue(g, count_a * count_b, g->coef);
}

static int resnorms_queue(pf_graph* g, int32_t ax_first, int32_t x_first, const double* lam, int32_t count, bool args_ok) {
    PF_TRY(pf_check_slots(g, ax_first, count, "pf_resnorms"));
    PF_TRY(pf_check_slots(g, x_first, count, "pf_resnorms"));
    PF_CHECK(args_ok && lam != nullptr && count > 0, PF_E_ARG, "pf_resnorms: bad argument");
    hipStream_t st = g->ctx->stream;
    PF_TRY(pf_reduce_ensure(g, count));
    for (int32_t at = 0; at < count; at += PF_RESNORMS_MAX) {
        const int32_t nb = std::min(count - at, PF_RESNORMS_MAX);
        LamArgs la{};
        for (int32_t i = 0; i < nb; ++i) la.lam[i] = lam[at + i];
        k_resnorms_partial<<<dim3((unsigned)g->n_chunks, (unsigned)nb), PF_BLOCK, 0, st>>>(g->ws, g->n_pad, ax_first + at, x_first + at, la,
                                                                                        g->n_chunks, g->partials);
        PF_HIP(hipGetLastError());
        PF_TRY(finish_queue(g, nb, g->coef + at));
    }
    return PF_OK;
}

extern "C" {

int pf_gram(pf_graph* g, int32_t first_a, int32_t count_a, int32_t first_b, int32_t count_b, double* out) {
    PF_TRY(gram_queue(g, first_a, count_a, first_b, count_b, out != nullptr));
    return small_to_host(g, g->coef, out, (size_t)count_a * count_b);
}

// (one vector: the batched kernels with a count of one)
int pf_resnorm(pf_graph* g, int32_t ax, int32_t x, double lam, double* out) {
    PF_TRY(pf_check_slots(g, ax, 1, "pf_resnorm"));
    PF_TRY(pf_check_slots(g, x, 1, "pf_resnorm"));
    PF_CHECK(out != nullptr, PF_E_ARG, "pf_resnorm: out is NULL");
    PF_TRY(resnorms_queue(g, ax, x, &lam, 1, true));
    hipStream_t st = g->ctx->stream;
    double r2 = 0.0;
    PF_HIP(hipMemcpyAsync(&r2, g->coef, sizeof(double), hipMemcpyDeviceToHost, st));
    PF_HIP(hipStreamSynchronize(st));
    *out = sqrt(r2 > 0.0 ? r2 : 0.0);
    return PF_OK;
}

int pf_resnorms(pf_graph* g, int32_t ax_first, int32_t x_first, const double* lam, int32_t count, double* out) {
    PF_TRY(resnorms_queue(g, ax_first, x_first, lam, count, out != nullptr));
    PF_TRY(small_to_host(g, g->coef, out, (size_t)count));
    for (int32_t i = 0; i < count; ++i) out[i] = sqrt(out[i] > 0.0 ? out[i] : 0.0);
    return PF_OK;
}

}  // extern "C"

// pf_gram / pf_resnorms in two halves: _begin queues the kernels and a copy of the few results into a pinned block of the
// graph's own, with an event behind it; pf_small_end waits for that event only - what the stream holds behind it (the
// partner graph's extraction) keeps running.  One collection in flight per graph.
static int small_begin(pf_graph* g, const double* d_src, size_t count, bool root, bool append = false) {
    PF_CHECK(append ? g->small_pending > 0 && !g->small_root && !root : g->small_pending == 0, PF_E_STATE,
             "pf_gram_begin / pf_resnorms_begin: a previous result has not been collected");
    pf_ctx* c = g->ctx;
    hipStream_t st = c->stream;
    const size_t offset = append ? (size_t)g->small_pending : 0;
    if (append) {
        PF_CHECK((int64_t)(offset + count) <= g->small_land.cap, PF_E_STATE, "pf_gram_begin: no room to append");
    } else {  // (room for an appended block of the same size; an outgrown block may still be written to: drained first)
        PF_HIP(g->small_land.ensure(c->pools, (int32_t)(2 * count), 128, st));
    }
    PF_TRY(pf_copy_by_kernel(st, d_src, g->small_land.host + offset, sizeof(double) * count));
    PF_HIP(hipEventRecord(g->small_land.ev, st));
    g->small_pending = (int32_t)(offset + count);
    g->small_root = root;
    return PF_OK;
}

int pf_small_end(pf_graph* g, double* out) {
    PF_CHECK(g != nullptr && out != nullptr && g->small_pending > 0, PF_E_STATE, "pf_small_end: nothing to collect");
    PF_HIP(hipEventSynchronize(g->small_land.ev));
    const int32_t count = g->small_pending;
    g->small_pending = 0;
    for (int32_t i = 0; i < count; ++i) {
        const double v = g->small_land.host[i];
        out[i] = g->small_root ? sqrt(v > 0.0 ? v : 0.0) : v;
    }
    return PF_OK;
}

// (append: the result goes behind the one already waiting - of the same size at most - and pf_small_end returns both)
int pf_gram_begin(pf_graph* g, int32_t first_a, int32_t count_a, int32_t first_b, int32_t count_b, int32_t append) {
    PF_TRY(gram_queue(g, first_a, count_a, first_b, count_b, true));
    return small_begin(g, g->coef, (size_t)count_a * count_b, false, append != 0);
}

int pf_resnorms_begin(pf_graph* g, int32_t ax_first, int32_t x_first, const double* lam, int32_t count) {
    PF_TRY(resnorms_queue(g, ax_first, x_first, lam, count, true));
    return small_begin(g, g->coef, (size_t)count, true);
}
