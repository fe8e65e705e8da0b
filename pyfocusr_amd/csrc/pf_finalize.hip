// The end of a solve: the statistics of the Ritz vectors (VecStats), their scaling, sign and min-max into the resident
// [n][count] block in mesh order (pf_finalize_vectors_*), eigsort's remapped image of it (pf_final_remap_begin), the
// downloads of both - owed, released behind the next long kernel, collected by pf_finalize_vectors_end - and sampled rows
// of resident blocks (pf_final_rows, pf_point_rows).
#include <math.h>
#include <stdlib.h>

#include <algorithm>
#include <mutex>

#include "pf_internal.h"

namespace {

// ---- eigenvector post-processing -----------------------------------------------------------------
struct VecStats {
    double sumsq, vmin, vmax, absmax, at_absmax;
    int64_t arg;
};
static_assert(sizeof(VecStats) == PF_PARTIAL_BYTES, "pf_reduce_ensure sizes g->partials for VecStats");

__device__ __forceinline__ void stats_merge(VecStats& a, const VecStats& b) {
    a.sumsq += b.sumsq;
    a.vmin = fmin(a.vmin, b.vmin);
    a.vmax = fmax(a.vmax, b.vmax);
    if (b.absmax > a.absmax || (b.absmax == a.absmax && b.arg < a.arg)) {
        a.absmax = b.absmax;
        a.at_absmax = b.at_absmax;
        a.arg = b.arg;
    }
}

__device__ __forceinline__ VecStats stats_shfl(const VecStats& v, int off) {
    VecStats o;
    o.sumsq = __shfl_down(v.sumsq, off, PF_WAVE);
    o.vmin = __shfl_down(v.vmin, off, PF_WAVE);
    o.vmax = __shfl_down(v.vmax, off, PF_WAVE);
    o.absmax = __shfl_down(v.absmax, off, PF_WAVE);
    o.at_absmax = __shfl_down(v.at_absmax, off, PF_WAVE);
    o.arg = __shfl_down(v.arg, off, PF_WAVE);
    return o;
}

__global__ __launch_bounds__(PF_BLOCK) void k_vec_stats_partial(const double* __restrict__ ws, int64_t n_pad, int64_t n,
                                                                int32_t first, const double* __restrict__ sg,
                                                                const int32_t* __restrict__ perm, const int32_t* __restrict__ perm_m,
                                                                int32_t from_sym, int64_t n_chunks, VecStats* __restrict__ partial) {
    __shared__ VecStats red[PF_BLOCK / PF_WAVE];
    const int b = blockIdx.y;
    const double* x = ws + (int64_t)(first + b) * n_pad;
    const int64_t lo = (int64_t)blockIdx.x * PF_DOT_CHUNK;
    const int64_t hi0 = lo + PF_DOT_CHUNK;
    const int64_t hi = hi0 < n ? hi0 : n;
    VecStats st{0.0, INFINITY, -INFINITY, -1.0, 0.0, (int64_t)1 << 62};
    for (int64_t r = lo + threadIdx.x; r < hi; r += PF_BLOCK) {
        const int64_t i = perm[r];  // mesh-order index: the tie-break key of the sign convention
        double v = x[r];
        if (from_sym) v *= sg[perm_m[r]];  // (per-vertex arrays live in m-space)
        VecStats e{v * v, v, v, fabs(v), v, i};
        stats_merge(st, e);
    }
#pragma unroll
    for (int off = PF_WAVE / 2; off > 0; off >>= 1) {
        VecStats o = stats_shfl(st, off);
        stats_merge(st, o);
    }
    if ((threadIdx.x & (PF_WAVE - 1)) == 0) red[threadIdx.x / PF_WAVE] = st;
    __syncthreads();
    if (threadIdx.x == 0) {
        VecStats t = red[0];
        stats_merge(t, red[1]);
        stats_merge(t, red[2]);
        stats_merge(t, red[3]);
        partial[(int64_t)b * n_chunks + blockIdx.x] = t;
    }
}

__global__ __launch_bounds__(PF_WAVE) void k_vec_stats_finish(const VecStats* __restrict__ partial, int64_t n_chunks,
                                                              VecStats* __restrict__ out) {
    const int b = blockIdx.x;
    VecStats st{0.0, INFINITY, -INFINITY, -1.0, 0.0, (int64_t)1 << 62};
    for (int64_t k = threadIdx.x; k < n_chunks; k += PF_WAVE) stats_merge(st, partial[(int64_t)b * n_chunks + k]);
#pragma unroll
    for (int off = PF_WAVE / 2; off > 0; off >>= 1) {
        VecStats o = stats_shfl(st, off);
        stats_merge(st, o);
    }
    if (threadIdx.x == 0) out[b] = st;
}

// params[c] = {scale, vmin, vmax - vmin, shift} of vector c from its statistics (what pf_finalize_vectors documents:
// unit 2-norm, the largest-|entry| positive, min-max to [-0.5, 0.5] if asked)
__global__ void k_vec_params(const VecStats* __restrict__ fin, int32_t count, int32_t minmax, double* __restrict__ params) {
    for (int c = threadIdx.x; c < count; c += blockDim.x) {
        const VecStats s = fin[c];
        const double sgn = s.at_absmax < 0.0 ? -1.0 : 1.0;
        const double scale = sgn / sqrt(s.sumsq);
        const double vmin = (sgn > 0 ? s.vmin : s.vmax) * scale;  // monotone map: exact min/max of the scaled vector
        const double vmax = (sgn > 0 ? s.vmax : s.vmin) * scale;
        params[4 * c + 0] = scale;
        params[4 * c + 1] = minmax ? vmin : 0.0;
        params[4 * c + 2] = minmax ? (vmax - vmin) : 0.0;
        params[4 * c + 3] = minmax ? 0.5 : 0.0;
    }
}

// out[i][c] = (x_c[i] * scale_c - off_c) * inv_c - half_c       (row-major n x count)
__global__ __launch_bounds__(PF_BLOCK) void k_vec_apply(const double* __restrict__ ws, int64_t n_pad, int64_t n,
                                                        int32_t first, int32_t count, const double* __restrict__ sg,
                                                        const int32_t* __restrict__ iperm, const int32_t* __restrict__ mrank,
                                                        int32_t from_sym, const double* __restrict__ params, double* __restrict__ out) {
    const int64_t i = (int64_t)blockIdx.x * PF_BLOCK + threadIdx.x;
    if (i >= n) return;
    const int64_t r = iperm[i];
    const double s = from_sym ? sg[mrank ? mrank[i] : i] : 1.0;
    for (int c = 0; c < count; ++c) {
        const double scale = params[4 * c + 0], off = params[4 * c + 1], ptp = params[4 * c + 2], half = params[4 * c + 3];
        double v = (ws[(int64_t)(first + c) * n_pad + r] * s) * scale;
        if (ptp != 0.0) v = (v - off) / ptp - half;  // graph.py:254-257
        out[i * count + c] = v;
    }
}

// out[t][c] = final[rows[t]][c]: sampled rows of the resident eigenvector block (graph.py:266-267 on the device)
__global__ __launch_bounds__(PF_BLOCK) void k_final_rows(const double* __restrict__ fin, const int64_t* __restrict__ rows, int64_t n_rows,
                                                         int32_t fc, double* __restrict__ out) {
    const int64_t e = (int64_t)blockIdx.x * PF_BLOCK + threadIdx.x;
    if (e >= n_rows * fc) return;
    const int64_t t = e / fc;
    out[e] = fin[rows[t] * fc + (e - t * fc)];
}

}  // namespace

extern "C" {

// The eigenvector post-processing in two halves, so that the n x count download (10 MB per 250k-vertex graph) leaves the
// critical path: _begin queues the kernels on the ctx stream and the copies on the ctx's COPY stream behind an event -
// later work on the ctx stream (eigsort's cost matrices, the KNN, the partner graph's solve) overlaps with them - and
// _end waits for the copies and checks the statistics.  The block itself is resident and usable on the device as soon as
// _begin returns.  `out` should be pinned memory (pf_host_alloc): a pageable destination is staged in chunks by the
// runtime (measured: ~12 gaps of 82 us per 250k pair).
static bool downloads_deferred() {
    static const bool on = [] { const char* v = getenv("PF_DOWNLOAD_DEFER"); return !(v && v[0] == '0'); }();
    return on;
}

// the owed image of g goes onto the copy stream, behind everything the ctx stream holds at this moment
static int queue_download(pf_graph* g) {
    pf_ctx* ctx = g->ctx;
    const double* src = nullptr;
    {
        std::lock_guard<std::mutex> lk(ctx->deferred_mutex);
        auto it = std::find(ctx->deferred.begin(), ctx->deferred.end(), g);
        if (it != ctx->deferred.end()) ctx->deferred.erase(it);
        src = g->dl_src;
        g->dl_src = nullptr;
    }
    if (!src) return PF_OK;
    PF_HIP(hipEventRecord(g->final_land.ev, ctx->stream));
    PF_HIP(hipStreamWaitEvent(ctx->copy_stream, g->final_land.ev, 0));
    // (the runtime's copy: a download kernel of our own with a few blocks, at the copy stream's low priority, only got CUs
    // when the search had finished - KNN stage 1.50 ms instead of 1.20)
    PF_HIP(hipMemcpyAsync(g->dl_dst, src, g->dl_bytes, hipMemcpyDeviceToHost, ctx->copy_stream));
    PF_HIP(hipEventRecord(g->final_done, ctx->copy_stream));
    return PF_OK;
}

// the [n][count] image at src is owed to the caller's out from here on: held back until pf_downloads_release or whoever
// collects it first, or - PF_DOWNLOAD_DEFER=0 - queued at once
static int owe_download(pf_graph* g, const double* src, double* out, int32_t count) {
    pf_ctx* ctx = g->ctx;
    g->dl_src = src;
    g->dl_dst = out;
    g->dl_bytes = sizeof(double) * (size_t)g->n * count;
    if (downloads_deferred()) {
        std::lock_guard<std::mutex> lk(ctx->deferred_mutex);
        if (std::find(ctx->deferred.begin(), ctx->deferred.end(), g) == ctx->deferred.end()) ctx->deferred.push_back(g);
        return PF_OK;
    }
    return queue_download(g);
}

// forget the image owed to the caller's buffer (never queued: nothing will be written), or wait for the one in flight;
// the resident block on the device stays usable.  For callers that are about to report a failure.
extern "C++" int pf_download_cancel(pf_graph* g) {
    pf_ctx* ctx = g->ctx;
    bool owed = false;
    {
        std::lock_guard<std::mutex> lk(ctx->deferred_mutex);
        auto it = std::find(ctx->deferred.begin(), ctx->deferred.end(), g);
        if (it != ctx->deferred.end()) ctx->deferred.erase(it);
        owed = g->dl_src != nullptr;
        g->dl_src = nullptr;
    }
    if (g->final_pending != 0) {
        g->final_pending = 0;
        g->final_check = 0;
        if (!owed) (void)hipEventSynchronize(g->final_done);
        pf_free(ctx->stream, g->final_params);
        g->final_params = nullptr;
        pf_free(ctx->stream, g->final_tmp);
        g->final_tmp = nullptr;
    }
    return PF_OK;
}

extern "C++" int pf_downloads_release(pf_ctx* c) {
    for (;;) {
        pf_graph* g = nullptr;
        {
            std::lock_guard<std::mutex> lk(c->deferred_mutex);
            if (c->deferred.empty()) break;
            g = c->deferred.back();
        }
        PF_TRY(queue_download(g));
    }
    return PF_OK;
}

int pf_finalize_vectors_begin(pf_graph* g, int32_t first, int32_t count, int32_t from_sym, int32_t minmax, double* out) {
    PF_TRY(pf_check_slots(g, first, count, "pf_finalize_vectors"));
    PF_CHECK(out != nullptr && count > 0, PF_E_ARG, "pf_finalize_vectors: bad argument");
    PF_CHECK(!from_sym || g->is_symmetric, PF_E_ARG, "pf_finalize_vectors: from_sym on an asymmetric graph");
    PF_TRY(pf_finalize_vectors_end(g));  // an earlier result still on its way
    pf_ctx* ctx = g->ctx;
    hipStream_t st = ctx->stream;
    if (!ctx->copy_stream) PF_HIP(pf_create_side_stream(&ctx->copy_stream, true));
    // events and the pinned landing place of the statistics come from the ctx's pools (what freed graphs left behind:
    // hipHostMalloc / hipHostFree and event creation cost 0.1-0.2 ms each)
    // (the statistics use the two spare doubles of a block as well, and any pooled block that holds them will do: no floor
    // but for a new one; pf_finalize_vectors_end above has collected whatever was on its way into the block held)
    const int32_t stat_doubles = (int32_t)(sizeof(VecStats) / sizeof(double)) * count;
    PF_HIP(g->final_land.ensure(ctx->pools, stat_doubles - 2, 0, nullptr, std::max(stat_doubles, 384)));
    PF_HIP(ctx->pools.take_event(&g->final_done));
    PF_TRY(pf_reduce_ensure(g, count));
    VecStats* part = reinterpret_cast<VecStats*>(g->partials);
    VecStats* fin = part + (size_t)count * g->n_chunks;
    dim3 grid((unsigned)g->n_chunks, (unsigned)count);
    k_vec_stats_partial<<<grid, PF_BLOCK, 0, st>>>(g->ws, g->n_pad, g->n, first, g->sg, g->perm, g->perm_m, from_sym, g->n_chunks, part);
    PF_HIP(hipGetLastError());
    k_vec_stats_finish<<<(unsigned)count, PF_WAVE, 0, st>>>(part, g->n_chunks, fin);
    PF_HIP(hipGetLastError());
    // scale / sign / min-max parameters straight from the statistics, on the device (no read-back in between: the
    // statistics come to the host with the result and are checked then)
    double *d_params = nullptr, *d_out = nullptr;
    pf_free(st, g->final_vecs);  // the result stays resident (pf_final_rows, pf_knn1_graphs) until the next call
    g->final_vecs = nullptr;
    g->final_count = 0;
    // parameters, and a copy of the statistics that later reductions on the ctx stream cannot overwrite
    PF_HIP(pf_malloc(st, (void**)&d_params, sizeof(double) * 4 * (size_t)count + sizeof(VecStats) * (size_t)count));
    VecStats* d_stats = reinterpret_cast<VecStats*>(d_params + 4 * (size_t)count);
    hipError_t e = pf_malloc(st, (void**)&d_out, sizeof(double) * (size_t)g->n * count);
    if (e == hipSuccess) {
        k_vec_params<<<1, PF_WAVE, 0, st>>>(fin, count, minmax, d_params);
        k_vec_apply<<<pf_blocks(g->n), PF_BLOCK, 0, st>>>(g->ws, g->n_pad, g->n, first, count, g->sg, g->iperm, g->mrank, from_sym, d_params, d_out);
        e = hipGetLastError();
    }
    if (e == hipSuccess) e = hipMemcpyAsync(d_stats, fin, sizeof(VecStats) * count, hipMemcpyDeviceToDevice, st);
    if (e == hipSuccess) e = hipEventRecord(g->final_land.ev, st);
    if (e == hipSuccess) e = hipStreamWaitEvent(ctx->copy_stream, g->final_land.ev, 0);
    if (e == hipSuccess) e = hipMemcpyAsync(g->final_land.host, d_stats, sizeof(VecStats) * count, hipMemcpyDeviceToHost, ctx->copy_stream);
    if (e == hipSuccess) e = hipEventRecord(g->final_done, ctx->copy_stream);
    if (e != hipSuccess) {
        (void)hipStreamSynchronize(ctx->copy_stream);
        pf_free(st, d_params);
        pf_free(st, d_out);
        PF_HIP(e);
    }
    g->final_vecs = d_out;
    g->final_count = count;
    g->final_params = d_params;
    g->final_pending = count;
    g->final_check = count;
    // The n x count image itself is OWED, not queued: while a 10 MB download runs, the next kernel boundary of the ctx
    // stream waits for it to drain (kernel trace: the partner's k_vec_params, eigsort's k_es_minmax and the search's first
    // kernel each took the download's 180 us) - beside small dependent kernels a download costs what it would cost in
    // line.  It leaves behind the next LONG kernel (pf_downloads_release: the 1-NN search), or when somebody collects it.
    return owe_download(g, d_out, out, count);
}

int pf_finalize_vectors_end(pf_graph* g) {
    PF_CHECK(g != nullptr, PF_E_ARG, "pf_finalize_vectors_end: NULL graph");
    if (g->final_pending == 0) return PF_OK;
    g->final_pending = 0;
    const int32_t count = g->final_check;
    g->final_check = 0;
    int rc = queue_download(g);  // (nobody released it: now)
    const hipError_t e = hipEventSynchronize(g->final_done);
    pf_free(g->ctx->stream, g->final_params);
    g->final_params = nullptr;
    pf_free(g->ctx->stream, g->final_tmp);
    g->final_tmp = nullptr;
    PF_TRY(rc);
    if (count <= 0) {  // only a remapped image of a block whose statistics have been looked at
        PF_HIP(e);
        return PF_OK;
    }
    const VecStats* hs = reinterpret_cast<const VecStats*>(g->final_land.host);
    bool sane = e == hipSuccess;
    int32_t bad = 0;
    for (int32_t c = 0; c < count && sane; ++c)
        if (!(hs[c].sumsq > 0.0 && isfinite(hs[c].sumsq))) sane = false, bad = c;
    if (!sane) {
        pf_free(g->ctx->stream, g->final_vecs);
        g->final_vecs = nullptr;
        g->final_count = 0;
    }
    PF_HIP(e);
    PF_CHECK(sane, PF_E_STATE, "pf_finalize_vectors: vector %d has norm^2 %g", bad, hs[(size_t)bad].sumsq);
    return PF_OK;
}

int pf_finalize_vectors(pf_graph* g, int32_t first, int32_t count, int32_t from_sym, int32_t minmax, double* out) {
    PF_TRY(pf_finalize_vectors_begin(g, first, count, from_sym, minmax, out));
    return pf_finalize_vectors_end(g);
}

struct RemapArgs {
    int32_t col[64];
    double sign[64];
};
__global__ __launch_bounds__(PF_BLOCK) void k_final_remap(const double* __restrict__ fin, int64_t n, int32_t fc, int32_t count, RemapArgs m,
                                                          double* __restrict__ out) {
    const int64_t e = (int64_t)blockIdx.x * PF_BLOCK + threadIdx.x;
    if (e >= n * count) return;
    const int64_t i = e / count;
    const int32_t c = (int32_t)(e - i * count);
    out[e] = fin[i * fc + m.col[c]] * m.sign[c];  // (sign = +-1: exact)
}

// eigsort's sign flips and column moves (eigsort.py:108-122) applied to the resident block's image on the host:
// out[i][c] = block[i][col[c]] * sign[c], computed on the device and copied on the copy stream - O(n k) strided host
// work (0.25 ms at 250k x 5, several ms at 1M x 10) becomes one DMA that overlaps with the KNN.  Collected by
// pf_finalize_vectors_end like the first download; the resident block itself is unchanged.
int pf_final_remap_begin(pf_graph* g, const int32_t* col, const double* sign, int32_t count, double* out) {
    PF_CHECK(g && col && sign && out, PF_E_ARG, "pf_final_remap_begin: NULL argument");
    // An image that is still owed to the same array is simply replaced by the remapped one (its statistics are looked at
    // when that is collected); one that is in flight, or owed to another array, is collected first.
    if (!(g->dl_src && g->dl_dst == out)) PF_TRY(pf_finalize_vectors_end(g));
    PF_CHECK(g->final_vecs != nullptr, PF_E_STATE, "pf_final_remap_begin: no pf_finalize_vectors result is resident");
    PF_CHECK(count >= 1 && count <= 64 && count <= g->final_count, PF_E_ARG, "pf_final_remap_begin: count %d out of range", count);
    RemapArgs m{};
    for (int32_t c = 0; c < count; ++c) {
        PF_CHECK(col[c] >= 0 && col[c] < g->final_count, PF_E_ARG, "pf_final_remap_begin: column %d out of range", col[c]);
        m.col[c] = col[c];
        m.sign[c] = sign[c];
    }
    pf_ctx* ctx = g->ctx;
    hipStream_t st = ctx->stream;
    PF_CHECK(ctx->copy_stream && g->final_land.ev && g->final_done, PF_E_STATE, "pf_final_remap_begin: no download machinery (call after pf_finalize_vectors_begin)");
    double* d_tmp = nullptr;
    PF_HIP(pf_malloc(st, (void**)&d_tmp, sizeof(double) * (size_t)g->n * count));
    k_final_remap<<<pf_blocks(g->n * count), PF_BLOCK, 0, st>>>(g->final_vecs, g->n, g->final_count, count, m, d_tmp);
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) {
        pf_free(st, d_tmp);
        PF_HIP(e);
    }
    pf_free(st, g->final_tmp);  // (an earlier remapped image that was never sent: behind its last use in stream order)
    g->final_tmp = d_tmp;
    g->final_pending = count;
    return owe_download(g, d_tmp, out, count);
}

// out[t][c] = src[rows[t]][c] for a resident [n][width] block of the graph
static int rows_to_host(pf_graph* g, const double* src, int32_t width, const int64_t* rows, int64_t n_rows, double* out,
                        const char* who) {
    if (n_rows == 0) return PF_OK;
    PF_HIP(hipSetDevice(g->ctx->device));
    hipStream_t st = g->ctx->stream;
    for (int64_t i = 0; i < n_rows; ++i)
        PF_CHECK(rows[i] >= 0 && rows[i] < g->n, PF_E_ARG, "%s: row %lld out of range", who, (long long)rows[i]);
    Scratch sc(st);
    int64_t* d_rows = sc.get<int64_t>((size_t)n_rows);
    PF_HIP(sc.err);  // (nothing queued yet: no wait)
    double* d_out = sc.get<double>((size_t)n_rows * width);
    sc.upload(d_rows, rows, (size_t)n_rows);
    if (sc.ok()) {
        k_final_rows<<<pf_blocks(n_rows * width), PF_BLOCK, 0, st>>>(src, d_rows, n_rows, width, d_out);
        sc.launched();
    }
    sc.download(out, d_out, (size_t)n_rows * width);
    const hipError_t e2 = hipStreamSynchronize(st);  // (whatever failed: the copies queued so far read or write the caller's arrays)
    PF_HIP(sc.err);
    PF_HIP(e2);
    return PF_OK;
}

int pf_final_rows(pf_graph* g, const int64_t* rows, int64_t n_rows, double* out) {
    PF_CHECK(g != nullptr && rows != nullptr && out != nullptr && n_rows >= 0, PF_E_ARG, "pf_final_rows: bad argument");
    PF_CHECK(g->final_vecs != nullptr, PF_E_STATE, "pf_final_rows: no pf_finalize_vectors result is resident");
    return rows_to_host(g, g->final_vecs, g->final_count, rows, n_rows, out, "pf_final_rows");
}

int pf_point_rows(pf_graph* g, const int64_t* rows, int64_t n_rows, double* out) {
    PF_CHECK(g != nullptr && rows != nullptr && out != nullptr && n_rows >= 0, PF_E_ARG, "pf_point_rows: bad argument");
    PF_CHECK(g->pts != nullptr, PF_E_STATE, "pf_point_rows: this graph was not built from a mesh");
    return rows_to_host(g, g->pts, 3, rows, n_rows, out, "pf_point_rows");
}

}  // extern "C"
