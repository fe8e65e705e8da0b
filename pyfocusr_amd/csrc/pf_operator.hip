// Eigensolver kernels, the operator's unit: the fused SpMV + Chebyshev three-term recurrence over the SELL-64
// operator storage (one step per launch here; the whole recurrence in one resident launch is pf_persist.hip's), the
// workspace of slots the solve's vectors live in, and its start and null vectors.  The dense-vector kernels of the
// Krylov-Schur driver have units of their own: pf_orth.hip (Gram-Schmidt step), pf_reduce.hip (dot products, Gram
// matrices, residual norms, basis rotation), pf_finalize.hip (eigenvector post-processing and downloads), pf_rows.hip
// (mean filter, row sets of the row-partitioned solve).
//
// These replace the ARPACK/SuperLU machinery behind `scipy.sparse.linalg.eigs(L, k,
// sigma=1e-10, which="LM", ncv=4k)` (pyfocusr/graph.py:372 of the reference).  Everything here
// is HBM/L2-bandwidth-bound: one thread per matrix row, 64 consecutive rows per wave reading
// 64 consecutive SELL entries per step (512 B of values + 256 B of column indices per wave
// instruction), x gathered through L2.  Reductions are two-stage and atomic-free, so results
// are bitwise reproducible run to run.
#include <math.h>

#include <algorithm>

#include "pf_internal.h"
#include "pf_launch.h"

namespace {

// tuning knobs of the operator kernel (tools/tune_spmv.sh builds variants with -D...)
#ifndef PF_OP_BLOCK
#define PF_OP_BLOCK 256
#endif
// out = alpha * (shift * x - A x) - beta * prev          (A = diag + SELL off-diagonals)
//   SpMV:            alpha = -1, shift = 0, beta = 0      -> out = A x
//   Chebyshev k = 1: alpha = 1/e, shift = c, beta = 0
//   Chebyshev k > 1: alpha = 2/e, shift = c, beta = 1     (out may alias prev)
struct OpArgs {
    const int64_t* slice_ptr;
    const int32_t* scol;
    const double* sval;
    const double* diag;
    const double* x;
    const double* prev;
    double* out;
    double alpha, shift, beta;
    unsigned n_blocks;  // multiple of 8
};

template <bool HAS_PREV>
__device__ __forceinline__ void sell_op_block(const OpArgs& a, unsigned bid) {
#pragma clang fp contract(fast)
    // Blocks are dealt round-robin over the 8 XCDs (private 4 MiB L2 each).  Give every XCD one
    // contiguous eighth of the (Morton-ordered) rows: its slice of the matrix (~2.6 MB at 250k
    // vertices) and of x then stays in its own L2 from one launch to the next.  n_blocks is a
    // multiple of 8 (n_pad is a multiple of 8 * PF_BLOCK); placement affects speed only.
    const unsigned per_xcd = a.n_blocks >> 3;
    const unsigned blk = (bid & 7u) * per_xcd + (bid >> 3);
    const int64_t row = (int64_t)blk * PF_OP_BLOCK + threadIdx.x;
    const int64_t s = row >> 6;
    const int lane = threadIdx.x & (PF_WAVE - 1);
    const int64_t base = a.slice_ptr[s];
    const int width = (int)((a.slice_ptr[s + 1] - base) >> 6);
    const double* __restrict__ x = a.x;
    const double xi = x[row];
    double acc = a.diag[row] * xi;
    // pairs of entries per lane (pf_sell_index): one 16-byte load of two values + one 8-byte load of two columns
    const int pairs = width >> 1;
    const double2* __restrict__ vp2 = reinterpret_cast<const double2*>(a.sval + base) + lane;
    const int2* __restrict__ cp2 = reinterpret_cast<const int2*>(a.scol + base) + lane;
    int j = 0;
    for (; j + 2 <= pairs; j += 2) {
        const int2 c0 = cp2[(int64_t)(j + 0) * PF_WAVE], c1 = cp2[(int64_t)(j + 1) * PF_WAVE];
        const double2 v0 = vp2[(int64_t)(j + 0) * PF_WAVE], v1 = vp2[(int64_t)(j + 1) * PF_WAVE];
        const double x0 = x[c0.x], x1 = x[c0.y], x2 = x[c1.x], x3 = x[c1.y];
        acc += v0.x * x0;
        acc += v0.y * x1;
        acc += v1.x * x2;
        acc += v1.y * x3;
    }
    for (; j < pairs; ++j) {
        const int2 c0 = cp2[(int64_t)j * PF_WAVE];
        const double2 v0 = vp2[(int64_t)j * PF_WAVE];
        acc += v0.x * x[c0.x];
        acc += v0.y * x[c0.y];
    }
    if (width & 1) {
        const int64_t t = base + (int64_t)pairs * (2 * PF_WAVE) + lane;
        acc += a.sval[t] * x[a.scol[t]];
    }
    double r = a.alpha * (a.shift * xi - acc);
    if (HAS_PREV) r -= a.beta * a.prev[row];
    a.out[row] = r;
}

template <bool HAS_PREV>
__global__ __launch_bounds__(PF_OP_BLOCK) void k_sell_op(OpArgs a) {
    sell_op_block<HAS_PREV>(a, blockIdx.x);
}

// the plain product for `gridDim.y` consecutive workspace slots in one launch (the Rayleigh-Ritz tail of a solve: S Z for
// the 6-11 Ritz vectors was one launch per vector, each mostly launch latency): block row y takes slot y
__global__ __launch_bounds__(PF_OP_BLOCK) void k_sell_op_slots(OpArgs a, int64_t slot_stride) {
    a.x += (int64_t)blockIdx.y * slot_stride;
    a.out += (int64_t)blockIdx.y * slot_stride;
    sell_op_block<false>(a, blockIdx.x);
}

// the same step for two independent graphs in one launch (target and source mesh of a pair run
// their Chebyshev recurrences in lockstep): a 250k-vertex step alone is ~5 us, of which ~3 us is
// launch/ramp latency; two per launch amortise it.
template <bool HAS_PREV>
__global__ __launch_bounds__(PF_OP_BLOCK) void k_sell_op2(OpArgs a, OpArgs b) {
    if (blockIdx.x < a.n_blocks) sell_op_block<HAS_PREV>(a, blockIdx.x);
    else sell_op_block<HAS_PREV>(b, blockIdx.x - a.n_blocks);
}

__global__ __launch_bounds__(PF_BLOCK) void k_mask_isolated(double* __restrict__ x, const int32_t* __restrict__ rowptr,
                                                            const int32_t* __restrict__ perm, int64_t n) {
    const int64_t r = (int64_t)blockIdx.x * PF_BLOCK + threadIdx.x;
    if (r >= n) return;
    const int32_t i = perm[r];
    if (rowptr[i + 1] == rowptr[i]) x[r] = 0.0;
}

// Krylov start vector, part 2: smooth part + counter-based noise (splitmix64 of (seed, vertex)), zero
// on isolated vertices and padding.  Noise keeps every eigenmode present whatever the geometry.
__device__ __forceinline__ void d_start_vector(double* __restrict__ x, const double* __restrict__ smooth,
                                               const int32_t* __restrict__ perm, const int32_t* __restrict__ perm_m,
                                               const int32_t* __restrict__ rowptr,
                                               int64_t n_pad, unsigned long long seed, double noise) {
    const int64_t r = (int64_t)blockIdx.x * PF_BLOCK + threadIdx.x;
    if (r >= n_pad) return;
    const int32_t i = perm[r];    // the caller's vertex number: what the noise is keyed by, whatever the internal order
    const int32_t m = perm_m[r];  // the row of CSR(W)
    double v = 0.0;
    if (i >= 0 && rowptr[m + 1] > rowptr[m]) {
        unsigned long long z = seed + 0x9E3779B97F4A7C15ull * (unsigned long long)(i + 1);
        z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
        z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
        z ^= z >> 31;
        const double u = (double)(z >> 11) * (1.0 / 9007199254740992.0) - 0.5;  // uniform in [-0.5, 0.5)
        v = smooth[r] + noise * u;
    }
    x[r] = v;
}
__global__ __launch_bounds__(PF_BLOCK) void k_start_vector(double* __restrict__ x, const double* __restrict__ smooth,
                                                           const int32_t* __restrict__ perm, const int32_t* __restrict__ perm_m,
                                                           const int32_t* __restrict__ rowptr,
                                                           int64_t n_pad, unsigned long long seed, double noise) {
    d_start_vector(x, smooth, perm, perm_m, rowptr, n_pad, seed, noise);
}
struct f_start_vector {
    static constexpr int BOUNDS = PF_BLOCK;
    static __device__ __forceinline__ void run(double* x, const double* smooth, const int32_t* perm, const int32_t* perm_m, const int32_t* rowptr,
                                               int64_t n_pad, unsigned long long seed, double noise) {
        d_start_vector(x, smooth, perm, perm_m, rowptr, n_pad, seed, noise);
    }
};

// host order <-> solver order
__global__ __launch_bounds__(PF_BLOCK) void k_permute_in(const double* __restrict__ src_old, const int32_t* __restrict__ perm,
                                                         int64_t n_pad, double* __restrict__ dst_new) {
    const int64_t r = (int64_t)blockIdx.x * PF_BLOCK + threadIdx.x;
    if (r >= n_pad) return;
    const int32_t i = perm[r];
    dst_new[r] = i >= 0 ? src_old[i] : 0.0;
}

__global__ __launch_bounds__(PF_BLOCK) void k_permute_out(const double* __restrict__ ws, int64_t n_pad, int32_t first,
                                                          int32_t count, const int32_t* __restrict__ iperm, int64_t n,
                                                          double* __restrict__ dst_old /* [count][n] */) {
    const int64_t i = (int64_t)blockIdx.x * PF_BLOCK + threadIdx.x;
    if (i >= n) return;
    const int64_t r = iperm[i];
    for (int c = 0; c < count; ++c) dst_old[(int64_t)c * n + i] = ws[(int64_t)(first + c) * n_pad + r];
}

__device__ __forceinline__ void d_null_vector(double* __restrict__ x, const int32_t* __restrict__ label,
                                              const int32_t* __restrict__ rowptr,
                                              const double* __restrict__ deg, const int32_t* __restrict__ perm,
                                              int64_t n_pad, int32_t root, int32_t sym,
                                              const double* __restrict__ weight) {
    // null vector of the iterated operator on one component: 1_C for L = G (D - W) and for a general matrix with zero
    // row sums (G = I: sym == 0 is passed), G^-1/2 1_C = sqrt(deg + 1e-8) 1_C for S = G^1/2 (D - W) G^1/2 of a mesh graph;
    // `weight` (cotangent graphs: sqrt(m), the null vector of M^-1/2 (D - W) M^-1/2) replaces both
    const int64_t r = (int64_t)blockIdx.x * PF_BLOCK + threadIdx.x;
    if (r >= n_pad) return;
    const int32_t i = perm[r];
    double v = 0.0;
    if (i >= 0 && label[i] == root && rowptr[i + 1] > rowptr[i]) v = weight ? weight[i] : (sym ? sqrt(deg[i] + 1e-8) : 1.0);
    x[r] = v;
}
__global__ __launch_bounds__(PF_BLOCK) void k_null_vector(double* __restrict__ x, const int32_t* __restrict__ label,
                                                          const int32_t* __restrict__ rowptr,
                                                          const double* __restrict__ deg, const int32_t* __restrict__ perm,
                                                          int64_t n_pad, int32_t root, int32_t sym,
                                                          const double* __restrict__ weight) {
    d_null_vector(x, label, rowptr, deg, perm, n_pad, root, sym, weight);
}
struct f_null_vector {
    static constexpr int BOUNDS = PF_BLOCK;
    static __device__ __forceinline__ void run(double* x, const int32_t* label, const int32_t* rowptr, const double* deg, const int32_t* perm,
                                               int64_t n_pad, int32_t root, int32_t sym, const double* weight) {
        d_null_vector(x, label, rowptr, deg, perm, n_pad, root, sym, weight);
    }
};

OpArgs op_args(pf_graph* g, const double* vals, const double* x, const double* prev, double* out, double alpha, double shift,
               double beta) {
    return OpArgs{g->slice_ptr, g->scol, vals, g->diag, x, prev, out, alpha, shift, beta, (unsigned)(g->n_pad / PF_OP_BLOCK)};
}

int launch_op2(pf_graph* ga, const OpArgs& a, const OpArgs& b, bool has_prev) {
    hipStream_t st = ga->ctx->stream;
    if (has_prev)
        k_sell_op2<true><<<a.n_blocks + b.n_blocks, PF_OP_BLOCK, 0, st>>>(a, b);
    else
        k_sell_op2<false><<<a.n_blocks + b.n_blocks, PF_OP_BLOCK, 0, st>>>(a, b);
    PF_HIP(hipGetLastError());
    return PF_OK;
}

// One Chebyshev recurrence: y0 = src; y1 = (c y0 - A y0)/(e rho); y_{k+1} = (2/(e rho))(c y_k - A y_k) - y_{k-1}/rho^2
// (rho > 1: scaled by rho^-k, so the result is T_p(.)/rho^p and high degrees cannot overflow).  Steps run one per
// launch (sell_op_block) through rotating temporaries; the caller's src is never overwritten and the last step
// lands in dst.
struct ChebRun {
    pf_graph* g;
    const double* vals;
    const double* src;
    double* dst;
    int32_t degree;
    double c, e, rho;
    const double* yp = nullptr;  // y_{done-1}
    const double* yc = nullptr;  // y_done
    int32_t done = 0;

    int32_t left() const { return degree - done; }
    double* free_tmp(int which) const {  // the which-th temporary that holds neither y_{done-1} nor y_done
        for (int t = 0; t < PF_WS_TMPS; ++t) {
            double* b = pf_tmp(g, t);
            if (b != yp && b != yc && which-- == 0) return b;
        }
        return nullptr;
    }
    OpArgs first() {  // step 1
        double* target = degree == 1 ? dst : pf_tmp(g, 0);
        const OpArgs a = op_args(g, vals, src, nullptr, target, 1.0 / (e * rho), c, 0.0);
        yp = src, yc = target, done = 1;
        return a;
    }
    OpArgs single() {  // one step k > 1
        double* target = left() == 1 ? dst : free_tmp(0);
        const OpArgs a = op_args(g, vals, yc, yp, target, 2.0 / (e * rho), c, 1.0 / (rho * rho));
        yp = yc, yc = target, done += 1;
        return a;
    }
};

}  // namespace

int pf_check_slots(pf_graph* g, int32_t first, int32_t count, const char* who) {
    PF_CHECK(g != nullptr, PF_E_ARG, "%s: graph is NULL", who);
    PF_HIP(hipSetDevice(g->ctx->device));  // the calling host thread may have another current device
    PF_CHECK(first >= 0 && count >= 0 && first + count <= g->n_slots, PF_E_ARG, "%s: slots [%d,%d) outside workspace of %d",
             who, first, first + count, g->n_slots);
    return PF_OK;
}

const double* pf_op_values(pf_graph* g, int32_t op) {
    if (op == PF_OP_RW) return g->sval_rw;
    if (op == PF_OP_SYM) return g->sval_sym;
    return nullptr;
}

int64_t pf_op_bytes(const pf_graph* g) {  // 12 nnz + 20 n + 4, nnz counted with the diagonal
    return 12 * (g->nnz_w + g->n - g->n_isolated) + 20 * g->n + 4;
}

int pf_launch_op(pf_graph* g, const double* vals, const double* x, const double* prev, double* out, double alpha, double shift,
                 double beta) {
    hipStream_t st = g->ctx->stream;
    const OpArgs a = op_args(g, vals, x, prev, out, alpha, shift, beta);
    if (prev)
        k_sell_op<true><<<a.n_blocks, PF_OP_BLOCK, 0, st>>>(a);
    else
        k_sell_op<false><<<a.n_blocks, PF_OP_BLOCK, 0, st>>>(a);
    PF_HIP(hipGetLastError());
    return PF_OK;
}

OpTimer::OpTimer(pf_ctx* ctx, int64_t n, double b) : c(ctx), launches(n), bytes(b), on(ctx->timing) {
    if (on && ctx->timing_stride > 1) on = (ctx->timing_count++ % ctx->timing_stride) == 0;
    if (!on) return;
    if (c->spans_pending.size() >= 4096) (void)pf_timing_collect(c);  // bound the number of live events
    if (!c->spans_free.empty()) {
        e0 = c->spans_free.back().first;
        e1 = c->spans_free.back().second;
        c->spans_free.pop_back();
    } else if (hipEventCreate(&e0) != hipSuccess || hipEventCreate(&e1) != hipSuccess) {
        on = false;
        return;
    }
    hipEventRecord(e0, c->stream);
}
int OpTimer::finish() {  // never blocks: the span is resolved in pf_timing_get
    if (!on) return PF_OK;
    PF_HIP(hipEventRecord(e1, c->stream));
    c->spans_pending.push_back({e0, e1, launches, bytes, persist_steps, lds_bytes});
    return PF_OK;
}

extern "C" {

int pf_ws_ensure(pf_graph* g, int32_t n_slots) {
    PF_CHECK(g != nullptr && n_slots > 0, PF_E_ARG, "pf_ws_ensure: bad argument");
    if (n_slots <= g->n_slots) return PF_OK;
    PF_HIP(hipSetDevice(g->ctx->device));
    hipStream_t st = g->ctx->stream;
    double* nw = nullptr;
    const size_t bytes = sizeof(double) * (size_t)(n_slots + PF_WS_TMPS) * (size_t)g->n_pad;
    // Not cleared (250k rows x 100 slots: 200 MB per graph and solve, written through the cache the operator had just been
    // assembled into): a slot is read only after a kernel has written all n_pad rows of it - k_null_vector, k_start_vector,
    // k_permute_in, the operator kernels' out / dst (the Chebyshev temporaries behind the slots included: step 1 has no
    // prev term), k_combine, the slot copies; the row kernels of the row-partitioned solve touch up slots that one of
    // these has filled.  pf_pool_poison shows a reader that comes first (profiles/front_of_step.md, slot by slot).
    PF_HIP(pf_malloc(st, (void**)&nw, bytes));
    if (g->ws && g->n_slots > 0)
        PF_HIP(hipMemcpyAsync(nw, g->ws, sizeof(double) * (size_t)g->n_slots * g->n_pad, hipMemcpyDeviceToDevice, st));
    pf_free(st, g->ws);
    g->ws = nw;
    g->n_slots = n_slots;
    return PF_OK;
}

int pf_ws_upload(pf_graph* g, int32_t slot, const double* x) {
    PF_TRY(pf_check_slots(g, slot, 1, "pf_ws_upload"));
    PF_CHECK(x != nullptr, PF_E_ARG, "pf_ws_upload: x is NULL");
    hipStream_t st = g->ctx->stream;
    PF_HIP(g->stage.grow(st, g->n));
    PF_HIP(hipMemcpyAsync(g->stage.p, x, sizeof(double) * g->n, hipMemcpyHostToDevice, st));
    k_permute_in<<<pf_blocks(g->n_pad), PF_BLOCK, 0, st>>>(g->stage.p, g->perm, g->n_pad, pf_slot(g, slot));
    PF_HIP(hipGetLastError());
    PF_HIP(hipStreamSynchronize(st));  // x may be a temporary on the host side
    return PF_OK;
}

int pf_ws_download(pf_graph* g, int32_t first, int32_t count, double* out) {
    PF_TRY(pf_check_slots(g, first, count, "pf_ws_download"));
    PF_CHECK(out != nullptr, PF_E_ARG, "pf_ws_download: out is NULL");
    if (count == 0) return PF_OK;
    hipStream_t st = g->ctx->stream;
    PF_HIP(g->stage.grow(st, (int64_t)count * g->n));
    k_permute_out<<<pf_blocks(g->n), PF_BLOCK, 0, st>>>(g->ws, g->n_pad, first, count, g->iperm, g->n, g->stage.p);
    PF_HIP(hipGetLastError());
    PF_HIP(hipMemcpyAsync(out, g->stage.p, sizeof(double) * (size_t)count * g->n, hipMemcpyDeviceToHost, st));
    PF_HIP(hipStreamSynchronize(st));
    return pf_persist_check(g->ctx);
}

int pf_ws_copy(pf_graph* g, int32_t src, int32_t dst, int32_t count) {
    PF_TRY(pf_check_slots(g, src, count, "pf_ws_copy"));
    PF_TRY(pf_check_slots(g, dst, count, "pf_ws_copy"));
    PF_CHECK(src + count <= dst || dst + count <= src || src == dst, PF_E_ARG, "pf_ws_copy: overlapping ranges");
    if (src == dst || count == 0) return PF_OK;
    PF_HIP(hipMemcpyAsync(pf_slot(g, dst), pf_slot(g, src), sizeof(double) * (size_t)count * g->n_pad,
                          hipMemcpyDeviceToDevice, g->ctx->stream));
    return PF_OK;
}

int pf_mask_isolated(pf_graph* g, int32_t slot) {
    PF_TRY(pf_check_slots(g, slot, 1, "pf_mask_isolated"));
    if (g->n_isolated == 0) return PF_OK;
    k_mask_isolated<<<pf_blocks(g->n), PF_BLOCK, 0, g->ctx->stream>>>(pf_slot(g, slot), g->rowptr, g->perm_m, g->n);
    PF_HIP(hipGetLastError());
    return PF_OK;
}

int pf_start_vector(pf_graph* g, int32_t slot, uint64_t seed) {
    PF_TRY(pf_check_slots(g, slot, 1, "pf_start_vector"));
    if (pfl::tl_rec) {  // (the head of a pair's solve: one launch for both graphs' start vectors)
        pfl::launch<f_start_vector>(dim3(pf_blocks(g->n_pad)), dim3(PF_BLOCK), 0, g->ctx->stream, pf_slot(g, slot), g->smooth, g->perm, g->perm_m, g->rowptr,
                                    g->n_pad, (unsigned long long)seed, 0.5);
        return PF_OK;
    }
    k_start_vector<<<pf_blocks(g->n_pad), PF_BLOCK, 0, g->ctx->stream>>>(pf_slot(g, slot), g->smooth, g->perm, g->perm_m, g->rowptr, g->n_pad,
                                                                    (unsigned long long)seed, 0.5);
    PF_HIP(hipGetLastError());
    return PF_OK;
}

int pf_lock_null_vectors(pf_graph* g, int32_t op, int32_t* n_locked) {
    PF_CHECK(g != nullptr && n_locked != nullptr, PF_E_ARG, "pf_lock_null_vectors: NULL argument");
    PF_HIP(hipSetDevice(g->ctx->device));
    PF_CHECK(op == PF_OP_RW || (op == PF_OP_SYM && g->is_symmetric), PF_E_ARG,
             "pf_lock_null_vectors: operator %d not available (W symmetric: %d)", op, g->is_symmetric);
    const int32_t nc = g->n_components;
    PF_TRY(pf_ws_ensure(g, nc + 1));
    hipStream_t st = g->ctx->stream;
    PF_TRY(pf_reduce_ensure(g, 1));
    const bool rec = pfl::tl_rec != nullptr;  // the head of a pair's solve: recorded, the partner's launches share these
    const int32_t sym_w = op == PF_OP_SYM && !g->unit_g;
    const double* weight = g->is_cotan ? g->cot_sqrtm : nullptr;
    for (int32_t c = 0; c < nc; ++c) {
        if (rec) pfl::launch<f_null_vector>(dim3(pf_blocks(g->n_pad)), dim3(PF_BLOCK), 0, st, pf_slot(g, c), g->label, g->rowptr, g->deg, g->perm_m, g->n_pad, g->roots[c], sym_w, weight);
        else k_null_vector<<<pf_blocks(g->n_pad), PF_BLOCK, 0, st>>>(pf_slot(g, c), g->label, g->rowptr, g->deg, g->perm_m, g->n_pad, g->roots[c], sym_w, weight);
        PF_HIP(hipGetLastError());
        // normalised with the norm still on the device (the same 1 / sqrt as on the host: the same bits; a component has at
        // least two vertices, so the norm is positive) - no wait at the head of a solve
        PF_TRY(pf_dots_device(g, c, c, 1, g->coef, nullptr, 0));
        PF_TRY(pf_scale_rsqrt(g, pf_slot(g, c), g->coef));
    }
    *n_locked = nc;
    return PF_OK;
}

int pf_spmv(pf_graph* g, int32_t op, int32_t src, int32_t dst) {
    PF_TRY(pf_check_slots(g, src, 1, "pf_spmv"));
    PF_TRY(pf_check_slots(g, dst, 1, "pf_spmv"));
    const double* vals = pf_op_values(g, op);
    PF_CHECK(vals != nullptr && src != dst, PF_E_ARG, "pf_spmv: operator %d unavailable or src == dst", op);
    OpTimer t(g->ctx, 1, (double)pf_op_bytes(g));
    PF_TRY(pf_launch_op(g, vals, pf_slot(g, src), nullptr, pf_slot(g, dst), -1.0, 0.0, 0.0));
    return t.finish();
}

int pf_spmv_multi(pf_graph* g, int32_t op, int32_t src_first, int32_t dst_first, int32_t count) {
    PF_CHECK(count >= 0, PF_E_ARG, "pf_spmv_multi: negative count");
    PF_TRY(pf_check_slots(g, src_first, count, "pf_spmv_multi"));
    PF_TRY(pf_check_slots(g, dst_first, count, "pf_spmv_multi"));
    const double* vals = pf_op_values(g, op);
    PF_CHECK(vals != nullptr && (src_first + count <= dst_first || dst_first + count <= src_first), PF_E_ARG,
             "pf_spmv_multi: operator %d unavailable or the slot ranges overlap", op);
    if (count == 0) return PF_OK;
    OpTimer t(g->ctx, count, (double)count * (double)pf_op_bytes(g));
    {
        const OpArgs a = op_args(g, vals, pf_slot(g, src_first), nullptr, pf_slot(g, dst_first), -1.0, 0.0, 0.0);
        k_sell_op_slots<<<dim3(a.n_blocks, (unsigned)count), PF_OP_BLOCK, 0, g->ctx->stream>>>(a, g->n_pad);
        PF_HIP(hipGetLastError());
    }
    return t.finish();
}

int pf_cheb(pf_graph* g, int32_t op, int32_t src, int32_t dst, int32_t degree, double c, double e, double rho) {
    PF_TRY(pf_check_slots(g, src, 1, "pf_cheb"));
    PF_TRY(pf_check_slots(g, dst, 1, "pf_cheb"));
    const double* vals = pf_op_values(g, op);
    PF_CHECK(vals != nullptr && src != dst, PF_E_ARG, "pf_cheb: operator %d unavailable or src == dst", op);
    PF_CHECK(degree >= 1 && e > 0.0 && rho >= 1.0, PF_E_ARG, "pf_cheb: degree %d / half-width %g / rho %g invalid", degree, e, rho);
    OpTimer t(g->ctx, degree, (double)degree * pf_op_bytes(g));
    {  // the whole recurrence in one kernel with the operator in LDS, when it fits (pf_persist.hip)
        const pf_persist_args pa{g, vals, pf_slot(g, src), pf_slot(g, dst), degree, c, e, rho};
        int done = 0;
        PF_TRY(pf_persist_cheb(&pa, nullptr, &done, &t.lds_bytes));
        if (done) {
            t.launches = 1;
            t.persist_steps = degree;
            return t.finish();
        }
    }
    ChebRun r{g, vals, pf_slot(g, src), pf_slot(g, dst), degree, c, e, rho};
    int64_t launches = 1;
    {
        const OpArgs a = r.first();
        PF_TRY(pf_launch_op(g, a.sval, a.x, a.prev, a.out, a.alpha, a.shift, a.beta));
    }
    while (r.left() > 0) {
        const OpArgs a = r.single();
        PF_TRY(pf_launch_op(g, a.sval, a.x, a.prev, a.out, a.alpha, a.shift, a.beta));
        ++launches;
    }
    t.launches = launches;
    return t.finish();
}

int pf_cheb2(pf_graph* ga, int32_t op_a, int32_t src_a, int32_t dst_a, int32_t degree_a, double c_a, double e_a, double rho_a,
             pf_graph* gb, int32_t op_b, int32_t src_b, int32_t dst_b, int32_t degree_b, double c_b, double e_b, double rho_b) {
    PF_TRY(pf_check_slots(ga, src_a, 1, "pf_cheb2"));
    PF_TRY(pf_check_slots(ga, dst_a, 1, "pf_cheb2"));
    PF_TRY(pf_check_slots(gb, src_b, 1, "pf_cheb2"));
    PF_TRY(pf_check_slots(gb, dst_b, 1, "pf_cheb2"));
    PF_CHECK(ga != gb && ga->ctx == gb->ctx, PF_E_ARG, "pf_cheb2: the two graphs must differ and share one ctx (stream)");
    const double* va = pf_op_values(ga, op_a);
    const double* vb = pf_op_values(gb, op_b);
    PF_CHECK(va && vb && src_a != dst_a && src_b != dst_b, PF_E_ARG, "pf_cheb2: operator unavailable or src == dst");
    PF_CHECK(degree_a >= 1 && degree_b >= 1 && e_a > 0.0 && e_b > 0.0 && rho_a >= 1.0 && rho_b >= 1.0, PF_E_ARG,
             "pf_cheb2: bad degree / half-width / rho");
    OpTimer t(ga->ctx, std::max(degree_a, degree_b), (double)degree_a * pf_op_bytes(ga) + (double)degree_b * pf_op_bytes(gb));
    {
        const pf_persist_args pa{ga, va, pf_slot(ga, src_a), pf_slot(ga, dst_a), degree_a, c_a, e_a, rho_a};
        const pf_persist_args pb{gb, vb, pf_slot(gb, src_b), pf_slot(gb, dst_b), degree_b, c_b, e_b, rho_b};
        int done = 0;
        PF_TRY(pf_persist_cheb(&pa, &pb, &done, &t.lds_bytes));
        if (done) {
            t.launches = 1;
            t.persist_steps = degree_a + degree_b;
            return t.finish();
        }
        // The pair does not fit one resident launch (windows of 2048+ rows: registers / LDS): each graph in its own
        // resident launch still beats one step per launch by far (1M rows: 2 x 4 us per step against 30 us shared).
        // Only then: when the window structures do not cover one of the two graphs (px_state 0: pf_windows.hip), that
        // graph streams whatever happens, and the pair streams as a pair - two graphs per launch - instead of splitting.
        int done_a = 0, done_b = 0;
        if (ga->px_state != 0 && gb->px_state != 0) {
            PF_TRY(pf_persist_cheb(&pa, nullptr, &done_a, &t.lds_bytes, false));
            PF_TRY(pf_persist_cheb(&pb, nullptr, &done_b, &t.lds_bytes, false));
        }
        if (done_a || done_b) {
            t.launches = done_a + done_b;
            t.persist_steps = (done_a ? degree_a : 0) + (done_b ? degree_b : 0);
            for (int q = 0; q < 2; ++q) {
                if (q == 0 ? done_a : done_b) continue;
                ChebRun r = q == 0 ? ChebRun{ga, va, pf_slot(ga, src_a), pf_slot(ga, dst_a), degree_a, c_a, e_a, rho_a}
                                   : ChebRun{gb, vb, pf_slot(gb, src_b), pf_slot(gb, dst_b), degree_b, c_b, e_b, rho_b};
                OpArgs a = r.first();
                PF_TRY(pf_launch_op(r.g, a.sval, a.x, a.prev, a.out, a.alpha, a.shift, a.beta));
                ++t.launches;
                while (r.left() > 0) {
                    a = r.single();
                    PF_TRY(pf_launch_op(r.g, a.sval, a.x, a.prev, a.out, a.alpha, a.shift, a.beta));
                    ++t.launches;
                }
            }
            return t.finish();
        }
    }
    ChebRun ra{ga, va, pf_slot(ga, src_a), pf_slot(ga, dst_a), degree_a, c_a, e_a, rho_a};
    ChebRun rb{gb, vb, pf_slot(gb, src_b), pf_slot(gb, dst_b), degree_b, c_b, e_b, rho_b};
    int64_t launches = 1;
    {
        const OpArgs a = ra.first(), b = rb.first();
        PF_TRY(launch_op2(ga, a, b, false));
    }
    while (ra.left() > 0 || rb.left() > 0) {
        if (ra.left() > 0 && rb.left() > 0) {
            const OpArgs a = ra.single(), b = rb.single();
            PF_TRY(launch_op2(ga, a, b, true));
        } else {  // the longer recurrence finishes alone
            ChebRun& r = ra.left() > 0 ? ra : rb;
            const OpArgs a = r.single();
            PF_TRY(pf_launch_op(r.g, a.sval, a.x, a.prev, a.out, a.alpha, a.shift, a.beta));
        }
        ++launches;
    }
    t.launches = launches;
    return t.finish();
}

int pf_spmv_host(pf_graph* g, int32_t op, const double* x, double* y) {
    PF_CHECK(g != nullptr && x != nullptr && y != nullptr, PF_E_ARG, "pf_spmv_host: NULL argument");
    const double* vals = pf_op_values(g, op);
    PF_CHECK(vals != nullptr, PF_E_ARG, "pf_spmv_host: operator %d unavailable", op);
    PF_TRY(pf_ws_ensure(g, 2));
    PF_TRY(pf_ws_upload(g, 0, x));
    PF_TRY(pf_launch_op(g, vals, pf_slot(g, 0), nullptr, pf_slot(g, 1), -1.0, 0.0, 0.0));
    return pf_ws_download(g, 1, 1, y);
}

}  // extern "C"
