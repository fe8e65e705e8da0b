// Row-wise work on a graph outside the eigensolver's own loop: the mean filter over [n][ncols] arrays in mesh order, and
// the primitives of the row-partitioned solve (pyfocusr_amd/rowpart.py) - single operator and Chebyshev steps, an axpy
// with host coefficients, and row sets (pf_rows_*) that gather, scatter and fill boundary / ghost rows of workspace slots.
#include <algorithm>
#include <vector>

#include "pf_internal.h"

namespace {

// Mean filter (graph.py:349-353): out = ((D+I)^-1 (W+I)) in, applied `iterations` times to an n x ncols array.
// scipy forms average_mat = D_inv @ (W + I) as a sparse-sparse product whose rows come out in DESCENDING column
// order (SMMP linked list), and average_mat @ v then sums in that order with the products (dinv*w)*v.  The same
// terms in the same order are kept here, but rows and gathers live in the solver's Morton/degree order (SELL-64,
// coalesced entry loads, neighbours close in memory) instead of the mesh's own vertex order.
__global__ __launch_bounds__(PF_BLOCK) void k_fill_mean_filter(const int32_t* __restrict__ rowptr, const int32_t* __restrict__ col,
                                                               const double* __restrict__ w, const double* __restrict__ deg,
                                                               const int32_t* __restrict__ perm, const int32_t* __restrict__ iperm,
                                                               const int32_t* __restrict__ key, int64_t n_pad,
                                                               const int64_t* __restrict__ slice_ptr,
                                                               int32_t* __restrict__ mf_col, double* __restrict__ mf_val) {
    const int64_t row = (int64_t)blockIdx.x * PF_BLOCK + threadIdx.x;
    if (row >= n_pad) return;
    const int64_t s = row / PF_WAVE;
    const int lane = (int)(row & (PF_WAVE - 1));
    const int32_t width = (int32_t)((slice_ptr[s + 1] - slice_ptr[s]) / PF_WAVE) + 1;
    const int64_t base = slice_ptr[s] + (int64_t)PF_WAVE * s;
    const int32_t i = perm[row];
    int32_t e = 0;
    if (i >= 0) {
        const double dinv = 1.0 / (1.0 + deg[i]);
        bool diag_done = false;
        const int32_t ki = key ? key[i] : i;  // (scipy's order is that of the caller's vertex numbers; perm / iperm / col: m-space)
        for (int32_t a = rowptr[i + 1] - 1; a >= rowptr[i]; --a) {
            const int32_t j = col[a];
            if (!diag_done && (key ? key[j] : j) < ki) {
                mf_col[base + (int64_t)PF_WAVE * e + lane] = (int32_t)row;
                mf_val[base + (int64_t)PF_WAVE * e + lane] = dinv;
                ++e;
                diag_done = true;
            }
            mf_col[base + (int64_t)PF_WAVE * e + lane] = iperm[j];
            mf_val[base + (int64_t)PF_WAVE * e + lane] = dinv * w[a];
            ++e;
        }
        if (!diag_done) {
            mf_col[base + (int64_t)PF_WAVE * e + lane] = (int32_t)row;
            mf_val[base + (int64_t)PF_WAVE * e + lane] = dinv;
            ++e;
        }
    }
    for (; e < width; ++e) {  // padding: 0 * own value
        mf_col[base + (int64_t)PF_WAVE * e + lane] = (int32_t)row;
        mf_val[base + (int64_t)PF_WAVE * e + lane] = 0.0;
    }
}

// NC > 0: compile-time column count; NC == 0: run-time ncols (one pass over the entries per column)
template <int NC>
__global__ __launch_bounds__(PF_BLOCK) void k_mean_filter(const int64_t* __restrict__ slice_ptr, const int32_t* __restrict__ mf_col,
                                                          const double* __restrict__ mf_val, const int32_t* __restrict__ perm,
                                                          int64_t n_pad, int32_t ncols, const double* __restrict__ in,
                                                          double* __restrict__ out) {
    const int64_t row = (int64_t)blockIdx.x * PF_BLOCK + threadIdx.x;
    if (row >= n_pad) return;
    const int64_t s = row / PF_WAVE;
    const int lane = (int)(row & (PF_WAVE - 1));
    const int32_t width = (int32_t)((slice_ptr[s + 1] - slice_ptr[s]) / PF_WAVE) + 1;
    const int64_t base = slice_ptr[s] + (int64_t)PF_WAVE * s + lane;
    const bool real = perm[row] >= 0;
    if constexpr (NC > 0) {
        double acc[NC];
#pragma unroll
        for (int c = 0; c < NC; ++c) acc[c] = 0.0;
        for (int32_t e = 0; e < width; ++e) {
            const int64_t j = mf_col[base + (int64_t)PF_WAVE * e];
            const double v = mf_val[base + (int64_t)PF_WAVE * e];
            // padding entries (0 * own value) must not touch the sum: 0 * inf or -0.0 would change bits
            if (v != 0.0 || j != row) {
#pragma unroll
                for (int c = 0; c < NC; ++c) acc[c] += v * in[j * NC + c];
            }
        }
#pragma unroll
        for (int c = 0; c < NC; ++c) out[row * NC + c] = real ? acc[c] : 0.0;
    } else {
        for (int32_t c = 0; c < ncols; ++c) {
            double acc = 0.0;
            for (int32_t e = 0; e < width; ++e) {
                const double v = mf_val[base + (int64_t)PF_WAVE * e];
                const int64_t j = mf_col[base + (int64_t)PF_WAVE * e];
                if (v != 0.0 || j != row) acc += v * in[j * ncols + c];
            }
            out[row * ncols + c] = real ? acc : 0.0;
        }
    }
}

// rows between mesh order [n][ncols] and solver order [n_pad][ncols]
__global__ __launch_bounds__(PF_BLOCK) void k_rows_in(const double* __restrict__ src, const int32_t* __restrict__ perm, int64_t n_pad,
                                                      int32_t ncols, double* __restrict__ dst) {
    const int64_t t = (int64_t)blockIdx.x * PF_BLOCK + threadIdx.x;
    if (t >= n_pad * ncols) return;
    const int64_t row = t / ncols;
    const int32_t old = perm[row];
    dst[t] = old >= 0 ? src[(int64_t)old * ncols + (t - row * ncols)] : 0.0;
}
__global__ __launch_bounds__(PF_BLOCK) void k_rows_out(const double* __restrict__ src, const int32_t* __restrict__ iperm, int64_t n,
                                                       int32_t ncols, double* __restrict__ dst) {
    const int64_t t = (int64_t)blockIdx.x * PF_BLOCK + threadIdx.x;
    if (t >= n * ncols) return;
    const int64_t old = t / ncols;
    dst[t] = src[(int64_t)iperm[old] * ncols + (t - old * ncols)];
}

// ---- row subsets (pf_rows_*): boundary / ghost rows of a row-partitioned solve, addressed in solver order
__global__ __launch_bounds__(PF_BLOCK) void k_rows_to_new(const int64_t* __restrict__ old_idx, const int32_t* __restrict__ iperm,
                                                          int64_t cnt, int32_t* __restrict__ new_idx) {
    const int64_t t = (int64_t)blockIdx.x * PF_BLOCK + threadIdx.x;
    if (t < cnt) new_idx[t] = iperm[old_idx[t]];
}
__global__ __launch_bounds__(PF_BLOCK) void k_rows_gather(const double* __restrict__ x, const int32_t* __restrict__ idx, int64_t cnt,
                                                          double* __restrict__ out) {
    const int64_t t = (int64_t)blockIdx.x * PF_BLOCK + threadIdx.x;
    if (t < cnt) out[t] = x[idx[t]];
}
__global__ __launch_bounds__(PF_BLOCK) void k_rows_scatter(double* __restrict__ x, const int32_t* __restrict__ idx, int64_t cnt,
                                                           const double* __restrict__ in) {
    const int64_t t = (int64_t)blockIdx.x * PF_BLOCK + threadIdx.x;
    if (t < cnt) x[idx[t]] = in[t];
}
// both recurrence vectors of a boundary exchange in one launch each way
__global__ __launch_bounds__(PF_BLOCK) void k_rows_gather2(const double* __restrict__ xa, const double* __restrict__ xb,
                                                           const int32_t* __restrict__ idx, int64_t cnt, int64_t stride,
                                                           double* __restrict__ out) {
    const int64_t t = (int64_t)blockIdx.x * PF_BLOCK + threadIdx.x;
    if (t >= cnt) return;
    const int32_t r = idx[t];
    out[t] = xa[r];
    if (xb) out[stride + t] = xb[r];
}
__global__ __launch_bounds__(PF_BLOCK) void k_rows_scatter2(double* __restrict__ xa, double* __restrict__ xb,
                                                            const int32_t* __restrict__ idx, const int64_t* __restrict__ off,
                                                            int64_t cnt, int64_t stride, const double* __restrict__ src) {
    const int64_t t = (int64_t)blockIdx.x * PF_BLOCK + threadIdx.x;
    if (t >= cnt) return;
    const int32_t r = idx[t];
    const int64_t o = off[t];
    xa[r] = src[o];
    if (xb) xb[r] = src[o + stride];
}
__global__ __launch_bounds__(PF_BLOCK) void k_rows_fill(double* __restrict__ x, const int32_t* __restrict__ idx, int64_t cnt,
                                                        double value) {
    const int64_t t = (int64_t)blockIdx.x * PF_BLOCK + threadIdx.x;
    if (t < cnt) x[idx[t]] = value;
}

}  // namespace

extern "C" {

int pf_mean_filter(pf_graph* g, const double* values, int32_t ncols, int32_t iterations, double* out) {
    PF_CHECK(g != nullptr && values != nullptr && out != nullptr && ncols > 0 && iterations >= 0, PF_E_ARG,
             "pf_mean_filter: bad argument");
    PF_HIP(hipSetDevice(g->ctx->device));
    hipStream_t st = g->ctx->stream;
    if (!g->mf_col) {  // first use: the filter's rows in solver order
        const size_t entries = (size_t)(g->sell_entries + g->n_pad);
        PF_HIP(pf_malloc(st, (void**)&g->mf_col, sizeof(int32_t) * entries));
        PF_HIP(pf_malloc(st, (void**)&g->mf_val, sizeof(double) * entries));
        // (a cotangent graph filters with its cotangent weights: g->w / g->deg hold the entries of S there)
        k_fill_mean_filter<<<pf_blocks(g->n_pad), PF_BLOCK, 0, st>>>(g->rowptr, g->col, g->is_cotan ? g->cot_w : g->w, g->is_cotan ? g->cot_diag : g->deg, g->perm_m, g->iperm_m, g->morder, g->n_pad,
                                                                g->slice_ptr, g->mf_col, g->mf_val);
        PF_HIP(hipGetLastError());
    }
    const size_t n_mesh = (size_t)g->n * ncols, n_padded = (size_t)g->n_pad * ncols;
    Scratch sc(st);
    double* m = sc.get<double>(n_mesh);
    PF_HIP(sc.err);  // (only the fill above is queued: no wait)
    double* a = sc.get<double>(n_padded);
    double* b = sc.get<double>(n_padded);
    sc.upload(m, values, n_mesh);
    if (sc.ok()) {
        k_rows_in<<<pf_blocks(g->n_pad * ncols), PF_BLOCK, 0, st>>>(m, g->perm, g->n_pad, ncols, a);
        for (int32_t it = 0; it < iterations; ++it) {
            if (ncols == 3) k_mean_filter<3><<<pf_blocks(g->n_pad), PF_BLOCK, 0, st>>>(g->slice_ptr, g->mf_col, g->mf_val, g->perm, g->n_pad, ncols, a, b);
            else if (ncols == 1) k_mean_filter<1><<<pf_blocks(g->n_pad), PF_BLOCK, 0, st>>>(g->slice_ptr, g->mf_col, g->mf_val, g->perm, g->n_pad, ncols, a, b);
            else k_mean_filter<0><<<pf_blocks(g->n_pad), PF_BLOCK, 0, st>>>(g->slice_ptr, g->mf_col, g->mf_val, g->perm, g->n_pad, ncols, a, b);
            std::swap(a, b);
        }
        k_rows_out<<<pf_blocks(g->n * ncols), PF_BLOCK, 0, st>>>(a, g->iperm, g->n, ncols, m);
        sc.launched();
    }
    sc.download(out, m, n_mesh);
    const hipError_t e2 = hipStreamSynchronize(st);  // (whatever failed: the copies queued so far read or write the caller's arrays)
    PF_HIP(sc.err);
    PF_HIP(e2);
    return PF_OK;
}

// ---- primitives of the row-partitioned solve (pyfocusr_amd/rowpart.py)
int pf_op_step(pf_graph* g, int32_t op, int32_t x, int32_t prev, int32_t out, double alpha, double shift, double beta) {
    PF_TRY(pf_check_slots(g, x, 1, "pf_op_step"));
    PF_TRY(pf_check_slots(g, out, 1, "pf_op_step"));
    if (prev >= 0) PF_TRY(pf_check_slots(g, prev, 1, "pf_op_step"));
    const double* vals = pf_op_values(g, op);
    PF_CHECK(vals != nullptr && x != out, PF_E_ARG, "pf_op_step: operator %d unavailable or x == out", op);
    OpTimer t(g->ctx, 1, (double)pf_op_bytes(g));
    PF_TRY(pf_launch_op(g, vals, pf_slot(g, x), prev >= 0 ? pf_slot(g, prev) : nullptr, pf_slot(g, out), alpha, shift, beta));
    return t.finish();
}

int pf_cheb_steps(pf_graph* g, int32_t op, int32_t prev, int32_t cur, int32_t k_first, int32_t n_steps, double c, double e,
                  double rho, int32_t* out_prev, int32_t* out_cur) {
    PF_TRY(pf_check_slots(g, prev, 1, "pf_cheb_steps"));
    PF_TRY(pf_check_slots(g, cur, 1, "pf_cheb_steps"));
    const double* vals = pf_op_values(g, op);
    PF_CHECK(vals != nullptr && prev != cur && out_prev && out_cur, PF_E_ARG, "pf_cheb_steps: bad operator / slots");
    PF_CHECK(k_first >= 1 && n_steps >= 0 && e > 0.0 && rho >= 1.0, PF_E_ARG, "pf_cheb_steps: k_first %d / n_steps %d invalid",
             k_first, n_steps);
    OpTimer t(g->ctx, n_steps, (double)n_steps * pf_op_bytes(g));
    int32_t a = prev, b = cur;  // b holds y_{k-1} of the step about to run, a receives y_k (step 1: a is overwritten, no prev term)
    for (int32_t k = k_first; k < k_first + n_steps; ++k) {
        if (k == 1) PF_TRY(pf_launch_op(g, vals, pf_slot(g, b), nullptr, pf_slot(g, a), 1.0 / (e * rho), c, 0.0));
        else PF_TRY(pf_launch_op(g, vals, pf_slot(g, b), pf_slot(g, a), pf_slot(g, a), 2.0 / (e * rho), c, 1.0 / (rho * rho)));
        std::swap(a, b);
    }
    *out_prev = a;
    *out_cur = b;
    return t.finish();
}

int pf_axpy(pf_graph* g, int32_t w, int32_t first, int32_t count, const double* coef) {
    PF_TRY(pf_check_slots(g, w, 1, "pf_axpy"));
    PF_TRY(pf_check_slots(g, first, count, "pf_axpy"));
    PF_CHECK(coef != nullptr || count == 0, PF_E_ARG, "pf_axpy: coef is NULL");
    PF_CHECK(w < first || w >= first + count, PF_E_ARG, "pf_axpy: w inside the basis range");
    if (count == 0) return PF_OK;
    hipStream_t st = g->ctx->stream;
    PF_TRY(pf_reduce_ensure(g, count));
    std::vector<double> neg(coef, coef + count);
    for (double& v : neg) v = -v;  // k_multi_axpy subtracts
    PF_HIP(hipMemcpyAsync(g->coef, neg.data(), sizeof(double) * count, hipMemcpyHostToDevice, st));
    PF_TRY(pf_multi_axpy(g, w, first, count, g->coef));
    PF_HIP(hipStreamSynchronize(st));  // neg goes out of scope
    return PF_OK;
}

struct pf_rows {
    pf_graph* g = nullptr;
    int32_t* idx = nullptr;  // solver-order row of every entry
    double* buf = nullptr;   // device staging [n]
    int64_t* off = nullptr;  // optional: where each row's value sits in a receive buffer (pf_rows_set_sources)
    int64_t n = 0;
};

void pf_rows_free(pf_rows* r) {
    if (!r) return;
    hipSetDevice(r->g->ctx->device);
    hipStream_t st = r->g->ctx->stream;
    hipStreamSynchronize(st);
    pf_free(st, r->idx);
    pf_free(st, r->buf);
    pf_free(st, r->off);
    delete r;
}

int pf_rows_create(pf_graph* g, const int64_t* rows, int64_t n, pf_rows** out) {
    PF_CHECK(g && out && (rows || n == 0) && n >= 0, PF_E_ARG, "pf_rows_create: bad argument");
    for (int64_t i = 0; i < n; ++i)
        PF_CHECK(rows[i] >= 0 && rows[i] < g->n, PF_E_ARG, "pf_rows_create: row %lld outside [0, %lld)", (long long)rows[i],
                 (long long)g->n);
    PF_HIP(hipSetDevice(g->ctx->device));
    hipStream_t st = g->ctx->stream;
    pf_rows* r = new pf_rows();
    r->g = g;
    r->n = n;
    if (n > 0) {
        Scratch sc(st);
        r->idx = sc.keep<int32_t>((size_t)n);  // (the row set's own: pf_rows_free)
        r->buf = sc.keep<double>((size_t)n);
        int64_t* tmp = sc.get<int64_t>((size_t)n);
        sc.upload(tmp, rows, (size_t)n);
        if (sc.ok()) {
            k_rows_to_new<<<pf_blocks(n), PF_BLOCK, 0, st>>>(tmp, g->iperm, n, r->idx);
            sc.launched();
        }
        sc.sync();
        if (!sc.ok()) {
            pf_set_error("pf_rows_create: %s", hipGetErrorString(sc.err));
            pf_rows_free(r);
            return PF_E_HIP;
        }
    }
    *out = r;
    return PF_OK;
}

int pf_rows_gather(pf_rows* r, int32_t slot, double* out) {
    PF_CHECK(r && (out || r->n == 0), PF_E_ARG, "pf_rows_gather: NULL argument");
    PF_TRY(pf_check_slots(r->g, slot, 1, "pf_rows_gather"));
    if (r->n == 0) return PF_OK;
    hipStream_t st = r->g->ctx->stream;
    k_rows_gather<<<pf_blocks(r->n), PF_BLOCK, 0, st>>>(pf_slot(r->g, slot), r->idx, r->n, r->buf);
    PF_HIP(hipGetLastError());
    PF_HIP(hipMemcpyAsync(out, r->buf, sizeof(double) * r->n, hipMemcpyDeviceToHost, st));
    PF_HIP(hipStreamSynchronize(st));
    return PF_OK;
}

int pf_rows_scatter(pf_rows* r, int32_t slot, const double* in) {
    PF_CHECK(r && (in || r->n == 0), PF_E_ARG, "pf_rows_scatter: NULL argument");
    PF_TRY(pf_check_slots(r->g, slot, 1, "pf_rows_scatter"));
    if (r->n == 0) return PF_OK;
    hipStream_t st = r->g->ctx->stream;
    PF_HIP(hipMemcpyAsync(r->buf, in, sizeof(double) * r->n, hipMemcpyHostToDevice, st));
    k_rows_scatter<<<pf_blocks(r->n), PF_BLOCK, 0, st>>>(pf_slot(r->g, slot), r->idx, r->n, r->buf);
    PF_HIP(hipGetLastError());
    PF_HIP(hipStreamSynchronize(st));  // `in` is the caller's again
    return PF_OK;
}

// device-pointer forms: `dst` / `src` are device buffers of r->n doubles owned by the caller (e.g. a torch tensor that
// RCCL sends / has received).  Enqueued on the ctx stream without a host sync: the caller orders the two streams
// (pf_sync before the peer library reads dst; the peer library's own sync before src is read here).
int pf_rows_gather_dev(pf_rows* r, int32_t slot, double* dst) {
    PF_CHECK(r && (dst || r->n == 0), PF_E_ARG, "pf_rows_gather_dev: NULL argument");
    PF_TRY(pf_check_slots(r->g, slot, 1, "pf_rows_gather_dev"));
    if (r->n == 0) return PF_OK;
    k_rows_gather<<<pf_blocks(r->n), PF_BLOCK, 0, r->g->ctx->stream>>>(pf_slot(r->g, slot), r->idx, r->n, dst);
    PF_HIP(hipGetLastError());
    return PF_OK;
}

int pf_rows_scatter_dev(pf_rows* r, int32_t slot, const double* src) {
    PF_CHECK(r && (src || r->n == 0), PF_E_ARG, "pf_rows_scatter_dev: NULL argument");
    PF_TRY(pf_check_slots(r->g, slot, 1, "pf_rows_scatter_dev"));
    if (r->n == 0) return PF_OK;
    k_rows_scatter<<<pf_blocks(r->n), PF_BLOCK, 0, r->g->ctx->stream>>>(pf_slot(r->g, slot), r->idx, r->n, src);
    PF_HIP(hipGetLastError());
    return PF_OK;
}

int pf_rows_set_sources(pf_rows* r, const int64_t* offsets) {
    PF_CHECK(r && (offsets || r->n == 0), PF_E_ARG, "pf_rows_set_sources: NULL argument");
    if (r->n == 0) return PF_OK;
    hipStream_t st = r->g->ctx->stream;
    PF_HIP(hipSetDevice(r->g->ctx->device));
    if (!r->off) PF_HIP(pf_malloc(st, (void**)&r->off, sizeof(int64_t) * r->n));
    PF_HIP(hipMemcpyAsync(r->off, offsets, sizeof(int64_t) * r->n, hipMemcpyHostToDevice, st));
    PF_HIP(hipStreamSynchronize(st));
    return PF_OK;
}

int pf_rows_gather2_dev(pf_rows* r, int32_t slot_a, int32_t slot_b, double* dst, int64_t stride) {
    PF_CHECK(r && (dst || r->n == 0) && stride >= r->n, PF_E_ARG, "pf_rows_gather2_dev: bad argument");
    PF_TRY(pf_check_slots(r->g, slot_a, 1, "pf_rows_gather2_dev"));
    if (slot_b >= 0) PF_TRY(pf_check_slots(r->g, slot_b, 1, "pf_rows_gather2_dev"));
    if (r->n == 0) return PF_OK;
    k_rows_gather2<<<pf_blocks(r->n), PF_BLOCK, 0, r->g->ctx->stream>>>(pf_slot(r->g, slot_a), slot_b >= 0 ? pf_slot(r->g, slot_b) : nullptr,
                                                                  r->idx, r->n, stride, dst);
    PF_HIP(hipGetLastError());
    return PF_OK;
}

int pf_rows_scatter2_dev(pf_rows* r, int32_t slot_a, int32_t slot_b, const double* src, int64_t stride) {
    PF_CHECK(r && (src || r->n == 0), PF_E_ARG, "pf_rows_scatter2_dev: NULL argument");
    PF_CHECK(r->off || r->n == 0, PF_E_STATE, "pf_rows_scatter2_dev: no source offsets (pf_rows_set_sources)");
    PF_TRY(pf_check_slots(r->g, slot_a, 1, "pf_rows_scatter2_dev"));
    if (slot_b >= 0) PF_TRY(pf_check_slots(r->g, slot_b, 1, "pf_rows_scatter2_dev"));
    if (r->n == 0) return PF_OK;
    k_rows_scatter2<<<pf_blocks(r->n), PF_BLOCK, 0, r->g->ctx->stream>>>(pf_slot(r->g, slot_a), slot_b >= 0 ? pf_slot(r->g, slot_b) : nullptr,
                                                                   r->idx, r->off, r->n, stride, src);
    PF_HIP(hipGetLastError());
    return PF_OK;
}

int pf_rows_fill(pf_rows* r, int32_t slot, double value) {
    PF_CHECK(r != nullptr, PF_E_ARG, "pf_rows_fill: NULL argument");
    PF_TRY(pf_check_slots(r->g, slot, 1, "pf_rows_fill"));
    if (r->n == 0) return PF_OK;
    k_rows_fill<<<pf_blocks(r->n), PF_BLOCK, 0, r->g->ctx->stream>>>(pf_slot(r->g, slot), r->idx, r->n, value);
    PF_HIP(hipGetLastError());
    return PF_OK;
}

}  // extern "C"
