// Exact linear assignment on Euclidean costs (pf_assign): what `linear_sum_assignment(cdist(rows, cols))` computes for
// focusr.py:340-349, without an n x n matrix anywhere.
//
// The problem is padded to square: rows n_rows .. n_cols-1 are virtual rows whose cost to every column is 0 (never
// stored; a branch on the row index).  In cost form a row i values column j at C_ij + p_j (p: column prices, >= 0 and
// only rising); the forward auction (Bertsekas) with Jacobi bidding runs in eps-scaling phases:
//   round: every unassigned row finds its best (lowest) and second-best value and bids  p_j + (second - best) + eps
//          for its best column j; each column takes the highest bid, the lowest row index among equal bids (two passes:
//          a 64-bit atomic max on the bid's bit pattern - prices are >= 0, so the bits order like the values - then an
//          atomic min on the index of the rows that match it); the winner's bid becomes the price and the previous
//          owner becomes unassigned.
//   phase: eps shrinks by AS_SCALE; rows whose assignment is no longer eps-optimal at the new eps are released first.
// Candidate lists keep a bid cheap without changing it: each real row keeps its AS_K nearest columns and r_i, the
// largest distance on the list.  Any other column is worth at least r_i + p_min, so when the list's second-best value is
// <= r_i + p_min the list holds the row's best and second-best values and the bid is the bid of the dense auction;
// otherwise the row scans all columns (k_as_dense).  Every bid is therefore a bid of the dense auction.
// After the last phase k_as_cert computes u_i = min_j (C_ij + p_j) over ALL columns: with v_j = -p_j the pair (u, v)
// is dual-feasible, and the sum of the slacks C_i,col(i) + p_col(i) - u_i (each in [0, eps]) bounds the gap to the
// optimum.  All decisions are order-independent (atomic max / min, index tie-breaks, block reductions in a fixed
// shape, sums on the host in index order): identical inputs give identical outputs.
//
// Memory: coordinates, the lists (AS_K indices and costs per row) and a handful of per-row / per-column vectors:
// O(n (d + AS_K)) bytes.
#include <math.h>

#include <algorithm>
#include <cmath>
#include <cstring>
#include <vector>

#include "pf_internal.h"

namespace {

constexpr int AS_K = 16;          // candidates per row
constexpr int AS_DMAX = 16;       // largest d
constexpr int AS_TILE = 128;      // columns per LDS tile (k_as_topk, k_as_cert)
constexpr int AS_PARTS = 256;     // partial results of the price reduction
constexpr int AS_DENSE_BLOCKS = 1024;  // blocks of k_as_dense (each takes queued rows in turn)
constexpr double AS_SCALE = 8.0;  // eps divisor per phase
constexpr double AS_REL = 1e-10;  // target: gap_bound <= AS_REL * total_cost
constexpr int64_t AS_MAX_ROUNDS = 1000000;  // a safety net: far above what any phase needs

struct AsState {
    double pmin, pmin2, pmax;
    int32_t pargmin;
    int32_t dense_count;  // rows queued for a dense bid this round
    int32_t unassigned;   // padded rows without a column
    int32_t pad;
    unsigned long long bids, dense_bids, rounds;
};

inline unsigned nblk(int64_t n, int b = PF_BLOCK) { return (unsigned)((n + b - 1) / b); }

// cdist's `euclidean`: squared differences summed left to right from 0, no contraction (-ffp-contract=off)
__device__ __forceinline__ double as_d2(const double (&x)[AS_DMAX], const double* __restrict__ q, int d) {
    double s = 0.0;
#pragma unroll
    for (int c = 0; c < AS_DMAX; ++c) {
        if (c < d) {
            const double df = x[c] - q[c];
            s += df * df;
        }
    }
    return s;
}

__device__ __forceinline__ void as_load_row(double (&x)[AS_DMAX], const double* __restrict__ p, int d, bool live) {
#pragma unroll
    for (int c = 0; c < AS_DMAX; ++c) x[c] = (live && c < d) ? p[c] : 0.0;
}

// (best value, its column, second-best value): lowest column index among equal best values
struct Top2 {
    double b;
    int32_t j;
    double s;
};

__device__ __forceinline__ void top2_push(Top2& t, double v, int32_t j) {
    if (v < t.b || (v == t.b && j < t.j)) {
        t.s = t.b;
        t.b = v;
        t.j = j;
    } else if (v < t.s) {
        t.s = v;
    }
}

__device__ __forceinline__ Top2 top2_merge(const Top2& a, const Top2& c) {
    Top2 r;
    if (c.b < a.b || (c.b == a.b && c.j < a.j)) {
        r.b = c.b;
        r.j = c.j;
        r.s = fmin(c.s, a.b);
    } else {
        r.b = a.b;
        r.j = a.j;
        r.s = fmin(a.s, c.b);
    }
    return r;
}

// block-wide Top2 (+ max) over PF_BLOCK threads; the result is valid in thread 0
__device__ Top2 top2_block(Top2 t, double& mx) {
    __shared__ double sb[PF_BLOCK], ss[PF_BLOCK], sm[PF_BLOCK];
    __shared__ int32_t sj[PF_BLOCK];
    const int tid = threadIdx.x;
    sb[tid] = t.b;
    ss[tid] = t.s;
    sj[tid] = t.j;
    sm[tid] = mx;
    __syncthreads();
    for (int w = PF_BLOCK / 2; w > 0; w >>= 1) {
        if (tid < w) {
            Top2 a{sb[tid], sj[tid], ss[tid]}, c{sb[tid + w], sj[tid + w], ss[tid + w]};
            Top2 r = top2_merge(a, c);
            sb[tid] = r.b;
            ss[tid] = r.s;
            sj[tid] = r.j;
            sm[tid] = fmax(sm[tid], sm[tid + w]);
        }
        __syncthreads();
    }
    Top2 r{sb[0], sj[0], ss[0]};
    mx = sm[0];
    __syncthreads();  // the arrays may be reused by the caller's next call
    return r;
}

// ---- candidate lists: the AS_K nearest columns of every real row (brute force over LDS tiles of the columns) --------
__global__ __launch_bounds__(PF_BLOCK) void k_as_topk(const double* __restrict__ rows, int64_t n_r,
                                                     const double* __restrict__ cols, int64_t n_c, int d,
                                                     int32_t* __restrict__ cand_j, double* __restrict__ cand_c,
                                                     double* __restrict__ rad, double* __restrict__ rmin) {
    __shared__ double tile[AS_TILE * AS_DMAX];
    const int64_t i = (int64_t)blockIdx.x * PF_BLOCK + threadIdx.x;
    const bool live = i < n_r;
    double x[AS_DMAX];
    as_load_row(x, rows + (live ? i : 0) * d, d, live);
    double bd[AS_K];
    int32_t bj[AS_K];
#pragma unroll
    for (int k = 0; k < AS_K; ++k) {
        bd[k] = INFINITY;
        bj[k] = -1;
    }
    for (int64_t t0 = 0; t0 < n_c; t0 += AS_TILE) {
        const int cnt = (int)((n_c - t0) < AS_TILE ? (n_c - t0) : AS_TILE);
        __syncthreads();
        for (int e = threadIdx.x; e < cnt * d; e += PF_BLOCK) tile[e] = cols[t0 * d + e];
        __syncthreads();
        if (!live) continue;
        for (int jj = 0; jj < cnt; ++jj) {
            const double s = as_d2(x, tile + jj * d, d);
            if (s < bd[AS_K - 1]) {  // strict: on equal distances the lower column index (seen first) stays ahead
                const int32_t j = (int32_t)(t0 + jj);
#pragma unroll
                for (int k = AS_K - 1; k > 0; --k) {
                    if (s < bd[k - 1]) {
                        bd[k] = bd[k - 1];
                        bj[k] = bj[k - 1];
                    } else if (s < bd[k]) {
                        bd[k] = s;
                        bj[k] = j;
                    }
                }
                if (s < bd[0]) {
                    bd[0] = s;
                    bj[0] = j;
                }
            }
        }
    }
    if (!live) return;
#pragma unroll
    for (int k = 0; k < AS_K; ++k) {
        cand_j[i * AS_K + k] = bj[k];
        cand_c[i * AS_K + k] = sqrt(bd[k]);
    }
    // every column off the list costs >= rad; a complete list (n_c <= AS_K) leaves nothing outside
    rad[i] = n_c > AS_K ? sqrt(bd[AS_K - 1]) : INFINITY;
    rmin[i] = sqrt(bd[0]);
}

// ---- prices: smallest (lowest index on ties), second smallest and largest, in two launches --------------------------
__global__ __launch_bounds__(PF_BLOCK) void k_as_prices_part(const double* __restrict__ p, int64_t n_c,
                                                            double* __restrict__ part) {
    Top2 t{INFINITY, INT32_MAX, INFINITY};
    double mx = 0.0;
    for (int64_t j = (int64_t)blockIdx.x * PF_BLOCK + threadIdx.x; j < n_c; j += (int64_t)gridDim.x * PF_BLOCK) {
        const double v = p[j];
        top2_push(t, v, (int32_t)j);
        mx = fmax(mx, v);
    }
    t = top2_block(t, mx);
    if (threadIdx.x == 0) {
        part[4 * blockIdx.x + 0] = t.b;
        part[4 * blockIdx.x + 1] = t.s;
        part[4 * blockIdx.x + 2] = mx;
        part[4 * blockIdx.x + 3] = (double)t.j;
    }
}

__global__ __launch_bounds__(PF_BLOCK) void k_as_prices_final(const double* __restrict__ part, int nparts,
                                                             AsState* __restrict__ st) {
    Top2 t{INFINITY, INT32_MAX, INFINITY};
    double mx = 0.0;
    if ((int)threadIdx.x < nparts) {
        const int q = threadIdx.x;
        t = Top2{part[4 * q], (int32_t)part[4 * q + 3], part[4 * q + 1]};
        mx = part[4 * q + 2];
    }
    t = top2_block(t, mx);
    if (threadIdx.x == 0) {
        st->pmin = t.b;
        st->pmin2 = t.s;
        st->pmax = mx;
        st->pargmin = t.j;
        st->dense_count = 0;
        if (st->unassigned > 0) st->rounds += 1;
    }
}

// ---- phase start: release the rows whose assignment is not eps-optimal at the new eps -------------------------------
__global__ __launch_bounds__(PF_BLOCK) void k_as_release(const double* __restrict__ rows, int64_t n_r,
                                                        const double* __restrict__ cols, int64_t n_c, int d,
                                                        const int32_t* __restrict__ cand_j,
                                                        const double* __restrict__ cand_c,
                                                        const double* __restrict__ rad, const double* __restrict__ p,
                                                        int32_t* __restrict__ owner, int32_t* __restrict__ col_of,
                                                        AsState* __restrict__ st, double eps) {
    const int64_t i = (int64_t)blockIdx.x * PF_BLOCK + threadIdx.x;
    if (i >= n_c) return;
    const int32_t j = col_of[i];
    if (j < 0) return;
    const double pmin = st->pmin;
    bool keep;
    if (i >= n_r) {
        keep = p[j] - pmin <= eps;
    } else {
        const int L = n_c < AS_K ? (int)n_c : AS_K;
        double best = INFINITY;
        for (int k = 0; k < L; ++k) best = fmin(best, cand_c[i * AS_K + k] + p[cand_j[i * AS_K + k]]);
        double x[AS_DMAX];
        as_load_row(x, rows + i * d, d, true);
        const double c = sqrt(as_d2(x, cols + (int64_t)j * d, d));
        keep = best <= rad[i] + pmin && c + p[j] - best <= eps;
    }
    if (!keep) {
        col_of[i] = -1;
        owner[j] = -1;
        atomicAdd(&st->unassigned, 1);
    }
}

// ---- one Jacobi round -------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(PF_BLOCK) void k_as_bid(int64_t n_r, int64_t n_c, const int32_t* __restrict__ cand_j,
                                                    const double* __restrict__ cand_c, const double* __restrict__ rad,
                                                    const double* __restrict__ p, const int32_t* __restrict__ col_of,
                                                    int32_t* __restrict__ bid_col, double* __restrict__ bid_val,
                                                    unsigned long long* __restrict__ key, int32_t* __restrict__ queue,
                                                    AsState* __restrict__ st, double eps) {
    const int64_t i = (int64_t)blockIdx.x * PF_BLOCK + threadIdx.x;
    if (i >= n_c || col_of[i] >= 0) return;
    const double pmin = st->pmin;
    Top2 t;
    if (i >= n_r) {  // virtual row: cost 0 everywhere, its values are the prices
        t = Top2{pmin, st->pargmin, st->pmin2};
    } else {
        t = Top2{INFINITY, INT32_MAX, INFINITY};
        const int L = n_c < AS_K ? (int)n_c : AS_K;
        for (int k = 0; k < L; ++k) {
            const int32_t j = cand_j[i * AS_K + k];
            top2_push(t, cand_c[i * AS_K + k] + p[j], j);
        }
        if (!(t.s <= rad[i] + pmin)) {  // a column off the list may be better than the second: scan them all
            queue[atomicAdd(&st->dense_count, 1)] = (int32_t)i;
            atomicAdd(&st->dense_bids, 1ull);
            return;
        }
    }
    const double bid = p[t.j] + (t.s - t.b) + eps;
    bid_col[i] = t.j;
    bid_val[i] = bid;
    atomicMax(&key[t.j], (unsigned long long)__double_as_longlong(bid));
    atomicAdd(&st->bids, 1ull);
}

__global__ __launch_bounds__(PF_BLOCK) void k_as_dense(const double* __restrict__ rows, const double* __restrict__ cols,
                                                      int64_t n_c, int d, const double* __restrict__ p,
                                                      const int32_t* __restrict__ queue, int32_t* __restrict__ bid_col,
                                                      double* __restrict__ bid_val,
                                                      unsigned long long* __restrict__ key, AsState* __restrict__ st,
                                                      double eps) {
    const int count = st->dense_count;
    for (int q = blockIdx.x; q < count; q += gridDim.x) {
        const int32_t i = queue[q];
        double x[AS_DMAX];
        as_load_row(x, rows + (int64_t)i * d, d, true);
        Top2 t{INFINITY, INT32_MAX, INFINITY};
        for (int64_t j = threadIdx.x; j < n_c; j += PF_BLOCK)
            top2_push(t, sqrt(as_d2(x, cols + j * d, d)) + p[j], (int32_t)j);
        double unused = 0.0;
        t = top2_block(t, unused);
        if (threadIdx.x == 0) {
            const double bid = p[t.j] + (t.s - t.b) + eps;
            bid_col[i] = t.j;
            bid_val[i] = bid;
            atomicMax(&key[t.j], (unsigned long long)__double_as_longlong(bid));
            atomicAdd(&st->bids, 1ull);
        }
    }
}

__global__ __launch_bounds__(PF_BLOCK) void k_as_win(int64_t n_c, const int32_t* __restrict__ bid_col,
                                                    const double* __restrict__ bid_val,
                                                    const unsigned long long* __restrict__ key,
                                                    int32_t* __restrict__ win) {
    const int64_t i = (int64_t)blockIdx.x * PF_BLOCK + threadIdx.x;
    if (i >= n_c) return;
    const int32_t j = bid_col[i];
    if (j >= 0 && (unsigned long long)__double_as_longlong(bid_val[i]) == key[j]) atomicMin(&win[j], (int32_t)i);
}

__global__ __launch_bounds__(PF_BLOCK) void k_as_assign(int64_t n_c, int32_t* __restrict__ bid_col,
                                                       const double* __restrict__ bid_val,
                                                       unsigned long long* __restrict__ key, int32_t* __restrict__ win,
                                                       int32_t* __restrict__ owner, int32_t* __restrict__ col_of,
                                                       double* __restrict__ p, AsState* __restrict__ st) {
    const int64_t i = (int64_t)blockIdx.x * PF_BLOCK + threadIdx.x;
    if (i >= n_c) return;
    const int32_t j = bid_col[i];
    if (j < 0) return;
    bid_col[i] = -1;
    if (win[j] != (int32_t)i) return;  // only the winner writes column j's state (and the losers never read it)
    const int32_t o = owner[j];
    if (o >= 0)
        col_of[o] = -1;  // the previous owner placed no bid this round: nobody else touches its entry
    else
        atomicSub(&st->unassigned, 1);
    owner[j] = (int32_t)i;
    col_of[i] = j;
    p[j] = bid_val[i];
    key[j] = 0ull;
    win[j] = INT32_MAX;
}

// ---- dense certificate: u_i = min_j (C_ij + p_j) over every column; cost of the assigned pair -----------------------
__global__ __launch_bounds__(PF_BLOCK) void k_as_cert(const double* __restrict__ rows, int64_t n_r,
                                                     const double* __restrict__ cols, int64_t n_c, int d,
                                                     const double* __restrict__ p, const int32_t* __restrict__ col_of,
                                                     double* __restrict__ u, double* __restrict__ cost) {
    __shared__ double tile[AS_TILE * AS_DMAX];
    __shared__ double tp[AS_TILE];
    const int64_t i = (int64_t)blockIdx.x * PF_BLOCK + threadIdx.x;
    const bool live = i < n_r;
    double x[AS_DMAX];
    as_load_row(x, rows + (live ? i : 0) * d, d, live);
    double ui = INFINITY;
    for (int64_t t0 = 0; t0 < n_c; t0 += AS_TILE) {
        const int cnt = (int)((n_c - t0) < AS_TILE ? (n_c - t0) : AS_TILE);
        __syncthreads();
        for (int e = threadIdx.x; e < cnt * d; e += PF_BLOCK) tile[e] = cols[t0 * d + e];
        for (int e = threadIdx.x; e < cnt; e += PF_BLOCK) tp[e] = p[t0 + e];
        __syncthreads();
        if (!live) continue;
        for (int jj = 0; jj < cnt; ++jj) {
            const double pj = tp[jj];
            const double s = as_d2(x, tile + jj * d, d);
            // sqrt(s) + p_j < u_i needs sqrt(s) < u_i - p_j: skip the square root unless s is below (u_i - p_j)^2,
            // with a margin well above the rounding of u_i - p_j (the minimum itself is exact and order-independent)
            const double t = ui - pj;
            if (t < 0.0) continue;
            const double tm = t + 0x1p-40 * (ui + pj);
            if (s <= tm * tm) ui = fmin(ui, sqrt(s) + pj);
        }
    }
    if (!live) return;
    u[i] = ui;
    cost[i] = sqrt(as_d2(x, cols + (int64_t)col_of[i] * d, d));
}

double host_cost(const double* a, const double* b, int d) {
    double s = 0.0;
    for (int c = 0; c < d; ++c) {
        const double df = a[c] - b[c];
        s += df * df;
    }
    return std::sqrt(s);
}

}  // namespace

extern "C" {

int pf_assign(pf_ctx* ctx, const double* rows, int64_t n_rows, const double* cols, int64_t n_cols, int32_t d,
              int64_t* col_of_row, double* u_out, double* v_out, pf_assign_stats* stats) {
    PF_CHECK(ctx && rows && cols && col_of_row, PF_E_ARG, "pf_assign: NULL argument");
    PF_CHECK(d >= 1 && d <= AS_DMAX && n_rows >= 1 && n_rows <= n_cols && n_cols < ((int64_t)1 << 30), PF_E_ARG,
             "pf_assign: n_rows %lld, n_cols %lld, d %d out of range (1 <= d <= 16, 1 <= n_rows <= n_cols < 2^30)",
             (long long)n_rows, (long long)n_cols, d);
    pf_assign_stats S;
    memset(&S, 0, sizeof(S));
    S.k = AS_K;
    // finite coordinates, and the bounding box of both sets: max C <= its diagonal
    double lo[AS_DMAX], hi[AS_DMAX];
    for (int c = 0; c < d; ++c) {
        lo[c] = INFINITY;
        hi[c] = -INFINITY;
    }
    for (int which = 0; which < 2; ++which) {
        const double* a = which ? cols : rows;
        const int64_t n = which ? n_cols : n_rows;
        for (int64_t i = 0; i < n; ++i)
            for (int c = 0; c < d; ++c) {
                const double v = a[i * d + c];
                PF_CHECK(std::isfinite(v), PF_E_ARG, "pf_assign: non-finite coordinate in %s row %lld",
                         which ? "cols" : "rows", (long long)i);
                lo[c] = std::min(lo[c], v);
                hi[c] = std::max(hi[c], v);
            }
    }
    double diag2 = 0.0;
    for (int c = 0; c < d; ++c) diag2 += (hi[c] - lo[c]) * (hi[c] - lo[c]);
    const double max_c = std::sqrt(diag2);
    if (n_cols == 1 || max_c == 0.0) {
        // one column, or every point the same: every assignment is optimal; row i takes column i
        double total = 0.0;
        for (int64_t i = 0; i < n_rows; ++i) {
            col_of_row[i] = i;
            const double c = host_cost(rows + i * d, cols + i * d, d);
            total += c;
            if (u_out) u_out[i] = c;
        }
        if (v_out)
            for (int64_t j = 0; j < n_cols; ++j) v_out[j] = 0.0;
        if (stats) {
            S.total_cost = S.lower_bound = total;
            *stats = S;
        }
        return PF_OK;
    }

    PF_HIP(hipSetDevice(ctx->device));
    hipStream_t st = ctx->stream;
    const int64_t n_r = n_rows, n_c = n_cols;
    Scratch B(st);
    double* dR = B.get<double>(n_r * d);
    double* dC = B.get<double>(n_c * d);
    int32_t* cand_j = B.get<int32_t>(n_r * AS_K);
    double* cand_c = B.get<double>(n_r * AS_K);
    double* rad = B.get<double>(n_r);
    double* u = B.get<double>(n_r);
    double* cost = B.get<double>(n_r);
    double* p = B.get<double>(n_c);
    double* bid_val = B.get<double>(n_c);
    unsigned long long* key = B.get<unsigned long long>(n_c);
    int32_t* owner = B.get<int32_t>(n_c);
    int32_t* col_of = B.get<int32_t>(n_c);
    int32_t* bid_col = B.get<int32_t>(n_c);
    int32_t* win = B.get<int32_t>(n_c);
    int32_t* queue = B.get<int32_t>(n_c);
    double* part = B.get<double>(4 * AS_PARTS);
    AsState* dst = B.get<AsState>(1);
    if (!B.ok()) {
        pf_set_error("pf_assign: device allocation: %s", hipGetErrorString(B.err));
        (void)hipGetLastError();
        return PF_E_HIP;
    }
    S.device_bytes = (int64_t)B.bytes;
    S.candidate_edges = n_r * (n_c < AS_K ? n_c : AS_K);
    AsState* hst = nullptr;
    PF_TRY(pf_pinned_scratch(ctx, sizeof(AsState), (void**)&hst));
    hipEvent_t ev[4] = {nullptr, nullptr, nullptr, nullptr};
    for (auto& e : ev) PF_HIP(hipEventCreate(&e));
    struct EvGuard {
        hipEvent_t* e;
        ~EvGuard() {
            for (int k = 0; k < 4; ++k)
                if (e[k]) (void)hipEventDestroy(e[k]);
        }
    } ev_guard{ev};

    PF_HIP(hipMemcpyAsync(dR, rows, sizeof(double) * n_r * d, hipMemcpyHostToDevice, st));
    PF_HIP(hipMemcpyAsync(dC, cols, sizeof(double) * n_c * d, hipMemcpyHostToDevice, st));
    PF_HIP(hipMemsetAsync(p, 0, sizeof(double) * n_c, st));
    PF_HIP(hipMemsetAsync(key, 0, sizeof(unsigned long long) * n_c, st));
    PF_HIP(hipMemsetAsync(owner, 0xFF, sizeof(int32_t) * n_c, st));
    PF_HIP(hipMemsetAsync(col_of, 0xFF, sizeof(int32_t) * n_c, st));
    PF_HIP(hipMemsetAsync(bid_col, 0xFF, sizeof(int32_t) * n_c, st));
    PF_HIP(hipMemsetAsync(win, 0x7F, sizeof(int32_t) * n_c, st));  // 0x7F7F7F7F > any row index (n_cols < 2^30)
    AsState init;
    memset(&init, 0, sizeof(init));
    init.unassigned = (int32_t)n_c;
    *hst = init;
    PF_HIP(hipMemcpyAsync(dst, hst, sizeof(AsState), hipMemcpyHostToDevice, st));

    int64_t launches = 0;
    PF_HIP(hipEventRecord(ev[0], st));
    k_as_topk<<<nblk(n_r), PF_BLOCK, 0, st>>>(dR, n_r, dC, n_c, d, cand_j, cand_c, rad, u);
    ++launches;
    PF_HIP(hipGetLastError());
    PF_HIP(hipEventRecord(ev[1], st));
    std::vector<double> h_u(n_r), h_cost(n_r), h_p(n_c);
    std::vector<int32_t> h_col(n_c);
    PF_HIP(hipMemcpyAsync(h_u.data(), u, sizeof(double) * n_r, hipMemcpyDeviceToHost, st));
    PF_HIP(hipStreamSynchronize(st));
    double lb = 0.0;
    for (int64_t i = 0; i < n_r; ++i) lb += h_u[i];
    S.lower_bound = lb;

    // eps schedule: from a few mean nearest distances (the scale on which rows compete; max C / 4 at most) down to
    // eps_target, where n_cols eps <= AS_REL * (a lower bound of the optimum); never below the float64 floor
    const double eps_target = AS_REL * lb / (double)n_c;
    double eps = std::min(max_c / 4.0, 4.0 * lb / (double)n_r);
    eps = std::max(eps, eps_target);
    eps = std::max(eps, 0x1p-43 * max_c);
    S.eps_initial = eps;
    const unsigned parts = std::min<unsigned>(AS_PARTS, nblk(n_c));
    const unsigned grid_c = nblk(n_c);
    double pmin = 0.0, pmax = 0.0;
    int64_t rounds_host = 0;
    bool done = false;
    while (!done) {
        // phase: release what is not eps-optimal any more, then bid until every padded row holds a column
        k_as_prices_part<<<parts, PF_BLOCK, 0, st>>>(p, n_c, part);
        k_as_prices_final<<<1, PF_BLOCK, 0, st>>>(part, (int)parts, dst);
        k_as_release<<<grid_c, PF_BLOCK, 0, st>>>(dR, n_r, dC, n_c, d, cand_j, cand_c, rad, p, owner, col_of, dst, eps);
        launches += 3;
        PF_HIP(hipGetLastError());
        int batch = 4;
        for (;;) {
            for (int b = 0; b < batch; ++b) {
                k_as_prices_part<<<parts, PF_BLOCK, 0, st>>>(p, n_c, part);
                k_as_prices_final<<<1, PF_BLOCK, 0, st>>>(part, (int)parts, dst);
                k_as_bid<<<grid_c, PF_BLOCK, 0, st>>>(n_r, n_c, cand_j, cand_c, rad, p, col_of, bid_col, bid_val, key, queue,
                                                      dst, eps);
                k_as_dense<<<AS_DENSE_BLOCKS, PF_BLOCK, 0, st>>>(dR, dC, n_c, d, p, queue, bid_col, bid_val, key, dst, eps);
                k_as_win<<<grid_c, PF_BLOCK, 0, st>>>(n_c, bid_col, bid_val, key, win);
                k_as_assign<<<grid_c, PF_BLOCK, 0, st>>>(n_c, bid_col, bid_val, key, win, owner, col_of, p, dst);
                launches += 6;
            }
            PF_HIP(hipGetLastError());
            rounds_host += batch;
            PF_HIP(hipMemcpyAsync(hst, dst, sizeof(AsState), hipMemcpyDeviceToHost, st));
            PF_HIP(hipStreamSynchronize(st));
            if (hst->unassigned == 0) break;
            PF_CHECK(rounds_host < AS_MAX_ROUNDS, PF_E_STATE,
                     "pf_assign: the auction did not finish within %lld rounds (eps %g, %d rows unassigned)",
                     (long long)AS_MAX_ROUNDS, eps, hst->unassigned);
            batch = std::min(batch * 2, 64);
        }
        S.phases += 1;
        // the prices after the phase (the floor of eps follows the largest)
        k_as_prices_part<<<parts, PF_BLOCK, 0, st>>>(p, n_c, part);
        k_as_prices_final<<<1, PF_BLOCK, 0, st>>>(part, (int)parts, dst);
        launches += 2;
        PF_HIP(hipMemcpyAsync(hst, dst, sizeof(AsState), hipMemcpyDeviceToHost, st));
        PF_HIP(hipStreamSynchronize(st));
        pmin = hst->pmin;
        pmax = hst->pmax;
        const double floor_eps = 0x1p-43 * (max_c + pmax);
        S.eps_floor = floor_eps;
        if (eps > eps_target && eps > floor_eps) {
            eps = std::max(std::max(eps / AS_SCALE, eps_target), floor_eps);
            continue;
        }
        // dense certificate pass
        PF_HIP(hipEventRecord(ev[2], st));
        k_as_cert<<<nblk(n_r), PF_BLOCK, 0, st>>>(dR, n_r, dC, n_c, d, p, col_of, u, cost);
        ++launches;
        PF_HIP(hipGetLastError());
        PF_HIP(hipEventRecord(ev[3], st));
        S.dense_passes += 1;
        PF_HIP(hipMemcpyAsync(h_u.data(), u, sizeof(double) * n_r, hipMemcpyDeviceToHost, st));
        PF_HIP(hipMemcpyAsync(h_cost.data(), cost, sizeof(double) * n_r, hipMemcpyDeviceToHost, st));
        PF_HIP(hipMemcpyAsync(h_p.data(), p, sizeof(double) * n_c, hipMemcpyDeviceToHost, st));
        PF_HIP(hipMemcpyAsync(h_col.data(), col_of, sizeof(int32_t) * n_c, hipMemcpyDeviceToHost, st));
        PF_HIP(hipStreamSynchronize(st));
        double total = 0.0, gap = 0.0;
        for (int64_t i = 0; i < n_r; ++i) {
            total += h_cost[i];
            gap += h_cost[i] + h_p[h_col[i]] - h_u[i];
        }
        for (int64_t i = n_r; i < n_c; ++i) gap += h_p[h_col[i]] - pmin;
        S.total_cost = total;
        S.gap_bound = gap;
        S.eps_final = eps;
        S.eps_floor_hit = gap > AS_REL * total ? 1 : 0;
        if (gap <= AS_REL * total) {
            done = true;
        } else if (eps > floor_eps) {
            eps = std::max(eps / AS_SCALE, floor_eps);  // rounding kept the bound above the target: one more phase
        } else if (gap <= (double)n_c * eps * (1.0 + 1e-6)) {
            done = true;  // eps cannot shrink further: the auction's own promise, n_cols * eps, is what is certified
        } else {
            PF_CHECK(false, PF_E_STATE,
                     "pf_assign: gap bound %.3g exceeds n_cols * eps = %.3g at the float64 floor of eps; costs %.3g, prices %.3g",
                     gap, (double)n_c * eps, max_c, pmax);
        }
    }
    for (int64_t i = 0; i < n_r; ++i) col_of_row[i] = h_col[i];
    // the duals in the rectangular problem's form: v_j = p_min - p_j <= 0, u_i = min_j (C_ij - v_j) = u_i - p_min
    if (u_out)
        for (int64_t i = 0; i < n_r; ++i) u_out[i] = h_u[i] - pmin;
    if (v_out)
        for (int64_t j = 0; j < n_c; ++j) v_out[j] = pmin - h_p[j];
    S.bids = (int64_t)hst->bids;
    S.dense_bids = (int64_t)hst->dense_bids;
    S.rounds = (int64_t)hst->rounds;
    S.launches = launches;
    float ms = 0.f;
    if (hipEventElapsedTime(&ms, ev[0], ev[1]) == hipSuccess) S.ms_candidates = ms;
    if (hipEventElapsedTime(&ms, ev[1], ev[2]) == hipSuccess) S.ms_auction = ms;
    if (hipEventElapsedTime(&ms, ev[2], ev[3]) == hipSuccess) S.ms_certificate = ms;
    (void)hipGetLastError();
    if (stats) *stats = S;
    return PF_OK;
}

}  // extern "C"
