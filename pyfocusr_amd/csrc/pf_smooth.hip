// Explicit smoothing of a triangle mesh (pf_smoother_*): Laplacian and Taubin fairing of the points, or of any field of
// 1..32 columns on the vertices, by Jacobi sweeps over a CSR adjacency that is built once per mesh.  The definitions are
// in include/pyfocusr_hip.h; tests/_smoothing_ref.py restates them in numpy and the device returns its bits.
//
// The build is the half-edge pass of pf_halfedge.h as far as the edges, then a second sort:
//   k_sm_triangles  one thread per triangle: the keys of its three half-edges' edges, h as the sort's value; for cotangent
//                   weights the half cotangent at every corner
//   (stable sort by edge key; k_sm_heads flags the first half-edge of every run whose ends differ; exclusive scan: the
//    edges numbered in key order; the one read-back of the build: their count)
//   k_sm_edges      one thread per edge (the head of its run): the weight summed over the run in ascending h, whether the
//                   run is a single half-edge, the two directed entries 2 p (lo -> hi) and 2 p + 1 (hi -> lo) as keys
//                   (source vertex) and values of the second sort; the edge counts
//   (stable sort by source vertex: emitted in key order, a vertex's entries arrive in ascending neighbour)
//   k_sm_gather     one thread per sorted entry: column, weight, boundary flag
//   k_sm_rows       one thread per vertex: its row's start by bisection (he_vertex_run)
//   k_sm_kinds      one thread per vertex: boundary | pinned | movable, the largest row, the movable count
// and a run is n_sweeps launches of
//   k_sm_sweep3     ncols = 3: one thread per vertex, the row gathered in ascending neighbour, the clamp folded in
//   k_sm_sweep      any ncols: one thread per (vertex, column)
// that ping-pong two buffers; the input stays as it is, for the clamp and the stats:
//   k_sm_volume_terms, k_sm_max_move, and k_tree_level (pf_tree.h) for the two volumes and the vertex mean.
// A sweep reads every neighbour's previous value, so it stays one launch: no block waits for another.  No floating-point
// atomics; the counts and the largest move are integer atomics: two calls give the same bits.  Arithmetic: f64, separate
// multiplies and adds (-ffp-contract=off), dot products left to right.
#include <cmath>
#include <cstring>

#include "pf_halfedge.h"
#include "pf_tree.h"

enum { SM_BOUNDARY = 1, SM_PINNED = 2, SM_MOVABLE = 4 };  // bits of a vertex's kind
// counts: edges | boundary edges | non-manifold edges | entries | largest row | movable vertices
enum { SM_N_EDGES, SM_N_BOUNDARY, SM_N_NONMANIFOLD, SM_N_ENTRIES, SM_N_MAXROW, SM_N_MOVABLE, SM_N_COUNTS };

struct pf_smoother {
    pf_ctx* ctx = nullptr;
    int64_t n = 0, n_faces = 0, nnz = 0;
    int32_t weights = 0, mode = 0;
    double* pts = nullptr;      // [n][3]
    int32_t* faces = nullptr;   // [n_faces][3]: the volumes of the stats
    int32_t* rowptr = nullptr;  // [n + 1]
    int32_t* col = nullptr;     // [nnz] ascending inside a row
    double* w = nullptr;        // [nnz] cotangent weights; NULL: uniform
    uint8_t* ebf = nullptr;     // [nnz] 1: the entry's edge is a boundary edge; kept for PF_SMOOTH_CURVE only
    uint8_t* kind = nullptr;    // [n]
    int64_t counts[SM_N_COUNTS] = {0, 0, 0, 0, 0, 0};
};

namespace {

typedef unsigned long long u64;

// counts[slot] += the lanes of the wave for which `on` holds: one atomic per wave (every lane of the wave calls this)
__device__ __forceinline__ void count_lanes(u64* __restrict__ counts, int slot, bool on) {
    const u64 mask = __ballot(on);
    if (mask != 0ull && (int)(threadIdx.x & (PF_WAVE - 1)) == __ffsll((long long)mask) - 1) atomicAdd(&counts[slot], (u64)__popcll(mask));
}

// One thread per triangle: per half-edge 3 t + j the key of its edge and h itself; with hcot, per corner k the half
// cotangent 0.5 (u . v) / |u x v| of the edges u, v that leave it for the next and the one after - 0 at all three corners
// when |u x v| is 0 or not finite at one of them.
__global__ __launch_bounds__(PF_BLOCK) void k_sm_triangles(const double* __restrict__ pts, const int32_t* __restrict__ faces, int64_t n_tri,
                                                           int nb, u64* __restrict__ ekey, int32_t* __restrict__ hval,
                                                           double* __restrict__ hcot) {
    const int64_t t = (int64_t)blockIdx.x * PF_BLOCK + threadIdx.x;
    if (t >= n_tri) return;
    const int32_t v[3] = {faces[3 * t], faces[3 * t + 1], faces[3 * t + 2]};
#pragma unroll
    for (int j = 0; j < 3; ++j) {
        ekey[3 * t + j] = he_edge_key(v[j], v[he_next(j)], nb);
        hval[3 * t + j] = (int32_t)(3 * t + j);
    }
    if (!hcot) return;
    double x[3][3], hc[3];
#pragma unroll
    for (int c = 0; c < 3; ++c)
#pragma unroll
        for (int a = 0; a < 3; ++a) x[c][a] = pts[3 * (int64_t)v[c] + a];
    bool area = true;
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        const int k1 = he_next(k), k2 = he_prev(k);
        const double u[3] = {x[k1][0] - x[k][0], x[k1][1] - x[k][1], x[k1][2] - x[k][2]};
        const double w[3] = {x[k2][0] - x[k][0], x[k2][1] - x[k][1], x[k2][2] - x[k][2]};
        double c[3];
        cross3(u, w, c);
        const double nrm = sqrt(dot3(c, c));
        area = area && nrm > 0.0 && std::isfinite(nrm);
        hc[k] = 0.5 * (dot3(u, w) / nrm);
    }
#pragma unroll
    for (int k = 0; k < 3; ++k) hcot[3 * t + k] = area ? hc[k] : 0.0;
}

// flag [n_half + 1]: 1 at the sorted position that heads the run of an edge whose two ends differ; 0 elsewhere and at
// n_half (the scan's total lands there)
__global__ __launch_bounds__(PF_BLOCK) void k_sm_heads(const u64* __restrict__ ekey, int64_t n_half, int nb, int32_t* __restrict__ flag) {
    const int64_t i = (int64_t)blockIdx.x * PF_BLOCK + threadIdx.x;
    if (i > n_half) return;
    int32_t f = 0;
    if (i < n_half) {
        const u64 key = ekey[i];
        const bool head = i == 0 || ekey[i - 1] != key;
        f = head && (key >> nb) != (key & ((1ull << nb) - 1ull)) ? 1 : 0;
    }
    flag[i] = f;
}

// One thread per edge: the flagged position i, whose run is in ascending h (the sort is stable).  Edge p = pos[i] in key
// order: its ends lo < hi, its weight (1.0, or with hcot max(0, the sum over the run of the half cotangent at the corner
// opposite each half-edge)), whether the run is a single half-edge, and its two directed entries for the second sort.
__global__ __launch_bounds__(PF_BLOCK) void k_sm_edges(const u64* __restrict__ ekey, const int32_t* __restrict__ hedge, int64_t n_half, int nb,
                                                       const int32_t* __restrict__ flag, const int32_t* __restrict__ pos,
                                                       const double* __restrict__ hcot, int32_t* __restrict__ elo,
                                                       int32_t* __restrict__ ehi, double* __restrict__ ew, uint8_t* __restrict__ ebnd,
                                                       unsigned* __restrict__ skey, int32_t* __restrict__ sval, u64* __restrict__ counts) {
    const int64_t i = (int64_t)blockIdx.x * PF_BLOCK + threadIdx.x;
    if (i >= n_half || !flag[i]) return;
    const u64 key = ekey[i];
    int64_t end = i + 1;
    while (end < n_half && ekey[end] == key) ++end;
    double w = 1.0;
    if (hcot) {
        double s = 0.0;
        for (int64_t k = i; k < end; ++k) {
            const int64_t h = hedge[k], t = h / 3;
            s += hcot[3 * t + he_prev((int)(h - 3 * t))];
        }
        w = s > 0.0 ? s : 0.0;
    }
    const int64_t p = pos[i];
    const int32_t lo = (int32_t)(key >> nb), hi = (int32_t)(key & ((1ull << nb) - 1ull));
    elo[p] = lo, ehi[p] = hi, ew[p] = w, ebnd[p] = end - i == 1 ? 1 : 0;
    skey[2 * p] = (unsigned)lo, sval[2 * p] = (int32_t)(2 * p);
    skey[2 * p + 1] = (unsigned)hi, sval[2 * p + 1] = (int32_t)(2 * p + 1);
    he_count_edge(counts, end - i, false, true);  // (orientation is not looked at here: counts[3] stays 0)
}

// one thread per entry in row order: entry e = 2 p + d of edge p goes from lo to hi (d = 0) or back
__global__ __launch_bounds__(PF_BLOCK) void k_sm_gather(const int32_t* __restrict__ sval, int64_t nnz, const int32_t* __restrict__ elo,
                                                        const int32_t* __restrict__ ehi, const double* __restrict__ ew,
                                                        const uint8_t* __restrict__ ebnd, int32_t* __restrict__ col, double* __restrict__ w,
                                                        uint8_t* __restrict__ ebf) {
    const int64_t i = (int64_t)blockIdx.x * PF_BLOCK + threadIdx.x;
    if (i >= nnz) return;
    const int32_t e = sval[i], p = e >> 1;
    col[i] = (e & 1) ? elo[p] : ehi[p];
    if (w) w[i] = ew[p];
    ebf[i] = ebnd[p];
}

__global__ __launch_bounds__(PF_BLOCK) void k_sm_rows(const unsigned* __restrict__ skey, int64_t nnz, int64_t n, int32_t* __restrict__ rowptr) {
    const int64_t v = (int64_t)blockIdx.x * PF_BLOCK + threadIdx.x;
    if (v <= n) rowptr[v] = (int32_t)he_vertex_run(skey, nnz, v);
}

// One thread per vertex: boundary (an entry of its row is a boundary edge), pinned, and movable: neither pinned nor, with
// PF_SMOOTH_FIXED, boundary, and the weights a sweep divides by sum to more than 0 (summed as the sweep sums them).
__global__ __launch_bounds__(PF_BLOCK) void k_sm_kinds(int64_t n, const int32_t* __restrict__ rowptr, const double* __restrict__ w,
                                                       const uint8_t* __restrict__ ebf, const uint8_t* __restrict__ pinned, int mode,
                                                       uint8_t* __restrict__ kind, u64* __restrict__ counts) {
    const int64_t v = (int64_t)blockIdx.x * PF_BLOCK + threadIdx.x;
    const bool live = v < n;
    bool movable = false;
    if (live) {
        const int32_t lo = rowptr[v], hi = rowptr[v + 1];
        bool boundary = false;
        for (int32_t e = lo; e < hi; ++e) boundary = boundary || ebf[e];
        double sw = (double)(hi - lo);
        if (w && !(mode == PF_SMOOTH_CURVE && boundary)) {
            sw = 0.0;
            for (int32_t e = lo; e < hi; ++e) sw += w[e];
        }
        const bool pin = pinned && pinned[v];
        movable = !pin && !(mode == PF_SMOOTH_FIXED && boundary) && sw > 0.0;
        kind[v] = (uint8_t)((boundary ? SM_BOUNDARY : 0) | (pin ? SM_PINNED : 0) | (movable ? SM_MOVABLE : 0));
        if (hi > lo) atomicMax(&counts[SM_N_MAXROW], (u64)(hi - lo));
    }
    count_lanes(counts, SM_N_MOVABLE, movable);
}

// This thread's row of vertex v for column a of `in` [n][ncols]: s = the running sum of w x_u in ascending u and sw the
// sum of the w; plain sums and the count without w; over the boundary entries alone with curve.
template <bool WEIGHTED>
__device__ __forceinline__ void row_sum(const int32_t* __restrict__ col, const double* __restrict__ w, const uint8_t* __restrict__ ebf,
                                        bool curve, int32_t lo, int32_t hi, const double* __restrict__ in, int ncols, int a, double& s,
                                        double& sw) {
    s = 0.0, sw = 0.0;
    if (curve) {
        for (int32_t e = lo; e < hi; ++e)
            if (ebf[e]) {
                s += in[(int64_t)col[e] * ncols + a];
                sw += 1.0;
            }
    } else if (WEIGHTED) {
        for (int32_t e = lo; e < hi; ++e) {
            const double we = w[e];
            s += we * in[(int64_t)col[e] * ncols + a];
            sw += we;
        }
    } else {
        for (int32_t e = lo; e < hi; ++e) s += in[(int64_t)col[e] * ncols + a];
        sw = (double)(hi - lo);
    }
}

// One sweep with factor f over three columns, one thread per vertex: x' = x + f (s / sw - x) for a movable vertex, then
// with CLAMP x' into [x0 - c, x0 + c]; every other vertex keeps its bits.  ebf: PF_SMOOTH_CURVE (else NULL).
template <bool WEIGHTED, bool CLAMP>
__global__ __launch_bounds__(PF_BLOCK) void k_sm_sweep3(int64_t n, const int32_t* __restrict__ rowptr, const int32_t* __restrict__ col,
                                                        const double* __restrict__ w, const uint8_t* __restrict__ ebf,
                                                        const uint8_t* __restrict__ kind, const double* __restrict__ in,
                                                        const double* __restrict__ x0, double c0, double c1, double c2, double f,
                                                        double* __restrict__ out) {
    const int64_t v = (int64_t)blockIdx.x * PF_BLOCK + threadIdx.x;
    if (v >= n) return;
    double y[3] = {in[3 * v], in[3 * v + 1], in[3 * v + 2]};
    const int k = kind[v];
    if (k & SM_MOVABLE) {
        const int32_t lo = rowptr[v], hi = rowptr[v + 1];
        double s[3] = {0.0, 0.0, 0.0}, sw = 0.0;
        if (ebf && (k & SM_BOUNDARY)) {
            for (int32_t e = lo; e < hi; ++e)
                if (ebf[e]) {
                    const double* p = in + 3 * (int64_t)col[e];
                    s[0] += p[0], s[1] += p[1], s[2] += p[2];
                    sw += 1.0;
                }
        } else if (WEIGHTED) {
            for (int32_t e = lo; e < hi; ++e) {
                const double we = w[e];
                const double* p = in + 3 * (int64_t)col[e];
                s[0] += we * p[0], s[1] += we * p[1], s[2] += we * p[2];
                sw += we;
            }
        } else {
            for (int32_t e = lo; e < hi; ++e) {
                const double* p = in + 3 * (int64_t)col[e];
                s[0] += p[0], s[1] += p[1], s[2] += p[2];
            }
            sw = (double)(hi - lo);
        }
        const double c[3] = {c0, c1, c2};
#pragma unroll
        for (int a = 0; a < 3; ++a) {
            double r = y[a] + f * (s[a] / sw - y[a]);
            if (CLAMP) {
                const double b0 = x0[3 * v + a] - c[a], b1 = x0[3 * v + a] + c[a];
                r = r < b0 ? b0 : r;
                r = r > b1 ? b1 : r;
            }
            y[a] = r;
        }
    }
    out[3 * v] = y[0], out[3 * v + 1] = y[1], out[3 * v + 2] = y[2];
}

// The same sweep for any ncols, one thread per (vertex, column); clamp [ncols] on the device, or NULL.
template <bool WEIGHTED>
__global__ __launch_bounds__(PF_BLOCK) void k_sm_sweep(int64_t n, int ncols, const int32_t* __restrict__ rowptr, const int32_t* __restrict__ col,
                                                       const double* __restrict__ w, const uint8_t* __restrict__ ebf,
                                                       const uint8_t* __restrict__ kind, const double* __restrict__ in,
                                                       const double* __restrict__ x0, const double* __restrict__ clamp, double f,
                                                       double* __restrict__ out) {
    const int64_t idx = (int64_t)blockIdx.x * PF_BLOCK + threadIdx.x;
    if (idx >= n * ncols) return;
    const int64_t v = idx / ncols;
    const int a = (int)(idx - v * ncols);
    double y = in[idx];
    const int k = kind[v];
    if (k & SM_MOVABLE) {
        double s, sw;
        row_sum<WEIGHTED>(col, w, ebf, ebf && (k & SM_BOUNDARY), rowptr[v], rowptr[v + 1], in, ncols, a, s, sw);
        y = y + f * (s / sw - y);
        if (clamp) {
            const double b0 = x0[idx] - clamp[a], b1 = x0[idx] + clamp[a];
            y = y < b0 ? b0 : y;
            y = y > b1 ? b1 : y;
        }
    }
    out[idx] = y;
}

// term [n_tri][2]: a . (b x c) of the face's corners in x0, then in x
__global__ __launch_bounds__(PF_BLOCK) void k_sm_volume_terms(const int32_t* __restrict__ faces, int64_t n_tri, const double* __restrict__ x0,
                                                              const double* __restrict__ x, double* __restrict__ term) {
    const int64_t t = (int64_t)blockIdx.x * PF_BLOCK + threadIdx.x;
    if (t >= n_tri) return;
    const int64_t v0 = faces[3 * t], v1 = faces[3 * t + 1], v2 = faces[3 * t + 2];
#pragma unroll
    for (int q = 0; q < 2; ++q) {
        const double* p = q ? x : x0;
        const double a[3] = {p[3 * v0], p[3 * v0 + 1], p[3 * v0 + 2]}, b[3] = {p[3 * v1], p[3 * v1 + 1], p[3 * v1 + 2]};
        const double c[3] = {p[3 * v2], p[3 * v2 + 1], p[3 * v2 + 2]};
        double cr[3];
        cross3(b, c, cr);
        term[2 * t + q] = dot3(a, cr);
    }
}

// *most = the largest |x - x0| over `count` components, as the bits of a non-negative double (which order like integers);
// the wave's largest first, one atomic per wave
__global__ __launch_bounds__(PF_BLOCK) void k_sm_max_move(const double* __restrict__ x0, const double* __restrict__ x, int64_t count,
                                                          u64* __restrict__ most) {
    const int64_t i = (int64_t)blockIdx.x * PF_BLOCK + threadIdx.x;
    double d = i < count ? fabs(x[i] - x0[i]) : 0.0;
    if (!(d >= 0.0)) d = 0.0;
#pragma unroll
    for (int off = PF_WAVE / 2; off > 0; off >>= 1) {
        const double o = __shfl_xor(d, off);
        d = o > d ? o : d;
    }
    if ((threadIdx.x & (PF_WAVE - 1)) == 0 && d > 0.0) atomicMax(most, (u64)__double_as_longlong(d));
}

void release(pf_smoother* h) {
    hipStream_t st = h->ctx->stream;
    pf_free(st, h->pts);
    pf_free(st, h->faces);
    pf_free(st, h->rowptr);
    pf_free(st, h->col);
    pf_free(st, h->w);
    pf_free(st, h->ebf);
    pf_free(st, h->kind);
    delete h;
}

}  // namespace

extern "C" {

void pf_smoother_free(pf_smoother* h) {
    if (!h) return;
    hipSetDevice(h->ctx->device);
    hipStreamSynchronize(h->ctx->stream);
    release(h);
}

int pf_smoother_create(pf_ctx* ctx, const double* pts, int64_t n, const int32_t* faces, int64_t n_faces, int32_t weights,
                       int32_t boundary_mode, const uint8_t* pinned, pf_smoother** out) {
    PF_CHECK(ctx && pts && faces && out, PF_E_ARG, "pf_smoother_create: NULL argument");
    PF_CHECK(n > 0 && n < ((int64_t)1 << 31), PF_E_ARG, "pf_smoother_create: n = %lld out of range", (long long)n);
    PF_CHECK(n_faces > 0 && 3 * n_faces < ((int64_t)1 << 31), PF_E_ARG, "pf_smoother_create: %lld faces out of range (3 n_faces < 2^31)",
             (long long)n_faces);
    PF_CHECK(weights == PF_SMOOTH_UNIFORM || weights == PF_SMOOTH_COTANGENT, PF_E_ARG, "pf_smoother_create: weights = %d", (int)weights);
    PF_CHECK(boundary_mode == PF_SMOOTH_FREE || boundary_mode == PF_SMOOTH_FIXED || boundary_mode == PF_SMOOTH_CURVE, PF_E_ARG,
             "pf_smoother_create: boundary_mode = %d", (int)boundary_mode);
    const int64_t T = n_faces, H = 3 * T;
    PF_TRY(pf_check_faces("pf_smoother_create", faces, T, 3, n, false));
    const int nb = pf_index_bits(n);  // bits of a vertex index
    const bool cot = weights == PF_SMOOTH_COTANGENT;
    PF_HIP(hipSetDevice(ctx->device));
    hipStream_t st = ctx->stream;
    pf_smoother* h = new pf_smoother();
    h->ctx = ctx, h->n = n, h->n_faces = T, h->weights = weights, h->mode = boundary_mode;
    u64 counts[SM_N_COUNTS] = {0, 0, 0, 0, 0, 0};
    hipError_t err;
    {
        Scratch sc(st);  // what is kept is the handle's: release gives back whatever a failure leaves
        h->pts = sc.keep<double>(3 * n);
        h->faces = sc.keep<int32_t>(H);
        h->rowptr = sc.keep<int32_t>(n + 1);
        h->kind = sc.keep<uint8_t>(n);
        u64 *ek0 = sc.get<u64>(H), *ek1 = sc.get<u64>(H);
        int32_t *h0 = sc.get<int32_t>(H), *h1 = sc.get<int32_t>(H);
        double* hcot = cot ? sc.get<double>(H) : nullptr;
        int32_t *flag = sc.get<int32_t>(H + 1), *pos = sc.get<int32_t>(H + 1);
        uint8_t* d_pinned = pinned ? sc.get<uint8_t>(n) : nullptr;
        u64* cnt = sc.get<u64>(SM_N_COUNTS);
        sc.upload(h->pts, pts, 3 * n);
        sc.upload(h->faces, faces, H);
        if (pinned) sc.upload(d_pinned, pinned, n);
        sc.zero(cnt, sizeof(u64) * SM_N_COUNTS);
        if (sc.ok()) {
            k_sm_triangles<<<pf_blocks(T), PF_BLOCK, 0, st>>>(h->pts, h->faces, T, nb, ek0, h0, hcot);
            sc.launched();
        }
        pf_sort_pairs(sc, ek0, ek1, h0, h1, H, 2 * nb);  // stable: the half-edges of an edge stay in ascending h
        if (sc.ok()) {
            k_sm_heads<<<pf_blocks(H + 1), PF_BLOCK, 0, st>>>(ek1, H, nb, flag);
            sc.launched();
        }
        if (sc.ok() && pf_exclusive_scan_i32(st, flag, pos, H + 1) != PF_OK) sc.note(hipErrorUnknown);
        int32_t n_edges = 0;  // the one read-back before the entries are sized
        sc.download(&n_edges, pos + H, 1);
        sc.sync();
        const int64_t E = n_edges, nnz = 2 * E;
        if (nnz >= ((int64_t)1 << 31)) {  // the adjacency is int32
            release(h);
            pf_set_error("pf_smoother_create: %lld entries out of range (2 edges < 2^31)", (long long)nnz);
            return PF_E_ARG;
        }
        h->nnz = nnz;
        int32_t *elo = sc.get<int32_t>(E), *ehi = sc.get<int32_t>(E);
        double* ew = sc.get<double>(E);
        uint8_t* ebnd = sc.get<uint8_t>(E);
        unsigned *sk0 = sc.get<unsigned>(nnz), *sk1 = sc.get<unsigned>(nnz);
        int32_t *sv0 = sc.get<int32_t>(nnz), *sv1 = sc.get<int32_t>(nnz);
        h->col = sc.keep<int32_t>(nnz);
        if (cot) h->w = sc.keep<double>(nnz);
        h->ebf = sc.keep<uint8_t>(nnz);
        if (sc.ok() && E > 0) {
            k_sm_edges<<<pf_blocks(H), PF_BLOCK, 0, st>>>(ek1, h1, H, nb, flag, pos, hcot, elo, ehi, ew, ebnd, sk0, sv0, cnt);
            sc.launched();
        }
        // stable, from edge-key order: the entries of a vertex arrive as (u, v), u < v ascending, then (v, u), u > v ascending
        if (E > 0) pf_sort_pairs(sc, sk0, sk1, sv0, sv1, nnz, nb);
        if (sc.ok()) {
            if (E > 0) k_sm_gather<<<pf_blocks(nnz), PF_BLOCK, 0, st>>>(sv1, nnz, elo, ehi, ew, ebnd, h->col, h->w, h->ebf);
            k_sm_rows<<<pf_blocks(n + 1), PF_BLOCK, 0, st>>>(sk1, nnz, n, h->rowptr);
            k_sm_kinds<<<pf_blocks(n), PF_BLOCK, 0, st>>>(n, h->rowptr, h->w, h->ebf, d_pinned, (int)boundary_mode, h->kind, cnt);
            sc.launched();
        }
        sc.download(counts, cnt, SM_N_COUNTS);
        sc.sync();
        err = sc.err;
    }
    if (err == hipSuccess && boundary_mode != PF_SMOOTH_CURVE) {  // only the curve mode's sweeps read the entries' flags
        pf_free(st, h->ebf);
        h->ebf = nullptr;
    }
    if (err != hipSuccess) {
        release(h);
        return pf_hip_failed("pf_smoother_create", err);
    }
    for (int k = 0; k < SM_N_COUNTS; ++k) h->counts[k] = (int64_t)counts[k];
    h->counts[SM_N_ENTRIES] = h->nnz;
    *out = h;
    return PF_OK;
}

int pf_smoother_info(const pf_smoother* h, int64_t* counts) {
    PF_CHECK(h && counts, PF_E_ARG, "pf_smoother_info: NULL argument");
    for (int k = 0; k < SM_N_COUNTS; ++k) counts[k] = h->counts[k];
    return PF_OK;
}

int pf_smoother_adjacency(pf_smoother* h, int32_t* rowptr, int32_t* col, double* w, uint8_t* kind) {
    PF_CHECK(h != nullptr, PF_E_ARG, "pf_smoother_adjacency: NULL handle");
    PF_HIP(hipSetDevice(h->ctx->device));
    Scratch sc(h->ctx->stream);
    sc.download(rowptr, h->rowptr, h->n + 1);
    if (h->nnz) sc.download(col, h->col, h->nnz);
    if (h->nnz && h->w) sc.download(w, h->w, h->nnz);
    sc.download(kind, h->kind, h->n);
    sc.sync();
    if (!sc.ok()) return pf_hip_failed("pf_smoother_adjacency", sc.err);
    for (int64_t e = 0; w && !h->w && e < h->nnz; ++e) w[e] = 1.0;
    return PF_OK;
}

int pf_smoother_run(pf_smoother* h, const double* values, int32_t ncols, const double* factors, int32_t n_sweeps, int32_t clamp_every,
                    const double* clamp, double* out, double* stats, double* device_ms) {
    PF_CHECK(h && out, PF_E_ARG, "pf_smoother_run: NULL argument");
    PF_CHECK(ncols >= 1 && ncols <= 32, PF_E_ARG, "pf_smoother_run: ncols = %d out of range (1..32)", (int)ncols);
    PF_CHECK(values || ncols == 3, PF_E_ARG, "pf_smoother_run: the points have 3 columns, not %d", (int)ncols);
    PF_CHECK(!stats || !values, PF_E_ARG, "pf_smoother_run: the stats are those of the mesh's own points");
    PF_CHECK(n_sweeps >= 0 && (n_sweeps == 0 || factors), PF_E_ARG, "pf_smoother_run: %d sweeps need their factors", (int)n_sweeps);
    for (int32_t s = 0; s < n_sweeps; ++s)
        PF_CHECK(std::isfinite(factors[s]), PF_E_ARG, "pf_smoother_run: factor %d is not finite", (int)s);
    PF_CHECK(!clamp || clamp_every >= 1, PF_E_ARG, "pf_smoother_run: clamp_every = %d", (int)clamp_every);
    for (int a = 0; clamp && a < ncols; ++a)
        PF_CHECK(clamp[a] >= 0.0, PF_E_ARG, "pf_smoother_run: bound %d is negative or not a number", a);
    PF_HIP(hipSetDevice(h->ctx->device));
    hipStream_t st = h->ctx->stream;
    const int64_t n = h->n, T = h->n_faces, count = n * ncols;
    StreamTimer timer(device_ms != nullptr);
    double vol[2] = {0.0, 0.0}, mean[3] = {0.0, 0.0, 0.0};
    u64 most = 0;
    hipError_t err;
    {
        Scratch sc(st);
        double* d_in = values ? sc.get<double>(count) : nullptr;
        double* buf[2] = {nullptr, nullptr};
        for (int b = 0; b < 2 && b < n_sweeps; ++b) buf[b] = sc.get<double>(count);
        double* d_clamp = clamp && ncols != 3 ? sc.get<double>(ncols) : nullptr;
        if (values) sc.upload(d_in, values, count);
        if (d_clamp) sc.upload(d_clamp, clamp, ncols);
        const double* x0 = values ? d_in : h->pts;
        const double* cur = x0;
        timer.start(sc);
        for (int32_t s = 0; s < n_sweeps && sc.ok(); ++s) {
            double* dst = buf[s & 1];
            const bool clamped = clamp && (s + 1) % clamp_every == 0;
            const double f = factors[s];
            if (ncols == 3) {
                const double c0 = clamped ? clamp[0] : 0.0, c1 = clamped ? clamp[1] : 0.0, c2 = clamped ? clamp[2] : 0.0;
                const unsigned grid = pf_blocks(n);
                if (h->w && clamped)
                    k_sm_sweep3<true, true><<<grid, PF_BLOCK, 0, st>>>(n, h->rowptr, h->col, h->w, h->ebf, h->kind, cur, x0, c0, c1, c2, f, dst);
                else if (h->w)
                    k_sm_sweep3<true, false><<<grid, PF_BLOCK, 0, st>>>(n, h->rowptr, h->col, h->w, h->ebf, h->kind, cur, x0, c0, c1, c2, f, dst);
                else if (clamped)
                    k_sm_sweep3<false, true><<<grid, PF_BLOCK, 0, st>>>(n, h->rowptr, h->col, h->w, h->ebf, h->kind, cur, x0, c0, c1, c2, f, dst);
                else
                    k_sm_sweep3<false, false><<<grid, PF_BLOCK, 0, st>>>(n, h->rowptr, h->col, h->w, h->ebf, h->kind, cur, x0, c0, c1, c2, f, dst);
            } else {
                const double* dc = clamped ? d_clamp : nullptr;
                if (h->w)
                    k_sm_sweep<true><<<pf_blocks(count), PF_BLOCK, 0, st>>>(n, (int)ncols, h->rowptr, h->col, h->w, h->ebf, h->kind, cur, x0, dc, f, dst);
                else
                    k_sm_sweep<false><<<pf_blocks(count), PF_BLOCK, 0, st>>>(n, (int)ncols, h->rowptr, h->col, h->w, h->ebf, h->kind, cur, x0, dc, f, dst);
            }
            sc.launched();
            cur = dst;
        }
        if (stats) {
            double* term = sc.get<double>(2 * T);
            u64* d_most = sc.get<u64>(1);
            sc.zero(d_most, sizeof(u64));
            if (sc.ok()) {
                k_sm_volume_terms<<<pf_blocks(T), PF_BLOCK, 0, st>>>(h->faces, T, x0, cur, term);
                k_sm_max_move<<<pf_blocks(count), PF_BLOCK, 0, st>>>(x0, cur, count, d_most);
                sc.launched();
            }
            const double* d_vol = pf_tree_reduce(sc, term, T, 2, 0);
            const double* d_mean = pf_tree_reduce(sc, cur, n, 3, 0);
            timer.stop(sc);
            sc.download(vol, d_vol, 2);
            sc.download(mean, d_mean, 3);
            sc.download(&most, d_most, 1);
        } else {
            timer.stop(sc);
        }
        sc.download(out, cur, count);
        sc.sync();
        timer.read(sc, device_ms);
        err = sc.err;
    }
    if (err != hipSuccess) return pf_hip_failed("pf_smoother_run", err);
    if (stats) {
        double d;
        memcpy(&d, &most, sizeof(d));
        stats[0] = vol[0] / 6.0, stats[1] = vol[1] / 6.0;
        for (int a = 0; a < 3; ++a) stats[2 + a] = mean[a] / (double)n;
        stats[5] = d;
    }
    return PF_OK;
}

}  // extern "C"
