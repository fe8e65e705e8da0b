// Uniform resampling of a triangle mesh by clustering (pf_mesh_cluster): Lloyd iterations over the vertices, one
// representative per cluster, and the triangulation that the clusters' adjacency induces.  The definition is in
// include/pyfocusr_hip.h; tests/_remesh_ref.py restates it in numpy and the device returns its bits.
//
// d2(i, j) = ((dx * dx + dy * dy) + dz * dz), separate multiplies and adds (the library is built without contraction), as in
// pf_fps.hip and pf_knn.hip.  Every choice is total - smaller d2, then lower index - so no order of evaluation matters.
//
// Assignment (n vertices against m moving centroids, every iteration):
//   k_grid_spec    one block: the centroids' bounding box and from it a uniform grid of about 2 m cells of edge h over the
//                  axes that have an extent (an axis without one has a single layer of cells)
//   k_cell_ids     one thread per centroid: its cell; one stable radix sort by cell
//   k_cell_starts  one thread per sorted centroid: start[] of every cell up to its own (CSR; the gaps of empty cells are
//                  filled by the thread behind them), and the centroid's coordinates and index in sorted order
//   k_assign       one thread per vertex.  The best so far starts at the centroid of the vertex's previous label.  The cells
//                  are visited in rings r = 0, 1, ... of equal Chebyshev distance around the vertex's own (clamped) cell,
//                  each row of a ring as one contiguous range of the sorted centroids, until the ring's lower bound
//                  ((r - 1) h)^2 (1 - 2^-20) is strictly greater than the best (an equal candidate with a lower index must
//                  still be seen), or the grid is exhausted.
//                  Why the bound holds in floating point.  cell(v) = floor(fl(fl(v - lo) * inv_h)), clamped, is the same
//                  monotone function for vertices and centroids.  A centroid r cells away along an axis is, in exact
//                  arithmetic, more than (r - 1) h (1 - 2^-29) away (two roundings of relative 2^-53 on a cell coordinate
//                  below 2^21; clamping only ever moves a cell towards the other point), and the computed d2 is at least the
//                  computed square of that one difference, three more roundings.  2^-20 covers all of it many times over.
// Update:
//   one stable radix sort of the vertices by label; k_label_starts (CSR as above); k_run_sums one thread per run of 64
//   consecutive members: a_i x_i, a_i y_i, a_i z_i, a_i from 0.0, left to right; k_centroids one thread per cluster over
//   its run sums, left to right, then num / den (den == 0 keeps the centroid).
// Representatives: the smallest d2 of a cluster by a 64-bit integer atomicMin on its bits (d2 >= 0 orders as an integer),
//   then the lowest vertex that has it by a second atomicMin.  Integer atomics only.
// Dual: k_dual_keys one thread per face (the key of a candidate is its sorted label triple in 3 x 21 bits, the value
//   (face << 1 | orientation)), one stable 64-bit radix sort, k_dual_flags + an exclusive scan, k_dual_emit one thread per
//   run of equal keys.
// No floating-point atomics, no kernel waits for another block: two calls give the same bits in every output.
#include <hipcub/hipcub.hpp>

#include <vector>

#include "pf_internal.h"

namespace {

typedef unsigned long long u64;

constexpr int RM_RUN = 64;                         // members per run of the update's two-level sum
constexpr int RM_LABEL_BITS = 21;                  // a label in the dual's key
constexpr int64_t RM_MAX_CLUSTERS = ((int64_t)1 << RM_LABEL_BITS) - 1;
constexpr int RM_AXIS_CELLS = 1 << 20;             // cells along one axis at most
constexpr u64 RM_NO_KEY = ~0ull >> 1;              // a face that is no candidate: behind every key (a key has three distinct labels)
constexpr double RM_SLACK = 1.0 - 1.0 / 1048576.0; // on a ring's squared lower bound

struct GridSpec {
    double lo[3];
    double inv_h, h;   // h = 0 and inv_h = 0 when all centroids coincide
    int32_t G[3];
    int32_t cells;
};

struct SortedCentroid {
    double x, y, z;
    int64_t j;
};

__device__ __forceinline__ double dist2(double px, double py, double pz, double cx, double cy, double cz) {
    const double dx = px - cx, dy = py - cy, dz = pz - cz;
    return (dx * dx + dy * dy) + dz * dz;
}

// the cell of coordinate v along an axis of G cells: monotone in v, inside 0 .. G - 1 whatever v and the spec hold
__device__ __forceinline__ int32_t cell_of(double v, double lo, double inv_h, int32_t G) {
    const double t = (v - lo) * inv_h;
    if (!(t >= 0.0)) return 0;
    return t >= (double)G ? G - 1 : (int32_t)t;
}

__device__ __forceinline__ int32_t axis_cells(double ext, double inv_h, int32_t g) {
    if (!(ext > 0.0)) return 1;
    const double t = ceil(ext * inv_h);
    if (!(t < (double)g)) return g;
    return t < 1.0 ? 1 : (int32_t)t;
}

__device__ inline void spec_for(const double* ext, double max_ext, int32_t g, GridSpec& s, int64_t& cells) {
    s.inv_h = (double)g / max_ext;
    s.h = max_ext / (double)g;
    cells = 1;
    for (int x = 0; x < 3; ++x) {
        s.G[x] = axis_cells(ext[x], s.inv_h, g);
        cells *= s.G[x];
    }
}

// gk[k - 1]: cells along the longest axis when k axes have an extent (gk[k - 1]^k <= capacity); the edge is then halved
// while the grid has fewer than `target` cells and stays within `capacity` (thin axes leave room)
__global__ __launch_bounds__(PF_BLOCK) void k_grid_spec(const double* __restrict__ C, int64_t m, int32_t g1, int32_t g2, int32_t g3,
                                                        int64_t target, int64_t capacity, GridSpec* __restrict__ spec) {
    __shared__ double s_lo[3][PF_BLOCK], s_hi[3][PF_BLOCK];
    const double inf = __longlong_as_double(0x7ff0000000000000ll);
    double lo[3] = {inf, inf, inf}, hi[3] = {-inf, -inf, -inf};
    for (int64_t j = threadIdx.x; j < m; j += PF_BLOCK)
        for (int x = 0; x < 3; ++x) {
            const double v = C[3 * j + x];
            lo[x] = fmin(lo[x], v);
            hi[x] = fmax(hi[x], v);
        }
    for (int x = 0; x < 3; ++x) s_lo[x][threadIdx.x] = lo[x], s_hi[x][threadIdx.x] = hi[x];
    __syncthreads();
    for (int off = PF_BLOCK / 2; off > 0; off >>= 1) {
        if ((int)threadIdx.x < off)
            for (int x = 0; x < 3; ++x) {
                s_lo[x][threadIdx.x] = fmin(s_lo[x][threadIdx.x], s_lo[x][threadIdx.x + off]);
                s_hi[x][threadIdx.x] = fmax(s_hi[x][threadIdx.x], s_hi[x][threadIdx.x + off]);
            }
        __syncthreads();
    }
    if (threadIdx.x != 0) return;
    GridSpec s;
    double ext[3], max_ext = 0.0;
    int k = 0;
    for (int x = 0; x < 3; ++x) {
        s.lo[x] = s_lo[x][0];
        ext[x] = s_hi[x][0] - s_lo[x][0];
        if (ext[x] > 0.0) ++k;
        max_ext = fmax(max_ext, ext[x]);
    }
    int64_t cells = 1;
    if (k == 0) {
        s.inv_h = 0.0, s.h = 0.0, s.G[0] = s.G[1] = s.G[2] = 1;
    } else {
        int32_t g = k == 1 ? g1 : (k == 2 ? g2 : g3);
        spec_for(ext, max_ext, g, s, cells);
        while (cells < target && 2 * g <= RM_AXIS_CELLS) {
            GridSpec finer = s;
            int64_t finer_cells;
            spec_for(ext, max_ext, 2 * g, finer, finer_cells);
            if (finer_cells > capacity || finer_cells <= cells) break;
            s = finer, cells = finer_cells, g *= 2;
        }
    }
    s.cells = (int32_t)cells;
    *spec = s;
}

__global__ __launch_bounds__(PF_BLOCK) void k_cell_ids(const double* __restrict__ C, int64_t m, const GridSpec* __restrict__ spec,
                                                       unsigned* __restrict__ cell, int32_t* __restrict__ idx) {
    const int64_t j = (int64_t)blockIdx.x * PF_BLOCK + threadIdx.x;
    if (j >= m) return;
    const GridSpec s = *spec;
    const int32_t cx = cell_of(C[3 * j], s.lo[0], s.inv_h, s.G[0]), cy = cell_of(C[3 * j + 1], s.lo[1], s.inv_h, s.G[1]),
                  cz = cell_of(C[3 * j + 2], s.lo[2], s.inv_h, s.G[2]);
    cell[j] = (unsigned)((cz * s.G[1] + cy) * s.G[0] + cx);
    idx[j] = (int32_t)j;
}

// keys sorted ascending, each below n_keys: start[q] = the first position whose key is >= q, for q = 0 .. n_keys (CSR).
// The thread of position i fills (key[i - 1], key[i]], the last one also (key[i], n_keys].  n_keys < 0: read it from spec.
__device__ __forceinline__ void fill_starts(const unsigned* __restrict__ key, int64_t i, int64_t count, int64_t n_keys,
                                            int32_t* __restrict__ start) {
    const int64_t k = key[i], before = i == 0 ? -1 : (int64_t)key[i - 1];
    for (int64_t q = before + 1; q <= k; ++q) start[q] = (int32_t)i;
    if (i == count - 1)
        for (int64_t q = k + 1; q <= n_keys; ++q) start[q] = (int32_t)count;
}

__global__ __launch_bounds__(PF_BLOCK) void k_cell_starts(const unsigned* __restrict__ cell, const int32_t* __restrict__ idx, int64_t m,
                                                          const double* __restrict__ C, const GridSpec* __restrict__ spec,
                                                          int32_t* __restrict__ start, SortedCentroid* __restrict__ sorted) {
    const int64_t i = (int64_t)blockIdx.x * PF_BLOCK + threadIdx.x;
    if (i >= m) return;
    fill_starts(cell, i, m, spec->cells, start);
    const int64_t j = idx[i];
    SortedCentroid c;
    c.x = C[3 * j], c.y = C[3 * j + 1], c.z = C[3 * j + 2], c.j = j;
    sorted[i] = c;
}

// labels[i] in: any label in 0 .. m - 1 (the warm start), out: argmin_j d2(i, j), the lowest j on ties.
// *changed += labels that differ; *evals += distances evaluated.
__global__ __launch_bounds__(PF_BLOCK) void k_assign(const double* __restrict__ P, int64_t n, const double* __restrict__ C,
                                                     const GridSpec* __restrict__ spec, const int32_t* __restrict__ start,
                                                     const SortedCentroid* __restrict__ sorted, int32_t* __restrict__ labels,
                                                     int32_t* __restrict__ changed, u64* __restrict__ evals) {
    const int64_t i = (int64_t)blockIdx.x * PF_BLOCK + threadIdx.x;
    const bool valid = i < n;
    bool moved = false;
    u64 seen = 0;
    if (valid) {
        const GridSpec s = *spec;
        const double px = P[3 * i], py = P[3 * i + 1], pz = P[3 * i + 2];
        const int32_t before = labels[i];
        int32_t bj = before;
        double best = dist2(px, py, pz, C[3 * (int64_t)bj], C[3 * (int64_t)bj + 1], C[3 * (int64_t)bj + 2]);
        seen = 1;
        const int32_t cx = cell_of(px, s.lo[0], s.inv_h, s.G[0]), cy = cell_of(py, s.lo[1], s.inv_h, s.G[1]),
                      cz = cell_of(pz, s.lo[2], s.inv_h, s.G[2]);
        const int32_t r_max = max(max(max(cx, s.G[0] - 1 - cx), max(cy, s.G[1] - 1 - cy)), max(cz, s.G[2] - 1 - cz));
        for (int32_t r = 0; r <= r_max; ++r) {
            const double reach = (double)(r - 1) * s.h;
            if (r >= 2 && (reach * reach) * RM_SLACK > best) break;
            const int32_t z0 = max(cz - r, 0), z1 = min(cz + r, s.G[2] - 1), y0 = max(cy - r, 0), y1 = min(cy + r, s.G[1] - 1);
            const int32_t x0 = max(cx - r, 0), x1 = min(cx + r, s.G[0] - 1);
            for (int32_t z = z0; z <= z1; ++z)
                for (int32_t y = y0; y <= y1; ++y) {
                    const int64_t row = ((int64_t)z * s.G[1] + y) * s.G[0];
                    const bool whole = r == 0 || z == cz - r || z == cz + r || y == cy - r || y == cy + r;
                    // a row on a face of the ring: one contiguous range of cells; elsewhere the two cells at cx -+ r
                    for (int part = 0; part < (whole ? 1 : 2); ++part) {
                        int32_t a = x0, b = x1;
                        if (!whole) {
                            a = b = part == 0 ? cx - r : cx + r;
                            if (a < 0 || a >= s.G[0]) continue;
                        }
                        const int32_t s0 = start[row + a], s1 = start[row + b + 1];
                        seen += (u64)(s1 - s0);
                        for (int32_t q = s0; q < s1; ++q) {
                            const SortedCentroid c = sorted[q];
                            const double d = dist2(px, py, pz, c.x, c.y, c.z);
                            if (d < best || (d == best && (int32_t)c.j < bj)) best = d, bj = (int32_t)c.j;
                        }
                    }
                }
        }
        labels[i] = bj;
        moved = bj != before;
    }
    const int n_moved = __popcll(__ballot(moved));
#pragma unroll
    for (int off = PF_WAVE / 2; off > 0; off >>= 1) seen += __shfl_down(seen, off, PF_WAVE);
    if ((threadIdx.x & (PF_WAVE - 1)) == 0) {
        if (n_moved) atomicAdd(changed, n_moved);
        atomicAdd(evals, seen);
    }
}

__global__ __launch_bounds__(PF_BLOCK) void k_seed_centroids(const double* __restrict__ P, const int64_t* __restrict__ seeds, int64_t m,
                                                             double* __restrict__ C) {
    const int64_t j = (int64_t)blockIdx.x * PF_BLOCK + threadIdx.x;
    if (j >= m) return;
    const int64_t v = seeds[j];
    C[3 * j] = P[3 * v], C[3 * j + 1] = P[3 * v + 1], C[3 * j + 2] = P[3 * v + 2];
}

__global__ __launch_bounds__(PF_BLOCK) void k_iota(int32_t* __restrict__ v, int64_t n, int32_t fill, bool count_up) {
    const int64_t i = (int64_t)blockIdx.x * PF_BLOCK + threadIdx.x;
    if (i < n) v[i] = count_up ? (int32_t)i : fill;
}

__global__ __launch_bounds__(PF_BLOCK) void k_label_starts(const unsigned* __restrict__ key, int64_t n, int64_t m,
                                                           int32_t* __restrict__ start) {
    const int64_t i = (int64_t)blockIdx.x * PF_BLOCK + threadIdx.x;
    if (i < n) fill_starts(key, i, n, m, start);
}

// the thread of the first member of every run of 64: sums[4 i ..] = sum a x | a y | a z | a over the run, left to right
__global__ __launch_bounds__(PF_BLOCK) void k_run_sums(const unsigned* __restrict__ key, const int32_t* __restrict__ member, int64_t n,
                                                       const int32_t* __restrict__ start, const double* __restrict__ P,
                                                       const double* __restrict__ mass, double* __restrict__ sums) {
    const int64_t i = (int64_t)blockIdx.x * PF_BLOCK + threadIdx.x;
    if (i >= n) return;
    const int64_t j = key[i];
    if ((i - start[j]) % RM_RUN != 0) return;
    const int64_t end = min(i + RM_RUN, (int64_t)start[j + 1]);
    double sx = 0.0, sy = 0.0, sz = 0.0, sa = 0.0;
    for (int64_t q = i; q < end; ++q) {
        const int64_t v = member[q];
        const double a = mass[v];
        sx += a * P[3 * v], sy += a * P[3 * v + 1], sz += a * P[3 * v + 2], sa += a;
    }
    sums[4 * i] = sx, sums[4 * i + 1] = sy, sums[4 * i + 2] = sz, sums[4 * i + 3] = sa;
}

__global__ __launch_bounds__(PF_BLOCK) void k_centroids(const int32_t* __restrict__ start, int64_t m, const double* __restrict__ sums,
                                                        double* __restrict__ C) {
    const int64_t j = (int64_t)blockIdx.x * PF_BLOCK + threadIdx.x;
    if (j >= m) return;
    double sx = 0.0, sy = 0.0, sz = 0.0, sa = 0.0;
    for (int64_t q = start[j], end = start[j + 1]; q < end; q += RM_RUN)
        sx += sums[4 * q], sy += sums[4 * q + 1], sz += sums[4 * q + 2], sa += sums[4 * q + 3];
    if (sa == 0.0) return;  // no members, or none with a mass: the centroid stays
    C[3 * j] = sx / sa, C[3 * j + 1] = sy / sa, C[3 * j + 2] = sz / sa;
}

// ---- representatives: rep_d2[j] starts at all ones, rep[j] at INT32_MAX, count[j] at 0
__global__ __launch_bounds__(PF_BLOCK) void k_rep_min(const double* __restrict__ P, int64_t n, const double* __restrict__ C,
                                                      const int32_t* __restrict__ labels, u64* __restrict__ d2_bits,
                                                      u64* __restrict__ rep_d2, int32_t* __restrict__ count) {
    const int64_t i = (int64_t)blockIdx.x * PF_BLOCK + threadIdx.x;
    if (i >= n) return;
    const int64_t j = labels[i];
    const u64 bits = (u64)__double_as_longlong(dist2(P[3 * i], P[3 * i + 1], P[3 * i + 2], C[3 * j], C[3 * j + 1], C[3 * j + 2]));
    d2_bits[i] = bits;
    atomicMin(&rep_d2[j], bits);
    atomicAdd(&count[j], 1);
}

__global__ __launch_bounds__(PF_BLOCK) void k_rep_pick(const u64* __restrict__ d2_bits, int64_t n, const int32_t* __restrict__ labels,
                                                       const u64* __restrict__ rep_d2, int32_t* __restrict__ rep) {
    const int64_t i = (int64_t)blockIdx.x * PF_BLOCK + threadIdx.x;
    if (i >= n) return;
    const int64_t j = labels[i];
    if (d2_bits[i] == rep_d2[j]) atomicMin(&rep[j], (int32_t)i);
}

__global__ __launch_bounds__(PF_BLOCK) void k_rep_none(int32_t* __restrict__ rep, int64_t m) {
    const int64_t j = (int64_t)blockIdx.x * PF_BLOCK + threadIdx.x;
    if (j < m && rep[j] == 0x7fffffff) rep[j] = -1;
}

// ---- the dual
__global__ __launch_bounds__(PF_BLOCK) void k_dual_keys(const int32_t* __restrict__ faces, int64_t n_tri, const int32_t* __restrict__ labels,
                                                        u64* __restrict__ key, unsigned* __restrict__ val, int32_t* __restrict__ n_cand) {
    const int64_t t = (int64_t)blockIdx.x * PF_BLOCK + threadIdx.x;
    if (t >= n_tri) return;
    const int32_t a = labels[faces[3 * t]], b = labels[faces[3 * t + 1]], c = labels[faces[3 * t + 2]];
    val[t] = (unsigned)t << 1;
    if (a == b || b == c || a == c) {
        key[t] = RM_NO_KEY;
        return;
    }
    // rotated so that the smallest label leads: (l0, l1, l2)
    const int32_t l0 = min(a, min(b, c));
    const int32_t l1 = l0 == a ? b : (l0 == b ? c : a), l2 = l0 == a ? c : (l0 == b ? a : b);
    key[t] = ((u64)l0 << (2 * RM_LABEL_BITS)) | ((u64)min(l1, l2) << RM_LABEL_BITS) | (u64)max(l1, l2);
    val[t] |= l1 > l2 ? 1u : 0u;
    atomicAdd(n_cand, 1);
}

__global__ __launch_bounds__(PF_BLOCK) void k_dual_flags(const u64* __restrict__ key, int64_t n_tri, int32_t* __restrict__ flag) {
    const int64_t i = (int64_t)blockIdx.x * PF_BLOCK + threadIdx.x;
    if (i < n_tri) flag[i] = key[i] != RM_NO_KEY && (i == 0 || key[i - 1] != key[i]) ? 1 : 0;
}

// one thread per run of equal keys; the run is in ascending face index
__global__ __launch_bounds__(PF_BLOCK) void k_dual_emit(const u64* __restrict__ key, const unsigned* __restrict__ val, int64_t n_tri,
                                                        const int32_t* __restrict__ flag, const int32_t* __restrict__ pos,
                                                        int32_t* __restrict__ out_faces, int32_t* __restrict__ face_src,
                                                        int32_t* __restrict__ votes, int32_t* __restrict__ n_out) {
    const int64_t i = (int64_t)blockIdx.x * PF_BLOCK + threadIdx.x;
    if (i >= n_tri) return;
    if (i == n_tri - 1) *n_out = pos[i] + flag[i];
    if (!flag[i]) return;
    const u64 k = key[i];
    int32_t n0 = 0, n1 = 0;
    for (int64_t q = i; q < n_tri && key[q] == k; ++q) (val[q] & 1u) ? ++n1 : ++n0;
    const bool swapped = n1 > n0 || (n1 == n0 && (val[i] & 1u));
    const int32_t mask = (1 << RM_LABEL_BITS) - 1;
    const int32_t l0 = (int32_t)(k >> (2 * RM_LABEL_BITS)), mid = (int32_t)(k >> RM_LABEL_BITS) & mask, hi = (int32_t)k & mask;
    const int64_t o = pos[i];
    out_faces[3 * o] = l0, out_faces[3 * o + 1] = swapped ? hi : mid, out_faces[3 * o + 2] = swapped ? mid : hi;
    face_src[o] = (int32_t)(val[i] >> 1);
    votes[2 * o] = swapped ? n1 : n0, votes[2 * o + 1] = swapped ? n0 : n1;
}

int32_t root_up(int64_t value, int k, int32_t cap) {  // the least g >= 1 with g^k >= value, at most cap
    int32_t g = 1;
    for (;;) {
        int64_t p = 1;
        for (int x = 0; x < k; ++x) p *= g;
        if (p >= value || g >= cap) return g;
        ++g;
    }
}

}  // namespace

extern "C" int pf_mesh_cluster(pf_ctx* ctx, const double* pts, int64_t n, const int32_t* faces, int64_t n_faces, const double* mass,
                               const int64_t* seeds, int64_t m, int32_t n_iter, uint32_t flags, const double* centroids_in,
                               const int32_t* labels_in, int32_t* labels, double* centroids, int32_t* rep, int32_t* count,
                               int32_t* changed, int32_t* out_faces, int32_t* face_src, int32_t* votes, int64_t* report,
                               double* device_ms) {
    PF_CHECK(ctx && pts && mass, PF_E_ARG, "pf_mesh_cluster: NULL argument");
    PF_CHECK(n > 0 && n < ((int64_t)1 << 31), PF_E_ARG, "pf_mesh_cluster: n = %lld out of range", (long long)n);
    PF_CHECK(n_faces >= 0 && 3 * n_faces < ((int64_t)1 << 31) && (faces || n_faces == 0), PF_E_ARG,
             "pf_mesh_cluster: %lld faces out of range (3 n_faces < 2^31)", (long long)n_faces);
    PF_CHECK(m <= RM_MAX_CLUSTERS, PF_E_ARG, "pf_mesh_cluster: m = %lld does not fit the 21 bits of a label in a face key",
             (long long)m);
    PF_CHECK(m >= 1 && m <= n, PF_E_ARG, "pf_mesh_cluster: m = %lld outside 1 .. n = %lld", (long long)m, (long long)n);
    PF_CHECK(n_iter >= 0, PF_E_ARG, "pf_mesh_cluster: n_iter = %d is negative", n_iter);
    PF_CHECK((flags & ~(uint32_t)PF_CLUSTER_UPDATE_ONLY) == 0, PF_E_ARG, "pf_mesh_cluster: unknown flags 0x%x", (unsigned)flags);
    PF_CHECK((seeds != nullptr) != (centroids_in != nullptr), PF_E_ARG, "pf_mesh_cluster: give either seeds or centroids_in");
    const bool update_only = (flags & PF_CLUSTER_UPDATE_ONLY) != 0;
    PF_CHECK(!update_only || (labels_in && n_iter == 1), PF_E_ARG, "pf_mesh_cluster: an update step needs labels_in and n_iter = 1");
    const int64_t T = n_faces;
    for (int64_t i = 0; i < n; ++i) {
        for (int x = 0; x < 3; ++x)
            PF_CHECK(std::isfinite(pts[3 * i + x]), PF_E_ARG, "pf_mesh_cluster: a coordinate of vertex %lld is not finite", (long long)i);
        PF_CHECK(std::isfinite(mass[i]) && mass[i] >= 0.0, PF_E_ARG, "pf_mesh_cluster: the mass of vertex %lld is negative or not finite",
                 (long long)i);
        PF_CHECK(!labels_in || (labels_in[i] >= 0 && labels_in[i] < m), PF_E_ARG, "pf_mesh_cluster: labels_in[%lld] = %d outside 0 .. m - 1",
                 (long long)i, labels_in ? labels_in[i] : 0);
    }
    for (int64_t j = 0; j < m; ++j) {
        PF_CHECK(!seeds || (seeds[j] >= 0 && seeds[j] < n), PF_E_ARG, "pf_mesh_cluster: seed %lld = %lld outside 0 .. n - 1", (long long)j,
                 seeds ? (long long)seeds[j] : 0ll);
        for (int x = 0; centroids_in && x < 3; ++x)
            PF_CHECK(std::isfinite(centroids_in[3 * j + x]), PF_E_ARG, "pf_mesh_cluster: a coordinate of centroid %lld is not finite",
                     (long long)j);
    }
    PF_TRY(pf_check_faces("pf_mesh_cluster", faces, T, 3, n, true));
    // the grid: about 2 m cells; gk^k and every refinement the device accepts stay within the capacity
    const int64_t target = 2 * m, capacity = 8 * m + 64;
    const int32_t g1 = root_up(target, 1, RM_AXIS_CELLS), g2 = root_up(target, 2, 1024), g3 = root_up(target, 3, 128);
    const int cell_bits = pf_index_bits(capacity), label_bits = pf_index_bits(m);
    PF_HIP(hipSetDevice(ctx->device));
    hipStream_t st = ctx->stream;
    StreamTimer timer(device_ms != nullptr);
    std::vector<int32_t> h_changed((size_t)n_iter + 1, 0);
    int32_t iters = 0, passes = 0, h_counts[2] = {0, 0};  // output faces | candidates
    u64 h_evals = 0;
    GridSpec h_spec = {};
    hipError_t err;
    {
        Scratch sc(st);
        double *d_P = sc.get<double>(3 * n), *d_mass = sc.get<double>(n), *d_C = sc.get<double>(3 * m);
        int32_t* d_faces = sc.get<int32_t>(3 * T);
        int64_t* d_seeds = seeds ? sc.get<int64_t>(m) : nullptr;
        int32_t* d_lab = sc.get<int32_t>(n);
        // the grid of an assignment
        GridSpec* d_spec = sc.get<GridSpec>(1);
        unsigned *cell0 = sc.get<unsigned>(m), *cell1 = sc.get<unsigned>(m);
        int32_t *cidx0 = sc.get<int32_t>(m), *cidx1 = sc.get<int32_t>(m), *cstart = sc.get<int32_t>(capacity + 1);
        SortedCentroid* sorted = sc.get<SortedCentroid>(m);
        // the update's order
        int32_t *iota = sc.get<int32_t>(n), *member = sc.get<int32_t>(n), *lstart = sc.get<int32_t>(m + 1);
        unsigned* lkey = sc.get<unsigned>(n);
        double* sums = sc.get<double>(4 * n);
        // zeroed together: changed per iteration and one for the start | evaluations (u64, 8-byte aligned) | counts
        u64* words = sc.get<u64>((size_t)(n_iter + 2) / 2 + 1 + 1);
        int32_t* d_changed = (int32_t*)words;
        u64* d_evals = words + (n_iter + 2) / 2;
        int32_t* d_counts = (int32_t*)(d_evals + 1);  // output faces | candidates
        u64 *d2_bits = sc.get<u64>(n), *rep_d2 = sc.get<u64>(m);
        int32_t *d_rep = sc.get<int32_t>(m), *d_count = sc.get<int32_t>(m);
        sc.upload(d_P, pts, 3 * n);
        sc.upload(d_mass, mass, n);
        if (T) sc.upload(d_faces, faces, 3 * T);
        if (seeds) sc.upload(d_seeds, seeds, m);
        if (centroids_in) sc.upload(d_C, centroids_in, 3 * m);
        if (labels_in) sc.upload(d_lab, labels_in, n);
        sc.zero(words, sizeof(u64) * ((size_t)(n_iter + 2) / 2 + 2));
        sc.zero(d_count, sizeof(int32_t) * m);
        if (sc.ok()) sc.note(hipMemsetAsync(rep_d2, 0xff, sizeof(u64) * m, st));
        timer.start(sc);
        if (sc.ok()) {
            if (seeds) k_seed_centroids<<<pf_blocks(m), PF_BLOCK, 0, st>>>(d_P, d_seeds, m, d_C);
            if (!labels_in) k_iota<<<pf_blocks(n), PF_BLOCK, 0, st>>>(d_lab, n, 0, false);
            k_iota<<<pf_blocks(n), PF_BLOCK, 0, st>>>(iota, n, 0, true);
            k_iota<<<pf_blocks(m), PF_BLOCK, 0, st>>>(d_rep, m, 0x7fffffff, false);
            sc.launched();
        }
        // slot n_iter of d_changed takes the start's count, which is no output
        auto assign = [&](int32_t slot) {
            if (!sc.ok()) return;
            k_grid_spec<<<1, PF_BLOCK, 0, st>>>(d_C, m, g1, g2, g3, target, capacity, d_spec);
            k_cell_ids<<<pf_blocks(m), PF_BLOCK, 0, st>>>(d_C, m, d_spec, cell0, cidx0);
            sc.launched();
            pf_sort_pairs(sc, cell0, cell1, cidx0, cidx1, m, cell_bits);
            if (!sc.ok()) return;
            k_cell_starts<<<pf_blocks(m), PF_BLOCK, 0, st>>>(cell1, cidx1, m, d_C, d_spec, cstart, sorted);
            k_assign<<<pf_blocks(n), PF_BLOCK, 0, st>>>(d_P, n, d_C, d_spec, cstart, sorted, d_lab, d_changed + slot, d_evals);
            sc.launched();
            ++passes;
        };
        auto update = [&]() {
            pf_sort_pairs(sc, (const unsigned*)d_lab, lkey, iota, member, n, label_bits);
            if (!sc.ok()) return;
            k_label_starts<<<pf_blocks(n), PF_BLOCK, 0, st>>>(lkey, n, m, lstart);
            k_run_sums<<<pf_blocks(n), PF_BLOCK, 0, st>>>(lkey, member, n, lstart, d_P, d_mass, sums);
            k_centroids<<<pf_blocks(m), PF_BLOCK, 0, st>>>(lstart, m, sums, d_C);
            sc.launched();
        };
        if (update_only) {
            update();
            iters = 1;
        } else {
            assign(n_iter);
            for (int32_t t = 0; sc.ok() && t < n_iter; ++t) {
                const size_t mark = sc.blocks.size();  // the two sorts' temporaries go back with every iteration
                update();
                assign(t);
                sc.download(&h_changed[t], d_changed + t, 1);  // the one word the host reads per iteration
                sc.sync();
                sc.release_from(mark);
                if (!sc.ok()) break;
                ++iters;
                if (h_changed[t] == 0) break;
            }
        }
        if (sc.ok()) {
            k_rep_min<<<pf_blocks(n), PF_BLOCK, 0, st>>>(d_P, n, d_C, d_lab, d2_bits, rep_d2, d_count);
            k_rep_pick<<<pf_blocks(n), PF_BLOCK, 0, st>>>(d2_bits, n, d_lab, rep_d2, d_rep);
            k_rep_none<<<pf_blocks(m), PF_BLOCK, 0, st>>>(d_rep, m);
            sc.launched();
        }
        int32_t *d_out = nullptr, *d_src = nullptr, *d_votes = nullptr;
        if (T) {
            u64 *dk0 = sc.get<u64>(T), *dk1 = sc.get<u64>(T);
            unsigned *dv0 = sc.get<unsigned>(T), *dv1 = sc.get<unsigned>(T);
            int32_t *flag = sc.get<int32_t>(T), *pos = sc.get<int32_t>(T);
            d_out = sc.get<int32_t>(3 * T), d_src = sc.get<int32_t>(T), d_votes = sc.get<int32_t>(2 * T);
            size_t need_s = 0;
            if (sc.ok()) sc.note(hipcub::DeviceScan::ExclusiveSum(nullptr, need_s, flag, pos, (int)T, st));
            void* tmp_s = sc.get<char>(need_s);
            if (sc.ok()) {
                k_dual_keys<<<pf_blocks(T), PF_BLOCK, 0, st>>>(d_faces, T, d_lab, dk0, dv0, d_counts + 1);
                sc.launched();
            }
            pf_sort_pairs(sc, dk0, dk1, dv0, dv1, T, 3 * RM_LABEL_BITS);
            if (sc.ok()) {
                k_dual_flags<<<pf_blocks(T), PF_BLOCK, 0, st>>>(dk1, T, flag);
                sc.launched();
            }
            if (sc.ok()) sc.note(hipcub::DeviceScan::ExclusiveSum(tmp_s, need_s, flag, pos, (int)T, st));
            if (sc.ok()) {
                k_dual_emit<<<pf_blocks(T), PF_BLOCK, 0, st>>>(dk1, dv1, T, flag, pos, d_out, d_src, d_votes, d_counts);
                sc.launched();
            }
        }
        sc.download(labels, d_lab, n);
        sc.download(centroids, d_C, 3 * m);
        sc.download(rep, d_rep, m);
        sc.download(count, d_count, m);
        sc.download(h_counts, d_counts, 2);
        sc.download(&h_evals, d_evals, 1);
        sc.download(&h_spec, d_spec, 1);
        sc.sync();  // the number of output faces is known from here
        if (T && h_counts[0] > 0) {
            sc.download(out_faces, d_out, 3 * (size_t)h_counts[0]);
            sc.download(face_src, d_src, (size_t)h_counts[0]);
            sc.download(votes, d_votes, 2 * (size_t)h_counts[0]);
        }
        timer.stop(sc);
        sc.sync();
        timer.read(sc, device_ms);
        err = sc.err;
    }
    if (err != hipSuccess) return pf_hip_failed("pf_mesh_cluster", err);
    if (changed && !update_only)
        for (int32_t t = 0; t < iters; ++t) changed[t] = h_changed[t];
    if (report) {
        report[0] = iters;
        report[1] = h_counts[0];
        report[2] = h_counts[1];
        report[3] = passes ? h_spec.cells : 0;
        report[4] = (int64_t)h_evals;
        report[5] = passes;
        report[6] = report[7] = 0;
    }
    return PF_OK;
}
