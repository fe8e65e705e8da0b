// Exact 1-nearest-neighbour search for DEEP coordinates (d >= 7 by default): a bounding-box hierarchy over ALL d coordinates.
//
// Replaces `scipy.spatial.KDTree(target).query(source)` of /root/reference/pyfocusr/focusr.py:351-353 where the
// spectral embedding is deep (BASELINE config C5: 1M x 1M vertices, d = 10).  pf_knn.hip prunes with a grid over the
// reference set's two widest axes: every reference within sqrt(best) of a query ON THOSE TWO AXES is a candidate.  For a
// 2-manifold embedded in 10 dimensions whose two clouds are poorly aligned (nearest distances ~0.15 of the cube) that
// rectangle holds 50-100k references per query, of which the other eight coordinates would have excluded all but a few
// thousand - what scipy's k-d tree exploits (~2000 visited per query), and why the grid scan took 127 ms at C5.
//
// Structure (built per call, ~0.5 ms at 1M x 10):
//   * references sorted along a Morton curve over their (up to) five widest axes: points of one patch of the embedded
//     surface become neighbours in the order;
//   * LEAVES of 64 consecutive points, coordinate-major inside a leaf (a wave reads one coordinate of a leaf as 512
//     contiguous bytes), each with its axis-aligned bounding box in all d coordinates;
//   * SUPERS of 64 consecutive leaves with the box of their boxes; the supers' boxes are the top level (244 at 1M).
// Search: a wave owns G Morton-consecutive queries (their coordinates in scalar registers).  Lane l tests box l of the
// level at hand; the nearest super's nearest leaf gives the first bound; then every super / leaf whose box is within a
// query's current bound is visited, a leaf's 64 points one per lane against all G queries, and after every few leaves the
// lanes' (distance, original index) pairs are reduced lexicographically across the wave.
//
// Exactness.  The squared distance is pf_knn.hip's: sum over the coordinates, left to right, of (q_c - r_c)^2, separate
// multiply and add (-ffp-contract=off); smallest wins, lowest reference index on exact ties.  A box's distance is the SAME
// accumulation over gap_c = max(lo_c - q_c, q_c - hi_c, 0).  For every point r of the box |q_c - r_c| >= gap_c in real
// numbers, and every operation of the accumulation (the subtraction, the square, each addition) is monotone under
// rounding, so the computed box distance is <= the computed distance of every point in it: a box is skipped only when its
// distance is > a query's bound - no candidate that could win or tie is ever dropped, and the minimum of (distance, index)
// does not depend on the order of the visits.  Indices and distances are bit-identical to a brute force.
//
// k nearest neighbours (pf_knn_topk, 1 <= k <= 64).  The same hierarchy (tree_build, shared by both searches), the same
// groups, the same box_d2; the single best of a query becomes a LIST of its 64 smallest (distance, index) pairs, kept
// across the lanes of the wave: lane j holds the j-th smallest, (+inf, 0x7fffffff) while there is none.  The k-th entry is
// the query's bound.  After a leaf's 64 distances are known the lanes whose (distance, index) is lexicographically below
// the bound are collected with a ballot - empty for most leaves - and go in one at a time: the candidate is broadcast,
// every lane compares it with its own entry, and the lanes at or behind its place take their left neighbour's entry.  No
// LDS, no register array indexed at run time.
// Exactness of the list.  A box is opened only if box_d2 <= the query's k-th best distance, which is +inf until k real
// candidates are held: by the argument above every point that is skipped has a distance > the bound, so it is behind k
// points already held.  The test is <=, not <: a point AT the bound's distance with a lower index still has to get in.
// (distance, index) is a total order (an index occurs once: the first leaf is scanned once and skipped when its turn
// comes again, and the copies that pad the last leaf - index 0x7fffffff - take the distance +inf and never enter), so the k
// smallest do not depend on the order of the visits.  16 < d <= 128: the same list over an exhaustive scan, 64
// references at a time from a coordinate-major copy, the depth a run-time value (k_knn_topk_wide).
#include <hipcub/hipcub.hpp>

#include <algorithm>

#include "pf_internal.h"
#include "pf_wave.h"

namespace {

constexpr int TREE_AXES = 5;

struct TreeGrid {
    int na;                 // axes in the key
    int bits;               // bits per axis
    int axis[TREE_AXES];
    double lo[TREE_AXES];
    double scale[TREE_AXES];  // cells per unit length (0 when the extent is 0)
};

// the (up to) five widest axes of the reference set, widest first; 30 key bits shared between them
__global__ void k_tree_grid(const unsigned long long* __restrict__ ext /* [2][16]: encoded min, max */, int d, TreeGrid* g) {
    if (threadIdx.x | blockIdx.x) return;
    double w[16];
    bool used[16];
    for (int a = 0; a < d; ++a) {
        w[a] = dec_f64(ext[16 + a]) - dec_f64(ext[a]);
        used[a] = false;
    }
    const int na = d < TREE_AXES ? d : TREE_AXES;
    g->na = na;
    g->bits = 30 / na;
    for (int k = 0; k < na; ++k) {
        int b = -1;
        for (int a = 0; a < d; ++a)
            if (!used[a] && (b < 0 || w[a] > w[b])) b = a;
        used[b] = true;
        g->axis[k] = b;
        g->lo[k] = dec_f64(ext[b]);
        g->scale[k] = (w[b] > 0.0 && isfinite(w[b])) ? (double)(1 << g->bits) / w[b] : 0.0;
    }
}

// Morton key of a point over the grid's axes (bit j of axis k lands at position j * na + k); points outside the
// reference set's box (queries) are clamped
__global__ __launch_bounds__(PF_BLOCK) void k_tree_keys(const double* __restrict__ pts, int64_t n, int d, const TreeGrid* __restrict__ gp,
                                                        unsigned* __restrict__ keys, int32_t* __restrict__ vals) {
    const int64_t i = (int64_t)blockIdx.x * PF_BLOCK + threadIdx.x;
    if (i >= n) return;
    // (the grid is read where it lies: a local copy indexed by the run-time axis number k would live in SCRATCH memory -
    // 0.78 ms per million points instead of ~0.03)
    const int na = gp->na, bits = gp->bits;
    unsigned key = 0;
    const int cells = 1 << bits;
    for (int k = 0; k < na; ++k) {
        const double t = (pts[i * d + gp->axis[k]] - gp->lo[k]) * gp->scale[k];
        const unsigned c = t > 0.0 ? (t >= (double)cells ? (unsigned)(cells - 1) : (unsigned)t) : 0u;
        for (int j = 0; j < bits; ++j) key |= ((c >> j) & 1u) << (j * na + k);
    }
    keys[i] = key;
    vals[i] = (int32_t)i;
}

// leaf storage: point p of the sorted order -> leaf p / 64, place p % 64, coordinate-major inside the leaf; the last
// leaf is filled up with copies of the last point under the index INT_MAX (they lose every tie)
__global__ __launch_bounds__(PF_BLOCK) void k_tree_leaves(const double* __restrict__ ref, const int32_t* __restrict__ order, int64_t n,
                                                          int d, int64_t n_slots, double* __restrict__ pts, int32_t* __restrict__ orig) {
    const int64_t p = (int64_t)blockIdx.x * PF_BLOCK + threadIdx.x;
    if (p >= n_slots) return;
    const int64_t src = order[p < n ? p : n - 1];
    orig[p] = p < n ? (int32_t)src : 0x7fffffff;
    double* out = pts + (p >> 6) * (int64_t)d * PF_WAVE + (p & (PF_WAVE - 1));
    for (int c = 0; c < d; ++c) out[(int64_t)c * PF_WAVE] = ref[src * d + c];
}

// boxes of the leaves, stored per super: leaf_lo[(S * d + c) * 64 + leaf % 64]; leaves past the end get an empty box
// (lo = +inf, hi = -inf: infinitely far from everything)
__global__ __launch_bounds__(PF_BLOCK) void k_tree_leaf_boxes(const double* __restrict__ pts, int32_t n_leaf, int32_t n_sup, int d,
                                                              double* __restrict__ leaf_lo, double* __restrict__ leaf_hi) {
    const int64_t e = (int64_t)blockIdx.x * PF_BLOCK + threadIdx.x;
    if (e >= (int64_t)n_sup * PF_WAVE * d) return;
    const int32_t L = (int32_t)(e / d);
    const int c = (int)(e - (int64_t)L * d);
    double lo = INFINITY, hi = -INFINITY;
    if (L < n_leaf) {
        const double* p = pts + ((int64_t)L * d + c) * PF_WAVE;
        for (int j = 0; j < PF_WAVE; ++j) {
            const double v = p[j];
            lo = v < lo ? v : lo;
            hi = v > hi ? v : hi;
        }
    }
    const int64_t o = ((int64_t)(L >> 6) * d + c) * PF_WAVE + (L & (PF_WAVE - 1));
    leaf_lo[o] = lo;
    leaf_hi[o] = hi;
}

// boxes of the supers: sup_lo[c * ns_pad + S]
__global__ __launch_bounds__(PF_BLOCK) void k_tree_super_boxes(const double* __restrict__ leaf_lo, const double* __restrict__ leaf_hi,
                                                               int32_t n_sup, int32_t ns_pad, int d, double* __restrict__ sup_lo,
                                                               double* __restrict__ sup_hi) {
    const int64_t e = (int64_t)blockIdx.x * PF_BLOCK + threadIdx.x;
    if (e >= (int64_t)ns_pad * d) return;
    const int32_t S = (int32_t)(e / d);
    const int c = (int)(e - (int64_t)S * d);
    double lo = INFINITY, hi = -INFINITY;
    if (S < n_sup) {
        const double* pl = leaf_lo + ((int64_t)S * d + c) * PF_WAVE;
        const double* ph = leaf_hi + ((int64_t)S * d + c) * PF_WAVE;
        for (int j = 0; j < PF_WAVE; ++j) {
            lo = pl[j] < lo ? pl[j] : lo;
            hi = ph[j] > hi ? ph[j] : hi;
        }
    }
    sup_lo[(int64_t)c * ns_pad + S] = lo;
    sup_hi[(int64_t)c * ns_pad + S] = hi;
}

struct TreeArgs {
    const double* pts;
    const int32_t* orig;
    const double* leaf_lo;
    const double* leaf_hi;
    const double* sup_lo;
    const double* sup_hi;
    const double* qry;
    const int32_t* qry_order;
    int64_t n_qry;
    int32_t n_leaf, n_sup, ns_pad;
    int64_t* idx_out;
    double* d2_out;
    unsigned long long* counters;  // nullable: [0] leaves scanned, [1] supers opened (diagnostics)
};

// squared distance of q to the box [lo, hi] (one coordinate every `cs` doubles): the accumulation of the point distance
template <int D>
__device__ __forceinline__ double box_d2(const double (&q)[D], const double* __restrict__ lo, const double* __restrict__ hi, int64_t cs) {
    double s = 0.0;
#pragma unroll
    for (int c = 0; c < D; ++c) {
        const double t1 = lo[(int64_t)c * cs] - q[c], t2 = q[c] - hi[(int64_t)c * cs];
        const double g = fmax(fmax(t1, t2), 0.0);
        const double sq = g * g;
        s = (c == 0) ? sq : s + sq;
    }
    return s;
}

constexpr int tree_group(int d) { return d <= 12 ? 4 : 2; }
constexpr int TREE_BATCH = 2;  // leaves scanned between two reductions of the lanes' bests

template <int D>
__global__ __launch_bounds__(PF_BLOCK) void k_knn_tree(TreeArgs t) {
    constexpr int G = tree_group(D);
    const int lane = threadIdx.x & (PF_WAVE - 1);
    const int64_t group = (int64_t)blockIdx.x * (PF_BLOCK / PF_WAVE) + __builtin_amdgcn_readfirstlane((int)(threadIdx.x / PF_WAVE));
    const int64_t q0 = group * G;
    if (q0 >= t.n_qry) return;  // (wave-uniform)
    const int nq = t.n_qry - q0 < G ? (int)(t.n_qry - q0) : G;
    double q[G][D];  // wave-uniform (a short group replays its last query)
    int32_t qdst[G];
    double best[G];
    int32_t bidx[G];
#pragma unroll
    for (int i = 0; i < G; ++i) {
        qdst[i] = t.qry_order[q0 + (i < nq ? i : nq - 1)];
#pragma unroll
        for (int c = 0; c < D; ++c) q[i][c] = t.qry[(int64_t)qdst[i] * D + c];
        best[i] = INFINITY;
        bidx[i] = 0x7fffffff;
    }
    unsigned long long n_scanned = 0, n_opened = 0;

    auto scan_leaf = [&](int32_t L) {
        const double* p = t.pts + (int64_t)L * D * PF_WAVE + lane;
        double x[D];
#pragma unroll
        for (int c = 0; c < D; ++c) x[c] = p[c * PF_WAVE];
        const int32_t o = t.orig[(int64_t)L * PF_WAVE + lane];
        ++n_scanned;
#pragma unroll
        for (int i = 0; i < G; ++i) {
            double s = 0.0;
            constexpr int P = D >= 6 ? D / 2 : D;  // most candidates are out after half of the coordinates
#pragma unroll
            for (int c = 0; c < P; ++c) {
                const double df = q[i][c] - x[c];
                const double sq = df * df;
                s = (c == 0) ? sq : s + sq;
            }
            if constexpr (P < D) {
                if (!__any(s <= best[i])) continue;  // (the partial sum is a prefix of the same accumulation and only grows)
#pragma unroll
                for (int c = P; c < D; ++c) {
                    const double df = q[i][c] - x[c];
                    s = s + df * df;
                }
            }
            if (s < best[i] || (s == best[i] && o < bidx[i])) {
                best[i] = s;
                bidx[i] = o;
            }
        }
    };
    auto reduce = [&]() {
#pragma unroll
        for (int i = 0; i < G; ++i) wave_argmin(best[i], bidx[i]);
    };

    // ---- the first bound: the leaf nearest to the group's first query inside the super nearest to it
    int32_t L0;
    {
        double sb = INFINITY;
        int32_t sa = 0;
        for (int32_t s0 = 0; s0 < t.ns_pad; s0 += PF_WAVE) {
            const double dd = box_d2<D>(q[0], t.sup_lo + s0 + lane, t.sup_hi + s0 + lane, t.ns_pad);
            if (dd < sb) sb = dd, sa = s0 + lane;
        }
        wave_argmin(sb, sa);
        const int64_t lb = (int64_t)sa * D * PF_WAVE + lane;
        double lbest = box_d2<D>(q[0], t.leaf_lo + lb, t.leaf_hi + lb, PF_WAVE);
        int32_t la = lane;
        wave_argmin(lbest, la);
        L0 = sa * PF_WAVE + la;
        scan_leaf(L0);
        reduce();
    }
    // ---- every super whose box is within a query's bound, every leaf of it whose box is
    for (int32_t s0 = 0; s0 < t.ns_pad; s0 += PF_WAVE) {
        double sd[G];
#pragma unroll
        for (int i = 0; i < G; ++i) sd[i] = box_d2<D>(q[i], t.sup_lo + s0 + lane, t.sup_hi + s0 + lane, t.ns_pad);
        unsigned long long sdone = 0ull;
        while (true) {
            bool need = false;
#pragma unroll
            for (int i = 0; i < G; ++i) need = need || sd[i] <= best[i];
            const unsigned long long sm = __ballot(need) & ~sdone;
            if (!sm) break;
            const int sbit = __ffsll((long long)sm) - 1;
            sdone |= 1ull << sbit;
            const int32_t S = s0 + sbit;
            if (S >= t.n_sup) continue;
            ++n_opened;
            const int64_t lb = (int64_t)S * D * PF_WAVE + lane;
            double ld[G];
#pragma unroll
            for (int i = 0; i < G; ++i) ld[i] = box_d2<D>(q[i], t.leaf_lo + lb, t.leaf_hi + lb, PF_WAVE);
            unsigned long long ldone = 0ull;
            while (true) {
                bool ln = false;
#pragma unroll
                for (int i = 0; i < G; ++i) ln = ln || ld[i] <= best[i];
                unsigned long long lm = __ballot(ln) & ~ldone;
                if (!lm) break;
                for (int b = 0; b < TREE_BATCH && lm; ++b) {
                    const int lbit = __ffsll((long long)lm) - 1;
                    lm &= lm - 1ull;
                    ldone |= 1ull << lbit;
                    const int32_t L = S * PF_WAVE + lbit;
                    if (L < t.n_leaf && L != L0) scan_leaf(L);
                }
                reduce();
            }
        }
    }
#pragma unroll
    for (int i = 0; i < G; ++i) {
        if (lane == i && i < nq) {
            t.idx_out[qdst[i]] = bidx[i];
            t.d2_out[qdst[i]] = best[i];
        }
    }
    if (t.counters && lane == 0) {
        atomicAdd(t.counters, n_scanned);
        atomicAdd(t.counters + 1, n_opened);
    }
}

// ---- the list of a query's 64 smallest (distance, index) pairs, one per lane, ascending (see the file header)

// one candidate (wave-uniform) into the list: the lanes whose entry it precedes move one place to the right
__device__ __forceinline__ void list_insert(double& nd, int32_t& ni, double cs, int32_t co, int lane) {
    const bool before = cs < nd || (cs == nd && co < ni);
    const double pd = __shfl_up(nd, 1, PF_WAVE);
    const int32_t pi = __shfl_up(ni, 1, PF_WAVE);
    const bool before_left = lane > 0 && (cs < pd || (cs == pd && co < pi));
    if (before) {
        nd = before_left ? pd : cs;
        ni = before_left ? pi : co;
    }
}

// the lanes' candidates (s, o) into the list; (kd, ki) is the list's k-th entry, wave-uniform: the bound.  A lane that
// has no candidate offers s = +inf with o = 0x7fffffff, which is below no bound.
__device__ __forceinline__ void list_offer(double& nd, int32_t& ni, double& kd, int32_t& ki, double s, int32_t o, int k, int lane) {
    unsigned long long m = __ballot(s < kd || (s == kd && o < ki));
    while (m) {
        const int b = __ffsll((long long)m) - 1;
        m &= m - 1ull;
        const double cs = __shfl(s, b, PF_WAVE);
        const int32_t co = __shfl(o, b, PF_WAVE);
        if (!(cs < kd || (cs == kd && co < ki))) continue;  // (the bound has moved since the ballot)
        list_insert(nd, ni, cs, co, lane);
        kd = __shfl(nd, k - 1, PF_WAVE);
        ki = __shfl(ni, k - 1, PF_WAVE);
    }
}

// k_knn_tree with a list per query: t.idx_out / t.d2_out are [n_qry][k]
template <int D>
__global__ __launch_bounds__(PF_BLOCK) void k_knn_tree_topk(TreeArgs t, int k) {
    constexpr int G = tree_group(D);
    const int lane = threadIdx.x & (PF_WAVE - 1);
    const int64_t group = (int64_t)blockIdx.x * (PF_BLOCK / PF_WAVE) + __builtin_amdgcn_readfirstlane((int)(threadIdx.x / PF_WAVE));
    const int64_t q0 = group * G;
    if (q0 >= t.n_qry) return;  // (wave-uniform)
    const int nq = t.n_qry - q0 < G ? (int)(t.n_qry - q0) : G;
    double q[G][D];  // wave-uniform (a short group replays its last query)
    int32_t qdst[G];
    double nd[G], kd[G];  // this lane's entry of each list; each list's k-th entry
    int32_t ni[G], ki[G];
#pragma unroll
    for (int i = 0; i < G; ++i) {
        qdst[i] = t.qry_order[q0 + (i < nq ? i : nq - 1)];
#pragma unroll
        for (int c = 0; c < D; ++c) q[i][c] = t.qry[(int64_t)qdst[i] * D + c];
        nd[i] = kd[i] = INFINITY;
        ni[i] = ki[i] = 0x7fffffff;
    }

    auto scan_leaf = [&](int32_t L) {
        const double* p = t.pts + (int64_t)L * D * PF_WAVE + lane;
        double x[D];
#pragma unroll
        for (int c = 0; c < D; ++c) x[c] = p[c * PF_WAVE];
        const int32_t o = t.orig[(int64_t)L * PF_WAVE + lane];
#pragma unroll
        for (int i = 0; i < G; ++i) {
            double s = 0.0;
            constexpr int P = D >= 6 ? D / 2 : D;
#pragma unroll
            for (int c = 0; c < P; ++c) {
                const double df = q[i][c] - x[c];
                const double sq = df * df;
                s = (c == 0) ? sq : s + sq;
            }
            if constexpr (P < D) {
                if (!__any(s <= kd[i])) continue;  // (the partial sum is a prefix of the same accumulation and only grows)
#pragma unroll
                for (int c = P; c < D; ++c) {
                    const double df = q[i][c] - x[c];
                    s = s + df * df;
                }
            }
            // the copies that fill the last leaf are no neighbours
            list_offer(nd[i], ni[i], kd[i], ki[i], o == 0x7fffffff ? (double)INFINITY : s, o, k, lane);
        }
    };

    // ---- the first candidates: the leaf nearest to the group's first query inside the super nearest to it
    int32_t L0;
    {
        double sb = INFINITY;
        int32_t sa = 0;
        for (int32_t s0 = 0; s0 < t.ns_pad; s0 += PF_WAVE) {
            const double dd = box_d2<D>(q[0], t.sup_lo + s0 + lane, t.sup_hi + s0 + lane, t.ns_pad);
            if (dd < sb) sb = dd, sa = s0 + lane;
        }
        wave_argmin(sb, sa);
        sa = sa < t.n_sup ? sa : 0;  // (the supers past the end are infinitely far and lose every tie: a guard, not a case)
        const int64_t lb = (int64_t)sa * D * PF_WAVE + lane;
        double lbest = box_d2<D>(q[0], t.leaf_lo + lb, t.leaf_hi + lb, PF_WAVE);
        int32_t la = lane;
        wave_argmin(lbest, la);
        L0 = sa * PF_WAVE + la;
        if (L0 < t.n_leaf)
            scan_leaf(L0);
        else
            L0 = -1;
    }
    // ---- every super whose box is within a query's bound, every leaf of it whose box is; the bound may move with every leaf
    for (int32_t s0 = 0; s0 < t.ns_pad; s0 += PF_WAVE) {
        double sd[G];
#pragma unroll
        for (int i = 0; i < G; ++i) sd[i] = box_d2<D>(q[i], t.sup_lo + s0 + lane, t.sup_hi + s0 + lane, t.ns_pad);
        unsigned long long sdone = 0ull;
        while (true) {
            bool need = false;
#pragma unroll
            for (int i = 0; i < G; ++i) need = need || sd[i] <= kd[i];
            const unsigned long long sm = __ballot(need) & ~sdone;
            if (!sm) break;
            const int sbit = __ffsll((long long)sm) - 1;
            sdone |= 1ull << sbit;
            const int32_t S = s0 + sbit;
            if (S >= t.n_sup) continue;
            const int64_t lb = (int64_t)S * D * PF_WAVE + lane;
            double bd[G];
#pragma unroll
            for (int i = 0; i < G; ++i) bd[i] = box_d2<D>(q[i], t.leaf_lo + lb, t.leaf_hi + lb, PF_WAVE);
            unsigned long long ldone = 0ull;
            while (true) {
                bool ln = false;
#pragma unroll
                for (int i = 0; i < G; ++i) ln = ln || bd[i] <= kd[i];
                const unsigned long long lm = __ballot(ln) & ~ldone;
                if (!lm) break;
                const int lbit = __ffsll((long long)lm) - 1;
                ldone |= 1ull << lbit;
                const int32_t L = S * PF_WAVE + lbit;
                if (L < t.n_leaf && L != L0) scan_leaf(L);
            }
        }
    }
#pragma unroll
    for (int i = 0; i < G; ++i) {
        if (i < nq && lane < k) {
            t.idx_out[(int64_t)qdst[i] * k + lane] = ni[i];
            t.d2_out[(int64_t)qdst[i] * k + lane] = nd[i];
        }
    }
}

// out[c][i] = in[i][c]: the references coordinate-major, so that a wave reads one coordinate of 64 of them as 512
// contiguous bytes
__global__ __launch_bounds__(PF_BLOCK) void k_topk_transpose(const double* __restrict__ in, int64_t n, int32_t d, double* __restrict__ out) {
    const int64_t e = (int64_t)blockIdx.x * PF_BLOCK + threadIdx.x;
    if (e >= n * d) return;
    const int64_t c = e / n, i = e - c * n;
    out[e] = in[i * d + c];
}

// 16 < d <= 128 (any d >= 1 is correct): the lists of WIDE_G consecutive queries per wave over ALL references, 64 at a
// time, one per lane; the queries' coordinates are wave-uniform loads
constexpr int WIDE_G = 4;
__global__ __launch_bounds__(PF_BLOCK) void k_knn_topk_wide(const double* __restrict__ rt /* [d][n_ref] */, int64_t n_ref,
                                                            const double* __restrict__ qry, int64_t n_qry, int d, int k,
                                                            int64_t* __restrict__ idx_out, double* __restrict__ d2_out) {
    const int lane = threadIdx.x & (PF_WAVE - 1);
    const int64_t group = (int64_t)blockIdx.x * (PF_BLOCK / PF_WAVE) + __builtin_amdgcn_readfirstlane((int)(threadIdx.x / PF_WAVE));
    const int64_t q0 = group * WIDE_G;
    if (q0 >= n_qry) return;  // (wave-uniform)
    const int nq = n_qry - q0 < WIDE_G ? (int)(n_qry - q0) : WIDE_G;
    const double* qp[WIDE_G];  // (a short group replays its last query)
    double nd[WIDE_G], kd[WIDE_G];
    int32_t ni[WIDE_G], ki[WIDE_G];
#pragma unroll
    for (int i = 0; i < WIDE_G; ++i) {
        qp[i] = qry + (q0 + (i < nq ? i : nq - 1)) * d;
        nd[i] = kd[i] = INFINITY;
        ni[i] = ki[i] = 0x7fffffff;
    }
    for (int64_t r0 = 0; r0 < n_ref; r0 += PF_WAVE) {
        const bool real = r0 + lane < n_ref;
        const double* p = rt + (real ? r0 + lane : n_ref - 1);  // (lanes past the end read the last reference and offer nothing)
        double s[WIDE_G];
#pragma unroll
        for (int i = 0; i < WIDE_G; ++i) s[i] = 0.0;  // 0 + x^2 is x^2: the sum starts at coordinate 0
#pragma unroll 4
        for (int c = 0; c < d; ++c) {
            const double x = p[(int64_t)c * n_ref];
#pragma unroll
            for (int i = 0; i < WIDE_G; ++i) {
                const double df = qp[i][c] - x;
                s[i] = s[i] + df * df;
            }
        }
        const int32_t o = real ? (int32_t)(r0 + lane) : 0x7fffffff;
#pragma unroll
        for (int i = 0; i < WIDE_G; ++i) list_offer(nd[i], ni[i], kd[i], ki[i], real ? s[i] : (double)INFINITY, o, k, lane);
    }
#pragma unroll
    for (int i = 0; i < WIDE_G; ++i) {
        if (i < nq && lane < k) {
            idx_out[(q0 + i) * k + lane] = ni[i];
            d2_out[(q0 + i) * k + lane] = nd[i];
        }
    }
}

int tree_launched(const char* what) {
    const hipError_t e = hipGetLastError();
    PF_CHECK(e == hipSuccess, PF_E_HIP, "%s (box hierarchy): %s", what, hipGetErrorString(e));
    return PF_OK;
}

template <int D>
int launch_tree(pf_ctx* c, const TreeArgs& a) {
    const int64_t waves = (a.n_qry + tree_group(D) - 1) / tree_group(D);
    k_knn_tree<D><<<(unsigned)((waves + PF_BLOCK / PF_WAVE - 1) / (PF_BLOCK / PF_WAVE)), PF_BLOCK, 0, c->stream>>>(a);
    return tree_launched("pf_knn");
}

template <int D>
int launch_tree_topk(pf_ctx* c, const TreeArgs& a, int k) {
    const int64_t waves = (a.n_qry + tree_group(D) - 1) / tree_group(D);
    k_knn_tree_topk<D><<<(unsigned)((waves + PF_BLOCK / PF_WAVE - 1) / (PF_BLOCK / PF_WAVE)), PF_BLOCK, 0, c->stream>>>(a, k);
    return tree_launched("pf_knn_topk");
}

// The hierarchy over the n references (row-major, d <= 16; ext: their encoded extents, as pf_knn_extent leaves them) and the
// nq queries' order along the references' Morton curve, queued on the ctx's stream into the ctx's pf_knn_tree buffers:
// keys, sort, leaves, leaf boxes, super boxes, query order.  Fills every field of `a` but the two outputs.
int tree_build(pf_ctx* c, const double* ref, int64_t n, const double* qry, int64_t nq, int d, const unsigned long long* ext, TreeArgs* a) {
    hipStream_t st = c->stream;
    pf_knn_tree& T = c->knn_tree;
    const int64_t n_leaf = (n + PF_WAVE - 1) / PF_WAVE;
    const int64_t n_sup = (n_leaf + PF_WAVE - 1) / PF_WAVE;
    const int64_t ns_pad = (n_sup + PF_WAVE - 1) & ~(int64_t)(PF_WAVE - 1);
    PF_CHECK(n_leaf < ((int64_t)1 << 31) / PF_WAVE, PF_E_ARG, "pf_knn: too many references for the box hierarchy");
    PF_HIP(T.pts.grow(st, n_leaf * PF_WAVE * d));
    PF_HIP(T.orig.grow(st, n_leaf * PF_WAVE));
    PF_HIP(T.leaf_lo.grow(st, 2 * n_sup * PF_WAVE * d));
    PF_HIP(T.sup_lo.grow(st, 2 * ns_pad * d));
    PF_HIP(T.qry_order.grow(st, nq));
    Scratch s(st);
    if (!T.grid) T.grid = s.keep<TreeGrid>(1);
    if (!T.counters) T.counters = s.keep<unsigned long long>(2);
    PF_HIP(s.err);
    PF_HIP(hipMemsetAsync(T.counters, 0, 2 * sizeof(unsigned long long), st));
    double* leaf_hi = T.leaf_lo.p + n_sup * PF_WAVE * d;
    double* sup_hi = T.sup_lo.p + ns_pad * d;
    const int64_t nmax = std::max(n, nq);
    unsigned *k0 = s.get<unsigned>(nmax), *k1 = s.get<unsigned>(nmax);
    int32_t *v0 = s.get<int32_t>(nmax), *v1 = s.get<int32_t>(nmax);
    PF_CHECK(s.ok(), PF_E_HIP, "pf_knn: out of device memory (box hierarchy)");
    k_tree_grid<<<1, 1, 0, st>>>(ext, d, (TreeGrid*)T.grid);
    k_tree_keys<<<pf_blocks(n), PF_BLOCK, 0, st>>>(ref, n, d, (const TreeGrid*)T.grid, k0, v0);
    pf_sort_pairs(s, k0, k1, v0, v1, n, 30);
    if (s.ok()) {
        k_tree_leaves<<<pf_blocks(n_leaf * PF_WAVE), PF_BLOCK, 0, st>>>(ref, v1, n, d, n_leaf * PF_WAVE, T.pts.p, T.orig.p);
        k_tree_leaf_boxes<<<pf_blocks(n_sup * PF_WAVE * d), PF_BLOCK, 0, st>>>(T.pts.p, (int32_t)n_leaf, (int32_t)n_sup, d, T.leaf_lo.p, leaf_hi);
        k_tree_super_boxes<<<pf_blocks(ns_pad * d), PF_BLOCK, 0, st>>>(T.leaf_lo.p, leaf_hi, (int32_t)n_sup, (int32_t)ns_pad, d, T.sup_lo.p, sup_hi);
        k_tree_keys<<<pf_blocks(nq), PF_BLOCK, 0, st>>>(qry, nq, d, (const TreeGrid*)T.grid, k0, v0);
    }
    pf_sort_pairs(s, k0, k1, v0, T.qry_order.p, nq, 30);
    PF_HIP(s.err);
    *a = TreeArgs{T.pts.p, T.orig.p, T.leaf_lo.p, leaf_hi, T.sup_lo.p, sup_hi, qry, T.qry_order.p, nq, (int32_t)n_leaf, (int32_t)n_sup,
                  (int32_t)ns_pad, nullptr, nullptr, T.count_visits ? T.counters : nullptr};
    return PF_OK;
}

}  // namespace

// The search of pf_knn_run for k = 1 through the box hierarchy: c->knn_ref / knn_qry hold the coordinates (row-major),
// c->knn_ext the encoded extents of the references; results into c->knn_idx / knn_d2.
int pf_knn_tree_run(pf_ctx* c) {
    const int d = c->knn_d;
    TreeArgs a{};
    PF_TRY(tree_build(c, c->knn_ref.p, c->knn_nref, c->knn_qry.p, c->knn_nqry, d, c->knn_ext, &a));
    a.idx_out = c->knn_idx.p;
    a.d2_out = c->knn_d2.p;
    return pf_dispatch_d<1, 16>(d, [&](auto D) { return launch_tree<D()>(c, a); }, "pf_knn: no box hierarchy for d = %d");
}

// k nearest neighbours, 1 <= k <= 64, 1 <= d <= 128 (include/pyfocusr_hip.h): the lists over the box hierarchy for
// d <= 16, over an exhaustive scan beyond
extern "C" int pf_knn_topk(pf_ctx* c, const double* ref, int64_t n_ref, const double* qry, int64_t n_qry, int32_t d, int32_t k,
                           int64_t* idx_out, double* d2_out) {
    PF_CHECK(c && ref && qry && idx_out, PF_E_ARG, "pf_knn_topk: NULL argument");
    PF_CHECK(n_ref > 0 && n_ref < ((int64_t)1 << 31) && n_qry > 0 && n_qry < ((int64_t)1 << 31) && d >= 1 && d <= 128, PF_E_ARG,
             "pf_knn_topk: n_ref %lld, n_qry %lld, d %d out of range (1 <= d <= 128)", (long long)n_ref, (long long)n_qry, d);
    PF_CHECK(k >= 1 && k <= PF_WAVE && k <= n_ref, PF_E_ARG, "pf_knn_topk: k = %d out of range (1..64, <= n_ref)", k);
    PF_HIP(hipSetDevice(c->device));
    Scratch s(c->stream);
    const size_t count = (size_t)n_qry * k;
    double* d_ref = s.get<double>((size_t)(n_ref * d));
    double* d_qry = s.get<double>((size_t)(n_qry * d));
    int64_t* d_idx = s.get<int64_t>(count);
    double* d_d2 = s.get<double>(count);
    s.upload(d_ref, ref, (size_t)(n_ref * d));
    s.upload(d_qry, qry, (size_t)(n_qry * d));
    PF_CHECK(s.ok(), PF_E_HIP, "pf_knn_topk: %s", hipGetErrorString(s.err));
    PF_HIP(hipEventRecord(c->ev0, s.st));
    if (d <= PF_ND_MAX) {
        unsigned long long* ext = s.get<unsigned long long>(32);
        PF_CHECK(s.ok(), PF_E_HIP, "pf_knn_topk: %s", hipGetErrorString(s.err));
        PF_TRY(pf_knn_extent(s.st, d_ref, n_ref, d, ext));
        TreeArgs a{};
        PF_TRY(tree_build(c, d_ref, n_ref, d_qry, n_qry, d, ext, &a));
        a.idx_out = d_idx;
        a.d2_out = d_d2;
        const int rc = pf_dispatch_d<1, 16>(d, [&](auto D) { return launch_tree_topk<D()>(c, a, k); }, "pf_knn_topk: no box hierarchy for d = %d");
        PF_TRY(rc);
    } else {
        double* d_rt = s.get<double>((size_t)(n_ref * d));
        PF_CHECK(s.ok(), PF_E_HIP, "pf_knn_topk: %s", hipGetErrorString(s.err));
        k_topk_transpose<<<pf_blocks(n_ref * d), PF_BLOCK, 0, s.st>>>(d_ref, n_ref, d, d_rt);
        const int64_t waves = (n_qry + WIDE_G - 1) / WIDE_G;
        k_knn_topk_wide<<<(unsigned)((waves + PF_BLOCK / PF_WAVE - 1) / (PF_BLOCK / PF_WAVE)), PF_BLOCK, 0, s.st>>>(d_rt, n_ref, d_qry, n_qry, d, k,
                                                                                                                  d_idx, d_d2);
        PF_TRY(tree_launched("pf_knn_topk"));
    }
    PF_HIP(hipEventRecord(c->ev1, s.st));
    // one read-back: both halves queued, one wait
    s.download(idx_out, d_idx, count);
    s.download(d2_out, d_d2, count);
    s.sync();
    PF_CHECK(s.ok(), PF_E_HIP, "pf_knn_topk: %s", hipGetErrorString(s.err));
    float ms = 0.f;
    PF_HIP(hipEventElapsedTime(&ms, c->ev0, c->ev1));
    c->knn_ms = ms;
    return PF_OK;
}

// diagnostics of the last box-hierarchy search (pf_knn_tree_count(ctx, 1) switches the counting on): leaves scanned and
// supers opened, summed over the waves
extern "C" int pf_knn_tree_stats(pf_ctx* c, int32_t enable_counting, int64_t* leaves_scanned, int64_t* supers_opened) {
    PF_CHECK(c != nullptr, PF_E_ARG, "pf_knn_tree_stats: ctx is NULL");
    unsigned long long h[2] = {0ull, 0ull};
    if (c->knn_tree.counters) {
        PF_HIP(hipMemcpyAsync(h, c->knn_tree.counters, sizeof(h), hipMemcpyDeviceToHost, c->stream));
        PF_HIP(hipStreamSynchronize(c->stream));
    }
    if (leaves_scanned) *leaves_scanned = (int64_t)h[0];
    if (supers_opened) *supers_opened = (int64_t)h[1];
    c->knn_tree.count_visits = enable_counting != 0;
    return PF_OK;
}
