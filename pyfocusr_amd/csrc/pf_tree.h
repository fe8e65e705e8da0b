// The library's fixed tree of a sum over n terms in ascending order (pf_map_quality.hip states it first): 256 consecutive
// terms left to right from 0.0, 256 of those sums likewise, the rest in order.  Here for `rows` quantities at once whose
// terms lie as [node][quantity]: the sums of pf_shapes.hip over the vertices of a population, and the volumes and the
// vertex mean of pf_smooth.hip.  Included per unit (no device code crosses translation units).
#pragma once
#include "pf_internal.h"

constexpr int PF_TREE_GROUP = 256;  // terms per node of the tree

inline int64_t pf_tree_runs(int64_t n) { return (n + PF_TREE_GROUP - 1) / PF_TREE_GROUP; }

// One level of the tree over `rows` quantities, partials as [node][quantity]: out[o][q] = in[group o .. group (o + 1))[q]
// summed left to right from 0.0 as far as the nodes go; group == 0: every node (n_out == 1).
static __global__ __launch_bounds__(PF_BLOCK) void k_tree_level(const double* __restrict__ in, int64_t n_in, double* __restrict__ out,
                                                                int64_t n_out, int64_t rows, int64_t group) {
    const int64_t idx = (int64_t)blockIdx.x * PF_BLOCK + threadIdx.x;
    if (idx >= rows * n_out) return;
    const int64_t o = idx / rows, q = idx - o * rows;
    const int64_t lo = group * o, hi = group ? min(lo + group, n_in) : n_in;
    double sum = 0.0;
    for (int64_t k = lo; k < hi; ++k) sum += in[k * rows + q];
    out[o * rows + q] = sum;
}

// The levels above lev [n_nodes][rows], whose nodes are at `level` of the tree (0: the terms themselves, 1: sums of 256
// terms, 2: sums of 65 536) -> the device block of the `rows` sums, scratch of sc
inline double* pf_tree_reduce(Scratch& sc, const double* lev, int64_t n_nodes, int64_t rows, int level) {
    hipStream_t st = sc.st;
    for (; level < 2; ++level) {
        const int64_t n_up = pf_tree_runs(n_nodes);
        double* up = sc.get<double>(n_up * rows);
        if (sc.ok()) k_tree_level<<<pf_blocks(rows * n_up), PF_BLOCK, 0, st>>>(lev, n_nodes, up, n_up, rows, PF_TREE_GROUP);
        lev = up, n_nodes = n_up;
    }
    double* sums = sc.get<double>(rows);
    if (sc.ok()) {
        k_tree_level<<<pf_blocks(rows), PF_BLOCK, 0, st>>>(lev, n_nodes, sums, 1, rows, 0);
        sc.launched();
    }
    return sums;
}
