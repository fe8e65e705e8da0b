// The half-edge pass that the mesh-analysis units share (pf_surface.hip: signed distances; pf_curvature.hip;
// pf_topology.hip): device pieces, included per unit, so no device code crosses translation units.
//
// Half-edge h = 3 t + j leaves corner j of triangle t for corner next(j).  One stable radix sort of the half-edges by
// their edge's key (min << nb | max, nb = pf_index_bits(n)) makes the half-edges of an edge a run in ascending h, so a
// run's first half-edge belongs to its lowest triangle; a second one by the corner's vertex makes the half-edges that
// leave a vertex a run in ascending h.  A kernel over edges has one thread per sorted position and lets the thread that
// heads a run act for the edge (he_run_end); a kernel over vertices finds its run by bisection (he_vertex_run).
// Arithmetic: separate multiplies and adds (the library is built without contraction), dot products left to right.
#pragma once
#include <cmath>

#include "pf_internal.h"

__device__ __forceinline__ int he_next(int j) { return j == 2 ? 0 : j + 1; }
__device__ __forceinline__ int he_prev(int j) { return j == 0 ? 2 : j - 1; }

// the key of edge {a, b} under nb bits per vertex index
__device__ __forceinline__ unsigned long long he_edge_key(int32_t a, int32_t b, int nb) {
    const unsigned lo = (unsigned)min(a, b), hi = (unsigned)max(a, b);
    return ((unsigned long long)lo << nb) | hi;
}

__device__ __forceinline__ double dot3(const double a[3], const double b[3]) { return a[0] * b[0] + a[1] * b[1] + a[2] * b[2]; }
__device__ __forceinline__ void cross3(const double a[3], const double b[3], double c[3]) {
    c[0] = a[1] * b[2] - a[2] * b[1];
    c[1] = a[2] * b[0] - a[0] * b[2];
    c[2] = a[0] * b[1] - a[1] * b[0];
}

// The triangle pass, for the thread of triangle t with corners v: unit normal, corner angles atan2(|e1 x e2|, e1 . e2)
// and, where tarea is given, area - all zero for a zero-area or non-finite triangle; per half-edge 3 t + j the key of its
// edge, its corner's vertex, and h itself as the value of both sorts.
__device__ __forceinline__ void he_triangle(const double* __restrict__ pts, const int32_t v[3], int64_t t, int nb,
                                            double* __restrict__ tnrm, double* __restrict__ tang, double* __restrict__ tarea,
                                            unsigned long long* __restrict__ ekey, unsigned* __restrict__ vkey,
                                            int32_t* __restrict__ hval) {
    double x[3][3];
#pragma unroll
    for (int c = 0; c < 3; ++c)
#pragma unroll
        for (int a = 0; a < 3; ++a) x[c][a] = pts[3 * (int64_t)v[c] + a];
    const double u[3] = {x[1][0] - x[0][0], x[1][1] - x[0][1], x[1][2] - x[0][2]};
    const double w[3] = {x[2][0] - x[0][0], x[2][1] - x[0][1], x[2][2] - x[0][2]};
    double cr[3];
    cross3(u, w, cr);
    const double len = sqrt(dot3(cr, cr));
    const bool area = len > 0.0 && std::isfinite(len);
#pragma unroll
    for (int a = 0; a < 3; ++a) tnrm[3 * t + a] = area ? cr[a] / len : 0.0;
    if (tarea) tarea[t] = area ? len / 2.0 : 0.0;
#pragma unroll
    for (int j = 0; j < 3; ++j) {
        const int j1 = he_next(j), j2 = he_prev(j);
        const double e1[3] = {x[j1][0] - x[j][0], x[j1][1] - x[j][1], x[j1][2] - x[j][2]};
        const double e2[3] = {x[j2][0] - x[j][0], x[j2][1] - x[j][1], x[j2][2] - x[j][2]};
        double c[3];
        cross3(e1, e2, c);
        tang[3 * t + j] = area ? atan2(sqrt(dot3(c, c)), dot3(e1, e2)) : 0.0;
        ekey[3 * t + j] = he_edge_key(v[j], v[j1], nb);
        vkey[3 * t + j] = (unsigned)v[j];
        hval[3 * t + j] = (int32_t)(3 * t + j);
    }
}

// Sorted position i of n_half edge keys: the end of the run of equal keys that i heads, or i itself when it heads none
// (it lies inside a run, or behind the last key).
__device__ __forceinline__ int64_t he_run_end(const unsigned long long* __restrict__ ekey, int64_t n_half, int64_t i) {
    if (i >= n_half || (i > 0 && ekey[i - 1] == ekey[i])) return i;
    const unsigned long long key = ekey[i];
    int64_t end = i + 1;
    while (end < n_half && ekey[end] == key) ++end;
    return end;
}

// counts: edges | boundary | non-manifold | inconsistent, for the edge of a run of m half-edges; fwd0 and fwd1 (read for
// m == 2 only) say whether its two half-edges go from the lower vertex to the higher one.  Integer atomics: the same on
// every run.
__device__ __forceinline__ void he_count_edge(unsigned long long* __restrict__ counts, int64_t m, bool fwd0, bool fwd1) {
    atomicAdd(&counts[0], 1ull);
    if (m == 1) atomicAdd(&counts[1], 1ull);
    if (m > 2) atomicAdd(&counts[2], 1ull);
    if (m == 2 && fwd0 == fwd1) atomicAdd(&counts[3], 1ull);
}

// the first sorted position whose vertex key is >= v: where the run of the half-edges that leave v starts, if it has one
__device__ __forceinline__ int64_t he_vertex_run(const unsigned* __restrict__ vkey, int64_t n_half, int64_t v) {
    int64_t lo = 0, hi = n_half;
    while (lo < hi) {
        const int64_t mid = (lo + hi) >> 1;
        if (vkey[mid] < (unsigned)v) lo = mid + 1;
        else hi = mid;
    }
    return lo;
}
