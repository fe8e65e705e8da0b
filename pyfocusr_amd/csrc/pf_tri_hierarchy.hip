// The build of the triangle hierarchy (pf_tri_hierarchy.h has the structure): Morton keys of centroids or points, the
// stable sort, the gather into SoA, the chunk and super-chunk boxes; and its release.  Every kernel has the instance
// D = 3 of the 3-D surface and the instance D = 0 for any other depth.
#include <cmath>

#include "pf_tri_hierarchy.h"

namespace {

// 30-bit Morton key of the leading coordinates of a point in box bb: 10 bits per axis, the first lowest; outside the box
// clamps, NaN and a flat axis give 0.  The point comes as coord(axis), so that an axis is loaded where it is used
// (registers: as few as the loops this replaces).
template <int D, class Coord>
__device__ __forceinline__ unsigned morton_key(Coord coord, const KeyBox& bb) {
    const int nk = D ? (D < 3 ? D : 3) : bb.nk;
    unsigned code = 0;
#pragma unroll
    for (int a = 0; a < 3; ++a) {
        if (a >= nk) break;
        double u = bb.ext[a] > 0.0 ? (coord(a) - bb.lo[a]) / bb.ext[a] : 0.0;
        u = u < 0.0 ? 0.0 : (u > 1.0 ? 1.0 : u);
        if (!(u == u)) u = 0.0;  // the clamp lets NaN through
        code |= spread10((unsigned)(u * 1023.0)) << a;
    }
    return code;
}

template <int D>
__global__ __launch_bounds__(PF_BLOCK) void k_tri_keys(const double* __restrict__ pts, int32_t d_any, const int32_t* __restrict__ faces,
                                                       int32_t vpf, int64_t n_tri, KeyBox bb, unsigned* __restrict__ keys,
                                                       int32_t* __restrict__ vals) {
    const int d = D ? D : d_any;
    const int64_t t = (int64_t)blockIdx.x * PF_BLOCK + threadIdx.x;
    if (t >= n_tri) return;
    int32_t v[3];
    tri_corners(faces, vpf, t, v);
    const auto centroid = [&](int a) { return (pts[(int64_t)v[0] * d + a] + pts[(int64_t)v[1] * d + a] + pts[(int64_t)v[2] * d + a]) / 3.0; };
    keys[t] = morton_key<D>(centroid, bb);
    vals[t] = (int32_t)t;
}

template <int D>
__global__ __launch_bounds__(PF_BLOCK) void k_qry_keys(const double* __restrict__ qry, int32_t d_any, int64_t n, KeyBox bb,
                                                       unsigned* __restrict__ keys, int32_t* __restrict__ vals) {
    const int d = D ? D : d_any;
    const int64_t i = (int64_t)blockIdx.x * PF_BLOCK + threadIdx.x;
    if (i >= n) return;
    keys[i] = morton_key<D>([&](int a) { return qry[i * d + a]; }, bb);
    vals[i] = (int32_t)i;
}

template <int D>
__global__ __launch_bounds__(PF_BLOCK) void k_tri_gather(const double* __restrict__ pts, int32_t d_any, const int32_t* __restrict__ faces,
                                                         int32_t vpf, int64_t n_tri, const int32_t* __restrict__ order,
                                                         double* __restrict__ tri, int32_t* __restrict__ tri_orig) {
    const int d = D ? D : d_any;
    const int64_t s = (int64_t)blockIdx.x * PF_BLOCK + threadIdx.x;
    if (s >= n_tri) return;
    const int32_t t = order[s];
    int32_t v[3];
    tri_corners(faces, vpf, t, v);
#pragma unroll
    for (int c = 0; c < 3; ++c) PF_FOR_DEPTH(k) tri[(int64_t)(c * d + k) * n_tri + s] = pts[(int64_t)v[c] * d + k];
    tri_orig[s] = t;
}

// one wave per chunk, one triangle per lane
template <int D>
__global__ __launch_bounds__(PF_WAVE) void k_chunk_boxes(const double* __restrict__ tri, int64_t n_tri, int32_t d_any, double* __restrict__ box) {
    const int d = D ? D : d_any;
    const int64_t c = blockIdx.x;
    const int lane = threadIdx.x;
    const int64_t s = c * PF_TRI_CHUNK + lane;
    const double inf = std::numeric_limits<double>::infinity();
    PF_FOR_DEPTH(k) {
        double lo = inf, hi = -inf;
        if (s < n_tri) {
#pragma unroll
            for (int cr = 0; cr < 3; ++cr) {
                const double x = tri[(int64_t)(cr * d + k) * n_tri + s];
                lo = fmin(lo, x);  // fmin/fmax ignore NaN: a NaN vertex never widens a box
                hi = fmax(hi, x);
            }
        }
        lo = wave_min(lo), hi = wave_max(hi);
        if (lane == 0) {
            box[2 * d * c + k] = lo;
            box[2 * d * c + d + k] = hi;
        }
    }
}

// one wave per super-chunk: union of its 64 chunk boxes
template <int D>
__global__ __launch_bounds__(PF_WAVE) void k_super_boxes(const double* __restrict__ box, int64_t n_chunks, int32_t d_any,
                                                         double* __restrict__ sbox) {
    const int d = D ? D : d_any;
    const int64_t c = (int64_t)blockIdx.x * PF_WAVE + threadIdx.x;
    const double inf = std::numeric_limits<double>::infinity();
    PF_FOR_DEPTH(k) {
        const double lo = wave_min(c < n_chunks ? box[2 * d * c + k] : inf), hi = wave_max(c < n_chunks ? box[2 * d * c + d + k] : -inf);
        if (threadIdx.x == 0) {
            sbox[2 * d * (int64_t)blockIdx.x + k] = lo;
            sbox[2 * d * (int64_t)blockIdx.x + d + k] = hi;
        }
    }
}

template <int D>
void launch_keys(hipStream_t st, const double* d_pts, int32_t d, const int32_t* d_faces, int32_t vpf, int64_t n, const KeyBox& bb,
                 unsigned* keys, int32_t* vals) {
    if (d_faces)
        k_tri_keys<D><<<pf_blocks(n), PF_BLOCK, 0, st>>>(d_pts, d, d_faces, vpf, n, bb, keys, vals);
    else
        k_qry_keys<D><<<pf_blocks(n), PF_BLOCK, 0, st>>>(d_pts, d, n, bb, keys, vals);
}

template <int D>
void launch_build(hipStream_t st, const TriHierarchy& h, const double* d_pts, const int32_t* d_faces, int32_t vpf, const int32_t* order) {
    k_tri_gather<D><<<pf_blocks(h.n_tri), PF_BLOCK, 0, st>>>(d_pts, h.d, d_faces, vpf, h.n_tri, order, h.tri, h.tri_orig);
    k_chunk_boxes<D><<<(unsigned)h.n_chunks, PF_WAVE, 0, st>>>(h.tri, h.n_tri, h.d, h.box);
    k_super_boxes<D><<<(unsigned)h.n_super, PF_WAVE, 0, st>>>(h.box, h.n_chunks, h.d, h.sbox);
}

}  // namespace

KeyBox pf_key_box(const double* pts, int64_t n, int32_t d, bool finite_only) {
    KeyBox bb;
    bb.nk = d < 3 ? d : 3;
    for (int a = 0; a < 3; ++a) {
        bb.lo[a] = bb.ext[a] = 0.0;
        if (a >= bb.nk) continue;
        double lo = std::numeric_limits<double>::infinity(), hi = -lo;
        for (int64_t i = 0; i < n; ++i) {
            const double x = pts[i * d + a];
            if (finite_only && !std::isfinite(x)) continue;
            if (x < lo) lo = x;
            if (x > hi) hi = x;
        }
        bb.lo[a] = lo;
        bb.ext[a] = hi - lo;
        if (!(bb.ext[a] > 0.0) || !std::isfinite(bb.ext[a])) bb.ext[a] = 0.0;
    }
    return bb;
}

const int32_t* pf_surface_morton_order(Scratch& sc, const double* d_pts, int32_t d, const int32_t* d_faces, int32_t vpf, int64_t n,
                                       const KeyBox& bb) {
    unsigned *k0 = sc.get<unsigned>(n), *k1 = sc.get<unsigned>(n);
    int32_t *v0 = sc.get<int32_t>(n), *v1 = sc.get<int32_t>(n);
    if (sc.ok()) {
        if (d == 3)
            launch_keys<3>(sc.st, d_pts, d, d_faces, vpf, n, bb, k0, v0);
        else
            launch_keys<0>(sc.st, d_pts, d, d_faces, vpf, n, bb, k0, v0);
        sc.launched();
    }
    pf_sort_pairs(sc, k0, k1, v0, v1, n, 30);
    return sc.ok() ? v1 : nullptr;
}

void pf_tri_hierarchy_build(Scratch& sc, TriHierarchy& h, const double* d_pts, int32_t d, const int32_t* d_faces, int64_t n_faces,
                            int32_t vpf, const KeyBox& bb) {
    h.d = d;
    h.n_tri = n_faces * (vpf - 2);
    h.n_chunks = (h.n_tri + PF_TRI_CHUNK - 1) / PF_TRI_CHUNK;
    h.n_super = (h.n_chunks + PF_WAVE - 1) / PF_WAVE;
    h.tri = sc.keep<double>(3 * d * h.n_tri);
    h.tri_orig = sc.keep<int32_t>(h.n_tri);
    h.box = sc.keep<double>(2 * d * h.n_chunks);
    h.sbox = sc.keep<double>(2 * d * h.n_super);
    const int32_t* order = pf_surface_morton_order(sc, d_pts, d, d_faces, vpf, h.n_tri, bb);
    if (sc.ok()) {
        if (d == 3)
            launch_build<3>(sc.st, h, d_pts, d_faces, vpf, order);
        else
            launch_build<0>(sc.st, h, d_pts, d_faces, vpf, order);
        sc.launched();
    }
}

void pf_tri_hierarchy_free(hipStream_t st, TriHierarchy& h) {
    pf_free(st, h.tri), pf_free(st, h.tri_orig), pf_free(st, h.box), pf_free(st, h.sbox);
    h = TriHierarchy();
}
