// Queries against a triangulated surface: closest points, many-query distances, signed distances, winding numbers,
// ray casting.  All five work on one structure, built once per surface (pf_surface_create): the triangle hierarchy of
// pf_tri_hierarchy.h at d = 3 - fan triangles along a Morton curve, chunks of 64 with their boxes, super-chunks of 64
// chunks - which that header describes together with the argument why pruning by its boxes changes no result.  In the
// order of the file:
//
// Closest point (pf_surface_closest, k_closest) - the search inside the ICP pre-alignment (reference:
// vtk_functions.py:12-29 -> vtkIterativeClosestPointTransform, whose inner loop asks a vtkCellLocator for the closest
// surface point of <= 1000 landmarks, 100 times).  Exact, no approximation: the answer is the minimum
// over ALL triangles of the exact point-triangle distance (ties: lowest triangle index), the same as a brute-force scan;
// pruning only removes triangles that provably cannot win.  ONE BLOCK (4 waves) PER QUERY POINT.  (1) the nearest
// super-chunk, then the nearest chunk inside it, by point-box distance (one box per lane, nearest_chunk); that chunk is
// scanned first and yields an upper bound.  (2) one ballot over the super-chunk boxes, then per surviving super-chunk
// one ballot over its 64 chunk boxes; the surviving chunks are dealt round-robin to the 4 waves, which scan them one
// triangle per lane, 4 chunks per step (loads issued together), re-deriving the bound after every step.  Measured on a
// 250k pair: 41 chunk scans per landmark on average but 420 for the farthest one, and the kernel lasts as long as its
// slowest query - hence 4 waves x 4 chunks per step on that chain of dependent loads.
// The arithmetic of closest_on_triangle is Ericson's region walk, operation for operation the one in
// oracle/icp_port.py (compiled with -ffp-contract=off), so points and distances are bit-identical to it.  There is one
// body of it; every exact test of the file goes through it.
//
// Many-query distances (pf_surface_distance, k_distance): the queries are Morton-sorted too and walk the same
// hierarchy one packet of neighbouring queries per wave, with the same exact tests and tie rule as k_closest.
//
// Signed distances (pf_surface_prepare_signed / pf_surface_signed_distance): angle-weighted pseudonormals, built once
// per surface on request by the half-edge pass of pf_halfedge.h, and one per-query kernel after the unchanged k_distance
// search that names the feature (face, edge, vertex) of the winning triangle the closest point lies on.
//
// Generalized winding numbers (pf_surface_prepare_winding / pf_surface_winding): the solid angles of all triangles,
// summed over the same chunks, exactly or with far clusters replaced by their dipoles.
//
// Ray casting (pf_surface_raycast, k_raycast): first hit, barycentric coordinates and crossing count of many rays, by
// one exact FP64 Moeller-Trumbore test over the same boxes; pf_surface_vertex_normals hands out the vertex pseudonormals
// of the signed structure as ray directions.
//
// Each section's own comment has the details.  The entry points (extern "C", at the end) keep their device scratch in a
// Scratch, and sort along the Morton curve through pf_surface_morton_order.
#include <cmath>
#include <limits>

#include "pf_halfedge.h"
#include "pf_tri_hierarchy.h"

struct pf_surface {
    pf_ctx* ctx = nullptr;
    int64_t n_points = 0, n_faces = 0;
    int32_t vpf = 0;
    TriHierarchy h;              // d = 3: tri SoA [9][n_tri] ax ay az bx by bz cx cy cz, boxes [6] lo xyz, hi xyz
    // signed distances (pf_surface_prepare_signed; NULL until then)
    double* pts = nullptr;       // [n_points][3]
    int32_t* faces = nullptr;    // [n_faces][vpf]
    double* tnrm = nullptr;      // [n_tri][3] unit face normal of triangle (face * (vpf-2) + fan position)
    double* enrm = nullptr;      // [n_tri][3 edge slots][3] edge pseudonormal; slot j = edge (corner j, corner j+1)
    double* vnrm = nullptr;      // [n_points][3] angle-weighted vertex pseudonormal
    // winding numbers (pf_surface_prepare_winding; NULL until then)
    double* dip = nullptr;       // [n_chunks][8] dipole of a chunk: Nx Ny Nz | A | centroid xyz | radius
    double* sdip = nullptr;      // [n_super][8] the same per super-chunk
};

namespace {

// Ericson, Real-Time Collision Detection 5.1.5; same operation order as oracle/icp_port.py.  Returns the Voronoi region
// of the result: 0 1 2 = corner a b c, 3 = edge ab, 4 = edge bc, 5 = edge ca, 6 = interior (PF_REGION_*); only k_signed
// asks for it.
enum { PF_REGION_EDGE_AB = 3, PF_REGION_EDGE_BC = 4, PF_REGION_EDGE_CA = 5, PF_REGION_FACE = 6 };
__device__ __forceinline__ int closest_on_triangle(const double p[3], const double a[3], const double b[3], const double c[3],
                                                   double out[3]) {
    double ab[3], ac[3], ap[3], bp[3], cp[3];
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        ab[k] = b[k] - a[k];
        ac[k] = c[k] - a[k];
        ap[k] = p[k] - a[k];
        bp[k] = p[k] - b[k];
        cp[k] = p[k] - c[k];
    }
    const double d1 = dot3(ab, ap), d2 = dot3(ac, ap);
    if (d1 <= 0.0 && d2 <= 0.0) {
        out[0] = a[0], out[1] = a[1], out[2] = a[2];
        return 0;
    }
    const double d3 = dot3(ab, bp), d4 = dot3(ac, bp);
    if (d3 >= 0.0 && d4 <= d3) {
        out[0] = b[0], out[1] = b[1], out[2] = b[2];
        return 1;
    }
    const double vc = d1 * d4 - d3 * d2;
    if (vc <= 0.0 && d1 >= 0.0 && d3 <= 0.0) {
        const double v = d1 / (d1 - d3);
#pragma unroll
        for (int k = 0; k < 3; ++k) out[k] = a[k] + v * ab[k];
        return PF_REGION_EDGE_AB;
    }
    const double d5 = dot3(ab, cp), d6 = dot3(ac, cp);
    if (d6 >= 0.0 && d5 <= d6) {
        out[0] = c[0], out[1] = c[1], out[2] = c[2];
        return 2;
    }
    const double vb = d5 * d2 - d1 * d6;
    if (vb <= 0.0 && d2 >= 0.0 && d6 <= 0.0) {
        const double w = d2 / (d2 - d6);
#pragma unroll
        for (int k = 0; k < 3; ++k) out[k] = a[k] + w * ac[k];
        return PF_REGION_EDGE_CA;
    }
    const double va = d3 * d6 - d5 * d4;
    if (va <= 0.0 && (d4 - d3) >= 0.0 && (d5 - d6) >= 0.0) {
        const double w = (d4 - d3) / ((d4 - d3) + (d5 - d6));
#pragma unroll
        for (int k = 0; k < 3; ++k) out[k] = b[k] + w * (c[k] - b[k]);
        return PF_REGION_EDGE_BC;
    }
    const double denom = 1.0 / (va + vb + vc);
    const double v = vb * denom, w = vc * denom;
#pragma unroll
    for (int k = 0; k < 3; ++k) out[k] = (a[k] + ab[k] * v) + ac[k] * w;
    return PF_REGION_FACE;
}

struct Best {
    double d2;
    int32_t orig;  // triangle index (tie-break: lowest)
    double pt[3];
};

// One triangle per lane from each of NB chunks: all loads are issued before the arithmetic, so the NB memory
// latencies overlap (the kernel is latency-bound: few waves, dependent loads).  Slots past the end of the mesh or
// repeated chunk indices re-evaluate a triangle that is already accounted for, which changes nothing.
template <int NB>
__device__ __forceinline__ void scan_chunks(const double* __restrict__ tri, const int32_t* __restrict__ tri_orig, int64_t n_tri,
                                            const int64_t (&chunk)[NB], int lane, const double p[3], Best& best) {
    double v[NB][9];
    int32_t orig[NB];
#pragma unroll
    for (int b = 0; b < NB; ++b) {
        int64_t s = chunk[b] * PF_TRI_CHUNK + lane;
        s = s < n_tri ? s : n_tri - 1;
#pragma unroll
        for (int k = 0; k < 9; ++k) v[b][k] = tri[(int64_t)k * n_tri + s];
        orig[b] = tri_orig[s];
    }
#pragma unroll
    for (int b = 0; b < NB; ++b) {
        const double a[3] = {v[b][0], v[b][1], v[b][2]}, bb[3] = {v[b][3], v[b][4], v[b][5]}, cc[3] = {v[b][6], v[b][7], v[b][8]};
        double q[3];
        closest_on_triangle(p, a, bb, cc, q);
        const double dx = p[0] - q[0], dy = p[1] - q[1], dz = p[2] - q[2];
        const double d2 = dx * dx + dy * dy + dz * dz;
        if (better(d2, orig[b], best.d2, best.orig)) {  // NaN distances compare false: never win
            best.d2 = d2;
            best.orig = orig[b];
            best.pt[0] = q[0], best.pt[1] = q[1], best.pt[2] = q[2];
        }
    }
}

// one block of PF_CLOSEST_WAVES waves per query point (8 waves measured slower: 0.29 vs 0.25 ms per 1000 landmarks)
constexpr int PF_CLOSEST_WAVES = 4;

__global__ __launch_bounds__(PF_CLOSEST_WAVES* PF_WAVE) void k_closest(const double* __restrict__ tri, const int32_t* __restrict__ tri_orig,
                                                      const double* __restrict__ box, const double* __restrict__ sbox,
                                                      int64_t n_tri, int64_t n_chunks, int64_t n_super,
                                                      const double* __restrict__ qry, int64_t n_qry, int32_t per_face,
                                                      double* __restrict__ out_pt, int32_t* __restrict__ out_face,
                                                      double* __restrict__ out_d2) {
    constexpr int NW = PF_CLOSEST_WAVES;
    constexpr int NB = 4;  // chunks scanned per step of a wave
    __shared__ double w_d2[NW], w_pt[NW][3];
    __shared__ int32_t w_orig[NW];
    const int lane = threadIdx.x & (PF_WAVE - 1), wave = threadIdx.x >> 6;
    const int64_t qi = blockIdx.x;
    const double p[3] = {qry[3 * qi], qry[3 * qi + 1], qry[3 * qi + 2]};
    const double inf = std::numeric_limits<double>::infinity();

    // (1) the chunk nearest to the query - every wave, same result
    const int64_t c0 = nearest_chunk<3>([&](const double* __restrict__ bx) { return box_dist2<3>(p, bx); }, box, sbox, n_chunks, n_super, lane);
    Best best;
    best.d2 = inf, best.orig = 0x7fffffff, best.pt[0] = best.pt[1] = best.pt[2] = 0.0;
    if (c0 < n_chunks) {
        const int64_t one[1] = {c0};
        scan_chunks<1>(tri, tri_orig, n_tri, one, lane, p, best);
    }
    double bound = wave_min(best.d2);

    // (2) every chunk whose box is within the bound, super-chunk by super-chunk; of a super-chunk's surviving
    // chunks, wave w takes those at positions w, w+4, ... and scans NB of them per step
    static_assert(NW == 4, "the mask deals chunk positions to 4 waves");
    const unsigned long long mine = 0x1111111111111111ull << wave;
    for (int64_t sb = 0; sb < n_super; sb += PF_WAVE) {
        const int64_t s = sb + lane;
        unsigned long long smask = __ballot(s < n_super && box_dist2<3>(p, sbox + 6 * s) <= bound * PF_BOX_SLACK);
        while (smask) {
            const int64_t ss = sb + __ffsll((long long)smask) - 1;
            smask &= smask - 1;
            if (box_dist2<3>(p, sbox + 6 * ss) > bound * PF_BOX_SLACK) continue;  // the bound has shrunk since the ballot
            const int64_t c = ss * PF_WAVE + lane;
            unsigned long long mask = __ballot(c < n_chunks && c != c0 && box_dist2<3>(p, box + 6 * c) <= bound * PF_BOX_SLACK) & mine;
            while (mask) {
                int64_t batch[NB];
#pragma unroll
                for (int b = 0; b < NB; ++b) {
                    if (mask) {
                        batch[b] = ss * PF_WAVE + __ffsll((long long)mask) - 1;
                        mask &= mask - 1;
                    } else {
                        batch[b] = batch[0];
                    }
                }
                scan_chunks<NB>(tri, tri_orig, n_tri, batch, lane, p, best);
                bound = wave_min(best.d2);
                // drop the remaining chunks the tighter bound excludes (one box per lane, as in the ballot above)
                mask &= __ballot(c < n_chunks && box_dist2<3>(p, box + 6 * c) <= bound * PF_BOX_SLACK);
            }
        }
    }

    // winner of the wave, then of the block: smallest distance, lowest triangle index
    double wd = best.d2;
    int32_t wo = best.orig;
    for (int off = PF_WAVE / 2; off > 0; off >>= 1) {
        const double od = __shfl_xor(wd, off, PF_WAVE);
        const int32_t oo = __shfl_xor(wo, off, PF_WAVE);
        if (better(od, oo, wd, wo)) wd = od, wo = oo;
    }
    if (lane == 0) w_d2[wave] = wd, w_orig[wave] = wo;
    if (best.orig == wo && best.d2 == wd && wo != 0x7fffffff) {  // the lane(s) holding (wd, wo) hold the same point
        w_pt[wave][0] = best.pt[0], w_pt[wave][1] = best.pt[1], w_pt[wave][2] = best.pt[2];
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        int win = 0;
        for (int w = 1; w < NW; ++w)
            if (better(w_d2[w], w_orig[w], w_d2[win], w_orig[win])) win = w;
        if (w_orig[win] != 0x7fffffff) {
            out_pt[3 * qi] = w_pt[win][0], out_pt[3 * qi + 1] = w_pt[win][1], out_pt[3 * qi + 2] = w_pt[win][2];
            out_face[qi] = w_orig[win] / per_face;
            out_d2[qi] = w_d2[win];
        } else {  // NaN query or no finite triangle
            out_pt[3 * qi] = out_pt[3 * qi + 1] = out_pt[3 * qi + 2] = __longlong_as_double(0x7ff8000000000000ll);
            out_face[qi] = -1;
            out_d2[qi] = inf;
        }
    }
}

// ---- many-query distances (pf_surface_distance) ------------------------------------------------------------------
// Queries are Morton-sorted in their own bounding box and cut into packets of 16 consecutive ones (4 when there are
// fewer than 16 x 4096 queries), one packet per wave.  The wave walks the same super-chunk / chunk hierarchy as
// k_closest, but a chunk is loaded ONCE per packet: its 64 triangles are staged in LDS (one coalesced load per lane)
// and the lanes of each query share them out, reading from LDS by broadcast.  A triangle whose own box is farther than
// the query's bound is skipped before the exact test.  Every exact test is the one of k_closest (same
// closest_on_triangle / better, same PF_BOX_SLACK); pf_tri_hierarchy.h has the argument for the packet's tests.

// the larger distance wins; lowest query index on ties; idx < 0 = none
__device__ __forceinline__ bool later_max(double d2, int64_t idx, double bd2, int64_t bidx) {
    return idx >= 0 && (bidx < 0 || d2 > bd2 || (d2 == bd2 && idx < bidx));
}

constexpr int PF_DIST_STATS = 6;  // n_finite | n_nan | sum d | sum d^2 | max d | argmax

// one wave (= one block) per packet of PACKET sorted queries; lane = query (lane % PACKET) x triangle subset
// (lane / PACKET): each of a query's 64 / PACKET lanes tests every (64 / PACKET)-th triangle of a chunk.  Larger
// packets share each chunk load among more queries; smaller ones give more waves when there are few queries.
template <int PACKET>
__global__ __launch_bounds__(PF_WAVE) void k_distance(const double* __restrict__ tri, const int32_t* __restrict__ tri_orig,
                                                      const double* __restrict__ box, const double* __restrict__ sbox,
                                                      int64_t n_tri, int64_t n_chunks, int64_t n_super,
                                                      const double* __restrict__ qry, const int32_t* __restrict__ perm,
                                                      int64_t n_qry, int32_t per_face, double* __restrict__ out_d2,
                                                      int32_t* __restrict__ out_face, double* __restrict__ partial) {
    __shared__ double s_tri[9][PF_TRI_CHUNK];  // 4.5 KiB: one chunk, SoA as in HBM
    __shared__ int32_t s_orig[PF_TRI_CHUNK];
    constexpr int SUB = PF_WAVE / PACKET;  // lanes per query
    static_assert(PF_WAVE % PACKET == 0, "a packet divides the wave");
    const int lane = threadIdx.x, sub = lane / PACKET;
    const int64_t i = (int64_t)blockIdx.x * PACKET + (lane % PACKET);
    const bool live = i < n_qry;
    const int64_t qi = live ? perm[i] : -1;  // the caller's index of this lane's query
    const double inf = std::numeric_limits<double>::infinity();
    double p[3] = {0.0, 0.0, 0.0};
    if (live) p[0] = qry[3 * qi], p[1] = qry[3 * qi + 1], p[2] = qry[3 * qi + 2];
    const bool ok = live && std::isfinite(p[0]) && std::isfinite(p[1]) && std::isfinite(p[2]);

    Best best;
    best.d2 = inf, best.orig = 0x7fffffff;
    // the query's bound: the least distance its SUB lanes have found
    auto query_min = [&](double v) {
        for (int off = PACKET; off < PF_WAVE; off <<= 1) v = fmin(v, __shfl_xor(v, off, PF_WAVE));
        return v;
    };
    if (__ballot(ok)) {
        // the packet's box
        double lo[3], hi[3];
#pragma unroll
        for (int a = 0; a < 3; ++a) {
            lo[a] = ok ? p[a] : inf, hi[a] = ok ? p[a] : -inf;
            for (int off = PF_WAVE / 2; off > 0; off >>= 1) {
                lo[a] = fmin(lo[a], __shfl_xor(lo[a], off, PF_WAVE));
                hi[a] = fmax(hi[a], __shfl_xor(hi[a], off, PF_WAVE));
            }
        }
        double qbest = inf;
        auto scan = [&](int64_t c) {  // stage chunk c in LDS, test its triangles against every query
            const int64_t s = c * PF_TRI_CHUNK + lane;
            const int cnt = (int)(n_tri - c * PF_TRI_CHUNK < PF_TRI_CHUNK ? n_tri - c * PF_TRI_CHUNK : PF_TRI_CHUNK);
            __syncthreads();  // the previous chunk's reads are done
            if (lane < cnt) {
#pragma unroll
                for (int k = 0; k < 9; ++k) s_tri[k][lane] = tri[(int64_t)k * n_tri + s];
                s_orig[lane] = tri_orig[s];
            }
            __syncthreads();
            if (ok) {
                for (int t = sub; t < cnt; t += SUB) {
                    const double a[3] = {s_tri[0][t], s_tri[1][t], s_tri[2][t]}, b[3] = {s_tri[3][t], s_tri[4][t], s_tri[5][t]},
                                 cc[3] = {s_tri[6][t], s_tri[7][t], s_tri[8][t]};
                    // the triangle's own box first: it is never farther than the triangle (the chunk-box argument)
                    double tb = 0.0;
#pragma unroll
                    for (int k = 0; k < 3; ++k) {
                        const double d = fmax(fmax(fmin(fmin(a[k], b[k]), cc[k]) - p[k], p[k] - fmax(fmax(a[k], b[k]), cc[k])), 0.0);
                        tb += d * d;
                    }
                    if (tb > fmin(best.d2, qbest) * PF_BOX_SLACK) continue;
                    double q[3];
                    closest_on_triangle(p, a, b, cc, q);
                    const double dx = p[0] - q[0], dy = p[1] - q[1], dz = p[2] - q[2];
                    const double d2 = dx * dx + dy * dy + dz * dz;
                    const int32_t o = s_orig[t];
                    if (better(d2, o, best.d2, best.orig)) best.d2 = d2, best.orig = o;  // NaN distances never win
                }
            }
            qbest = query_min(best.d2);
        };
        // does any query's own point-box test (k_closest's) keep chunk c?
        auto wanted = [&](int64_t c) { return __ballot(ok && box_dist2<3>(p, box + 6 * c) <= qbest * PF_BOX_SLACK) != 0; };

        // (1) seed: the chunk nearest to the packet's centre
        const double ctr[3] = {0.5 * (lo[0] + hi[0]), 0.5 * (lo[1] + hi[1]), 0.5 * (lo[2] + hi[2])};
        const int64_t c0 = nearest_chunk<3>([&](const double* __restrict__ bx) { return box_dist2<3>(ctr, bx); }, box, sbox, n_chunks,
                                            n_super, lane);
        if (c0 < n_chunks) scan(c0);
        double bound = wave_max(ok ? qbest : -inf);  // the packet's bound: its worst query

        // (2) every chunk whose box is within the bound of the packet's box and of some query
        for (int64_t sb = 0; sb < n_super; sb += PF_WAVE) {
            const int64_t s = sb + lane;
            unsigned long long smask = __ballot(s < n_super && boxbox_dist2<3>(lo, hi, sbox + 6 * s) <= bound * PF_BOX_SLACK);
            while (smask) {
                const int64_t ss = sb + __ffsll((long long)smask) - 1;
                smask &= smask - 1;
                if (boxbox_dist2<3>(lo, hi, sbox + 6 * ss) > bound * PF_BOX_SLACK) continue;  // the bound has shrunk
                const int64_t c = ss * PF_WAVE + lane;
                unsigned long long mask = __ballot(c < n_chunks && c != c0 && boxbox_dist2<3>(lo, hi, box + 6 * c) <= bound * PF_BOX_SLACK);
                while (mask) {
                    const int64_t cc = ss * PF_WAVE + __ffsll((long long)mask) - 1;
                    mask &= mask - 1;
                    if (boxbox_dist2<3>(lo, hi, box + 6 * cc) > bound * PF_BOX_SLACK || !wanted(cc)) continue;
                    scan(cc);
                    bound = wave_max(ok ? qbest : -inf);
                }
            }
        }
    }

    // the query's winner over its lanes (smallest distance, lowest triangle index), outputs in the caller's order
    for (int off = PACKET; off < PF_WAVE; off <<= 1) {
        const double od = __shfl_xor(best.d2, off, PF_WAVE);
        const int32_t oo = __shfl_xor(best.orig, off, PF_WAVE);
        if (better(od, oo, best.d2, best.orig)) best.d2 = od, best.orig = oo;
    }
    const bool found = ok && best.orig != 0x7fffffff;
    const double d2 = found ? best.d2 : (ok ? inf : __longlong_as_double(0x7ff8000000000000ll));
    const bool mine = live && sub == 0;  // one lane per query writes and counts
    if (mine) {
        if (out_d2) out_d2[qi] = d2;
        if (out_face) out_face[qi] = found ? best.orig / per_face : -1;
    }
    // the packet's partial statistics
    const bool fin = mine && std::isfinite(d2);
    const double d = fin ? sqrt(d2) : 0.0;
    double md2 = fin ? d2 : -inf;
    int64_t mi = fin ? qi : -1;
    for (int off = PF_WAVE / 2; off > 0; off >>= 1) {
        const double od = __shfl_xor(md2, off, PF_WAVE);
        const int64_t oi = __shfl_xor(mi, off, PF_WAVE);
        if (later_max(od, oi, md2, mi)) md2 = od, mi = oi;
    }
    const double n_fin = wave_sum(fin ? 1.0 : 0.0), n_bad = wave_sum(mine && !fin ? 1.0 : 0.0);
    const double sd = wave_sum(d), sdd = wave_sum(d * d);
    if (lane == 0) {
        double* w = partial + (int64_t)PF_DIST_STATS * blockIdx.x;
        w[0] = n_fin, w[1] = n_bad, w[2] = sd, w[3] = sdd, w[4] = md2, w[5] = (double)mi;
    }
}

// one block: the packets' partials in a fixed order (strided sequential sums per thread, then a fixed tree)
__global__ __launch_bounds__(PF_BLOCK) void k_distance_stats(const double* __restrict__ partial, int64_t n_part,
                                                             double* __restrict__ stats) {
    __shared__ double s_v[4][PF_BLOCK];
    __shared__ double s_m[PF_BLOCK];
    __shared__ int64_t s_i[PF_BLOCK];
    const int t = threadIdx.x;
    double v[4] = {0.0, 0.0, 0.0, 0.0}, m = -std::numeric_limits<double>::infinity();
    int64_t mi = -1;
    for (int64_t w = t; w < n_part; w += PF_BLOCK) {
        const double* x = partial + (int64_t)PF_DIST_STATS * w;
#pragma unroll
        for (int k = 0; k < 4; ++k) v[k] += x[k];
        const int64_t xi = (int64_t)x[5];
        if (later_max(x[4], xi, m, mi)) m = x[4], mi = xi;
    }
#pragma unroll
    for (int k = 0; k < 4; ++k) s_v[k][t] = v[k];
    s_m[t] = m, s_i[t] = mi;
    __syncthreads();
    for (int h = PF_BLOCK / 2; h > 0; h >>= 1) {
        if (t < h) {
#pragma unroll
            for (int k = 0; k < 4; ++k) s_v[k][t] += s_v[k][t + h];
            if (later_max(s_m[t + h], s_i[t + h], s_m[t], s_i[t])) s_m[t] = s_m[t + h], s_i[t] = s_i[t + h];
        }
        __syncthreads();
    }
    if (t == 0) {
#pragma unroll
        for (int k = 0; k < 4; ++k) stats[k] = s_v[k][0];
        stats[4] = s_i[0] >= 0 ? sqrt(s_m[0]) : __longlong_as_double(0x7ff8000000000000ll);
        stats[5] = (double)s_i[0];
    }
}

// ---- signed distances (pf_surface_prepare_signed, pf_surface_signed_distance) -----------------------------------
// Angle-weighted pseudonormals (Baerentzen & Aanaes 2005) of the fan triangles: the sign of (p - c) . n over the
// feature (interior, edge, corner) of the winning triangle that the closest point c lies on is the exact inside /
// outside sign on a closed, consistently oriented mesh.  Fan diagonals are edges like any other.  Every sum runs in a
// fixed order (triangle order for an edge, sorted (vertex, half-edge) order for a vertex): no floating-point atomics.
// The half-edge pass itself - the triangle pass, the run walks, the edge counts - is pf_halfedge.h's.

// one thread per fan triangle: he_triangle, without the area
__global__ __launch_bounds__(PF_BLOCK) void k_tri_normals(const double* __restrict__ pts, const int32_t* __restrict__ faces,
                                                          int32_t vpf, int64_t n_tri, int nb, double* __restrict__ tnrm,
                                                          double* __restrict__ tang, unsigned long long* __restrict__ ekey,
                                                          unsigned* __restrict__ vkey, int32_t* __restrict__ hval) {
    const int64_t t = (int64_t)blockIdx.x * PF_BLOCK + threadIdx.x;
    if (t >= n_tri) return;
    int32_t v[3];
    tri_corners(faces, vpf, t, v);
    he_triangle(pts, v, t, nb, tnrm, tang, nullptr, ekey, vkey, hval);
}

// one thread per edge (the first half-edge of each run of equal keys; runs are in triangle order, the sort being
// stable): the sum of its triangles' normals, stored for each of its half-edges; counts: he_count_edge
__global__ __launch_bounds__(PF_BLOCK) void k_edge_normals(const unsigned long long* __restrict__ ekey, const int32_t* __restrict__ hedge,
                                                           int64_t n_half, const int32_t* __restrict__ faces, int32_t vpf,
                                                           const double* __restrict__ tnrm, double* __restrict__ enrm,
                                                           unsigned long long* __restrict__ counts) {
    const int64_t i = (int64_t)blockIdx.x * PF_BLOCK + threadIdx.x;
    const int64_t end = he_run_end(ekey, n_half, i);
    if (end == i) return;
    double s[3] = {0.0, 0.0, 0.0};
    for (int64_t k = i; k < end; ++k) {
        const int64_t t = hedge[k] / 3;
#pragma unroll
        for (int a = 0; a < 3; ++a) s[a] += tnrm[3 * t + a];
    }
    for (int64_t k = i; k < end; ++k)
#pragma unroll
        for (int a = 0; a < 3; ++a) enrm[3 * (int64_t)hedge[k] + a] = s[a];
    const int64_t m = end - i;
    bool fwd[2] = {false, false};
    for (int k = 0; m == 2 && k < 2; ++k) {
        const int32_t h = hedge[i + k];
        int32_t v[3];
        tri_corners(faces, vpf, h / 3, v);
        const int j = h % 3;
        fwd[k] = v[j] < v[he_next(j)];
    }
    he_count_edge(counts, m, fwd[0], fwd[1]);
}

// one thread per vertex: sum of corner angle x unit normal over its corners, in sorted (vertex, half-edge) order
__global__ __launch_bounds__(PF_BLOCK) void k_vertex_normals(const unsigned* __restrict__ vkey, const int32_t* __restrict__ hedge,
                                                             int64_t n_half, int64_t n_points, const double* __restrict__ tnrm,
                                                             const double* __restrict__ tang, double* __restrict__ vnrm) {
    const int64_t v = (int64_t)blockIdx.x * PF_BLOCK + threadIdx.x;
    if (v >= n_points) return;
    double s[3] = {0.0, 0.0, 0.0};
    for (int64_t lo = he_vertex_run(vkey, n_half, v); lo < n_half && vkey[lo] == (unsigned)v; ++lo) {
        const int32_t h = hedge[lo];
        const double ang = tang[h];
#pragma unroll
        for (int a = 0; a < 3; ++a) s[a] += ang * tnrm[3 * (int64_t)(h / 3) + a];
    }
#pragma unroll
    for (int a = 0; a < 3; ++a) vnrm[3 * v + a] = s[a];
}

// one thread per query, after k_distance: the fan triangles of the winning face are evaluated again with the same
// arithmetic and tie rule, which gives the search's winner, its closest point and its region; the sign is that of
// (p - c) . pseudonormal of the region's feature, the magnitude sqrt of the search's own d2
__global__ __launch_bounds__(PF_BLOCK) void k_signed(const double* __restrict__ pts, const int32_t* __restrict__ faces, int32_t vpf,
                                                     const double* __restrict__ tnrm, const double* __restrict__ enrm,
                                                     const double* __restrict__ vnrm, const double* __restrict__ qry, int64_t n_qry,
                                                     const double* __restrict__ d2s, const int32_t* __restrict__ face,
                                                     double* __restrict__ out_sd, int32_t* __restrict__ out_feature,
                                                     unsigned long long* __restrict__ n_ambiguous) {
    const int64_t i = (int64_t)blockIdx.x * PF_BLOCK + threadIdx.x;
    if (i >= n_qry) return;
    const double p[3] = {qry[3 * i], qry[3 * i + 1], qry[3 * i + 2]};
    const double d2 = d2s[i];
    const int32_t f = face[i];
    if (f < 0) {  // a non-finite query (NaN) or no finite triangle (+inf)
        out_sd[i] = sqrt(d2);
        out_feature[i] = -1;
        return;
    }
    const int32_t per = vpf - 2;
    double bd2 = std::numeric_limits<double>::infinity(), bq[3] = {0.0, 0.0, 0.0};
    int32_t bt = 0x7fffffff, bv[3] = {0, 0, 0};
    int breg = PF_REGION_FACE;
    for (int32_t j = 0; j < per; ++j) {
        const int32_t t = f * per + j;
        int32_t v[3];
        tri_corners(faces, vpf, t, v);
        const double a[3] = {pts[3 * (int64_t)v[0]], pts[3 * (int64_t)v[0] + 1], pts[3 * (int64_t)v[0] + 2]};
        const double b[3] = {pts[3 * (int64_t)v[1]], pts[3 * (int64_t)v[1] + 1], pts[3 * (int64_t)v[1] + 2]};
        const double c[3] = {pts[3 * (int64_t)v[2]], pts[3 * (int64_t)v[2] + 1], pts[3 * (int64_t)v[2] + 2]};
        double q[3];
        const int reg = closest_on_triangle(p, a, b, c, q);
        const double dx = p[0] - q[0], dy = p[1] - q[1], dz = p[2] - q[2];
        const double e2 = dx * dx + dy * dy + dz * dz;
        if (better(e2, t, bd2, bt)) {
            bd2 = e2, bt = t, breg = reg;
            bq[0] = q[0], bq[1] = q[1], bq[2] = q[2];
            bv[0] = v[0], bv[1] = v[1], bv[2] = v[2];
        }
    }
    double n[3] = {0.0, 0.0, 0.0};
    int feature = 0;
    if (bt != 0x7fffffff) {
        const double* src;
        if (breg == PF_REGION_FACE) {
            src = tnrm + 3 * (int64_t)bt;
        } else if (breg >= PF_REGION_EDGE_AB) {
            src = enrm + 9 * (int64_t)bt + 3 * (breg - PF_REGION_EDGE_AB);
            feature = 1;
        } else {
            src = vnrm + 3 * (int64_t)bv[breg];
            feature = 2;
        }
        n[0] = src[0], n[1] = src[1], n[2] = src[2];
    }
    const double s = (p[0] - bq[0]) * n[0] + (p[1] - bq[1]) * n[1] + (p[2] - bq[2]) * n[2];
    const double d = sqrt(d2);
    double sd = d;
    if (d2 == 0.0) sd = 0.0;
    else if (s < 0.0) sd = -d;
    else if (!(s > 0.0)) atomicAdd(n_ambiguous, 1ull);  // zero (or NaN) pseudonormal component: + and counted
    out_sd[i] = sd;
    out_feature[i] = feature;
}

// ---- generalized winding numbers (pf_surface_prepare_winding, pf_surface_winding) -------------------------------
// w(q) = (1 / 4 pi) sum_t Omega_t(q), the signed solid angles of all triangles seen from q (Jacobson et al. 2013): 1
// inside and 0 outside a closed outward-oriented mesh, smooth across holes, no normals, edges or manifoldness needed.
// Nothing can be culled: every triangle contributes to every query.
//   prepare  per chunk and per super-chunk the dipole data of its triangles: N = sum 1/2 (b - a) x (c - a), A = sum
//            area, the area-weighted centroid (the box centre if A = 0), r = max |corner - centroid|.
//   query    queries Morton-sorted (k_qry_keys), ONE WAVE PER PACKET of PF_WIND_PACKET neighbouring queries.  A
//            chunk's 64 triangles are loaded once per packet, one triangle per lane; the lane evaluates its triangle
//            against each query of the packet (coordinates broadcast through scalar registers) and adds the term to
//            that query's accumulator in its own registers; one butterfly per query at the very end.  One atan2 per
//            (triangle, query).  f64 throughout.
//   beta > 1 Barill et al. 2018, two levels: a super-chunk, then a chunk, whose centroid is at d >= beta r from EVERY
//            finite query of the packet contributes N . (p - q) / (4 pi d^3) and the bound A r / (2 pi (d - r)^3) on
//            what that drops (derived in DESIGN.md 5); otherwise it is opened for the whole packet (lane = chunk, then lane =
//            triangle).  Opening more than a single query would need only makes that query more exact.
// Reproducible: run to run, bit for bit (a lane adds its terms in chunk order, the butterfly is fixed, no atomics; the
// packet a query falls in depends only on the query set).  Not against numpy: summation order, FMA contraction and the
// device's atan2 / sqrt differ from libm, so the tests compare with a derived tolerance, not bit for bit.

constexpr int PF_WIND_PACKET = 8;  // queries per wave: 8 accumulators (+ 8 bounds) per lane, the term unrolled 8 times
constexpr int PF_DIPOLE = 8;       // Nx Ny Nz | A | px py pz | r

__device__ __forceinline__ double lane_bcast(double v, int l) {  // l uniform: the value lands in scalar registers
    return __hiloint2double(__builtin_amdgcn_readlane(__double2hiint(v), l), __builtin_amdgcn_readlane(__double2loint(v), l));
}

// half the signed solid angle of triangle (a, b, c), corners relative to the query (Van Oosterom & Strackee 1983);
// positive where the normal (b - a) x (c - a) points away from the query; 0 with a corner at the query
__device__ __forceinline__ double half_solid_angle(const double a[3], const double b[3], const double c[3]) {
#pragma clang fp contract(fast)
    const double la = sqrt(a[0] * a[0] + a[1] * a[1] + a[2] * a[2]);
    const double lb = sqrt(b[0] * b[0] + b[1] * b[1] + b[2] * b[2]);
    const double lc = sqrt(c[0] * c[0] + c[1] * c[1] + c[2] * c[2]);
    const double det = a[0] * (b[1] * c[2] - b[2] * c[1]) + a[1] * (b[2] * c[0] - b[0] * c[2]) + a[2] * (b[0] * c[1] - b[1] * c[0]);
    const double ab = a[0] * b[0] + a[1] * b[1] + a[2] * b[2];
    const double bc = b[0] * c[0] + b[1] * c[1] + b[2] * c[2];
    const double ca = c[0] * a[0] + c[1] * a[1] + c[2] * a[2];
    const double den = la * lb * lc + ab * lc + bc * la + ca * lb;
    return (la == 0.0 || lb == 0.0 || lc == 0.0) ? 0.0 : atan2(det, den);
}

// one wave per chunk, one triangle per lane; sums by the fixed butterfly
__global__ __launch_bounds__(PF_WAVE) void k_chunk_dipoles(const double* __restrict__ tri, int64_t n_tri, const double* __restrict__ box,
                                                           double* __restrict__ dip) {
    const int64_t c = blockIdx.x;
    const int lane = threadIdx.x;
    const int64_t s = c * PF_TRI_CHUNK + lane;
    const bool have = s < n_tri;
    double x[9];
#pragma unroll
    for (int k = 0; k < 9; ++k) x[k] = have ? tri[(int64_t)k * n_tri + s] : 0.0;
    const double u[3] = {x[3] - x[0], x[4] - x[1], x[5] - x[2]}, v[3] = {x[6] - x[0], x[7] - x[1], x[8] - x[2]};
    const double n[3] = {0.5 * (u[1] * v[2] - u[2] * v[1]), 0.5 * (u[2] * v[0] - u[0] * v[2]), 0.5 * (u[0] * v[1] - u[1] * v[0])};
    const double area = sqrt(dot3(n, n));
    const double N[3] = {wave_sum(n[0]), wave_sum(n[1]), wave_sum(n[2])};
    const double A = wave_sum(area);
    double p[3];
#pragma unroll
    for (int a = 0; a < 3; ++a) {
        const double m = wave_sum(area * ((x[a] + x[3 + a] + x[6 + a]) / 3.0));
        p[a] = A > 0.0 ? m / A : 0.5 * (box[6 * c + a] + box[6 * c + 3 + a]);
    }
    double r2 = 0.0;
    if (have) {
#pragma unroll
        for (int k = 0; k < 3; ++k) {
            const double d[3] = {x[3 * k] - p[0], x[3 * k + 1] - p[1], x[3 * k + 2] - p[2]};
            r2 = fmax(r2, dot3(d, d));
        }
    }
    r2 = wave_max(r2);
    if (lane == 0) {
        double* o = dip + PF_DIPOLE * c;
        o[0] = N[0], o[1] = N[1], o[2] = N[2], o[3] = A, o[4] = p[0], o[5] = p[1], o[6] = p[2], o[7] = sqrt(r2);
    }
}

// one wave per super-chunk: its chunks' sums, one chunk per lane, then the radius over all its triangles' corners
__global__ __launch_bounds__(PF_WAVE) void k_super_dipoles(const double* __restrict__ tri, int64_t n_tri, const double* __restrict__ dip,
                                                           int64_t n_chunks, const double* __restrict__ sbox, double* __restrict__ sdip) {
    const int64_t ss = blockIdx.x;
    const int lane = threadIdx.x;
    const int64_t c = ss * PF_WAVE + lane;
    const bool have = c < n_chunks;
    double d[PF_DIPOLE];
#pragma unroll
    for (int k = 0; k < PF_DIPOLE; ++k) d[k] = have ? dip[PF_DIPOLE * c + k] : 0.0;
    const double N[3] = {wave_sum(d[0]), wave_sum(d[1]), wave_sum(d[2])};
    const double A = wave_sum(d[3]);
    double p[3];
#pragma unroll
    for (int a = 0; a < 3; ++a) {
        const double m = wave_sum(d[3] * d[4 + a]);
        p[a] = A > 0.0 ? m / A : 0.5 * (sbox[6 * ss + a] + sbox[6 * ss + 3 + a]);
    }
    double r2 = 0.0;
    const int64_t end = (ss + 1) * PF_WAVE * PF_TRI_CHUNK < n_tri ? (ss + 1) * PF_WAVE * PF_TRI_CHUNK : n_tri;
    for (int64_t s = ss * PF_WAVE * PF_TRI_CHUNK + lane; s < end; s += PF_WAVE) {
#pragma unroll
        for (int k = 0; k < 3; ++k) {
            const double e[3] = {tri[(int64_t)(3 * k) * n_tri + s] - p[0], tri[(int64_t)(3 * k + 1) * n_tri + s] - p[1],
                                 tri[(int64_t)(3 * k + 2) * n_tri + s] - p[2]};
            r2 = fmax(r2, dot3(e, e));
        }
    }
    r2 = wave_max(r2);
    if (lane == 0) {
        double* o = sdip + PF_DIPOLE * ss;
        o[0] = N[0], o[1] = N[1], o[2] = N[2], o[3] = A, o[4] = p[0], o[5] = p[1], o[6] = p[2], o[7] = sqrt(r2);
    }
}

// one wave (= one block) per packet of PF_WIND_PACKET sorted queries.  acc[j] holds this lane's share of sum Omega / 2 of
// query j, bnd[j] of its bound; HIER = false never touches the dipoles and leaves the bound 0.
template <bool HIER>
__global__ __launch_bounds__(PF_WAVE) void k_winding(const double* __restrict__ tri, int64_t n_tri, int64_t n_chunks, int64_t n_super,
                                                     const double* __restrict__ dip, const double* __restrict__ sdip,
                                                     const double* __restrict__ qry, const int32_t* __restrict__ perm, int64_t n_qry,
                                                     double beta, double* __restrict__ out_w, double* __restrict__ out_bound) {
#pragma clang fp contract(fast)
    constexpr int P = PF_WIND_PACKET;
    const int lane = threadIdx.x;
    const int64_t i = (int64_t)blockIdx.x * P + lane;
    const bool live = lane < P && i < n_qry;
    const int64_t qi = live ? perm[i] : -1;  // the caller's index of this lane's query
    double p[3] = {0.0, 0.0, 0.0};
    if (live) p[0] = qry[3 * qi], p[1] = qry[3 * qi + 1], p[2] = qry[3 * qi + 2];
    const bool ok = live && std::isfinite(p[0]) && std::isfinite(p[1]) && std::isfinite(p[2]);
    if (!ok) p[0] = p[1] = p[2] = 0.0;  // a dead slot computes on the origin and is never written
    const unsigned long long okmask = __ballot(ok);
    double q[P][3], acc[P], bnd[P];
#pragma unroll
    for (int j = 0; j < P; ++j) {
        q[j][0] = lane_bcast(p[0], j), q[j][1] = lane_bcast(p[1], j), q[j][2] = lane_bcast(p[2], j);
        acc[j] = 0.0, bnd[j] = 0.0;
    }

    auto scan = [&](int64_t c) {  // chunk c: one triangle per lane against every query of the packet
        const int64_t s = c * PF_TRI_CHUNK + lane;
        const bool have = s < n_tri;
        const int64_t sc = have ? s : n_tri - 1;
        double x[9];
#pragma unroll
        for (int k = 0; k < 9; ++k) x[k] = tri[(int64_t)k * n_tri + sc];
#pragma unroll
        for (int j = 0; j < P; ++j) {
            const double a[3] = {x[0] - q[j][0], x[1] - q[j][1], x[2] - q[j][2]};
            const double b[3] = {x[3] - q[j][0], x[4] - q[j][1], x[5] - q[j][2]};
            const double cc[3] = {x[6] - q[j][0], x[7] - q[j][1], x[8] - q[j][2]};
            const double h = half_solid_angle(a, b, cc);
            acc[j] += have ? h : 0.0;
        }
    };
    // cluster data d of this lane (if have): is it far from every finite query of the packet?  If so its dipole term
    // and bound are added for each query.  Returns whether the lane's cluster has to be opened.
    auto cluster = [&](bool have, const double* __restrict__ d) {
        double v[PF_DIPOLE];
#pragma unroll
        for (int k = 0; k < PF_DIPOLE; ++k) v[k] = have ? d[k] : 0.0;
        const double br = beta * v[7];
        bool far = have;
#pragma unroll
        for (int j = 0; j < P; ++j) {
            const double e[3] = {v[4] - q[j][0], v[5] - q[j][1], v[6] - q[j][2]};
            const double d2 = e[0] * e[0] + e[1] * e[1] + e[2] * e[2];
            far = far && (!((okmask >> j) & 1ull) || (d2 >= br * br && d2 > 0.0));
        }
        if (far) {
#pragma unroll
            for (int j = 0; j < P; ++j) {
                const double e[3] = {v[4] - q[j][0], v[5] - q[j][1], v[6] - q[j][2]};
                const double d2 = e[0] * e[0] + e[1] * e[1] + e[2] * e[2];
                const double dd = sqrt(d2), gap = dd - v[7];
                acc[j] += 0.5 * (v[0] * e[0] + v[1] * e[1] + v[2] * e[2]) / (d2 * dd);
                bnd[j] += v[3] * v[7] / (6.283185307179586 * (gap * gap * gap));
            }
        }
        return have && !far;
    };

    if (HIER) {
        for (int64_t sb = 0; sb < n_super; sb += PF_WAVE) {
            const int64_t s = sb + lane;
            unsigned long long smask = __ballot(cluster(s < n_super, sdip + PF_DIPOLE * (s < n_super ? s : 0)));
            while (smask) {
                const int64_t ss = sb + __ffsll((long long)smask) - 1;
                smask &= smask - 1;
                const int64_t c = ss * PF_WAVE + lane;
                unsigned long long mask = __ballot(cluster(c < n_chunks, dip + PF_DIPOLE * (c < n_chunks ? c : 0)));
                while (mask) {
                    scan(ss * PF_WAVE + __ffsll((long long)mask) - 1);
                    mask &= mask - 1;
                }
            }
        }
    } else {
        for (int64_t c = 0; c < n_chunks; ++c) scan(c);
    }

    double w = 0.0, b = 0.0;
#pragma unroll
    for (int j = 0; j < P; ++j) {
        const double sw = wave_sum(acc[j]), sb = HIER ? wave_sum(bnd[j]) : 0.0;
        if (lane == j) w = sw / 6.283185307179586, b = sb;
    }
    if (live) {
        const double nan = __longlong_as_double(0x7ff8000000000000ll);
        if (out_w) out_w[qi] = ok ? w : nan;
        if (out_bound) out_bound[qi] = ok ? b : nan;
    }
}

// ---- ray casting (pf_surface_raycast) -----------------------------------------------------------------------------
// For every ray o + t d: the least t in [t_min, t_max] at which it meets a fan triangle (ties: lowest triangle index),
// that triangle's face and barycentric (u, v), and the number of triangles it meets in the interval.  d is not
// normalised: t is in units of |d|.
//
// The exact test, ray_triangle, is Moeller-Trumbore in FP64, ONE body that every decision goes through, written out
// operation by operation (no FMA: -ffp-contract=off; true divisions by det) so that a numpy restatement rounds the same:
//   e1 = b - a, e2 = c - a, p = d x e2, det = e1 . p, tv = o - a, u = (tv . p) / det, q = tv x e1, v = (d . q) / det,
//   t = (e2 . q) / det;  accepted when det != 0, u >= 0, v >= 0, u + v <= 1, t_min <= t <= t_max (both inclusive) and
//   facing allows the side: 0 any, +1 only det > 0 (the ray meets the side the face normal points to), -1 only det < 0.
// A NaN anywhere fails a comparison, so a NaN triangle never passes; a zero-area triangle has det = 0 in exact
// arithmetic.  NOT watertight: a ray exactly through an edge or a vertex may be accepted by both neighbours or by
// neither (u, v and u + v are rounded per triangle), and that is left as it is: the result is defined as what this
// test says over ALL triangles, the same as a brute-force loop.
//
// Traversal.  Rays are Morton-sorted by origin in the box of the finite origins; one wave per packet of 16 neighbouring
// rays (4 when there are fewer than 16 x 4096 rays: the same rule and reason as k_distance, small sets still fill the
// GPU).  Lane = ray (lane % PACKET) x triangle subset (lane / PACKET).  The packet's rays sit in LDS (origin,
// direction and the ray's current upper end t_hi), so that in a box ballot lane = box and every lane runs through the
// packet's rays by broadcast.  One ballot over the super-chunk boxes, per surviving super-chunk one over its 64 chunk
// boxes; at both levels the survivors are taken nearest first (least entry parameter over the packet) so that t_hi
// shrinks early, and the rest of a level is dropped once its least entry parameter exceeds every ray's t_hi.  A chunk
// some ray still wants is staged in LDS once per packet, as in k_distance, and each ray's lanes share its triangles out.
// COUNT = true (out_count requested) never shrinks t_hi below t_max: every chunk is scanned at most once per packet
// and every triangle of it tested by exactly one lane of each ray that wants the chunk, so the count is exact, and the
// same launch still yields the first hit.
//
// Pruning never changes a result: ray_box keeps every box that holds a triangle which ray_triangle accepts for that
// ray with t in [t_lo, t_hi].  The accepted t, u, v are rounded values, so the point o + t d may lie outside the
// triangle, hence outside its box, by a rounding error; the slab test therefore runs on the box widened on every side by
//   w = PF_RAY_SLACK * m,  m = max over the axes of max(|lo - o|, |hi - o|)   (the box's farthest face from the origin).
// Argument.  Let x = (u, v, t) be the accepted values, sigma = |det| / (|d| |e1| |e2|) (the sine of the triangle's angle
// at a times the cosine between the ray and the normal), and L = |e1| + |e2| + |tv| + |t||d|.  Each of the four triple
// products is computed with an error of at most 10 eps times the product of the lengths of its three vectors (two
// roundings per cross-product component, three per dot, one per difference of the inputs).  x solves [e1 e2 -d] x = tv
// by Cramer's rule, and from x_i = N_i / det with those errors, |u|, |v| <= 1 and the division's own rounding, the
// residual r = (o + t d) - (a + u e1 + v e2) obeys |r| <= 64 eps L / sigma.  a + u e1 + v e2 is a point of the triangle
// (u, v >= 0, u + v <= 1 + eps), so o + t d lies within 64 eps L / sigma + eps L of the chunk's box.  No corner of that box
// is farther from o than sqrt(3) m: |tv| and |t||d| - |r| are at most that, |e1| and |e2| at most twice that, so
// L <= 11 m and |r| <= 704 eps m / sigma.  The slab arithmetic itself ((lo - o) - w, then one division per face; min, max and
// the comparison are exact) moves a bound by at most 4 eps m.  With PF_RAY_SLACK = 2^-20 the widened, rounded slabs
// contain o + t d on every axis, so their intersection with [t_lo, t_hi] contains t and the box is kept, whenever
//   704 eps / sigma + 5 eps <= 2^-20,  i.e.  sigma >= 8.2e-8:
// every triangle-ray pair except a ray within 1e-7 rad of the triangle's plane or a needle with an angle below that.
// No box test can do without such a condition: for a ray IN the plane of a triangle all four triple products are pure
// rounding noise and the exact test may accept at any distance from the triangle.  (Overflow and underflow aside.)
// An axis with d = +0.0 or -0.0 has no slab parameters (0 * inf): there the origin is tested against the widened slab.
// A reciprocal of d is not used: it overflows for a subnormal d and turns a zero numerator into NaN.  NaN (an empty
// box of NaN triangles, an infinite corner) is ignored by fmin / fmax and by the outside test, which keeps the box.
//
// gfx950, -Rpass-analysis=kernel-resource-usage: 16-ray packets 94 VGPRs (96 with COUNT), 5 waves per SIMD, 5760 bytes
// of LDS; 4-ray packets 100 (102) VGPRs, 4 waves per SIMD, 5088 bytes; no scratch, no spill in any of the four.

constexpr double PF_RAY_SLACK = 1.0 / 1048576.0;  // 2^-20: see the argument above

// Moeller-Trumbore, operation for operation as in tests/_ray_ref.py.  t, u, v are set when it returns true.
__device__ __forceinline__ bool ray_triangle(const double o[3], const double d[3], const double a[3], const double b[3],
                                             const double c[3], double t_min, double t_max, int32_t facing, double& t, double& u,
                                             double& v) {
    const double e1[3] = {b[0] - a[0], b[1] - a[1], b[2] - a[2]};
    const double e2[3] = {c[0] - a[0], c[1] - a[1], c[2] - a[2]};
    const double p[3] = {d[1] * e2[2] - d[2] * e2[1], d[2] * e2[0] - d[0] * e2[2], d[0] * e2[1] - d[1] * e2[0]};
    const double det = e1[0] * p[0] + e1[1] * p[1] + e1[2] * p[2];
    if (det == 0.0 || (facing > 0 && !(det > 0.0)) || (facing < 0 && !(det < 0.0))) return false;
    const double tv[3] = {o[0] - a[0], o[1] - a[1], o[2] - a[2]};
    u = (tv[0] * p[0] + tv[1] * p[1] + tv[2] * p[2]) / det;
    if (!(u >= 0.0)) return false;  // also a NaN det
    const double q[3] = {tv[1] * e1[2] - tv[2] * e1[1], tv[2] * e1[0] - tv[0] * e1[2], tv[0] * e1[1] - tv[1] * e1[0]};
    v = (d[0] * q[0] + d[1] * q[1] + d[2] * q[2]) / det;
    if (!(v >= 0.0) || !(u + v <= 1.0)) return false;
    t = (e2[0] * q[0] + e2[1] * q[1] + e2[2] * q[2]) / det;
    return t_min <= t && t <= t_max;
}

// Can the ray meet, with t in [t_lo, t_hi], a triangle inside box bx (lo xyz, hi xyz)?  Never false for a triangle that
// ray_triangle accepts (the section comment); near = where the ray enters the widened box, at least t_lo.
__device__ __forceinline__ bool ray_box(const double o[3], const double d[3], double t_lo, double t_hi, const double* __restrict__ bx,
                                        double& near) {
    double lo[3], hi[3], m = 0.0;
#pragma unroll
    for (int a = 0; a < 3; ++a) {
        lo[a] = bx[a] - o[a], hi[a] = bx[3 + a] - o[a];
        m = fmax(m, fmax(fabs(lo[a]), fabs(hi[a])));
    }
    const double w = PF_RAY_SLACK * m;
    double tn = t_lo, tf = t_hi;
    bool outside = false;
#pragma unroll
    for (int a = 0; a < 3; ++a) {
        const double nl = lo[a] - w, nh = hi[a] + w;
        if (d[a] == 0.0) {  // +0.0 and -0.0: the ray stays at o on this axis
            outside = outside || nl > 0.0 || nh < 0.0;
        } else {
            const double t1 = nl / d[a], t2 = nh / d[a];
            tn = fmax(tn, fmin(t1, t2));
            tf = fmin(tf, fmax(t1, t2));
        }
    }
    near = tn;
    return !outside && tn <= tf;
}

struct Hit {
    double t;
    int32_t orig;  // triangle index (tie-break: lowest)
    double u, v;
};

// one wave (= one block) per packet of PACKET sorted rays; lane = ray (lane % PACKET) x triangle subset (lane / PACKET)
template <int PACKET, bool COUNT>
__global__ __launch_bounds__(PF_WAVE) void k_raycast(const double* __restrict__ tri, const int32_t* __restrict__ tri_orig,
                                                     const double* __restrict__ box, const double* __restrict__ sbox, int64_t n_tri,
                                                     int64_t n_chunks, int64_t n_super, const double* __restrict__ org,
                                                     const double* __restrict__ dir, const int32_t* __restrict__ perm, int64_t n_rays,
                                                     double t_min, double t_max, int32_t facing, int32_t per_face,
                                                     double* __restrict__ out_t, int32_t* __restrict__ out_face,
                                                     double* __restrict__ out_uv, int32_t* __restrict__ out_count) {
    __shared__ double s_tri[9][PF_TRI_CHUNK];  // one chunk, SoA as in HBM
    __shared__ int32_t s_orig[PF_TRI_CHUNK];
    __shared__ double s_ray[7][PACKET];  // ox oy oz dx dy dz t_hi of the packet's rays
    constexpr int SUB = PF_WAVE / PACKET;  // lanes per ray
    static_assert(PF_WAVE % PACKET == 0, "a packet divides the wave");
    const int lane = threadIdx.x, slot = lane % PACKET, sub = lane / PACKET;
    const int64_t i = (int64_t)blockIdx.x * PACKET + slot;
    const bool live = i < n_rays;
    const int64_t ri = live ? perm[i] : -1;  // the caller's index of this lane's ray
    const double inf = std::numeric_limits<double>::infinity(), nan = __longlong_as_double(0x7ff8000000000000ll);
    double o[3] = {0.0, 0.0, 0.0}, d[3] = {0.0, 0.0, 0.0};
    if (live) {
#pragma unroll
        for (int a = 0; a < 3; ++a) o[a] = org[3 * ri + a], d[a] = dir[3 * ri + a];
    }
    bool ok = live && (d[0] != 0.0 || d[1] != 0.0 || d[2] != 0.0);
#pragma unroll
    for (int a = 0; a < 3; ++a) ok = ok && std::isfinite(o[a]) && std::isfinite(d[a]);
    // a dead slot (past the end, non-finite, zero direction) is a ray at the origin with an empty interval
    if (!ok) o[0] = o[1] = o[2] = d[0] = d[1] = d[2] = 0.0;
    double t_hi = ok ? t_max : -inf;  // the ray's upper end: min(t_max, its least accepted t) unless COUNT
    if (sub == 0) {
#pragma unroll
        for (int a = 0; a < 3; ++a) s_ray[a][slot] = o[a], s_ray[3 + a][slot] = d[a];
        s_ray[6][slot] = t_hi;
    }
    __syncthreads();

    Hit best;
    best.t = inf, best.orig = 0x7fffffff, best.u = best.v = nan;
    int32_t count = 0;

    // lane = box: the least entry parameter over the packet's rays that may meet box bx; false if none may
    auto packet_box = [&](const double* __restrict__ bx, double& near) {
        bool any = false;
        near = inf;
        for (int j = 0; j < PACKET; ++j) {
            const double ro[3] = {s_ray[0][j], s_ray[1][j], s_ray[2][j]}, rd[3] = {s_ray[3][j], s_ray[4][j], s_ray[5][j]};
            double tn;
            if (ray_box(ro, rd, t_min, s_ray[6][j], bx, tn)) any = true, near = fmin(near, tn);
        }
        return any;
    };
    // stage chunk c in LDS and test its triangles against every ray that may meet its box; true if any ray did
    auto scan = [&](int64_t c) {
        double tn;
        const bool want = ok && ray_box(o, d, t_min, t_hi, box + 6 * c, tn);
        if (!__ballot(want)) return;
        const int64_t s = c * PF_TRI_CHUNK + lane;
        const int cnt = (int)(n_tri - c * PF_TRI_CHUNK < PF_TRI_CHUNK ? n_tri - c * PF_TRI_CHUNK : PF_TRI_CHUNK);
        __syncthreads();  // the previous chunk's reads are done
        if (lane < cnt) {
#pragma unroll
            for (int k = 0; k < 9; ++k) s_tri[k][lane] = tri[(int64_t)k * n_tri + s];
            s_orig[lane] = tri_orig[s];
        }
        __syncthreads();
        if (want) {
            for (int k = sub; k < cnt; k += SUB) {
                const double a[3] = {s_tri[0][k], s_tri[1][k], s_tri[2][k]}, b[3] = {s_tri[3][k], s_tri[4][k], s_tri[5][k]},
                             cc[3] = {s_tri[6][k], s_tri[7][k], s_tri[8][k]};
                double t, u, v;
                if (!ray_triangle(o, d, a, b, cc, t_min, t_hi, facing, t, u, v)) continue;
                ++count;
                const int32_t og = s_orig[k];
                if (better(t, og, best.t, best.orig)) best.t = t, best.orig = og, best.u = u, best.v = v;
            }
        }
        if (!COUNT) {  // the ray's new upper end: the least t its SUB lanes have found (t == t_hi may still win the tie)
            double q = best.t;
            for (int off = PACKET; off < PF_WAVE; off <<= 1) q = fmin(q, __shfl_xor(q, off, PF_WAVE));
            if (ok) t_hi = fmin(t_max, q);
            if (sub == 0) s_ray[6][slot] = t_hi;
            __syncthreads();
        }
    };
    // Of the lanes with keep set, the one with the least near (lowest lane on ties), or -1; near > bound for it means the
    // same for all that remain.  The chosen lane is cleared.
    auto take = [&](bool& keep, double near) {
        double k = keep ? near : inf;
        int64_t l = keep ? lane : PF_WAVE + lane;  // a kept lane wins a tie at +inf against the others
        wave_argmin(k, l);
        if (l >= PF_WAVE) return -1;
        if (l == lane) keep = false;
        return (int)l;
    };

    double bound = wave_max(t_hi);  // the packet's upper end: that of its farthest-reaching ray
    for (int64_t sb = 0; sb < n_super && bound >= t_min; sb += PF_WAVE) {
        const int64_t s = sb + lane;
        double snear = inf;
        bool skeep = s < n_super && packet_box(sbox + 6 * s, snear);
        for (int sl = take(skeep, snear); sl >= 0; sl = take(skeep, snear)) {
            if (__shfl(snear, sl, PF_WAVE) > bound) break;  // t_hi has shrunk since the ballot: nothing left reaches in
            const int64_t c = (sb + sl) * PF_WAVE + lane;
            double cnear = inf;
            bool ckeep = c < n_chunks && packet_box(box + 6 * c, cnear);
            for (int cl = take(ckeep, cnear); cl >= 0; cl = take(ckeep, cnear)) {
                if (__shfl(cnear, cl, PF_WAVE) > bound) break;
                scan((sb + sl) * PF_WAVE + cl);
                bound = wave_max(t_hi);
            }
        }
    }

    // the ray's winner over its lanes (least t, lowest triangle index) and its count, outputs in the caller's order
    for (int off = PACKET; off < PF_WAVE; off <<= 1) {
        const double ot = __shfl_xor(best.t, off, PF_WAVE), ou = __shfl_xor(best.u, off, PF_WAVE), ov = __shfl_xor(best.v, off, PF_WAVE);
        const int32_t oo = __shfl_xor(best.orig, off, PF_WAVE);
        if (better(ot, oo, best.t, best.orig)) best.t = ot, best.orig = oo, best.u = ou, best.v = ov;
        count += __shfl_xor(count, off, PF_WAVE);
    }
    if (live && sub == 0) {
        const bool found = ok && best.orig != 0x7fffffff;
        if (out_t) out_t[ri] = found ? best.t : (ok ? inf : nan);
        if (out_face) out_face[ri] = found ? best.orig / per_face : -1;
        if (out_uv) out_uv[2 * ri] = found ? best.u : nan, out_uv[2 * ri + 1] = found ? best.v : nan;
        if (out_count) out_count[ri] = count;
    }
}

// ---- host side ---------------------------------------------------------------------------------------------------------

// the search of pf_surface_distance on queries already in HBM (d_q): Morton sort, k_distance, the fixed-order
// statistics.  d_d2 / d_face may be NULL; d_stats [PF_DIST_STATS] may not.
hipError_t distance_search(pf_surface* s, hipStream_t st, const double* d_q, int64_t n_qry, const KeyBox& bb, double* d_d2,
                           int32_t* d_face, double* d_stats) {
    // 16 queries per wave once that gives >= 4096 waves (4 per SIMD), else 4 (measured: profiles/surface_distance.md)
    const bool big = n_qry >= (int64_t)16 * 4096;
    const int64_t n_pack = big ? (n_qry + 15) / 16 : (n_qry + 3) / 4;
    const TriHierarchy& h = s->h;
    // no synchronise here: the scratch goes back at enqueue time, and the cache hands these blocks out again only to work
    // queued behind the kernels below
    Scratch sc(st);
    const int32_t* perm = pf_surface_morton_order(sc, d_q, 3, nullptr, 0, n_qry, bb);
    double* d_part = sc.get<double>(PF_DIST_STATS * n_pack);
    if (sc.ok()) {
        if (big)
            k_distance<16><<<(unsigned)n_pack, PF_WAVE, 0, st>>>(h.tri, h.tri_orig, h.box, h.sbox, h.n_tri, h.n_chunks, h.n_super,
                                                                 d_q, perm, n_qry, s->vpf - 2, d_d2, d_face, d_part);
        else
            k_distance<4><<<(unsigned)n_pack, PF_WAVE, 0, st>>>(h.tri, h.tri_orig, h.box, h.sbox, h.n_tri, h.n_chunks, h.n_super,
                                                                d_q, perm, n_qry, s->vpf - 2, d_d2, d_face, d_part);
        k_distance_stats<<<1, PF_BLOCK, 0, st>>>(d_part, n_pack, d_stats);
        sc.launched();
    }
    return sc.err;
}

// the per-surface arrays of the signed distances: gone, as before pf_surface_prepare_signed
void release_signed(pf_surface* s, hipStream_t st) {
    pf_free(st, s->pts), pf_free(st, s->faces), pf_free(st, s->tnrm), pf_free(st, s->enrm), pf_free(st, s->vnrm);
    s->pts = s->tnrm = s->enrm = s->vnrm = nullptr;
    s->faces = nullptr;
}

}  // namespace

extern "C" {

void pf_surface_free(pf_surface* s) {
    if (!s) return;
    hipSetDevice(s->ctx->device);
    hipStreamSynchronize(s->ctx->stream);
    hipStream_t st = s->ctx->stream;
    pf_tri_hierarchy_free(st, s->h);
    pf_free(st, s->pts);
    pf_free(st, s->faces);
    pf_free(st, s->tnrm);
    pf_free(st, s->enrm);
    pf_free(st, s->vnrm);
    pf_free(st, s->dip);
    pf_free(st, s->sdip);
    delete s;
}

int pf_surface_create(pf_ctx* ctx, const double* pts, int64_t n, const int32_t* faces, int64_t n_faces, int32_t vpf,
                      pf_surface** out) {
    PF_CHECK(ctx && pts && faces && out, PF_E_ARG, "pf_surface_create: NULL argument");
    PF_CHECK(n > 0 && n < ((int64_t)1 << 31), PF_E_ARG, "pf_surface_create: n = %lld out of range", (long long)n);
    PF_CHECK(vpf >= 3 && vpf <= 16 && n_faces > 0 && n_faces * (vpf - 2) < ((int64_t)1 << 31), PF_E_ARG,
             "pf_surface_create: faces %lld x %d out of range", (long long)n_faces, vpf);
    PF_TRY(pf_check_faces("pf_surface_create", faces, n_faces, vpf, n, false));
    const KeyBox bb = pf_key_box(pts, n, 3, false);
    PF_HIP(hipSetDevice(ctx->device));
    hipStream_t st = ctx->stream;
    pf_surface* s = new pf_surface();
    s->ctx = ctx;
    s->n_points = n, s->n_faces = n_faces, s->vpf = vpf;
    hipError_t e;
    {
        Scratch sc(st);
        double* d_pts = sc.get<double>(3 * n);
        int32_t* d_faces = sc.get<int32_t>(n_faces * vpf);
        sc.upload(d_pts, pts, 3 * n);
        sc.upload(d_faces, faces, n_faces * vpf);
        pf_tri_hierarchy_build(sc, s->h, d_pts, 3, d_faces, n_faces, vpf, bb);
        sc.sync();  // the host arrays may go away after the call
        e = sc.err;
    }
    if (e != hipSuccess) {
        pf_set_error("pf_surface_create: %s", hipGetErrorString(e));
        pf_surface_free(s);
        return PF_E_HIP;
    }
    *out = s;
    return PF_OK;
}

int pf_surface_closest(pf_surface* s, const double* qry, int64_t n_qry, double* out_pts, int32_t* out_face, double* out_d2) {
    PF_CHECK(s && (qry || n_qry == 0), PF_E_ARG, "pf_surface_closest: NULL argument");
    PF_CHECK(n_qry >= 0 && n_qry < ((int64_t)1 << 31), PF_E_ARG, "pf_surface_closest: n_qry = %lld out of range", (long long)n_qry);
    if (n_qry == 0) return PF_OK;
    PF_HIP(hipSetDevice(s->ctx->device));
    hipStream_t st = s->ctx->stream;
    const TriHierarchy& h = s->h;
    Scratch sc(st);
    double *d_q = sc.get<double>(3 * n_qry), *d_pt = sc.get<double>(3 * n_qry), *d_d2 = sc.get<double>(n_qry);
    int32_t* d_face = sc.get<int32_t>(n_qry);
    sc.upload(d_q, qry, 3 * n_qry);
    if (sc.ok()) {
        k_closest<<<(unsigned)n_qry, PF_CLOSEST_WAVES * PF_WAVE, 0, st>>>(h.tri, h.tri_orig, h.box, h.sbox, h.n_tri, h.n_chunks,
                                                                          h.n_super, d_q, n_qry, s->vpf - 2, d_pt, d_face, d_d2);
        sc.launched();
    }
    sc.download(out_pts, d_pt, 3 * n_qry);
    sc.download(out_face, d_face, n_qry);
    sc.download(out_d2, d_d2, n_qry);
    sc.sync();
    if (!sc.ok()) {
        pf_set_error("pf_surface_closest: %s", hipGetErrorString(sc.err));
        return PF_E_HIP;
    }
    return PF_OK;
}

int pf_surface_distance(pf_surface* s, const double* qry, int64_t n_qry, double* out_d2, int32_t* out_face, double* stats) {
    PF_CHECK(s && qry, PF_E_ARG, "pf_surface_distance: NULL argument");
    PF_CHECK(n_qry >= 1 && n_qry < ((int64_t)1 << 31), PF_E_ARG, "pf_surface_distance: n_qry = %lld out of range", (long long)n_qry);
    const KeyBox bb = pf_key_box(qry, n_qry, 3, true);
    PF_HIP(hipSetDevice(s->ctx->device));
    hipStream_t st = s->ctx->stream;
    Scratch sc(st);
    double* d_q = sc.get<double>(3 * n_qry);
    double* d_d2 = out_d2 ? sc.get<double>(n_qry) : nullptr;
    int32_t* d_face = out_face ? sc.get<int32_t>(n_qry) : nullptr;
    double* d_stats = sc.get<double>(PF_DIST_STATS);
    sc.upload(d_q, qry, 3 * n_qry);
    if (sc.ok()) sc.note(distance_search(s, st, d_q, n_qry, bb, d_d2, d_face, d_stats));
    sc.download(out_d2, d_d2, n_qry);
    sc.download(out_face, d_face, n_qry);
    sc.download(stats, d_stats, PF_DIST_STATS);
    sc.sync();
    if (!sc.ok()) {
        pf_set_error("pf_surface_distance: %s", hipGetErrorString(sc.err));
        return PF_E_HIP;
    }
    return PF_OK;
}

int pf_surface_prepare_signed(pf_surface* s, const double* points, const int32_t* faces, int64_t* topology) {
    PF_CHECK(s && points && faces, PF_E_ARG, "pf_surface_prepare_signed: NULL argument");
    const int64_t n = s->n_points, T = s->h.n_tri, H = 3 * T, nf = s->n_faces * s->vpf;
    PF_CHECK(H < ((int64_t)1 << 31), PF_E_ARG, "pf_surface_prepare_signed: %lld half-edges out of range", (long long)H);
    // the same arrays as at pf_surface_create, or at least indices within them
    PF_TRY(pf_check_faces("pf_surface_prepare_signed", faces, s->n_faces, s->vpf, n, false));
    const int nb = pf_index_bits(n);  // bits of a vertex index
    PF_HIP(hipSetDevice(s->ctx->device));
    hipStream_t st = s->ctx->stream;
    release_signed(s, st);  // a second call builds afresh from the arrays it is given
    unsigned long long counts[4] = {0, 0, 0, 0};
    hipError_t e;
    {
        Scratch sc(st);
        s->pts = sc.keep<double>(3 * n);
        s->faces = sc.keep<int32_t>(nf);
        s->tnrm = sc.keep<double>(3 * T);
        s->enrm = sc.keep<double>(3 * H);
        s->vnrm = sc.keep<double>(3 * n);
        double* tang = sc.get<double>(H);
        unsigned long long *ek0 = sc.get<unsigned long long>(H), *ek1 = sc.get<unsigned long long>(H);
        unsigned *vk0 = sc.get<unsigned>(H), *vk1 = sc.get<unsigned>(H);
        int32_t *h0 = sc.get<int32_t>(H), *h1 = sc.get<int32_t>(H);
        unsigned long long* cnt = sc.get<unsigned long long>(4);
        sc.upload(s->pts, points, 3 * n);
        sc.upload(s->faces, faces, nf);
        sc.zero(cnt, sizeof(unsigned long long) * 4);
        if (sc.ok()) {
            k_tri_normals<<<pf_blocks(T), PF_BLOCK, 0, st>>>(s->pts, s->faces, s->vpf, T, nb, s->tnrm, tang, ek0, vk0, h0);
            sc.launched();
        }
        // both sorts are stable and start from half-edge order: equal keys stay in triangle order.  They share the value
        // arrays, and the stream runs the vertex sort after k_edge_normals has read the edge sort's h1.
        pf_sort_pairs(sc, ek0, ek1, h0, h1, H, 2 * nb);
        if (sc.ok()) {
            k_edge_normals<<<pf_blocks(H), PF_BLOCK, 0, st>>>(ek1, h1, H, s->faces, s->vpf, s->tnrm, s->enrm, cnt);
            sc.launched();
        }
        pf_sort_pairs(sc, vk0, vk1, h0, h1, H, nb);
        if (sc.ok()) {
            k_vertex_normals<<<pf_blocks(n), PF_BLOCK, 0, st>>>(vk1, h1, H, n, s->tnrm, tang, s->vnrm);
            sc.launched();
        }
        sc.download(counts, cnt, 4);
        sc.sync();  // the host arrays may go away after the call
        e = sc.err;
    }
    if (e != hipSuccess) {
        release_signed(s, st);
        pf_set_error("pf_surface_prepare_signed: %s", hipGetErrorString(e));
        return PF_E_HIP;
    }
    if (topology)
        for (int k = 0; k < 4; ++k) topology[k] = (int64_t)counts[k];
    return PF_OK;
}

int pf_surface_signed_distance(pf_surface* s, const double* qry, int64_t n_qry, double* out_sd, int32_t* out_face,
                               int32_t* out_feature, int64_t* n_ambiguous) {
    PF_CHECK(s && qry, PF_E_ARG, "pf_surface_signed_distance: NULL argument");
    PF_CHECK(n_qry >= 1 && n_qry < ((int64_t)1 << 31), PF_E_ARG, "pf_surface_signed_distance: n_qry = %lld out of range",
             (long long)n_qry);
    PF_CHECK(s->vnrm, PF_E_ARG, "pf_surface_signed_distance: pf_surface_prepare_signed has not been called");
    const KeyBox bb = pf_key_box(qry, n_qry, 3, true);
    PF_HIP(hipSetDevice(s->ctx->device));
    hipStream_t st = s->ctx->stream;
    Scratch sc(st);
    double *d_q = sc.get<double>(3 * n_qry), *d_d2 = sc.get<double>(n_qry);
    int32_t* d_face = sc.get<int32_t>(n_qry);
    double *d_stats = sc.get<double>(PF_DIST_STATS), *d_sd = sc.get<double>(n_qry);
    int32_t* d_feat = sc.get<int32_t>(n_qry);
    unsigned long long* d_amb = sc.get<unsigned long long>(1);
    unsigned long long amb = 0;
    sc.upload(d_q, qry, 3 * n_qry);
    sc.zero(d_amb, sizeof(unsigned long long));
    if (sc.ok()) sc.note(distance_search(s, st, d_q, n_qry, bb, d_d2, d_face, d_stats));
    if (sc.ok()) {
        k_signed<<<pf_blocks(n_qry), PF_BLOCK, 0, st>>>(s->pts, s->faces, s->vpf, s->tnrm, s->enrm, s->vnrm, d_q, n_qry, d_d2, d_face,
                                                   d_sd, d_feat, d_amb);
        sc.launched();
    }
    sc.download(out_sd, d_sd, n_qry);
    sc.download(out_face, d_face, n_qry);
    sc.download(out_feature, d_feat, n_qry);
    sc.download(&amb, d_amb, 1);
    sc.sync();
    if (!sc.ok()) {
        pf_set_error("pf_surface_signed_distance: %s", hipGetErrorString(sc.err));
        return PF_E_HIP;
    }
    if (n_ambiguous) *n_ambiguous = (int64_t)amb;
    return PF_OK;
}

int pf_surface_prepare_winding(pf_surface* s) {
    PF_CHECK(s, PF_E_ARG, "pf_surface_prepare_winding: NULL argument");
    if (s->dip) return PF_OK;  // built once: the triangles never change
    PF_HIP(hipSetDevice(s->ctx->device));
    hipStream_t st = s->ctx->stream;
    const TriHierarchy& h = s->h;
    Scratch sc(st);  // no scratch, two blocks to keep: published only when everything worked
    double *dip = sc.keep<double>(PF_DIPOLE * h.n_chunks), *sdip = sc.keep<double>(PF_DIPOLE * h.n_super);
    if (sc.ok()) {
        k_chunk_dipoles<<<(unsigned)h.n_chunks, PF_WAVE, 0, st>>>(h.tri, h.n_tri, h.box, dip);
        k_super_dipoles<<<(unsigned)h.n_super, PF_WAVE, 0, st>>>(h.tri, h.n_tri, dip, h.n_chunks, h.sbox, sdip);
        sc.launched();
    }
    sc.sync();
    if (!sc.ok()) {
        pf_free(st, dip);
        pf_free(st, sdip);
        pf_set_error("pf_surface_prepare_winding: %s", hipGetErrorString(sc.err));
        return PF_E_HIP;
    }
    s->dip = dip, s->sdip = sdip;
    return PF_OK;
}

int pf_surface_winding(pf_surface* s, const double* qry, int64_t n_qry, double beta, double* out_w, double* out_bound) {
    PF_CHECK(s && qry, PF_E_ARG, "pf_surface_winding: NULL argument");
    PF_CHECK(n_qry >= 1 && n_qry < ((int64_t)1 << 31), PF_E_ARG, "pf_surface_winding: n_qry = %lld out of range", (long long)n_qry);
    PF_CHECK(s->dip, PF_E_ARG, "pf_surface_winding: pf_surface_prepare_winding has not been called");
    // beta <= 0: exact.  A query may lie inside a cluster's ball for beta <= 1, where the dropped part has no bound.
    PF_CHECK(beta <= 0.0 || (beta > 1.0 && std::isfinite(beta)), PF_E_ARG,
             "pf_surface_winding: beta = %g: use beta <= 0 (exact) or a finite beta > 1", beta);
    const KeyBox bb = pf_key_box(qry, n_qry, 3, true);
    PF_HIP(hipSetDevice(s->ctx->device));
    hipStream_t st = s->ctx->stream;
    const TriHierarchy& h = s->h;
    const int64_t n_pack = (n_qry + PF_WIND_PACKET - 1) / PF_WIND_PACKET;
    Scratch sc(st);
    double* d_q = sc.get<double>(3 * n_qry);
    double* d_w = out_w ? sc.get<double>(n_qry) : nullptr;
    double* d_b = out_bound ? sc.get<double>(n_qry) : nullptr;
    sc.upload(d_q, qry, 3 * n_qry);
    const int32_t* perm = pf_surface_morton_order(sc, d_q, 3, nullptr, 0, n_qry, bb);
    if (sc.ok()) {
        if (beta > 0.0)
            k_winding<true><<<(unsigned)n_pack, PF_WAVE, 0, st>>>(h.tri, h.n_tri, h.n_chunks, h.n_super, s->dip, s->sdip, d_q, perm,
                                                                  n_qry, beta, d_w, d_b);
        else
            k_winding<false><<<(unsigned)n_pack, PF_WAVE, 0, st>>>(h.tri, h.n_tri, h.n_chunks, h.n_super, s->dip, s->sdip, d_q, perm,
                                                                   n_qry, 0.0, d_w, d_b);
        sc.launched();
    }
    sc.download(out_w, d_w, n_qry);
    sc.download(out_bound, d_b, n_qry);
    sc.sync();
    if (!sc.ok()) {
        pf_set_error("pf_surface_winding: %s", hipGetErrorString(sc.err));
        return PF_E_HIP;
    }
    return PF_OK;
}

int pf_surface_raycast(pf_surface* s, const double* origins, const double* dirs, int64_t n_rays, double t_min, double t_max,
                       int32_t facing, double* out_t, int32_t* out_face, double* out_uv, int32_t* out_count) {
    PF_CHECK(s && origins && dirs, PF_E_ARG, "pf_surface_raycast: NULL argument");
    PF_CHECK(n_rays >= 1 && n_rays < ((int64_t)1 << 31), PF_E_ARG, "pf_surface_raycast: n_rays = %lld out of range", (long long)n_rays);
    PF_CHECK(t_min <= t_max, PF_E_ARG, "pf_surface_raycast: the interval [%g, %g] is empty or NaN", t_min, t_max);
    PF_CHECK(facing >= -1 && facing <= 1, PF_E_ARG, "pf_surface_raycast: facing = %d: use -1 (back), 0 (any) or 1 (front)", facing);
    const KeyBox bb = pf_key_box(origins, n_rays, 3, true);
    PF_HIP(hipSetDevice(s->ctx->device));
    hipStream_t st = s->ctx->stream;
    const TriHierarchy& h = s->h;
    // the packet rule of distance_search: 16 rays per wave once that gives >= 4096 waves, else 4
    const bool big = n_rays >= (int64_t)16 * 4096;
    const unsigned n_pack = (unsigned)(big ? (n_rays + 15) / 16 : (n_rays + 3) / 4);
    Scratch sc(st);
    double *d_o = sc.get<double>(3 * n_rays), *d_d = sc.get<double>(3 * n_rays);
    double* d_t = out_t ? sc.get<double>(n_rays) : nullptr;
    int32_t* d_face = out_face ? sc.get<int32_t>(n_rays) : nullptr;
    double* d_uv = out_uv ? sc.get<double>(2 * n_rays) : nullptr;
    int32_t* d_cnt = out_count ? sc.get<int32_t>(n_rays) : nullptr;
    sc.upload(d_o, origins, 3 * n_rays);
    sc.upload(d_d, dirs, 3 * n_rays);
    const int32_t* perm = pf_surface_morton_order(sc, d_o, 3, nullptr, 0, n_rays, bb);
    if (sc.ok()) {
        const auto launch = [&](auto kernel) {
            kernel<<<n_pack, PF_WAVE, 0, st>>>(h.tri, h.tri_orig, h.box, h.sbox, h.n_tri, h.n_chunks, h.n_super, d_o, d_d, perm,
                                               n_rays, t_min, t_max, facing, s->vpf - 2, d_t, d_face, d_uv, d_cnt);
        };
        if (big)
            out_count ? launch(k_raycast<16, true>) : launch(k_raycast<16, false>);
        else
            out_count ? launch(k_raycast<4, true>) : launch(k_raycast<4, false>);
        sc.launched();
    }
    sc.download(out_t, d_t, n_rays);
    sc.download(out_face, d_face, n_rays);
    sc.download(out_uv, d_uv, 2 * n_rays);
    sc.download(out_count, d_cnt, n_rays);
    sc.sync();
    if (!sc.ok()) {
        pf_set_error("pf_surface_raycast: %s", hipGetErrorString(sc.err));
        return PF_E_HIP;
    }
    return PF_OK;
}

int pf_surface_vertex_normals(pf_surface* s, double* out) {
    PF_CHECK(s && out, PF_E_ARG, "pf_surface_vertex_normals: NULL argument");
    PF_CHECK(s->vnrm, PF_E_ARG, "pf_surface_vertex_normals: pf_surface_prepare_signed has not been called");
    PF_HIP(hipSetDevice(s->ctx->device));
    Scratch sc(s->ctx->stream);
    sc.download(out, s->vnrm, 3 * s->n_points);
    sc.sync();
    if (!sc.ok()) {
        pf_set_error("pf_surface_vertex_normals: %s", hipGetErrorString(sc.err));
        return PF_E_HIP;
    }
    return PF_OK;
}

}  // extern "C"
