// Closest point on a triangulated surface embedded in d dimensions (1 <= d <= 16): face, corners, barycentric weights
// and squared distance for many queries (pf_surface_nd_*).  This is the sub-vertex correspondence of FOCUSR: the target
// mesh is a 2-manifold in spectral coordinates, and a source vertex maps to a point of one of its triangles, not to one
// of its vertices.
//
// Structure (pf_surface_nd_create), the one of pf_surface.hip in d coordinates: the fan triangles (0, j+1, j+2) are
// sorted along a Morton curve of their centroids (hipCUB radix sort, stable) and cut into chunks of 64 consecutive ones,
// each with its d-dimensional bounding box; 64 consecutive chunks form a super-chunk with its own box.  Coordinates are
// stored SoA, [corner][coordinate][triangle], so a wave reads 64 consecutive triangles coalesced.
// The Morton key takes 10 bits from each of the LEADING min(d, 3) coordinates only.  Spectral coordinates come ordered by
// eigenvalue: the first ones are the smoothest eigenfunctions and carry the coarse geometry of the surface, the later
// ones oscillate and would scatter neighbours along the curve; three coordinates at 10 bits fill the 30-bit key the
// 3-D code sorts by, and a 2-manifold needs no more to be cut into compact pieces.  The key only decides which triangles
// share a chunk, that is how tight the boxes are; the boxes themselves span all d coordinates and the result does not
// depend on the order.
//
// Search (pf_surface_nd_closest, k_closest_nd): the queries are Morton-sorted by the same kind of key and cut into packets
// of PF_ND_PACKET = 8 consecutive ones, ONE WAVE (= one block) PER PACKET; lane = query (lane % 8) x triangle subset
// (lane / 8).  One packet size for every query count: 8 queries share each chunk load, 250k queries still give 31k waves,
// and a staged chunk at d = 16 is 64 x 3 x 16 x 8 B = 24 KiB of LDS, so 6 waves fit a CU's 160 KiB.  (1) the chunk nearest
// to the centre of the packet's box is scanned first and gives every query an upper bound; (2) one ballot over the
// super-chunk boxes, then per surviving super-chunk one ballot over its 64 chunk boxes; a surviving chunk is staged ONCE
// per packet in LDS (one coalesced load per lane and row) and each query's 8 lanes share its triangles out, reading LDS
// by broadcast.  The query's coordinates stay in registers: the kernel is templated on d for d = 3, 4, 5, 6, 8, 10 (the
// depths FOCUSR uses: 3 after smoothing, n_spectral_features + extras before), and every other d runs the generic
// instance, whose loops are unrolled to 16 with a uniform k < d guard, so no array is indexed at run time.
//
// Exactness.  The result of a query is the minimum over ALL fan triangles of the exact point-triangle squared distance,
// lowest fan-triangle index on exact ties, NaN distances never winning - what the exhaustive mode computes by testing
// every triangle.  The pruned search skips (a) a super-chunk or chunk whose box is farther from the packet's box than
// the packet's bound (the largest of its queries' current best distances) times PF_ND_SLACK, (b) a chunk that is farther
// than bound x slack from every single query, (c) a triangle whose own box is farther than the query's best x slack.  A
// box contains its triangles, a packet's box its queries, so in exact arithmetic each of these distances is a lower bound
// of the point-triangle distance, and what is skipped is strictly farther than a triangle already found: it can neither
// win nor tie.  In floating point the box distance (d subtractions, squares and additions) carries a relative error of
// about (d + 2) eps <= 4e-15, and so does the exact test's d2; the slack of 1e-9 covers both a million times over, and a
// triangle within the slack is tested, not skipped.  Bounds only shrink, so a test made against an older, larger bound
// errs on the side of testing.  The lanes of a query merge with the same (d2, index) rule.
//
// Arithmetic, fixed so the host can reproduce every bit (tests/_surface_nd_ref.py): Ericson's region walk (Real-Time
// Collision Detection 5.1.5), operation for operation closest_on_triangle of pf_surface.hip and
// oracle/icp_port.py:closest_point_on_triangles, with every dot product summed left to right over coordinates 0 .. d-1
// and no FMA (-ffp-contract=off); the closest point formed per coordinate as a | b | c | a + v ab | a + w ac |
// b + w (c - b) | (a + ab v) + ac w by region; d2 the sum of squared coordinate differences, left to right.  The weights
// are (1, 0, 0) | (0, 1, 0) | (0, 0, 1) | (1 - v, v, 0) | (1 - w, 0, w) | (0, 1 - w, w) | ((1 - v) - w, v, w).
// No floating-point atomics: two calls give identical bits.
#include <hipcub/hipcub.hpp>

#include <cmath>
#include <limits>

#include "pf_internal.h"

struct pf_surface_nd {
    pf_ctx* ctx = nullptr;
    int64_t n_points = 0, n_faces = 0, n_tri = 0, n_chunks = 0, n_super = 0;
    int32_t vpf = 0, d = 0;
    double* tri = nullptr;        // SoA [3 corners][d][n_tri], Morton order
    int32_t* tri_orig = nullptr;  // [n_tri] sorted position -> fan-triangle index (face * (vpf-2) + fan position)
    double* box = nullptr;        // [n_chunks][2][d] lo, hi
    double* sbox = nullptr;       // [n_super][2][d] boxes of 64 consecutive chunks
    int32_t* faces = nullptr;     // [n_faces][vpf] device copy: the corners of the winning triangle
    int64_t last_chunks = 0, last_packets = 0;  // chunks staged / packets of the last search (pf_surface_nd_last_search)
};

namespace {

constexpr int PF_ND_MAX = 16;     // coordinates (the limit of pf_knn_upload and pf_assign)
constexpr int PF_ND_CHUNK = 64;   // triangles per chunk: one per lane when a chunk is staged
constexpr int PF_ND_PACKET = 8;   // queries per wave
constexpr double PF_ND_SLACK = 1.0 + 1e-9;  // a box test must never reject on a rounding error (see above)
enum { PF_ND_A = 0, PF_ND_B = 1, PF_ND_C = 2, PF_ND_AB = 3, PF_ND_BC = 4, PF_ND_CA = 5, PF_ND_FACE = 6 };

inline unsigned nd_blocks(int64_t n) { return (unsigned)((n + PF_BLOCK - 1) / PF_BLOCK); }

// the box the keys are taken in: the leading nk = min(d, 3) coordinates
struct KeyBox {
    double lo[3], ext[3];
    int32_t nk;
};

__device__ __forceinline__ unsigned nd_spread10(unsigned v) {  // bit i -> bit 3 i
    v &= 0x3ffu;
    v = (v | (v << 16)) & 0x030000ffu;
    v = (v | (v << 8)) & 0x0300f00fu;
    v = (v | (v << 4)) & 0x030c30c3u;
    v = (v | (v << 2)) & 0x09249249u;
    return v;
}

// 30-bit key of the leading coordinates; outside the box clamps, NaN and a flat axis give 0
template <class Coord>
__device__ __forceinline__ unsigned nd_key(Coord coord, const KeyBox& bb) {
    unsigned code = 0;
#pragma unroll
    for (int a = 0; a < 3; ++a) {
        if (a >= bb.nk) break;
        double u = bb.ext[a] > 0.0 ? (coord(a) - bb.lo[a]) / bb.ext[a] : 0.0;
        u = u < 0.0 ? 0.0 : (u > 1.0 ? 1.0 : u);
        if (!(u == u)) u = 0.0;
        code |= nd_spread10((unsigned)(u * 1023.0)) << a;
    }
    return code;
}

__device__ __forceinline__ void nd_corners(const int32_t* __restrict__ faces, int32_t vpf, int64_t t, int32_t v[3]) {
    const int32_t per = vpf - 2;
    const int64_t f = t / per;
    const int32_t j = (int32_t)(t - f * per);
    v[0] = faces[f * vpf];
    v[1] = faces[f * vpf + j + 1];
    v[2] = faces[f * vpf + j + 2];
}

__global__ __launch_bounds__(PF_BLOCK) void k_nd_tri_keys(const double* __restrict__ pts, int32_t d, const int32_t* __restrict__ faces,
                                                          int32_t vpf, int64_t n_tri, KeyBox bb, unsigned* __restrict__ keys,
                                                          int32_t* __restrict__ vals) {
    const int64_t t = (int64_t)blockIdx.x * PF_BLOCK + threadIdx.x;
    if (t >= n_tri) return;
    int32_t v[3];
    nd_corners(faces, vpf, t, v);
    keys[t] = nd_key([&](int a) { return (pts[(int64_t)v[0] * d + a] + pts[(int64_t)v[1] * d + a] + pts[(int64_t)v[2] * d + a]) / 3.0; }, bb);
    vals[t] = (int32_t)t;
}

__global__ __launch_bounds__(PF_BLOCK) void k_nd_qry_keys(const double* __restrict__ qry, int32_t d, int64_t n, KeyBox bb,
                                                          unsigned* __restrict__ keys, int32_t* __restrict__ vals) {
    const int64_t i = (int64_t)blockIdx.x * PF_BLOCK + threadIdx.x;
    if (i >= n) return;
    keys[i] = nd_key([&](int a) { return qry[i * d + a]; }, bb);
    vals[i] = (int32_t)i;
}

__global__ __launch_bounds__(PF_BLOCK) void k_nd_gather(const double* __restrict__ pts, int32_t d, const int32_t* __restrict__ faces,
                                                        int32_t vpf, int64_t n_tri, const int32_t* __restrict__ order,
                                                        double* __restrict__ tri, int32_t* __restrict__ tri_orig) {
    const int64_t s = (int64_t)blockIdx.x * PF_BLOCK + threadIdx.x;
    if (s >= n_tri) return;
    const int32_t t = order[s];
    int32_t v[3];
    nd_corners(faces, vpf, t, v);
    for (int c = 0; c < 3; ++c)
        for (int k = 0; k < d; ++k) tri[(int64_t)(c * d + k) * n_tri + s] = pts[(int64_t)v[c] * d + k];
    tri_orig[s] = t;
}

// one wave per chunk, one triangle per lane
__global__ __launch_bounds__(PF_WAVE) void k_nd_chunk_boxes(const double* __restrict__ tri, int64_t n_tri, int32_t d, double* __restrict__ box) {
    const int64_t c = blockIdx.x;
    const int lane = threadIdx.x;
    const int64_t s = c * PF_ND_CHUNK + lane;
    const double inf = std::numeric_limits<double>::infinity();
    for (int k = 0; k < d; ++k) {
        double lo = inf, hi = -inf;
        if (s < n_tri) {
            for (int cr = 0; cr < 3; ++cr) {
                const double x = tri[(int64_t)(cr * d + k) * n_tri + s];
                lo = fmin(lo, x);  // fmin/fmax ignore NaN: a NaN vertex never widens a box
                hi = fmax(hi, x);
            }
        }
        for (int off = PF_WAVE / 2; off > 0; off >>= 1) {
            lo = fmin(lo, __shfl_xor(lo, off, PF_WAVE));
            hi = fmax(hi, __shfl_xor(hi, off, PF_WAVE));
        }
        if (lane == 0) {
            box[2 * d * c + k] = lo;
            box[2 * d * c + d + k] = hi;
        }
    }
}

// one wave per super-chunk: union of its 64 chunk boxes
__global__ __launch_bounds__(PF_WAVE) void k_nd_super_boxes(const double* __restrict__ box, int64_t n_chunks, int32_t d,
                                                            double* __restrict__ sbox) {
    const int64_t c = (int64_t)blockIdx.x * PF_WAVE + threadIdx.x;
    const double inf = std::numeric_limits<double>::infinity();
    for (int k = 0; k < d; ++k) {
        double lo = c < n_chunks ? box[2 * d * c + k] : inf, hi = c < n_chunks ? box[2 * d * c + d + k] : -inf;
        for (int off = PF_WAVE / 2; off > 0; off >>= 1) {
            lo = fmin(lo, __shfl_xor(lo, off, PF_WAVE));
            hi = fmax(hi, __shfl_xor(hi, off, PF_WAVE));
        }
        if (threadIdx.x == 0) {
            sbox[2 * d * (int64_t)blockIdx.x + k] = lo;
            sbox[2 * d * (int64_t)blockIdx.x + d + k] = hi;
        }
    }
}

__device__ __forceinline__ bool nd_better(double d2, int32_t orig, double bd2, int32_t borig) {
    return d2 < bd2 || (d2 == bd2 && orig < borig);
}

// every loop over coordinates: unrolled to the instance's depth; the generic instance (D = 0) guards with the uniform k < d
#define PF_ND_FOR(k) _Pragma("unroll") for (int k = 0; k < M; ++k) if (D != 0 || k < d)

// one wave (= one block) per packet of PF_ND_PACKET sorted queries.  D: the depth this instance is compiled for, 0 = any
// d <= PF_ND_MAX.  out_face / out_verts / out_bary / out_d2 may be NULL; opened [n_packets] = chunks the packet staged.
template <int D>
__global__ __launch_bounds__(PF_WAVE) void k_closest_nd(const double* __restrict__ tri, const int32_t* __restrict__ tri_orig,
                                                        const double* __restrict__ box, const double* __restrict__ sbox,
                                                        int64_t n_tri, int64_t n_chunks, int64_t n_super, int32_t d_any,
                                                        const int32_t* __restrict__ faces, int32_t vpf,
                                                        const double* __restrict__ qry, const int32_t* __restrict__ perm,
                                                        int64_t n_qry, int32_t exhaustive, int32_t* __restrict__ out_face,
                                                        int32_t* __restrict__ out_verts, double* __restrict__ out_bary,
                                                        double* __restrict__ out_d2, int32_t* __restrict__ opened) {
    constexpr int M = D ? D : PF_ND_MAX;
    constexpr int PACKET = PF_ND_PACKET, SUB = PF_WAVE / PACKET;
    static_assert(PF_WAVE % PACKET == 0, "a packet divides the wave");
    __shared__ double s_tri[3 * M][PF_ND_CHUNK];  // one chunk, SoA as in HBM: row = corner * d + coordinate
    __shared__ int32_t s_orig[PF_ND_CHUNK];
    const int d = D ? D : d_any;
    const int lane = threadIdx.x, sub = lane / PACKET;
    const int64_t i = (int64_t)blockIdx.x * PACKET + (lane % PACKET);
    const bool live = i < n_qry;
    const int64_t qi = live ? perm[i] : -1;  // the caller's index of this lane's query
    const double inf = std::numeric_limits<double>::infinity();
    const double nan = __longlong_as_double(0x7ff8000000000000ll);
    double p[M];
    bool ok = live;
    PF_ND_FOR(k) {
        p[k] = live ? qry[qi * d + k] : 0.0;
        ok = ok && std::isfinite(p[k]);
    }

    double best_d2 = inf, best_b0 = nan, best_b1 = nan, best_b2 = nan;
    int32_t best_orig = 0x7fffffff;
    int32_t n_opened = 0;
    // the query's bound: the least distance its SUB lanes have found
    auto query_min = [&](double v) {
        for (int off = PACKET; off < PF_WAVE; off <<= 1) v = fmin(v, __shfl_xor(v, off, PF_WAVE));
        return v;
    };
    auto wave_max = [&](double v) {
        for (int off = PF_WAVE / 2; off > 0; off >>= 1) v = fmax(v, __shfl_xor(v, off, PF_WAVE));
        return v;
    };
    if (__ballot(ok)) {
        double qbest = inf;
        auto scan = [&](int64_t c) {  // stage chunk c in LDS, test its triangles against every query
            const int64_t s = c * PF_ND_CHUNK + lane;
            const int cnt = (int)(n_tri - c * PF_ND_CHUNK < PF_ND_CHUNK ? n_tri - c * PF_ND_CHUNK : PF_ND_CHUNK);
            ++n_opened;
            __syncthreads();  // the previous chunk's reads are done
            if (lane < cnt) {
#pragma unroll
                for (int r = 0; r < 3 * M; ++r)
                    if (D != 0 || r < 3 * d) s_tri[r][lane] = tri[(int64_t)r * n_tri + s];
                s_orig[lane] = tri_orig[s];
            }
            __syncthreads();
            if (ok) {
                for (int t = sub; t < cnt; t += SUB) {
                    // first pass over the coordinates: the six dot products of the walk, and the triangle's own box
                    double d1 = 0.0, d2 = 0.0, d3 = 0.0, d4 = 0.0, d5 = 0.0, d6 = 0.0, tb = 0.0;
                    PF_ND_FOR(k) {
                        const double a = s_tri[k][t], b = s_tri[d + k][t], cc = s_tri[2 * d + k][t];
                        const double ab = b - a, ac = cc - a, ap = p[k] - a, bp = p[k] - b, cp = p[k] - cc;
                        const double e = fmax(fmax(fmin(fmin(a, b), cc) - p[k], p[k] - fmax(fmax(a, b), cc)), 0.0);
                        if (k == 0) {  // the sums start at their first term, not at +0.0 (the sign of a zero sum)
                            d1 = ab * ap, d2 = ac * ap, d3 = ab * bp, d4 = ac * bp, d5 = ab * cp, d6 = ac * cp, tb = e * e;
                        } else {
                            d1 += ab * ap, d2 += ac * ap, d3 += ab * bp, d4 += ac * bp, d5 += ab * cp, d6 += ac * cp, tb += e * e;
                        }
                    }
                    // the triangle's own box is never farther than the triangle (the chunk-box argument)
                    if (!exhaustive && tb > fmin(best_d2, qbest) * PF_ND_SLACK) continue;
                    int reg = PF_ND_FACE;
                    double v = 0.0, w = 0.0;
                    if (d1 <= 0.0 && d2 <= 0.0) {
                        reg = PF_ND_A;
                    } else if (d3 >= 0.0 && d4 <= d3) {
                        reg = PF_ND_B;
                    } else {
                        const double vc = d1 * d4 - d3 * d2;
                        if (vc <= 0.0 && d1 >= 0.0 && d3 <= 0.0) {
                            reg = PF_ND_AB, v = d1 / (d1 - d3);
                        } else if (d6 >= 0.0 && d5 <= d6) {
                            reg = PF_ND_C;
                        } else {
                            const double vb = d5 * d2 - d1 * d6;
                            if (vb <= 0.0 && d2 >= 0.0 && d6 <= 0.0) {
                                reg = PF_ND_CA, w = d2 / (d2 - d6);
                            } else {
                                const double va = d3 * d6 - d5 * d4;
                                if (va <= 0.0 && (d4 - d3) >= 0.0 && (d5 - d6) >= 0.0) {
                                    reg = PF_ND_BC, w = (d4 - d3) / ((d4 - d3) + (d5 - d6));
                                } else {
                                    const double denom = 1.0 / (va + vb + vc);
                                    v = vb * denom, w = vc * denom;
                                }
                            }
                        }
                    }
                    // second pass: the closest point coordinate by coordinate, and its squared distance
                    double dist2 = 0.0;
                    PF_ND_FOR(k) {
                        const double a = s_tri[k][t], b = s_tri[d + k][t], cc = s_tri[2 * d + k][t];
                        double q;
                        switch (reg) {
                            case PF_ND_A: q = a; break;
                            case PF_ND_B: q = b; break;
                            case PF_ND_C: q = cc; break;
                            case PF_ND_AB: q = a + v * (b - a); break;
                            case PF_ND_CA: q = a + w * (cc - a); break;
                            case PF_ND_BC: q = b + w * (cc - b); break;
                            default: q = (a + (b - a) * v) + (cc - a) * w; break;
                        }
                        const double diff = p[k] - q;
                        if (k == 0) dist2 = diff * diff;
                        else dist2 += diff * diff;
                    }
                    const int32_t o = s_orig[t];
                    if (nd_better(dist2, o, best_d2, best_orig)) {  // NaN distances compare false: never win
                        best_d2 = dist2, best_orig = o;
                        switch (reg) {
                            case PF_ND_A: best_b0 = 1.0, best_b1 = 0.0, best_b2 = 0.0; break;
                            case PF_ND_B: best_b0 = 0.0, best_b1 = 1.0, best_b2 = 0.0; break;
                            case PF_ND_C: best_b0 = 0.0, best_b1 = 0.0, best_b2 = 1.0; break;
                            case PF_ND_AB: best_b0 = 1.0 - v, best_b1 = v, best_b2 = 0.0; break;
                            case PF_ND_CA: best_b0 = 1.0 - w, best_b1 = 0.0, best_b2 = w; break;
                            case PF_ND_BC: best_b0 = 0.0, best_b1 = 1.0 - w, best_b2 = w; break;
                            default: best_b0 = (1.0 - v) - w, best_b1 = v, best_b2 = w; break;
                        }
                    }
                }
            }
            qbest = query_min(best_d2);
        };

        if (exhaustive) {
            for (int64_t c = 0; c < n_chunks; ++c) scan(c);
        } else {
            // the packet's box
            double lo[M], hi[M];
            PF_ND_FOR(k) {
                lo[k] = ok ? p[k] : inf, hi[k] = ok ? p[k] : -inf;
                for (int off = PF_WAVE / 2; off > 0; off >>= 1) {
                    lo[k] = fmin(lo[k], __shfl_xor(lo[k], off, PF_WAVE));
                    hi[k] = fmax(hi[k], __shfl_xor(hi[k], off, PF_WAVE));
                }
            }
            // squared distances to a box bx = lo[d] | hi[d]: of this lane's query, of the packet's box (never larger than
            // the former for any query of the packet), of the packet's centre
            auto point_box = [&](const double* __restrict__ bx) {
                double s = 0.0;
                PF_ND_FOR(k) {
                    const double e = fmax(fmax(bx[k] - p[k], p[k] - bx[d + k]), 0.0);
                    s += e * e;
                }
                return s;
            };
            auto packet_box = [&](const double* __restrict__ bx) {
                double s = 0.0;
                PF_ND_FOR(k) {
                    const double e = fmax(fmax(bx[k] - hi[k], lo[k] - bx[d + k]), 0.0);
                    s += e * e;
                }
                return s;
            };
            auto centre_box = [&](const double* __restrict__ bx) {
                double s = 0.0;
                PF_ND_FOR(k) {
                    const double ctr = 0.5 * (lo[k] + hi[k]);
                    const double e = fmax(fmax(bx[k] - ctr, ctr - bx[d + k]), 0.0);
                    s += e * e;
                }
                return s;
            };
            // the least (dist, index) of the wave, in every lane; lowest index on ties
            auto wave_argmin = [&](double& dist, int64_t& idx) {
                for (int off = PF_WAVE / 2; off > 0; off >>= 1) {
                    const double od = __shfl_xor(dist, off, PF_WAVE);
                    const int64_t oi = __shfl_xor(idx, off, PF_WAVE);
                    if (od < dist || (od == dist && oi < idx)) dist = od, idx = oi;
                }
            };
            // does any query's own point-box test keep chunk c?
            auto wanted = [&](int64_t c) { return __ballot(ok && point_box(box + 2 * d * c) <= qbest * PF_ND_SLACK) != 0; };

            // (1) seed: the chunk nearest to the packet's centre (nearest super-chunk, then nearest chunk inside it); only
            // a heuristic for a good first bound, n_chunks when there is no finite box
            int64_t c0 = n_chunks;
            {
                double nd = inf;
                int64_t ns = n_super;
                for (int64_t s = lane; s < n_super; s += PF_WAVE) {
                    const double e = centre_box(sbox + 2 * d * s);
                    if (e < nd) nd = e, ns = s;
                }
                wave_argmin(nd, ns);
                if (ns < n_super) {
                    c0 = ns * PF_WAVE + lane;
                    nd = c0 < n_chunks ? centre_box(box + 2 * d * c0) : inf;
                    if (!(nd < inf)) c0 = n_chunks;
                    wave_argmin(nd, c0);
                }
            }
            if (c0 < n_chunks) scan(c0);
            double bound = wave_max(ok ? qbest : -inf);  // the packet's bound: its worst query

            // (2) every chunk whose box is within the bound of the packet's box and of some query
            for (int64_t sb = 0; sb < n_super; sb += PF_WAVE) {
                const int64_t s = sb + lane;
                unsigned long long smask = __ballot(s < n_super && packet_box(sbox + 2 * d * s) <= bound * PF_ND_SLACK);
                while (smask) {
                    const int64_t ss = sb + __ffsll((long long)smask) - 1;
                    smask &= smask - 1;
                    if (packet_box(sbox + 2 * d * ss) > bound * PF_ND_SLACK) continue;  // the bound has shrunk
                    const int64_t c = ss * PF_WAVE + lane;
                    unsigned long long mask = __ballot(c < n_chunks && c != c0 && packet_box(box + 2 * d * c) <= bound * PF_ND_SLACK);
                    while (mask) {
                        const int64_t cc = ss * PF_WAVE + __ffsll((long long)mask) - 1;
                        mask &= mask - 1;
                        if (packet_box(box + 2 * d * cc) > bound * PF_ND_SLACK || !wanted(cc)) continue;
                        scan(cc);
                        bound = wave_max(ok ? qbest : -inf);
                    }
                }
            }
        }
    }

    // the query's winner over its lanes (smallest distance, lowest triangle index), outputs in the caller's order
    for (int off = PACKET; off < PF_WAVE; off <<= 1) {
        const double od = __shfl_xor(best_d2, off, PF_WAVE);
        const int32_t oo = __shfl_xor(best_orig, off, PF_WAVE);
        const double o0 = __shfl_xor(best_b0, off, PF_WAVE), o1 = __shfl_xor(best_b1, off, PF_WAVE), o2 = __shfl_xor(best_b2, off, PF_WAVE);
        if (nd_better(od, oo, best_d2, best_orig)) best_d2 = od, best_orig = oo, best_b0 = o0, best_b1 = o1, best_b2 = o2;
    }
    if (live && sub == 0) {
        const bool found = ok && best_orig != 0x7fffffff;  // else: a non-finite query, or no triangle with a finite distance
        if (out_face) out_face[qi] = found ? best_orig / (vpf - 2) : -1;
        if (out_verts) {
            int32_t v[3] = {-1, -1, -1};
            if (found) nd_corners(faces, vpf, best_orig, v);
            out_verts[3 * qi] = v[0], out_verts[3 * qi + 1] = v[1], out_verts[3 * qi + 2] = v[2];
        }
        if (out_bary) out_bary[3 * qi] = found ? best_b0 : nan, out_bary[3 * qi + 1] = found ? best_b1 : nan, out_bary[3 * qi + 2] = found ? best_b2 : nan;
        if (out_d2) out_d2[qi] = found ? best_d2 : nan;
    }
    if (lane == 0) opened[blockIdx.x] = n_opened;
}

#undef PF_ND_FOR

// the box of the leading coordinates of n points of depth d.  finite_only leaves every non-finite coordinate out
// (queries); without it only NaN is left out and an infinite coordinate flattens its axis (vertices), as in pf_surface.hip
KeyBox key_box(const double* pts, int64_t n, int32_t d, bool finite_only) {
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

// stable sort of n (key, value) pairs already in k0 / v0; the permutation (sorted position -> item), NULL after a failure
const int32_t* sort_by_key(Scratch& sc, unsigned* k0, int32_t* v0, int64_t n) {
    unsigned* k1 = sc.get<unsigned>(n);
    int32_t* v1 = sc.get<int32_t>(n);
    size_t need = 0;
    if (sc.ok()) sc.note(hipcub::DeviceRadixSort::SortPairs(nullptr, need, k0, k1, v0, v1, (int)n, 0, 30, sc.st));
    void* tmp = sc.get<char>(need);
    if (sc.ok()) sc.note(hipcub::DeviceRadixSort::SortPairs(tmp, need, k0, k1, v0, v1, (int)n, 0, 30, sc.st));
    return sc.ok() ? v1 : nullptr;
}

}  // namespace

extern "C" {

void pf_surface_nd_free(pf_surface_nd* s) {
    if (!s) return;
    hipSetDevice(s->ctx->device);
    hipStreamSynchronize(s->ctx->stream);
    hipStream_t st = s->ctx->stream;
    pf_free(st, s->tri);
    pf_free(st, s->tri_orig);
    pf_free(st, s->box);
    pf_free(st, s->sbox);
    pf_free(st, s->faces);
    delete s;
}

int pf_surface_nd_create(pf_ctx* ctx, const double* coords, int64_t n, int32_t d, const int32_t* faces, int64_t n_faces, int32_t vpf,
                         pf_surface_nd** out) {
    PF_CHECK(ctx && coords && faces && out, PF_E_ARG, "pf_surface_nd_create: NULL argument");
    PF_CHECK(d >= 1 && d <= PF_ND_MAX, PF_E_ARG, "pf_surface_nd_create: d = %d outside 1..%d", d, PF_ND_MAX);
    PF_CHECK(n > 0 && n < ((int64_t)1 << 31) / d, PF_E_ARG, "pf_surface_nd_create: n = %lld out of range", (long long)n);
    PF_CHECK(vpf >= 3 && vpf <= 16 && n_faces > 0 && n_faces * (vpf - 2) < ((int64_t)1 << 31) / (3 * d), PF_E_ARG,
             "pf_surface_nd_create: faces %lld x %d out of range", (long long)n_faces, vpf);
    for (int64_t i = 0; i < n_faces * vpf; ++i)
        PF_CHECK(faces[i] >= 0 && faces[i] < n, PF_E_ARG, "pf_surface_nd_create: face %lld references vertex %d of %lld",
                 (long long)(i / vpf), faces[i], (long long)n);
    const KeyBox bb = key_box(coords, n, d, false);
    PF_HIP(hipSetDevice(ctx->device));
    hipStream_t st = ctx->stream;
    pf_surface_nd* s = new pf_surface_nd();
    s->ctx = ctx;
    s->n_points = n, s->n_faces = n_faces, s->vpf = vpf, s->d = d;
    s->n_tri = n_faces * (vpf - 2);
    s->n_chunks = (s->n_tri + PF_ND_CHUNK - 1) / PF_ND_CHUNK;
    s->n_super = (s->n_chunks + PF_WAVE - 1) / PF_WAVE;
    const int64_t T = s->n_tri;
    hipError_t e;
    {
        Scratch sc(st);
        double* d_pts = sc.get<double>(n * d);
        s->faces = sc.keep<int32_t>(n_faces * vpf);
        s->tri = sc.keep<double>(3 * d * T);
        s->tri_orig = sc.keep<int32_t>(T);
        s->box = sc.keep<double>(2 * d * s->n_chunks);
        s->sbox = sc.keep<double>(2 * d * s->n_super);
        unsigned* keys = sc.get<unsigned>(T);
        int32_t* vals = sc.get<int32_t>(T);
        sc.upload(d_pts, coords, n * d);
        sc.upload(s->faces, faces, n_faces * vpf);
        if (sc.ok()) {
            k_nd_tri_keys<<<nd_blocks(T), PF_BLOCK, 0, st>>>(d_pts, d, s->faces, vpf, T, bb, keys, vals);
            sc.launched();
        }
        const int32_t* order = sort_by_key(sc, keys, vals, T);
        if (sc.ok()) {
            k_nd_gather<<<nd_blocks(T), PF_BLOCK, 0, st>>>(d_pts, d, s->faces, vpf, T, order, s->tri, s->tri_orig);
            k_nd_chunk_boxes<<<(unsigned)s->n_chunks, PF_WAVE, 0, st>>>(s->tri, T, d, s->box);
            k_nd_super_boxes<<<(unsigned)s->n_super, PF_WAVE, 0, st>>>(s->box, s->n_chunks, d, s->sbox);
            sc.launched();
        }
        sc.sync();  // the host arrays may go away after the call
        e = sc.err;
    }
    if (e != hipSuccess) {
        pf_set_error("pf_surface_nd_create: %s", hipGetErrorString(e));
        pf_surface_nd_free(s);
        return PF_E_HIP;
    }
    *out = s;
    return PF_OK;
}

int pf_surface_nd_closest(pf_surface_nd* s, const double* qry, int64_t n_qry, int32_t* out_face, int32_t* out_verts, double* out_bary,
                          double* out_d2, int32_t exhaustive) {
    PF_CHECK(s && qry, PF_E_ARG, "pf_surface_nd_closest: NULL argument");
    PF_CHECK(n_qry >= 1 && n_qry < ((int64_t)1 << 31) / s->d, PF_E_ARG, "pf_surface_nd_closest: n_qry = %lld out of range",
             (long long)n_qry);
    const int32_t d = s->d;
    const KeyBox bb = key_box(qry, n_qry, d, true);
    const int64_t n_pack = (n_qry + PF_ND_PACKET - 1) / PF_ND_PACKET;
    PF_HIP(hipSetDevice(s->ctx->device));
    hipStream_t st = s->ctx->stream;
    std::vector<int32_t> opened((size_t)n_pack);
    Scratch sc(st);
    double* d_q = sc.get<double>(n_qry * d);
    int32_t* d_face = out_face ? sc.get<int32_t>(n_qry) : nullptr;
    int32_t* d_verts = out_verts ? sc.get<int32_t>(3 * n_qry) : nullptr;
    double* d_bary = out_bary ? sc.get<double>(3 * n_qry) : nullptr;
    double* d_d2 = out_d2 ? sc.get<double>(n_qry) : nullptr;
    int32_t* d_opened = sc.get<int32_t>(n_pack);
    unsigned* keys = sc.get<unsigned>(n_qry);
    int32_t* vals = sc.get<int32_t>(n_qry);
    sc.upload(d_q, qry, n_qry * d);
    if (sc.ok()) {
        k_nd_qry_keys<<<nd_blocks(n_qry), PF_BLOCK, 0, st>>>(d_q, d, n_qry, bb, keys, vals);
        sc.launched();
    }
    const int32_t* perm = sort_by_key(sc, keys, vals, n_qry);
    if (sc.ok()) {
#define PF_ND_LAUNCH(D)                                                                                                          \
    k_closest_nd<D><<<(unsigned)n_pack, PF_WAVE, 0, st>>>(s->tri, s->tri_orig, s->box, s->sbox, s->n_tri, s->n_chunks, s->n_super, d, \
                                                          s->faces, s->vpf, d_q, perm, n_qry, exhaustive ? 1 : 0, d_face, d_verts,   \
                                                          d_bary, d_d2, d_opened)
        switch (d) {
            case 3: PF_ND_LAUNCH(3); break;
            case 4: PF_ND_LAUNCH(4); break;
            case 5: PF_ND_LAUNCH(5); break;
            case 6: PF_ND_LAUNCH(6); break;
            case 8: PF_ND_LAUNCH(8); break;
            case 10: PF_ND_LAUNCH(10); break;
            default: PF_ND_LAUNCH(0); break;
        }
#undef PF_ND_LAUNCH
        sc.launched();
    }
    sc.download(out_face, d_face, n_qry);
    sc.download(out_verts, d_verts, 3 * n_qry);
    sc.download(out_bary, d_bary, 3 * n_qry);
    sc.download(out_d2, d_d2, n_qry);
    sc.download(opened.data(), d_opened, n_pack);
    sc.sync();
    if (!sc.ok()) {
        pf_set_error("pf_surface_nd_closest: %s", hipGetErrorString(sc.err));
        return PF_E_HIP;
    }
    s->last_packets = n_pack;
    s->last_chunks = 0;
    for (int32_t c : opened) s->last_chunks += c;
    return PF_OK;
}

int pf_surface_nd_last_search(pf_surface_nd* s, int64_t* chunks_opened, int64_t* packets, int64_t* n_chunks) {
    PF_CHECK(s, PF_E_ARG, "pf_surface_nd_last_search: NULL argument");
    if (chunks_opened) *chunks_opened = s->last_chunks;
    if (packets) *packets = s->last_packets;
    if (n_chunks) *n_chunks = s->n_chunks;
    return PF_OK;
}

}  // extern "C"
