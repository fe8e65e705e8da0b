// Closest point on a triangulated surface embedded in d dimensions (1 <= d <= 16): face, corners, barycentric weights
// and squared distance for many queries (pf_surface_nd_*).  This is the sub-vertex correspondence of FOCUSR: the target
// mesh is a 2-manifold in spectral coordinates, and a source vertex maps to a point of one of its triangles, not to one
// of its vertices.
//
// Structure (pf_surface_nd_create): the triangle hierarchy of pf_tri_hierarchy.h, the one pf_surface.hip searches at
// d = 3, with its Morton key over the leading min(d, 3) coordinates.
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
// Exactness: pf_tri_hierarchy.h.  The exhaustive mode tests every triangle of every chunk and skips nothing.
//
// Arithmetic, fixed so the host can reproduce every bit (tests/_surface_nd_ref.py): Ericson's region walk (Real-Time
// Collision Detection 5.1.5), operation for operation closest_on_triangle of pf_surface.hip and
// oracle/icp_port.py:closest_point_on_triangles, with every dot product summed left to right over coordinates 0 .. d-1
// and no FMA (-ffp-contract=off); the closest point formed per coordinate as a | b | c | a + v ab | a + w ac |
// b + w (c - b) | (a + ab v) + ac w by region; d2 the sum of squared coordinate differences, left to right.  The weights
// are (1, 0, 0) | (0, 1, 0) | (0, 0, 1) | (1 - v, v, 0) | (1 - w, 0, w) | (0, 1 - w, w) | ((1 - v) - w, v, w).
// No floating-point atomics: two calls give identical bits.
#include <cmath>
#include <limits>

#include "pf_tri_hierarchy.h"

struct pf_surface_nd {
    pf_ctx* ctx = nullptr;
    int64_t n_points = 0, n_faces = 0;
    int32_t vpf = 0;
    TriHierarchy h;               // the fan triangles in h.d coordinates
    int32_t* faces = nullptr;     // [n_faces][vpf] device copy: the corners of the winning triangle
    int64_t last_chunks = 0, last_packets = 0;  // chunks staged / packets of the last search (pf_surface_nd_last_search)
};

namespace {

constexpr int PF_ND_PACKET = 8;   // queries per wave
enum { PF_ND_A = 0, PF_ND_B = 1, PF_ND_C = 2, PF_ND_AB = 3, PF_ND_BC = 4, PF_ND_CA = 5, PF_ND_FACE = 6 };

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
    __shared__ double s_tri[3 * M][PF_TRI_CHUNK];  // one chunk, SoA as in HBM: row = corner * d + coordinate
    __shared__ int32_t s_orig[PF_TRI_CHUNK];
    const int d = D ? D : d_any;
    const int lane = threadIdx.x, sub = lane / PACKET;
    const int64_t i = (int64_t)blockIdx.x * PACKET + (lane % PACKET);
    const bool live = i < n_qry;
    const int64_t qi = live ? perm[i] : -1;  // the caller's index of this lane's query
    const double inf = std::numeric_limits<double>::infinity();
    const double nan = __longlong_as_double(0x7ff8000000000000ll);
    double p[M];
    bool ok = live;
    PF_FOR_DEPTH(k) {
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
    if (__ballot(ok)) {
        double qbest = inf;
        auto scan = [&](int64_t c) {  // stage chunk c in LDS, test its triangles against every query
            const int64_t s = c * PF_TRI_CHUNK + lane;
            const int cnt = (int)(n_tri - c * PF_TRI_CHUNK < PF_TRI_CHUNK ? n_tri - c * PF_TRI_CHUNK : PF_TRI_CHUNK);
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
                    PF_FOR_DEPTH(k) {
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
                    if (!exhaustive && tb > fmin(best_d2, qbest) * PF_BOX_SLACK) continue;
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
                    PF_FOR_DEPTH(k) {
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
                    if (better(dist2, o, best_d2, best_orig)) {  // NaN distances compare false: never win
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
            PF_FOR_DEPTH(k) {
                lo[k] = ok ? p[k] : inf, hi[k] = ok ? p[k] : -inf;
                for (int off = PF_WAVE / 2; off > 0; off >>= 1) {
                    lo[k] = fmin(lo[k], __shfl_xor(lo[k], off, PF_WAVE));
                    hi[k] = fmax(hi[k], __shfl_xor(hi[k], off, PF_WAVE));
                }
            }
            // does any query's own point-box test keep chunk c?
            auto wanted = [&](int64_t c) { return __ballot(ok && box_dist2<D>(p, box + 2 * d * c, d) <= qbest * PF_BOX_SLACK) != 0; };

            // (1) seed: the chunk nearest to the packet's centre
            const int64_t c0 = nearest_chunk<D>([&](const double* __restrict__ bx) { return centre_dist2<D>(lo, hi, bx, d); }, box, sbox,
                                                n_chunks, n_super, lane, d);
            if (c0 < n_chunks) scan(c0);
            double bound = wave_max(ok ? qbest : -inf);  // the packet's bound: its worst query

            // (2) every chunk whose box is within the bound of the packet's box and of some query
            for (int64_t sb = 0; sb < n_super; sb += PF_WAVE) {
                const int64_t s = sb + lane;
                unsigned long long smask = __ballot(s < n_super && boxbox_dist2<D>(lo, hi, sbox + 2 * d * s, d) <= bound * PF_BOX_SLACK);
                while (smask) {
                    const int64_t ss = sb + __ffsll((long long)smask) - 1;
                    smask &= smask - 1;
                    if (boxbox_dist2<D>(lo, hi, sbox + 2 * d * ss, d) > bound * PF_BOX_SLACK) continue;  // the bound has shrunk
                    const int64_t c = ss * PF_WAVE + lane;
                    unsigned long long mask = __ballot(c < n_chunks && c != c0 && boxbox_dist2<D>(lo, hi, box + 2 * d * c, d) <= bound * PF_BOX_SLACK);
                    while (mask) {
                        const int64_t cc = ss * PF_WAVE + __ffsll((long long)mask) - 1;
                        mask &= mask - 1;
                        if (boxbox_dist2<D>(lo, hi, box + 2 * d * cc, d) > bound * PF_BOX_SLACK || !wanted(cc)) continue;
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
        if (better(od, oo, best_d2, best_orig)) best_d2 = od, best_orig = oo, best_b0 = o0, best_b1 = o1, best_b2 = o2;
    }
    if (live && sub == 0) {
        const bool found = ok && best_orig != 0x7fffffff;  // else: a non-finite query, or no triangle with a finite distance
        if (out_face) out_face[qi] = found ? best_orig / (vpf - 2) : -1;
        if (out_verts) {
            int32_t v[3] = {-1, -1, -1};
            if (found) tri_corners(faces, vpf, best_orig, v);
            out_verts[3 * qi] = v[0], out_verts[3 * qi + 1] = v[1], out_verts[3 * qi + 2] = v[2];
        }
        if (out_bary) out_bary[3 * qi] = found ? best_b0 : nan, out_bary[3 * qi + 1] = found ? best_b1 : nan, out_bary[3 * qi + 2] = found ? best_b2 : nan;
        if (out_d2) out_d2[qi] = found ? best_d2 : nan;
    }
    if (lane == 0) opened[blockIdx.x] = n_opened;
}

}  // namespace

extern "C" {

void pf_surface_nd_free(pf_surface_nd* s) {
    if (!s) return;
    hipSetDevice(s->ctx->device);
    hipStreamSynchronize(s->ctx->stream);
    hipStream_t st = s->ctx->stream;
    pf_tri_hierarchy_free(st, s->h);
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
    PF_TRY(pf_check_faces("pf_surface_nd_create", faces, n_faces, vpf, n, false));
    const KeyBox bb = pf_key_box(coords, n, d, false);
    PF_HIP(hipSetDevice(ctx->device));
    hipStream_t st = ctx->stream;
    pf_surface_nd* s = new pf_surface_nd();
    s->ctx = ctx;
    s->n_points = n, s->n_faces = n_faces, s->vpf = vpf;
    hipError_t e;
    {
        Scratch sc(st);
        double* d_pts = sc.get<double>(n * d);
        s->faces = sc.keep<int32_t>(n_faces * vpf);
        sc.upload(d_pts, coords, n * d);
        sc.upload(s->faces, faces, n_faces * vpf);
        pf_tri_hierarchy_build(sc, s->h, d_pts, d, s->faces, n_faces, vpf, bb);
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
    PF_CHECK(n_qry >= 1 && n_qry < ((int64_t)1 << 31) / s->h.d, PF_E_ARG, "pf_surface_nd_closest: n_qry = %lld out of range",
             (long long)n_qry);
    const TriHierarchy& h = s->h;
    const int32_t d = h.d;
    const KeyBox bb = pf_key_box(qry, n_qry, d, true);
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
    sc.upload(d_q, qry, n_qry * d);
    const int32_t* perm = pf_surface_morton_order(sc, d_q, d, nullptr, 0, n_qry, bb);
    if (sc.ok()) {
#define PF_ND_LAUNCH(D)                                                                                                       \
    k_closest_nd<D><<<(unsigned)n_pack, PF_WAVE, 0, st>>>(h.tri, h.tri_orig, h.box, h.sbox, h.n_tri, h.n_chunks, h.n_super, d, s->faces, \
                                                          s->vpf, d_q, perm, n_qry, exhaustive ? 1 : 0, d_face, d_verts, d_bary, d_d2, \
                                                          d_opened)
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
    if (n_chunks) *n_chunks = s->h.n_chunks;
    return PF_OK;
}

}  // extern "C"
