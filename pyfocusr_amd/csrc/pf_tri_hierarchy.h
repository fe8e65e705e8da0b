// The triangle hierarchy under every surface query (pf_surface.hip: d = 3; pf_surface_nd.hip: 1 <= d <= 16), and the
// device helpers its searches share (the wave reductions and the tie rule `better` are pf_wave.h's).  Built in
// pf_tri_hierarchy.hip (pf_tri_hierarchy_build, declared in pf_internal.h).
//
// Structure.  The fan triangles (0, j+1, j+2) of the faces are sorted along a Morton curve of their centroids (hipCUB
// radix sort, stable) and cut into chunks of PF_TRI_CHUNK = 64 consecutive ones, each with its d-dimensional bounding
// box lo[d] | hi[d]; 64 consecutive chunks form a super-chunk with its own box (two levels are enough: 500k triangles =
// 7813 chunks = 123 super-chunks, two per lane).  Coordinates are stored SoA, [corner][coordinate][triangle], so a wave
// reads 64 consecutive triangles coalesced.  The Morton key takes 10 bits from each of the LEADING min(d, 3) coordinates
// only.  Spectral coordinates come ordered by eigenvalue: the first ones are the smoothest eigenfunctions and carry the
// coarse geometry of the surface, the later ones oscillate and would scatter neighbours along the curve; three
// coordinates at 10 bits fill the 30-bit key, and a 2-manifold needs no more to be cut into compact pieces.  The key only
// decides which triangles share a chunk, that is how tight the boxes are; the boxes span all d coordinates and no
// closest-point result depends on the order (the winding sums do: their order is the triangles').
//
// Exactness of the closest-point searches (k_closest, k_distance, k_closest_nd).  The result of a query is the minimum
// over ALL fan triangles of the exact point-triangle squared distance, lowest fan-triangle index on exact ties (better),
// NaN distances never winning - what a brute-force scan computes.  A search skips (a) a super-chunk or chunk whose box is
// farther from the query, or from the box of a packet of queries, than the bound (the query's best distance so far; for
// a packet the largest of its queries') times PF_BOX_SLACK, (b) in a packet, a chunk farther than that from every single
// query, (c) a triangle whose own box is farther than the query's best x slack.  A box contains its triangles, a
// packet's box its queries, so in exact arithmetic each of these distances is a lower bound of the point-triangle
// distance, and what is skipped is strictly farther than a triangle already found: it can neither win nor tie.  In
// floating point the argument is monotone rounding, not an error bound relative to d2 (d2 is computed from a ROUNDED
// closest point c, whose absolute error is about eps |coordinate|: against d2 that is eps |coordinate| / distance, which
// no fixed slack covers in a frame far from the origin).  Per coordinate k the box term e_k = max(lo_k - p_k,
// p_k - hi_k, 0) and the exact test's p_k - c_k are each ONE rounded subtraction from the same p_k.  If lo_k <= c_k <=
// hi_k then |p_k - c_k| >= e_k as real numbers, rounding keeps that order, and squaring and adding non-negative terms
// left to right keep it too: the COMPUTED d2 of a triangle is never below the COMPUTED distance of a box that holds
// its computed closest point, with no slack at all.  c is in every box of its triangle (a) when it is a corner: the
// vertex regions return the stored coordinates; (b) on an edge, a + v ab with 0 <= v <= 1, and in the face,
// (a + ab v) + ac w with v, w, v + w in [0, 1], whenever the differences ab, ac are exact: then every partial sum lies
// between two stored corner coordinates as a real number and rounding cannot carry it past a representable bound.  ab
// and ac ARE exact when a triangle's coordinates share a binade (Sterbenz), which is the case of every triangle in a
// frame whose offset is large against the mesh - the far frame is the safe one.  Only where corners differ in sign or
// by more than a factor 2 in some coordinate (meshes around the origin) can c_k leave [lo_k, hi_k], by at most about one
// ulp u of the larger corner coordinate and only if the exact closest point is within u of that face of the box (v, or
// v + w, within eps of 1); d2 then falls short of the box distance by at most 2 u x distance, relatively 2 u /
// distance, and PF_BOX_SLACK = 1 + 1e-9 covers that for every query farther than 4.5e-7 of that coordinate from the
// surface.  Nearer than that, and with the exact point within an ulp of a box face that the query lies beyond, this
// argument does not decide; no such query is known (tests/test_surface_hostile.py and the sweeps
// tests/fuzz_surfaces.py, tests/fuzz_surface_nd.py compare with brute force bit for bit in frames up to 1e6 extents
// out, on needles, coincident sheets and queries from rounding distance outwards; profiles/surface_fuzz.md).  A
// triangle within the slack is tested, not skipped.  Bounds only shrink, so a test made against an older, larger bound
// errs on the side of testing.  Lanes and waves of a query merge with the same (d2, index) rule.
//
// Depth.  Every helper that loops over coordinates is templated on D: the depth it is compiled for (loops unrolled, d
// ignored), or D = 0 for any d <= PF_ND_MAX, unrolled to 16 behind the uniform guard k < d so that no array is indexed at
// run time.
#pragma once
#include <limits>

#include "pf_internal.h"
#include "pf_wave.h"

constexpr int PF_TRI_CHUNK = 64;             // triangles per chunk: one per lane and scan
constexpr double PF_BOX_SLACK = 1.0 + 1e-9;  // a box test must never reject on a rounding error (see above)

#define PF_FOR_DEPTH(k) _Pragma("unroll") for (int k = 0; k < (D ? D : PF_ND_MAX); ++k) if (D != 0 || k < d)

// corners of fan triangle t = face * (vpf - 2) + fan position
__device__ __forceinline__ void tri_corners(const int32_t* __restrict__ faces, int32_t vpf, int64_t t, int32_t v[3]) {
    const int32_t per = vpf - 2;
    const int64_t f = t / per;
    const int32_t j = (int32_t)(t - f * per);
    v[0] = faces[f * vpf];
    v[1] = faces[f * vpf + j + 1];
    v[2] = faces[f * vpf + j + 2];
}

// Squared distances to a box bx = lo[d] | hi[d], 0 inside: of a point; of a box lo | hi (never larger than the former
// for any point of that box); of that box's centre
template <int D>
__device__ __forceinline__ double box_dist2(const double* p, const double* __restrict__ bx, int d = D) {
    double s = 0.0;
    PF_FOR_DEPTH(k) {
        const double e = fmax(fmax(bx[k] - p[k], p[k] - bx[d + k]), 0.0);
        s += e * e;
    }
    return s;
}

template <int D>
__device__ __forceinline__ double boxbox_dist2(const double* lo, const double* hi, const double* __restrict__ bx, int d = D) {
    double s = 0.0;
    PF_FOR_DEPTH(k) {
        const double e = fmax(fmax(bx[k] - hi[k], lo[k] - bx[d + k]), 0.0);
        s += e * e;
    }
    return s;
}

template <int D>
__device__ __forceinline__ double centre_dist2(const double* lo, const double* hi, const double* __restrict__ bx, int d = D) {
    double s = 0.0;
    PF_FOR_DEPTH(k) {
        const double ctr = 0.5 * (lo[k] + hi[k]);
        const double e = fmax(fmax(bx[k] - ctr, ctr - bx[d + k]), 0.0);
        s += e * e;
    }
    return s;
}

// The seed of a search, for a whole wave: the nearest super-chunk, then the nearest chunk inside it, by dist(box) (one
// box per lane), lowest index on ties; n_chunks when there is none (a NaN point, no finite box).  Only a heuristic for a
// good first bound.  Every lane returns the same.
template <int D, class Dist>
__device__ __forceinline__ int64_t nearest_chunk(Dist dist, const double* __restrict__ box, const double* __restrict__ sbox,
                                                 int64_t n_chunks, int64_t n_super, int lane, int d = D) {
    const double inf = std::numeric_limits<double>::infinity();
    double nd = inf;
    int64_t ns = n_super;  // sentinel: none
    for (int64_t s = lane; s < n_super; s += PF_WAVE) {
        const double e = dist(sbox + 2 * d * s);
        if (e < nd) nd = e, ns = s;
    }
    wave_argmin(nd, ns);
    int64_t c0 = n_chunks;
    if (ns < n_super) {
        c0 = ns * PF_WAVE + lane;
        nd = c0 < n_chunks ? dist(box + 2 * d * c0) : inf;
        if (!(nd < inf)) c0 = n_chunks;
        wave_argmin(nd, c0);
    }
    return c0;
}
