// Distortion and coverage of a correspondence as a map between surfaces (pf_map_distortion): per source face the two
// singular values of the linear map onto its image triangle, the area ratio and whether the image is collapsed or turned
// over; per source vertex the area-weighted means and the flags of its faces; per target vertex how many source vertices
// it owns and their area; the totals.  The definitions are in include/pyfocusr_hip.h; tests/_map_quality_ref.py restates
// them in numpy.
//
//   k_mq_images    one thread per source vertex: the image point, the image normal, the owner as the key of the coverage
//                  sort (n_tgt for an unmapped vertex: behind every owner)
//   k_mq_faces     one thread per source face: the singular values, the area ratio, the flags, the seven terms of the
//                  totals, the vertex sort's keys and values (half-edge h = 3 t + j under its corner's vertex, as
//                  pf_halfedge.h has them), the five face counts
//   k_mq_vertices  one thread per source vertex over the run of the half-edges that leave it, in ascending h (the run is
//                  found as pf_curvature.hip finds it): area, weighted means, flags; the count of flipped vertices
//   k_mq_coverage  one thread per target vertex over the run of the source vertices it owns, in ascending index: the
//                  count, and their area in runs of 64 summed left to right, the run sums added left to right
//   k_mq_level x 3 the totals along the fixed tree: 256 consecutive terms, 256 of those sums, the rest in order
// Two stable radix sorts (pf_sort.hip): the half-edges by vertex, the source vertices by owner.  Every floating-point sum
// has a fixed order, the counts are integer atomics (sums, one maximum): two calls give the same bits.  No kernel waits
// for another block.  Arithmetic: separate multiplies and adds (-ffp-contract=off), dot products left to right.
#include <cmath>

#include "pf_halfedge.h"

namespace {

typedef unsigned long long u64;

constexpr int MQ_RUN = 64;     // owned vertices per run of the coverage's two-level sum
constexpr int MQ_GROUP = 256;  // terms per node of the totals' tree
constexpr int MQ_TERMS = 7;    // totals that are sums (totals[7] is 0)
enum { MQ_VALID = 1, MQ_COLLAPSED = 2, MQ_FLIPPED = 4, MQ_UNMAPPED = 8 };
// counts: valid | collapsed | flipped | invalid | unmapped corner | targets hit | largest count | flipped vertices
enum { MQ_N_VALID, MQ_N_COLLAPSED, MQ_N_FLIPPED, MQ_N_INVALID, MQ_N_UNMAPPED, MQ_N_HIT, MQ_N_MAXCOUNT, MQ_N_VFLIPPED, MQ_N_COUNTS };

// counts[slot] += the lanes of the wave for which `on` holds: one atomic per wave (every lane of the wave calls this)
__device__ __forceinline__ void count_lanes(u64* __restrict__ counts, int slot, bool on) {
    const u64 mask = __ballot(on);
    if (mask != 0ull && (int)(threadIdx.x & (PF_WAVE - 1)) == __ffsll((long long)mask) - 1) atomicAdd(&counts[slot], (u64)__popcll(mask));
}

// One thread per source vertex i.  c == 1: y = tgt[T]; c == 3: y = (w0 x_a + w1 x_b) + w2 x_c per coordinate, the normal
// likewise; the owner is T, or the corner with the largest weight (the lowest corner on ties).  An unmapped vertex (first
// map vertex -1) gets a zero image and the key n_tgt.
__global__ __launch_bounds__(PF_BLOCK) void k_mq_images(int64_t n_src, const double* __restrict__ tgt, const double* __restrict__ tnrm,
                                                        int64_t n_tgt, const int32_t* __restrict__ mapv, const double* __restrict__ mapw,
                                                        int c, double* __restrict__ img, double* __restrict__ imgn,
                                                        unsigned* __restrict__ okey, int32_t* __restrict__ oval) {
    const int64_t i = (int64_t)blockIdx.x * PF_BLOCK + threadIdx.x;
    if (i >= n_src) return;
    double y[3] = {0.0, 0.0, 0.0}, m[3] = {0.0, 0.0, 0.0};
    unsigned owner = (unsigned)n_tgt;
    const int64_t a = mapv[c * i];
    if (a >= 0) {
        if (c == 1) {
            owner = (unsigned)a;
#pragma unroll
            for (int k = 0; k < 3; ++k) y[k] = tgt[3 * a + k];
            if (tnrm)
#pragma unroll
                for (int k = 0; k < 3; ++k) m[k] = tnrm[3 * a + k];
        } else {
            const int64_t b = mapv[3 * i + 1], d = mapv[3 * i + 2];
            const double w0 = mapw[3 * i], w1 = mapw[3 * i + 1], w2 = mapw[3 * i + 2];
            int best = 0;
            if (w1 > w0) best = 1;
            if (w2 > (best == 0 ? w0 : w1)) best = 2;
            owner = (unsigned)(best == 0 ? a : (best == 1 ? b : d));
#pragma unroll
            for (int k = 0; k < 3; ++k) y[k] = (w0 * tgt[3 * a + k] + w1 * tgt[3 * b + k]) + w2 * tgt[3 * d + k];
            if (tnrm)
#pragma unroll
                for (int k = 0; k < 3; ++k) m[k] = (w0 * tnrm[3 * a + k] + w1 * tnrm[3 * b + k]) + w2 * tnrm[3 * d + k];
        }
    }
#pragma unroll
    for (int k = 0; k < 3; ++k) img[3 * i + k] = y[k];
    if (imgn)
#pragma unroll
        for (int k = 0; k < 3; ++k) imgn[3 * i + k] = m[k];
    okey[i] = owner;
    oval[i] = (int32_t)i;
}

// One thread per source face.  harea[t] = a_s / 2 of a face whose a_s is finite and not 0, mapped or not (the vertex area
// is the source's own); sigma, ratio, flags and the terms as the header defines them.  term is [MQ_TERMS][n_tri].
__global__ __launch_bounds__(PF_BLOCK) void k_mq_faces(const double* __restrict__ pts, const int32_t* __restrict__ faces, int64_t n_tri,
                                                       const double* __restrict__ img, const double* __restrict__ imgn,
                                                       const unsigned* __restrict__ okey, unsigned unmapped_key,
                                                       double* __restrict__ harea, double* __restrict__ sigma, double* __restrict__ ratio,
                                                       uint8_t* __restrict__ flags, double* __restrict__ term,
                                                       unsigned* __restrict__ vkey, int32_t* __restrict__ hval, u64* __restrict__ counts) {
    const int64_t t = (int64_t)blockIdx.x * PF_BLOCK + threadIdx.x;
    const bool live = t < n_tri;
    uint8_t fl = 0;
    if (live) {
        const int32_t v[3] = {faces[3 * t], faces[3 * t + 1], faces[3 * t + 2]};
        double x[3][3], y[3][3];
#pragma unroll
        for (int c = 0; c < 3; ++c)
#pragma unroll
            for (int a = 0; a < 3; ++a) x[c][a] = pts[3 * (int64_t)v[c] + a], y[c][a] = img[3 * (int64_t)v[c] + a];
        const bool mapped = okey[v[0]] != unmapped_key && okey[v[1]] != unmapped_key && okey[v[2]] != unmapped_key;
        const double u[3] = {x[1][0] - x[0][0], x[1][1] - x[0][1], x[1][2] - x[0][2]};
        const double w[3] = {x[2][0] - x[0][0], x[2][1] - x[0][1], x[2][2] - x[0][2]};
        const double U[3] = {y[1][0] - y[0][0], y[1][1] - y[0][1], y[1][2] - y[0][2]};
        const double W[3] = {y[2][0] - y[0][0], y[2][1] - y[0][1], y[2][2] - y[0][2]};
        double cs[3], ci[3];
        cross3(u, w, cs);
        cross3(U, W, ci);
        const double as = sqrt(dot3(cs, cs)), ai = sqrt(dot3(ci, ci));
        const bool area = as > 0.0 && std::isfinite(as);
        const double hs = area ? as / 2.0 : 0.0;
        double s1 = 0.0, s2 = 0.0, ar = 0.0, tm[MQ_TERMS] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
        if (area && mapped) {
            fl = MQ_VALID;
            const double E = dot3(u, u), F = dot3(u, w), G = dot3(w, w);
            const double Ei = dot3(U, U), Fi = dot3(U, W), Gi = dot3(W, W);
            if (ai == 0.0) {
                fl |= MQ_COLLAPSED;
                const double num = (G * Ei - (2.0 * F) * Fi) + E * Gi;
                s1 = sqrt((num < 0.0 ? 0.0 : num) / (as * as));
            } else {
                const double l = sqrt(E), li = sqrt(Ei);
                const double p = li / l;
                const double q = ((Fi * l) / li - (li * F) / l) / as;
                const double s = (ai * l) / (li * as);
                const double hp = (p + s) / 2.0, hm = (p - s) / 2.0, hq = q / 2.0;
                const double Q = sqrt(hp * hp + hq * hq), R = sqrt(hm * hm + hq * hq);
                s1 = Q + R;
                s2 = fabs(Q - R);
                ar = ai / as;
                if (imgn) {
                    double ms[3];
#pragma unroll
                    for (int a = 0; a < 3; ++a)
                        ms[a] = (imgn[3 * (int64_t)v[0] + a] + imgn[3 * (int64_t)v[1] + a]) + imgn[3 * (int64_t)v[2] + a];
                    if (dot3(ci, ms) < 0.0) fl |= MQ_FLIPPED;
                }
            }
            tm[0] = hs;
            tm[1] = ai / 2.0;
            tm[2] = hs * (s1 * s1 + s2 * s2);
            tm[3] = hs * s1;
            tm[4] = hs * s2;
            tm[5] = (fl & MQ_COLLAPSED) ? hs : 0.0;
            tm[6] = (fl & MQ_FLIPPED) ? hs : 0.0;
        } else if (!mapped) {
            fl = MQ_UNMAPPED;
        }
        harea[t] = hs;
        sigma[2 * t] = s1;
        sigma[2 * t + 1] = s2;
        ratio[t] = ar;
        flags[t] = fl;
#pragma unroll
        for (int k = 0; k < MQ_TERMS; ++k) term[k * n_tri + t] = tm[k];
#pragma unroll
        for (int j = 0; j < 3; ++j) {
            vkey[3 * t + j] = (unsigned)v[j];
            hval[3 * t + j] = (int32_t)(3 * t + j);
        }
    }
    count_lanes(counts, MQ_N_VALID, live && (fl & MQ_VALID));
    count_lanes(counts, MQ_N_COLLAPSED, live && (fl & MQ_COLLAPSED));
    count_lanes(counts, MQ_N_FLIPPED, live && (fl & MQ_FLIPPED));
    count_lanes(counts, MQ_N_INVALID, live && !(fl & MQ_VALID));
    count_lanes(counts, MQ_N_UNMAPPED, live && (fl & MQ_UNMAPPED));
}

// One thread per source vertex, over the half-edges that leave it in ascending h: A = (sum a_s / 2) / 3 as pf_curvatures
// has it; the means of sigma over the valid faces, weighted by a_s / 2; the OR of the faces' flags.
__global__ __launch_bounds__(PF_BLOCK) void k_mq_vertices(const unsigned* __restrict__ vkey, const int32_t* __restrict__ hedge, int64_t n_half,
                                                          int64_t n_points, const double* __restrict__ harea, const double* __restrict__ sigma,
                                                          const uint8_t* __restrict__ flags, double* __restrict__ varea,
                                                          double* __restrict__ vsigma, uint8_t* __restrict__ vflags, u64* __restrict__ counts) {
    const int64_t v = (int64_t)blockIdx.x * PF_BLOCK + threadIdx.x;
    const bool live = v < n_points;
    uint8_t fl = 0;
    if (live) {
        double asum = 0.0, wsum = 0.0, n1 = 0.0, n2 = 0.0;
        for (int64_t lo = he_vertex_run(vkey, n_half, v); lo < n_half && vkey[lo] == (unsigned)v; ++lo) {
            const int64_t t = hedge[lo] / 3;
            const double hs = harea[t];
            const uint8_t f = flags[t];
            asum += hs;
            if (f & MQ_VALID) {
                wsum += hs;
                n1 += hs * sigma[2 * t];
                n2 += hs * sigma[2 * t + 1];
            }
            fl |= f;
        }
        const double A = asum / 3.0;
        varea[v] = A > 0.0 ? A : 0.0;
        vsigma[2 * v] = wsum > 0.0 ? n1 / wsum : 0.0;
        vsigma[2 * v + 1] = wsum > 0.0 ? n2 / wsum : 0.0;
        vflags[v] = fl;
    }
    count_lanes(counts, MQ_N_VFLIPPED, live && (fl & MQ_FLIPPED));
}

// One thread per target vertex j, over the run of the sorted owners that equal j (the sort is stable: ascending source
// vertex): the count, and the areas in consecutive runs of MQ_RUN, each summed left to right from 0.0, the run sums added
// left to right from 0.0.
__global__ __launch_bounds__(PF_BLOCK) void k_mq_coverage(const unsigned* __restrict__ okey, const int32_t* __restrict__ member, int64_t n_src,
                                                          int64_t n_tgt, const double* __restrict__ varea, int32_t* __restrict__ count,
                                                          double* __restrict__ premass, u64* __restrict__ counts) {
    const int64_t j = (int64_t)blockIdx.x * PF_BLOCK + threadIdx.x;
    const bool live = j < n_tgt;
    int64_t cnt = 0;
    if (live) {
        const int64_t lo = he_vertex_run(okey, n_src, j);
        double total = 0.0, run = 0.0;
        for (int64_t q = lo; q < n_src && okey[q] == (unsigned)j; ++q, ++cnt) {
            if (cnt && cnt % MQ_RUN == 0) {
                total += run;
                run = 0.0;
            }
            run += varea[member[q]];
        }
        if (cnt) total += run;
        count[j] = (int32_t)cnt;
        premass[j] = total;
        if (cnt) atomicMax(&counts[MQ_N_MAXCOUNT], (u64)cnt);
    }
    count_lanes(counts, MQ_N_HIT, live && cnt > 0);
}

// One level of the totals' tree over MQ_TERMS rows: out[k][i] = in[k][group i .. group (i + 1)) summed left to right from
// 0.0 as far as the row goes; group == 0: the whole row (n_out == 1).
__global__ __launch_bounds__(PF_BLOCK) void k_mq_level(const double* __restrict__ in, int64_t n_in, double* __restrict__ out, int64_t n_out,
                                                       int64_t group) {
    const int64_t g = (int64_t)blockIdx.x * PF_BLOCK + threadIdx.x;
    if (g >= MQ_TERMS * n_out) return;
    const int64_t k = g / n_out, i = g - k * n_out;
    const int64_t lo = group * i, hi = group ? min(lo + group, n_in) : n_in;
    const double* row = in + k * n_in;
    double sum = 0.0;
    for (int64_t q = lo; q < hi; ++q) sum += row[q];
    out[k * n_out + i] = sum;
}

bool finite3(const double* p) { return std::isfinite(p[0]) && std::isfinite(p[1]) && std::isfinite(p[2]); }

// the checks that need the data, before anything is launched: every mapped row's indices, weights and the points and
// normals it reads
int check_map(const double* src_pts, int64_t n_src, const double* tgt_pts, int64_t n_tgt, const double* tgt_normals, const int32_t* mapv,
              const double* mapw, int c) {
    for (int64_t i = 0; i < n_src; ++i) {
        const int32_t* row = mapv + c * i;
        if (row[0] == -1) continue;
        for (int k = 0; k < c; ++k) {
            PF_CHECK(row[k] >= 0 && row[k] < n_tgt, PF_E_ARG, "pf_map_distortion: row %lld maps to vertex %d of %lld", (long long)i, row[k],
                     (long long)n_tgt);
            PF_CHECK(finite3(tgt_pts + 3 * (int64_t)row[k]), PF_E_ARG, "pf_map_distortion: target point %d is not finite", row[k]);
            PF_CHECK(!tgt_normals || finite3(tgt_normals + 3 * (int64_t)row[k]), PF_E_ARG, "pf_map_distortion: target normal %d is not finite",
                     row[k]);
            PF_CHECK(!mapw || std::isfinite(mapw[c * i + k]), PF_E_ARG, "pf_map_distortion: a weight of row %lld is not finite", (long long)i);
        }
        PF_CHECK(finite3(src_pts + 3 * i), PF_E_ARG, "pf_map_distortion: source point %lld is mapped and not finite", (long long)i);
    }
    return PF_OK;
}

}  // namespace

extern "C" int pf_map_distortion(pf_ctx* ctx, const double* src_pts, int64_t n_src, const int32_t* src_faces, int64_t n_faces,
                                 const double* tgt_pts, int64_t n_tgt, const double* tgt_normals, const int32_t* map_vertices,
                                 const double* map_weights, int32_t c, double* face_sigma, double* face_area_ratio, uint8_t* face_flags,
                                 double* vertex_area, double* vertex_sigma, uint8_t* vertex_flags, int32_t* target_count,
                                 double* target_premass, double* totals, int64_t* report, double* device_ms) {
    PF_CHECK(ctx && src_pts && src_faces && tgt_pts && map_vertices, PF_E_ARG, "pf_map_distortion: NULL argument");
    PF_CHECK(c == 1 || c == 3, PF_E_ARG, "pf_map_distortion: c = %d, a map row has 1 or 3 vertices", (int)c);
    PF_CHECK(c == 1 || map_weights, PF_E_ARG, "pf_map_distortion: a map of 3 corners needs its weights");
    PF_CHECK(n_src > 0 && n_src < ((int64_t)1 << 31), PF_E_ARG, "pf_map_distortion: n_src = %lld out of range", (long long)n_src);
    PF_CHECK(n_tgt > 0 && n_tgt < ((int64_t)1 << 31), PF_E_ARG, "pf_map_distortion: n_tgt = %lld out of range", (long long)n_tgt);
    PF_CHECK(n_faces > 0 && 3 * n_faces < ((int64_t)1 << 31), PF_E_ARG, "pf_map_distortion: %lld faces out of range (3 n_faces < 2^31)",
             (long long)n_faces);
    const int64_t T = n_faces, H = 3 * T;
    PF_TRY(pf_check_faces("pf_map_distortion", src_faces, T, 3, n_src, true));
    const double* mapw = c == 3 ? map_weights : nullptr;
    PF_TRY(check_map(src_pts, n_src, tgt_pts, n_tgt, tgt_normals, map_vertices, mapw, c));
    const int nb = pf_index_bits(n_src);      // bits of a source vertex
    const int ob = pf_index_bits(n_tgt + 1);  // bits of an owner and of the value n_tgt
    const int64_t n1 = (T + MQ_GROUP - 1) / MQ_GROUP, n2 = (n1 + MQ_GROUP - 1) / MQ_GROUP;
    PF_HIP(hipSetDevice(ctx->device));
    hipStream_t st = ctx->stream;
    StreamTimer timer(device_ms != nullptr);
    u64 counts[MQ_N_COUNTS] = {0, 0, 0, 0, 0, 0, 0, 0};
    double sums[MQ_TERMS] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
    hipError_t err;
    {
        Scratch sc(st);
        double* d_src = sc.get<double>(3 * n_src);
        int32_t* d_faces = sc.get<int32_t>(H);
        double* d_tgt = sc.get<double>(3 * n_tgt);
        double* d_tnrm = tgt_normals ? sc.get<double>(3 * n_tgt) : nullptr;
        int32_t* d_mapv = sc.get<int32_t>(c * n_src);
        double* d_mapw = mapw ? sc.get<double>(3 * n_src) : nullptr;
        double* img = sc.get<double>(3 * n_src);
        double* imgn = tgt_normals ? sc.get<double>(3 * n_src) : nullptr;
        unsigned *ok0 = sc.get<unsigned>(n_src), *ok1 = sc.get<unsigned>(n_src);
        int32_t *ov0 = sc.get<int32_t>(n_src), *ov1 = sc.get<int32_t>(n_src);
        double *harea = sc.get<double>(T), *sigma = sc.get<double>(2 * T), *ratio = sc.get<double>(T);
        uint8_t* flags = sc.get<uint8_t>(T);
        double *term = sc.get<double>(MQ_TERMS * T), *lev1 = sc.get<double>(MQ_TERMS * n1), *lev2 = sc.get<double>(MQ_TERMS * n2);
        double* d_sums = sc.get<double>(MQ_TERMS);
        unsigned *vk0 = sc.get<unsigned>(H), *vk1 = sc.get<unsigned>(H);
        int32_t *h0 = sc.get<int32_t>(H), *h1 = sc.get<int32_t>(H);
        double *varea = sc.get<double>(n_src), *vsigma = sc.get<double>(2 * n_src);
        uint8_t* vflags = sc.get<uint8_t>(n_src);
        int32_t* count = sc.get<int32_t>(n_tgt);
        double* premass = sc.get<double>(n_tgt);
        u64* cnt = sc.get<u64>(MQ_N_COUNTS);
        sc.upload(d_src, src_pts, 3 * n_src);
        sc.upload(d_faces, src_faces, H);
        sc.upload(d_tgt, tgt_pts, 3 * n_tgt);
        if (d_tnrm) sc.upload(d_tnrm, tgt_normals, 3 * n_tgt);
        sc.upload(d_mapv, map_vertices, c * n_src);
        if (d_mapw) sc.upload(d_mapw, mapw, 3 * n_src);
        sc.zero(cnt, sizeof(u64) * MQ_N_COUNTS);
        timer.start(sc);
        if (sc.ok()) {
            k_mq_images<<<pf_blocks(n_src), PF_BLOCK, 0, st>>>(n_src, d_tgt, d_tnrm, n_tgt, d_mapv, d_mapw, (int)c, img, imgn, ok0, ov0);
            k_mq_faces<<<pf_blocks(T), PF_BLOCK, 0, st>>>(d_src, d_faces, T, img, imgn, ok0, (unsigned)n_tgt, harea, sigma, ratio, flags, term,
                                                          vk0, h0, cnt);
            k_mq_level<<<pf_blocks(MQ_TERMS * n1), PF_BLOCK, 0, st>>>(term, T, lev1, n1, MQ_GROUP);
            k_mq_level<<<pf_blocks(MQ_TERMS * n2), PF_BLOCK, 0, st>>>(lev1, n1, lev2, n2, MQ_GROUP);
            k_mq_level<<<1, PF_BLOCK, 0, st>>>(lev2, n2, d_sums, 1, 0);
            sc.launched();
        }
        // both sorts are stable: the half-edges of a vertex stay in ascending h, the vertices of an owner in ascending index
        pf_sort_pairs(sc, vk0, vk1, h0, h1, H, nb);
        if (sc.ok()) {
            k_mq_vertices<<<pf_blocks(n_src), PF_BLOCK, 0, st>>>(vk1, h1, H, n_src, harea, sigma, flags, varea, vsigma, vflags, cnt);
            sc.launched();
        }
        pf_sort_pairs(sc, ok0, ok1, ov0, ov1, n_src, ob);
        if (sc.ok()) {
            k_mq_coverage<<<pf_blocks(n_tgt), PF_BLOCK, 0, st>>>(ok1, ov1, n_src, n_tgt, varea, count, premass, cnt);
            sc.launched();
        }
        timer.stop(sc);
        sc.download(face_sigma, sigma, 2 * T);
        sc.download(face_area_ratio, ratio, T);
        sc.download(face_flags, flags, T);
        sc.download(vertex_area, varea, n_src);
        sc.download(vertex_sigma, vsigma, 2 * n_src);
        sc.download(vertex_flags, vflags, n_src);
        sc.download(target_count, count, n_tgt);
        sc.download(target_premass, premass, n_tgt);
        sc.download(sums, d_sums, MQ_TERMS);
        sc.download(counts, cnt, MQ_N_COUNTS);
        sc.sync();
        timer.read(sc, device_ms);
        err = sc.err;
    }
    if (err != hipSuccess) return pf_hip_failed("pf_map_distortion", err);
    if (totals) {
        for (int k = 0; k < MQ_TERMS; ++k) totals[k] = sums[k];
        totals[2] = 0.5 * sums[2];
        totals[7] = 0.0;
    }
    if (report) {
        for (int k = 0; k < MQ_N_COUNTS; ++k) report[k] = (int64_t)counts[k];
        if (!tgt_normals) report[MQ_N_FLIPPED] = report[MQ_N_VFLIPPED] = -1;
    }
    return PF_OK;
}
