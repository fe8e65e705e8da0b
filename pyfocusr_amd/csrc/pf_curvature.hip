// Discrete curvatures of a triangle mesh (pf_curvatures): per vertex the barycentric area, the Gaussian curvature (angle
// defect), the signed mean curvature (dihedral angles), the principal curvatures derived from the two, the edge-based
// curvature tensor with its principal curvatures and directions, the unit vertex normal and a boundary mask.  The
// definitions are in include/pyfocusr_hip.h; tests/_curvature_ref.py restates them in numpy.
//
// The structure is the half-edge pass of pf_halfedge.h, as in the signed distances of pf_surface.hip: the half-edges
// sorted by their edge's key are walked one run per edge, sorted by their corner's vertex one run per vertex.  The
// triangle pass, the run walks and the edge counts are that header's; the kernels here add what is curvature's own.
//   k_curv_triangles  one thread per triangle: unit normal, corner angles, area; keys and values of both sorts
//   k_curv_edges      one thread per run of equal edge keys: |e| beta_e and the unit edge vector, written to each of the
//                     run's half-edges; whether the edge is a boundary edge; the four edge counts
//   k_curv_vertices   one thread per vertex over its run: every sum in ascending h, then the derived fields in registers
// Every floating-point sum has a fixed order and the counts are integer atomics: two calls give the same bits.
// Arithmetic: separate multiplies and adds (-ffp-contract=off), dot products left to right.
#include <cmath>

#include "pf_halfedge.h"

namespace {

constexpr double PF_TWO_PI = 6.283185307179586;

// one thread per triangle: he_triangle, with the area
__global__ __launch_bounds__(PF_BLOCK) void k_curv_triangles(const double* __restrict__ pts, const int32_t* __restrict__ faces,
                                                             int64_t n_tri, int nb, double* __restrict__ tnrm,
                                                             double* __restrict__ tang, double* __restrict__ tarea,
                                                             unsigned long long* __restrict__ ekey, unsigned* __restrict__ vkey,
                                                             int32_t* __restrict__ hval) {
    const int64_t t = (int64_t)blockIdx.x * PF_BLOCK + threadIdx.x;
    if (t >= n_tri) return;
    const int32_t v[3] = {faces[3 * t], faces[3 * t + 1], faces[3 * t + 2]};
    he_triangle(pts, v, t, nb, tnrm, tang, tarea, ekey, vkey, hval);
}

// One thread per edge: the first half-edge of each run of equal keys; a run is in ascending h, the sort being stable, so
// its first half-edge belongs to the lower-numbered triangle f.  For an edge of exactly two triangles with areas that
// traverse it in opposite directions, with f going a -> b: e = (x_b - x_a) / |x_b - x_a| and
// beta = atan2((n_f x n_g) . e, n_f . n_g); every other edge has beta = 0 and e = 0.  wb = |e| beta and e go to each
// half-edge of the run, bnd says whether the run is a single half-edge.  counts: he_count_edge.
__global__ __launch_bounds__(PF_BLOCK) void k_curv_edges(const unsigned long long* __restrict__ ekey, const int32_t* __restrict__ hedge,
                                                         int64_t n_half, const double* __restrict__ pts,
                                                         const int32_t* __restrict__ faces, const double* __restrict__ tnrm,
                                                         const double* __restrict__ tarea, double* __restrict__ wb,
                                                         double* __restrict__ evec, uint8_t* __restrict__ bnd,
                                                         unsigned long long* __restrict__ counts) {
    const int64_t i = (int64_t)blockIdx.x * PF_BLOCK + threadIdx.x;
    const int64_t end = he_run_end(ekey, n_half, i);
    if (end == i) return;
    const int64_t m = end - i;
    double w = 0.0, e[3] = {0.0, 0.0, 0.0};
    bool fwd0 = false, fwd1 = false;
    if (m == 2) {
        const int32_t h0 = hedge[i], h1 = hedge[i + 1];
        const int64_t t0 = h0 / 3, t1 = h1 / 3;
        const int j0 = h0 % 3, j1 = h1 % 3;
        const int32_t a0 = faces[3 * t0 + j0], b0 = faces[3 * t0 + he_next(j0)];
        const int32_t a1 = faces[3 * t1 + j1], b1 = faces[3 * t1 + he_next(j1)];
        fwd0 = a0 < b0, fwd1 = a1 < b1;
        if (fwd0 != fwd1 && tarea[t0] > 0.0 && tarea[t1] > 0.0) {
            const double d[3] = {pts[3 * (int64_t)b0] - pts[3 * (int64_t)a0], pts[3 * (int64_t)b0 + 1] - pts[3 * (int64_t)a0 + 1],
                                 pts[3 * (int64_t)b0 + 2] - pts[3 * (int64_t)a0 + 2]};
            const double len = sqrt(dot3(d, d));
            if (len > 0.0 && std::isfinite(len)) {
                const double nf[3] = {tnrm[3 * t0], tnrm[3 * t0 + 1], tnrm[3 * t0 + 2]};
                const double ng[3] = {tnrm[3 * t1], tnrm[3 * t1 + 1], tnrm[3 * t1 + 2]};
                double c[3];
                cross3(nf, ng, c);
#pragma unroll
                for (int a = 0; a < 3; ++a) e[a] = d[a] / len;
                w = len * atan2(dot3(c, e), dot3(nf, ng));
            }
        }
    }
    he_count_edge(counts, m, fwd0, fwd1);
    for (int64_t k = i; k < end; ++k) {
        const int64_t h = hedge[k];
        wb[h] = w;
        bnd[h] = m == 1 ? 1 : 0;
#pragma unroll
        for (int a = 0; a < 3; ++a) evec[3 * h + a] = e[a];
    }
}

// v with its largest-|component| entry positive (lowest index on ties)
__device__ __forceinline__ void sign_rule(double v[3]) {
    int k = 0;
    if (fabs(v[1]) > fabs(v[k])) k = 1;
    if (fabs(v[2]) > fabs(v[k])) k = 2;
    if (v[k] < 0.0) v[0] = -v[0], v[1] = -v[1], v[2] = -v[2];
}

// One thread per vertex, over the half-edges that leave it in ascending h: area, angle sum, angle-weighted normal, sum of
// |e| beta, tensor sum; then K, H, the principal curvatures from (H, K), the tensor in the tangent frame (t1, t2) of the
// unit normal and its closed-form 2 x 2 decomposition.  A vertex without area gets zeros everywhere; one without a
// finite non-zero normal gets a zero normal, zero tensor curvatures and zero directions.  A vertex is a boundary vertex
// when a half-edge that leaves it, or the one that arrives at it in the same triangle, is its edge's only one.
__global__ __launch_bounds__(PF_BLOCK) void k_curv_vertices(const unsigned* __restrict__ vkey, const int32_t* __restrict__ hedge,
                                                            int64_t n_half, int64_t n_points, const double* __restrict__ tnrm,
                                                            const double* __restrict__ tang, const double* __restrict__ tarea,
                                                            const double* __restrict__ wb, const double* __restrict__ evec,
                                                            const uint8_t* __restrict__ bnd, double* __restrict__ out_area,
                                                            double* __restrict__ out_gauss, double* __restrict__ out_mean,
                                                            double* __restrict__ out_tensor, double* __restrict__ out_k,
                                                            double* __restrict__ out_dirs, double* __restrict__ out_nrm,
                                                            uint8_t* __restrict__ out_bnd, unsigned long long* __restrict__ counts) {
    const int64_t v = (int64_t)blockIdx.x * PF_BLOCK + threadIdx.x;
    if (v >= n_points) return;
    int64_t lo = he_vertex_run(vkey, n_half, v);
    double asum = 0.0, angsum = 0.0, hsum = 0.0, ns[3] = {0.0, 0.0, 0.0}, T[6] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
    bool boundary = false;
    for (; lo < n_half && vkey[lo] == (unsigned)v; ++lo) {
        const int64_t h = hedge[lo], t = h / 3;
        const int j = (int)(h - 3 * t);
        const double ang = tang[h], w = wb[h], c = 0.5 * w;
        const double e[3] = {evec[3 * h], evec[3 * h + 1], evec[3 * h + 2]};
        asum += tarea[t];
        angsum += ang;
        hsum += w;
#pragma unroll
        for (int a = 0; a < 3; ++a) ns[a] += ang * tnrm[3 * t + a];
        T[0] += (c * e[0]) * e[0], T[1] += (c * e[1]) * e[1], T[2] += (c * e[2]) * e[2];
        T[3] += (c * e[0]) * e[1], T[4] += (c * e[0]) * e[2], T[5] += (c * e[1]) * e[2];
        boundary = boundary || bnd[h] || bnd[3 * t + he_prev(j)];
    }
    const double A = asum / 3.0;
    const bool have = A > 0.0;
    double K = 0.0, H = 0.0, k[4] = {0.0, 0.0, 0.0, 0.0}, d[6] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0}, n[3] = {0.0, 0.0, 0.0};
    if (have) {
        K = (PF_TWO_PI - angsum) / A;
        H = hsum / (4.0 * A);
#pragma unroll
        for (int a = 0; a < 6; ++a) T[a] = T[a] / A;
        double disc = H * H - K;
        if (disc < 0.0) {
            disc = 0.0;
            atomicAdd(&counts[4], 1ull);
        }
        const double s = sqrt(disc);
        k[0] = H - s, k[1] = H + s;
        const double nl = sqrt(dot3(ns, ns));
        if (nl > 0.0 && std::isfinite(nl)) {
#pragma unroll
            for (int a = 0; a < 3; ++a) n[a] = ns[a] / nl;
            int ax = 0;  // the coordinate axis the normal has the least of
            if (fabs(n[1]) < fabs(n[ax])) ax = 1;
            if (fabs(n[2]) < fabs(n[ax])) ax = 2;
            const double na = ax == 0 ? n[0] : (ax == 1 ? n[1] : n[2]);
            double t1[3] = {(ax == 0 ? 1.0 : 0.0) - na * n[0], (ax == 1 ? 1.0 : 0.0) - na * n[1], (ax == 2 ? 1.0 : 0.0) - na * n[2]};
            const double tl = sqrt(dot3(t1, t1));
#pragma unroll
            for (int a = 0; a < 3; ++a) t1[a] = t1[a] / tl;
            double t2[3];
            cross3(n, t1, t2);
            const double Tt1[3] = {T[0] * t1[0] + T[3] * t1[1] + T[4] * t1[2], T[3] * t1[0] + T[1] * t1[1] + T[5] * t1[2],
                                   T[4] * t1[0] + T[5] * t1[1] + T[2] * t1[2]};
            const double Tt2[3] = {T[0] * t2[0] + T[3] * t2[1] + T[4] * t2[2], T[3] * t2[0] + T[1] * t2[1] + T[5] * t2[2],
                                   T[4] * t2[0] + T[5] * t2[1] + T[2] * t2[2]};
            const double s11 = dot3(t1, Tt1), s12 = dot3(t2, Tt1), s22 = dot3(t2, Tt2);
            const double mid = (s11 + s22) / 2.0, dif = (s11 - s22) / 2.0;
            const double r = sqrt(dif * dif + s12 * s12);
            const double theta = 0.5 * atan2(2.0 * s12, s11 - s22);
            const double ct = cos(theta), st = sin(theta);
            k[2] = mid - r, k[3] = mid + r;
            double wv[3] = {ct * t1[0] + st * t2[0], ct * t1[1] + st * t2[1], ct * t1[2] + st * t2[2]};
            double dm[3];
            cross3(n, wv, dm);
            sign_rule(wv);
            sign_rule(dm);
#pragma unroll
            for (int a = 0; a < 3; ++a) d[a] = wv[a], d[3 + a] = dm[a];
        }
    } else {
#pragma unroll
        for (int a = 0; a < 6; ++a) T[a] = 0.0;
    }
    if (out_area) out_area[v] = have ? A : 0.0;
    if (out_gauss) out_gauss[v] = K;
    if (out_mean) out_mean[v] = H;
    if (out_tensor)
#pragma unroll
        for (int a = 0; a < 6; ++a) out_tensor[6 * v + a] = T[a];
    if (out_k)
#pragma unroll
        for (int a = 0; a < 4; ++a) out_k[4 * v + a] = k[a];
    if (out_dirs)
#pragma unroll
        for (int a = 0; a < 6; ++a) out_dirs[6 * v + a] = d[a];
    if (out_nrm)
#pragma unroll
        for (int a = 0; a < 3; ++a) out_nrm[3 * v + a] = n[a];
    if (out_bnd) out_bnd[v] = boundary ? 1 : 0;
}

}  // namespace

extern "C" int pf_curvatures(pf_ctx* ctx, const double* pts, int64_t n, const int32_t* faces, int64_t n_faces, double* out_area,
                             double* out_gauss, double* out_mean, double* out_tensor6, double* out_kminmax, double* out_dirs,
                             double* out_normals, uint8_t* out_boundary, int64_t* topology, double* device_ms) {
    PF_CHECK(ctx && pts && faces, PF_E_ARG, "pf_curvatures: NULL argument");
    PF_CHECK(n > 0 && n < ((int64_t)1 << 31), PF_E_ARG, "pf_curvatures: n = %lld out of range", (long long)n);
    PF_CHECK(n_faces > 0 && 3 * n_faces < ((int64_t)1 << 31), PF_E_ARG, "pf_curvatures: %lld faces out of range (3 n_faces < 2^31)",
             (long long)n_faces);
    const int64_t T = n_faces, H = 3 * T;
    PF_TRY(pf_check_faces("pf_curvatures", faces, T, 3, n, false));
    const int nb = pf_index_bits(n);  // bits of a vertex index
    PF_HIP(hipSetDevice(ctx->device));
    hipStream_t st = ctx->stream;
    StreamTimer timer(device_ms != nullptr);
    unsigned long long counts[5] = {0, 0, 0, 0, 0};
    hipError_t err;
    {
        Scratch sc(st);
        double* d_pts = sc.get<double>(3 * n);
        int32_t* d_faces = sc.get<int32_t>(H);
        double *tnrm = sc.get<double>(3 * T), *tang = sc.get<double>(H), *tarea = sc.get<double>(T);
        double *wb = sc.get<double>(H), *evec = sc.get<double>(3 * H);
        uint8_t* bnd = sc.get<uint8_t>(H);
        unsigned long long *ek0 = sc.get<unsigned long long>(H), *ek1 = sc.get<unsigned long long>(H);
        unsigned *vk0 = sc.get<unsigned>(H), *vk1 = sc.get<unsigned>(H);
        int32_t *h0 = sc.get<int32_t>(H), *h1 = sc.get<int32_t>(H);
        unsigned long long* cnt = sc.get<unsigned long long>(5);
        // the outputs the caller asked for, one block each: the kernel skips a NULL one
        double* o_area = out_area ? sc.get<double>(n) : nullptr;
        double* o_gauss = out_gauss ? sc.get<double>(n) : nullptr;
        double* o_mean = out_mean ? sc.get<double>(n) : nullptr;
        double* o_tensor = out_tensor6 ? sc.get<double>(6 * n) : nullptr;
        double* o_k = out_kminmax ? sc.get<double>(4 * n) : nullptr;
        double* o_dirs = out_dirs ? sc.get<double>(6 * n) : nullptr;
        double* o_nrm = out_normals ? sc.get<double>(3 * n) : nullptr;
        uint8_t* o_bnd = out_boundary ? sc.get<uint8_t>(n) : nullptr;
        sc.upload(d_pts, pts, 3 * n);
        sc.upload(d_faces, faces, H);
        sc.zero(cnt, sizeof(unsigned long long) * 5);
        timer.start(sc);
        if (sc.ok()) {
            k_curv_triangles<<<pf_blocks(T), PF_BLOCK, 0, st>>>(d_pts, d_faces, T, nb, tnrm, tang, tarea, ek0, vk0, h0);
            sc.launched();
        }
        // both sorts are stable and start from half-edge order: equal keys stay in ascending h.  They share the value
        // arrays, and the stream runs the vertex sort after k_curv_edges has read the edge sort's h1.
        pf_sort_pairs(sc, ek0, ek1, h0, h1, H, 2 * nb);
        if (sc.ok()) {
            k_curv_edges<<<pf_blocks(H), PF_BLOCK, 0, st>>>(ek1, h1, H, d_pts, d_faces, tnrm, tarea, wb, evec, bnd, cnt);
            sc.launched();
        }
        pf_sort_pairs(sc, vk0, vk1, h0, h1, H, nb);
        if (sc.ok()) {
            k_curv_vertices<<<pf_blocks(n), PF_BLOCK, 0, st>>>(vk1, h1, H, n, tnrm, tang, tarea, wb, evec, bnd, o_area, o_gauss, o_mean,
                                                               o_tensor, o_k, o_dirs, o_nrm, o_bnd, cnt);
            sc.launched();
        }
        timer.stop(sc);
        sc.download(out_area, o_area, n);
        sc.download(out_gauss, o_gauss, n);
        sc.download(out_mean, o_mean, n);
        sc.download(out_tensor6, o_tensor, 6 * n);
        sc.download(out_kminmax, o_k, 4 * n);
        sc.download(out_dirs, o_dirs, 6 * n);
        sc.download(out_normals, o_nrm, 3 * n);
        sc.download(out_boundary, o_bnd, n);
        sc.download(counts, cnt, 5);
        sc.sync();
        timer.read(sc, device_ms);
        err = sc.err;
    }
    if (err != hipSuccess) return pf_hip_failed("pf_curvatures", err);
    if (topology)
        for (int k = 0; k < 5; ++k) topology[k] = (int64_t)counts[k];
    return PF_OK;
}
