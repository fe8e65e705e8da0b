// Cotangent Laplace-Beltrami operator of a triangle mesh, assembled on the device.
//
// The reference has no counterpart: its Laplacian weighs an edge by 1 / length and measures the
// triangulation.  This is the FEM discretisation of the surface's own operator (Pinkall & Polthier 1993; Meyer et al. 2003):
//   w_ij = 1/2 sum over the faces that contain the undirected edge (i, j) of cot(angle opposite the edge),
//   d_i  = sum_j w_ij,  m_i = 1/3 sum of the areas of the faces at i (lumped barycentric mass),
//   L = M^-1 (D - W), solved through the symmetric S = M^-1/2 (D - W) M^-1/2 (same spectrum, eigenvectors M^1/2 phi).
// Per corner p with edge vectors u, v: cot = (u . v) / |u x v|, the dot product and the squared norm summed left to
// right, no FMA (the library is compiled with -ffp-contract=off); area = |u x v| / 2 at corner 0.  Weights may be negative
// (obtuse angles) and stay so.
//
// No floating-point atomics: every face hands its six directed entries (i -> j, the half-cotangent opposite (i, j), the face
// number) to the source vertices' segments (an integer count decides the slot), each vertex sorts its segment by (column,
// face) and sums equal columns in ascending face order, the areas in ascending face order; rows are summed left to right in
// column order.  Two builds of a mesh give identical bits, and w_ij == w_ji bit for bit (the same terms in the same order).
//
// The graph that comes out is a general-matrix graph (unit_g: w = -S_ij, deg = S_ii, g = sg = 1) in the caller's vertex
// numbering, so the operator storage, the component labels and the whole eigensolver path are the ones of
// pf_graph_from_matrix (pf_graph_finish_general); its null vectors are sqrt(m) on each component (pf_lock_null_vectors).
#include <string.h>

#include <algorithm>
#include <vector>

#include "pf_internal.h"

namespace {

constexpr int PF_COTAN_MAX_COLS = 8;

__device__ __forceinline__ bool face_usable(const int32_t* __restrict__ faces, int64_t f, int64_t n, int32_t* i) {
    i[0] = faces[3 * f], i[1] = faces[3 * f + 1], i[2] = faces[3 * f + 2];
    const bool in_range = i[0] >= 0 && i[0] < n && i[1] >= 0 && i[1] < n && i[2] >= 0 && i[2] < n;
    return in_range && i[0] != i[1] && i[1] != i[2] && i[0] != i[2];
}

// one thread per face: the three half-cotangents, the area, and two places in each corner vertex's segment.
// flags: 1 index out of range, 2 repeated vertex, 4 zero (or non-finite) |u x v|
__global__ __launch_bounds__(PF_BLOCK) void k_cotan_faces(const int32_t* __restrict__ faces, const double* __restrict__ pts,
                                                          int64_t n_faces, int64_t n, double* __restrict__ half_cot,
                                                          double* __restrict__ area, int32_t* __restrict__ cnt,
                                                          int32_t* __restrict__ rank, int32_t* __restrict__ flags) {
    const int64_t f = (int64_t)blockIdx.x * PF_BLOCK + threadIdx.x;
    if (f >= n_faces) return;
    int32_t v[3];
    area[f] = 0.0;
    if (!face_usable(faces, f, n, v)) {
        const bool in_range = v[0] >= 0 && v[0] < n && v[1] >= 0 && v[1] < n && v[2] >= 0 && v[2] < n;
        atomicOr(flags, in_range ? 2 : 1);
        return;
    }
    double p[3][3];
#pragma unroll
    for (int k = 0; k < 3; ++k)
#pragma unroll
        for (int c = 0; c < 3; ++c) p[k][c] = pts[3 * (int64_t)v[k] + c];
    bool bad = false;
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        const int a = (k + 1) % 3, b = (k + 2) % 3;
        const double ux = p[a][0] - p[k][0], uy = p[a][1] - p[k][1], uz = p[a][2] - p[k][2];
        const double vx = p[b][0] - p[k][0], vy = p[b][1] - p[k][1], vz = p[b][2] - p[k][2];
        const double dot = (ux * vx + uy * vy) + uz * vz;
        const double cx = uy * vz - uz * vy, cy = uz * vx - ux * vz, cz = ux * vy - uy * vx;
        const double nrm = sqrt((cx * cx + cy * cy) + cz * cz);
        if (!(nrm > 0.0) || !isfinite(nrm)) bad = true;
        half_cot[3 * f + k] = 0.5 * (dot / nrm);
        if (k == 0) area[f] = nrm / 2.0;
    }
    if (bad) atomicOr(flags, 4);
#pragma unroll
    for (int k = 0; k < 3; ++k) rank[3 * f + k] = atomicAdd(&cnt[v[k]], 2);
}

// the face's six directed entries into the segments of their source vertices.  key = column << 32 | face << 1 | second: a
// sort by key is a sort by (column, face); bit 0 marks the second of the two entries a face leaves at a vertex
__global__ __launch_bounds__(PF_BLOCK) void k_cotan_scatter(const int32_t* __restrict__ faces, int64_t n_faces, int64_t n,
                                                            const double* __restrict__ half_cot, const int32_t* __restrict__ start,
                                                            const int32_t* __restrict__ rank, long long* __restrict__ key,
                                                            double* __restrict__ val) {
    const int64_t f = (int64_t)blockIdx.x * PF_BLOCK + threadIdx.x;
    if (f >= n_faces) return;
    int32_t v[3];
    if (!face_usable(faces, f, n, v)) return;  // flagged by k_cotan_faces, which counted nothing for it either
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        const int a = (k + 1) % 3, b = (k + 2) % 3;
        const int64_t slot = (int64_t)start[v[k]] + rank[3 * f + k];
        key[slot] = ((long long)v[a] << 32) | ((long long)f << 1);
        val[slot] = half_cot[3 * f + b];  // edge (k, a): opposite corner b
        key[slot + 1] = ((long long)v[b] << 32) | ((long long)f << 1) | 1;
        val[slot + 1] = half_cot[3 * f + a];
    }
}

// one thread per vertex: the mass from its faces in ascending face order, then the segment sorted by (column, face),
// equal columns summed in that order, the row sum left to right
__global__ __launch_bounds__(PF_BLOCK) void k_cotan_rows(const int32_t* __restrict__ start, int64_t n, long long* __restrict__ key,
                                                         double* __restrict__ val, const double* __restrict__ area,
                                                         int32_t* __restrict__ rcol, double* __restrict__ rw,
                                                         int32_t* __restrict__ ucnt, double* __restrict__ diag,
                                                         double* __restrict__ mass, double* __restrict__ sqrtm) {
    const int64_t i = (int64_t)blockIdx.x * PF_BLOCK + threadIdx.x;
    if (i > n) return;
    if (i == n) {
        ucnt[n] = 0;  // (the scan's extra element)
        return;
    }
    const int32_t b = start[i], e = start[i + 1];
    double a_sum = 0.0;
    for (int32_t last = -1;;) {  // a face leaves two entries at the vertex: the first of them stands for it
        int32_t best = 0x7fffffff;
        for (int32_t a = b; a < e; ++a) {
            const long long k = key[a];
            const int32_t f = (int32_t)((k & 0xffffffffll) >> 1);
            if (!(k & 1) && f > last && f < best) best = f;
        }
        if (best == 0x7fffffff) break;
        a_sum += area[best];
        last = best;
    }
    const double m = a_sum / 3.0;
    mass[i] = m;
    sqrtm[i] = sqrt(m);
    for (int32_t a = b + 1; a < e; ++a) {
        const long long kk = key[a];
        const double vv = val[a];
        int32_t p = a - 1;
        while (p >= b && key[p] > kk) {
            key[p + 1] = key[p];
            val[p + 1] = val[p];
            --p;
        }
        key[p + 1] = kk;
        val[p + 1] = vv;
    }
    int32_t u = 0;
    double d = 0.0, acc = 0.0;
    int32_t cur = -1;
    for (int32_t a = b; a < e; ++a) {
        const int32_t c = (int32_t)(key[a] >> 32);
        if (c != cur) {
            if (cur >= 0) {
                rcol[b + u] = cur;
                rw[b + u] = acc;
                d += acc;
                ++u;
            }
            cur = c;
            acc = val[a];
        } else {
            acc += val[a];
        }
    }
    if (cur >= 0) {
        rcol[b + u] = cur;
        rw[b + u] = acc;
        d += acc;
        ++u;
    }
    ucnt[i] = u;
    diag[i] = d;
}

// CSR: the columns, the cotangent weights beside them, and the entries of S = M^-1/2 (D - W) M^-1/2 where the general-matrix
// path keeps them (w = -S_ij, deg = S_ii).  sqrt(m_i) sqrt(m_j) is one product whichever end computes it: S_ij == S_ji.
// hi: max over the rows of sum |S_ij| (bits of a non-negative double order like the integer)
__global__ __launch_bounds__(PF_BLOCK) void k_cotan_compact(const int32_t* __restrict__ start, const int32_t* __restrict__ rowptr,
                                                            int64_t n, const int32_t* __restrict__ rcol,
                                                            const double* __restrict__ rw, const double* __restrict__ diag,
                                                            const double* __restrict__ mass, const double* __restrict__ sqrtm,
                                                            int32_t* __restrict__ col, double* __restrict__ cot_w,
                                                            double* __restrict__ w, double* __restrict__ deg,
                                                            double* __restrict__ g, double* __restrict__ sg,
                                                            unsigned long long* __restrict__ hi_bits) {
    __shared__ double red[PF_BLOCK / PF_WAVE];
    const int64_t i = (int64_t)blockIdx.x * PF_BLOCK + threadIdx.x;
    double row_abs = 0.0;
    if (i < n) {
        const int32_t src = start[i];
        const int32_t b = rowptr[i], cnt = rowptr[i + 1] - b;
        const double si = sqrtm[i], mi = mass[i];
        const double sii = mi > 0.0 ? diag[i] / mi : 0.0;
        row_abs = fabs(sii);
        for (int32_t a = 0; a < cnt; ++a) {
            const int32_t j = rcol[src + a];
            const double wv = rw[src + a];
            const double s = wv / (si * sqrtm[j]);
            col[b + a] = j;
            cot_w[b + a] = wv;
            w[b + a] = s;
            row_abs += fabs(s);
        }
        deg[i] = sii;
        g[i] = 1.0;
        sg[i] = 1.0;
    }
    if (!(row_abs >= 0.0)) row_abs = 0.0;  // (NaN: reported through the flags)
#pragma unroll
    for (int off = PF_WAVE / 2; off > 0; off >>= 1) {
        const double o = __shfl_down(row_abs, off, PF_WAVE);
        row_abs = o > row_abs ? o : row_abs;
    }
    if ((threadIdx.x & (PF_WAVE - 1)) == 0) red[threadIdx.x / PF_WAVE] = row_abs;
    __syncthreads();
    if (threadIdx.x == 0) {
        double m = red[0];
        for (int k = 1; k < PF_BLOCK / PF_WAVE; ++k) m = red[k] > m ? red[k] : m;
        atomicMax(hi_bits, (unsigned long long)__double_as_longlong(m));
    }
}

// the faces' areas, one partial sum per block in a fixed tree order (the host adds the partials in block order)
__global__ __launch_bounds__(PF_BLOCK) void k_cotan_area(const double* __restrict__ area, int64_t n_faces, double* __restrict__ partial) {
    __shared__ double red[PF_BLOCK];
    const int64_t f = (int64_t)blockIdx.x * PF_BLOCK + threadIdx.x;
    red[threadIdx.x] = f < n_faces ? area[f] : 0.0;
    __syncthreads();
    for (int off = PF_BLOCK / 2; off > 0; off >>= 1) {
        if ((int)threadIdx.x < off) red[threadIdx.x] += red[threadIdx.x + off];
        __syncthreads();
    }
    if (threadIdx.x == 0) partial[blockIdx.x] = red[0];
}

// out_i = (sum_j w_ij (x_i - x_j)) / m_i per column, the row left to right; 0 where m_i == 0
__global__ __launch_bounds__(PF_BLOCK) void k_cotan_apply(const int32_t* __restrict__ rowptr, const int32_t* __restrict__ col,
                                                          const double* __restrict__ cot_w, const double* __restrict__ mass,
                                                          int64_t n, int32_t ncols, const double* __restrict__ x,
                                                          double* __restrict__ out) {
    const int64_t i = (int64_t)blockIdx.x * PF_BLOCK + threadIdx.x;
    if (i >= n) return;
    double acc[PF_COTAN_MAX_COLS], xi[PF_COTAN_MAX_COLS];
#pragma unroll
    for (int c = 0; c < PF_COTAN_MAX_COLS; ++c) {
        acc[c] = 0.0;
        xi[c] = c < ncols ? x[i * ncols + c] : 0.0;
    }
    for (int32_t a = rowptr[i]; a < rowptr[i + 1]; ++a) {
        const int64_t j = col[a];
        const double wv = cot_w[a];
#pragma unroll
        for (int c = 0; c < PF_COTAN_MAX_COLS; ++c)
            if (c < ncols) acc[c] += wv * (xi[c] - x[j * ncols + c]);
    }
    const double m = mass[i];
#pragma unroll
    for (int c = 0; c < PF_COTAN_MAX_COLS; ++c)
        if (c < ncols) out[i * ncols + c] = m > 0.0 ? acc[c] / m : 0.0;
}

// until the build has succeeded, the graph itself is the build's to free
struct CotanBuild {
    pf_graph* g = nullptr;
    bool ok = false;
    ~CotanBuild() {
        if (!ok && g) pf_graph_free(g);
    }
};

}  // namespace

extern "C" {

int pf_graph_build_cotan(pf_mesh* mesh, int32_t mass_kind, pf_graph** out) {
    PF_CHECK(mesh && out, PF_E_ARG, "pf_graph_build_cotan: NULL argument");
    *out = nullptr;
    PF_CHECK(mesh->vpf == 3, PF_E_ARG, "pf_graph_build_cotan: triangles only (verts_per_face = %d)", mesh->vpf);
    PF_CHECK(mass_kind == 0, PF_E_ARG, "pf_graph_build_cotan: mass_kind %d unknown (0 = barycentric)", mass_kind);
    pf_ctx* ctx = mesh->ctx;
    const int64_t n = mesh->n, n_faces = mesh->n_faces, n_entries = 6 * n_faces;
    PF_CHECK(n_entries < (int64_t)1 << 31, PF_E_ARG, "pf_graph_build_cotan: %lld faces are too many", (long long)n_faces);
    PF_HIP(hipSetDevice(ctx->device));
    hipStream_t st = ctx->stream;
    CotanBuild job;
    pf_graph* g = job.g = new pf_graph();
    Scratch sc(st);  // (declared after job: the temporaries go back before the graph of a failed build does)
    g->ctx = ctx;
    g->unit_g = 1;
    g->is_cotan = 1;
    g->n = n;
    g->n_faces = n_faces;
    g->vpf = 3;
    g->n_pad = (n + 4095) / 4096 * 4096;
    g->win_rows = pf_window_rows(g->n_pad);
    g->n_slices = g->n_pad / PF_WAVE;
    g->n_chunks = (g->n_pad + PF_DOT_CHUNK - 1) / PF_DOT_CHUNK;

    const unsigned face_blocks = pf_blocks(n_faces);
    double* half_cot = sc.get<double>(3 * n_faces);
    double* area = sc.get<double>(n_faces);
    double* partial = sc.get<double>(face_blocks);
    int32_t* cnt = sc.get<int32_t>(n + 1);
    int32_t* start = sc.get<int32_t>(n + 1);
    int32_t* rank = sc.get<int32_t>(3 * n_faces);
    long long* key = sc.get<long long>(n_entries);
    double* val = sc.get<double>(n_entries);
    int32_t* rcol = sc.get<int32_t>(n_entries);
    double* rw = sc.get<double>(n_entries);
    int32_t* ucnt = sc.get<int32_t>(n + 1);
    int32_t* flags = sc.get<int32_t>(8);
    unsigned long long* hi_bits = sc.get<unsigned long long>(1);
    g->rowptr = sc.keep<int32_t>(n + 1);
    g->deg = sc.keep<double>(g->n_pad);
    g->g = sc.keep<double>(g->n_pad);
    g->sg = sc.keep<double>(g->n_pad);
    g->diag = sc.keep<double>(g->n_pad);
    g->label = sc.keep<int32_t>(g->n_pad);
    g->perm = sc.keep<int32_t>(g->n_pad);
    g->iperm = sc.keep<int32_t>(g->n_pad);
    g->smooth = sc.keep<double>(g->n_pad);
    g->slice_ptr = sc.keep<int64_t>(g->n_slices + 1);
    g->cot_diag = sc.keep<double>(n);
    g->cot_mass = sc.keep<double>(n);
    g->cot_sqrtm = sc.keep<double>(n);
    g->pts = sc.keep<double>(3 * n);
    PF_HIP(sc.err);
    PF_HIP(hipMemsetAsync(cnt, 0, sizeof(int32_t) * (size_t)(n + 1), st));
    PF_HIP(hipMemsetAsync(flags, 0, sizeof(int32_t) * 8, st));
    PF_HIP(hipMemsetAsync(hi_bits, 0, sizeof(unsigned long long), st));
    PF_HIP(hipMemsetAsync(g->deg, 0, sizeof(double) * (size_t)g->n_pad, st));
    PF_HIP(hipMemsetAsync(g->g, 0, sizeof(double) * (size_t)g->n_pad, st));
    PF_HIP(hipMemsetAsync(g->sg, 0, sizeof(double) * (size_t)g->n_pad, st));
    PF_HIP(hipEventRecord(ctx->ev0, st));
    PF_HIP(hipMemcpyAsync(g->pts, mesh->pts, sizeof(double) * 3 * (size_t)n, hipMemcpyDeviceToDevice, st));
    if (n_faces) {
        k_cotan_faces<<<face_blocks, PF_BLOCK, 0, st>>>(mesh->faces, mesh->pts, n_faces, n, half_cot, area, cnt, rank, flags);
        PF_HIP(hipGetLastError());
        k_cotan_area<<<face_blocks, PF_BLOCK, 0, st>>>(area, n_faces, partial);
        PF_HIP(hipGetLastError());
    }
    PF_TRY(pf_exclusive_scan_i32(st, cnt, start, n + 1));
    if (n_faces) {
        k_cotan_scatter<<<face_blocks, PF_BLOCK, 0, st>>>(mesh->faces, n_faces, n, half_cot, start, rank, key, val);
        PF_HIP(hipGetLastError());
    }
    k_cotan_rows<<<pf_blocks(n + 1), PF_BLOCK, 0, st>>>(start, n, key, val, area, rcol, rw, ucnt, g->cot_diag, g->cot_mass, g->cot_sqrtm);
    PF_HIP(hipGetLastError());
    PF_TRY(pf_exclusive_scan_i32(st, ucnt, g->rowptr, n + 1));
    // the one read-back before the storage is sized: the flags, the entry count, the area's partial sums
    int32_t h_flags = 0, nnz32 = 0;
    std::vector<double> h_partial(face_blocks, 0.0);
    PF_HIP(hipMemcpyAsync(&h_flags, flags, sizeof(int32_t), hipMemcpyDeviceToHost, st));
    PF_HIP(hipMemcpyAsync(&nnz32, g->rowptr + n, sizeof(int32_t), hipMemcpyDeviceToHost, st));
    if (n_faces) PF_HIP(hipMemcpyAsync(h_partial.data(), partial, sizeof(double) * face_blocks, hipMemcpyDeviceToHost, st));
    PF_HIP(hipStreamSynchronize(st));
    PF_CHECK(!(h_flags & 1), PF_E_ARG, "pf_graph_build_cotan: face index out of range [0,%lld)", (long long)n);
    PF_CHECK(!(h_flags & 2), PF_E_DEGENERATE, "pf_graph_build_cotan: a face repeats a vertex");
    PF_CHECK(!(h_flags & 4), PF_E_DEGENERATE, "pf_graph_build_cotan: a face has zero area or non-finite coordinates");
    double total = 0.0;
    for (double p : h_partial) total += p;
    g->cot_area = total;
    g->nnz_w = nnz32;
    g->col = sc.keep<int32_t>(g->nnz_w);
    g->w = sc.keep<double>(g->nnz_w);
    g->cot_w = sc.keep<double>(g->nnz_w);
    PF_HIP(sc.err);
    k_cotan_compact<<<pf_blocks(n), PF_BLOCK, 0, st>>>(start, g->rowptr, n, rcol, rw, g->cot_diag, g->cot_mass, g->cot_sqrtm, g->col, g->cot_w,
                                                 g->w, g->deg, g->g, g->sg, hi_bits);
    PF_HIP(hipGetLastError());
    PF_TRY(pf_graph_finish_general(g, g->pts));
    unsigned long long h_hi = 0;
    PF_HIP(hipMemcpy(&h_hi, hi_bits, sizeof(h_hi), hipMemcpyDeviceToHost));
    memcpy(&g->cot_hi, &h_hi, sizeof(double));
    g->spectral_bound = g->cot_hi;
    job.ok = true;
    *out = g;
    return PF_OK;
}

int pf_graph_cotan_info(pf_graph* g, double* hi, double* total_area) {
    PF_CHECK(g != nullptr && g->is_cotan, PF_E_ARG, "pf_graph_cotan_info: not a cotangent graph");
    if (hi) *hi = g->cot_hi;
    if (total_area) *total_area = g->cot_area;
    return PF_OK;
}

int pf_graph_cotan_download(pf_graph* g, double* w, double* diag, double* mass) {
    PF_CHECK(g != nullptr && g->is_cotan, PF_E_ARG, "pf_graph_cotan_download: not a cotangent graph");
    PF_HIP(hipSetDevice(g->ctx->device));
    hipStream_t st = g->ctx->stream;
    if (w && g->nnz_w) PF_HIP(hipMemcpyAsync(w, g->cot_w, sizeof(double) * (size_t)g->nnz_w, hipMemcpyDeviceToHost, st));
    if (diag) PF_HIP(hipMemcpyAsync(diag, g->cot_diag, sizeof(double) * (size_t)g->n, hipMemcpyDeviceToHost, st));
    if (mass) PF_HIP(hipMemcpyAsync(mass, g->cot_mass, sizeof(double) * (size_t)g->n, hipMemcpyDeviceToHost, st));
    PF_HIP(hipStreamSynchronize(st));
    return PF_OK;
}

int pf_cotan_apply(pf_graph* g, const double* x, int32_t ncols, double* out) {
    PF_CHECK(g != nullptr && g->is_cotan, PF_E_ARG, "pf_cotan_apply: not a cotangent graph");
    PF_CHECK(x != nullptr && out != nullptr && ncols >= 1 && ncols <= PF_COTAN_MAX_COLS, PF_E_ARG,
             "pf_cotan_apply: NULL argument or ncols = %d outside 1..%d", ncols, PF_COTAN_MAX_COLS);
    PF_HIP(hipSetDevice(g->ctx->device));
    Scratch s(g->ctx->stream);
    const size_t count = (size_t)g->n * (size_t)ncols;
    double* d_x = s.get<double>(count);
    double* d_out = s.get<double>(count);
    s.upload(d_x, x, count);
    if (s.ok()) {
        k_cotan_apply<<<pf_blocks(g->n), PF_BLOCK, 0, s.st>>>(g->rowptr, g->col, g->cot_w, g->cot_mass, g->n, ncols, d_x, d_out);
        s.launched();
    }
    s.download(out, d_out, count);
    s.sync();
    PF_HIP(s.err);
    return PF_OK;
}

}  // extern "C"
