// The isosurface of a sampled scalar field (pf_isosurface_*): marching tetrahedra on the Kuhn decomposition of every cube
// of the lattice, welded vertices, faces in a fixed order.  The definition is in include/pyfocusr_hip.h;
// tests/_isosurface_ref.py restates it in numpy and the device returns its bits.
//
// The volume is read once to classify it; every later pass reads bits, and the values again only at crossing edges.
//   k_iso_classify  a wave's 64 lanes are 64 samples along k: their `value < level` predicates are one 64-bit word
//                   (__ballot); a row of nz samples owns ceil(nz / 64) words; a block writes 16 words: one whole line
//   k_iso_edges     one thread per lattice point: the 7-bit mask of the edge kinds that leave it and cross the level, and
//                   its popcount.  The exclusive scan of the counts is each point's first vertex number, and the number
//                   of an edge is first[p] + popcount(mask[p] & ((1 << kind) - 1)): welding needs no sort and no hash
//   k_iso_cells     one thread per cell: its 8 corner bits and, from a 256-entry table, its triangle count; scanned too
//   (the host reads the two totals - the call's one wait before the outputs are sized - and checks their range)
//   k_iso_vertices  one thread per lattice point with a crossing edge: t, the position, the edge's key
//   k_iso_faces     one thread per crossing cell: its tetrahedra in permutation order, the triangles of each from the
//                   case table, three vertex numbers each looked up as above; the cell index per face
// The tables (ISO) are derived at compile time from the orientation rule; nothing is typed in.  Ordinary launches only: no
// block waits for another, the totals are integer atomics, there is no floating-point sum at all: two calls give the same
// bits.  Arithmetic: separate multiplies and adds (-ffp-contract=off).
// pf_isosurface_create checks and uploads; everything above is pf_isosurface_extract, over values that are on the device,
// which pf_edt_isosurface (pf_edt.hip) calls on the distance field it holds.
#include <cmath>

#include "pf_internal.h"

struct pf_isosurface {
    pf_ctx* ctx = nullptr;
    int64_t n_vertices = 0, n_faces = 0;
    double* pts = nullptr;       // [V][3]
    int32_t* faces = nullptr;    // [F][3]
    int64_t* vkey = nullptr;     // [V]
    int32_t* fcell = nullptr;    // [F]
};

namespace {

// A cube corner is the number 4 di + 2 dj + dk of its offset; an edge kind 0..6 is (1,0,0) (0,1,0) (0,0,1) (1,1,0) (1,0,1)
// (0,1,1) (1,1,1).  A triangle's vertex is a lattice edge: corner << 3 | kind, the corner being the edge's lower end.
struct IsoTables {
    uint8_t tet_corner[6][4];  // the four corners of the tetrahedron of each axis permutation, in local order
    uint8_t n_tri[6][16];      // triangles of a tetrahedron by case; bit v of the case = local vertex v is inside
    uint8_t edge[6][16][6];    // their vertices, [3 r + e] of triangle r
    uint8_t cell_tris[256];    // triangles of a cell by its corner bits; bit c = corner c is inside
};

constexpr int iso_kind_of(int diff) {  // the kind of the edge whose ends differ by the corner `diff`
    constexpr int kind[8] = {-1, 2, 1, 5, 0, 4, 3, 6};
    return kind[diff];
}

constexpr IsoTables iso_make_tables() {
    IsoTables T{};
    int t = 0;
    for (int a = 0; a < 3; ++a)  // (a, b, c) in lexicographic order: the order of itertools.permutations
        for (int b = 0; b < 3; ++b) {
            if (b == a) continue;
            const int v1 = 4 >> a, v2 = v1 | (4 >> b);
            T.tet_corner[t][0] = 0, T.tet_corner[t][1] = (uint8_t)v1, T.tet_corner[t][2] = (uint8_t)v2, T.tet_corner[t][3] = 7;
            ++t;
        }
    for (t = 0; t < 6; ++t)
        for (int cs = 1; cs < 15; ++cs) {
            int ins[4] = {0, 0, 0, 0}, outs[4] = {0, 0, 0, 0}, n_in = 0, n_out = 0;
            for (int v = 0; v < 4; ++v) {
                if ((cs >> v) & 1)
                    ins[n_in++] = v;
                else
                    outs[n_out++] = v;
            }
            // the triangles as pairs of local vertices, before orientation
            int tri[2][3][2] = {};
            int n_tri = 1;
            if (n_in == 1 || n_out == 1) {
                const int lone = n_in == 1 ? ins[0] : outs[0];
                int e = 0;
                for (int v = 0; v < 4; ++v)
                    if (v != lone) tri[0][e][0] = lone, tri[0][e][1] = v, ++e;
            } else {
                const int A = ins[0], B = ins[1], Cc = outs[0], D = outs[1];
                const int quad[4][2] = {{A, Cc}, {A, D}, {B, D}, {B, Cc}};
                const int pick[2][3] = {{0, 1, 2}, {0, 2, 3}};
                n_tri = 2;
                for (int r = 0; r < 2; ++r)
                    for (int e = 0; e < 3; ++e) tri[r][e][0] = quad[pick[r][e]][0], tri[r][e][1] = quad[pick[r][e]][1];
            }
            // n_in n_out (centroid of the outside corners - centroid of the inside corners), in integers
            int dir[3] = {0, 0, 0};
            for (int ax = 0; ax < 3; ++ax) {
                int s_in = 0, s_out = 0;
                for (int q = 0; q < n_in; ++q) s_in += (T.tet_corner[t][ins[q]] >> (2 - ax)) & 1;
                for (int q = 0; q < n_out; ++q) s_out += (T.tet_corner[t][outs[q]] >> (2 - ax)) & 1;
                dir[ax] = n_in * s_out - n_out * s_in;
            }
            T.n_tri[t][cs] = (uint8_t)n_tri;
            for (int r = 0; r < n_tri; ++r) {
                int M[3][3] = {};  // twice the edge midpoints
                for (int e = 0; e < 3; ++e)
                    for (int ax = 0; ax < 3; ++ax)
                        M[e][ax] = ((T.tet_corner[t][tri[r][e][0]] >> (2 - ax)) & 1) + ((T.tet_corner[t][tri[r][e][1]] >> (2 - ax)) & 1);
                const int u[3] = {M[1][0] - M[0][0], M[1][1] - M[0][1], M[1][2] - M[0][2]};
                const int w[3] = {M[2][0] - M[0][0], M[2][1] - M[0][1], M[2][2] - M[0][2]};
                const int nrm[3] = {u[1] * w[2] - u[2] * w[1], u[2] * w[0] - u[0] * w[2], u[0] * w[1] - u[1] * w[0]};
                const bool flip = nrm[0] * dir[0] + nrm[1] * dir[1] + nrm[2] * dir[2] < 0;
                for (int e = 0; e < 3; ++e) {
                    const int src = flip && e ? 3 - e : e;  // a flip swaps the last two vertices
                    int lo = tri[r][src][0], hi = tri[r][src][1];
                    if (lo > hi) {
                        const int s = lo;
                        lo = hi, hi = s;
                    }
                    const int c_lo = T.tet_corner[t][lo], c_hi = T.tet_corner[t][hi];
                    T.edge[t][cs][3 * r + e] = (uint8_t)(c_lo << 3 | iso_kind_of(c_hi - c_lo));
                }
            }
        }
    for (int bits = 0; bits < 256; ++bits) {
        int n = 0;
        for (t = 0; t < 6; ++t) {
            int cs = 0;
            for (int v = 0; v < 4; ++v) cs |= ((bits >> T.tet_corner[t][v]) & 1) << v;
            n += T.n_tri[t][cs];
        }
        T.cell_tris[bits] = (uint8_t)n;
    }
    return T;
}

__constant__ IsoTables ISO = iso_make_tables();

struct IsoGrid {
    int64_t nx, ny, nz;
    int64_t words;  // 64-bit words of a row of nz samples
    double level, spacing[3], origin[3];
};

// whether the sample (row = i ny + j, k) is inside
__device__ __forceinline__ unsigned iso_bit(const unsigned long long* __restrict__ bits, int64_t words, int64_t row, int64_t k) {
    return (unsigned)(bits[row * words + (k >> 6)] >> (k & 63)) & 1u;
}

// the wave's sum of v is added to *slot; every lane of the wave calls it
__device__ __forceinline__ void iso_total(unsigned long long* slot, int v) {
#pragma unroll
    for (int off = PF_WAVE / 2; off > 0; off >>= 1) v += __shfl_xor(v, off, PF_WAVE);
    if ((threadIdx.x & (PF_WAVE - 1)) == 0 && v) atomicAdd(slot, (unsigned long long)v);
}

// A block classifies the samples of ISO_LINE consecutive words, a wave ISO_LINE / 4 of them one after the other (its 64
// lanes are the word's samples along k; lane t keeps word t) and stores them with one instruction: every 128-byte line of
// `bits` is written whole by one block, not by four blocks on four XCDs.
constexpr int ISO_LINE = 16;  // words of a block: 128 bytes, the blocks of `bits` being 256-byte aligned
static_assert(ISO_LINE % (PF_BLOCK / PF_WAVE) == 0, "every wave of k_iso_classify takes the same number of words");

__global__ __launch_bounds__(PF_BLOCK) void k_iso_classify(const double* __restrict__ values, IsoGrid g,
                                                           unsigned long long* __restrict__ bits) {
    constexpr int PER_WAVE = ISO_LINE / (PF_BLOCK / PF_WAVE);
    const int lane = threadIdx.x & (PF_WAVE - 1);
    const int64_t n_words = g.nx * g.ny * g.words;
    const int64_t w0 = (int64_t)blockIdx.x * ISO_LINE + (threadIdx.x / PF_WAVE) * PER_WAVE;
    unsigned long long mine = 0;
#pragma unroll
    for (int t = 0; t < PER_WAVE; ++t) {
        const int64_t w = w0 + t, row = w / g.words, k = (w - row * g.words) * PF_WAVE + lane;
        const bool inside = w < n_words && k < g.nz && values[row * g.nz + k] < g.level;
        const unsigned long long word = __ballot(inside);
        if (lane == t) mine = word;
    }
    if (lane < PER_WAVE && w0 + lane < n_words) bits[w0 + lane] = mine;
}

// One thread per lattice point: mask[p], cnt[p]; totals[0] += cnt[p].
__global__ __launch_bounds__(PF_BLOCK) void k_iso_edges(const unsigned long long* __restrict__ bits, IsoGrid g, uint8_t* __restrict__ mask,
                                                        int32_t* __restrict__ cnt, unsigned long long* __restrict__ totals) {
    const int64_t p = (int64_t)blockIdx.x * PF_BLOCK + threadIdx.x, n = g.nx * g.ny * g.nz;
    int c = 0;
    if (p < n) {
        const int64_t row = p / g.nz, k = p - row * g.nz, i = row / g.ny, j = row - i * g.ny;
        // the eight corners of the cube above p, read like k_iso_cells reads them, an index past the volume clamped to
        // the last one; `exist` then drops the kinds whose edge leaves the volume
        const unsigned xi = i + 1 < g.nx, yj = j + 1 < g.ny, zk = k + 1 < g.nz;
        unsigned b = 0;
#pragma unroll
        for (int q = 0; q < 8; ++q)
            b |= iso_bit(bits, g.words, row + ((q >> 2) & xi) * g.ny + ((q >> 1) & 1 & yj), k + (q & 1 & zk)) << q;
        const unsigned me = b & 1u, x = me ? ~b : b;  // bit q of x: corner q differs from p
        // kinds 0..6 end at the corners 4 2 1 6 5 3 7
        const unsigned m_all = ((x >> 4) & 1u) | ((x >> 2) & 1u) << 1 | ((x >> 1) & 1u) << 2 | ((x >> 6) & 1u) << 3 | ((x >> 5) & 1u) << 4 |
                               ((x >> 3) & 1u) << 5 | ((x >> 7) & 1u) << 6;
        const unsigned exist = xi | yj << 1 | zk << 2 | (xi & yj) << 3 | (xi & zk) << 4 | (yj & zk) << 5 | (xi & yj & zk) << 6;
        const unsigned m = m_all & exist;
        c = __popc(m);
        mask[p] = (uint8_t)m;
        cnt[p] = c;
    }
    iso_total(&totals[0], c);
}

// One thread per cell: corner[cell] (bit 4 di + 2 dj + dk), tcnt[cell]; totals[1] += triangles, totals[2] += crossing cells.
__global__ __launch_bounds__(PF_BLOCK) void k_iso_cells(const unsigned long long* __restrict__ bits, IsoGrid g, uint8_t* __restrict__ corner,
                                                        int32_t* __restrict__ tcnt, unsigned long long* __restrict__ totals) {
    const int64_t cell = (int64_t)blockIdx.x * PF_BLOCK + threadIdx.x;
    const int64_t cy = g.ny - 1, cz = g.nz - 1, n_cells = (g.nx - 1) * cy * cz;
    int c = 0;
    if (cell < n_cells) {
        const int64_t ij = cell / cz, k = cell - ij * cz, i = ij / cy, j = ij - i * cy;
        unsigned b = 0;
#pragma unroll
        for (int q = 0; q < 8; ++q) b |= iso_bit(bits, g.words, (i + (q >> 2)) * g.ny + j + ((q >> 1) & 1), k + (q & 1)) << q;
        c = ISO.cell_tris[b];
        corner[cell] = (uint8_t)b;
        tcnt[cell] = c;
    }
    iso_total(&totals[1], c);
    iso_total(&totals[2], c ? 1 : 0);
}

// One thread per lattice point: the vertices of its crossing edges, numbered first[p] .. in ascending kind.
// t = (level - v_p) / (v_q - v_p); per coordinate P + t (Q - P) with P = origin + i spacing, Q = origin + (i + d) spacing.
__global__ __launch_bounds__(PF_BLOCK) void k_iso_vertices(const double* __restrict__ values, IsoGrid g, const uint8_t* __restrict__ mask,
                                                           const int32_t* __restrict__ first, double* __restrict__ pts,
                                                           int64_t* __restrict__ vkey) {
    const int64_t p = (int64_t)blockIdx.x * PF_BLOCK + threadIdx.x;
    if (p >= g.nx * g.ny * g.nz) return;
    const unsigned m = mask[p];
    if (!m) return;
    const int64_t row = p / g.nz, k = p - row * g.nz, i = row / g.ny, j = row - i * g.ny;
    const int64_t at[3] = {i, j, k};
    const double vp = values[p];
    int64_t v = first[p];
    double P[3];
#pragma unroll
    for (int a = 0; a < 3; ++a) P[a] = g.origin[a] + (double)at[a] * g.spacing[a];
#pragma unroll
    for (int kind = 0; kind < 7; ++kind) {
        if (!((m >> kind) & 1)) continue;
        // the offsets of the kinds, as corners: 4 2 1 6 5 3 7
        const int d = kind == 0 ? 4 : kind == 1 ? 2 : kind == 2 ? 1 : kind == 3 ? 6 : kind == 4 ? 5 : kind == 5 ? 3 : 7;
        const int dd[3] = {d >> 2, (d >> 1) & 1, d & 1};
        const double vq = values[p + (dd[0] * g.ny + dd[1]) * g.nz + dd[2]];
        const double t = (g.level - vp) / (vq - vp);
#pragma unroll
        for (int a = 0; a < 3; ++a) {
            const double Q = g.origin[a] + (double)(at[a] + dd[a]) * g.spacing[a];
            pts[3 * v + a] = P[a] + t * (Q - P[a]);
        }
        vkey[v] = 7 * p + kind;
        ++v;
    }
}

// One thread per cell: its triangles, numbered tfirst[cell] .., tetrahedra in permutation order.
__global__ __launch_bounds__(PF_BLOCK) void k_iso_faces(IsoGrid g, const uint8_t* __restrict__ corner, const int32_t* __restrict__ tfirst,
                                                        const uint8_t* __restrict__ mask, const int32_t* __restrict__ first,
                                                        int32_t* __restrict__ faces, int32_t* __restrict__ fcell) {
    const int64_t cell = (int64_t)blockIdx.x * PF_BLOCK + threadIdx.x;
    const int64_t cy = g.ny - 1, cz = g.nz - 1;
    if (cell >= (g.nx - 1) * cy * cz) return;
    const unsigned b = corner[cell];
    if (!ISO.cell_tris[b]) return;
    const int64_t ij = cell / cz, k = cell - ij * cz, i = ij / cy, j = ij - i * cy;
    const int64_t p = (i * g.ny + j) * g.nz + k;
    int64_t f = tfirst[cell];
    for (int t = 0; t < 6; ++t) {
        int cs = 0;
#pragma unroll
        for (int v = 0; v < 4; ++v) cs |= ((b >> ISO.tet_corner[t][v]) & 1) << v;
        const int n_tri = ISO.n_tri[t][cs];
        for (int r = 0; r < n_tri; ++r, ++f) {
#pragma unroll
            for (int e = 0; e < 3; ++e) {
                const int code = ISO.edge[t][cs][3 * r + e], c = code >> 3, kind = code & 7;
                const int64_t q = p + ((c >> 2) * g.ny + ((c >> 1) & 1)) * g.nz + (c & 1);
                faces[3 * f + e] = first[q] + __popc(mask[q] & ((1u << kind) - 1u));
            }
            fcell[f] = (int32_t)cell;
        }
    }
}

}  // namespace

// The extraction itself, over values that are on the device already: pf_isosurface_create uploads and calls it,
// pf_edt_isosurface (pf_edt.hip) hands it the distance field it holds.
int pf_isosurface_extract(pf_ctx* ctx, const char* fn, Scratch& sc, const double* d_values, int64_t nx, int64_t ny, int64_t nz,
                          double level, const double* spacing, const double* origin, pf_isosurface** out, int64_t* report,
                          double* device_ms) {
    const int64_t lim = (int64_t)1 << 31;
    const int64_t N = nx * ny * nz, n_cells = (nx - 1) * (ny - 1) * (nz - 1);
    IsoGrid g;
    g.nx = nx, g.ny = ny, g.nz = nz, g.words = (nz + 63) / 64, g.level = level;
    for (int a = 0; a < 3; ++a) g.spacing[a] = spacing[a], g.origin[a] = origin[a];
    hipStream_t st = ctx->stream;
    StreamTimer timer(device_ms != nullptr);
    unsigned long long totals[3] = {0, 0, 0};
    pf_isosurface* h = new pf_isosurface();
    h->ctx = ctx;
    int rc = PF_OK;
    unsigned long long* bits = sc.get<unsigned long long>(nx * ny * g.words);
    uint8_t* mask = sc.get<uint8_t>(N);
    int32_t *cnt = sc.get<int32_t>(N), *first = sc.get<int32_t>(N);
    uint8_t* corner = sc.get<uint8_t>(n_cells);
    int32_t *tcnt = sc.get<int32_t>(n_cells), *tfirst = sc.get<int32_t>(n_cells);
    unsigned long long* d_totals = sc.get<unsigned long long>(3);
    sc.zero(d_totals, sizeof(unsigned long long) * 3);
    timer.start(sc);
    if (sc.ok()) {
        k_iso_classify<<<(unsigned)((nx * ny * g.words + ISO_LINE - 1) / ISO_LINE), PF_BLOCK, 0, st>>>(d_values, g, bits);
        k_iso_edges<<<pf_blocks(N), PF_BLOCK, 0, st>>>(bits, g, mask, cnt, d_totals);
        k_iso_cells<<<pf_blocks(n_cells), PF_BLOCK, 0, st>>>(bits, g, corner, tcnt, d_totals);
        sc.launched();
    }
    sc.download(totals, d_totals, 3);
    // (the totals are the atomics' 64-bit sums: one of 2^31 or more wraps the 32-bit scans, whose output is then not used)
    if (sc.ok() && pf_exclusive_scan_i32(st, cnt, first, N) != PF_OK) sc.note(hipErrorUnknown);
    if (sc.ok() && pf_exclusive_scan_i32(st, tcnt, tfirst, n_cells) != PF_OK) sc.note(hipErrorUnknown);
    sc.sync();  // the one wait before the outputs are sized
    const int64_t V = (int64_t)totals[0], F = (int64_t)totals[1];
    if (sc.ok() && V >= lim) {
        pf_set_error("%s: %lld vertices out of range (< 2^31)", fn, (long long)V);
        rc = PF_E_ARG;
    } else if (sc.ok() && 3 * F >= lim) {
        pf_set_error("%s: %lld faces out of range (3 faces < 2^31)", fn, (long long)F);
        rc = PF_E_ARG;
    }
    if (rc == PF_OK) {
        h->n_vertices = V, h->n_faces = F;
        h->pts = sc.keep<double>(3 * V);
        h->vkey = sc.keep<int64_t>(V);
        h->faces = sc.keep<int32_t>(3 * F);
        h->fcell = sc.keep<int32_t>(F);
        if (sc.ok() && V > 0) {
            k_iso_vertices<<<pf_blocks(N), PF_BLOCK, 0, st>>>(d_values, g, mask, first, h->pts, h->vkey);
            sc.launched();
        }
        if (sc.ok() && F > 0) {
            k_iso_faces<<<pf_blocks(n_cells), PF_BLOCK, 0, st>>>(g, corner, tfirst, mask, first, h->faces, h->fcell);
            sc.launched();
        }
        timer.stop(sc);
        sc.sync();
        timer.read(sc, device_ms);
    }
    if (!sc.ok() || rc != PF_OK) {
        pf_isosurface_free(h);
        return !sc.ok() ? pf_hip_failed(fn, sc.err) : rc;
    }
    if (report) {
        report[0] = h->n_vertices, report[1] = h->n_faces, report[2] = (int64_t)totals[2], report[3] = N, report[4] = n_cells;
        report[5] = report[6] = report[7] = 0;
    }
    *out = h;
    return PF_OK;
}

extern "C" {

void pf_isosurface_free(pf_isosurface* h) {
    if (!h) return;
    (void)hipSetDevice(h->ctx->device);
    (void)hipStreamSynchronize(h->ctx->stream);
    hipStream_t st = h->ctx->stream;
    pf_free(st, h->pts);
    pf_free(st, h->faces);
    pf_free(st, h->vkey);
    pf_free(st, h->fcell);
    delete h;
}

int pf_isosurface_create(pf_ctx* ctx, const double* values, int64_t nx, int64_t ny, int64_t nz, double level, const double* spacing,
                         const double* origin, uint32_t flags, pf_isosurface** out, int64_t* report, double* device_ms) {
    PF_CHECK(ctx && values && spacing && origin && out, PF_E_ARG, "pf_isosurface_create: NULL argument");
    PF_CHECK(flags == 0, PF_E_ARG, "pf_isosurface_create: unknown flags 0x%x", flags);
    const int64_t lim = (int64_t)1 << 31;
    PF_CHECK(nx >= 2 && ny >= 2 && nz >= 2 && nx < lim && ny < lim && nz < lim, PF_E_ARG,
             "pf_isosurface_create: extents %lld x %lld x %lld out of range (each 2..2^31-1)", (long long)nx, (long long)ny, (long long)nz);
    PF_CHECK(nx * ny < lim && nx * ny * nz < lim, PF_E_ARG, "pf_isosurface_create: %lld x %lld x %lld samples out of range (< 2^31)",
             (long long)nx, (long long)ny, (long long)nz);
    PF_CHECK(std::isfinite(level), PF_E_ARG, "pf_isosurface_create: the level is not finite");
    for (int a = 0; a < 3; ++a)
        PF_CHECK(std::isfinite(spacing[a]) && std::isfinite(origin[a]), PF_E_ARG, "pf_isosurface_create: spacing or origin is not finite");
    const int64_t N = nx * ny * nz;
    for (int64_t i = 0; i < N; ++i) PF_CHECK(std::isfinite(values[i]), PF_E_ARG, "pf_isosurface_create: value %lld is not finite", (long long)i);
    PF_HIP(hipSetDevice(ctx->device));
    Scratch sc(ctx->stream);
    double* d_values = sc.get<double>(N);
    sc.upload(d_values, values, N);
    return pf_isosurface_extract(ctx, "pf_isosurface_create", sc, d_values, nx, ny, nz, level, spacing, origin, out, report, device_ms);
}

int pf_isosurface_fetch(pf_isosurface* h, double* pts, int32_t* faces, int64_t* vertex_key, int32_t* face_cell) {
    PF_CHECK(h != nullptr, PF_E_ARG, "pf_isosurface_fetch: NULL handle");
    PF_CHECK((pts || !h->n_vertices) && (faces || !h->n_faces), PF_E_ARG, "pf_isosurface_fetch: NULL pts or faces");
    PF_HIP(hipSetDevice(h->ctx->device));
    Scratch sc(h->ctx->stream);
    if (h->n_vertices) {
        sc.download(pts, h->pts, 3 * h->n_vertices);
        sc.download(vertex_key, h->vkey, h->n_vertices);
    }
    if (h->n_faces) {
        sc.download(faces, h->faces, 3 * h->n_faces);
        sc.download(face_cell, h->fcell, h->n_faces);
    }
    sc.sync();
    return sc.ok() ? PF_OK : pf_hip_failed("pf_isosurface_fetch", sc.err);
}

}  // extern "C"
