// Topology of a triangle mesh (pf_mesh_topology): the face across every half-edge, the patches (faces connected across
// two-face edges), whether a patch is orientable, the faces to reverse so that all faces of a patch agree - and, for a
// closed patch with points, point outward - and the boundary loops.  The definitions are in include/pyfocusr_hip.h;
// tests/_topology_ref.py restates them in numpy / scipy.
//
// The half-edges sorted by their edge's key are walked one run per edge (pf_halfedge.h has the keys, the run walk and
// the edge counts).
//   k_topo_halfedges  one thread per face: the three keys, and (h << 1 | direction) as the sort's value
//   k_topo_edges      one thread per run of equal keys: the edge's class, face_neighbours, the parity of a two-face
//                     edge on both of its half-edges, the four counts, the faces that touch an edge of one or of
//                     three and more faces
//   k_topo_hook       union-find over the faces that carries the parity relative to the parent: the word of face t is
//   k_topo_compress   (parent << 1 | parity), so one 64-bit atomicMin moves both.  Per two-face edge the larger root
//                     goes under the smaller one; then every face is pointed at its root.  Parents only ever decrease,
//                     so no walk can cycle; every word ever stored is a true statement about its face (in an orientable
//                     patch), so walks that run beside the hooks stay right.  A round is two ordinary launches; the host
//                     reads a flag after each round and stops when no edge had two roots.  The last root of a patch is
//                     its smallest face, so the parities are the unique ones with rel[smallest face] = 0.
//   k_topo_orient     one thread per two-face edge: rel[a] ^ rel[b] != p marks the patch as not orientable
//   k_topo_count      faces, faces with rel = 1 and "touches an open edge" per patch: integer atomics, one per wave where
//                     a wave's faces share their patch
//   k_topo_rule       per patch: reverse rel where it would reverse more than half of the faces
//   k_topo_terms, k_seg_start, k_seg_sum x 3, k_topo_outward
//                     (with points and the outward flag) the faces sorted by patch, stable; 6 V of a patch as the sum of
//                     a . (b x c) over its faces in ascending order along a fixed tree: 256 consecutive terms, 256 of
//                     those sums, then the rest in order.  A closed orientable patch with V < 0 is reversed.
//   k_topo_flip       flip per face
//   k_loop_keys, k_loop_hook, k_loop_compress
//                     the boundary half-edges twice, under (patch, vertex) for each end, sorted: neighbours in a run
//                     share a vertex and are hooked as the faces are, without parity.  Skipped without boundary edges.
// The host turns roots into dense ascending ids (patches by their smallest face, loops by their smallest half-edge).
// No floating-point atomics, no kernel waits for another block: two calls give the same bits.
#include <vector>

#include "pf_halfedge.h"

namespace {

typedef unsigned long long u64;

__device__ __forceinline__ u64 word_load(const u64* p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
__device__ __forceinline__ int32_t link_load(const int32_t* p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }

__global__ __launch_bounds__(PF_BLOCK) void k_topo_halfedges(const int32_t* __restrict__ faces, int64_t n_tri, int nb,
                                                             u64* __restrict__ ekey, unsigned* __restrict__ hval) {
    const int64_t t = (int64_t)blockIdx.x * PF_BLOCK + threadIdx.x;
    if (t >= n_tri) return;
    const int32_t v[3] = {faces[3 * t], faces[3 * t + 1], faces[3 * t + 2]};
#pragma unroll
    for (int j = 0; j < 3; ++j) {
        const int32_t a = v[j], b = v[he_next(j)];
        ekey[3 * t + j] = he_edge_key(a, b, nb);
        hval[3 * t + j] = ((unsigned)(3 * t + j) << 1) | (a < b ? 0u : 1u);
    }
}

// One thread per edge: the first half-edge of each run of equal keys; the run is in ascending h.  counts: he_count_edge.
__global__ __launch_bounds__(PF_BLOCK) void k_topo_edges(const u64* __restrict__ ekey, const unsigned* __restrict__ hval, int64_t n_half,
                                                         int32_t* __restrict__ nbr, uint8_t* __restrict__ hpar,
                                                         uint8_t* __restrict__ fopen, u64* __restrict__ counts) {
    const int64_t i = (int64_t)blockIdx.x * PF_BLOCK + threadIdx.x;
    const int64_t end = he_run_end(ekey, n_half, i);
    if (end == i) return;
    const int64_t m = end - i;
    const unsigned w0 = hval[i], w1 = m == 2 ? hval[i + 1] : 0u;
    he_count_edge(counts, m, !(w0 & 1u), !(w1 & 1u));
    if (m == 2) {
        const int64_t h0 = w0 >> 1, h1 = w1 >> 1;
        const uint8_t p = (w0 & 1u) == (w1 & 1u) ? 1 : 0;
        nbr[h0] = (int32_t)(h1 / 3);
        nbr[h1] = (int32_t)(h0 / 3);
        hpar[h0] = p;
        hpar[h1] = p;
        return;
    }
    for (int64_t k = i; k < end; ++k) {
        const int64_t h = hval[k] >> 1;
        nbr[h] = m == 1 ? -1 : -2;
        hpar[h] = 0;
        fopen[h / 3] = 1;  // several threads may store the same 1
    }
}

__global__ __launch_bounds__(PF_BLOCK) void k_topo_init(u64* __restrict__ pw, int64_t n_tri) {
    const int64_t t = (int64_t)blockIdx.x * PF_BLOCK + threadIdx.x;
    if (t < n_tri) pw[t] = (u64)t << 1;
}

// the root of face t and the parity of t relative to it; parents are smaller than their children, so the walk ends
__device__ __forceinline__ void face_find(const u64* pw, int64_t t, int64_t& root, unsigned& par) {
    par = 0;
    for (;;) {
        const u64 w = word_load(&pw[t]);
        const int64_t p = (int64_t)(w >> 1);
        if (p == t) break;
        par ^= (unsigned)(w & 1ull);
        t = p;
    }
    root = t;
}

// one thread per half-edge; the lower face of a two-face edge acts for the edge
__global__ __launch_bounds__(PF_BLOCK) void k_topo_hook(const int32_t* __restrict__ nbr, const uint8_t* __restrict__ hpar, int64_t n_half,
                                                        u64* pw, int32_t* __restrict__ changed) {
    const int64_t h = (int64_t)blockIdx.x * PF_BLOCK + threadIdx.x;
    if (h >= n_half) return;
    const int64_t a = h / 3, b = nbr[h];
    if (b <= a) return;
    int64_t ra, rb;
    unsigned pa, pb;
    face_find(pw, a, ra, pa);
    face_find(pw, b, rb, pb);
    if (ra == rb) return;
    *changed = 1;
    const int64_t hi = ra > rb ? ra : rb, lo = ra > rb ? rb : ra;
    const unsigned q = pa ^ pb ^ (unsigned)hpar[h];  // rel[hi] ^ rel[lo]
    atomicMin(&pw[hi], ((u64)lo << 1) | q);
}

__global__ __launch_bounds__(PF_BLOCK) void k_topo_compress(u64* pw, int64_t n_tri) {
    const int64_t t = (int64_t)blockIdx.x * PF_BLOCK + threadIdx.x;
    if (t >= n_tri) return;
    int64_t r;
    unsigned par;
    face_find(pw, t, r, par);
    __hip_atomic_store(&pw[t], ((u64)r << 1) | par, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// after the labelling: pw[t] = (root << 1 | rel)
__global__ __launch_bounds__(PF_BLOCK) void k_topo_orient(const int32_t* __restrict__ nbr, const uint8_t* __restrict__ hpar, int64_t n_half,
                                                          const u64* __restrict__ pw, uint8_t* __restrict__ nonor) {
    const int64_t h = (int64_t)blockIdx.x * PF_BLOCK + threadIdx.x;
    if (h >= n_half) return;
    const int64_t a = h / 3, b = nbr[h];
    if (b <= a) return;
    const u64 wa = pw[a], wb = pw[b];
    if ((unsigned)((wa ^ wb) & 1ull) != (unsigned)hpar[h]) nonor[wa >> 1] = 1;
}

__global__ __launch_bounds__(PF_BLOCK) void k_topo_count(const u64* __restrict__ pw, const uint8_t* __restrict__ fopen, int64_t n_tri,
                                                         int32_t* __restrict__ n_in, int32_t* __restrict__ n_rel,
                                                         int32_t* __restrict__ popen) {
    const int64_t t = (int64_t)blockIdx.x * PF_BLOCK + threadIdx.x;
    const bool valid = t < n_tri;
    const u64 w = valid ? pw[t] : 0ull;
    const long long root = valid ? (long long)(w >> 1) : -1;
    const bool rel = valid && (w & 1ull), open = valid && fopen[t];
    const u64 live = __ballot(valid);
    if (live == 0ull) return;
    const int first = __ffsll((long long)live) - 1;
    const long long r0 = __shfl(root, first);
    if (__ballot(valid && root != r0) == 0ull) {  // one patch in this wave: one atomic each
        const int c_in = __popcll(live), c_rel = __popcll(__ballot(rel));
        const bool any_open = __ballot(open) != 0ull;
        if ((int)(threadIdx.x & (PF_WAVE - 1)) == first) {
            atomicAdd(&n_in[r0], c_in);
            if (c_rel) atomicAdd(&n_rel[r0], c_rel);
            if (any_open) atomicOr(&popen[r0], 1);
        }
        return;
    }
    if (!valid) return;
    atomicAdd(&n_in[root], 1);
    if (rel) atomicAdd(&n_rel[root], 1);
    if (open) atomicOr(&popen[root], 1);
}

// inv[root]: rel is reversed for the patch (it would reverse more than half of the faces; a tie keeps the root)
__global__ __launch_bounds__(PF_BLOCK) void k_topo_rule(const u64* __restrict__ pw, int64_t n_tri, const int32_t* __restrict__ n_in,
                                                        const int32_t* __restrict__ n_rel, const uint8_t* __restrict__ nonor,
                                                        uint8_t* __restrict__ inv) {
    const int64_t t = (int64_t)blockIdx.x * PF_BLOCK + threadIdx.x;
    if (t >= n_tri || (int64_t)(pw[t] >> 1) != t) return;
    inv[t] = !nonor[t] && 2 * (int64_t)n_rel[t] > (int64_t)n_in[t] ? 1 : 0;
}

__global__ __launch_bounds__(PF_BLOCK) void k_topo_terms(const u64* __restrict__ pw, int64_t n_tri, unsigned* __restrict__ rkey,
                                                         int32_t* __restrict__ fval) {
    const int64_t t = (int64_t)blockIdx.x * PF_BLOCK + threadIdx.x;
    if (t >= n_tri) return;
    rkey[t] = (unsigned)(pw[t] >> 1);
    fval[t] = (int32_t)t;
}

// faces sorted by patch: where each patch starts, and a . (b x c) of the face as it is after rel ^ inv
__global__ __launch_bounds__(PF_BLOCK) void k_seg_start(const unsigned* __restrict__ rkey, const int32_t* __restrict__ fval, int64_t n_tri,
                                                        const double* __restrict__ pts, const int32_t* __restrict__ faces,
                                                        const u64* __restrict__ pw, const uint8_t* __restrict__ inv,
                                                        int32_t* __restrict__ start, double* __restrict__ term) {
    const int64_t i = (int64_t)blockIdx.x * PF_BLOCK + threadIdx.x;
    if (i >= n_tri) return;
    const unsigned root = rkey[i];
    if (i == 0 || rkey[i - 1] != root) start[root] = (int32_t)i;
    const int64_t t = fval[i];
    const bool swap = ((unsigned)(pw[t] & 1ull) ^ (unsigned)inv[root]) != 0u;
    const int64_t va = faces[3 * t], vb = faces[3 * t + (swap ? 2 : 1)], vc = faces[3 * t + (swap ? 1 : 2)];
    const double a[3] = {pts[3 * va], pts[3 * va + 1], pts[3 * va + 2]};
    const double b[3] = {pts[3 * vb], pts[3 * vb + 1], pts[3 * vb + 2]};
    const double c[3] = {pts[3 * vc], pts[3 * vc + 1], pts[3 * vc + 2]};
    const double cr[3] = {b[1] * c[2] - b[2] * c[1], b[2] * c[0] - b[0] * c[2], b[0] * c[1] - b[1] * c[0]};
    term[i] = a[0] * cr[0] + a[1] * cr[1] + a[2] * cr[2];
}

// One level of the fixed tree.  With r the position inside its segment: the thread of a position with r % (256 stride)
// == 0 adds up to 256 entries of `in`, stride apart, as far as the segment goes; span == 0: the thread of the segment's
// first position adds every entry, stride apart.
__global__ __launch_bounds__(PF_BLOCK) void k_seg_sum(const unsigned* __restrict__ rkey, const int32_t* __restrict__ start, int64_t n_tri,
                                                      const double* __restrict__ in, double* __restrict__ out, int64_t stride,
                                                      int64_t span) {
    const int64_t i = (int64_t)blockIdx.x * PF_BLOCK + threadIdx.x;
    if (i >= n_tri) return;
    const unsigned root = rkey[i];
    const int64_t r = i - start[root];
    if (span ? r % span != 0 : r != 0) return;
    double sum = 0.0;
    for (int64_t k = 0, j = i; (span == 0 || k < 256) && j < n_tri && rkey[j] == root; ++k, j += stride) sum += in[j];
    out[i] = sum;
}

// the outward rule, per patch: sum6[start] = 6 V of the patch as rel ^ inv leaves it
__global__ __launch_bounds__(PF_BLOCK) void k_topo_outward(const u64* __restrict__ pw, int64_t n_tri, const int32_t* __restrict__ start,
                                                           const double* __restrict__ sum6, const uint8_t* __restrict__ nonor,
                                                           const int32_t* __restrict__ popen, uint8_t* __restrict__ inv,
                                                           double* __restrict__ vol) {
    const int64_t t = (int64_t)blockIdx.x * PF_BLOCK + threadIdx.x;
    if (t >= n_tri || (int64_t)(pw[t] >> 1) != t) return;
    if (nonor[t] || popen[t]) return;  // vol stays 0
    double v = sum6[start[t]] / 6.0;
    if (v < 0.0) {
        v = -v;
        inv[t] ^= 1;
    }
    vol[t] = v;
}

__global__ __launch_bounds__(PF_BLOCK) void k_topo_flip(const u64* __restrict__ pw, int64_t n_tri, const uint8_t* __restrict__ nonor,
                                                        const uint8_t* __restrict__ inv, int32_t* __restrict__ root_out,
                                                        uint8_t* __restrict__ flip) {
    const int64_t t = (int64_t)blockIdx.x * PF_BLOCK + threadIdx.x;
    if (t >= n_tri) return;
    const u64 w = pw[t];
    const int64_t root = (int64_t)(w >> 1);
    root_out[t] = (int32_t)root;
    flip[t] = nonor[root] ? 0 : (uint8_t)((unsigned)(w & 1ull) ^ (unsigned)inv[root]);
}

// ---- boundary loops: entries 2 h and 2 h + 1 are the two ends of half-edge h under (patch root << nb | vertex); every
// other half-edge goes behind them under (n_tri << nb)
__global__ __launch_bounds__(PF_BLOCK) void k_loop_keys(const int32_t* __restrict__ faces, const int32_t* __restrict__ nbr,
                                                        const u64* __restrict__ pw, int64_t n_half, int64_t n_tri, int nb,
                                                        u64* __restrict__ lkey, int32_t* __restrict__ lval, int32_t* __restrict__ lw) {
    const int64_t h = (int64_t)blockIdx.x * PF_BLOCK + threadIdx.x;
    if (h >= n_half) return;
    const int64_t t = h / 3;
    const int j = (int)(h - 3 * t);
    lval[2 * h] = lval[2 * h + 1] = (int32_t)h;
    if (nbr[h] != -1) {
        lkey[2 * h] = lkey[2 * h + 1] = (u64)n_tri << nb;
        lw[h] = -1;
        return;
    }
    const u64 root = pw[t] >> 1;
    lkey[2 * h] = (root << nb) | (u64)(unsigned)faces[h];
    lkey[2 * h + 1] = (root << nb) | (u64)(unsigned)faces[3 * t + he_next(j)];
    lw[h] = (int32_t)h;
}

__device__ __forceinline__ int32_t loop_find(const int32_t* lw, int32_t h) {
    for (;;) {
        const int32_t p = link_load(&lw[h]);
        if (p == h) return h;
        h = p;
    }
}

__global__ __launch_bounds__(PF_BLOCK) void k_loop_hook(const u64* __restrict__ lkey, const int32_t* __restrict__ lval, int64_t n_ent,
                                                        int64_t n_tri, int nb, int32_t* lw, int32_t* __restrict__ changed) {
    const int64_t i = (int64_t)blockIdx.x * PF_BLOCK + threadIdx.x;
    if (i + 1 >= n_ent) return;
    const u64 key = lkey[i];
    if ((int64_t)(key >> nb) >= n_tri || lkey[i + 1] != key) return;
    const int32_t ra = loop_find(lw, lval[i]), rb = loop_find(lw, lval[i + 1]);
    if (ra == rb) return;
    *changed = 1;
    atomicMin(&lw[ra > rb ? ra : rb], ra > rb ? rb : ra);
}

__global__ __launch_bounds__(PF_BLOCK) void k_loop_compress(int32_t* lw, int64_t n_half) {
    const int64_t h = (int64_t)blockIdx.x * PF_BLOCK + threadIdx.x;
    if (h >= n_half || link_load(&lw[h]) < 0) return;
    __hip_atomic_store(&lw[h], loop_find(lw, (int32_t)h), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

}  // namespace

extern "C" int pf_mesh_topology(pf_ctx* ctx, const double* pts, int64_t n, const int32_t* faces, int64_t n_faces, uint32_t flags,
                                int32_t* face_neighbours, int32_t* patch, uint8_t* flip, int32_t* boundary_loop,
                                uint8_t* patch_orientable, double* patch_volume, int64_t* report, double* device_ms) {
    PF_CHECK(ctx && faces, PF_E_ARG, "pf_mesh_topology: NULL argument");
    PF_CHECK(n > 0 && n < ((int64_t)1 << 31), PF_E_ARG, "pf_mesh_topology: n = %lld out of range", (long long)n);
    PF_CHECK(n_faces > 0 && 3 * n_faces < ((int64_t)1 << 31), PF_E_ARG,
             "pf_mesh_topology: %lld faces out of range (3 n_faces < 2^31)", (long long)n_faces);
    PF_CHECK((flags & ~(uint32_t)PF_TOPOLOGY_OUTWARD) == 0, PF_E_ARG, "pf_mesh_topology: unknown flags 0x%x", (unsigned)flags);
    const int64_t T = n_faces, H = 3 * T;
    PF_TRY(pf_check_faces("pf_mesh_topology", faces, T, 3, n, true));
    const int nb = pf_index_bits(n);       // bits of a vertex index
    const int rb = pf_index_bits(T + 1);   // bits of a face index and of the value T
    const bool volumes = pts && (flags & PF_TOPOLOGY_OUTWARD);
    PF_HIP(hipSetDevice(ctx->device));
    hipStream_t st = ctx->stream;
    StreamTimer timer(device_ms != nullptr);
    u64 counts[4] = {0, 0, 0, 0};
    int64_t rounds = 0, loop_rounds = 0;
    bool capped = false;
    std::vector<int32_t> h_root, h_loop;
    std::vector<uint8_t> h_nonor;
    std::vector<double> h_vol;
    hipError_t err;
    {
        Scratch sc(st);
        h_root.resize(T);
        if (boundary_loop) h_loop.assign(H, -1);
        if (patch_orientable) h_nonor.resize(T);
        if (patch_volume) h_vol.resize(T);
        double* d_pts = volumes ? sc.get<double>(3 * n) : nullptr;
        int32_t* d_faces = sc.get<int32_t>(H);
        u64 *ek0 = sc.get<u64>(H), *ek1 = sc.get<u64>(H);
        unsigned *hv0 = sc.get<unsigned>(H), *hv1 = sc.get<unsigned>(H);
        int32_t* nbr = sc.get<int32_t>(H);
        uint8_t* hpar = sc.get<uint8_t>(H);
        u64* pw = sc.get<u64>(T);
        // zeroed together: counts [4] | changed (as one u64) | per face: n_in, n_rel, popen (int32), vol (f64), fopen, nonor, inv
        u64* cnt = sc.get<u64>(5);
        int32_t* changed = (int32_t*)(cnt + 4);
        int32_t *n_in = sc.get<int32_t>(T), *n_rel = sc.get<int32_t>(T), *popen = sc.get<int32_t>(T);
        double* vol = sc.get<double>(T);
        uint8_t *fopen = sc.get<uint8_t>(T), *nonor = sc.get<uint8_t>(T), *inv = sc.get<uint8_t>(T), *d_flip = sc.get<uint8_t>(T);
        int32_t* d_root = sc.get<int32_t>(T);
        if (volumes) sc.upload(d_pts, pts, 3 * n);
        sc.upload(d_faces, faces, H);
        sc.zero(cnt, sizeof(u64) * 5);
        sc.zero(n_in, sizeof(int32_t) * T);
        sc.zero(n_rel, sizeof(int32_t) * T);
        sc.zero(popen, sizeof(int32_t) * T);
        sc.zero(vol, sizeof(double) * T);
        sc.zero(fopen, T);
        sc.zero(nonor, T);
        sc.zero(inv, T);
        timer.start(sc);
        if (sc.ok()) {
            k_topo_halfedges<<<pf_blocks(T), PF_BLOCK, 0, st>>>(d_faces, T, nb, ek0, hv0);
            sc.launched();
        }
        pf_sort_pairs(sc, ek0, ek1, hv0, hv1, H, 2 * nb);
        if (sc.ok()) {
            k_topo_edges<<<pf_blocks(H), PF_BLOCK, 0, st>>>(ek1, hv1, H, nbr, hpar, fopen, cnt);
            k_topo_init<<<pf_blocks(T), PF_BLOCK, 0, st>>>(pw, T);
            sc.launched();
        }
        sc.download(face_neighbours, nbr, H);
        // the labelling: a round hooks and compresses; the host reads the flag (the first time with the counts)
        for (bool more = true; sc.ok() && more;) {
            if (rounds > T) {
                capped = true;
                break;
            }
            int32_t h_changed = 0;
            if (rounds) sc.zero(changed, sizeof(int32_t));
            if (sc.ok()) {
                k_topo_hook<<<pf_blocks(H), PF_BLOCK, 0, st>>>(nbr, hpar, H, pw, changed);
                k_topo_compress<<<pf_blocks(T), PF_BLOCK, 0, st>>>(pw, T);
                sc.launched();
            }
            if (!rounds) sc.download(counts, cnt, 4);
            sc.download(&h_changed, changed, 1);
            sc.sync();
            ++rounds;
            more = h_changed != 0;
        }
        if (sc.ok() && !capped) {
            k_topo_orient<<<pf_blocks(H), PF_BLOCK, 0, st>>>(nbr, hpar, H, pw, nonor);
            k_topo_count<<<pf_blocks(T), PF_BLOCK, 0, st>>>(pw, fopen, T, n_in, n_rel, popen);
            k_topo_rule<<<pf_blocks(T), PF_BLOCK, 0, st>>>(pw, T, n_in, n_rel, nonor, inv);
            sc.launched();
        }
        if (volumes && !capped) {
            unsigned *rk0 = sc.get<unsigned>(T), *rk1 = sc.get<unsigned>(T);
            int32_t *fv0 = sc.get<int32_t>(T), *fv1 = sc.get<int32_t>(T), *start = sc.get<int32_t>(T);
            double *sa = sc.get<double>(T), *sb = sc.get<double>(T);
            if (sc.ok()) {
                k_topo_terms<<<pf_blocks(T), PF_BLOCK, 0, st>>>(pw, T, rk0, fv0);
                sc.launched();
            }
            pf_sort_pairs(sc, rk0, rk1, fv0, fv1, T, rb);
            if (sc.ok()) {
                k_seg_start<<<pf_blocks(T), PF_BLOCK, 0, st>>>(rk1, fv1, T, d_pts, d_faces, pw, inv, start, sa);
                k_seg_sum<<<pf_blocks(T), PF_BLOCK, 0, st>>>(rk1, start, T, sa, sb, 1, 256);
                k_seg_sum<<<pf_blocks(T), PF_BLOCK, 0, st>>>(rk1, start, T, sb, sa, 256, 65536);
                k_seg_sum<<<pf_blocks(T), PF_BLOCK, 0, st>>>(rk1, start, T, sa, sb, 65536, 0);
                k_topo_outward<<<pf_blocks(T), PF_BLOCK, 0, st>>>(pw, T, start, sb, nonor, popen, inv, vol);
                sc.launched();
            }
        }
        if (sc.ok() && !capped) {
            k_topo_flip<<<pf_blocks(T), PF_BLOCK, 0, st>>>(pw, T, nonor, inv, d_root, d_flip);
            sc.launched();
        }
        if (!capped) {
            sc.download(h_root.data(), d_root, T);
            sc.download(flip, d_flip, T);
            sc.download(patch_orientable ? h_nonor.data() : nullptr, nonor, T);
            sc.download(patch_volume ? h_vol.data() : nullptr, vol, T);
        }
        if (boundary_loop && counts[1] > 0 && !capped) {
            const int64_t E = 2 * H;
            u64 *lk0 = sc.get<u64>(E), *lk1 = sc.get<u64>(E);
            int32_t *lv0 = sc.get<int32_t>(E), *lv1 = sc.get<int32_t>(E), *lw = sc.get<int32_t>(H);
            if (sc.ok()) {
                k_loop_keys<<<pf_blocks(H), PF_BLOCK, 0, st>>>(d_faces, nbr, pw, H, T, nb, lk0, lv0, lw);
                sc.launched();
            }
            pf_sort_pairs(sc, lk0, lk1, lv0, lv1, E, nb + rb);
            for (bool more = true; sc.ok() && more;) {
                if (loop_rounds > H) {
                    capped = true;
                    break;
                }
                int32_t h_changed = 0;
                sc.zero(changed, sizeof(int32_t));
                if (sc.ok()) {
                    k_loop_hook<<<pf_blocks(E), PF_BLOCK, 0, st>>>(lk1, lv1, E, T, nb, lw, changed);
                    k_loop_compress<<<pf_blocks(H), PF_BLOCK, 0, st>>>(lw, H);
                    sc.launched();
                }
                sc.download(&h_changed, changed, 1);
                sc.sync();
                ++loop_rounds;
                more = h_changed != 0;
            }
            sc.download(h_loop.data(), lw, H);
        }
        timer.stop(sc);
        sc.sync();
        timer.read(sc, device_ms);
        err = sc.err;
    }
    if (err != hipSuccess) return pf_hip_failed("pf_mesh_topology", err);
    PF_CHECK(!capped, PF_E_INTERNAL, "pf_mesh_topology: the labelling did not settle within %lld rounds (faces) / %lld rounds (loops)",
             (long long)rounds, (long long)loop_rounds);
    // dense ids in ascending order of the smallest member: a root is its set's smallest member, and never follows a member
    int64_t n_patches = 0, n_loops = 0;
    {
        std::vector<int32_t> id(T);
        for (int64_t t = 0; t < T; ++t) {
            const int32_t r = h_root[t];
            if (r == t) {
                if (patch_orientable) patch_orientable[n_patches] = h_nonor[t] ? 0 : 1;
                if (patch_volume) patch_volume[n_patches] = h_vol[t];
                id[t] = (int32_t)n_patches++;
            }
            if (patch) patch[t] = id[r];
        }
    }
    if (boundary_loop) {
        std::vector<int32_t> id(H);
        for (int64_t h = 0; h < H; ++h) {
            const int32_t r = h_loop[h];
            if (r == h) id[h] = (int32_t)n_loops++;
            boundary_loop[h] = r < 0 ? -1 : id[r];
        }
    }
    if (report) {
        for (int k = 0; k < 4; ++k) report[k] = (int64_t)counts[k];
        report[4] = n_patches;
        report[5] = boundary_loop ? n_loops : -1;
        report[6] = rounds;
        report[7] = loop_rounds;
    }
    return PF_OK;
}
