// A population of S shapes in correspondence, resident in HBM (pf_shapes_*): what generalized Procrustes alignment and the
// principal modes of the population need from the device.  X [S][n][3], the weights w [n] (or none: every weight 1.0) and
// a reference shape r [n][3] stay on the device; the host gets the small sums (3 S centroids, 10 S + 1 alignment sums, the
// S x S Gram matrix, S x K scores) and sends the small parameters (S rotations, K x S coefficients).  Every dense step
// (3 x 3 SVD, S x S eigenproblem) is the caller's, on the host.  The definitions are in include/pyfocusr_hip.h;
// tests/_shape_model_ref.py restates them in numpy.
//
// T(.) is the sum over the vertices in ascending order along the library's fixed tree (pf_map_quality.hip): 256
// consecutive terms left to right from 0.0, 256 of those sums likewise, the rest in order.
//
//   k_sh_center_sums / k_sh_align_sums  one block per 256 consecutive vertices of one shape: thread i writes the terms of
//                  vertex i to LDS, thread q then adds the 256 terms of quantity q left to right: level 1 of the tree
//   k_sh_mean      one block per 256 vertices: thread i adds the shapes' coordinates left to right, divides, takes the
//                  term of `change` against the old reference and overwrites the reference; thread 0 adds the terms
//   k_tree_level   levels 2 and 3 of the tree for every quantity (pf_tree.h; partials are [node][quantity])
//   k_sh_pairs     T(w . dot3(a_s, b_t)) for 16 x 16 pairs (s, t) per block, one pair per thread, the 2 x 16 shapes
//                  staged through LDS 32 vertices at a time; the Gram (a = b = x - r, the tiles of the upper triangle) and
//                  the scores (b = the modes, every tile)
//   k_sh_center_apply, k_sh_transform, k_sh_combine  elementwise
//
// The split of k_sh_pairs.  Level-1 partial sums of every pair are n / 256 x (16-padded S)^2 / 2 doubles: 56 MB at S = 100,
// n = 250k, but 4 GB at S = 1024.  So a block either covers ONE run of 256 vertices and writes its level-1 sum (n / 256
// blocks per tile: enough blocks for any S), or - when those partials would pass SH_LEVEL1_MAX doubles (1 GiB) - it
// carries both levels in registers over the 65 536 consecutive vertices of one level-2 node and writes that node's sum
// (n / 65 536 blocks per tile, scratch 256 times smaller).  The second form is only taken when tiles x runs > 524 288, i.e.
// with at least 2048 blocks, more than the 1536 the 256 CUs hold at six per CU.  (With the threshold at 256 MB, S = 300 at
// n = 250k took the second form with 760 blocks: 15.6 ms against 11.1 ms for the first; forced onto S = 100 with its 112
// blocks: 12.7 ms against 1.9 ms - profiles/shape_model.md.)  Both add the same terms in the same order: the bits do not
// depend on the form.  (PF_SHAPES_LEVEL1_MAX in the environment overrides the threshold: the tests run both forms on
// small populations.)
//
// No floating-point atomics, no block waits for another: two calls give the same bits.  Arithmetic: f64, separate
// multiplies and adds (-ffp-contract=off), dot3(a, b) = (a0 b0 + a1 b1) + a2 b2.
#include <cmath>
#include <cstdlib>

#include "pf_internal.h"
#include "pf_tree.h"

struct pf_shapes {
    pf_ctx* ctx = nullptr;
    int32_t S = 0;
    int64_t n = 0;
    double* X = nullptr;  // [S][n][3]
    double* w = nullptr;  // [n], or NULL: every weight 1.0
    double* r = nullptr;  // [n][3] the reference shape
    double W = 0.0;       // T(w_i)
    bool timed = false;   // pf_shapes_device_ms
    double last_ms = 0.0;
};

namespace {

constexpr int SH_GROUP = 256;              // terms per node of the tree
constexpr int SH_STRIDE = SH_GROUP + 1;    // a quantity's terms in LDS: the rows of different quantities start on different banks
constexpr int SH_TILE = 16;                // shapes per side of a pair tile: 16 x 16 pairs = the block's 256 threads
constexpr int SH_SUB = 32;                 // vertices staged at a time: 2 x 16 x 32 x 3 doubles = 24 KB of LDS, six blocks per CU
constexpr int SH_ROW = 3 * SH_SUB + 1;     // a staged shape's row; odd, so that the 16 shapes a half-wave reads lie on 16 bank pairs
constexpr int SH_KT = 16;                  // outputs of pf_shapes_combine a thread keeps in registers per pass over the population
constexpr int64_t SH_LEVEL1_MAX = (int64_t)1 << 27;  // doubles of level-1 partials k_sh_pairs may write (1 GiB)
static_assert(SH_GROUP % SH_SUB == 0 && SH_TILE * SH_TILE == PF_BLOCK && SH_GROUP == PF_BLOCK, "k_sh_pairs' tiling");
static_assert(SH_GROUP == PF_TREE_GROUP, "level 1 here, the levels above it in pf_tree.h");

__device__ __forceinline__ double sh_dot3(const double* a, const double* b) { return (a[0] * b[0] + a[1] * b[1]) + a[2] * b[2]; }

// Level 1 of the centroids' sums.  Grid (runs, S).  lev1[run][3 s + a] = the run's sum of w_i x_sia.
__global__ __launch_bounds__(PF_BLOCK) void k_sh_center_sums(const double* __restrict__ X, const double* __restrict__ w, int64_t n,
                                                             int64_t rows, double* __restrict__ lev1) {
    __shared__ double term[3][SH_STRIDE];
    const int64_t g = blockIdx.x, s = blockIdx.y, i = g * SH_GROUP + threadIdx.x;
    const int cnt = (int)(n - g * SH_GROUP < SH_GROUP ? n - g * SH_GROUP : SH_GROUP);
    if (i < n) {
        const double wi = w ? w[i] : 1.0;
        const double* p = X + (s * n + i) * 3;
#pragma unroll
        for (int a = 0; a < 3; ++a) term[a][threadIdx.x] = wi * p[a];
    }
    __syncthreads();
    if (threadIdx.x < 3) {
        double sum = 0.0;
        for (int k = 0; k < cnt; ++k) sum += term[threadIdx.x][k];
        lev1[g * rows + s * 3 + threadIdx.x] = sum;
    }
}

__global__ __launch_bounds__(PF_BLOCK) void k_sh_divide(double* __restrict__ v, int64_t count, double by) {
    const int64_t i = (int64_t)blockIdx.x * PF_BLOCK + threadIdx.x;
    if (i < count) v[i] = v[i] / by;
}

// x_sia <- x_sia - c[3 s + a].  Grid (blocks of 3 n, S).
__global__ __launch_bounds__(PF_BLOCK) void k_sh_center_apply(double* __restrict__ X, int64_t n3, const double* __restrict__ c) {
    const int64_t e = (int64_t)blockIdx.x * PF_BLOCK + threadIdx.x, s = blockIdx.y;
    if (e >= n3) return;
    X[s * n3 + e] = X[s * n3 + e] - c[s * 3 + e % 3];
}

// m_i = ((x_first,i + x_first+1,i) + ...) / count per coordinate; lev1[run] = the run's sum of w_i dot3(m_i - r_i, m_i - r_i)
// against the reference as it was; then r_i <- m_i.  Grid (runs).
__global__ __launch_bounds__(PF_BLOCK) void k_sh_mean(const double* __restrict__ X, const double* __restrict__ w, double* __restrict__ r,
                                                      int64_t n, int32_t first, int32_t count, double* __restrict__ lev1) {
    __shared__ double term[SH_GROUP];
    const int64_t g = blockIdx.x, i = g * SH_GROUP + threadIdx.x;
    const int cnt = (int)(n - g * SH_GROUP < SH_GROUP ? n - g * SH_GROUP : SH_GROUP);
    if (i < n) {
        double d[3];
#pragma unroll
        for (int a = 0; a < 3; ++a) {
            double acc = X[((int64_t)first * n + i) * 3 + a];
            for (int32_t s = 1; s < count; ++s) acc += X[((int64_t)(first + s) * n + i) * 3 + a];
            const double m = acc / (double)count;
            d[a] = m - r[i * 3 + a];
            r[i * 3 + a] = m;
        }
        term[threadIdx.x] = (w ? w[i] : 1.0) * sh_dot3(d, d);
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        double sum = 0.0;
        for (int k = 0; k < cnt; ++k) sum += term[k];
        lev1[g] = sum;
    }
}

// Level 1 of the alignment sums.  Grid (runs, S).  Quantities 10 s + 3 a + b: (w_i x_sia) r_ib; 10 s + 9: w_i dot3(x_si, x_si);
// 10 S (written by the blocks of shape 0): w_i dot3(r_i, r_i).
__global__ __launch_bounds__(PF_BLOCK) void k_sh_align_sums(const double* __restrict__ X, const double* __restrict__ w,
                                                            const double* __restrict__ r, int64_t n, int32_t S, int64_t rows,
                                                            double* __restrict__ lev1) {
    __shared__ double term[11][SH_STRIDE];
    const int64_t g = blockIdx.x, s = blockIdx.y, i = g * SH_GROUP + threadIdx.x;
    const int cnt = (int)(n - g * SH_GROUP < SH_GROUP ? n - g * SH_GROUP : SH_GROUP);
    if (i < n) {
        const double wi = w ? w[i] : 1.0;
        const double* p = X + (s * n + i) * 3;
        const double x[3] = {p[0], p[1], p[2]}, ri[3] = {r[i * 3], r[i * 3 + 1], r[i * 3 + 2]};
#pragma unroll
        for (int a = 0; a < 3; ++a) {
            const double wx = wi * x[a];
#pragma unroll
            for (int b = 0; b < 3; ++b) term[3 * a + b][threadIdx.x] = wx * ri[b];
        }
        term[9][threadIdx.x] = wi * sh_dot3(x, x);
        term[10][threadIdx.x] = wi * sh_dot3(ri, ri);
    }
    __syncthreads();
    const int q = threadIdx.x;
    if (q < 10 || (q == 10 && s == 0)) {
        double sum = 0.0;
        for (int k = 0; k < cnt; ++k) sum += term[q][k];
        lev1[g * rows + (q < 10 ? s * 10 + q : (int64_t)S * 10)] = sum;
    }
}

// y_b = scale_s ((x0 R[0][b] + x1 R[1][b]) + x2 R[2][b]) (+ t_s[b]) in place.  P [S][13] = R [9] | scale | t [3].  Grid (blocks of n, S).
__global__ __launch_bounds__(PF_BLOCK) void k_sh_transform(double* __restrict__ X, int64_t n, const double* __restrict__ P, int has_t) {
    const int64_t i = (int64_t)blockIdx.x * PF_BLOCK + threadIdx.x, s = blockIdx.y;
    if (i >= n) return;
    const double* R = P + s * 13;
    double* p = X + (s * n + i) * 3;
    const double x0 = p[0], x1 = p[1], x2 = p[2], scale = R[9];
#pragma unroll
    for (int b = 0; b < 3; ++b) {
        const double y = scale * ((x0 * R[b] + x1 * R[3 + b]) + x2 * R[6 + b]);
        p[b] = has_t ? y + R[10 + b] : y;
    }
}

// part[node][256 y + 16 ty + tx] = the node's sum of w_i dot3(a_i, b_i) for a = A[16 ta + ty] - ra, b = B[16 tb + tx] - rb
// (ra, rb may be NULL: nothing is subtracted); a shape beyond SA / SB counts as zeros.  carry == 0: a node is one run of 256
// vertices (level 1).  carry == 1: a node is 65 536 vertices, the run sums added left to right from 0.0 (level 2).
// Grid (nodes, tiles).
__global__ __launch_bounds__(PF_BLOCK) void k_sh_pairs(const double* __restrict__ A, const double* __restrict__ ra, int32_t SA,
                                                       const double* __restrict__ B, const double* __restrict__ rb, int32_t SB,
                                                       const double* __restrict__ w, int64_t n, int tri, int tiles_b, int carry, int64_t rows,
                                                       double* __restrict__ part) {
    __shared__ double la[SH_TILE][SH_ROW], lb[SH_TILE][SH_ROW], lw[SH_SUB];
    const int tx = threadIdx.x % SH_TILE, ty = threadIdx.x / SH_TILE;
    // the tile (ta, tb): the blockIdx.y-th of the upper triangle, column by column (tri), or of the tiles_b-wide rectangle
    const int y = (int)blockIdx.y;
    int ta = y / tiles_b, tb = y - ta * tiles_b;
    if (tri) {
        tb = 0;
        while ((tb + 1) * (tb + 2) / 2 <= y) ++tb;
        ta = y - tb * (tb + 1) / 2;
    }
    const int a0 = ta * SH_TILE, b0 = tb * SH_TILE;
    const int64_t span = carry ? (int64_t)SH_GROUP * SH_GROUP : SH_GROUP;
    const int64_t v_lo = (int64_t)blockIdx.x * span, v_hi = v_lo + span < n ? v_lo + span : n;
    double acc2 = 0.0;
    for (int64_t run = v_lo; run < v_hi; run += SH_GROUP) {
        const int64_t run_hi = run + SH_GROUP < v_hi ? run + SH_GROUP : v_hi;
        double acc1 = 0.0;
        for (int64_t v0 = run; v0 < run_hi; v0 += SH_SUB) {
            const int cnt = (int)(run_hi - v0 < SH_SUB ? run_hi - v0 : SH_SUB);
            __syncthreads();
            for (int idx = threadIdx.x; idx < SH_TILE * 3 * SH_SUB; idx += PF_BLOCK) {
                const int sh = idx / (3 * SH_SUB), off = idx - sh * (3 * SH_SUB);
                double va = 0.0, vb = 0.0;
                if (off < 3 * cnt) {
                    if (a0 + sh < SA) {
                        va = A[((int64_t)(a0 + sh) * n + v0) * 3 + off];
                        if (ra) va = va - ra[v0 * 3 + off];
                    }
                    if (b0 + sh < SB) {
                        vb = B[((int64_t)(b0 + sh) * n + v0) * 3 + off];
                        if (rb) vb = vb - rb[v0 * 3 + off];
                    }
                }
                la[sh][off] = va;
                lb[sh][off] = vb;
            }
            if (threadIdx.x < SH_SUB) lw[threadIdx.x] = (int)threadIdx.x < cnt ? (w ? w[v0 + threadIdx.x] : 1.0) : 0.0;
            __syncthreads();
            for (int k = 0; k < cnt; ++k) acc1 += lw[k] * sh_dot3(&la[ty][3 * k], &lb[tx][3 * k]);
        }
        acc2 = carry ? acc2 + acc1 : acc1;
    }
    part[(int64_t)blockIdx.x * rows + (int64_t)blockIdx.y * PF_BLOCK + threadIdx.x] = acc2;
}

// The pair sums out of their tiles: out[s][t] (SA x SB, row-major); tri: s <= t is read and written to [s][t] and [t][s].
__global__ __launch_bounds__(PF_BLOCK) void k_sh_pairs_finish(const double* __restrict__ sums, int32_t SA, int32_t SB, int tri, int tiles_b,
                                                              double* __restrict__ out) {
    const int64_t idx = (int64_t)blockIdx.x * PF_BLOCK + threadIdx.x;
    if (idx >= (int64_t)SA * SB) return;
    const int s = (int)(idx / SB), t = (int)(idx - (int64_t)s * SB);
    if (tri && s > t) return;
    const int ta = s / SH_TILE, tb = t / SH_TILE;
    const int64_t y = tri ? (int64_t)tb * (tb + 1) / 2 + ta : (int64_t)ta * tiles_b + tb;
    const double v = sums[y * PF_BLOCK + (s % SH_TILE) * SH_TILE + t % SH_TILE];
    out[(int64_t)s * SB + t] = v;
    if (tri) out[(int64_t)t * SB + s] = v;
}

// out[k][e] = sum over s, left to right from 0.0, of coeff[k][s] (x_s[e] - r[e]) for the SH_KT values of k of blockIdx.y.
__global__ __launch_bounds__(PF_BLOCK) void k_sh_combine(const double* __restrict__ X, const double* __restrict__ r, int64_t n3, int32_t S,
                                                         const double* __restrict__ coeff, int32_t K, double* __restrict__ out) {
    const int64_t e = (int64_t)blockIdx.x * PF_BLOCK + threadIdx.x;
    const int k0 = blockIdx.y * SH_KT;
    if (e >= n3) return;
    const double* row[SH_KT];  // (a k beyond K reads the last row and is not written)
#pragma unroll
    for (int j = 0; j < SH_KT; ++j) row[j] = coeff + (int64_t)(k0 + j < K ? k0 + j : K - 1) * S;
    double acc[SH_KT];
#pragma unroll
    for (int j = 0; j < SH_KT; ++j) acc[j] = 0.0;
    const double re = r[e];
    for (int32_t s = 0; s < S; ++s) {
        const double d = X[(int64_t)s * n3 + e] - re;
#pragma unroll
        for (int j = 0; j < SH_KT; ++j) acc[j] += row[j][s] * d;
    }
#pragma unroll
    for (int j = 0; j < SH_KT; ++j)
        if (k0 + j < K) out[(int64_t)(k0 + j) * n3 + e] = acc[j];
}

bool all_finite(const double* p, int64_t count) {
    for (int64_t i = 0; i < count; ++i)
        if (!std::isfinite(p[i])) return false;
    return true;
}

// T(w_i) on the host, as k_tree_level adds it
double tree_sum_host(const double* w, int64_t n) {
    double total = 0.0, a2 = 0.0, a1 = 0.0;
    int c1 = 0, c2 = 0;
    for (int64_t i = 0; i < n; ++i) {
        a1 += w[i];
        if (++c1 == SH_GROUP) {
            a2 += a1, a1 = 0.0, c1 = 0;
            if (++c2 == SH_GROUP) total += a2, a2 = 0.0, c2 = 0;
        }
    }
    if (c1) a2 += a1, ++c2;
    if (c2) total += a2;
    return total;
}

int64_t runs_of(int64_t n) { return (n + SH_GROUP - 1) / SH_GROUP; }

// the pair sums of k_sh_pairs on the device as out [SA][SB] (a Scratch block)
double* pair_sums(Scratch& sc, const pf_shapes* h, const double* B, const double* rb, int32_t SB, int tri) {
    const int64_t n = h->n, n1 = runs_of(n), n2 = runs_of(n1);
    const int tiles_a = (h->S + SH_TILE - 1) / SH_TILE, tiles_b = (SB + SH_TILE - 1) / SH_TILE;
    const int tiles = tri ? tiles_a * (tiles_a + 1) / 2 : tiles_a * tiles_b;
    const int64_t rows = (int64_t)tiles * PF_BLOCK;
    int64_t cap = SH_LEVEL1_MAX;
    if (const char* env = getenv("PF_SHAPES_LEVEL1_MAX")) cap = atoll(env);
    const int carry = n1 * rows > cap;
    const int64_t nodes = carry ? n2 : n1;
    double* part = sc.get<double>(nodes * rows);
    double* out = sc.get<double>((int64_t)h->S * SB);
    if (sc.ok())
        k_sh_pairs<<<dim3((unsigned)nodes, (unsigned)tiles), PF_BLOCK, 0, sc.st>>>(h->X, h->r, h->S, B, rb, SB, h->w, n, tri, tiles_b, carry, rows, part);
    double* sums = pf_tree_reduce(sc, part, nodes, rows, carry ? 2 : 1);
    if (sc.ok()) {
        k_sh_pairs_finish<<<pf_blocks((int64_t)h->S * SB), PF_BLOCK, 0, sc.st>>>(sums, h->S, SB, tri, tiles_b, out);
        sc.launched();
    }
    return out;
}

// the end of every entry point, behind timer.stop and the downloads: the wait, the device time where it is kept, the error
int finish(pf_shapes* h, Scratch& sc, StreamTimer& timer, const char* fn) {
    sc.sync();
    timer.read(sc, &h->last_ms);
    return sc.ok() ? PF_OK : pf_hip_failed(fn, sc.err);
}

}  // namespace

extern "C" {

void pf_shapes_free(pf_shapes* h) {
    if (!h) return;
    hipSetDevice(h->ctx->device);
    hipStreamSynchronize(h->ctx->stream);
    hipStream_t st = h->ctx->stream;
    pf_free(st, h->X);
    pf_free(st, h->w);
    pf_free(st, h->r);
    delete h;
}

int pf_shapes_create(pf_ctx* ctx, const double* shapes, int32_t S, int64_t n, const double* weights, pf_shapes** out) {
    PF_CHECK(ctx && shapes && out, PF_E_ARG, "pf_shapes_create: NULL argument");
    PF_CHECK(S >= 1 && S <= 1024, PF_E_ARG, "pf_shapes_create: S = %d out of range (1..1024)", (int)S);
    PF_CHECK(n >= 1 && n < ((int64_t)1 << 31), PF_E_ARG, "pf_shapes_create: n = %lld out of range (1..2^31-1)", (long long)n);
    PF_CHECK(all_finite(shapes, (int64_t)S * n * 3), PF_E_ARG, "pf_shapes_create: a coordinate is not finite");
    double W = (double)n;
    if (weights) {
        for (int64_t i = 0; i < n; ++i)
            PF_CHECK(std::isfinite(weights[i]) && weights[i] >= 0.0, PF_E_ARG, "pf_shapes_create: weight %lld is negative or not finite",
                     (long long)i);
        W = tree_sum_host(weights, n);
    }
    PF_CHECK(W > 0.0, PF_E_DEGENERATE, "pf_shapes_create: the weights sum to 0");
    PF_CHECK(std::isfinite(W), PF_E_ARG, "pf_shapes_create: the weights' sum is not finite");
    PF_HIP(hipSetDevice(ctx->device));
    pf_shapes* h = new pf_shapes();
    h->ctx = ctx, h->S = S, h->n = n, h->W = W;
    Scratch sc(ctx->stream);  // every block is kept: the handle owns them, and pf_shapes_free gives back whatever a failure leaves
    h->X = sc.keep<double>((size_t)S * n * 3);
    h->r = sc.keep<double>((size_t)n * 3);
    if (weights) h->w = sc.keep<double>((size_t)n);
    sc.upload(h->X, shapes, (size_t)S * n * 3);
    if (weights) sc.upload(h->w, weights, (size_t)n);
    sc.zero(h->r, sizeof(double) * (size_t)n * 3);
    sc.sync();
    if (!sc.ok()) {
        const hipError_t err = sc.err;
        pf_shapes_free(h);
        return pf_hip_failed("pf_shapes_create", err);
    }
    *out = h;
    return PF_OK;
}

int pf_shapes_center(pf_shapes* h, double* centroids_out) {
    PF_CHECK(h != nullptr, PF_E_ARG, "pf_shapes_center: NULL handle");
    PF_HIP(hipSetDevice(h->ctx->device));
    hipStream_t st = h->ctx->stream;
    const int64_t n = h->n, n1 = runs_of(n), rows = (int64_t)h->S * 3;
    Scratch sc(st);
    StreamTimer timer(h->timed);
    double* lev1 = sc.get<double>(n1 * rows);
    timer.start(sc);
    if (sc.ok()) k_sh_center_sums<<<dim3((unsigned)n1, (unsigned)h->S), PF_BLOCK, 0, st>>>(h->X, h->w, n, rows, lev1);
    double* c = pf_tree_reduce(sc, lev1, n1, rows, 1);
    if (sc.ok()) {
        k_sh_divide<<<pf_blocks(rows), PF_BLOCK, 0, st>>>(c, rows, h->W);
        k_sh_center_apply<<<dim3(pf_blocks(3 * n), (unsigned)h->S), PF_BLOCK, 0, st>>>(h->X, 3 * n, c);
        sc.launched();
    }
    timer.stop(sc);
    sc.download(centroids_out, c, rows);
    return finish(h, sc, timer, "pf_shapes_center");
}

int pf_shapes_mean(pf_shapes* h, int32_t first, int32_t count, double* mean_out, double* change_out) {
    PF_CHECK(h != nullptr, PF_E_ARG, "pf_shapes_mean: NULL handle");
    PF_CHECK(first >= 0 && count >= 1 && first < h->S && count <= h->S - first, PF_E_ARG,
             "pf_shapes_mean: shapes %d .. %d + %d out of range (S = %d)", (int)first, (int)first, (int)count, (int)h->S);
    PF_HIP(hipSetDevice(h->ctx->device));
    hipStream_t st = h->ctx->stream;
    const int64_t n = h->n, n1 = runs_of(n);
    Scratch sc(st);
    StreamTimer timer(h->timed);
    double* lev1 = sc.get<double>(n1);
    timer.start(sc);
    if (sc.ok()) k_sh_mean<<<(unsigned)n1, PF_BLOCK, 0, st>>>(h->X, h->w, h->r, n, first, count, lev1);
    double* change = pf_tree_reduce(sc, lev1, n1, 1, 1);
    timer.stop(sc);
    sc.download(mean_out, h->r, 3 * n);
    sc.download(change_out, change, 1);
    return finish(h, sc, timer, "pf_shapes_mean");
}

int pf_shapes_align_sums(pf_shapes* h, double* cross_out, double* norm2_out, double* ref_norm2_out) {
    PF_CHECK(h != nullptr, PF_E_ARG, "pf_shapes_align_sums: NULL handle");
    PF_HIP(hipSetDevice(h->ctx->device));
    hipStream_t st = h->ctx->stream;
    const int32_t S = h->S;
    const int64_t n = h->n, n1 = runs_of(n), rows = (int64_t)S * 10 + 1;
    std::vector<double> sums((size_t)rows);
    Scratch sc(st);
    StreamTimer timer(h->timed);
    double* lev1 = sc.get<double>(n1 * rows);
    timer.start(sc);
    if (sc.ok()) k_sh_align_sums<<<dim3((unsigned)n1, (unsigned)S), PF_BLOCK, 0, st>>>(h->X, h->w, h->r, n, S, rows, lev1);
    double* d_sums = pf_tree_reduce(sc, lev1, n1, rows, 1);
    timer.stop(sc);
    sc.download(sums.data(), d_sums, rows);
    PF_TRY(finish(h, sc, timer, "pf_shapes_align_sums"));
    for (int32_t s = 0; s < S; ++s) {
        if (cross_out)
            for (int q = 0; q < 9; ++q) cross_out[s * 9 + q] = sums[(size_t)s * 10 + q];
        if (norm2_out) norm2_out[s] = sums[(size_t)s * 10 + 9];
    }
    if (ref_norm2_out) *ref_norm2_out = sums[(size_t)S * 10];
    return PF_OK;
}

int pf_shapes_transform(pf_shapes* h, const double* R, const double* scale, const double* t) {
    PF_CHECK(h && R && scale, PF_E_ARG, "pf_shapes_transform: NULL argument");
    const int32_t S = h->S;
    PF_CHECK(all_finite(R, (int64_t)S * 9), PF_E_ARG, "pf_shapes_transform: a rotation is not finite");
    PF_CHECK(all_finite(scale, S), PF_E_ARG, "pf_shapes_transform: a scale is not finite");
    PF_CHECK(!t || all_finite(t, (int64_t)S * 3), PF_E_ARG, "pf_shapes_transform: a translation is not finite");
    std::vector<double> P((size_t)S * 13, 0.0);
    for (int32_t s = 0; s < S; ++s) {
        for (int q = 0; q < 9; ++q) P[(size_t)s * 13 + q] = R[s * 9 + q];
        P[(size_t)s * 13 + 9] = scale[s];
        for (int b = 0; t && b < 3; ++b) P[(size_t)s * 13 + 10 + b] = t[s * 3 + b];
    }
    PF_HIP(hipSetDevice(h->ctx->device));
    hipStream_t st = h->ctx->stream;
    Scratch sc(st);
    StreamTimer timer(h->timed);
    double* d_P = sc.get<double>(P.size());
    sc.upload(d_P, P.data(), P.size());
    timer.start(sc);
    if (sc.ok()) {
        k_sh_transform<<<dim3(pf_blocks(h->n), (unsigned)S), PF_BLOCK, 0, st>>>(h->X, h->n, d_P, t != nullptr);
        sc.launched();
    }
    timer.stop(sc);
    return finish(h, sc, timer, "pf_shapes_transform");  // (P is the call's own: the wait ends its use)
}

int pf_shapes_gram(pf_shapes* h, double* gram_out) {
    PF_CHECK(h && gram_out, PF_E_ARG, "pf_shapes_gram: NULL argument");
    PF_HIP(hipSetDevice(h->ctx->device));
    Scratch sc(h->ctx->stream);
    StreamTimer timer(h->timed);
    timer.start(sc);
    double* G = pair_sums(sc, h, h->X, h->r, h->S, 1);
    timer.stop(sc);
    sc.download(gram_out, G, (size_t)h->S * h->S);
    return finish(h, sc, timer, "pf_shapes_gram");
}

int pf_shapes_scores(pf_shapes* h, const double* modes, int32_t K, double* scores_out) {
    PF_CHECK(h && modes && scores_out, PF_E_ARG, "pf_shapes_scores: NULL argument");
    PF_CHECK(K >= 1 && K <= 1024, PF_E_ARG, "pf_shapes_scores: K = %d out of range (1..1024)", (int)K);
    PF_CHECK(all_finite(modes, (int64_t)K * h->n * 3), PF_E_ARG, "pf_shapes_scores: a mode's coordinate is not finite");
    PF_HIP(hipSetDevice(h->ctx->device));
    Scratch sc(h->ctx->stream);
    StreamTimer timer(h->timed);
    double* d_modes = sc.get<double>((size_t)K * h->n * 3);
    sc.upload(d_modes, modes, (size_t)K * h->n * 3);
    timer.start(sc);
    double* b = pair_sums(sc, h, d_modes, nullptr, K, 0);
    timer.stop(sc);
    sc.download(scores_out, b, (size_t)h->S * K);
    return finish(h, sc, timer, "pf_shapes_scores");
}

int pf_shapes_combine(pf_shapes* h, const double* coeff, int32_t K, double* out) {
    PF_CHECK(h && coeff && out, PF_E_ARG, "pf_shapes_combine: NULL argument");
    PF_CHECK(K >= 1 && K <= h->S, PF_E_ARG, "pf_shapes_combine: K = %d out of range (1..S = %d)", (int)K, (int)h->S);
    PF_CHECK(all_finite(coeff, (int64_t)K * h->S), PF_E_ARG, "pf_shapes_combine: a coefficient is not finite");
    PF_HIP(hipSetDevice(h->ctx->device));
    hipStream_t st = h->ctx->stream;
    const int64_t n3 = 3 * h->n;
    Scratch sc(st);
    StreamTimer timer(h->timed);
    double* d_coeff = sc.get<double>((size_t)K * h->S);
    double* d_out = sc.get<double>((size_t)K * n3);
    sc.upload(d_coeff, coeff, (size_t)K * h->S);
    timer.start(sc);
    if (sc.ok()) {
        k_sh_combine<<<dim3(pf_blocks(n3), (unsigned)((K + SH_KT - 1) / SH_KT)), PF_BLOCK, 0, st>>>(h->X, h->r, n3, h->S, d_coeff, K, d_out);
        sc.launched();
    }
    timer.stop(sc);
    sc.download(out, d_out, (size_t)K * n3);
    return finish(h, sc, timer, "pf_shapes_combine");
}

int pf_shapes_set_reference(pf_shapes* h, const double* ref) {
    PF_CHECK(h && ref, PF_E_ARG, "pf_shapes_set_reference: NULL argument");
    PF_CHECK(all_finite(ref, 3 * h->n), PF_E_ARG, "pf_shapes_set_reference: a coordinate is not finite");
    PF_HIP(hipSetDevice(h->ctx->device));
    PF_HIP(hipMemcpyAsync(h->r, ref, sizeof(double) * 3 * (size_t)h->n, hipMemcpyHostToDevice, h->ctx->stream));
    PF_HIP(hipStreamSynchronize(h->ctx->stream));
    return PF_OK;
}

int pf_shapes_download(pf_shapes* h, double* shapes_out) {
    PF_CHECK(h && shapes_out, PF_E_ARG, "pf_shapes_download: NULL argument");
    PF_HIP(hipSetDevice(h->ctx->device));
    PF_HIP(hipMemcpyAsync(shapes_out, h->X, sizeof(double) * 3 * (size_t)h->n * h->S, hipMemcpyDeviceToHost, h->ctx->stream));
    PF_HIP(hipStreamSynchronize(h->ctx->stream));
    return PF_OK;
}

int pf_shapes_weight_sum(pf_shapes* h, double* weight_sum) {
    PF_CHECK(h && weight_sum, PF_E_ARG, "pf_shapes_weight_sum: NULL argument");
    *weight_sum = h->W;
    return PF_OK;
}

int pf_shapes_device_ms(pf_shapes* h, int32_t enable, double* last_ms) {
    PF_CHECK(h != nullptr, PF_E_ARG, "pf_shapes_device_ms: NULL handle");
    if (last_ms) *last_ms = h->last_ms;
    h->timed = enable != 0;
    return PF_OK;
}

}  // extern "C"
