// Functional maps on the device: the gathered mass-weighted projection of a point map onto two Laplace-Beltrami bases,
// the conversion of a functional map back into a point map, ZoomOut (Melzi et al. 2019), and the exact nearest-neighbour
// search in up to 128 dimensions that the conversion needs.
//
// Direction (Focusr's): T[i] in [0, n_t) for every SOURCE vertex i.
//   project  C[a][b] = sum_i m_s[i] phi_s[i][a] phi_t[T[i]][b]                    k_s x k_t
//   convert  Q = phi_s[:, :k_s] C  (each entry summed over a ascending),  T[i] = the row of phi_t[:, :k_t] nearest to Q[i]
//
// Arithmetic of the search: pf_knn.hip's - the squared distance is the sum over the coordinates, left to right, of
// (q_c - r_c)^2 with separate multiply and add (the file is compiled without contraction); the smallest value wins, the
// lowest reference index on exact ties.  Indices and distances are the bits of a numpy brute force.
//
// k_knn_wide.  Every search of the library up to here bins the points on two axes; at d = 20 .. 128 two axes prune
// nothing, so this one is the tiled exhaustive scan.  A block of 256 lanes owns 512 queries, two per lane, and a range
// of the references (the grid's y: short query sets are split over the references to fill the device; k_wide_merge
// joins the ranges in ascending order).  Tiles of the references - all their coordinates, 32 KiB - stream through LDS
// by coalesced loads; every lane reads the same reference word (a broadcast), one read serving both of its queries.  A
// lane cannot hold a 128-double query in registers, so d is cut into chunks of 8: for 16 references at a time the lane
// keeps 2 x 16 partial sums in registers (64 VGPRs) and walks the chunks in coordinate order, loading its two queries'
// 8 coordinates of the chunk (32 VGPRs) from a coordinate-major copy of the queries, so that the loads of a wave are
// contiguous.  Each of the 32 sums advances left to right: the tiling does not change a bit.  Coordinates past d are
// zero on both sides and add +0.  After each chunk the wave drops the 16 references if none of its 2048 partial sums is
// still below its lane's best: the terms are non-negative and rounding is monotone, so a sum that has reached the best
// cannot come back under it, and an equal one would lose the tie to the lower index already held.
// Budget (MI355X_MICROARCH: 512 registers per lane and SIMD, 160 KiB LDS per CU): the sums and the chunk need 96 VGPRs;
// hipcc schedules the LDS reads far ahead of their use and takes 191 -> 2 waves per SIMD, 2 blocks and 64 KiB of LDS
// per CU.  (Held to 128 registers for 4 waves it spills 139 of them to scratch; held to 168 for 3, 21: left alone.)
// The 32 independent sums per lane are the latency hiding.  Per reference word read from LDS (2 LDS cycles per wave) a
// wave issues 6 FP64 instructions (24 SIMD cycles): four SIMDs keep the LDS under a third busy.  The queries' chunks
// come from L2, 16 loads of 512 B per wave and 768 FP64 instructions: ~11 B per clock and CU at the full FP64 rate.
//
// k_fmap_tile.  Projection and Q are the same small FP64 product out[x][y] = sum_z L(z, x) R(z, y) with other loaders:
// a block computes 64 x 64 outputs, 4 x 4 per lane, from LDS tiles of 32 z.  The projection cuts the rows into
// fixed blocks of 512, each block's partial sum in its own slot; k_fmap_combine adds the slots in block order.  No
// floating-point atomic: the order of every sum is fixed by the shapes alone, two calls give the same bits.
//
// ZoomOut on sub-samples (pf_fmap_set_samples, pf_fmap_zoomout_sampled).  The rows phi_s[S_s] and phi_t[S_t] are gathered
// once into compact blocks A and B; the rounds run project's and convert's kernels on those (FmapView), so a round costs
// q_s q_t k instead of n_s n_t k.  The fit on the samples is the least-squares one, (A_k^T A_k) C = A_k^T B[Tsub, :k]: both
// Gram products are projections with unit weights (A^T A through the identity map into A itself), the k x k system is
// solved on the host (chol_solve).  An entry of A^T A is the same sum in the same order whatever k, so the product is
// formed once at k_end and its leading k x k block serves every round.
#include <math.h>
#include <string.h>

#include <algorithm>
#include <vector>

#include "pf_internal.h"

namespace {

constexpr int WIDE_TQ = 2;       // queries per lane
constexpr int WIDE_RT = 16;      // references whose partial sums a lane holds at a time
constexpr int WIDE_DC = 8;       // coordinates per chunk
constexpr int WIDE_LDS = 4096;   // doubles of a reference tile (32 KiB)
constexpr int WIDE_QB = WIDE_TQ * PF_BLOCK;  // queries per block
constexpr int FMAP_MAX_K = 128;
constexpr int TILE = 64;         // outputs per side of a k_fmap_tile block
constexpr int TILE_Z = 32;       // contraction steps per LDS tile
constexpr int TILE_LD = TILE + 1;
constexpr int PROJ_ROWS = 512;   // rows per partial sum of the projection

inline int pad_d(int d) { return (d + WIDE_DC - 1) / WIDE_DC * WIDE_DC; }
__host__ __device__ inline int64_t imin(int64_t a, int64_t b) { return a < b ? a : b; }

// out[c][i] = in[i][c] for c < d, 0 for d <= c < d_pad; rows i < ld (those past n are zero)
__global__ __launch_bounds__(PF_BLOCK) void k_wide_transpose(const double* __restrict__ in, int64_t n, int32_t stride, int32_t d,
                                                             int32_t d_pad, int64_t ld, double* __restrict__ out) {
    const int64_t e = (int64_t)blockIdx.x * PF_BLOCK + threadIdx.x;
    if (e >= ld * d_pad) return;
    const int64_t c = e / ld, i = e - c * ld;
    out[e] = (c < d && i < n) ? in[i * stride + c] : 0.0;
}

template <bool COUNT>
__global__ __launch_bounds__(PF_BLOCK) void k_knn_wide(const double* __restrict__ ref, int64_t n_ref, int32_t ref_stride,
                                                       const double* __restrict__ qt /* [d_pad][ld] */, int64_t n_qry, int64_t ld,
                                                       int32_t d, int32_t d_pad, int32_t tile_refs, int64_t refs_per_split,
                                                       double* __restrict__ best_out /* [splits][n_qry] */,
                                                       int32_t* __restrict__ idx_out, unsigned long long* __restrict__ counter) {
    __shared__ double tile[WIDE_LDS];
    const int tid = threadIdx.x;
    const int64_t q_base = (int64_t)blockIdx.x * WIDE_QB;
    // a lane past the end works on the last query and stores nothing: rows of qt past n_qry are never read
    int64_t qi[WIDE_TQ];
#pragma unroll
    for (int t = 0; t < WIDE_TQ; ++t) qi[t] = imin(q_base + t * PF_BLOCK + tid, n_qry - 1);
    double best[WIDE_TQ];
    int32_t bidx[WIDE_TQ];
#pragma unroll
    for (int t = 0; t < WIDE_TQ; ++t) best[t] = __longlong_as_double(0x7ff0000000000000ll), bidx[t] = 0;
    const int64_t r_begin = (int64_t)blockIdx.y * refs_per_split;
    const int64_t r_end = imin(r_begin + refs_per_split, n_ref);
    const int n_chunks = d_pad / WIDE_DC;
    unsigned long long evaluated = 0;  // chunks of 16 references this wave went through
    for (int64_t j0 = r_begin; j0 < r_end; j0 += tile_refs) {
        const int nt = (int)imin(tile_refs, r_end - j0);
        const int nt_pad = (nt + WIDE_RT - 1) / WIDE_RT * WIDE_RT;  // <= tile_refs, a multiple of WIDE_RT
        __syncthreads();
        for (int e = tid; e < nt_pad * d_pad; e += PF_BLOCK) {
            const int r = e / d_pad, c = e - r * d_pad;
            tile[e] = (r < nt && c < d) ? ref[(j0 + r) * ref_stride + c] : 0.0;
        }
        __syncthreads();
        for (int rg = 0; rg < nt_pad; rg += WIDE_RT) {
            double acc[WIDE_TQ][WIDE_RT];
#pragma unroll
            for (int t = 0; t < WIDE_TQ; ++t)
#pragma unroll
                for (int r = 0; r < WIDE_RT; ++r) acc[t][r] = 0.0;
            bool dropped = false;
            for (int ch = 0; ch < n_chunks; ++ch) {
                double q[WIDE_TQ][WIDE_DC];
#pragma unroll
                for (int t = 0; t < WIDE_TQ; ++t)
#pragma unroll
                    for (int c = 0; c < WIDE_DC; ++c) q[t][c] = qt[(int64_t)(ch * WIDE_DC + c) * ld + qi[t]];
                const double* rp = tile + rg * d_pad + ch * WIDE_DC;
#pragma unroll
                for (int r = 0; r < WIDE_RT; ++r) {
#pragma unroll
                    for (int c = 0; c < WIDE_DC; ++c) {
                        const double rv = rp[r * d_pad + c];
#pragma unroll
                        for (int t = 0; t < WIDE_TQ; ++t) {
                            const double diff = q[t][c] - rv;
                            acc[t][r] += diff * diff;
                        }
                    }
                }
                if (COUNT) ++evaluated;
                if (ch + 1 < n_chunks) {
                    bool alive = false;
#pragma unroll
                    for (int t = 0; t < WIDE_TQ; ++t)
#pragma unroll
                        for (int r = 0; r < WIDE_RT; ++r) alive |= acc[t][r] < best[t];
                    if (!__any(alive)) {
                        dropped = true;
                        break;
                    }
                }
            }
            if (!dropped) {
#pragma unroll
                for (int r = 0; r < WIDE_RT; ++r) {
                    if (rg + r < nt) {
#pragma unroll
                        for (int t = 0; t < WIDE_TQ; ++t)
                            if (acc[t][r] < best[t]) best[t] = acc[t][r], bidx[t] = (int32_t)(j0 + rg + r);
                    }
                }
            }
        }
    }
#pragma unroll
    for (int t = 0; t < WIDE_TQ; ++t) {
        const int64_t i = q_base + t * PF_BLOCK + tid;
        if (i < n_qry) {
            best_out[(int64_t)blockIdx.y * n_qry + i] = best[t];
            idx_out[(int64_t)blockIdx.y * n_qry + i] = bidx[t];
        }
    }
    if (COUNT && (tid & (PF_WAVE - 1)) == 0) atomicAdd(counter, evaluated);
}

// the ranges of the references in ascending order, strict <: the lowest index wins a tie (range 0 starts from index 0
// at +inf, which is what a brute force's argmin gives when every distance is +inf)
__global__ __launch_bounds__(PF_BLOCK) void k_wide_merge(const double* __restrict__ best, const int32_t* __restrict__ idx, int64_t n_qry,
                                                         int32_t splits, double* __restrict__ d2_out, int32_t* __restrict__ idx_out) {
    const int64_t i = (int64_t)blockIdx.x * PF_BLOCK + threadIdx.x;
    if (i >= n_qry) return;
    double b = best[i];
    int32_t j = idx[i];
    for (int32_t s = 1; s < splits; ++s) {
        const double v = best[(int64_t)s * n_qry + i];
        if (v < b) b = v, j = idx[(int64_t)s * n_qry + i];
    }
    d2_out[i] = b;
    idx_out[i] = j;
}

// The search on device blocks: ref rows with a stride, queries coordinate-major (d_pad x ld, zero past d and past n_qry).
// d2_out / idx_out [n_qry] on the device.  Everything is queued on the ctx stream; nothing waits.
int wide_search(pf_ctx* c, Scratch& s, const double* ref, int64_t n_ref, int32_t ref_stride, const double* qt, int64_t n_qry, int64_t ld,
                int32_t d, double* d2_out, int32_t* idx_out) {
    const int32_t d_pad = pad_d(d);
    const int32_t tile_refs = WIDE_LDS / d_pad / WIDE_RT * WIDE_RT;  // >= 32 at d_pad = 128
    const int64_t q_blocks = (n_qry + WIDE_QB - 1) / WIDE_QB;
    // about four blocks per CU (1024) when the queries alone give fewer, as long as a range keeps whole tiles
    int64_t splits = std::max<int64_t>(1, std::min<int64_t>((1024 + q_blocks - 1) / q_blocks, (n_ref + tile_refs - 1) / tile_refs));
    splits = std::min<int64_t>(splits, 4096);
    int64_t per = (n_ref + splits - 1) / splits;
    per = (per + tile_refs - 1) / tile_refs * tile_refs;
    splits = (n_ref + per - 1) / per;
    double* pb = splits > 1 ? s.get<double>((size_t)splits * n_qry) : d2_out;
    int32_t* pi = splits > 1 ? s.get<int32_t>((size_t)splits * n_qry) : idx_out;
    if (c->wide_count_on && !c->wide_count) c->wide_count = s.keep<unsigned long long>(1);
    if (c->wide_count_on) s.zero(c->wide_count, sizeof(unsigned long long));
    if (!s.ok()) return PF_OK;  // the caller reads s.err
    const dim3 grid((unsigned)q_blocks, (unsigned)splits);
    if (c->wide_count_on)
        k_knn_wide<true><<<grid, PF_BLOCK, 0, s.st>>>(ref, n_ref, ref_stride, qt, n_qry, ld, d, d_pad, tile_refs, per, pb, pi, c->wide_count);
    else
        k_knn_wide<false><<<grid, PF_BLOCK, 0, s.st>>>(ref, n_ref, ref_stride, qt, n_qry, ld, d, d_pad, tile_refs, per, pb, pi, nullptr);
    if (splits > 1) k_wide_merge<<<pf_blocks(n_qry), PF_BLOCK, 0, s.st>>>(pb, pi, n_qry, (int32_t)splits, d2_out, idx_out);
    s.launched();
    return PF_OK;
}

// ---- out[x][y] = sum_z L(z, x) R(z, y), z ascending, one accumulator per output ------------------------------------

struct ProjLoad {  // z: source row, x: a, y: b
    const double* phi_s;
    const double* phi_t;
    const double* mass;
    const int32_t* T;
    int32_t K;
    __device__ double left(int64_t z, int64_t x) const { return mass[z] * phi_s[z * K + x]; }
    __device__ double right(int64_t z, int64_t y) const { return phi_t[(int64_t)T[z] * K + y]; }
};
struct QLoad {  // z: a, x: source row, y: b
    const double* phi_s;
    const double* C;
    int32_t K, k_t;
    __device__ double left(int64_t z, int64_t x) const { return phi_s[x * K + z]; }
    __device__ double right(int64_t z, int64_t y) const { return C[z * k_t + y]; }
};

// grid: (x tiles, y tiles, z blocks); the block z0 .. z0 + z_per writes out + blockIdx.z * out_block at [x * ldx + y * ldy]
template <class Load, bool Z_FAST /* consecutive lanes load consecutive z of L (its rows are z-contiguous) */>
__global__ __launch_bounds__(PF_BLOCK) void k_fmap_tile(Load ld, int64_t nx, int64_t ny, int64_t nz, int64_t z_per, double* __restrict__ out,
                                                        int64_t out_block, int64_t ldx, int64_t ldy) {
    __shared__ double ls[TILE_Z * TILE_LD], rs[TILE_Z * TILE_LD];
    const int tid = threadIdx.x, tx = tid & 15, ty = tid >> 4;
    const int64_t x0 = (int64_t)blockIdx.x * TILE, y0 = (int64_t)blockIdx.y * TILE;
    const int64_t z_begin = (int64_t)blockIdx.z * z_per, z_end = imin(z_begin + z_per, nz);
    double acc[4][4];
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int j = 0; j < 4; ++j) acc[i][j] = 0.0;
    for (int64_t z0 = z_begin; z0 < z_end; z0 += TILE_Z) {
        __syncthreads();
        for (int e = tid; e < TILE_Z * TILE; e += PF_BLOCK) {
            const int zl = Z_FAST ? (e & (TILE_Z - 1)) : e / TILE, xl = Z_FAST ? e / TILE_Z : (e & (TILE - 1));
            const int64_t z = z0 + zl, x = x0 + xl;
            ls[zl * TILE_LD + xl] = (z < z_end && x < nx) ? ld.left(z, x) : 0.0;
        }
        for (int e = tid; e < TILE_Z * TILE; e += PF_BLOCK) {
            const int zl = e / TILE, yl = e & (TILE - 1);
            const int64_t z = z0 + zl, y = y0 + yl;
            rs[zl * TILE_LD + yl] = (z < z_end && y < ny) ? ld.right(z, y) : 0.0;
        }
        __syncthreads();
        const int nzl = (int)imin(TILE_Z, z_end - z0);  // rows past the end would add +0: skipped all the same
        for (int zl = 0; zl < nzl; ++zl) {
            double a[4], b[4];
#pragma unroll
            for (int i = 0; i < 4; ++i) a[i] = ls[zl * TILE_LD + ty + 16 * i], b[i] = rs[zl * TILE_LD + tx + 16 * i];
#pragma unroll
            for (int i = 0; i < 4; ++i)
#pragma unroll
                for (int j = 0; j < 4; ++j) acc[i][j] += a[i] * b[j];
        }
    }
    double* o = out + (int64_t)blockIdx.z * out_block;
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const int64_t x = x0 + ty + 16 * i, y = y0 + tx + 16 * j;
            if (x < nx && y < ny) o[x * ldx + y * ldy] = acc[i][j];
        }
}

__global__ __launch_bounds__(PF_BLOCK) void k_fmap_combine(const double* __restrict__ part, int64_t count, int64_t blocks, double* __restrict__ out) {
    const int64_t e = (int64_t)blockIdx.x * PF_BLOCK + threadIdx.x;
    if (e >= count) return;
    double s = part[e];
    for (int64_t b = 1; b < blocks; ++b) s += part[b * count + e];
    out[e] = s;
}

__global__ __launch_bounds__(PF_BLOCK) void k_fmap_set_map(const int64_t* __restrict__ in, int64_t n, int64_t n_t, int32_t* __restrict__ T,
                                                           int32_t* __restrict__ bad) {
    const int64_t i = (int64_t)blockIdx.x * PF_BLOCK + threadIdx.x;
    if (i >= n) return;
    const int64_t v = in[i];
    const bool ok = v >= 0 && v < n_t;
    T[i] = ok ? (int32_t)v : 0;
    if (!ok) atomicOr(bad, 1);
}

__global__ __launch_bounds__(PF_BLOCK) void k_fmap_take_knn(const int64_t* __restrict__ idx, const double* __restrict__ d2, int64_t n,
                                                            int32_t* __restrict__ T, double* __restrict__ d2_out) {
    const int64_t i = (int64_t)blockIdx.x * PF_BLOCK + threadIdx.x;
    if (i >= n) return;
    T[i] = (int32_t)idx[i];
    d2_out[i] = d2[i];
}

// dst[i][c] = src[rows[i]][c], K columns
__global__ __launch_bounds__(PF_BLOCK) void k_fmap_gather_rows(const double* __restrict__ src, int32_t K, const int32_t* __restrict__ rows,
                                                               int64_t q, double* __restrict__ dst) {
    const int64_t e = (int64_t)blockIdx.x * PF_BLOCK + threadIdx.x;
    if (e >= q * K) return;
    const int64_t i = e / K, c = e - i * K;
    dst[e] = src[(int64_t)rows[i] * K + c];
}

// unit weights and the identity map of the samples
__global__ __launch_bounds__(PF_BLOCK) void k_fmap_unit(double* __restrict__ ones, int32_t* __restrict__ ident, int64_t q) {
    const int64_t i = (int64_t)blockIdx.x * PF_BLOCK + threadIdx.x;
    if (i < q) ones[i] = 1.0, ident[i] = (int32_t)i;
}

__global__ __launch_bounds__(PF_BLOCK) void k_fmap_widen(const int32_t* __restrict__ T, int64_t n, int64_t* __restrict__ out) {
    const int64_t i = (int64_t)blockIdx.x * PF_BLOCK + threadIdx.x;
    if (i < n) out[i] = T[i];
}

// R <- the solution X of G[:k, :k] X = R (k x k, row-major) for a symmetric positive definite G with leading dimension
// ldg, of which the lower triangle is read: Cholesky G = L L^T, then a forward and a back substitution over the rows of R.
// False when a pivot is not positive - not above tol times its diagonal entry of G, the rounding of the sums behind it
// (a pivot that is zero in exact arithmetic comes out as noise of either sign).
bool chol_solve(const double* G, int ldg, int k, double tol, double* R) {
    std::vector<double> L((size_t)k * k, 0.0);
    for (int j = 0; j < k; ++j) {
        double s = G[(size_t)j * ldg + j];
        for (int p = 0; p < j; ++p) s -= L[(size_t)j * k + p] * L[(size_t)j * k + p];
        if (!(s > tol * G[(size_t)j * ldg + j])) return false;
        const double ljj = sqrt(s);
        L[(size_t)j * k + j] = ljj;
        for (int i = j + 1; i < k; ++i) {
            double t = G[(size_t)i * ldg + j];
            for (int p = 0; p < j; ++p) t -= L[(size_t)i * k + p] * L[(size_t)j * k + p];
            L[(size_t)i * k + j] = t / ljj;
        }
    }
    for (int i = 0; i < k; ++i) {  // L Y = R
        double* ri = R + (size_t)i * k;
        for (int p = 0; p < i; ++p) {
            const double l = L[(size_t)i * k + p];
            const double* rp = R + (size_t)p * k;
            for (int c = 0; c < k; ++c) ri[c] -= l * rp[c];
        }
        for (int c = 0; c < k; ++c) ri[c] /= L[(size_t)i * k + i];
    }
    for (int i = k - 1; i >= 0; --i) {  // L^T X = Y
        double* ri = R + (size_t)i * k;
        for (int p = i + 1; p < k; ++p) {
            const double l = L[(size_t)p * k + i];
            const double* rp = R + (size_t)p * k;
            for (int c = 0; c < k; ++c) ri[c] -= l * rp[c];
        }
        for (int c = 0; c < k; ++c) ri[c] /= L[(size_t)i * k + i];
    }
    return true;
}

}  // namespace

struct pf_fmap {
    pf_ctx* ctx = nullptr;
    int64_t n_t = 0, n_s = 0, ld_q = 0;
    int32_t K = 0;
    double* phi_t = nullptr;  // [n_t][K]
    double* phi_s = nullptr;  // [n_s][K]
    double* mass = nullptr;   // [n_s]
    int32_t* T = nullptr;     // [n_s] the point map
    double* d2 = nullptr;     // [n_s] squared distances of the last conversion
    double* C = nullptr;      // [c_ks][c_kt] the resident functional map
    double* Q = nullptr;      // [n_s][k_t] (narrow search) or [pad(k_t)][ld_q] (wide search)
    int32_t c_ks = 0, c_kt = 0;
    bool has_T = false, has_d2 = false;
    // the samples of pf_fmap_set_samples
    int64_t q_t = 0, q_s = 0, ld_qs = 0;
    double* A = nullptr;        // [q_s][K] phi_s[S_s]
    double* B = nullptr;        // [q_t][K] phi_t[S_t]
    double* ones = nullptr;     // [q_s] unit weights
    int32_t* ident = nullptr;   // [q_s] the identity map (A^T A)
    int32_t* T_sub = nullptr;   // [q_s] the samples' map into B
    double* d2_sub = nullptr;   // [q_s]
    double* Q_sub = nullptr;    // Q of the samples, laid out like Q
    double* G = nullptr;        // [K][K] A^T A
    double* R = nullptr;        // [K][K] A^T B[T_sub]
    bool has_samples = false;
};

// what project and convert work on: the full bases, or the samples' compact blocks
struct FmapView {
    const double* phi_t;
    int64_t n_t;
    const double* phi_s;
    int64_t n_s;
    const double* mass;
    int32_t* T;
    double* d2;
    double* Q;
    int64_t ld_q;
};
static FmapView fmap_full(pf_fmap* h) { return {h->phi_t, h->n_t, h->phi_s, h->n_s, h->mass, h->T, h->d2, h->Q, h->ld_q}; }
static FmapView fmap_sub(pf_fmap* h) { return {h->B, h->q_t, h->A, h->q_s, h->ones, h->T_sub, h->d2_sub, h->Q_sub, h->ld_qs}; }

// out (k_s x k_t on the device); out == h->C makes it the resident functional map
static int fmap_project(pf_fmap* h, const FmapView& v, int32_t k_s, int32_t k_t, double* out) {
    pf_ctx* c = h->ctx;
    Scratch s(c->stream);
    const int64_t blocks = (v.n_s + PROJ_ROWS - 1) / PROJ_ROWS, count = (int64_t)k_s * k_t;
    double* part = blocks > 1 ? s.get<double>((size_t)(blocks * count)) : out;
    if (s.ok()) {
        const ProjLoad ld{v.phi_s, v.phi_t, v.mass, v.T, h->K};
        const dim3 grid((unsigned)((k_s + TILE - 1) / TILE), (unsigned)((k_t + TILE - 1) / TILE), (unsigned)blocks);
        k_fmap_tile<ProjLoad, false><<<grid, PF_BLOCK, 0, s.st>>>(ld, k_s, k_t, v.n_s, PROJ_ROWS, part, count, k_t, 1);
        if (blocks > 1) k_fmap_combine<<<pf_blocks(count), PF_BLOCK, 0, s.st>>>(part, count, blocks, out);
        s.launched();
    }
    PF_CHECK(s.ok(), PF_E_HIP, "pf_fmap_project: %s", hipGetErrorString(s.err));
    if (out == h->C) h->c_ks = k_s, h->c_kt = k_t;
    return PF_OK;
}

// the resident functional map (k_s x k_t) -> v.T, v.d2
static int fmap_convert(pf_fmap* h, const FmapView& v, int32_t k_s, int32_t k_t) {
    pf_ctx* c = h->ctx;
    const bool wide = k_t > 16;
    {
        Scratch s(c->stream);
        const QLoad ld{v.phi_s, h->C, h->K, k_t};
        const dim3 grid((unsigned)((v.n_s + TILE - 1) / TILE), (unsigned)((k_t + TILE - 1) / TILE), 1);
        const int32_t d_pad = pad_d(k_t);
        // the wide search reads zeros in the coordinates past k_t
        if (wide && d_pad > k_t) s.zero(v.Q + (int64_t)k_t * v.ld_q, sizeof(double) * (size_t)((d_pad - k_t) * v.ld_q));
        if (s.ok()) {
            if (wide)
                k_fmap_tile<QLoad, true><<<grid, PF_BLOCK, 0, s.st>>>(ld, v.n_s, k_t, k_s, k_s, v.Q, 0, 1, v.ld_q);
            else
                k_fmap_tile<QLoad, true><<<grid, PF_BLOCK, 0, s.st>>>(ld, v.n_s, k_t, k_s, k_s, v.Q, 0, k_t, 1);
            s.launched();
        }
        if (wide) PF_TRY(wide_search(c, s, v.phi_t, v.n_t, h->K, v.Q, v.n_s, v.ld_q, k_t, v.d2, v.T));
        PF_CHECK(s.ok(), PF_E_HIP, "pf_fmap_convert: %s", hipGetErrorString(s.err));
    }
    if (!wide) {
        PF_TRY(pf_knn1_device(c, v.phi_t, v.n_t, h->K, v.Q, v.n_s, k_t, k_t));
        k_fmap_take_knn<<<pf_blocks(v.n_s), PF_BLOCK, 0, c->stream>>>(c->knn_idx.p, c->knn_d2.p, v.n_s, v.T, v.d2);
        PF_HIP(hipGetLastError());
    }
    if (v.T == h->T) h->has_T = h->has_d2 = true;
    return PF_OK;
}

static void fmap_free_samples(pf_fmap* h) {
    hipStream_t st = h->ctx->stream;
    for (void* p : {(void*)h->A, (void*)h->B, (void*)h->ones, (void*)h->ident, (void*)h->T_sub, (void*)h->d2_sub, (void*)h->Q_sub, (void*)h->G,
                    (void*)h->R})
        if (p) pf_free(st, p);
    h->A = h->B = h->ones = h->d2_sub = h->Q_sub = h->G = h->R = nullptr;
    h->ident = h->T_sub = nullptr;
    h->has_samples = false;
}

extern "C" {

int pf_knn1_wide(pf_ctx* c, const double* ref, int64_t n_ref, const double* qry, int64_t n_qry, int32_t d, int64_t* idx_out,
                 double* d2_out) {
    PF_CHECK(c && ref && qry && idx_out, PF_E_ARG, "pf_knn1_wide: NULL argument");
    PF_CHECK(n_ref > 0 && n_ref < ((int64_t)1 << 31) && n_qry > 0 && n_qry < ((int64_t)1 << 31) && d >= 1 && d <= FMAP_MAX_K, PF_E_ARG,
             "pf_knn1_wide: n_ref %lld, n_qry %lld, d %d out of range (1 <= d <= 128)", (long long)n_ref, (long long)n_qry, d);
    PF_HIP(hipSetDevice(c->device));
    Scratch s(c->stream);
    const int32_t d_pad = pad_d(d);
    const int64_t ld = (n_qry + PF_WAVE - 1) & ~(int64_t)(PF_WAVE - 1);
    double* d_ref = s.get<double>((size_t)(n_ref * d));
    double* d_qry = s.get<double>((size_t)(n_qry * d));
    double* d_qt = s.get<double>((size_t)(ld * d_pad));
    double* d_d2 = s.get<double>((size_t)n_qry);
    int32_t* d_idx = s.get<int32_t>((size_t)n_qry);
    int64_t* d_idx64 = s.get<int64_t>((size_t)n_qry);
    s.upload(d_ref, ref, (size_t)(n_ref * d));
    s.upload(d_qry, qry, (size_t)(n_qry * d));
    if (s.ok()) {
        k_wide_transpose<<<pf_blocks(ld * d_pad), PF_BLOCK, 0, s.st>>>(d_qry, n_qry, d, d, d_pad, ld, d_qt);
        s.launched();
    }
    PF_TRY(wide_search(c, s, d_ref, n_ref, d, d_qt, n_qry, ld, d, d_d2, d_idx));
    if (s.ok()) {
        k_fmap_widen<<<pf_blocks(n_qry), PF_BLOCK, 0, s.st>>>(d_idx, n_qry, d_idx64);
        s.launched();
    }
    s.download(idx_out, d_idx64, (size_t)n_qry);
    s.download(d2_out, d_d2, (size_t)n_qry);
    s.sync();
    PF_CHECK(s.ok(), PF_E_HIP, "pf_knn1_wide: %s", hipGetErrorString(s.err));
    return PF_OK;
}

int pf_knn1_wide_count(pf_ctx* c, int32_t enable_counting, int64_t* chunk_pairs) {
    PF_CHECK(c != nullptr, PF_E_ARG, "pf_knn1_wide_count: ctx is NULL");
    unsigned long long waves = 0ull;
    if (c->wide_count) {
        PF_HIP(hipMemcpyAsync(&waves, c->wide_count, sizeof(waves), hipMemcpyDeviceToHost, c->stream));
        PF_HIP(hipStreamSynchronize(c->stream));
    }
    // a wave adds one per (16 references x 8 coordinates) it went through, for its 128 queries
    if (chunk_pairs) *chunk_pairs = (int64_t)waves * WIDE_RT * WIDE_DC * WIDE_TQ * PF_WAVE;
    c->wide_count_on = enable_counting != 0;
    return PF_OK;
}

int pf_fmap_create(pf_ctx* c, const double* phi_t, int64_t n_t, const double* phi_s, int64_t n_s, const double* mass_s, int32_t K,
                   pf_fmap** out) {
    PF_CHECK(c && phi_t && phi_s && mass_s && out, PF_E_ARG, "pf_fmap_create: NULL argument");
    PF_CHECK(n_t > 0 && n_t < ((int64_t)1 << 31) && n_s > 0 && n_s < ((int64_t)1 << 31) && K >= 1 && K <= FMAP_MAX_K, PF_E_ARG,
             "pf_fmap_create: n_t %lld, n_s %lld, K %d out of range (1 <= K <= 128)", (long long)n_t, (long long)n_s, K);
    PF_HIP(hipSetDevice(c->device));
    *out = nullptr;
    pf_fmap* h = new pf_fmap();
    h->ctx = c, h->n_t = n_t, h->n_s = n_s, h->K = K;
    h->ld_q = (n_s + PF_WAVE - 1) & ~(int64_t)(PF_WAVE - 1);
    Scratch s(c->stream);
    const size_t q_count = (size_t)(h->ld_q * pad_d(K));  // >= n_s * K, the narrow layout
    h->phi_t = s.keep<double>((size_t)(n_t * K));
    h->phi_s = s.keep<double>((size_t)(n_s * K));
    h->mass = s.keep<double>((size_t)n_s);
    h->T = s.keep<int32_t>((size_t)n_s);
    h->d2 = s.keep<double>((size_t)n_s);
    h->C = s.keep<double>((size_t)K * K);
    h->Q = s.keep<double>(q_count);
    s.upload(h->phi_t, phi_t, (size_t)(n_t * K));
    s.upload(h->phi_s, phi_s, (size_t)(n_s * K));
    s.upload(h->mass, mass_s, (size_t)n_s);
    s.zero(h->Q, sizeof(double) * q_count);
    s.sync();
    if (!s.ok()) {
        pf_set_error("pf_fmap_create: %s", hipGetErrorString(s.err));
        pf_fmap_free(h);
        return PF_E_HIP;
    }
    *out = h;
    return PF_OK;
}

void pf_fmap_free(pf_fmap* h) {
    if (!h) return;
    hipStream_t st = h->ctx->stream;
    for (void* p : {(void*)h->phi_t, (void*)h->phi_s, (void*)h->mass, (void*)h->T, (void*)h->d2, (void*)h->C, (void*)h->Q})
        if (p) pf_free(st, p);
    fmap_free_samples(h);
    delete h;
}

int pf_fmap_set_p2p(pf_fmap* h, const int64_t* T) {
    PF_CHECK(h && T, PF_E_ARG, "pf_fmap_set_p2p: NULL argument");
    pf_ctx* c = h->ctx;
    PF_HIP(hipSetDevice(c->device));
    h->has_T = h->has_d2 = false;
    int32_t bad = 0;
    {
        Scratch s(c->stream);
        int64_t* d_in = s.get<int64_t>((size_t)h->n_s);
        int32_t* d_bad = s.get<int32_t>(1);
        s.upload(d_in, T, (size_t)h->n_s);
        s.zero(d_bad, sizeof(int32_t));
        if (s.ok()) {
            k_fmap_set_map<<<pf_blocks(h->n_s), PF_BLOCK, 0, s.st>>>(d_in, h->n_s, h->n_t, h->T, d_bad);
            s.launched();
        }
        s.download(&bad, d_bad, 1);
        s.sync();
        PF_CHECK(s.ok(), PF_E_HIP, "pf_fmap_set_p2p: %s", hipGetErrorString(s.err));
    }
    PF_CHECK(bad == 0, PF_E_ARG, "pf_fmap_set_p2p: an index lies outside 0 .. n_t - 1 = %lld", (long long)(h->n_t - 1));
    h->has_T = true;
    return PF_OK;
}

int pf_fmap_get_p2p(pf_fmap* h, int64_t* T_out, double* d2_out) {
    PF_CHECK(h && T_out, PF_E_ARG, "pf_fmap_get_p2p: NULL argument");
    PF_CHECK(h->has_T, PF_E_STATE, "pf_fmap_get_p2p: no point map yet (pf_fmap_set_p2p or pf_fmap_convert)");
    PF_CHECK(!d2_out || h->has_d2, PF_E_STATE, "pf_fmap_get_p2p: distances exist only after pf_fmap_convert");
    pf_ctx* c = h->ctx;
    PF_HIP(hipSetDevice(c->device));
    Scratch s(c->stream);
    int64_t* d_out = s.get<int64_t>((size_t)h->n_s);
    if (s.ok()) {
        k_fmap_widen<<<pf_blocks(h->n_s), PF_BLOCK, 0, s.st>>>(h->T, h->n_s, d_out);
        s.launched();
    }
    s.download(T_out, d_out, (size_t)h->n_s);
    s.download(d2_out, h->d2, (size_t)h->n_s);
    s.sync();
    PF_CHECK(s.ok(), PF_E_HIP, "pf_fmap_get_p2p: %s", hipGetErrorString(s.err));
    return PF_OK;
}

static int fmap_download_c(pf_fmap* h, double* C_out) {
    if (!C_out) return PF_OK;
    PF_HIP(hipMemcpyAsync(C_out, h->C, sizeof(double) * (size_t)h->c_ks * h->c_kt, hipMemcpyDeviceToHost, h->ctx->stream));
    PF_HIP(hipStreamSynchronize(h->ctx->stream));
    return PF_OK;
}

int pf_fmap_project(pf_fmap* h, int32_t k_s, int32_t k_t, double* C_out) {
    PF_CHECK(h != nullptr, PF_E_ARG, "pf_fmap_project: NULL handle");
    PF_CHECK(k_s >= 1 && k_s <= h->K && k_t >= 1 && k_t <= h->K, PF_E_ARG, "pf_fmap_project: k_s %d, k_t %d outside 1 .. K = %d", k_s, k_t,
             h->K);
    PF_CHECK(h->has_T, PF_E_STATE, "pf_fmap_project: no point map yet (pf_fmap_set_p2p or pf_fmap_convert)");
    PF_HIP(hipSetDevice(h->ctx->device));
    PF_TRY(fmap_project(h, fmap_full(h), k_s, k_t, h->C));
    return fmap_download_c(h, C_out);
}

int pf_fmap_convert(pf_fmap* h, const double* C, int32_t k_s, int32_t k_t) {
    PF_CHECK(h != nullptr, PF_E_ARG, "pf_fmap_convert: NULL handle");
    PF_CHECK(k_s >= 1 && k_s <= h->K && k_t >= 1 && k_t <= h->K, PF_E_ARG, "pf_fmap_convert: k_s %d, k_t %d outside 1 .. K = %d", k_s, k_t,
             h->K);
    PF_HIP(hipSetDevice(h->ctx->device));
    if (C) {
        PF_HIP(hipMemcpyAsync(h->C, C, sizeof(double) * (size_t)k_s * k_t, hipMemcpyHostToDevice, h->ctx->stream));
        PF_HIP(hipStreamSynchronize(h->ctx->stream));  // the caller's array is free again
        h->c_ks = k_s, h->c_kt = k_t;
    }
    PF_CHECK(h->c_ks == k_s && h->c_kt == k_t, PF_E_STATE, "pf_fmap_convert: the resident functional map is %d x %d, not %d x %d", h->c_ks,
             h->c_kt, k_s, k_t);
    return fmap_convert(h, fmap_full(h), k_s, k_t);
}

int pf_fmap_zoomout(pf_fmap* h, int32_t k_start, int32_t k_end, int32_t step, int32_t n_iter_at_end, double* C_out) {
    PF_CHECK(h != nullptr, PF_E_ARG, "pf_fmap_zoomout: NULL handle");
    PF_CHECK(k_start >= 1 && k_start <= k_end && k_end <= h->K && step >= 1 && n_iter_at_end >= 0, PF_E_ARG,
             "pf_fmap_zoomout: k_start %d, k_end %d (K = %d), step %d, n_iter_at_end %d out of range", k_start, k_end, h->K, step,
             n_iter_at_end);
    PF_CHECK(h->has_T, PF_E_STATE, "pf_fmap_zoomout: no point map yet (pf_fmap_set_p2p)");
    PF_HIP(hipSetDevice(h->ctx->device));
    for (int32_t k = k_start;;) {
        PF_TRY(fmap_project(h, fmap_full(h), k, k, h->C));
        PF_TRY(fmap_convert(h, fmap_full(h), k, k));
        if (k == k_end) break;
        k = std::min(k + step, k_end);
    }
    for (int32_t it = 0; it < n_iter_at_end; ++it) {
        PF_TRY(fmap_project(h, fmap_full(h), k_end, k_end, h->C));
        PF_TRY(fmap_convert(h, fmap_full(h), k_end, k_end));
    }
    return fmap_download_c(h, C_out);
}

int pf_fmap_set_samples(pf_fmap* h, const int64_t* S_t, int64_t q_t, const int64_t* S_s, int64_t q_s) {
    PF_CHECK(h && S_t && S_s, PF_E_ARG, "pf_fmap_set_samples: NULL argument");
    PF_CHECK(q_t >= 1 && q_t < ((int64_t)1 << 31) && q_s >= 1 && q_s < ((int64_t)1 << 31), PF_E_ARG,
             "pf_fmap_set_samples: q_t %lld, q_s %lld out of range (at least 1 each)", (long long)q_t, (long long)q_s);
    pf_ctx* c = h->ctx;
    PF_HIP(hipSetDevice(c->device));
    fmap_free_samples(h);
    int32_t bad = 0;
    {
        Scratch s(c->stream);
        const int32_t K = h->K;
        h->q_t = q_t, h->q_s = q_s;
        h->ld_qs = (q_s + PF_WAVE - 1) & ~(int64_t)(PF_WAVE - 1);
        const size_t q_count = (size_t)(h->ld_qs * pad_d(K));
        h->A = s.keep<double>((size_t)(q_s * K));
        h->B = s.keep<double>((size_t)(q_t * K));
        h->ones = s.keep<double>((size_t)q_s);
        h->ident = s.keep<int32_t>((size_t)q_s);
        h->T_sub = s.keep<int32_t>((size_t)q_s);
        h->d2_sub = s.keep<double>((size_t)q_s);
        h->Q_sub = s.keep<double>(q_count);
        h->G = s.keep<double>((size_t)K * K);
        h->R = s.keep<double>((size_t)K * K);
        int64_t* d_in_t = s.get<int64_t>((size_t)q_t);
        int64_t* d_in_s = s.get<int64_t>((size_t)q_s);
        int32_t* d_rows_t = s.get<int32_t>((size_t)q_t);
        int32_t* d_rows_s = s.get<int32_t>((size_t)q_s);
        int32_t* d_bad = s.get<int32_t>(1);
        s.upload(d_in_t, S_t, (size_t)q_t);
        s.upload(d_in_s, S_s, (size_t)q_s);
        s.zero(d_bad, sizeof(int32_t));
        s.zero(h->Q_sub, sizeof(double) * q_count);
        if (s.ok()) {
            // an index out of range is flagged and read as row 0: the gathers stay inside the bases either way
            k_fmap_set_map<<<pf_blocks(q_t), PF_BLOCK, 0, s.st>>>(d_in_t, q_t, h->n_t, d_rows_t, d_bad);
            k_fmap_set_map<<<pf_blocks(q_s), PF_BLOCK, 0, s.st>>>(d_in_s, q_s, h->n_s, d_rows_s, d_bad);
            k_fmap_gather_rows<<<pf_blocks(q_t * K), PF_BLOCK, 0, s.st>>>(h->phi_t, K, d_rows_t, q_t, h->B);
            k_fmap_gather_rows<<<pf_blocks(q_s * K), PF_BLOCK, 0, s.st>>>(h->phi_s, K, d_rows_s, q_s, h->A);
            k_fmap_unit<<<pf_blocks(q_s), PF_BLOCK, 0, s.st>>>(h->ones, h->ident, q_s);
            s.launched();
        }
        s.download(&bad, d_bad, 1);
        s.sync();
        if (!s.ok()) {
            pf_set_error("pf_fmap_set_samples: %s", hipGetErrorString(s.err));
            fmap_free_samples(h);
            return PF_E_HIP;
        }
    }
    if (bad != 0) {
        pf_set_error("pf_fmap_set_samples: an index lies outside 0 .. n_t - 1 = %lld (target) or 0 .. n_s - 1 = %lld (source)",
                     (long long)(h->n_t - 1), (long long)(h->n_s - 1));
        fmap_free_samples(h);
        return PF_E_ARG;
    }
    h->has_samples = true;
    return PF_OK;
}

int pf_fmap_zoomout_sampled(pf_fmap* h, int32_t k_start, int32_t k_end, int32_t step, int32_t n_iter_at_end, double* C_out) {
    PF_CHECK(h != nullptr, PF_E_ARG, "pf_fmap_zoomout_sampled: NULL handle");
    PF_CHECK(k_start >= 1 && k_start <= k_end && k_end <= h->K && step >= 1 && n_iter_at_end >= 0, PF_E_ARG,
             "pf_fmap_zoomout_sampled: k_start %d, k_end %d (K = %d), step %d, n_iter_at_end %d out of range", k_start, k_end, h->K, step,
             n_iter_at_end);
    PF_CHECK(h->has_samples, PF_E_STATE, "pf_fmap_zoomout_sampled: no samples yet (pf_fmap_set_samples)");
    PF_CHECK(h->has_T, PF_E_STATE, "pf_fmap_zoomout_sampled: no point map yet (pf_fmap_set_p2p)");
    PF_CHECK(h->q_s >= k_end, PF_E_ARG, "pf_fmap_zoomout_sampled: %lld source samples cannot determine a fit with k_end = %d functions",
             (long long)h->q_s, k_end);
    pf_ctx* c = h->ctx;
    PF_HIP(hipSetDevice(c->device));
    const FmapView sub = fmap_sub(h);
    FmapView gram = sub;  // A^T A: the identity map into A itself
    gram.phi_t = h->A, gram.n_t = h->q_s, gram.T = h->ident;
    std::vector<double> G((size_t)k_end * k_end), X((size_t)k_end * k_end);
    PF_TRY(fmap_project(h, gram, k_end, k_end, h->G));
    PF_HIP(hipMemcpyAsync(G.data(), h->G, sizeof(double) * G.size(), hipMemcpyDeviceToHost, c->stream));
    PF_HIP(hipStreamSynchronize(c->stream));  // once per call: no copy into G is in flight if a later step fails
    int32_t k = k_start, extra = n_iter_at_end;
    PF_TRY(fmap_project(h, fmap_full(h), k, k, h->C));
    for (;;) {
        PF_TRY(fmap_convert(h, sub, k, k));
        const bool last = k == k_end && extra == 0;
        if (k == k_end && !last) --extra;
        k = std::min(k + step, k_end);
        PF_TRY(fmap_project(h, sub, k, k, h->R));
        const size_t count = (size_t)k * k;
        PF_HIP(hipMemcpyAsync(X.data(), h->R, sizeof(double) * count, hipMemcpyDeviceToHost, c->stream));
        PF_HIP(hipStreamSynchronize(c->stream));  // the one wait of the round
        // G's entries carry the rounding of q_s terms each, the pivot's sum that of k more
        PF_CHECK(chol_solve(G.data(), k_end, k, (double)(h->q_s + k) * 2.220446049250313e-16, X.data()), PF_E_DEGENERATE,
                 "pf_fmap_zoomout_sampled: A^T A is not positive definite at k = %d: the %lld source samples are too few or degenerate for "
                 "this many basis functions", k, (long long)h->q_s);
        PF_HIP(hipMemcpyAsync(h->C, X.data(), sizeof(double) * count, hipMemcpyHostToDevice, c->stream));
        PF_HIP(hipStreamSynchronize(c->stream));  // X is written again in the next round
        h->c_ks = h->c_kt = k;
        if (last) break;
    }
    PF_TRY(fmap_convert(h, fmap_full(h), k_end, k_end));
    if (C_out) memcpy(C_out, X.data(), sizeof(double) * (size_t)k_end * k_end);
    PF_HIP(hipStreamSynchronize(c->stream));
    return PF_OK;
}

}  // extern "C"
