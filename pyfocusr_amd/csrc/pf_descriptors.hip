// Spectral descriptors on the device: every descriptor of the form
//   F[i][t] = sum_a phi[i][a]^2 g_t(lambda_a)
// (heat kernel signature: g_t = exp(-lambda tau_t); wave kernel signature: a normalised log-normal band around e_t; ...)
// is one product of the squared basis with a small host-made table G[K][T], and its mass-weighted projection onto the
// basis
//   A[a][t] = sum_i mass[i] phi[i][a] F[i][t]
// is what a functional map is fitted to.  Two entry points, both FP64, no handle, no state:
//
// pf_spectral_descriptors.  F as above; a ascends, every term is (p * p) * g with a separate multiply and a separate add
// (the file is compiled without contraction): the bits of the obvious numpy loop.
//
// pf_descriptor_coefficients.  A as above without F ever reaching memory (n = 250k, T = 200: 400 MB).  Each term is
// phi[i][a] * (mass[i] * F[i][t]); a block owns 512 rows and adds them in row order, its partial sum in its own slot;
// k_desc_combine adds the slots in block order.  No floating-point atomic: two calls give the same bits.
//
// form_rows.  Both kernels form F the same way.  A block of 256 lanes owns 512 rows, two per lane (rows tid and
// tid + 256), and a tile of TT columns of G, all K rows of it, in LDS (K = 128, TT = 16: 16 KiB).  A lane keeps its
// 2 x TT sums in registers and walks a in ascending order, eight at a time: it loads eight phi of each of its rows (64
// contiguous bytes of a row-major row), squares them, and reads G[a][t] from LDS - every lane of a wave the same word,
// a broadcast, one read serving both rows.  Per word read from LDS a wave issues four FP64 instructions.  T is cut into
// tiles (the grid's y) because G[128][512] is 512 KiB; each tile reads phi again, from L2.
//
// k_desc_project.  TT = 8: the lanes put mass[i] * F[i][t] of the block's 512 rows into LDS (36 KiB beside 8 KiB of G:
// three blocks per CU), then every lane owns one column t and up to four basis functions a (a = tid / 8 + 32 j) and
// walks the rows in ascending order, reading phi[i][a] from memory (eight neighbouring words per wave and load).
// Rows with mass 0 and rows whose phi is all zero add exactly 0; rows past n are never visited.
//
// Nothing here has been timed on an MI355X yet (profiles/spectral_descriptors.md; tools/bench_descriptors.py).
#include "pf_internal.h"

namespace {

constexpr int DESC_MAX_K = 128;
constexpr int DESC_MAX_T = 512;
constexpr int DESC_ROWS = 512;   // rows per block: two per lane
constexpr int DESC_AC = 8;       // basis functions per chunk of a lane's loads
constexpr int EVAL_TT = 16;      // columns of G per block of k_desc_eval
constexpr int PROJ_TT = 8;       // ... of k_desc_project
constexpr int PROJ_LD = PROJ_TT + 1;  // row stride of the F tile in LDS (odd: the lanes' stores spread over the banks)
constexpr int PROJ_AJ = DESC_MAX_K / (PF_BLOCK / PROJ_TT);  // basis functions per lane of the projection: 4

__host__ __device__ inline int64_t imin(int64_t a, int64_t b) { return a < b ? a : b; }

// gs[a][j] = G[a][t0 + j] for a < K, j < TT; 0 past T
template <int TT>
__device__ void stage_g(const double* __restrict__ G, int32_t K, int32_t T, int32_t t0, double* __restrict__ gs) {
    for (int e = threadIdx.x; e < K * TT; e += PF_BLOCK) {
        const int a = e / TT, j = e - a * TT;
        gs[e] = (t0 + j < T) ? G[(int64_t)a * T + t0 + j] : 0.0;
    }
}

// acc[r][j] = sum_a phi[row_r][a]^2 gs[a][j], a ascending, separate multiply and add
template <int TT>
__device__ void form_rows(const double* __restrict__ phi, int32_t K, const int64_t (&row)[2], const double* __restrict__ gs,
                          double (&acc)[2][TT]) {
#pragma unroll
    for (int r = 0; r < 2; ++r)
#pragma unroll
        for (int j = 0; j < TT; ++j) acc[r][j] = 0.0;
    for (int a0 = 0; a0 < K; a0 += DESC_AC) {
        const int na = K - a0 < DESC_AC ? K - a0 : DESC_AC;
        double p2[2][DESC_AC];
#pragma unroll
        for (int r = 0; r < 2; ++r)
#pragma unroll
            for (int c = 0; c < DESC_AC; ++c) {
                const double p = c < na ? phi[row[r] * K + a0 + c] : 0.0;
                p2[r][c] = p * p;
            }
#pragma unroll
        for (int c = 0; c < DESC_AC; ++c) {
            if (c < na) {  // uniform over the block
#pragma unroll
                for (int j = 0; j < TT; ++j) {
                    const double g = gs[(a0 + c) * TT + j];
#pragma unroll
                    for (int r = 0; r < 2; ++r) acc[r][j] += p2[r][c] * g;
                }
            }
        }
    }
}

// grid: (blocks of 512 rows, tiles of EVAL_TT columns)
__global__ __launch_bounds__(PF_BLOCK) void k_desc_eval(const double* __restrict__ phi, int64_t n, int32_t K, const double* __restrict__ G,
                                                        int32_t T, double* __restrict__ out) {
    __shared__ double gs[DESC_MAX_K * EVAL_TT];
    const int tid = threadIdx.x;
    const int32_t t0 = (int32_t)blockIdx.y * EVAL_TT;
    const int64_t row0 = (int64_t)blockIdx.x * DESC_ROWS;
    stage_g<EVAL_TT>(G, K, T, t0, gs);
    __syncthreads();
    // a lane past the end works on the last row and stores nothing
    const int64_t row[2] = {imin(row0 + tid, n - 1), imin(row0 + PF_BLOCK + tid, n - 1)};
    double acc[2][EVAL_TT];
    form_rows<EVAL_TT>(phi, K, row, gs, acc);
#pragma unroll
    for (int r = 0; r < 2; ++r) {
        const int64_t i = row0 + r * PF_BLOCK + tid;
        if (i < n) {
#pragma unroll
            for (int j = 0; j < EVAL_TT; ++j)
                if (t0 + j < T) out[i * T + t0 + j] = acc[r][j];
        }
    }
}

// grid: (blocks of 512 rows, tiles of PROJ_TT columns); block b writes part + b * k_out * T
__global__ __launch_bounds__(PF_BLOCK) void k_desc_project(const double* __restrict__ phi, const double* __restrict__ mass, int64_t n,
                                                           int32_t K, const double* __restrict__ G, int32_t T, int32_t k_out,
                                                           double* __restrict__ part) {
    __shared__ double gs[DESC_MAX_K * PROJ_TT];
    __shared__ double fs[DESC_ROWS * PROJ_LD];
    const int tid = threadIdx.x;
    const int32_t t0 = (int32_t)blockIdx.y * PROJ_TT;
    const int64_t row0 = (int64_t)blockIdx.x * DESC_ROWS;
    const int nr = (int)imin(DESC_ROWS, n - row0);
    stage_g<PROJ_TT>(G, K, T, t0, gs);
    __syncthreads();
    {
        const int64_t row[2] = {imin(row0 + tid, n - 1), imin(row0 + PF_BLOCK + tid, n - 1)};
        double acc[2][PROJ_TT];
        form_rows<PROJ_TT>(phi, K, row, gs, acc);
#pragma unroll
        for (int r = 0; r < 2; ++r) {
            const double m = mass[row[r]];
#pragma unroll
            for (int j = 0; j < PROJ_TT; ++j) fs[(r * PF_BLOCK + tid) * PROJ_LD + j] = m * acc[r][j];  // rows >= nr: never read
        }
    }
    __syncthreads();
    const int j = tid & (PROJ_TT - 1), a_lo = tid / PROJ_TT;  // a = a_lo + 32 q
    double sum[PROJ_AJ];
#pragma unroll
    for (int q = 0; q < PROJ_AJ; ++q) sum[q] = 0.0;
    const double* prow = phi + row0 * K;
    for (int r = 0; r < nr; ++r, prow += K) {
        const double f = fs[r * PROJ_LD + j];
#pragma unroll
        for (int q = 0; q < PROJ_AJ; ++q) {
            const int a = a_lo + q * (PF_BLOCK / PROJ_TT);
            if (a < k_out) sum[q] += prow[a] * f;
        }
    }
    double* o = part + (int64_t)blockIdx.x * k_out * T;
    if (t0 + j < T) {
#pragma unroll
        for (int q = 0; q < PROJ_AJ; ++q) {
            const int a = a_lo + q * (PF_BLOCK / PROJ_TT);
            if (a < k_out) o[(int64_t)a * T + t0 + j] = sum[q];
        }
    }
}

__global__ __launch_bounds__(PF_BLOCK) void k_desc_combine(const double* __restrict__ part, int64_t count, int64_t blocks, double* __restrict__ out) {
    const int64_t e = (int64_t)blockIdx.x * PF_BLOCK + threadIdx.x;
    if (e >= count) return;
    double s = part[e];
    for (int64_t b = 1; b < blocks; ++b) s += part[b * count + e];
    out[e] = s;
}

}  // namespace

extern "C" {

int pf_spectral_descriptors(pf_ctx* c, const double* phi, int64_t n, int32_t K, const double* G, int32_t T, double* out) {
    PF_CHECK(c && phi && G && out, PF_E_ARG, "pf_spectral_descriptors: NULL argument");
    PF_CHECK(n >= 1 && n < ((int64_t)1 << 31) && K >= 1 && K <= DESC_MAX_K && T >= 1 && T <= DESC_MAX_T, PF_E_ARG,
             "pf_spectral_descriptors: n %lld, K %d, T %d out of range (n >= 1, 1 <= K <= 128, 1 <= T <= 512)", (long long)n, K, T);
    PF_HIP(hipSetDevice(c->device));
    Scratch s(c->stream);
    double* d_phi = s.get<double>((size_t)(n * K));
    double* d_g = s.get<double>((size_t)K * T);
    double* d_out = s.get<double>((size_t)(n * T));
    s.upload(d_phi, phi, (size_t)(n * K));
    s.upload(d_g, G, (size_t)K * T);
    if (s.ok()) {
        const dim3 grid((unsigned)((n + DESC_ROWS - 1) / DESC_ROWS), (unsigned)((T + EVAL_TT - 1) / EVAL_TT));
        k_desc_eval<<<grid, PF_BLOCK, 0, s.st>>>(d_phi, n, K, d_g, T, d_out);
        s.launched();
    }
    s.download(out, d_out, (size_t)(n * T));
    s.sync();
    PF_CHECK(s.ok(), PF_E_HIP, "pf_spectral_descriptors: %s", hipGetErrorString(s.err));
    return PF_OK;
}

int pf_descriptor_coefficients(pf_ctx* c, const double* phi, const double* mass, int64_t n, int32_t K, const double* G, int32_t T,
                               int32_t k_out, double* A_out) {
    PF_CHECK(c && phi && mass && G && A_out, PF_E_ARG, "pf_descriptor_coefficients: NULL argument");
    PF_CHECK(n >= 1 && n < ((int64_t)1 << 31) && K >= 1 && K <= DESC_MAX_K && T >= 1 && T <= DESC_MAX_T && k_out >= 1 && k_out <= K,
             PF_E_ARG, "pf_descriptor_coefficients: n %lld, K %d, T %d, k_out %d out of range (n >= 1, 1 <= k_out <= K <= 128, 1 <= T <= 512)",
             (long long)n, K, T, k_out);
    PF_HIP(hipSetDevice(c->device));
    Scratch s(c->stream);
    const int64_t blocks = (n + DESC_ROWS - 1) / DESC_ROWS, count = (int64_t)k_out * T;
    double* d_phi = s.get<double>((size_t)(n * K));
    double* d_mass = s.get<double>((size_t)n);
    double* d_g = s.get<double>((size_t)K * T);
    double* d_a = s.get<double>((size_t)count);
    double* part = blocks > 1 ? s.get<double>((size_t)(blocks * count)) : d_a;
    s.upload(d_phi, phi, (size_t)(n * K));
    s.upload(d_mass, mass, (size_t)n);
    s.upload(d_g, G, (size_t)K * T);
    if (s.ok()) {
        const dim3 grid((unsigned)blocks, (unsigned)((T + PROJ_TT - 1) / PROJ_TT));
        k_desc_project<<<grid, PF_BLOCK, 0, s.st>>>(d_phi, d_mass, n, K, d_g, T, k_out, part);
        if (blocks > 1) k_desc_combine<<<pf_blocks(count), PF_BLOCK, 0, s.st>>>(part, count, blocks, d_a);
        s.launched();
    }
    s.download(A_out, d_a, (size_t)count);
    s.sync();
    PF_CHECK(s.ok(), PF_E_HIP, "pf_descriptor_coefficients: %s", hipGetErrorString(s.err));
    return PF_OK;
}

}  // extern "C"
