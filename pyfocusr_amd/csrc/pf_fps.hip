// Farthest-point sampling on the device: m well-spread rows of an n x d point set (1 <= d <= 16), with the Voronoi owner
// and the squared distance to the nearest sample of every point.
//
// Definition (tests/_fps_ref.py states it in numpy; the two agree bit for bit).  d2(i, c) = the sum over the coordinates,
// left to right, of (P[i][x] - c[x])^2 with separate multiply and add (the file is compiled without contraction).
//   start >= 0: the first sample.  start = -1: the point with the largest d2 to the centroid, the lowest index on ties; the
//   centroid is the per-coordinate mean summed in index order - on the host, in the pass that hands the points over, so it
//   is the reference's to the bit.
//   dmin = +inf, owner = 0, cur = the first sample; round j = 0 .. m - 1:  sel[j] = cur;  every i with d2(i, cur) < dmin[i]
//   (strict) takes dmin[i] = d2(i, cur), owner[i] = j;  cur = argmax dmin, the lowest index on ties.
// Once every dmin is 0 (m beyond the number of distinct points) the argmax is index 0 again and again: samples repeat.
//
// Launch structure.  Two launches per sample, m times back to back on the ctx stream, no host wait in between:
//   k_fps_round  a grid-stride pass over the points (coordinate-major: the loads of a wave are contiguous).  The current
//                sample is read through sel[j], which the launch before wrote.  Every lane updates its points and keeps the
//                best (value, lowest index) of them; shuffles reduce a wave, LDS the block's four waves; the block's best goes
//                into its own slot (at most FPS_MAX_BLOCKS of them).
//   k_fps_pick   one block reduces the slots to sel[j + 1].
// The kernel boundary is what publishes the slots: no ticket, no fence, no wait of one block for another, nothing that
// could hang.  The comparison is total - larger value, then lower index - so the order of the reduction does not matter.
// A NaN never wins a comparison and an empty result falls back to index 0: every index read stays inside the set whatever
// the input holds; non-finite input is flagged by k_fps_prepare and refused after the one download.
#include <algorithm>

#include "pf_internal.h"

namespace {

constexpr int FPS_MAX_BLOCKS = 2048;
constexpr int FPS_WAVES = PF_BLOCK / PF_WAVE;
constexpr int32_t FPS_NONE = 0x7fffffff;

__device__ inline bool fps_better(double v, int32_t i, double bv, int32_t bi) { return v > bv || (v == bv && i < bi); }

// the block's best (value, lowest index) in thread 0
__device__ inline void fps_block_best(double& v, int32_t& i) {
    __shared__ double sv[FPS_WAVES];
    __shared__ int32_t si[FPS_WAVES];
#pragma unroll
    for (int off = PF_WAVE / 2; off > 0; off >>= 1) {
        const double ov = __shfl_down(v, off, PF_WAVE);
        const int32_t oi = __shfl_down(i, off, PF_WAVE);
        if (fps_better(ov, oi, v, i)) v = ov, i = oi;
    }
    const int lane = threadIdx.x & (PF_WAVE - 1), wave = threadIdx.x / PF_WAVE;
    if (lane == 0) sv[wave] = v, si[wave] = i;
    __syncthreads();
    if (threadIdx.x == 0) {
#pragma unroll
        for (int w = 1; w < FPS_WAVES; ++w)
            if (fps_better(sv[w], si[w], v, i)) v = sv[w], i = si[w];
    }
}

// pt[x][i] = in[i][x]; dmin = +inf, owner = 0; *bad |= 1 for a coordinate that is not finite
__global__ __launch_bounds__(PF_BLOCK) void k_fps_prepare(const double* __restrict__ in, int64_t n, int32_t d, double* __restrict__ pt,
                                                          double* __restrict__ dmin, int32_t* __restrict__ owner, int32_t* __restrict__ bad) {
    const int64_t e = (int64_t)blockIdx.x * PF_BLOCK + threadIdx.x;
    if (e >= n * d) return;
    const int64_t x = e / n, i = e - x * n;
    const double v = in[i * d + x];
    pt[e] = v;
    if (!(fabs(v) < __longlong_as_double(0x7ff0000000000000ll))) atomicOr(bad, 1);
    if (e < n) dmin[e] = __longlong_as_double(0x7ff0000000000000ll), owner[e] = 0;
}

__global__ void k_fps_set_first(int64_t* __restrict__ sel, int64_t start) { sel[0] = start; }

// D > 0: the depth at compile time; 0: a loop over d.  FIRST: distances to `center` (the centroid) and nothing stored but
// the block's best; otherwise round j against the point sel[j].
template <int D, bool FIRST>
__global__ __launch_bounds__(PF_BLOCK) void k_fps_round(const double* __restrict__ pt, int64_t n, int32_t d, const double* __restrict__ center,
                                                        const int64_t* __restrict__ sel, int32_t j, double* __restrict__ dmin,
                                                        int32_t* __restrict__ owner, double* __restrict__ part_v,
                                                        int32_t* __restrict__ part_i) {
    const int32_t dd = D > 0 ? D : d;
    // the current point's coordinate x is cp[x * cs]: every lane reads the same word
    const double* cp = FIRST ? center : pt + sel[j];
    const int64_t cs = FIRST ? 1 : n;
    double c[D > 0 ? D : 1];
    if (D > 0) {
#pragma unroll
        for (int x = 0; x < D; ++x) c[x] = cp[x * cs];
    }
    double bv = -1.0;
    int32_t bi = FPS_NONE;
    const int64_t stride = (int64_t)gridDim.x * PF_BLOCK;
    for (int64_t i = (int64_t)blockIdx.x * PF_BLOCK + threadIdx.x; i < n; i += stride) {  // ascending: > keeps the lowest index
        double acc = 0.0;
        if (D > 0) {
#pragma unroll
            for (int x = 0; x < D; ++x) {
                const double diff = pt[x * n + i] - c[x];
                acc += diff * diff;
            }
        } else {
            for (int x = 0; x < dd; ++x) {
                const double diff = pt[x * n + i] - cp[x * cs];
                acc += diff * diff;
            }
        }
        double v = acc;
        if (!FIRST) {
            v = dmin[i];
            if (acc < v) {
                v = acc;
                dmin[i] = acc;
                owner[i] = j;
            }
        }
        if (v > bv) bv = v, bi = (int32_t)i;
    }
    fps_block_best(bv, bi);
    if (threadIdx.x == 0) part_v[blockIdx.x] = bv, part_i[blockIdx.x] = bi;
}

__global__ __launch_bounds__(PF_BLOCK) void k_fps_pick(const double* __restrict__ part_v, const int32_t* __restrict__ part_i, int32_t parts,
                                                       int64_t* __restrict__ sel_next) {
    double bv = -1.0;
    int32_t bi = FPS_NONE;
    for (int32_t p = threadIdx.x; p < parts; p += PF_BLOCK)
        if (fps_better(part_v[p], part_i[p], bv, bi)) bv = part_v[p], bi = part_i[p];
    fps_block_best(bv, bi);
    if (threadIdx.x == 0) *sel_next = bi == FPS_NONE ? 0 : bi;  // nothing compared (NaN everywhere): stay inside the set
}

template <bool FIRST>
void fps_launch(hipStream_t st, unsigned blocks, const double* pt, int64_t n, int32_t d, const double* center, const int64_t* sel, int32_t j,
                double* dmin, int32_t* owner, double* part_v, int32_t* part_i) {
    if (d == 1)
        k_fps_round<1, FIRST><<<blocks, PF_BLOCK, 0, st>>>(pt, n, d, center, sel, j, dmin, owner, part_v, part_i);
    else if (d == 2)
        k_fps_round<2, FIRST><<<blocks, PF_BLOCK, 0, st>>>(pt, n, d, center, sel, j, dmin, owner, part_v, part_i);
    else if (d == 3)
        k_fps_round<3, FIRST><<<blocks, PF_BLOCK, 0, st>>>(pt, n, d, center, sel, j, dmin, owner, part_v, part_i);
    else
        k_fps_round<0, FIRST><<<blocks, PF_BLOCK, 0, st>>>(pt, n, d, center, sel, j, dmin, owner, part_v, part_i);
}

}  // namespace

extern "C" int pf_fps(pf_ctx* c, const double* points, int64_t n, int32_t d, int64_t m, int64_t start, int64_t* sel_out, int32_t* owner_out,
                      double* dmin_out) {
    PF_CHECK(c && points && sel_out, PF_E_ARG, "pf_fps: NULL argument");
    PF_CHECK(d >= 1 && d <= PF_ND_MAX, PF_E_ARG, "pf_fps: d = %d outside 1 .. %d", d, PF_ND_MAX);
    PF_CHECK(n >= 1 && n < ((int64_t)1 << 31), PF_E_ARG, "pf_fps: n = %lld outside 1 .. 2^31 - 1", (long long)n);
    PF_CHECK(m >= 1 && m <= n, PF_E_ARG, "pf_fps: m = %lld outside 1 .. n = %lld", (long long)m, (long long)n);
    PF_CHECK(start >= -1 && start < n, PF_E_ARG, "pf_fps: start = %lld outside -1 .. n - 1 = %lld", (long long)start, (long long)(n - 1));
    PF_HIP(hipSetDevice(c->device));
    double center[PF_ND_MAX] = {0.0};
    if (start < 0) {  // the centroid, summed in index order
        for (int64_t i = 0; i < n; ++i)
            for (int32_t x = 0; x < d; ++x) center[x] += points[i * d + x];
        for (int32_t x = 0; x < d; ++x) center[x] /= (double)n;
    }
    Scratch s(c->stream);
    const unsigned blocks = (unsigned)std::min<int64_t>(pf_blocks(n), FPS_MAX_BLOCKS);
    double* d_in = s.get<double>((size_t)(n * d));
    double* d_pt = s.get<double>((size_t)(n * d));
    double* d_dmin = s.get<double>((size_t)n);
    int32_t* d_owner = s.get<int32_t>((size_t)n);
    int64_t* d_sel = s.get<int64_t>((size_t)m);
    double* d_part_v = s.get<double>(blocks);
    int32_t* d_part_i = s.get<int32_t>(blocks);
    double* d_center = s.get<double>(PF_ND_MAX);
    int32_t* d_bad = s.get<int32_t>(1);
    int32_t bad = 0;
    s.upload(d_in, points, (size_t)(n * d));
    s.upload(d_center, center, (size_t)PF_ND_MAX);
    s.zero(d_bad, sizeof(int32_t));
    if (s.ok()) {
        k_fps_prepare<<<pf_blocks(n * d), PF_BLOCK, 0, s.st>>>(d_in, n, d, d_pt, d_dmin, d_owner, d_bad);
        if (start < 0) {
            fps_launch<true>(s.st, blocks, d_pt, n, d, d_center, d_sel, 0, d_dmin, d_owner, d_part_v, d_part_i);
            k_fps_pick<<<1, PF_BLOCK, 0, s.st>>>(d_part_v, d_part_i, (int32_t)blocks, d_sel);
        } else {
            k_fps_set_first<<<1, 1, 0, s.st>>>(d_sel, start);
        }
        for (int64_t j = 0; j < m; ++j) {
            fps_launch<false>(s.st, blocks, d_pt, n, d, d_center, d_sel, (int32_t)j, d_dmin, d_owner, d_part_v, d_part_i);
            if (j + 1 < m) k_fps_pick<<<1, PF_BLOCK, 0, s.st>>>(d_part_v, d_part_i, (int32_t)blocks, d_sel + j + 1);
        }
        s.launched();
    }
    s.download(sel_out, d_sel, (size_t)m);
    s.download(owner_out, d_owner, (size_t)n);
    s.download(dmin_out, d_dmin, (size_t)n);
    s.download(&bad, d_bad, 1);
    s.sync();  // the uploads' sources (the caller's points, center) are free again from here
    PF_CHECK(s.ok(), PF_E_HIP, "pf_fps: %s", hipGetErrorString(s.err));
    PF_CHECK(bad == 0, PF_E_ARG, "pf_fps: a coordinate is not finite");
    return PF_OK;
}
