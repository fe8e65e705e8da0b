// The exact Euclidean distance transform of a binary volume with anisotropic spacing, and its feature transform
// (pf_edt_*).  The definition is in include/pyfocusr_hip.h; tests/_edt_ref.py restates it in numpy and the device returns
// its bits.  Three separable passes, every one an ordinary launch with one lane per voxel:
//   k_edt_pack   the mask (or its complement) as one bit per voxel, a z-line of nz voxels in ceil(nz / 64) words (__ballot,
//                as k_iso_classify packs its sign bits); the wave's popcounts are the report's foreground count
//   k_edt_z      the nearest set bit below and above the voxel on its own z-line: count-leading / count-trailing zeros
//                over the voxel's word and then its neighbours; the nearer wins, the lower on a tie
//   k_edt_line   (axis y, then x) a search outward from the voxel's own position, r = 0, 1, 2, ..., the candidate at
//                pos - r before the one at pos + r, until t(r) = (s r)(s r) > best.  The lanes of a wave are consecutive
//                in k, so a wave walks one line offset together and every candidate read is coalesced
//   k_edt_signed the combine of signed mode: the passes ran on the mask and on its complement
// Between the passes a voxel carries (value, nearest): 12 bytes, the value not recomputed from the index.  No block waits
// for another, no floating-point atomics (the one integer atomic is the foreground count): two calls give the same bits.
// Arithmetic: separate multiplies and adds (-ffp-contract=off).
#include <cmath>

#include "pf_internal.h"

struct pf_edt {
    pf_ctx* ctx = nullptr;
    int64_t nx = 0, ny = 0, nz = 0, foreground = 0;
    int32_t mode = 0;
    double spacing[3] = {1.0, 1.0, 1.0};
    double* dist = nullptr;     // [N]
    double* dist2 = nullptr;    // [N]
    int32_t* nearest = nullptr; // [N]
};

namespace {

struct EdtGrid {
    int64_t nx, ny, nz;
    int64_t words;  // 64-bit words of a z-line
};

constexpr int EDT_LINE = 16;  // words of a block of k_edt_pack: one 128-byte line of `bits`
static_assert(EDT_LINE % (PF_BLOCK / PF_WAVE) == 0, "every wave of k_edt_pack takes the same number of words");

// bits[w]: bit t of word w of z-line `row` is the voxel k = 64 (w mod words) + t; bits past nz are 0.  invert: the
// complement's bits.  *count (may be NULL) += the set bits.
__global__ __launch_bounds__(PF_BLOCK) void k_edt_pack(const uint8_t* __restrict__ mask, EdtGrid g, int invert,
                                                       unsigned long long* __restrict__ bits, unsigned long long* __restrict__ count) {
    constexpr int PER_WAVE = EDT_LINE / (PF_BLOCK / PF_WAVE);
    const int lane = threadIdx.x & (PF_WAVE - 1);
    const int64_t n_words = g.nx * g.ny * g.words;
    const int64_t w0 = (int64_t)blockIdx.x * EDT_LINE + (threadIdx.x / PF_WAVE) * PER_WAVE;
    unsigned long long mine = 0;
    int set = 0;
#pragma unroll
    for (int t = 0; t < PER_WAVE; ++t) {
        const int64_t w = w0 + t, row = w / g.words, k = (w - row * g.words) * PF_WAVE + lane;
        const bool valid = w < n_words && k < g.nz;
        const bool on = valid && ((mask[row * g.nz + k] != 0) != (invert != 0));
        const unsigned long long word = __ballot(on);
        if (lane == t) mine = word;
        set += __popcll(word);
    }
    if (lane < PER_WAVE && w0 + lane < n_words) bits[w0 + lane] = mine;
    if (count && lane == 0 && set) atomicAdd(count, (unsigned long long)set);
}

// Stage z.  One lane per voxel: val = t_z of the nearest feature of its own z-line, near = that feature's flat index;
// +inf and -1 on a line without one.  t_z grows strictly with |d| (pf_edt_create refuses the spacings where it would
// not), so the nearest in |d| is the minimiser and the lower one wins the tie of the two sides.
__global__ __launch_bounds__(PF_BLOCK) void k_edt_z(const unsigned long long* __restrict__ bits, EdtGrid g, double sz,
                                                    double* __restrict__ val, int32_t* __restrict__ near) {
    const int64_t p = (int64_t)blockIdx.x * PF_BLOCK + threadIdx.x;
    if (p >= g.nx * g.ny * g.nz) return;
    const int64_t row = p / g.nz, k = p - row * g.nz;
    const unsigned long long* __restrict__ W = bits + row * g.words;
    const int64_t w = k >> 6;
    const int b = (int)(k & 63);
    int64_t kl = -1, kr = -1;
    unsigned long long m = W[w] & (~0ull >> (63 - b));  // the bits at or below k
    for (int64_t ww = w;;) {
        if (m) {
            kl = ww * 64 + 63 - __clzll((long long)m);
            break;
        }
        if (--ww < 0) break;
        m = W[ww];
    }
    m = W[w] & ((~0ull << b) << 1);  // the bits above k
    for (int64_t ww = w;;) {
        if (m) {
            kr = ww * 64 + __ffsll((long long)m) - 1;
            break;
        }
        if (++ww >= g.words) break;
        m = W[ww];
    }
    if (kl < 0 && kr < 0) {
        val[p] = INFINITY;
        near[p] = -1;
        return;
    }
    const int64_t kk = kr < 0 || (kl >= 0 && k - kl <= kr - k) ? kl : kr;
    const double a = sz * (double)(k - kk);
    val[p] = a * a;
    near[p] = (int32_t)(row * g.nz + kk);
}

// Stages y (axis 1) and x (axis 0).  One lane per voxel, at position `pos` of its line of `len` voxels `stride` apart:
// out = min over the line's positions c of fl(g_in[c] + t(|pos - c|)), the lower c on a tie, and that candidate's
// `near`.  Every candidate at offset r costs at least t(r) (g >= 0, the addition is monotone) and t does not decrease
// with r, so stopping at t(r) > best, strictly, loses neither a minimiser nor a tie.  A candidate of infinite cost is one
// without a feature: it never replaces anything, so a line without any carries +inf and -1 through.
// root (may be NULL): sqrt(out) with the device's double square root.
__global__ __launch_bounds__(PF_BLOCK) void k_edt_line(EdtGrid g, int axis, double s, const double* __restrict__ g_in,
                                                       const int32_t* __restrict__ near_in, double* __restrict__ g_out,
                                                       int32_t* __restrict__ near_out, double* __restrict__ root) {
    const int64_t p = (int64_t)blockIdx.x * PF_BLOCK + threadIdx.x;
    if (p >= g.nx * g.ny * g.nz) return;
    const int64_t row = p / g.nz, i = row / g.ny, j = row - i * g.ny;
    const int64_t pos = axis == 1 ? j : i, len = axis == 1 ? g.ny : g.nx, stride = axis == 1 ? g.nz : g.ny * g.nz;
    double best = g_in[p];  // r = 0: t = 0 and fl(g + 0) = g
    int64_t at = p;
    const int64_t r_max = pos > len - 1 - pos ? pos : len - 1 - pos;
    for (int64_t r = 1; r <= r_max; ++r) {
        const double a = s * (double)r, t = a * a;
        if (t > best) break;
        const bool has_lo = r <= pos, has_hi = pos + r < len;
        const int64_t q_lo = p - r * stride, q_hi = p + r * stride;
        const double g_lo = has_lo ? g_in[q_lo] : INFINITY, g_hi = has_hi ? g_in[q_hi] : INFINITY;
        const double c_lo = g_lo + t, c_hi = g_hi + t;
        if (c_lo <= best && c_lo < INFINITY) best = c_lo, at = q_lo;  // lower than every candidate before it
        if (c_hi < best) best = c_hi, at = q_hi;                      // higher than every candidate before it
    }
    g_out[p] = best;
    near_out[p] = near_in[at];
    if (root) root[p] = sqrt(best);
}

// Signed mode: (d2f, nf) of the mask's transform, (dist2, nearest) of its complement's, in place.
// dist = sqrt(d2f) - sqrt(d2b): one of the two is 0.  dist2 and nearest are those of the other class.
__global__ __launch_bounds__(PF_BLOCK) void k_edt_signed(const uint8_t* __restrict__ mask, int64_t n, const double* __restrict__ d2f,
                                                         const int32_t* __restrict__ nf, double* __restrict__ dist2,
                                                         int32_t* __restrict__ nearest, double* __restrict__ dist) {
    const int64_t p = (int64_t)blockIdx.x * PF_BLOCK + threadIdx.x;
    if (p >= n) return;
    const double f = d2f[p], b = dist2[p];
    dist[p] = sqrt(f) - sqrt(b);
    if (!mask[p]) dist2[p] = f, nearest[p] = nf[p];
}

// t(1) is a normal number and t(n - 1) finite along an axis of n voxels: then t grows strictly with the offset
bool edt_spacing_ok(double s, int64_t n) {
    if (!(std::isfinite(s) && s > 0.0)) return false;
    const double a = s * (double)(n > 1 ? n - 1 : 1);
    return s * s >= 2.2250738585072014e-308 && std::isfinite(a * a);
}

}  // namespace

extern "C" {

void pf_edt_free(pf_edt* h) {
    if (!h) return;
    (void)hipSetDevice(h->ctx->device);
    (void)hipStreamSynchronize(h->ctx->stream);
    hipStream_t st = h->ctx->stream;
    pf_free(st, h->dist);
    pf_free(st, h->dist2);
    pf_free(st, h->nearest);
    delete h;
}

int pf_edt_create(pf_ctx* ctx, const uint8_t* mask, int64_t nx, int64_t ny, int64_t nz, const double* spacing, int32_t mode,
                  uint32_t flags, pf_edt** out, int64_t* report, double* device_ms) {
    PF_CHECK(ctx && mask && spacing && out, PF_E_ARG, "pf_edt_create: NULL argument");
    PF_CHECK(flags == 0, PF_E_ARG, "pf_edt_create: unknown flags 0x%x", flags);
    PF_CHECK(mode == PF_EDT_UNSIGNED || mode == PF_EDT_SIGNED, PF_E_ARG, "pf_edt_create: unknown mode %d", mode);
    const int64_t lim = (int64_t)1 << 31;
    PF_CHECK(nx >= 1 && ny >= 1 && nz >= 1 && nx < lim && ny < lim && nz < lim, PF_E_ARG,
             "pf_edt_create: extents %lld x %lld x %lld out of range (each 1..2^31-1)", (long long)nx, (long long)ny, (long long)nz);
    PF_CHECK(nx * ny < lim && nx * ny * nz < lim, PF_E_ARG, "pf_edt_create: %lld x %lld x %lld samples out of range (< 2^31)",
             (long long)nx, (long long)ny, (long long)nz);
    const int64_t extent[3] = {nx, ny, nz};
    double t_max = 0.0;
    for (int a = 0; a < 3; ++a) {
        PF_CHECK(std::isfinite(spacing[a]) && spacing[a] > 0.0, PF_E_ARG, "pf_edt_create: spacing %d is not positive and finite", a);
        PF_CHECK(edt_spacing_ok(spacing[a], extent[a]), PF_E_ARG,
                 "pf_edt_create: spacing %d = %g: its squared distances leave the range of normal doubles", a, spacing[a]);
        const double d = spacing[a] * (double)(extent[a] - 1);
        t_max += d * d;
    }
    PF_CHECK(std::isfinite(t_max), PF_E_ARG, "pf_edt_create: the squared diagonal of the volume is not finite");
    const int64_t N = nx * ny * nz;
    EdtGrid g;
    g.nx = nx, g.ny = ny, g.nz = nz, g.words = (nz + 63) / 64;
    const int64_t n_words = nx * ny * g.words;
    PF_HIP(hipSetDevice(ctx->device));
    hipStream_t st = ctx->stream;
    StreamTimer timer(device_ms != nullptr);
    unsigned long long foreground = 0;
    pf_edt* h = new pf_edt();
    h->ctx = ctx, h->nx = nx, h->ny = ny, h->nz = nz, h->mode = mode;
    for (int a = 0; a < 3; ++a) h->spacing[a] = spacing[a];
    hipError_t err;
    {
        Scratch sc(st);
        const bool is_signed = mode == PF_EDT_SIGNED;
        uint8_t* d_mask = sc.get<uint8_t>(N);
        unsigned long long* bits = sc.get<unsigned long long>(n_words);
        double *va = sc.get<double>(N), *vb = sc.get<double>(N);
        int32_t *na = sc.get<int32_t>(N), *nb = sc.get<int32_t>(N);
        double* vf = is_signed ? sc.get<double>(N) : nullptr;  // the mask's own transform, until the combine
        int32_t* nf = is_signed ? sc.get<int32_t>(N) : nullptr;
        unsigned long long* d_count = sc.get<unsigned long long>(1);
        h->dist = sc.keep<double>(N);
        h->dist2 = sc.keep<double>(N);
        h->nearest = sc.keep<int32_t>(N);
        sc.upload(d_mask, mask, N);
        sc.zero(d_count, sizeof(unsigned long long));
        timer.start(sc);
        const unsigned pack_blocks = (unsigned)((n_words + EDT_LINE - 1) / EDT_LINE);
        // the three passes of the mask (invert = 0) or of its complement, the last one into (v_out, n_out[, root])
        auto transform = [&](int invert, double* v_out, int32_t* n_out, double* root) {
            if (!sc.ok()) return;
            k_edt_pack<<<pack_blocks, PF_BLOCK, 0, st>>>(d_mask, g, invert, bits, invert ? nullptr : d_count);
            k_edt_z<<<pf_blocks(N), PF_BLOCK, 0, st>>>(bits, g, spacing[2], va, na);
            k_edt_line<<<pf_blocks(N), PF_BLOCK, 0, st>>>(g, 1, spacing[1], va, na, vb, nb, nullptr);
            k_edt_line<<<pf_blocks(N), PF_BLOCK, 0, st>>>(g, 0, spacing[0], vb, nb, v_out, n_out, root);
            sc.launched();
        };
        if (!is_signed) {
            transform(0, h->dist2, h->nearest, h->dist);
        } else {
            transform(0, vf, nf, nullptr);
            transform(1, h->dist2, h->nearest, nullptr);
            if (sc.ok()) {
                k_edt_signed<<<pf_blocks(N), PF_BLOCK, 0, st>>>(d_mask, N, vf, nf, h->dist2, h->nearest, h->dist);
                sc.launched();
            }
        }
        timer.stop(sc);
        sc.download(&foreground, d_count, 1);
        sc.sync();
        timer.read(sc, device_ms);
        err = sc.err;
    }
    if (err != hipSuccess) {
        pf_edt_free(h);
        return pf_hip_failed("pf_edt_create", err);
    }
    h->foreground = (int64_t)foreground;
    if (report) {
        report[0] = N, report[1] = h->foreground, report[2] = N - h->foreground;
        report[3] = report[4] = report[5] = report[6] = report[7] = 0;
    }
    *out = h;
    return PF_OK;
}

int pf_edt_fetch(pf_edt* h, double* dist, double* dist2, int32_t* nearest) {
    PF_CHECK(h != nullptr, PF_E_ARG, "pf_edt_fetch: NULL handle");
    PF_HIP(hipSetDevice(h->ctx->device));
    const int64_t N = h->nx * h->ny * h->nz;
    Scratch sc(h->ctx->stream);
    sc.download(dist, h->dist, N);
    sc.download(dist2, h->dist2, N);
    sc.download(nearest, h->nearest, N);
    sc.sync();
    return sc.ok() ? PF_OK : pf_hip_failed("pf_edt_fetch", sc.err);
}

int pf_edt_isosurface(pf_edt* h, double level, const double* origin, pf_isosurface** out, int64_t* report, double* device_ms) {
    PF_CHECK(h && origin && out, PF_E_ARG, "pf_edt_isosurface: NULL argument");
    PF_CHECK(h->nx >= 2 && h->ny >= 2 && h->nz >= 2, PF_E_ARG, "pf_edt_isosurface: extents %lld x %lld x %lld out of range (each >= 2)",
             (long long)h->nx, (long long)h->ny, (long long)h->nz);
    PF_CHECK(std::isfinite(level), PF_E_ARG, "pf_edt_isosurface: the level is not finite");
    for (int a = 0; a < 3; ++a) PF_CHECK(std::isfinite(origin[a]), PF_E_ARG, "pf_edt_isosurface: the origin is not finite");
    const int64_t N = h->nx * h->ny * h->nz;
    PF_CHECK(h->foreground > 0 && (h->mode == PF_EDT_UNSIGNED || h->foreground < N), PF_E_ARG,
             "pf_edt_isosurface: the field is not finite: the mask has no %s", h->foreground > 0 ? "background" : "foreground");
    PF_HIP(hipSetDevice(h->ctx->device));
    Scratch sc(h->ctx->stream);
    return pf_isosurface_extract(h->ctx, "pf_edt_isosurface", sc, h->dist, h->nx, h->ny, h->nz, level, h->spacing, origin, out, report,
                                 device_ms);
}

}  // extern "C"
