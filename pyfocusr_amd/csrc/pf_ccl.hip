// Connected components of a mask or a label map, with exact integer statistics per component (pf_ccl_*).  The definition
// is in include/pyfocusr_hip.h; tests/_ccl_ref.py restates it in numpy and the device returns its bytes.  Every kernel is
// an ordinary launch:
//   k_ccl_pack      one lane per voxel, a z-line of nz voxels in ceil(nz / 64) words (__ballot, as k_edt_pack): `fg`, the
//                   voxels that are labelled, and `start`, those among them that are not joined with their predecessor on
//                   the line (the first voxel of a run; in by-value mode a change of value starts a run too)
//   k_ccl_runs      one lane per voxel: parent = the start of the voxel's run (the highest start bit at or below it:
//                   count-leading-zeros over the voxel's word, then the words before it), -1 on the background.  The
//                   z-connectivity is settled here without a union; only run starts are ever joined, the other voxels
//                   hang below them as leaves (a walk may start at one, and path halving may lift its link)
//   k_ccl_hook      one lane per word, for every run that starts in it: the backward half of the neighbouring lines
//                   ((i-1, j) and (i, j-1); for 18 and 26 also (i-1, j-1) and (i-1, j+1)), the runs there that overlap
//                   [k0 - r, k1 + r] (r = 1 where the connectivity reaches diagonally in z), found by count-trailing-zeros
//                   on the words; each is joined with a lock-free union: the larger root goes under the smaller by
//                   atomicMin, and a union whose root was taken meanwhile goes on with the value it displaced or met, so
//                   no join is lost and there are no rounds.  Parents only ever decrease: every walk ends, every retry
//                   strictly lowers the index it retries with, no thread waits for another.  A component's last root is
//                   its lowest voxel whatever the order of the unions
//   k_ccl_compress  every voxel's parent becomes its root; flag = (the voxel is a root)
//   (pf_scan)       rank = the exclusive scan of flag: roots in ascending order, so the components are numbered by root
//   k_ccl_number    component = rank[root] + 1, and the statistics: a wave whose labelled lanes share one component reduces
//                   count, sums and box with shuffles and sends one atomic per field; a mixed wave sends one per lane.
//                   Integer atomics only (add, min, max): the tables do not depend on their order
//   k_ccl_largest   the largest count
//   k_ccl_select    out = component > 0 && keep[component - 1]
// The one read-back inside pf_ccl_create is C, which sizes the tables.  No floating point anywhere.
#include <climits>

#include "pf_internal.h"

struct pf_ccl {
    pf_ctx* ctx = nullptr;
    int64_t nx = 0, ny = 0, nz = 0, C = 0;
    int32_t* component = nullptr;  // [N + 1] (the roots' flags with their sentinel, until the numbering)
    int64_t* count = nullptr;      // [C]
    int32_t* value = nullptr;      // [C]
    int32_t* root = nullptr;       // [C]
    int32_t* lo = nullptr;         // [C][3]
    int32_t* hi = nullptr;         // [C][3]
    uint8_t* border = nullptr;     // [C]
    int64_t* sum = nullptr;        // [C][3]
};

namespace {

typedef unsigned long long u64;

std::atomic<int> g_ccl_combine{1};  // pf_ccl_combine_stats

struct CclGrid {
    int64_t nx, ny, nz;
    int64_t words;  // 64-bit words of a z-line
};

struct CclTables {
    u64* count;
    int32_t* value;
    int32_t* root;
    int32_t* lo;
    int32_t* hi;
    uint8_t* border;
    u64* sum;
};

constexpr int CCL_LINE = 16;  // words of a block of k_ccl_pack
static_assert(CCL_LINE % (PF_BLOCK / PF_WAVE) == 0, "every wave of k_ccl_pack takes the same number of words");

__device__ __forceinline__ bool ccl_labelled(int32_t v, int mode) { return (v != 0) != (mode == PF_CCL_BACKGROUND); }

// fg[w], start[w]: bit t of word w of z-line `row` is the voxel k = 64 (w mod words) + t; bits past nz are 0.
// *n_fg += the labelled voxels.
__global__ __launch_bounds__(PF_BLOCK) void k_ccl_pack(const int32_t* __restrict__ vol, CclGrid g, int mode, u64* __restrict__ fg,
                                                       u64* __restrict__ start, u64* __restrict__ n_fg) {
    constexpr int PER_WAVE = CCL_LINE / (PF_BLOCK / PF_WAVE);
    const int lane = threadIdx.x & (PF_WAVE - 1);
    const int64_t n_words = g.nx * g.ny * g.words;
    const int64_t w0 = (int64_t)blockIdx.x * CCL_LINE + (threadIdx.x / PF_WAVE) * PER_WAVE;
    u64 my_fg = 0, my_start = 0;
    int set = 0;
#pragma unroll
    for (int t = 0; t < PER_WAVE; ++t) {
        const int64_t w = w0 + t, row = w / g.words, k = (w - row * g.words) * PF_WAVE + lane;
        const bool valid = w < n_words && k < g.nz;
        const int32_t v = valid ? vol[row * g.nz + k] : 0;
        const bool on = valid && ccl_labelled(v, mode);
        bool first = on;
        if (on && k > 0) {
            const int32_t u = vol[row * g.nz + k - 1];
            first = !ccl_labelled(u, mode) || (mode == PF_CCL_BY_VALUE && u != v);
        }
        const u64 word_fg = __ballot(on), word_start = __ballot(first);
        if (lane == t) my_fg = word_fg, my_start = word_start;
        set += __popcll(word_fg);
    }
    if (lane < PER_WAVE && w0 + lane < n_words) fg[w0 + lane] = my_fg, start[w0 + lane] = my_start;
    if (lane == 0 && set) atomicAdd(n_fg, (u64)set);
}

__global__ __launch_bounds__(PF_BLOCK) void k_ccl_runs(const u64* __restrict__ fg, const u64* __restrict__ start, CclGrid g,
                                                       int32_t* __restrict__ parent) {
    const int64_t p = (int64_t)blockIdx.x * PF_BLOCK + threadIdx.x;
    if (p >= g.nx * g.ny * g.nz) return;
    const int64_t row = p / g.nz, k = p - row * g.nz;
    int64_t w = k >> 6;
    const int b = (int)(k & 63);
    if (!((fg[row * g.words + w] >> b) & 1ull)) {
        parent[p] = -1;
        return;
    }
    const u64* __restrict__ S = start + row * g.words;
    u64 m = S[w] & (~0ull >> (63 - b));  // the starts at or below k: a labelled voxel has one
    while (!m && w > 0) m = S[--w];
    parent[p] = m ? (int32_t)(row * g.nz + w * 64 + 63 - __clzll((long long)m)) : (int32_t)p;
}

__device__ __forceinline__ int32_t link_load(const int32_t* p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }

// The root above x as far as this thread can see it.  Parents are never larger than their children, so the walk ends.
// x may be any labelled voxel, not only a run start: k_ccl_runs pointed it at the start of its run, which is a node.
// HALVE: every voxel passed is pointed at its grandparent q by atomicMin, whatever value that displaces or meets.
// The invariant that makes this safe is not "a link is replaced by an ancestor" (the value displaced may be a lower
// voxel that a concurrent union has just written, and no ancestor of q): it is that every value ever stored in
// parent[x] stays connected to x's tree through its writer's obligations.  A union that writes b over `old` goes on
// to join old with b (ccl_union); a halving that writes q read q as parent[p] with p read as parent[x], so x ~ p ~ q by
// two stored values, each of which is covered by its own writer in the same way.  So whichever value survives in
// parent[x], every other one is joined to it by the end of the launch, and dropping one loses nothing.
template <bool HALVE>
__device__ __forceinline__ int32_t ccl_find(int32_t* parent, int32_t x) {
    for (;;) {
        const int32_t p = link_load(&parent[x]);
        if (p == x) return x;
        const int32_t q = link_load(&parent[p]);
        if (q == p) return p;
        if (HALVE) atomicMin(&parent[x], q);
        x = q;
    }
}

// Join the sets of a and b.  The larger root a goes under the smaller b.  If a was a root no more when the atomicMin
// arrived, its parent then (`old` < a) either stays (old <= b) or was displaced by b: in both cases old and b are what
// is left to join, and old < a: the loop ends.  Returns the retries.  a and b are labelled voxels; k_ccl_hook passes a
// run start and the first voxel of the neighbouring run inside its window, which need not be that run's start: the
// first step of its walk leads there (or, after a halving, above it).
__device__ __forceinline__ int ccl_union(int32_t* parent, int32_t a, int32_t b) {
    int retries = 0;
    for (;;) {
        a = ccl_find<true>(parent, a);
        b = ccl_find<true>(parent, b);
        if (a == b) return retries;
        if (a < b) {
            const int32_t t = a;
            a = b, b = t;
        }
        const int32_t old = atomicMin(&parent[a], b);
        if (old == a) return retries;
        a = old;
        ++retries;
    }
}

// The first k of [from, to] (inside the line) whose bit is set in F (END = false), or in S | ~F (END = true: a run cannot
// go on over k); -1 if there is none.
template <bool END>
__device__ __forceinline__ int64_t ccl_scan_up(const u64* __restrict__ F, const u64* __restrict__ S, int64_t from, int64_t to) {
    if (from > to) return -1;
    int64_t w = from >> 6;
    const int64_t w_end = to >> 6;
    u64 m = (END ? (S[w] | ~F[w]) : F[w]) & (~0ull << (from & 63));
    for (;;) {
        if (m) {
            const int64_t k = w * 64 + __ffsll((long long)m) - 1;
            return k <= to ? k : -1;
        }
        if (++w > w_end) return -1;
        m = END ? (S[w] | ~F[w]) : F[w];
    }
}

// the last voxel of the run that holds k
__device__ __forceinline__ int64_t ccl_run_end(const u64* __restrict__ F, const u64* __restrict__ S, int64_t k, int64_t nz) {
    const int64_t e = ccl_scan_up<true>(F, S, k + 1, nz - 1);
    return e < 0 ? nz - 1 : e - 1;
}

// One lane per word: every run that starts in it against the backward lines.  n_lines of (di, dj, reach in z).
struct CclLines {
    int n;
    int di[4], dj[4], reach[4];
};

__global__ __launch_bounds__(PF_BLOCK) void k_ccl_hook(const int32_t* __restrict__ vol, const u64* __restrict__ fg,
                                                       const u64* __restrict__ start, CclGrid g, int by_value, CclLines lines,
                                                       int32_t* parent, u64* __restrict__ n_retries) {
    const int64_t w = (int64_t)blockIdx.x * PF_BLOCK + threadIdx.x;
    if (w >= g.nx * g.ny * g.words) return;
    u64 todo = start[w];
    if (!todo) return;
    const int64_t row = w / g.words, wi = w - row * g.words, i = row / g.ny, j = row - i * g.ny;
    const u64 *F = fg + row * g.words, *S = start + row * g.words;
    int retries = 0;
    while (todo) {
        const int64_t k0 = wi * 64 + __ffsll((long long)todo) - 1;
        todo &= todo - 1;
        const int64_t k1 = ccl_run_end(F, S, k0, g.nz), p = row * g.nz + k0;
        const int32_t mine = by_value ? vol[p] : 0;
        for (int l = 0; l < lines.n; ++l) {
            const int64_t i2 = i + lines.di[l], j2 = j + lines.dj[l];
            if (i2 < 0 || j2 < 0 || j2 >= g.ny) continue;
            const int64_t row2 = i2 * g.ny + j2;
            const u64 *F2 = fg + row2 * g.words, *S2 = start + row2 * g.words;
            const int64_t lo = k0 - lines.reach[l] < 0 ? 0 : k0 - lines.reach[l];
            const int64_t hi = k1 + lines.reach[l] > g.nz - 1 ? g.nz - 1 : k1 + lines.reach[l];
            for (int64_t t = lo;;) {
                const int64_t q = ccl_scan_up<false>(F2, S2, t, hi);
                if (q < 0) break;
                if (!by_value || vol[row2 * g.nz + q] == mine) retries += ccl_union(parent, (int32_t)p, (int32_t)(row2 * g.nz + q));
                t = ccl_run_end(F2, S2, q, g.nz) + 1;
            }
        }
    }
    if (retries) atomicAdd(n_retries, (u64)retries);
}

// flag [n + 1]: 1 on the roots, 0 elsewhere and on the sentinel
__global__ __launch_bounds__(PF_BLOCK) void k_ccl_compress(int32_t* parent, int64_t n, int32_t* __restrict__ flag) {
    const int64_t p = (int64_t)blockIdx.x * PF_BLOCK + threadIdx.x;
    if (p > n) return;
    int32_t r = -1;
    if (p < n && link_load(&parent[p]) >= 0) {
        r = ccl_find<false>(parent, (int32_t)p);
        __hip_atomic_store(&parent[p], r, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
    flag[p] = r == (int32_t)p ? 1 : 0;
}

__global__ __launch_bounds__(PF_BLOCK) void k_ccl_tables_init(CclTables s, int64_t C) {
    const int64_t c = (int64_t)blockIdx.x * PF_BLOCK + threadIdx.x;
    if (c >= C) return;
    s.count[c] = 0;
    s.border[c] = 0;
    for (int a = 0; a < 3; ++a) s.lo[3 * c + a] = INT_MAX, s.hi[3 * c + a] = -1, s.sum[3 * c + a] = 0;
}

template <class T, class F>
__device__ __forceinline__ T wave_reduce(T v, F f) {
#pragma unroll
    for (int o = PF_WAVE / 2; o > 0; o >>= 1) v = f(v, __shfl_xor(v, o));
    return v;
}

__device__ __forceinline__ void ccl_send(const CclTables& s, int32_t c, u64 count, const long long* sum, const int* lo, const int* hi,
                                         bool border) {
    atomicAdd(&s.count[c], count);
    for (int a = 0; a < 3; ++a) {
        atomicAdd(&s.sum[3 * c + a], (u64)sum[a]);
        atomicMin(&s.lo[3 * c + a], lo[a]);
        atomicMax(&s.hi[3 * c + a], hi[a]);
    }
    if (border) s.border[c] = 1;  // several threads may store the same 1
}

// s.count == NULL: the labelling only (C = 0)
__global__ __launch_bounds__(PF_BLOCK) void k_ccl_number(const int32_t* __restrict__ parent, const int32_t* __restrict__ rank,
                                                         const int32_t* __restrict__ vol, CclGrid g, int mode, int combine,
                                                         int32_t* __restrict__ component, CclTables s) {
    const int64_t p = (int64_t)blockIdx.x * PF_BLOCK + threadIdx.x;
    const bool valid = p < g.nx * g.ny * g.nz;
    const int32_t par = valid ? parent[p] : -1;
    const bool on = par >= 0;
    const int32_t c = on ? rank[par] : -1;
    if (valid) component[p] = c + 1;
    if (!s.count) return;
    const u64 members = __ballot(on);
    if (!members) return;
    const int64_t row = valid ? p / g.nz : 0, k = valid ? p - row * g.nz : 0, i = row / g.ny, j = row - i * g.ny;
    const int at[3] = {(int)i, (int)j, (int)k};
    const bool border = on && (i == 0 || i == g.nx - 1 || j == 0 || j == g.ny - 1 || k == 0 || k == g.nz - 1);
    if (on && par == (int32_t)p) {
        s.root[c] = par;
        s.value[c] = mode == PF_CCL_BACKGROUND ? 0 : vol[p];
    }
    const int first = __ffsll((long long)members) - 1;
    const int32_t c0 = __shfl(c, first);
    const bool one = combine && __ballot(on && c != c0) == 0;
    if (one) {
        long long sum[3];
        int lo[3], hi[3];
        for (int a = 0; a < 3; ++a) {
            sum[a] = wave_reduce((long long)(on ? at[a] : 0), [](long long x, long long y) { return x + y; });
            lo[a] = wave_reduce(on ? at[a] : INT_MAX, [](int x, int y) { return x < y ? x : y; });
            hi[a] = wave_reduce(on ? at[a] : -1, [](int x, int y) { return x > y ? x : y; });
        }
        const bool any_border = __ballot(border) != 0;
        if ((int)(threadIdx.x & (PF_WAVE - 1)) == first) ccl_send(s, c0, (u64)__popcll(members), sum, lo, hi, any_border);
    } else if (on) {
        const long long sum[3] = {at[0], at[1], at[2]};
        ccl_send(s, c, 1, sum, at, at, border);
    }
}

__global__ __launch_bounds__(PF_BLOCK) void k_ccl_largest(const u64* __restrict__ count, int64_t C, u64* __restrict__ largest) {
    const int64_t c = (int64_t)blockIdx.x * PF_BLOCK + threadIdx.x;
    const long long m = wave_reduce((long long)(c < C ? count[c] : 0), [](long long x, long long y) { return x > y ? x : y; });
    if ((threadIdx.x & (PF_WAVE - 1)) == 0 && m) atomicMax(largest, (u64)m);
}

__global__ __launch_bounds__(PF_BLOCK) void k_ccl_select(const int32_t* __restrict__ component, int64_t n, const uint8_t* __restrict__ keep,
                                                         uint8_t* __restrict__ out) {
    const int64_t p = (int64_t)blockIdx.x * PF_BLOCK + threadIdx.x;
    if (p >= n) return;
    const int32_t c = component[p];
    out[p] = c > 0 && keep[c - 1] ? 1 : 0;
}

CclLines ccl_lines(int32_t connectivity) {
    CclLines l;
    const int di[4] = {-1, 0, -1, -1}, dj[4] = {0, -1, -1, 1};
    l.n = connectivity == 6 ? 2 : 4;
    for (int t = 0; t < 4; ++t) {
        l.di[t] = di[t], l.dj[t] = dj[t];
        // 6: the same k only; 18: +-1 in z next to one other axis; 26: everywhere
        l.reach[t] = connectivity == 26 || (connectivity == 18 && t < 2) ? 1 : 0;
    }
    return l;
}

}  // namespace

extern "C" {

int pf_ccl_combine_stats(int on) {
    g_ccl_combine.store(on ? 1 : 0);
    return PF_OK;
}

void pf_ccl_free(pf_ccl* h) {
    if (!h) return;
    (void)hipSetDevice(h->ctx->device);
    (void)hipStreamSynchronize(h->ctx->stream);
    hipStream_t st = h->ctx->stream;
    pf_free(st, h->component);
    pf_free(st, h->count);
    pf_free(st, h->value);
    pf_free(st, h->root);
    pf_free(st, h->lo);
    pf_free(st, h->hi);
    pf_free(st, h->border);
    pf_free(st, h->sum);
    delete h;
}

int pf_ccl_create(pf_ctx* ctx, const int32_t* vol, int64_t nx, int64_t ny, int64_t nz, int32_t connectivity, int32_t mode, uint32_t flags,
                  pf_ccl** out, int64_t* report, double* device_ms) {
    PF_CHECK(ctx && vol && out, PF_E_ARG, "pf_ccl_create: NULL argument");
    PF_CHECK(flags == 0, PF_E_ARG, "pf_ccl_create: unknown flags 0x%x", flags);
    PF_CHECK(mode == PF_CCL_BINARY || mode == PF_CCL_BY_VALUE || mode == PF_CCL_BACKGROUND, PF_E_ARG, "pf_ccl_create: unknown mode %d", mode);
    PF_CHECK(connectivity == 6 || connectivity == 18 || connectivity == 26, PF_E_ARG, "pf_ccl_create: connectivity %d is not 6, 18 or 26",
             connectivity);
    const int64_t lim = (int64_t)1 << 31;
    PF_CHECK(nx >= 1 && ny >= 1 && nz >= 1 && nx < lim && ny < lim && nz < lim, PF_E_ARG,
             "pf_ccl_create: extents %lld x %lld x %lld out of range (each 1..2^31-1)", (long long)nx, (long long)ny, (long long)nz);
    PF_CHECK(nx * ny < lim && nx * ny * nz < lim, PF_E_ARG, "pf_ccl_create: %lld x %lld x %lld samples out of range (< 2^31)",
             (long long)nx, (long long)ny, (long long)nz);
    const int64_t N = nx * ny * nz;
    CclGrid g;
    g.nx = nx, g.ny = ny, g.nz = nz, g.words = (nz + 63) / 64;
    const int64_t n_words = nx * ny * g.words;
    const CclLines lines = ccl_lines(connectivity);
    const int combine = g_ccl_combine.load();
    PF_HIP(hipSetDevice(ctx->device));
    hipStream_t st = ctx->stream;
    StreamTimer timer(device_ms != nullptr);
    u64 counters[4] = {0, 0, 0, 0};  // labelled voxels | retries | largest count | -
    int32_t n_components = 0;
    pf_ccl* h = new pf_ccl();
    h->ctx = ctx, h->nx = nx, h->ny = ny, h->nz = nz;
    hipError_t err;
    {
        Scratch sc(st);
        int32_t* d_vol = sc.get<int32_t>(N);
        u64 *fg = sc.get<u64>(n_words), *start = sc.get<u64>(n_words);
        int32_t *parent = sc.get<int32_t>(N), *rank = sc.get<int32_t>(N + 1);
        u64* d_counters = sc.get<u64>(4);
        h->component = sc.keep<int32_t>(N + 1);
        sc.upload(d_vol, vol, N);
        sc.zero(d_counters, sizeof(counters));
        timer.start(sc);
        if (sc.ok()) {
            k_ccl_pack<<<(unsigned)((n_words + CCL_LINE - 1) / CCL_LINE), PF_BLOCK, 0, st>>>(d_vol, g, mode, fg, start, d_counters);
            k_ccl_runs<<<pf_blocks(N), PF_BLOCK, 0, st>>>(fg, start, g, parent);
            k_ccl_hook<<<pf_blocks(n_words), PF_BLOCK, 0, st>>>(d_vol, fg, start, g, mode == PF_CCL_BY_VALUE, lines, parent, d_counters + 1);
            k_ccl_compress<<<pf_blocks(N + 1), PF_BLOCK, 0, st>>>(parent, N, h->component);
            sc.launched();
        }
        if (sc.ok() && pf_exclusive_scan_i32(st, h->component, rank, N + 1) != PF_OK) sc.note(hipErrorUnknown);
        sc.download(&n_components, rank + N, 1);  // the one read-back before the tables are sized
        sc.sync();
        const int64_t C = h->C = n_components;
        CclTables s = {nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr};
        if (C > 0) {
            s.count = (u64*)(h->count = sc.keep<int64_t>(C));
            s.value = h->value = sc.keep<int32_t>(C);
            s.root = h->root = sc.keep<int32_t>(C);
            s.lo = h->lo = sc.keep<int32_t>(3 * C);
            s.hi = h->hi = sc.keep<int32_t>(3 * C);
            s.border = h->border = sc.keep<uint8_t>(C);
            s.sum = (u64*)(h->sum = sc.keep<int64_t>(3 * C));
        }
        if (sc.ok()) {
            if (C > 0) k_ccl_tables_init<<<pf_blocks(C), PF_BLOCK, 0, st>>>(s, C);
            k_ccl_number<<<pf_blocks(N), PF_BLOCK, 0, st>>>(parent, rank, d_vol, g, mode, combine, h->component, s);
            if (C > 0) k_ccl_largest<<<pf_blocks(C), PF_BLOCK, 0, st>>>(s.count, C, d_counters + 2);
            sc.launched();
        }
        timer.stop(sc);
        sc.download(counters, d_counters, 4);
        sc.sync();
        timer.read(sc, device_ms);
        err = sc.err;
    }
    if (err != hipSuccess) {
        pf_ccl_free(h);
        return pf_hip_failed("pf_ccl_create", err);
    }
    if (report) {
        report[0] = N, report[1] = (int64_t)counters[0], report[2] = h->C, report[3] = (int64_t)counters[1];
        report[4] = (int64_t)counters[2], report[5] = report[6] = report[7] = 0;
    }
    *out = h;
    return PF_OK;
}

int pf_ccl_info(const pf_ccl* h, int64_t* n_components) {
    PF_CHECK(h && n_components, PF_E_ARG, "pf_ccl_info: NULL argument");
    *n_components = h->C;
    return PF_OK;
}

int pf_ccl_fetch(pf_ccl* h, int32_t* component, int64_t* count, int32_t* value, int32_t* root, int32_t* lo, int32_t* hi, uint8_t* border,
                 int64_t* sum) {
    PF_CHECK(h != nullptr, PF_E_ARG, "pf_ccl_fetch: NULL handle");
    PF_HIP(hipSetDevice(h->ctx->device));
    const int64_t N = h->nx * h->ny * h->nz, C = h->C;
    Scratch sc(h->ctx->stream);
    sc.download(component, h->component, N);
    if (C > 0) {
        sc.download(count, h->count, C);
        sc.download(value, h->value, C);
        sc.download(root, h->root, C);
        sc.download(lo, h->lo, 3 * C);
        sc.download(hi, h->hi, 3 * C);
        sc.download(border, h->border, C);
        sc.download(sum, h->sum, 3 * C);
    }
    sc.sync();
    return sc.ok() ? PF_OK : pf_hip_failed("pf_ccl_fetch", sc.err);
}

int pf_ccl_select(pf_ccl* h, const uint8_t* keep, uint8_t* out) {
    PF_CHECK(h && out && (keep || h->C == 0), PF_E_ARG, "pf_ccl_select: NULL argument");
    PF_HIP(hipSetDevice(h->ctx->device));
    const int64_t N = h->nx * h->ny * h->nz, C = h->C;
    hipStream_t st = h->ctx->stream;
    Scratch sc(st);
    uint8_t *d_keep = sc.get<uint8_t>(C), *d_out = sc.get<uint8_t>(N);
    if (C > 0) sc.upload(d_keep, keep, C);
    if (sc.ok()) {
        k_ccl_select<<<pf_blocks(N), PF_BLOCK, 0, st>>>(h->component, N, d_keep, d_out);
        sc.launched();
    }
    sc.download(out, d_out, N);
    sc.sync();
    return sc.ok() ? PF_OK : pf_hip_failed("pf_ccl_select", sc.err);
}

}  // extern "C"
