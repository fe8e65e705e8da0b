// The failure paths of Scratch, DevBuf and StreamTimer (pyfocusr_amd/csrc/pf_scratch.h), run on the CPU.
//
// On a GPU an allocation only fails when the device is out of memory, so no GPU test can walk these paths.  Here the
// header is compiled by the host compiler over a test double of the library's allocator: pf_malloc / pf_free are backed
// by the heap, count the blocks that are live, and fail on the n-th call; the four HIP calls the header makes are trivial
// stand-ins over host memory.  No HIP runtime is linked.  For n = 0 .. (number of allocations) a call-shaped sequence
// runs - several get, one keep, a DevBuf grown twice - with the n-th allocation failing (the last n: none fails), and the
// program checks what the callers of the library rely on:
//   * the first error is the one the call reports, whatever is noted after it;
//   * every request after it is a no-op that returns NULL: no allocation, no copy, no wait;
//   * when the call's scope ends every get block has been freed exactly once and the keep block is still live;
//   * a DevBuf whose grow failed is empty, and can be grown or released again;
//   * blocks released in the middle of a call (release_from) are freed once, and only they.
// StreamTimer runs over stand-ins of the four event calls - an event is a heap block, so the sanitizer sees one destroyed
// twice, used after it, or never destroyed - with the n-th hipEventCreate failing, wanted and not wanted, through start,
// stop and read and through every early end of a call: each event created is destroyed exactly once, the failure is the
// call's error, and a timer that is not wanted makes no event call at all.
// HostLanding runs over stand-ins of hipHostMalloc / hipHostFree (heap blocks of exactly the size asked for) and of
// hipEventCreateWithFlags, each failing on the n-th call, against a HostPools of its own: a pooled block of cap >= need
// is taken and leaves the pool, a smaller one is skipped; a block that is large enough is kept without any call; a grow
// returns the old block to the pool exactly once, and only after the drain where the caller named a stream; after a
// failed ensure - no block, no event, a failed grow - the landing is empty and may be ensured or released again; release
// twice is harmless; and after every step each live block and each live event is held exactly once, by a landing or by a
// pool, until the teardown frees each of them once.
// Built with -fsanitize=address,undefined (tests/test_scratch_paths.py): a block freed twice, used after its release or
// overrun by a copy stops the program there.  Exit status 0 and "ok" on the last line: every check held.
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <map>

#include "../../pyfocusr_amd/csrc/pf_scratch.h"

namespace {

int g_failures = 0;
#define CHECK(cond)                                                               \
    do {                                                                          \
        if (!(cond)) {                                                            \
            printf("FAILED (fail_at %d) %s:%d: %s\n", g_fail_at, __FILE__, __LINE__, #cond); \
            ++g_failures;                                                         \
        }                                                                         \
    } while (0)

// ---- the allocator's test double
int g_fail_at = -1;      // the pf_malloc call (counted from 0) that fails; -1: none
int g_malloc_calls = 0;
int g_bad_frees = 0;     // pf_free of a block that is not live: freed twice, or never ours
int g_hip_calls = 0;     // copies, memsets and waits that reached the stand-ins
std::map<void*, size_t> g_live;
const hipStream_t ST = reinterpret_cast<hipStream_t>(0x10);
const hipError_t ALLOC_ERROR = hipErrorOutOfMemory;

void reset(int fail_at) {
    g_fail_at = fail_at;
    g_malloc_calls = g_bad_frees = g_hip_calls = 0;
}

}  // namespace

hipError_t pf_malloc(hipStream_t st, void** p, size_t bytes) {
    *p = nullptr;
    if (st != ST) return hipErrorInvalidValue;
    if (g_malloc_calls++ == g_fail_at) return ALLOC_ERROR;
    *p = malloc(bytes ? bytes : 1);  // exactly what was asked for: the sanitizer sees any overrun
    g_live[*p] = bytes;
    return hipSuccess;
}

void pf_free(hipStream_t, void* p) {
    if (!p) return;
    const auto it = g_live.find(p);
    if (it == g_live.end()) {
        ++g_bad_frees;
        return;
    }
    g_live.erase(it);
    free(p);
}

// ---- the HIP calls of the header, over host memory
extern "C" {
hipError_t hipMemcpyAsync(void* dst, const void* src, size_t bytes, hipMemcpyKind, hipStream_t) {
    ++g_hip_calls;
    memcpy(dst, src, bytes);
    return hipSuccess;
}
hipError_t hipMemsetAsync(void* dst, int value, size_t bytes, hipStream_t) {
    ++g_hip_calls;
    memset(dst, value, bytes);
    return hipSuccess;
}
void (*g_on_sync)() = nullptr;  // what a sequence wants looked at while the stream is being drained
hipError_t hipStreamSynchronize(hipStream_t) {
    ++g_hip_calls;
    if (g_on_sync) g_on_sync();
    return hipSuccess;
}
hipError_t hipGetLastError(void) { return hipSuccess; }
}

// ---- the event calls of StreamTimer: an event is a heap block of one int
namespace {
int g_event_fail_at = -1;  // the hipEventCreate call (counted from 0) that fails; -1: none
int g_event_creates = 0, g_event_calls = 0, g_event_bad = 0;  // bad: a destroy, record or read of an event that is not live
std::map<void*, int> g_events;  // live event -> times recorded
const hipError_t EVENT_ERROR = hipErrorInvalidResourceHandle;
}  // namespace

extern "C" {
hipError_t hipEventCreate(hipEvent_t* e) {
    ++g_event_calls;
    if (g_event_creates++ == g_event_fail_at) return EVENT_ERROR;
    *e = reinterpret_cast<hipEvent_t>(malloc(sizeof(int)));
    g_events[*e] = 0;
    return hipSuccess;
}
hipError_t hipEventCreateWithFlags(hipEvent_t* e, unsigned) { return hipEventCreate(e); }
hipError_t hipEventDestroy(hipEvent_t e) {
    ++g_event_calls;
    if (g_events.erase(e) != 1) {
        ++g_event_bad;
        return hipErrorInvalidResourceHandle;
    }
    free(e);
    return hipSuccess;
}
hipError_t hipEventRecord(hipEvent_t e, hipStream_t) {
    ++g_event_calls;
    const auto it = g_events.find(e);
    if (it == g_events.end()) {
        ++g_event_bad;
        return hipErrorInvalidResourceHandle;
    }
    *reinterpret_cast<int*>(e) = ++it->second;
    return hipSuccess;
}
hipError_t hipEventElapsedTime(float* ms, hipEvent_t a, hipEvent_t b) {
    ++g_event_calls;
    if (g_events.count(a) != 1 || g_events.count(b) != 1 || g_events[a] != 1 || g_events[b] != 1) {
        ++g_event_bad;
        return hipErrorInvalidResourceHandle;
    }
    *ms = 1.5f;
    return hipSuccess;
}
}

// ---- the pinned allocation of HostLanding: heap blocks of exactly the size asked for
namespace {
int g_host_fail_at = -1;  // the hipHostMalloc call (counted from 0) that fails; -1: none
int g_host_calls = 0, g_host_bad = 0;  // bad: a hipHostFree of a block that is not live
std::map<void*, size_t> g_pinned;
const hipError_t HOST_ERROR = hipErrorOutOfMemory;
}  // namespace

extern "C" {
hipError_t hipHostMalloc(void** p, size_t bytes, unsigned) {
    *p = nullptr;
    if (g_host_calls++ == g_host_fail_at) return HOST_ERROR;
    *p = malloc(bytes);
    g_pinned[*p] = bytes;
    return hipSuccess;
}
hipError_t hipHostFree(void* p) {
    if (g_pinned.erase(p) != 1) {
        ++g_host_bad;
        return hipErrorInvalidValue;
    }
    free(p);
    return hipSuccess;
}
}

namespace {

constexpr int N_ALLOC = 6;  // allocations of one call: get, get, keep, get, grow, grow
constexpr size_t N = 100;

// One call of the library in miniature.  buf holds 8 elements on entry (a block that the first grow has to replace).
hipError_t call(DevBuf<double>& buf, double** kept) {
    const int before = g_malloc_calls;
    double h_in[N], h_out[N];
    for (size_t i = 0; i < N; ++i) h_in[i] = (double)i, h_out[i] = -1.0;
    void* blocks[3] = {nullptr, nullptr, nullptr};
    {
        Scratch s(ST);
        double* a = s.get<double>(N);
        int32_t* b = s.get<int32_t>(0);  // nothing asked for: served like one byte, freed like any block
        double* k = *kept = s.keep<double>(N);
        char* c = s.get<char>(77);
        blocks[0] = a, blocks[1] = b, blocks[2] = c;
        const int failed = g_fail_at >= 0 && g_fail_at < 4 ? g_fail_at : -1;  // among the scratch's four
        void* const got[4] = {a, b, k, c};
        for (int i = 0; i < 4; ++i) CHECK((got[i] != nullptr) == (failed < 0 || i < failed));  // NULL from the failure on
        CHECK(s.ok() == (failed < 0));
        CHECK(g_malloc_calls - before == (failed < 0 ? 4 : failed + 1));  // nothing was asked of the allocator after it
        CHECK(s.blocks.size() == (size_t)(failed < 0 ? 3 : (failed < 3 ? failed : 2)));
        if (failed < 0) CHECK(s.bytes == sizeof(double) * N + 0 + sizeof(double) * N + 77);
        const int hip_before = g_hip_calls;
        s.upload(a, h_in, N);
        s.zero(c, 77);
        s.launched();
        CHECK((g_hip_calls - hip_before) == (failed < 0 ? 2 : 0));  // no copy and no memset into a NULL block
        // the grow-only buffer, as a call uses it: PF_HIP(buf.grow(..)) - the call ends at the first failure
        if (s.ok()) {
            double* const old = buf.p;
            s.note(buf.grow(ST, 4));  // fits: no allocation, the block stays
            CHECK(s.ok() && buf.p == old && buf.cap == 8);
        }
        if (s.ok()) s.note(buf.grow(ST, 50));
        if (s.ok()) {
            CHECK(buf.p != nullptr && buf.cap == 50);
            buf.p[49] = 1.0;
            s.note(buf.grow(ST, 500));
            if (s.ok()) {
                CHECK(buf.p != nullptr && buf.cap == 500);
                buf.p[499] = 1.0;
            }
        }
        if (!s.ok() && failed < 0) CHECK(buf.p == nullptr && buf.cap == 0);  // a failed grow leaves the buffer empty
        const hipError_t first = s.err;
        if (!s.ok()) s.note(hipErrorUnknown);  // a later error does not replace the first
        CHECK(s.err == first);
        CHECK(first == (g_fail_at >= 0 && g_fail_at < N_ALLOC ? ALLOC_ERROR : hipSuccess));
        const int hip_late = g_hip_calls, malloc_late = g_malloc_calls;
        s.download(h_out, a, N);
        s.sync();
        if (s.ok()) {
            CHECK(g_hip_calls - hip_late == 2);
            CHECK(memcmp(h_in, h_out, sizeof(h_in)) == 0);
        } else {
            CHECK(g_hip_calls == hip_late);  // no read-back and no wait after a failure
            CHECK(s.get<double>(N) == nullptr && s.keep<char>(1) == nullptr && g_malloc_calls == malloc_late);
        }
        for (void* p : blocks) CHECK(p == nullptr || g_live.count(p) == 1);  // still the call's until its scope ends
        if (s.ok()) {  // a round's temporaries go back in the middle of the call: they, and nothing else
            g_fail_at = -1;  // (this is the sequence in which no allocation fails)
            const size_t mark = s.blocks.size(), live = g_live.size();
            char *t0 = s.get<char>(10), *t1 = s.get<char>(20);
            CHECK(t0 && t1 && g_live.size() == live + 2);
            s.release_from(mark);
            CHECK(s.blocks.size() == mark && g_live.size() == live && g_live.count(t0) == 0 && g_live.count(t1) == 0);
            s.release_from(mark);  // nothing left to release
            CHECK(g_bad_frees == 0 && g_live.count(a) == 1);
        }
        if (!s.ok()) return s.err;  // (the early return of PF_HIP: the scope ends here as well)
    }
    return hipSuccess;
}

void run(int fail_at) {
    DevBuf<double> buf;
    reset(-1);
    CHECK(buf.grow(ST, 8) == hipSuccess && buf.cap == 8);
    const size_t live_before = g_live.size();  // buf's block
    double* kept = nullptr;
    reset(fail_at);
    const hipError_t e = call(buf, &kept);
    const bool fails = fail_at >= 0 && fail_at < N_ALLOC;
    CHECK(e == (fails ? ALLOC_ERROR : hipSuccess));
    CHECK(g_bad_frees == 0);  // no block was freed twice
    // what is live now: the keep block if it was served, and buf's block unless its grow failed - every get block is gone
    const bool kept_live = !fails || fail_at > 2;
    const bool buf_live = !fails || fail_at < 4;
    CHECK((kept != nullptr) == kept_live);
    CHECK(kept == nullptr || g_live.count(kept) == 1);
    CHECK((buf.p != nullptr) == buf_live && (buf.cap != 0) == buf_live);
    CHECK(buf.p == nullptr || g_live.count(buf.p) == 1);
    CHECK(g_live.size() == live_before - 1 + (kept_live ? 1 : 0) + (buf_live ? 1 : 0));
    if (kept) kept[N - 1] = 1.0;  // the keep block is the caller's to use ...
    pf_free(ST, kept);            // ... and to free
    // the buffer after a failed grow: growing works again, releasing is safe, and so is releasing twice
    reset(-1);
    CHECK(buf.grow(ST, 20) == hipSuccess && buf.p != nullptr && buf.cap >= 20);
    buf.p[19] = 2.0;
    buf.release(ST);
    CHECK(buf.p == nullptr && buf.cap == 0);
    buf.release(ST);
    CHECK(g_bad_frees == 0 && g_live.empty());
    // a grow that fails on a buffer that holds nothing
    reset(0);
    CHECK(buf.grow(ST, 5) == ALLOC_ERROR && buf.p == nullptr && buf.cap == 0);
    buf.release(ST);
    CHECK(g_bad_frees == 0 && g_live.empty());
}

// One timed call in miniature: stop_early leaves before stop (a kernel failed), or before read.
void timed(bool wanted, int event_fail_at, int stop_early) {
    g_fail_at = -1;
    g_event_fail_at = event_fail_at;
    g_event_creates = g_event_calls = g_event_bad = 0;
    double ms = -1.0;
    hipError_t err;
    {
        StreamTimer timer(wanted);
        {
            Scratch s(ST);
            timer.start(s);
            const bool failed = wanted && event_fail_at >= 0 && event_fail_at < 2;
            CHECK(s.ok() == !failed);
            CHECK(g_events.size() == (size_t)(!wanted ? 0 : (failed ? event_fail_at : 2)));  // nothing is created after a failure
            if (stop_early == 1) s.note(hipErrorLaunchFailure);
            timer.stop(s);
            if (stop_early == 2) s.note(hipErrorLaunchFailure);
            s.sync();
            timer.read(s, &ms);
            CHECK((ms == 1.5) == (wanted && !failed && !stop_early));
            CHECK(ms == 1.5 || ms == -1.0);  // not written unless it was measured
            err = s.err;
            CHECK(err == (failed ? EVENT_ERROR : (stop_early ? hipErrorLaunchFailure : hipSuccess)));
        }
    }
    CHECK(g_events.empty());    // every event that was created has been destroyed ...
    for (auto& kv : g_events) free(kv.first);  // (a leaked event is this sequence's failed check, not the next one's too)
    g_events.clear();
    CHECK(g_event_bad == 0);    // ... once, and none was touched that was not live
    if (!wanted) CHECK(g_event_calls == 0);
}

// ---- HostLanding over a HostPools of the sequence's own
// every live block and every live event is held exactly once: by one of the landings, or by a pool
void held_once(const HostPools& pools, const HostLanding* const* ls, int n) {
    std::map<const void*, int> blocks, events;
    for (auto& pb : pools.pinned_pool) ++blocks[pb.second];
    for (hipEvent_t e : pools.event_pool) ++events[e];
    for (int i = 0; i < n; ++i) {
        CHECK((ls[i]->host != nullptr) == (ls[i]->ev != nullptr));  // both or neither
        CHECK((ls[i]->host != nullptr) == (ls[i]->cap != 0));
        if (ls[i]->host) ++blocks[ls[i]->host];
        if (ls[i]->ev) ++events[ls[i]->ev];
    }
    CHECK(blocks.size() == g_pinned.size() && events.size() == g_events.size());  // none leaked, none invented
    for (auto& kv : blocks) CHECK(kv.second == 1 && g_pinned.count(const_cast<void*>(kv.first)) == 1);
    for (auto& kv : events) CHECK(kv.second == 1 && g_events.count(const_cast<void*>(kv.first)) == 1);
    for (auto& pb : pools.pinned_pool) CHECK(g_pinned[pb.second] == sizeof(double) * (size_t)(pb.first + 2));
}

int in_pool(const HostPools& pools, const double* p) {
    int n = 0;
    for (auto& pb : pools.pinned_pool) n += pb.second == p;
    return n;
}

// pf_destroy in miniature: what the pools hold goes back to the runtime, each once
void teardown(HostPools& pools) {
    for (auto& pb : pools.pinned_pool) (void)hipHostFree(pb.second);
    for (hipEvent_t e : pools.event_pool) (void)hipEventDestroy(e);
    pools.pinned_pool.clear();
    pools.event_pool.clear();
    CHECK(g_pinned.empty() && g_events.empty() && g_host_bad == 0 && g_event_bad == 0);
    for (auto& kv : g_pinned) free(kv.first);  // (a leak is this sequence's failed check, not the next one's too)
    for (auto& kv : g_events) free(kv.first);
    g_pinned.clear();
    g_events.clear();
}

void landing_reset(int host_fail_at, int event_fail_at) {
    g_host_fail_at = host_fail_at, g_event_fail_at = event_fail_at;
    g_host_calls = g_host_bad = g_event_creates = g_event_calls = g_event_bad = g_hip_calls = 0;
    g_on_sync = nullptr;
}

const HostPools* g_watch_pools = nullptr;  // while the stream is drained, this block is not in this pool yet
const double* g_watch_block = nullptr;
int g_early_returns = 0;

void landings_take_grow_release() {
    landing_reset(-1, -1);
    HostPools pools;
    HostLanding a, b, c, d, e;
    const HostLanding* const all[5] = {&a, &b, &c, &d, &e};
    // nothing held, nothing pooled: a new block of the floor, with its two spare doubles, and a new event; no drain
    CHECK(a.ensure(pools, 10, 64, ST) == hipSuccess && a.host && a.cap == 64 && a.ev);
    a.host[65] = 1.0;
    CHECK(g_host_calls == 1 && g_event_creates == 1 && g_hip_calls == 0);
    held_once(pools, all, 5);
    // large enough: kept as it is, no call of any kind
    const double* const first = a.host;
    const hipEvent_t first_ev = a.ev;
    CHECK(a.ensure(pools, 64, 64, ST) == hipSuccess && a.host == first && a.cap == 64 && a.ev == first_ev);
    CHECK(g_host_calls == 1 && g_event_creates == 1 && g_hip_calls == 0);
    // outgrown: back to the pool once, and only after the stream the caller named has been drained; the event stays
    g_watch_pools = &pools, g_watch_block = first, g_early_returns = 0;
    g_on_sync = [] { g_early_returns += in_pool(*g_watch_pools, g_watch_block); };
    CHECK(a.ensure(pools, 65, 64, ST) == hipSuccess && a.host && a.host != first && a.cap == 65 && a.ev == first_ev);
    g_on_sync = nullptr;
    CHECK(g_hip_calls == 1 && g_early_returns == 0 && in_pool(pools, first) == 1 && g_host_calls == 2 && g_event_creates == 1);
    a.host[66] = 1.0;
    held_once(pools, all, 5);
    // the pooled block of 64 is too small for 200 (and for a floor of 128): skipped, it stays in the pool
    CHECK(b.ensure(pools, 200, 128, nullptr) == hipSuccess && b.cap == 200 && in_pool(pools, first) == 1 && g_host_calls == 3);
    CHECK(c.ensure(pools, 10, 128, nullptr) == hipSuccess && c.cap == 128 && in_pool(pools, first) == 1 && g_host_calls == 4);
    // cap >= need and no floor: taken, and it leaves the pool; `fresh` only sizes a new block
    CHECK(d.ensure(pools, 10, 0, nullptr, 384) == hipSuccess && d.host == first && d.cap == 64 && pools.pinned_pool.empty());
    CHECK(e.ensure(pools, 10, 0, nullptr, 384) == hipSuccess && e.cap == 384 && g_host_calls == 5);
    e.host[385] = 1.0;
    CHECK(g_hip_calls == 1);  // no drain where no stream was named, or nothing was held
    held_once(pools, all, 5);
    // a grow without a drain (the finaliser's): the old block is pooled all the same
    const double* const d_old = d.host;
    CHECK(d.ensure(pools, 100, 0, nullptr, 384) == hipSuccess && d.cap == 384 && in_pool(pools, d_old) == 1 && g_hip_calls == 1);
    held_once(pools, all, 5);
    // release gives both back; twice is harmless; the next landing is served from the pools without a call
    const double* const a_old = a.host;
    a.release(pools);
    CHECK(!a.host && !a.ev && a.cap == 0 && in_pool(pools, a_old) == 1 && pools.event_pool.size() == 1);
    a.release(pools);
    CHECK(in_pool(pools, a_old) == 1 && pools.event_pool.size() == 1);
    held_once(pools, all, 5);
    const int host_calls = g_host_calls, creates = g_event_creates;
    CHECK(a.ensure(pools, 65, 64, ST) == hipSuccess && a.host == a_old && a.ev == first_ev && pools.event_pool.empty());
    CHECK(g_host_calls == host_calls && g_event_creates == creates && g_hip_calls == 1);
    held_once(pools, all, 5);
    for (HostLanding* l : {&a, &b, &c, &d, &e}) l->release(pools);
    held_once(pools, all, 5);
    CHECK(pools.pinned_pool.size() == g_pinned.size() && g_pinned.size() == 6 && pools.event_pool.size() == 5);
    teardown(pools);
}

// which: 0 no pinned block to be had, 1 no event to be had, 2 a grow that finds no block
void landing_fails(int which) {
    landing_reset(-1, -1);
    HostPools pools;
    HostLanding a;
    const HostLanding* const all[1] = {&a};
    if (which == 2) {
        CHECK(a.ensure(pools, 10, 64, ST) == hipSuccess);
        g_host_fail_at = g_host_calls;
    } else if (which == 0) {
        g_host_fail_at = 0;
    } else {
        g_event_fail_at = 0;
    }
    const double* const old = a.host;
    const hipError_t err = a.ensure(pools, 100, 64, ST);
    CHECK(err == (which == 1 ? EVENT_ERROR : HOST_ERROR));
    CHECK(!a.host && !a.ev && a.cap == 0);  // empty: no stale pointer to the block that went back
    if (which == 2) CHECK(in_pool(pools, old) == 1 && pools.event_pool.size() == 1);  // ... once, and its event with it
    if (which == 1) CHECK(pools.pinned_pool.size() == 1 && pools.pinned_pool[0].first == 100);  // the block that had no event
    held_once(pools, all, 1);
    a.release(pools);  // safe, also twice
    a.release(pools);
    held_once(pools, all, 1);
    g_host_fail_at = g_event_fail_at = -1;
    CHECK(a.ensure(pools, 100, 64, ST) == hipSuccess && a.host && a.cap >= 100 && a.ev);  // and it can be ensured again
    a.host[a.cap + 1] = 1.0;
    held_once(pools, all, 1);
    a.release(pools);
    teardown(pools);
}

}  // namespace

int main() {
    for (int fail_at = 0; fail_at <= N_ALLOC; ++fail_at) run(fail_at);
    g_fail_at = -1;
    for (int wanted = 0; wanted < 2; ++wanted)
        for (int event_fail_at = -1; event_fail_at < 2; ++event_fail_at)
            for (int stop_early = 0; stop_early < 3; ++stop_early) timed(wanted != 0, event_fail_at, stop_early);
    landings_take_grow_release();
    for (int which = 0; which < 3; ++which) landing_fails(which);
    for (auto& kv : g_live) free(kv.first);
    printf("%d sequences, %d checks failed\n", N_ALLOC + 1, g_failures);
    if (g_failures) return 1;
    printf("ok\n");
    return 0;
}
