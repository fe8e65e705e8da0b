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
hipError_t hipStreamSynchronize(hipStream_t) {
    ++g_hip_calls;
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

}  // namespace

int main() {
    for (int fail_at = 0; fail_at <= N_ALLOC; ++fail_at) run(fail_at);
    g_fail_at = -1;
    for (int wanted = 0; wanted < 2; ++wanted)
        for (int event_fail_at = -1; event_fail_at < 2; ++event_fail_at)
            for (int stop_early = 0; stop_early < 3; ++stop_early) timed(wanted != 0, event_fail_at, stop_early);
    for (auto& kv : g_live) free(kv.first);
    printf("%d sequences, %d checks failed\n", N_ALLOC + 1, g_failures);
    if (g_failures) return 1;
    printf("ok\n");
    return 0;
}
