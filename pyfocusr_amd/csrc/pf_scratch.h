// Device memory as the host code of the library holds it: the scratch of one call (Scratch) and a buffer that grows and
// stays (DevBuf), both on top of the ctx's caching allocator (pf_api.hip); the timer of a call's stream work
// (StreamTimer); and the pinned host block with its event that a few results land in (HostLanding, over the ctx's
// HostPools).  Only the HIP C API is needed here, so the failure paths of all four run on the CPU over test doubles of
// the allocator, of the pinned allocation and of the event calls (tests/csrc/scratch_paths.cpp).
#pragma once
#include <hip/hip_runtime_api.h>
#include <stddef.h>
#include <stdint.h>
#include <algorithm>
#include <utility>
#include <vector>

// Caching device allocator, one cache per ctx (pf_api.hip).  Every use of a block is enqueued on
// the ctx's single stream, so a block released at enqueue time can be handed out again at once:
// later work is ordered behind earlier work by the stream.  After the first build the assembler's
// ~30 temporaries are recycled without a driver call (hipMalloc/hipFree cost 0.1-1 ms each and
// hipFree synchronises the device).  Blocks go back to the driver in pf_destroy.  A request of 0 bytes is served like
// one of 1; *p is NULL after a failure; pf_free(NULL) does nothing.
hipError_t pf_malloc(hipStream_t st, void** p, size_t bytes);
void pf_free(hipStream_t st, void* p);

// The device side of one call: scratch blocks from the ctx's cache, all given back when the call's scope ends (after
// whatever synchronise the call made: as late as the blocks can matter), and the stream work itself.  The first failure is
// kept in err and turns everything that follows into a no-op, so a call is written without branches: ok() before its
// kernels, err at the end.
struct Scratch {
    const hipStream_t st;
    hipError_t err = hipSuccess;
    std::vector<void*> blocks;
    size_t bytes = 0;  // sum of the sizes asked for and served, get and keep alike

    explicit Scratch(hipStream_t stream) : st(stream) {}
    Scratch(const Scratch&) = delete;
    Scratch& operator=(const Scratch&) = delete;
    ~Scratch() {
        for (void* p : blocks) pf_free(st, p);
    }
    bool ok() const { return err == hipSuccess; }
    void note(hipError_t e) {
        if (ok()) err = e;
    }
    template <class T>
    T* keep(size_t count) {  // a block that outlives the call: the caller owns it, also after a failure
        void* p = nullptr;
        if (ok()) {
            err = pf_malloc(st, &p, sizeof(T) * count);
            if (ok()) bytes += sizeof(T) * count;
        }
        return (T*)p;
    }
    template <class T>
    T* get(size_t count) {
        T* p = keep<T>(count);
        if (p) blocks.push_back(p);
        return p;
    }
    template <class T>
    void upload(T* dst, const T* src, size_t count) {
        if (ok()) err = hipMemcpyAsync(dst, src, sizeof(T) * count, hipMemcpyHostToDevice, st);
    }
    template <class T>
    void download(T* dst, const T* src, size_t count) {  // dst == NULL: the caller did not ask for it
        if (ok() && dst) err = hipMemcpyAsync(dst, src, sizeof(T) * count, hipMemcpyDeviceToHost, st);
    }
    void zero(void* p, size_t bytes_) {
        if (ok()) err = hipMemsetAsync(p, 0, bytes_, st);
    }
    void launched() { note(hipGetLastError()); }  // after the kernels of an ok() block
    void sync() {
        if (ok()) err = hipStreamSynchronize(st);
    }
    // the blocks got since blocks.size() was `mark` go back now (the stream orders their next user behind the work queued
    // so far): for a loop whose every round gets temporaries of its own
    void release_from(size_t mark) {
        for (; blocks.size() > mark; blocks.pop_back()) pf_free(st, blocks.back());
    }
};

// The device time of a call's stream work, for the entry points that report it (device_ms): two events around the work.
// Constructed with whether the caller wants the time - if not, nothing below does anything.  start creates the events
// and records the first, stop records the second, read (after the call's sync) gives the milliseconds between them;
// a failure is the Scratch's like any other.  The destructor destroys whatever was created.
struct StreamTimer {
    const bool wanted;
    hipEvent_t ev[2] = {nullptr, nullptr};

    explicit StreamTimer(bool wanted_) : wanted(wanted_) {}
    StreamTimer(const StreamTimer&) = delete;
    StreamTimer& operator=(const StreamTimer&) = delete;
    ~StreamTimer() {
        for (hipEvent_t e : ev)
            if (e) (void)hipEventDestroy(e);
    }
    void start(Scratch& sc) {
        if (!wanted) return;
        for (hipEvent_t& e : ev)
            if (sc.ok()) sc.note(hipEventCreate(&e));
        if (sc.ok()) sc.note(hipEventRecord(ev[0], sc.st));
    }
    void stop(Scratch& sc) {
        if (wanted && sc.ok()) sc.note(hipEventRecord(ev[1], sc.st));
    }
    void read(Scratch& sc, double* ms) {
        if (!wanted || !sc.ok()) return;
        float f = 0.0f;
        sc.note(hipEventElapsedTime(&f, ev[0], ev[1]));
        *ms = (double)f;
    }
};

// A device buffer that only grows and stays with its owner (the k-NN state of a ctx, the moment sums of a pf_cpd).  No
// destructor: the owner releases it, or pf_destroy's sweep over the ctx's blocks does.  grow does not carry the contents
// over; after a failed grow the buffer is empty (p == NULL, cap == 0) and may be grown or released again.
template <class T>
struct DevBuf {
    T* p = nullptr;
    int64_t cap = 0;  // elements

    hipError_t grow(hipStream_t st, int64_t need) {
        if (need <= cap) return hipSuccess;
        release(st);
        void* q = nullptr;
        const hipError_t e = pf_malloc(st, &q, sizeof(T) * (size_t)need);
        if (e != hipSuccess) return e;
        p = (T*)q;
        cap = need;
        return hipSuccess;
    }
    void release(hipStream_t st) {
        pf_free(st, p);
        p = nullptr;
        cap = 0;
    }
};

// Pinned host blocks and events of freed graphs, handed to the next graph (hipHostMalloc / hipHostFree and event creation
// cost 0.1-0.2 ms each: more than a 250k-vertex assembly kernel).  One per ctx; pf_destroy frees what is left.
struct HostPools {
    std::vector<std::pair<int32_t, double*>> pinned_pool;  // (capacity in doubles, block of capacity + 2)
    std::vector<hipEvent_t> event_pool;                    // created with hipEventDisableTiming

    hipError_t take_event(hipEvent_t* ev) {  // *ev stays as it is when it holds one; NULL after a failure
        if (*ev) return hipSuccess;
        if (!event_pool.empty()) {
            *ev = event_pool.back();
            event_pool.pop_back();
            return hipSuccess;
        }
        const hipError_t e = hipEventCreateWithFlags(ev, hipEventDisableTiming);
        if (e != hipSuccess) *ev = nullptr;
        return e;
    }
    void give_event(hipEvent_t* ev) {
        if (*ev) event_pool.push_back(*ev);
        *ev = nullptr;
    }
};

// Where a few doubles of a graph land on the host: a pinned block of cap + 2 doubles (the two spare ones are the caller's
// to use: the verdict and the ticket of a Gram-Schmidt step) and the event recorded behind the copy.  Block and event come
// from the ctx's pools and go back there; no destructor: the owner releases (pf_graph_free).  A landing holds both or
// neither: after a failed ensure it is empty, and may be ensured or released again.
struct HostLanding {
    double* host = nullptr;
    int32_t cap = 0;  // doubles
    hipEvent_t ev = nullptr;

    // A block with cap >= need, and an event.  The block held is kept when it is large enough (the common case: two
    // compares).  Otherwise it goes back to the pool - after `drain` has run dry, when the caller names a stream whose
    // work may still write to it - and the first pooled block of max(need, floor) doubles or more takes its place, or a new
    // one of that size (of `fresh` doubles, if that is more).
    hipError_t ensure(HostPools& pools, int32_t need, int32_t floor, hipStream_t drain, int32_t fresh = 0) {
        if (host && need <= cap) return hipSuccess;
        return replace(pools, std::max(need, floor), drain, fresh);
    }
    void release(HostPools& pools) {
        if (host) pools.pinned_pool.emplace_back(cap, host);
        host = nullptr;
        cap = 0;
        pools.give_event(&ev);
    }

   private:
    hipError_t replace(HostPools& pools, int32_t least, hipStream_t drain, int32_t fresh) {
        hipError_t e = host && drain ? hipStreamSynchronize(drain) : hipSuccess;
        if (host) pools.pinned_pool.emplace_back(cap, host);
        host = nullptr;
        cap = 0;
        for (size_t i = 0; e == hipSuccess && i < pools.pinned_pool.size(); ++i)
            if (pools.pinned_pool[i].first >= least) {  // a block a freed graph left behind
                cap = pools.pinned_pool[i].first;
                host = pools.pinned_pool[i].second;
                pools.pinned_pool.erase(pools.pinned_pool.begin() + (long)i);
                break;
            }
        if (e == hipSuccess && !host) {
            void* p = nullptr;
            const int32_t size = std::max(least, fresh);
            e = hipHostMalloc(&p, sizeof(double) * (size_t)(size + 2), hipHostMallocDefault);
            if (e == hipSuccess) host = (double*)p, cap = size;
        }
        if (e == hipSuccess) e = pools.take_event(&ev);
        if (e != hipSuccess) release(pools);
        return e;
    }
};
