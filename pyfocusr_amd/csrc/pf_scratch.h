// Device memory as the host code of the library holds it: the scratch of one call (Scratch) and a buffer that grows and
// stays (DevBuf), both on top of the ctx's caching allocator (pf_api.hip); and the timer of a call's stream work
// (StreamTimer).  Only the HIP C API is needed here, so the failure paths of all three run on the CPU over test doubles
// of the allocator and of the event calls (tests/csrc/scratch_paths.cpp).
#pragma once
#include <hip/hip_runtime_api.h>
#include <stddef.h>
#include <stdint.h>
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
