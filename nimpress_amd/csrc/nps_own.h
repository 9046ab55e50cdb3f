// nps_own.h -- the owners of the HIP resources of nps_engine.hip (internal: not part of the C-ABI, no kernel sees it).
//
// Four move-only types, one resource each, released by their destructors: a struct that holds them needs no list of
// frees, and a function that holds one may return from anywhere.  live_resources counts what is alive (one per device
// or pinned allocation, event and stream): nps_live_resources().
#pragma once
#include <hip/hip_runtime.h>

#include <atomic>
#include <cstdint>
#include <utility>

namespace nps {

inline std::atomic<int64_t> live_resources{0};

// a hipMalloc allocation of cap() elements of T
template <class T>
class DevBuf {
    T *p_ = nullptr;
    uint64_t cap_ = 0;

public:
    DevBuf() = default;
    DevBuf(DevBuf &&o) noexcept : p_(std::exchange(o.p_, nullptr)), cap_(std::exchange(o.cap_, 0)) {}
    ~DevBuf() { reset(); }
    T *get() const { return p_; }
    uint64_t cap() const { return cap_; }
    // a buffer of n elements, whatever it held before (empty on failure)
    hipError_t alloc(uint64_t n) {
        reset();
        const hipError_t e = hipMalloc(&p_, sizeof(T) * n);
        if (e != hipSuccess) p_ = nullptr;
        if (p_) {
            cap_ = n;
            ++live_resources;
        }
        return e;
    }
    // at least `need` elements afterwards, exactly `need` after growing (contents are not kept).  Growing waits for `st`,
    // whose queued work may still use the old allocation; on failure the buffer is empty, nothing else has changed.
    hipError_t ensure(uint64_t need, hipStream_t st, bool *grew = nullptr) {
        if (need <= cap_) return hipSuccess;
        const hipError_t e = hipStreamSynchronize(st);
        if (e != hipSuccess) return e;
        if (grew) *grew = true;
        return alloc(need);
    }
    void reset() {
        if (p_) {
            (void)hipFree(p_);
            --live_resources;
        }
        p_ = nullptr;
        cap_ = 0;
    }
};

// a hipHostMalloc allocation of cap() bytes
class PinnedBuf {
    void *p_ = nullptr;
    size_t cap_ = 0;

public:
    PinnedBuf() = default;
    PinnedBuf(PinnedBuf &&o) noexcept : p_(std::exchange(o.p_, nullptr)), cap_(std::exchange(o.cap_, 0)) {}
    ~PinnedBuf() { reset(); }
    void *get() const { return p_; }
    size_t cap() const { return cap_; }
    hipError_t alloc(size_t bytes) {
        reset();
        const hipError_t e = hipHostMalloc(&p_, bytes);
        if (e != hipSuccess) p_ = nullptr;
        if (p_) {
            cap_ = bytes;
            ++live_resources;
        }
        return e;
    }
    void reset() {
        if (p_) {
            (void)hipHostFree(p_);
            --live_resources;
        }
        p_ = nullptr;
        cap_ = 0;
    }
};

class Event {
    hipEvent_t ev_ = nullptr;

public:
    Event() = default;
    Event(Event &&o) noexcept : ev_(std::exchange(o.ev_, nullptr)) {}
    ~Event() {
        if (!ev_) return;
        (void)hipEventDestroy(ev_);
        --live_resources;
    }
    hipEvent_t get() const { return ev_; }
    hipError_t create(unsigned flags) {  // (an empty one)
        const hipError_t e = hipEventCreateWithFlags(&ev_, flags);
        if (e != hipSuccess) ev_ = nullptr;
        if (ev_) ++live_resources;
        return e;
    }
};

class Stream {
    hipStream_t st_ = nullptr;

public:
    Stream() = default;
    Stream(Stream &&o) noexcept : st_(std::exchange(o.st_, nullptr)) {}
    ~Stream() {
        if (!st_) return;
        (void)hipStreamDestroy(st_);
        --live_resources;
    }
    hipStream_t get() const { return st_; }
    hipError_t create() {  // (an empty one)
        const hipError_t e = hipStreamCreateWithFlags(&st_, hipStreamNonBlocking);
        if (e != hipSuccess) st_ = nullptr;
        if (st_) ++live_resources;
        return e;
    }
};

}  // namespace nps
