// nps_own.h -- the owners of the HIP resources of the C-ABI's objects (internal: included through nps_engine.h by the four
// units that implement them, not part of the C-ABI, no kernel sees it).
//
// Five move-only types, released by their destructors: a struct that holds them needs no list of frees, and a function
// that holds one may return from anywhere.  Four hold one resource each; the fifth, StagingRing, is made of two of the
// others.  live_resources counts what is alive (one per device or pinned allocation, event and stream):
// nps_live_resources().
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
    ~Event() { reset(); }
    hipEvent_t get() const { return ev_; }
    hipError_t create(unsigned flags) {  // (an empty one)
        const hipError_t e = hipEventCreateWithFlags(&ev_, flags);
        if (e != hipSuccess) ev_ = nullptr;
        if (ev_) ++live_resources;
        return e;
    }
    void reset() {
        if (ev_) {
            (void)hipEventDestroy(ev_);
            --live_resources;
        }
        ev_ = nullptr;
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

// A ring of pinned host slots between a caller's buffer and the device.  The caller's row is copied into acquire()'s slot,
// the work that reads the slot (a kernel, over PCIe, or a copy) is queued on a stream, and release() records the slot's
// event behind it: the caller may reuse its buffer at once, and a slot is written again only after its last reader has
// finished.  One pinned allocation holds the slots, each rounded up to 4 KiB; the ring is built or empty, never between.
class StagingRing {
public:
    static constexpr int kMaxSlots = 8;
    explicit StagingRing(int slots) : slots_(slots < kMaxSlots ? slots : kMaxSlots) {}
    StagingRing(StagingRing &&) noexcept = default;  // (the ring moved from holds no memory: it is empty)
    bool built() const { return mem_.get() != nullptr; }
    size_t slot_bytes() const { return mem_.cap() / slots_; }
    // Slots of at least `bytes` afterwards.  Nothing to do while the ring is built and large enough; a built ring that
    // is too small waits for `st`, whose queued work may still read the old slots, and is released first.  The new slots
    // hold exactly `bytes` plus the rounding.  On failure the ring is empty and the next call builds it again (only a
    // failed wait leaves the old ring as it was: its slots may still be read).
    hipError_t ensure(size_t bytes, hipStream_t st) {
        if (built() && bytes <= slot_bytes()) return hipSuccess;
        if (built()) {
            const hipError_t e = hipStreamSynchronize(st);
            if (e != hipSuccess) return e;
        }
        reset();
        const size_t each = ((bytes ? bytes : 1) + 4095) / 4096 * 4096;
        hipError_t e = mem_.alloc(each * slots_);
        for (int k = 0; e == hipSuccess && k < slots_; ++k) e = ev_[k].create(hipEventDisableTiming);
        if (e != hipSuccess) reset();
        return e;
    }
    // the next slot in turn, once its last reader has finished: waits on that slot's event only, never on a stream
    hipError_t acquire(void **slot) {
        const hipError_t e = hipEventSynchronize(ev_[next_].get());
        if (e != hipSuccess) return e;
        held_ = next_;
        next_ = (next_ + 1) % slots_;
        *slot = static_cast<char *>(mem_.get()) + (size_t)held_ * slot_bytes();
        return hipSuccess;
    }
    // the work that reads the acquired slot has been queued on `st`.  (A launch that failed is followed by no release:
    // nothing reads the slot, and its event stays as it was.)
    hipError_t release(hipStream_t st) { return hipEventRecord(ev_[held_].get(), st); }
    void reset() {
        for (Event &e : ev_) e.reset();
        mem_.reset();
        next_ = held_ = 0;
    }

private:
    PinnedBuf mem_;
    Event ev_[kMaxSlots];
    int slots_;
    int next_ = 0, held_ = 0;
};

}  // namespace nps
