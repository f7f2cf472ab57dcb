// Owners of what the host side allocates from HIP: device arrays, pinned host arrays, events, and the scope-bound DeviceMem of the
// volume functions.  Every hipMalloc / hipFree / hipHostMalloc / hipHostFree / hipEventDestroy of the C ABI is in this file.  It includes
// nothing of the project and only the runtime's API header, so that a host program can compile it and stand in for the runtime
// (tests/host_harness/device_buffer_main.cpp).
#ifndef BLOK_DEVICE_BUFFER_H
#define BLOK_DEVICE_BUFFER_H
#include <hip/hip_runtime_api.h>

#include <algorithm>
#include <cstddef>
#include <cstdint>
#include <type_traits>
#include <utility>
#include <vector>

namespace blok {

// What has to finish before an array that is being replaced may be freed: nothing (a blocking entry, or the caller has waited), the work
// of one stream (per-stream scratch), or the device (buffers that frames on any stream use).
struct FreeAfter {
    enum Kind { kNothing, kStream, kDevice } kind = kNothing;
    hipStream_t stream = nullptr;
    static FreeAfter nothing() { return {}; }
    static FreeAfter work_on(hipStream_t s) { return {kStream, s}; }
    static FreeAfter device() { return {kDevice, nullptr}; }
    hipError_t wait() const { return kind == kStream ? hipStreamSynchronize(stream) : kind == kDevice ? hipDeviceSynchronize() : hipSuccess; }
};

// An array of `capacity()` elements of T (bytes for T = void) in device memory, or in pinned host memory.  Move-only; frees on destruction,
// and a reset is the assignment of a fresh value.  Converts to the plain pointer the kernels' arguments take.
template <class T, bool Pinned = false>
class Buffer {
public:
    Buffer() = default;
    Buffer(Buffer&& o) noexcept : p_(std::exchange(o.p_, nullptr)), n_(std::exchange(o.n_, 0)) {}
    Buffer& operator=(Buffer&& o) noexcept {
        if (this != &o) { reset(); p_ = std::exchange(o.p_, nullptr); n_ = std::exchange(o.n_, 0); }
        return *this;
    }
    ~Buffer() { reset(); }
    T* get() const { return p_; }
    operator T*() const { return p_; }
    size_t capacity() const { return n_; }
    void reset() {
        if (p_) (void)(Pinned ? hipHostFree(p_) : hipFree(p_));
        p_ = nullptr; n_ = 0;
    }
    // Takes over an array of n elements that somebody else allocated (the device builders hand their trees over so).
    void adopt(T* p, size_t n) { reset(); p_ = p; n_ = p ? n : 0; }
    // Grow-only.  Enough room already: one comparison, no HIP call, *replaced false.  Else: `wait` (only when there is an old array; if it
    // fails, its error, and the old array stays), free, allocate; *replaced true — the caller fills the new array, in stream order, and
    // resets whatever counted on the old one.  On a failed allocation the array is empty, *replaced false, and HIP's sticky error is
    // cleared: the caller reports the returned code, and the next hipGetLastError() behind a launch must not find this one.
    hipError_t reserve(size_t count, FreeAfter wait, bool* replaced = nullptr) {
        if (replaced) *replaced = false;
        if (count <= n_) return hipSuccess;
        if (p_) {
            const hipError_t w = wait.wait();
            if (w != hipSuccess) return w;
            reset();
        }
        void* raw = nullptr;
        const size_t bytes = count * kElement;
        const hipError_t e = Pinned ? hipHostMalloc(&raw, bytes, hipHostMallocDefault) : hipMalloc(&raw, bytes);
        if (e != hipSuccess) { (void)hipGetLastError(); return e; }
        p_ = static_cast<T*>(raw); n_ = count;
        if (replaced) *replaced = true;
        return hipSuccess;
    }

private:
    static constexpr size_t kElement = sizeof(std::conditional_t<std::is_void_v<T>, char, T>);
    T* p_ = nullptr;
    size_t n_ = 0;
};
template <class T> using DeviceArray = Buffer<T, false>;
template <class T> using PinnedArray = Buffer<T, true>;
using DeviceBytes = DeviceArray<void>;

// A hipEvent_t that is destroyed with its holder.  create() makes it once: a second call is no HIP call.
class Event {
public:
    Event() = default;
    Event(Event&& o) noexcept : e_(std::exchange(o.e_, nullptr)) {}
    Event& operator=(Event&& o) noexcept {
        if (this != &o) { reset(); e_ = std::exchange(o.e_, nullptr); }
        return *this;
    }
    ~Event() { reset(); }
    hipEvent_t get() const { return e_; }
    operator hipEvent_t() const { return e_; }
    hipError_t create(unsigned flags = hipEventDisableTiming) { return e_ ? hipSuccess : hipEventCreateWithFlags(&e_, flags); }
    void reset() {
        if (e_) (void)hipEventDestroy(e_);
        e_ = nullptr;
    }

private:
    hipEvent_t e_ = nullptr;
};

// Several allocations of one function: frees what it still owns on scope exit.  release(p) hands p to the caller (a null p is fine).
struct DeviceMem {
    std::vector<void*> ptrs;
    DeviceMem() = default;
    DeviceMem(const DeviceMem&) = delete;
    DeviceMem& operator=(const DeviceMem&) = delete;
    ~DeviceMem() { for (void* p : ptrs) if (p) (void)hipFree(p); }
    // `count` elements (at least one).  On failure *p is null and the sticky error is cleared, as in Buffer::reserve.
    template <class T> hipError_t alloc(T** p, uint64_t count) {
        *p = nullptr;
        void* raw = nullptr;
        const hipError_t e = hipMalloc(&raw, std::max<uint64_t>(count, 1u) * sizeof(T));
        if (e != hipSuccess) { (void)hipGetLastError(); return e; }
        ptrs.push_back(raw); *p = static_cast<T*>(raw);
        return hipSuccess;
    }
    void release(void* p) { for (void*& q : ptrs) if (q == p) q = nullptr; }
};

}  // namespace blok
#endif
