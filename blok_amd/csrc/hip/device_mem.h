// Host-side plumbing of the functions behind gpu_build.h: device allocations that are freed on scope exit, and the one way a failed HIP
// call becomes a GpuBuildStatus.
#ifndef BLOK_DEVICE_MEM_H
#define BLOK_DEVICE_MEM_H
#include <hip/hip_runtime.h>

#include <algorithm>
#include <string>
#include <vector>

#include "gpu_build.h"

namespace blok {

// Frees what it still owns on scope exit.  release(p) hands p to the caller (a null p is fine).
struct DeviceMem {
    std::vector<void*> ptrs;
    ~DeviceMem() { for (void* p : ptrs) if (p) (void)hipFree(p); }
    // `count` elements (at least one).  On failure *p is null and the sticky error is cleared: the caller reports the returned code, and
    // the next hipGetLastError() after a launch must not find this one.
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

// In a function that returns GpuBuildStatus and has `std::string* why`: a failed call's text into *why, its status returned.
#define BLOK_GPU_TRY(call) do { hipError_t e_ = (call); if (e_ != hipSuccess) { *why = std::string(#call) + ": " + hipGetErrorString(e_); \
                                return e_ == hipErrorOutOfMemory ? ::blok::GpuBuildStatus::OutOfMemory : ::blok::GpuBuildStatus::HipError; } } while (0)

}  // namespace blok
#endif
