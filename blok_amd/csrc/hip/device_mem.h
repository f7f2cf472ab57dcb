// Host-side plumbing of the functions behind gpu_build.h: the one way a failed HIP call becomes a GpuBuildStatus, and the small things
// every entry there starts with.  Their allocations are DeviceMem's (device_buffer.h).
#ifndef BLOK_DEVICE_MEM_H
#define BLOK_DEVICE_MEM_H
#include <hip/hip_runtime.h>

#include <string>

#include "device_buffer.h"
#include "gpu_build.h"

namespace blok {

// In a function that returns GpuBuildStatus and has `std::string* why`: a failed call's text into *why, its status returned.
#define BLOK_GPU_TRY(call) do { hipError_t e_ = (call); if (e_ != hipSuccess) { *why = std::string(#call) + ": " + hipGetErrorString(e_); \
                                return e_ == hipErrorOutOfMemory ? ::blok::GpuBuildStatus::OutOfMemory : ::blok::GpuBuildStatus::HipError; } } while (0)

// Workgroups of 256 lanes for n items, a lane each.
inline uint32_t blocks_for(uint64_t n) { return static_cast<uint32_t>((n + 255u) / 256u); }

// The kernels index the volume's cells in 32 bits.  False, with `entry` (the caller's name) in *why, for a volume they cannot address: the
// caller returns Unsupported.
inline bool cells_fit_32_bits(const GpuVolume* v, const char* entry, std::string* why) {
    if (v->cells() <= 0xFFFFFFFFull) return true;
    *why = std::string(entry) + ": volume larger than 2^32 cells";
    return false;
}

// What the field builders (gpu_build.h: GpuField) begin with: *out reset, the 2^32 check with the entry's name in the text, the info's version, flags, lo and ext and
// the holder's lo from the box-local region [lo, hi), ext[].  False: nothing to compute, and *st says why — Unsupported, or Ok for a region
// without a cell.
template <class Field>
bool gpu_field_begin(const GpuVolume* v, const char* entry, const uint32_t lo[3], const uint32_t hi[3], uint32_t flags, Field* out, uint32_t ext[3],
                     GpuBuildStatus* st, std::string* why) {
    *out = Field{};
    *st = GpuBuildStatus::Unsupported;
    if (!cells_fit_32_bits(v, entry, why)) return false;
    out->info.version = 1u; out->info.flags = flags;
    for (int k = 0; k < 3; ++k) {
        out->lo[k] = lo[k]; ext[k] = hi[k] > lo[k] ? hi[k] - lo[k] : 0u;
        out->info.lo[k] = v->origin[k] + static_cast<int32_t>(lo[k]); out->info.ext[k] = ext[k];
    }
    *st = GpuBuildStatus::Ok;
    return ext[0] && ext[1] && ext[2];
}

}  // namespace blok
#endif
