// Stamping a placed model into a voxel volume and capturing a region as a model (include/blok_hip.h: blok_hip_volume_stamp_models and
// blok_hip_volume_capture_model have the contract).  The one place the placement's arithmetic lives: the kernel (hip/stamp_kernels.hip)
// and the host build (host/stamp.cpp) both include this header.  No HIP types.  Every sum is 64-bit, so an offset near the ends of int32
// never wraps before the result is clipped against the box.
#ifndef BLOK_STAMP_CORE_H
#define BLOK_STAMP_CORE_H
#include <stdint.h>

#include "blok_hip.h"

#if defined(__HIPCC__)
#define BLOK_STAMP_HD __host__ __device__ __forceinline__
#else
#define BLOK_STAMP_HD inline
#endif

namespace blok {
namespace stamp {

// Component `a` (0, 1, 2) of a triple, by selects: the permutation is data, and an array indexed by it would live in scratch on the device.
BLOK_STAMP_HD int64_t pick(uint32_t a, int64_t x, int64_t y, int64_t z) { return a == 0u ? x : (a == 1u ? y : z); }

// The record itself: axis a permutation of 0, 1, 2, only the three flip bits, reserved words zero (blok_hip.h: Limits).  The one
// predicate for it: instance_core.h's instance_well_formed is this function.
BLOK_STAMP_HD bool well_formed(const blok_instance& I) {
    const uint32_t a0 = I.axis[0], a1 = I.axis[1], a2 = I.axis[2];
    const bool perm = a0 < 3u && a1 < 3u && a2 < 3u && ((1u << a0) | (1u << a1) | (1u << a2)) == 7u;
    return perm && I.flip < 8u && (I.reserved[0] | I.reserved[1] | I.reserved[2]) == 0u;
}

BLOK_STAMP_HD bool mode_known(int mode) { return mode == BLOK_STAMP_SET || mode == BLOK_STAMP_KEEP || mode == BLOK_STAMP_ERASE; }
// A volume's voxel is filled iff its density > 0: zero of either sign, negative values and NaN are empty (the rebuild's rule).
BLOK_STAMP_HD bool filled(float density) { return density > 0.0f; }

// "Record back to world space" (blok_hip.h): local coordinate v of local axis k, along world axis I.axis[k].
BLOK_STAMP_HD int64_t to_world(const blok_instance& I, uint32_t k, int64_t v) {
    const int64_t o = pick(I.axis[k], I.offset[0], I.offset[1], I.offset[2]);
    return ((I.flip >> k) & 1u) ? o - 1 - v : o + v;
}
// Its inverse: the local coordinate of local axis k whose voxel lands on w along world axis I.axis[k].
BLOK_STAMP_HD int64_t to_local(const blok_instance& I, uint32_t k, int64_t w) {
    const int64_t o = pick(I.axis[k], I.offset[0], I.offset[1], I.offset[2]);
    return ((I.flip >> k) & 1u) ? o - 1 - w : w - o;
}

// The local coordinates of local axis k, half open, whose voxels land inside the world interval [wlo, whi) of axis I.axis[k].  (A flip
// maps the interval's ends onto each other: the voxel that lands on whi - 1 is the first one.)
BLOK_STAMP_HD void local_span(const blok_instance& I, uint32_t k, int64_t wlo, int64_t whi, int64_t& lo, int64_t& hi) {
    if ((I.flip >> k) & 1u) { lo = to_local(I, k, whi - 1); hi = to_local(I, k, wlo) + 1; }
    else { lo = to_local(I, k, wlo); hi = to_local(I, k, whi); }
}
// The world interval, half open, along axis I.axis[k] that the local interval [lo, hi) of local axis k lands on.
BLOK_STAMP_HD void world_span(const blok_instance& I, uint32_t k, int64_t lo, int64_t hi, int64_t& wlo, int64_t& whi) {
    if ((I.flip >> k) & 1u) { wlo = to_world(I, k, hi - 1); whi = to_world(I, k, lo) + 1; }
    else { wlo = to_world(I, k, lo); whi = to_world(I, k, hi); }
}

// What one mapped model voxel does to the volume's voxel: true iff it is written, and then with (out_density, out_id).
BLOK_STAMP_HD bool apply(int mode, float value, uint32_t material, float present, float& out_density, uint32_t& out_id) {
    if (mode == BLOK_STAMP_ERASE) { out_density = 0.0f; out_id = 0u; return true; }
    if (mode == BLOK_STAMP_KEEP && filled(present)) return false;
    out_density = value; out_id = material;
    return true;
}

}  // namespace stamp
}  // namespace blok
#endif
