// The scroll of the resident volume (include/blok_hip.h: blok_hip_volume_scroll has the contract).  The one place its arithmetic lives: the
// kernels (hip/scroll_kernels.hip), the entry (hip/api_volume.hip) and the host builds (host/scroll.cpp) all include this header.  No HIP
// types.  Integer arithmetic only.
#ifndef BLOK_SCROLL_CORE_H
#define BLOK_SCROLL_CORE_H
#include <stdint.h>

#include "blok_hip.h"

#if defined(__HIPCC__)
#define BLOK_SCROLL_HD __host__ __device__ inline
#else
#define BLOK_SCROLL_HD inline
#endif

namespace blok {
namespace scroll {

constexpr uint32_t kFlags = BLOK_SCROLL_PLAN_ONLY;
constexpr int64_t kLatticeLo = -32768, kLatticeHi = 32768;      // the int16 lattice of the hit records (gpu_volume_create's rule)

// ---- the argument rule --------------------------------------------------------------------------------------------------------------------
// 0 = fine, otherwise the rule that failed (status, rule_text).  origin, dims: the box before the call.
inline int check_args(const int32_t origin[3], const uint32_t dims[3], const int32_t* delta, uint32_t flags) {
    if (!delta) return 1;
    for (int a = 0; a < 3; ++a) if (delta[a] % 4 != 0) return 2;
    if (flags & ~kFlags) return 3;
    for (int a = 0; a < 3; ++a) {
        const int64_t lo = int64_t(origin[a]) + delta[a];
        if (lo < kLatticeLo || lo + int64_t(dims[a]) > kLatticeHi) return 4;
    }
    return 0;
}
inline int status(int rule) { return rule == 0 ? BLOK_OK : rule == 4 ? BLOK_ERR_UNSUPPORTED : BLOK_ERR_INVALID_ARG; }
inline const char* rule_text(int rule) {
    static const char* const kText[] = {"", "null delta", "a component of delta is not a multiple of 4", "unknown flag bits",
                                        "the new box leaves the int16 lattice [-32768, 32768]"};
    return kText[rule];
}

// ---- the plan -----------------------------------------------------------------------------------------------------------------------------
// The boxes of `box` (world, [blo, bhi)) outside the kept box C = [clo, chi), C non-empty and inside `box`: the z slab, the y slab, the x
// slab, in this order and only where non-empty.  On an axis C touches at least one end of `box` (the two boxes have the same size), so
// box \ C is one interval there.
inline uint32_t boxes_outside(const int64_t blo[3], const int64_t bhi[3], const int64_t clo[3], const int64_t chi[3], blok_scroll_box out[3]) {
    uint32_t n = 0;
    for (int a = 2; a >= 0; --a) {
        const int64_t lo = clo[a] > blo[a] ? blo[a] : chi[a], hi = clo[a] > blo[a] ? clo[a] : bhi[a];      // box \ C along a
        if (hi <= lo) continue;
        blok_scroll_box& b = out[n++];
        for (int k = 0; k < 3; ++k) {
            const bool kept = k > a;                   // the axes above a are cut to C, the ones below span the box
            b.lo[k] = static_cast<int32_t>(k == a ? lo : kept ? clo[k] : blo[k]);
            b.hi[k] = static_cast<int32_t>(k == a ? hi : kept ? chi[k] : bhi[k]);
        }
    }
    return n;
}

// Everything of *info but the two filled counts (left 0), for arguments that have passed check_args.
inline void plan(const int32_t origin[3], const uint32_t dims[3], const int32_t delta[3], blok_scroll_info* info) {
    *info = blok_scroll_info{};
    int64_t old_lo[3], old_hi[3], new_lo[3], new_hi[3], clo[3], chi[3];
    bool keeps = true;
    for (int a = 0; a < 3; ++a) {
        old_lo[a] = origin[a]; old_hi[a] = old_lo[a] + dims[a];
        new_lo[a] = old_lo[a] + delta[a]; new_hi[a] = new_lo[a] + dims[a];
        clo[a] = old_lo[a] > new_lo[a] ? old_lo[a] : new_lo[a]; chi[a] = old_hi[a] < new_hi[a] ? old_hi[a] : new_hi[a];
        keeps = keeps && chi[a] > clo[a];
        info->origin[a] = static_cast<int32_t>(new_lo[a]); info->delta[a] = delta[a];
    }
    if (!keeps) {
        info->n_exposed = info->n_leaving = 1u;
        for (int a = 0; a < 3; ++a) {
            info->exposed[0].lo[a] = static_cast<int32_t>(new_lo[a]); info->exposed[0].hi[a] = static_cast<int32_t>(new_hi[a]);
            info->leaving[0].lo[a] = static_cast<int32_t>(old_lo[a]); info->leaving[0].hi[a] = static_cast<int32_t>(old_hi[a]);
        }
        return;
    }
    info->n_exposed = boxes_outside(new_lo, new_hi, clo, chi, info->exposed);
    info->n_leaving = boxes_outside(old_lo, old_hi, clo, chi, info->leaving);
    info->n_cells_kept = static_cast<uint64_t>(chi[0] - clo[0]) * static_cast<uint64_t>(chi[1] - clo[1]) * static_cast<uint64_t>(chi[2] - clo[2]);
}

// ---- the per-cell source rule -------------------------------------------------------------------------------------------------------------
// Cell c (box-local, one axis) of the new box holds the world cell that was cell c + delta of the old box: *src, when that lies in
// [0, dim); false = exposed.  The same rule in units of bricks takes delta / 4 and the axis's brick count.
BLOK_SCROLL_HD bool source(uint32_t c, int32_t delta, uint32_t dim, uint32_t* src) {
    const int64_t s = int64_t(c) + delta;
    if (s < 0 || s >= int64_t(dim)) return false;
    *src = static_cast<uint32_t>(s);
    return true;
}
// The cells of the new box along one axis for which source() holds: [*lo, *hi), empty (0, 0) when nothing is kept on the axis.
BLOK_SCROLL_HD void kept_range(int32_t delta, uint32_t dim, uint32_t* lo, uint32_t* hi) {
    const int64_t l = delta < 0 ? -int64_t(delta) : 0, h = delta > 0 ? int64_t(dim) - delta : int64_t(dim);
    *lo = h > l ? static_cast<uint32_t>(l) : 0u; *hi = h > l ? static_cast<uint32_t>(h) : 0u;
}

// ---- the cut of a brick mask by the box's ragged end --------------------------------------------------------------------------------------
// The bits (x + 4 y + 16 z) of brick b along one axis whose cells lie below `dim`: a mask bit never refers to a cell outside the box.
BLOK_SCROLL_HD uint64_t axis_bits(uint32_t axis, uint32_t b, uint32_t dim) {
    const uint32_t n = dim - 4u * b >= 4u ? 4u : dim - 4u * b;      // cells of the brick inside the box, 1..4 (b is a brick of the box)
    if (n == 4u) return ~0ull;
    if (axis == 0u) return 0x1111111111111111ull * ((1u << n) - 1u);
    if (axis == 1u) return 0x0001000100010001ull * ((1u << (4u * n)) - 1u);
    return (1ull << (16u * n)) - 1ull;
}
BLOK_SCROLL_HD uint64_t cut_mask(uint64_t mask, uint32_t bx, uint32_t by, uint32_t bz, uint32_t nx, uint32_t ny, uint32_t nz) {
    return mask & axis_bits(0u, bx, nx) & axis_bits(1u, by, ny) & axis_bits(2u, bz, nz);
}

}  // namespace scroll
}  // namespace blok
#endif
