// Sweeping a placed model against a voxel volume (include/blok_hip.h: blok_hip_volume_sweep_models has the contract).  The one place the
// sweep's arithmetic lives: the kernel (hip/sweep_kernels.hip) and the host build (host/sweep.cpp) both include this header.  No HIP
// types.  The placement's mapping is stamp_core.h's; coordinates are 64-bit, so a start far outside the box never wraps.
#ifndef BLOK_SWEEP_CORE_H
#define BLOK_SWEEP_CORE_H
#include <stdint.h>

#include "blok_hip.h"
#include "stamp_core.h"

namespace blok {
namespace sweep {

// Direction d in blok_hit::face numbering (0 +X, 1 -X, 2 +Y, 3 -Y, 4 +Z, 5 -Z): its world axis and the sign of its unit vector.
BLOK_STAMP_HD bool direction_known(uint32_t d) { return d < 6u; }
BLOK_STAMP_HD uint32_t direction_axis(uint32_t d) { return d >> 1; }
BLOK_STAMP_HD int direction_sign(uint32_t d) { return (d & 1u) ? -1 : 1; }
BLOK_STAMP_HD bool flags_known(uint32_t flags) { return (flags & ~BLOK_SWEEP_BOX_IS_SOLID) == 0u; }
// The outside-the-box rule: a cell outside the volume's box is empty, or filled with BLOK_SWEEP_BOX_IS_SOLID.
BLOK_STAMP_HD bool outside_filled(uint32_t flags) { return (flags & BLOK_SWEEP_BOX_IS_SOLID) != 0u; }

// The world direction in a placement's local lattice: the local axis that runs along the world axis, and the sign a step of +1 along
// the world direction has there (the direction's sign times the flip).
BLOK_STAMP_HD uint32_t local_axis(const blok_instance& I, uint32_t world_axis) {
    return I.axis[0] == world_axis ? 0u : (I.axis[1] == world_axis ? 1u : 2u);
}
BLOK_STAMP_HD int local_sign(const blok_instance& I, uint32_t local_k, int world_sign) {
    return ((I.flip >> local_k) & 1u) ? -world_sign : world_sign;
}

// Bit of voxel (x, y, z) of a 4^3 brick in its 64-bit mask, and the distance between the bits of neighbours along an axis.
BLOK_STAMP_HD uint32_t brick_bit(uint32_t x, uint32_t y, uint32_t z) { return x | (y << 2) | (z << 4); }
BLOK_STAMP_HD uint32_t bit_stride(uint32_t axis) { return axis == 0u ? 1u : (axis == 1u ? 4u : 16u); }
// The 4-bit column of a brick mask along `axis` through the voxel with in-brick coordinates (x, y, z) (the one along the axis is not
// looked at): bit i = the voxel with coordinate i along the axis.  Along x the column is 4 adjacent bits, along y every 4th, along z every 16th.
BLOK_STAMP_HD uint32_t column4(uint64_t mask, uint32_t axis, uint32_t x, uint32_t y, uint32_t z) {
    const uint32_t base = axis == 0u ? brick_bit(0u, y, z) : (axis == 1u ? brick_bit(x, 0u, z) : brick_bit(x, y, 0u));
    const uint32_t s = bit_stride(axis);
    const uint64_t m = mask >> base;
    return static_cast<uint32_t>((m & 1ull) | (((m >> s) & 1ull) << 1) | (((m >> (2u * s)) & 1ull) << 2) | (((m >> (3u * s)) & 1ull) << 3));
}
// First filled cell of a 4-bit column from position p (0..3) in direction sign: the number of steps to it, p itself being 0 steps; 4 = none.
BLOK_STAMP_HD uint32_t first_filled(uint32_t column, uint32_t p, int sign) {
    if (sign > 0) {
        const uint32_t t = (column & 0xFu) >> p;
        return t == 0u ? 4u : ((t & 1u) ? 0u : ((t & 2u) ? 1u : ((t & 4u) ? 2u : 3u)));
    }
    const uint32_t t = (column << (3u - p)) & 0xFu;              // bit 3 = position p, bit 2 = p - 1, ...
    return t == 0u ? 4u : ((t & 8u) ? 0u : ((t & 4u) ? 1u : ((t & 2u) ? 2u : 3u)));
}

// free(v') of the contract for a voxel whose column lies inside the box in the two perpendicular axes.  p: box-local coordinate of the
// start cell along the sweep's axis (any value: the start may lie outside the box); n: the box's extent along it.  column(b) is the 4-bit
// column of cells 4 b .. 4 b + 3 of that axis (0 <= b < ceil(n / 4)); best() is a value no smaller than which the answer is of no use
// (the caller's running minimum; 0xFFFFFFFF: none): the walk may stop there with a lower bound.  At most ceil(n / 4) + 1 columns are
// fetched whatever max_distance is: outside the box every cell is alike.
template <class Column, class Best>
BLOK_STAMP_HD uint32_t free_travel(int64_t p, int64_t n, int sign, uint32_t max_distance, bool solid_outside, Column column, Best best) {
    if (max_distance == 0u) return 0u;
    const uint64_t cap = max_distance;
    int64_t c = p + sign;                                         // the first cell looked at: the start cell itself is not
    if (sign > 0 ? c < 0 : c >= n) {                              // still in front of the box
        if (solid_outside) return 0u;
        c = sign > 0 ? 0 : n - 1;
    }
    while (c >= 0 && c < n) {
        const uint64_t dist = static_cast<uint64_t>(sign > 0 ? c - p : p - c);      // >= 1
        if (dist > cap) return max_distance;
        if (dist - 1u >= best()) return static_cast<uint32_t>(dist - 1u);
        const uint32_t f = first_filled(column(c >> 2), static_cast<uint32_t>(c & 3), sign);
        if (f < 4u) {
            const int64_t hit = c + sign * static_cast<int64_t>(f);
            if (hit >= 0 && hit < n) { const uint64_t k = dist - 1u + f; return static_cast<uint32_t>(k < cap ? k : cap); }
        }
        if (sign > 0) { c = ((c >> 2) + 1) * 4; if (c > n) c = n; }     // the next brick's first cell in this direction; the last brick
        else c = (c >> 2) * 4 - 1;                                       // may be partial (n % 4 != 0): the walk leaves the box at n, not past it
    }
    if (!solid_outside) return max_distance;
    const uint64_t k = static_cast<uint64_t>(sign > 0 ? c - p : p - c) - 1u;      // c: the first cell behind the box on the way
    return static_cast<uint32_t>(k < cap ? k : cap);
}

}  // namespace sweep
}  // namespace blok
#endif
