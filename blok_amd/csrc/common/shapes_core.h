// The rules of blok_hip_volume_apply_shapes (include/blok_hip.h), each defined once: the limits of a record, the inside test
// of the four kinds, the voxel box of a shape, the seven operations.  Included by the kernels (../hip/shapes_kernels.hip), by the entry and
// by the host build (../host/shapes.cpp).  No HIP types; every product is 64-bit and below 2^63 by the limits (see the bounds at inside()).
// All coordinates are in half-voxel units: the centre of world voxel w is c = 2 w + 1.
#ifndef BLOK_SHAPES_CORE_H
#define BLOK_SHAPES_CORE_H
#include <stdint.h>

#include "blok_hip.h"

#if defined(__HIPCC__)
#define BLOK_SHAPES_HD __host__ __device__ inline
#else
#define BLOK_SHAPES_HD inline
#endif

namespace blok {
namespace shapes {

constexpr int64_t kCoordMax = 1 << 17;       // |a|, |b|
constexpr int64_t kRadiusMax = 1024;         // 512 voxels
constexpr int64_t kSpanMax = 4096;           // |b - a| per axis of a capsule or cylinder

// ---- limits -----------------------------------------------------------------------------------------------------------------------------
// 0 = the record is within the limits, else the number of the first rule it breaks (rule_text).
enum Rule { kOk = 0, kKind, kOp, kReserved, kCoord, kRadius, kUnused, kBoxOrder, kSpan, kCylinder, kValueFinite, kValuePositive };

BLOK_SHAPES_HD bool finite(float v) {          // (no <cmath>: the bits say it)
    uint32_t u;
    __builtin_memcpy(&u, &v, sizeof u);
    return (u & 0x7F800000u) != 0x7F800000u;
}

BLOK_SHAPES_HD int check(const blok_shape& s) {
    if (s.kind > BLOK_SHAPE_CYLINDER) return kKind;
    if (s.op > BLOK_SHAPE_SUBTRACT) return kOp;
    if (s.reserved[0] || s.reserved[1]) return kReserved;
    for (int k = 0; k < 3; ++k) {
        if (s.a[k] < -kCoordMax || s.a[k] > kCoordMax || s.b[k] < -kCoordMax || s.b[k] > kCoordMax) return kCoord;
        if (s.r[k] > kRadiusMax) return kRadius;
    }
    if (s.kind == BLOK_SHAPE_BOX) {
        if (s.r[0] || s.r[1] || s.r[2]) return kUnused;
        for (int k = 0; k < 3; ++k) if (s.a[k] > s.b[k]) return kBoxOrder;
    } else if (s.kind == BLOK_SHAPE_ELLIPSOID) {
        if (s.b[0] || s.b[1] || s.b[2]) return kUnused;
    } else {
        if (s.r[1] || s.r[2]) return kUnused;
        bool same = true;
        for (int k = 0; k < 3; ++k) {
            const int64_t d = int64_t(s.b[k]) - s.a[k];
            if (d < -kSpanMax || d > kSpanMax) return kSpan;
            same = same && d == 0;
        }
        if (s.kind == BLOK_SHAPE_CYLINDER && same) return kCylinder;
    }
    if (!finite(s.value)) return kValueFinite;
    if ((s.op == BLOK_SHAPE_SET || s.op == BLOK_SHAPE_KEEP) && !(s.value > 0.0f)) return kValuePositive;
    return kOk;
}

inline const char* rule_text(int rule) {
    static const char* const kText[] = {"", "unknown kind", "unknown op", "reserved words are not zero", "a or b outside [-2^17, 2^17]", "a radius above 1024",
                                        "a field the kind does not use is not zero", "box with a > b", "|b - a| above 4096 on an axis",
                                        "cylinder with a == b", "value is not finite", "value must be > 0 for SET and KEEP"};
    return kText[rule];
}

// ---- the box of a shape -----------------------------------------------------------------------------------------------------------------
BLOK_SHAPES_HD int64_t floor_half(int64_t v) { return (v >= 0 ? v : v - 1) / 2; }      // floor(v / 2), at negative v too

// The extent of the shape along axis k, half-voxel units, both ends included: every inside centre has lo <= c[k] <= hi.
BLOK_SHAPES_HD void extent(const blok_shape& s, int k, int64_t& lo, int64_t& hi) {
    if (s.kind == BLOK_SHAPE_BOX) { lo = s.a[k]; hi = s.b[k]; }
    else if (s.kind == BLOK_SHAPE_ELLIPSOID) { lo = int64_t(s.a[k]) - s.r[k]; hi = int64_t(s.a[k]) + s.r[k]; }
    else {
        const int64_t a = s.a[k], b = s.b[k];
        lo = (a < b ? a : b) - s.r[0]; hi = (a < b ? b : a) + s.r[0];
    }
}

// The voxel box of a shape, world voxels, half open: the smallest w has 2 w + 1 >= lo, the largest 2 w + 1 <= hi.  The only place that
// derives it.  (May be empty: a box between two voxel centres.)
BLOK_SHAPES_HD void bounds(const blok_shape& s, int64_t lo[3], int64_t hi[3]) {
    for (int k = 0; k < 3; ++k) {
        int64_t e0, e1;
        extent(s, k, e0, e1);
        lo[k] = floor_half(e0);                // = ceil((e0 - 1) / 2)
        hi[k] = floor_half(e1 - 1) + 1;
    }
}

// ---- inside -----------------------------------------------------------------------------------------------------------------------------
// Whether the voxel centre c (= 2 w + 1 per axis) lies inside a shape that has passed check().  The extent is tested first, for every kind:
// it holds for every inside centre (|dx_k| <= r_k is the ellipsoid's own rule; a capsule lies within r of its segment, and a cylinder
// within its capsule), so it changes no answer, and behind it the products are bounded whatever c the caller passes:
//  - ellipsoid: dx_k^2 <= 2^20 and the product of two r^2 <= 2^40, so the sum is below 3 * 2^60;
//  - capsule, cylinder: |p_k| <= 4096 + 1024 < 2^13, so |p|^2 < 2^28, dd <= 3 * 2^24 < 2^26, |s| < 2^27: |p|^2 dd, s^2 and r^2 dd are below 2^54.
BLOK_SHAPES_HD bool inside(const blok_shape& s, int64_t cx, int64_t cy, int64_t cz) {
    const int64_t c[3] = {cx, cy, cz};
    for (int k = 0; k < 3; ++k) {
        int64_t lo, hi;
        extent(s, k, lo, hi);
        if (c[k] < lo || c[k] > hi) return false;
    }
    if (s.kind == BLOK_SHAPE_BOX) return true;
    if (s.kind == BLOK_SHAPE_ELLIPSOID) {
        const int64_t x = cx - s.a[0], y = cy - s.a[1], z = cz - s.a[2];
        const int64_t rx = int64_t(s.r[0]) * s.r[0], ry = int64_t(s.r[1]) * s.r[1], rz = int64_t(s.r[2]) * s.r[2];
        return x * x * (ry * rz) + y * y * (rx * rz) + z * z * (rx * ry) <= rx * ry * rz;
    }
    const int64_t dx = int64_t(s.b[0]) - s.a[0], dy = int64_t(s.b[1]) - s.a[1], dz = int64_t(s.b[2]) - s.a[2];
    const int64_t px = cx - s.a[0], py = cy - s.a[1], pz = cz - s.a[2];
    const int64_t dd = dx * dx + dy * dy + dz * dz, ss = px * dx + py * dy + pz * dz, pp = px * px + py * py + pz * pz;
    const int64_t rr = int64_t(s.r[0]) * s.r[0];
    if (s.kind == BLOK_SHAPE_CYLINDER) return ss >= 0 && ss <= dd && pp * dd - ss * ss <= rr * dd;
    if (dd == 0 || ss <= 0) return pp <= rr;
    if (ss >= dd) {
        const int64_t qx = cx - s.b[0], qy = cy - s.b[1], qz = cz - s.b[2];
        return qx * qx + qy * qy + qz * qz <= rr;
    }
    return pp * dd - ss * ss <= rr * dd;
}

// ---- the operations ---------------------------------------------------------------------------------------------------------------------
// One voxel inside the shape: (d, m) before -> after.  True = the rule writes (counted), whether or not a bit changes.  Densities are copied
// or selected, never computed: -0.0f and NaN payloads survive ADD and SUBTRACT as std::max / std::min leave them.
BLOK_SHAPES_HD bool apply(const blok_shape& s, float& d, uint32_t& m) {
    const bool filled = d > 0.0f;
    switch (s.op) {
        case BLOK_SHAPE_SET: d = s.value; m = s.material; return true;
        case BLOK_SHAPE_KEEP: if (filled) return false; d = s.value; m = s.material; return true;
        case BLOK_SHAPE_ERASE: d = 0.0f; m = 0u; return true;
        case BLOK_SHAPE_PAINT: if (!filled) return false; m = s.material; return true;
        case BLOK_SHAPE_REPLACE: if (!filled || m != s.match) return false; m = s.material; return true;
        case BLOK_SHAPE_ADD: d = d < s.value ? s.value : d; return true;
        default: d = s.value < d ? s.value : d; return true;      // BLOK_SHAPE_SUBTRACT
    }
}

// Whether the operation can make an empty voxel filled (gpu_build.h: Edit::MayFill).
BLOK_SHAPES_HD bool may_fill(const blok_shape& s) {
    return s.op == BLOK_SHAPE_SET || s.op == BLOK_SHAPE_KEEP || (s.op == BLOK_SHAPE_ADD && s.value > 0.0f);
}

}  // namespace shapes
}  // namespace blok
#endif
