// The miss pixels of a packed frame, written by the walk's own launch (trace_kernels.hip: packed_frame_kernel, packed_frame_own_kernel).
// Plain C++, no HIP: the kernels, the launch functions and tests/host_harness/fill_units_shim.cpp share this arithmetic.
//
// A fill unit is 64 consecutive pixels of one row of the launch rectangle: up to eight octets of 8 pixels, each inside one wave tile, 1 KB
// of records and 256 B of RGBA8 to a wave.  Lane l of unit (row, block) owns pixel (64 block + l, row); it writes that pixel's miss iff the
// pixel is inside the rectangle and its wave tile is empty by the view's finer bounds — the complement of what pack_build_kernel lists.
// The grid has G = max(n_groups, ceil(U / k)) workgroups: the first n_groups walk their group of the list, and workgroup b of all G writes
// the units b, b + G, b + 2G, ... below U — at most k of them once G >= ceil(U / k), so k caps what a walk wave carries.
#pragma once
#include <cstdint>

namespace blok {

constexpr uint32_t kFillUnit = 64u;                     // pixels per unit: one to a lane

struct FillGrid {
    uint32_t units_x;                                   // units per row of the rectangle
    uint32_t n_units;                                   // U = h * units_x
    uint32_t grid;                                      // G
};

constexpr uint32_t fill_units_x(uint32_t w) { return (w + kFillUnit - 1u) / kFillUnit; }

// w, h < 65 535 (pack_applies): U < 2^26.  k >= 1.
constexpr FillGrid fill_grid(uint32_t w, uint32_t h, uint32_t n_groups, uint32_t k) {
    const uint32_t units_x = fill_units_x(w), n_units = h * units_x;
    const uint32_t by_cap = (n_units + k - 1u) / k;
    return FillGrid{units_x, n_units, n_groups > by_cap ? n_groups : by_cap};
}

// Unit u -> its row and the rectangle x of its lane 0.
constexpr uint32_t fill_unit_row(uint32_t u, uint32_t units_x) { return u / units_x; }
constexpr uint32_t fill_unit_x0(uint32_t u, uint32_t units_x) { return (u % units_x) * kFillUnit; }

// The i-th unit of workgroup b (i = 0, 1, ...); the workgroup's units end at the first one that is not below U.
constexpr uint32_t fill_unit_of(uint32_t b, uint32_t i, uint32_t grid) { return b + i * grid; }

}  // namespace blok
