// TEST INFRASTRUCTURE: exposes the fill units of a packed frame's one launch in blok_amd/csrc/hip/fill_units.h (pure C++, no HIP) — the
// grid, the units of a workgroup, a unit's row and pixels — to tests/test_packed_fill_host.py, walked the way the kernels walk them
// (trace_kernels.hip: fill_units_of_workgroup).  Built with -DFILL_UNITS_SHIM_MAIN it is a stand-alone program instead (the same sweep, for
// a sanitizer build).
#include "fill_units.h"

#include <cstddef>

extern "C" {
// -> G; through the pointers: U, units per row, the most units any workgroup has, the units met that are not below U (always 0: the walk
// stops there, counted by asking once more), and owners[y * w + x] += 1 for every (workgroup, unit, lane) whose pixel lies in the rectangle;
// outside[0] += 1 for every lane whose pixel does not (the kernel's lane writes nothing).
uint32_t fill_units_walk(uint32_t w, uint32_t h, uint32_t n_groups, uint32_t k, uint32_t* out_units, uint32_t* out_units_x, uint32_t* out_most, uint32_t* out_beyond, uint32_t* owners,
                         uint64_t* outside) {
    const blok::FillGrid g = blok::fill_grid(w, h, n_groups, k);
    uint32_t most = 0u, beyond = 0u;
    for (uint32_t b = 0; b < g.grid; ++b) {
        uint32_t i = 0u;
        for (uint32_t u; (u = blok::fill_unit_of(b, i, g.grid)) < g.n_units; ++i) {
            const uint32_t row = blok::fill_unit_row(u, g.units_x), x0 = blok::fill_unit_x0(u, g.units_x);
            if (row >= h || x0 >= w) { ++beyond; continue; }
            for (uint32_t lane = 0; lane < blok::kFillUnit; ++lane) {
                if (x0 + lane < w) owners[static_cast<size_t>(row) * w + x0 + lane] += 1u;
                else *outside += 1u;
            }
        }
        if (i > most) most = i;
    }
    *out_units = g.n_units; *out_units_x = g.units_x; *out_most = most; *out_beyond = beyond;
    return g.grid;
}
}

#ifdef FILL_UNITS_SHIM_MAIN
#include <stdio.h>
#include <initializer_list>
#include <vector>

int main() {
    unsigned long long mismatches = 0, cases = 0;
    for (uint32_t w : {1u, 7u, 8u, 63u, 64u, 65u, 77u, 200u, 3840u})
        for (uint32_t h : {1u, 8u, 61u, 136u})
            for (uint32_t n_groups : {0u, 1u, 37u, 5000u})
                for (uint32_t k : {1u, 4u, 1000u}) {
                    std::vector<uint32_t> owners(static_cast<size_t>(w) * h, 0u);
                    uint32_t units, units_x, most, beyond;
                    uint64_t outside = 0;
                    const uint32_t grid = fill_units_walk(w, h, n_groups, k, &units, &units_x, &most, &beyond, owners.data(), &outside);
                    const uint32_t by_cap = (units + k - 1u) / k;
                    mismatches += units != h * ((w + 63u) / 64u) || grid != (n_groups > by_cap ? n_groups : by_cap) || most > k || beyond != 0u;
                    mismatches += outside != static_cast<uint64_t>(units) * 64u - static_cast<uint64_t>(w) * h;
                    for (uint32_t c : owners) mismatches += c != 1u;
                    ++cases;
                }
    printf("%llu cases, %llu mismatches\n", cases, mismatches);
    return mismatches ? 1 : 0;
}
#endif
