// The light grid on the host (include/blok_world.h: blok_light_grid_build): the contract of blok_hip_build_light_grid (blok_hip.h, "the
// light grid") over a host table, through the functions the kernels use (../common/lights_core.h).  Lights are visited in table order, so
// every list is in ascending table index by construction.
#include "blok_world.h"
#include "../common/lights_core.h"

#include <algorithm>
#include <vector>

namespace L = blok::lights;

extern "C" {

int blok_light_grid_build(const blok_light* lights, uint64_t n, uint32_t cell_log2, uint32_t reach, uint32_t share, uint32_t* out_start,
                          uint32_t* out_faces, blok_light_grid_item* out_items, uint64_t cells_capacity, uint64_t items_capacity,
                          blok_light_grid_info* out_info) {
    if (out_info) *out_info = blok_light_grid_info{};
    if (!lights || n == 0 || !L::grid_params_ok(cell_log2, reach, share)) return BLOK_ERR_INVALID_ARG;
    const bool count_only = !out_start && !out_faces && !out_items;
    if (!count_only && (!out_start || !out_faces || !out_items)) return BLOK_ERR_INVALID_ARG;
    uint64_t faces = 0, index = 0;
    if (const int rule = L::check_table(lights, n, &faces, &index)) return rule == 4 ? BLOK_ERR_UNSUPPORTED : BLOK_ERR_INVALID_ARG;

    blok_light_grid_info info{};
    info.cell_log2 = cell_log2; info.reach = reach; info.share = share;
    L::GridBounds bounds = L::no_bounds();
    for (uint64_t i = 0; i < n; ++i) {
        const L::CellRange r = L::light_cells(lights[i], cell_log2);
        bounds = L::join(bounds, L::GridBounds{{r.lo[0], r.lo[1], r.lo[2]}, {r.hi[0], r.hi[1], r.hi[2]}});
        info.n_items += L::listed_cells(r, reach);
    }
    L::grid_box(bounds, reach, &info);
    if (info.n_cells > L::kGridMaxCells || info.n_items >= L::kGridMaxItems) {
        if (out_info) *out_info = info;
        return BLOK_ERR_UNSUPPORTED;
    }
    info.bytes = L::grid_bytes(info.n_cells, info.n_items);
    if (!count_only && (cells_capacity < info.n_cells || items_capacity < info.n_items)) {
        if (out_info) *out_info = info;
        return BLOK_ERR_INVALID_ARG;
    }
    // the lists' lengths, then their offsets
    std::vector<uint32_t> start(info.n_cells + 1u, 0u);
    for (uint64_t i = 0; i < n; ++i) {
        const L::CellRange r = L::light_cells(lights[i], cell_log2);
        const uint32_t cells = static_cast<uint32_t>(L::listed_cells(r, reach));
        for (uint32_t k = 0; k < cells; ++k) start[L::listed_cell_index(r, reach, k, info.cell_lo, info.dim) + 1u] += 1u;
    }
    for (uint64_t g = 0; g < info.n_cells; ++g) {
        info.n_nonempty += start[g + 1u] ? 1u : 0u;
        info.max_items = std::max(info.max_items, start[g + 1u]);
        start[g + 1u] += start[g];
    }
    if (out_info) *out_info = info;
    if (count_only) return BLOK_OK;
    // the items: a cursor per cell, the running face sum of a list in out_faces
    std::vector<uint32_t> cursor(start.begin(), start.end() - 1);
    std::fill(out_faces, out_faces + info.n_cells, 0u);
    for (uint64_t i = 0; i < n; ++i) {
        const L::CellRange r = L::light_cells(lights[i], cell_log2);
        const uint32_t cells = static_cast<uint32_t>(L::listed_cells(r, reach)), area = lights[i].du * lights[i].dv;
        for (uint32_t k = 0; k < cells; ++k) {
            const uint32_t g = L::listed_cell_index(r, reach, k, info.cell_lo, info.dim);
            out_items[cursor[g]++] = blok_light_grid_item{static_cast<uint32_t>(i), out_faces[g]};
            out_faces[g] += area;
        }
    }
    std::copy(start.begin(), start.end(), out_start);
    return BLOK_OK;
}

}  // extern "C"
