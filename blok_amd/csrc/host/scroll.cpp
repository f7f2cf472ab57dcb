// The scroll of the resident volume on the host (include/blok_world.h: blok_scroll_plan, blok_scroll_voxels): the contract of
// blok_hip_volume_scroll (blok_hip.h) over host arrays, through the rules the kernels use (../common/scroll_core.h).  The move is a loop
// over the new box's rows: a row whose source row lies outside the old box is zeros, any other is zeros with one run of copied cells.
#include "blok_world.h"
#include "../common/scroll_core.h"

#include <cstdint>
#include <cstring>

namespace K = blok::scroll;

extern "C" {

int blok_scroll_plan(const int32_t origin[3], uint32_t nx, uint32_t ny, uint32_t nz, const int32_t delta[3], blok_scroll_info* out_info) {
    if (!nx || !ny || !nz || !out_info) return BLOK_ERR_INVALID_ARG;
    const int32_t o[3] = {origin ? origin[0] : 0, origin ? origin[1] : 0, origin ? origin[2] : 0};
    const uint32_t dims[3] = {nx, ny, nz};
    if (const int rule = K::check_args(o, dims, delta, 0u)) return K::status(rule);
    K::plan(o, dims, delta, out_info);
    return BLOK_OK;
}

int blok_scroll_voxels(const float* density, const uint32_t* material_ids, const int32_t origin[3], uint32_t nx, uint32_t ny, uint32_t nz,
                       const int32_t delta[3], float* out_density, uint32_t* out_material_ids, blok_scroll_info* out_info) {
    if (!density || !material_ids || !out_density || !out_material_ids) return BLOK_ERR_INVALID_ARG;
    blok_scroll_info info;
    const int rc = blok_scroll_plan(origin, nx, ny, nz, delta, &info);
    if (rc != BLOK_OK) return rc;
    const size_t cells = size_t(nx) * ny * nz;
    for (size_t i = 0; i < cells; ++i) info.n_filled_before += density[i] > 0.0f;
    // the run of a row's cells that have a source: x in [x0, x1), from source cells [x0 + delta[0], x1 + delta[0])
    uint32_t x0, x1, first = 0;
    K::kept_range(delta[0], nx, &x0, &x1);
    if (x1 > x0) (void)K::source(x0, delta[0], nx, &first);
    for (uint32_t z = 0; z < nz; ++z)
        for (uint32_t y = 0; y < ny; ++y) {
            float* d_row = out_density + (size_t(z) * ny + y) * nx;
            uint32_t* m_row = out_material_ids + (size_t(z) * ny + y) * nx;
            std::memset(d_row, 0, nx * sizeof(float));
            std::memset(m_row, 0, nx * sizeof(uint32_t));
            uint32_t sy, sz;
            if (x1 <= x0 || !K::source(y, delta[1], ny, &sy) || !K::source(z, delta[2], nz, &sz)) continue;
            const size_t src = (size_t(sz) * ny + sy) * nx + first;
            std::memcpy(d_row + x0, density + src, (x1 - x0) * sizeof(float));                 // (bit patterns: -0.0f and NaN payloads survive)
            std::memcpy(m_row + x0, material_ids + src, (x1 - x0) * sizeof(uint32_t));
            for (uint32_t x = x0; x < x1; ++x) info.n_filled_kept += d_row[x] > 0.0f;
        }
    if (out_info) *out_info = info;
    return BLOK_OK;
}

}  // extern "C"
