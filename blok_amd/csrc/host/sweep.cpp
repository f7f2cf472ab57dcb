// A placed model swept against a voxel volume on the host (include/blok_world.h: blok_sweep_voxels): the contract of
// blok_hip_volume_sweep_models (blok_hip.h) over host arrays and a voxel list, through the arithmetic the kernel uses
// (../common/sweep_core.h, ../common/stamp_core.h).  Voxel by voxel: every voxel walks its own column, nothing is skipped.
#include "blok_world.h"
#include "../common/sweep_core.h"

#include <algorithm>
#include <cstdint>

namespace S = blok::stamp;
namespace W = blok::sweep;

extern "C" {

int blok_sweep_voxels(const float* density, const int32_t origin[3], uint32_t nx, uint32_t ny, uint32_t nz, const int32_t* model_xyz, size_t n,
                      const blok_instance* placement, uint32_t direction, uint32_t max_distance, uint32_t flags, blok_sweep_result* out_result) {
    if (!placement || !S::well_formed(*placement) || !W::direction_known(direction) || !W::flags_known(flags) || !out_result) return BLOK_ERR_INVALID_ARG;
    if (n && !model_xyz) return BLOK_ERR_INVALID_ARG;
    if (uint64_t(nx) * ny * nz > 0xFFFFFFFFull) return BLOK_ERR_UNSUPPORTED;
    if (n && !density && uint64_t(nx) * ny * nz != 0u) return BLOK_ERR_INVALID_ARG;
    const blok_instance& I = *placement;
    const int64_t dims[3] = {nx, ny, nz};
    const int64_t org[3] = {origin ? origin[0] : 0, origin ? origin[1] : 0, origin ? origin[2] : 0};
    const uint32_t axis = W::direction_axis(direction);
    const int sign = W::direction_sign(direction);
    const bool solid = W::outside_filled(flags);
    const int64_t strides[3] = {1, dims[0], dims[0] * dims[1]};
    uint64_t n_overlap = 0;
    uint32_t travel = max_distance;
    for (size_t i = 0; i < n; ++i) {
        int64_t w[3] = {0, 0, 0};
        for (uint32_t k = 0; k < 3u; ++k) w[I.axis[k]] = S::to_world(I, k, model_xyz[3 * i + k]) - org[I.axis[k]];
        bool in[3];
        for (int a = 0; a < 3; ++a) in[a] = w[a] >= 0 && w[a] < dims[a];
        const bool in_column = (axis == 0u || in[0]) && (axis == 1u || in[1]) && (axis == 2u || in[2]);
        const bool here = in[0] && in[1] && in[2] ? S::filled(density[w[0] + w[1] * strides[1] + w[2] * strides[2]]) : solid;
        n_overlap += here ? 1u : 0u;
        uint32_t k_free;
        if (!in_column) k_free = solid ? 0u : max_distance;
        else {
            // the 4-bit column of cells 4 b .. 4 b + 3 along the axis, from the densities (cells past the box's end read as empty)
            const int64_t base = w[0] * strides[0] + w[1] * strides[1] + w[2] * strides[2] - w[axis] * strides[axis];
            k_free = W::free_travel(w[axis], dims[axis], sign, max_distance, solid,
                [&](int64_t b) {
                    uint32_t column = 0;
                    for (int64_t j = 0; j < 4; ++j)
                        if (4 * b + j < dims[axis] && S::filled(density[base + (4 * b + j) * strides[axis]])) column |= 1u << j;
                    return column;
                },
                []() { return 0xFFFFFFFFu; });
        }
        travel = std::min(travel, k_free);
    }
    out_result->n_overlap = n_overlap;
    out_result->travel = travel;
    out_result->blocked = travel < max_distance ? 1u : 0u;
    return BLOK_OK;
}

}  // extern "C"
