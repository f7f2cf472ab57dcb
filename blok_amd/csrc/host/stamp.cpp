// Models into a voxel volume and back on the host (include/blok_world.h: blok_stamp_voxels, blok_capture_voxels): the contracts of
// blok_hip_volume_stamp_models and blok_hip_volume_capture_model (blok_hip.h) over host arrays, through the arithmetic the kernel uses
// (../common/stamp_core.h).
#include "blok_world.h"
#include "../common/stamp_core.h"

#include <algorithm>
#include <cmath>
#include <cstdint>
#include <vector>

namespace S = blok::stamp;

extern "C" {

int blok_stamp_voxels(float* density, uint32_t* material_ids, const int32_t origin[3], uint32_t nx, uint32_t ny, uint32_t nz,
                      const int32_t* model_xyz, const uint32_t* model_materials, size_t n,
                      const blok_instance* placement, int mode, float value, uint64_t* out_n_voxels) {
    if (out_n_voxels) *out_n_voxels = 0;
    if (!placement || !S::well_formed(*placement) || !S::mode_known(mode)) return BLOK_ERR_INVALID_ARG;
    if (mode != BLOK_STAMP_ERASE && (!std::isfinite(value) || !(value > 0.0f))) return BLOK_ERR_INVALID_ARG;
    if (n && (!model_xyz || (mode != BLOK_STAMP_ERASE && !model_materials))) return BLOK_ERR_INVALID_ARG;
    if (uint64_t(nx) * ny * nz > 0xFFFFFFFFull) return BLOK_ERR_UNSUPPORTED;
    if (n == 0) return BLOK_OK;
    if (!density || !material_ids) return BLOK_ERR_INVALID_ARG;
    const blok_instance& I = *placement;
    const int64_t dims[3] = {nx, ny, nz};
    const int64_t org[3] = {origin ? origin[0] : 0, origin ? origin[1] : 0, origin ? origin[2] : 0};
    // the voxels that land inside the box, as (cell index, list index)
    struct Hit { uint64_t cell; size_t at; };
    std::vector<Hit> hits;
    hits.reserve(n);
    for (size_t i = 0; i < n; ++i) {
        int64_t w[3] = {0, 0, 0};
        for (uint32_t k = 0; k < 3u; ++k) w[I.axis[k]] = S::to_world(I, k, model_xyz[3 * i + k]) - org[I.axis[k]];
        if (w[0] < 0 || w[1] < 0 || w[2] < 0 || w[0] >= dims[0] || w[1] >= dims[1] || w[2] >= dims[2]) continue;
        hits.push_back(Hit{uint64_t(w[0] + (w[1] + w[2] * dims[1]) * dims[0]), i});
    }
    // the mapping is a bijection, so two entries share a cell only when the list names a voxel twice: the last one wins
    std::stable_sort(hits.begin(), hits.end(), [](const Hit& a, const Hit& b) { return a.cell < b.cell; });
    uint64_t written = 0;
    for (size_t j = 0; j < hits.size(); ++j) {
        if (j + 1 < hits.size() && hits[j + 1].cell == hits[j].cell) continue;
        float d; uint32_t m;
        if (!S::apply(mode, value, model_materials ? model_materials[hits[j].at] : 0u, density[hits[j].cell], d, m)) continue;
        density[hits[j].cell] = d;
        material_ids[hits[j].cell] = m;
        ++written;
    }
    if (out_n_voxels) *out_n_voxels = written;
    return BLOK_OK;
}

int blok_capture_voxels(const float* density, const uint32_t* material_ids, const int32_t origin[3], uint32_t nx, uint32_t ny, uint32_t nz,
                        const int32_t region_lo[3], const int32_t region_hi[3], int32_t* xyz_out, uint32_t* materials_out,
                        uint64_t capacity, uint64_t* out_n) {
    if (out_n) *out_n = 0;
    if ((region_lo == nullptr) != (region_hi == nullptr)) return BLOK_ERR_INVALID_ARG;
    const int64_t dims[3] = {nx, ny, nz};
    const int64_t org[3] = {origin ? origin[0] : 0, origin ? origin[1] : 0, origin ? origin[2] : 0};
    int64_t lo[3], hi[3];
    for (int a = 0; a < 3; ++a) {
        lo[a] = region_lo ? int64_t(region_lo[a]) - org[a] : 0;
        hi[a] = region_hi ? int64_t(region_hi[a]) - org[a] : dims[a];
        if (lo[a] > hi[a]) return BLOK_ERR_INVALID_ARG;
    }
    for (int a = 0; a < 3; ++a) if (lo[a] < 0 || hi[a] > dims[a]) return BLOK_ERR_UNSUPPORTED;
    if (uint64_t(nx) * ny * nz > 0xFFFFFFFFull) return BLOK_ERR_UNSUPPORTED;
    if (lo[0] == hi[0] || lo[1] == hi[1] || lo[2] == hi[2]) return BLOK_OK;
    if (!density || (xyz_out && materials_out && !material_ids)) return BLOK_ERR_INVALID_ARG;
    uint64_t count = 0;
    for (int64_t z = lo[2]; z < hi[2]; ++z)
        for (int64_t y = lo[1]; y < hi[1]; ++y)
            for (int64_t x = lo[0]; x < hi[0]; ++x) {
                const size_t cell = static_cast<size_t>(x + (y + z * dims[1]) * dims[0]);
                if (!S::filled(density[cell])) continue;
                if (xyz_out && count < capacity) {
                    xyz_out[3 * count] = int32_t(x - lo[0]); xyz_out[3 * count + 1] = int32_t(y - lo[1]); xyz_out[3 * count + 2] = int32_t(z - lo[2]);
                    if (materials_out) materials_out[count] = material_ids[cell];
                }
                ++count;
            }
    if (out_n) *out_n = count;
    return BLOK_OK;
}

}  // extern "C"
