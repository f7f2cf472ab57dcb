// The flood on the host (include/blok_world.h: blok_flood_field, blok_flood_edit): the contracts of blok_hip_volume_flood_field and
// blok_hip_volume_edit_by_flood (blok_hip.h) over host arrays, through the rules the kernels use (../common/flood_core.h).  The field is
// a plain queue BFS over the region's passable cells: it is the definition the device's rounds are held against.
#include "blok_world.h"
#include "../common/flood_core.h"
#include "../common/field_edit_core.h"

#include <cstdint>
#include <vector>

namespace F = blok::flood;

extern "C" {

int blok_flood_field(const float* density, const uint32_t* material_ids, const int32_t origin[3], uint32_t nx, uint32_t ny, uint32_t nz,
                     const int32_t region_lo[3], const int32_t region_hi[3], const int32_t* seeds_xyz, uint64_t n_seeds, uint32_t max_steps,
                     uint32_t flags, uint32_t material, uint16_t* out_field, blok_flood_info* out_info) {
    if (F::check_field_args(seeds_xyz, n_seeds, max_steps, flags) != F::kFine) return BLOK_ERR_INVALID_ARG;
    const uint32_t dims[3] = {nx, ny, nz};
    uint32_t lo[3], hi[3];
    const int rc = blok::region::status(blok::region::local(origin, dims, region_lo, region_hi, lo, hi));
    if (rc != BLOK_OK) return rc;
    if (uint64_t(nx) * ny * nz > 0xFFFFFFFFull) return BLOK_ERR_UNSUPPORTED;
    blok_flood_info info{};
    info.version = 1u; info.flags = flags; info.max_steps = max_steps;
    size_t ext[3];
    for (int a = 0; a < 3; ++a) { ext[a] = hi[a] - lo[a]; info.lo[a] = (origin ? origin[a] : 0) + static_cast<int32_t>(lo[a]); info.ext[a] = hi[a] - lo[a]; }
    // a listed seed outside the region, before anything is written
    for (uint64_t i = 0; i < n_seeds; ++i)
        for (int a = 0; a < 3; ++a) {
            const int64_t c = int64_t(seeds_xyz[3 * i + a]) - info.lo[a];
            if (c < 0 || c >= int64_t(ext[a])) return BLOK_ERR_INVALID_ARG;
        }
    const size_t cells = ext[0] * ext[1] * ext[2];
    if (cells && (!density || !out_field || (F::same_material(flags) && !material_ids))) return BLOK_ERR_INVALID_ARG;
    if (cells) {
        const auto at = [&](size_t x, size_t y, size_t z) { return x + ext[0] * (y + ext[1] * z); };
        std::vector<uint8_t> pass(cells);
        for (size_t z = 0; z < ext[2]; ++z)
            for (size_t y = 0; y < ext[1]; ++y)
                for (size_t x = 0; x < ext[0]; ++x) {
                    const size_t cell = (lo[0] + x) + ((lo[2] + z) * ny + (lo[1] + y)) * nx;
                    pass[at(x, y, z)] = F::passable(F::filled(density[cell]), material_ids ? material_ids[cell] : 0u, flags, material);
                }
        for (size_t i = 0; i < cells; ++i) out_field[i] = static_cast<uint16_t>(F::kFar);
        std::vector<uint32_t> queue;                              // region cell indices, in the order they were reached: distances never decrease along it
        queue.reserve(1024);
        const auto seed = [&](size_t i) { if (pass[i] && out_field[i] != 0u) { out_field[i] = 0u; queue.push_back(static_cast<uint32_t>(i)); } };
        for (uint64_t i = 0; i < n_seeds; ++i)
            seed(at(size_t(seeds_xyz[3 * i] - info.lo[0]), size_t(seeds_xyz[3 * i + 1] - info.lo[1]), size_t(seeds_xyz[3 * i + 2] - info.lo[2])));
        for (uint32_t f = 0; f < 6u; ++f) {
            if (!F::seeds_face(flags, f)) continue;
            const uint32_t a = F::face_axis(f), b = (a + 1u) % 3u, c = (a + 2u) % 3u;
            size_t p[3];
            p[a] = F::face_layer(f, 0u, static_cast<uint32_t>(ext[a]));
            for (p[c] = 0; p[c] < ext[c]; ++p[c])
                for (p[b] = 0; p[b] < ext[b]; ++p[b]) seed(at(p[0], p[1], p[2]));
        }
        const size_t stride[3] = {1u, ext[0], ext[0] * ext[1]};
        for (size_t head = 0; head < queue.size(); ++head) {
            const size_t i = queue[head];
            const uint32_t d = out_field[i];
            const size_t p[3] = {i % ext[0], (i / ext[0]) % ext[1], i / (ext[0] * ext[1])};
            for (int a = 0; a < 3; ++a)
                for (int s = 0; s < 2; ++s) {
                    if (s ? p[a] + 1u >= ext[a] : p[a] == 0u) continue;
                    const size_t j = s ? i + stride[a] : i - stride[a];
                    if (!pass[j]) continue;
                    const uint32_t now = F::relax(out_field[j], d, max_steps);
                    if (now != out_field[j]) { out_field[j] = static_cast<uint16_t>(now); queue.push_back(static_cast<uint32_t>(j)); }
                }
        }
        for (size_t i = 0; i < cells; ++i) {
            const uint32_t d = out_field[i];
            if (d == 0u) ++info.n_seed;
            else if (d != F::kFar) { ++info.n_reached; if (d > info.farthest) info.farthest = d; }
            else if (pass[i]) ++info.n_unreached;
        }
    }
    if (out_info) *out_info = info;
    return BLOK_OK;
}

int blok_flood_edit(float* density, uint32_t* material_ids, const int32_t origin[3], uint32_t nx, uint32_t ny, uint32_t nz, const uint16_t* field,
                    const blok_flood_info* info, int op, uint32_t d, float density_value, uint32_t material, uint64_t* out_n_voxels) {
    if (out_n_voxels) *out_n_voxels = 0;
    if (!info || F::check_edit_args(*info, op, d, density_value) != F::kFine) return BLOK_ERR_INVALID_ARG;
    return blok::field_edit::edit_host(density, material_ids, origin, nx, ny, nz, field, *info, blok::field_edit::flood_rule(op, d, density_value, material), out_n_voxels);
}

}  // extern "C"
