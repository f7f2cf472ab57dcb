// Procedural terrain on the host (include/blok_world.h: blok_terrain_*): the function of blok_hip_volume_generate_terrain through the
// same header the kernels include (../common/terrain_core.h), voxel by voxel.
#include "blok_world.h"
#include "../common/terrain_core.h"

#include <algorithm>
#include <cstdint>
#include <vector>

namespace T = blok::terrain;

extern "C" {

int blok_terrain_default_params(uint32_t n, uint32_t seed, blok_terrain_params* out) {
    if (!out || n == 0u || n > 65536u) return BLOK_ERR_INVALID_ARG;
    uint32_t log2n = 0;
    while ((2u << log2n) <= n) ++log2n;
    blok_terrain_params p{};
    p.seed = seed;
    p.base_height = static_cast<int32_t>(n / 8u);
    p.amplitude = std::max(1u, 3u * n / 8u);
    p.height_cell_log2 = std::clamp<uint32_t>(log2n > 2u ? log2n - 2u : 0u, 2u, 12u);      // hills a quarter of the box wide
    p.height_octaves = std::min(4u, p.height_cell_log2 + 1u);
    p.cave_cell_log2 = std::clamp<uint32_t>(log2n > 4u ? log2n - 4u : 0u, 3u, 12u);
    p.cave_octaves = 2u;
    p.cave_threshold = 22000u;
    p.cave_roof = 3u;
    p.soil_depth = 3u;
    p.ore_cell_log2 = 3u;
    p.ore_threshold = 52000u;
    p.surface_material = 1u; p.soil_material = 2u; p.rock_material = 3u; p.ore_material = 4u;
    p.density = 1.0f;
    p.flags = 0u;
    *out = p;
    return BLOK_OK;
}

int blok_terrain_validate(const blok_terrain_params* params) {
    return params && T::check_params(*params) == 0 ? BLOK_OK : BLOK_ERR_INVALID_ARG;
}

int blok_terrain_height(const blok_terrain_params* params, const int32_t* xz, size_t n, int32_t* out) {
    if (blok_terrain_validate(params) != BLOK_OK || (n && (!xz || !out))) return BLOK_ERR_INVALID_ARG;
    for (size_t i = 0; i < n; ++i) out[i] = T::height(*params, xz[2 * i], xz[2 * i + 1]);
    return BLOK_OK;
}

int blok_terrain_eval(const blok_terrain_params* params, const int32_t lo[3], const int32_t hi[3], float* density, uint32_t* ids,
                      uint64_t* out_n_voxels) {
    if (out_n_voxels) *out_n_voxels = 0;
    if (blok_terrain_validate(params) != BLOK_OK || !lo || !hi) return BLOK_ERR_INVALID_ARG;
    for (int a = 0; a < 3; ++a) if (lo[a] > hi[a]) return BLOK_ERR_INVALID_ARG;
    const blok_terrain_params& p = *params;
    const int64_t nx = int64_t(hi[0]) - lo[0], ny = int64_t(hi[1]) - lo[1], nz = int64_t(hi[2]) - lo[2];
    if (nx == 0 || ny == 0 || nz == 0) return BLOK_OK;
    if (!density || !ids) return BLOK_ERR_INVALID_ARG;
    const bool shell = p.flags & BLOK_TERRAIN_SHELL, closed = p.flags & BLOK_TERRAIN_CLOSE_SIDES, add = p.flags & BLOK_TERRAIN_ADD;
    // solid() over the region and, for SHELL, one voxel around it: index (x + 1) + ((y + 1) + (z + 1) * ay) * ax with apron a = 1
    const int64_t a = shell ? 1 : 0, ax = nx + 2 * a, ay = ny + 2 * a, az = nz + 2 * a;
    std::vector<int32_t> H(static_cast<size_t>(ax * az));
    for (int64_t z = 0; z < az; ++z)
        for (int64_t x = 0; x < ax; ++x)
            H[static_cast<size_t>(x + z * ax)] = T::height(p, T::step(lo[0], static_cast<int32_t>(x - a)), T::step(lo[2], static_cast<int32_t>(z - a)));
    std::vector<uint8_t> S(static_cast<size_t>(ax * ay * az));
    T::Walker w;
    T::walker_reset(w);
    for (int64_t z = 0; z < az; ++z)
        for (int64_t y = 0; y < ay; ++y)
            for (int64_t x = 0; x < ax; ++x) {
                const bool outside_xz = x < a || x >= a + nx || z < a || z >= a + nz;
                const int32_t X = T::step(lo[0], static_cast<int32_t>(x - a)), Y = T::step(lo[1], static_cast<int32_t>(y - a)), Z = T::step(lo[2], static_cast<int32_t>(z - a));
                S[static_cast<size_t>(x + (y + z * ay) * ax)] = (closed && outside_xz) ? 0 : T::solid(p, w, X, Y, Z, H[static_cast<size_t>(x + z * ax)]);
            }
    uint64_t written = 0;
    for (int64_t z = 0; z < nz; ++z)
        for (int64_t y = 0; y < ny; ++y)
            for (int64_t x = 0; x < nx; ++x) {
                const size_t s = static_cast<size_t>((x + a) + ((y + a) + (z + a) * ay) * ax);
                bool fill = S[s];
                if (fill && shell)
                    fill = !(S[s - 1] && S[s + 1] && S[s - static_cast<size_t>(ax)] && S[s + static_cast<size_t>(ax)] &&
                             S[s - static_cast<size_t>(ax * ay)] && S[s + static_cast<size_t>(ax * ay)]);
                const size_t o = static_cast<size_t>(x + (y + z * ny) * nx);
                if (fill) {
                    density[o] = p.density;
                    ids[o] = T::material(p, w, T::step(lo[0], static_cast<int32_t>(x)), T::step(lo[1], static_cast<int32_t>(y)), T::step(lo[2], static_cast<int32_t>(z)),
                                         H[static_cast<size_t>((x + a) + (z + a) * ax)]);
                    ++written;
                } else if (!add) {
                    density[o] = 0.0f;
                    ids[o] = 0u;
                }
            }
    if (out_n_voxels) *out_n_voxels = written;
    return BLOK_OK;
}

}  // extern "C"
