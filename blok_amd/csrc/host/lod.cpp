// The reduction of a volume to a pyramid of coarser levels on the host (include/blok_world.h: blok_lod_reduce): the contract of
// blok_hip_volume_reduce (blok_hip.h) over host arrays, through the rules the kernels use (../common/lod_core.h).  Brick masks are made
// from density > 0, every brick's exposed cells from its mask and its six neighbours', then level 1 from the bits and the ids, and every
// further level from the planes below it.
#include "blok_world.h"
#include "../common/lod_core.h"
#include "../common/region_core.h"

#include <cstdint>
#include <vector>

namespace K = blok::lod;

extern "C" {

int blok_lod_reduce(const float* density, const uint32_t* material_ids, const int32_t origin[3], uint32_t nx, uint32_t ny, uint32_t nz,
                    const int32_t region_lo[3], const int32_t region_hi[3], uint32_t levels, uint32_t flags, void* out_planes,
                    uint64_t capacity_bytes, blok_lod_info* out_info) {
    if (K::check_args(levels, flags) != 0) return BLOK_ERR_INVALID_ARG;
    const uint32_t dims[3] = {nx, ny, nz};
    uint32_t lo[3], hi[3];
    const int rc = blok::region::status(blok::region::local(origin, dims, region_lo, region_hi, lo, hi));
    if (rc != BLOK_OK) return rc;
    if (uint64_t(nx) * ny * nz > 0xFFFFFFFFull) return BLOK_ERR_UNSUPPORTED;
    const int32_t o[3] = {origin ? origin[0] : 0, origin ? origin[1] : 0, origin ? origin[2] : 0};
    blok_lod_info info;
    K::plan(o, lo, hi, levels, flags, &info);
    const uint64_t bytes = K::total_bytes(info);
    if (!out_planes || !bytes) {                            // the plan alone: the grids, and what the planes take
        if (out_info) *out_info = info;
        return BLOK_OK;
    }
    if (!density || !material_ids || capacity_bytes < bytes) return BLOK_ERR_INVALID_ARG;
    // the brick masks, row-major, and each brick's exposed cells
    const uint32_t nb[3] = {(nx + 3u) / 4u, (ny + 3u) / 4u, (nz + 3u) / 4u};
    std::vector<uint64_t> masks(size_t(nb[0]) * nb[1] * nb[2], 0ull), open(masks.size(), 0ull);
    const auto brick = [&](uint32_t bx, uint32_t by, uint32_t bz) { return bx + (size_t(bz) * nb[1] + by) * nb[0]; };
    for (uint32_t z = 0; z < nz; ++z)
        for (uint32_t y = 0; y < ny; ++y)
            for (uint32_t x = 0; x < nx; ++x)
                if (density[(size_t(z) * ny + y) * nx + x] > 0.0f) masks[brick(x >> 2, y >> 2, z >> 2)] |= 1ull << ((x & 3u) | ((y & 3u) << 2) | ((z & 3u) << 4));
    const auto mask_at = [&](uint32_t bx, uint32_t by, uint32_t bz) { return masks[brick(bx, by, bz)]; };
    for (uint32_t bz = 0; bz < nb[2]; ++bz)
        for (uint32_t by = 0; by < nb[1]; ++by)
            for (uint32_t bx = 0; bx < nb[0]; ++bx) {
                uint64_t m;
                open[brick(bx, by, bz)] = K::brick_exposed(mask_at, bx, by, bz, nb, dims, &m);
            }
    char* base = static_cast<char*>(out_planes);
    for (uint32_t j = 1; j <= levels; ++j) {
        blok_lod_level& L = info.level[j - 1u];
        char* at = base + K::level_offset(info, j);
        uint16_t* out_n = reinterpret_cast<uint16_t*>(at + K::plane_offset(L.n_cells, 0u));
        uint16_t* out_e = reinterpret_cast<uint16_t*>(at + K::plane_offset(L.n_cells, 1u));
        uint32_t* out_id = reinterpret_cast<uint32_t*>(at + K::plane_offset(L.n_cells, 2u));
        K::Below below{};
        if (j >= 2u) below = K::below_of(info, j, base);
        uint64_t i = 0;
        for (uint32_t cz = 0; cz < L.cext[2]; ++cz)
            for (uint32_t cy = 0; cy < L.cext[1]; ++cy)
                for (uint32_t cx = 0; cx < L.cext[0]; ++cx, ++i) {
                    uint32_t n, e, id;
                    if (j >= 2u) K::cell_above(below, cx, cy, cz, flags, &n, &e, &id);
                    else {
                        uint32_t cn[8], ce[8], cid[8];
                        const uint32_t c3[3] = {cx, cy, cz};
                        for (uint32_t c = 0; c < 8u; ++c) {
                            cn[c] = ce[c] = cid[c] = 0u;
                            int64_t v[3];                    // the child, box-local
                            bool in = true;
                            for (int a = 0; a < 3; ++a) {
                                v[a] = 2 * (int64_t(L.clo[a]) + c3[a]) + ((c >> a) & 1u) - o[a];
                                in = in && v[a] >= int64_t(lo[a]) && v[a] < int64_t(hi[a]);
                            }
                            if (!in) continue;
                            const uint32_t x = uint32_t(v[0]), y = uint32_t(v[1]), z = uint32_t(v[2]);
                            const uint32_t bit = (x & 3u) | ((y & 3u) << 2) | ((z & 3u) << 4);
                            const size_t b = brick(x >> 2, y >> 2, z >> 2);
                            cn[c] = uint32_t((masks[b] >> bit) & 1ull);
                            ce[c] = uint32_t((open[b] >> bit) & 1ull);
                            if (cn[c]) cid[c] = material_ids[(size_t(z) * ny + y) * nx + x];
                        }
                        K::cell_of(cn, ce, cid, flags, &n, &e, &id);
                    }
                    out_n[i] = static_cast<uint16_t>(n); out_e[i] = static_cast<uint16_t>(e); out_id[i] = id;
                    L.n_filled += n ? 1u : 0u; L.n_exposed += e ? 1u : 0u; L.sum_n += n; L.sum_e += e;
                }
    }
    if (out_info) *out_info = info;
    return BLOK_OK;
}

}  // extern "C"
