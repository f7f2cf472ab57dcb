// The reduction of a volume to a pyramid of coarser levels on the host (include/blok_world.h: blok_lod_reduce): the contract of
// blok_hip_volume_reduce (blok_hip.h) over host arrays, through the rules the kernels use (../common/lod_core.h).  Brick masks are made
// from density > 0, every brick's exposed cells from its mask and its six neighbours', then level 1 from the bits and the ids, and every
// further level from the planes below it.
// blok_terrain_reduce is the contract of blok_hip_terrain_reduce: level 1 from the terrain function, tile by tile through the column words
// the kernel uses (../common/terrain_lod_core.h), no voxel array anywhere; the further levels are the same loop.
#include "blok_world.h"
#include "../common/lod_core.h"
#include "../common/region_core.h"
#include "../common/terrain_lod_core.h"

#include <cstdint>
#include <vector>

namespace K = blok::lod;
namespace T = blok::terrain;
namespace TL = blok::terrain_lod;

namespace {

// The planes of every level of `info` into `base`, and the counts into the info: level 1 by level1(cx, cy, cz) -> cell, called in any order
// the producer likes through each_cell(visit), every further level from the planes below it.
struct Cell {
    uint32_t n, e, id;
};
template <class EachLevel1Cell>
void fill_levels(blok_lod_info& info, char* base, uint32_t flags, const EachLevel1Cell& each_level1_cell) {
    for (uint32_t j = 1; j <= info.levels; ++j) {
        blok_lod_level& L = info.level[j - 1u];
        char* at = base + K::level_offset(info, j);
        uint16_t* out_n = reinterpret_cast<uint16_t*>(at + K::plane_offset(L.n_cells, 0u));
        uint16_t* out_e = reinterpret_cast<uint16_t*>(at + K::plane_offset(L.n_cells, 1u));
        uint32_t* out_id = reinterpret_cast<uint32_t*>(at + K::plane_offset(L.n_cells, 2u));
        const auto put = [&](uint32_t cx, uint32_t cy, uint32_t cz, const Cell& c) {
            const uint64_t i = cx + L.cext[0] * (cy + uint64_t(L.cext[1]) * cz);
            out_n[i] = static_cast<uint16_t>(c.n); out_e[i] = static_cast<uint16_t>(c.e); out_id[i] = c.id;
            L.n_filled += c.n ? 1u : 0u; L.n_exposed += c.e ? 1u : 0u; L.sum_n += c.n; L.sum_e += c.e;
        };
        if (j == 1u) { each_level1_cell(put); continue; }
        const K::Below below = K::below_of(info, j, base);
        for (uint32_t cz = 0; cz < L.cext[2]; ++cz)
            for (uint32_t cy = 0; cy < L.cext[1]; ++cy)
                for (uint32_t cx = 0; cx < L.cext[0]; ++cx) {
                    Cell c;
                    K::cell_above(below, cx, cy, cz, flags, &c.n, &c.e, &c.id);
                    put(cx, cy, cz, c);
                }
    }
}

// One tile of the terrain's level 1 (terrain_lod_core.h): the column words of the tile at world (x0, y0, z0) and of its halo.
struct Tile {
    std::vector<TL::Column> column = std::vector<TL::Column>(TL::kCols);
    std::vector<int32_t> height = std::vector<int32_t>(TL::kCols);
    std::vector<TL::Words> words = std::vector<TL::Words>(TL::kInner);

    static uint32_t halo_index(uint32_t i) { return (i % TL::kTileX + 1u) + (i / TL::kTileX + 1u) * TL::kColsX; }

    void build(const blok_terrain_params& p, const int32_t lo[3], const int32_t hi[3], uint32_t flags, int32_t x0, int32_t y0, int32_t z0) {
        const int32_t grow = (flags & BLOK_LOD_SEAMLESS) ? 1 : 0;
        T::Walker w;
        for (uint32_t c = 0; c < TL::kCols; ++c) {
            const uint32_t hx = c % TL::kColsX, hz = c / TL::kColsX;
            const int32_t X = x0 - 1 + static_cast<int32_t>(hx), Z = z0 - 1 + static_cast<int32_t>(hz);
            const bool corner = (hx == 0u || hx == TL::kColsX - 1u) && (hz == 0u || hz == TL::kColsZ - 1u);
            column[c] = TL::outside(); height[c] = 0;
            if (corner || X < lo[0] - grow || X >= hi[0] + grow || Z < lo[2] - grow || Z >= hi[2] + grow) continue;
            height[c] = T::height(p, X, Z);
            T::walker_reset(w);
            column[c] = TL::column_solid(p, w, X, Z, height[c], y0, lo[1] - grow, hi[1] + grow);
        }
        const uint64_t rows = TL::rows_in(y0, lo[1], hi[1]);
        for (uint32_t i = 0; i < TL::kInner; ++i) {
            const uint32_t c = halo_index(i);
            const int32_t X = x0 + static_cast<int32_t>(i % TL::kTileX), Z = z0 + static_cast<int32_t>(i / TL::kTileX);
            TL::Words& s = words[i];
            s.filled = (X >= lo[0] && X < hi[0] && Z >= lo[2] && Z < hi[2]) ? column[c].solid & rows : 0ull;
            s.exposed = TL::exposed(s.filled, column[c], column[c - 1u].solid, column[c + 1u].solid, column[c - TL::kColsX].solid, column[c + TL::kColsX].solid);
            TL::depth_words(height[c], y0, p.soil_depth, &s.soil, &s.deep);
        }
        for (uint32_t i = 0; i < TL::kInner; ++i) {
            const uint64_t cell_exposed = words[i].exposed | words[i ^ 1u].exposed | words[i ^ TL::kTileX].exposed | words[i ^ 1u ^ TL::kTileX].exposed;
            const uint64_t want = TL::voters(words[i].filled, words[i].exposed, cell_exposed, flags) & words[i].deep;
            T::walker_reset(w);
            words[i].ore = TL::column_ore(p, w, x0 + static_cast<int32_t>(i % TL::kTileX), z0 + static_cast<int32_t>(i / TL::kTileX), height[halo_index(i)], y0, want);
        }
    }
};

}  // namespace

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
    const blok_lod_level& L1 = info.level[0];
    const auto level1 = [&](uint32_t cx, uint32_t cy, uint32_t cz) {
        uint32_t cn[8], ce[8], cid[8];
        const uint32_t c3[3] = {cx, cy, cz};
        for (uint32_t c = 0; c < 8u; ++c) {
            cn[c] = ce[c] = cid[c] = 0u;
            int64_t v[3];                    // the child, box-local
            bool in = true;
            for (int a = 0; a < 3; ++a) {
                v[a] = 2 * (int64_t(L1.clo[a]) + c3[a]) + ((c >> a) & 1u) - o[a];
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
        Cell out;
        K::cell_of(cn, ce, cid, flags, &out.n, &out.e, &out.id);
        return out;
    };
    fill_levels(info, static_cast<char*>(out_planes), flags, [&](const auto& put) {
        for (uint32_t cz = 0; cz < L1.cext[2]; ++cz)
            for (uint32_t cy = 0; cy < L1.cext[1]; ++cy)
                for (uint32_t cx = 0; cx < L1.cext[0]; ++cx) put(cx, cy, cz, level1(cx, cy, cz));
    });
    if (out_info) *out_info = info;
    return BLOK_OK;
}

int blok_terrain_reduce(const blok_terrain_params* params, const int32_t region_lo[3], const int32_t region_hi[3], uint32_t levels, uint32_t flags,
                        void* out_planes, uint64_t capacity_bytes, blok_lod_info* out_info) {
    if (!params || T::check_params(*params) != 0 || params->flags != 0u) return BLOK_ERR_INVALID_ARG;
    if (K::check_args(levels, flags, TL::kFlags) != 0 || !region_lo || !region_hi) return BLOK_ERR_INVALID_ARG;
    if (const int rc = TL::check_region(region_lo, region_hi)) return rc;
    blok_lod_info info;
    TL::plan(region_lo, region_hi, levels, flags, &info);
    const uint64_t bytes = K::total_bytes(info);
    if (!out_planes || !bytes) {                            // the plan alone: the grids, and what the planes take
        if (out_info) *out_info = info;
        return BLOK_OK;
    }
    if (capacity_bytes < bytes) return BLOK_ERR_INVALID_ARG;
    // level 1 tile by tile, as the kernel's workgroups take it
    const blok_lod_level& L1 = info.level[0];
    const uint32_t cells[3] = {TL::kTileX / 2u, TL::kSlab / 2u, TL::kTileZ / 2u};
    Tile tile;
    fill_levels(info, static_cast<char*>(out_planes), flags, [&](const auto& put) {
        for (uint32_t tz = 0; tz * cells[2] < L1.cext[2]; ++tz)
            for (uint32_t ty = 0; ty * cells[1] < L1.cext[1]; ++ty)
                for (uint32_t tx = 0; tx * cells[0] < L1.cext[0]; ++tx) {
                    tile.build(*params, region_lo, region_hi, flags, 2 * L1.clo[0] + static_cast<int32_t>(tx * TL::kTileX), 2 * L1.clo[1] + static_cast<int32_t>(ty * TL::kSlab),
                               2 * L1.clo[2] + static_cast<int32_t>(tz * TL::kTileZ));
                    for (uint32_t lz = 0; lz < cells[2] && tz * cells[2] + lz < L1.cext[2]; ++lz)
                        for (uint32_t lx = 0; lx < cells[0] && tx * cells[0] + lx < L1.cext[0]; ++lx) {
                            TL::Words col[4];
                            for (uint32_t q = 0; q < 4u; ++q) col[q] = tile.words[2u * lx + (q & 1u) + (2u * lz + (q >> 1)) * TL::kTileX];
                            for (uint32_t pair = 0; pair < cells[1] && ty * cells[1] + pair < L1.cext[1]; ++pair) {
                                Cell c;
                                TL::cell(col, pair, *params, flags, &c.n, &c.e, &c.id);
                                put(tx * cells[0] + lx, ty * cells[1] + pair, tz * cells[2] + lz, c);
                            }
                        }
                }
    });
    if (out_info) *out_info = info;
    return BLOK_OK;
}

}  // extern "C"
