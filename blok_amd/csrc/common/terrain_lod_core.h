// Procedural terrain reduced to coarse levels without a volume (include/blok_hip.h: blok_hip_terrain_reduce has the contract).  The one
// place the tile arithmetic of its level-1 producer lives, shared by the kernel (hip/lod_kernels.hip: terrain_lod_kernel) and the host
// build (host/terrain_lod.cpp).  The terrain is terrain_core.h's, the vote lod_core.h's; this header only carries a column of voxels as
// bits along y.  No HIP types.
//
// A tile is kTileX x kTileZ columns and kSlab rows, its corner at even world coordinates, so it holds whole level-1 cells.  A column of the
// tile and of its one-column halo is one 64-bit word, bit k = row y0 + k, and two halo bits for the rows y0 - 1 and y0 + kSlab:
//   solid     what the neighbours see of the voxel: the function where it is evaluated, all ones elsewhere (outside the region without
//             BLOK_LOD_SEAMLESS: the faces of the region expose nothing; with it the region grown by one voxel is evaluated);
//   filled    solid restricted to the region;
//   exposed   filled with an empty neighbour: bit-parallel along y from the column's own word and its four neighbour columns';
//   ore       the voters below the soil whose 3-D noise says ore.  The terrain has four material classes per voxel — surface and soil by
//             the depth under the column's height, rock and ore below — so the ids of a column are its height and this one word.
// A level-1 cell is the 2-bit pairs of 2 x 2 columns.
#ifndef BLOK_TERRAIN_LOD_CORE_H
#define BLOK_TERRAIN_LOD_CORE_H
#include <stdint.h>

#include "lod_core.h"
#include "terrain_core.h"

namespace blok {
namespace terrain_lod {

constexpr uint32_t kTileX = 64u, kTileZ = 16u, kSlab = 64u;                  // a tile's columns and rows (voxels); even, kSlab the word's width
constexpr uint32_t kColsX = kTileX + 2u, kColsZ = kTileZ + 2u;               // with the halo
constexpr uint32_t kCols = kColsX * kColsZ, kInner = kTileX * kTileZ;
constexpr uint32_t kFlags = BLOK_LOD_VOTE_EXPOSED | BLOK_LOD_SEAMLESS;
constexpr int32_t kMaxCoordinate = 1 << 30;
constexpr uint32_t kMaxExtent = 65536u;

// The region's rules: 0 = fine, else the status.
inline int check_region(const int32_t lo[3], const int32_t hi[3]) {
    for (int a = 0; a < 3; ++a) if (lo[a] > hi[a]) return BLOK_ERR_INVALID_ARG;
    uint64_t cells = 1;
    for (int a = 0; a < 3; ++a) {
        if (lo[a] < -kMaxCoordinate || hi[a] > kMaxCoordinate || int64_t(hi[a]) - lo[a] > int64_t(kMaxExtent)) return BLOK_ERR_UNSUPPORTED;
        cells *= static_cast<uint64_t>(((int64_t(hi[a]) + 1) >> 1) - (int64_t(lo[a]) >> 1));
    }
    return cells >= (1ull << 31) ? BLOK_ERR_UNSUPPORTED : BLOK_OK;
}
// The info of the call, counts zero: lod::plan of a box that is the region.
inline void plan(const int32_t lo[3], const int32_t hi[3], uint32_t levels, uint32_t flags, blok_lod_info* info) {
    const uint32_t zero[3] = {0u, 0u, 0u};
    const uint32_t ext[3] = {static_cast<uint32_t>(hi[0] - lo[0]), static_cast<uint32_t>(hi[1] - lo[1]), static_cast<uint32_t>(hi[2] - lo[2])};
    lod::plan(lo, zero, ext, levels, flags, info);
}

// ---- words along y -----------------------------------------------------------------------------------------------------------------------
BLOK_LOD_HD uint64_t low_bits(int64_t count) { return count <= 0 ? 0ull : count >= 64 ? ~0ull : (1ull << count) - 1ull; }
// The rows of the slab at y0 that lie in [lo, hi).
BLOK_LOD_HD uint64_t rows_in(int32_t y0, int32_t lo, int32_t hi) { return low_bits(int64_t(hi) - y0) & ~low_bits(int64_t(lo) - y0); }

struct Column {
    uint64_t solid;
    uint32_t halo;            // bit 0: row y0 - 1, bit 1: row y0 + kSlab
};
// A column nobody evaluates.
BLOK_LOD_HD Column outside() { return Column{~0ull, 3u}; }

// Column (X, Z) of height H over the rows y0 - 1 .. y0 + kSlab: the rows in [glo, ghi) by the function, one solid() each and none above
// the height; every other row all ones.  (No 3-D noise is touched where the rows lie above H.)
BLOK_LOD_HD Column column_solid(const blok_terrain_params& p, terrain::Walker& w, int32_t X, int32_t Z, int32_t H, int32_t y0, int32_t glo, int32_t ghi) {
    Column c;
    c.solid = ~rows_in(y0, glo, ghi);
    c.halo = ((y0 - 1 >= glo && y0 - 1 < ghi) ? 0u : 1u) | ((y0 + 64 >= glo && y0 + 64 < ghi) ? 0u : 2u);
    const int32_t first = y0 - 1 > glo ? y0 - 1 : glo;
    int32_t last = y0 + 64 < ghi - 1 ? y0 + 64 : ghi - 1;
    if (H < last) last = H;
#if defined(__HIP_DEVICE_COMPILE__)
#pragma unroll 1
#endif
    for (int32_t Y = first; Y <= last; ++Y) {
        if (!terrain::solid(p, w, X, Y, Z, H)) continue;
        const int32_t k = Y - y0;
        if (k < 0) c.halo |= 1u;
        else if (k >= 64) c.halo |= 2u;
        else c.solid |= 1ull << k;
    }
    return c;
}
// The filled voxels `filled` of a column with an empty neighbour: c the column itself, xm .. zp the solid words of its four neighbours.
BLOK_LOD_HD uint64_t exposed(uint64_t filled, const Column& c, uint64_t xm, uint64_t xp, uint64_t zm, uint64_t zp) {
    const uint64_t up = (c.solid >> 1) | (static_cast<uint64_t>((c.halo >> 1) & 1u) << 63), down = (c.solid << 1) | (c.halo & 1u);
    return filled & ~(up & down & xm & xp & zm & zp);
}
// The voxels of a column whose id can vote in their level-1 cell: the filled ones; under VOTE_EXPOSED, in a cell that has an exposed
// voxel, the exposed ones alone.  cell_exposed: the exposed words of the cell's 2 x 2 columns, or-ed.
BLOK_LOD_HD uint64_t voters(uint64_t filled, uint64_t exposed_bits, uint64_t cell_exposed, uint32_t flags) {
    if (!(flags & BLOK_LOD_VOTE_EXPOSED)) return filled;
    uint64_t any = (cell_exposed | (cell_exposed >> 1)) & 0x5555555555555555ull;
    any |= any << 1;
    return (filled & ~any) | (exposed_bits & any);
}
// The rows of the slab under the surface voxel of a column of height H: in the soil, and below it.
BLOK_LOD_HD void depth_words(int32_t H, int32_t y0, uint32_t soil_depth, uint64_t* soil, uint64_t* deep) {
    *deep = low_bits(int64_t(H) - int64_t(soil_depth) - y0);
    *soil = low_bits(int64_t(H) - y0) & ~*deep;
}
// The voxels of `want` (rows under the soil) whose material is the ore's: terrain::material each, rising, so the walker keeps its cell.
BLOK_LOD_HD uint64_t column_ore(const blok_terrain_params& p, terrain::Walker& w, int32_t X, int32_t Z, int32_t H, int32_t y0, uint64_t want) {
    uint64_t ore = 0ull;
#if defined(__HIP_DEVICE_COMPILE__)
#pragma unroll 1
#endif
    while (want) {
        const uint32_t k = static_cast<uint32_t>(__builtin_ctzll(want));
        want &= want - 1ull;
        if (terrain::material(p, w, X, y0 + static_cast<int32_t>(k), Z, H) == p.ore_material) ore |= 1ull << k;
    }
    return ore;
}

// ---- a level-1 cell ------------------------------------------------------------------------------------------------------------------------
struct Words {
    uint64_t filled, exposed, soil, deep, ore;
};
// Cell `pair` (rows 2 pair, 2 pair + 1) of the columns col[dx | dz << 1]: n, e and the vote over the voxels' real ids (two classes may carry
// one id: lod::vote adds their weights).
BLOK_LOD_HD void cell(const Words col[4], uint32_t pair, const blok_terrain_params& p, uint32_t flags, uint32_t* out_n, uint32_t* out_e, uint32_t* out_id) {
    uint32_t n[8], e[8], id[8];
    for (uint32_t q = 0; q < 4u; ++q)
        for (uint32_t dy = 0; dy < 2u; ++dy) {
            const uint32_t c = (q & 1u) | (dy << 1) | ((q >> 1) << 2), bit = 2u * pair + dy;
            n[c] = static_cast<uint32_t>(col[q].filled >> bit) & 1u;
            e[c] = static_cast<uint32_t>(col[q].exposed >> bit) & 1u;
            const bool deep = (col[q].deep >> bit) & 1ull, soil = (col[q].soil >> bit) & 1ull, ore = (col[q].ore >> bit) & 1ull;
            id[c] = !n[c] ? 0u : deep ? (ore ? p.ore_material : p.rock_material) : soil ? p.soil_material : p.surface_material;
        }
    lod::cell_of(n, e, id, flags, out_n, out_e, out_id);
}

}  // namespace terrain_lod
}  // namespace blok
#endif
