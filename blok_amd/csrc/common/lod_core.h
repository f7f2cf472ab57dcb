// The reduction of a voxel volume to a pyramid of coarser levels (include/blok_hip.h: blok_hip_volume_reduce has the contract).  The one
// place its rule lives — the grids of the levels, the exposure of a brick's 64 cells, the vote of eight children — shared by the kernels
// (hip/lod_kernels.hip) and the host build (host/lod.cpp).  No HIP types.
//
// A brick's mask is bit x | y << 2 | z << 4 of its 4^3 cells, as everywhere (gpu_build.h).  Exposure is computed on whole masks: the six
// neighbour states of all 64 cells are six shifted words, the cells on a brick's face taking theirs from the neighbour brick's mask.
#ifndef BLOK_LOD_CORE_H
#define BLOK_LOD_CORE_H
#include <stdint.h>

#include "blok_hip.h"

#if defined(__HIPCC__)
#define BLOK_LOD_HD __host__ __device__ __forceinline__
#else
#define BLOK_LOD_HD inline
#endif

static_assert(sizeof(blok_lod_level) == 64 && sizeof(blok_lod_info) == 360, "the sizes the header states");

namespace blok {
namespace lod {

constexpr uint32_t kFlags = BLOK_LOD_VOTE_EXPOSED;

// 0 = fine, otherwise the rule that failed (all BLOK_ERR_INVALID_ARG).
enum Rule { kFine = 0, kLevels, kUnknownFlags };
inline int check_args(uint32_t levels, uint32_t flags) {
    if (levels == 0u || levels > BLOK_LOD_MAX_LEVELS) return kLevels;
    if (flags & ~kFlags) return kUnknownFlags;
    return kFine;
}
// The same for an entry that knows more flag bits than kFlags (terrain_lod_core.h: blok_hip_terrain_reduce takes BLOK_LOD_SEAMLESS).
inline int check_args(uint32_t levels, uint32_t flags, uint32_t known) {
    if (levels == 0u || levels > BLOK_LOD_MAX_LEVELS) return kLevels;
    if (flags & ~known) return kUnknownFlags;
    return kFine;
}
inline const char* rule_text(int rule) { return rule == kLevels ? "levels must be 1 .. 5" : rule == kUnknownFlags ? "unknown flag bits" : ""; }

// ---- the grids ---------------------------------------------------------------------------------------------------------------------------
// The info of a reduce of the box-local region [lo, hi) of a box at world `origin`, counts zero: level j runs from the floor of lo / 2^j to
// the ceiling of hi / 2^j per axis; an empty region has no cell at any level.
inline void plan(const int32_t origin[3], const uint32_t lo[3], const uint32_t hi[3], uint32_t levels, uint32_t flags, blok_lod_info* info) {
    *info = blok_lod_info{};
    info->version = 1u; info->flags = flags; info->levels = levels;
    bool empty = false;
    for (int a = 0; a < 3; ++a) {
        info->lo[a] = static_cast<int32_t>(int64_t(origin[a]) + lo[a]);
        info->ext[a] = hi[a] > lo[a] ? hi[a] - lo[a] : 0u;
        empty = empty || info->ext[a] == 0u;
    }
    for (uint32_t j = 1; j <= levels; ++j) {
        blok_lod_level& L = info->level[j - 1u];
        L.n_cells = empty ? 0u : 1u;
        for (int a = 0; a < 3; ++a) {
            const int64_t wlo = int64_t(origin[a]) + lo[a], whi = int64_t(origin[a]) + hi[a];
            const int64_t clo = wlo >> j, chi = (whi + (int64_t(1) << j) - 1) >> j;
            L.clo[a] = static_cast<int32_t>(clo);
            L.cext[a] = empty ? 0u : static_cast<uint32_t>(chi - clo);
            L.n_cells *= L.cext[a];
        }
    }
}
// A level's three planes lie one behind the other, level behind level, in one array: bytes.
BLOK_LOD_HD uint64_t level_bytes(uint64_t n_cells) { return 8u * n_cells; }
BLOK_LOD_HD uint64_t plane_offset(uint64_t n_cells, uint32_t plane) { return plane == 0u ? 0u : plane == 1u ? 2u * n_cells : 4u * n_cells; }
inline uint64_t level_offset(const blok_lod_info& info, uint32_t level) {
    uint64_t at = 0;
    for (uint32_t j = 1; j < level; ++j) at += level_bytes(info.level[j - 1u].n_cells);
    return at;
}
inline uint64_t total_bytes(const blok_lod_info& info) { return level_offset(info, info.levels + 1u); }

// ---- exposure of a brick -----------------------------------------------------------------------------------------------------------------
constexpr uint64_t kX0 = 0x1111111111111111ull;      // the cells with x == 0; << i: x == i
constexpr uint64_t kY0 = 0x000F000F000F000Full;      // y == 0; << 4 i
constexpr uint64_t kZ0 = 0x000000000000FFFFull;      // z == 0; << 16 i

// The cells of a brick at coordinate b of an axis of n cells that lie past the box's end, from the pattern of that axis: outside the
// box, and so filled to their neighbours.
BLOK_LOD_HD uint64_t past_end(uint32_t b, uint32_t n, uint64_t pattern, uint32_t step) {
    uint64_t bits = 0;
    for (uint32_t i = 0; i < 4u; ++i)
        if (4u * b + i >= n) bits |= pattern << (step * i);
    return bits;
}
// What the neighbours of brick (bx, by, bz) see of it: its mask, and as filled every cell of it outside the box of `dims` cells.  A brick
// beyond the brick grid is all outside (the caller passes mask 0).
BLOK_LOD_HD uint64_t solid(uint64_t mask, uint32_t bx, uint32_t by, uint32_t bz, const uint32_t dims[3]) {
    return mask | past_end(bx, dims[0], kX0, 1u) | past_end(by, dims[1], kY0, 4u) | past_end(bz, dims[2], kZ0, 16u);
}
// The filled cells of `mask` with an empty neighbour.  s: solid() of the brick itself; xm .. zp: solid() of the six neighbour bricks.
BLOK_LOD_HD uint64_t exposed(uint64_t mask, uint64_t s, uint64_t xm, uint64_t xp, uint64_t ym, uint64_t yp, uint64_t zm, uint64_t zp) {
    const uint64_t px = ((s >> 1) & ~(kX0 << 3)) | ((xp << 3) & (kX0 << 3));
    const uint64_t mx = ((s << 1) & ~kX0) | ((xm >> 3) & kX0);
    const uint64_t py = ((s >> 4) & ~(kY0 << 12)) | ((yp << 12) & (kY0 << 12));
    const uint64_t my = ((s << 4) & ~kY0) | ((ym >> 12) & kY0);
    const uint64_t pz = (s >> 16) | (zp << 48);
    const uint64_t mz = (s << 16) | (zm >> 48);
    return mask & ~(px & mx & py & my & pz & mz);
}
// exposed() of brick (bx, by, bz) of a grid of nb bricks over a box of dims cells; at(bx, by, bz) is the mask of a brick inside the grid.
template <class At>
BLOK_LOD_HD uint64_t brick_exposed(const At& at, uint32_t bx, uint32_t by, uint32_t bz, const uint32_t nb[3], const uint32_t dims[3], uint64_t* out_mask) {
    const auto solid_at = [&](uint32_t x, uint32_t y, uint32_t z) -> uint64_t {      // (a coordinate below 0 wraps and fails)
        return (x < nb[0] && y < nb[1] && z < nb[2]) ? solid(at(x, y, z), x, y, z, dims) : ~0ull;
    };
    const uint64_t m = at(bx, by, bz);
    *out_mask = m;
    if (!m) return 0ull;                                // nothing filled, nothing exposed: the neighbours are not read
    return exposed(m, solid(m, bx, by, bz, dims), solid_at(bx - 1u, by, bz), solid_at(bx + 1u, by, bz), solid_at(bx, by - 1u, bz), solid_at(bx, by + 1u, bz),
                   solid_at(bx, by, bz - 1u), solid_at(bx, by, bz + 1u));
}

// ---- the vote ----------------------------------------------------------------------------------------------------------------------------
// Eight (weight, id) pairs: weights of equal ids add, the largest sum wins, a tie goes to the smallest id; no weight gives 0.
BLOK_LOD_HD uint32_t vote(const uint32_t w[8], const uint32_t id[8]) {
    uint32_t best_sum = 0u, best_id = 0u;
    for (uint32_t i = 0; i < 8u; ++i) {
        if (!w[i]) continue;
        uint32_t sum = 0u;
        for (uint32_t k = 0; k < 8u; ++k) sum += id[k] == id[i] ? w[k] : 0u;
        if (sum > best_sum || (sum == best_sum && id[i] < best_id)) { best_sum = sum; best_id = id[i]; }
    }
    return best_id;
}
// A cell from its eight children (child dx | dy << 1 | dz << 2; a child that does not exist has n = e = 0).
BLOK_LOD_HD void cell_of(const uint32_t n[8], const uint32_t e[8], const uint32_t id[8], uint32_t flags, uint32_t* out_n, uint32_t* out_e, uint32_t* out_id) {
    uint32_t sn = 0u, se = 0u;
    for (uint32_t c = 0; c < 8u; ++c) { sn += n[c]; se += e[c]; }
    *out_n = sn; *out_e = se;
    *out_id = !sn ? 0u : vote(((flags & BLOK_LOD_VOTE_EXPOSED) && se) ? e : n, id);
}

// The level below a level j >= 2, as its cells read it: the planes, the grid's extent, and off = 2 clo_j - clo_(j-1) per axis (0 or -1).
struct Below {
    const uint16_t* n; const uint16_t* e; const uint32_t* id;
    uint32_t cext[3];
    int32_t off[3];
};
// Cell (cx, cy, cz) of the level above, counted from its grid's corner.
BLOK_LOD_HD void cell_above(const Below& b, uint32_t cx, uint32_t cy, uint32_t cz, uint32_t flags, uint32_t* out_n, uint32_t* out_e, uint32_t* out_id) {
    uint32_t n[8], e[8], id[8];
    for (uint32_t c = 0; c < 8u; ++c) {
        const int64_t x = int64_t(2u * cx + (c & 1u)) + b.off[0], y = int64_t(2u * cy + ((c >> 1) & 1u)) + b.off[1], z = int64_t(2u * cz + (c >> 2)) + b.off[2];
        n[c] = e[c] = id[c] = 0u;
        if (x < 0 || y < 0 || z < 0 || x >= int64_t(b.cext[0]) || y >= int64_t(b.cext[1]) || z >= int64_t(b.cext[2])) continue;
        const uint64_t i = uint64_t(x) + b.cext[0] * (uint64_t(y) + uint64_t(b.cext[1]) * uint64_t(z));
        n[c] = b.n[i];
        if (n[c]) { e[c] = b.e[i]; id[c] = b.id[i]; }      // (e <= n: an empty child has neither)
    }
    cell_of(n, e, id, flags, out_n, out_e, out_id);
}
inline Below below_of(const blok_lod_info& info, uint32_t level, const void* base) {      // level >= 2; base: the snapshot's array
    const blok_lod_level& L = info.level[level - 2u];
    const char* at = static_cast<const char*>(base) + level_offset(info, level - 1u);
    Below b{};
    b.n = reinterpret_cast<const uint16_t*>(at + plane_offset(L.n_cells, 0u));
    b.e = reinterpret_cast<const uint16_t*>(at + plane_offset(L.n_cells, 1u));
    b.id = reinterpret_cast<const uint32_t*>(at + plane_offset(L.n_cells, 2u));
    for (int a = 0; a < 3; ++a) { b.cext[a] = L.cext[a]; b.off[a] = static_cast<int32_t>(2 * int64_t(info.level[level - 1u].clo[a]) - L.clo[a]); }
    return b;
}

}  // namespace lod
}  // namespace blok
#endif
