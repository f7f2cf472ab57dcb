// Neighbour-count rules stepped over a voxel volume (include/blok_hip.h: blok_hip_volume_automaton has the contract).  The one place the
// rule lives — the argument check, the 26 offsets and their neighbourhoods, the vote of a born cell, and the arithmetic that decides the
// 64 cells of a brick at once from its mask and its 26 neighbours' — shared by the kernels (hip/automaton_kernels.hip), the host build
// (host/automaton.cpp, which decides cell by cell) and the host harness (tests/host_harness/automaton_main.cpp, which runs the brick
// arithmetic beside the cell loop).  No HIP types.
//
// A brick's mask is bit x | y << 2 | z << 4 of its 4^3 cells, as everywhere (gpu_build.h).  The state of the cell at offset (dx, dy, dz) of
// each of a brick's 64 cells is one word: the brick's mask shifted along x, y and z, the cells that leave the brick taken from the
// neighbour brick's word.  Up to 26 such words are added into five bit planes — bit c of plane k is bit k of cell c's count — with
// carry-save adders, and a rule's 27-entry truth table is evaluated on the planes by a tree of selections.
#ifndef BLOK_AUTOMATON_CORE_H
#define BLOK_AUTOMATON_CORE_H
#include <float.h>
#include <stdint.h>

#include "blok_hip.h"
#include "lod_core.h"

#if defined(__HIPCC__)
#define BLOK_AUTOMATON_HD __host__ __device__ __forceinline__
#else
#define BLOK_AUTOMATON_HD inline
#endif

static_assert(sizeof(blok_automaton_rule) == 32 && sizeof(blok_automaton_info) == 64, "the sizes the header states");

namespace blok {
namespace automaton {

constexpr uint32_t kFlags = BLOK_AUTOMATON_BOX_IS_SOLID | BLOK_AUTOMATON_FIXED_MATERIAL;
constexpr uint32_t kMaxSteps = 255u;

// 0 = fine, otherwise the rule that failed (all BLOK_ERR_INVALID_ARG).
enum Rule { kFine = 0, kNullRule, kNeighbourhood, kSurviveBits, kBirthBits, kUnknownFlags, kReserved, kSteps, kDensity };
inline int check(const blok_automaton_rule* r) {
    if (!r) return kNullRule;
    if (r->neighbourhood != 6u && r->neighbourhood != 18u && r->neighbourhood != 26u) return kNeighbourhood;
    const uint32_t counts = (2u << r->neighbourhood) - 1u;      // bits 0 .. neighbourhood
    if (r->survive & ~counts) return kSurviveBits;
    if (r->birth & ~counts) return kBirthBits;
    if (r->flags & ~kFlags) return kUnknownFlags;
    if (r->reserved != 0u) return kReserved;
    if (r->steps == 0u || r->steps > kMaxSteps) return kSteps;
    if (r->birth != 0u && !(r->density > 0.0f && r->density <= FLT_MAX)) return kDensity;
    return kFine;
}
inline const char* rule_text(int rule) {
    static const char* const kText[] = {"", "null rule", "neighbourhood must be 6, 18 or 26", "a survive bit above the neighbourhood's size",
                                        "a birth bit above the neighbourhood's size", "unknown flag bits", "reserved must be 0", "steps must be 1 .. 255",
                                        "a rule with births needs a finite density > 0"};
    return rule >= 0 && rule <= kDensity ? kText[rule] : "";
}
// The info of a call over the box-local region [lo, hi) of a box at world `origin`, counts zero.
inline void plan(const int32_t origin[3], const uint32_t lo[3], const uint32_t hi[3], uint32_t flags, blok_automaton_info* info) {
    *info = blok_automaton_info{};
    info->version = 1u; info->flags = flags;
    for (int a = 0; a < 3; ++a) {
        info->lo[a] = static_cast<int32_t>(int64_t(origin[a]) + lo[a]);
        info->ext[a] = hi[a] > lo[a] ? hi[a] - lo[a] : 0u;
    }
}

// ---- the offsets -------------------------------------------------------------------------------------------------------------------------
// Offset i of 26, as cell (dx + 1) + 3 (dy + 1) + 9 (dz + 1) of the 3^3 block around a cell: the six faces first, then the twelve edges,
// then the eight corners, so that offset i belongs to neighbourhood n (6, 18, 26) iff i < n.
BLOK_AUTOMATON_HD uint32_t cell27(uint32_t i) {
    const uint8_t t[26] = {12, 14, 10, 16, 4, 22, 9, 11, 15, 17, 3, 5, 21, 23, 1, 7, 19, 25, 0, 2, 6, 8, 18, 20, 24, 26};
    return t[i];
}
BLOK_AUTOMATON_HD void offset(uint32_t i, int32_t d[3]) {
    const uint32_t c = cell27(i);
    d[0] = static_cast<int32_t>(c % 3u) - 1; d[1] = static_cast<int32_t>((c / 3u) % 3u) - 1; d[2] = static_cast<int32_t>(c / 9u) - 1;
}

// ---- the vote ----------------------------------------------------------------------------------------------------------------------------
// The id of a born cell from its voters: offset i < n votes iff bit i of `voters` is set, for the id id_of(i); the most votes win, a tie goes
// to the smallest id, no voter gives `fallback`.  A voter is counted against the voters behind it only: the first voter of an id so gets the
// id's full count, a later one of the same id a smaller count, which never wins against it.
template <class IdOf>
BLOK_AUTOMATON_HD uint32_t vote(const IdOf& id_of, uint32_t n, uint32_t voters, uint32_t fallback) {
    uint32_t best_n = 0u, best_id = fallback;
    for (uint32_t i = 0; i < n; ++i) {
        if (!((voters >> i) & 1u)) continue;
        const uint32_t id = id_of(i);
        uint32_t count = 1u;
        for (uint32_t k = i + 1u; k < n; ++k) count += ((voters >> k) & 1u) && id_of(k) == id ? 1u : 0u;
        if (count > best_n || (count == best_n && id < best_id)) { best_n = count; best_id = id; }
    }
    return best_id;
}

// ---- a whole brick -----------------------------------------------------------------------------------------------------------------------
// What its neighbours see of brick (bx, by, bz) of a box of `dims` cells: its mask, and with `solid` every cell of it past the box's end
// as filled (lod_core.h: solid).  A brick beyond the brick grid is all outside: in_grid false, the mask ignored.
BLOK_AUTOMATON_HD uint64_t seen(uint64_t mask, bool in_grid, uint32_t bx, uint32_t by, uint32_t bz, const uint32_t dims[3], bool solid) {
    if (!in_grid) return solid ? ~0ull : 0ull;
    return solid ? lod::solid(mask, bx, by, bz, dims) : mask;
}
// The cells of brick b of an axis that lie in [lo, hi), from the pattern of that axis.
BLOK_AUTOMATON_HD uint64_t span(uint32_t b, uint32_t lo, uint32_t hi, uint64_t pattern, uint32_t step) {
    uint64_t bits = 0;
    for (uint32_t i = 0; i < 4u; ++i)
        if (4u * b + i >= lo && 4u * b + i < hi) bits |= pattern << (step * i);
    return bits;
}
// The cells of brick (bx, by, bz) inside the box-local region [lo, hi).
BLOK_AUTOMATON_HD uint64_t region_cells(uint32_t bx, uint32_t by, uint32_t bz, const uint32_t lo[3], const uint32_t hi[3]) {
    return span(bx, lo[0], hi[0], lod::kX0, 1u) & span(by, lo[1], hi[1], lod::kY0, 4u) & span(bz, lo[2], hi[2], lod::kZ0, 16u);
}

// Word c shifted by d (-1, 0, 1) along an axis: bit (x, y, z) of the result is the state of the cell one step along d, which for the cells
// on the brick's face is a cell of the neighbour brick's word (m: below, p: above).
BLOK_AUTOMATON_HD uint64_t shift_x(uint64_t m, uint64_t c, uint64_t p, int d) {
    return d == 0 ? c : d > 0 ? ((c >> 1) & ~(lod::kX0 << 3)) | ((p << 3) & (lod::kX0 << 3)) : ((c << 1) & ~lod::kX0) | ((m >> 3) & lod::kX0);
}
BLOK_AUTOMATON_HD uint64_t shift_y(uint64_t m, uint64_t c, uint64_t p, int d) {
    return d == 0 ? c : d > 0 ? ((c >> 4) & ~(lod::kY0 << 12)) | ((p << 12) & (lod::kY0 << 12)) : ((c << 4) & ~lod::kY0) | ((m >> 12) & lod::kY0);
}
BLOK_AUTOMATON_HD uint64_t shift_z(uint64_t m, uint64_t c, uint64_t p, int d) { return d == 0 ? c : d > 0 ? (c >> 16) | (p << 48) : (c << 16) | (m >> 48); }

// Numbers in bit planes, least significant plane first.  a + b, `n_out` planes (the caller knows the sum fits).
BLOK_AUTOMATON_HD void add_planes(const uint64_t* a, uint32_t na, const uint64_t* b, uint32_t nb, uint64_t* out, uint32_t n_out) {
    uint64_t carry = 0ull;
    for (uint32_t k = 0; k < n_out; ++k) {
        const uint64_t x = k < na ? a[k] : 0ull, y = k < nb ? b[k] : 0ull, t = x ^ y;
        out[k] = t ^ carry;
        carry = (x & y) | (carry & t);
    }
}
// Six words added into three planes: two carry-save adders, then their sums and carries.
BLOK_AUTOMATON_HD void sum6(const uint64_t w[6], uint64_t out[3]) {
    const uint64_t s0 = w[0] ^ w[1] ^ w[2], c0 = (w[0] & w[1]) | (w[2] & (w[0] ^ w[1]));
    const uint64_t s1 = w[3] ^ w[4] ^ w[5], c1 = (w[3] & w[4]) | (w[5] & (w[3] ^ w[4]));
    const uint64_t c2 = s0 & s1;
    out[0] = s0 ^ s1;
    out[1] = c0 ^ c1 ^ c2;
    out[2] = (c0 & c1) | (c2 & (c0 ^ c1));
}
// The counts of the 64 cells of a brick over neighbourhood NB, in five planes.  seen27: seen() of the 27 bricks around it and of
// itself, brick (jx, jy, jz) in -1 .. 1 at (jx + 1) + 3 (jy + 1) + 9 (jz + 1).
template <uint32_t NB>
BLOK_AUTOMATON_HD void brick_counts(const uint64_t seen27[27], uint64_t planes[5]) {
    // the 27 shifted words, axis by axis: ax[dx][row], then ay[dx][dy][jz], then s[cell27]
    uint64_t s[27];
    for (int dx = -1; dx <= 1; ++dx) {
        uint64_t ax[9];
        for (uint32_t row = 0; row < 9u; ++row) ax[row] = shift_x(seen27[3u * row], seen27[3u * row + 1u], seen27[3u * row + 2u], dx);
        for (int dy = -1; dy <= 1; ++dy) {
            uint64_t ay[3];
            for (uint32_t jz = 0; jz < 3u; ++jz) ay[jz] = shift_y(ax[3u * jz], ax[3u * jz + 1u], ax[3u * jz + 2u], dy);
            for (int dz = -1; dz <= 1; ++dz) s[(dx + 1) + 3 * (dy + 1) + 9 * (dz + 1)] = shift_z(ay[0], ay[1], ay[2], dz);
        }
    }
    uint64_t w[26];
    for (uint32_t i = 0; i < 26u; ++i) w[i] = s[cell27(i)];
    uint64_t faces[3];
    sum6(w, faces);                                         // <= 6
    if (NB == 6u) { planes[0] = faces[0]; planes[1] = faces[1]; planes[2] = faces[2]; planes[3] = planes[4] = 0ull; return; }
    uint64_t e0[3], e1[3], edges[4], near[5];
    sum6(w + 6, e0); sum6(w + 12, e1);
    add_planes(e0, 3u, e1, 3u, edges, 4u);                  // <= 12
    add_planes(faces, 3u, edges, 4u, near, 5u);             // <= 18
    if (NB == 18u) { for (uint32_t k = 0; k < 5u; ++k) planes[k] = near[k]; return; }
    uint64_t c0[3], corners[4];
    sum6(w + 18, c0);
    const uint64_t pair[2] = {w[24] ^ w[25], w[24] & w[25]};
    add_planes(c0, 3u, pair, 2u, corners, 4u);              // <= 8
    add_planes(near, 5u, corners, 4u, planes, 5u);          // <= 26
}
// A truth table over counts 0 .. 31 evaluated on the planes: bit c of the result is bit (count of cell c) of `table`.  The table is the
// same for every brick (on the device: wave-uniform), so the first level is a choice among 0, ~0, plane 0 and its complement.
BLOK_AUTOMATON_HD uint64_t table_on_planes(uint32_t table, const uint64_t planes[5]) {
    uint64_t g[16];
    for (uint32_t i = 0; i < 16u; ++i) {
        const uint32_t two = (table >> (2u * i)) & 3u;
        g[i] = two == 0u ? 0ull : two == 3u ? ~0ull : two == 2u ? planes[0] : ~planes[0];
    }
    for (uint32_t k = 1; k < 5u; ++k)
        for (uint32_t i = 0; i < (16u >> k); ++i) g[i] = (g[2u * i] & ~planes[k]) | (g[2u * i + 1u] & planes[k]);
    return g[0];
}
// One step for a brick: the cells of `cells` (the brick's cells in the region) that are born and that die.  mask: the brick's own.
BLOK_AUTOMATON_HD void brick_step(const uint64_t seen27[27], uint64_t mask, uint64_t cells, uint32_t neighbourhood, uint32_t survive, uint32_t birth,
                                  uint64_t* born, uint64_t* died) {
    uint64_t planes[5];
    if (neighbourhood == 6u) brick_counts<6u>(seen27, planes);
    else if (neighbourhood == 18u) brick_counts<18u>(seen27, planes);
    else brick_counts<26u>(seen27, planes);
    *born = table_on_planes(birth, planes) & ~mask & cells;
    *died = ~table_on_planes(survive, planes) & mask & cells;
}

}  // namespace automaton
}  // namespace blok
#endif
