// The column field of the resident volume and scatter (include/blok_hip.h: blok_hip_volume_column_field and
// blok_hip_volume_scatter_models have the contracts).  The one place their arithmetic lives: the kernels (hip/columns_kernels.hip) and the
// host build (host/columns.cpp) both include this header.  No HIP types.  Integer arithmetic only.
#ifndef BLOK_COLUMNS_CORE_H
#define BLOK_COLUMNS_CORE_H
#include <stdint.h>

#include "blok_hip.h"
#include "terrain_core.h"

#if defined(__HIPCC__)
#define BLOK_COLUMNS_HD __host__ __device__ inline
#else
#define BLOK_COLUMNS_HD inline
#endif

namespace blok {
namespace columns {

constexpr uint32_t kNone = BLOK_COLUMNS_NONE;
constexpr uint32_t kFieldFlags = BLOK_COLUMNS_FROM_LOW;
constexpr uint32_t kScatterFlags = BLOK_SCATTER_ANY_MATERIAL | BLOK_SCATTER_ROTATE | BLOK_SCATTER_MIRROR;
constexpr uint32_t kNoLimit = 0xFFFFu;
constexpr uint32_t kSaltCandidate = 0x5CA70001u, kSaltPlacement = 0x5CA70002u;

// ---- the field ----------------------------------------------------------------------------------------------------------------------------
BLOK_COLUMNS_HD bool from_low(uint32_t flags) { return (flags & BLOK_COLUMNS_FROM_LOW) != 0u; }
// The two axes other than `axis`, p < q: a column's index is cp + ext[p] * cq.
BLOK_COLUMNS_HD uint32_t axis_p(uint32_t axis) { return axis == 0u ? 1u : 0u; }
BLOK_COLUMNS_HD uint32_t axis_q(uint32_t axis) { return axis == 2u ? 1u : 2u; }

// The four cells along `axis` of a brick's mask word (bit x + 4 y + 16 z) in the brick's column (ip, iq), as a nibble: bit k = cell k.
BLOK_COLUMNS_HD uint32_t mask_column(uint64_t mask, uint32_t axis, uint32_t ip, uint32_t iq) {
    const uint32_t stride = 2u * axis;                 // log2 of the bit distance between neighbours along the axis
    const uint64_t m = mask >> ((ip << (2u * axis_p(axis))) | (iq << (2u * axis_q(axis))));
    return static_cast<uint32_t>((m & 1u) | (((m >> (1u << stride)) & 1u) << 1) | (((m >> (2u << stride)) & 1u) << 2) | (((m >> (3u << stride)) & 1u) << 3));
}
// The sixteen cells along the axis of a column through four consecutive bricks, from their nibbles: bit k = cell k of the group.
BLOK_COLUMNS_HD uint32_t group_bits(uint32_t n0, uint32_t n1, uint32_t n2, uint32_t n3) { return n0 | (n1 << 4) | (n2 << 8) | (n3 << 12); }
// The first set cell of a group's bits among cells [k_lo, k_hi) (0 <= k_lo < k_hi <= 16: the region's cut), met from the low or the high
// end; 16 = none.
BLOK_COLUMNS_HD uint32_t first_cell(uint32_t bits, uint32_t k_lo, uint32_t k_hi, bool low) {
    const uint32_t n = bits & ((1u << k_hi) - 1u) & ~((1u << k_lo) - 1u);
    if (n == 0u) return 16u;
    return low ? static_cast<uint32_t>(__builtin_ctz(n)) : 31u - static_cast<uint32_t>(__builtin_clz(n));
}
// The top of one column over the box-local cells [a_lo, a_hi) along the axis (a_lo < a_hi): bits_at(g) is group_bits of the column's
// bricks 4 g .. 4 g + 3 along the axis (bricks that hold no cell of [a_lo, a_hi) may be given as 0).  Region-local, or kNone.
template <class BitsAt>
BLOK_COLUMNS_HD uint32_t column_top(BitsAt&& bits_at, uint32_t a_lo, uint32_t a_hi, bool low) {
    const uint32_t g_first = a_lo >> 4, g_last = (a_hi - 1u) >> 4;
    for (uint32_t i = 0; i <= g_last - g_first; ++i) {
        const uint32_t g = low ? g_first + i : g_last - i;
        const uint32_t k = first_cell(bits_at(g), g == g_first ? (a_lo & 15u) : 0u, g == g_last ? ((a_hi - 1u) & 15u) + 1u : 16u, low);
        if (k != 16u) return 16u * g + k - a_lo;
    }
    return kNone;
}

// 0 = fine, otherwise the rule that failed (field_rule_text).
BLOK_COLUMNS_HD int check_field_args(uint32_t axis, uint32_t flags) {
    if (flags & ~kFieldFlags) return 1;
    if (axis > 2u) return 2;
    return 0;
}
inline const char* field_rule_text(int rule) {
    static const char* const kText[] = {"", "unknown flag bits", "axis above 2"};
    return kText[rule];
}

// ---- scatter ------------------------------------------------------------------------------------------------------------------------------
// A column snapshot as scatter reads it (axis 1: column (x, z) at x + ext[0] * z), in host or in device memory.
struct Field {
    const uint16_t* top;
    const uint32_t* material;
    int32_t lo[3];
    uint32_t ext[3];
};
BLOK_COLUMNS_HD Field field_of(const uint16_t* top, const uint32_t* material, const blok_columns_info& info) {
    Field f;
    f.top = top; f.material = material;
    for (int a = 0; a < 3; ++a) { f.lo[a] = info.lo[a]; f.ext[a] = info.ext[a]; }
    return f;
}

// What becomes of a region column: not its cell's candidate, placed, or the test that rejected it first (n_rejected[verdict - kRejected]).
enum Verdict { kNotCandidate = 0, kPlaced = 1, kRejected = 2, kRejectedFootprint = 6, kVerdicts = 7 };

BLOK_COLUMNS_HD int32_t wrap_add(int32_t a, uint32_t b) { return static_cast<int32_t>(static_cast<uint32_t>(a) + b); }
BLOK_COLUMNS_HD int32_t cell_of(int32_t world, uint32_t c) { return world >> c; }
BLOK_COLUMNS_HD uint32_t hash_cell(int32_t cx, int32_t cz, uint32_t salt, uint32_t seed) {
    return hash3(static_cast<uint32_t>(cx), salt, static_cast<uint32_t>(cz), seed);
}
// The candidate column of cell (cx, cz).
BLOK_COLUMNS_HD void candidate(int32_t cx, int32_t cz, uint32_t c, uint32_t h1, int32_t& X, int32_t& Z) {
    const uint32_t m = (1u << c) - 1u;
    X = static_cast<int32_t>((static_cast<uint32_t>(cx) << c) + (h1 & m));
    Z = static_cast<int32_t>((static_cast<uint32_t>(cz) << c) + ((h1 >> 8) & m));
}

// The verdict on the region column (x, z) (region-local, inside the region).
BLOK_COLUMNS_HD int judge(const Field& f, const blok_scatter_params& p, uint32_t x, uint32_t z) {
    const int32_t X = wrap_add(f.lo[0], x), Z = wrap_add(f.lo[2], z);
    const int32_t cx = cell_of(X, p.cell_log2), cz = cell_of(Z, p.cell_log2);
    const uint32_t h1 = hash_cell(cx, cz, kSaltCandidate, p.seed);
    int32_t CX, CZ;
    candidate(cx, cz, p.cell_log2, h1, CX, CZ);
    if (CX != X || CZ != Z) return kNotCandidate;
    if (!((h1 >> 16) < p.probability)) return kRejected + 0;
    const uint64_t column = x + static_cast<uint64_t>(f.ext[0]) * z;
    const uint32_t top = f.top[column];
    if (top == kNone) return kRejected + 1;
    const int64_t y = static_cast<int64_t>(f.lo[1]) + top;
    if (y < p.min_y || y > p.max_y) return kRejected + 2;
    if (!(p.flags & BLOK_SCATTER_ANY_MATERIAL) && f.material[column] != p.surface_material) return kRejected + 3;
    const uint32_t r = p.radius;
    const uint32_t x0 = x > r ? x - r : 0u, x1 = x + r < f.ext[0] ? x + r : f.ext[0] - 1u;
    const uint32_t z0 = z > r ? z - r : 0u, z1 = z + r < f.ext[2] ? z + r : f.ext[2] - 1u;
    for (uint32_t fz = z0; fz <= z1; ++fz)
        for (uint32_t fx = x0; fx <= x1; ++fx) {
            const uint32_t t = f.top[fx + static_cast<uint64_t>(f.ext[0]) * fz];
            if (p.max_rise != kNoLimit && !(t <= top + p.max_rise)) return kRejectedFootprint;
            if (p.max_drop != kNoLimit && !(t != kNone && t + p.max_drop >= top)) return kRejectedFootprint;
        }
    return kPlaced;
}

// The instance of a placed column.  weight_sum: the sum of the entries' weights.
BLOK_COLUMNS_HD blok_instance place(const Field& f, const blok_scatter_params& p, const blok_scatter_entry* entries, uint32_t n_entries, uint32_t weight_sum,
                                    uint32_t x, uint32_t z) {
    const int32_t X = wrap_add(f.lo[0], x), Z = wrap_add(f.lo[2], z);
    const uint32_t h2 = hash_cell(cell_of(X, p.cell_log2), cell_of(Z, p.cell_log2), kSaltPlacement, p.seed);
    const uint32_t pick = (h2 & 0xFFFFu) % weight_sum;
    uint32_t e = 0, cumulative = entries[0].weight;
    while (e + 1u < n_entries && !(cumulative > pick)) { ++e; cumulative += entries[e].weight; }
    const uint32_t r = (p.flags & BLOK_SCATTER_ROTATE) ? (h2 >> 16) & 3u : 0u;
    const uint32_t m = (p.flags & BLOK_SCATTER_MIRROR) ? (h2 >> 18) & 1u : 0u;
    const uint32_t flip = ((0x1540u >> (4u * r)) & 0xFu) ^ m;          // {0, 4, 5, 1}[r]
    const uint32_t top = f.top[x + static_cast<uint64_t>(f.ext[0]) * z];
    const int32_t T[3] = {X, static_cast<int32_t>(static_cast<int64_t>(f.lo[1]) + top + 1 - entries[e].sink), Z};
    blok_instance out;
    out.model = entries[e].model;
    out.axis[0] = (r & 1u) ? 2u : 0u; out.axis[1] = 1u; out.axis[2] = (r & 1u) ? 0u : 2u;
    out.flip = static_cast<uint8_t>(flip);
    for (uint32_t k = 0; k < 3u; ++k) {
        const uint32_t A = out.axis[k];
        out.offset[A] = ((flip >> k) & 1u) ? wrap_add(wrap_add(T[A], 1u), static_cast<uint32_t>(entries[e].anchor[k]))
                                           : wrap_add(T[A], 0u - static_cast<uint32_t>(entries[e].anchor[k]));
    }
    out.reserved[0] = out.reserved[1] = out.reserved[2] = 0u;
    return out;
}

// 0 = fine, otherwise the rule that failed (scatter_rule_text).  info: the column snapshot's, null when there is none.
inline int check_scatter_args(const blok_columns_info* info, const blok_scatter_params* p, const blok_scatter_entry* entries, uint32_t n_entries) {
    if (!p || !entries) return 1;
    if (p->flags & ~kScatterFlags) return 2;
    for (int i = 0; i < 6; ++i) if (p->reserved[i]) return 3;
    if (p->cell_log2 > 8u) return 4;
    if (p->probability > 65536u) return 5;
    if (p->radius > 8u) return 6;
    if (p->max_rise > kNoLimit || p->max_drop > kNoLimit) return 7;
    if (n_entries == 0u || n_entries > BLOK_SCATTER_MAX_ENTRIES) return 8;
    for (uint32_t i = 0; i < n_entries; ++i) if (entries[i].weight == 0u || entries[i].weight > 65535u) return 9;
    if (p->min_y > p->max_y) return 10;
    if (!info) return 11;
    if (info->version != 1u || info->axis != 1u || from_low(info->flags)) return 12;
    return 0;
}
inline const char* scatter_rule_text(int rule) {
    static const char* const kText[] = {"", "null parameters or entries", "unknown flag bits", "non-zero reserved words", "cell_log2 above 8", "probability above 65536",
                                        "radius above 8", "max_rise or max_drop above 0xFFFF", "n_entries of 0 or above 16", "a weight of 0 or above 65535",
                                        "min_y above max_y", "no column snapshot (blok_hip_volume_column_field)", "the column snapshot is not along +y from the top"};
    return kText[rule];
}
inline uint32_t weight_sum(const blok_scatter_entry* entries, uint32_t n_entries) {
    uint32_t w = 0;
    for (uint32_t i = 0; i < n_entries; ++i) w += entries[i].weight;
    return w;
}

}  // namespace columns
}  // namespace blok
#endif
