// The flood of the resident volume from seeds and the edits that threshold it (include/blok_hip.h: blok_hip_volume_flood_field has the
// contract).  The one place the flood's rules live: the kernels (hip/flood_kernels.hip) and the host build (host/flood.cpp) both include
// this header.  No HIP types.  Integer arithmetic only, apart from the rule density > 0.
#ifndef BLOK_FLOOD_CORE_H
#define BLOK_FLOOD_CORE_H
#include <stdint.h>

#include "blok_hip.h"

#if defined(__HIPCC__)
#define BLOK_FLOOD_HD __host__ __device__ inline
#else
#define BLOK_FLOOD_HD inline
#endif

namespace blok {
namespace flood {

constexpr uint32_t kFar = BLOK_FLOOD_FAR;
constexpr uint32_t kMaxSteps = BLOK_FLOOD_MAX_STEPS;
constexpr uint32_t kFaceShift = 8u;
constexpr uint32_t kFaceBits = 0x3Fu << kFaceShift;
constexpr uint32_t kFlags = BLOK_FLOOD_THROUGH_FILLED | BLOK_FLOOD_SAME_MATERIAL | kFaceBits;

// ---- passable cells ---------------------------------------------------------------------------------------------------------------------
// A cell is filled iff its density > 0: zeros of either sign, negative and NaN densities are empty.
BLOK_FLOOD_HD bool filled(float density) { return density > 0.0f; }
BLOK_FLOOD_HD bool through_filled(uint32_t flags) { return (flags & BLOK_FLOOD_THROUGH_FILLED) != 0u; }
BLOK_FLOOD_HD bool same_material(uint32_t flags) { return (flags & BLOK_FLOOD_SAME_MATERIAL) != 0u; }
// A region cell: the empty ones by default, the filled ones with THROUGH_FILLED, with SAME_MATERIAL those of them whose id is `material`.
// (A cell outside the region is impassable: the callers never ask about one.)
BLOK_FLOOD_HD bool passable(bool cell_filled, uint32_t id, uint32_t flags, uint32_t material) {
    if (!through_filled(flags)) return !cell_filled;
    return cell_filled && (!same_material(flags) || id == material);
}
// The 64 cells of a brick at once, from its mask word (bit x + 4 y + 16 z), in the two modes that need no ids.
BLOK_FLOOD_HD uint64_t passable_word(uint64_t filled_mask, uint32_t flags) { return through_filled(flags) ? filled_mask : ~filled_mask; }
// Side f of a box (blok_hit::face numbering: 0 +X, 1 -X, 2 +Y, 3 -Y, 4 +Z, 5 -Z) is a seed layer; its axis; the coordinate of its layer.
BLOK_FLOOD_HD bool seeds_face(uint32_t flags, uint32_t f) { return ((flags >> (kFaceShift + f)) & 1u) != 0u; }
BLOK_FLOOD_HD uint32_t face_axis(uint32_t f) { return f >> 1; }
BLOK_FLOOD_HD uint32_t face_layer(uint32_t f, uint32_t lo, uint32_t hi) { return (f & 1u) ? lo : hi - 1u; }      // (of a non-empty [lo, hi))

// ---- the capped step ----------------------------------------------------------------------------------------------------------------------
// What a passable cell holding `d` holds after looking at a neighbour holding `neighbour`: neighbour + 1 when that is lower and within the
// cap.  Above the cap the cell is not written.  FAR + 1 = 65536 lies above every cap (K <= 65534), so the sentinel needs no test of its own.
BLOK_FLOOD_HD uint32_t relax(uint32_t d, uint32_t neighbour, uint32_t max_steps) {
    const uint32_t c = neighbour + 1u;
    return (c <= max_steps && c < d) ? c : d;
}

// ---- the edits ----------------------------------------------------------------------------------------------------------------------------
BLOK_FLOOD_HD bool op_known(int op) { return op >= BLOK_FLOOD_FILL && op <= BLOK_FLOOD_CLEAR; }
// FILL and FILL_UNREACHED threshold a through-empty field, PAINT and CLEAR a through-filled one.
BLOK_FLOOD_HD bool op_needs_through_filled(int op) { return op == BLOK_FLOOD_PAINT || op == BLOK_FLOOD_CLEAR; }
BLOK_FLOOD_HD bool op_fills(int op) { return op == BLOK_FLOOD_FILL || op == BLOK_FLOOD_FILL_UNREACHED; }
// Whether the edit writes a cell whose snapshot value is `dist` and which is `filled_now` (d <= K < FAR: "dist <= d" never admits FAR).
BLOK_FLOOD_HD bool fill_writes(uint32_t dist, uint32_t d, bool filled_now) { return dist <= d && !filled_now; }
BLOK_FLOOD_HD bool fill_unreached_writes(uint32_t dist, bool filled_now) { return dist == kFar && !filled_now; }
BLOK_FLOOD_HD bool paint_writes(uint32_t dist, uint32_t d, bool filled_now) { return dist <= d && filled_now; }
BLOK_FLOOD_HD bool clear_writes(uint32_t dist, uint32_t d, bool filled_now) { return dist <= d && filled_now; }
BLOK_FLOOD_HD bool edit_writes(int op, uint32_t dist, uint32_t d, bool filled_now) {
    return op == BLOK_FLOOD_FILL ? fill_writes(dist, d, filled_now) : op == BLOK_FLOOD_FILL_UNREACHED ? fill_unreached_writes(dist, filled_now)
         : op == BLOK_FLOOD_PAINT ? paint_writes(dist, d, filled_now) : clear_writes(dist, d, filled_now);
}
// What a written cell gets: PAINT keeps its density.
BLOK_FLOOD_HD bool op_writes_density(int op) { return op != BLOK_FLOOD_PAINT; }
BLOK_FLOOD_HD float written_density(int op, float density) { return op_fills(op) ? density : 0.0f; }
BLOK_FLOOD_HD uint32_t written_material(int op, uint32_t material) { return op == BLOK_FLOOD_CLEAR ? 0u : material; }

// ---- argument checks: 0 = fine, otherwise the rule that failed (rule_text) ----------------------------------------------------------------
enum Rule { kFine = 0, kUnknownFlags, kMaterialFlag, kSteps, kNullSeeds, kUnknownOp, kWrongField, kThreshold, kDensity, kVersion };
inline const char* rule_text(int rule) {
    static const char* const kText[] = {"", "unknown flag bits", "SAME_MATERIAL needs THROUGH_FILLED", "max_steps above 65534", "null seed array with n_seeds > 0", "unknown op",
                                        "the op needs the other kind of field (FILL and FILL_UNREACHED a through-empty one, PAINT and CLEAR a THROUGH_FILLED one)",
                                        "d above the snapshot's max_steps", "density must be finite and > 0", "info version is not 1"};
    return kText[rule];
}
BLOK_FLOOD_HD int check_field_args(const void* seeds, uint64_t n_seeds, uint32_t max_steps, uint32_t flags) {
    if (flags & ~kFlags) return kUnknownFlags;
    if (same_material(flags) && !through_filled(flags)) return kMaterialFlag;
    if (max_steps > kMaxSteps) return kSteps;
    if (n_seeds && !seeds) return kNullSeeds;
    return kFine;
}
BLOK_FLOOD_HD bool finite_positive(float v) { return v > 0.0f && v <= 3.402823466e+38f; }      // (NaN fails the first test, +inf the second)
BLOK_FLOOD_HD int check_edit_args(const blok_flood_info& info, int op, uint32_t d, float density) {
    if (info.version != 1u) return kVersion;
    if (info.flags & ~kFlags) return kUnknownFlags;               // (a host caller's info is its own: nothing about it is taken on trust)
    if (same_material(info.flags) && !through_filled(info.flags)) return kMaterialFlag;
    if (info.max_steps > kMaxSteps) return kSteps;
    if (!op_known(op)) return kUnknownOp;
    if (op_needs_through_filled(op) != through_filled(info.flags)) return kWrongField;
    if (op != BLOK_FLOOD_FILL_UNREACHED && d > info.max_steps) return kThreshold;
    if (op_fills(op) && !finite_positive(density)) return kDensity;
    return kFine;
}

}  // namespace flood
}  // namespace blok
#endif
