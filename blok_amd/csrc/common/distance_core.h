// The capped squared distance field of the resident volume and the edits that threshold it (include/blok_hip.h:
// blok_hip_volume_distance_field has the contract).  The one place the field's rules live: the kernels (hip/distance_kernels.hip) and the
// host build (host/distance.cpp) both include this header.  No HIP types.  Integer arithmetic only, apart from the rule density > 0.
#ifndef BLOK_DISTANCE_CORE_H
#define BLOK_DISTANCE_CORE_H
#include <stdint.h>

#include "blok_hip.h"

#if defined(__HIPCC__)
#define BLOK_DISTANCE_HD __host__ __device__ inline
#else
#define BLOK_DISTANCE_HD inline
#endif

namespace blok {
namespace distance {

constexpr uint32_t kFar = BLOK_DISTANCE_FAR;
constexpr uint32_t kMaxRadius = 255u;
constexpr uint32_t kFlags = BLOK_DISTANCE_TO_EMPTY | BLOK_DISTANCE_BOX_IS_SOLID;

// ---- cell state and sources ---------------------------------------------------------------------------------------------------------
// Inside the box a cell is filled iff its density > 0: zeros of either sign, negative and NaN densities are empty.
BLOK_DISTANCE_HD bool filled(float density) { return density > 0.0f; }
// Outside the box a cell is empty; with BOX_IS_SOLID it is filled.
BLOK_DISTANCE_HD bool outside_filled(uint32_t flags) { return (flags & BLOK_DISTANCE_BOX_IS_SOLID) != 0u; }
BLOK_DISTANCE_HD bool to_empty(uint32_t flags) { return (flags & BLOK_DISTANCE_TO_EMPTY) != 0u; }
// The sources are the filled cells, with TO_EMPTY the empty ones — inside the box and outside it alike.
BLOK_DISTANCE_HD bool is_source(bool cell_filled, uint32_t flags) { return cell_filled != to_empty(flags); }
BLOK_DISTANCE_HD bool outside_is_source(uint32_t flags) { return is_source(outside_filled(flags), flags); }
// What a position outside the box enters a pass as: every cell of its row (of its plane) lies outside too, so the partial minimum over
// the axes already done is 0 when the outside is a source and FAR when it is not.
BLOK_DISTANCE_HD uint32_t outside_value(uint32_t flags) { return outside_is_source(flags) ? 0u : kFar; }

// ---- the capped min-plus step ---------------------------------------------------------------------------------------------------------
// One axis of the field: out(i) = min over |d| <= R of g(i + d) + d^2, FAR when that exceeds R^2.  g is 0 .. R^2 or FAR; FAR + d^2 is
// above R^2 <= 65025 whatever d is, so the sentinel needs no test of its own.  The capped passes compose exactly: a partial sum above
// R^2 can never lead to a total within R^2.
BLOK_DISTANCE_HD uint32_t min_plus_tap(uint32_t best, uint32_t g, int32_t d) {
    const uint32_t c = g + static_cast<uint32_t>(d * d);
    return c < best ? c : best;
}
BLOK_DISTANCE_HD uint32_t min_plus_cap(uint32_t best, uint32_t r2) { return best <= r2 ? best : kFar; }
template <class G>
BLOK_DISTANCE_HD uint32_t capped_min_plus(int32_t radius, G g) {
    uint32_t best = kFar;
    for (int32_t d = -radius; d <= radius; ++d) best = min_plus_tap(best, g(d), d);
    return min_plus_cap(best, static_cast<uint32_t>(radius * radius));
}
// The first axis, from the distances to the nearest source at or below a cell and at or above it along the axis (kNone: there is none).
constexpr uint32_t kNone = 0xFFFFFFFFu;
BLOK_DISTANCE_HD uint32_t axis_value(uint32_t below, uint32_t above, uint32_t radius) {
    const uint32_t d = below < above ? below : above;
    return d <= radius ? d * d : kFar;
}

// The distance from bit `p` of a bit string (64-bit words, bit i of the string = bit i % 64 of word i / 64) down to the nearest set bit at
// or below it, and up to the nearest at or above it; kNone when none lies within `radius`.  The caller's string reaches at least `radius`
// bits beyond p on the side searched.
BLOK_DISTANCE_HD uint32_t count_leading_zeros64(uint64_t w) {
#if defined(__HIP_DEVICE_COMPILE__)
    return static_cast<uint32_t>(__clzll(static_cast<long long>(w)));
#else
    return static_cast<uint32_t>(__builtin_clzll(w));
#endif
}
BLOK_DISTANCE_HD uint32_t count_trailing_zeros64(uint64_t w) {
#if defined(__HIP_DEVICE_COMPILE__)
    return static_cast<uint32_t>(__ffsll(static_cast<long long>(w))) - 1u;
#else
    return static_cast<uint32_t>(__builtin_ctzll(w));
#endif
}
template <class W>
BLOK_DISTANCE_HD uint32_t nearest_below(W word, uint32_t p, uint32_t radius) {
    uint32_t wi = p >> 6;
    const uint32_t b = p & 63u;
    uint64_t m = word(wi) & (b == 63u ? ~0ull : (1ull << (b + 1u)) - 1ull);
    uint32_t base = 0u;                                           // distance from p to bit 63 of word wi, less (63 - b)
    for (;;) {
        if (m) { const uint32_t d = base + b - (63u - count_leading_zeros64(m)); return d <= radius ? d : kNone; }
        if (base + b + 1u > radius || wi == 0u) return kNone;     // the next word starts beyond the radius
        base += 64u; --wi;
        m = word(wi);
    }
}
template <class W>
BLOK_DISTANCE_HD uint32_t nearest_above(W word, uint32_t p, uint32_t radius, uint32_t n_words) {
    uint32_t wi = p >> 6;
    const uint32_t b = p & 63u;
    uint64_t m = word(wi) & (~0ull << b);
    uint32_t base = 0u;
    for (;;) {
        if (m) { const uint32_t d = base + count_trailing_zeros64(m) - b; return d <= radius ? d : kNone; }
        if (base + (64u - b) > radius || wi + 1u >= n_words) return kNone;
        base += 64u; ++wi;
        m = word(wi);
    }
}

// ---- the edits ----------------------------------------------------------------------------------------------------------------------------
BLOK_DISTANCE_HD bool op_known(int op) { return op == BLOK_DISTANCE_GROW || op == BLOK_DISTANCE_SHRINK || op == BLOK_DISTANCE_HOLLOW; }
// GROW thresholds a to-filled field, SHRINK and HOLLOW a to-empty one.
BLOK_DISTANCE_HD bool op_needs_to_empty(int op) { return op != BLOK_DISTANCE_GROW; }
// Whether the edit writes a cell whose snapshot value is `dist` and which is `filled_now`: GROW the empty cells within d2 of a filled one,
// SHRINK the filled cells within d2 of an empty one, HOLLOW the filled cells farther than d2 from every empty one (FAR included).
BLOK_DISTANCE_HD bool grow_writes(uint32_t dist, uint32_t d2, bool filled_now) { return dist >= 1u && dist <= d2 && !filled_now; }
BLOK_DISTANCE_HD bool shrink_writes(uint32_t dist, uint32_t d2, bool filled_now) { return dist >= 1u && dist <= d2 && filled_now; }
BLOK_DISTANCE_HD bool hollow_writes(uint32_t dist, uint32_t d2, bool filled_now) { return dist > d2 && filled_now; }
BLOK_DISTANCE_HD bool edit_writes(int op, uint32_t dist, uint32_t d2, bool filled_now) {
    return op == BLOK_DISTANCE_GROW ? grow_writes(dist, d2, filled_now) : op == BLOK_DISTANCE_SHRINK ? shrink_writes(dist, d2, filled_now)
                                                                                                    : hollow_writes(dist, d2, filled_now);
}

// ---- argument checks: 0 = fine, otherwise the rule that failed (rule_text) ----------------------------------------------------------------
enum Rule { kFine = 0, kUnknownFlags, kRadius, kUnknownOp, kWrongField, kThreshold, kDensity, kVersion };
inline const char* rule_text(int rule) {
    static const char* const kText[] = {"", "unknown flag bits", "max_radius above 255", "unknown op", "the op needs the other kind of field (GROW a to-filled one, SHRINK and HOLLOW a to-empty one)",
                                        "d2 above the snapshot's max_radius squared", "density must be finite and > 0", "info version is not 1"};
    return kText[rule];
}
BLOK_DISTANCE_HD int check_field_args(uint32_t max_radius, uint32_t flags) {
    if (flags & ~kFlags) return kUnknownFlags;
    if (max_radius > kMaxRadius) return kRadius;
    return kFine;
}
BLOK_DISTANCE_HD bool finite_positive(float v) { return v > 0.0f && v <= 3.402823466e+38f; }      // (NaN fails the first test, +inf the second)
BLOK_DISTANCE_HD int check_edit_args(const blok_distance_info& info, int op, uint32_t d2, float density) {
    if (info.version != 1u) return kVersion;
    if (info.flags & ~kFlags) return kUnknownFlags;               // (a host caller's info is its own: nothing about it is taken on trust)
    if (info.max_radius > kMaxRadius) return kRadius;
    if (!op_known(op)) return kUnknownOp;
    if (op_needs_to_empty(op) != to_empty(info.flags)) return kWrongField;
    if (d2 > info.max_radius * info.max_radius) return kThreshold;
    if (op == BLOK_DISTANCE_GROW && !finite_positive(density)) return kDensity;
    return kFine;
}

}  // namespace distance
}  // namespace blok
#endif
