// Posed models (include/blok_hip.h: blok_pose, "Posed models"): the limits of the record's fifteen floats, shared by the kernels
// (hip/posed_core.h), the entries' host check (hip/api_instances.hip) and the host helpers (host/pose.cpp).  No HIP types.
#ifndef BLOK_POSE_CORE_H
#define BLOK_POSE_CORE_H
#include <stdint.h>

#include "blok_hip.h"
#include "stamp_core.h"

namespace blok {
namespace pose {

constexpr float kMaxM = 1024.0f, kMaxPoint = 1048576.0f;       // |m_kj| <= 2^10; |pivot_j|, |local_k| <= 2^20

// 0 = fine, otherwise the rule that failed (rule_text).
enum Rule { kFine = 0, kNotFinite, kMatrix, kPivot, kLocal };
inline const char* rule_text(int rule) {
    static const char* const kText[] = {"", "a value is not finite", "|m| above 1024", "|pivot| above 2^20", "|local| above 2^20"};
    return kText[rule];
}

// x is neither infinite nor NaN, by its exponent bits.
BLOK_STAMP_HD bool finite(float x) { return (__builtin_bit_cast(uint32_t, x) & 0x7F800000u) != 0x7F800000u; }

BLOK_STAMP_HD int floats_rule(const blok_pose& P) {
    for (int k = 0; k < 3; ++k) {
        for (int j = 0; j < 3; ++j) if (!finite(P.m[k][j])) return kNotFinite;
        if (!finite(P.pivot[k]) || !finite(P.local[k])) return kNotFinite;
    }
    for (int k = 0; k < 3; ++k) {
        for (int j = 0; j < 3; ++j) if (!(__builtin_fabsf(P.m[k][j]) <= kMaxM)) return kMatrix;
    }
    for (int k = 0; k < 3; ++k) if (!(__builtin_fabsf(P.pivot[k]) <= kMaxPoint)) return kPivot;
    for (int k = 0; k < 3; ++k) if (!(__builtin_fabsf(P.local[k]) <= kMaxPoint)) return kLocal;
    return kFine;
}

}  // namespace pose
}  // namespace blok
#endif
