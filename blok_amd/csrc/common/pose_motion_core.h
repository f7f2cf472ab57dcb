// Object motion of posed models (include/blok_hip.h, "Object motion for posed models"): the tracking rule and the build of
// one blok_pose_motion record from this frame's and the previous frame's blok_pose.  Shared by the prepare kernel (hip/post_kernels.hip),
// the host helper blok_pose_motion_record (host/pose.cpp) and the CPU shim of the tests.  No HIP types.
//
// The record carries prev o cur^-1 about the two pivots: a world point p on the pose was, one frame earlier, at
//   p_prev = pivot_prev + A (p - pivot_cur) + c,      A = prev.m^-1 cur.m,      c = prev.m^-1 (cur.local - prev.local)
// (both frames put the point on the same LOCAL point: cur.m (p - pivot_cur) + cur.local = prev.m (p_prev - pivot_prev) + prev.local), and
// its normal goes over by A^-T = cof(A) / det(A); the per-pixel normalisation takes the magnitude, so the record keeps cof(A) with the sign
// of det(A) and needs neither a second inverse nor an invertible cur.
//
// State 2 is computed in double, every operation rounded separately in the order written below (the units are built with
// -ffp-contract=off): IEEE add, multiply and one divide, no square root, so a numpy float64 restatement gives the same bits.
#ifndef BLOK_POSE_MOTION_CORE_H
#define BLOK_POSE_MOTION_CORE_H
#include <stdint.h>

#include "blok_hip.h"
#include "pose_core.h"

#if defined(__clang__)
#pragma clang fp contract(off)
#endif

namespace blok {
namespace pose {

static_assert(sizeof(blok_pose_motion) == 128, "one motion record is 128 bytes, a cache line");

constexpr double kDetFloor = 1.0 / 1048576.0;                 // = posed_core.h's kPoseDetFloor: |det| <= this * the product of the row norms
constexpr double kDetFloorSquared = kDetFloor * kDetFloor;    // 2^-40, exact

BLOK_STAMP_HD bool same_bytes(const blok_pose& a, const blok_pose& b) {
    bool same = a.model == b.model;
    for (int k = 0; k < 3; ++k) {
        for (int j = 0; j < 3; ++j) same = same && __builtin_bit_cast(uint32_t, a.m[k][j]) == __builtin_bit_cast(uint32_t, b.m[k][j]);
        same = same && __builtin_bit_cast(uint32_t, a.pivot[k]) == __builtin_bit_cast(uint32_t, b.pivot[k]) &&
               __builtin_bit_cast(uint32_t, a.local[k]) == __builtin_bit_cast(uint32_t, b.local[k]);
    }
    return same;
}

// adj: the adjugate of the row-major 3 x 3 matrix m, in the term order of pose_world_box (posed_core.h); returns the determinant.
BLOK_STAMP_HD double adjugate(const double m[9], double adj[9]) {
    adj[0] = m[4] * m[8] - m[5] * m[7]; adj[1] = m[2] * m[7] - m[1] * m[8]; adj[2] = m[1] * m[5] - m[2] * m[4];
    adj[3] = m[5] * m[6] - m[3] * m[8]; adj[4] = m[0] * m[8] - m[2] * m[6]; adj[5] = m[2] * m[3] - m[0] * m[5];
    adj[6] = m[3] * m[7] - m[4] * m[6]; adj[7] = m[1] * m[6] - m[0] * m[7]; adj[8] = m[0] * m[4] - m[1] * m[3];
    return (m[0] * adj[0] + m[1] * adj[3]) + m[2] * adj[6];
}

// The record of pose `cur` that was `prev` one frame earlier (has_prev false: the index lies beyond the previous table, prev is not read).
// model_usable: the model cur names is live and passes the pose limits of the store (posed_core.h: pose_usable without the floats).  Every
// word of `out` is written: state 0 and 1 leave all others zero.
BLOK_STAMP_HD void motion_record(const blok_pose& cur, const blok_pose& prev, bool has_prev, bool model_usable, blok_pose_motion& out) {
    out.state = 0u;
    for (int i = 0; i < 3; ++i) {
        for (int j = 0; j < 3; ++j) { out.a[i][j] = 0.0f; out.n[i][j] = 0.0f; }
        out.c[i] = 0.0f; out.pivot_cur[i] = 0.0f; out.pivot_prev[i] = 0.0f;
    }
    for (int k = 0; k < 4; ++k) out.reserved[k] = 0u;
    if (!has_prev || !model_usable || prev.model != cur.model) return;
    if (floats_rule(cur) != kFine || floats_rule(prev) != kFine) return;
    if (same_bytes(cur, prev)) { out.state = 1u; return; }           // the identity, with no arithmetic (and no inverse: prev may be singular)

    double pm[9], cm[9], adj[9];
    for (int k = 0; k < 3; ++k)
        for (int j = 0; j < 3; ++j) { pm[3 * k + j] = prev.m[k][j]; cm[3 * k + j] = cur.m[k][j]; }
    const double det = adjugate(pm, adj);
    const double s0 = (pm[0] * pm[0] + pm[1] * pm[1]) + pm[2] * pm[2], s1 = (pm[3] * pm[3] + pm[4] * pm[4]) + pm[5] * pm[5],
                 s2 = (pm[6] * pm[6] + pm[7] * pm[7]) + pm[8] * pm[8];
    if (!(det * det > kDetFloorSquared * ((s0 * s1) * s2))) return;   // prev is singular in float terms (NaN cannot occur: the floats are bounded)
    const double id = 1.0 / det;
    double inv[9], A[9], c[3], dl[3];
    for (int k = 0; k < 9; ++k) inv[k] = adj[k] * id;
    for (int j = 0; j < 3; ++j) dl[j] = static_cast<double>(cur.local[j]) - static_cast<double>(prev.local[j]);
    for (int i = 0; i < 3; ++i) {
        for (int j = 0; j < 3; ++j) A[3 * i + j] = (inv[3 * i] * cm[j] + inv[3 * i + 1] * cm[3 + j]) + inv[3 * i + 2] * cm[6 + j];
        c[i] = (inv[3 * i] * dl[0] + inv[3 * i + 1] * dl[1]) + inv[3 * i + 2] * dl[2];
    }
    double adjA[9];
    const double detA = adjugate(A, adjA);
    const bool negate = detA < 0.0;
    bool all_finite = true;
    for (int i = 0; i < 3; ++i) {
        for (int j = 0; j < 3; ++j) {
            out.a[i][j] = static_cast<float>(A[3 * i + j]);
            const double cof = adjA[3 * j + i];                        // the cofactor matrix is the adjugate's transpose
            out.n[i][j] = static_cast<float>(negate ? -cof : cof);
            all_finite = all_finite && finite(out.a[i][j]) && finite(out.n[i][j]);
        }
        out.c[i] = static_cast<float>(c[i]);
        all_finite = all_finite && finite(out.c[i]);
    }
    if (!all_finite) {
        for (int i = 0; i < 3; ++i) {
            for (int j = 0; j < 3; ++j) { out.a[i][j] = 0.0f; out.n[i][j] = 0.0f; }
            out.c[i] = 0.0f;
        }
        return;
    }
    for (int i = 0; i < 3; ++i) { out.pivot_cur[i] = cur.pivot[i]; out.pivot_prev[i] = prev.pivot[i]; }
    out.state = 2u;
}

}  // namespace pose
}  // namespace blok
#endif
