// A model resampled into a voxel volume through an affine map (include/blok_hip.h: blok_hip_volume_stamp_affine has the contract).  The one
// place the map's arithmetic lives: the kernel (hip/affine_kernels.hip), the entry's cull (the same file) and the host build
// (host/affine.cpp) all include this header.  No HIP types.  Integer arithmetic only.
//
// The rule.  For a world voxel w:  P_k(w) = t_k + sum_j m[k][j] * (w_j - anchor_j),  v_k = P_k >> 16  (arithmetic: a floor).
//
// No sum here overflows.  A well-formed record (well_formed below, against the box it is used on) has
//   |m[k][j]| <= 2^22,   |t_k| <= 2^40,   |w_j - anchor_j| < 2^20 for every cell w of the box,
// so every product is below 2^42 in magnitude and
//   |P_k(w)| <= 2^40 + 3 * 2^22 * (2^20 - 1) < 2^40 + 3 * 2^42 = 13 * 2^40 < 2^44.
// The kernels do not evaluate P from the record but from a Frame: the same sum regrouped around the box's corner, with a model-space origin o
// (|o_k| <= 2^23: a model's box lies within 2^22 of zero and its tree's corner at most 16 below it) taken off,
//   P'_k(c) = base_k + sum_j m[k][j] * c_j,   base_k = t_k + sum_j m[k][j] * (box_origin_j - anchor_j) - o_k * 2^16,   c = w - box_origin.
// base is P(box_origin) - o * 2^16, and every partial sum of base + m * c taken term by term is P at a cell of the box (the cell whose
// later coordinates are still the corner's) minus o * 2^16: all of them are below 13 * 2^40 + 2^39 < 2^44 < 2^45.  Integer addition without overflow is
// associative, so P'(c) >> 16 = (P(w) >> 16) - o exactly: host and device agree bit for bit however they group the sum.
// tile_interval adds to a corner's value, per term, min or max of 0 and m * (extent - 1): each partial sum is again P' at a corner of the
// tile, so the same bound holds, and the result is exact — the extremes of a sum of independent monotone terms over a box.
#ifndef BLOK_AFFINE_CORE_H
#define BLOK_AFFINE_CORE_H
#include <stdint.h>

#include "blok_hip.h"
#include "stamp_core.h"

namespace blok {
namespace affine {

constexpr int64_t kMaxM = int64_t(1) << 22, kMaxT = int64_t(1) << 40, kMaxReach = int64_t(1) << 20;
constexpr uint32_t kMaxScaleLog2 = 8;      // from_instance: the exponents blok_hip_model_set_scale takes

// 0 = fine, otherwise the rule that failed (rule_text).
enum Rule { kFine = 0, kReserved, kMatrix, kTranslation, kAnchor };
inline const char* rule_text(int rule) {
    static const char* const kText[] = {"", "reserved word not zero", "|m| above 2^22", "|t| above 2^40", "a cell of the box lies 2^20 or more from the anchor"};
    return kText[rule];
}

// The record against the box of `dims` cells at world `origin` it is to be used on.
BLOK_STAMP_HD int well_formed(const blok_affine& A, const int32_t origin[3], const uint32_t dims[3]) {
    if (A.reserved[0] | A.reserved[1] | A.reserved[2] | A.reserved[3] | A.reserved[4]) return kReserved;
    for (int k = 0; k < 3; ++k) {
        for (int j = 0; j < 3; ++j) if (A.m[k][j] > kMaxM || A.m[k][j] < -kMaxM) return kMatrix;
        if (A.t[k] > kMaxT || A.t[k] < -kMaxT) return kTranslation;
    }
    for (int j = 0; j < 3; ++j) {
        const int64_t first = int64_t(origin[j]) - A.anchor[j], last = first + int64_t(dims[j]) - 1;      // (a box without a cell has none out of reach)
        if (dims[j] && (first <= -kMaxReach || first >= kMaxReach || last <= -kMaxReach || last >= kMaxReach)) return kAnchor;
    }
    return kFine;
}

// The rule itself, from the record: the model voxel a world voxel samples.
BLOK_STAMP_HD void sample(const blok_affine& A, const int64_t w[3], int64_t v[3]) {
    for (int k = 0; k < 3; ++k) {
        int64_t P = A.t[k];
        for (int j = 0; j < 3; ++j) P += int64_t(A.m[k][j]) * (w[j] - int64_t(A.anchor[j]));
        v[k] = P >> 16;
    }
}

// The record as seen from a box (the header's comment): P'(c) for the box-local cell c, model coordinates counted from `model_origin`.
struct Frame {
    int64_t base[3];
    int32_t m[3][3];
};
BLOK_STAMP_HD Frame frame(const blok_affine& A, const int32_t box_origin[3], const int32_t model_origin[3]) {
    Frame F;
    for (int k = 0; k < 3; ++k) {
        int64_t P = A.t[k];
        for (int j = 0; j < 3; ++j) { F.m[k][j] = A.m[k][j]; P += int64_t(A.m[k][j]) * (int64_t(box_origin[j]) - int64_t(A.anchor[j])); }
        F.base[k] = P - int64_t(model_origin[k]) * 65536;
    }
    return F;
}
// P'_k of the box-local cell (x, y, z).
BLOK_STAMP_HD int64_t value(const Frame& F, int k, uint32_t x, uint32_t y, uint32_t z) {
    return F.base[k] + int64_t(F.m[k][0]) * int64_t(x) + int64_t(F.m[k][1]) * int64_t(y) + int64_t(F.m[k][2]) * int64_t(z);
}
BLOK_STAMP_HD int64_t voxel(int64_t P) { return P >> 16; }

// The exact range of P'_k over the cells [tile_lo, tile_lo + extent) (extent >= 1 on every axis): [Plo[k], Phi[k]], both ends attained.
BLOK_STAMP_HD void tile_interval(const Frame& F, const uint32_t tile_lo[3], const uint32_t extent[3], int64_t Plo[3], int64_t Phi[3]) {
    for (int k = 0; k < 3; ++k) {
        int64_t lo = value(F, k, tile_lo[0], tile_lo[1], tile_lo[2]), hi = lo;
        for (int j = 0; j < 3; ++j) {
            const int64_t d = int64_t(F.m[k][j]) * int64_t(extent[j] - 1u);
            if (d < 0) lo += d; else hi += d;
        }
        Plo[k] = lo; Phi[k] = hi;
    }
}
// Does the voxel range of an interval meet the model-local box [blo, bhi)?
BLOK_STAMP_HD bool meets(const int64_t Plo[3], const int64_t Phi[3], const int32_t blo[3], const int32_t bhi[3]) {
    bool hit = true;
    for (int k = 0; k < 3; ++k) hit = hit && voxel(Phi[k]) >= int64_t(blo[k]) && voxel(Plo[k]) < int64_t(bhi[k]);
    return hit;
}

// A placement and a scale exponent e as a record, exactly (blok_hip.h, "Scaled models": the cells the tracer shows).  For local axis k
// along world axis a = axis[k]:  v_k = floor((w_a - o_a) / 2^e), or floor((o_a - 1 - w_a) / 2^e) under a flip.  With d = w_a - o_a, an
// integer, floor(d / 2^e) = floor((d + 1/2) / 2^e) and floor((-d - 1) / 2^e) = floor((-d - 1/2) / 2^e): m = +-2^(16 - e), t = +-2^(15 - e).
// False: a malformed placement or e above kMaxScaleLog2.
BLOK_STAMP_HD bool from_instance(const blok_instance& I, uint32_t scale_log2, blok_affine& out) {
    if (!stamp::well_formed(I) || scale_log2 > kMaxScaleLog2) return false;
    out = blok_affine{};
    out.model = I.model;
    for (int j = 0; j < 3; ++j) out.anchor[j] = I.offset[j];
    for (uint32_t k = 0; k < 3u; ++k) {
        const int32_t sign = ((I.flip >> k) & 1u) ? -1 : 1;
        out.m[k][I.axis[k]] = sign * (int32_t(1) << (16u - scale_log2));
        out.t[k] = int64_t(sign) * (int64_t(1) << (15u - scale_log2));
    }
    return true;
}

}  // namespace affine
}  // namespace blok
#endif
