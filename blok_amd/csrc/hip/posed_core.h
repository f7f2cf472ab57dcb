// Posed models (include/blok_hip.h: blok_pose, "Posed models"): the device math of the posed kernels (placed_kernels.hip over
// PoseKind, at the end of this file).
//
// A pose places a model under any affine map.  The ray goes into local space by the rule below, every operation rounded separately
// (the units are built with -ffp-contract=off), the local walk is the canonical walk of trace_core.h at the model's own voxel size, and
// the record keeps the LOCAL voxel and face: the composed record is specified bit for bit, as a lattice instance's is.
//   r_j  = fl(o_j - pivot_j)
//   o'_k = fl( fl( fl( fl(m_k0 r_0) + fl(m_k1 r_1) ) + fl(m_k2 r_2) ) + local_k )
//   d'_k = fl( fl( fl(m_k0 d_0) + fl(m_k1 d_1) ) + fl(m_k2 d_2) )             tmin, tmax unchanged; d' is not renormalised
// A ray whose o' or d' is not finite does not enter the pose.  Candidates come after the world and the lattice instances, pose 0, 1, ...;
// one replaces the record only with a strictly smaller t.
//
// Face codes.  trace_core.h: walk_hit reports face 2k + n with n = 0 where the hit point lies on the + side of the voxel's centre along
// axis k (ex > 0 -> face 0): n = 0 is the face whose outward normal is +local axis k.  A plane's normal goes back to the world through the
// transpose of the world -> local map: +local axis k becomes row k of m.  So the outward world normal of face 2k + n is parallel to
// s * (m_k0, m_k1, m_k2), s = +1 for n = 0, -1 for n = 1 (pose_shade_face).
//
// The screen bins' margin (pose_world_box).  The bins must list a pose for every pixel whose ray the pose's walk reports a voxel for.
// Such a ray has a parameter t at which the LOCAL point p' = o' + t d' lies in the model's box [lo, hi) * vs, up to the rounding of the
// walk's plane parameters (T = fl(fl(p - o') * inv): three roundings, a displacement below 3u |p - o'| per axis, u = 2^-24).  Were o' and d'
// exact, p' would be m (w - pivot) + local for the world point w = o + t d of the pixel's ray.  They are rounded: along local axis k
//   |o'_k - exact| <= 5u (S_k(|r|) + |local_k|),   |d'_k - exact| <= 3u S_k(|d|),   S_k(x) = sum_j |m_kj| x_j
// (r_j carries one rounding, each product one, each of the three sums one; every partial sum is bounded by S_k + |local_k|).  So the exact
// image of w lies within
//   delta_k = 16u (S_k(|r| + t |d|) + |local_k| + max(|lo_k|, |hi_k|) vs)
// of the box along local axis k: 5 + 3 + 3 ulps of terms each bounded by the bracket, rounded up to 16.  |r_j| + t |d_j| is bounded
// by 2 |cam_j - pivot_j| + B_j where B_j bounds |w_j - pivot_j| over the preimage (t |d_j| = |w_j - o_j| <= |w_j - pivot_j| + |pivot_j - o_j|;
// B is taken over the box widened by twice itself, pass 1 below, which absorbs the second-order term).  Hence w lies in the preimage of the
// box WIDENED by delta in local space, w = pivot + m^-1 (c - local): a parallelepiped, whose bounding box is that of its 8 corners.  The map
// back is linear and costs nothing in tightness; the conditioning of m enters only through m^-1, which stretches delta exactly as it
// stretches the box.  m^-1 is formed in double (adjugate over determinant): with |det| above 2^-20 of the product of the row norms its
// relative error is below 2^-30, and the box is finally widened by 2^-20 of its own magnitude, which also covers the conversion to float.
// What remains is project_box's own 1-pixel margin, argued in instance_core.h for the rounding of the primary ray and of the projection:
// unchanged.  A pose with |det| at or below that floor (rank < 3 in float terms), or any non-finite result, covers every bin — the
// fallback project_box returning false already has.  tests/test_posed_instances_*.py hold the bins against the unbinned rays kernel.
#ifndef BLOK_POSED_CORE_H
#define BLOK_POSED_CORE_H

#include "instance_core.h"
#include "../common/pose_core.h"

#if defined(__clang__)
#define BLOK_POSE_UNROLL _Pragma("unroll")
#else
#define BLOK_POSE_UNROLL
#endif

namespace blok {

static_assert(sizeof(blok_pose) == 64, "one pose record is 64 bytes");

constexpr double kPoseDetFloor = 1.0 / 1048576.0;       // |det| <= this * product of the row norms: the pose covers every bin
constexpr double kPoseUlps = 16.0 / 16777216.0;         // 16 u, u = 2^-24 (the margin argument above)

// Everything the blocking entries check, for the kernels (a pose of the device entries that fails it is skipped).  M: the store's device
// copy of the descriptor (nodes == null: destroyed, or too large a voxel in this world).  The record's voxel is the model's own, int16.
BLOK_HD bool pose_model_box_usable(const ModelDesc& M) {
    for (uint32_t a = 0; a < 3u; ++a) {
        const int64_t lo = static_cast<int64_t>(M.lo[a]) >> M.scale_log2, hi = static_cast<int64_t>(M.hi[a]) >> M.scale_log2;      // (multiples of 2^e: exact)
        if (lo < kLatticeMin || hi > kLatticeMax) return false;
    }
    return true;
}
BLOK_HD bool pose_usable(const blok_pose& P, const ModelDesc& M) {
    return pose::floats_rule(P) == pose::kFine && M.nodes && pose_model_box_usable(M);
}

// The ray in the pose's local space.  false: a component is not finite, the ray does not enter the pose (l is then not to be walked).
BLOK_DEV bool pose_ray(const blok_pose& P, const RayIn& r, RayIn& l) {
    const float r0 = rn_sub(r.ox, P.pivot[0]), r1 = rn_sub(r.oy, P.pivot[1]), r2 = rn_sub(r.oz, P.pivot[2]);
    l.ox = rn_add(rn_add(rn_add(rn_mul(P.m[0][0], r0), rn_mul(P.m[0][1], r1)), rn_mul(P.m[0][2], r2)), P.local[0]);
    l.oy = rn_add(rn_add(rn_add(rn_mul(P.m[1][0], r0), rn_mul(P.m[1][1], r1)), rn_mul(P.m[1][2], r2)), P.local[1]);
    l.oz = rn_add(rn_add(rn_add(rn_mul(P.m[2][0], r0), rn_mul(P.m[2][1], r1)), rn_mul(P.m[2][2], r2)), P.local[2]);
    l.dx = rn_add(rn_add(rn_mul(P.m[0][0], r.dx), rn_mul(P.m[0][1], r.dy)), rn_mul(P.m[0][2], r.dz));
    l.dy = rn_add(rn_add(rn_mul(P.m[1][0], r.dx), rn_mul(P.m[1][1], r.dy)), rn_mul(P.m[1][2], r.dz));
    l.dz = rn_add(rn_add(rn_mul(P.m[2][0], r.dx), rn_mul(P.m[2][1], r.dy)), rn_mul(P.m[2][2], r.dz));
    l.tmin = r.tmin; l.tmax = r.tmax;
    return pose::finite(l.ox) && pose::finite(l.oy) && pose::finite(l.oz) && pose::finite(l.dx) && pose::finite(l.dy) && pose::finite(l.dz);
}

// A local hit as a record (the 16-byte blok_hit layout): the model's local voxel and the local face.
BLOK_DEV uint4 pose_record(const HitInfo& h) {
    uint4 rec;
    rec.x = __float_as_uint(h.t);
    rec.y = h.material;
    rec.z = (static_cast<uint32_t>(h.vx) & 0xFFFFu) | (static_cast<uint32_t>(h.vy) << 16);
    rec.w = (static_cast<uint32_t>(h.vz) & 0xFFFFu) | (h.face << 16) | (1u << 24);
    return rec;
}

// The world face shade_rgba takes for local face 2k + n: of s * row k of m the component of largest magnitude (ties: the lowest axis)
// names the axis, its sign the side (a zero counts as positive).  Shading only.
BLOK_DEV uint32_t pose_shade_face(const blok_pose& P, uint32_t face) {
    const uint32_t k = face >> 1;
    const float s = (face & 1u) ? -1.0f : 1.0f;
    const float x = s * pick3(k, P.m[0][0], P.m[1][0], P.m[2][0]);
    const float y = s * pick3(k, P.m[0][1], P.m[1][1], P.m[2][1]);
    const float z = s * pick3(k, P.m[0][2], P.m[1][2], P.m[2][2]);
    const float ax = fabsf(x), ay = fabsf(y), az = fabsf(z);
    if (ax >= ay && ax >= az) return x < 0.0f ? 1u : 0u;
    if (ay >= az) return y < 0.0f ? 3u : 2u;
    return z < 0.0f ? 5u : 4u;
}

// The world box [flo, fhi] (world units) that holds every world point a ray can have where the pose's walk reports a voxel, for a camera at
// `cam`: the margin argument at the head of this file.  false: the pose may cover anything (a degenerate m, a non-finite result).
BLOK_DEV bool pose_world_box(const blok_pose& P, const ModelDesc& M, float vs, const float cam[3], float flo[3], float fhi[3]) {
    const double m00 = P.m[0][0], m01 = P.m[0][1], m02 = P.m[0][2], m10 = P.m[1][0], m11 = P.m[1][1], m12 = P.m[1][2],
                 m20 = P.m[2][0], m21 = P.m[2][1], m22 = P.m[2][2];
    // adjugate: inv[j][k] = c_jk / det
    const double c00 = m11 * m22 - m12 * m21, c01 = m02 * m21 - m01 * m22, c02 = m01 * m12 - m02 * m11;
    const double c10 = m12 * m20 - m10 * m22, c11 = m00 * m22 - m02 * m20, c12 = m02 * m10 - m00 * m12;
    const double c20 = m10 * m21 - m11 * m20, c21 = m01 * m20 - m00 * m21, c22 = m00 * m11 - m01 * m10;
    const double det = m00 * c00 + m01 * c10 + m02 * c20;
    const double norms = __builtin_sqrt(m00 * m00 + m01 * m01 + m02 * m02) * __builtin_sqrt(m10 * m10 + m11 * m11 + m12 * m12) *
                         __builtin_sqrt(m20 * m20 + m21 * m21 + m22 * m22);
    if (!(__builtin_fabs(det) > kPoseDetFloor * norms)) return false;
    const double id = 1.0 / det;
    const double i00 = c00 * id, i01 = c01 * id, i02 = c02 * id, i10 = c10 * id, i11 = c11 * id, i12 = c12 * id, i20 = c20 * id, i21 = c21 * id, i22 = c22 * id;
    const double l0 = P.local[0], l1 = P.local[1], l2 = P.local[2];
    const double v = vs;
    const double blo0 = M.lo[0] * v, blo1 = M.lo[1] * v, blo2 = M.lo[2] * v, bhi0 = M.hi[0] * v, bhi1 = M.hi[1] * v, bhi2 = M.hi[2] * v;
    // pass 1: how far the preimage reaches from the pivot, B_j (doubled: the widened box of pass 2 stays inside it unless delta exceeds the
    // box's own reach, and then the final check below fails over to "covers everything")
    double B0 = 0.0, B1 = 0.0, B2 = 0.0;
    BLOK_POSE_UNROLL
    for (int c = 0; c < 8; ++c) {
        const double x = ((c & 1) ? bhi0 : blo0) - l0, y = ((c & 2) ? bhi1 : blo1) - l1, z = ((c & 4) ? bhi2 : blo2) - l2;
        B0 = __builtin_fmax(B0, __builtin_fabs(i00 * x + i01 * y + i02 * z));
        B1 = __builtin_fmax(B1, __builtin_fabs(i10 * x + i11 * y + i12 * z));
        B2 = __builtin_fmax(B2, __builtin_fabs(i20 * x + i21 * y + i22 * z));
    }
    B0 *= 2.0; B1 *= 2.0; B2 *= 2.0;
    const double q0 = 2.0 * __builtin_fabs(double(cam[0]) - double(P.pivot[0])) + B0, q1 = 2.0 * __builtin_fabs(double(cam[1]) - double(P.pivot[1])) + B1,
                 q2 = 2.0 * __builtin_fabs(double(cam[2]) - double(P.pivot[2])) + B2;
    const double d0 = kPoseUlps * (__builtin_fabs(m00) * q0 + __builtin_fabs(m01) * q1 + __builtin_fabs(m02) * q2 + __builtin_fabs(l0) + __builtin_fmax(__builtin_fabs(blo0), __builtin_fabs(bhi0)));
    const double d1 = kPoseUlps * (__builtin_fabs(m10) * q0 + __builtin_fabs(m11) * q1 + __builtin_fabs(m12) * q2 + __builtin_fabs(l1) + __builtin_fmax(__builtin_fabs(blo1), __builtin_fabs(bhi1)));
    const double d2 = kPoseUlps * (__builtin_fabs(m20) * q0 + __builtin_fabs(m21) * q1 + __builtin_fabs(m22) * q2 + __builtin_fabs(l2) + __builtin_fmax(__builtin_fabs(blo2), __builtin_fabs(bhi2)));
    // pass 2: the bounding box of the widened box's preimage
    double lo0 = 1.0e300, lo1 = 1.0e300, lo2 = 1.0e300, hi0 = -1.0e300, hi1 = -1.0e300, hi2 = -1.0e300;
    double R0 = 0.0, R1 = 0.0, R2 = 0.0;
    BLOK_POSE_UNROLL
    for (int c = 0; c < 8; ++c) {
        const double x = ((c & 1) ? bhi0 + d0 : blo0 - d0) - l0, y = ((c & 2) ? bhi1 + d1 : blo1 - d1) - l1, z = ((c & 4) ? bhi2 + d2 : blo2 - d2) - l2;
        const double w0 = i00 * x + i01 * y + i02 * z, w1 = i10 * x + i11 * y + i12 * z, w2 = i20 * x + i21 * y + i22 * z;
        R0 = __builtin_fmax(R0, __builtin_fabs(w0)); R1 = __builtin_fmax(R1, __builtin_fabs(w1)); R2 = __builtin_fmax(R2, __builtin_fabs(w2));
        lo0 = __builtin_fmin(lo0, w0); hi0 = __builtin_fmax(hi0, w0);
        lo1 = __builtin_fmin(lo1, w1); hi1 = __builtin_fmax(hi1, w1);
        lo2 = __builtin_fmin(lo2, w2); hi2 = __builtin_fmax(hi2, w2);
    }
    if (!(R0 <= B0 && R1 <= B1 && R2 <= B2)) return false;           // the margin outgrew the bound it was formed from (NaN included)
    const double p0 = P.pivot[0], p1 = P.pivot[1], p2 = P.pivot[2];
    constexpr double kRel = 1.0 / 1048576.0;
    const double e0 = kRel * (__builtin_fabs(p0) + R0), e1 = kRel * (__builtin_fabs(p1) + R1), e2 = kRel * (__builtin_fabs(p2) + R2);
    flo[0] = static_cast<float>(p0 + lo0 - e0); fhi[0] = static_cast<float>(p0 + hi0 + e0);
    flo[1] = static_cast<float>(p1 + lo1 - e1); fhi[1] = static_cast<float>(p1 + hi1 + e1);
    flo[2] = static_cast<float>(p2 + lo2 - e2); fhi[2] = static_cast<float>(p2 + hi2 + e2);
    return pose::finite(flo[0]) && pose::finite(flo[1]) && pose::finite(flo[2]) && pose::finite(fhi[0]) && pose::finite(fhi[1]) && pose::finite(fhi[2]);
}

// Arguments of the three posed kernels (placed_kernels.hip): the instance kernels' (frame, bins, view, model store, outputs, LDS stack; its
// instance table unused) and the pose table.  The bins are the posed pass's own (per-stream scratch), laid out as the instance bins are.
struct PosedArgs {
    InstanceArgs frame;
    const blok_pose* poses;              // device memory, n_poses records
    uint32_t n_poses;
};

// The poses as a kind of placed model (instance_core.h: what a kind is).
struct PoseKind {
    using Record = blok_pose;
    using Args = PosedArgs;
    static BLOK_DEV const InstanceArgs& frame(const Args& a) { return a.frame; }
    static BLOK_DEV const Record* table(const Args& a) { return a.poses; }
    static BLOK_DEV uint32_t count(const Args& a) { return a.n_poses; }
    static BLOK_DEV bool usable(const Record& S, const ModelDesc& M) { return pose_usable(S, M); }
    static BLOK_DEV bool local_ray(const Record& S, float, const RayIn& r, RayIn& l) { return pose_ray(S, r, l); }
    static BLOK_DEV bool world_box(const Record& S, const ModelDesc& M, float vs, const float cam[3], float flo[3], float fhi[3]) {
        return pose_world_box(S, M, vs, cam, flo, fhi);
    }
    struct Hit {
        uint4 rec{};
        uint32_t face = 0u;                                                           // the record's face is the model's own
        BLOK_DEV uint32_t shade_face() const { return face; }
    };
    static BLOK_DEV Hit record(const Record& S, const ModelDesc&, const HitInfo& h) { return Hit{pose_record(h), pose_shade_face(S, h.face)}; }
    static constexpr bool owns_ids = false;
    static constexpr uint32_t id_tag = BLOK_POSE_ID;
};

#ifdef BLOK_TRACE_HOST_HARNESS
// One pose's candidate as a plain function, as instance_candidate is one instance's: true (and rec) iff the walk of r with tmax = best_t
// reports a voxel.  For host harnesses that want no kind.
inline bool pose_candidate(const blok_pose& P, const ModelDesc& M, float vs, float inv_vs, const RayIn& r, float best_t, uint4* stk, uint4& rec) {
    PoseKind::Hit hit;
    if (!placed_candidate<PoseKind>(P, M, vs, inv_vs, r, best_t, stk, hit)) return false;
    rec = hit.rec;
    return true;
}
#endif

#ifndef BLOK_TRACE_HOST_HARNESS
void launch_posed_bins(const PosedArgs& args, hipStream_t stream);
void launch_posed_pass(const PosedArgs& args, hipStream_t stream);
void launch_posed_rays(const PosedArgs& args, hipStream_t stream);
#endif

}  // namespace blok
#endif
