// The pose BVH of the posed path frame: a second tree beside the instance BVH of tlas_core.h, in the same node format —
// heap order, Morton sort on the box centre, escape links, the empty-node rule, kTlasMax poses per tree (above: the linear loop).  Build steps
// here, host-compilable (tests/host_harness/pose_tlas_shim.cpp runs them serially; trace_kernels.hip: pose_tlas_build_kernel in one
// workgroup); the traversal is posed_paths_core.h's.  The frame is DEFINED as if every pose were tested for every ray: the tree only skips.
//
// The leaf box.  A leaf's box must hold every world point o + t d at which its pose's walk can report a voxel, for ANY ray of the launch:
// primary rays from the camera, shadow and bounce rays from wherever a path stands.  posed_core.h argues the bound for rays from the
// camera (pose_world_box): the exact image of the ray's point w lies within delta_k = 16u (S_k(|r| + t|d|) + |local_k| + max(|lo_k|, |hi_k|) vs)
// of the model's box, and the origin enters only through |r_j| + t |d_j| <= 2 |o_j - pivot_j| + B_j (t |d_j| = |w_j - o_j| <= |w_j - pivot_j| +
// |pivot_j - o_j|).  Nothing else in that argument knows where the ray starts.  So for origins anywhere in a box [olo, ohi] the term
// 2 |cam_j - pivot_j| becomes 2 max(|olo_j - pivot_j|, |ohi_j - pivot_j|) — the largest |o_j - pivot_j| over the box, |.| being convex —
// and every other line stands (pose_world_box_from: pose_world_box with that one term; pose_world_box stays as it is for its kernels).
// The origin box of a launch is the union of
//   - the camera position (primary rays);
//   - the lattice in world units, [-32768 vs, 32768 vs)^3: every world voxel and every voxel of a usable lattice instance lies there
//     (kLatticeMin / kLatticeMax), so every shadow or bounce ray that leaves a world or instance hit starts there;
//   - every usable pose's own UNWIDENED preimage box (pose_preimage_box): a shadow or bounce ray that leaves a posed hit starts on a pose;
// grown on every side by g = vs + 2^-12 max(|olo|, |ohi|): a path's origin is hit_pos + n * 0.001 or * 0.002 with |n| = 1, and hit_pos = fl(o + t d)
// carries a few float roundings of coordinates below the box's magnitude (2^-12 of it covers 2^12 ulps).  A posed hit lies not in its pose's
// preimage but in the preimage WIDENED by that pose's own margin, delta mapped back to the world: up to x_j = sum_k |inv_jk| delta_k + e_j beyond
// the preimage along world axis j.  The final check of pose_world_box_from (R <= B) only keeps that below the preimage's own reach, which is not
// g; so pose_world_box_from also demands x_j <= g_j / 2 (the other half of g stays for the offsets and roundings above), and a pose that fails it —
// strongly sheared or near-singular, yet usable — gets no box and sets the linear flag like any other pose whose bound fails.  With it every
// origin of the launch lies in O, and the margin argument holds as stated.
// Two passes therefore: the preimages and their union first, the margins, leaves and refit second.
// Boxes are stored as int32 world voxels: floor(flo / vs) and ceil(fhi / vs), clamped to int32 less the pad, then padded by kTlasPad, which
// covers the rounding of the slab test (tlas_box_hit) as it does for the instance tree.
// A usable pose whose bound fails — |det| at or below kPoseDetFloor of the row norms' product, a margin that outgrew its bound, a non-finite
// result — gets no box, and the header's linear flag (node 0: lo[0] = 1) sends every query of the launch through the linear loop over the
// table: the same result, slower, in a rare case.  (A blanket leaf instead would also make the origin box unbounded.)
#ifndef BLOK_POSE_TLAS_CORE_H
#define BLOK_POSE_TLAS_CORE_H

#include "tlas_core.h"
#include "posed_core.h"

namespace blok {

// A box of world points in double: a pose's preimage, the union of them.
struct PoseBoxD { double lo[3], hi[3]; };
// The launch's box of ray origins, and the growth g it was given per axis (the head of this file).
struct PoseOrigins { PoseBoxD box; double g[3]; };

BLOK_DEV PoseBoxD pose_box_empty() { PoseBoxD b; for (int a = 0; a < 3; ++a) { b.lo[a] = 1.0e300; b.hi[a] = -1.0e300; } return b; }
BLOK_DEV void pose_box_join(PoseBoxD& b, const PoseBoxD& o) {
    for (int a = 0; a < 3; ++a) { b.lo[a] = __builtin_fmin(b.lo[a], o.lo[a]); b.hi[a] = __builtin_fmax(b.hi[a], o.hi[a]); }
}

// The adjugate inverse of m in double; false: |det| at or below the floor (posed_core.h).
struct PoseInverse { double i[3][3]; };
BLOK_DEV bool pose_inverse(const blok_pose& P, PoseInverse& inv) {
    const double m00 = P.m[0][0], m01 = P.m[0][1], m02 = P.m[0][2], m10 = P.m[1][0], m11 = P.m[1][1], m12 = P.m[1][2],
                 m20 = P.m[2][0], m21 = P.m[2][1], m22 = P.m[2][2];
    const double c00 = m11 * m22 - m12 * m21, c01 = m02 * m21 - m01 * m22, c02 = m01 * m12 - m02 * m11;
    const double c10 = m12 * m20 - m10 * m22, c11 = m00 * m22 - m02 * m20, c12 = m02 * m10 - m00 * m12;
    const double c20 = m10 * m21 - m11 * m20, c21 = m01 * m20 - m00 * m21, c22 = m00 * m11 - m01 * m10;
    const double det = m00 * c00 + m01 * c10 + m02 * c20;
    const double norms = __builtin_sqrt(m00 * m00 + m01 * m01 + m02 * m02) * __builtin_sqrt(m10 * m10 + m11 * m11 + m12 * m12) *
                         __builtin_sqrt(m20 * m20 + m21 * m21 + m22 * m22);
    if (!(__builtin_fabs(det) > kPoseDetFloor * norms)) return false;
    const double id = 1.0 / det;
    inv.i[0][0] = c00 * id; inv.i[0][1] = c01 * id; inv.i[0][2] = c02 * id;
    inv.i[1][0] = c10 * id; inv.i[1][1] = c11 * id; inv.i[1][2] = c12 * id;
    inv.i[2][0] = c20 * id; inv.i[2][1] = c21 * id; inv.i[2][2] = c22 * id;
    return true;
}

// Pass 1: the bounding box of the UNWIDENED preimage of the model's box, w = pivot + m^-1 (c - local) over its 8 corners.  false: no inverse
// or a non-finite corner (the pose will get no leaf box either).
BLOK_DEV bool pose_preimage_box(const blok_pose& P, const ModelDesc& M, float vs, PoseBoxD& out) {
    PoseInverse inv;
    if (!pose_inverse(P, inv)) return false;
    const double v = vs;
    out = pose_box_empty();
    bool finite = true;
    BLOK_POSE_UNROLL
    for (int c = 0; c < 8; ++c) {
        const double x = ((c & 1) ? M.hi[0] : M.lo[0]) * v - double(P.local[0]), y = ((c & 2) ? M.hi[1] : M.lo[1]) * v - double(P.local[1]),
                     z = ((c & 4) ? M.hi[2] : M.lo[2]) * v - double(P.local[2]);
        for (int j = 0; j < 3; ++j) {
            const double w = double(P.pivot[j]) + (inv.i[j][0] * x + inv.i[j][1] * y + inv.i[j][2] * z);
            finite = finite && (__builtin_fabs(w) < 1.0e300);
            out.lo[j] = __builtin_fmin(out.lo[j], w); out.hi[j] = __builtin_fmax(out.hi[j], w);
        }
    }
    return finite;
}

// The origin box of a launch from the union U of the usable poses' preimages (pass 1's result; empty if there is none): with the camera and
// the lattice, grown by g (the head of this file).
BLOK_DEV PoseOrigins pose_origin_box(const PoseBoxD& U, const float cam[3], float vs) {
    PoseOrigins o;
    o.box = U;
    for (int a = 0; a < 3; ++a) {
        o.box.lo[a] = __builtin_fmin(__builtin_fmin(o.box.lo[a], double(cam[a])), double(kLatticeMin) * double(vs));
        o.box.hi[a] = __builtin_fmax(__builtin_fmax(o.box.hi[a], double(cam[a])), double(kLatticeMax) * double(vs));
        o.g[a] = double(vs) + __builtin_fmax(__builtin_fabs(o.box.lo[a]), __builtin_fabs(o.box.hi[a])) * (1.0 / 4096.0);
        o.box.lo[a] -= o.g[a]; o.box.hi[a] += o.g[a];
    }
    return o;
}

// pose_world_box (posed_core.h) for ray origins anywhere in the box of `origins` instead of at the camera: the one term of the margin that knows the
// origin, 2 |cam_j - pivot_j|, is 2 max(|O.lo_j - pivot_j|, |O.hi_j - pivot_j|).  Everything else is that function's, line for line, plus the
// demand that the pose's own widening in the world stays within half the origin box's growth (the head of this file).
BLOK_DEV bool pose_world_box_from(const blok_pose& P, const ModelDesc& M, float vs, const PoseOrigins& origins, double flo[3], double fhi[3]) {
    const PoseBoxD& O = origins.box;
    PoseInverse inv;
    if (!pose_inverse(P, inv)) return false;
    const double l[3] = {P.local[0], P.local[1], P.local[2]};
    const double v = vs;
    const double blo[3] = {M.lo[0] * v, M.lo[1] * v, M.lo[2] * v}, bhi[3] = {M.hi[0] * v, M.hi[1] * v, M.hi[2] * v};
    double B[3] = {0.0, 0.0, 0.0};
    BLOK_POSE_UNROLL
    for (int c = 0; c < 8; ++c) {
        const double x = ((c & 1) ? bhi[0] : blo[0]) - l[0], y = ((c & 2) ? bhi[1] : blo[1]) - l[1], z = ((c & 4) ? bhi[2] : blo[2]) - l[2];
        for (int j = 0; j < 3; ++j) B[j] = __builtin_fmax(B[j], __builtin_fabs(inv.i[j][0] * x + inv.i[j][1] * y + inv.i[j][2] * z));
    }
    double q[3], d[3];
    for (int j = 0; j < 3; ++j) {
        B[j] *= 2.0;
        q[j] = 2.0 * __builtin_fmax(__builtin_fabs(O.lo[j] - double(P.pivot[j])), __builtin_fabs(O.hi[j] - double(P.pivot[j]))) + B[j];
    }
    for (int k = 0; k < 3; ++k)
        d[k] = kPoseUlps * (__builtin_fabs(double(P.m[k][0])) * q[0] + __builtin_fabs(double(P.m[k][1])) * q[1] + __builtin_fabs(double(P.m[k][2])) * q[2] +
                            __builtin_fabs(l[k]) + __builtin_fmax(__builtin_fabs(blo[k]), __builtin_fabs(bhi[k])));
    double lo[3] = {1.0e300, 1.0e300, 1.0e300}, hi[3] = {-1.0e300, -1.0e300, -1.0e300}, R[3] = {0.0, 0.0, 0.0};
    BLOK_POSE_UNROLL
    for (int c = 0; c < 8; ++c) {
        const double x = ((c & 1) ? bhi[0] + d[0] : blo[0] - d[0]) - l[0], y = ((c & 2) ? bhi[1] + d[1] : blo[1] - d[1]) - l[1],
                     z = ((c & 4) ? bhi[2] + d[2] : blo[2] - d[2]) - l[2];
        for (int j = 0; j < 3; ++j) {
            const double w = inv.i[j][0] * x + inv.i[j][1] * y + inv.i[j][2] * z;
            R[j] = __builtin_fmax(R[j], __builtin_fabs(w));
            lo[j] = __builtin_fmin(lo[j], w); hi[j] = __builtin_fmax(hi[j], w);
        }
    }
    if (!(R[0] <= B[0] && R[1] <= B[1] && R[2] <= B[2])) return false;           // the margin outgrew the bound it was formed from (NaN included)
    constexpr double kRel = 1.0 / 1048576.0;
    bool finite = true;
    for (int j = 0; j < 3; ++j) {
        const double p = P.pivot[j], e = kRel * (__builtin_fabs(p) + R[j]);
        const double x = (__builtin_fabs(inv.i[j][0]) * d[0] + __builtin_fabs(inv.i[j][1]) * d[1] + __builtin_fabs(inv.i[j][2]) * d[2]) + e;
        if (!(x <= 0.5 * origins.g[j])) return false;                             // a hit on this pose could start a ray outside the origin box
        flo[j] = p + lo[j] - e; fhi[j] = p + hi[j] + e;
        finite = finite && __builtin_fabs(flo[j]) < 1.0e300 && __builtin_fabs(fhi[j]) < 1.0e300;
    }
    return finite;
}

// What the build makes of pose i.
enum PoseLeafKind : uint32_t { kPoseLeafSkipped = 0u, kPoseLeafBoxed = 1u, kPoseLeafUnbounded = 2u };   // not usable; has a box; usable, its bound fails

// The leaf box of pose i in int32 world voxels, padded: rounded outwards, clamped to int32 less the pad.
BLOK_DEV PoseLeafKind pose_leaf_box(const blok_pose* poses, const ModelDesc* models, uint32_t n_models, uint32_t i, float vs, const PoseOrigins& O,
                                    int32_t lo[3], int32_t hi[3]) {
    const blok_pose P = poses[i];
    if (P.model >= n_models) return kPoseLeafSkipped;
    const ModelDesc M = models[P.model];
    if (!pose_usable(P, M)) return kPoseLeafSkipped;
    double flo[3], fhi[3];
    if (!pose_world_box_from(P, M, vs, O, flo, fhi)) return kPoseLeafUnbounded;
    constexpr double kMin = -2147483648.0 + kTlasPad, kMax = 2147483647.0 - kTlasPad;
    for (int a = 0; a < 3; ++a) {
        const double l = __builtin_floor(flo[a] / double(vs)), h = __builtin_ceil(fhi[a] / double(vs));
        lo[a] = static_cast<int32_t>(__builtin_fmin(__builtin_fmax(l, kMin), kMax)) - kTlasPad;
        hi[a] = static_cast<int32_t>(__builtin_fmin(__builtin_fmax(h, kMin), kMax)) + kTlasPad;
    }
    return kPoseLeafBoxed;
}

// The sort key of pose i: (Morton of the leaf box's centre << 32) | i, the centre clamped to the 10-bit cells of tlas_key's lattice;
// (0xFFFFFFFF << 32) | i for a pose without a box (sorted last).  kind: what the pose is.
BLOK_DEV uint64_t pose_tlas_key(const blok_pose* poses, const ModelDesc* models, uint32_t n_models, uint32_t i, float vs, const PoseOrigins& O, PoseLeafKind& kind) {
    int32_t lo[3], hi[3];
    kind = pose_leaf_box(poses, models, n_models, i, vs, O, lo, hi);
    if (kind != kPoseLeafBoxed) return (0xFFFFFFFFull << 32) | i;
    uint32_t code = 0u;
    for (uint32_t a = 0; a < 3u; ++a) {
        const int64_t c = (static_cast<int64_t>(lo[a]) + static_cast<int64_t>(hi[a]) + 65536) >> 7;
        code |= tlas_spread10(static_cast<uint32_t>(c < 0 ? 0 : (c > 1023 ? 1023 : c))) << a;
    }
    return (static_cast<uint64_t>(code) << 32) | i;
}

// Leaf P + j from the j-th sorted key (the box is formed again: one workgroup keeps the keys in LDS, not the boxes).
BLOK_DEV TlasNode pose_tlas_leaf(const blok_pose* poses, const ModelDesc* models, uint32_t n_models, uint32_t slots, uint32_t j, uint64_t key, float vs,
                                 const PoseOrigins& O) {
    const uint32_t k = slots + j;
    if (!tlas_key_usable(key)) return tlas_empty_node(k, kTlasEmpty);
    const uint32_t i = static_cast<uint32_t>(key);
    TlasNode nd;
    (void)pose_leaf_box(poses, models, n_models, i, vs, O, nd.lo, nd.hi);
    nd.child = kTlasLeaf | i; nd.escape = tlas_escape(k);
    return nd;
}

// The header: slot count, poses with a box, and in lo[0] the linear flag (1: a usable pose has no box, every query loops over the table).
BLOK_DEV TlasNode pose_tlas_header(uint32_t slots, uint32_t boxed, bool linear) {
    TlasNode nd = tlas_header(slots, boxed);
    nd.lo[0] = linear ? 1 : 0;
    return nd;
}
BLOK_DEV bool pose_tlas_linear(const TlasNode& header) { return header.lo[0] != 0; }

#ifdef BLOK_TRACE_HOST_HARNESS
// The serial build: preimages and their union, origin box, keys, sort, leaves, refit, header.  out: tlas_nodes(n) nodes.  1 <= n <= kTlasMax.
inline void pose_tlas_build_host(const blok_pose* poses, uint32_t n, const ModelDesc* models, uint32_t n_models, float vs, const float cam[3], TlasNode* out) {
    PoseBoxD U = pose_box_empty();
    for (uint32_t i = 0; i < n; ++i) {
        PoseBoxD b;
        if (poses[i].model < n_models && pose_usable(poses[i], models[poses[i].model]) && pose_preimage_box(poses[i], models[poses[i].model], vs, b)) pose_box_join(U, b);
    }
    const PoseOrigins O = pose_origin_box(U, cam, vs);
    const uint32_t P = tlas_slots(n);
    std::vector<uint64_t> keys(P, ~0ull);
    bool linear = false;
    for (uint32_t i = 0; i < n; ++i) { PoseLeafKind kind; keys[i] = pose_tlas_key(poses, models, n_models, i, vs, O, kind); linear = linear || kind == kPoseLeafUnbounded; }
    std::sort(keys.begin(), keys.end());
    uint32_t boxed = 0;
    for (uint32_t j = 0; j < P; ++j) { out[P + j] = pose_tlas_leaf(poses, models, n_models, P, j, keys[j], vs, O); boxed += tlas_key_usable(keys[j]) ? 1u : 0u; }
    for (uint32_t k = P - 1u; k >= 1u; --k) out[k] = tlas_internal(k, out[2u * k], out[2u * k + 1u]);
    out[0] = pose_tlas_header(P, boxed, linear);
}
#else
// Builds the tree of n <= kTlasMax poses into nodes (tlas_nodes(n) of them) on the stream: one workgroup, no host synchronise.
void launch_pose_tlas_build(const blok_pose* poses, uint32_t n, const ModelDesc* models, uint32_t n_models, float vs, const float cam[3], TlasNode* nodes,
                            hipStream_t stream);
#endif

}  // namespace blok
#endif
