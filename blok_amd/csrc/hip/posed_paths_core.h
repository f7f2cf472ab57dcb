// Posed models in the path loop (include/blok_hip.h: "Path-traced frames with poses"): what shade_pixel<…, kPosed> adds to
// the instanced composition of tlas_core.h.  Host-compilable like posed_core.h (tests/host_harness/posed_paths_shim.cpp).
//
// Order.  Every ray of the path loop is composed world first, then the lattice instances (tlas_core.h, unchanged), then poses 0 .. p-1.
//   Closest hit (primary and bounce rays): the poses are asked with tmax = the best t so far, each walk accepts t < tmax only, so a pose
//   never takes a tie from the world or an instance and the lowest pose keeps a tie among poses.  Any hit (shadow rays): the poses are
//   asked only when neither the world nor an instance reported a voxel, on the uncapped interval [0.001, 1000).
// A pose's ray goes over by pose_ray, its walk is the model's canonical walk (posed_core.h): the candidate below is placed_candidate<PoseKind>
//   with a per-lane descriptor, in the shape of instance_candidate (the lanes of a path wave ask different poses' models).
// Every pose is tested for every ray: that is the frame's DEFINITION.  The pose BVH (pose_tlas_core.h) is an optimisation of it: the queries below
//   walk it by tlas_closest / tlas_any's rule — a pose below the current winning pose walks with tmax = nextafter(best_t) and wins on
//   t <= best_t, any other with tmax = best_t and wins on t < best_t — started with the composed t and NO pose as the winner, so that a pose
//   never takes a tie from the world or an instance.  Without a tree (more than kTlasMax poses, blok_hip_set_pose_tlas(0)) or with the
//   header's linear flag set, they loop over the table in index order.
//
// The normal of a posed hit.  A posed face has a real world normal, not one of six; the path loop uses it for the shadow ray's origin, n.l,
//   the sampling frame and the G-buffer.  For local face 2k + n of pose P, s = +1 (n = 0) or -1 (n = 1):
//     v_j = s * m_kj        q = fl(fl(fl(v_0 v_0) + fl(v_1 v_1)) + fl(v_2 v_2))
//     !(q > 0) (a zero row of a singular map, underflow): the axis normal of pose_shade_face(P, face)
//     otherwise len = rn_sqrt(q), n_j = fl(v_j / len) + 0.0f                     (+ 0.0f: every zero is +0, as in the axis normal's literals)
//   For a pose made by blok_pose_from_instance row k is a signed unit vector (times a power of two under a model scale): q is an exact
//   power of four, len exact, v_j / len is +-1 or +-0: the axis normal of the lattice instance bit for bit.
#ifndef BLOK_POSED_PATHS_CORE_H
#define BLOK_POSED_PATHS_CORE_H

#include "pose_tlas_core.h"

#if defined(__clang__)
#pragma clang fp contract(off)
#endif

namespace blok {

// The pose part of a posed path launch: the table and its count (the model store is the TlasScene's).
struct PoseScene {
    const blok_pose* poses;
    uint32_t n_poses;
    const TlasNode* nodes;           // the pose BVH (pose_tlas_core.h); null: the linear loop
};

// The axis normal of world face f (0 .. 5), zeros +0: the expression of shade_pixel.
BLOK_DEV void axis_normal(uint32_t face, float& nx, float& ny, float& nz) {
    nx = face == 0u ? 1.0f : (face == 1u ? -1.0f : 0.0f);
    ny = face == 2u ? 1.0f : (face == 3u ? -1.0f : 0.0f);
    nz = face == 4u ? 1.0f : (face == 5u ? -1.0f : 0.0f);
}

// The world normal of local face 2k + n of pose P by the rule above (before the flip against the ray).
BLOK_DEV void pose_world_normal(const blok_pose& P, uint32_t face, float& nx, float& ny, float& nz) {
    const uint32_t k = face >> 1;
    const float s = (face & 1u) ? -1.0f : 1.0f;
    const float v0 = s * pick3(k, P.m[0][0], P.m[1][0], P.m[2][0]);
    const float v1 = s * pick3(k, P.m[0][1], P.m[1][1], P.m[2][1]);
    const float v2 = s * pick3(k, P.m[0][2], P.m[1][2], P.m[2][2]);
    const float q = rn_add(rn_add(rn_mul(v0, v0), rn_mul(v1, v1)), rn_mul(v2, v2));
    if (!(q > 0.0f)) { axis_normal(pose_shade_face(P, face), nx, ny, nz); return; }
    const float len = rn_sqrt(q);
    nx = v0 / len + 0.0f; ny = v1 / len + 0.0f; nz = v2 / len + 0.0f;
}

// One pose's candidate with a per-lane descriptor: the pose's walk of world ray r with tmax = best_t; true (and rec, the local record of
// pose_record) iff it reports a voxel, whose t is then < best_t.  walk() of trace_core.h piece by piece, as instance_candidate is.
BLOK_DEV bool pose_path_candidate(const blok_pose& P, const ModelDesc& M, float vs, float inv_vs, const RayIn& r, float best_t, uint4* stk, uint4& rec) {
    RayIn l;
    if (!pose_ray(P, r, l)) return false;
    l.tmax = best_t;
    if (!instance_box_entered(M, vs, l)) return false;
    BLOK_STAT(4, 0);                       // a walk begins
    TraceArgs a = model_args(M, vs, inv_vs);
    const WalkRay R = walk_ray(a, l.ox, l.oy, l.oz, safe_inv(l.dx), safe_inv(l.dy), safe_inv(l.dz));
    WalkState s;
    walk_enter(a, R, l.tmin, l.tmax, s);
    walk_loop(a, R, l.tmax, s, stk);
    if (!s.found) return false;
    const uint32_t e = as_written(M.scale_log2);                 // (vm is formed again behind the loop: instance_candidate)
    a.voxel_size = __builtin_bit_cast(float, __builtin_bit_cast(uint32_t, vs) + (e << 23));
    rec = pose_record(walk_hit(a, l, R, s));
    return true;
}

// One pose's candidate under the ordering rule of a tree walk (tlas_leaf_candidate's, among poses); best_t / best / rec updated when it wins.
BLOK_DEV void pose_leaf_candidate(const PoseScene& S, const ModelDesc* models, uint32_t n_models, float vs, float inv_vs, const RayIn& r, uint32_t i,
                                  uint4* stk, float& best_t, uint32_t& best, uint4& rec) {
    const blok_pose P = S.poses[i];
    if (P.model >= n_models) return;
    const ModelDesc M = models[P.model];
    if (!pose_usable(P, M)) return;
    const bool below = best != kInstanceNone && i < best;              // (the world and the instances, best == none, win every tie)
    const float tmax = below ? nextafterf(best_t, 3.0e38f) : best_t;
    uint4 c;
    if (!pose_path_candidate(P, M, vs, inv_vs, r, tmax, stk, c)) return;
    const float t = __uint_as_float(c.x);
    if (t < best_t || (below && t == best_t)) { rec = c; best_t = t; best = i; }
}

BLOK_DEV bool pose_tree_usable(const PoseScene& S) { return S.nodes != nullptr && !pose_tlas_linear(S.nodes[0]); }

// Closest hit of world ray r over the poses, given the composed answer of the world and the instances: best_t = its t (or r's tmax on a
// miss).  Returns the winning pose's index (rec = its record, local voxel and local face) or kInstanceNone.
BLOK_DEV uint32_t poses_closest(const PoseScene& S, const ModelDesc* models, uint32_t n_models, float vs, float inv_vs, const RayIn& r, float best_t,
                                uint4* stk, uint4& rec) {
    uint32_t best = kInstanceNone;
    if (!pose_tree_usable(S)) {                                          // the linear loop, index order
        for (uint32_t i = 0; i < S.n_poses; ++i) pose_leaf_candidate(S, models, n_models, vs, inv_vs, r, i, stk, best_t, best, rec);
        return best;
    }
    const float ix = safe_inv(r.dx), iy = safe_inv(r.dy), iz = safe_inv(r.dz);
    uint32_t k = 1u;
    while (k != 0u) {
        const TlasNode nd = S.nodes[k];
        // a tie of a lower pose may still replace the current winning pose: test the box up to just past best_t
        const float tmax = best != kInstanceNone ? nextafterf(best_t, 3.0e38f) : best_t;
        if (nd.child != kTlasEmpty && tlas_box_hit(nd, vs, r, ix, iy, iz, tmax)) {
            if (nd.child & kTlasLeaf) {
                pose_leaf_candidate(S, models, n_models, vs, inv_vs, r, nd.child & ~kTlasLeaf, stk, best_t, best, rec);
                k = nd.escape;
            } else k = nd.child;
        } else k = nd.escape;
    }
    return best;
}

// Any hit of r in [r.tmin, r.tmax) over the poses (shadow rays).
BLOK_DEV bool poses_any(const PoseScene& S, const ModelDesc* models, uint32_t n_models, float vs, float inv_vs, const RayIn& r, uint4* stk) {
    uint4 rec;
    const auto usable_hit = [&](uint32_t i) {
        const blok_pose P = S.poses[i];
        if (P.model >= n_models) return false;
        const ModelDesc M = models[P.model];
        return pose_usable(P, M) && pose_path_candidate(P, M, vs, inv_vs, r, r.tmax, stk, rec);
    };
    if (!pose_tree_usable(S)) {
        for (uint32_t i = 0; i < S.n_poses; ++i) if (usable_hit(i)) return true;
        return false;
    }
    const float ix = safe_inv(r.dx), iy = safe_inv(r.dy), iz = safe_inv(r.dz);
    uint32_t k = 1u;
    while (k != 0u) {
        const TlasNode nd = S.nodes[k];
        if (nd.child != kTlasEmpty && tlas_box_hit(nd, vs, r, ix, iy, iz, r.tmax)) {
            if (nd.child & kTlasLeaf) {
                if (usable_hit(nd.child & ~kTlasLeaf)) return true;
                k = nd.escape;
            } else k = nd.child;
        } else k = nd.escape;
    }
    return false;
}

}  // namespace blok
#endif
