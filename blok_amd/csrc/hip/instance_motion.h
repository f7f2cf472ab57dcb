// Object motion of moving instances (include/blok_hip.h: blok_hip_instance_motion_device, blok_hip_denoise_instanced*,
// blok_hip_draw_frame_rt_instanced_motion): the map from a first-hit surface point of this frame to the same point one
// frame earlier.
//
// Tracking.  Instance i of this frame's table `cur` is tracked when i < n_prev, prev[i].model == cur[i].model and both records pass
// instance_usable with that model's descriptor; otherwise it is untracked (it appeared this frame or changed model).  The map below does
// not contain the model's scale, and is wrong across a change of it: blok_hip_model_set_scale empties the context's previous table, and
// callers of the *_device entries keep that rule themselves.
//
// The map.  §11's transform takes world point o to the model's local lattice as o'_k = s_k * (o[axis[k]] - offset[axis[k]] * vs).  For a
// tracked instance, prev o cur^-1 moves a world point p on it (and its normal n) to the previous frame: for each local axis k, with
// a = cur.axis[k], b = prev.axis[k], s / s' the signs of cur's / prev's flip bit k and c = s * s',
//   p_prev[b] = fl(c * p[a] + float(prev.offset[b] - c * cur.offset[a]) * vs)      (integer difference exact, * vs exact: a power of two)
//   n_prev[b] = c * n[a]                                                          (exact)
// one rounding per axis.  Equal offset, axis and flip: the identity with no arithmetic (p_prev = p, n_prev = n bit for bit), so a
// stationary instance gets exactly the camera-only motion.  Object motion = cu - project_prev(prev_view_proj, p_prev) with
// cu = (px + 0.5) / frame_w (post_core.h), the operations of the path kernel's motion plane (path_core.h: store_narrow).
//
// tests/test_instance_motion_cpu.py compiles this header with post_core.h for the host (tests/host_harness/motion_shim.cpp).
#ifndef BLOK_INSTANCE_MOTION_H
#define BLOK_INSTANCE_MOTION_H

#include "path_core.h"

namespace blok {

// Both frames' instance tables and the first-hit instance per pixel, as the motion kernel and the instanced temporal pass read them.
struct MotionTables {
    const uint32_t* ids;                 // per pixel: this frame's first-hit instance or kInstanceNone
    const blok_instance *cur, *prev;     // device memory, n_cur / n_prev records
    uint32_t n_cur, n_prev;
    const ModelDesc* models;             // the context's model store
    uint32_t n_models;
    float vs;                            // the world's voxel size
};

BLOK_HD bool instance_tracked(const MotionTables& M, uint32_t i) {
    if (i >= M.n_cur || i >= M.n_prev) return false;
    const blok_instance& c = M.cur[i];
    const blok_instance& p = M.prev[i];
    if (p.model != c.model || c.model >= M.n_models) return false;
    const ModelDesc& d = M.models[c.model];
    return instance_usable(c, d) && instance_usable(p, d);
}

BLOK_HD bool same_placement(const blok_instance& a, const blok_instance& b) {
    return a.offset[0] == b.offset[0] && a.offset[1] == b.offset[1] && a.offset[2] == b.offset[2] && a.axis[0] == b.axis[0] &&
           a.axis[1] == b.axis[1] && a.axis[2] == b.axis[2] && a.flip == b.flip;
}

// World axis b of the previous frame: the local axis k with prev.axis[k] == b, cur's world axis a = cur.axis[k] and c = s * s' (true: -1).
BLOK_DEV void motion_axis(const blok_instance& C, const blok_instance& P, uint32_t b, uint32_t& a, bool& negate) {
    const uint32_t k = local_axis(P, b);
    a = pick3(k, int32_t(C.axis[0]), int32_t(C.axis[1]), int32_t(C.axis[2]));
    negate = (((C.flip ^ P.flip) >> k) & 1u) != 0u;
}
BLOK_DEV float map_coord(const blok_instance& C, const blok_instance& P, float vs, V3 p, uint32_t b) {
    uint32_t a; bool negate;
    motion_axis(C, P, b, a, negate);
    const float pa = pick3(a, p.x, p.y, p.z);
    const int64_t oa = pick3(a, C.offset[0], C.offset[1], C.offset[2]), ob = pick3(b, P.offset[0], P.offset[1], P.offset[2]);
    const int64_t d = negate ? ob + oa : ob - oa;
    return rn_add(negate ? -pa : pa, rn_mul(static_cast<float>(d), vs));
}
BLOK_DEV float map_normal_coord(const blok_instance& C, const blok_instance& P, V3 n, uint32_t b) {
    uint32_t a; bool negate;
    motion_axis(C, P, b, a, negate);
    const float na = pick3(a, n.x, n.y, n.z);
    return negate ? -na : na;
}
// p_prev and n_prev of a point on instance C (this frame) that was P (previous frame).
BLOK_DEV V3 map_point(const blok_instance& C, const blok_instance& P, float vs, V3 p) {
    if (same_placement(C, P)) return p;
    return v3(map_coord(C, P, vs, p, 0u), map_coord(C, P, vs, p, 1u), map_coord(C, P, vs, p, 2u));
}
BLOK_DEV V3 map_normal(const blok_instance& C, const blok_instance& P, V3 n) {
    if (same_placement(C, P)) return n;
    return v3(map_normal_coord(C, P, n, 0u), map_normal_coord(C, P, n, 1u), map_normal_coord(C, P, n, 2u));
}

}  // namespace blok
#endif
