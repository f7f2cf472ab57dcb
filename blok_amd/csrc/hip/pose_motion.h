// Object motion of posed models (include/blok_hip.h, "Object motion for posed models": blok_hip_posed_motion_device,
// blok_hip_denoise_posed*, blok_hip_draw_frame_rt_posed_motion): the per-pixel map from a first-hit surface point of this
// frame on a pose to the same point one frame earlier, and the dispatch of a pixel's id between the poses and the lattice instances of
// instance_motion.h, so that a frame holding both kinds runs one pass.
//
// The tracking rule and the record (one per pose, built once per launch by pose_motion_prepare_kernel) are ../common/pose_motion_core.h's.
// The map, every operation a separately rounded float one in the manner of pose_ray (posed_core.h), R the pose's record in state 2:
//   r_j      = fl(p_j - pivot_cur_j)
//   q_i      = fl( fl( fl( fl(a_i0 r_0) + fl(a_i1 r_1) ) + fl(a_i2 r_2) ) + c_i )
//   p_prev_i = fl(pivot_prev_i + q_i)
//   v_i      = fl( fl( fl(n_i0 n_0) + fl(n_i1 n_1) ) + fl(n_i2 n_2) )
//   qq       = fl( fl( fl(v_0 v_0) + fl(v_1 v_1) ) + fl(v_2 v_2) )
//   n_prev   = !(qq > 0) ? n : fl(v_i / rn_sqrt(qq))
// State 1 is the identity with no arithmetic; state 0 (and an index beyond the table) is untracked.
//
// tests/test_pose_motion_cpu.py compiles this header with post_core.h for the host (tests/host_harness/pose_motion_shim.cpp).
#ifndef BLOK_POSE_MOTION_H
#define BLOK_POSE_MOTION_H

#include "instance_motion.h"
#include "posed_core.h"
#include "../common/pose_motion_core.h"

namespace blok {

static_assert(pose::kDetFloor == kPoseDetFloor, "one determinant floor for the screen bins, the pose BVH and the motion records");

// The id plane, the instance tables and the poses' records, as the posed motion kernel and the posed temporal pass read them.
struct PoseMotionTables {
    MotionTables inst;                    // ids: the posed path entries' plane (BLOK_POSE_ID | index, an instance index or kInstanceNone)
    const blok_pose_motion* records;      // device memory, n_cur records: pose i of this frame against pose i of the previous one
    uint32_t n_cur;
};

BLOK_DEV V3 pose_map_point(const blok_pose_motion& R, V3 p) {
    const float r0 = rn_sub(p.x, R.pivot_cur[0]), r1 = rn_sub(p.y, R.pivot_cur[1]), r2 = rn_sub(p.z, R.pivot_cur[2]);
    const float q0 = rn_add(rn_add(rn_add(rn_mul(R.a[0][0], r0), rn_mul(R.a[0][1], r1)), rn_mul(R.a[0][2], r2)), R.c[0]);
    const float q1 = rn_add(rn_add(rn_add(rn_mul(R.a[1][0], r0), rn_mul(R.a[1][1], r1)), rn_mul(R.a[1][2], r2)), R.c[1]);
    const float q2 = rn_add(rn_add(rn_add(rn_mul(R.a[2][0], r0), rn_mul(R.a[2][1], r1)), rn_mul(R.a[2][2], r2)), R.c[2]);
    return v3(rn_add(R.pivot_prev[0], q0), rn_add(R.pivot_prev[1], q1), rn_add(R.pivot_prev[2], q2));
}
BLOK_DEV V3 pose_map_normal(const blok_pose_motion& R, V3 n) {
    const float v0 = rn_add(rn_add(rn_mul(R.n[0][0], n.x), rn_mul(R.n[0][1], n.y)), rn_mul(R.n[0][2], n.z));
    const float v1 = rn_add(rn_add(rn_mul(R.n[1][0], n.x), rn_mul(R.n[1][1], n.y)), rn_mul(R.n[1][2], n.z));
    const float v2 = rn_add(rn_add(rn_mul(R.n[2][0], n.x), rn_mul(R.n[2][1], n.y)), rn_mul(R.n[2][2], n.z));
    const float qq = rn_add(rn_add(rn_mul(v0, v0), rn_mul(v1, v1)), rn_mul(v2, v2));
    if (!(qq > 0.0f)) return n;
    const float len = rn_sqrt(qq);
    return v3(rn_div(v0, len), rn_div(v1, len), rn_div(v2, len));
}

// Whose pixel a first-hit id is: the world's or the sky's (its history is its own), a tracked pose's or instance's (its history lies where
// placed_map says), or an untracked one's (no history).  Reads the id's table entry only: the 4-byte state of a pose's record.
enum PlacedHistory : int { kHistoryOwn = 0, kHistoryMapped = 1, kHistoryNone = 2 };
BLOK_DEV PlacedHistory placed_state(const PoseMotionTables& M, uint32_t id) {
    if (id == kInstanceNone) return kHistoryOwn;
    if (id & BLOK_POSE_ID) {
        const uint32_t i = id & ~BLOK_POSE_ID;
        return i < M.n_cur && M.records[i].state != 0u ? kHistoryMapped : kHistoryNone;
    }
    return instance_tracked(M.inst, id) ? kHistoryMapped : kHistoryNone;
}
// Where the surface point (world, normal) of a kHistoryMapped pixel was one frame earlier; was / was_normal come in as world / normal and
// stay so under the identity.  An instance goes through instance_motion.h's functions, unchanged.
template <bool kWithNormal>
BLOK_DEV void placed_map(const PoseMotionTables& M, uint32_t id, V3 world, [[maybe_unused]] V3 normal, V3& was, [[maybe_unused]] V3& was_normal) {
    if (id & BLOK_POSE_ID) {
        const blok_pose_motion& R = M.records[id & ~BLOK_POSE_ID];
        if (R.state != 2u) return;
        was = pose_map_point(R, world);
        if constexpr (kWithNormal) was_normal = pose_map_normal(R, normal);
        return;
    }
    const blok_instance C = M.inst.cur[id], P = M.inst.prev[id];
    was = map_point(C, P, M.inst.vs, world);
    if constexpr (kWithNormal) was_normal = map_normal(C, P, normal);
}

// pose_motion_prepare_kernel's work for pose i: the record of cur[i] against prev[i] with the context's model store.
BLOK_HD void pose_motion_prepare(const blok_pose* cur, uint32_t n_cur, const blok_pose* prev, uint32_t n_prev, const ModelDesc* models,
                                 uint32_t n_models, uint32_t i, blok_pose_motion* out) {
    if (i >= n_cur) return;
    const blok_pose C = cur[i];
    const bool has_prev = i < n_prev;
    const blok_pose P = has_prev ? prev[i] : C;
    const bool model_usable = C.model < n_models && models[C.model].nodes && pose_model_box_usable(models[C.model]);
    blok_pose_motion R;
    pose::motion_record(C, P, has_prev, model_usable, R);
    out[i] = R;
}

}  // namespace blok
#endif
