// TEST INFRASTRUCTURE: the object motion of posed models (blok_amd/csrc/common/pose_motion_core.h, blok_amd/csrc/hip/pose_motion.h) and the
// temporal pass of post_core.h in its posed mode, compiled for the CPU.  Never linked into the shipped libraries.
// -DPOSE_MOTION_SHIM_MAIN: a stand-alone program that replays a case file of tests/test_pose_motion_cpu.py, for the sanitizers.
#define BLOK_TRACE_HOST_HARNESS 1
#include "pose_motion.h"
#include "post_core.h"

#include <cstdio>
#include <cstring>
#include <vector>

using namespace blok;

namespace {
// Model descriptors with only what the tracking rules read: the local box, and a non-null tree for a live model.
std::vector<ModelDesc> descs(const int32_t* lohi, const uint8_t* alive, uint32_t n_models) {
    static const uint4 dummy{};
    std::vector<ModelDesc> d(n_models);
    for (uint32_t m = 0; m < n_models; ++m) {
        d[m] = ModelDesc{};
        d[m].nodes = alive[m] ? &dummy : nullptr;
        for (int a = 0; a < 3; ++a) { d[m].lo[a] = lohi[6 * m + a]; d[m].hi[a] = lohi[6 * m + 3 + a]; }
    }
    return d;
}
}  // namespace

extern "C" {

// pose::motion_record of one pair (prev == null: beyond the previous table).
void pm_record(const blok_pose* cur, const blok_pose* prev, int model_usable, blok_pose_motion* out) {
    pose::motion_record(*cur, prev ? *prev : *cur, prev != nullptr, model_usable != 0, *out);
}

// The prepare kernel's body for every pose of `cur`; lohi: per model lo[3], hi[3]; alive: per model 0 = destroyed.
void pm_prepare(const blok_pose* cur, uint32_t n_cur, const blok_pose* prev, uint32_t n_prev, const int32_t* lohi, const uint8_t* alive, uint32_t n_models,
                blok_pose_motion* out) {
    const std::vector<ModelDesc> d = descs(lohi, alive, n_models);
    for (uint32_t i = 0; i < n_cur; ++i) pose_motion_prepare(cur, n_cur, prev, n_prev, d.data(), n_models, i, out);
}

// pose_map_point / pose_map_normal of n points (float3) and normals under record R (state 2), or what placed_map does with R in any state
// (through != 0: the id dispatch, which leaves the point alone in state 1).
void pm_map(const blok_pose_motion* R, int through, const float* p, const float* nrm, size_t n, float* out_p, float* out_n) {
    PoseMotionTables M{};
    M.records = R; M.n_cur = 1u;
    for (size_t i = 0; i < n; ++i) {
        const V3 w = v3(p[3 * i], p[3 * i + 1], p[3 * i + 2]), k = v3(nrm[3 * i], nrm[3 * i + 1], nrm[3 * i + 2]);
        V3 q = w, m = k;
        if (through) placed_map<true>(M, BLOK_POSE_ID | 0u, w, k, q, m);
        else { q = pose_map_point(*R, w); m = pose_map_normal(*R, k); }
        out_p[3 * i] = q.x; out_p[3 * i + 1] = q.y; out_p[3 * i + 2] = q.z;
        out_n[3 * i] = m.x; out_n[3 * i + 1] = m.y; out_n[3 * i + 2] = m.z;
    }
}

// instance_motion.h's map_point / map_normal, the lattice map the pose map is held against.
void pm_lattice_map(const blok_instance* cur, const blok_instance* prev, float vs, const float* p, const float* nrm, size_t n, float* out_p, float* out_n) {
    for (size_t i = 0; i < n; ++i) {
        const V3 q = map_point(*cur, *prev, vs, v3(p[3 * i], p[3 * i + 1], p[3 * i + 2]));
        const V3 m = map_normal(*cur, *prev, v3(nrm[3 * i], nrm[3 * i + 1], nrm[3 * i + 2]));
        out_p[3 * i] = q.x; out_p[3 * i + 1] = q.y; out_p[3 * i + 2] = q.z;
        out_n[3 * i] = m.x; out_n[3 * i + 1] = m.y; out_n[3 * i + 2] = m.z;
    }
}

// placed_state of n ids against the tables (0 own, 1 mapped, 2 none).
void pm_states(const uint32_t* ids, size_t n, const blok_instance* cur, uint32_t n_cur, const blok_instance* prev, uint32_t n_prev, const int32_t* lohi,
               const uint8_t* alive, uint32_t n_models, const blok_pose_motion* records, uint32_t n_poses, uint8_t* out) {
    const std::vector<ModelDesc> d = descs(lohi, alive, n_models);
    PoseMotionTables Q{};
    Q.inst.cur = cur; Q.inst.n_cur = n_cur; Q.inst.prev = prev; Q.inst.n_prev = n_prev; Q.inst.models = d.data(); Q.inst.n_models = n_models; Q.inst.vs = 1.0f;
    Q.records = records; Q.n_cur = n_poses;
    for (size_t i = 0; i < n; ++i) out[i] = static_cast<uint8_t>(placed_state(Q, ids[i]));
}

// One temporal pass over a w x h frame; planes as tests/host_harness/motion_shim.cpp's ms_temporal.  ids == null: temporal_pixel; else
// temporal_pixel_posed with the instance tables and the poses' records.
void pm_temporal(uint32_t w, uint32_t h, uint32_t frame_count, const float* prev_view_proj, const DenoiseSettings* s, void* const* planes,
                 const uint32_t* ids, const blok_instance* cur, uint32_t n_cur, const blok_instance* prev, uint32_t n_prev, const int32_t* lohi,
                 const uint8_t* alive, uint32_t n_models, float vs, const blok_pose_motion* records, uint32_t n_poses) {
    TemporalArgs t{};
    t.f.w = w; t.f.h = h; t.f.frame_count = frame_count; t.f.s = *s;
    std::memcpy(t.f.prev_view_proj, prev_view_proj, 16 * sizeof(float));
    t.color = static_cast<const float*>(planes[0]); t.world_pos = static_cast<const float*>(planes[1]);
    t.normal_roughness = static_cast<const float*>(planes[2]); t.motion_in = static_cast<const float*>(planes[3]);
    t.prev_color = static_cast<const float*>(planes[4]); t.prev_moments = static_cast<const float*>(planes[5]);
    t.prev_world_pos = static_cast<const float*>(planes[6]); t.prev_hist_len = static_cast<const uint16_t*>(planes[7]);
    t.prev_unit_normals = static_cast<const float*>(planes[8]);
    t.out_color = static_cast<float*>(planes[9]); t.out_moments = static_cast<float*>(planes[10]); t.hist_world_pos = static_cast<float*>(planes[11]);
    t.unit_normals = static_cast<float*>(planes[12]); t.out_hist_len = static_cast<uint16_t*>(planes[13]); t.motion = static_cast<uint16_t*>(planes[14]);
    if (!ids) {
        for (uint32_t y = 0; y < h; ++y) for (uint32_t x = 0; x < w; ++x) temporal_pixel(t, int(x), int(y));
        return;
    }
    const std::vector<ModelDesc> d = descs(lohi, alive, n_models);
    TemporalPosedArgs a{};
    a.t = t;
    a.m.inst.ids = ids; a.m.inst.cur = cur; a.m.inst.n_cur = n_cur; a.m.inst.prev = prev; a.m.inst.n_prev = n_prev;
    a.m.inst.models = d.data(); a.m.inst.n_models = n_models; a.m.inst.vs = vs;
    a.m.records = records; a.m.n_cur = n_poses;
    for (uint32_t y = 0; y < h; ++y) for (uint32_t x = 0; x < w; ++x) temporal_pixel_posed(a, int(x), int(y));
}

// blok_hip_posed_motion_device's pixel body over a w x h rectangle at (x0, y0) of a frame_w x frame_h frame; motion: float2.
void pm_motion(uint32_t x0, uint32_t y0, uint32_t w, uint32_t h, uint32_t frame_w, uint32_t frame_h, const float* prev_view_proj, const float* world_pos,
               const uint32_t* ids, const blok_pose_motion* records, uint32_t n_poses, uint16_t* motion_h, float* motion) {
    PosedMotionArgs a{};
    a.m.inst.ids = ids; a.m.records = records; a.m.n_cur = n_poses;
    a.world_pos = world_pos;
    a.x0 = x0; a.y0 = y0; a.w = w; a.h = h; a.frame_w = frame_w; a.frame_h = frame_h;
    std::memcpy(a.prev_view_proj, prev_view_proj, 16 * sizeof(float));
    a.motion_h = motion_h; a.motion = motion;
    for (uint32_t y = 0; y < h; ++y) for (uint32_t x = 0; x < w; ++x) posed_motion_pixel(a, int(x), int(y));
}

}  // extern "C"

#ifdef POSE_MOTION_SHIM_MAIN
// Case file: uint32 n_cur, n_prev, n_points; n_cur poses; n_prev poses; n_points float3 points; n_points float3 normals.  Every pose of cur
// against prev through the prepare body (one live model 0 .. 3 each, a box inside the lattice), every record's map of every point, then a
// small posed temporal pass and motion pass whose ids walk through the poses, one past the table and an instance id with no tables.
int main(int argc, char** argv) {
    if (argc < 2) { std::fprintf(stderr, "usage: %s case-file\n", argv[0]); return 2; }
    std::FILE* f = std::fopen(argv[1], "rb");
    if (!f) { std::perror(argv[1]); return 2; }
    uint32_t head[3];
    if (std::fread(head, sizeof(uint32_t), 3, f) != 3) return 2;
    const uint32_t n_cur = head[0], n_prev = head[1], n_pts = head[2];
    std::vector<blok_pose> cur(n_cur), prev(n_prev);
    std::vector<float> p(3 * size_t(n_pts)), nrm(3 * size_t(n_pts));
    if (std::fread(cur.data(), sizeof(blok_pose), n_cur, f) != n_cur || std::fread(prev.data(), sizeof(blok_pose), n_prev, f) != n_prev ||
        std::fread(p.data(), sizeof(float), p.size(), f) != p.size() || std::fread(nrm.data(), sizeof(float), nrm.size(), f) != nrm.size())
        return 2;
    std::fclose(f);
    const int32_t lohi[24] = {0, 0, 0, 16, 2, 16, 0, 0, 0, 3, 3, 3, 0, 0, 0, 16, 2, 16, 0, 0, 0, 40000, 1, 1};
    const uint8_t alive[4] = {1, 1, 0, 1};
    std::vector<blok_pose_motion> rec(n_cur);
    pm_prepare(cur.data(), n_cur, prev.data(), n_prev, lohi, alive, 4u, rec.data());
    uint32_t states[3] = {0, 0, 0};
    std::vector<float> op(p.size()), on(p.size());
    double sum = 0.0;
    for (uint32_t i = 0; i < n_cur; ++i) {
        if (rec[i].state > 2u) return 1;
        ++states[rec[i].state];
        pm_map(&rec[i], 1, p.data(), nrm.data(), n_pts, op.data(), on.data());
        if (rec[i].state == 2u) for (float v : op) if (pose::finite(v)) sum += v;
    }
    // a frame of 24 x 10 pixels: every plane the same ramp, ids cycling over the poses, one index past the table, an instance id and the world
    const uint32_t w = 24, h = 10, n = w * h;
    std::vector<float> col(4 * n), wp(4 * n), nr(4 * n), z4(4 * n, 0.0f), z2(2 * n, 0.0f), o4a(4 * n), o4b(4 * n), o4c(4 * n), o2(2 * n), mo(2 * n);
    std::vector<uint16_t> hl(n, 0), ohl(n), omo(2 * n), moh(2 * n);
    std::vector<uint32_t> ids(n);
    for (uint32_t i = 0; i < n; ++i) {
        const uint32_t k = i % (n_cur + 3u);
        ids[i] = k < n_cur + 1u ? (BLOK_POSE_ID | k) : (k == n_cur + 1u ? 7u : kInstanceNone);
        for (int c = 0; c < 4; ++c) { col[4 * i + c] = 0.5f; wp[4 * i + c] = n_pts ? p[(3 * (i % n_pts) + c) % p.size()] : 1.0f; nr[4 * i + c] = c == 1 ? 1.0f : 0.0f; }
        wp[4 * i + 3] = 10.0f;
    }
    float vp[16] = {0.1f, 0, 0, 0, 0, 0, 0, 0, 0, 0.1f, 0, 0, -1, -1, 0, 1};
    DenoiseSettings s{0.05f, 0.2f, 1.5f, 0.1f, 0.95f, 0.5f, 128.0f, 0.1f, 4, 1.5f, 4};
    void* planes[15] = {col.data(), wp.data(), nr.data(), nullptr, z4.data(), z2.data(), wp.data(), hl.data(), nr.data(),
                        o4a.data(), o2.data(), o4b.data(), o4c.data(), ohl.data(), omo.data()};
    pm_temporal(w, h, 1u, vp, &s, planes, ids.data(), nullptr, 0u, nullptr, 0u, lohi, alive, 4u, 1.0f, rec.data(), n_cur);
    pm_motion(2u, 1u, w, h, w + 4u, h + 2u, vp, wp.data(), ids.data(), rec.data(), n_cur, moh.data(), mo.data());
    std::printf("untracked %u identity %u moving %u checksum %.17g\n", states[0], states[1], states[2], sum);
    return 0;
}
#endif
