// TEST INFRASTRUCTURE: the object motion of moving instances (blok_amd/csrc/hip/instance_motion.h) and the temporal pass of post_core.h,
// plain and instanced, compiled for the CPU.  Never linked into the shipped libraries.
#define BLOK_TRACE_HOST_HARNESS 1
#include "instance_motion.h"
#include "post_core.h"

#include <cstring>
#include <vector>

using namespace blok;

namespace {
// Model descriptors with only what instance_usable reads: the local box, and a non-null tree for a live model.
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

// map_point / map_normal of n points (float3) and normals on instance `cur` that was `prev`.
void ms_map(const blok_instance* cur, const blok_instance* prev, float vs, const float* p, const float* nrm, size_t n, float* out_p, float* out_n) {
    for (size_t i = 0; i < n; ++i) {
        const V3 q = map_point(*cur, *prev, vs, v3(p[3 * i], p[3 * i + 1], p[3 * i + 2]));
        const V3 m = map_normal(*cur, *prev, v3(nrm[3 * i], nrm[3 * i + 1], nrm[3 * i + 2]));
        out_p[3 * i] = q.x; out_p[3 * i + 1] = q.y; out_p[3 * i + 2] = q.z;
        out_n[3 * i] = m.x; out_n[3 * i + 1] = m.y; out_n[3 * i + 2] = m.z;
    }
}

// instance_tracked for every index of `cur`; lohi: per model lo[3], hi[3]; alive: per model 0 = destroyed.
void ms_tracked(const blok_instance* cur, uint32_t n_cur, const blok_instance* prev, uint32_t n_prev, const int32_t* lohi, const uint8_t* alive,
                uint32_t n_models, uint8_t* out) {
    const std::vector<ModelDesc> d = descs(lohi, alive, n_models);
    MotionTables M{};
    M.cur = cur; M.n_cur = n_cur; M.prev = prev; M.n_prev = n_prev; M.models = d.data(); M.n_models = n_models; M.vs = 1.0f;
    for (uint32_t i = 0; i < n_cur; ++i) out[i] = instance_tracked(M, i) ? 1 : 0;
}

// One temporal pass over a w x h frame.  planes: color, world_pos, normal_roughness (float4), motion_in (float2 or null), prev_color,
// prev_moments, prev_world_pos, prev_hist_len (half), prev_unit_normals; outputs out_color, out_moments, hist_world_pos, unit_normals,
// out_hist_len (half), motion (half2).  ids == null: temporal_pixel; else temporal_pixel_instanced with the tables.
void ms_temporal(uint32_t w, uint32_t h, uint32_t frame_count, const float* prev_view_proj, const DenoiseSettings* s, void* const* planes,
                 const uint32_t* ids, const blok_instance* cur, uint32_t n_cur, const blok_instance* prev, uint32_t n_prev, const int32_t* lohi,
                 const uint8_t* alive, uint32_t n_models, float vs) {
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
    TemporalInstancedArgs a{};
    a.t = t;
    a.m.ids = ids; a.m.cur = cur; a.m.n_cur = n_cur; a.m.prev = prev; a.m.n_prev = n_prev; a.m.models = d.data(); a.m.n_models = n_models; a.m.vs = vs;
    for (uint32_t y = 0; y < h; ++y) for (uint32_t x = 0; x < w; ++x) temporal_pixel_instanced(a, int(x), int(y));
}

}  // extern "C"
