// TEST INFRASTRUCTURE: the lit path loop (blok_amd/csrc/hip/path_core.h: shade_pixel<…, kLit>, light_sample; csrc/common/lights_core.h)
// compiled for the CPU on top of posed_paths_shim.cpp: the posed superset body over a world tree, a model store, an instance table and a
// pose table (both may be empty; the loops over them are the linear ones), with or without a light table.  Never linked into the shipped
// libraries.  -DLIT_PATHS_SHIM_MAIN: a small stand-alone program over the same entries, for the sanitizers.
#include "posed_paths_shim.cpp"

extern "C" {

// One frame of the path loop, planes as the kernel writes them (float4 per pixel; ids may be null).  n_lights == 0: the posed body
// (what the dispatch point launches without a table); else the lit body with the table, its owned set (65536 bits) and its totals.
void lp_render(const void* world, void* const* models, size_t n_models, const blok_instance* inst, uint32_t n_inst, const blok_pose* poses, uint32_t n_poses,
               float vs, const blok_camera* cam, const blok_material* materials, uint32_t n_materials, uint32_t width, uint32_t height, uint32_t spp,
               uint32_t max_bounces, uint32_t frame_index, const blok_light* lights, uint32_t n_lights, const uint32_t* owned, uint32_t n_faces,
               float area_world, float* color, float* world_pos, float* normal_roughness, float* albedo_metallic, uint32_t* ids) {
    const float inv_vs = 1.0f / vs;
    const std::vector<ModelDesc> d = store_descs(models, n_models, vs);
    PathArgs p{};
    p.trace = model_args(static_cast<const Tree*>(world)->desc, vs, inv_vs);
    p.trace.tmin = BLOK_RAY_TMIN; p.trace.tmax = BLOK_RAY_TMAX;
    p.trace.cam = *cam; p.trace.frame_w = width; p.trace.frame_h = height; p.trace.w = width; p.trace.h = height;
    p.trace.mat_table = materials; p.trace.n_materials = n_materials;
    p.spp = spp; p.max_bounces = max_bounces; p.frame_count = frame_index;
    p.color = color; p.world_pos = world_pos; p.normal_roughness = normal_roughness; p.albedo_metallic = albedo_metallic;
    const TlasScene S{inst, d.data(), nullptr, ids, n_inst, static_cast<uint32_t>(n_models)};
    const PoseScene Q{poses, n_poses, nullptr};
    const LightScene L{lights, owned, n_lights, n_faces, area_world};
    std::vector<uint4> stack(size_t(kMaxLevels) * 2 * kBlock);
    for (uint32_t y = 0; y < height; ++y)
        for (uint32_t x = 0; x < width; ++x) {
            const size_t i = size_t(y) * width + x;
            if (n_lights) shade_pixel<false, false, true, true, true>(p, x, y, i, stack.data(), 0.0f, nullptr, nullptr, nullptr, nullptr, &S, &Q, &L);
            else shade_pixel<false, false, true, true>(p, x, y, i, stack.data(), 0.0f, nullptr, nullptr, nullptr, nullptr, &S, &Q);
        }
}

// light_sample for one surface point and three draws: returns 1 with q, Le and g, or 0 (no term and no ray).  The material table is the
// one the light's emission is read from.
int lp_light_sample(const blok_light* lights, uint32_t n_lights, uint32_t n_faces, float area_world, const blok_material* materials, uint32_t n_materials,
                    float vs, const float* hit_pos, const float* n, uint32_t r, float u1, float u2, float* q, float* le, float* g) {
    const LightScene L{lights, nullptr, n_lights, n_faces, area_world};
    V3 vq = v3(0, 0, 0), vle = v3(0, 0, 0);
    float vg = 0.0f;
    const bool has = light_sample(L, materials, n_materials, vs, v3(hit_pos[0], hit_pos[1], hit_pos[2]), v3(n[0], n[1], n[2]), r, u1, u2, vq, vle, vg);
    q[0] = vq.x; q[1] = vq.y; q[2] = vq.z; le[0] = vle.x; le[1] = vle.y; le[2] = vle.z; *g = vg;
    return has ? 1 : 0;
}

}  // extern "C"

#ifdef LIT_PATHS_SHIM_MAIN
// A closed room with a glowing ceiling patch and a floating cube model as an instance and as a pose: a lit and an unlit frame, both finite;
// the G-buffers equal; a floor pixel under the patch brighter with the table.
#include <cmath>
#include <cstdio>

#define LP_REQUIRE(x) do { if (!(x)) { std::fprintf(stderr, "lit_paths_shim: %s failed at line %d\n", #x, __LINE__); return 1; } } while (0)

int main() {
    const int N = 12;
    std::vector<int32_t> xyz; std::vector<uint32_t> ids;
    for (int z = 0; z < N; ++z) for (int y = 0; y < N; ++y) for (int x = 0; x < N; ++x) {
        const bool wall = x == 0 || y == 0 || z == 0 || x == N - 1 || y >= N - 2 || z == N - 1;
        if (!wall) continue;
        xyz.insert(xyz.end(), {x, y, z});
        ids.push_back(y == N - 2 && x >= 5 && x < 7 && z >= 5 && z < 7 ? 2u : 1u);
    }
    const char* why = "";
    void* world = is_model(xyz.data(), ids.data(), ids.size(), &why);
    LP_REQUIRE(world != nullptr);
    const int32_t cube_xyz[] = {0, 0, 0, 1, 0, 0};
    const uint32_t cube_ids[] = {1u, 1u};
    void* model = is_model(cube_xyz, cube_ids, 2, &why);
    LP_REQUIRE(model != nullptr);
    blok_material mats[3] = {};
    for (blok_material& m : mats) { m.albedo[0] = m.albedo[1] = m.albedo[2] = 0.6f; m.flags = 230u << 16; }
    mats[2].emission[0] = 4.0f; mats[2].emission[1] = 3.0f; mats[2].emission[2] = 2.0f;
    const blok_light light = {{5, N - 2, 5}, 2, 2, 2u, 3u, 0u};
    uint32_t owned[blok::lights::kSetWords] = {};
    owned[0] = 1u << 2;
    blok_instance inst{};
    inst.model = 0; inst.offset[0] = 3; inst.offset[1] = 4; inst.offset[2] = 6; inst.axis[0] = 0; inst.axis[1] = 1; inst.axis[2] = 2;
    blok_pose pose{};
    pose.model = 0; pose.m[0][0] = 0.8f; pose.m[0][2] = 0.6f; pose.m[1][1] = 1.0f; pose.m[2][0] = -0.6f; pose.m[2][2] = 0.8f;
    pose.pivot[0] = 8.0f; pose.pivot[1] = 3.0f; pose.pivot[2] = 6.0f; pose.local[0] = 1.0f; pose.local[1] = 0.5f; pose.local[2] = 0.5f;
    blok_camera cam{};
    cam.pos[0] = 6.0f; cam.pos[1] = 7.0f; cam.pos[2] = 2.0f;
    const float f[3] = {0.0f, -0.6f, 0.8f};
    for (int a = 0; a < 3; ++a) cam.fwd[a] = f[a];
    cam.right[0] = 1.0f; cam.up[1] = 0.8f; cam.up[2] = 0.6f;
    cam.tan_half_fov = 0.7f; cam.aspect = 4.0f / 3.0f;
    const uint32_t w = 16, h = 12;
    std::vector<float> lit(4 * w * h), unlit(4 * w * h), g_lit(12 * w * h), g_unlit(12 * w * h);
    std::vector<uint32_t> pix(w * h);
    void* models[1] = {model};
    lp_render(world, models, 1, &inst, 1, &pose, 1, 1.0f, &cam, mats, 3, w, h, 4, 3, 2, &light, 1, owned, 4, 4.0f, lit.data(), g_lit.data(), g_lit.data() + 4 * w * h,
              g_lit.data() + 8 * w * h, pix.data());
    lp_render(world, models, 1, &inst, 1, &pose, 1, 1.0f, &cam, mats, 3, w, h, 4, 3, 2, nullptr, 0, nullptr, 0, 0.0f, unlit.data(), g_unlit.data(),
              g_unlit.data() + 4 * w * h, g_unlit.data() + 8 * w * h, pix.data());
    LP_REQUIRE(std::memcmp(g_lit.data(), g_unlit.data(), g_lit.size() * sizeof(float)) == 0);
    double sum_lit = 0.0, sum_unlit = 0.0;
    for (size_t i = 0; i < lit.size(); ++i) { LP_REQUIRE(std::isfinite(lit[i]) && std::isfinite(unlit[i])); sum_lit += lit[i]; sum_unlit += unlit[i]; }
    LP_REQUIRE(sum_lit > 0.0 && sum_unlit > 0.0);
    std::printf("lit_paths_shim: lit %.6g unlit %.6g\n", sum_lit, sum_unlit);
    is_free(world); is_free(model);
    std::puts("lit_paths_shim: ok");
    return 0;
}
#endif
