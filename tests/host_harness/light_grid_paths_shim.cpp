// TEST INFRASTRUCTURE: the lit path loop under a light grid (blok_amd/csrc/hip/path_core.h: shade_pixel<…, kLit, false, kGrid>,
// grid_light_sample; csrc/common/lights_core.h) compiled for the CPU on top of lit_paths_shim.cpp.  Never linked into the shipped libraries.
#include "lit_paths_shim.cpp"

extern "C" {

// lp_render's frame with the grid's arrays and figures; has_grid == 0: the lit body (the grid flag off).
void gp_render(const void* world, void* const* models, size_t n_models, const blok_instance* inst, uint32_t n_inst, const blok_pose* poses, uint32_t n_poses,
               float vs, const blok_camera* cam, const blok_material* materials, uint32_t n_materials, uint32_t width, uint32_t height, uint32_t spp,
               uint32_t max_bounces, uint32_t frame_index, const blok_light* lights, uint32_t n_lights, const uint32_t* owned, uint32_t n_faces,
               float area_world, int has_grid, const uint32_t* start, const uint32_t* faces, const blok_light_grid_item* items, const blok_light_grid_info* info,
               float* color, float* world_pos, float* normal_roughness, float* albedo_metallic, uint32_t* ids) {
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
    GridScene G{};
    if (has_grid) G = GridScene{start, faces, items, {info->cell_lo[0], info->cell_lo[1], info->cell_lo[2]}, {info->dim[0], info->dim[1], info->dim[2]},
                                info->cell_log2, info->reach, info->share};
    std::vector<uint4> stack(size_t(kMaxLevels) * 2 * kBlock);
    for (uint32_t y = 0; y < height; ++y)
        for (uint32_t x = 0; x < width; ++x) {
            const size_t i = size_t(y) * width + x;
            if (has_grid) shade_pixel<false, false, true, true, true, false, true>(p, x, y, i, stack.data(), 0.0f, nullptr, nullptr, nullptr, nullptr, &S, &Q, &L, nullptr, &G);
            else shade_pixel<false, false, true, true, true>(p, x, y, i, stack.data(), 0.0f, nullptr, nullptr, nullptr, nullptr, &S, &Q, &L);
        }
}

// grid_light_sample over the world's table for one surface point and four draws: returns 1 with q, Le and g, or 0.
int gp_light_sample(const blok_light* lights, uint32_t n_lights, uint32_t n_faces, const uint32_t* start, const uint32_t* faces, const blok_light_grid_item* items,
                    const blok_light_grid_info* info, const blok_material* materials, uint32_t n_materials, float vs, const float* hit_pos, const float* n, uint32_t r,
                    float u1, float u2, uint32_t m, float* q, float* le, float* g) {
    const LightScene L{lights, nullptr, n_lights, n_faces, 0.0f};
    const GridScene G{start, faces, items, {info->cell_lo[0], info->cell_lo[1], info->cell_lo[2]}, {info->dim[0], info->dim[1], info->dim[2]}, info->cell_log2, info->reach,
                      info->share};
    V3 vq = v3(0, 0, 0), vle = v3(0, 0, 0);
    float vg = 0.0f;
    const bool has = grid_light_sample(L, G, materials, n_materials, vs, v3(hit_pos[0], hit_pos[1], hit_pos[2]), v3(n[0], n[1], n[2]), r, u1,
                                              u2, m, vq, vle, vg);
    q[0] = vq.x; q[1] = vq.y; q[2] = vq.z; le[0] = vle.x; le[1] = vle.y; le[2] = vle.z; *g = vg;
    return has ? 1 : 0;
}

}  // extern "C"
