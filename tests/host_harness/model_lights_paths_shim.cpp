// TEST INFRASTRUCTURE: the lit path loop over lattice instances whose models carry light tables (blok_amd/csrc/hip/path_core.h:
// shade_pixel<…, kLit, kPlacedLit>, placed_light_sample; csrc/common/lights_core.h) compiled for the CPU on top of lit_paths_shim.cpp.
// The launch's prefix is formed here by the rule's own functions (instance_usable, lights::instance_faces, lights::instance_lights_fit),
// one instance after the other.  Never linked into the shipped libraries.
#include "lit_paths_shim.cpp"

extern "C" {

// lp_render with the models' light tables: tables[m] / table_n[m] for model m (null / 0: none).  The dispatch point's rule: with some
// table and an instance the placed lit body, else what lp_render runs.  out_header (may be null) takes the launch's header, out_icum
// (may be null) its n_inst + 1 words.
void mlp_render(const void* world, void* const* models, size_t n_models, const blok_instance* inst, uint32_t n_inst, const blok_pose* poses, uint32_t n_poses,
                float vs, const blok_camera* cam, const blok_material* materials, uint32_t n_materials, uint32_t width, uint32_t height, uint32_t spp,
                uint32_t max_bounces, uint32_t frame_index, const blok_light* lights, uint32_t n_lights, const uint32_t* owned, uint32_t n_faces,
                float area_world, const blok_light* const* tables, const uint32_t* table_n, float* color, float* world_pos, float* normal_roughness,
                float* albedo_metallic, uint32_t* ids, blok_instance_lights_info* out_header, uint32_t* out_icum) {
    bool any_table = false;
    for (size_t m = 0; m < n_models; ++m) any_table = any_table || (tables && tables[m] && table_n[m]);
    if (!any_table || !n_inst) {
        lp_render(world, models, n_models, inst, n_inst, poses, n_poses, vs, cam, materials, n_materials, width, height, spp, max_bounces, frame_index, lights, n_lights,
                  owned, n_faces, area_world, color, world_pos, normal_roughness, albedo_metallic, ids);
        return;
    }
    const float inv_vs = 1.0f / vs;
    const std::vector<ModelDesc> d = store_descs(models, n_models, vs);
    std::vector<lights::ModelLightTable> T(n_models);
    for (size_t m = 0; m < n_models; ++m) T[m] = lights::ModelLightTable{tables[m], tables[m] ? table_n[m] : 0u, 0u};
    std::vector<uint64_t> faces(n_inst, 0ull);
    uint64_t a_inst = 0;
    for (uint32_t i = 0; i < n_inst; ++i) {
        const blok_instance& I = inst[i];
        if (I.model >= n_models) continue;
        faces[i] = lights::instance_faces(instance_usable(I, d[I.model]) && T[I.model].table != nullptr, T[I.model].n, lights::scale_exponent(d[I.model].scale_log2));
        a_inst += faces[i];
    }
    const bool fit = lights::instance_lights_fit(n_lights ? n_faces : 0u, a_inst);
    std::vector<uint32_t> icum(size_t(n_inst) + 1u, 0u);
    blok_instance_lights_info header{};
    uint64_t sum = 0;
    for (uint32_t i = 0; i < n_inst; ++i) {
        icum[i] = static_cast<uint32_t>(sum);
        if (fit && faces[i]) { sum += faces[i]; header.n_lit += 1u; }
    }
    icum[n_inst] = static_cast<uint32_t>(sum);
    header.a_inst = sum; header.a_total = (n_lights ? n_faces : 0u) + sum; header.area_world = lights::lights_area_world(header.a_total, vs);
    header.disabled = fit ? 0u : 1u;
    if (out_header) *out_header = header;
    if (out_icum) for (size_t i = 0; i < icum.size(); ++i) out_icum[i] = icum[i];
    std::vector<uint32_t> glows(lights::kSetWords);
    lights::emissive_set(materials, n_materials, glows.data());

    PathArgs p{};
    p.trace = model_args(static_cast<const Tree*>(world)->desc, vs, inv_vs);
    p.trace.tmin = BLOK_RAY_TMIN; p.trace.tmax = BLOK_RAY_TMAX;
    p.trace.cam = *cam; p.trace.frame_w = width; p.trace.frame_h = height; p.trace.w = width; p.trace.h = height;
    p.trace.mat_table = materials; p.trace.n_materials = n_materials;
    p.spp = spp; p.max_bounces = max_bounces; p.frame_count = frame_index;
    p.color = color; p.world_pos = world_pos; p.normal_roughness = normal_roughness; p.albedo_metallic = albedo_metallic;
    const TlasScene S{inst, d.data(), nullptr, ids, n_inst, static_cast<uint32_t>(n_models)};
    const PoseScene Q{poses, n_poses, nullptr};
    const LightScene L = n_lights ? LightScene{lights, owned, n_lights, n_faces, area_world} : LightScene{nullptr, nullptr, 0u, 0u, 0.0f};
    const InstanceLightScene IL{icum.data(), &header, T.data(), static_cast<uint32_t>(n_models), glows.data()};
    std::vector<uint4> stack(size_t(kMaxLevels) * 2 * kBlock);
    for (uint32_t y = 0; y < height; ++y)
        for (uint32_t x = 0; x < width; ++x)
            shade_pixel<false, false, true, true, true, true>(p, x, y, size_t(y) * width + x, stack.data(), 0.0f, nullptr, nullptr, nullptr, nullptr, &S, &Q, &L, &IL);
}

}  // extern "C"
