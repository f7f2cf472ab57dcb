// Instanced voxel models (include/blok_hip.h, instance_core.h): the model store on the context and the instanced trace entries.
#include "api_internal.h"
#include "posed_core.h"

#include <algorithm>
#include <limits>

namespace blok_api {

namespace {

// The device copy of the descriptors after a change (the callers have synchronised the device), and the LDS stack the kernels need.
// The limit of a scaled model's voxel size is settled here, once per model: the kernels see such a model as they see a destroyed one.
int upload_models(blok_hip_ctx* ctx) {
    auto& M = ctx->models;
    if (M.d_desc.capacity() < M.desc.size())
        BLOK_HIP_TRY(ctx, M.d_desc.reserve(std::max<size_t>(16, M.desc.size() * 2), blok::FreeAfter::nothing()));
    if (!M.desc.empty()) {
        std::vector<blok::ModelDesc> copy = M.desc;
        for (blok::ModelDesc& m : copy)
            if (!blok::model_size_usable(m, ctx->world_voxel_size)) m.nodes = nullptr;
        BLOK_HIP_TRY(ctx, hipMemcpy(M.d_desc, copy.data(), copy.size() * sizeof(blok::ModelDesc), hipMemcpyHostToDevice));
    }
    M.uploaded_voxel_size = ctx->world_voxel_size;
    uint32_t slots = 1;
    for (const auto& m : M.desc)
        if (m.nodes && m.levels > 1) slots = std::max(slots, m.levels - 1u);
    M.stack_levels = slots;
    return BLOK_OK;
}

// The kernels' copy of the models' light tables, one entry per model id, with `with` standing in model `model`'s place (the table about to
// be installed; null: none).  Waits for the device first when the array in use is replaced: frames in flight may read it.
int upload_model_lights(blok_hip_ctx* ctx, uint32_t model, const blok_light* with, uint32_t with_n) {
    auto& M = ctx->models;
    std::vector<blok::lights::ModelLightTable> copy(M.desc.size(), blok::lights::ModelLightTable{nullptr, 0u, 0u});
    for (size_t i = 0; i < M.lights.size() && i < copy.size(); ++i) copy[i] = blok::lights::ModelLightTable{M.lights[i].table.get(), M.lights[i].n, 0u};
    if (model < copy.size()) copy[model] = blok::lights::ModelLightTable{with, with ? with_n : 0u, 0u};
    if (copy.empty()) return BLOK_OK;
    BLOK_HIP_TRY(ctx, hipDeviceSynchronize());
    BLOK_HIP_TRY(ctx, M.d_lights.reserve(std::max<size_t>(16, copy.size()), blok::FreeAfter::nothing()));
    M.n_lights_uploaded = 0u;
    BLOK_HIP_TRY(ctx, hipMemcpy(M.d_lights, copy.data(), copy.size() * sizeof(copy[0]), hipMemcpyHostToDevice));
    M.n_lights_uploaded = static_cast<uint32_t>(copy.size());
    return BLOK_OK;
}

// Model `model` goes without a light table from here on (its id is known to be in range of desc).
int drop_model_lights(blok_hip_ctx* ctx, uint32_t model) {
    auto& M = ctx->models;
    if (model >= M.lights.size() || !M.lights[model].n) return BLOK_OK;
    const int rc = upload_model_lights(ctx, model, nullptr, 0u);        // (synchronises: nothing reads the table any more)
    if (rc != BLOK_OK) return rc;
    M.lights[model] = blok_hip_ctx::Models::LightTable{};
    M.n_light_tables -= 1u;
    if (!M.n_light_tables) M.d_glows.reset();           // (kept while any model has a table; the upload above has synchronised)
    return BLOK_OK;
}

void model_lights_info_of(const blok_hip_ctx* ctx, uint32_t model, blok_lights_info* out) {
    if (!out) return;
    *out = blok_lights_info{};
    const auto& T = ctx->models.lights;
    if (model >= T.size()) return;
    out->n = T[model].n; out->n_faces = T[model].n; out->bytes = static_cast<uint64_t>(T[model].n) * sizeof(blok_light);
}

int check_table(blok_hip_ctx* ctx, const blok_instance* inst, uint32_t n) {
    if (n && !inst) return set_error(ctx, BLOK_ERR_INVALID_ARG, "null instance table with non-zero count");
    for (uint32_t i = 0; i < n; ++i) {
        const blok_instance& I = inst[i];
        const std::string at = "instance " + std::to_string(i) + ": ";
        if (!blok::instance_well_formed(I)) {
            if (I.reserved[0] | I.reserved[1] | I.reserved[2]) return set_error(ctx, BLOK_ERR_INVALID_ARG, at + "reserved field is not zero");
            if (I.flip >= 8u) return set_error(ctx, BLOK_ERR_INVALID_ARG, at + "flip has bits above the three axes");
            return set_error(ctx, BLOK_ERR_INVALID_ARG, at + "axis is not a permutation of 0, 1, 2");
        }
        if (!known_model(ctx, I.model))
            return set_error(ctx, BLOK_ERR_INVALID_ARG, at + "unknown model " + std::to_string(I.model));
        if (!blok::instance_usable(I, ctx->models.desc[I.model]))
            return set_error(ctx, BLOK_ERR_INVALID_ARG, at + "world box outside the int16 lattice of hit records");
        if (!blok::model_size_usable(ctx->models.desc[I.model], ctx->world_voxel_size))
            return set_error(ctx, BLOK_ERR_INVALID_ARG, at + "the scaled model's voxel size (world voxel size * 2^scale) is above 256");
    }
    return BLOK_OK;
}

// The limits of a pose table (blok_hip.h, "Posed models"), naming the first pose that breaks one.
int check_pose_table(blok_hip_ctx* ctx, const blok_pose* poses, uint32_t n) {
    if (n && !poses) return set_error(ctx, BLOK_ERR_INVALID_ARG, "null pose table with non-zero count");
    if (n >= BLOK_POSE_ID) return set_error(ctx, BLOK_ERR_INVALID_ARG, "more than 2^31 - 1 poses");
    for (uint32_t i = 0; i < n; ++i) {
        const blok_pose& S = poses[i];
        const std::string at = "pose " + std::to_string(i) + ": ";
        if (const int rule = blok::pose::floats_rule(S)) return set_error(ctx, BLOK_ERR_INVALID_ARG, at + blok::pose::rule_text(rule));
        if (!known_model(ctx, S.model))
            return set_error(ctx, BLOK_ERR_INVALID_ARG, at + "unknown model " + std::to_string(S.model));
        if (!blok::pose_model_box_usable(ctx->models.desc[S.model]))
            return set_error(ctx, BLOK_ERR_INVALID_ARG, at + "the model's own voxel box lies outside the int16 lattice of hit records");
        if (!blok::model_size_usable(ctx->models.desc[S.model], ctx->world_voxel_size))
            return set_error(ctx, BLOK_ERR_INVALID_ARG, at + "the scaled model's voxel size (world voxel size * 2^scale) is above 256");
    }
    return BLOK_OK;
}

// Where the camera's basis puts a world point on screen (instance_core.h: BinView).
blok::BinView bin_view(const blok_hip_ctx* ctx, const blok_camera& c) {
    blok::BinView V{};
    auto cross = [](const float* a, const float* b, float* o) {
        o[0] = a[1] * b[2] - a[2] * b[1]; o[1] = a[2] * b[0] - a[0] * b[2]; o[2] = a[0] * b[1] - a[1] * b[0];
    };
    float ru[3], uf[3], fr[3];
    cross(c.right, c.up, ru); cross(c.up, c.fwd, uf); cross(c.fwd, c.right, fr);
    const float det = c.fwd[0] * ru[0] + c.fwd[1] * ru[1] + c.fwd[2] * ru[2];
    auto norm = [](const float* a) { return std::sqrt(a[0] * a[0] + a[1] * a[1] + a[2] * a[2]); };
    const float scale = norm(c.fwd) * norm(c.right) * norm(c.up);
    V.usable = std::isfinite(det) && std::fabs(det) > 1e-6f * scale;
    if (!V.usable) return V;
    for (int k = 0; k < 3; ++k) {
        V.pos[k] = c.pos[k];
        V.cl[k] = ru[k] / det; V.cu[k] = uf[k] / det; V.cv[k] = fr[k] / det;
    }
    // camera_plane_uv (trace_core.h) inverted: pixel index x (centre at x + 0.5 in frame units) of camera-plane u, y of v
    const float W = static_cast<float>(ctx->width), H = static_cast<float>(ctx->height);
    const float jx = (2.0f * ctx->jitter_px[0]) / W, jy = (2.0f * ctx->jitter_px[1]) / H;
    V.sx = W / (2.0f * c.tan_half_fov * c.aspect);
    V.bx = (1.0f - jx) * 0.5f * W - 0.5f;
    V.sy = -H / (2.0f * c.tan_half_fov);
    V.by = (1.0f - jy) * 0.5f * H - 0.5f;
    return V;
}

blok::InstanceArgs instance_args(const blok_hip_ctx* ctx, const blok::TraceArgs& world, const blok_instance* inst, uint32_t n, blok_hit* hits,
                                 uint32_t* rgba, uint32_t* ids) {
    blok::InstanceArgs P{};
    P.world = world;
    P.instances = inst; P.n_instances = n;
    P.models = ctx->models.d_desc; P.n_models = static_cast<uint32_t>(ctx->models.desc.size());
    P.hits = hits; P.rgba = rgba; P.ids = ids;
    P.stack_levels = ctx->models.stack_levels;
    return P;
}

// ---- what the instanced and the posed entries share ----------------------------------------------------------------------------------------
// The table pointers of a device entry (the tables themselves are the kernels' to judge: instance_usable, pose_usable).
int check_device_tables(blok_hip_ctx* ctx, const blok_instance* inst, uint32_t n_inst, const blok_pose* poses, uint32_t n_poses) {
    if (n_inst && !inst) return set_error(ctx, BLOK_ERR_INVALID_ARG, "null instance table with non-zero count");
    if (n_poses && !poses) return set_error(ctx, BLOK_ERR_INVALID_ARG, "null pose table with non-zero count");
    if (n_poses >= BLOK_POSE_ID) return set_error(ctx, BLOK_ERR_INVALID_ARG, "more than 2^31 - 1 poses");
    return BLOK_OK;
}

// The arguments of a frame's device entry, in the order the entries have always checked them.
int check_frame(blok_hip_ctx* ctx, const blok_camera* cam, uint32_t x0, uint32_t y0, uint32_t w, uint32_t h, bool any_output,
                const blok_instance* inst, uint32_t n_inst, const blok_pose* poses, uint32_t n_poses) {
    const int rc = check_trace(ctx, cam);
    if (rc != BLOK_OK) return rc;
    if (!any_output || !rect_inside(ctx, x0, y0, w, h)) return set_error(ctx, BLOK_ERR_INVALID_ARG, "rectangle outside the frame or no output");
    return check_device_tables(ctx, inst, n_inst, poses, n_poses);
}

// The arguments of a rays entry, host or device, up to its tables.  BLOK_OK with n == 0: nothing to trace, the entry returns BLOK_OK.
int check_rays(blok_hip_ctx* ctx, const blok_ray* rays, size_t n, bool any_output) {
    if (!ctx) return BLOK_ERR_INVALID_ARG;
    if (!ctx->has_world) return set_error(ctx, BLOK_ERR_NO_WORLD, "no world uploaded");
    if (n != 0 && (!rays || !any_output || n > 0x7FFFFFFFu)) return set_error(ctx, BLOK_ERR_INVALID_ARG, "bad ray arguments");
    return BLOK_OK;
}

// The set-up of a frame pass (lattice or posed) over the rectangle: the kernels' arguments but for the table, with the rectangle, the bins'
// dimensions and view, room in `bins` (the stream's scratch for this pass) and the stream's scratch records where the caller passes none.
int frame_pass(blok_hip_ctx* ctx, const blok_camera* cam, uint32_t x0, uint32_t y0, uint32_t w, uint32_t h, hipStream_t stream,
               blok::DeviceArray<uint32_t>& bins, void* out_hits_dev, void* out_rgba_dev, uint32_t* out_instance_dev, blok::InstanceArgs& P) {
    blok_hit* hits = static_cast<blok_hit*>(out_hits_dev);
    if (!hits) {
        auto& sc = ctx->beam_buffers[stream];
        BLOK_HIP_TRY(ctx, sc.inst_hits.reserve(static_cast<size_t>(w) * h, blok::FreeAfter::work_on(stream)));
        hits = sc.inst_hits;
    }
    blok::TraceArgs world = base_args(ctx, cam);
    world.x0 = x0; world.y0 = y0; world.w = w; world.h = h;
    P = instance_args(ctx, world, nullptr, 0u, hits, static_cast<uint32_t*>(out_rgba_dev), out_instance_dev);
    P.bins_x = (w + blok::kBinPixels - 1u) / blok::kBinPixels;
    P.bins_y = (h + blok::kBinPixels - 1u) / blok::kBinPixels;
    P.view = bin_view(ctx, *cam);
    BLOK_HIP_TRY(ctx, bins.reserve(static_cast<size_t>(P.bins_x) * P.bins_y * blok::kBinWords, blok::FreeAfter::work_on(stream)));
    P.bins = bins;
    return BLOK_OK;
}

// ... of a rays pass: the rays, and the stream's scratch records where the caller passes none.
int rays_pass(blok_hip_ctx* ctx, const blok_ray* rays_dev, size_t n, hipStream_t stream, blok_hit* out_hits_dev, uint32_t* out_instance_dev,
              blok::InstanceArgs& P) {
    blok_hit* hits = out_hits_dev;
    if (!hits) {
        auto& sc = ctx->beam_buffers[stream];
        BLOK_HIP_TRY(ctx, sc.inst_hits.reserve(n, blok::FreeAfter::work_on(stream)));
        hits = sc.inst_hits;
    }
    blok::TraceArgs world = base_args(ctx, nullptr);
    world.rays = rays_dev; world.n_rays = static_cast<uint32_t>(n);
    P = instance_args(ctx, world, nullptr, 0u, hits, nullptr, out_instance_dev);
    return BLOK_OK;
}

// The blocking primary frame of both tables (an empty pose table: the instanced entry's), named `entry` in a HIP failure's text.
int trace_primary_placed(blok_hip_ctx* ctx, const char* entry, const blok_camera* cam, uint32_t x0, uint32_t y0, uint32_t w, uint32_t h,
                         const blok_instance* instances_host, uint32_t n_instances, const blok_pose* poses_host, uint32_t n_poses,
                         blok_hit* out_hits_host, uint32_t* out_rgba_host, uint32_t* out_instance_host) {
    int rc = check_trace(ctx, cam);
    if (rc != BLOK_OK) return rc;
    if ((!out_hits_host && !out_rgba_host && !out_instance_host) || !rect_inside(ctx, x0, y0, w, h))
        return set_error(ctx, BLOK_ERR_INVALID_ARG, "rectangle outside the frame or no output");
    rc = check_table(ctx, instances_host, n_instances);
    if (rc == BLOK_OK) rc = check_pose_table(ctx, poses_host, n_poses);
    if (rc != BLOK_OK) return rc;
    const size_t n = static_cast<size_t>(w) * h;
    StagedBlock d;
    const auto inst = d.input(instances_host, n_instances);
    const auto poses = d.input(poses_host, n_poses);
    const auto hits = d.output(out_hits_host, n);
    const auto rgba = d.output(out_rgba_host, n);
    const auto ids = d.output(out_instance_host, n);
    rc = d.stage(ctx, entry);
    if (rc != BLOK_OK) return rc;
    rc = blok_hip_trace_primary_posed_device(ctx, cam, x0, y0, w, h, d.at(inst), n_instances, d.at(poses), n_poses, d.at(hits), d.wanted(rgba),
                                             d.wanted(ids), nullptr);
    return d.collect(ctx, entry, rc);
}

// ... and the blocking rays.
int trace_rays_placed(blok_hip_ctx* ctx, const char* entry, const blok_ray* rays_host, size_t n, const blok_instance* instances_host,
                      uint32_t n_instances, const blok_pose* poses_host, uint32_t n_poses, blok_hit* out_hits_host, uint32_t* out_instance_host) {
    int rc = check_rays(ctx, rays_host, n, out_hits_host || out_instance_host);
    if (rc != BLOK_OK || n == 0) return rc;
    rc = check_table(ctx, instances_host, n_instances);
    if (rc == BLOK_OK) rc = check_pose_table(ctx, poses_host, n_poses);
    if (rc != BLOK_OK) return rc;
    BLOK_HIP_TRY(ctx, hipSetDevice(ctx->device));
    StagedBlock d;
    const auto inst = d.input(instances_host, n_instances);
    const auto poses = d.input(poses_host, n_poses);
    const auto rays = d.input(rays_host, n);
    const auto hits = d.output(out_hits_host, n);
    const auto ids = d.output(out_instance_host, n);
    rc = d.stage(ctx, entry);
    if (rc != BLOK_OK) return rc;
    rc = blok_hip_trace_rays_posed_device(ctx, d.at(rays), n, d.at(inst), n_instances, d.at(poses), n_poses, d.at(hits), d.wanted(ids), nullptr);
    return d.collect(ctx, entry, rc);
}

}  // namespace

int check_instance_table(blok_hip_ctx* ctx, const blok_instance* inst, uint32_t n) { return check_table(ctx, inst, n); }

void clear_model_lights(blok_hip_ctx* ctx) {
    auto& M = ctx->models;
    if (!M.n_light_tables) { M.d_glows.reset(); return; }      // (a set left by a build that failed behind it: no frame reads it without a table)
    (void)hipDeviceSynchronize();                       // whatever still reads the tables
    M.lights.clear(); M.n_light_tables = 0u; M.d_glows.reset();
    M.n_lights_uploaded = 0u;                           // the kernels' copy names no table any more: every id counts as none
}
int check_placed_device_tables(blok_hip_ctx* ctx, const blok_instance* inst, uint32_t n_inst, const blok_pose* poses, uint32_t n_poses) {
    return check_device_tables(ctx, inst, n_inst, poses, n_poses);
}

int refuse_scaled_model(blok_hip_ctx* ctx, const char* op, uint32_t model) {
    if (known_model(ctx, model) && ctx->models.desc[model].scale_log2 != 0u)
        return set_error(ctx, BLOK_ERR_UNSUPPORTED, std::string(op) + ": model " + std::to_string(model) + " has a scale (blok_hip_model_set_scale); the volume takes scale-0 models only");
    return BLOK_OK;
}

int models_follow_voxel_size(blok_hip_ctx* ctx) {
    auto& M = ctx->models;
    if (M.uploaded_voxel_size == ctx->world_voxel_size) return BLOK_OK;
    bool changes = false;
    blok::ModelDesc probe{};
    for (const blok::ModelDesc& m : M.desc) {
        probe.scale_log2 = m.scale_log2;
        changes = changes || (m.nodes && blok::model_size_usable(probe, M.uploaded_voxel_size) != blok::model_size_usable(probe, ctx->world_voxel_size));
    }
    if (!changes) { M.uploaded_voxel_size = ctx->world_voxel_size; return BLOK_OK; }
    BLOK_HIP_TRY(ctx, hipDeviceSynchronize());           // frames in flight read the descriptor array
    return upload_models(ctx);
}

int add_model(blok_hip_ctx* ctx, const blok::ModelDesc& m, blok_hip_ctx::Models::Arrays own, uint32_t* out_model) {
    // a new model has scale 0: its descriptor's box is the box in its own voxels, which the store keeps for blok_hip_model_set_scale.
    // Every producer's box lies within 2^17 of the model's origin (the lattice of the records, a volume's extent), so its 2^8-fold fits.
    for (int a = 0; a < 3; ++a) {
        if (m.lo[a] < -(1 << 22) || m.hi[a] > (1 << 22)) return set_error(ctx, BLOK_ERR_INTERNAL, "model box beyond 2^22 voxels");
        own.box_lo[a] = m.lo[a]; own.box_hi[a] = m.hi[a];
    }
    // frames in flight may read the descriptor array that the upload replaces
    hipError_t e = hipDeviceSynchronize();
    int rc = BLOK_OK;
    if (e != hipSuccess) rc = set_error(ctx, BLOK_ERR_HIP, std::string("hipDeviceSynchronize: ") + hipGetErrorString(e));
    if (rc == BLOK_OK) {
        ctx->models.desc.push_back(m);
        rc = upload_models(ctx);
        if (rc != BLOK_OK) ctx->models.desc.pop_back();
    }
    if (rc != BLOK_OK) return rc;                       // (`own` frees the arrays)
    ctx->models.own.resize(ctx->models.desc.size());
    ctx->models.own.back() = std::move(own);
    *out_model = static_cast<uint32_t>(ctx->models.desc.size() - 1u);
    return BLOK_OK;
}

blok::MotionTables motion_tables(const blok_hip_ctx* ctx, const uint32_t* ids, const blok_instance* cur, uint32_t n_cur, const blok_instance* prev,
                                 uint32_t n_prev) {
    blok::MotionTables M{};
    M.ids = ids;
    M.cur = cur; M.n_cur = n_cur;
    M.prev = prev; M.n_prev = n_prev;
    M.models = ctx->models.d_desc; M.n_models = ctx->models.d_desc ? static_cast<uint32_t>(ctx->models.desc.size()) : 0u;
    M.vs = ctx->world_voxel_size;
    return M;
}

int prepare_pose_motion(blok_hip_ctx* ctx, const blok_pose* cur, uint32_t n_cur, const blok_pose* prev, uint32_t n_prev, hipStream_t stream,
                        const blok_pose_motion** out) {
    *out = nullptr;
    if (!n_cur) return BLOK_OK;
    auto& scratch = ctx->beam_buffers[stream];
    BLOK_HIP_TRY(ctx, scratch.pose_motion.reserve(n_cur, blok::FreeAfter::work_on(stream)));
    blok::launch_pose_motion_prepare(cur, n_cur, prev, n_prev, ctx->models.d_desc, ctx->models.d_desc ? static_cast<uint32_t>(ctx->models.desc.size()) : 0u,
                                     scratch.pose_motion, stream);
    BLOK_HIP_TRY(ctx, hipGetLastError());
    *out = scratch.pose_motion;
    return BLOK_OK;
}

blok::PoseMotionTables pose_motion_tables(const blok_hip_ctx* ctx, const uint32_t* ids, const blok_instance* cur, uint32_t n_cur, const blok_instance* prev,
                                          uint32_t n_prev, const blok_pose_motion* records, uint32_t n_cur_poses) {
    blok::PoseMotionTables Q{};
    Q.inst = motion_tables(ctx, ids, cur, n_cur, prev, n_prev);
    Q.records = records; Q.n_cur = records ? n_cur_poses : 0u;
    return Q;
}

int posed_motion_pass(blok_hip_ctx* ctx, uint32_t x0, uint32_t y0, uint32_t w, uint32_t h, const float* world_pos_dev, const blok::PoseMotionTables& tables,
                      const float prev_view_proj[16], uint16_t* motion_h_dev, float* motion_dev, hipStream_t stream) {
    blok::PosedMotionArgs a{};
    a.m = tables;
    a.world_pos = world_pos_dev;
    a.x0 = x0; a.y0 = y0; a.w = w; a.h = h; a.frame_w = ctx->width; a.frame_h = ctx->height;
    for (int k = 0; k < 16; ++k) a.prev_view_proj[k] = prev_view_proj[k];
    a.motion_h = motion_h_dev; a.motion = motion_dev;
    blok::launch_posed_motion(a, stream);
    BLOK_HIP_TRY(ctx, hipGetLastError());
    return BLOK_OK;
}

}  // namespace blok_api

using namespace blok_api;

extern "C" {

int blok_hip_model_create(blok_hip_ctx* ctx, const int32_t* xyz, const uint32_t* material_ids, size_t n, uint32_t* out_model) {
    if (!ctx) return BLOK_ERR_INVALID_ARG;
    if (!xyz || !material_ids || !out_model || n == 0) return set_error(ctx, BLOK_ERR_INVALID_ARG, "model needs at least one voxel and an output id");
    if (ctx->models.desc.size() >= std::numeric_limits<uint32_t>::max() - 1u) return set_error(ctx, BLOK_ERR_INVALID_ARG, "model ids exhausted");
    std::vector<blok::VoxelRec> voxels(n);
    int32_t lo[3] = {std::numeric_limits<int32_t>::max(), std::numeric_limits<int32_t>::max(), std::numeric_limits<int32_t>::max()};
    int32_t hi[3] = {std::numeric_limits<int32_t>::min(), std::numeric_limits<int32_t>::min(), std::numeric_limits<int32_t>::min()};
    for (size_t i = 0; i < n; ++i) {
        voxels[i] = blok::VoxelRec{xyz[3 * i], xyz[3 * i + 1], xyz[3 * i + 2], material_ids[i]};
        for (int a = 0; a < 3; ++a) { lo[a] = std::min(lo[a], xyz[3 * i + a]); hi[a] = std::max(hi[a], xyz[3 * i + a]); }
    }
    blok::HostTree tree;
    const char* why = "";
    if (!blok::build_tree(voxels, tree, &why)) return set_error(ctx, BLOK_ERR_UNSUPPORTED, std::string("model: ") + why);
    BLOK_HIP_TRY(ctx, hipSetDevice(ctx->device));
    blok::ModelDesc m{};
    const size_t node_bytes = tree.nodes.size() * sizeof(blok::TreeNode), mat_bytes = tree.materials.size() * sizeof(uint32_t);
    blok_hip_ctx::Models::Arrays own;
    hipError_t e = own.nodes.reserve(tree.nodes.size(), blok::FreeAfter::nothing());
    if (e == hipSuccess) e = own.materials.reserve(tree.materials.size(), blok::FreeAfter::nothing());
    if (e == hipSuccess) e = hipMemcpy(own.nodes, tree.nodes.data(), node_bytes, hipMemcpyHostToDevice);
    if (e == hipSuccess) e = hipMemcpy(own.materials, tree.materials.data(), mat_bytes, hipMemcpyHostToDevice);
    if (e != hipSuccess) return set_error(ctx, e == hipErrorOutOfMemory ? BLOK_ERR_OOM : BLOK_ERR_HIP, std::string("model upload: ") + hipGetErrorString(e));
    m.nodes = own.nodes; m.materials = own.materials; m.levels = tree.levels;
    own.n_nodes = static_cast<uint32_t>(tree.nodes.size()); own.n_materials = static_cast<uint32_t>(tree.materials.size());
    for (int a = 0; a < 3; ++a) { m.origin[a] = tree.origin[a]; m.lo[a] = lo[a]; m.hi[a] = hi[a] + 1; }
    return add_model(ctx, m, std::move(own), out_model);
}

int blok_hip_model_destroy(blok_hip_ctx* ctx, uint32_t model) {
    if (!ctx) return BLOK_ERR_INVALID_ARG;
    if (!known_model(ctx, model)) return set_error(ctx, BLOK_ERR_INVALID_ARG, "unknown model " + std::to_string(model));
    BLOK_HIP_TRY(ctx, hipSetDevice(ctx->device));
    BLOK_HIP_TRY(ctx, hipDeviceSynchronize());           // frames in flight may still walk it
    const int rc_lights = drop_model_lights(ctx, model);
    if (rc_lights != BLOK_OK) return rc_lights;
    ctx->models.own[model] = blok_hip_ctx::Models::Arrays{};
    ctx->models.desc[model] = blok::ModelDesc{};         // the id stays taken and unknown
    return upload_models(ctx);
}

// ---- emissive models as lights (blok_hip.h; lights_kernels.hip) -------------------------------------------------------------

int blok_hip_model_lights(blok_hip_ctx* ctx, uint32_t model, uint32_t flags, blok_lights_info* out_info) {
    if (!ctx) return BLOK_ERR_INVALID_ARG;
    if (!known_model(ctx, model)) return set_error(ctx, BLOK_ERR_INVALID_ARG, "model_lights: unknown model " + std::to_string(model));
    if (flags) return set_error(ctx, BLOK_ERR_INVALID_ARG, "model_lights: unknown flag bits");
    if (!ctx->n_materials || ctx->material_glows.size() != blok::lights::kSetWords) return set_error(ctx, BLOK_ERR_INVALID_ARG, "model_lights: no material table");
    BLOK_HIP_TRY(ctx, hipSetDevice(ctx->device));
    auto& M = ctx->models;
    blok::DeviceArray<uint32_t> glows;
    BLOK_HIP_TRY(ctx, glows.reserve(blok::lights::kSetWords, blok::FreeAfter::nothing()));
    BLOK_HIP_TRY(ctx, hipMemcpy(glows, ctx->material_glows.data(), blok::lights::kSetWords * sizeof(uint32_t), hipMemcpyHostToDevice));
    const blok::ModelDesc& d = M.desc[model];
    const auto& own = M.own[model];
    blok::GpuLights made;
    std::string why;
    const uint32_t n_mat = static_cast<uint32_t>(std::min<size_t>(ctx->n_materials, blok::lights::kSetBits));
    const blok::GpuBuildStatus st = blok::gpu_model_lights(d.nodes, own.n_nodes, d.materials, own.n_materials, d.levels, d.origin, glows, n_mat, &made, &why);
    if (st != blok::GpuBuildStatus::Ok)
        return set_error(ctx, st == blok::GpuBuildStatus::OutOfMemory ? BLOK_ERR_OOM : st == blok::GpuBuildStatus::Unsupported ? BLOK_ERR_UNSUPPORTED :
                              st == blok::GpuBuildStatus::HipError ? BLOK_ERR_HIP : BLOK_ERR_INTERNAL, why);
    blok::DeviceArray<blok_light> table;
    table.adopt(made.d_lights, made.n);
    if (!made.n) {                                      // no faces: no table
        const int rc = drop_model_lights(ctx, model);
        if (rc != BLOK_OK) return rc;
        model_lights_info_of(ctx, model, out_info);
        return BLOK_OK;
    }
    // the emissive set for the path loop's rule (e), kept while any model has a table: written once, when it is allocated (no frame reads it
    // before a table exists, and every table goes with the material table it was built for, so the words never change while it lives)
    if (!M.d_glows) {
        BLOK_HIP_TRY(ctx, M.d_glows.reserve(blok::lights::kSetWords, blok::FreeAfter::nothing()));
        BLOK_HIP_TRY_FILL(ctx, M.d_glows, hipMemcpy(M.d_glows, glows, blok::lights::kSetWords * sizeof(uint32_t), hipMemcpyDeviceToDevice));
    }
    const int rc = upload_model_lights(ctx, model, table.get(), made.n);
    if (rc != BLOK_OK) return rc;                       // (`table` frees the new one; the old one stays)
    if (M.lights.size() < M.desc.size()) M.lights.resize(M.desc.size());
    if (!M.lights[model].n) M.n_light_tables += 1u;
    M.lights[model].table = std::move(table); M.lights[model].n = made.n;
    model_lights_info_of(ctx, model, out_info);
    return BLOK_OK;
}

int blok_hip_model_lights_info(blok_hip_ctx* ctx, uint32_t model, blok_lights_info* out_info) {
    if (!ctx) return BLOK_ERR_INVALID_ARG;
    if (!known_model(ctx, model)) return set_error(ctx, BLOK_ERR_INVALID_ARG, "model_lights_info: unknown model " + std::to_string(model));
    if (!out_info) return set_error(ctx, BLOK_ERR_INVALID_ARG, "model_lights_info: null output");
    model_lights_info_of(ctx, model, out_info);
    return BLOK_OK;
}

int blok_hip_model_lights_download(blok_hip_ctx* ctx, uint32_t model, blok_light* out_host, uint64_t first, uint64_t count) {
    if (!ctx) return BLOK_ERR_INVALID_ARG;
    if (!known_model(ctx, model)) return set_error(ctx, BLOK_ERR_INVALID_ARG, "model_lights_download: unknown model " + std::to_string(model));
    const auto& T = ctx->models.lights;
    const uint64_t n = model < T.size() ? T[model].n : 0u;
    if (first > n || count > n - first) return set_error(ctx, BLOK_ERR_INVALID_ARG, "model_lights_download: range past the end of the table");
    if (count == 0) return BLOK_OK;
    if (!out_host) return set_error(ctx, BLOK_ERR_INVALID_ARG, "model_lights_download: null output");
    BLOK_HIP_TRY(ctx, hipSetDevice(ctx->device));
    BLOK_HIP_TRY(ctx, hipMemcpy(out_host, T[model].table.get() + first, count * sizeof(blok_light), hipMemcpyDeviceToHost));
    return BLOK_OK;
}

int blok_hip_model_lights_clear(blok_hip_ctx* ctx, uint32_t model) {
    if (!ctx) return BLOK_ERR_INVALID_ARG;
    if (!known_model(ctx, model)) return set_error(ctx, BLOK_ERR_INVALID_ARG, "model_lights_clear: unknown model " + std::to_string(model));
    BLOK_HIP_TRY(ctx, hipSetDevice(ctx->device));
    return drop_model_lights(ctx, model);
}

int blok_hip_instance_lights_info(blok_hip_ctx* ctx, const blok_instance* instances_host, uint32_t n, blok_instance_lights_info* out,
                                  uint32_t* out_icum_host) {
    if (!ctx) return BLOK_ERR_INVALID_ARG;
    if (n && !instances_host) return set_error(ctx, BLOK_ERR_INVALID_ARG, "null instance table with non-zero count");
    if (!out) return set_error(ctx, BLOK_ERR_INVALID_ARG, "instance_lights_info: null output");
    BLOK_HIP_TRY(ctx, hipSetDevice(ctx->device));
    StagedBlock d;
    const auto inst = d.input(instances_host, n);
    const auto icum = d.output(out_icum_host, static_cast<size_t>(n) + 1u);
    const auto header = d.output(out, 1);
    int rc = d.stage(ctx, "instance_lights_info");
    if (rc != BLOK_OK) return rc;
    const auto& M = ctx->models;
    blok::launch_instance_lights_prefix(d.at(inst), n, M.d_desc, M.d_lights, std::min<uint32_t>(static_cast<uint32_t>(M.desc.size()), M.n_lights_uploaded),
                                        ctx->lights.n_faces, ctx->world_voxel_size, d.at(icum), d.at(header), nullptr);
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) rc = set_error(ctx, BLOK_ERR_HIP, std::string("instance_lights_info: ") + hipGetErrorString(e));
    return d.collect(ctx, "instance_lights_info", rc);
}

int blok_hip_model_set_scale(blok_hip_ctx* ctx, uint32_t model, uint32_t scale_log2) {
    if (!ctx) return BLOK_ERR_INVALID_ARG;
    if (!known_model(ctx, model)) return set_error(ctx, BLOK_ERR_INVALID_ARG, "unknown model " + std::to_string(model));
    if (scale_log2 > blok::kMaxScaleLog2)
        return set_error(ctx, BLOK_ERR_INVALID_ARG, "model_set_scale: scale_log2 above " + std::to_string(blok::kMaxScaleLog2));
    BLOK_HIP_TRY(ctx, hipSetDevice(ctx->device));
    BLOK_HIP_TRY(ctx, hipDeviceSynchronize());           // frames in flight read the descriptor the upload replaces
    blok::ModelDesc& d = ctx->models.desc[model];
    const blok::ModelDesc before = d;
    const auto& own = ctx->models.own[model];
    d.scale_log2 = scale_log2;
    for (int a = 0; a < 3; ++a) { d.lo[a] = own.box_lo[a] * (1 << scale_log2); d.hi[a] = own.box_hi[a] * (1 << scale_log2); }      // (|box| <= 2^22: add_model)
    const int rc = upload_models(ctx);
    if (rc != BLOK_OK) { d = before; return rc; }
    // the object-motion maps (instance_motion.h, pose_motion.h) do not hold across a change of scale: the next frame's instances and poses
    // are untracked
    ctx->post.rt_prev_n = 0u;
    ctx->post.rt_prev_n_poses = 0u;
    return BLOK_OK;
}

int blok_hip_model_scale(blok_hip_ctx* ctx, uint32_t model, uint32_t* out_scale_log2) {
    if (!ctx) return BLOK_ERR_INVALID_ARG;
    if (!known_model(ctx, model)) return set_error(ctx, BLOK_ERR_INVALID_ARG, "unknown model " + std::to_string(model));
    if (!out_scale_log2) return set_error(ctx, BLOK_ERR_INVALID_ARG, "model_scale: null output");
    *out_scale_log2 = ctx->models.desc[model].scale_log2;
    return BLOK_OK;
}

int blok_hip_check_instances(blok_hip_ctx* ctx, const blok_instance* instances_host, uint32_t n_instances) {
    if (!ctx) return BLOK_ERR_INVALID_ARG;
    return check_table(ctx, instances_host, n_instances);
}

int blok_hip_trace_primary_instanced_device(blok_hip_ctx* ctx, const blok_camera* cam, uint32_t x0, uint32_t y0, uint32_t w, uint32_t h,
                                            const blok_instance* instances_dev, uint32_t n_instances,
                                            void* out_hits_dev, void* out_rgba_dev, uint32_t* out_instance_dev, void* hip_stream) {
    int rc = check_frame(ctx, cam, x0, y0, w, h, out_hits_dev || out_rgba_dev || out_instance_dev, instances_dev, n_instances, nullptr, 0u);
    if (rc != BLOK_OK) return rc;
    hipStream_t stream = static_cast<hipStream_t>(hip_stream);
    blok::InstanceArgs P{};
    P.hits = static_cast<blok_hit*>(out_hits_dev);
    if (n_instances) {                                   // (the instance pass needs the world records)
        rc = frame_pass(ctx, cam, x0, y0, w, h, stream, ctx->beam_buffers[stream].inst_bins, out_hits_dev, out_rgba_dev, out_instance_dev, P);
        if (rc != BLOK_OK) return rc;
    }
    // the world pass: blok_hip_trace_primary_device's launch, unchanged
    if (P.hits || out_rgba_dev) {
        rc = blok_hip_trace_primary_device(ctx, cam, x0, y0, w, h, P.hits, out_rgba_dev, hip_stream);
        if (rc != BLOK_OK) return rc;
    }
    if (!n_instances) {
        if (out_instance_dev) BLOK_HIP_TRY(ctx, hipMemsetAsync(out_instance_dev, 0xFF, static_cast<size_t>(w) * h * sizeof(uint32_t), stream));
        return BLOK_OK;
    }
    P.instances = instances_dev; P.n_instances = n_instances;
    blok::launch_instance_bins(P, stream);
    BLOK_HIP_TRY(ctx, hipGetLastError());
    blok::launch_instance_pass(P, stream);
    BLOK_HIP_TRY(ctx, hipGetLastError());
    return BLOK_OK;
}

int blok_hip_trace_primary_instanced(blok_hip_ctx* ctx, const blok_camera* cam, uint32_t x0, uint32_t y0, uint32_t w, uint32_t h,
                                     const blok_instance* instances_host, uint32_t n_instances,
                                     blok_hit* out_hits_host, uint32_t* out_rgba_host, uint32_t* out_instance_host) {
    return trace_primary_placed(ctx, "trace_primary_instanced", cam, x0, y0, w, h, instances_host, n_instances, nullptr, 0u, out_hits_host, out_rgba_host,
                                out_instance_host);
}

int blok_hip_trace_rays_instanced_device(blok_hip_ctx* ctx, const blok_ray* rays_dev, size_t n, const blok_instance* instances_dev,
                                         uint32_t n_instances, blok_hit* out_hits_dev, uint32_t* out_instance_dev, void* hip_stream) {
    int rc = check_rays(ctx, rays_dev, n, out_hits_dev || out_instance_dev);
    if (rc != BLOK_OK || n == 0) return rc;
    rc = check_device_tables(ctx, instances_dev, n_instances, nullptr, 0u);
    if (rc != BLOK_OK) return rc;
    BLOK_HIP_TRY(ctx, hipSetDevice(ctx->device));
    hipStream_t stream = static_cast<hipStream_t>(hip_stream);
    if (!n_instances && !out_hits_dev) {
        BLOK_HIP_TRY(ctx, hipMemsetAsync(out_instance_dev, 0xFF, n * sizeof(uint32_t), stream));
        return BLOK_OK;
    }
    blok::InstanceArgs P{};
    rc = rays_pass(ctx, rays_dev, n, stream, out_hits_dev, out_instance_dev, P);
    if (rc != BLOK_OK) return rc;
    blok::TraceArgs world = P.world;
    world.out = P.hits;
    rc = launch_timed(ctx, blok::RayMode::Rays, world, static_cast<uint32_t>((n + blok::kBlock - 1) / blok::kBlock), stream);
    if (rc != BLOK_OK) return rc;
    if (!n_instances) {
        if (out_instance_dev) BLOK_HIP_TRY(ctx, hipMemsetAsync(out_instance_dev, 0xFF, n * sizeof(uint32_t), stream));
        return BLOK_OK;
    }
    P.instances = instances_dev; P.n_instances = n_instances;
    blok::launch_instance_rays(P, stream);
    BLOK_HIP_TRY(ctx, hipGetLastError());
    return BLOK_OK;
}

int blok_hip_trace_rays_instanced(blok_hip_ctx* ctx, const blok_ray* rays_host, size_t n, const blok_instance* instances_host,
                                  uint32_t n_instances, blok_hit* out_hits_host, uint32_t* out_instance_host) {
    return trace_rays_placed(ctx, "trace_rays_instanced", rays_host, n, instances_host, n_instances, nullptr, 0u, out_hits_host, out_instance_host);
}

// ---- posed models (posed_core.h): the instanced entries, then the pose pass on the same stream ---------------------------------------------
int blok_hip_check_poses(blok_hip_ctx* ctx, const blok_pose* poses_host, uint32_t n_poses) {
    if (!ctx) return BLOK_ERR_INVALID_ARG;
    return check_pose_table(ctx, poses_host, n_poses);
}

int blok_hip_trace_primary_posed_device(blok_hip_ctx* ctx, const blok_camera* cam, uint32_t x0, uint32_t y0, uint32_t w, uint32_t h,
                                        const blok_instance* instances_dev, uint32_t n_instances, const blok_pose* poses_dev, uint32_t n_poses,
                                        void* out_hits_dev, void* out_rgba_dev, uint32_t* out_instance_dev, void* hip_stream) {
    int rc = check_frame(ctx, cam, x0, y0, w, h, out_hits_dev || out_rgba_dev || out_instance_dev, instances_dev, n_instances, poses_dev, n_poses);
    if (rc != BLOK_OK) return rc;
    if (!n_poses)                                        // the instanced entry itself: the same launches, the same bytes
        return blok_hip_trace_primary_instanced_device(ctx, cam, x0, y0, w, h, instances_dev, n_instances, out_hits_dev, out_rgba_dev, out_instance_dev, hip_stream);
    hipStream_t stream = static_cast<hipStream_t>(hip_stream);
    blok::PosedArgs Q{};                                 // (the pose pass needs the composed records)
    rc = frame_pass(ctx, cam, x0, y0, w, h, stream, ctx->beam_buffers[stream].pose_bins, out_hits_dev, out_rgba_dev, out_instance_dev, Q.frame);
    if (rc != BLOK_OK) return rc;
    rc = blok_hip_trace_primary_instanced_device(ctx, cam, x0, y0, w, h, instances_dev, n_instances, Q.frame.hits, out_rgba_dev, out_instance_dev, hip_stream);
    if (rc != BLOK_OK) return rc;
    Q.poses = poses_dev; Q.n_poses = n_poses;
    blok::launch_posed_bins(Q, stream);
    BLOK_HIP_TRY(ctx, hipGetLastError());
    blok::launch_posed_pass(Q, stream);
    BLOK_HIP_TRY(ctx, hipGetLastError());
    return BLOK_OK;
}

int blok_hip_trace_primary_posed(blok_hip_ctx* ctx, const blok_camera* cam, uint32_t x0, uint32_t y0, uint32_t w, uint32_t h,
                                 const blok_instance* instances_host, uint32_t n_instances, const blok_pose* poses_host, uint32_t n_poses,
                                 blok_hit* out_hits_host, uint32_t* out_rgba_host, uint32_t* out_instance_host) {
    return trace_primary_placed(ctx, "trace_primary_posed", cam, x0, y0, w, h, instances_host, n_instances, poses_host, n_poses, out_hits_host,
                                out_rgba_host, out_instance_host);
}

int blok_hip_trace_rays_posed_device(blok_hip_ctx* ctx, const blok_ray* rays_dev, size_t n, const blok_instance* instances_dev, uint32_t n_instances,
                                     const blok_pose* poses_dev, uint32_t n_poses, blok_hit* out_hits_dev, uint32_t* out_instance_dev,
                                     void* hip_stream) {
    int rc = check_rays(ctx, rays_dev, n, out_hits_dev || out_instance_dev);
    if (rc != BLOK_OK || n == 0) return rc;
    rc = check_device_tables(ctx, instances_dev, n_instances, poses_dev, n_poses);
    if (rc != BLOK_OK) return rc;
    if (!n_poses) return blok_hip_trace_rays_instanced_device(ctx, rays_dev, n, instances_dev, n_instances, out_hits_dev, out_instance_dev, hip_stream);
    BLOK_HIP_TRY(ctx, hipSetDevice(ctx->device));
    hipStream_t stream = static_cast<hipStream_t>(hip_stream);
    blok::PosedArgs Q{};
    rc = rays_pass(ctx, rays_dev, n, stream, out_hits_dev, out_instance_dev, Q.frame);
    if (rc != BLOK_OK) return rc;
    rc = blok_hip_trace_rays_instanced_device(ctx, rays_dev, n, instances_dev, n_instances, Q.frame.hits, out_instance_dev, hip_stream);
    if (rc != BLOK_OK) return rc;
    Q.poses = poses_dev; Q.n_poses = n_poses;
    blok::launch_posed_rays(Q, stream);
    BLOK_HIP_TRY(ctx, hipGetLastError());
    return BLOK_OK;
}

int blok_hip_trace_rays_posed(blok_hip_ctx* ctx, const blok_ray* rays_host, size_t n, const blok_instance* instances_host, uint32_t n_instances,
                              const blok_pose* poses_host, uint32_t n_poses, blok_hit* out_hits_host, uint32_t* out_instance_host) {
    return trace_rays_placed(ctx, "trace_rays_posed", rays_host, n, instances_host, n_instances, poses_host, n_poses, out_hits_host, out_instance_host);
}

// ---- path-traced frames with instances (tlas_core.h) ----------------------------------------------------------------------------

int blok_hip_trace_paths_instanced_device(blok_hip_ctx* ctx, const blok_camera* cam, uint32_t x0, uint32_t y0, uint32_t w, uint32_t h,
                                          uint32_t spp, uint32_t max_bounces, uint32_t frame_index, const blok_instance* instances_dev,
                                          uint32_t n_instances, const blok_gbuffer* planes_dev, uint32_t* out_instance_dev, void* hip_stream) {
    if (!ctx) return BLOK_ERR_INVALID_ARG;
    if (!planes_dev) return set_error(ctx, BLOK_ERR_INVALID_ARG, "bad path-trace arguments");
    if (n_instances && !instances_dev) return set_error(ctx, BLOK_ERR_INVALID_ARG, "null instance table with non-zero count");
    blok::PathArgs p{};
    p.color = planes_dev->color; p.world_pos = planes_dev->world_pos;
    p.normal_roughness = planes_dev->normal_roughness; p.albedo_metallic = planes_dev->albedo_metallic;
    const PathInstances inst{instances_dev, n_instances, out_instance_dev};
    return launch_path_frame(ctx, cam, x0, y0, w, h, spp, max_bounces, frame_index, p, hip_stream, &inst);
}

int blok_hip_trace_paths_instanced_ref_device(blok_hip_ctx* ctx, const blok_camera* cam, uint32_t x0, uint32_t y0, uint32_t w, uint32_t h,
                                              uint32_t spp, uint32_t max_bounces, uint32_t frame_index, const blok_instance* instances_dev,
                                              uint32_t n_instances, const float prev_view_proj[16], const blok_gbuffer_ref* planes_dev,
                                              uint32_t* out_instance_dev, void* hip_stream) {
    if (!ctx) return BLOK_ERR_INVALID_ARG;
    if (!planes_dev || (planes_dev->motion && !prev_view_proj))
        return set_error(ctx, BLOK_ERR_INVALID_ARG, "bad path-trace arguments (a motion plane needs prevViewProj)");
    if (n_instances && !instances_dev) return set_error(ctx, BLOK_ERR_INVALID_ARG, "null instance table with non-zero count");
    blok::PathArgs p{};
    p.color = planes_dev->color; p.world_pos = planes_dev->world_pos;
    p.normal_roughness_h = planes_dev->normal_roughness; p.albedo_metallic_u8 = planes_dev->albedo_metallic; p.motion_h = planes_dev->motion;
    if (prev_view_proj) for (int k = 0; k < 16; ++k) p.prev_view_proj[k] = prev_view_proj[k];
    const PathInstances inst{instances_dev, n_instances, out_instance_dev};
    return launch_path_frame(ctx, cam, x0, y0, w, h, spp, max_bounces, frame_index, p, hip_stream, &inst);
}

int blok_hip_trace_paths_instanced(blok_hip_ctx* ctx, const blok_camera* cam, uint32_t x0, uint32_t y0, uint32_t w, uint32_t h, uint32_t spp,
                                   uint32_t max_bounces, uint32_t frame_index, const blok_instance* instances_host, uint32_t n_instances,
                                   const blok_gbuffer* planes_host, uint32_t* out_instance_host) {
    if (!ctx) return BLOK_ERR_INVALID_ARG;
    if (!planes_host) return set_error(ctx, BLOK_ERR_INVALID_ARG, "null planes");
    int rc = check_trace(ctx, cam);
    if (rc != BLOK_OK) return rc;
    if (!rect_inside(ctx, x0, y0, w, h)) return set_error(ctx, BLOK_ERR_INVALID_ARG, "rectangle outside the frame");
    rc = check_table(ctx, instances_host, n_instances);
    if (rc != BLOK_OK) return rc;
    const size_t n = static_cast<size_t>(w) * h;
    float* const host[4] = {planes_host->color, planes_host->world_pos, planes_host->normal_roughness, planes_host->albedo_metallic};
    StagedBlock d;
    const auto inst = d.input(instances_host, n_instances);
    StagedBlock::Seg<float> plane[4];
    for (int i = 0; i < 4; ++i) plane[i] = d.output(host[i], n * 4);
    const auto ids = d.output(out_instance_host, n);
    rc = d.stage(ctx, "trace_paths_instanced");
    if (rc != BLOK_OK) return rc;
    const blok_gbuffer planes_dev{d.wanted(plane[0]), d.wanted(plane[1]), d.wanted(plane[2]), d.wanted(plane[3])};
    rc = blok_hip_trace_paths_instanced_device(ctx, cam, x0, y0, w, h, spp, max_bounces, frame_index, d.at(inst), n_instances, &planes_dev, d.wanted(ids),
                                               nullptr);
    return d.collect(ctx, "trace_paths_instanced", rc);
}

// ---- path-traced frames with poses (posed_paths_core.h): the instanced entries with a pose table behind the instances --------------------

int blok_hip_trace_paths_posed_device(blok_hip_ctx* ctx, const blok_camera* cam, uint32_t x0, uint32_t y0, uint32_t w, uint32_t h, uint32_t spp,
                                      uint32_t max_bounces, uint32_t frame_index, const blok_instance* instances_dev, uint32_t n_instances,
                                      const blok_pose* poses_dev, uint32_t n_poses, const blok_gbuffer* planes_dev, uint32_t* out_instance_dev,
                                      void* hip_stream) {
    if (!ctx) return BLOK_ERR_INVALID_ARG;
    if (!planes_dev) return set_error(ctx, BLOK_ERR_INVALID_ARG, "bad path-trace arguments");
    const int rc = check_device_tables(ctx, instances_dev, n_instances, poses_dev, n_poses);
    if (rc != BLOK_OK) return rc;
    if (!n_poses)                                        // the instanced entry itself: the same launches, the same bytes
        return blok_hip_trace_paths_instanced_device(ctx, cam, x0, y0, w, h, spp, max_bounces, frame_index, instances_dev, n_instances, planes_dev,
                                                     out_instance_dev, hip_stream);
    blok::PathArgs p{};
    p.color = planes_dev->color; p.world_pos = planes_dev->world_pos;
    p.normal_roughness = planes_dev->normal_roughness; p.albedo_metallic = planes_dev->albedo_metallic;
    const PathInstances inst{instances_dev, n_instances, out_instance_dev};
    const PathPoses poses{poses_dev, n_poses};
    return launch_path_frame(ctx, cam, x0, y0, w, h, spp, max_bounces, frame_index, p, hip_stream, &inst, &poses);
}

int blok_hip_trace_paths_posed_ref_device(blok_hip_ctx* ctx, const blok_camera* cam, uint32_t x0, uint32_t y0, uint32_t w, uint32_t h, uint32_t spp,
                                          uint32_t max_bounces, uint32_t frame_index, const blok_instance* instances_dev, uint32_t n_instances,
                                          const blok_pose* poses_dev, uint32_t n_poses, const float prev_view_proj[16],
                                          const blok_gbuffer_ref* planes_dev, uint32_t* out_instance_dev, void* hip_stream) {
    if (!ctx) return BLOK_ERR_INVALID_ARG;
    if (!planes_dev || (planes_dev->motion && !prev_view_proj))
        return set_error(ctx, BLOK_ERR_INVALID_ARG, "bad path-trace arguments (a motion plane needs prevViewProj)");
    const int rc = check_device_tables(ctx, instances_dev, n_instances, poses_dev, n_poses);
    if (rc != BLOK_OK) return rc;
    if (!n_poses)
        return blok_hip_trace_paths_instanced_ref_device(ctx, cam, x0, y0, w, h, spp, max_bounces, frame_index, instances_dev, n_instances, prev_view_proj,
                                                         planes_dev, out_instance_dev, hip_stream);
    blok::PathArgs p{};
    p.color = planes_dev->color; p.world_pos = planes_dev->world_pos;
    p.normal_roughness_h = planes_dev->normal_roughness; p.albedo_metallic_u8 = planes_dev->albedo_metallic; p.motion_h = planes_dev->motion;
    if (prev_view_proj) for (int k = 0; k < 16; ++k) p.prev_view_proj[k] = prev_view_proj[k];
    const PathInstances inst{instances_dev, n_instances, out_instance_dev};
    const PathPoses poses{poses_dev, n_poses};
    return launch_path_frame(ctx, cam, x0, y0, w, h, spp, max_bounces, frame_index, p, hip_stream, &inst, &poses);
}

int blok_hip_trace_paths_posed(blok_hip_ctx* ctx, const blok_camera* cam, uint32_t x0, uint32_t y0, uint32_t w, uint32_t h, uint32_t spp,
                               uint32_t max_bounces, uint32_t frame_index, const blok_instance* instances_host, uint32_t n_instances,
                               const blok_pose* poses_host, uint32_t n_poses, const blok_gbuffer* planes_host, uint32_t* out_instance_host) {
    if (!ctx) return BLOK_ERR_INVALID_ARG;
    if (!planes_host) return set_error(ctx, BLOK_ERR_INVALID_ARG, "null planes");
    int rc = check_trace(ctx, cam);
    if (rc != BLOK_OK) return rc;
    if (!rect_inside(ctx, x0, y0, w, h)) return set_error(ctx, BLOK_ERR_INVALID_ARG, "rectangle outside the frame");
    rc = check_table(ctx, instances_host, n_instances);
    if (rc == BLOK_OK) rc = check_pose_table(ctx, poses_host, n_poses);
    if (rc != BLOK_OK) return rc;
    const size_t n = static_cast<size_t>(w) * h;
    float* const host[4] = {planes_host->color, planes_host->world_pos, planes_host->normal_roughness, planes_host->albedo_metallic};
    StagedBlock d;
    const auto inst = d.input(instances_host, n_instances);
    const auto poses = d.input(poses_host, n_poses);
    StagedBlock::Seg<float> plane[4];
    for (int i = 0; i < 4; ++i) plane[i] = d.output(host[i], n * 4);
    const auto ids = d.output(out_instance_host, n);
    rc = d.stage(ctx, "trace_paths_posed");
    if (rc != BLOK_OK) return rc;
    const blok_gbuffer planes_dev{d.wanted(plane[0]), d.wanted(plane[1]), d.wanted(plane[2]), d.wanted(plane[3])};
    rc = blok_hip_trace_paths_posed_device(ctx, cam, x0, y0, w, h, spp, max_bounces, frame_index, d.at(inst), n_instances, d.at(poses), n_poses,
                                           &planes_dev, d.wanted(ids), nullptr);
    return d.collect(ctx, "trace_paths_posed", rc);
}

// ---- object motion of moving instances (instance_motion.h) -----------------------------------------------------------------------

int blok_hip_instance_motion_device(blok_hip_ctx* ctx, uint32_t x0, uint32_t y0, uint32_t w, uint32_t h, const float* world_pos_dev,
                                    const uint32_t* instance_ids_dev, const blok_instance* cur_dev, uint32_t n_cur, const blok_instance* prev_dev,
                                    uint32_t n_prev, const float prev_view_proj[16], uint16_t* motion_h_dev, float* motion_dev, void* hip_stream) {
    if (!ctx) return BLOK_ERR_INVALID_ARG;
    if (!world_pos_dev || !instance_ids_dev) return set_error(ctx, BLOK_ERR_INVALID_ARG, "instance motion: world position and id planes are required");
    if ((n_cur && !cur_dev) || (n_prev && !prev_dev)) return set_error(ctx, BLOK_ERR_INVALID_ARG, "null instance table with non-zero count");
    if (!motion_h_dev && !motion_dev) return set_error(ctx, BLOK_ERR_INVALID_ARG, "instance motion: no motion output");
    if (!rect_inside(ctx, x0, y0, w, h)) return set_error(ctx, BLOK_ERR_INVALID_ARG, "rectangle outside the frame");
    if (!prev_view_proj) return set_error(ctx, BLOK_ERR_INVALID_ARG, "instance motion: prevViewProj is required");
    BLOK_HIP_TRY(ctx, hipSetDevice(ctx->device));
    if (!n_cur || !n_prev) return BLOK_OK;                       // nothing is tracked
    blok::InstanceMotionArgs a{};
    a.m = motion_tables(ctx, instance_ids_dev, cur_dev, n_cur, prev_dev, n_prev);
    a.world_pos = world_pos_dev;
    a.x0 = x0; a.y0 = y0; a.w = w; a.h = h; a.frame_w = ctx->width; a.frame_h = ctx->height;
    for (int k = 0; k < 16; ++k) a.prev_view_proj[k] = prev_view_proj[k];
    a.motion_h = motion_h_dev; a.motion = motion_dev;
    blok::launch_instance_motion(a, static_cast<hipStream_t>(hip_stream));
    BLOK_HIP_TRY(ctx, hipGetLastError());
    return BLOK_OK;
}

// ---- object motion of moving poses (pose_motion.h) ---------------------------------------------------------------------------------

int blok_hip_posed_motion_device(blok_hip_ctx* ctx, uint32_t x0, uint32_t y0, uint32_t w, uint32_t h, const float* world_pos_dev,
                                 const uint32_t* ids_dev, const blok_instance* cur_dev, uint32_t n_cur, const blok_instance* prev_dev, uint32_t n_prev,
                                 const blok_pose* cur_poses_dev, uint32_t n_cur_poses, const blok_pose* prev_poses_dev, uint32_t n_prev_poses,
                                 const float prev_view_proj[16], uint16_t* motion_h_dev, float* motion_dev, void* hip_stream) {
    if (!ctx) return BLOK_ERR_INVALID_ARG;
    if (!world_pos_dev || !ids_dev) return set_error(ctx, BLOK_ERR_INVALID_ARG, "instance motion: world position and id planes are required");
    if ((n_cur && !cur_dev) || (n_prev && !prev_dev)) return set_error(ctx, BLOK_ERR_INVALID_ARG, "null instance table with non-zero count");
    int rc = check_device_tables(ctx, nullptr, 0u, cur_poses_dev, n_cur_poses);
    if (rc == BLOK_OK) rc = check_device_tables(ctx, nullptr, 0u, prev_poses_dev, n_prev_poses);
    if (rc != BLOK_OK) return rc;
    if (!motion_h_dev && !motion_dev) return set_error(ctx, BLOK_ERR_INVALID_ARG, "instance motion: no motion output");
    if (!rect_inside(ctx, x0, y0, w, h)) return set_error(ctx, BLOK_ERR_INVALID_ARG, "rectangle outside the frame");
    if (!prev_view_proj) return set_error(ctx, BLOK_ERR_INVALID_ARG, "instance motion: prevViewProj is required");
    BLOK_HIP_TRY(ctx, hipSetDevice(ctx->device));
    if ((!n_cur || !n_prev) && (!n_cur_poses || !n_prev_poses)) return BLOK_OK;          // nothing is tracked
    hipStream_t stream = static_cast<hipStream_t>(hip_stream);
    const blok_pose_motion* records = nullptr;
    rc = prepare_pose_motion(ctx, cur_poses_dev, n_cur_poses, prev_poses_dev, n_prev_poses, stream, &records);
    if (rc != BLOK_OK) return rc;
    return posed_motion_pass(ctx, x0, y0, w, h, world_pos_dev, pose_motion_tables(ctx, ids_dev, cur_dev, n_cur, prev_dev, n_prev, records, n_cur_poses),
                             prev_view_proj, motion_h_dev, motion_dev, stream);
}

int blok_hip_debug_pose_motion_records(blok_hip_ctx* ctx, const blok_pose* cur_host, uint32_t n_cur, const blok_pose* prev_host, uint32_t n_prev,
                                       blok_pose_motion* out_records_host) {
    if (!ctx) return BLOK_ERR_INVALID_ARG;
    if ((n_cur && !cur_host) || (n_prev && !prev_host)) return set_error(ctx, BLOK_ERR_INVALID_ARG, "null pose table with non-zero count");
    if (n_cur >= BLOK_POSE_ID || n_prev >= BLOK_POSE_ID) return set_error(ctx, BLOK_ERR_INVALID_ARG, "more than 2^31 - 1 poses");
    if (n_cur && !out_records_host) return set_error(ctx, BLOK_ERR_INVALID_ARG, "pose_motion_records: null output");
    if (!n_cur) return BLOK_OK;
    BLOK_HIP_TRY(ctx, hipSetDevice(ctx->device));
    StagedBlock d;
    const auto cur = d.input(cur_host, n_cur);
    const auto prev = d.input(prev_host, n_prev);
    const auto out = d.output(out_records_host, n_cur);
    int rc = d.stage(ctx, "pose_motion_records");
    if (rc != BLOK_OK) return rc;
    blok::launch_pose_motion_prepare(d.at(cur), n_cur, d.at(prev), n_prev, ctx->models.d_desc,
                                     ctx->models.d_desc ? static_cast<uint32_t>(ctx->models.desc.size()) : 0u, d.at(out), nullptr);
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) rc = set_error(ctx, BLOK_ERR_HIP, std::string("pose_motion_records: ") + hipGetErrorString(e));
    return d.collect(ctx, "pose_motion_records", rc);
}

int blok_hip_debug_build_tlas(blok_hip_ctx* ctx, const blok_instance* instances_dev, uint32_t n_instances, void* out_nodes_host, size_t capacity,
                              uint32_t* out_count) {
    if (!ctx) return BLOK_ERR_INVALID_ARG;
    if (!n_instances || n_instances > blok::kTlasMax || !instances_dev || !out_nodes_host)
        return set_error(ctx, BLOK_ERR_INVALID_ARG, "the tree needs 1 .. kTlasMax instances and an output");
    const uint32_t count = blok::tlas_nodes(n_instances);
    if (out_count) *out_count = count;
    if (capacity < count) return set_error(ctx, BLOK_ERR_INVALID_ARG, "output too small for " + std::to_string(count) + " nodes");
    BLOK_HIP_TRY(ctx, hipSetDevice(ctx->device));
    blok::DeviceArray<blok::TlasNode> d;
    BLOK_HIP_TRY(ctx, d.reserve(count, blok::FreeAfter::nothing()));
    blok::launch_tlas_build(instances_dev, n_instances, ctx->models.d_desc, static_cast<uint32_t>(ctx->models.desc.size()), d, nullptr);
    hipError_t e = hipGetLastError();
    if (e == hipSuccess) e = hipMemcpy(out_nodes_host, d, count * sizeof(blok::TlasNode), hipMemcpyDeviceToHost);
    if (e != hipSuccess) return set_error(ctx, BLOK_ERR_HIP, std::string("build_tlas: ") + hipGetErrorString(e));
    return BLOK_OK;
}

int blok_hip_debug_build_pose_tlas(blok_hip_ctx* ctx, const blok_camera* cam, const blok_pose* poses_dev, uint32_t n_poses, void* out_nodes_host,
                                   size_t capacity, uint32_t* out_count) {
    if (!ctx) return BLOK_ERR_INVALID_ARG;
    if (!cam || !n_poses || n_poses > blok::kTlasMax || !poses_dev || !out_nodes_host)
        return set_error(ctx, BLOK_ERR_INVALID_ARG, "the pose tree needs a camera, 1 .. kTlasMax poses and an output");
    const uint32_t count = blok::tlas_nodes(n_poses);
    if (out_count) *out_count = count;
    if (capacity < count) return set_error(ctx, BLOK_ERR_INVALID_ARG, "output too small for " + std::to_string(count) + " nodes");
    BLOK_HIP_TRY(ctx, hipSetDevice(ctx->device));
    blok::DeviceArray<blok::TlasNode> d;
    BLOK_HIP_TRY(ctx, d.reserve(count, blok::FreeAfter::nothing()));
    blok::launch_pose_tlas_build(poses_dev, n_poses, ctx->models.d_desc, static_cast<uint32_t>(ctx->models.desc.size()), ctx->world_voxel_size, cam->pos, d,
                                 nullptr);
    hipError_t e = hipGetLastError();
    if (e == hipSuccess) e = hipMemcpy(out_nodes_host, d, count * sizeof(blok::TlasNode), hipMemcpyDeviceToHost);
    if (e != hipSuccess) return set_error(ctx, BLOK_ERR_HIP, std::string("build_pose_tlas: ") + hipGetErrorString(e));
    return BLOK_OK;
}

}  // extern "C"
