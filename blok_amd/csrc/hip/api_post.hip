// C ABI, image-space chain: denoiser, TAA, sharpen, the one-call ray-tracing frame (include/blok_hip.h; kernels in post_core.h).
#include "api_internal.h"
#include "../common/taa_jitter.h"

using namespace blok_api;

namespace {
// A plane of the chain, `count` elements, zeroed with a blocking fill (the planes are fresh: ensure_post and draw_frame_rt start from a
// reset `post`, and a failure resets it again).
template <class T> int zeroed_plane(blok_hip_ctx* ctx, blok::DeviceArray<T>* plane, size_t count) {
    BLOK_HIP_TRY(ctx, plane->reserve(count, blok::FreeAfter::nothing()));
    BLOK_HIP_TRY(ctx, hipMemset(plane->get(), 0, count * sizeof(T)));
    return BLOK_OK;
}
}  // namespace

extern "C" {

// ---- image-space chain ------------------------------------------------------------------------------------------------
namespace {
int ensure_post(blok_hip_ctx* ctx) {
    const size_t n = static_cast<size_t>(ctx->width) * ctx->height;
    auto& P = ctx->post;
    if (P.pixels == n && P.width == ctx->width && P.height == ctx->height) return BLOK_OK;     // same shape: history stays valid
    P = blok_hip_ctx::Post{};       // any resize — also one that keeps the pixel count (320x200 -> 200x320) — drops the history planes
    int rc = BLOK_OK;
    for (int k = 0; k < 2 && rc == BLOK_OK; ++k) {
        rc = zeroed_plane(ctx, &P.hist_color[k], 4 * n);
        if (rc == BLOK_OK) rc = zeroed_plane(ctx, &P.moments[k], 2 * n);
        if (rc == BLOK_OK) rc = zeroed_plane(ctx, &P.world_pos[k], 4 * n);
        if (rc == BLOK_OK) rc = zeroed_plane(ctx, &P.hist_len[k], n);
        if (rc == BLOK_OK) rc = zeroed_plane(ctx, &P.unit_normals[k], 4 * n);
        if (rc == BLOK_OK) rc = zeroed_plane(ctx, &P.taa_hist[k], 4 * n);
    }
    if (rc == BLOK_OK) rc = zeroed_plane(ctx, &P.motion, 2 * n);
    if (rc == BLOK_OK) rc = zeroed_plane(ctx, &P.variance, n);
    if (rc == BLOK_OK) rc = zeroed_plane(ctx, &P.ping, 4 * n);
    if (rc == BLOK_OK) rc = zeroed_plane(ctx, &P.pong, 4 * n);
    if (rc == BLOK_OK) rc = zeroed_plane(ctx, &P.widen, 2 * n);
    if (rc != BLOK_OK) { P = blok_hip_ctx::Post{}; return rc; }
    P.pixels = n; P.width = ctx->width; P.height = ctx->height;
    return BLOK_OK;
}
blok::DenoiseSettings to_settings(const blok_denoise_settings& s) {
    blok::DenoiseSettings d;
    d.temporal_alpha = s.temporal_alpha; d.moment_alpha = s.moment_alpha; d.variance_clip_gamma = s.variance_clip_gamma;
    d.depth_threshold = s.depth_threshold; d.normal_threshold = s.normal_threshold;
    d.phi_color = s.phi_color; d.phi_normal = s.phi_normal; d.phi_depth = s.phi_depth;
    d.atrous_iterations = s.atrous_iterations; d.variance_boost = s.variance_boost; d.min_history_length = s.min_history_length;
    return d;
}
}  // namespace

void blok_denoise_settings_default(blok_denoise_settings* s) {       // renderer_denoising.hpp:49-66
    if (!s) return;
    s->temporal_alpha = 0.05f; s->moment_alpha = 0.2f; s->variance_clip_gamma = 1.5f;
    s->depth_threshold = 0.1f; s->normal_threshold = 0.95f;
    s->phi_color = 0.5f; s->phi_normal = 128.0f; s->phi_depth = 0.1f;
    s->atrous_iterations = 4; s->variance_boost = 1.5f; s->min_history_length = 4;
}

// One frame through temporal accumulation, variance and the a-trous iterations; the frame's planes come in `in` (float4 planes,
// or the reference-format halves of normal + roughness / motion).  inst: the id plane and tables of a frame with instances (the
// instanced temporal pass), or null.  posed: the same with the poses' records (the posed temporal pass), or null; never both.
static int denoise_frame(blok_hip_ctx* ctx, const blok::TemporalArgs& in, const float prev_view_proj[16], uint32_t frame_count,
                         const blok_denoise_settings* settings, float* out_color_dev, void* hip_stream, const blok::MotionTables* inst = nullptr,
                         const blok::PoseMotionTables* posed = nullptr) {
    if (!in.color || !in.world_pos || (!in.normal_roughness && !in.normal_roughness_h) || !prev_view_proj || !out_color_dev)
        return set_error(ctx, BLOK_ERR_INVALID_ARG, "denoise: colour, world position and normal planes, prevViewProj and an output are required");
    blok_denoise_settings def;
    blok_denoise_settings_default(&def);
    const blok_denoise_settings& S = settings ? *settings : def;
    if (S.atrous_iterations < 0 || S.atrous_iterations > 5) return set_error(ctx, BLOK_ERR_INVALID_ARG, "denoise: 0..5 a-trous iterations");
    BLOK_HIP_TRY(ctx, hipSetDevice(ctx->device));
    int rc = ensure_post(ctx);
    if (rc != BLOK_OK) return rc;
    auto& P = ctx->post;
    hipStream_t stream = static_cast<hipStream_t>(hip_stream);
    const int cur = P.cur, prev = cur ^ 1;
    blok::PostFrame f{};
    f.w = ctx->width; f.h = ctx->height; f.frame_count = frame_count; f.s = to_settings(S);
    for (int k = 0; k < 16; ++k) f.prev_view_proj[k] = prev_view_proj[k];

    blok::TemporalArgs t = in;
    t.f = f;

    t.prev_color = P.hist_color[prev]; t.prev_moments = P.moments[prev]; t.prev_world_pos = P.world_pos[prev];
    t.prev_hist_len = P.hist_len[prev]; t.prev_unit_normals = P.unit_normals[prev];
    t.out_color = P.hist_color[cur]; t.out_moments = P.moments[cur]; t.hist_world_pos = P.world_pos[cur];
    t.out_hist_len = P.hist_len[cur]; t.unit_normals = P.unit_normals[cur]; t.motion = P.motion;
    if (posed) {
        blok::TemporalPosedArgs tp{};
        tp.t = t; tp.m = *posed;
        blok::launch_temporal_posed(tp, stream);
    } else if (inst) {
        blok::TemporalInstancedArgs ti{};
        ti.t = t; ti.m = *inst;
        blok::launch_temporal_instanced(ti, stream);
    } else {
        blok::launch_temporal(t, stream);
    }

    blok::VarianceArgs v{};
    v.f = f;
    v.color = P.hist_color[cur]; v.moments = P.moments[cur]; v.world_pos = P.world_pos[cur];
    v.hist_len = P.hist_len[cur]; v.unit_normals = P.unit_normals[cur]; v.variance = P.variance;
    blok::launch_variance(v, stream);

    // iteration 0 reads the temporal output; then ping <-> pong (renderer_denoising.cpp:520-536); the last one writes the caller's plane
    const float* src = P.hist_color[cur];
    for (int it = 0; it < S.atrous_iterations; ++it) {
        blok::AtrousArgs a{};
        a.w = f.w; a.h = f.h; a.step = 1 << it; a.phi_color = S.phi_color; a.phi_depth = S.phi_depth;
        a.color = src; a.variance = P.variance; a.world_pos = P.world_pos[cur]; a.unit_normals = P.unit_normals[cur];
        a.out = it == S.atrous_iterations - 1 ? out_color_dev : ((it & 1) ? P.pong : P.ping);
        blok::launch_atrous(a, stream);
        src = a.out;
    }
    if (S.atrous_iterations == 0)
        BLOK_HIP_TRY(ctx, hipMemcpyAsync(out_color_dev, P.hist_color[cur], P.pixels * 4 * sizeof(float), hipMemcpyDeviceToDevice, stream));
    BLOK_HIP_TRY(ctx, hipGetLastError());
    P.cur = prev;                                          // swapHistoryBuffers
    P.has_motion = true;
    return BLOK_OK;
}

int blok_hip_denoise_device(blok_hip_ctx* ctx, const blok_gbuffer* planes, const float* motion_dev, const float prev_view_proj[16],
                            uint32_t frame_count, const blok_denoise_settings* settings, float* out_color_dev, void* hip_stream) {
    if (!ctx) return BLOK_ERR_INVALID_ARG;
    if (!planes) return set_error(ctx, BLOK_ERR_INVALID_ARG, "denoise: null planes");
    blok::TemporalArgs t{};
    t.color = planes->color; t.world_pos = planes->world_pos; t.normal_roughness = planes->normal_roughness; t.motion_in = motion_dev;
    return denoise_frame(ctx, t, prev_view_proj, frame_count, settings, out_color_dev, hip_stream);
}

int blok_hip_denoise_ref_device(blok_hip_ctx* ctx, const blok_gbuffer_ref* planes, const float prev_view_proj[16],
                                uint32_t frame_count, const blok_denoise_settings* settings, float* out_color_dev, void* hip_stream) {
    if (!ctx) return BLOK_ERR_INVALID_ARG;
    if (!planes) return set_error(ctx, BLOK_ERR_INVALID_ARG, "denoise: null planes");
    blok::TemporalArgs t{};
    t.color = planes->color; t.world_pos = planes->world_pos; t.normal_roughness_h = planes->normal_roughness; t.motion_in_h = planes->motion;
    return denoise_frame(ctx, t, prev_view_proj, frame_count, settings, out_color_dev, hip_stream);
}

// The instanced entries' own arguments (a null id plane or table is refused before any other check).
static int check_instanced(blok_hip_ctx* ctx, const uint32_t* ids, const blok_instance* cur, uint32_t n_cur, const blok_instance* prev, uint32_t n_prev) {
    if (!ids) return set_error(ctx, BLOK_ERR_INVALID_ARG, "denoise: null instance id plane");
    if ((n_cur && !cur) || (n_prev && !prev)) return set_error(ctx, BLOK_ERR_INVALID_ARG, "null instance table with non-zero count");
    return BLOK_OK;
}

int blok_hip_denoise_instanced_device(blok_hip_ctx* ctx, const blok_gbuffer* planes, const float* motion_dev, const float prev_view_proj[16],
                                      uint32_t frame_count, const blok_denoise_settings* settings, const uint32_t* instance_ids_dev,
                                      const blok_instance* cur_dev, uint32_t n_cur, const blok_instance* prev_dev, uint32_t n_prev,
                                      float* out_color_dev, void* hip_stream) {
    if (!ctx) return BLOK_ERR_INVALID_ARG;
    if (!planes) return set_error(ctx, BLOK_ERR_INVALID_ARG, "denoise: null planes");
    const int rc = check_instanced(ctx, instance_ids_dev, cur_dev, n_cur, prev_dev, n_prev);
    if (rc != BLOK_OK) return rc;
    blok::TemporalArgs t{};
    t.color = planes->color; t.world_pos = planes->world_pos; t.normal_roughness = planes->normal_roughness; t.motion_in = motion_dev;
    const blok::MotionTables M = motion_tables(ctx, instance_ids_dev, cur_dev, n_cur, prev_dev, n_prev);
    return denoise_frame(ctx, t, prev_view_proj, frame_count, settings, out_color_dev, hip_stream, &M);
}

int blok_hip_denoise_instanced_ref_device(blok_hip_ctx* ctx, const blok_gbuffer_ref* planes, const float prev_view_proj[16],
                                          uint32_t frame_count, const blok_denoise_settings* settings, const uint32_t* instance_ids_dev,
                                          const blok_instance* cur_dev, uint32_t n_cur, const blok_instance* prev_dev, uint32_t n_prev,
                                          float* out_color_dev, void* hip_stream) {
    if (!ctx) return BLOK_ERR_INVALID_ARG;
    if (!planes) return set_error(ctx, BLOK_ERR_INVALID_ARG, "denoise: null planes");
    const int rc = check_instanced(ctx, instance_ids_dev, cur_dev, n_cur, prev_dev, n_prev);
    if (rc != BLOK_OK) return rc;
    blok::TemporalArgs t{};
    t.color = planes->color; t.world_pos = planes->world_pos; t.normal_roughness_h = planes->normal_roughness; t.motion_in_h = planes->motion;
    const blok::MotionTables M = motion_tables(ctx, instance_ids_dev, cur_dev, n_cur, prev_dev, n_prev);
    return denoise_frame(ctx, t, prev_view_proj, frame_count, settings, out_color_dev, hip_stream, &M);
}

// The posed entries: the instanced entries' checks, then the pose tables', then the records' build on the stream.
static int denoise_posed(blok_hip_ctx* ctx, const blok::TemporalArgs& t, const float prev_view_proj[16], uint32_t frame_count,
                         const blok_denoise_settings* settings, const uint32_t* ids_dev, const blok_instance* cur_dev, uint32_t n_cur,
                         const blok_instance* prev_dev, uint32_t n_prev, const blok_pose* cur_poses_dev, uint32_t n_cur_poses,
                         const blok_pose* prev_poses_dev, uint32_t n_prev_poses, float* out_color_dev, void* hip_stream) {
    int rc = check_instanced(ctx, ids_dev, cur_dev, n_cur, prev_dev, n_prev);
    if (rc == BLOK_OK) rc = check_placed_device_tables(ctx, nullptr, 0u, cur_poses_dev, n_cur_poses);
    if (rc == BLOK_OK) rc = check_placed_device_tables(ctx, nullptr, 0u, prev_poses_dev, n_prev_poses);
    if (rc != BLOK_OK) return rc;
    // (the checks denoise_frame makes before it touches the device, made here before the records' kernel is issued)
    if (!t.color || !t.world_pos || (!t.normal_roughness && !t.normal_roughness_h) || !prev_view_proj || !out_color_dev)
        return set_error(ctx, BLOK_ERR_INVALID_ARG, "denoise: colour, world position and normal planes, prevViewProj and an output are required");
    if (settings && (settings->atrous_iterations < 0 || settings->atrous_iterations > 5)) return set_error(ctx, BLOK_ERR_INVALID_ARG, "denoise: 0..5 a-trous iterations");
    BLOK_HIP_TRY(ctx, hipSetDevice(ctx->device));
    const blok_pose_motion* records = nullptr;
    rc = prepare_pose_motion(ctx, cur_poses_dev, n_cur_poses, prev_poses_dev, n_prev_poses, static_cast<hipStream_t>(hip_stream), &records);
    if (rc != BLOK_OK) return rc;
    const blok::PoseMotionTables Q = pose_motion_tables(ctx, ids_dev, cur_dev, n_cur, prev_dev, n_prev, records, n_cur_poses);
    return denoise_frame(ctx, t, prev_view_proj, frame_count, settings, out_color_dev, hip_stream, nullptr, &Q);
}

int blok_hip_denoise_posed_device(blok_hip_ctx* ctx, const blok_gbuffer* planes, const float* motion_dev, const float prev_view_proj[16],
                                  uint32_t frame_count, const blok_denoise_settings* settings, const uint32_t* ids_dev,
                                  const blok_instance* cur_dev, uint32_t n_cur, const blok_instance* prev_dev, uint32_t n_prev,
                                  const blok_pose* cur_poses_dev, uint32_t n_cur_poses, const blok_pose* prev_poses_dev, uint32_t n_prev_poses,
                                  float* out_color_dev, void* hip_stream) {
    if (!ctx) return BLOK_ERR_INVALID_ARG;
    if (!planes) return set_error(ctx, BLOK_ERR_INVALID_ARG, "denoise: null planes");
    blok::TemporalArgs t{};
    t.color = planes->color; t.world_pos = planes->world_pos; t.normal_roughness = planes->normal_roughness; t.motion_in = motion_dev;
    return denoise_posed(ctx, t, prev_view_proj, frame_count, settings, ids_dev, cur_dev, n_cur, prev_dev, n_prev, cur_poses_dev, n_cur_poses,
                         prev_poses_dev, n_prev_poses, out_color_dev, hip_stream);
}

int blok_hip_denoise_posed_ref_device(blok_hip_ctx* ctx, const blok_gbuffer_ref* planes, const float prev_view_proj[16],
                                      uint32_t frame_count, const blok_denoise_settings* settings, const uint32_t* ids_dev,
                                      const blok_instance* cur_dev, uint32_t n_cur, const blok_instance* prev_dev, uint32_t n_prev,
                                      const blok_pose* cur_poses_dev, uint32_t n_cur_poses, const blok_pose* prev_poses_dev, uint32_t n_prev_poses,
                                      float* out_color_dev, void* hip_stream) {
    if (!ctx) return BLOK_ERR_INVALID_ARG;
    if (!planes) return set_error(ctx, BLOK_ERR_INVALID_ARG, "denoise: null planes");
    blok::TemporalArgs t{};
    t.color = planes->color; t.world_pos = planes->world_pos; t.normal_roughness_h = planes->normal_roughness; t.motion_in_h = planes->motion;
    return denoise_posed(ctx, t, prev_view_proj, frame_count, settings, ids_dev, cur_dev, n_cur, prev_dev, n_prev, cur_poses_dev, n_cur_poses,
                         prev_poses_dev, n_prev_poses, out_color_dev, hip_stream);
}

int blok_hip_denoise_state(blok_hip_ctx* ctx, float* history_color, float* moments, float* history_length, float* variance, float* motion) {
    if (!ctx) return BLOK_ERR_INVALID_ARG;
    auto& P = ctx->post;
    if (!P.pixels || !P.has_motion) return set_error(ctx, BLOK_ERR_INVALID_ARG, "no denoised frame yet");
    BLOK_HIP_TRY(ctx, hipSetDevice(ctx->device));
    BLOK_HIP_TRY(ctx, hipDeviceSynchronize());
    const int last = P.cur ^ 1;                            // the slot the last frame wrote
    const size_t n = P.pixels;
    if (history_color) BLOK_HIP_TRY(ctx, hipMemcpy(history_color, P.hist_color[last], 4 * n * sizeof(float), hipMemcpyDeviceToHost));
    if (moments) BLOK_HIP_TRY(ctx, hipMemcpy(moments, P.moments[last], 2 * n * sizeof(float), hipMemcpyDeviceToHost));
    if (variance) BLOK_HIP_TRY(ctx, hipMemcpy(variance, P.variance, n * sizeof(float), hipMemcpyDeviceToHost));
    if (history_length) {
        blok::launch_widen(P.hist_len[last], P.widen, n, nullptr);
        BLOK_HIP_TRY(ctx, hipMemcpy(history_length, P.widen, n * sizeof(float), hipMemcpyDeviceToHost));
    }
    if (motion) {
        blok::launch_widen(P.motion, P.widen, 2 * n, nullptr);
        BLOK_HIP_TRY(ctx, hipMemcpy(motion, P.widen, 2 * n * sizeof(float), hipMemcpyDeviceToHost));
    }
    return BLOK_OK;
}

namespace {
__global__ __launch_bounds__(256) void narrow_motion_kernel(const float* src, uint16_t* dst, size_t n) {
    const size_t i = static_cast<size_t>(blockIdx.x) * 256u + threadIdx.x;
    if (i < n) dst[i] = __half_as_ushort(__float2half_rn(src[i]));
}
}  // namespace

int blok_hip_taa_device(blok_hip_ctx* ctx, const float* color_dev, const float* motion_dev, float feedback_min, float feedback_max,
                        uint32_t frame_count, float* out_color_dev, void* hip_stream) {
    if (!ctx) return BLOK_ERR_INVALID_ARG;
    if (!color_dev || !out_color_dev) return set_error(ctx, BLOK_ERR_INVALID_ARG, "taa: null plane");
    BLOK_HIP_TRY(ctx, hipSetDevice(ctx->device));
    int rc = ensure_post(ctx);
    if (rc != BLOK_OK) return rc;
    auto& P = ctx->post;
    hipStream_t stream = static_cast<hipStream_t>(hip_stream);
    if (motion_dev) {
        const size_t n = 2 * P.pixels;
        hipLaunchKernelGGL(narrow_motion_kernel, dim3(static_cast<uint32_t>((n + 255) / 256)), dim3(256), 0, stream, motion_dev, P.motion, n);
        P.has_motion = true;
    } else if (!P.has_motion) {
        return set_error(ctx, BLOK_ERR_INVALID_ARG, "taa: no motion vectors (pass a plane or denoise a frame first)");
    }
    blok::TaaArgs a{};
    a.w = ctx->width; a.h = ctx->height; a.frame_count = frame_count; a.feedback_min = feedback_min; a.feedback_max = feedback_max;
    a.color = color_dev; a.history = P.taa_hist[P.taa_cur ^ 1]; a.motion = P.motion;
    a.out = out_color_dev; a.out_history = P.taa_hist[P.taa_cur];
    blok::launch_taa(a, stream);
    BLOK_HIP_TRY(ctx, hipGetLastError());
    P.taa_cur ^= 1;
    return BLOK_OK;
}

int blok_hip_sharpen_device(blok_hip_ctx* ctx, const uint32_t* rgba8_dev, float strength, uint32_t* out_rgba8_dev, void* hip_stream) {
    if (!ctx) return BLOK_ERR_INVALID_ARG;
    if (!rgba8_dev || !out_rgba8_dev || rgba8_dev == out_rgba8_dev) return set_error(ctx, BLOK_ERR_INVALID_ARG, "sharpen: two distinct planes are required");
    BLOK_HIP_TRY(ctx, hipSetDevice(ctx->device));
    blok::SharpenArgs a{};
    a.w = ctx->width; a.h = ctx->height; a.strength = strength; a.in = rgba8_dev; a.out = out_rgba8_dev;
    blok::launch_sharpen(a, static_cast<hipStream_t>(hip_stream));
    BLOK_HIP_TRY(ctx, hipGetLastError());
    return BLOK_OK;
}

namespace {
// Column-major prevViewProj of a camera basis: uv = ndc.xy * 0.5 + 0.5 reproduces the basis' own pixel mapping
// (x + 0.5 = u * width, y + 0.5 = v * height), the role FrameUBO::prevViewProj plays for the reference's shaders.
void view_proj_of(const blok_camera& c, float M[16]) {
    const double ta = double(c.tan_half_fov) * double(c.aspect), t = double(c.tan_half_fov);
    double rows[4][4] = {};
    for (int a = 0; a < 3; ++a) {
        rows[0][a] = double(c.right[a]) / ta; rows[0][3] -= double(c.right[a]) * double(c.pos[a]) / ta;
        rows[1][a] = -double(c.up[a]) / t;    rows[1][3] += double(c.up[a]) * double(c.pos[a]) / t;
        rows[2][a] = double(c.fwd[a]);        rows[2][3] -= double(c.fwd[a]) * double(c.pos[a]);
    }
    for (int a = 0; a < 4; ++a) rows[3][a] = rows[2][a];
    for (int col = 0; col < 4; ++col) for (int r = 0; r < 4; ++r) M[col * 4 + r] = static_cast<float>(rows[r][col]);
}
}  // namespace

void blok_camera_view_proj(const blok_camera* cam, float out_view_proj[16]) { if (cam && out_view_proj) view_proj_of(*cam, out_view_proj); }

namespace {
// blok_hip_draw_frame_rt(_instanced(_motion)): the path pass (with the device table instances_dev of n records, or world-only when null), then
// the post chain; one post state and one frame counter for all.  object_motion (and n_instances > 0): the path pass also writes the id
// plane, the motion of tracked instance pixels is corrected against the previous frame's table (ctx->rt_prev_instances, rt_prev_n
// records) and the temporal pass is the instanced one.  object_motion with poses (blok_hip_draw_frame_rt_posed_motion): the posed path pass
// writes the id plane, the poses' records against the previous frame's pose table (ctx->rt_prev_poses, rt_prev_n_poses records) are built
// once, and the motion pass and the temporal pass are the posed ones, which handle the instances too.
int draw_frame_rt(blok_hip_ctx* ctx, const blok_camera* cam, uint32_t spp, uint32_t max_bounces, const blok_denoise_settings* settings,
                  const blok_instance* instances_dev, uint32_t n_instances, uint32_t* out_rgba8_host, uint32_t* out_frame_count,
                  bool object_motion = false, const blok_pose* poses_dev = nullptr, uint32_t n_poses = 0u) {
    int rc = check_trace(ctx, cam);
    if (rc != BLOK_OK) return rc;
    if (!spp || !max_bounces) return set_error(ctx, BLOK_ERR_INVALID_ARG, "spp and bounces must be positive");
    rc = ensure_post(ctx);
    if (rc != BLOK_OK) return rc;
    auto& P = ctx->post;
    const size_t n = P.pixels;
    if (!P.rt_final) {
        // the frame's G-buffer in the reference's image formats (raygen.rgen:55-59): 2 x RGBA32F, RGBA16F, RGBA8, RG16F = 48 B/pixel
        for (int k = 0; k < 2 && rc == BLOK_OK; ++k) rc = zeroed_plane(ctx, &P.rt_planes[k], 4 * n);
        if (rc == BLOK_OK) rc = zeroed_plane(ctx, &P.rt_normal_roughness_h, 4 * n);
        if (rc == BLOK_OK) rc = zeroed_plane(ctx, &P.rt_albedo_metallic_u8, n);
        if (rc == BLOK_OK) rc = zeroed_plane(ctx, &P.rt_motion_h, 2 * n);
        if (rc == BLOK_OK) rc = zeroed_plane(ctx, &P.rt_denoised, 4 * n);
        if (rc == BLOK_OK) rc = zeroed_plane(ctx, &P.rt_resolved, 4 * n);
        if (rc == BLOK_OK) rc = zeroed_plane(ctx, &P.rt_ldr, n);
        if (rc == BLOK_OK) rc = zeroed_plane(ctx, &P.rt_final, n);
        if (rc != BLOK_OK) { P = blok_hip_ctx::Post{}; return rc; }
        P.rt_frame = 0;
    }
    const bool pose_motion = object_motion && n_poses;
    const bool motion = object_motion && ((instances_dev && n_instances) || pose_motion);
    if (motion && !P.rt_ids) {
        rc = zeroed_plane(ctx, &P.rt_ids, n);
        if (rc != BLOK_OK) { P = blok_hip_ctx::Post{}; return rc; }
    }
    const uint32_t frame = P.rt_frame;
    float prev_vp[16];
    view_proj_of(frame ? P.rt_prev_cam : *cam, prev_vp);            // Denoiser::updatePreviousFrameData: last frame's matrices
    const blok_gbuffer_ref planes{P.rt_planes[0], P.rt_planes[1], P.rt_normal_roughness_h, P.rt_albedo_metallic_u8, P.rt_motion_h};
    // the frame's projection carries jitterSequence[frame mod 16] (renderer_draw.cpp:64-81; the index advances once per frame,
    // renderer_postprocess.cpp:660-663); prevViewProj above stays un-jittered, as Denoiser::updatePreviousFrameData is fed
    // (renderer_draw.cpp:313-328 passes the base matrices)
    const float saved_jitter[2] = {ctx->jitter_px[0], ctx->jitter_px[1]};
    if (ctx->rt_taa_jitter) blok::taa_jitter_px(frame, ctx->jitter_px);
    rc = n_poses       ? blok_hip_trace_paths_posed_ref_device(ctx, cam, 0, 0, ctx->width, ctx->height, spp, max_bounces, frame, instances_dev, n_instances,
                                                               poses_dev, n_poses, prev_vp, &planes, pose_motion ? P.rt_ids : nullptr, nullptr)
       : instances_dev ? blok_hip_trace_paths_instanced_ref_device(ctx, cam, 0, 0, ctx->width, ctx->height, spp, max_bounces, frame, instances_dev,
                                                                   n_instances, prev_vp, &planes, motion ? P.rt_ids : nullptr, nullptr)
                       : blok_hip_trace_paths_ref_device(ctx, cam, 0, 0, ctx->width, ctx->height, spp, max_bounces, frame, prev_vp, &planes, nullptr);
    ctx->jitter_px[0] = saved_jitter[0]; ctx->jitter_px[1] = saved_jitter[1];
    if (pose_motion) {
        const blok_pose_motion* records = nullptr;
        if (rc == BLOK_OK) rc = prepare_pose_motion(ctx, poses_dev, n_poses, ctx->rt_prev_poses, P.rt_prev_n_poses, nullptr, &records);
        const blok::PoseMotionTables Q = pose_motion_tables(ctx, P.rt_ids, instances_dev, n_instances, ctx->rt_prev_instances, P.rt_prev_n, records, n_poses);
        if (rc == BLOK_OK) rc = posed_motion_pass(ctx, 0, 0, ctx->width, ctx->height, P.rt_planes[1], Q, prev_vp, P.rt_motion_h, nullptr, nullptr);
        if (rc == BLOK_OK) {
            blok::TemporalArgs t{};
            t.color = planes.color; t.world_pos = planes.world_pos; t.normal_roughness_h = planes.normal_roughness; t.motion_in_h = planes.motion;
            rc = denoise_frame(ctx, t, prev_vp, frame, settings, P.rt_denoised, nullptr, nullptr, &Q);
        }
    } else if (motion) {
        const uint32_t n_prev = P.rt_prev_n;
        if (rc == BLOK_OK)
            rc = blok_hip_instance_motion_device(ctx, 0, 0, ctx->width, ctx->height, P.rt_planes[1], P.rt_ids, instances_dev, n_instances,
                                                 ctx->rt_prev_instances, n_prev, prev_vp, P.rt_motion_h, nullptr, nullptr);
        if (rc == BLOK_OK)
            rc = blok_hip_denoise_instanced_ref_device(ctx, &planes, prev_vp, frame, settings, P.rt_ids, instances_dev, n_instances,
                                                       ctx->rt_prev_instances, n_prev, P.rt_denoised, nullptr);
    } else if (rc == BLOK_OK) {
        rc = blok_hip_denoise_ref_device(ctx, &planes, prev_vp, frame, settings, P.rt_denoised, nullptr);
    }
    if (rc == BLOK_OK) rc = blok_hip_taa_device(ctx, P.rt_denoised, nullptr, 0.93f, 0.98f, frame, P.rt_resolved, nullptr);       // renderer_postprocess.hpp:104-106
    if (rc == BLOK_OK) rc = blok_hip_tonemap_device(ctx, P.rt_resolved, static_cast<uint32_t>(n), 1.0f, 1.15f, 1, P.rt_ldr, nullptr);   // :110-113
    if (rc == BLOK_OK) rc = blok_hip_sharpen_device(ctx, P.rt_ldr, 0.5f, P.rt_final, nullptr);                                     // :117-118
    if (rc != BLOK_OK) return rc;
    P.rt_prev_cam = *cam;
    P.rt_frame = frame + 1;
    P.rt_prev_n = object_motion ? n_instances : 0u;        // the table itself: the motion entry swaps the buffers after this call
    P.rt_prev_n_poses = pose_motion ? n_poses : 0u;        // ... and the pose table, likewise
    if (out_frame_count) *out_frame_count = P.rt_frame;
    if (out_rgba8_host) BLOK_HIP_TRY(ctx, hipMemcpy(out_rgba8_host, P.rt_final, n * sizeof(uint32_t), hipMemcpyDeviceToHost));
    else BLOK_HIP_TRY(ctx, hipDeviceSynchronize());
    return BLOK_OK;
}
}  // namespace

int blok_hip_draw_frame_rt(blok_hip_ctx* ctx, const blok_camera* cam, uint32_t spp, uint32_t max_bounces,
                           const blok_denoise_settings* settings, uint32_t* out_rgba8_host, uint32_t* out_frame_count) {
    return draw_frame_rt(ctx, cam, spp, max_bounces, settings, nullptr, 0u, out_rgba8_host, out_frame_count);
}

namespace {
// The host table, checked, in the context's device buffer rt_instances (the previous frame's call ended with a synchronising copy or a
// device synchronise).
int upload_rt_table(blok_hip_ctx* ctx, const blok_camera* cam, const blok_instance* instances_host, uint32_t n_instances) {
    int rc = check_trace(ctx, cam);
    if (rc != BLOK_OK) return rc;
    rc = blok_hip_check_instances(ctx, instances_host, n_instances);
    if (rc != BLOK_OK) return rc;
    BLOK_HIP_TRY(ctx, ctx->rt_instances.reserve(n_instances ? n_instances : 1u, blok::FreeAfter::nothing()));
    if (n_instances) BLOK_HIP_TRY(ctx, hipMemcpy(ctx->rt_instances, instances_host, n_instances * sizeof(blok_instance), hipMemcpyHostToDevice));
    return BLOK_OK;
}
}  // namespace

int blok_hip_draw_frame_rt_instanced(blok_hip_ctx* ctx, const blok_camera* cam, uint32_t spp, uint32_t max_bounces,
                                     const blok_denoise_settings* settings, const blok_instance* instances_host, uint32_t n_instances,
                                     uint32_t* out_rgba8_host, uint32_t* out_frame_count) {
    const int rc = upload_rt_table(ctx, cam, instances_host, n_instances);
    if (rc != BLOK_OK) return rc;
    return draw_frame_rt(ctx, cam, spp, max_bounces, settings, ctx->rt_instances, n_instances, out_rgba8_host, out_frame_count);
}

int blok_hip_draw_frame_rt_posed(blok_hip_ctx* ctx, const blok_camera* cam, uint32_t spp, uint32_t max_bounces, const blok_denoise_settings* settings,
                                 const blok_instance* instances_host, uint32_t n_instances, const blok_pose* poses_host, uint32_t n_poses,
                                 uint32_t* out_rgba8_host, uint32_t* out_frame_count) {
    int rc = check_trace(ctx, cam);                       // both tables are checked before either is uploaded
    if (rc == BLOK_OK) rc = blok_hip_check_instances(ctx, instances_host, n_instances);
    if (rc == BLOK_OK) rc = blok_hip_check_poses(ctx, poses_host, n_poses);
    if (rc == BLOK_OK) rc = upload_rt_table(ctx, cam, instances_host, n_instances);
    if (rc != BLOK_OK) return rc;
    if (n_poses) {
        BLOK_HIP_TRY(ctx, ctx->rt_poses.reserve(n_poses, blok::FreeAfter::nothing()));
        BLOK_HIP_TRY(ctx, hipMemcpy(ctx->rt_poses, poses_host, n_poses * sizeof(blok_pose), hipMemcpyHostToDevice));
    }
    return draw_frame_rt(ctx, cam, spp, max_bounces, settings, ctx->rt_instances, n_instances, out_rgba8_host, out_frame_count, false, ctx->rt_poses, n_poses);
}

int blok_hip_draw_frame_rt_instanced_motion(blok_hip_ctx* ctx, const blok_camera* cam, uint32_t spp, uint32_t max_bounces,
                                            const blok_denoise_settings* settings, const blok_instance* instances_host, uint32_t n_instances,
                                            uint32_t* out_rgba8_host, uint32_t* out_frame_count) {
    const int rc = upload_rt_table(ctx, cam, instances_host, n_instances);
    if (rc != BLOK_OK) return rc;
    const int drawn = draw_frame_rt(ctx, cam, spp, max_bounces, settings, ctx->rt_instances, n_instances, out_rgba8_host, out_frame_count, true);
    if (drawn != BLOK_OK) return drawn;
    // this frame's table becomes the previous one (the frame ended with a synchronise; the next upload overwrites the older buffer)
    std::swap(ctx->rt_instances, ctx->rt_prev_instances);
    return BLOK_OK;
}

int blok_hip_draw_frame_rt_posed_motion(blok_hip_ctx* ctx, const blok_camera* cam, uint32_t spp, uint32_t max_bounces,
                                        const blok_denoise_settings* settings, const blok_instance* instances_host, uint32_t n_instances,
                                        const blok_pose* poses_host, uint32_t n_poses, uint32_t* out_rgba8_host, uint32_t* out_frame_count) {
    int rc = check_trace(ctx, cam);                       // both tables are checked before either is uploaded
    if (rc == BLOK_OK) rc = blok_hip_check_instances(ctx, instances_host, n_instances);
    if (rc == BLOK_OK) rc = blok_hip_check_poses(ctx, poses_host, n_poses);
    if (rc != BLOK_OK) return rc;
    if (!n_poses)                                        // the instanced motion entry itself: the same launches, the same bytes
        return blok_hip_draw_frame_rt_instanced_motion(ctx, cam, spp, max_bounces, settings, instances_host, n_instances, out_rgba8_host, out_frame_count);
    rc = upload_rt_table(ctx, cam, instances_host, n_instances);
    if (rc != BLOK_OK) return rc;
    BLOK_HIP_TRY(ctx, ctx->rt_poses.reserve(n_poses, blok::FreeAfter::nothing()));
    BLOK_HIP_TRY(ctx, hipMemcpy(ctx->rt_poses, poses_host, n_poses * sizeof(blok_pose), hipMemcpyHostToDevice));
    rc = draw_frame_rt(ctx, cam, spp, max_bounces, settings, ctx->rt_instances, n_instances, out_rgba8_host, out_frame_count, true, ctx->rt_poses, n_poses);
    if (rc != BLOK_OK) return rc;
    // this frame's tables become the previous ones (the frame ended with a synchronise; the next uploads overwrite the older buffers)
    std::swap(ctx->rt_instances, ctx->rt_prev_instances);
    std::swap(ctx->rt_poses, ctx->rt_prev_poses);
    return BLOK_OK;
}

int blok_hip_post_reset(blok_hip_ctx* ctx) {
    if (!ctx) return BLOK_ERR_INVALID_ARG;
    (void)hipSetDevice(ctx->device);
    (void)hipDeviceSynchronize();
    ctx->post = blok_hip_ctx::Post{};
    return BLOK_OK;
}

}  // extern "C"
