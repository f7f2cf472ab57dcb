// The entries of include/blok_hip_debug.h: tuning switches that were measured against each other, read-backs and hooks for the tests and the
// experiment scripts.  Nothing a drop-in user of include/blok_hip.h needs; split from api.hip in round 4.
#include "api_internal.h"
#include <cstdlib>
#include <cstdio>

using namespace blok_api;

extern "C" {

int blok_hip_set_host_build(blok_hip_ctx* ctx, int enabled) {
    if (!ctx) return BLOK_ERR_INVALID_ARG;
    ctx->force_host_build = enabled != 0;
    return BLOK_OK;
}

int blok_hip_world_built_on_device(const blok_hip_ctx* ctx) { return ctx && ctx->has_world && ctx->built_on_device ? 1 : 0; }

int blok_hip_download_tree(const blok_hip_ctx* ctx, void* nodes_out, size_t node_capacity, uint32_t* materials_out,
                           size_t material_capacity) {
    if (!ctx || !ctx->has_world) return BLOK_ERR_NO_WORLD;
    if ((nodes_out && node_capacity < ctx->stats.n_tree_nodes) || (materials_out && material_capacity < ctx->stats.n_voxels))
        return BLOK_ERR_INVALID_ARG;
    if (nodes_out && hipMemcpy(nodes_out, ctx->d_nodes, ctx->stats.n_tree_nodes * sizeof(blok::TreeNode), hipMemcpyDeviceToHost) != hipSuccess)
        return BLOK_ERR_HIP;
    if (materials_out && ctx->stats.n_voxels &&
        hipMemcpy(materials_out, ctx->d_tree_materials, ctx->stats.n_voxels * sizeof(uint32_t), hipMemcpyDeviceToHost) != hipSuccess)
        return BLOK_ERR_HIP;
    return BLOK_OK;
}

int blok_hip_download_model(blok_hip_ctx* ctx, uint32_t model, void* nodes_out, size_t node_capacity, uint32_t* materials_out, size_t material_capacity,
                            blok_model_info* out_info) {
    if (!ctx) return BLOK_ERR_INVALID_ARG;
    if (!known_model(ctx, model)) return set_error(ctx, BLOK_ERR_INVALID_ARG, "unknown model " + std::to_string(model));
    const blok::ModelDesc& m = ctx->models.desc[model];
    const uint32_t n_nodes = ctx->models.own[model].n_nodes, n_materials = ctx->models.own[model].n_materials;
    if ((nodes_out && node_capacity < n_nodes) || (materials_out && material_capacity < n_materials))
        return set_error(ctx, BLOK_ERR_INVALID_ARG, "download_model: output smaller than the model's array");
    BLOK_HIP_TRY(ctx, hipSetDevice(ctx->device));
    if (nodes_out && n_nodes) BLOK_HIP_TRY(ctx, hipMemcpy(nodes_out, m.nodes, n_nodes * sizeof(blok::TreeNode), hipMemcpyDeviceToHost));
    if (materials_out && n_materials) BLOK_HIP_TRY(ctx, hipMemcpy(materials_out, m.materials, n_materials * sizeof(uint32_t), hipMemcpyDeviceToHost));
    if (out_info) {
        out_info->levels = m.levels;
        const auto& own = ctx->models.own[model];        // (the box in the model's own voxels, whatever its scale)
        for (int a = 0; a < 3; ++a) { out_info->origin[a] = m.origin[a]; out_info->lo[a] = own.box_lo[a]; out_info->hi[a] = own.box_hi[a]; }
        out_info->n_nodes = n_nodes; out_info->n_materials = n_materials;
    }
    return BLOK_OK;
}

// The pre-pass alone: start parameter (and node visits) per beam tile of the rectangle, to the host.
int blok_hip_beam_prepass(blok_hip_ctx* ctx, const blok_camera* cam, uint32_t x0, uint32_t y0, uint32_t w, uint32_t h,
                          float* out_t0_host, uint32_t* out_visits_host, size_t capacity) {
    int rc = check_trace(ctx, cam);
    if (rc != BLOK_OK) return rc;
    if (!out_t0_host || !rect_inside(ctx, x0, y0, w, h)) return set_error(ctx, BLOK_ERR_INVALID_ARG, "rectangle outside the frame or no output");
    if (!ctx->beam_tile) return set_error(ctx, BLOK_ERR_INVALID_ARG, "the beam pre-pass is off (blok_hip_set_beam)");
    blok::TraceArgs a = base_args(ctx, cam);
    a.x0 = x0; a.y0 = y0; a.w = w; a.h = h;
    uint32_t n_beams = 0;
    rc = prepare_beam(ctx, blok::RayMode::Rect, a, nullptr, 0, &n_beams);
    if (rc != BLOK_OK) return rc;
    if (!n_beams || capacity < n_beams) return set_error(ctx, BLOK_ERR_INVALID_ARG, "output too small for the rectangle's beam tiles");
    blok::DeviceArray<uint32_t> d_visits;
    if (out_visits_host) BLOK_HIP_TRY(ctx, d_visits.reserve(n_beams, blok::FreeAfter::nothing()));
    a.debug_visits = d_visits;
    a.miss_in_walk = 1u;                               // nothing is written but the start parameters
    blok::launch_beam(blok::RayMode::Rect, a, n_beams, nullptr);
    hipError_t e = hipGetLastError();
    if (e == hipSuccess) e = hipMemcpy(out_t0_host, a.beam, n_beams * sizeof(float), hipMemcpyDeviceToHost);
    if (e == hipSuccess && d_visits) e = hipMemcpy(out_visits_host, d_visits, n_beams * sizeof(uint32_t), hipMemcpyDeviceToHost);
    BLOK_HIP_TRY(ctx, e);
    return BLOK_OK;
}

// The shadow rays' last-occluder map as it lies in device memory, with its frame and update_sun_map's bookkeeping.  The copy goes through
// the null stream, where every raise and tighten launch was enqueued: it sees them all.
int blok_hip_sun_map_download(blok_hip_ctx* ctx, blok_sun_map_info* out_info, float* map_out, size_t capacity) {
    if (!ctx) return BLOK_ERR_INVALID_ARG;
    if (!out_info) return set_error(ctx, BLOK_ERR_INVALID_ARG, "sun map: no info struct");
    *out_info = blok_sun_map_info{};
    if (!ctx->has_sun_map || !ctx->d_sun_map) return BLOK_OK;
    const blok::SunMapArgs& m = ctx->sun;
    for (int a = 0; a < 3; ++a) { out_info->u[a] = m.u[a]; out_info->v[a] = m.v[a]; out_info->s[a] = m.s[a]; }
    out_info->u0 = m.u0; out_info->v0 = m.v0; out_info->texel = m.texel; out_info->nu = m.nu; out_info->nv = m.nv;
    out_info->has_map = 1u;
    out_info->loose_edits = ctx->sun_loose_edits;
    out_info->tighten_pending = ctx->sun_tighten_pending ? 1u : 0u;
    if (ctx->sun_tighten_pending) {
        out_info->pending_u0 = ctx->sun_tighten_u0; out_info->pending_u1 = ctx->sun_tighten_u1;
        out_info->pending_v0 = ctx->sun_tighten_v0; out_info->pending_v1 = ctx->sun_tighten_v1;
    }
    if (!map_out) return BLOK_OK;
    const size_t n = static_cast<size_t>(m.nu) * m.nv;
    if (capacity < n) return set_error(ctx, BLOK_ERR_INVALID_ARG, "sun map: output smaller than nu * nv floats");
    BLOK_HIP_TRY(ctx, hipSetDevice(ctx->device));
    BLOK_HIP_TRY(ctx, hipMemcpy(map_out, ctx->d_sun_map, n * sizeof(float), hipMemcpyDeviceToHost));
    return BLOK_OK;
}

// The counting sort behind a moving camera's frames (tile_order.h), on the caller's costs: order, its inverse, the live prefix and the
// depth sums, to the host.
int blok_hip_debug_class_order(blok_hip_ctx* ctx, const uint32_t* cost_host, uint32_t tiles_x, uint32_t tiles_y, uint32_t radius, const float* beam_host, uint32_t n_beams,
                               uint32_t* out_order_host, uint32_t* out_rank_of_host, uint32_t* out_live, float* out_depth_sums3) {
    if (!ctx) return BLOK_ERR_INVALID_ARG;
    if (!cost_host || !out_order_host || !out_rank_of_host || !out_live || !tiles_x || !tiles_y || static_cast<uint64_t>(tiles_x) * tiles_y > (1u << 24) || radius > 8u)
        return set_error(ctx, BLOK_ERR_INVALID_ARG, "class order: costs, outputs, a grid of at most 2^24 tiles and a radius of at most 8");
    BLOK_HIP_TRY(ctx, hipSetDevice(ctx->device));
    const uint32_t n = tiles_x * tiles_y;
    blok::DeviceMem mem;
    uint32_t *d_cost = nullptr, *d_order = nullptr, *d_rank = nullptr, *d_live = nullptr;
    float *d_beam = nullptr, *d_depth = nullptr;
    unsigned char* d_scratch = nullptr;
    hipError_t e = mem.alloc(&d_cost, n);
    if (e == hipSuccess) e = mem.alloc(&d_order, n);
    if (e == hipSuccess) e = mem.alloc(&d_rank, n);
    if (e == hipSuccess) e = mem.alloc(&d_live, 1);
    if (e == hipSuccess) e = mem.alloc(&d_depth, blok::kOrderDepthPartials * 3);
    if (e == hipSuccess) e = mem.alloc(&d_beam, n_beams);
    if (e == hipSuccess) e = mem.alloc(&d_scratch, blok::tile_order_class_sort_bytes(tiles_x, tiles_y));
    if (e == hipSuccess) e = hipMemcpy(d_cost, cost_host, n * sizeof(uint32_t), hipMemcpyHostToDevice);
    if (e == hipSuccess && n_beams && beam_host) e = hipMemcpy(d_beam, beam_host, n_beams * sizeof(float), hipMemcpyHostToDevice);
    if (e == hipSuccess) e = hipMemset(d_order, 0xFF, n * sizeof(uint32_t));
    if (e == hipSuccess) e = hipMemset(d_rank, 0xFF, n * sizeof(uint32_t));
    if (e == hipSuccess) e = blok::launch_tile_order_class_sort(d_cost, tiles_x, tiles_y, radius, d_scratch, d_order, d_rank, d_live, d_beam, nullptr, 0u, beam_host ? n_beams : 0u, d_depth, nullptr);
    if (e == hipSuccess) e = hipMemcpy(out_order_host, d_order, n * sizeof(uint32_t), hipMemcpyDeviceToHost);
    if (e == hipSuccess) e = hipMemcpy(out_rank_of_host, d_rank, n * sizeof(uint32_t), hipMemcpyDeviceToHost);
    if (e == hipSuccess) e = hipMemcpy(out_live, d_live, sizeof(uint32_t), hipMemcpyDeviceToHost);
    if (e == hipSuccess && out_depth_sums3) {
        float part[blok::kOrderDepthPartials * 3];
        e = hipMemcpy(part, d_depth, sizeof(part), hipMemcpyDeviceToHost);
        out_depth_sums3[0] = out_depth_sums3[1] = out_depth_sums3[2] = 0.0f;
        for (uint32_t k = 0; k < blok::kOrderDepthPartials; ++k) for (int c = 0; c < 3; ++c) out_depth_sums3[c] += part[k * 3 + c];
    }
    BLOK_HIP_TRY(ctx, e);
    return BLOK_OK;
}

// Walks exactly the listed 8x8-pixel wave tiles of the rectangle, in list order (walk workgroup j takes entry j).
int blok_hip_trace_wave_tiles_device(blok_hip_ctx* ctx, const blok_camera* cam, uint32_t x0, uint32_t y0, uint32_t w, uint32_t h,
                                     const uint32_t* tiles_host, const float* t0_host, size_t n_tiles, void* out_hits_dev, void* out_rgba_dev, void* hip_stream) {
    int rc = check_trace(ctx, cam);
    if (rc != BLOK_OK) return rc;
    if ((!out_hits_dev && !out_rgba_dev) || !rect_inside(ctx, x0, y0, w, h)) return set_error(ctx, BLOK_ERR_INVALID_ARG, "rectangle outside the frame or no output");
    if (blok::kBlock != 64) return set_error(ctx, BLOK_ERR_UNSUPPORTED, "wave-tile lists need the one-wave-per-workgroup build");
    if (!n_tiles) return BLOK_OK;
    if (!tiles_host) return set_error(ctx, BLOK_ERR_INVALID_ARG, "null tile list");
    const uint32_t bx_count = (w + blok::kTileW - 1u) / blok::kTileW, by_count = (h + blok::kTileH - 1u) / blok::kTileH;
    if (static_cast<uint64_t>(bx_count) * by_count >= (1u << blok::kListTaskBits) || n_tiles > 0x7FFFFFFFu) return set_error(ctx, BLOK_ERR_UNSUPPORTED, "rectangle too large for a wave-tile list");
    for (size_t i = 0; i < n_tiles; ++i) {
        if (tiles_host[i] >= bx_count * by_count) return set_error(ctx, BLOK_ERR_INVALID_ARG, "wave tile index outside the rectangle");
        if (t0_host && !(t0_host[i] >= 0.0f && t0_host[i] < blok::kBeamNone)) return set_error(ctx, BLOK_ERR_INVALID_ARG, "start parameters must be finite and >= 0");
    }
    hipStream_t stream = static_cast<hipStream_t>(hip_stream);
    blok::TraceArgs a = base_args(ctx, cam);
    a.x0 = x0; a.y0 = y0; a.w = w; a.h = h;
    a.out = static_cast<blok_hit*>(out_hits_dev);
    a.out_rgba = static_cast<uint32_t*>(out_rgba_dev);
    a.beam_tile = blok::kWaveW;                          // one entry per "search": the list's capacity arithmetic
    rc = live_list(ctx, a, stream, static_cast<uint32_t>(n_tiles), 1u);
    if (rc != BLOK_OK) return rc;
    const size_t cap = a.list.seg_capacity;
    const uint32_t cls = blok::kListUnknownClass;          // one class: the caller's order is the order
    std::vector<unsigned long long> entries(cap * blok::kListSegments * blok::kListClasses, 0ull), ctl(blok::kListSegments * blok::kListCtlWords, 0ull);
    uint32_t count[blok::kListSegments] = {};
    for (size_t i = 0; i < n_tiles; ++i) {                 // entry i -> segment i mod 8, slot i / 8: walk workgroup i takes it
        const uint32_t seg = static_cast<uint32_t>(i % blok::kListSegments);
        const float t0 = t0_host ? t0_host[i] : 0.0f;
        uint32_t bits; std::memcpy(&bits, &t0, sizeof(bits));
        entries[(seg * blok::kListClasses + cls) * cap + i / blok::kListSegments] = (static_cast<unsigned long long>(a.list.serial) << 44) | (static_cast<unsigned long long>(tiles_host[i]) << 23) | (bits >> 8);
        count[seg] += 1u;
    }
    for (uint32_t seg = 0; seg < blok::kListSegments; ++seg)
        for (uint32_t c = 0; c < blok::kListClasses; ++c)
            ctl[seg * blok::kListCtlWords + blok::kListFinal + c] = (static_cast<unsigned long long>(a.list.serial) << 32) | (c == cls ? count[seg] : 0u);
    BLOK_HIP_TRY(ctx, hipStreamSynchronize(stream));     // the stream's list may still be in use by an earlier launch
    BLOK_HIP_TRY(ctx, hipMemcpy(a.list.entries, entries.data(), entries.size() * sizeof(unsigned long long), hipMemcpyHostToDevice));
    BLOK_HIP_TRY(ctx, hipMemcpy(a.list.ctl, ctl.data(), ctl.size() * sizeof(unsigned long long), hipMemcpyHostToDevice));
    ctx->beam_buffers[stream].list_hint_valid = false;   // this list says nothing about the next frame's
    a.list.hint = nullptr;
    const uint32_t walkers = static_cast<uint32_t>((n_tiles + blok::kListSegments - 1u) / blok::kListSegments) * blok::kListSegments;
    for (uint32_t c = 0; c < blok::kListClasses; ++c) a.list.walkers[c] = c == cls ? walkers / blok::kListSegments : 0u;
    if (ctx->timing) BLOK_HIP_TRY(ctx, hipEventRecord(ctx->ev_begin, stream));
    blok::launch_list_walk(blok::RayMode::Rect, a, nullptr, walkers, stream);
    BLOK_HIP_TRY(ctx, hipGetLastError());
    if (ctx->timing) { BLOK_HIP_TRY(ctx, hipEventRecord(ctx->ev_end, stream)); ctx->timed = true; }
    return BLOK_OK;
}

int blok_hip_set_debug_wave_clocks(blok_hip_ctx* ctx, void* clocks_dev) {
    if (!ctx) return BLOK_ERR_INVALID_ARG;
    ctx->debug_clocks = static_cast<uint32_t*>(clocks_dev);
    return BLOK_OK;
}

int blok_hip_set_path_start(blok_hip_ctx* ctx, int resume_from_anchor, int wave_tile_beam) {
    if (!ctx) return BLOK_ERR_INVALID_ARG;
    ctx->path_resume = resume_from_anchor != 0; ctx->path_fine_beam = wave_tile_beam != 0;
    return BLOK_OK;
}

int blok_hip_set_pose_tlas(blok_hip_ctx* ctx, int enabled) {
    if (!ctx) return BLOK_ERR_INVALID_ARG;
    ctx->pose_tlas = enabled != 0;
    return BLOK_OK;
}

int blok_hip_set_ray_batching(blok_hip_ctx* ctx, int enabled) {
    if (!ctx) return BLOK_ERR_INVALID_ARG;
    if (enabled < 0 || enabled > 3) return set_error(ctx, BLOK_ERR_INVALID_ARG, "ray batching: 0 off, 1 by kind, 2 by sample and kind, 3 and the bounce rounds' tail pool");
    ctx->ray_batching = static_cast<uint32_t>(enabled);
    if (const char* caps = std::getenv("BLOK_TAIL_CAPS")) {      // "24,32": experiments
        unsigned a = 0, b = 0;
        if (std::sscanf(caps, "%u,%u", &a, &b) == 2 && a && b) { ctx->tail_cap = a; ctx->tail_cap_parked = b; }
    }
    return BLOK_OK;
}

int blok_hip_set_sun_map(blok_hip_ctx* ctx, int enabled) {
    if (!ctx) return BLOK_ERR_INVALID_ARG;
    ctx->sun_map_enabled = enabled != 0;
    return BLOK_OK;
}

int blok_hip_set_beam(blok_hip_ctx* ctx, uint32_t beam_tile_pixels) {
    if (!ctx) return BLOK_ERR_INVALID_ARG;
    if (beam_tile_pixels != 0 && beam_tile_pixels != 8 && beam_tile_pixels != 16 && beam_tile_pixels != 32 && beam_tile_pixels != 64)
        return set_error(ctx, BLOK_ERR_INVALID_ARG, "beam tile must be 0 (off), 8, 16, 32 or 64 pixels");
    ctx->beam_tile = beam_tile_pixels;
    return BLOK_OK;
}

int blok_hip_set_fused(blok_hip_ctx* ctx, int enabled) {
    if (!ctx) return BLOK_ERR_INVALID_ARG;
    if (enabled < 0 || enabled > 5) return set_error(ctx, BLOK_ERR_INVALID_ARG, "launch form: 0 (two launches), 1 (one persistent launch with queues), 2 (joint launch), 3 (automatic), 4 (list-fed joint launch) or 5 (list-fed walk behind the beam launch)");
    ctx->launch_form = enabled;
    return BLOK_OK;
}

int blok_hip_frame_queue_stalls(blok_hip_ctx* ctx, uint32_t* out_stalled_waves) {
    if (!ctx || !out_stalled_waves) return BLOK_ERR_INVALID_ARG;
    *out_stalled_waves = 0;
    BLOK_HIP_TRY(ctx, hipSetDevice(ctx->device));
    BLOK_HIP_TRY(ctx, hipDeviceSynchronize());
    for (auto& kv : ctx->beam_buffers) {
        if (kv.second.gave_up) {                                         // joint launch: walk waves that stopped waiting for their tile's search
            uint32_t n = 0;
            BLOK_HIP_TRY(ctx, hipMemcpy(&n, kv.second.gave_up, sizeof(n), hipMemcpyDeviceToHost));
            *out_stalled_waves += n;
        }
        if (!kv.second.ctl) continue;
        for (uint32_t part = 0; part < blok::kFrameParts; ++part) {      // all possible parts: the words of unused ones stay 0
            uint32_t n = 0;
            BLOK_HIP_TRY(ctx, hipMemcpy(&n, kv.second.ctl + part * blok::kFramePartWords + blok::kFrameStalledWord, sizeof(n), hipMemcpyDeviceToHost));
            *out_stalled_waves += n;
        }
    }
    return BLOK_OK;
}

int blok_hip_last_launch_kind(const blok_hip_ctx* ctx) { return ctx ? ctx->last_launch_kind : -1; }

int blok_hip_set_tile_ordering(blok_hip_ctx* ctx, int resort_every_n_frames) {
    if (!ctx) return BLOK_ERR_INVALID_ARG;
    if (resort_every_n_frames < 0) return set_error(ctx, BLOK_ERR_INVALID_ARG, "tile ordering: interval must be >= 0");
    ctx->order.enabled = resort_every_n_frames != 0;
    if (resort_every_n_frames) ctx->order.interval = ctx->order.interval_now = static_cast<uint32_t>(resort_every_n_frames);
    return BLOK_OK;
}

int blok_hip_set_rank_tile_ordering(blok_hip_ctx* ctx, int enabled) {
    if (!ctx) return BLOK_ERR_INVALID_ARG;
    ctx->order.rank_tiles = enabled != 0;
    return BLOK_OK;
}

int blok_hip_debug_force_order_shift(blok_hip_ctx* ctx, int enabled, uint32_t shift_x, uint32_t shift_y) {
    if (!ctx) return BLOK_ERR_INVALID_ARG;
    ctx->order.debug_shift = enabled != 0; ctx->order.debug_sx = shift_x; ctx->order.debug_sy = shift_y;
    return BLOK_OK;
}

int64_t blok_hip_last_fallback_tiles(const blok_hip_ctx* ctx) {
    if (!ctx || !ctx->order.h_fallback) return -1;
    return static_cast<int64_t>(*static_cast<volatile uint32_t*>(ctx->order.h_fallback));
}

int blok_hip_set_moving_order(blok_hip_ctx* ctx, int enabled) {
    if (!ctx) return BLOK_ERR_INVALID_ARG;
    ctx->order.moving = enabled != 0;
    return BLOK_OK;
}

int blok_hip_last_order_use(const blok_hip_ctx* ctx, int32_t* out_shift_x, int32_t* out_shift_y) {
    if (!ctx) return -1;
    if (out_shift_x) *out_shift_x = static_cast<int32_t>(ctx->order.last_sx);
    if (out_shift_y) *out_shift_y = static_cast<int32_t>(ctx->order.last_sy);
    return ctx->order.last_use;
}

int blok_hip_set_joint_prefix_limit(blok_hip_ctx* ctx, uint32_t max_walk_waves) {
    if (!ctx) return BLOK_ERR_INVALID_ARG;
    ctx->order.prefix_limit = max_walk_waves;
    return BLOK_OK;
}

int blok_hip_set_list_classes(blok_hip_ctx* ctx, int enabled) {
    if (!ctx) return BLOK_ERR_INVALID_ARG;
    ctx->list_classes = enabled != 0;
    return BLOK_OK;
}

int blok_hip_set_miss_writer(blok_hip_ctx* ctx, int in_walk) {
    if (!ctx) return BLOK_ERR_INVALID_ARG;
    ctx->miss_in_walk = in_walk != 0;
    return BLOK_OK;
}

int blok_hip_set_beam_cache(blok_hip_ctx* ctx, int mode) {
    if (!ctx) return BLOK_ERR_INVALID_ARG;
    ctx->beam_cache.enabled = mode != 0;
    ctx->beam_cache.refine = mode >= 2;
    ctx->beam_cache.packed = mode >= 3;
    ctx->beam_cache.policy.own_starts = mode >= 4;
    ctx->beam_cache.policy.node_restart = mode >= 5;
    blok::beam_cache_clear(ctx->beam_cache.policy);      // off: every launch searches, as before there was a cache; on again: views are admitted afresh
    if (!ctx->beam_cache.packed) return BLOK_OK;
    BLOK_HIP_TRY(ctx, hipSetDevice(ctx->device));
    return beam_list_buffers(ctx);                       // (a blocking entry: the lists' buffers are allocated here, not by a launch)
}

int blok_hip_set_beam_list_after(blok_hip_ctx* ctx, uint32_t hits) {
    if (!ctx) return BLOK_ERR_INVALID_ARG;
    ctx->beam_cache.policy.list_after = hits ? hits : blok::kBeamListAfter;
    return BLOK_OK;
}

uint32_t blok_hip_pack_area(void) { return blok::kPackArea; }

int blok_hip_beam_cache_list_builds(const blok_hip_ctx* ctx, uint64_t* out_builds) {
    if (!ctx) return BLOK_ERR_INVALID_ARG;
    if (out_builds) *out_builds = ctx->beam_cache.list_builds;
    return BLOK_OK;
}

// The packed list of the slot the latest rectangle launch counted for or walked packed from, as it lies in device memory once everything
// enqueued has finished: the areas' stretches, the sorted table and its length, and the trips of the latest count launch.
int blok_hip_beam_cache_download_list(blok_hip_ctx* ctx, int* out_state, uint32_t* out_n_areas, uint32_t* out_n_groups, uint32_t* out_list_host, size_t list_capacity,
                                      uint32_t* out_table_host, size_t table_capacity, uint8_t* out_trips_host, size_t trips_capacity) {
    if (!ctx) return BLOK_ERR_INVALID_ARG;
    const auto& B = ctx->beam_cache;
    if (out_state) *out_state = B.last_list;
    if (out_n_areas) *out_n_areas = 0u;
    if (out_n_groups) *out_n_groups = 0u;
    if (!B.last_list) return BLOK_OK;
    if (B.last_slot < 0 || static_cast<uint32_t>(B.last_slot) >= blok::kBeamCacheSlots || !B.slots[B.last_slot].d_list)
        return set_error(ctx, BLOK_ERR_INVALID_ARG, "beam cache: the latest launch's slot is gone (a resize)");
    const auto& sl = B.slots[B.last_slot];
    const uint32_t n_areas = sl.n_words / blok::kPackGroups;
    const size_t entries = static_cast<size_t>(n_areas) * blok::kPackStretch, pixels = static_cast<size_t>(B.last_w) * B.last_h;
    if (entries > B.list_capacity || sl.n_words > B.words_capacity || pixels > B.d_trips.capacity()) return set_error(ctx, BLOK_ERR_INVALID_ARG, "beam cache: the list's buffers are gone (a resize)");
    if ((out_list_host && list_capacity < entries) || (out_table_host && table_capacity < sl.n_words) || (out_trips_host && trips_capacity < pixels))
        return set_error(ctx, BLOK_ERR_INVALID_ARG, "beam cache: output smaller than the list, the table or the rectangle");
    if (out_n_areas) *out_n_areas = n_areas;
    if (!out_n_groups && !out_list_host && !out_table_host && !out_trips_host) return BLOK_OK;      // the state alone: waits for nothing
    BLOK_HIP_TRY(ctx, hipSetDevice(ctx->device));
    BLOK_HIP_TRY(ctx, hipDeviceSynchronize());
    if (out_n_groups) *out_n_groups = B.last_list == 2 ? sl.n_groups : std::min(B.h_groups[B.last_slot], sl.n_words);      // (a build just issued has finished by now)
    if (out_list_host) BLOK_HIP_TRY(ctx, hipMemcpy(out_list_host, sl.d_list, entries * sizeof(uint32_t), hipMemcpyDeviceToHost));
    if (out_table_host) BLOK_HIP_TRY(ctx, hipMemcpy(out_table_host, sl.d_table, sl.n_words * sizeof(uint32_t), hipMemcpyDeviceToHost));
    if (out_trips_host) BLOK_HIP_TRY(ctx, hipMemcpy(out_trips_host, B.d_trips, pixels, hipMemcpyDeviceToHost));
    return BLOK_OK;
}

// The starts of that slot's list, in list order, and the restarted trips of the latest count launch (mode 4).
int blok_hip_beam_cache_download_starts(blok_hip_ctx* ctx, int* out_state, float* out_starts_host, size_t starts_capacity, uint8_t* out_restarts_host, size_t restarts_capacity) {
    if (!ctx) return BLOK_ERR_INVALID_ARG;
    const auto& B = ctx->beam_cache;
    if (out_state) *out_state = B.last_starts;
    if (!out_starts_host && !out_restarts_host) return BLOK_OK;      // the state alone: waits for nothing
    if (!B.last_list || B.last_slot < 0 || static_cast<uint32_t>(B.last_slot) >= blok::kBeamCacheSlots || !B.policy.starts[B.last_slot] || !B.slots[B.last_slot].d_start)
        return set_error(ctx, BLOK_ERR_INVALID_ARG, "beam cache: the latest launch's slot has no list with starts");
    const auto& sl = B.slots[B.last_slot];
    const size_t entries = static_cast<size_t>(sl.n_words / blok::kPackGroups) * blok::kPackStretch, pixels = static_cast<size_t>(B.last_w) * B.last_h;
    if (entries > sl.d_start.capacity() || pixels > B.d_restarts.capacity()) return set_error(ctx, BLOK_ERR_INVALID_ARG, "beam cache: the starts' buffers are gone (a resize)");
    if ((out_starts_host && starts_capacity < entries) || (out_restarts_host && restarts_capacity < pixels))
        return set_error(ctx, BLOK_ERR_INVALID_ARG, "beam cache: output smaller than the list or the rectangle");
    BLOK_HIP_TRY(ctx, hipSetDevice(ctx->device));
    BLOK_HIP_TRY(ctx, hipDeviceSynchronize());
    if (out_starts_host) BLOK_HIP_TRY(ctx, hipMemcpy(out_starts_host, sl.d_start, entries * sizeof(float), hipMemcpyDeviceToHost));
    if (out_restarts_host) BLOK_HIP_TRY(ctx, hipMemcpy(out_restarts_host, B.d_restarts, pixels, hipMemcpyDeviceToHost));
    return BLOK_OK;
}

int blok_hip_beam_cache_start_counters(const blok_hip_ctx* ctx, uint64_t* out_from_starts, uint64_t* out_other_key) {
    if (!ctx) return BLOK_ERR_INVALID_ARG;
    if (out_from_starts) *out_from_starts = ctx->beam_cache.start_hits;
    if (out_other_key) *out_other_key = ctx->beam_cache.start_other_key;
    return BLOK_OK;
}

// The node words of that slot's list, in list order, and the per-pixel words of the latest count launch (mode 5).
int blok_hip_beam_cache_download_nodes(blok_hip_ctx* ctx, int* out_has_nodes, uint32_t* out_entry_words_host, size_t entry_capacity, uint32_t* out_pixel_words_host, size_t pixel_capacity) {
    if (!ctx) return BLOK_ERR_INVALID_ARG;
    const auto& B = ctx->beam_cache;
    const bool has = B.last_list && B.last_slot >= 0 && static_cast<uint32_t>(B.last_slot) < blok::kBeamCacheSlots && B.policy.starts[B.last_slot] && B.policy.nodes[B.last_slot] &&
                     B.slots[B.last_slot].d_node;
    if (out_has_nodes) *out_has_nodes = has ? 1 : 0;
    if (!out_entry_words_host && !out_pixel_words_host) return BLOK_OK;      // the state alone: waits for nothing
    if (!has) return set_error(ctx, BLOK_ERR_INVALID_ARG, "beam cache: the latest launch's slot has no list with node words");
    const auto& sl = B.slots[B.last_slot];
    const size_t entries = static_cast<size_t>(sl.n_words / blok::kPackGroups) * blok::kPackStretch, pixels = static_cast<size_t>(B.last_w) * B.last_h;
    if (entries > sl.d_node.capacity() || pixels > B.d_ray_node.capacity()) return set_error(ctx, BLOK_ERR_INVALID_ARG, "beam cache: the node words' buffers are gone (a resize)");
    if ((out_entry_words_host && entry_capacity < entries) || (out_pixel_words_host && pixel_capacity < pixels))
        return set_error(ctx, BLOK_ERR_INVALID_ARG, "beam cache: output smaller than the list or the rectangle");
    BLOK_HIP_TRY(ctx, hipSetDevice(ctx->device));
    BLOK_HIP_TRY(ctx, hipDeviceSynchronize());
    if (out_entry_words_host) BLOK_HIP_TRY(ctx, hipMemcpy(out_entry_words_host, sl.d_node, entries * sizeof(uint32_t), hipMemcpyDeviceToHost));
    if (out_pixel_words_host) BLOK_HIP_TRY(ctx, hipMemcpy(out_pixel_words_host, B.d_ray_node, pixels * sizeof(uint32_t), hipMemcpyDeviceToHost));
    return BLOK_OK;
}

int blok_hip_beam_cache_node_counters(const blok_hip_ctx* ctx, uint64_t* out_from_nodes) {
    if (!ctx) return BLOK_ERR_INVALID_ARG;
    if (out_from_nodes) *out_from_nodes = ctx->beam_cache.node_hits;
    return BLOK_OK;
}

int blok_hip_set_packed_fill(blok_hip_ctx* ctx, uint32_t units_per_wave) {
    if (!ctx) return BLOK_ERR_INVALID_ARG;
    ctx->beam_cache.packed_fill = units_per_wave;        // (read by the next launch; the lists and the bounds are the same for both forms)
    return BLOK_OK;
}

int blok_hip_packed_fill_counters(const blok_hip_ctx* ctx, uint64_t* out_one_launch_frames, uint64_t* out_fill_only_workgroups) {
    if (!ctx) return BLOK_ERR_INVALID_ARG;
    if (out_one_launch_frames) *out_one_launch_frames = ctx->beam_cache.one_launch_frames;
    if (out_fill_only_workgroups) *out_fill_only_workgroups = ctx->beam_cache.fill_only_workgroups;
    return BLOK_OK;
}

int blok_hip_beam_cache_counters(const blok_hip_ctx* ctx, uint64_t* out_hits, uint64_t* out_fills) {
    if (!ctx) return BLOK_ERR_INVALID_ARG;
    if (out_hits) *out_hits = ctx->beam_cache.hits;
    if (out_fills) *out_fills = ctx->beam_cache.fills;
    return BLOK_OK;
}

int blok_hip_set_beam_refine_after(blok_hip_ctx* ctx, uint32_t hits) {
    if (!ctx) return BLOK_ERR_INVALID_ARG;
    ctx->beam_cache.policy.refine_after = hits ? hits : blok::kBeamRefineAfter;
    return BLOK_OK;
}

int blok_hip_beam_cache_refines(const blok_hip_ctx* ctx, uint64_t* out_refines) {
    if (!ctx) return BLOK_ERR_INVALID_ARG;
    if (out_refines) *out_refines = ctx->beam_cache.refines;
    return BLOK_OK;
}

// What the latest rectangle launch did about the kept bounds and, where it filled or walked from a slot, that slot's floats as they lie
// in device memory once everything enqueued has finished.
int blok_hip_beam_cache_download(blok_hip_ctx* ctx, int* out_action, uint32_t* out_n_beams, float* out_t0_host, size_t capacity) {
    if (!ctx) return BLOK_ERR_INVALID_ARG;
    const auto& B = ctx->beam_cache;
    if (out_action) *out_action = B.last_action;
    if (out_n_beams) *out_n_beams = B.last_action ? B.last_n_beams : 0u;
    if (!out_t0_host || !B.last_action) return BLOK_OK;
    if (B.last_slot < 0 || static_cast<uint32_t>(B.last_slot) >= blok::kBeamCacheSlots || !B.slots[B.last_slot].d_beam || B.last_n_beams > B.capacity)
        return set_error(ctx, BLOK_ERR_INVALID_ARG, "beam cache: the latest launch's slot is gone (a resize)");
    if (capacity < B.last_n_beams) return set_error(ctx, BLOK_ERR_INVALID_ARG, "beam cache: output smaller than the launch's beam tiles");
    BLOK_HIP_TRY(ctx, hipSetDevice(ctx->device));
    BLOK_HIP_TRY(ctx, hipDeviceSynchronize());
    BLOK_HIP_TRY(ctx, hipMemcpy(out_t0_host, B.slots[B.last_slot].d_beam, B.last_n_beams * sizeof(float), hipMemcpyDeviceToHost));
    return BLOK_OK;
}

// The same for the slot's finer bounds.
int blok_hip_beam_cache_download_fine(blok_hip_ctx* ctx, int* out_state, uint32_t* out_n_tiles, float* out_t0_host, size_t capacity) {
    if (!ctx) return BLOK_ERR_INVALID_ARG;
    const auto& B = ctx->beam_cache;
    if (out_state) *out_state = B.last_fine;
    if (out_n_tiles) *out_n_tiles = B.last_n_fine;
    if (!out_t0_host || !B.last_fine) return BLOK_OK;
    if (B.last_slot < 0 || static_cast<uint32_t>(B.last_slot) >= blok::kBeamCacheSlots || !B.slots[B.last_slot].d_fine || B.last_n_fine > B.capacity)
        return set_error(ctx, BLOK_ERR_INVALID_ARG, "beam cache: the latest launch's slot is gone (a resize)");
    if (capacity < B.last_n_fine) return set_error(ctx, BLOK_ERR_INVALID_ARG, "beam cache: output smaller than the launch's wave tiles");
    BLOK_HIP_TRY(ctx, hipSetDevice(ctx->device));
    BLOK_HIP_TRY(ctx, hipDeviceSynchronize());
    BLOK_HIP_TRY(ctx, hipMemcpy(out_t0_host, B.slots[B.last_slot].d_fine, B.last_n_fine * sizeof(float), hipMemcpyDeviceToHost));
    return BLOK_OK;
}

int blok_hip_set_beam_budget(blok_hip_ctx* ctx, uint32_t max_node_visits) {
    if (!ctx) return BLOK_ERR_INVALID_ARG;
    ctx->beam_budget = max_node_visits;
    return BLOK_OK;
}

}  // extern "C"
