// C ABI, device-resident dense voxel store (include/blok_hip.h: blok_hip_volume_*; kernels in gpu_build.hip).
#include "api_internal.h"
#include "../common/terrain_core.h"
#include "../common/stamp_core.h"
#include "../common/affine_core.h"
#include "../common/sweep_core.h"
#include "../common/bricks_core.h"
#include "../common/distance_core.h"
#include "../common/flood_core.h"
#include "../common/columns_core.h"
#include "../common/region_core.h"
#include "../common/scroll_core.h"
#include "../common/shapes_core.h"
#include "../common/lod_core.h"
#include "../common/terrain_lod_core.h"
#include "../common/automaton_core.h"
#include "../common/lights_core.h"
#include "device_mem.h"
#include <chrono>
#include <cstdlib>
#include <limits>

using namespace blok_api;

namespace blok_api {
void clear_lights(blok_hip_ctx* ctx) {
    if (ctx->lights.table) (void)hipDeviceSynchronize();      // frames that still sample it
    ctx->lights = blok_hip_ctx::Lights{};
    ctx->light_grid = blok_hip_ctx::LightGrid{};              // (a statement about that table)
}

void free_volume_snapshots(blok_hip_ctx* ctx) {
    blok::gpu_quads_free(&ctx->quads);
    blok::gpu_components_free(&ctx->components);
    blok::gpu_bricks_free(&ctx->bricks);
    blok::gpu_field_free(&ctx->distance);
    blok::gpu_field_free(&ctx->flood);
    blok::gpu_columns_free(&ctx->columns);
    blok::gpu_scatter_free(&ctx->scatter);
    blok::gpu_lod_free(&ctx->lod);
}

namespace {
// A holder whose region [lo, lo + ext) is box-local, behind a move of the box by `delta`: the corner follows when the region still lies
// wholly in the box of `dims`; false = it does not (the caller frees the holder).  A holder that was not taken stays as it is.
bool follow_box(bool taken, uint32_t lo[3], const uint32_t ext[3], const int32_t delta[3], const uint32_t dims[3]) {
    if (!taken) return true;
    int64_t l[3];
    for (int a = 0; a < 3; ++a) {
        l[a] = int64_t(lo[a]) - delta[a];
        if (l[a] < 0 || l[a] + int64_t(ext[a]) > int64_t(dims[a])) return false;
    }
    for (int a = 0; a < 3; ++a) lo[a] = static_cast<uint32_t>(l[a]);
    return true;
}
}  // namespace

// The snapshots behind a scroll of the box by `delta` (the volume still holds its dims).  They are of world cells: the quads hold no position
// and the brick stream holds its region in world voxels, so both stay; the holders with a box-local corner follow the box or are freed.
void scroll_volume_snapshots(blok_hip_ctx* ctx, const int32_t delta[3]) {
    const uint32_t dims[3] = {ctx->volume.nx, ctx->volume.ny, ctx->volume.nz};
    if (!follow_box(ctx->components.taken, ctx->components.lo, ctx->components.ext, delta, dims)) blok::gpu_components_free(&ctx->components);
    if (!follow_box(ctx->distance.taken, ctx->distance.lo, ctx->distance.info.ext, delta, dims)) blok::gpu_field_free(&ctx->distance);
    if (!follow_box(ctx->flood.taken, ctx->flood.lo, ctx->flood.info.ext, delta, dims)) blok::gpu_field_free(&ctx->flood);
    if (!follow_box(ctx->columns.taken, ctx->columns.lo, ctx->columns.info.ext, delta, dims)) {
        blok::gpu_columns_free(&ctx->columns);
        blok::gpu_scatter_free(&ctx->scatter);                 // (made from the snapshot that has just gone)
    }
}
}  // namespace blok_api

extern "C" {

namespace {
int volume_status(blok_hip_ctx* ctx, blok::GpuBuildStatus st, const std::string& why) {
    switch (st) {
        case blok::GpuBuildStatus::Ok: return BLOK_OK;
        case blok::GpuBuildStatus::Unsupported: return set_error(ctx, BLOK_ERR_UNSUPPORTED, why);
        case blok::GpuBuildStatus::OutOfMemory: return set_error(ctx, BLOK_ERR_OOM, why);
        case blok::GpuBuildStatus::HipError: return set_error(ctx, BLOK_ERR_HIP, why);
        case blok::GpuBuildStatus::Internal: return set_error(ctx, BLOK_ERR_INTERNAL, why);
        default: return set_error(ctx, BLOK_ERR_INVALID_ARG, why.empty() ? "volume operation not applicable" : why);
    }
}
int need_volume(blok_hip_ctx* ctx) {
    if (!ctx) return BLOK_ERR_INVALID_ARG;
    if (!ctx->has_volume) return set_error(ctx, BLOK_ERR_NO_WORLD, "no resident volume (blok_hip_volume_create)");
    BLOK_HIP_TRY(ctx, hipSetDevice(ctx->device));
    return BLOK_OK;
}
// A table that has passed check_instance_table: BLOK_ERR_UNSUPPORTED if any of its models has a scale (nothing has been touched yet).
int refuse_scaled_table(blok_hip_ctx* ctx, const char* op, const blok_instance* placements, uint32_t n) {
    for (uint32_t i = 0; i < n; ++i) {
        const int rc = refuse_scaled_model(ctx, op, placements[i].model);
        if (rc != BLOK_OK) return rc;
    }
    return BLOK_OK;
}
// The models of a table that has passed check_instance_table, as the stamp and the sweep read them.
std::vector<blok::StampModel> placed_models(const blok_hip_ctx* ctx, const blok_instance* placements, uint32_t n) {
    std::vector<blok::StampModel> models(n);
    for (uint32_t i = 0; i < n; ++i) {
        const blok::ModelDesc& d = ctx->models.desc[placements[i].model];
        blok::StampModel& m = models[i];
        m.nodes = d.nodes; m.materials = d.materials; m.levels = d.levels;
        for (int a = 0; a < 3; ++a) { m.origin[a] = d.origin[a]; m.lo[a] = d.lo[a]; m.hi[a] = d.hi[a]; }
    }
    return models;
}
// The box-local region [lo, hi) of an entry's world region_lo / region_hi (both null: the whole box), with the entry's name in the messages.
int volume_region(blok_hip_ctx* ctx, const char* op, const int32_t* region_lo, const int32_t* region_hi, uint32_t lo[3], uint32_t hi[3]) {
    static const char* const kText[] = {"", ": one region pointer is null", ": region_lo above region_hi", ": region leaves the resident volume"};
    const blok::GpuVolume& v = ctx->volume;
    const uint32_t dims[3] = {v.nx, v.ny, v.nz};
    const int rule = blok::region::local(v.origin, dims, region_lo, region_hi, lo, hi);
    return rule ? set_error(ctx, blok::region::status(rule), std::string(op) + kText[rule]) : BLOK_OK;
}
// A tree built on the device (gpu_volume_capture*) into the model store; box_lo / box_hi: the box of its voxels, model coordinates.
int add_captured_model(blok_hip_ctx* ctx, const blok::GpuTree& tree, const int32_t box_lo[3], const int32_t box_hi[3], uint32_t* out_model) {
    blok::ModelDesc m{};
    m.nodes = tree.d_nodes; m.materials = tree.d_materials; m.levels = tree.levels;
    for (int a = 0; a < 3; ++a) { m.origin[a] = tree.origin[a]; m.lo[a] = box_lo[a]; m.hi[a] = box_hi[a]; }
    blok_hip_ctx::Models::Arrays own;
    own.n_nodes = static_cast<uint32_t>(tree.n_nodes); own.n_materials = static_cast<uint32_t>(tree.n_voxels);
    own.nodes.adopt(tree.d_nodes, tree.n_nodes); own.materials.adopt(tree.d_materials, tree.n_voxels);
    return add_model(ctx, m, std::move(own), out_model);
}
// Lets go of the present volume, if there is one, and of the world installed from its arrays (it lives in them: it goes with them).  strict:
// a failing wait for the frames that still read that world is the call's failure, and nothing is freed.
int release_volume(blok_hip_ctx* ctx, bool strict) {
    if (!ctx->has_volume) return BLOK_OK;
    if (ctx->tree_owned_by_volume) {
        if (strict) BLOK_HIP_TRY(ctx, hipDeviceSynchronize()); else (void)hipDeviceSynchronize();
        free_world(ctx);
    }
    blok::gpu_volume_destroy(&ctx->volume); ctx->has_volume = false;
    return BLOK_OK;
}
// Elements [first, first + count) of a snapshot's array of n elements of elem_bytes each, to host memory: the tail of every *_download entry
// (`entry`, with the call that takes its snapshot in the message), behind its null-context check.
int ranged_download(blok_hip_ctx* ctx, const char* entry, const char* taken_by, bool taken, uint64_t n, const void* base, size_t elem_bytes,
                    void* out_host, uint64_t first, uint64_t count) {
    if (!taken) return set_error(ctx, BLOK_ERR_INVALID_ARG, std::string(entry) + ": no snapshot (" + taken_by + ")");
    if (first > n || count > n - first) return set_error(ctx, BLOK_ERR_INVALID_ARG, std::string(entry) + ": range past the end of the snapshot");
    if (count == 0) return BLOK_OK;
    if (!out_host) return set_error(ctx, BLOK_ERR_INVALID_ARG, std::string(entry) + ": null output");
    BLOK_HIP_TRY(ctx, hipSetDevice(ctx->device));
    BLOK_HIP_TRY(ctx, hipMemcpy(out_host, static_cast<const char*>(base) + first * elem_bytes, count * elem_bytes, hipMemcpyDeviceToHost));
    return BLOK_OK;
}
uint64_t field_cells(const uint32_t ext[3]) { return static_cast<uint64_t>(ext[0]) * ext[1] * ext[2]; }
}  // namespace

int blok_hip_volume_create(blok_hip_ctx* ctx, const int32_t origin[3], uint32_t nx, uint32_t ny, uint32_t nz,
                           uint32_t chunk_size, float voxel_size) {
    if (!ctx) return BLOK_ERR_INVALID_ARG;
    BLOK_HIP_TRY(ctx, hipSetDevice(ctx->device));
    const int rc = release_volume(ctx, true);
    if (rc != BLOK_OK) return rc;
    free_volume_snapshots(ctx);
    const int32_t o[3] = {origin ? origin[0] : 0, origin ? origin[1] : 0, origin ? origin[2] : 0};
    std::string why;
    const blok::GpuBuildStatus st = blok::gpu_volume_create(o, nx, ny, nz, chunk_size, voxel_size, &ctx->volume, &why, ctx->volume_keyed_layout);
    ctx->has_volume = st == blok::GpuBuildStatus::Ok;
    return volume_status(ctx, st, why);
}

int blok_hip_set_volume_layout(blok_hip_ctx* ctx, int keyed) {
    if (!ctx) return BLOK_ERR_INVALID_ARG;
    ctx->volume_keyed_layout = keyed != 0;
    return BLOK_OK;
}

int blok_hip_volume_refresh_counts(blok_hip_ctx* ctx, uint64_t out_counts[3]) {
    int rc = need_volume(ctx);
    if (rc != BLOK_OK) return rc;
    if (!out_counts) return set_error(ctx, BLOK_ERR_INVALID_ARG, "null output");
    for (int i = 0; i < 3; ++i) out_counts[i] = ctx->volume.refreshes[i];
    return BLOK_OK;
}

int blok_hip_volume_destroy(blok_hip_ctx* ctx) {
    if (!ctx) return BLOK_ERR_INVALID_ARG;
    if (ctx->has_volume) (void)hipSetDevice(ctx->device);
    (void)release_volume(ctx, false);
    free_volume_snapshots(ctx);
    return BLOK_OK;
}

int blok_hip_volume_upload(blok_hip_ctx* ctx, const float* density, const uint32_t* material_ids) {
    int rc = need_volume(ctx);
    if (rc != BLOK_OK) return rc;
    std::string why;
    return volume_status(ctx, blok::gpu_volume_upload(&ctx->volume, density, material_ids, &why), why);
}

int blok_hip_volume_download(blok_hip_ctx* ctx, float* density, uint32_t* material_ids) {
    int rc = need_volume(ctx);
    if (rc != BLOK_OK) return rc;
    std::string why;
    return volume_status(ctx, blok::gpu_volume_download(&ctx->volume, density, material_ids, &why), why);
}

int blok_hip_volume_set_voxels(blok_hip_ctx* ctx, const int32_t* xyz, const uint32_t* material_ids, const float* density, size_t n) {
    int rc = need_volume(ctx);
    if (rc != BLOK_OK) return rc;
    if (n && !xyz) return set_error(ctx, BLOK_ERR_INVALID_ARG, "null voxel list");
    std::string why;
    return volume_status(ctx, blok::gpu_volume_set_voxels(&ctx->volume, xyz, material_ids, density, n, &why), why);
}

int blok_hip_volume_apply_brush(blok_hip_ctx* ctx, const float center[3], float radius, float value, int mode) {
    int rc = need_volume(ctx);
    if (rc != BLOK_OK) return rc;
    if (!center || (mode != 0 && mode != 1) || !(radius >= 0.0f)) return set_error(ctx, BLOK_ERR_INVALID_ARG, "bad brush arguments");
    std::string why;
    // enqueued on the null stream, like the rebuild that follows it: nothing waits here (a failing kernel shows at the next call that does)
    return volume_status(ctx, blok::gpu_volume_brush(&ctx->volume, center, radius, value, mode, &why), why);
}

int blok_hip_volume_voxelize_mesh(blok_hip_ctx* ctx, const float* positions, size_t n_vertices, const uint32_t* triangles, size_t n_triangles,
                                  const uint32_t* triangle_materials, uint32_t material, float density, int mode, uint64_t* out_n_voxels) {
    if (out_n_voxels) *out_n_voxels = 0;
    int rc = need_volume(ctx);
    if (rc != BLOK_OK) return rc;
    if ((n_vertices && !positions) || (n_triangles && !triangles)) return set_error(ctx, BLOK_ERR_INVALID_ARG, "voxelize: null array with a non-zero count");
    if (!std::isfinite(density) || !(density > 0.0f)) return set_error(ctx, BLOK_ERR_INVALID_ARG, "voxelize: density must be finite and > 0");
    if (mode != BLOK_VOXELIZE_SURFACE && mode != BLOK_VOXELIZE_SOLID) return set_error(ctx, BLOK_ERR_INVALID_ARG, "voxelize: unknown mode");
    std::string why;
    bool invalid = false;
    const blok::GpuBuildStatus st = blok::gpu_volume_voxelize(&ctx->volume, positions, n_vertices, triangles, n_triangles, triangle_materials, material, density,
                                                               mode == BLOK_VOXELIZE_SOLID, out_n_voxels, &invalid, &why);
    if (invalid) return set_error(ctx, BLOK_ERR_INVALID_ARG, why);
    return volume_status(ctx, st, why);
}

int blok_hip_volume_generate_terrain(blok_hip_ctx* ctx, const blok_terrain_params* params, const int32_t region_lo[3], const int32_t region_hi[3],
                                     uint64_t* out_n_voxels) {
    if (out_n_voxels) *out_n_voxels = 0;
    int rc = need_volume(ctx);
    if (rc != BLOK_OK) return rc;
    if (!params) return set_error(ctx, BLOK_ERR_INVALID_ARG, "generate_terrain: null parameters");
    static const char* const kRules[] = {"", "height octaves / cell", "cave octaves / cell", "ore cell", "a threshold above 65536", "amplitude above 65536",
                                         "|base_height| above 2^24", "density not finite or <= 0", "unknown flag bits", "CLOSE_SIDES without SHELL"};
    if (const int rule = blok::terrain::check_params(*params)) return set_error(ctx, BLOK_ERR_INVALID_ARG, std::string("generate_terrain: ") + kRules[rule]);
    uint32_t lo[3], hi[3];
    rc = volume_region(ctx, "generate_terrain", region_lo, region_hi, lo, hi);
    if (rc != BLOK_OK) return rc;
    std::string why;
    return volume_status(ctx, blok::gpu_volume_generate_terrain(&ctx->volume, *params, lo, hi, out_n_voxels, &why), why);
}

int blok_hip_volume_extract_quads(blok_hip_ctx* ctx, const int32_t region_lo[3], const int32_t region_hi[3], uint32_t flags,
                                  uint64_t* out_n_quads, uint64_t* out_n_faces) {
    if (out_n_quads) *out_n_quads = 0;
    if (out_n_faces) *out_n_faces = 0;
    int rc = need_volume(ctx);
    if (rc != BLOK_OK) return rc;
    if (flags & ~(BLOK_QUADS_IGNORE_MATERIAL | BLOK_QUADS_COUNT_ONLY)) return set_error(ctx, BLOK_ERR_INVALID_ARG, "extract_quads: unknown flag bits");
    uint32_t lo[3], hi[3];
    rc = volume_region(ctx, "extract_quads", region_lo, region_hi, lo, hi);
    if (rc != BLOK_OK) return rc;
    std::string why;
    blok::GpuQuads snapshot;
    uint64_t n_faces = 0;
    // (edits are enqueued on the null stream, and so is this: it reads what they leave)
    const blok::GpuBuildStatus st = blok::gpu_volume_extract_quads(&ctx->volume, lo, hi, flags, &snapshot, &n_faces, &why);
    if (st != blok::GpuBuildStatus::Ok) return volume_status(ctx, st, why);
    if (!(flags & BLOK_QUADS_COUNT_ONLY)) {
        blok::gpu_quads_free(&ctx->quads);
        ctx->quads = snapshot; ctx->quads.taken = true; ctx->quads.flags = flags;      // (blok_hip_lights_from_quads asks whether the keys are material ids)
    }
    if (out_n_quads) *out_n_quads = snapshot.n_quads;
    if (out_n_faces) *out_n_faces = n_faces;
    return BLOK_OK;
}

int blok_hip_volume_quads_download(blok_hip_ctx* ctx, blok_quad* out_host, uint64_t first, uint64_t count) {
    if (!ctx) return BLOK_ERR_INVALID_ARG;
    const blok::GpuQuads& q = ctx->quads;
    return ranged_download(ctx, "quads_download", "blok_hip_volume_extract_quads", q.taken, q.n_quads, q.d_quads, sizeof(blok_quad), out_host, first, count);
}

int blok_hip_volume_stamp_models(blok_hip_ctx* ctx, const blok_instance* placements_host, uint32_t n_placements, int mode, float density,
                                 uint64_t* out_n_voxels) {
    if (out_n_voxels) *out_n_voxels = 0;
    int rc = need_volume(ctx);
    if (rc != BLOK_OK) return rc;
    rc = check_instance_table(ctx, placements_host, n_placements);
    if (rc == BLOK_OK) rc = refuse_scaled_table(ctx, "stamp_models", placements_host, n_placements);
    if (rc != BLOK_OK) return rc;
    if (!blok::stamp::mode_known(mode)) return set_error(ctx, BLOK_ERR_INVALID_ARG, "stamp_models: unknown mode");
    if (mode != BLOK_STAMP_ERASE && (!std::isfinite(density) || !(density > 0.0f)))
        return set_error(ctx, BLOK_ERR_INVALID_ARG, "stamp_models: density must be finite and > 0");
    const std::vector<blok::StampModel> models = placed_models(ctx, placements_host, n_placements);
    std::string why;
    // (edits are enqueued on the null stream, and so is this: placement after placement, in stream order)
    return volume_status(ctx, blok::gpu_volume_stamp(&ctx->volume, models.data(), placements_host, n_placements, mode, density, out_n_voxels, &why), why);
}

int blok_hip_volume_stamp_affine(blok_hip_ctx* ctx, const blok_affine* table_host, uint32_t n, const int32_t region_lo[3],
                                 const int32_t region_hi[3], int mode, float density, uint64_t* out_n_voxels) {
    if (out_n_voxels) *out_n_voxels = 0;
    int rc = need_volume(ctx);
    if (rc != BLOK_OK) return rc;
    if (n && !table_host) return set_error(ctx, BLOK_ERR_INVALID_ARG, "stamp_affine: null table with a non-zero count");
    const blok::GpuVolume& v = ctx->volume;
    const uint32_t dims[3] = {v.nx, v.ny, v.nz};
    // the one volume entry that takes a model of any scale exponent: the exponent is not looked at, the box is the model's own
    std::vector<blok::StampModel> models(n);
    for (uint32_t i = 0; i < n; ++i) {
        const uint32_t model = table_host[i].model;
        if (!known_model(ctx, model))
            return set_error(ctx, BLOK_ERR_INVALID_ARG, "stamp_affine: record " + std::to_string(i) + ": unknown model " + std::to_string(model));
        if (const int rule = blok::affine::well_formed(table_host[i], v.origin, dims))
            return set_error(ctx, BLOK_ERR_INVALID_ARG, "stamp_affine: record " + std::to_string(i) + ": " + blok::affine::rule_text(rule));
        const blok::ModelDesc& d = ctx->models.desc[model];
        const auto& own = ctx->models.own[model];
        blok::StampModel& m = models[i];
        m.nodes = d.nodes; m.materials = d.materials; m.levels = d.levels;
        for (int a = 0; a < 3; ++a) { m.origin[a] = d.origin[a]; m.lo[a] = own.box_lo[a]; m.hi[a] = own.box_hi[a]; }
    }
    if (!blok::stamp::mode_known(mode)) return set_error(ctx, BLOK_ERR_INVALID_ARG, "stamp_affine: unknown mode");
    if (mode != BLOK_STAMP_ERASE && (!std::isfinite(density) || !(density > 0.0f)))
        return set_error(ctx, BLOK_ERR_INVALID_ARG, "stamp_affine: density must be finite and > 0");
    uint32_t lo[3], hi[3];
    rc = volume_region(ctx, "stamp_affine", region_lo, region_hi, lo, hi);
    if (rc != BLOK_OK) return rc;
    std::string why;
    // (edits are enqueued on the null stream, and so is this: record after record, in stream order)
    return volume_status(ctx, blok::gpu_volume_stamp_affine(&ctx->volume, models.data(), table_host, n, lo, hi, mode, density, out_n_voxels, &why), why);
}

int blok_hip_volume_apply_shapes(blok_hip_ctx* ctx, const blok_shape* shapes_host, uint32_t n_shapes, uint64_t* out_n_written) {
    if (out_n_written) *out_n_written = 0;
    int rc = need_volume(ctx);
    if (rc != BLOK_OK) return rc;
    if (n_shapes > BLOK_SHAPES_MAX) return set_error(ctx, BLOK_ERR_INVALID_ARG, "apply_shapes: more than BLOK_SHAPES_MAX shapes");
    if (n_shapes && !shapes_host) return set_error(ctx, BLOK_ERR_INVALID_ARG, "apply_shapes: null table with a non-zero count");
    for (uint32_t i = 0; i < n_shapes; ++i)
        if (const int rule = blok::shapes::check(shapes_host[i]))
            return set_error(ctx, BLOK_ERR_INVALID_ARG, "apply_shapes: shape " + std::to_string(i) + ": " + blok::shapes::rule_text(rule));
    std::string why;
    // (edits are enqueued on the null stream, and so is this: it reads what they leave)
    return volume_status(ctx, blok::gpu_volume_apply_shapes(&ctx->volume, shapes_host, n_shapes, out_n_written, &why), why);
}

int blok_hip_volume_capture_model(blok_hip_ctx* ctx, const int32_t region_lo[3], const int32_t region_hi[3], uint32_t flags, uint32_t* out_model,
                                  uint64_t* out_n_voxels) {
    if (out_n_voxels) *out_n_voxels = 0;
    int rc = need_volume(ctx);
    if (rc != BLOK_OK) return rc;
    if (flags & ~BLOK_CAPTURE_CUT) return set_error(ctx, BLOK_ERR_INVALID_ARG, "capture_model: unknown flag bits");
    if (!out_model) return set_error(ctx, BLOK_ERR_INVALID_ARG, "capture_model: null output id");
    uint32_t lo[3], hi[3];
    rc = volume_region(ctx, "capture_model", region_lo, region_hi, lo, hi);
    if (rc != BLOK_OK) return rc;
    if (ctx->models.desc.size() >= std::numeric_limits<uint32_t>::max() - 1u) return set_error(ctx, BLOK_ERR_INVALID_ARG, "model ids exhausted");
    blok::GpuVolume& v = ctx->volume;
    std::string why;
    blok::GpuTree tree;
    int32_t box_lo[3] = {0, 0, 0}, box_hi[3] = {0, 0, 0};
    uint64_t n_voxels = 0;
    const blok::GpuBuildStatus st = blok::gpu_volume_capture(&v, lo, hi, &tree, box_lo, box_hi, &n_voxels, &why);
    if (st != blok::GpuBuildStatus::Ok) return volume_status(ctx, st, why);
    if (!n_voxels) return set_error(ctx, BLOK_ERR_UNSUPPORTED, "capture_model: the region holds no filled voxel");
    rc = add_captured_model(ctx, tree, box_lo, box_hi, out_model);
    if (rc != BLOK_OK) return rc;                      // (nothing is cut when there is no model)
    if (out_n_voxels) *out_n_voxels = n_voxels;
    if (flags & BLOK_CAPTURE_CUT) {
        // the captured voxels are the filled voxels of the region, and all of them lie in the model's box
        uint32_t clo[3], chi[3];
        for (int a = 0; a < 3; ++a) { clo[a] = lo[a] + static_cast<uint32_t>(box_lo[a]); chi[a] = lo[a] + static_cast<uint32_t>(box_hi[a]); }
        return volume_status(ctx, blok::gpu_volume_clear_filled(&v, clo, chi, &why), why);
    }
    return BLOK_OK;
}

int blok_hip_volume_label_components(blok_hip_ctx* ctx, const int32_t region_lo[3], const int32_t region_hi[3], uint32_t flags,
                                     uint64_t* out_n_components, uint64_t* out_n_voxels) {
    if (out_n_components) *out_n_components = 0;
    if (out_n_voxels) *out_n_voxels = 0;
    int rc = need_volume(ctx);
    if (rc != BLOK_OK) return rc;
    if (flags) return set_error(ctx, BLOK_ERR_INVALID_ARG, "label_components: unknown flag bits");
    uint32_t lo[3], hi[3];
    rc = volume_region(ctx, "label_components", region_lo, region_hi, lo, hi);
    if (rc != BLOK_OK) return rc;
    std::string why;
    blok::GpuComponents snapshot;
    const blok::GpuBuildStatus st = blok::gpu_volume_label_components(&ctx->volume, lo, hi, &snapshot, &why);
    if (st != blok::GpuBuildStatus::Ok) return volume_status(ctx, st, why);
    blok::gpu_components_free(&ctx->components);
    ctx->components = snapshot; ctx->components.taken = true;
    if (out_n_components) *out_n_components = snapshot.n_components;
    if (out_n_voxels) *out_n_voxels = snapshot.n_voxels;
    return BLOK_OK;
}

int blok_hip_volume_components_download(blok_hip_ctx* ctx, blok_component* out_host, uint64_t first, uint64_t count) {
    if (!ctx) return BLOK_ERR_INVALID_ARG;
    const blok::GpuComponents& c = ctx->components;
    return ranged_download(ctx, "components_download", "blok_hip_volume_label_components", c.taken, c.n_components, c.d_records, sizeof(blok_component), out_host, first, count);
}

int blok_hip_volume_labels_download(blok_hip_ctx* ctx, uint32_t* out_host, uint64_t first, uint64_t count) {
    if (!ctx) return BLOK_ERR_INVALID_ARG;
    const blok::GpuComponents& c = ctx->components;
    return ranged_download(ctx, "labels_download", "blok_hip_volume_label_components", c.taken, c.n_cells, c.d_labels, sizeof(uint32_t), out_host, first, count);
}

int blok_hip_volume_capture_component(blok_hip_ctx* ctx, uint32_t label, uint32_t flags, uint32_t* out_model, int32_t out_origin[3],
                                      uint64_t* out_n_voxels) {
    if (out_n_voxels) *out_n_voxels = 0;
    int rc = need_volume(ctx);
    if (rc != BLOK_OK) return rc;
    if (flags & ~BLOK_COMPONENT_CUT) return set_error(ctx, BLOK_ERR_INVALID_ARG, "capture_component: unknown flag bits");
    if (!out_model) return set_error(ctx, BLOK_ERR_INVALID_ARG, "capture_component: null output id");
    if (!ctx->components.taken) return set_error(ctx, BLOK_ERR_INVALID_ARG, "capture_component: no snapshot (blok_hip_volume_label_components)");
    if (ctx->models.desc.size() >= std::numeric_limits<uint32_t>::max() - 1u) return set_error(ctx, BLOK_ERR_INVALID_ARG, "model ids exhausted");
    std::string why;
    blok_component rec{};
    bool found = false;
    blok::GpuBuildStatus st = blok::gpu_components_find(&ctx->components, label, &rec, &found, &why);
    if (st != blok::GpuBuildStatus::Ok) return volume_status(ctx, st, why);
    if (!found) return set_error(ctx, BLOK_ERR_INVALID_ARG, "capture_component: no component of the snapshot has this label");
    blok::GpuVolume& v = ctx->volume;
    uint32_t lo[3], hi[3];                             // the record's box, box-local: inside the labelled region, which lies inside the box
    for (int a = 0; a < 3; ++a) { lo[a] = static_cast<uint32_t>(rec.lo[a] - v.origin[a]); hi[a] = static_cast<uint32_t>(rec.hi[a] - v.origin[a]); }
    blok::GpuTree tree;
    int32_t box_lo[3] = {0, 0, 0}, box_hi[3] = {0, 0, 0};
    uint64_t n_voxels = 0;
    st = blok::gpu_volume_capture_labelled(&v, &ctx->components, label, lo, hi, &tree, box_lo, box_hi, &n_voxels, &why);
    if (st != blok::GpuBuildStatus::Ok) return volume_status(ctx, st, why);
    if (!n_voxels) return set_error(ctx, BLOK_ERR_UNSUPPORTED, "capture_component: none of the component's voxels is still filled");
    rc = add_captured_model(ctx, tree, box_lo, box_hi, out_model);
    if (rc != BLOK_OK) return rc;                      // (nothing is cut when there is no model)
    if (out_n_voxels) *out_n_voxels = n_voxels;
    if (out_origin) for (int a = 0; a < 3; ++a) out_origin[a] = rec.lo[a];
    if (flags & BLOK_COMPONENT_CUT) return volume_status(ctx, blok::gpu_volume_clear_labelled(&v, &ctx->components, label, lo, hi, &why), why);
    return BLOK_OK;
}

int blok_hip_volume_sweep_models(blok_hip_ctx* ctx, const blok_instance* placements_host, uint32_t n_placements, uint32_t direction,
                                 uint32_t max_distance, uint32_t flags, blok_sweep_result* out_results_host) {
    int rc = need_volume(ctx);
    if (rc != BLOK_OK) return rc;
    rc = check_instance_table(ctx, placements_host, n_placements);      // the stamp's check, with its messages
    if (rc == BLOK_OK) rc = refuse_scaled_table(ctx, "sweep_models", placements_host, n_placements);
    if (rc != BLOK_OK) return rc;
    if (!blok::sweep::direction_known(direction)) return set_error(ctx, BLOK_ERR_INVALID_ARG, "sweep_models: direction above 5");
    if (!blok::sweep::flags_known(flags)) return set_error(ctx, BLOK_ERR_INVALID_ARG, "sweep_models: unknown flag bits");
    if (n_placements && !out_results_host) return set_error(ctx, BLOK_ERR_INVALID_ARG, "sweep_models: null result array with non-zero count");
    const std::vector<blok::StampModel> models = placed_models(ctx, placements_host, n_placements);
    std::string why;
    // (on the null stream, behind every edit enqueued so far; reads only, so no snapshot and no edit state is touched)
    return volume_status(ctx, blok::gpu_volume_sweep(&ctx->volume, models.data(), placements_host, n_placements, direction, max_distance, flags,
                                                     out_results_host, &why), why);
}

namespace {
// The box-local corner of a stream's destination [dst_lo, dst_lo + ext) (dst_lo null: where the stream was taken).
int bricks_destination(blok_hip_ctx* ctx, const char* op, const blok_bricks_info& info, const int32_t* dst_lo, uint32_t lo[3]) {
    const blok::GpuVolume& v = ctx->volume;
    const int64_t dims[3] = {v.nx, v.ny, v.nz};
    for (int a = 0; a < 3; ++a) {
        const int64_t l = int64_t(dst_lo ? dst_lo[a] : info.lo[a]) - v.origin[a];
        if (l < 0 || l + int64_t(info.ext[a]) > dims[a]) return set_error(ctx, BLOK_ERR_UNSUPPORTED, std::string(op) + ": destination leaves the resident volume");
        lo[a] = static_cast<uint32_t>(l);
    }
    return BLOK_OK;
}
}  // namespace

int blok_hip_volume_encode_bricks(blok_hip_ctx* ctx, const int32_t region_lo[3], const int32_t region_hi[3], uint32_t flags, blok_bricks_info* out_info) {
    int rc = need_volume(ctx);
    if (rc != BLOK_OK) return rc;
    if (flags & ~blok::bricks::kEncodeFlags) return set_error(ctx, BLOK_ERR_INVALID_ARG, "encode_bricks: unknown flag bits");
    uint32_t lo[3], hi[3];
    rc = volume_region(ctx, "encode_bricks", region_lo, region_hi, lo, hi);
    if (rc != BLOK_OK) return rc;
    std::string why;
    blok::GpuBricks snapshot;
    // (edits are enqueued on the null stream, and so is this: it reads what they leave)
    const blok::GpuBuildStatus st = blok::gpu_volume_encode_bricks(&ctx->volume, lo, hi, flags, &snapshot, &why);
    if (st != blok::GpuBuildStatus::Ok) return volume_status(ctx, st, why);
    blok::gpu_bricks_free(&ctx->bricks);
    ctx->bricks = snapshot; ctx->bricks.taken = true;
    if (out_info) *out_info = snapshot.info;
    return BLOK_OK;
}

int blok_hip_volume_bricks_info(blok_hip_ctx* ctx, blok_bricks_info* out_info) {
    if (!ctx) return BLOK_ERR_INVALID_ARG;
    if (!ctx->bricks.taken) return set_error(ctx, BLOK_ERR_INVALID_ARG, "bricks_info: no snapshot (blok_hip_volume_encode_bricks)");
    if (!out_info) return set_error(ctx, BLOK_ERR_INVALID_ARG, "bricks_info: null output");
    *out_info = ctx->bricks.info;
    return BLOK_OK;
}

int blok_hip_volume_bricks_download(blok_hip_ctx* ctx, blok_brick_record* out_host, uint64_t first, uint64_t count) {
    if (!ctx) return BLOK_ERR_INVALID_ARG;
    const blok::GpuBricks& b = ctx->bricks;
    return ranged_download(ctx, "bricks_download", "blok_hip_volume_encode_bricks", b.taken, b.info.n_bricks, b.d_records, sizeof(blok_brick_record), out_host, first, count);
}

int blok_hip_volume_brick_payload_download(blok_hip_ctx* ctx, uint32_t plane, uint32_t* out_u32_host, uint64_t first, uint64_t count) {
    if (!ctx) return BLOK_ERR_INVALID_ARG;
    const blok::GpuBricks& b = ctx->bricks;
    if (b.taken && plane > 1u) return set_error(ctx, BLOK_ERR_INVALID_ARG, "brick_payload_download: plane above 1");
    return ranged_download(ctx, "brick_payload_download", "blok_hip_volume_encode_bricks", b.taken, plane == 0u ? b.info.n_density : b.info.n_material,
                           plane == 0u ? b.d_density : b.d_material, sizeof(uint32_t), out_u32_host, first, count);
}

int blok_hip_volume_restore_bricks(blok_hip_ctx* ctx, const int32_t dst_lo[3], uint32_t flags) {
    int rc = need_volume(ctx);
    if (rc != BLOK_OK) return rc;
    if (flags & ~blok::bricks::kDecodeFlags) return set_error(ctx, BLOK_ERR_INVALID_ARG, "restore_bricks: unknown flag bits");
    if (!ctx->bricks.taken) return set_error(ctx, BLOK_ERR_INVALID_ARG, "restore_bricks: no snapshot (blok_hip_volume_encode_bricks)");
    uint32_t lo[3];
    rc = bricks_destination(ctx, "restore_bricks", ctx->bricks.info, dst_lo, lo);
    if (rc != BLOK_OK) return rc;
    std::string why;
    return volume_status(ctx, blok::gpu_volume_decode_bricks(&ctx->volume, &ctx->bricks, lo, flags, &why), why);
}

int blok_hip_volume_decode_bricks(blok_hip_ctx* ctx, const blok_bricks_info* info, const blok_brick_record* records, const uint32_t* density_payload,
                                  const uint32_t* material_payload, const int32_t dst_lo[3], uint32_t flags) {
    int rc = need_volume(ctx);
    if (rc != BLOK_OK) return rc;
    if (flags & ~blok::bricks::kDecodeFlags) return set_error(ctx, BLOK_ERR_INVALID_ARG, "decode_bricks: unknown flag bits");
    if (!info) return set_error(ctx, BLOK_ERR_INVALID_ARG, "decode_bricks: null info");
    // on the host, before anything is uploaded or written
    uint64_t bad = 0;
    if (const int rule = blok::bricks::validate(*info, records, density_payload, material_payload, &bad)) {
        std::string msg = std::string("decode_bricks: ") + blok::bricks::rule_text(rule);
        if (bad < info->n_bricks) msg += " (record " + std::to_string(bad) + ")";
        return set_error(ctx, BLOK_ERR_INVALID_ARG, msg);
    }
    uint32_t lo[3];
    rc = bricks_destination(ctx, "decode_bricks", *info, dst_lo, lo);
    if (rc != BLOK_OK) return rc;
    std::string why_text;
    std::string* why = &why_text;
    blok::DeviceMem mem;
    blok::GpuBricks stream;
    stream.info = *info;
    const auto upload = [&]() -> blok::GpuBuildStatus {
        if (info->n_bricks) {
            BLOK_GPU_TRY(mem.alloc(&stream.d_records, info->n_bricks));
            BLOK_GPU_TRY(hipMemcpy(stream.d_records, records, info->n_bricks * sizeof(blok_brick_record), hipMemcpyHostToDevice));
        }
        if (info->n_density) {
            BLOK_GPU_TRY(mem.alloc(&stream.d_density, info->n_density));
            BLOK_GPU_TRY(hipMemcpy(stream.d_density, density_payload, info->n_density * sizeof(uint32_t), hipMemcpyHostToDevice));
        }
        if (info->n_material) {
            BLOK_GPU_TRY(mem.alloc(&stream.d_material, info->n_material));
            BLOK_GPU_TRY(hipMemcpy(stream.d_material, material_payload, info->n_material * sizeof(uint32_t), hipMemcpyHostToDevice));
        }
        return blok::GpuBuildStatus::Ok;
    };
    blok::GpuBuildStatus st = upload();
    if (st == blok::GpuBuildStatus::Ok) st = blok::gpu_volume_decode_bricks(&ctx->volume, &stream, lo, flags, why);      // (blocking: the arrays outlive the kernels)
    return volume_status(ctx, st, why_text);
}

int blok_hip_volume_distance_field(blok_hip_ctx* ctx, const int32_t region_lo[3], const int32_t region_hi[3], uint32_t max_radius, uint32_t flags,
                                   blok_distance_info* out_info) {
    int rc = need_volume(ctx);
    if (rc != BLOK_OK) return rc;
    if (const int rule = blok::distance::check_field_args(max_radius, flags)) return set_error(ctx, BLOK_ERR_INVALID_ARG, std::string("distance_field: ") + blok::distance::rule_text(rule));
    uint32_t lo[3], hi[3];
    rc = volume_region(ctx, "distance_field", region_lo, region_hi, lo, hi);
    if (rc != BLOK_OK) return rc;
    std::string why;
    blok::GpuDistance snapshot;
    // (edits are enqueued on the null stream, and so is this: it reads the masks they leave)
    const blok::GpuBuildStatus st = blok::gpu_volume_distance_field(&ctx->volume, lo, hi, max_radius, flags, &snapshot, &why);
    if (st != blok::GpuBuildStatus::Ok) return volume_status(ctx, st, why);
    blok::gpu_field_free(&ctx->distance);
    ctx->distance = snapshot; ctx->distance.taken = true;
    if (out_info) *out_info = snapshot.info;
    return BLOK_OK;
}

int blok_hip_volume_distance_info(blok_hip_ctx* ctx, blok_distance_info* out_info) {
    if (!ctx) return BLOK_ERR_INVALID_ARG;
    if (!ctx->distance.taken) return set_error(ctx, BLOK_ERR_INVALID_ARG, "distance_info: no snapshot (blok_hip_volume_distance_field)");
    if (!out_info) return set_error(ctx, BLOK_ERR_INVALID_ARG, "distance_info: null output");
    *out_info = ctx->distance.info;
    return BLOK_OK;
}

int blok_hip_volume_distance_download(blok_hip_ctx* ctx, uint16_t* out_host, uint64_t first, uint64_t count) {
    if (!ctx) return BLOK_ERR_INVALID_ARG;
    const blok::GpuDistance& d = ctx->distance;
    return ranged_download(ctx, "distance_download", "blok_hip_volume_distance_field", d.taken, field_cells(d.info.ext), d.d_field, sizeof(uint16_t), out_host, first, count);
}

int blok_hip_volume_edit_by_distance(blok_hip_ctx* ctx, int op, uint32_t d2, float density, uint32_t material, uint64_t* out_n_voxels) {
    if (out_n_voxels) *out_n_voxels = 0;
    int rc = need_volume(ctx);
    if (rc != BLOK_OK) return rc;
    if (!ctx->distance.taken) return set_error(ctx, BLOK_ERR_INVALID_ARG, "edit_by_distance: no snapshot (blok_hip_volume_distance_field)");
    if (const int rule = blok::distance::check_edit_args(ctx->distance.info, op, d2, density))
        return set_error(ctx, BLOK_ERR_INVALID_ARG, std::string("edit_by_distance: ") + blok::distance::rule_text(rule));
    std::string why;
    uint64_t n_voxels = 0;
    // (the snapshot's region lies in the box: a new volume drops the snapshot)
    const blok::GpuBuildStatus st = blok::gpu_volume_edit_by_distance(&ctx->volume, &ctx->distance, op, d2, density, material, &n_voxels, &why);
    if (out_n_voxels) *out_n_voxels = n_voxels;
    return volume_status(ctx, st, why);
}

int blok_hip_volume_flood_field(blok_hip_ctx* ctx, const int32_t region_lo[3], const int32_t region_hi[3], const int32_t* seeds_xyz_host,
                                uint64_t n_seeds, uint32_t max_steps, uint32_t flags, uint32_t material, blok_flood_info* out_info) {
    int rc = need_volume(ctx);
    if (rc != BLOK_OK) return rc;
    if (const int rule = blok::flood::check_field_args(seeds_xyz_host, n_seeds, max_steps, flags))
        return set_error(ctx, BLOK_ERR_INVALID_ARG, std::string("flood_field: ") + blok::flood::rule_text(rule));
    uint32_t lo[3], hi[3];
    rc = volume_region(ctx, "flood_field", region_lo, region_hi, lo, hi);
    if (rc != BLOK_OK) return rc;
    for (uint64_t i = 0; i < n_seeds; ++i)
        for (int a = 0; a < 3; ++a) {
            const int64_t c = int64_t(seeds_xyz_host[3 * i + a]) - ctx->volume.origin[a];
            if (c < int64_t(lo[a]) || c >= int64_t(hi[a])) return set_error(ctx, BLOK_ERR_INVALID_ARG, "flood_field: seed " + std::to_string(i) + " lies outside the region");
        }
    std::string why;
    blok::GpuFlood snapshot;
    // (edits are enqueued on the null stream, and so is this: it reads the masks they leave)
    const blok::GpuBuildStatus st = blok::gpu_volume_flood_field(&ctx->volume, lo, hi, seeds_xyz_host, n_seeds, max_steps, flags, material, &snapshot, &why);
    if (st != blok::GpuBuildStatus::Ok) return volume_status(ctx, st, why);
    blok::gpu_field_free(&ctx->flood);
    ctx->flood = snapshot; ctx->flood.taken = true;
    if (out_info) *out_info = snapshot.info;
    return BLOK_OK;
}

int blok_hip_volume_flood_info(blok_hip_ctx* ctx, blok_flood_info* out_info) {
    if (!ctx) return BLOK_ERR_INVALID_ARG;
    if (!ctx->flood.taken) return set_error(ctx, BLOK_ERR_INVALID_ARG, "flood_info: no snapshot (blok_hip_volume_flood_field)");
    if (!out_info) return set_error(ctx, BLOK_ERR_INVALID_ARG, "flood_info: null output");
    *out_info = ctx->flood.info;
    return BLOK_OK;
}

int blok_hip_volume_flood_download(blok_hip_ctx* ctx, uint16_t* out_host, uint64_t first, uint64_t count) {
    if (!ctx) return BLOK_ERR_INVALID_ARG;
    const blok::GpuFlood& f = ctx->flood;
    return ranged_download(ctx, "flood_download", "blok_hip_volume_flood_field", f.taken, field_cells(f.info.ext), f.d_field, sizeof(uint16_t), out_host, first, count);
}

int blok_hip_volume_flood_counters(blok_hip_ctx* ctx, uint64_t out_counts[2]) {
    if (!ctx) return BLOK_ERR_INVALID_ARG;
    if (!ctx->flood.taken) return set_error(ctx, BLOK_ERR_INVALID_ARG, "flood_counters: no snapshot (blok_hip_volume_flood_field)");
    if (!out_counts) return set_error(ctx, BLOK_ERR_INVALID_ARG, "flood_counters: null output");
    out_counts[0] = ctx->flood.rounds; out_counts[1] = ctx->flood.visits;
    return BLOK_OK;
}

int blok_hip_volume_edit_by_flood(blok_hip_ctx* ctx, int op, uint32_t d, float density, uint32_t material, uint64_t* out_n_voxels) {
    if (out_n_voxels) *out_n_voxels = 0;
    int rc = need_volume(ctx);
    if (rc != BLOK_OK) return rc;
    if (!ctx->flood.taken) return set_error(ctx, BLOK_ERR_INVALID_ARG, "edit_by_flood: no snapshot (blok_hip_volume_flood_field)");
    if (const int rule = blok::flood::check_edit_args(ctx->flood.info, op, d, density))
        return set_error(ctx, BLOK_ERR_INVALID_ARG, std::string("edit_by_flood: ") + blok::flood::rule_text(rule));
    std::string why;
    uint64_t n_voxels = 0;
    // (the snapshot's region lies in the box: a new volume drops the snapshot)
    const blok::GpuBuildStatus st = blok::gpu_volume_edit_by_flood(&ctx->volume, &ctx->flood, op, d, density, material, &n_voxels, &why);
    if (out_n_voxels) *out_n_voxels = n_voxels;
    return volume_status(ctx, st, why);
}

int blok_hip_volume_column_field(blok_hip_ctx* ctx, const int32_t region_lo[3], const int32_t region_hi[3], uint32_t axis, uint32_t flags,
                                 blok_columns_info* out_info) {
    int rc = need_volume(ctx);
    if (rc != BLOK_OK) return rc;
    if (const int rule = blok::columns::check_field_args(axis, flags)) return set_error(ctx, BLOK_ERR_INVALID_ARG, std::string("column_field: ") + blok::columns::field_rule_text(rule));
    uint32_t lo[3], hi[3];
    rc = volume_region(ctx, "column_field", region_lo, region_hi, lo, hi);
    if (rc != BLOK_OK) return rc;
    std::string why;
    blok::GpuColumns snapshot;
    // (edits are enqueued on the null stream, and so is this: it reads the masks they leave)
    const blok::GpuBuildStatus st = blok::gpu_volume_column_field(&ctx->volume, lo, hi, axis, flags, &snapshot, &why);
    if (st != blok::GpuBuildStatus::Ok) return volume_status(ctx, st, why);
    blok::gpu_columns_free(&ctx->columns);
    blok::gpu_scatter_free(&ctx->scatter);                 // (made from the snapshot that has just gone)
    ctx->columns = snapshot; ctx->columns.taken = true;
    if (out_info) *out_info = snapshot.info;
    return BLOK_OK;
}

int blok_hip_volume_columns_info(blok_hip_ctx* ctx, blok_columns_info* out_info) {
    if (!ctx) return BLOK_ERR_INVALID_ARG;
    if (!ctx->columns.taken) return set_error(ctx, BLOK_ERR_INVALID_ARG, "columns_info: no snapshot (blok_hip_volume_column_field)");
    if (!out_info) return set_error(ctx, BLOK_ERR_INVALID_ARG, "columns_info: null output");
    *out_info = ctx->columns.info;
    return BLOK_OK;
}

int blok_hip_volume_columns_download(blok_hip_ctx* ctx, uint32_t plane, void* out_host, uint64_t first, uint64_t count) {
    if (!ctx) return BLOK_ERR_INVALID_ARG;
    const blok::GpuColumns& c = ctx->columns;
    if (c.taken && plane > 1u) return set_error(ctx, BLOK_ERR_INVALID_ARG, "columns_download: plane above 1");
    return ranged_download(ctx, "columns_download", "blok_hip_volume_column_field", c.taken, c.info.n_columns, plane == 0u ? static_cast<const void*>(c.d_top) : c.d_material,
                           plane == 0u ? sizeof(uint16_t) : sizeof(uint32_t), out_host, first, count);
}

int blok_hip_volume_scatter_models(blok_hip_ctx* ctx, const blok_scatter_params* params, const blok_scatter_entry* entries_host, uint32_t n_entries,
                                   blok_scatter_info* out_info) {
    if (!ctx) return BLOK_ERR_INVALID_ARG;
    if (const int rule = blok::columns::check_scatter_args(ctx->columns.taken ? &ctx->columns.info : nullptr, params, entries_host, n_entries))
        return set_error(ctx, BLOK_ERR_INVALID_ARG, std::string("scatter_models: ") + blok::columns::scatter_rule_text(rule));
    for (uint32_t i = 0; i < n_entries; ++i) {           // (the anchors are model voxels: a scaled model's would not land on the cell)
        const int rc = refuse_scaled_model(ctx, "scatter_models", entries_host[i].model);
        if (rc != BLOK_OK) return rc;
    }
    BLOK_HIP_TRY(ctx, hipSetDevice(ctx->device));
    std::string why;
    blok::GpuScatter table;
    const blok::GpuBuildStatus st = blok::gpu_columns_scatter(&ctx->columns, *params, entries_host, n_entries, &table, &why);
    if (st != blok::GpuBuildStatus::Ok) return volume_status(ctx, st, why);
    blok::gpu_scatter_free(&ctx->scatter);
    ctx->scatter = table; ctx->scatter.taken = true;
    if (out_info) *out_info = table.info;
    return BLOK_OK;
}

int blok_hip_volume_scatter_info(blok_hip_ctx* ctx, blok_scatter_info* out_info) {
    if (!ctx) return BLOK_ERR_INVALID_ARG;
    if (!ctx->scatter.taken) return set_error(ctx, BLOK_ERR_INVALID_ARG, "scatter_info: no table (blok_hip_volume_scatter_models)");
    if (!out_info) return set_error(ctx, BLOK_ERR_INVALID_ARG, "scatter_info: null output");
    *out_info = ctx->scatter.info;
    return BLOK_OK;
}

int blok_hip_volume_scatter_download(blok_hip_ctx* ctx, blok_instance* out_host, uint64_t first, uint64_t count) {
    if (!ctx) return BLOK_ERR_INVALID_ARG;
    const blok::GpuScatter& s = ctx->scatter;
    return ranged_download(ctx, "scatter_download", "blok_hip_volume_scatter_models", s.taken, s.info.n_placed, s.d_table, sizeof(blok_instance), out_host, first, count);
}

int blok_hip_volume_scatter_device(blok_hip_ctx* ctx, const blok_instance** out_dev, uint64_t* out_count) {
    if (!ctx) return BLOK_ERR_INVALID_ARG;
    if (!ctx->scatter.taken) return set_error(ctx, BLOK_ERR_INVALID_ARG, "scatter_device: no table (blok_hip_volume_scatter_models)");
    if (!out_dev || !out_count) return set_error(ctx, BLOK_ERR_INVALID_ARG, "scatter_device: null output");
    *out_dev = ctx->scatter.d_table; *out_count = ctx->scatter.info.n_placed;
    return BLOK_OK;
}

int blok_hip_volume_scroll(blok_hip_ctx* ctx, const int32_t delta[3], uint32_t flags, blok_scroll_info* out_info) {
    int rc = need_volume(ctx);
    if (rc != BLOK_OK) return rc;
    blok::GpuVolume& v = ctx->volume;
    const uint32_t dims[3] = {v.nx, v.ny, v.nz};
    if (const int rule = blok::scroll::check_args(v.origin, dims, delta, flags))
        return set_error(ctx, blok::scroll::status(rule), std::string("volume_scroll: ") + blok::scroll::rule_text(rule));
    blok_scroll_info info;
    blok::scroll::plan(v.origin, dims, delta, &info);
    // a zero delta changes nothing: it is planned and counted like PLAN_ONLY
    const bool write = !(flags & BLOK_SCROLL_PLAN_ONLY) && (delta[0] != 0 || delta[1] != 0 || delta[2] != 0);
    std::string why;
    // (edits are enqueued on the null stream, and so is this: it moves what they leave)
    const blok::GpuBuildStatus st = blok::gpu_volume_scroll(&v, delta, write, &info.n_filled_before, &info.n_filled_kept, &why);
    if (st != blok::GpuBuildStatus::Ok) return volume_status(ctx, st, why);
    if (write) {
        scroll_volume_snapshots(ctx, delta);
        for (int a = 0; a < 3; ++a) v.origin[a] = info.origin[a];
        const uint32_t lo[3] = {0, 0, 0};
        v.edits.note(lo, dims, true);                      // the whole box, MayFill: to the installed world every cell may hold another voxel
    }
    if (out_info) *out_info = info;
    return BLOK_OK;
}

int blok_hip_volume_reduce(blok_hip_ctx* ctx, const int32_t region_lo[3], const int32_t region_hi[3], uint32_t levels, uint32_t flags,
                           blok_lod_info* out_info) {
    int rc = need_volume(ctx);
    if (rc != BLOK_OK) return rc;
    if (const int rule = blok::lod::check_args(levels, flags)) return set_error(ctx, BLOK_ERR_INVALID_ARG, std::string("volume_reduce: ") + blok::lod::rule_text(rule));
    uint32_t lo[3], hi[3];
    rc = volume_region(ctx, "volume_reduce", region_lo, region_hi, lo, hi);
    if (rc != BLOK_OK) return rc;
    std::string why;
    blok::GpuLod snapshot;
    // (edits are enqueued on the null stream, and so is this: it reads the masks and the ids they leave)
    const blok::GpuBuildStatus st = blok::gpu_volume_reduce(&ctx->volume, lo, hi, levels, flags, &snapshot, &why);
    if (st != blok::GpuBuildStatus::Ok) return volume_status(ctx, st, why);
    blok::gpu_lod_free(&ctx->lod);
    ctx->lod = snapshot; ctx->lod.taken = true;
    if (out_info) *out_info = snapshot.info;
    return BLOK_OK;
}

int blok_hip_terrain_reduce(blok_hip_ctx* ctx, const blok_terrain_params* params, const int32_t region_lo[3], const int32_t region_hi[3],
                            uint32_t levels, uint32_t flags, blok_lod_info* out_info) {
    if (!ctx) return BLOK_ERR_INVALID_ARG;
    if (!params) return set_error(ctx, BLOK_ERR_INVALID_ARG, "terrain_reduce: null parameters");
    if (blok::terrain::check_params(*params) != 0) return set_error(ctx, BLOK_ERR_INVALID_ARG, "terrain_reduce: parameters outside their limits (blok_terrain_validate)");
    if (params->flags != 0u) return set_error(ctx, BLOK_ERR_INVALID_ARG, "terrain_reduce: params->flags must be 0 (SHELL, CLOSE_SIDES and ADD describe writes into a volume)");
    if (const int rule = blok::lod::check_args(levels, flags, blok::terrain_lod::kFlags)) return set_error(ctx, BLOK_ERR_INVALID_ARG, std::string("terrain_reduce: ") + blok::lod::rule_text(rule));
    if (!region_lo || !region_hi) return set_error(ctx, BLOK_ERR_INVALID_ARG, "terrain_reduce: both region corners are required");
    if (const int rc = blok::terrain_lod::check_region(region_lo, region_hi))
        return set_error(ctx, rc, rc == BLOK_ERR_INVALID_ARG ? "terrain_reduce: region lo > hi" : "terrain_reduce: a coordinate beyond 2^30, an extent above 65536 or 2^31 level-1 cells");
    BLOK_HIP_TRY(ctx, hipSetDevice(ctx->device));
    std::string why;
    blok::GpuLod snapshot;
    const blok::GpuBuildStatus st = blok::gpu_terrain_reduce(*params, region_lo, region_hi, levels, flags, &snapshot, &why);
    if (st != blok::GpuBuildStatus::Ok) return volume_status(ctx, st, why);
    blok::gpu_lod_free(&ctx->lod);
    ctx->lod = snapshot; ctx->lod.taken = true;
    if (out_info) *out_info = snapshot.info;
    return BLOK_OK;
}

int blok_hip_volume_lod_info(blok_hip_ctx* ctx, blok_lod_info* out_info) {
    if (!ctx) return BLOK_ERR_INVALID_ARG;
    if (!ctx->lod.taken) return set_error(ctx, BLOK_ERR_INVALID_ARG, "lod_info: no snapshot (blok_hip_volume_reduce)");
    if (!out_info) return set_error(ctx, BLOK_ERR_INVALID_ARG, "lod_info: null output");
    *out_info = ctx->lod.info;
    return BLOK_OK;
}

int blok_hip_volume_lod_download(blok_hip_ctx* ctx, uint32_t level, uint32_t plane, void* out_host, uint64_t first, uint64_t count) {
    if (!ctx) return BLOK_ERR_INVALID_ARG;
    const blok::GpuLod& l = ctx->lod;
    if (l.taken && (level == 0u || level > l.info.levels)) return set_error(ctx, BLOK_ERR_INVALID_ARG, "lod_download: level 0 or above the snapshot's levels");
    if (l.taken && plane > 2u) return set_error(ctx, BLOK_ERR_INVALID_ARG, "lod_download: plane above 2");
    const uint64_t n = l.taken ? l.info.level[level - 1u].n_cells : 0u;
    const char* base = l.taken && l.d_planes ? static_cast<const char*>(l.d_planes) + blok::lod::level_offset(l.info, level) + blok::lod::plane_offset(n, plane) : nullptr;
    return ranged_download(ctx, "lod_download", "blok_hip_volume_reduce", l.taken, n, base, plane == 2u ? sizeof(uint32_t) : sizeof(uint16_t), out_host, first, count);
}

int blok_hip_volume_lod_model(blok_hip_ctx* ctx, uint32_t level, uint32_t min_count, uint32_t* out_model, uint64_t* out_n_voxels) {
    if (out_n_voxels) *out_n_voxels = 0;
    if (!ctx) return BLOK_ERR_INVALID_ARG;
    const blok::GpuLod& l = ctx->lod;
    if (!l.taken) return set_error(ctx, BLOK_ERR_INVALID_ARG, "lod_model: no snapshot (blok_hip_volume_reduce)");
    if (level == 0u || level > l.info.levels) return set_error(ctx, BLOK_ERR_INVALID_ARG, "lod_model: level 0 or above the snapshot's levels");
    if (min_count == 0u || min_count > (1u << (3u * level))) return set_error(ctx, BLOK_ERR_INVALID_ARG, "lod_model: min_count 0 or above 8^level");
    if (!out_model) return set_error(ctx, BLOK_ERR_INVALID_ARG, "lod_model: null output id");
    if (ctx->models.desc.size() >= std::numeric_limits<uint32_t>::max() - 1u) return set_error(ctx, BLOK_ERR_INVALID_ARG, "model ids exhausted");
    BLOK_HIP_TRY(ctx, hipSetDevice(ctx->device));
    std::string why;
    blok::GpuTree tree;
    int32_t box_lo[3] = {0, 0, 0}, box_hi[3] = {0, 0, 0};
    uint64_t n_voxels = 0;
    if (l.info.level[level - 1u].n_cells) {
        const blok::GpuBuildStatus st = blok::gpu_lod_capture(&l, level, min_count, &tree, box_lo, box_hi, &n_voxels, &why);
        if (st != blok::GpuBuildStatus::Ok) return volume_status(ctx, st, why);
    }
    if (!n_voxels) return set_error(ctx, BLOK_ERR_UNSUPPORTED, "lod_model: the level holds no cell with that many filled voxels");
    const int rc = add_captured_model(ctx, tree, box_lo, box_hi, out_model);
    if (rc != BLOK_OK) return rc;
    if (out_n_voxels) *out_n_voxels = n_voxels;
    return BLOK_OK;
}

int blok_hip_volume_automaton(blok_hip_ctx* ctx, const int32_t region_lo[3], const int32_t region_hi[3], const blok_automaton_rule* rule,
                              uint64_t* out_step_counts, blok_automaton_info* out_info) {
    int rc = need_volume(ctx);
    if (rc != BLOK_OK) return rc;
    if (const int failed = blok::automaton::check(rule)) return set_error(ctx, BLOK_ERR_INVALID_ARG, std::string("volume_automaton: ") + blok::automaton::rule_text(failed));
    uint32_t lo[3], hi[3];
    rc = volume_region(ctx, "volume_automaton", region_lo, region_hi, lo, hi);
    if (rc != BLOK_OK) return rc;
    std::string why;
    blok_automaton_info info;
    // (edits are enqueued on the null stream, and so is this: it steps what they leave)
    const blok::GpuBuildStatus st = blok::gpu_volume_automaton(&ctx->volume, lo, hi, *rule, out_step_counts, &info, &why);
    if (st != blok::GpuBuildStatus::Ok) return volume_status(ctx, st, why);
    if (out_info) *out_info = info;
    return BLOK_OK;
}

int blok_hip_volume_rebuild(blok_hip_ctx* ctx, const blok_material* materials, size_t n_materials) {
    int rc = need_volume(ctx);
    if (rc != BLOK_OK) return rc;
    if (n_materials && !materials) return set_error(ctx, BLOK_ERR_INVALID_ARG, "null material table");
    const bool timing = std::getenv("BLOK_VOLUME_TIMING") != nullptr;
    const auto t_begin = std::chrono::steady_clock::now();
    BLOK_HIP_TRY(ctx, hipDeviceSynchronize());            // frames still reading a tree of an earlier build
    const auto t_synced = std::chrono::steady_clock::now();
    blok::GpuVolume& v = ctx->volume;
    blok::GpuTree gpu;
    std::string why;
    const blok::GpuBuildStatus st = blok::gpu_volume_build(&v, &gpu, &why);
    const auto t_built = std::chrono::steady_clock::now();
    // the edits this build has taken in (whether or not it succeeded), in world voxels: for the shadow rays' last-occluder map
    const uint32_t dims[3] = {v.nx, v.ny, v.nz};
    const blok::EditLog::Taken edits = v.edits.take(v.origin, dims);
    if (st == blok::GpuBuildStatus::UseHostBuilder) {      // nothing filled: an empty world
        blok::HostTree tree;
        std::vector<blok::VoxelRec> none;
        const char* w = "";
        if (!blok::build_tree(none, tree, &w)) return set_error(ctx, BLOK_ERR_UNSUPPORTED, w);
        return install_tree(ctx, tree, materials, n_materials);
    }
    if (st != blok::GpuBuildStatus::Ok) return volume_status(ctx, st, why);
    // the world it replaces: same lattice = the maps laid out over it stay valid where nothing was edited
    const bool same_lattice = ctx->has_world && ctx->built_on_device && ctx->stats.levels == gpu.levels && ctx->stats.origin[0] == gpu.origin[0] &&
                              ctx->stats.origin[1] == gpu.origin[1] && ctx->stats.origin[2] == gpu.origin[2] && ctx->world_voxel_size == 1.0f;
    // the material table is uploaded again only when it differs from the installed one
    const bool same_materials = same_lattice && ctx->d_materials && ctx->n_materials == n_materials && ctx->volume_materials.size() == n_materials * sizeof(blok_material) &&
                                (n_materials == 0 || std::memcmp(ctx->volume_materials.data(), materials, n_materials * sizeof(blok_material)) == 0);
    blok::DeviceArray<float> keep_sun; const bool keep_has_sun = ctx->has_sun_map;
    blok::DeviceArray<blok_material> keep_mat; const size_t keep_n_mat = ctx->n_materials;
    if (same_lattice) keep_sun = std::move(ctx->d_sun_map);      // survive free_world
    if (same_materials) keep_mat = std::move(ctx->d_materials);
    free_world(ctx);
    adopt_tree(ctx, gpu);
    if (same_materials) { ctx->d_materials = std::move(keep_mat); ctx->n_materials = keep_n_mat; }
    else {
        rc = install_materials(ctx, materials, n_materials);
        if (rc != BLOK_OK) { free_world(ctx); return rc; }
        ctx->volume_materials.assign(reinterpret_cast<const unsigned char*>(materials), reinterpret_cast<const unsigned char*>(materials) + n_materials * sizeof(blok_material));
    }
    ctx->stats.n_voxels = gpu.n_voxels;
    ctx->stats.n_tree_nodes = gpu.n_nodes;
    ctx->stats.tree_bytes = gpu.n_nodes * sizeof(blok::TreeNode) + gpu.n_voxels * sizeof(uint32_t);
    ctx->stats.levels = gpu.levels;
    for (int a = 0; a < 3; ++a) ctx->stats.origin[a] = gpu.origin[a];
    ctx->has_world = true; ctx->tree_version += 1u;      // (not world_version: see below — but what was computed from the tree, the beam bounds of a view at rest, goes)
    // (an edited world keeps the view's order: a brush changes few tiles' costs, and the tiles that have become live are walked by their
    // search waves until the next sort — which comes at the base interval again; measured, a brush of radius 10 before every frame: 207 us
    // per frame with the order kept, 270 with it dropped)
    ctx->order.interval_now = ctx->order.interval;
    ctx->built_on_device = true;
    const int rc_models = models_follow_voxel_size(ctx);       // (the volume's world has voxel size 1: behind another world's, scaled models may be back under their limit)
    if (rc_models != BLOK_OK) return rc_models;
    if (same_lattice) { ctx->d_sun_map = std::move(keep_sun); ctx->has_sun_map = keep_has_sun; }
    const auto t_installed = std::chrono::steady_clock::now();
    // a fill of the whole box is a new world to the map: raised over every texel it would stay loose until kSunMapLooseEdits further
    // edits (api.hip), so it is searched anew as for a changed lattice — one search per texel behind an edit that wrote every cell
    rc = update_sun_map(ctx, edits.lo, edits.hi, same_lattice && !(edits.whole && edits.may_fill), edits.may_fill);
    if (timing) {
        const auto us = [](auto a, auto b) { return std::chrono::duration<double, std::micro>(b - a).count(); };
        std::fprintf(stderr, "[volume_rebuild us] wait-for-device %.1f build %.1f install %.1f sun-map %.1f\n", us(t_begin, t_synced), us(t_synced, t_built), us(t_built, t_installed), us(t_installed, std::chrono::steady_clock::now()));
    }
    return rc;
}

// ---- emissive voxels as lights (blok_hip.h; lights_kernels.hip) ----
namespace {
void lights_info_of(const blok_hip_ctx* ctx, blok_lights_info* out) {
    if (!out) return;
    const blok_hip_ctx::Lights& l = ctx->lights;
    *out = blok_lights_info{};
    out->n = l.n; out->n_owned = l.n_owned; out->n_faces = l.n_faces; out->area_world = l.area_world;
    out->bytes = l.n ? static_cast<uint64_t>(l.n) * sizeof(blok_light) + blok::lights::kSetWords * sizeof(uint32_t) : 0u;
}
// A new table of n records and its owned set, both in device memory, take the old one's place.
int install_lights(blok_hip_ctx* ctx, blok::DeviceArray<blok_light>&& table, uint32_t n, uint64_t n_faces, blok::DeviceArray<uint32_t>&& owned, blok_lights_info* out_info) {
    if (n == 0) { clear_lights(ctx); lights_info_of(ctx, out_info); return BLOK_OK; }
    std::vector<uint32_t> words(blok::lights::kSetWords);
    BLOK_HIP_TRY(ctx, hipMemcpy(words.data(), owned, words.size() * sizeof(uint32_t), hipMemcpyDeviceToHost));
    clear_lights(ctx);
    blok_hip_ctx::Lights& l = ctx->lights;
    l.table = std::move(table); l.owned = std::move(owned);
    l.n = n; l.n_faces = n_faces;
    for (const uint32_t w : words) l.n_owned += static_cast<uint32_t>(__builtin_popcount(w));
    l.area_world = static_cast<float>(n_faces) * ctx->world_voxel_size * ctx->world_voxel_size;      // formed once, here
    lights_info_of(ctx, out_info);
    return BLOK_OK;
}
}  // namespace

int blok_hip_lights_from_quads(blok_hip_ctx* ctx, uint32_t flags, blok_lights_info* out_info) {
    if (!ctx) return BLOK_ERR_INVALID_ARG;
    if (!ctx->has_world) return set_error(ctx, BLOK_ERR_NO_WORLD, "lights_from_quads: no world");
    if (flags) return set_error(ctx, BLOK_ERR_INVALID_ARG, "lights_from_quads: unknown flag bits");
    if (!ctx->quads.taken) return set_error(ctx, BLOK_ERR_INVALID_ARG, "lights_from_quads: no quads snapshot (blok_hip_volume_extract_quads)");
    if (ctx->quads.flags & BLOK_QUADS_IGNORE_MATERIAL) return set_error(ctx, BLOK_ERR_INVALID_ARG, "lights_from_quads: the snapshot was taken with BLOK_QUADS_IGNORE_MATERIAL");
    if (!ctx->n_materials || ctx->material_glows.size() != blok::lights::kSetWords) return set_error(ctx, BLOK_ERR_INVALID_ARG, "lights_from_quads: no material table");
    BLOK_HIP_TRY(ctx, hipSetDevice(ctx->device));
    blok::DeviceArray<uint32_t> glows, owned;
    BLOK_HIP_TRY(ctx, glows.reserve(blok::lights::kSetWords, blok::FreeAfter::nothing()));
    BLOK_HIP_TRY(ctx, owned.reserve(blok::lights::kSetWords, blok::FreeAfter::nothing()));
    BLOK_HIP_TRY(ctx, hipMemcpy(glows, ctx->material_glows.data(), blok::lights::kSetWords * sizeof(uint32_t), hipMemcpyHostToDevice));
    blok::GpuLights made;
    std::string why;
    const uint32_t n_mat = static_cast<uint32_t>(std::min<size_t>(ctx->n_materials, blok::lights::kSetBits));
    // (edits and the extraction are enqueued on the null stream, and so is this)
    const blok::GpuBuildStatus st = blok::gpu_lights_from_quads(ctx->quads.d_quads, ctx->quads.n_quads, glows, n_mat, owned, &made, &why);
    if (st != blok::GpuBuildStatus::Ok) return volume_status(ctx, st, why);
    blok::DeviceArray<blok_light> table;
    table.adopt(made.d_lights, made.n);
    return install_lights(ctx, std::move(table), made.n, made.n_faces, std::move(owned), out_info);
}

int blok_hip_set_lights(blok_hip_ctx* ctx, const blok_light* lights_host, uint32_t n, blok_lights_info* out_info) {
    if (!ctx) return BLOK_ERR_INVALID_ARG;
    if (!lights_host || n == 0) { clear_lights(ctx); lights_info_of(ctx, out_info); return BLOK_OK; }
    static const char* const kRules[] = {"", "face above 5", "du or dv is 0", "cum is not the running sum of du * dv", "2^31 or more lights, or 2^32 or more unit faces",
                                         "a corner outside [-32768, 32768]"};
    uint64_t faces = 0, index = 0;
    if (const int rule = blok::lights::check_table(lights_host, n, &faces, &index))
        return set_error(ctx, rule == 4 ? BLOK_ERR_UNSUPPORTED : BLOK_ERR_INVALID_ARG, "set_lights: light " + std::to_string(index) + ": " + kRules[rule]);
    if (!ctx->has_world) return set_error(ctx, BLOK_ERR_NO_WORLD, "set_lights: no world");
    BLOK_HIP_TRY(ctx, hipSetDevice(ctx->device));
    std::vector<uint32_t> words(blok::lights::kSetWords, 0u);
    const uint32_t n_mat = static_cast<uint32_t>(std::min<size_t>(ctx->n_materials, blok::lights::kSetBits));
    for (uint32_t i = 0; i < n; ++i) { const uint32_t m = blok::lights::material_index(lights_host[i].material, n_mat); words[m >> 5] |= 1u << (m & 31u); }
    blok::DeviceArray<blok_light> table;
    blok::DeviceArray<uint32_t> owned;
    BLOK_HIP_TRY(ctx, table.reserve(n, blok::FreeAfter::nothing()));
    BLOK_HIP_TRY(ctx, owned.reserve(blok::lights::kSetWords, blok::FreeAfter::nothing()));
    BLOK_HIP_TRY(ctx, hipMemcpy(table, lights_host, static_cast<size_t>(n) * sizeof(blok_light), hipMemcpyHostToDevice));
    BLOK_HIP_TRY(ctx, hipMemcpy(owned, words.data(), words.size() * sizeof(uint32_t), hipMemcpyHostToDevice));
    return install_lights(ctx, std::move(table), n, faces, std::move(owned), out_info);
}

int blok_hip_lights_info(blok_hip_ctx* ctx, blok_lights_info* out_info) {
    if (!ctx) return BLOK_ERR_INVALID_ARG;
    if (!out_info) return set_error(ctx, BLOK_ERR_INVALID_ARG, "lights_info: null output");
    lights_info_of(ctx, out_info);
    return BLOK_OK;
}

int blok_hip_lights_download(blok_hip_ctx* ctx, blok_light* out_host, uint64_t first, uint64_t count) {
    if (!ctx) return BLOK_ERR_INVALID_ARG;
    const blok_hip_ctx::Lights& l = ctx->lights;
    return ranged_download(ctx, "lights_download", "blok_hip_lights_from_quads or blok_hip_set_lights", true, l.n, l.table.get(), sizeof(blok_light), out_host, first, count);
}

// ---- the light grid (blok_hip.h; lights_kernels.hip) ----
int blok_hip_build_light_grid(blok_hip_ctx* ctx, uint32_t cell_log2, uint32_t reach, uint32_t share, uint32_t flags, blok_light_grid_info* out) {
    if (!ctx) return BLOK_ERR_INVALID_ARG;
    if (flags) return set_error(ctx, BLOK_ERR_INVALID_ARG, "build_light_grid: unknown flag bits");
    if (!blok::lights::grid_params_ok(cell_log2, reach, share))
        return set_error(ctx, BLOK_ERR_INVALID_ARG, "build_light_grid: cell_log2 must be 2..12, reach 0..3, share 1..255");
    if (ctx->lights.n == 0u) return set_error(ctx, BLOK_ERR_INVALID_ARG, "build_light_grid: no light table (blok_hip_lights_from_quads or blok_hip_set_lights)");
    BLOK_HIP_TRY(ctx, hipSetDevice(ctx->device));
    blok::GpuLightGrid made;
    std::string why;
    // (the table's builders and uploads are on the null stream, and so is this)
    const blok::GpuBuildStatus st = blok::gpu_light_grid_build(ctx->lights.table, ctx->lights.n, cell_log2, reach, share, &made, &why);
    if (st != blok::GpuBuildStatus::Ok) return volume_status(ctx, st, why);
    blok_hip_ctx::LightGrid& g = ctx->light_grid;
    if (g.info.n_cells != 0u) (void)hipDeviceSynchronize();   // frames that still sample the old one
    g.start.adopt(made.d_start, made.info.n_cells + 1u);
    g.faces.adopt(made.d_faces, made.info.n_cells);
    g.items.adopt(made.d_items, made.info.n_items);
    g.info = made.info;
    if (out) *out = g.info;
    return BLOK_OK;
}

int blok_hip_light_grid_info(blok_hip_ctx* ctx, blok_light_grid_info* out) {
    if (!ctx) return BLOK_ERR_INVALID_ARG;
    if (!out) return set_error(ctx, BLOK_ERR_INVALID_ARG, "light_grid_info: null output");
    *out = ctx->light_grid.info;
    return BLOK_OK;
}

int blok_hip_light_grid_download(blok_hip_ctx* ctx, uint32_t what, void* out_host, uint64_t first, uint64_t count) {
    if (!ctx) return BLOK_ERR_INVALID_ARG;
    const blok_hip_ctx::LightGrid& g = ctx->light_grid;
    if (what > 2u) return set_error(ctx, BLOK_ERR_INVALID_ARG, "light_grid_download: what must be 0 (start), 1 (faces) or 2 (items)");
    const bool built = g.info.n_cells != 0u;
    const uint64_t n = !built ? 0u : what == 0u ? g.info.n_cells + 1u : what == 1u ? g.info.n_cells : g.info.n_items;
    const void* base = what == 0u ? static_cast<const void*>(g.start.get()) : what == 1u ? static_cast<const void*>(g.faces.get()) : static_cast<const void*>(g.items.get());
    return ranged_download(ctx, "light_grid_download", "blok_hip_build_light_grid", built, n, base, what == 2u ? sizeof(blok_light_grid_item) : sizeof(uint32_t), out_host, first, count);
}

int blok_hip_light_grid_clear(blok_hip_ctx* ctx) {
    if (!ctx) return BLOK_ERR_INVALID_ARG;
    if (ctx->light_grid.info.n_cells != 0u) (void)hipDeviceSynchronize();     // frames that still sample it
    ctx->light_grid = blok_hip_ctx::LightGrid{};
    return BLOK_OK;
}

}  // extern "C"
