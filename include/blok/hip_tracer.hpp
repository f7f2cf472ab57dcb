// C++20 host side of the gfx950 backend, above the C ABI (blok_hip.h / blok_world.h).
//
// Mirrors the reference's own types so that an `App`-like driver calls it the way blok's App calls its
// backends (reference blok/src/app.cpp:73-128,130-192):
//   blok::GraphicsApi      reference blok/include/backend.hpp:9-12, plus the third enumerator HIP
//   blok::Camera           reference blok/include/camera.hpp:15-84 (same fields, defaults, key/mouse steps)
//   blok::WorldSvoGpu      reference blok/include/resources.hpp:195-203 (the three host arrays only)
//   blok::ChunkManager     reference blok/include/chunk_manager.hpp:18-52 (+ rebuildDirtyChunks, packChunksToGpuSvo)
//   blok::HipTracer        reference blok/include/cuda_tracer.hpp:23-58 (lifecycle) and
//                          blok/include/renderer.hpp:40-72 (addWorld / updateWorld / cleanupWorld)
// Failures throw std::runtime_error, as the reference's backends do (caught once in main,
// reference blok/src/main.cpp:19-22).  Header-only; link libblok_hip.so and libblok_host.so.
#ifndef BLOK_HIP_TRACER_HPP
#define BLOK_HIP_TRACER_HPP

#include <algorithm>
#include <array>
#include <cmath>
#include <cstdint>
#include <stdexcept>
#include <string>
#include <vector>

#include "../blok_hip.h"
#include "../blok_world.h"

namespace blok {

enum class GraphicsApi { OpenGL, Vulkan, HIP };

struct Camera {
    float position[3] = {0.0f, 10.0f, -5.0f};
    float yaw = 0.0f;
    float pitch = 0.0f;
    float fov = 60.0f;
    mutable bool cameraChanged = false;

    // basis through the same code the tests pin (blok_camera_from_yaw_pitch)
    blok_camera basis(unsigned width, unsigned height) const {
        blok_camera c{};
        if (blok_camera_from_yaw_pitch(position, yaw, pitch, fov, width, height, &c) != BLOK_OK)
            throw std::runtime_error("Camera::basis: bad frame size");
        return c;
    }
    void processKeyboard(char key, float dt) {           // reference camera.hpp:61-71
        const blok_camera c = basis(1, 1);
        const float speed = 40.0f * dt;
        auto move = [&](const float d[3], float s) { for (int a = 0; a < 3; ++a) position[a] += d[a] * s; };
        const float worldUp[3] = {0.0f, 1.0f, 0.0f};
        if (key == 'W') move(c.fwd, speed);
        if (key == 'S') move(c.fwd, -speed);
        if (key == 'A') move(c.right, -speed);
        if (key == 'D') move(c.right, speed);
        if (key == 'X') move(worldUp, speed);
        if (key == 'Z') move(worldUp, -speed);
        cameraChanged = true;
    }
    void processMouse(float dx, float dy) {               // reference camera.hpp:72-81
        const float sens = 0.01f;
        yaw += dx * sens;
        pitch += dy * sens;
        if (pitch > 89.0f) pitch = 89.0f;
        if (pitch < -89.0f) pitch = -89.0f;
        cameraChanged = true;
    }
};

struct WorldSvoGpu {
    std::vector<blok_svo_node> globalNodes;
    std::vector<blok_sub_chunk> globalSubChunks;
    std::vector<blok_material> materials;
};

class ChunkManager {
public:
    uint32_t C;
    float voxelSize;

    ChunkManager(uint32_t C_, float voxelSize_) : C(C_), voxelSize(voxelSize_) {
        if (blok_world_create(&w_, C_, voxelSize_) != BLOK_OK) throw std::runtime_error("ChunkManager: bad chunk size");
    }
    ~ChunkManager() { blok_world_destroy(w_); }
    ChunkManager(const ChunkManager&) = delete;
    ChunkManager& operator=(const ChunkManager&) = delete;

    void setVoxelMaterial(const float worldPos[3], uint32_t materialId, float density = 1.0f) {
        check(blok_world_set_voxel(w_, worldPos, materialId, density));
    }
    uint32_t getVoxelMaterial(const float worldPos[3]) const { return blok_world_get_voxel_material(w_, worldPos); }
    blok_world* handle() { return w_; }

    friend int rebuildDirtyChunks(ChunkManager& mgr, int maxPerFrame) {
        const int n = blok_world_rebuild_dirty(mgr.w_, maxPerFrame);
        if (n < 0) mgr.check(n);
        return n;
    }
    friend void packChunksToGpuSvo(ChunkManager& mgr, WorldSvoGpu& gpuWorld) {
        mgr.check(blok_world_pack(mgr.w_));
        const blok_svo_node* n = blok_world_nodes(mgr.w_);
        const blok_sub_chunk* s = blok_world_sub_chunks(mgr.w_);
        gpuWorld.globalNodes.assign(n, n + blok_world_node_count(mgr.w_));
        gpuWorld.globalSubChunks.assign(s, s + blok_world_sub_chunk_count(mgr.w_));
    }

private:
    void check(int rc) const { if (rc < 0) throw std::runtime_error(std::string("ChunkManager: ") + blok_world_last_error(w_)); }
    blok_world* w_ = nullptr;
};

// = blok::Brush / applyBrush (reference blok/include/brush.hpp:14-21, blok/src/brush.cpp:13-63)
struct Brush {
    float centerWS[3];
    float radiusWS;
    float value;
    enum Mode { ADD, SUBTRACT } mode;
};
inline void applyBrush(ChunkManager& mgr, const Brush& brush) {
    if (blok_world_apply_brush(mgr.handle(), brush.centerWS, brush.radiusWS, brush.value, brush.mode == Brush::ADD ? 0 : 1) != BLOK_OK)
        throw std::runtime_error(std::string("applyBrush: ") + blok_world_last_error(mgr.handle()));
}

// = blok::MaterialLibrary (reference blok/include/material.hpp:116-163), RAII over the C ABI.
class MaterialLibrary {
public:
    MaterialLibrary() { if (blok_material_library_create(&lib_) != BLOK_OK) throw std::runtime_error("MaterialLibrary: allocation failed"); }
    ~MaterialLibrary() { blok_material_library_destroy(lib_); }
    MaterialLibrary(const MaterialLibrary&) = delete;
    MaterialLibrary& operator=(const MaterialLibrary&) = delete;
    uint32_t addMaterial(const blok_material_desc& m) { return blok_material_library_add(lib_, &m); }
    uint32_t getOrCreateFromColor(uint8_t r, uint8_t g, uint8_t b) { return blok_material_library_from_color(lib_, r, g, b); }
    uint32_t getMaterialFromVoxPalette(uint8_t i) const { return blok_material_library_from_vox_palette(lib_, i); }
    size_t size() const { return blok_material_library_size(lib_); }
    std::vector<blok_material> packForGpu() const {
        std::vector<blok_material> out(size());
        if (blok_material_library_pack(lib_, out.data(), out.size()) != BLOK_OK) throw std::runtime_error("MaterialLibrary::packForGpu");
        return out;
    }
    blok_material_library* handle() { return lib_; }
private:
    blok_material_library* lib_ = nullptr;
};

// = loadAndImportVox (reference blok/src/vox_loader.cpp:432-462)
inline bool loadAndImportVox(const std::string& filepath, ChunkManager& chunkMgr, MaterialLibrary* materialLib = nullptr,
                             const float worldOffset[3] = nullptr, uint32_t modelIndex = 0, std::string* errorMsg = nullptr) {
    char err[256] = {0};
    const int rc = blok_load_and_import_vox(filepath.c_str(), chunkMgr.handle(), materialLib ? materialLib->handle() : nullptr,
                                            worldOffset, modelIndex, err, sizeof(err));
    if (rc != BLOK_OK && errorMsg) *errorMsg = err;
    return rc == BLOK_OK;
}

class HipTracer {
public:
    HipTracer(unsigned int width, unsigned int height, int device = 0) : m_width(width), m_height(height), m_device(device) {}
    ~HipTracer() { shutdown(); }
    HipTracer(const HipTracer&) = delete;
    HipTracer& operator=(const HipTracer&) = delete;

    void init() {
        if (m_ctx) return;
        if (blok_hip_create(&m_ctx, m_device, m_width, m_height) != BLOK_OK)
            throw std::runtime_error(std::string("HipTracer::init: ") + blok_hip_last_error(nullptr));
        m_hits.resize(static_cast<size_t>(m_width) * m_height);
    }
    void shutdown() { if (m_ctx) { blok_hip_destroy(m_ctx); m_ctx = nullptr; } m_world = nullptr; }
    void beginFrame() {}
    void endFrame() {}
    void resize(unsigned int w, unsigned int h) {
        check(blok_hip_resize(m_ctx, w, h));
        m_width = w; m_height = h;
        m_hits.assign(static_cast<size_t>(w) * h, blok_hit{});
    }
    void resetAccum() { check(blok_hip_reset_accum(m_ctx)); m_frameIndex = 0; }

    // = Renderer::addWorld: keeps a non-owning pointer to the caller's world, owns the device copies
    // ChunkManager's voxelSize for the worlds added from now on (a power of two; reference chunk_manager.cpp:19-25, app.cpp:37)
    void setVoxelSize(float voxelSize) { check(blok_hip_set_voxel_size(m_ctx, voxelSize)); }
    void addWorld(WorldSvoGpu& gpuWorld) { m_world = &gpuWorld; updateWorld(); }
    void updateWorld() {
        if (!m_world) return;
        check(blok_hip_upload_world(m_ctx, m_world->globalNodes.data(), m_world->globalNodes.size(),
                                    m_world->globalSubChunks.data(), m_world->globalSubChunks.size(),
                                    m_world->materials.data(), m_world->materials.size()));
    }
    void cleanupWorld() {
        check(blok_hip_upload_world(m_ctx, nullptr, 0, nullptr, 0, nullptr, 0));
        m_world = nullptr;
    }

    // = CudaTracer::drawFrame(cam, ...): one frame of primary first-hit records, blocking
    void drawFrame(Camera& cam) {
        const blok_camera c = cam.basis(m_width, m_height);
        check(blok_hip_trace_primary(m_ctx, &c, 0, 0, m_width, m_height, m_hits.data()));
        cam.cameraChanged = false;
        ++m_frameIndex;
    }
    // RGBA8 view of the same frame (the CUDA backend's output format, reference cuda_tracer.cu:385-386)
    const std::vector<uint32_t>& drawFrameRgba8(Camera& cam) {
        const blok_camera c = cam.basis(m_width, m_height);
        m_pixels.resize(static_cast<size_t>(m_width) * m_height);
        check(blok_hip_shade_rgba8(m_ctx, &c, 0, 0, m_width, m_height, m_pixels.data()));
        return m_pixels;
    }

    // = CudaTracer::drawFrame in its progressive mode (reference cuda_tracer.cu:484-555): path-traced samples added to the
    // accumulation buffer, which is cleared when the camera moved; returns the ACES + gamma 2.2 RGBA8 running average
    const std::vector<uint32_t>& drawFrameProgressive(Camera& cam, uint32_t sppPerFrame = 1, uint32_t maxBounces = 2) {
        const blok_camera c = cam.basis(m_width, m_height);
        m_pixels.resize(static_cast<size_t>(m_width) * m_height);
        check(blok_hip_draw_frame_accumulate(m_ctx, &c, sppPerFrame, maxBounces, m_pixels.data(), &m_frameIndex));
        cam.cameraChanged = false;
        return m_pixels;
    }
    uint32_t framesAccumulated() const { return m_frameIndex; }

    // ---- device-resident dense store (blok_hip_volume_*): ChunkManager's edit API for one box of the world, with the
    // arrays, the edits and the rebuild in HBM.  rebuildVolume() = rebuildDirtyChunks + packChunksToGpuSvo + updateWorld.
    void createVolume(const int32_t origin[3], uint32_t nx, uint32_t ny, uint32_t nz, uint32_t chunkSize = 128, float voxelSize = 1.0f) {
        check(blok_hip_volume_create(m_ctx, origin, nx, ny, nz, chunkSize, voxelSize));
    }
    void uploadVolume(const float* density, const uint32_t* materialIds) { check(blok_hip_volume_upload(m_ctx, density, materialIds)); }
    void setVoxelMaterial(const int32_t voxel[3], uint32_t materialId, float density = 1.0f) {
        check(blok_hip_volume_set_voxels(m_ctx, voxel, &materialId, &density, 1));
    }
    void applyBrush(const Brush& brush) {
        check(blok_hip_volume_apply_brush(m_ctx, brush.centerWS, brush.radiusWS, brush.value, brush.mode == Brush::ADD ? 0 : 1));
    }
    // Mesh voxelization into the volume (blok_hip_volume_voxelize_mesh): positions xyz per vertex, three indices per triangle, per-triangle
    // material ids (empty: `material` for all).  Returns the voxels written.
    uint64_t voxelizeMesh(const std::vector<float>& positions, const std::vector<uint32_t>& triangles, const std::vector<uint32_t>& triangleMaterials,
                          uint32_t material = 1, float density = 1.0f, bool solid = false) {
        if (positions.size() % 3 || triangles.size() % 3) throw std::invalid_argument("voxelizeMesh: positions and triangles come in threes");
        if (!triangleMaterials.empty() && triangleMaterials.size() != triangles.size() / 3)
            throw std::invalid_argument("voxelizeMesh: one material id per triangle");
        uint64_t n = 0;
        check(blok_hip_volume_voxelize_mesh(m_ctx, positions.data(), positions.size() / 3, triangles.data(), triangles.size() / 3,
                                            triangleMaterials.empty() ? nullptr : triangleMaterials.data(), material, density,
                                            solid ? BLOK_VOXELIZE_SOLID : BLOK_VOXELIZE_SURFACE, &n));
        return n;
    }
    // Procedural terrain into the volume (blok_hip_volume_generate_terrain): the region in world voxels, half-open (both null = the whole
    // box).  blok_terrain_default_params gives a starting landscape, blok_terrain_height the ground under a point.  Returns the filled voxels.
    uint64_t generateTerrain(const blok_terrain_params& params, const int32_t* regionLo = nullptr, const int32_t* regionHi = nullptr) {
        uint64_t n = 0;
        check(blok_hip_volume_generate_terrain(m_ctx, &params, regionLo, regionHi, &n));
        return n;
    }
    // The volume's surface as merged quads in canonical order (blok_hip_volume_extract_quads, then the snapshot fetched `page` records at
    // a time): the region in world voxels, half-open (both null = the whole box).  outFaces: the exposed unit faces.
    std::vector<blok_quad> extractQuads(const int32_t* regionLo = nullptr, const int32_t* regionHi = nullptr, bool ignoreMaterial = false,
                                        uint64_t* outFaces = nullptr, uint64_t page = uint64_t(1) << 22) {
        uint64_t n = 0, faces = 0;
        check(blok_hip_volume_extract_quads(m_ctx, regionLo, regionHi, ignoreMaterial ? BLOK_QUADS_IGNORE_MATERIAL : 0u, &n, &faces));
        if (outFaces) *outFaces = faces;
        std::vector<blok_quad> quads(n);
        for (uint64_t at = 0; at < n; at += page) check(blok_hip_volume_quads_download(m_ctx, quads.data() + at, at, std::min(page, n - at)));
        return quads;
    }
    // Emissive voxels as lights (blok_hip.h): the light table built on the device from the latest quads snapshot and the installed
    // material table (after rebuildVolume and extractQuads).  While a table with lights is installed every path-traced frame samples it.
    blok_lights_info lightsFromQuads() {
        blok_lights_info info{};
        check(blok_hip_lights_from_quads(m_ctx, 0u, &info));
        return info;
    }
    // A host-built table (blok_lights_from_quads, blok_world.h) installed; an empty vector clears.
    blok_lights_info setLights(const std::vector<blok_light>& lights) {
        blok_lights_info info{};
        check(blok_hip_set_lights(m_ctx, lights.empty() ? nullptr : lights.data(), static_cast<uint32_t>(lights.size()), &info));
        return info;
    }
    void clearLights() { check(blok_hip_set_lights(m_ctx, nullptr, 0u, nullptr)); }
    blok_lights_info lightsInfo() const {
        blok_lights_info info{};
        check(blok_hip_lights_info(m_ctx, &info));
        return info;
    }
    std::vector<blok_light> downloadLights(uint64_t page = uint64_t(1) << 22) const {
        const uint64_t n = lightsInfo().n;
        std::vector<blok_light> lights(n);
        for (uint64_t at = 0; at < n; at += page) check(blok_hip_lights_download(m_ctx, lights.data() + at, at, std::min(page, n - at)));
        return lights;
    }
    // The light grid (blok_hip.h): per-cell lists over the installed light table, built on the device; dropped with the table.
    blok_light_grid_info buildLightGrid(uint32_t cell_log2, uint32_t reach = 1u, uint32_t share = 128u) {
        blok_light_grid_info info{};
        check(blok_hip_build_light_grid(m_ctx, cell_log2, reach, share, 0u, &info));
        return info;
    }
    blok_light_grid_info lightGridInfo() const {
        blok_light_grid_info info{};
        check(blok_hip_light_grid_info(m_ctx, &info));
        return info;
    }
    void clearLightGrid() { check(blok_hip_light_grid_clear(m_ctx)); }
    // The installed grid's arrays: start (n_cells + 1 words), faces (n_cells words), items.
    std::vector<uint32_t> downloadLightGridWords(bool faces, uint64_t page = uint64_t(1) << 22) const {
        const blok_light_grid_info info = lightGridInfo();
        const uint64_t n = info.n_cells ? (faces ? info.n_cells : info.n_cells + 1u) : 0u;
        std::vector<uint32_t> words(n);
        for (uint64_t at = 0; at < n; at += page) check(blok_hip_light_grid_download(m_ctx, faces ? 1u : 0u, words.data() + at, at, std::min(page, n - at)));
        return words;
    }
    std::vector<blok_light_grid_item> downloadLightGridItems(uint64_t page = uint64_t(1) << 22) const {
        const uint64_t n = lightGridInfo().n_items;
        std::vector<blok_light_grid_item> items(n);
        for (uint64_t at = 0; at < n; at += page) check(blok_hip_light_grid_download(m_ctx, 2u, items.data() + at, at, std::min(page, n - at)));
        return items;
    }
    // Emissive models as lights (blok_hip.h): the table of a model's exposed emissive unit faces, built on the device from the model's
    // own tree under the installed material table; no faces: no table.  Dropped with the model and with every new material table.
    blok_lights_info modelLights(uint32_t model) {
        blok_lights_info info{};
        check(blok_hip_model_lights(m_ctx, model, 0u, &info));
        return info;
    }
    blok_lights_info modelLightsInfo(uint32_t model) const {
        blok_lights_info info{};
        check(blok_hip_model_lights_info(m_ctx, model, &info));
        return info;
    }
    std::vector<blok_light> downloadModelLights(uint32_t model, uint64_t page = uint64_t(1) << 22) const {
        const uint64_t n = modelLightsInfo(model).n;
        std::vector<blok_light> lights(n);
        for (uint64_t at = 0; at < n; at += page) check(blok_hip_model_lights_download(m_ctx, model, lights.data() + at, at, std::min(page, n - at)));
        return lights;
    }
    void clearModelLights(uint32_t model) { check(blok_hip_model_lights_clear(m_ctx, model)); }
    // The light prefix of an instance table over the models' tables: the header, and the n + 1 words of icum where `icum` is not null.
    blok_instance_lights_info instanceLightsInfo(const std::vector<blok_instance>& instances, std::vector<uint32_t>* icum = nullptr) const {
        blok_instance_lights_info info{};
        if (icum) icum->assign(instances.size() + 1, 0u);
        check(blok_hip_instance_lights_info(m_ctx, instances.empty() ? nullptr : instances.data(), static_cast<uint32_t>(instances.size()), &info,
                                            icum ? icum->data() : nullptr));
        return info;
    }
    // Placed models written into the resident volume, in table order (blok_hip_volume_stamp_models; mode BLOK_STAMP_SET / KEEP / ERASE):
    // returns the voxels written.  A later rebuildVolume installs the world.
    uint64_t stampModels(const std::vector<blok_instance>& placements, int mode = BLOK_STAMP_SET, float density = 1.0f) {
        uint64_t n = 0;
        check(blok_hip_volume_stamp_models(m_ctx, placements.data(), static_cast<uint32_t>(placements.size()), mode, density, &n));
        return n;
    }
    // Models resampled into the resident volume through affine maps, in table order (blok_hip_volume_stamp_affine; records from
    // blok_affine_from_instance / blok_affine_from_matrix, blok_world.h): any rotation, scale, mirror or shear, a model of any scale
    // exponent; the region in world voxels, half-open (both null = the whole box).  Returns the cells written.  A later rebuildVolume
    // installs the world.
    uint64_t stampAffine(const std::vector<blok_affine>& records, const int32_t* regionLo = nullptr, const int32_t* regionHi = nullptr,
                         int mode = BLOK_STAMP_SET, float density = 1.0f) {
        uint64_t n = 0;
        check(blok_hip_volume_stamp_affine(m_ctx, records.data(), static_cast<uint32_t>(records.size()), regionLo, regionHi, mode, density, &n));
        return n;
    }
    // A table of shapes applied to the resident volume in one pass, in table order (blok_hip_volume_apply_shapes; coordinates in
    // half-voxel units, the centre of world voxel w at 2 w + 1): returns the number of writes.  A later rebuildVolume installs the world.
    uint64_t applyShapes(const std::vector<blok_shape>& shapes) {
        uint64_t n = 0;
        check(blok_hip_volume_apply_shapes(m_ctx, shapes.data(), static_cast<uint32_t>(shapes.size()), &n));
        return n;
    }
    // The capsules of a stroke through world points given in half-voxel units, radius in half-voxel units: point k to point k + 1, so
    // that the chain has no gaps; one point is a sphere.
    static std::vector<blok_shape> strokeShapes(const std::vector<std::array<int32_t, 3>>& points, uint32_t radius, uint32_t op, uint32_t material = 0,
                                                float value = 1.0f, uint32_t match = 0) {
        std::vector<blok_shape> out;
        const size_t n = points.size() > 1 ? points.size() - 1 : points.size();
        for (size_t k = 0; k < n; ++k) {
            blok_shape s{};
            s.kind = BLOK_SHAPE_CAPSULE; s.op = op; s.material = material; s.match = match; s.value = value; s.r[0] = radius;
            const auto& p = points[k];
            const auto& q = points[std::min(k + 1, points.size() - 1)];
            for (int a = 0; a < 3; ++a) { s.a[a] = p[a]; s.b[a] = q[a]; }
            out.push_back(s);
        }
        return out;
    }
    // A region of the resident volume (world voxels, half-open; both null = the whole box) as a new model whose voxel (0, 0, 0) is the
    // region's corner (blok_hip_volume_capture_model): returns the model id.  cut: the captured voxels are cleared in the volume.
    uint32_t captureModel(const int32_t* regionLo = nullptr, const int32_t* regionHi = nullptr, bool cut = false, uint64_t* outVoxels = nullptr) {
        uint32_t model = 0;
        check(blok_hip_volume_capture_model(m_ctx, regionLo, regionHi, cut ? BLOK_CAPTURE_CUT : 0u, &model, outVoxels));
        return model;
    }
    // The connected components (6-neighbour) of a region of the resident volume (blok_hip_volume_label_components; world voxels, half-open,
    // both null = the whole box): the records sorted by label, fetched `page` at a time.  The snapshot stays on the device until the next
    // call.  outVoxels: the filled voxels.
    std::vector<blok_component> labelComponents(const int32_t* regionLo = nullptr, const int32_t* regionHi = nullptr, uint64_t* outVoxels = nullptr,
                                                uint64_t page = uint64_t(1) << 22) {
        uint64_t n = 0;
        check(blok_hip_volume_label_components(m_ctx, regionLo, regionHi, 0u, &n, outVoxels));
        std::vector<blok_component> records(n);
        for (uint64_t at = 0; at < n; at += page) check(blok_hip_volume_components_download(m_ctx, records.data() + at, at, std::min(page, n - at)));
        return records;
    }
    // Cells [first, first + count) of that snapshot's label array: one per region voxel, x fastest; BLOK_LABEL_EMPTY for an empty cell.
    std::vector<uint32_t> componentLabels(uint64_t first, uint64_t count) {
        std::vector<uint32_t> labels(count);
        check(blok_hip_volume_labels_download(m_ctx, labels.data(), first, count));
        return labels;
    }
    // The still-filled voxels of the last labelling's component `label` as a new model whose voxel (0, 0, 0) is the record's lo, returned
    // in outOrigin (blok_hip_volume_capture_component): an instance {model, offset = outOrigin, identity} shows the piece where it was.
    // cut: those voxels are cleared in the volume.
    uint32_t captureComponent(uint32_t label, bool cut = false, int32_t outOrigin[3] = nullptr, uint64_t* outVoxels = nullptr) {
        uint32_t model = 0;
        check(blok_hip_volume_capture_component(m_ctx, label, cut ? BLOK_COMPONENT_CUT : 0u, &model, outOrigin, outVoxels));
        return model;
    }
    // Placed models swept against the resident volume (blok_hip_volume_sweep_models): per placement the voxels that overlap filled cells
    // and the free travel along `direction` (blok_hit::face numbering, 3 = down), at most maxDistance.  Each placement on its own; the
    // volume is not changed.  boxIsSolid: cells outside the volume's box stop the model.
    std::vector<blok_sweep_result> sweepModels(const std::vector<blok_instance>& placements, uint32_t direction, uint32_t maxDistance,
                                               bool boxIsSolid = false) {
        std::vector<blok_sweep_result> results(placements.size());
        check(blok_hip_volume_sweep_models(m_ctx, placements.data(), static_cast<uint32_t>(placements.size()), direction, maxDistance,
                                           boxIsSolid ? BLOK_SWEEP_BOX_IS_SOLID : 0u, results.data()));
        return results;
    }
    // A region of the resident volume (world voxels, half-open; both null = the whole box) as a sparse brick stream kept on the device
    // until the next encode (blok_hip_volume_encode_bricks): returns what it holds.  downloadBricks fetches it `page` entries at a time,
    // restoreBricks writes it back (undo, or a paste at dstLo), decodeBricks does the same from host arrays (a loaded .bvol file).
    struct BrickStream {
        blok_bricks_info info{};
        std::vector<blok_brick_record> records;
        std::vector<uint32_t> density, material;      // the payloads: density bit patterns, material ids
    };
    blok_bricks_info encodeBricks(const int32_t* regionLo = nullptr, const int32_t* regionHi = nullptr, bool filledOnly = false) {
        blok_bricks_info info{};
        check(blok_hip_volume_encode_bricks(m_ctx, regionLo, regionHi, filledOnly ? BLOK_BRICKS_FILLED_ONLY : 0u, &info));
        return info;
    }
    BrickStream downloadBricks(uint64_t page = uint64_t(1) << 22) {
        BrickStream s;
        check(blok_hip_volume_bricks_info(m_ctx, &s.info));
        s.records.resize(s.info.n_bricks); s.density.resize(s.info.n_density); s.material.resize(s.info.n_material);
        for (uint64_t at = 0; at < s.info.n_bricks; at += page) check(blok_hip_volume_bricks_download(m_ctx, s.records.data() + at, at, std::min(page, s.info.n_bricks - at)));
        for (uint64_t at = 0; at < s.info.n_density; at += page) check(blok_hip_volume_brick_payload_download(m_ctx, 0u, s.density.data() + at, at, std::min(page, s.info.n_density - at)));
        for (uint64_t at = 0; at < s.info.n_material; at += page) check(blok_hip_volume_brick_payload_download(m_ctx, 1u, s.material.data() + at, at, std::min(page, s.info.n_material - at)));
        return s;
    }
    void restoreBricks(const int32_t* dstLo = nullptr, bool keepOthers = false) {
        check(blok_hip_volume_restore_bricks(m_ctx, dstLo, keepOthers ? BLOK_BRICKS_KEEP_OTHERS : 0u));
    }
    void decodeBricks(const BrickStream& s, const int32_t* dstLo = nullptr, bool keepOthers = false) {
        check(blok_hip_volume_decode_bricks(m_ctx, &s.info, s.records.data(), s.density.data(), s.material.data(), dstLo, keepOthers ? BLOK_BRICKS_KEEP_OTHERS : 0u));
    }
    // The capped squared distance field of a region of the resident volume (world voxels, half-open; both null = the whole box) to the
    // nearest filled cell — toEmpty: to the nearest empty one; boxIsSolid: the outside of the box counts as filled — kept on the device until
    // the next field (blok_hip_volume_distance_field): returns what it holds.  downloadDistance fetches the values `page` cells at a time,
    // x fastest; editByDistance thresholds them at the squared distance d2 (BLOK_DISTANCE_GROW / _SHRINK / _HOLLOW) and returns the cells written.
    blok_distance_info distanceField(const int32_t* regionLo, const int32_t* regionHi, uint32_t maxRadius, bool toEmpty = false, bool boxIsSolid = false) {
        blok_distance_info info{};
        check(blok_hip_volume_distance_field(m_ctx, regionLo, regionHi, maxRadius, (toEmpty ? BLOK_DISTANCE_TO_EMPTY : 0u) | (boxIsSolid ? BLOK_DISTANCE_BOX_IS_SOLID : 0u), &info));
        return info;
    }
    std::vector<uint16_t> downloadDistance(uint64_t page = uint64_t(1) << 24) {
        blok_distance_info info{};
        check(blok_hip_volume_distance_info(m_ctx, &info));
        const uint64_t n = uint64_t(info.ext[0]) * info.ext[1] * info.ext[2];
        std::vector<uint16_t> out(n);
        for (uint64_t at = 0; at < n; at += page) check(blok_hip_volume_distance_download(m_ctx, out.data() + at, at, std::min(page, n - at)));
        return out;
    }
    uint64_t editByDistance(int op, uint32_t d2, float density = 1.0f, uint32_t material = 0) {
        uint64_t written = 0;
        check(blok_hip_volume_edit_by_distance(m_ctx, op, d2, density, material, &written));
        return written;
    }
    // The flood of a region of the resident volume (world voxels, half-open; both null = the whole box) from the world cells `seeds`
    // (x, y, z each) and the sides named by BLOK_FLOOD_SEED_FACE bits in `flags`, through the empty cells — BLOK_FLOOD_THROUGH_FILLED: the
    // filled ones, with BLOK_FLOOD_SAME_MATERIAL those of id `material` — as the least number of 6-neighbour steps, capped at maxSteps, kept
    // on the device until the next flood (blok_hip_volume_flood_field): returns what it holds.  downloadFlood fetches the values `page`
    // cells at a time, x fastest; editByFlood thresholds them at d steps (BLOK_FLOOD_FILL / _FILL_UNREACHED / _PAINT / _CLEAR) and returns
    // the cells written.
    blok_flood_info floodField(const int32_t* regionLo, const int32_t* regionHi, const std::vector<int32_t>& seeds, uint32_t maxSteps = BLOK_FLOOD_MAX_STEPS,
                               uint32_t flags = 0, uint32_t material = 0) {
        blok_flood_info info{};
        check(blok_hip_volume_flood_field(m_ctx, regionLo, regionHi, seeds.empty() ? nullptr : seeds.data(), seeds.size() / 3, maxSteps, flags, material, &info));
        return info;
    }
    std::vector<uint16_t> downloadFlood(uint64_t page = uint64_t(1) << 24) {
        blok_flood_info info{};
        check(blok_hip_volume_flood_info(m_ctx, &info));
        const uint64_t n = uint64_t(info.ext[0]) * info.ext[1] * info.ext[2];
        std::vector<uint16_t> out(n);
        for (uint64_t at = 0; at < n; at += page) check(blok_hip_volume_flood_download(m_ctx, out.data() + at, at, std::min(page, n - at)));
        return out;
    }
    uint64_t editByFlood(int op, uint32_t d = 0, float density = 1.0f, uint32_t material = 0) {
        uint64_t written = 0;
        check(blok_hip_volume_edit_by_flood(m_ctx, op, d, density, material, &written));
        return written;
    }
    // The column field of a region of the resident volume (world voxels, half-open; both null = the whole box) along `axis`: per column the
    // first filled cell met from the hi face (BLOK_COLUMNS_FROM_LOW: from the lo face) and its material id, kept on the device until the
    // next field (blok_hip_volume_column_field): returns what it holds.  downloadColumnTops / downloadColumnMaterials fetch the planes
    // `page` columns at a time.
    blok_columns_info columnField(const int32_t* regionLo, const int32_t* regionHi, uint32_t axis = 1, uint32_t flags = 0) {
        blok_columns_info info{};
        check(blok_hip_volume_column_field(m_ctx, regionLo, regionHi, axis, flags, &info));
        return info;
    }
    // Moves the resident volume's box through the world by `delta` voxels, each a multiple of 4 (blok_hip_volume_scroll): the world voxels
    // that stay inside keep their values, the cells that come into view are empty.  Returns the new origin, the exposed boxes (the caller's
    // to fill) and the leaving ones, and the counts; planOnly fills the same record and changes nothing.  The next volumeRebuild installs
    // the world.
    blok_scroll_info volumeScroll(const int32_t delta[3], bool planOnly = false) {
        blok_scroll_info info{};
        check(blok_hip_volume_scroll(m_ctx, delta, planOnly ? BLOK_SCROLL_PLAN_ONLY : 0u, &info));
        return info;
    }
    std::vector<uint16_t> downloadColumnTops(uint64_t page = uint64_t(1) << 24) { return downloadColumnPlane<uint16_t>(0, page); }
    std::vector<uint32_t> downloadColumnMaterials(uint64_t page = uint64_t(1) << 24) { return downloadColumnPlane<uint32_t>(1, page); }
    // Scatter over the column field (along +y from the top): a table of placements sorted by column, kept on the device until the next
    // scatter or column field (blok_hip_volume_scatter_models): returns its counts.  downloadScatter fetches it, for stampModels or a check
    // with blok_hip_check_instances; scatterTable gives it where it lies, for the *Instanced entries that take a device table (they skip
    // instances that fail their limits).
    blok_scatter_info scatterModels(const blok_scatter_params& params, const std::vector<blok_scatter_entry>& entries) {
        blok_scatter_info info{};
        check(blok_hip_volume_scatter_models(m_ctx, &params, entries.data(), static_cast<uint32_t>(entries.size()), &info));
        return info;
    }
    std::vector<blok_instance> downloadScatter(uint64_t page = uint64_t(1) << 22) {
        blok_scatter_info info{};
        check(blok_hip_volume_scatter_info(m_ctx, &info));
        std::vector<blok_instance> out(info.n_placed);
        for (uint64_t at = 0; at < info.n_placed; at += page) check(blok_hip_volume_scatter_download(m_ctx, out.data() + at, at, std::min(page, info.n_placed - at)));
        return out;
    }
    const blok_instance* scatterTable(uint64_t* outCount) {
        const blok_instance* table = nullptr;
        check(blok_hip_volume_scatter_device(m_ctx, &table, outCount));
        return table;
    }
    // Reduces a region of the resident volume (world voxels, half-open, both null = the whole box) to `levels` coarser levels (1 .. 5), kept
    // on the device until the next reduce (blok_hip_volume_reduce): per cell of level j the counts of filled and of exposed voxels of its
    // 2^j cube and a voted material id (flags: BLOK_LOD_VOTE_EXPOSED).  Returns the grids and the counts.
    blok_lod_info reduceVolume(const int32_t* regionLo = nullptr, const int32_t* regionHi = nullptr, uint32_t levels = 1, uint32_t flags = 0) {
        blok_lod_info info{};
        check(blok_hip_volume_reduce(m_ctx, regionLo, regionHi, levels, flags, &info));
        return info;
    }
    // The terrain function over the world region [regionLo, regionHi) reduced to `levels` coarser levels without a volume
    // (blok_hip_terrain_reduce; flags: BLOK_LOD_VOTE_EXPOSED, BLOK_LOD_SEAMLESS): the snapshot reduceVolume fills, so lodInfo, downloadLod
    // and lodModel work behind it.  A volume that exists is left alone.
    blok_lod_info reduceTerrain(const blok_terrain_params& params, const int32_t* regionLo, const int32_t* regionHi, uint32_t levels = 1, uint32_t flags = 0) {
        blok_lod_info info{};
        check(blok_hip_terrain_reduce(m_ctx, &params, regionLo, regionHi, levels, flags, &info));
        return info;
    }
    blok_lod_info lodInfo() {
        blok_lod_info info{};
        check(blok_hip_volume_lod_info(m_ctx, &info));
        return info;
    }
    // A plane of a level of the last reduce, x fastest over the level's grid: plane 0 n and 1 e as uint16_t, 2 the ids as uint32_t.
    template <class T>
    std::vector<T> downloadLod(uint32_t level, uint32_t plane, uint64_t page = uint64_t(1) << 24) {
        if ((plane == 2) != (sizeof(T) == 4) || (sizeof(T) != 2 && sizeof(T) != 4)) throw std::runtime_error("blok::HipTracer: downloadLod: uint16_t for planes 0 and 1, uint32_t for plane 2");
        const blok_lod_info info = lodInfo();
        const uint64_t n = level >= 1 && level <= info.levels ? info.level[level - 1].n_cells : 0;
        std::vector<T> out(n);
        if (!n) check(blok_hip_volume_lod_download(m_ctx, level, plane, nullptr, 0, 0));
        for (uint64_t at = 0; at < n; at += page) check(blok_hip_volume_lod_download(m_ctx, level, plane, out.data() + at, at, std::min(page, n - at)));
        return out;
    }
    // The cells of a level of the last reduce with n >= minCount as a new model in the lattice of the level's grid (blok_hip_volume_lod_model).
    uint32_t lodModel(uint32_t level, uint32_t minCount = 1, uint64_t* outVoxels = nullptr) {
        uint32_t model = 0;
        check(blok_hip_volume_lod_model(m_ctx, level, minCount, &model, outVoxels));
        return model;
    }
    // Steps a neighbour-count rule over a region of the resident volume (world voxels, half-open, both null = the whole box), in place
    // (blok_hip_volume_automaton): smooth, despeckle, fill pits, caves, Life.  outStepCounts (may be null) takes the cells born and died
    // per step, 2 * rule.steps values.  Returns what the call did; the next rebuildVolume installs the world.
    blok_automaton_info volumeAutomaton(const blok_automaton_rule& rule, const int32_t* regionLo = nullptr, const int32_t* regionHi = nullptr,
                                        std::vector<uint64_t>* outStepCounts = nullptr) {
        blok_automaton_info info{};
        if (outStepCounts) outStepCounts->assign(rule.steps <= 255u ? 2 * size_t(rule.steps) : 0, 0);      // (more steps than that are refused)
        check(blok_hip_volume_automaton(m_ctx, regionLo, regionHi, &rule, outStepCounts && !outStepCounts->empty() ? outStepCounts->data() : nullptr, &info));
        return info;
    }
    void rebuildVolume(const std::vector<blok_material>& materials) { check(blok_hip_volume_rebuild(m_ctx, materials.data(), materials.size())); }

    // ---- image-space chain (Denoiser::denoise, PostProcess::process) over device planes; see include/blok_hip.h
    void denoise(const blok_gbuffer& planesDev, const float prevViewProj[16], uint32_t frameCount, float* outColorDev,
                 const blok_denoise_settings* settings = nullptr, const float* motionDev = nullptr, void* stream = nullptr) {
        check(blok_hip_denoise_device(m_ctx, &planesDev, motionDev, prevViewProj, frameCount, settings, outColorDev, stream));
    }
    void taa(const float* colorDev, float* outColorDev, uint32_t frameCount, float feedbackMin = 0.93f, float feedbackMax = 0.98f,
             const float* motionDev = nullptr, void* stream = nullptr) {
        check(blok_hip_taa_device(m_ctx, colorDev, motionDev, feedbackMin, feedbackMax, frameCount, outColorDev, stream));
    }
    // = Renderer::drawFrame's ray-tracing path: trace, denoise, TAA, tonemap, sharpen with the reference's default settings
    const std::vector<uint32_t>& drawFrameRT(Camera& cam, uint32_t sampleCount = 8, uint32_t maxBounces = 2) {
        const blok_camera c = cam.basis(m_width, m_height);
        m_pixels.resize(static_cast<size_t>(m_width) * m_height);
        check(blok_hip_draw_frame_rt(m_ctx, &c, sampleCount, maxBounces, nullptr, m_pixels.data(), &m_frameIndex));
        cam.cameraChanged = false;
        return m_pixels;
    }
    // drawFrameRT over the world plus instances (the same post state and frame counter)
    const std::vector<uint32_t>& drawFrameRTInstanced(Camera& cam, const std::vector<blok_instance>& instances, uint32_t sampleCount = 8,
                                                      uint32_t maxBounces = 2) {
        const blok_camera c = cam.basis(m_width, m_height);
        m_pixels.resize(static_cast<size_t>(m_width) * m_height);
        check(blok_hip_draw_frame_rt_instanced(m_ctx, &c, sampleCount, maxBounces, nullptr, instances.data(), static_cast<uint32_t>(instances.size()),
                                               m_pixels.data(), &m_frameIndex));
        cam.cameraChanged = false;
        return m_pixels;
    }
    // drawFrameRTInstanced with object motion: instance i keeps its history while its index and model stay the same from frame to frame
    const std::vector<uint32_t>& drawFrameRTInstancedMotion(Camera& cam, const std::vector<blok_instance>& instances, uint32_t sampleCount = 8,
                                                            uint32_t maxBounces = 2) {
        const blok_camera c = cam.basis(m_width, m_height);
        m_pixels.resize(static_cast<size_t>(m_width) * m_height);
        check(blok_hip_draw_frame_rt_instanced_motion(m_ctx, &c, sampleCount, maxBounces, nullptr, instances.data(),
                                                      static_cast<uint32_t>(instances.size()), m_pixels.data(), &m_frameIndex));
        cam.cameraChanged = false;
        return m_pixels;
    }
    // path-traced planes (host, any may be null) over the world plus instances; the first hit's instance per pixel in instanceIds()
    void tracePathsInstanced(Camera& cam, const std::vector<blok_instance>& instances, const blok_gbuffer& planesHost, uint32_t sampleCount = 8,
                             uint32_t maxBounces = 2, uint32_t frameIndex = 0) {
        const blok_camera c = cam.basis(m_width, m_height);
        m_instanceIds.resize(static_cast<size_t>(m_width) * m_height);
        check(blok_hip_trace_paths_instanced(m_ctx, &c, 0, 0, m_width, m_height, sampleCount, maxBounces, frameIndex, instances.data(),
                                             static_cast<uint32_t>(instances.size()), &planesHost, m_instanceIds.data()));
    }
    // drawFrameRTInstanced with posed models (blok_pose: any rotation, scale, mirror, shear) behind the instances; camera-only motion
    const std::vector<uint32_t>& drawFrameRtPosed(Camera& cam, const std::vector<blok_instance>& instances, const std::vector<blok_pose>& poses,
                                                  uint32_t sampleCount = 8, uint32_t maxBounces = 2) {
        const blok_camera c = cam.basis(m_width, m_height);
        m_pixels.resize(static_cast<size_t>(m_width) * m_height);
        check(blok_hip_draw_frame_rt_posed(m_ctx, &c, sampleCount, maxBounces, nullptr, instances.data(), static_cast<uint32_t>(instances.size()),
                                           poses.data(), static_cast<uint32_t>(poses.size()), m_pixels.data(), &m_frameIndex));
        cam.cameraChanged = false;
        return m_pixels;
    }
    // drawFrameRtPosed with object motion for tracked poses and instances (blok_hip.h, "Object motion for posed models"): the context keeps the
    // previous frame's two tables
    const std::vector<uint32_t>& drawFrameRtPosedMotion(Camera& cam, const std::vector<blok_instance>& instances, const std::vector<blok_pose>& poses,
                                                        uint32_t sampleCount = 8, uint32_t maxBounces = 2) {
        const blok_camera c = cam.basis(m_width, m_height);
        m_pixels.resize(static_cast<size_t>(m_width) * m_height);
        check(blok_hip_draw_frame_rt_posed_motion(m_ctx, &c, sampleCount, maxBounces, nullptr, instances.data(), static_cast<uint32_t>(instances.size()),
                                                  poses.data(), static_cast<uint32_t>(poses.size()), m_pixels.data(), &m_frameIndex));
        cam.cameraChanged = false;
        return m_pixels;
    }
    // tracePathsInstanced with posed models; instanceIds() holds BLOK_POSE_ID | index where a pose wins the first hit
    void tracePathsPosed(Camera& cam, const std::vector<blok_instance>& instances, const std::vector<blok_pose>& poses, const blok_gbuffer& planesHost,
                         uint32_t sampleCount = 8, uint32_t maxBounces = 2, uint32_t frameIndex = 0) {
        const blok_camera c = cam.basis(m_width, m_height);
        m_instanceIds.resize(static_cast<size_t>(m_width) * m_height);
        check(blok_hip_trace_paths_posed(m_ctx, &c, 0, 0, m_width, m_height, sampleCount, maxBounces, frameIndex, instances.data(),
                                         static_cast<uint32_t>(instances.size()), poses.data(), static_cast<uint32_t>(poses.size()), &planesHost,
                                         m_instanceIds.data()));
    }
    void sharpen(const uint32_t* rgba8Dev, uint32_t* outRgba8Dev, float strength = 0.5f, void* stream = nullptr) {
        check(blok_hip_sharpen_device(m_ctx, rgba8Dev, strength, outRgba8Dev, stream));
    }

    // ---- instanced voxel models (blok_hip.h): models uploaded once, placed per frame by an instance table
    uint32_t createModel(const std::vector<int32_t>& xyz, const std::vector<uint32_t>& materialIds) {
        if (xyz.size() != 3 * materialIds.size()) throw std::invalid_argument("HipTracer::createModel: three coordinates per voxel");
        uint32_t id = 0;
        check(blok_hip_model_create(m_ctx, xyz.data(), materialIds.data(), materialIds.size(), &id));
        return id;
    }
    void destroyModel(uint32_t model) { check(blok_hip_model_destroy(m_ctx, model)); }
    // one model voxel = a cube of 2^scaleLog2 world voxels (0..8; blok_hip.h: "Scaled models"); blocks, and forgets the previous frame's table
    void setModelScale(uint32_t model, uint32_t scaleLog2) { check(blok_hip_model_set_scale(m_ctx, model, scaleLog2)); }
    uint32_t modelScale(uint32_t model) {
        uint32_t e = 0;
        check(blok_hip_model_scale(m_ctx, model, &e));
        return e;
    }
    // drawFrame over the world plus instances: records in hits(), the winning instance per pixel in instanceIds()
    void drawFrameInstanced(Camera& cam, const std::vector<blok_instance>& instances) {
        const blok_camera c = cam.basis(m_width, m_height);
        m_instanceIds.resize(static_cast<size_t>(m_width) * m_height);
        check(blok_hip_trace_primary_instanced(m_ctx, &c, 0, 0, m_width, m_height, instances.data(), static_cast<uint32_t>(instances.size()),
                                               m_hits.data(), nullptr, m_instanceIds.data()));
        cam.cameraChanged = false;
        ++m_frameIndex;
    }
    // picking / line of sight: records and instance ids of explicit rays
    void traceRaysInstanced(const std::vector<blok_ray>& rays, const std::vector<blok_instance>& instances, std::vector<blok_hit>& outHits,
                            std::vector<uint32_t>& outInstanceIds) {
        outHits.resize(rays.size());
        outInstanceIds.resize(rays.size());
        check(blok_hip_trace_rays_instanced(m_ctx, rays.data(), rays.size(), instances.data(), static_cast<uint32_t>(instances.size()),
                                            outHits.data(), outInstanceIds.data()));
    }
    const std::vector<uint32_t>& instanceIds() const { return m_instanceIds; }
    // ---- posed models (blok_hip.h, "Posed models"): instanced models under any rotation, scale, mirror or shear (records from
    // blok_pose_from_instance / blok_pose_from_matrix, blok_world.h).  A pixel a pose wins has id BLOK_POSE_ID | index in instanceIds() and
    // the model's local voxel and face in its record.
    void checkPoses(const std::vector<blok_pose>& poses) { check(blok_hip_check_poses(m_ctx, poses.data(), static_cast<uint32_t>(poses.size()))); }
    // the first-hit frame (or a rectangle of it) over the world, the instances and the poses, into host arrays; any output may be null, not all
    void tracePrimaryPosed(Camera& cam, const std::vector<blok_instance>& instances, const std::vector<blok_pose>& poses, blok_hit* outHits,
                           uint32_t* outRgba, uint32_t* outIds, uint32_t x0 = 0, uint32_t y0 = 0, uint32_t w = 0, uint32_t h = 0) {
        const blok_camera c = cam.basis(m_width, m_height);
        check(blok_hip_trace_primary_posed(m_ctx, &c, x0, y0, w ? w : m_width, h ? h : m_height, instances.data(), static_cast<uint32_t>(instances.size()),
                                           poses.data(), static_cast<uint32_t>(poses.size()), outHits, outRgba, outIds));
    }
    // drawFrameInstanced with a pose table: records in hits(), ids in instanceIds()
    void drawFramePosed(Camera& cam, const std::vector<blok_instance>& instances, const std::vector<blok_pose>& poses) {
        m_instanceIds.resize(static_cast<size_t>(m_width) * m_height);
        tracePrimaryPosed(cam, instances, poses, m_hits.data(), nullptr, m_instanceIds.data());
        cam.cameraChanged = false;
        ++m_frameIndex;
    }

    const std::vector<blok_hit>& hits() const { return m_hits; }     // output accessor (getGLTex analogue)
    unsigned int width() const { return m_width; }
    unsigned int height() const { return m_height; }
    blok_hip_ctx* handle() { return m_ctx; }
    blok_world_stats worldStats() const {
        blok_world_stats s{};
        if (blok_hip_world_stats(m_ctx, &s) != BLOK_OK) throw std::runtime_error("HipTracer: no world");
        return s;
    }

private:
    void check(int rc) const { if (rc != BLOK_OK) throw std::runtime_error(std::string("HipTracer: ") + blok_hip_last_error(m_ctx)); }
    template <class T>
    std::vector<T> downloadColumnPlane(uint32_t plane, uint64_t page) {
        blok_columns_info info{};
        check(blok_hip_volume_columns_info(m_ctx, &info));
        std::vector<T> out(info.n_columns);
        for (uint64_t at = 0; at < info.n_columns; at += page) check(blok_hip_volume_columns_download(m_ctx, plane, out.data() + at, at, std::min(page, info.n_columns - at)));
        return out;
    }

    unsigned int m_width = 0, m_height = 0;
    int m_device = 0;
    blok_hip_ctx* m_ctx = nullptr;
    WorldSvoGpu* m_world = nullptr;       // non-owning, like reference renderer.hpp:195
    uint32_t m_frameIndex = 0;
    std::vector<blok_hit> m_hits;
    std::vector<uint32_t> m_pixels;
    std::vector<uint32_t> m_instanceIds;
};

// Several devices of one node, one process (blok_hip_multi_*, blok_hip.h): the frame is cut into tile x tile screen tiles dealt
// round-robin to the devices, the world is replicated, the RGBA8 tiles are gathered on the first device over xGMI (RCCL
// send / receive group, or peer copies) and un-permuted there.  No reference counterpart: blok is single-GPU.
class HipMultiTracer {
public:
    HipMultiTracer(const std::vector<int>& devices, unsigned width, unsigned height, unsigned tile = 32, bool allowRccl = true)
        : m_width(width), m_height(height) {
        if (blok_hip_multi_create(&m_multi, devices.data(), static_cast<uint32_t>(devices.size()), width, height, tile, allowRccl ? 1 : 0) != BLOK_OK)
            throw std::runtime_error(std::string("HipMultiTracer: ") + blok_hip_multi_last_error(nullptr));
    }
    ~HipMultiTracer() { shutdown(); }
    HipMultiTracer(const HipMultiTracer&) = delete;
    HipMultiTracer& operator=(const HipMultiTracer&) = delete;

    void shutdown() { if (m_multi) { blok_hip_multi_destroy(m_multi); m_multi = nullptr; } }
    unsigned deviceCount() const { return blok_hip_multi_device_count(m_multi); }
    std::string transport() const { return blok_hip_multi_transport(m_multi); }
    blok_hip_ctx* context(unsigned rank) { return blok_hip_multi_context(m_multi, rank); }

    void addWorld(const WorldSvoGpu& w) {                       // = Renderer::addWorld on every device
        check(blok_hip_multi_upload_world(m_multi, w.globalNodes.data(), w.globalNodes.size(), w.globalSubChunks.data(), w.globalSubChunks.size(),
                                          w.materials.data(), w.materials.size()));
    }
    // One frame: RGBA8, row-major, width x height, on the host.
    void drawFrame(const Camera& c, std::vector<uint32_t>& rgba8) {
        rgba8.resize(static_cast<size_t>(m_width) * m_height);
        const blok_camera basis = c.basis(m_width, m_height);
        check(blok_hip_multi_draw_frame(m_multi, &basis, rgba8.data()));
    }
    // Asynchronous form: the frame stays on the root device.
    const uint32_t* drawFrameDevice(const Camera& c) {
        const blok_camera basis = c.basis(m_width, m_height);
        const uint32_t* frame = nullptr;
        check(blok_hip_multi_draw_frame_device(m_multi, &basis, &frame));
        return frame;
    }
    void synchronize() { check(blok_hip_multi_synchronize(m_multi)); }
    // Several frames per call (1..BLOK_MAX_TILE_FRAMES cameras, one launch pair per device); the frames follow one another in rgba8.
    void drawFrames(const std::vector<Camera>& cams, std::vector<uint32_t>& rgba8) {
        std::vector<blok_camera> basis;
        for (const Camera& c : cams) basis.push_back(c.basis(m_width, m_height));
        rgba8.resize(cams.size() * static_cast<size_t>(m_width) * m_height);
        check(blok_hip_multi_draw_frames(m_multi, basis.data(), static_cast<uint32_t>(basis.size()), rgba8.data()));
    }
    // How the tiles reach the root: -1 = sparse-pull when possible (default), 0 = dense, 1 = sparse-pull or an exception (blok_hip.h).
    void setExchange(int mode) { check(blok_hip_multi_set_exchange(m_multi, mode)); }
    std::string exchange() const { return blok_hip_multi_exchange(m_multi); }

private:
    void check(int rc) const { if (rc != BLOK_OK) throw std::runtime_error(std::string("HipMultiTracer: ") + blok_hip_multi_last_error(m_multi)); }
    blok_hip_multi* m_multi = nullptr;
    unsigned m_width, m_height;
};

}  // namespace blok
#endif
