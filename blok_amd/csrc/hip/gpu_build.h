// Device-side build of the 64-tree (gpu_build.hip).
#ifndef BLOK_GPU_BUILD_H
#define BLOK_GPU_BUILD_H
#include <hip/hip_runtime.h>

#include <string>

#include "blok_hip.h"
#include "edit_log.h"
#include "tree.h"
#include "volume_device.h"

namespace blok {

struct GpuTree {
    uint4* d_nodes = nullptr;        // root first; ownership passes to the caller on Ok
    uint32_t* d_materials = nullptr;
    size_t n_nodes = 0;
    uint64_t n_voxels = 0;
    uint32_t levels = 0;
    int32_t origin[3] = {0, 0, 0};
    bool owned_by_volume = false;    // the arrays belong to a GpuVolume's scratch (never freed by the holder)
};

enum class GpuBuildStatus { Ok, UseHostBuilder, Unsupported, HipError, OutOfMemory, Internal };

// UseHostBuilder: the world is valid but outside what the kernels cover (empty, sub-chunks smaller than a brick or of
// mixed sizes, overlapping sub-chunks); the caller then takes the general host path (tree_build.cpp).
GpuBuildStatus gpu_build_tree(const blok_svo_node* nodes, size_t n_nodes, const blok_sub_chunk* subs, size_t n_subs,
                              GpuTree* out, std::string* why);

// Same, from a dense id grid ids[x + y*nx + z*nx*ny] (0 = empty) whose voxel (0,0,0) sits at world `origin`.
GpuBuildStatus gpu_build_tree_dense(const uint32_t* ids, uint32_t nx, uint32_t ny, uint32_t nz, const int32_t origin[3],
                                    GpuTree* out, std::string* why);

// ---- device-resident dense voxel store: the reference's Chunk::density / Chunk::materialIds (blok/src/chunk.hpp:33-42)
// for one box of the world, kept in HBM together with the 64-bit voxel mask of every 4^3 brick, so that edits
// (brush.cpp:13-63, chunk_manager.cpp:316-328) and the rebuild they trigger (chunk_manager.cpp:106-140) never leave
// the device.  A voxel is filled iff density > 0 (chunk_manager.cpp:121).
struct GpuVolume {
    float* d_density = nullptr;      // [x + y*nx + z*nx*ny]
    uint32_t* d_ids = nullptr;
    uint64_t* d_masks = nullptr;     // one per brick, brick (bx, by, bz) at bx + by*nbx + bz*nbx*nby
    uint32_t* d_flag = nullptr;      // mask != 0, total + 1 entries (the last one is a zero sentinel for the scan)
    uint32_t* d_slot = nullptr;      // scan scratch, total + 1
    uint32_t nx = 0, ny = 0, nz = 0, nbx = 0, nby = 0, nbz = 0, levels = 0;
    int32_t origin[3] = {0, 0, 0};
    uint32_t chunk = 128;            // ChunkManager's chunk edge (the brush computes voxel centres per chunk)
    float voxel_size = 1.0f;
    uint64_t cells() const { return static_cast<uint64_t>(nx) * ny * nz; }
    uint64_t bricks() const { return static_cast<uint64_t>(nbx) * nby * nbz; }

    // KEY layout (volumes whose tree has <= 5 levels, and larger ones that fill their cube; gpu_build.hip: rebuild in ~0.2 ms).  Bricks are
    // indexed by their key — the 2-bit digit triples of levels 1..L-1 of the brick's coordinates, least significant level first: the
    // order of the tree's level-1 nodes — so d_masks has 64^(L-1) entries and the non-empty bricks, taken in index order, ARE the sorted
    // brick list: no scan over all bricks, no sort.  Above the masks lies a pyramid of occupancy words: bit b of d_occ[l][c] = cell
    // 64 c + b of level l-1 holds a voxel (l = 2: brick 64 c + b), kept up to date by the edits for the cells they touch.  A non-zero
    // word IS the mask of the tree node of that cell, and the two exclusive scans of a level — of the words' popcounts and of
    // "word != 0" — are the nodes' child indices and the nodes' own ranks.  A rebuild is those scans (262 144 words at level 2 of a
    // 1024^3 world, a handful above), the gather of the non-empty bricks' masks and material ids, and the node writes.
    bool keyed = false;
    uint64_t n_keys = 0;                         // 64^(levels-1)
    uint64_t* d_occ[8] = {nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr};      // [2 .. levels]
    uint8_t* d_dirty = nullptr;                  // per brick key: its voxels may have changed since the last build (material ids are gathered again)
    // kept between rebuilds (grown on demand): scratch, and two sets of output arrays so that the tree the tracer holds stays valid while the next is built
    struct Scratch {
        void* d_scan_temp = nullptr; size_t scan_temp_bytes = 0;
        uint64_t* d_packed[8] = {};              // per level: (word != 0) << 32 | popcount(word), and ...
        uint64_t* d_scanned[8] = {};             // ... its exclusive scan: rank of the cell's node << 32 | index of its first child within the level below
        uint32_t* d_cells2 = nullptr; uint64_t cells2_capacity = 0;      // the non-empty level-2 cells, in order
        uint64_t* d_masks_sorted = nullptr; uint32_t *d_src = nullptr, *d_counts = nullptr, *d_mat_base = nullptr; uint64_t brick_capacity = 0;
        uint32_t* d_old_base = nullptr;          // per brick key: where the brick's material ids lie in the previous output (0xFFFFFFFF: nowhere)
        uint64_t* d_info = nullptr;              // device words the kernels pass totals through; [0..7] level totals, [8] voxels, [9..16] level offsets
        uint4* d_tree[2] = {nullptr, nullptr}; uint64_t tree_capacity[2] = {0, 0};
        uint32_t* d_materials[2] = {nullptr, nullptr}; uint64_t material_capacity[2] = {0, 0};
        int current = -1;                        // output set the tracer holds (-1: none)
        bool have_previous_materials = false;
    } scratch;
    EditLog edits;                               // the edits since the last build (edit_log.h): gpu_volume_commit notes, the rebuild takes
    uint64_t refreshes[3] = {0, 0, 0};           // diagnostic: mask refreshes since creation — keyed, an edit's path (a wave per brick, the pyramid in one workgroup); keyed, an upload's path (a lane per brick, a launch per level); general layout
};

// The volume's brick masks as a kernel reads them, in whichever layout the volume has (volume_device.h).
inline BrickMasks brick_masks_of(const GpuVolume& v) { return BrickMasks{v.d_masks, v.nbx, v.nby, v.keyed ? v.levels - 1u : 0u}; }

GpuBuildStatus gpu_volume_create(const int32_t origin[3], uint32_t nx, uint32_t ny, uint32_t nz, uint32_t chunk, float voxel_size,
                                 GpuVolume* out, std::string* why, bool allow_keyed = true);
void gpu_volume_destroy(GpuVolume* v);
// Whole-box upload from host arrays (either may be null = zeros) and recomputation of every brick mask.
GpuBuildStatus gpu_volume_upload(GpuVolume* v, const float* density, const uint32_t* ids, std::string* why);
GpuBuildStatus gpu_volume_download(const GpuVolume* v, float* density, uint32_t* ids, std::string* why);
// = ChunkManager::setVoxelMaterial for n world voxels (later entries win); voxels outside the box -> Unsupported.
GpuBuildStatus gpu_volume_set_voxels(GpuVolume* v, const int32_t* xyz, const uint32_t* material, const float* density, size_t n,
                                     std::string* why);
// What every operation that has written the store owes the rest of the system, in one call (the upload and the edits above, and every
// edit below; voxelize_kernels.hip and the others write the store themselves): the masks, occupancy words and dirty flags of the bricks
// that hold voxels [lo, hi) (box-local) recomputed from the dense store, on the null stream behind the writes, and the box and `kind`
// noted in v->edits.  MayFill: the operation may have made an empty voxel filled (density > 0); OnlyClears: it cannot have.  An empty
// box is Ok and notes nothing.
enum class Edit { OnlyClears, MayFill };
GpuBuildStatus gpu_volume_commit(GpuVolume* v, const uint32_t lo[3], const uint32_t hi[3], Edit kind, std::string* why);
// What an operation owes that has replaced the brick masks as a whole and kept them equal to density > 0 itself (the scroll): the
// occupancy words of every level from the masks as they are, by the launches of a whole-box commit; every brick dirty and without a place
// in the previous build's material array, so that the next build gathers every id from the store.  Reads no density.  Notes nothing in
// v->edits.
GpuBuildStatus gpu_volume_masks_replaced(GpuVolume* v, std::string* why);
// = blok_hip_volume_scroll (include/blok_hip.h; scroll_kernels.hip) by a delta that has passed scroll::check_args: the filled voxels of the
// old box and of the kept cells, from the old and the moved masks; with `write` the move itself — the dense arrays and the masks out of
// place into arrays allocated for the call (8 bytes per cell and a mask array beside the volume's own while it runs; an in-place move,
// with its ordering per axis, is next), which the volume adopts, the old ones freed once the device has finished, then
// gpu_volume_masks_replaced.  Without it nothing is written.  v->origin and v->edits are the caller's.  Blocking.  A failure before the
// arrays are adopted leaves the volume as it was.
GpuBuildStatus gpu_volume_scroll(GpuVolume* v, const int32_t delta[3], bool write, uint64_t* out_n_filled_before, uint64_t* out_n_filled_kept,
                                 std::string* why);
// = blok_hip_volume_apply_shapes (include/blok_hip.h; shapes_kernels.hip): a host table that has passed shapes::check, applied in order in
// one pass over the tiles its shapes touch, then one gpu_volume_commit per group of shapes whose brick-aligned boxes overlap.  Blocking.
GpuBuildStatus gpu_volume_apply_shapes(GpuVolume* v, const blok_shape* shapes, uint32_t n_shapes, uint64_t* out_n_written, std::string* why);
// = blok_hip_volume_voxelize_mesh (include/blok_hip.h; voxelize_kernels.hip).  Host arrays.  *invalid: a referenced vertex, an index or a
// triangle's extent is out of the limits (nothing written).
GpuBuildStatus gpu_volume_voxelize(GpuVolume* v, const float* positions, size_t n_vertices, const uint32_t* triangles, size_t n_triangles,
                                   const uint32_t* triangle_materials, uint32_t material, float density, bool solid, uint64_t* out_n_voxels,
                                   bool* invalid, std::string* why);
// = blok_hip_volume_generate_terrain (include/blok_hip.h; terrain_kernels.hip) over the box-local region [lo, hi); the parameters have
// passed terrain::check_params.
GpuBuildStatus gpu_volume_generate_terrain(GpuVolume* v, const blok_terrain_params& params, const uint32_t lo[3], const uint32_t hi[3],
                                           uint64_t* out_n_voxels, std::string* why);
// ---- snapshots ----
// What an entry leaves on the device for later calls is a holder that owns its arrays and knows whether it was taken: a default-constructed
// holder is no snapshot, a taken one whose pointers are null is the snapshot of an empty region.  The entry that takes a snapshot sets
// `taken`; gpu_*_free frees the arrays and leaves the holder default-constructed.
// = blok_hip_volume_extract_quads (include/blok_hip.h; quads_kernels.hip) over the box-local region [lo, hi).  Reads the store, changes
// nothing.  out->n_quads counts the records; without BLOK_QUADS_COUNT_ONLY out->d_quads is a new device array of them (null for none), the
// caller's to free.
struct GpuQuads {
    blok_quad* d_quads = nullptr;
    uint64_t n_quads = 0;
    bool taken = false;
    uint32_t flags = 0;             // of the extraction (BLOK_QUADS_IGNORE_MATERIAL: the keys are no material ids)
};
void gpu_quads_free(GpuQuads* q);
// = blok_hip_lights_from_quads (include/blok_hip.h; lights_kernels.hip): the quads whose key maps to a set bit of d_glows (the emissive
// material indices, lights_core.h), in the quads' order, with the running sum of du * dv; d_owned (kSetWords words) takes the set of
// the kept quads' material indices.  out->d_lights is a new device array (null for none), the caller's to free.  Unsupported: 2^31 or
// more lights, 2^32 or more unit faces.  One wait, for the two totals.
struct GpuLights {
    blok_light* d_lights = nullptr;
    uint32_t n = 0;
    uint64_t n_faces = 0;
};
GpuBuildStatus gpu_lights_from_quads(const blok_quad* d_quads, uint64_t n_quads, const uint32_t* d_glows, uint32_t n_materials, uint32_t* d_owned,
                                     GpuLights* out, std::string* why);
// = blok_hip_model_lights (lights_kernels.hip): the table of a model's exposed emissive unit faces from its own tree in device memory (the
// arrays' lengths as the store keeps them), in the order of its material array; out->n_faces == out->n.  Null stream; waits for the count.
GpuBuildStatus gpu_model_lights(const uint4* d_nodes, uint32_t n_nodes, const uint32_t* d_materials, uint32_t n_voxels, uint32_t levels, const int32_t origin[3],
                                const uint32_t* d_glows, uint32_t n_materials, GpuLights* out, std::string* why);
// = blok_hip_build_light_grid (include/blok_hip.h; lights_kernels.hip) over a table in device memory that has passed lights::check_table
// and parameters that have passed lights::grid_params_ok.  The three arrays are new device arrays, the caller's to free.  Unsupported: the
// grid's limits.  Null stream; waits once for {bounds, n_items} before it allocates the result, and once at the end for the two figures
// of the lists' lengths.
struct GpuLightGrid {
    uint32_t* d_start = nullptr;        // n_cells + 1
    uint32_t* d_faces = nullptr;        // n_cells
    blok_light_grid_item* d_items = nullptr;
    blok_light_grid_info info{};
};
GpuBuildStatus gpu_light_grid_build(const blok_light* d_lights, uint32_t n, uint32_t cell_log2, uint32_t reach, uint32_t share, GpuLightGrid* out,
                                    std::string* why);
struct ModelDesc;
namespace lights { struct ModelLightTable; }
// The per-launch prefix of an instance table (lights_core.h): icum, n + 1 words, and the 32-byte header behind them at `header`
// (= blok_instance_lights_info), on `stream`; one workgroup, no atomics.  tables: one entry per model id (n_models of both arrays).
void launch_instance_lights_prefix(const blok_instance* instances, uint32_t n, const ModelDesc* models, const lights::ModelLightTable* tables, uint32_t n_models,
                                   uint64_t a_world, float voxel_size, uint32_t* icum, blok_instance_lights_info* header, hipStream_t stream);
GpuBuildStatus gpu_volume_extract_quads(const GpuVolume* v, const uint32_t lo[3], const uint32_t hi[3], uint32_t flags, GpuQuads* out,
                                        uint64_t* out_n_faces, std::string* why);
// = blok_hip_volume_stamp_models (include/blok_hip.h; stamp_kernels.hip).  The placements have passed the entry's checks; models[i] is
// the model of placements[i], read in device memory through its tree.  One launch and one gpu_volume_commit per placement, in table order on the
// null stream; the only wait is the one for the count at the end.
struct StampModel {
    const uint4* nodes; const uint32_t* materials;      // tree.h, device memory
    uint32_t levels;
    int32_t origin[3], lo[3], hi[3];                    // the tree's corner and the box of its voxels, local coordinates
};
// The bricks of the model's tree, counted from its corner, that hold the voxels of the non-empty local box [clo, chi): [b0, b0 + nb).
inline void placed_brick_range(const StampModel& M, const int64_t clo[3], const int64_t chi[3], uint32_t b0[3], uint32_t nb[3]) {
    for (int k = 0; k < 3; ++k) {
        b0[k] = static_cast<uint32_t>((clo[k] - M.origin[k]) >> 2);
        nb[k] = static_cast<uint32_t>((chi[k] - 1 - M.origin[k]) >> 2) - b0[k] + 1u;
    }
}
GpuBuildStatus gpu_volume_stamp(GpuVolume* v, const StampModel* models, const blok_instance* placements, uint32_t n_placements, int mode,
                                float density, uint64_t* out_n_voxels, std::string* why);
// = blok_hip_volume_stamp_affine (include/blok_hip.h; affine_kernels.hip) over the box-local region [lo, hi).  The records have passed
// affine::well_formed against the volume's box; models[i] is the model of records[i], lo / hi the box of its voxels in its OWN voxels
// whatever its scale exponent.  Per record the host culls the region's coarse tiles by the exact interval of the map, then one launch over
// the surviving box and one gpu_volume_commit over it, in table order on the null stream; the only wait is the one for the count at the end.
GpuBuildStatus gpu_volume_stamp_affine(GpuVolume* v, const StampModel* models, const blok_affine* records, uint32_t n_records, const uint32_t lo[3],
                                       const uint32_t hi[3], int mode, float density, uint64_t* out_n_voxels, std::string* why);
// = blok_hip_volume_capture_model (include/blok_hip.h) over the box-local region [lo, hi): the tree of the region's filled voxels in the
// lattice whose voxel (0, 0, 0) is the region's corner, built on the device.  On Ok with *out_n_voxels > 0, out->d_nodes /
// d_materials are new device arrays, the caller's to free, and box_lo / box_hi the tight box of the voxels (half open, model
// coordinates); with *out_n_voxels == 0 (nothing filled) there is no tree.  Reads the store, changes nothing.
GpuBuildStatus gpu_volume_capture(const GpuVolume* v, const uint32_t lo[3], const uint32_t hi[3], GpuTree* out, int32_t box_lo[3],
                                  int32_t box_hi[3], uint64_t* out_n_voxels, std::string* why);
// Clears (density 0, id 0) the filled voxels of the box-local box [lo, hi) and commits it (Edit::OnlyClears): BLOK_CAPTURE_CUT.
GpuBuildStatus gpu_volume_clear_filled(GpuVolume* v, const uint32_t lo[3], const uint32_t hi[3], std::string* why);
// ---- connected components (include/blok_hip.h: blok_hip_volume_label_components; components_kernels.hip) ----
// The snapshot of one labelling, device memory owned by the holder: the label array of the region's cells, the records sorted by label,
// and — to find a label's record without a search — per row of 64 cells the bits of the cells that are roots and, packed in one word,
// the exclusive sums over the rows of (filled cells) << 32 | roots: record of root r = low word of d_row_base[r / 64] + popcount of
// d_root_bits[r / 64] below bit r % 64.
struct GpuComponents {
    uint32_t* d_labels = nullptr;
    blok_component* d_records = nullptr;
    uint64_t* d_root_bits = nullptr;
    uint64_t* d_row_base = nullptr;
    uint64_t n_cells = 0, n_components = 0, n_voxels = 0;
    uint32_t lo[3] = {0, 0, 0}, ext[3] = {0, 0, 0};      // the region, box-local
    bool taken = false;
};
void gpu_components_free(GpuComponents* c);
// Labels the box-local region [lo, hi) from the brick masks (which every edit leaves equal to density > 0).  Reads the store, changes
// nothing; *out is a new snapshot, the caller's to free (empty, all pointers null, when the region has no cell).  Blocking.
GpuBuildStatus gpu_volume_label_components(const GpuVolume* v, const uint32_t lo[3], const uint32_t hi[3], GpuComponents* out, std::string* why);
// The record of `label` in the snapshot; *found = false when no record has that label.
GpuBuildStatus gpu_components_find(const GpuComponents* c, uint32_t label, blok_component* out, bool* found, std::string* why);
// = blok_hip_volume_capture_component: gpu_volume_capture over the record's box [lo, hi) (box-local), restricted to the voxels whose
// cell in the snapshot holds `label`; model coordinates are relative to lo.
GpuBuildStatus gpu_volume_capture_labelled(const GpuVolume* v, const GpuComponents* c, uint32_t label, const uint32_t lo[3], const uint32_t hi[3],
                                           GpuTree* out, int32_t box_lo[3], int32_t box_hi[3], uint64_t* out_n_voxels, std::string* why);
// gpu_volume_clear_filled under the same restriction: BLOK_COMPONENT_CUT.
GpuBuildStatus gpu_volume_clear_labelled(GpuVolume* v, const GpuComponents* c, uint32_t label, const uint32_t lo[3], const uint32_t hi[3],
                                         std::string* why);
// = blok_hip_volume_sweep_models (include/blok_hip.h; sweep_kernels.hip).  The placements, direction and flags have passed the entry's
// checks; models[i] is the model of placements[i].  Reads the brick masks and the models' trees, changes nothing.  One upload, one launch
// for the whole table on the null stream, one download (the call's wait); out_results has n_placements records, host memory.
GpuBuildStatus gpu_volume_sweep(const GpuVolume* v, const StampModel* models, const blok_instance* placements, uint32_t n_placements,
                                uint32_t direction, uint32_t max_distance, uint32_t flags, blok_sweep_result* out_results, std::string* why);
// ---- the sparse brick stream (include/blok_hip.h: blok_hip_volume_encode_bricks; bricks_kernels.hip) ----
// A stream in device memory, owned by the holder: records sorted by brick, the two payloads, and the info that counts them.
struct GpuBricks {
    blok_brick_record* d_records = nullptr;
    uint32_t* d_density = nullptr;
    uint32_t* d_material = nullptr;
    blok_bricks_info info = {};
    bool taken = false;
};
void gpu_bricks_free(GpuBricks* b);
// Encodes the box-local region [lo, hi) (flags: BLOK_BRICKS_FILLED_ONLY or 0).  Reads the store (and, with FILLED_ONLY on a region whose
// corner lies on the brick grid, the brick masks), changes nothing; *out is a new stream, the caller's to free (all pointers null when
// nothing is stored).  Blocking.
GpuBuildStatus gpu_volume_encode_bricks(const GpuVolume* v, const uint32_t lo[3], const uint32_t hi[3], uint32_t flags, GpuBricks* out, std::string* why);
// Writes a stream whose arrays lie in device memory into [dst_lo, dst_lo + info.ext) (box-local, inside the box; flags:
// BLOK_BRICKS_KEEP_OTHERS or 0), then commits that box as every edit does (gpu_volume_commit).  The stream is one gpu_volume_encode_bricks made or one that
// has passed bricks::validate: the kernel trusts its indices.  Blocking.
GpuBuildStatus gpu_volume_decode_bricks(GpuVolume* v, const GpuBricks* stream, const uint32_t dst_lo[3], uint32_t flags, std::string* why);
// ---- the fields (distance_kernels.hip, flood_kernels.hip) ----
// A field in device memory, owned by the holder: one uint16 per region cell, x fastest, and an info that counts them.
struct GpuField {
    uint16_t* d_field = nullptr;
    uint32_t lo[3] = {0, 0, 0};                  // the region's corner, box-local
    bool taken = false;
};
template <class Field>
void gpu_field_free(Field* f) {
    if (f->d_field) (void)hipFree(f->d_field);
    *f = Field{};
}
// ---- the distance field (include/blok_hip.h: blok_hip_volume_distance_field; distance_kernels.hip) ----
struct GpuDistance : GpuField {
    blok_distance_info info = {};
};
// The field of the box-local region [lo, hi) with max_radius <= 255 and known flags, from the brick masks (which every edit leaves equal to
// density > 0).  Changes nothing; *out is a new snapshot, the caller's to free (d_field null when the region has no cell).  Blocking.
GpuBuildStatus gpu_volume_distance_field(const GpuVolume* v, const uint32_t lo[3], const uint32_t hi[3], uint32_t max_radius, uint32_t flags,
                                         GpuDistance* out, std::string* why);
// = blok_hip_volume_edit_by_distance over the snapshot's region (inside the box); the arguments have passed distance::check_edit_args.
// Writes the store, then commits the region as every edit does (gpu_volume_commit).  Blocking.
GpuBuildStatus gpu_volume_edit_by_distance(GpuVolume* v, const GpuDistance* field, int op, uint32_t d2, float density, uint32_t material,
                                           uint64_t* out_n_voxels, std::string* why);
// ---- the flood from seeds (include/blok_hip.h: blok_hip_volume_flood_field; flood_kernels.hip) ----
// rounds and visits say how the device got there (launches over a non-empty list, bricks taken off the lists): diagnostics, never part of
// the info.
struct GpuFlood : GpuField {
    blok_flood_info info = {};
    uint64_t rounds = 0, visits = 0;
};
// The field of the box-local region [lo, hi) from n_seeds world cells inside it (host memory) and the SEED_FACE bits; the arguments have
// passed flood::check_field_args.  Reads the brick masks (which every edit leaves equal to density > 0), with SAME_MATERIAL the store.
// Changes nothing; *out is a new snapshot, the caller's to free (d_field null when the region has no cell).  Blocking.  Internal: the
// rounds did not end within max_steps + 2.
GpuBuildStatus gpu_volume_flood_field(const GpuVolume* v, const uint32_t lo[3], const uint32_t hi[3], const int32_t* seeds_xyz, uint64_t n_seeds,
                                      uint32_t max_steps, uint32_t flags, uint32_t material, GpuFlood* out, std::string* why);
// = blok_hip_volume_edit_by_flood over the snapshot's region (inside the box); the arguments have passed flood::check_edit_args.
// Writes the store, then commits the region as every edit does (gpu_volume_commit).  Blocking.
GpuBuildStatus gpu_volume_edit_by_flood(GpuVolume* v, const GpuFlood* field, int op, uint32_t d, float density, uint32_t material,
                                        uint64_t* out_n_voxels, std::string* why);
// ---- the column field and scatter (include/blok_hip.h: blok_hip_volume_column_field, blok_hip_volume_scatter_models; columns_kernels.hip) ----
// The column snapshot in device memory, owned by the holder: one top and one material id per column, and the info that counts them.
struct GpuColumns {
    uint16_t* d_top = nullptr;
    uint32_t* d_material = nullptr;
    uint32_t lo[3] = {0, 0, 0};                  // the region's corner, box-local
    blok_columns_info info = {};
    bool taken = false;
};
void gpu_columns_free(GpuColumns* c);
// The field of the box-local region [lo, hi) along `axis` (arguments that have passed columns::check_field_args), from the brick masks
// (which every edit leaves equal to density > 0) and one id per column that hits.  Changes nothing; *out is a new snapshot, the caller's
// to free (pointers null when the region has no cell).  Blocking.
GpuBuildStatus gpu_volume_column_field(const GpuVolume* v, const uint32_t lo[3], const uint32_t hi[3], uint32_t axis, uint32_t flags, GpuColumns* out,
                                       std::string* why);
// The table scatter leaves in device memory, owned by the holder: info.n_placed records in column order.
struct GpuScatter {
    blok_instance* d_table = nullptr;
    blok_scatter_info info = {};
    bool taken = false;
};
void gpu_scatter_free(GpuScatter* s);
// = blok_hip_volume_scatter_models over a column snapshot; the arguments (entries in host memory) have passed columns::check_scatter_args.
// Reads the snapshot alone; *out is a new table, the caller's to free (d_table null when nothing was placed).  Blocking.
GpuBuildStatus gpu_columns_scatter(const GpuColumns* columns, const blok_scatter_params& params, const blok_scatter_entry* entries, uint32_t n_entries,
                                   GpuScatter* out, std::string* why);
// ---- the pyramid of coarser levels (include/blok_hip.h: blok_hip_volume_reduce; lod_kernels.hip) ----
// The snapshot in device memory, owned by the holder: one array with the levels' planes one behind the other (../common/lod_core.h:
// level_offset, plane_offset), and the info that counts them.
struct GpuLod {
    void* d_planes = nullptr;
    blok_lod_info info = {};
    bool taken = false;
};
void gpu_lod_free(GpuLod* l);
// Reduces the box-local region [lo, hi) `levels` times (arguments that have passed lod::check_args), from the brick masks (which every edit
// leaves equal to density > 0) and the ids of the filled cells.  Changes nothing; *out is a new snapshot, the caller's to free (d_planes
// null when the region has no cell).  Blocking.
GpuBuildStatus gpu_volume_reduce(const GpuVolume* v, const uint32_t lo[3], const uint32_t hi[3], uint32_t levels, uint32_t flags, GpuLod* out,
                                 std::string* why);
// = blok_hip_terrain_reduce: the same snapshot for the world region [lo, hi) of the terrain function, level 1 from the function itself
// (arguments that have passed terrain::check_params, lod::check_args and terrain_lod::check_region).  Needs no volume and touches none.
GpuBuildStatus gpu_terrain_reduce(const blok_terrain_params& params, const int32_t lo[3], const int32_t hi[3], uint32_t levels, uint32_t flags,
                                  GpuLod* out, std::string* why);
// = blok_hip_volume_lod_model: gpu_volume_capture over a level of the snapshot, a cell filled iff its n >= min_count, its id the voted one;
// model coordinates are relative to the level's grid corner.
GpuBuildStatus gpu_lod_capture(const GpuLod* l, uint32_t level, uint32_t min_count, GpuTree* out, int32_t box_lo[3], int32_t box_hi[3],
                               uint64_t* out_n_voxels, std::string* why);
// ---- neighbour-count rules (include/blok_hip.h: blok_hip_volume_automaton; automaton_kernels.hip) ----
// Steps a rule that has passed automaton::check over the box-local region [lo, hi).  Per step: the decision of every region brick from the
// brick masks (which every edit leaves equal to density > 0) into scratch owned by the call, the births, the deaths, then gpu_volume_commit
// over the region; the host reads the step's counts behind the decision and stops at a step that changes nothing.  out_step_counts: null,
// or 2 * rule.steps host values.  Blocking.  A failure before the first write leaves the volume as it was.
GpuBuildStatus gpu_volume_automaton(GpuVolume* v, const uint32_t lo[3], const uint32_t hi[3], const blok_automaton_rule& rule, uint64_t* out_step_counts,
                                    blok_automaton_info* out_info, std::string* why);
// = applyBrush (brush.cpp:13-63): mode 0 ADD (max), 1 SUBTRACT (min); the brush's bounding box must lie in the box.
GpuBuildStatus gpu_volume_brush(GpuVolume* v, const float center[3], float radius, float value, int mode, std::string* why);
// 64-tree of the current contents (UseHostBuilder = the volume is empty).  keyed volumes: out->d_nodes / d_materials stay OWNED BY THE
// VOLUME (out->owned_by_volume) and remain valid until the build after the next.
GpuBuildStatus gpu_volume_build(GpuVolume* v, GpuTree* out, std::string* why);

}  // namespace blok
#endif
