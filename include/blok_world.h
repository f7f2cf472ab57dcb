/*
 * blok_world.h — C ABI of the host-side voxel data model that feeds the trace path:
 * Morton codec, per-chunk sparse-voxel-octree build, sub-chunk packing, plus the
 * synthetic scene / camera helpers the benchmark uses.  Host code only (no GPU).
 *
 * Each entry names the reference interface it stands in for.  Byte layout of the
 * emitted records is the reference's (see blok_hip.h).  One documented deviation:
 * chunks are packed in sorted (cz,cy,cx) order; the reference iterates an
 * std::unordered_map (reference blok/src/chunk_manager.cpp:249), so its chunk order is
 * unspecified.  Node order inside a chunk is the reference's.
 */
#ifndef BLOK_WORLD_H
#define BLOK_WORLD_H

#include "blok_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* ----------------------------------------------------------------- morton */
/* = blok::morton3d::encode / decode / octantFromCode
 *   (reference blok/include/morton.hpp:23-33,46-53,55-58). */
uint64_t blok_morton_encode(int32_t x, int32_t y, int32_t z);
void     blok_morton_decode(uint64_t code, int32_t* x, int32_t* y, int32_t* z);
uint32_t blok_morton_octant(uint64_t code, uint32_t max_depth, uint32_t level);

/* ------------------------------------------------------------------ world */
typedef struct blok_world blok_world;

/* = ChunkManager::ChunkManager(C, voxelSize) (reference blok/src/chunk_manager.cpp:19-25).
 * chunk_size must be a power of two >= 8 (the reference app uses 128, app.cpp:37). */
int  blok_world_create(blok_world** out, uint32_t chunk_size, float voxel_size);
void blok_world_destroy(blok_world* w);
const char* blok_world_last_error(const blok_world* w);

/* = ChunkManager::setVoxelMaterial(worldPos, materialId, density)
 *   (reference blok/src/chunk_manager.cpp:316-328): floor -> chunk -> local, last write wins,
 *   marks the chunk dirty. */
int blok_world_set_voxel(blok_world* w, const float world_pos[3], uint32_t material_id, float density);
/* Bulk integer form of the same write (global voxel coordinates, density 1). */
int blok_world_set_voxels(blok_world* w, const int32_t* xyz, const uint32_t* material_ids, size_t n);
/* = ChunkManager::getVoxelMaterial (reference blok/src/chunk_manager.cpp:330-348). */
uint32_t blok_world_get_voxel_material(const blok_world* w, const float world_pos[3]);

/* = applyBrush(mgr, Brush{centerWS, radiusWS, value, mode}) (reference blok/src/brush.cpp:13-63,
 * blok/include/brush.hpp:14-21): sphere edit of the density field — mode 0 ADD: d = max(d, value),
 * mode 1 SUBTRACT: d = min(d, value); material ids are left as they are; every chunk the brush's bounding box
 * touches is created and every chunk with a voxel inside the sphere is marked dirty. */
int blok_world_apply_brush(blok_world* w, const float center[3], float radius, float value, int mode);

/* = rebuildDirtyChunks(mgr, maxPerFrame) (reference blok/src/chunk_manager.cpp:121-140):
 *   clear + re-insert every density>0 voxel in z,y,x order (x fastest, :106-119) through
 *   SvoTree::insertVoxel (reference blok/src/svo.cpp:59-101).  Returns chunks rebuilt (>=0). */
int blok_world_rebuild_dirty(blok_world* w, int max_per_frame);

/* = packChunksToGpuSvo (reference blok/src/chunk_manager.cpp:234-314). */
int blok_world_pack(blok_world* w);
size_t blok_world_node_count(const blok_world* w);
size_t blok_world_sub_chunk_count(const blok_world* w);
const blok_svo_node*  blok_world_nodes(const blok_world* w);
const blok_sub_chunk* blok_world_sub_chunks(const blok_world* w);

/* Per-chunk view (sorted order), for parity tests against the oracle's node arrays. */
size_t blok_world_chunk_count(const blok_world* w);
int    blok_world_chunk_info(const blok_world* w, size_t i, int32_t coord[3], uint64_t* n_nodes);
const blok_svo_node* blok_world_chunk_nodes(const blok_world* w, size_t i);
/* = SvoTree::findLeaf (reference blok/src/svo.cpp:103-130): node index in chunk i, or -1. */
int64_t blok_world_find_leaf(const blok_world* w, size_t i, uint32_t x, uint32_t y, uint32_t z);

/* -------------------------------------------------------------- materials */
/* = blok::Material (reference blok/include/material.hpp:27-44), C layout. */
typedef struct blok_material_desc {
    float   albedo[3];        /* default 1,1,1 */
    float   alpha;            /* 1 */
    float   metallic;         /* 0 */
    float   roughness;        /* 0.5 */
    float   ior;              /* 1.5 */
    float   specular;         /* 0.5 */
    float   emission[3];      /* 0 */
    float   emission_power;   /* 0 */
    uint8_t type;             /* MaterialType: 0 diffuse, 1 metallic, 2 glass, 3 emissive (material.hpp:18-24) */
    int16_t vox_palette_index;/* -1 */
    char    name[32];
} blok_material_desc;
void blok_material_desc_init(blok_material_desc* m);           /* the defaults above */
/* = MaterialGpu::pack (reference blok/include/material.hpp:96-112). */
void blok_material_pack(const blok_material_desc* m, blok_material* out);

/* = blok::MaterialLibrary (reference blok/include/material.hpp:116-163, blok/src/material.cpp):
 * id 0 is the default grey diffuse material; ids are indices into the packed GPU table. */
typedef struct blok_material_library blok_material_library;
int      blok_material_library_create(blok_material_library** out);
void     blok_material_library_destroy(blok_material_library* lib);
uint32_t blok_material_library_size(const blok_material_library* lib);
uint32_t blok_material_library_add(blok_material_library* lib, const blok_material_desc* m);          /* addMaterial */
uint32_t blok_material_library_add_or_find(blok_material_library* lib, const blok_material_desc* m);  /* addOrFindMaterial */
int      blok_material_library_get(const blok_material_library* lib, uint32_t id, blok_material_desc* out); /* getMaterial (id clamps to 0) */
uint32_t blok_material_library_id_by_name(const blok_material_library* lib, const char* name);        /* getMaterialIdByName */
uint32_t blok_material_library_from_color(blok_material_library* lib, uint8_t r, uint8_t g, uint8_t b); /* getOrCreateFromColor */
void     blok_material_library_set_vox_palette(blok_material_library* lib, uint8_t palette_index, uint32_t material_id);
uint32_t blok_material_library_from_vox_palette(const blok_material_library* lib, uint8_t palette_index);
int      blok_material_library_pack(const blok_material_library* lib, blok_material* out, size_t capacity); /* packForGpu */
void     blok_material_library_clear(blok_material_library* lib);
/* = ChunkManager::setMaterialLibrary (reference blok/include/chunk_manager.hpp:30): with a library
 * attached, colour writes go through getOrCreateFromColor, otherwise the id is r<<16|g<<8|b
 * (reference blok/src/chunk_manager.cpp:91-102). */
void blok_world_set_material_library(blok_world* w, blok_material_library* lib);
blok_material_library* blok_world_get_material_library(const blok_world* w);
int  blok_world_set_voxel_rgb(blok_world* w, const float world_pos[3], uint8_t r, uint8_t g, uint8_t b, float density);

/* ------------------------------------------------------------ .vox import */
/* MagicaVoxel .vox reader = loadVoxFile (reference blok/src/vox_loader.cpp:151-368): SIZE / XYZI / RGBA / MATL. */
typedef struct blok_vox blok_vox;
int  blok_vox_load_file(const char* path, blok_vox** out, char* err, size_t err_len);
int  blok_vox_load_memory(const void* data, size_t size, blok_vox** out, char* err, size_t err_len);
void blok_vox_free(blok_vox* v);
uint32_t blok_vox_model_count(const blok_vox* v);
int  blok_vox_model_info(const blok_vox* v, uint32_t model, uint32_t size_xyz[3], uint32_t* n_voxels);
/* voxels of a model as (x, y, z, colorIndex) bytes, file order */
const uint8_t* blok_vox_model_voxels(const blok_vox* v, uint32_t model);
const uint32_t* blok_vox_palette(const blok_vox* v);            /* 256 entries, ABGR */
/* = VoxFile::getMaterial (reference blok/src/vox_loader.cpp:116-149) */
int  blok_vox_get_material(const blok_vox* v, uint8_t palette_index, blok_material_desc* out);
/* = importVoxMaterials (reference blok/src/vox_loader.cpp:370-388) */
int  blok_vox_import_materials(const blok_vox* v, blok_material_library* lib, uint32_t palette_to_material[256]);
/* = importVoxToChunks (reference blok/src/vox_loader.cpp:390-430): VOX z is up -> world y. Returns voxels imported. */
uint32_t blok_vox_import_to_world(const blok_vox* v, blok_world* w, const float world_offset[3], uint32_t model_index);

/* -------------------------------------------------------------- Wavefront OBJ / MTL meshes (obj.cpp)
 * Triangles for blok_hip_volume_voxelize_mesh.  Geometry: `v x y z [w]` (w ignored); `f` with i, i/t, i//n or i/t/n and negative
 * (relative) indices, referring to vertices defined before the face; polygons are fan-triangulated from their first vertex.  vt, vn, o,
 * g, s, l, p and unknown statements are ignored; CRLF endings and a missing final newline are accepted.  Materials: the first `mtllib`,
 * resolved relative to the .obj's directory (load_memory: the given MTL text instead; NULL = none); `usemtl` selects the material of the
 * faces that follow.  From the MTL: newmtl -> name, Kd -> albedo, a non-zero Ke -> emission (type emissive, power 1), Pr -> roughness,
 * Pm -> metallic; each goes through blok_material_library_add_or_find.  Faces before any usemtl or naming an undefined material get id 0;
 * lib == NULL gives all zeros.  Errors (BLOK_ERR_INVALID_ARG, the line number in err): malformed numbers, index 0, out-of-range
 * indices, faces with fewer than three vertices, a missing MTL file. */
typedef struct blok_mesh blok_mesh;
int  blok_obj_load_file(const char* path, blok_material_library* lib, blok_mesh** out, char* err, size_t err_len);
int  blok_obj_load_memory(const char* obj, size_t obj_len, const char* mtl, size_t mtl_len, blok_material_library* lib, blok_mesh** out,
                          char* err, size_t err_len);
void blok_mesh_free(blok_mesh* m);
size_t blok_mesh_vertex_count(const blok_mesh* m);
size_t blok_mesh_triangle_count(const blok_mesh* m);
const float*    blok_mesh_positions(const blok_mesh* m);      /* xyz per vertex */
const uint32_t* blok_mesh_triangles(const blok_mesh* m);      /* three vertex indices per triangle */
const uint32_t* blok_mesh_materials(const blok_mesh* m);      /* one material id per triangle */
/* -------------------------------------------------------------- procedural terrain on the host (terrain.cpp)
 * The function of blok_hip_volume_generate_terrain (blok_hip.h has the contract), evaluated by the same code on the CPU.
 * default_params: a landscape for an n^3 box at the origin (surface between n/8 and n/2, caves, four materials 1..4): the values a user
 * starts from.  validate: BLOK_OK or BLOK_ERR_INVALID_ARG by the contract's limits.  height: H(x, z) for n (x, z) pairs, e.g. to put a
 * camera or a model on the ground.  eval: the region [lo, hi) of world voxels into the caller's arrays of exactly that region, x fastest
 * (flags honoured; for ADD the caller pre-fills them); out_n_voxels (may be NULL): filled voxels written. */
int blok_terrain_default_params(uint32_t n, uint32_t seed, blok_terrain_params* out);
int blok_terrain_validate(const blok_terrain_params* params);
int blok_terrain_height(const blok_terrain_params* params, const int32_t* xz, size_t n, int32_t* out);
int blok_terrain_eval(const blok_terrain_params* params, const int32_t region_lo[3], const int32_t region_hi[3], float* density,
                      uint32_t* material_ids, uint64_t* out_n_voxels);

/* -------------------------------------------------------------- a volume's surface as merged quads on the host (quads.cpp)
 * extract: the contract of blok_hip_volume_extract_quads (blok_hip.h) over host arrays density[x + y*nx + z*nx*ny] / material_ids of a
 * box whose voxel (0, 0, 0) sits at world `origin` (NULL = 0, 0, 0); the region in world voxels, half open, both NULL = the whole box.
 * Writes at most `capacity` records in canonical order (a prefix when there are more; none under BLOK_QUADS_COUNT_ONLY) and always
 * reports the totals (either pointer may be NULL).  Errors as the device entry: BLOK_ERR_INVALID_ARG for unknown flag bits, exactly one
 * region pointer NULL, lo > hi on an axis, a NULL array the call would use; BLOK_ERR_UNSUPPORTED for a region that leaves the box or a
 * box above 2^32 cells; an empty region is BLOK_OK with zero counts.
 * write_obj: n quads as a Wavefront OBJ: integer `v` lines, vertices shared between quads and numbered by first use (quads in the given
 * order, corners in winding order, each `v` line just before the first face that uses it), one four-index `f` line per quad, a
 * `usemtl m<id>` line before the first face and whenever the material changes.  With a library: a `mtllib` line and a sibling file (the
 * path with its extension replaced by .mtl) whose `newmtl m<id>` entries carry the material's albedo as `Kd`.  blok_obj_load_file reads
 * the result back: two triangles per quad, (c0, c1, c2) and (c0, c2, c3).  BLOK_ERR_INVALID_ARG (text in err): a file that cannot be
 * written, a record with face > 5 or a zero extent. */
int blok_quads_extract(const float* density, const uint32_t* material_ids, const int32_t origin[3], uint32_t nx, uint32_t ny, uint32_t nz,
                       const int32_t region_lo[3], const int32_t region_hi[3], uint32_t flags, blok_quad* out, uint64_t capacity,
                       uint64_t* out_n_quads, uint64_t* out_n_faces);
int blok_quads_write_obj(const char* path, const blok_quad* quads, uint64_t n, const blok_material_library* lib, char* err, size_t err_len);

/* -------------------------------------------------------------- emissive quads as a light table on the host (lights.cpp)
 * from_quads: the contract of blok_hip_lights_from_quads (blok_hip.h, "emissive voxels as lights") over host arrays, bit-identical to the
 * device's table: quad i is kept iff materials[index(quads[i].material)] is emissive, in the quads' order, cum the exclusive prefix sum
 * of du * dv.  Writes at most `capacity` records (a prefix when there are more; out may be NULL with capacity 0) and always fills
 * *out_info (may be NULL) with the totals.  BLOK_ERR_INVALID_ARG: a NULL array with a non-zero count, no material table;
 * BLOK_ERR_UNSUPPORTED: 2^31 or more lights, or 2^32 or more unit faces.
 * check: the rules blok_hip_set_lights holds a host table to.  BLOK_OK, or BLOK_ERR_INVALID_ARG / BLOK_ERR_UNSUPPORTED with "light I: rule"
 * in err (may be NULL).  *out_info (may be NULL) takes n, A and the bytes of a table that passes (area_world and n_owned are the
 * context's to fill: 0 here). */
int blok_lights_from_quads(const blok_quad* quads, uint64_t n_quads, const blok_material* materials, size_t n_materials, blok_light* out,
                           uint64_t capacity, float voxel_size, blok_lights_info* out_info);
int blok_lights_check(const blok_light* lights, uint64_t n, blok_lights_info* out_info, char* err, size_t err_len);
/* model_lights: the contract of blok_hip_model_lights (blok_hip.h, "emissive models as lights") for the model blok_hip_model_create makes
 * of the n voxels xyz[3*i..] / material_ids[i] (duplicates: the last one wins), bit-identical to the device's table: the model's tree is
 * built and walked.  Writes at most `capacity` records (out may be NULL with capacity 0); *out_n (may be NULL) takes the number of faces.
 * BLOK_ERR_INVALID_ARG: a NULL list, n == 0, no material table; BLOK_ERR_UNSUPPORTED: a list blok_hip_model_create refuses.
 * instance_light_record: the world-lattice rectangle of unit face *model_face of a model's table under *instance for a model of scale
 * exponent scale_log2 (0 .. 8; above: 8), by the rule of blok_hip.h; any NULL pointer: nothing is written. */
int blok_model_lights(const int32_t* xyz, const uint32_t* material_ids, size_t n, const blok_material* materials, size_t n_materials, blok_light* out,
                      uint64_t capacity, uint64_t* out_n);
void blok_instance_light_record(const blok_instance* instance, uint32_t scale_log2, const blok_light* model_face, blok_light* out);
/* light_grid_build (light_grid.cpp): the contract of blok_hip_build_light_grid (blok_hip.h, "the light grid") over a host table that passes
 * blok_lights_check, n >= 1; bit-identical to the device's three arrays.  *out_info (may be NULL) always takes the grid's figures.  With
 * all three arrays NULL that is all (the count call).  Otherwise all three are written: out_start n_cells + 1 words, out_faces n_cells
 * words, out_items n_items records, and cells_capacity >= n_cells, items_capacity >= n_items must hold.  BLOK_ERR_INVALID_ARG: a NULL or
 * empty table, a table the check refuses, a parameter out of range, some but not all arrays NULL, a capacity too small;
 * BLOK_ERR_UNSUPPORTED: n_cells > 2^24 or n_items >= 2^28 (nothing is allocated for such a grid). */
int blok_light_grid_build(const blok_light* lights, uint64_t n, uint32_t cell_log2, uint32_t reach, uint32_t share, uint32_t* out_start,
                          uint32_t* out_faces, blok_light_grid_item* out_items, uint64_t cells_capacity, uint64_t items_capacity,
                          blok_light_grid_info* out_info);

/* -------------------------------------------------------------- models into a volume and back on the host (stamp.cpp)
 * The contracts of blok_hip_volume_stamp_models and blok_hip_volume_capture_model (blok_hip.h) over host arrays density[x + y*nx + z*nx*ny]
 * / material_ids of a box whose voxel (0, 0, 0) sits at world `origin` (NULL = 0, 0, 0), through the arithmetic the kernel uses.
 * stamp_voxels: the model is the list of n voxels model_xyz[3*i..] (local lattice) with model_materials[i]; duplicates follow
 * blok_hip_model_create's rule, the last one wins.  One placement (its `model` field is not looked at), mode BLOK_STAMP_*, `value` the
 * density written by SET and KEEP.  out_n_voxels (may be NULL): voxels written.  BLOK_ERR_INVALID_ARG, nothing written: a NULL or
 * malformed placement, an unknown mode, for SET and KEEP a value that is not finite or <= 0, a NULL array the call would use;
 * BLOK_ERR_UNSUPPORTED: a box above 2^32 cells.
 * capture_voxels: the filled voxels (density > 0) of the region (world voxels, half open; both NULL = the whole box) as the list
 * {(w - region_lo, ids[w])}, x fastest, then y, then z: at most `capacity` records into xyz_out / materials_out (a prefix when there are
 * more; xyz_out NULL = count only), the total in *out_n.  Errors as blok_quads_extract. */
int blok_stamp_voxels(float* density, uint32_t* material_ids, const int32_t origin[3], uint32_t nx, uint32_t ny, uint32_t nz,
                      const int32_t* model_xyz, const uint32_t* model_materials, size_t n,
                      const blok_instance* placement, int mode, float value, uint64_t* out_n_voxels);
int blok_capture_voxels(const float* density, const uint32_t* material_ids, const int32_t origin[3], uint32_t nx, uint32_t ny, uint32_t nz,
                        const int32_t region_lo[3], const int32_t region_hi[3], int32_t* xyz_out, uint32_t* materials_out,
                        uint64_t capacity, uint64_t* out_n);

/* -------------------------------------------------------------- a model resampled into a volume through an affine map, on the host (affine.cpp)
 * blok_affine (blok_hip.h, blok_hip_volume_stamp_affine) maps the WORLD to the MODEL; these make one, and apply one to host arrays.
 * from_instance: the placement and a scale exponent e <= 8 folded into *out exactly: anchor = offset and, for local axis k along world axis
 *   a = axis[k], m[k][a] = +-2^(16 - e), t_k = +-2^(15 - e) (minus under flip bit k), all else zero, `model` the placement's.  With e = 0 the
 *   record writes what blok_hip_volume_stamp_models writes for the placement; with e > 0 the cells the tracer shows for a model of that
 *   exponent ("Scaled models", blok_hip.h).  BLOK_ERR_INVALID_ARG: a NULL pointer, a malformed placement, e > 8.
 * from_matrix: a convenience for a forward map, model -> world, 3 x 4 row major (world = F * model + T, both in voxels, a voxel v being the
 *   cube [v, v + 1)).  The map is inverted in double precision; anchor = floor(T), the cell that holds the image of the model-space origin;
 *   m = rint(F^-1 * 2^16), t = rint(F^-1 * (anchor + 1/2 - T) * 2^16); model = 0.  The signed permutations and the power-of-two scales
 *   with an integer T give from_instance's records exactly.  BLOK_ERR_INVALID_ARG: a NULL pointer, a value that is not finite, a singular
 *   matrix, |m| > 2^22, |t| > 2^40 or an anchor outside int32.
 * stamp_voxels: the contract of blok_hip_volume_stamp_affine for one record over host arrays density[x + y*nx + z*nx*ny] / material_ids of
 *   a box whose voxel (0, 0, 0) sits at world `origin` (NULL = 0, 0, 0), through the arithmetic the kernel uses.  The model is the list of n
 *   voxels model_xyz[3*i..] (local lattice) with model_materials[i]; the last duplicate wins.  The record's `model` field is not looked
 *   at.  The list is looked up through a dense array of its box, or a hash when the box is large: never a tree.  Errors as the device entry
 *   (a NULL record or a NULL array the call would use is BLOK_ERR_INVALID_ARG); nothing is written then. */
int blok_affine_from_instance(const blok_instance* placement, uint32_t scale_log2, blok_affine* out);
int blok_affine_from_matrix(const double forward[12], blok_affine* out);
int blok_affine_stamp_voxels(float* density, uint32_t* material_ids, const int32_t origin[3], uint32_t nx, uint32_t ny, uint32_t nz,
                             const int32_t* model_xyz, const uint32_t* model_materials, size_t n, const blok_affine* record,
                             const int32_t region_lo[3], const int32_t region_hi[3], int mode, float value, uint64_t* out_n_voxels);

/* -------------------------------------------------------------- posed models: making a blok_pose, and baking one (pose.cpp)
 * blok_pose (blok_hip.h, "Posed models") maps the WORLD to a model's LOCAL space; lengths are world units.  vs: the world's voxel size.
 * pose_from_instance: the placement as a pose: m the signed permutation (m[k][axis[k]] = -1 under flip bit k, else +1), pivot =
 *   fl(offset * vs), local = 0.  Its local ray is the lattice instance's, value for value (a zero may differ in sign), so its t, material
 *   and hit are the instance's.
 * pose_from_matrix: a forward map local -> world, row major 3 x 4 (world = F local + T, world units), inverted in double (adjugate over
 *   determinant) and rounded once to float.  pivot_local (NULL = the local origin): the local point about which the pose is most accurate;
 *   pivot = fl(F pivot_local + T), local = fl(pivot_local + F^-1 (pivot - (F pivot_local + T))).
 *   BLOK_ERR_INVALID_ARG: a NULL pointer, a value that is not finite, a singular matrix, a result beyond the limits of a pose.
 * affine_from_pose: the pose folded into blok_hip_volume_stamp_affine's record for a model of scale exponent e <= 8, so that a posed
 *   model that stops can be baked about where it was seen: anchor = floor(pivot / vs), m = rint(m * 2^16 / 2^e),
 *   t = rint((m ((anchor + 1/2) vs - pivot) + local) / (vs 2^e) * 2^16), in double.  For the poses of pose_from_instance it gives
 *   blok_affine_from_instance's record bit for bit; only that is pinned.  BLOK_ERR_INVALID_ARG: a NULL pointer, vs not a positive finite
 *   number, e > 8, a value that is not finite, a result beyond the record's limits (|m| > 2^22, |t| > 2^40, an anchor outside int32). */
int blok_pose_from_instance(const blok_instance* placement, float vs, blok_pose* out);
int blok_pose_from_matrix(const double forward[12], const double pivot_local[3], uint32_t model, blok_pose* out);
int blok_affine_from_pose(const blok_pose* pose, float vs, uint32_t scale_log2, blok_affine* out);
/* pose_motion_record: the motion record of pose `cur` that was `prev` one frame earlier (blok_hip.h, "Object motion for posed models"), bit for
 *   bit what the device builds.  prev == NULL: the pose's index lies beyond the previous table (untracked).  model_usable: non-zero iff the
 *   model `cur` names exists and passes the pose limits of the store (what blok_hip_check_poses checks besides the floats); the floats of both
 *   records are checked here.  Every byte of *out is written.  BLOK_ERR_INVALID_ARG: cur or out NULL. */
int blok_pose_motion_record(const blok_pose* cur, const blok_pose* prev, int model_usable, blok_pose_motion* out);

/* -------------------------------------------------------------- a volume's connected components on the host (components.cpp)
 * label: the contract of blok_hip_volume_label_components (blok_hip.h; blok_component is declared there) over the host array
 * density[x + y*nx + z*nx*ny] of a box whose voxel (0, 0, 0) sits at world `origin` (NULL = 0, 0, 0), through the union-find the kernels
 * use, run serially; the region in world voxels, half open, both NULL = the whole box; flags must be 0.  Writes at most `label_capacity`
 * cells of the label array into labels_out and at most `component_capacity` records into components_out (prefixes when there are more;
 * either pointer NULL = that output is not written) and always reports the totals (either pointer may be NULL).  Errors as the device
 * entry: BLOK_ERR_INVALID_ARG for unknown flag bits, exactly one region pointer NULL, lo > hi on an axis, a NULL density the call would
 * read; BLOK_ERR_UNSUPPORTED for a region that leaves the box or a box above 2^32 cells; an empty region is BLOK_OK with zero counts. */
int blok_components_label(const float* density, const int32_t origin[3], uint32_t nx, uint32_t ny, uint32_t nz,
                          const int32_t region_lo[3], const int32_t region_hi[3], uint32_t flags,
                          uint32_t* labels_out, uint64_t label_capacity, blok_component* components_out, uint64_t component_capacity,
                          uint64_t* out_n_components, uint64_t* out_n_voxels);

/* -------------------------------------------------------------- a placed model swept against a volume on the host (sweep.cpp)
 * The contract of blok_hip_volume_sweep_models (blok_hip.h; blok_sweep_result and BLOK_SWEEP_BOX_IS_SOLID are declared there) over the
 * host array density[x + y*nx + z*nx*ny] of a box whose voxel (0, 0, 0) sits at world `origin` (NULL = 0, 0, 0), through the arithmetic the
 * kernel uses, voxel by voxel.  The model is the list of n distinct voxels model_xyz[3*i..] (local lattice; a voxel listed twice is
 * counted twice in n_overlap).  One placement (its `model` field is not looked at), direction 0..5 in blok_hit::face numbering.  An empty
 * list gives {0, max_distance, 0}.  BLOK_ERR_INVALID_ARG, nothing written: a NULL or malformed placement, direction > 5, unknown flag
 * bits, a NULL result, a NULL array the call would read; BLOK_ERR_UNSUPPORTED: a box above 2^32 cells. */
int blok_sweep_voxels(const float* density, const int32_t origin[3], uint32_t nx, uint32_t ny, uint32_t nz, const int32_t* model_xyz, size_t n,
                      const blok_instance* placement, uint32_t direction, uint32_t max_distance, uint32_t flags, blok_sweep_result* out_result);

/* -------------------------------------------------------------- the sparse brick stream on the host (bricks.cpp)
 * The contracts of blok_hip_volume_encode_bricks and blok_hip_volume_decode_bricks (blok_hip.h; blok_brick_record, blok_bricks_info and the
 * flags are declared there) over host arrays density[x + y*nx + z*nx*ny] / material_ids of a box whose voxel (0, 0, 0) sits at world
 * `origin` (NULL = 0, 0, 0), through the rules the kernels use, brick by brick.
 * encode is called twice: with records NULL it fills *out_info alone (the counts), then with arrays of at least those sizes (a payload
 * array may be NULL when its count is 0).  The region is in world voxels, half open, both NULL = the whole box.  Errors as the device
 * entry; an array too small for the stream is BLOK_ERR_INVALID_ARG.
 * validate: the validation of a host stream; BLOK_ERR_INVALID_ARG with the rule and the first failing record in err.
 * decode: validates, then writes the stream into [dst_lo, dst_lo + ext) (NULL = info->lo), flags BLOK_BRICKS_KEEP_OTHERS or 0.  Nothing is
 * written on an error (codes as the device entry).
 * A .bvol file is, in order and little-endian: the 8 bytes "BLOKBVL1", the info, the records, the density payload, the material payload.
 * write_file validates first.  read_file checks every size against the file's length and fills *out_info; with all three arrays NULL
 * it stops there (the caller then knows what to allocate), otherwise it reads the arrays and validates them. */
int blok_bricks_encode(const float* density, const uint32_t* material_ids, const int32_t origin[3], uint32_t nx, uint32_t ny, uint32_t nz,
                       const int32_t region_lo[3], const int32_t region_hi[3], uint32_t flags, blok_bricks_info* out_info,
                       blok_brick_record* records, uint64_t record_capacity, uint32_t* density_payload, uint64_t density_capacity,
                       uint32_t* material_payload, uint64_t material_capacity);
int blok_bricks_validate(const blok_bricks_info* info, const blok_brick_record* records, const uint32_t* density_payload,
                         const uint32_t* material_payload, char* err, size_t err_len);
int blok_bricks_decode(float* density, uint32_t* material_ids, const int32_t origin[3], uint32_t nx, uint32_t ny, uint32_t nz,
                       const blok_bricks_info* info, const blok_brick_record* records, const uint32_t* density_payload,
                       const uint32_t* material_payload, const int32_t dst_lo[3], uint32_t flags, char* err, size_t err_len);
int blok_bricks_write_file(const char* path, const blok_bricks_info* info, const blok_brick_record* records, const uint32_t* density_payload,
                           const uint32_t* material_payload, char* err, size_t err_len);
int blok_bricks_read_file(const char* path, blok_bricks_info* out_info, blok_brick_record* records, uint32_t* density_payload,
                          uint32_t* material_payload, char* err, size_t err_len);

/* -------------------------------------------------------------- the distance field on the host (distance.cpp)
 * The contracts of blok_hip_volume_distance_field and blok_hip_volume_edit_by_distance (blok_hip.h; blok_distance_info, the flags and the
 * ops are declared there) over host arrays density[x + y*nx + z*nx*ny] / material_ids of a box whose voxel (0, 0, 0) sits at world
 * `origin` (NULL = 0, 0, 0), through the rules the kernels use, separable as the device's.
 * field: the region is in world voxels, half open, both NULL = the whole box; out_field takes one value per region cell, x fastest, and
 * *out_info (may be NULL) what the device's info holds.  Errors as the device entry; a NULL array with a non-empty region is
 * BLOK_ERR_INVALID_ARG.
 * edit: applies `op` at the threshold d2 to the two arrays from a field and its info, judged against the arrays as they are; *out_n_voxels
 * (may be NULL) is the number of cells written.  Errors as the device entry; an info whose version is not 1 is BLOK_ERR_INVALID_ARG, one
 * whose region leaves the box BLOK_ERR_UNSUPPORTED.  Nothing is written on an error. */
int blok_distance_field(const float* density, const int32_t origin[3], uint32_t nx, uint32_t ny, uint32_t nz, const int32_t region_lo[3],
                        const int32_t region_hi[3], uint32_t max_radius, uint32_t flags, uint16_t* out_field, blok_distance_info* out_info);
int blok_distance_edit(float* density, uint32_t* material_ids, const int32_t origin[3], uint32_t nx, uint32_t ny, uint32_t nz, const uint16_t* field,
                       const blok_distance_info* info, int op, uint32_t d2, float density_value, uint32_t material, uint64_t* out_n_voxels);

/* -------------------------------------------------------------- the flood from seeds on the host (flood.cpp)
 * The contracts of blok_hip_volume_flood_field and blok_hip_volume_edit_by_flood (blok_hip.h; blok_flood_info, the flags and the ops are
 * declared there) over host arrays of a box as above, through the rules the kernels use.  The field is a plain queue BFS: the definition.
 * field: the region and the seeds are in world voxels; material_ids may be NULL without BLOK_FLOOD_SAME_MATERIAL; out_field takes one value
 * per region cell, x fastest, and *out_info (may be NULL) what the device's info holds.  Errors as the device entry; a NULL array with a
 * non-empty region is BLOK_ERR_INVALID_ARG.
 * edit: applies `op` at the threshold d to the two arrays from a field and its info, judged against the arrays as they are; *out_n_voxels
 * (may be NULL) is the number of cells written.  Errors as the device entry; an info whose version is not 1 is BLOK_ERR_INVALID_ARG, one
 * whose region leaves the box BLOK_ERR_UNSUPPORTED.  Nothing is written on an error. */
int blok_flood_field(const float* density, const uint32_t* material_ids, const int32_t origin[3], uint32_t nx, uint32_t ny, uint32_t nz,
                     const int32_t region_lo[3], const int32_t region_hi[3], const int32_t* seeds_xyz, uint64_t n_seeds, uint32_t max_steps,
                     uint32_t flags, uint32_t material, uint16_t* out_field, blok_flood_info* out_info);
int blok_flood_edit(float* density, uint32_t* material_ids, const int32_t origin[3], uint32_t nx, uint32_t ny, uint32_t nz, const uint16_t* field,
                    const blok_flood_info* info, int op, uint32_t d, float density_value, uint32_t material, uint64_t* out_n_voxels);

/* -------------------------------------------------------------- the column field and scatter on the host (columns.cpp)
 * The contracts of blok_hip_volume_column_field and blok_hip_volume_scatter_models (blok_hip.h; the records and the flags are declared
 * there) over host arrays of a box as above, through the rules the kernels use.
 * column_field: the region is in world voxels; out_top and out_material take one value per column (index cp + ext[p] * cq) and *out_info
 * (may be NULL) what the device's info holds.  Errors as the device entry; a NULL array with a non-empty region is BLOK_ERR_INVALID_ARG.
 * scatter: top, material and columns_info are a column field's (axis 1, not FROM_LOW).  With out_instances NULL it only counts; otherwise
 * the table takes n_placed records in column order, and a capacity below n_placed is BLOK_ERR_INVALID_ARG with nothing written.  *out_info
 * (may be NULL) is what the device's info holds.  Errors as the device entry. */
int blok_column_field(const float* density, const uint32_t* material_ids, const int32_t origin[3], uint32_t nx, uint32_t ny, uint32_t nz,
                      const int32_t region_lo[3], const int32_t region_hi[3], uint32_t axis, uint32_t flags, uint16_t* out_top,
                      uint32_t* out_material, blok_columns_info* out_info);
int blok_scatter(const uint16_t* top, const uint32_t* material, const blok_columns_info* columns_info, const blok_scatter_params* params,
                 const blok_scatter_entry* entries, uint32_t n_entries, blok_instance* out_instances, uint64_t capacity, blok_scatter_info* out_info);

/* -------------------------------------------------------------- the scroll of the resident volume on the host (scroll.cpp)
 * The contract of blok_hip_volume_scroll (blok_hip.h; the records and the flag are declared there) over host arrays of a box as above,
 * through the rules the kernels use.
 * scroll_plan: *out_info takes the plan of moving the box [origin, origin + dims) by delta: the new origin, the exposed and the leaving
 * boxes, n_cells_kept; the two filled counts stay 0.
 * scroll_voxels: the out-of-place move.  out_density and out_ids take nx * ny * nz values each, the new box's arrays; *out_info (may be
 * NULL) takes everything the device's info holds.  The inputs are not written and may not overlap the outputs.
 * Errors as the device entry (NULL delta, a component that is not a multiple of 4: BLOK_ERR_INVALID_ARG; a new box that leaves the int16
 * lattice: BLOK_ERR_UNSUPPORTED); a NULL origin is (0, 0, 0); a zero dimension, a NULL out_info (plan) or a NULL array (voxels) is
 * BLOK_ERR_INVALID_ARG.  Nothing is written on an error. */
int blok_scroll_plan(const int32_t origin[3], uint32_t nx, uint32_t ny, uint32_t nz, const int32_t delta[3], blok_scroll_info* out_info);
int blok_scroll_voxels(const float* density, const uint32_t* material_ids, const int32_t origin[3], uint32_t nx, uint32_t ny, uint32_t nz,
                       const int32_t delta[3], float* out_density, uint32_t* out_material_ids, blok_scroll_info* out_info);

/* -------------------------------------------------------------- the shape table on the host (shapes.cpp)
 * The contract of blok_hip_volume_apply_shapes (blok_hip.h; the record and its constants are declared there) over host arrays of a box as
 * above, through the rules the kernels use.
 * shapes_check: BLOK_OK, or BLOK_ERR_INVALID_ARG with the first offending index in *out_index and "shape I: rule" in err (each may be NULL).
 * shape_bounds: the voxel box of one shape that passes the check, world voxels, half open (empty where no voxel centre fits).
 * shapes_voxels: the table applied shape by shape, in order, in place; *out_n_written (may be NULL) as the device entry counts.  A NULL
 * origin is (0, 0, 0); the box may lie anywhere in int32.  A NULL array or a zero dimension is BLOK_ERR_INVALID_ARG, a box above 2^32
 * cells BLOK_ERR_UNSUPPORTED.  Nothing is written on an error. */
int blok_shapes_check(const blok_shape* shapes, uint32_t n_shapes, uint32_t* out_index, char* err, size_t err_len);
int blok_shape_bounds(const blok_shape* shape, int32_t out_lo[3], int32_t out_hi[3]);
int blok_shapes_voxels(float* density, uint32_t* material_ids, const int32_t origin[3], uint32_t nx, uint32_t ny, uint32_t nz,
                       const blok_shape* shapes, uint32_t n_shapes, uint64_t* out_n_written);

/* -------------------------------------------------------------- the pyramid of coarser levels on the host (lod.cpp)
 * The contract of blok_hip_volume_reduce (blok_hip.h; the records and the flag are declared there) over host arrays of a box as above,
 * through the rules the kernels use.  The planes lie in one array, level behind level from level 1, and within a level of n_cells cells the
 * n plane (uint16_t) at byte 0, the e plane (uint16_t) at byte 2 n_cells and the id plane (uint32_t) at byte 4 n_cells: 8 n_cells bytes a
 * level.  With out_planes NULL nothing is reduced: *out_info takes the grids of the levels with zero counts, which say what the array must
 * hold.  Otherwise capacity_bytes below that sum, or a NULL array with a non-empty region, is BLOK_ERR_INVALID_ARG, and *out_info (may be
 * NULL) takes what the device's info holds.  Errors as the device entry. */
int blok_lod_reduce(const float* density, const uint32_t* material_ids, const int32_t origin[3], uint32_t nx, uint32_t ny, uint32_t nz,
                    const int32_t region_lo[3], const int32_t region_hi[3], uint32_t levels, uint32_t flags, void* out_planes,
                    uint64_t capacity_bytes, blok_lod_info* out_info);
/* The contract of blok_hip_terrain_reduce (blok_hip.h) on the host: the terrain function over the world region, reduced tile by tile
 * through the column words the kernel uses; no voxel array is made.  The planes, out_planes and capacity_bytes as blok_lod_reduce.
 * Errors as the device entry. */
int blok_terrain_reduce(const blok_terrain_params* params, const int32_t region_lo[3], const int32_t region_hi[3], uint32_t levels,
                        uint32_t flags, void* out_planes, uint64_t capacity_bytes, blok_lod_info* out_info);

/* -------------------------------------------------------------- neighbour-count rules on the host (automaton.cpp)
 * The contract of blok_hip_volume_automaton (blok_hip.h; the records and the flags are declared there) over host arrays of a box as above,
 * in place: a plain double-buffered loop per cell, through the check, the offsets and the vote the kernels use.
 * automaton_check: BLOK_OK, or BLOK_ERR_INVALID_ARG with the rule that failed in err (may be NULL).
 * automaton_voxels: out_step_counts (may be NULL) takes 2 * rule->steps values, *out_info (may be NULL) what the device's info holds.
 * Errors as the device entry; a NULL array with a non-empty region is BLOK_ERR_INVALID_ARG.  Nothing is written on an error. */
int blok_automaton_check(const blok_automaton_rule* rule, char* err, size_t err_len);
int blok_automaton_voxels(float* density, uint32_t* material_ids, const int32_t origin[3], uint32_t nx, uint32_t ny, uint32_t nz,
                          const int32_t region_lo[3], const int32_t region_hi[3], const blok_automaton_rule* rule, uint64_t* out_step_counts,
                          blok_automaton_info* out_info);

/* = loadAndImportVox (reference blok/src/vox_loader.cpp:432-462); lib may be NULL. */
int  blok_load_and_import_vox(const char* path, blok_world* w, blok_material_library* lib,
                              const float world_offset[3], uint32_t model_index, char* err, size_t err_len);

/* ----------------------------------------------------------------- camera */
/* = blok::Camera::forward/right/up + toDevice(Camera,w,h)
 *   (reference blok/include/camera.hpp:25-42, blok/src/cuda_tracer.cu:404-415). */
int blok_camera_from_yaw_pitch(const float pos[3], float yaw_deg, float pitch_deg, float fov_deg,
                               uint32_t width, uint32_t height, blok_camera* out);
/* Look-at convenience: derives yaw/pitch, then as above. */
int blok_camera_look_at(const float pos[3], const float target[3], float fov_deg,
                        uint32_t width, uint32_t height, blok_camera* out);

/* The matrices the reference's Vulkan path hands its shaders (FrameUBO, blok/include/resources.hpp:103-150), from the same
 * basis record: view = glm::lookAt(pos, pos + forward, up) (blok/include/camera.hpp:49-52), proj = glm::perspective(fov,
 * aspect, near, far) with depth 0..1 and p[1][1] *= -1 (camera.hpp:9,54-59), inverse = glm::inverse (FrameUBO::invView /
 * invProj, blok/src/renderer_denoising.cpp:669-670).  glm itself is absent from the reference tree (empty submodule): these
 * follow its published formulas; all 4x4 are column-major floats (M[col * 4 + row]).
 * With them a pixel's ray is  normalize(invView * (normalize((invProj * (ndc, 1, 1)).xyz), 0))  (raygen.rgen:201-205) — the
 * same ray as the basis form the kernels use, and with blok_jittered_projection the same ray as the basis form with the
 * jitter as a sub-pixel offset (tests/test_host_model.py). */
void blok_camera_view(const blok_camera* cam, float out_view[16]);
void blok_camera_projection(const blok_camera* cam, float z_near, float z_far, float out_proj[16]);
int  blok_mat4_inverse(const float m[16], float out[16]);
/* TAA jitter of frame `frame_index` in pixels: entry frame_index mod 16 of the Halton(2,3) - 0.5 sequence
 * (PostProcess::initJitterSequence / halton / advanceJitter, blok/src/renderer_postprocess.cpp:208-228,243,660-663);
 * frame 0 = (0, -1/6).  blok_taa_jitter_clip = getJitterClipSpace (:234-241); blok_jittered_projection = getJitteredProjection
 * (:254-268): proj[2][0] += 2 jx / width, proj[2][1] += 2 jy / height. */
void blok_taa_jitter(uint32_t frame_index, float out_px[2]);
void blok_taa_jitter_clip(const float jitter_px[2], uint32_t width, uint32_t height, float out_clip[2]);
void blok_jittered_projection(const float proj[16], const float jitter_px[2], uint32_t width, uint32_t height, float out[16]);

/* ------------------------------------------------- synthetic benchmark scene */
/* Integer-only generator G(N, seed) of SURVEY.md §8(d): terrain shell + 64 shell spheres,
 * materialId in [1,255].  Writes into `w` (chunk size as created), then the caller
 * rebuilds and packs.  Not reference behaviour — benchmark input synthesis. */
int blok_scene_generate(blok_world* w, uint32_t n, uint32_t seed, uint64_t* out_n_voxels);
/* Same voxel set as a dense id grid ids[x + y*n + z*n*n] (0 = empty); n <= 1024 (4 GiB of ids). */
int blok_scene_generate_dense(uint32_t n, uint32_t seed, uint32_t* ids, uint64_t* out_n_voxels);
/* 256 hashed diffuse materials (roughness 0.5, metallic 0: reference material.cpp:102-106). */
int blok_scene_materials(uint32_t seed, blok_material* out256);
/* Poses A(0) outside-corner, B(1) inside-grazing, C(2) top-down of SURVEY.md §8(d). */
int blok_scene_camera(uint32_t n, uint32_t seed, int pose, uint32_t width, uint32_t height, blok_camera* out);

#ifdef __cplusplus
}
#endif
#endif /* BLOK_WORLD_H */
