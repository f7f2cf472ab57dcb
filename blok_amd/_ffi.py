"""ctypes bindings for the two product libraries.

* ``libblok_host.so`` — host data model (include/blok_world.h), g++ only.
* ``libblok_hip.so``  — gfx950 trace backend (include/blok_hip.h), hipcc.

The bindings are the same stub a maintainer would write for any C consumer; see INTEGRATION.md
for the C++ one.  There is no fallback: a missing library raises ``BlokLibraryError``.
"""
from __future__ import annotations

import ctypes as C
import os
from pathlib import Path

import numpy as np

PKG_DIR = Path(__file__).resolve().parent
HOST_LIB = PKG_DIR / "libblok_host.so"
HIP_LIB = Path(os.environ.get("BLOK_HIP_LIB", PKG_DIR / "libblok_hip.so"))   # override: A/B builds of the kernels


class BlokLibraryError(RuntimeError):
    pass


class BlokError(RuntimeError):
    def __init__(self, status: int, message: str):
        super().__init__(f"blok status {status}: {message}")
        self.status = status


# ---------------------------------------------------------------- records (include/blok_hip.h)
SVO_NODE = np.dtype([("child_mask", "<u4"), ("first_child", "<u4"), ("material_id", "<u4"),
                     ("occupancy", "<f4")])
SUB_CHUNK = np.dtype([("node_offset", "<u4"), ("root_node_index", "<u4"), ("node_count", "<u4"),
                      ("start_depth", "<u4"), ("world_min", "<f4", 3), ("sub_chunk_size", "<f4"),
                      ("world_max", "<f4", 3), ("pad0", "<f4")])
MATERIAL = np.dtype([("albedo", "<f4", 3), ("flags", "<u4"), ("emission", "<f4", 3), ("ior", "<f4")])
CAMERA = np.dtype([("pos", "<f4", 3), ("fwd", "<f4", 3), ("right", "<f4", 3), ("up", "<f4", 3),
                   ("tan_half_fov", "<f4"), ("aspect", "<f4")])
HIT = np.dtype([("t", "<f4"), ("material_id", "<u4"), ("voxel", "<i2", 3), ("face", "u1"), ("hit", "u1")])
RAY = np.dtype([("org", "<f4", 3), ("tmin", "<f4"), ("dir", "<f4", 3), ("tmax", "<f4")])
# = blok_instance: a placed model (lattice offset, axis-aligned orientation), 32 bytes
INSTANCE = np.dtype([("model", "<u4"), ("offset", "<i4", 3), ("axis", "u1", 3), ("flip", "u1"), ("reserved", "<u4", 3)])
INSTANCE_NONE = 0xFFFFFFFF
# blok_pose (blok_hip.h, "Posed models"): a model under any affine map, world -> local; ids of pixels a pose wins carry POSE_ID
POSE = np.dtype([("model", "<u4"), ("m", "<f4", (3, 3)), ("pivot", "<f4", 3), ("local", "<f4", 3)])
POSE_ID = 0x80000000
# blok_pose_motion (blok_hip.h, "Object motion for posed models"): prev o cur^-1 of one pose about its pivots; state 0 untracked, 1 identity, 2 moving
POSE_MOTION = np.dtype([("state", "<u4"), ("a", "<f4", (3, 3)), ("c", "<f4", 3), ("n", "<f4", (3, 3)), ("pivot_cur", "<f4", 3), ("pivot_prev", "<f4", 3),
                        ("reserved", "<u4", 4)])
assert POSE_MOTION.itemsize == 128
# = blok_quad: one merged quad of a volume's surface, 32 bytes
QUAD = np.dtype([("lo", "<i4", 3), ("du", "<u4"), ("dv", "<u4"), ("material", "<u4"), ("face", "<u4"), ("reserved", "<u4")])
QUADS_IGNORE_MATERIAL, QUADS_COUNT_ONLY = 1, 2
# = blok_light (32 bytes): a quad whose reserved word is the running sum of du * dv; = blok_lights_info (32 bytes): what a light table holds
LIGHT = np.dtype([("lo", "<i4", 3), ("du", "<u4"), ("dv", "<u4"), ("material", "<u4"), ("face", "<u4"), ("cum", "<u4")])
LIGHTS_INFO = np.dtype([("n_faces", "<u8"), ("bytes", "<u8"), ("n", "<u4"), ("n_owned", "<u4"), ("area_world", "<f4"), ("reserved", "<u4")])
assert LIGHT.itemsize == 32 and LIGHTS_INFO.itemsize == 32
# = blok_instance_lights_info (32 bytes): the header of an instance table's light prefix
INSTANCE_LIGHTS_INFO = np.dtype([("a_inst", "<u8"), ("a_total", "<u8"), ("area_world", "<f4"), ("n_lit", "<u4"), ("disabled", "<u4"), ("reserved", "<u4")])
assert INSTANCE_LIGHTS_INFO.itemsize == 32
# = blok_light_grid_item (8 bytes): a list entry of the light grid; = blok_light_grid_info (72 bytes): what a grid holds
LIGHT_GRID_ITEM = np.dtype([("light", "<u4"), ("lcum", "<u4")])
LIGHT_GRID_INFO = np.dtype([("cell_lo", "<i4", 3), ("dim", "<u4", 3), ("cell_log2", "<u4"), ("reach", "<u4"), ("share", "<u4"), ("n_nonempty", "<u4"),
                            ("n_cells", "<u8"), ("n_items", "<u8"), ("bytes", "<u8"), ("max_items", "<u4"), ("reserved", "<u4")])
assert LIGHT_GRID_ITEM.itemsize == 8 and LIGHT_GRID_INFO.itemsize == 72
LIGHT_GRID_START, LIGHT_GRID_FACES, LIGHT_GRID_ITEMS = 0, 1, 2      # blok_hip_light_grid_download's `what`
STAMP_SET, STAMP_KEEP, STAMP_ERASE = 0, 1, 2      # = BLOK_STAMP_*
CAPTURE_CUT = 1                                   # = BLOK_CAPTURE_CUT
# = blok_component: one connected component of a labelled region, 40 bytes
COMPONENT = np.dtype([("label", "<u4"), ("touches", "<u4"), ("n_voxels", "<u8"), ("lo", "<i4", 3), ("hi", "<i4", 3)])
LABEL_EMPTY = 0xFFFFFFFF                          # = BLOK_LABEL_EMPTY
COMPONENT_CUT = 1                                 # = BLOK_COMPONENT_CUT
# = blok_sweep_result: one placement swept against the volume, 16 bytes
SWEEP_RESULT = np.dtype([("n_overlap", "<u8"), ("travel", "<u4"), ("blocked", "<u4")])
SWEEP_BOX_IS_SOLID = 1                            # = BLOK_SWEEP_BOX_IS_SOLID
# = blok_brick_record: one stored brick of a sparse brick stream, 24 bytes; = blok_bricks_info: what a stream holds, 64 bytes
BRICK_RECORD = np.dtype([("mask", "<u8"), ("brick", "<u4"), ("kind", "<u4"), ("density", "<u4"), ("material", "<u4")])
BRICKS_INFO = np.dtype([("version", "<u4"), ("flags", "<u4"), ("lo", "<i4", 3), ("ext", "<u4", 3), ("n_bricks", "<u8"), ("n_density", "<u8"),
                        ("n_material", "<u8"), ("n_voxels", "<u8")])
BRICKS_FILLED_ONLY = 1                            # = BLOK_BRICKS_FILLED_ONLY (encode)
BRICKS_KEEP_OTHERS = 1                            # = BLOK_BRICKS_KEEP_OTHERS (restore / decode)
# = blok_distance_info: what a distance field snapshot holds, 64 bytes
DISTANCE_INFO = np.dtype([("version", "<u4"), ("flags", "<u4"), ("lo", "<i4", 3), ("ext", "<u4", 3), ("max_radius", "<u4"), ("reserved", "<u4"),
                          ("n_zero", "<u8"), ("n_near", "<u8"), ("n_far", "<u8")])
DISTANCE_TO_EMPTY, DISTANCE_BOX_IS_SOLID = 1, 2   # = BLOK_DISTANCE_TO_EMPTY, BLOK_DISTANCE_BOX_IS_SOLID
DISTANCE_FAR = 0xFFFF                             # = BLOK_DISTANCE_FAR
DISTANCE_GROW, DISTANCE_SHRINK, DISTANCE_HOLLOW = 0, 1, 2      # = BLOK_DISTANCE_GROW / _SHRINK / _HOLLOW
# = blok_flood_info: what a flood snapshot holds, 64 bytes
FLOOD_INFO = np.dtype([("version", "<u4"), ("flags", "<u4"), ("lo", "<i4", 3), ("ext", "<u4", 3), ("max_steps", "<u4"), ("farthest", "<u4"),
                       ("n_seed", "<u8"), ("n_reached", "<u8"), ("n_unreached", "<u8")])
FLOOD_THROUGH_FILLED, FLOOD_SAME_MATERIAL = 1, 2  # = BLOK_FLOOD_THROUGH_FILLED, BLOK_FLOOD_SAME_MATERIAL
FLOOD_FAR = 0xFFFF                                # = BLOK_FLOOD_FAR
FLOOD_MAX_STEPS = 65534                           # = BLOK_FLOOD_MAX_STEPS
FLOOD_FILL, FLOOD_FILL_UNREACHED, FLOOD_PAINT, FLOOD_CLEAR = 0, 1, 2, 3      # = BLOK_FLOOD_FILL / _FILL_UNREACHED / _PAINT / _CLEAR
# = blok_sun_map_info: frame and bookkeeping of the shadow rays' last-occluder map, 84 bytes
SUN_MAP_INFO = np.dtype([("u", "<f4", 3), ("v", "<f4", 3), ("s", "<f4", 3), ("u0", "<f4"), ("v0", "<f4"), ("texel", "<f4"), ("nu", "<u4"), ("nv", "<u4"),
                         ("has_map", "<u4"), ("loose_edits", "<u4"), ("tighten_pending", "<u4"), ("pending_u0", "<u4"), ("pending_u1", "<u4"),
                         ("pending_v0", "<u4"), ("pending_v1", "<u4")])
# = blok_columns_info: what a column field snapshot holds, 64 bytes
COLUMNS_INFO = np.dtype([("version", "<u4"), ("flags", "<u4"), ("lo", "<i4", 3), ("ext", "<u4", 3), ("axis", "<u4"), ("min_top", "<u4"), ("max_top", "<u4"),
                         ("reserved", "<u4"), ("n_columns", "<u8"), ("n_hit", "<u8")])
COLUMNS_FROM_LOW = 1                              # = BLOK_COLUMNS_FROM_LOW
COLUMNS_NONE = 0xFFFF                             # = BLOK_COLUMNS_NONE
# = blok_scatter_entry (24 bytes), blok_scatter_params (64 bytes), blok_scatter_info (72 bytes)
SCATTER_ENTRY = np.dtype([("model", "<u4"), ("weight", "<u4"), ("anchor", "<i4", 3), ("sink", "<i4")])
SCATTER_PARAMS = np.dtype([("seed", "<u4"), ("flags", "<u4"), ("cell_log2", "<u4"), ("probability", "<u4"), ("surface_material", "<u4"), ("min_y", "<i4"),
                           ("max_y", "<i4"), ("radius", "<u4"), ("max_rise", "<u4"), ("max_drop", "<u4"), ("reserved", "<u4", 6)])
SCATTER_INFO = np.dtype([("version", "<u4"), ("flags", "<u4"), ("n_cells", "<u8"), ("n_placed", "<u8"), ("n_rejected", "<u8", 5), ("reserved", "<u8")])
SCATTER_ANY_MATERIAL, SCATTER_ROTATE, SCATTER_MIRROR = 1, 2, 4      # = BLOK_SCATTER_ANY_MATERIAL / _ROTATE / _MIRROR
SCATTER_MAX_ENTRIES = 16                          # = BLOK_SCATTER_MAX_ENTRIES
SCATTER_NO_LIMIT = 0xFFFF                         # max_rise / max_drop: no limit
# = blok_scroll_box (24 bytes) and blok_scroll_info (200 bytes): what a scroll of the volume's box did, or would do
SCROLL_BOX = np.dtype([("lo", "<i4", 3), ("hi", "<i4", 3)])
SCROLL_INFO = np.dtype([("origin", "<i4", 3), ("delta", "<i4", 3), ("n_exposed", "<u4"), ("n_leaving", "<u4"), ("exposed", SCROLL_BOX, 3), ("leaving", SCROLL_BOX, 3),
                        ("n_cells_kept", "<u8"), ("n_filled_before", "<u8"), ("n_filled_kept", "<u8")])
SCROLL_PLAN_ONLY = 1                              # = BLOK_SCROLL_PLAN_ONLY
# = blok_shape (64 bytes): one primitive of blok_hip_volume_apply_shapes with its operation; a, b, r in half-voxel units
SHAPE = np.dtype([("kind", "<u4"), ("op", "<u4"), ("a", "<i4", 3), ("b", "<i4", 3), ("r", "<u4", 3), ("material", "<u4"), ("match", "<u4"), ("value", "<f4"),
                  ("reserved", "<u4", 2)])
SHAPE_BOX, SHAPE_ELLIPSOID, SHAPE_CAPSULE, SHAPE_CYLINDER = 0, 1, 2, 3      # = BLOK_SHAPE_BOX .. _CYLINDER
SHAPE_SET, SHAPE_KEEP, SHAPE_ERASE, SHAPE_PAINT, SHAPE_REPLACE, SHAPE_ADD, SHAPE_SUBTRACT = range(7)      # = BLOK_SHAPE_SET .. _SUBTRACT
SHAPES_MAX = 65536                                # = BLOK_SHAPES_MAX
# = blok_lod_level (64 bytes) and blok_lod_info (360 bytes): the grids and counts of a pyramid of coarser levels, level j at ["level"][j - 1]
LOD_LEVEL = np.dtype([("clo", "<i4", 3), ("cext", "<u4", 3), ("n_cells", "<u8"), ("n_filled", "<u8"), ("n_exposed", "<u8"), ("sum_n", "<u8"), ("sum_e", "<u8")])
LOD_INFO = np.dtype([("version", "<u4"), ("flags", "<u4"), ("levels", "<u4"), ("reserved", "<u4"), ("lo", "<i4", 3), ("ext", "<u4", 3), ("level", LOD_LEVEL, 5)])
LOD_VOTE_EXPOSED = 1                              # = BLOK_LOD_VOTE_EXPOSED
LOD_MAX_LEVELS = 5                                # = BLOK_LOD_MAX_LEVELS
LOD_SEAMLESS = 2                                  # = BLOK_LOD_SEAMLESS (terrain_reduce only)
# = blok_affine (96 bytes): world -> model, m and t in units of 2^-16 model voxel (blok_amd.affine makes them)
AFFINE = np.dtype([("model", "<u4"), ("anchor", "<i4", 3), ("m", "<i4", (3, 3)), ("reserved", "<u4", 5), ("t", "<i8", 3)])
# = blok_automaton_rule (32 bytes) and blok_automaton_info (64 bytes): a neighbour-count rule and what a call of it did (blok_amd.automaton makes rules)
AUTOMATON_RULE = np.dtype([("neighbourhood", "<u4"), ("survive", "<u4"), ("birth", "<u4"), ("flags", "<u4"), ("density", "<f4"), ("material", "<u4"), ("steps", "<u4"),
                           ("reserved", "<u4")])
AUTOMATON_INFO = np.dtype([("version", "<u4"), ("flags", "<u4"), ("lo", "<i4", 3), ("ext", "<u4", 3), ("steps_run", "<u4"), ("reserved", "<u4"), ("n_born", "<u8"),
                           ("n_died", "<u8"), ("n_filled", "<u8")])
AUTOMATON_BOX_IS_SOLID, AUTOMATON_FIXED_MATERIAL = 1, 2      # = BLOK_AUTOMATON_BOX_IS_SOLID, _FIXED_MATERIAL


def flood_seed_face(f: int) -> int:
    """= BLOK_FLOOD_SEED_FACE(f): side f of the region (0 +X, 1 -X, 2 +Y, 3 -Y, 4 +Z, 5 -Z) is a seed layer."""
    return 1 << (8 + int(f))


assert SVO_NODE.itemsize == 16 and SUB_CHUNK.itemsize == 48 and MATERIAL.itemsize == 32
assert CAMERA.itemsize == 56 and HIT.itemsize == 16 and RAY.itemsize == 32 and INSTANCE.itemsize == 32 and QUAD.itemsize == 32
assert COMPONENT.itemsize == 40 and SWEEP_RESULT.itemsize == 16 and BRICK_RECORD.itemsize == 24 and BRICKS_INFO.itemsize == 64
assert DISTANCE_INFO.itemsize == 64 and FLOOD_INFO.itemsize == 64 and COLUMNS_INFO.itemsize == 64
assert SCATTER_ENTRY.itemsize == 24 and SCATTER_PARAMS.itemsize == 64 and SCATTER_INFO.itemsize == 72
assert SCROLL_BOX.itemsize == 24 and SCROLL_INFO.itemsize == 200 and SHAPE.itemsize == 64
assert LOD_LEVEL.itemsize == 64 and LOD_INFO.itemsize == 360 and AFFINE.itemsize == 96 and POSE.itemsize == 64
assert AUTOMATON_RULE.itemsize == 32 and AUTOMATON_INFO.itemsize == 64


class GBuffer(C.Structure):
    _fields_ = [("color", C.c_void_p), ("world_pos", C.c_void_p), ("normal_roughness", C.c_void_p),
                ("albedo_metallic", C.c_void_p)]


class GBufferRef(C.Structure):
    """= blok_gbuffer_ref: the reference's image formats (RGBA32F x 2, RGBA16F, RGBA8, RG16F)."""
    _fields_ = [("color", C.c_void_p), ("world_pos", C.c_void_p), ("normal_roughness", C.c_void_p),
                ("albedo_metallic", C.c_void_p), ("motion", C.c_void_p)]


class DenoiseSettings(C.Structure):
    """= blok_denoise_settings (Denoiser::Settings, reference blok/include/renderer_denoising.hpp:49-66)."""
    _fields_ = [("temporal_alpha", C.c_float), ("moment_alpha", C.c_float), ("variance_clip_gamma", C.c_float),
                ("depth_threshold", C.c_float), ("normal_threshold", C.c_float), ("phi_color", C.c_float),
                ("phi_normal", C.c_float), ("phi_depth", C.c_float), ("atrous_iterations", C.c_int32),
                ("variance_boost", C.c_float), ("min_history_length", C.c_int32)]


class TerrainParams(C.Structure):
    """= blok_terrain_params (include/blok_hip.h)."""
    _fields_ = [("seed", C.c_uint32), ("base_height", C.c_int32), ("amplitude", C.c_uint32), ("height_cell_log2", C.c_uint32),
                ("height_octaves", C.c_uint32), ("cave_cell_log2", C.c_uint32), ("cave_octaves", C.c_uint32), ("cave_threshold", C.c_uint32),
                ("cave_roof", C.c_uint32), ("soil_depth", C.c_uint32), ("ore_cell_log2", C.c_uint32), ("ore_threshold", C.c_uint32),
                ("surface_material", C.c_uint32), ("soil_material", C.c_uint32), ("rock_material", C.c_uint32), ("ore_material", C.c_uint32),
                ("density", C.c_float), ("flags", C.c_uint32)]


class ModelInfo(C.Structure):
    """= blok_model_info (include/blok_hip_debug.h)."""
    _fields_ = [("levels", C.c_uint32), ("origin", C.c_int32 * 3), ("lo", C.c_int32 * 3), ("hi", C.c_int32 * 3),
                ("n_nodes", C.c_uint64), ("n_materials", C.c_uint64)]


class WorldStats(C.Structure):
    _fields_ = [("n_voxels", C.c_uint64), ("n_ref_nodes", C.c_uint64), ("n_sub_chunks", C.c_uint64),
                ("n_tree_nodes", C.c_uint64), ("tree_bytes", C.c_uint64), ("levels", C.c_uint32),
                ("origin", C.c_int32 * 3)]


HOST_SYMBOLS = {
    "blok_morton_encode": (C.c_uint64, [C.c_int32, C.c_int32, C.c_int32]),
    "blok_morton_decode": (None, [C.c_uint64, C.POINTER(C.c_int32), C.POINTER(C.c_int32), C.POINTER(C.c_int32)]),
    "blok_morton_octant": (C.c_uint32, [C.c_uint64, C.c_uint32, C.c_uint32]),
    "blok_world_create": (C.c_int, [C.POINTER(C.c_void_p), C.c_uint32, C.c_float]),
    "blok_world_destroy": (None, [C.c_void_p]),
    "blok_world_last_error": (C.c_char_p, [C.c_void_p]),
    "blok_world_set_voxel": (C.c_int, [C.c_void_p, C.POINTER(C.c_float), C.c_uint32, C.c_float]),
    "blok_world_set_voxels": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t]),
    "blok_world_get_voxel_material": (C.c_uint32, [C.c_void_p, C.POINTER(C.c_float)]),
    "blok_world_apply_brush": (C.c_int, [C.c_void_p, C.POINTER(C.c_float), C.c_float, C.c_float, C.c_int]),
    "blok_world_rebuild_dirty": (C.c_int, [C.c_void_p, C.c_int]),
    "blok_world_pack": (C.c_int, [C.c_void_p]),
    "blok_world_node_count": (C.c_size_t, [C.c_void_p]),
    "blok_world_sub_chunk_count": (C.c_size_t, [C.c_void_p]),
    "blok_world_nodes": (C.c_void_p, [C.c_void_p]),
    "blok_world_sub_chunks": (C.c_void_p, [C.c_void_p]),
    "blok_world_chunk_count": (C.c_size_t, [C.c_void_p]),
    "blok_world_chunk_info": (C.c_int, [C.c_void_p, C.c_size_t, C.POINTER(C.c_int32), C.POINTER(C.c_uint64)]),
    "blok_world_chunk_nodes": (C.c_void_p, [C.c_void_p, C.c_size_t]),
    "blok_world_find_leaf": (C.c_int64, [C.c_void_p, C.c_size_t, C.c_uint32, C.c_uint32, C.c_uint32]),
    "blok_material_desc_init": (None, [C.c_void_p]),
    "blok_material_pack": (None, [C.c_void_p, C.c_void_p]),
    "blok_material_library_create": (C.c_int, [C.POINTER(C.c_void_p)]),
    "blok_material_library_destroy": (None, [C.c_void_p]),
    "blok_material_library_size": (C.c_uint32, [C.c_void_p]),
    "blok_material_library_add": (C.c_uint32, [C.c_void_p, C.c_void_p]),
    "blok_material_library_add_or_find": (C.c_uint32, [C.c_void_p, C.c_void_p]),
    "blok_material_library_get": (C.c_int, [C.c_void_p, C.c_uint32, C.c_void_p]),
    "blok_material_library_id_by_name": (C.c_uint32, [C.c_void_p, C.c_char_p]),
    "blok_material_library_from_color": (C.c_uint32, [C.c_void_p, C.c_uint8, C.c_uint8, C.c_uint8]),
    "blok_material_library_set_vox_palette": (None, [C.c_void_p, C.c_uint8, C.c_uint32]),
    "blok_material_library_from_vox_palette": (C.c_uint32, [C.c_void_p, C.c_uint8]),
    "blok_obj_load_file": (C.c_int, [C.c_char_p, C.c_void_p, C.POINTER(C.c_void_p), C.c_char_p, C.c_size_t]),
    "blok_obj_load_memory": (C.c_int, [C.c_char_p, C.c_size_t, C.c_char_p, C.c_size_t, C.c_void_p, C.POINTER(C.c_void_p), C.c_char_p, C.c_size_t]),
    "blok_mesh_free": (None, [C.c_void_p]),
    "blok_mesh_vertex_count": (C.c_size_t, [C.c_void_p]),
    "blok_mesh_triangle_count": (C.c_size_t, [C.c_void_p]),
    "blok_mesh_positions": (C.c_void_p, [C.c_void_p]),
    "blok_mesh_triangles": (C.c_void_p, [C.c_void_p]),
    "blok_mesh_materials": (C.c_void_p, [C.c_void_p]),
    "blok_material_library_pack": (C.c_int, [C.c_void_p, C.c_void_p, C.c_size_t]),
    "blok_material_library_clear": (None, [C.c_void_p]),
    "blok_world_set_material_library": (None, [C.c_void_p, C.c_void_p]),
    "blok_world_get_material_library": (C.c_void_p, [C.c_void_p]),
    "blok_world_set_voxel_rgb": (C.c_int, [C.c_void_p, C.POINTER(C.c_float), C.c_uint8, C.c_uint8, C.c_uint8, C.c_float]),
    "blok_vox_load_file": (C.c_int, [C.c_char_p, C.POINTER(C.c_void_p), C.c_char_p, C.c_size_t]),
    "blok_vox_load_memory": (C.c_int, [C.c_void_p, C.c_size_t, C.POINTER(C.c_void_p), C.c_char_p, C.c_size_t]),
    "blok_vox_free": (None, [C.c_void_p]),
    "blok_vox_model_count": (C.c_uint32, [C.c_void_p]),
    "blok_vox_model_info": (C.c_int, [C.c_void_p, C.c_uint32, C.POINTER(C.c_uint32), C.POINTER(C.c_uint32)]),
    "blok_vox_model_voxels": (C.c_void_p, [C.c_void_p, C.c_uint32]),
    "blok_vox_palette": (C.c_void_p, [C.c_void_p]),
    "blok_vox_get_material": (C.c_int, [C.c_void_p, C.c_uint8, C.c_void_p]),
    "blok_vox_import_materials": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p]),
    "blok_vox_import_to_world": (C.c_uint32, [C.c_void_p, C.c_void_p, C.POINTER(C.c_float), C.c_uint32]),
    "blok_load_and_import_vox": (C.c_int, [C.c_char_p, C.c_void_p, C.c_void_p, C.POINTER(C.c_float), C.c_uint32,
                                           C.c_char_p, C.c_size_t]),
    "blok_camera_from_yaw_pitch": (C.c_int, [C.POINTER(C.c_float), C.c_float, C.c_float, C.c_float,
                                             C.c_uint32, C.c_uint32, C.c_void_p]),
    "blok_camera_look_at": (C.c_int, [C.POINTER(C.c_float), C.POINTER(C.c_float), C.c_float,
                                      C.c_uint32, C.c_uint32, C.c_void_p]),
    "blok_camera_view": (None, [C.c_void_p, C.POINTER(C.c_float)]),
    "blok_camera_projection": (None, [C.c_void_p, C.c_float, C.c_float, C.POINTER(C.c_float)]),
    "blok_mat4_inverse": (C.c_int, [C.POINTER(C.c_float), C.POINTER(C.c_float)]),
    "blok_taa_jitter": (None, [C.c_uint32, C.POINTER(C.c_float)]),
    "blok_taa_jitter_clip": (None, [C.POINTER(C.c_float), C.c_uint32, C.c_uint32, C.POINTER(C.c_float)]),
    "blok_jittered_projection": (None, [C.POINTER(C.c_float), C.POINTER(C.c_float), C.c_uint32, C.c_uint32, C.POINTER(C.c_float)]),
    "blok_terrain_default_params": (C.c_int, [C.c_uint32, C.c_uint32, C.c_void_p]),
    "blok_terrain_validate": (C.c_int, [C.c_void_p]),
    "blok_terrain_height": (C.c_int, [C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p]),
    "blok_terrain_eval": (C.c_int, [C.c_void_p, C.POINTER(C.c_int32), C.POINTER(C.c_int32), C.c_void_p, C.c_void_p, C.POINTER(C.c_uint64)]),
    "blok_quads_extract": (C.c_int, [C.c_void_p, C.c_void_p, C.POINTER(C.c_int32), C.c_uint32, C.c_uint32, C.c_uint32, C.POINTER(C.c_int32),
                                     C.POINTER(C.c_int32), C.c_uint32, C.c_void_p, C.c_uint64, C.POINTER(C.c_uint64), C.POINTER(C.c_uint64)]),
    "blok_quads_write_obj": (C.c_int, [C.c_char_p, C.c_void_p, C.c_uint64, C.c_void_p, C.c_char_p, C.c_size_t]),
    "blok_lights_from_quads": (C.c_int, [C.c_void_p, C.c_uint64, C.c_void_p, C.c_size_t, C.c_void_p, C.c_uint64, C.c_float, C.c_void_p]),
    "blok_lights_check": (C.c_int, [C.c_void_p, C.c_uint64, C.c_void_p, C.c_char_p, C.c_size_t]),
    "blok_model_lights": (C.c_int, [C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p, C.c_size_t, C.c_void_p, C.c_uint64, C.c_void_p]),
    "blok_instance_light_record": (None, [C.c_void_p, C.c_uint32, C.c_void_p, C.c_void_p]),
    "blok_light_grid_build": (C.c_int, [C.c_void_p, C.c_uint64, C.c_uint32, C.c_uint32, C.c_uint32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint64, C.c_uint64, C.c_void_p]),
    "blok_stamp_voxels": (C.c_int, [C.c_void_p, C.c_void_p, C.POINTER(C.c_int32), C.c_uint32, C.c_uint32, C.c_uint32, C.c_void_p, C.c_void_p, C.c_size_t,
                                    C.c_void_p, C.c_int, C.c_float, C.POINTER(C.c_uint64)]),
    "blok_capture_voxels": (C.c_int, [C.c_void_p, C.c_void_p, C.POINTER(C.c_int32), C.c_uint32, C.c_uint32, C.c_uint32, C.POINTER(C.c_int32),
                                      C.POINTER(C.c_int32), C.c_void_p, C.c_void_p, C.c_uint64, C.POINTER(C.c_uint64)]),
    "blok_components_label": (C.c_int, [C.c_void_p, C.POINTER(C.c_int32), C.c_uint32, C.c_uint32, C.c_uint32, C.POINTER(C.c_int32), C.POINTER(C.c_int32),
                                        C.c_uint32, C.c_void_p, C.c_uint64, C.c_void_p, C.c_uint64, C.POINTER(C.c_uint64), C.POINTER(C.c_uint64)]),
    "blok_sweep_voxels": (C.c_int, [C.c_void_p, C.POINTER(C.c_int32), C.c_uint32, C.c_uint32, C.c_uint32, C.c_void_p, C.c_size_t, C.c_void_p, C.c_uint32,
                                    C.c_uint32, C.c_uint32, C.c_void_p]),
    "blok_bricks_encode": (C.c_int, [C.c_void_p, C.c_void_p, C.POINTER(C.c_int32), C.c_uint32, C.c_uint32, C.c_uint32, C.POINTER(C.c_int32),
                                     C.POINTER(C.c_int32), C.c_uint32, C.c_void_p, C.c_void_p, C.c_uint64, C.c_void_p, C.c_uint64, C.c_void_p, C.c_uint64]),
    "blok_bricks_validate": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_char_p, C.c_size_t]),
    "blok_bricks_decode": (C.c_int, [C.c_void_p, C.c_void_p, C.POINTER(C.c_int32), C.c_uint32, C.c_uint32, C.c_uint32, C.c_void_p, C.c_void_p, C.c_void_p,
                                     C.c_void_p, C.POINTER(C.c_int32), C.c_uint32, C.c_char_p, C.c_size_t]),
    "blok_bricks_write_file": (C.c_int, [C.c_char_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_char_p, C.c_size_t]),
    "blok_bricks_read_file": (C.c_int, [C.c_char_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_char_p, C.c_size_t]),
    "blok_distance_field": (C.c_int, [C.c_void_p, C.POINTER(C.c_int32), C.c_uint32, C.c_uint32, C.c_uint32, C.POINTER(C.c_int32), C.POINTER(C.c_int32),
                                      C.c_uint32, C.c_uint32, C.c_void_p, C.c_void_p]),
    "blok_distance_edit": (C.c_int, [C.c_void_p, C.c_void_p, C.POINTER(C.c_int32), C.c_uint32, C.c_uint32, C.c_uint32, C.c_void_p, C.c_void_p, C.c_int,
                                     C.c_uint32, C.c_float, C.c_uint32, C.POINTER(C.c_uint64)]),
    "blok_flood_field": (C.c_int, [C.c_void_p, C.c_void_p, C.POINTER(C.c_int32), C.c_uint32, C.c_uint32, C.c_uint32, C.POINTER(C.c_int32), C.POINTER(C.c_int32),
                                   C.c_void_p, C.c_uint64, C.c_uint32, C.c_uint32, C.c_uint32, C.c_void_p, C.c_void_p]),
    "blok_flood_edit": (C.c_int, [C.c_void_p, C.c_void_p, C.POINTER(C.c_int32), C.c_uint32, C.c_uint32, C.c_uint32, C.c_void_p, C.c_void_p, C.c_int,
                                  C.c_uint32, C.c_float, C.c_uint32, C.POINTER(C.c_uint64)]),
    "blok_column_field": (C.c_int, [C.c_void_p, C.c_void_p, C.POINTER(C.c_int32), C.c_uint32, C.c_uint32, C.c_uint32, C.POINTER(C.c_int32), C.POINTER(C.c_int32),
                                    C.c_uint32, C.c_uint32, C.c_void_p, C.c_void_p, C.c_void_p]),
    "blok_scatter": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint32, C.c_void_p, C.c_uint64, C.c_void_p]),
    "blok_scroll_plan": (C.c_int, [C.POINTER(C.c_int32), C.c_uint32, C.c_uint32, C.c_uint32, C.POINTER(C.c_int32), C.c_void_p]),
    "blok_scroll_voxels": (C.c_int, [C.c_void_p, C.c_void_p, C.POINTER(C.c_int32), C.c_uint32, C.c_uint32, C.c_uint32, C.POINTER(C.c_int32), C.c_void_p, C.c_void_p,
                                     C.c_void_p]),
    "blok_shapes_check": (C.c_int, [C.c_void_p, C.c_uint32, C.POINTER(C.c_uint32), C.c_char_p, C.c_size_t]),
    "blok_shape_bounds": (C.c_int, [C.c_void_p, C.POINTER(C.c_int32), C.POINTER(C.c_int32)]),
    "blok_shapes_voxels": (C.c_int, [C.c_void_p, C.c_void_p, C.POINTER(C.c_int32), C.c_uint32, C.c_uint32, C.c_uint32, C.c_void_p, C.c_uint32, C.POINTER(C.c_uint64)]),
    "blok_lod_reduce": (C.c_int, [C.c_void_p, C.c_void_p, C.POINTER(C.c_int32), C.c_uint32, C.c_uint32, C.c_uint32, C.POINTER(C.c_int32), C.POINTER(C.c_int32),
                                  C.c_uint32, C.c_uint32, C.c_void_p, C.c_uint64, C.c_void_p]),
    "blok_terrain_reduce": (C.c_int, [C.c_void_p, C.POINTER(C.c_int32), C.POINTER(C.c_int32), C.c_uint32, C.c_uint32, C.c_void_p, C.c_uint64, C.c_void_p]),
    "blok_automaton_check": (C.c_int, [C.c_void_p, C.c_char_p, C.c_size_t]),
    "blok_automaton_voxels": (C.c_int, [C.c_void_p, C.c_void_p, C.POINTER(C.c_int32), C.c_uint32, C.c_uint32, C.c_uint32, C.POINTER(C.c_int32), C.POINTER(C.c_int32),
                                        C.c_void_p, C.c_void_p, C.c_void_p]),
    "blok_affine_from_instance": (C.c_int, [C.c_void_p, C.c_uint32, C.c_void_p]),
    "blok_affine_from_matrix": (C.c_int, [C.POINTER(C.c_double), C.c_void_p]),
    "blok_pose_from_instance": (C.c_int, [C.c_void_p, C.c_float, C.c_void_p]),
    "blok_pose_from_matrix": (C.c_int, [C.POINTER(C.c_double), C.POINTER(C.c_double), C.c_uint32, C.c_void_p]),
    "blok_affine_from_pose": (C.c_int, [C.c_void_p, C.c_float, C.c_uint32, C.c_void_p]),
    "blok_pose_motion_record": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_void_p]),
    "blok_affine_stamp_voxels": (C.c_int, [C.c_void_p, C.c_void_p, C.POINTER(C.c_int32), C.c_uint32, C.c_uint32, C.c_uint32, C.c_void_p, C.c_void_p, C.c_size_t,
                                           C.c_void_p, C.POINTER(C.c_int32), C.POINTER(C.c_int32), C.c_int, C.c_float, C.POINTER(C.c_uint64)]),
    "blok_scene_generate": (C.c_int, [C.c_void_p, C.c_uint32, C.c_uint32, C.POINTER(C.c_uint64)]),
    "blok_scene_generate_dense": (C.c_int, [C.c_uint32, C.c_uint32, C.c_void_p, C.POINTER(C.c_uint64)]),
    "blok_scene_materials": (C.c_int, [C.c_uint32, C.c_void_p]),
    "blok_scene_camera": (C.c_int, [C.c_uint32, C.c_uint32, C.c_int, C.c_uint32, C.c_uint32, C.c_void_p]),
}

HIP_SYMBOLS = {
    "blok_hip_create": (C.c_int, [C.POINTER(C.c_void_p), C.c_int, C.c_uint32, C.c_uint32]),
    "blok_hip_resize": (C.c_int, [C.c_void_p, C.c_uint32, C.c_uint32]),
    "blok_hip_destroy": (None, [C.c_void_p]),
    "blok_hip_last_error": (C.c_char_p, [C.c_void_p]),
    "blok_hip_release_stream": (C.c_int, [C.c_void_p, C.c_void_p]),
    "blok_hip_upload_world": (C.c_int, [C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p, C.c_size_t,
                                        C.c_void_p, C.c_size_t]),
    "blok_hip_upload_dense": (C.c_int, [C.c_void_p, C.c_void_p, C.c_uint32, C.c_uint32, C.c_uint32,
                                        C.POINTER(C.c_int32), C.c_void_p, C.c_size_t]),
    "blok_hip_set_host_build": (C.c_int, [C.c_void_p, C.c_int]),
    "blok_hip_world_built_on_device": (C.c_int, [C.c_void_p]),
    "blok_hip_download_tree": (C.c_int, [C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p, C.c_size_t]),
    "blok_hip_world_stats": (C.c_int, [C.c_void_p, C.POINTER(WorldStats)]),
    "blok_hip_trace_primary": (C.c_int, [C.c_void_p, C.c_void_p, C.c_uint32, C.c_uint32, C.c_uint32,
                                         C.c_uint32, C.c_void_p]),
    "blok_hip_trace_primary_device": (C.c_int, [C.c_void_p, C.c_void_p, C.c_uint32, C.c_uint32,
                                                C.c_uint32, C.c_uint32, C.c_void_p, C.c_void_p, C.c_void_p]),
    "blok_hip_tiles_for_rank": (C.c_uint32, [C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32]),
    "blok_hip_trace_tiles_device": (C.c_int, [C.c_void_p, C.c_void_p, C.c_uint32, C.c_uint32, C.c_uint32,
                                              C.c_void_p, C.c_void_p, C.c_void_p]),
    "blok_hip_untile_device": (C.c_int, [C.c_void_p, C.c_void_p, C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32,
                                         C.c_void_p, C.c_void_p]),
    "blok_hip_trace_paths_device": (C.c_int, [C.c_void_p, C.c_void_p] + [C.c_uint32] * 7 + [C.POINTER(GBuffer), C.c_void_p]),
    "blok_hip_trace_paths": (C.c_int, [C.c_void_p, C.c_void_p] + [C.c_uint32] * 7 + [C.POINTER(GBuffer)]),
    "blok_hip_trace_paths_ref_device": (C.c_int, [C.c_void_p, C.c_void_p] + [C.c_uint32] * 7 + [C.POINTER(C.c_float), C.POINTER(GBufferRef), C.c_void_p]),
    "blok_hip_denoise_ref_device": (C.c_int, [C.c_void_p, C.POINTER(GBufferRef), C.POINTER(C.c_float), C.c_uint32, C.c_void_p, C.c_void_p, C.c_void_p]),
    "blok_hip_tonemap_device": (C.c_int, [C.c_void_p, C.c_void_p, C.c_uint32, C.c_float, C.c_float, C.c_int, C.c_void_p, C.c_void_p]),
    "blok_hip_tonemap": (C.c_int, [C.c_void_p, C.c_void_p, C.c_uint32, C.c_float, C.c_float, C.c_int, C.c_void_p]),
    "blok_hip_trace_rays": (C.c_int, [C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p]),
    "blok_hip_shade_rgba8": (C.c_int, [C.c_void_p, C.c_void_p, C.c_uint32, C.c_uint32, C.c_uint32,
                                       C.c_uint32, C.c_void_p]),
    "blok_hip_draw_frame_accumulate": (C.c_int, [C.c_void_p, C.c_void_p, C.c_uint32, C.c_uint32, C.c_void_p, C.POINTER(C.c_uint32)]),
    "blok_hip_accum_download": (C.c_int, [C.c_void_p, C.c_void_p]),
    "blok_hip_reset_accum": (C.c_int, [C.c_void_p]),
    "blok_hip_set_beam": (C.c_int, [C.c_void_p, C.c_uint32]),
    "blok_hip_set_fused": (C.c_int, [C.c_void_p, C.c_int]),
    "blok_hip_set_dense_dda": (C.c_int, [C.c_void_p, C.c_int]),
    "blok_hip_set_voxel_size": (C.c_int, [C.c_void_p, C.c_float]),
    "blok_hip_multi_create": (C.c_int, [C.POINTER(C.c_void_p), C.POINTER(C.c_int), C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32, C.c_int]),
    "blok_hip_multi_destroy": (None, [C.c_void_p]),
    "blok_hip_multi_last_error": (C.c_char_p, [C.c_void_p]),
    "blok_hip_multi_device_count": (C.c_uint32, [C.c_void_p]),
    "blok_hip_multi_transport": (C.c_char_p, [C.c_void_p]),
    "blok_hip_multi_context": (C.c_void_p, [C.c_void_p, C.c_uint32]),
    "blok_hip_multi_upload_world": (C.c_int, [C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p, C.c_size_t, C.c_void_p, C.c_size_t]),
    "blok_hip_multi_draw_frame_device": (C.c_int, [C.c_void_p, C.c_void_p, C.POINTER(C.c_void_p)]),
    "blok_hip_multi_synchronize": (C.c_int, [C.c_void_p]),
    "blok_hip_multi_draw_frame": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p]),
    "blok_hip_multi_set_exchange": (C.c_int, [C.c_void_p, C.c_int]),
    "blok_hip_multi_exchange": (C.c_char_p, [C.c_void_p]),
    "blok_hip_multi_debug_deny_peer_access": (C.c_int, [C.c_void_p, C.c_int]),
    "blok_hip_multi_draw_frames_device": (C.c_int, [C.c_void_p, C.c_void_p, C.c_uint32, C.POINTER(C.c_void_p)]),
    "blok_hip_multi_draw_frames": (C.c_int, [C.c_void_p, C.c_void_p, C.c_uint32, C.c_void_p]),
    "blok_hip_multi_download_hits": (C.c_int, [C.c_void_p, C.c_uint32, C.c_void_p, C.c_size_t]),
    "blok_hip_set_beam_budget": (C.c_int, [C.c_void_p, C.c_uint32]),
    "blok_hip_beam_cache_download": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t]),
    "blok_hip_set_miss_writer": (C.c_int, [C.c_void_p, C.c_int]),
    "blok_hip_set_beam_cache": (C.c_int, [C.c_void_p, C.c_int]),
    "blok_hip_beam_cache_counters": (C.c_int, [C.c_void_p, C.POINTER(C.c_uint64), C.POINTER(C.c_uint64)]),
    "blok_hip_beam_cache_download_starts": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p, C.c_size_t]),
    "blok_hip_beam_cache_start_counters": (C.c_int, [C.c_void_p, C.POINTER(C.c_uint64), C.POINTER(C.c_uint64)]),
    "blok_hip_beam_cache_download_nodes": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p, C.c_size_t]),
    "blok_hip_beam_cache_node_counters": (C.c_int, [C.c_void_p, C.POINTER(C.c_uint64)]),
    "blok_hip_set_packed_fill": (C.c_int, [C.c_void_p, C.c_uint32]),
    "blok_hip_packed_fill_counters": (C.c_int, [C.c_void_p, C.POINTER(C.c_uint64), C.POINTER(C.c_uint64)]),
    "blok_hip_beam_cache_refines": (C.c_int, [C.c_void_p, C.POINTER(C.c_uint64)]),
    "blok_hip_set_beam_refine_after": (C.c_int, [C.c_void_p, C.c_uint32]),
    "blok_hip_beam_cache_download_fine": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t]),
    "blok_hip_pack_area": (C.c_uint32, []),
    "blok_hip_set_beam_list_after": (C.c_int, [C.c_void_p, C.c_uint32]),
    "blok_hip_beam_cache_list_builds": (C.c_int, [C.c_void_p, C.POINTER(C.c_uint64)]),
    "blok_hip_beam_cache_download_list": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p, C.c_size_t, C.c_void_p, C.c_size_t]),
    "blok_hip_last_launch_kind": (C.c_int, [C.c_void_p]),
    "blok_hip_set_volume_layout": (C.c_int, [C.c_void_p, C.c_int]),
    "blok_hip_set_list_classes": (C.c_int, [C.c_void_p, C.c_int]),
    "blok_hip_set_joint_prefix_limit": (C.c_int, [C.c_void_p, C.c_uint32]),
    "blok_hip_set_tile_ordering": (C.c_int, [C.c_void_p, C.c_int]),
    "blok_hip_set_rank_tile_ordering": (C.c_int, [C.c_void_p, C.c_int]),
    "blok_hip_set_moving_order": (C.c_int, [C.c_void_p, C.c_int]),
    "blok_hip_last_fallback_tiles": (C.c_int64, [C.c_void_p]),
    "blok_hip_debug_force_order_shift": (C.c_int, [C.c_void_p, C.c_int, C.c_uint32, C.c_uint32]),
    "blok_hip_debug_class_order": (C.c_int, [C.c_void_p, C.c_void_p, C.c_uint32, C.c_uint32, C.c_uint32, C.c_void_p, C.c_uint32, C.c_void_p, C.c_void_p, C.POINTER(C.c_uint32), C.c_void_p]),
    "blok_hip_last_order_use": (C.c_int, [C.c_void_p, C.POINTER(C.c_int32), C.POINTER(C.c_int32)]),
    "blok_hip_beam_prepass": (C.c_int, [C.c_void_p, C.c_void_p] + [C.c_uint32] * 4 + [C.c_void_p, C.c_void_p, C.c_size_t]),
    "blok_hip_trace_wave_tiles_device": (C.c_int, [C.c_void_p, C.c_void_p] + [C.c_uint32] * 4 + [C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p, C.c_void_p, C.c_void_p]),
    "blok_hip_set_debug_wave_clocks": (C.c_int, [C.c_void_p, C.c_void_p]),
    "blok_hip_set_taa_jitter": (C.c_int, [C.c_void_p, C.POINTER(C.c_float)]),
    "blok_hip_set_rt_taa_jitter": (C.c_int, [C.c_void_p, C.c_int]),
    "blok_hip_compact_words": (C.c_size_t, [C.c_uint32, C.c_uint32]),
    "blok_hip_trace_tile_frames_device": (C.c_int, [C.c_void_p, C.c_void_p, C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32,
                                                    C.c_void_p, C.c_void_p, C.c_void_p]),
    "blok_hip_untile_frames_device": (C.c_int, [C.c_void_p, C.c_void_p, C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32,
                                                C.c_void_p, C.c_void_p]),
    "blok_hip_compact_tile_frames_device": (C.c_int, [C.c_void_p, C.c_void_p, C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32, C.c_void_p,
                                                      C.c_void_p]),
    "blok_hip_scatter_tile_frames_device": (C.c_int, [C.c_void_p, C.c_void_p, C.c_uint32, C.c_size_t, C.c_uint32, C.c_uint32, C.c_uint32,
                                                      C.c_void_p, C.c_void_p, C.c_void_p]),
    "blok_hip_exchange_code_bits": (C.c_uint32, [C.c_void_p]),
    "blok_hip_compact_code_words": (C.c_size_t, [C.c_uint32, C.c_uint32]),
    "blok_hip_compact_hit_tile_frames_device": (C.c_int, [C.c_void_p, C.c_void_p, C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32, C.c_void_p,
                                                          C.c_void_p]),
    "blok_hip_scatter_code_tile_frames_device": (C.c_int, [C.c_void_p, C.c_void_p, C.c_uint32, C.c_size_t, C.c_uint32, C.c_uint32, C.c_uint32,
                                                           C.c_void_p, C.c_void_p, C.c_void_p]),
    "blok_hip_compact_tiles_device": (C.c_int, [C.c_void_p, C.c_void_p, C.c_uint32, C.c_uint32, C.c_void_p, C.c_void_p]),
    "blok_hip_scatter_tiles_device": (C.c_int, [C.c_void_p, C.c_void_p, C.c_uint32, C.c_size_t, C.c_uint32, C.c_uint32, C.c_void_p, C.c_void_p]),
    "blok_hip_frame_queue_stalls": (C.c_int, [C.c_void_p, C.POINTER(C.c_uint32)]),
    "blok_hip_set_sun_map": (C.c_int, [C.c_void_p, C.c_int]),
    "blok_hip_sun_map_download": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t]),
    "blok_hip_set_ray_batching": (C.c_int, [C.c_void_p, C.c_int]),
    "blok_hip_set_path_start": (C.c_int, [C.c_void_p, C.c_int, C.c_int]),
    "blok_denoise_settings_default": (None, [C.c_void_p]),
    "blok_hip_denoise_device": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.POINTER(C.c_float), C.c_uint32, C.c_void_p,
                                          C.c_void_p, C.c_void_p]),
    "blok_hip_denoise_state": (C.c_int, [C.c_void_p] * 6),
    "blok_hip_taa_device": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_float, C.c_float, C.c_uint32, C.c_void_p, C.c_void_p]),
    "blok_hip_sharpen_device": (C.c_int, [C.c_void_p, C.c_void_p, C.c_float, C.c_void_p, C.c_void_p]),
    "blok_hip_post_reset": (C.c_int, [C.c_void_p]),
    "blok_camera_view_proj": (None, [C.c_void_p, C.POINTER(C.c_float)]),
    "blok_hip_draw_frame_rt": (C.c_int, [C.c_void_p, C.c_void_p, C.c_uint32, C.c_uint32, C.c_void_p, C.c_void_p, C.POINTER(C.c_uint32)]),
    "blok_hip_volume_create": (C.c_int, [C.c_void_p, C.POINTER(C.c_int32), C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32, C.c_float]),
    "blok_hip_volume_destroy": (C.c_int, [C.c_void_p]),
    "blok_hip_volume_upload": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p]),
    "blok_hip_volume_download": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p]),
    "blok_hip_volume_set_voxels": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t]),
    "blok_hip_volume_apply_brush": (C.c_int, [C.c_void_p, C.POINTER(C.c_float), C.c_float, C.c_float, C.c_int]),
    "blok_hip_volume_rebuild": (C.c_int, [C.c_void_p, C.c_void_p, C.c_size_t]),
    "blok_hip_volume_voxelize_mesh": (C.c_int, [C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p, C.c_size_t, C.c_void_p, C.c_uint32, C.c_float,
                                               C.c_int, C.POINTER(C.c_uint64)]),
    "blok_hip_volume_generate_terrain": (C.c_int, [C.c_void_p, C.c_void_p, C.POINTER(C.c_int32), C.POINTER(C.c_int32), C.POINTER(C.c_uint64)]),
    "blok_hip_volume_extract_quads": (C.c_int, [C.c_void_p, C.POINTER(C.c_int32), C.POINTER(C.c_int32), C.c_uint32, C.POINTER(C.c_uint64),
                                                C.POINTER(C.c_uint64)]),
    "blok_hip_volume_quads_download": (C.c_int, [C.c_void_p, C.c_void_p, C.c_uint64, C.c_uint64]),
    "blok_hip_lights_from_quads": (C.c_int, [C.c_void_p, C.c_uint32, C.c_void_p]),
    "blok_hip_set_lights": (C.c_int, [C.c_void_p, C.c_void_p, C.c_uint32, C.c_void_p]),
    "blok_hip_lights_info": (C.c_int, [C.c_void_p, C.c_void_p]),
    "blok_hip_lights_download": (C.c_int, [C.c_void_p, C.c_void_p, C.c_uint64, C.c_uint64]),
    "blok_hip_build_light_grid": (C.c_int, [C.c_void_p, C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32, C.c_void_p]),
    "blok_hip_light_grid_info": (C.c_int, [C.c_void_p, C.c_void_p]),
    "blok_hip_light_grid_download": (C.c_int, [C.c_void_p, C.c_uint32, C.c_void_p, C.c_uint64, C.c_uint64]),
    "blok_hip_light_grid_clear": (C.c_int, [C.c_void_p]),
    "blok_hip_model_lights": (C.c_int, [C.c_void_p, C.c_uint32, C.c_uint32, C.c_void_p]),
    "blok_hip_model_lights_info": (C.c_int, [C.c_void_p, C.c_uint32, C.c_void_p]),
    "blok_hip_model_lights_download": (C.c_int, [C.c_void_p, C.c_uint32, C.c_void_p, C.c_uint64, C.c_uint64]),
    "blok_hip_model_lights_clear": (C.c_int, [C.c_void_p, C.c_uint32]),
    "blok_hip_instance_lights_info": (C.c_int, [C.c_void_p, C.c_void_p, C.c_uint32, C.c_void_p, C.c_void_p]),
    "blok_hip_volume_stamp_models": (C.c_int, [C.c_void_p, C.c_void_p, C.c_uint32, C.c_int, C.c_float, C.POINTER(C.c_uint64)]),
    "blok_hip_volume_stamp_affine": (C.c_int, [C.c_void_p, C.c_void_p, C.c_uint32, C.POINTER(C.c_int32), C.POINTER(C.c_int32), C.c_int, C.c_float,
                                               C.POINTER(C.c_uint64)]),
    "blok_hip_volume_capture_model": (C.c_int, [C.c_void_p, C.POINTER(C.c_int32), C.POINTER(C.c_int32), C.c_uint32, C.POINTER(C.c_uint32),
                                                C.POINTER(C.c_uint64)]),
    "blok_hip_volume_label_components": (C.c_int, [C.c_void_p, C.POINTER(C.c_int32), C.POINTER(C.c_int32), C.c_uint32, C.POINTER(C.c_uint64),
                                                   C.POINTER(C.c_uint64)]),
    "blok_hip_volume_components_download": (C.c_int, [C.c_void_p, C.c_void_p, C.c_uint64, C.c_uint64]),
    "blok_hip_volume_labels_download": (C.c_int, [C.c_void_p, C.c_void_p, C.c_uint64, C.c_uint64]),
    "blok_hip_volume_capture_component": (C.c_int, [C.c_void_p, C.c_uint32, C.c_uint32, C.POINTER(C.c_uint32), C.POINTER(C.c_int32),
                                                    C.POINTER(C.c_uint64)]),
    "blok_hip_volume_sweep_models": (C.c_int, [C.c_void_p, C.c_void_p, C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32, C.c_void_p]),
    "blok_hip_volume_encode_bricks": (C.c_int, [C.c_void_p, C.POINTER(C.c_int32), C.POINTER(C.c_int32), C.c_uint32, C.c_void_p]),
    "blok_hip_volume_bricks_info": (C.c_int, [C.c_void_p, C.c_void_p]),
    "blok_hip_volume_bricks_download": (C.c_int, [C.c_void_p, C.c_void_p, C.c_uint64, C.c_uint64]),
    "blok_hip_volume_brick_payload_download": (C.c_int, [C.c_void_p, C.c_uint32, C.c_void_p, C.c_uint64, C.c_uint64]),
    "blok_hip_volume_restore_bricks": (C.c_int, [C.c_void_p, C.POINTER(C.c_int32), C.c_uint32]),
    "blok_hip_volume_decode_bricks": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.POINTER(C.c_int32), C.c_uint32]),
    "blok_hip_volume_distance_field": (C.c_int, [C.c_void_p, C.POINTER(C.c_int32), C.POINTER(C.c_int32), C.c_uint32, C.c_uint32, C.c_void_p]),
    "blok_hip_volume_distance_info": (C.c_int, [C.c_void_p, C.c_void_p]),
    "blok_hip_volume_distance_download": (C.c_int, [C.c_void_p, C.c_void_p, C.c_uint64, C.c_uint64]),
    "blok_hip_volume_edit_by_distance": (C.c_int, [C.c_void_p, C.c_int, C.c_uint32, C.c_float, C.c_uint32, C.POINTER(C.c_uint64)]),
    "blok_hip_volume_flood_field": (C.c_int, [C.c_void_p, C.POINTER(C.c_int32), C.POINTER(C.c_int32), C.c_void_p, C.c_uint64, C.c_uint32, C.c_uint32, C.c_uint32,
                                              C.c_void_p]),
    "blok_hip_volume_flood_info": (C.c_int, [C.c_void_p, C.c_void_p]),
    "blok_hip_volume_flood_download": (C.c_int, [C.c_void_p, C.c_void_p, C.c_uint64, C.c_uint64]),
    "blok_hip_volume_edit_by_flood": (C.c_int, [C.c_void_p, C.c_int, C.c_uint32, C.c_float, C.c_uint32, C.POINTER(C.c_uint64)]),
    "blok_hip_volume_column_field": (C.c_int, [C.c_void_p, C.POINTER(C.c_int32), C.POINTER(C.c_int32), C.c_uint32, C.c_uint32, C.c_void_p]),
    "blok_hip_volume_columns_info": (C.c_int, [C.c_void_p, C.c_void_p]),
    "blok_hip_volume_columns_download": (C.c_int, [C.c_void_p, C.c_uint32, C.c_void_p, C.c_uint64, C.c_uint64]),
    "blok_hip_volume_scatter_models": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint32, C.c_void_p]),
    "blok_hip_volume_scatter_info": (C.c_int, [C.c_void_p, C.c_void_p]),
    "blok_hip_volume_scatter_download": (C.c_int, [C.c_void_p, C.c_void_p, C.c_uint64, C.c_uint64]),
    "blok_hip_volume_scatter_device": (C.c_int, [C.c_void_p, C.POINTER(C.c_void_p), C.POINTER(C.c_uint64)]),
    "blok_hip_volume_scroll": (C.c_int, [C.c_void_p, C.POINTER(C.c_int32), C.c_uint32, C.c_void_p]),
    "blok_hip_volume_apply_shapes": (C.c_int, [C.c_void_p, C.c_void_p, C.c_uint32, C.POINTER(C.c_uint64)]),
    "blok_hip_volume_reduce": (C.c_int, [C.c_void_p, C.POINTER(C.c_int32), C.POINTER(C.c_int32), C.c_uint32, C.c_uint32, C.c_void_p]),
    "blok_hip_volume_lod_info": (C.c_int, [C.c_void_p, C.c_void_p]),
    "blok_hip_volume_lod_download": (C.c_int, [C.c_void_p, C.c_uint32, C.c_uint32, C.c_void_p, C.c_uint64, C.c_uint64]),
    "blok_hip_volume_lod_model": (C.c_int, [C.c_void_p, C.c_uint32, C.c_uint32, C.POINTER(C.c_uint32), C.POINTER(C.c_uint64)]),
    "blok_hip_terrain_reduce": (C.c_int, [C.c_void_p, C.c_void_p, C.POINTER(C.c_int32), C.POINTER(C.c_int32), C.c_uint32, C.c_uint32, C.c_void_p]),
    "blok_hip_volume_automaton": (C.c_int, [C.c_void_p, C.POINTER(C.c_int32), C.POINTER(C.c_int32), C.c_void_p, C.c_void_p, C.c_void_p]),
    "blok_hip_download_model": (C.c_int, [C.c_void_p, C.c_uint32, C.c_void_p, C.c_size_t, C.c_void_p, C.c_size_t, C.c_void_p]),
    "blok_hip_last_kernel_ms": (C.c_int, [C.c_void_p, C.POINTER(C.c_float)]),
    "blok_hip_set_timing": (C.c_int, [C.c_void_p, C.c_int]),
    "blok_hip_abi_version": (C.c_uint32, []),
    "blok_hip_model_create": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t, C.POINTER(C.c_uint32)]),
    "blok_hip_model_destroy": (C.c_int, [C.c_void_p, C.c_uint32]),
    "blok_hip_model_set_scale": (C.c_int, [C.c_void_p, C.c_uint32, C.c_uint32]),
    "blok_hip_model_scale": (C.c_int, [C.c_void_p, C.c_uint32, C.POINTER(C.c_uint32)]),
    "blok_hip_check_instances": (C.c_int, [C.c_void_p, C.c_void_p, C.c_uint32]),
    "blok_hip_trace_primary_instanced_device": (C.c_int, [C.c_void_p, C.c_void_p] + [C.c_uint32] * 4 + [C.c_void_p, C.c_uint32] + [C.c_void_p] * 4),
    "blok_hip_trace_primary_instanced": (C.c_int, [C.c_void_p, C.c_void_p] + [C.c_uint32] * 4 + [C.c_void_p, C.c_uint32] + [C.c_void_p] * 3),
    "blok_hip_trace_rays_instanced": (C.c_int, [C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p, C.c_uint32, C.c_void_p, C.c_void_p]),
    "blok_hip_trace_rays_instanced_device": (C.c_int, [C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p, C.c_uint32, C.c_void_p, C.c_void_p, C.c_void_p]),
    "blok_hip_check_poses": (C.c_int, [C.c_void_p, C.c_void_p, C.c_uint32]),
    "blok_hip_trace_primary_posed_device": (C.c_int, [C.c_void_p, C.c_void_p] + [C.c_uint32] * 4 + [C.c_void_p, C.c_uint32, C.c_void_p, C.c_uint32] + [C.c_void_p] * 4),
    "blok_hip_trace_primary_posed": (C.c_int, [C.c_void_p, C.c_void_p] + [C.c_uint32] * 4 + [C.c_void_p, C.c_uint32, C.c_void_p, C.c_uint32] + [C.c_void_p] * 3),
    "blok_hip_trace_rays_posed": (C.c_int, [C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p, C.c_uint32, C.c_void_p, C.c_uint32, C.c_void_p, C.c_void_p]),
    "blok_hip_trace_rays_posed_device": (C.c_int, [C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p, C.c_uint32, C.c_void_p, C.c_uint32, C.c_void_p, C.c_void_p, C.c_void_p]),
    "blok_hip_trace_paths_instanced_device": (C.c_int, [C.c_void_p, C.c_void_p] + [C.c_uint32] * 7 + [C.c_void_p, C.c_uint32, C.POINTER(GBuffer), C.c_void_p, C.c_void_p]),
    "blok_hip_trace_paths_instanced_ref_device": (C.c_int, [C.c_void_p, C.c_void_p] + [C.c_uint32] * 7 + [C.c_void_p, C.c_uint32, C.POINTER(C.c_float),
                                                                                                          C.POINTER(GBufferRef), C.c_void_p, C.c_void_p]),
    "blok_hip_trace_paths_instanced": (C.c_int, [C.c_void_p, C.c_void_p] + [C.c_uint32] * 7 + [C.c_void_p, C.c_uint32, C.POINTER(GBuffer), C.c_void_p]),
    "blok_hip_draw_frame_rt_instanced": (C.c_int, [C.c_void_p, C.c_void_p, C.c_uint32, C.c_uint32, C.c_void_p, C.c_void_p, C.c_uint32, C.c_void_p,
                                                   C.POINTER(C.c_uint32)]),
    "blok_hip_trace_paths_posed_device": (C.c_int, [C.c_void_p, C.c_void_p] + [C.c_uint32] * 7 + [C.c_void_p, C.c_uint32, C.c_void_p, C.c_uint32, C.POINTER(GBuffer),
                                                                                                  C.c_void_p, C.c_void_p]),
    "blok_hip_trace_paths_posed_ref_device": (C.c_int, [C.c_void_p, C.c_void_p] + [C.c_uint32] * 7 + [C.c_void_p, C.c_uint32, C.c_void_p, C.c_uint32,
                                                                                                      C.POINTER(C.c_float), C.POINTER(GBufferRef), C.c_void_p, C.c_void_p]),
    "blok_hip_trace_paths_posed": (C.c_int, [C.c_void_p, C.c_void_p] + [C.c_uint32] * 7 + [C.c_void_p, C.c_uint32, C.c_void_p, C.c_uint32, C.POINTER(GBuffer),
                                                                                           C.c_void_p]),
    "blok_hip_draw_frame_rt_posed": (C.c_int, [C.c_void_p, C.c_void_p, C.c_uint32, C.c_uint32, C.c_void_p, C.c_void_p, C.c_uint32, C.c_void_p, C.c_uint32,
                                               C.c_void_p, C.POINTER(C.c_uint32)]),
    "blok_hip_instance_motion_device": (C.c_int, [C.c_void_p] + [C.c_uint32] * 4 + [C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint32, C.c_void_p,
                                                                       C.c_uint32, C.POINTER(C.c_float), C.c_void_p, C.c_void_p, C.c_void_p]),
    "blok_hip_denoise_instanced_device": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.POINTER(C.c_float), C.c_uint32, C.c_void_p,
                                                    C.c_void_p, C.c_void_p, C.c_uint32, C.c_void_p, C.c_uint32, C.c_void_p, C.c_void_p]),
    "blok_hip_denoise_instanced_ref_device": (C.c_int, [C.c_void_p, C.POINTER(GBufferRef), C.POINTER(C.c_float), C.c_uint32, C.c_void_p,
                                                        C.c_void_p, C.c_void_p, C.c_uint32, C.c_void_p, C.c_uint32, C.c_void_p, C.c_void_p]),
    "blok_hip_draw_frame_rt_instanced_motion": (C.c_int, [C.c_void_p, C.c_void_p, C.c_uint32, C.c_uint32, C.c_void_p, C.c_void_p, C.c_uint32,
                                                          C.c_void_p, C.POINTER(C.c_uint32)]),
    "blok_hip_posed_motion_device": (C.c_int, [C.c_void_p] + [C.c_uint32] * 4 + [C.c_void_p, C.c_void_p] + [C.c_void_p, C.c_uint32] * 4 +
                                     [C.POINTER(C.c_float), C.c_void_p, C.c_void_p, C.c_void_p]),
    "blok_hip_denoise_posed_device": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.POINTER(C.c_float), C.c_uint32, C.c_void_p, C.c_void_p] +
                                      [C.c_void_p, C.c_uint32] * 4 + [C.c_void_p, C.c_void_p]),
    "blok_hip_denoise_posed_ref_device": (C.c_int, [C.c_void_p, C.POINTER(GBufferRef), C.POINTER(C.c_float), C.c_uint32, C.c_void_p, C.c_void_p] +
                                          [C.c_void_p, C.c_uint32] * 4 + [C.c_void_p, C.c_void_p]),
    "blok_hip_draw_frame_rt_posed_motion": (C.c_int, [C.c_void_p, C.c_void_p, C.c_uint32, C.c_uint32, C.c_void_p, C.c_void_p, C.c_uint32, C.c_void_p,
                                                      C.c_uint32, C.c_void_p, C.POINTER(C.c_uint32)]),
    "blok_hip_debug_pose_motion_records": (C.c_int, [C.c_void_p, C.c_void_p, C.c_uint32, C.c_void_p, C.c_uint32, C.c_void_p]),
    "blok_hip_volume_refresh_counts": (C.c_int, [C.c_void_p, C.POINTER(C.c_uint64)]),
    "blok_hip_volume_flood_counters": (C.c_int, [C.c_void_p, C.POINTER(C.c_uint64)]),
    "blok_hip_debug_build_pose_tlas": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint32, C.c_void_p, C.c_size_t, C.POINTER(C.c_uint32)]),
    "blok_hip_set_pose_tlas": (C.c_int, [C.c_void_p, C.c_int]),
    "blok_hip_debug_build_tlas": (C.c_int, [C.c_void_p, C.c_void_p, C.c_uint32, C.c_void_p, C.c_size_t, C.POINTER(C.c_uint32)]),
}


def _load(path: Path, symbols: dict) -> C.CDLL:
    if not path.exists():
        raise BlokLibraryError(
            f"{path.name} is not built (expected at {path}); run `python -c 'import __graft_entry__ as g; g.build()'`")
    try:
        lib = C.CDLL(os.fspath(path))
    except OSError as e:  # e.g. libamdhip64 missing
        raise BlokLibraryError(f"cannot load {path}: {e}") from e
    for name, (res, args) in symbols.items():
        try:
            fn = getattr(lib, name)
        except AttributeError as e:
            if "BLOK_HIP_LIB" in os.environ and path == HIP_LIB:      # an A/B build of another revision (scripts/build_variant.sh): bind what it has
                continue
            raise BlokLibraryError(f"{path.name} does not export {name}") from e
        fn.restype = res
        fn.argtypes = args
    return lib


_host = None
_hip = None


def host_lib() -> C.CDLL:
    global _host
    if _host is None:
        _host = _load(HOST_LIB, HOST_SYMBOLS)
    return _host


def hip_lib() -> C.CDLL:
    global _hip
    if _hip is None:
        # PyTorch ships its own libamdhip64; if this library pulled in /opt/rocm's copy first, torch would later
        # bind to that one and report no device.  Loading torch first makes both share torch's runtime.
        try:
            import torch  # noqa: F401
        except ImportError:
            pass
        _hip = _load(HIP_LIB, HIP_SYMBOLS)
    return _hip


def ptr(a: np.ndarray) -> C.c_void_p:
    return C.c_void_p(a.ctypes.data)


def as_array(address: int, count: int, dtype: np.dtype) -> np.ndarray:
    """Copy `count` records of `dtype` from a C pointer into a fresh numpy array."""
    if count == 0 or not address:
        return np.zeros(0, dtype=dtype)
    buf = (C.c_char * (count * dtype.itemsize)).from_address(address)
    return np.frombuffer(buf, dtype=dtype, count=count).copy()
