"""HipTracer — host-side mirror of the reference's compute backend class (blok::CudaTracer,
reference blok/include/cuda_tracer.hpp:23-58) over the C ABI in include/blok_hip.h.

Lifecycle follows the reference: ``HipTracer(w, h)`` → ``init()`` → ``add_world()``
(= Renderer::addWorld, reference blok/include/renderer.hpp:40-54) → ``draw_frame(cam)`` per frame →
``resize`` / ``shutdown``.  ``begin_frame`` / ``end_frame`` are no-ops as in the reference
(cuda_tracer.cu:450-456).  Errors raise ``BlokError`` (the reference throws std::runtime_error).
There is no CPU path: constructing or tracing without libblok_hip.so and a gfx950 device raises.
"""
from __future__ import annotations

import ctypes as C

import numpy as np

from . import _ffi
from ._ffi import BlokError, CAMERA, GBuffer, HIT, INSTANCE, MATERIAL, POSE, RAY, SUB_CHUNK, SVO_NODE, WorldStats


def _vec3(v):
    """Three world coordinates as the C ABI takes them; None passes through (a null pointer)."""
    return None if v is None else (C.c_int32 * 3)(*[int(c) for c in v])


class HipTracer:
    def __init__(self, width: int, height: int, device: int = 0):
        self.width, self.height, self.device = int(width), int(height), int(device)
        self._lib = None
        self._ctx = None
        self._beam_tile = 32

    # -- lifecycle -------------------------------------------------------------------------
    def init(self) -> "HipTracer":
        self._lib = _ffi.hip_lib()
        ctx = C.c_void_p()
        rc = self._lib.blok_hip_create(C.byref(ctx), self.device, self.width, self.height)
        if rc != 0:
            raise BlokError(rc, self._lib.blok_hip_last_error(None).decode())
        self._ctx = ctx
        return self

    def shutdown(self):
        if self._ctx:
            self._lib.blok_hip_destroy(self._ctx)
            self._ctx = None

    def __del__(self):
        try:
            self.shutdown()
        except Exception:
            pass

    def begin_frame(self):
        pass

    def end_frame(self):
        pass

    def resize(self, width: int, height: int):
        self._check(self._lib.blok_hip_resize(self._ctx, width, height))
        self.width, self.height = int(width), int(height)

    # -- device-resident dense store: edits and rebuilds without leaving HBM ----------------
    def _paged(self, fn, out, first, page, *lead, probe=True):
        """Fills `out` from a ranged *_download entry fn(ctx, *lead, out, first, count), `page` elements a call; probe: an empty `out`
        still makes one call with no array, which checks the snapshot and `first`."""
        if probe and len(out) == 0:
            self._check(fn(self._ctx, *lead, None, int(first), 0))
        for at in range(0, len(out), int(page)):
            n = min(int(page), len(out) - at)
            self._check(fn(self._ctx, *lead, _ffi.ptr(out[at:at + n]), int(first) + at, n))
        return out

    def _field_download(self, info_fn, fn, first, count, page):
        """Cells [first, first + count) of a field snapshot in region index order, or with both None the whole field shaped [z][y][x]."""
        if first is None and count is None:
            ext = [int(e) for e in info_fn()["ext"][0]]
            return self._paged(fn, np.zeros(ext[0] * ext[1] * ext[2], dtype=np.uint16), 0, page).reshape(ext[2], ext[1], ext[0])
        return self._paged(fn, np.zeros(int(count or 0), dtype=np.uint16), int(first or 0), page)

    def volume_create(self, origin, shape_xyz, chunk_size: int = 128, voxel_size: float = 1.0):
        o = (C.c_int32 * 3)(*[int(v) for v in origin])
        self._check(self._lib.blok_hip_volume_create(self._ctx, o, int(shape_xyz[0]), int(shape_xyz[1]), int(shape_xyz[2]),
                                                     int(chunk_size), float(voxel_size)))
        self._volume_shape = (int(shape_xyz[2]), int(shape_xyz[1]), int(shape_xyz[0]))        # arrays are [z][y][x]

    def set_volume_layout(self, keyed: bool):
        """Diagnostic (blok_hip.h): whether the next volume_create may use the keyed brick layout (default) or the row-major one."""
        self._check(self._lib.blok_hip_set_volume_layout(self._ctx, 1 if keyed else 0))

    def volume_refresh_counts(self):
        """Diagnostic (blok_hip_debug.h): mask refreshes since volume_create as (keyed edit path, keyed upload path, general layout)."""
        out = (C.c_uint64 * 3)()
        self._check(self._lib.blok_hip_volume_refresh_counts(self._ctx, out))
        return tuple(int(v) for v in out)

    def volume_destroy(self):
        self._check(self._lib.blok_hip_volume_destroy(self._ctx))

    def volume_upload(self, density=None, material_ids=None):
        d = None if density is None else np.ascontiguousarray(density, dtype=np.float32)
        m = None if material_ids is None else np.ascontiguousarray(material_ids, dtype=np.uint32)
        for a in (d, m):
            assert a is None or a.shape == self._volume_shape, "arrays are [z][y][x] over the whole box"
        self._check(self._lib.blok_hip_volume_upload(self._ctx, None if d is None else _ffi.ptr(d), None if m is None else _ffi.ptr(m)))

    def volume_download(self):
        d = np.zeros(self._volume_shape, dtype=np.float32)
        m = np.zeros(self._volume_shape, dtype=np.uint32)
        self._check(self._lib.blok_hip_volume_download(self._ctx, _ffi.ptr(d), _ffi.ptr(m)))
        return d, m

    def volume_set_voxels(self, xyz, material_ids=None, density=None):
        xyz = np.ascontiguousarray(xyz, dtype=np.int32).reshape(-1, 3)
        m = None if material_ids is None else np.ascontiguousarray(material_ids, dtype=np.uint32)
        d = None if density is None else np.ascontiguousarray(density, dtype=np.float32)
        self._check(self._lib.blok_hip_volume_set_voxels(self._ctx, _ffi.ptr(xyz), None if m is None else _ffi.ptr(m),
                                                         None if d is None else _ffi.ptr(d), len(xyz)))

    def volume_apply_brush(self, center, radius: float, value: float, mode: int):
        c = (C.c_float * 3)(*[float(v) for v in center])
        self._check(self._lib.blok_hip_volume_apply_brush(self._ctx, c, float(radius), float(value), int(mode)))

    def volume_voxelize_mesh(self, positions, triangles, materials=None, material: int = 1, density: float = 1.0, solid: bool = False) -> int:
        """Voxelize a triangle mesh into the resident volume (blok_hip.h: blok_hip_volume_voxelize_mesh): positions (n, 3) float32 in world
        units, triangles (m, 3) vertex indices, materials (m,) per-triangle ids or None (then `material`).  Returns the voxels written."""
        pos = np.ascontiguousarray(positions, dtype=np.float32).reshape(-1, 3)
        tri = np.ascontiguousarray(triangles, dtype=np.uint32).reshape(-1, 3)
        mats = None if materials is None else np.ascontiguousarray(materials, dtype=np.uint32).reshape(-1)
        if mats is not None and len(mats) != len(tri):
            raise ValueError(f"one material id per triangle: {len(mats)} ids for {len(tri)} triangles")
        n = C.c_uint64(0)
        self._check(self._lib.blok_hip_volume_voxelize_mesh(self._ctx, _ffi.ptr(pos) if len(pos) else None, len(pos), _ffi.ptr(tri) if len(tri) else None, len(tri),
                                                            None if mats is None else _ffi.ptr(mats), int(material), float(density), 1 if solid else 0,
                                                            C.byref(n)))
        return int(n.value)

    def volume_generate_terrain(self, params, region_lo=None, region_hi=None) -> int:
        """Procedural terrain into the resident volume (blok_hip.h: blok_hip_volume_generate_terrain): params a blok_amd.terrain.TerrainParams,
        the region in world voxels, half-open (both None = the whole box).  Returns the filled voxels written."""
        lo = _vec3(region_lo)
        hi = _vec3(region_hi)
        n = C.c_uint64(0)
        self._check(self._lib.blok_hip_volume_generate_terrain(self._ctx, C.byref(params), lo, hi, C.byref(n)))
        return int(n.value)

    def volume_extract_quads(self, lo=None, hi=None, ignore_material: bool = False, count_only: bool = False, page: int = 1 << 22):
        """The volume's surface as merged quads (blok_hip.h: blok_hip_volume_extract_quads): the region in world voxels, half-open (both
        None = the whole box).  Returns the records as a structured array of _ffi.QUAD in canonical order, fetched `page` records at a
        time; with count_only the pair (n_quads, n_faces) and nothing is kept."""
        rlo = _vec3(lo)
        rhi = _vec3(hi)
        flags = (_ffi.QUADS_IGNORE_MATERIAL if ignore_material else 0) | (_ffi.QUADS_COUNT_ONLY if count_only else 0)
        n_quads, n_faces = C.c_uint64(0), C.c_uint64(0)
        self._check(self._lib.blok_hip_volume_extract_quads(self._ctx, rlo, rhi, flags, C.byref(n_quads), C.byref(n_faces)))
        self.last_quad_faces = int(n_faces.value)
        if count_only:
            return int(n_quads.value), int(n_faces.value)
        return self.volume_quads_download(0, int(n_quads.value), page)

    def volume_quads_download(self, first: int, count: int, page: int = 1 << 22) -> np.ndarray:
        """Records [first, first + count) of the last extraction's snapshot."""
        return self._paged(self._lib.blok_hip_volume_quads_download, np.zeros(int(count), dtype=_ffi.QUAD), first, page)

    def volume_stamp_models(self, placements, mode: int = _ffi.STAMP_SET, density: float = 1.0) -> int:
        """Stamps placed models into the resident volume (blok_hip.h: blok_hip_volume_stamp_models): placements are INSTANCE records
        (blok_amd.stamp.placement), applied in table order; mode _ffi.STAMP_SET / STAMP_KEEP / STAMP_ERASE.  Returns the voxels written.
        The next volume_rebuild installs the world."""
        inst = np.ascontiguousarray(placements, dtype=INSTANCE).reshape(-1)
        n = C.c_uint64(0)
        self._check(self._lib.blok_hip_volume_stamp_models(self._ctx, _ffi.ptr(inst) if len(inst) else None, len(inst), int(mode), float(density), C.byref(n)))
        return int(n.value)

    def volume_stamp_affine(self, records, lo=None, hi=None, mode: int = _ffi.STAMP_SET, density: float = 1.0) -> int:
        """Resamples models into the resident volume through affine maps (blok_hip.h: blok_hip_volume_stamp_affine): records are _ffi.AFFINE
        records (blok_amd.affine: from_instance, from_matrix, rotation), applied in table order to the region (world voxels, half open;
        both None = the whole box); mode _ffi.STAMP_SET / STAMP_KEEP / STAMP_ERASE.  A model of any scale exponent is taken: the record
        carries all scale.  Returns the cells written.  The next volume_rebuild installs the world."""
        table = np.ascontiguousarray(records, dtype=_ffi.AFFINE).reshape(-1)
        n = C.c_uint64(0)
        self._check(self._lib.blok_hip_volume_stamp_affine(self._ctx, _ffi.ptr(table) if len(table) else None, len(table), _vec3(lo), _vec3(hi), int(mode),
                                                           float(density), C.byref(n)))
        return int(n.value)

    def volume_apply_shapes(self, shapes) -> int:
        """Applies a table of shapes to the resident volume in one pass (blok_hip.h: blok_hip_volume_apply_shapes): shapes are _ffi.SHAPE
        records (blok_amd.shapes: box, sphere, ellipsoid, capsule, cylinder, stroke), each with its own operation; the result is the table
        applied in order.  Returns the number of writes.  The next volume_rebuild installs the world."""
        table = np.ascontiguousarray(shapes, dtype=_ffi.SHAPE).reshape(-1)
        n = C.c_uint64(0)
        self._check(self._lib.blok_hip_volume_apply_shapes(self._ctx, _ffi.ptr(table) if len(table) else None, len(table), C.byref(n)))
        return int(n.value)

    def volume_capture_model(self, lo=None, hi=None, cut: bool = False) -> int:
        """A region of the resident volume (world voxels, half open; both None = the whole box) as a new model, in the lattice whose voxel
        (0, 0, 0) is the region's corner (blok_hip.h: blok_hip_volume_capture_model); cut = also clear the captured voxels.  Returns the
        model id; the model's voxel count is in last_capture_voxels."""
        rlo = _vec3(lo)
        rhi = _vec3(hi)
        model, n = C.c_uint32(0), C.c_uint64(0)
        self._check(self._lib.blok_hip_volume_capture_model(self._ctx, rlo, rhi, _ffi.CAPTURE_CUT if cut else 0, C.byref(model), C.byref(n)))
        self.last_capture_voxels = int(n.value)
        return int(model.value)

    def volume_label_components(self, lo=None, hi=None):
        """Labels the connected components (6-neighbour) of a region of the resident volume (blok_hip.h: blok_hip_volume_label_components):
        the region in world voxels, half open (both None = the whole box).  The snapshot stays on the device until the next labelling;
        volume_labels_download / volume_components_download fetch it.  Returns (n_components, n_voxels)."""
        rlo = _vec3(lo)
        rhi = _vec3(hi)
        n_components, n_voxels = C.c_uint64(0), C.c_uint64(0)
        self._check(self._lib.blok_hip_volume_label_components(self._ctx, rlo, rhi, 0, C.byref(n_components), C.byref(n_voxels)))
        return int(n_components.value), int(n_voxels.value)

    def volume_components_download(self, first: int, count: int, page: int = 1 << 22) -> np.ndarray:
        """Records [first, first + count) of the last labelling's snapshot: a structured array of _ffi.COMPONENT, sorted by label."""
        return self._paged(self._lib.blok_hip_volume_components_download, np.zeros(int(count), dtype=_ffi.COMPONENT), first, page)

    def volume_labels_download(self, first: int, count: int, page: int = 1 << 24) -> np.ndarray:
        """Cells [first, first + count) of the last labelling's label array (region index order; _ffi.LABEL_EMPTY = empty cell)."""
        return self._paged(self._lib.blok_hip_volume_labels_download, np.zeros(int(count), dtype=np.uint32), first, page)

    def volume_capture_component(self, label: int, cut: bool = False):
        """The voxels of the snapshot's component `label` that are still filled, as a new model in the lattice whose voxel (0, 0, 0) is the
        record's lo (blok_hip.h: blok_hip_volume_capture_component); cut = also clear them in the volume.  Returns (model id, origin):
        an instance {model, offset = origin, identity} shows the piece where it was.  The voxel count is in last_capture_voxels."""
        model, n = C.c_uint32(0), C.c_uint64(0)
        origin = (C.c_int32 * 3)(0, 0, 0)
        self.last_capture_voxels = 0
        self._check(self._lib.blok_hip_volume_capture_component(self._ctx, int(label), _ffi.COMPONENT_CUT if cut else 0, C.byref(model), origin,
                                                                C.byref(n)))
        self.last_capture_voxels = int(n.value)
        return int(model.value), (int(origin[0]), int(origin[1]), int(origin[2]))

    def volume_sweep_models(self, placements, direction: int, max_distance: int, flags: int = 0) -> np.ndarray:
        """Sweeps placed models against the resident volume (blok_hip.h: blok_hip_volume_sweep_models): for each INSTANCE record
        (blok_amd.stamp.placement) how many of the model's voxels land on filled cells and how far the model can travel along
        `direction` (0 +X, 1 -X, 2 +Y, 3 -Y, 4 +Z, 5 -Z) before one does, at most max_distance; flags _ffi.SWEEP_BOX_IS_SOLID.  Each
        placement on its own, the volume unchanged.  Returns a structured array of _ffi.SWEEP_RESULT, one per placement."""
        inst = np.ascontiguousarray(placements, dtype=INSTANCE).reshape(-1)
        out = np.zeros(len(inst), dtype=_ffi.SWEEP_RESULT)
        self._check(self._lib.blok_hip_volume_sweep_models(self._ctx, _ffi.ptr(inst) if len(inst) else None, len(inst), int(direction),
                                                           int(max_distance), int(flags), _ffi.ptr(out) if len(out) else None))
        return out

    def volume_encode_bricks(self, lo=None, hi=None, filled_only: bool = False) -> np.ndarray:
        """Encodes a region of the resident volume (world voxels, half open; both None = the whole box) as a sparse brick stream kept on
        the device (blok_hip.h: blok_hip_volume_encode_bricks) until the next encode.  Returns the stream's info, one _ffi.BRICKS_INFO
        record; volume_bricks_download fetches the stream, volume_restore_bricks writes it back."""
        rlo = _vec3(lo)
        rhi = _vec3(hi)
        info = np.zeros(1, dtype=_ffi.BRICKS_INFO)
        self._check(self._lib.blok_hip_volume_encode_bricks(self._ctx, rlo, rhi, _ffi.BRICKS_FILLED_ONLY if filled_only else 0, _ffi.ptr(info)))
        return info

    def volume_bricks_info(self) -> np.ndarray:
        info = np.zeros(1, dtype=_ffi.BRICKS_INFO)
        self._check(self._lib.blok_hip_volume_bricks_info(self._ctx, _ffi.ptr(info)))
        return info

    def volume_bricks_download(self, page: int = 1 << 22):
        """The last encode's stream as (info, records, density payload, material payload): _ffi.BRICKS_INFO, a structured array of
        _ffi.BRICK_RECORD and two uint32 arrays (bit patterns and ids), fetched `page` entries at a time."""
        info = self.volume_bricks_info()
        records = self._paged(self._lib.blok_hip_volume_bricks_download, np.zeros(int(info["n_bricks"][0]), dtype=_ffi.BRICK_RECORD), 0, page, probe=False)
        payloads = [self._paged(self._lib.blok_hip_volume_brick_payload_download, np.zeros(int(info[key][0]), dtype=np.uint32), 0, page, plane, probe=False)
                    for plane, key in ((0, "n_density"), (1, "n_material"))]
        return info, records, payloads[0], payloads[1]

    def volume_restore_bricks(self, dst_lo=None, keep_others: bool = False):
        """Writes the last encode's stream back into the volume at dst_lo (None = where it was taken): undo, or copy and paste.  By default
        every cell of the destination is written; keep_others writes the stored cells only.  The next volume_rebuild installs the world."""
        dlo = _vec3(dst_lo)
        self._check(self._lib.blok_hip_volume_restore_bricks(self._ctx, dlo, _ffi.BRICKS_KEEP_OTHERS if keep_others else 0))

    def volume_decode_bricks(self, info, records, density_payload, material_payload, dst_lo=None, keep_others: bool = False):
        """volume_restore_bricks from host arrays (a loaded file, the host build's stream); the stream is validated first."""
        info = np.ascontiguousarray(info, dtype=_ffi.BRICKS_INFO).reshape(1)
        records = np.ascontiguousarray(records, dtype=_ffi.BRICK_RECORD).reshape(-1)
        dp = np.ascontiguousarray(density_payload, dtype=np.uint32).reshape(-1)
        mp = np.ascontiguousarray(material_payload, dtype=np.uint32).reshape(-1)
        dlo = _vec3(dst_lo)
        self._check(self._lib.blok_hip_volume_decode_bricks(self._ctx, _ffi.ptr(info), _ffi.ptr(records) if len(records) else None,
                                                            _ffi.ptr(dp) if len(dp) else None, _ffi.ptr(mp) if len(mp) else None, dlo,
                                                            _ffi.BRICKS_KEEP_OTHERS if keep_others else 0))

    def volume_distance_field(self, lo=None, hi=None, max_radius: int = 0, to_empty: bool = False, box_is_solid: bool = False) -> np.ndarray:
        """Takes the capped squared distance field of a region of the resident volume (world voxels, half open; both None = the whole box)
        to the nearest filled cell — to_empty: to the nearest empty cell; box_is_solid: the outside of the box counts as filled — and keeps
        it on the device (blok_hip.h: blok_hip_volume_distance_field) until the next field.  Returns the field's info, one
        _ffi.DISTANCE_INFO record; volume_distance_download fetches the values, volume_edit_by_distance thresholds them."""
        rlo = _vec3(lo)
        rhi = _vec3(hi)
        flags = (_ffi.DISTANCE_TO_EMPTY if to_empty else 0) | (_ffi.DISTANCE_BOX_IS_SOLID if box_is_solid else 0)
        info = np.zeros(1, dtype=_ffi.DISTANCE_INFO)
        self._check(self._lib.blok_hip_volume_distance_field(self._ctx, rlo, rhi, int(max_radius), flags, _ffi.ptr(info)))
        return info

    def volume_distance_info(self) -> np.ndarray:
        info = np.zeros(1, dtype=_ffi.DISTANCE_INFO)
        self._check(self._lib.blok_hip_volume_distance_info(self._ctx, _ffi.ptr(info)))
        return info

    def volume_distance_download(self, first=None, count=None, page: int = 1 << 24) -> np.ndarray:
        """The last field's values (uint16, _ffi.DISTANCE_FAR = no source within the radius), fetched `page` cells at a time: cells
        [first, first + count) in region index order, or with both None the whole field shaped [z][y][x]."""
        return self._field_download(self.volume_distance_info, self._lib.blok_hip_volume_distance_download, first, count, page)

    def volume_edit_by_distance(self, op: int, d2: int, density: float = 1.0, material: int = 0) -> int:
        """Thresholds the last field at the squared distance d2 over its region (blok_hip.h: blok_hip_volume_edit_by_distance): op
        _ffi.DISTANCE_GROW fills the empty cells within d2 of a filled one with (density, material), DISTANCE_SHRINK clears the filled
        cells within d2 of an empty one, DISTANCE_HOLLOW clears the filled cells farther than d2 from every empty one.  Returns the number
        of cells written; the next volume_rebuild installs the world."""
        n = C.c_uint64(0)
        self._check(self._lib.blok_hip_volume_edit_by_distance(self._ctx, int(op), int(d2), float(density), int(material), C.byref(n)))
        return int(n.value)

    def volume_flood_field(self, lo=None, hi=None, seeds=None, max_steps: int = _ffi.FLOOD_MAX_STEPS, flags: int = 0, material: int = 0) -> np.ndarray:
        """Floods a region of the resident volume (world voxels, half open; both None = the whole box) from the world cells `seeds`
        ([n][3]) and, with flag bits _ffi.flood_seed_face(f), from the passable cells of the region's side f, through the empty cells —
        _ffi.FLOOD_THROUGH_FILLED: through the filled ones, with _ffi.FLOOD_SAME_MATERIAL only those whose id is `material` — and keeps
        the least number of 6-neighbour steps to every cell, capped at max_steps, on the device (blok_hip.h: blok_hip_volume_flood_field)
        until the next flood.  Returns the field's info, one _ffi.FLOOD_INFO record; volume_flood_download fetches the values,
        volume_edit_by_flood thresholds them."""
        rlo = _vec3(lo)
        rhi = _vec3(hi)
        xyz = np.zeros((0, 3), np.int32) if seeds is None else np.ascontiguousarray(seeds, dtype=np.int32).reshape(-1, 3)
        info = np.zeros(1, dtype=_ffi.FLOOD_INFO)
        self._check(self._lib.blok_hip_volume_flood_field(self._ctx, rlo, rhi, _ffi.ptr(xyz) if len(xyz) else None, len(xyz), int(max_steps), int(flags),
                                                          int(material), _ffi.ptr(info)))
        return info

    def volume_flood_info(self) -> np.ndarray:
        info = np.zeros(1, dtype=_ffi.FLOOD_INFO)
        self._check(self._lib.blok_hip_volume_flood_info(self._ctx, _ffi.ptr(info)))
        return info

    def volume_flood_counters(self):
        """Diagnostic (blok_hip_debug.h): (rounds run, bricks taken off the lists) of the last flood.  Scheduling-dependent."""
        out = (C.c_uint64 * 2)()
        self._check(self._lib.blok_hip_volume_flood_counters(self._ctx, out))
        return int(out[0]), int(out[1])

    def volume_flood_download(self, first=None, count=None, page: int = 1 << 24) -> np.ndarray:
        """The last flood's values (uint16, _ffi.FLOOD_FAR = not reached or impassable), fetched `page` cells at a time: cells
        [first, first + count) in region index order, or with both None the whole field shaped [z][y][x]."""
        return self._field_download(self.volume_flood_info, self._lib.blok_hip_volume_flood_download, first, count, page)

    def volume_edit_by_flood(self, op: int, d: int = 0, density: float = 1.0, material: int = 0) -> int:
        """Thresholds the last flood at d steps over its region (blok_hip.h: blok_hip_volume_edit_by_flood): op _ffi.FLOOD_FILL fills the
        empty cells within d steps with (density, material), FLOOD_FILL_UNREACHED the empty cells the flood did not reach, FLOOD_PAINT
        gives the filled cells within d steps the id `material`, FLOOD_CLEAR clears them.  Returns the number of cells written; the next
        volume_rebuild installs the world."""
        n = C.c_uint64(0)
        self._check(self._lib.blok_hip_volume_edit_by_flood(self._ctx, int(op), int(d), float(density), int(material), C.byref(n)))
        return int(n.value)

    def volume_column_field(self, lo=None, hi=None, axis: int = 1, flags: int = 0) -> np.ndarray:
        """Takes the column field of a region of the resident volume (world voxels, half open; both None = the whole box) along `axis`:
        per column the first filled cell met from the hi face (_ffi.COLUMNS_FROM_LOW: from the lo face), region-local, and its material id
        (blok_hip.h: blok_hip_volume_column_field), kept on the device until the next field.  Returns the field's info, one
        _ffi.COLUMNS_INFO record; volume_columns_download fetches the planes, volume_scatter_models places models on it."""
        rlo = _vec3(lo)
        rhi = _vec3(hi)
        info = np.zeros(1, dtype=_ffi.COLUMNS_INFO)
        self._check(self._lib.blok_hip_volume_column_field(self._ctx, rlo, rhi, int(axis), int(flags), _ffi.ptr(info)))
        return info

    def volume_columns_info(self) -> np.ndarray:
        info = np.zeros(1, dtype=_ffi.COLUMNS_INFO)
        self._check(self._lib.blok_hip_volume_columns_info(self._ctx, _ffi.ptr(info)))
        return info

    def volume_columns_download(self, plane: int = 0, first=None, count=None, page: int = 1 << 24) -> np.ndarray:
        """A plane of the last column field — 0: the tops (uint16, _ffi.COLUMNS_NONE = no filled cell), 1: the material ids (uint32) —
        fetched `page` columns at a time: columns [first, first + count), or with both None all of them."""
        dtype = np.uint32 if int(plane) == 1 else np.uint16
        if first is None and count is None:
            first, count = 0, int(self.volume_columns_info()["n_columns"][0])
        return self._paged(self._lib.blok_hip_volume_columns_download, np.zeros(int(count or 0), dtype=dtype), int(first or 0), page, int(plane))

    def volume_scatter_models(self, params, entries) -> np.ndarray:
        """Scatters models over the last column field, which must run along +y from the top (blok_hip.h: blok_hip_volume_scatter_models):
        params one _ffi.SCATTER_PARAMS record, entries _ffi.SCATTER_ENTRY records (blok_amd.columns builds both).  The table stays on the
        device until the next scatter or column field.  Returns the counts, one _ffi.SCATTER_INFO record."""
        params = np.ascontiguousarray(params, dtype=_ffi.SCATTER_PARAMS).reshape(1)
        entries = np.ascontiguousarray(entries, dtype=_ffi.SCATTER_ENTRY).reshape(-1)
        info = np.zeros(1, dtype=_ffi.SCATTER_INFO)
        self._check(self._lib.blok_hip_volume_scatter_models(self._ctx, _ffi.ptr(params), _ffi.ptr(entries) if len(entries) else None, len(entries),
                                                             _ffi.ptr(info)))
        return info

    def volume_scroll(self, delta, plan_only: bool = False) -> np.ndarray:
        """Moves the resident volume's box through the world by `delta` voxels, each a multiple of 4 (blok_hip.h: blok_hip_volume_scroll):
        the world voxels that stay inside keep their values, the cells that come into view are empty.  Returns one _ffi.SCROLL_INFO record:
        the new origin, the exposed boxes (the caller's to fill) and the leaving ones, and the counts.  plan_only fills the same record
        and changes nothing; (0, 0, 0) says where the box is.  The next volume_rebuild installs the world."""
        info = np.zeros(1, dtype=_ffi.SCROLL_INFO)
        self._check(self._lib.blok_hip_volume_scroll(self._ctx, _vec3(delta), _ffi.SCROLL_PLAN_ONLY if plan_only else 0, _ffi.ptr(info)))
        return info

    def volume_scatter_info(self) -> np.ndarray:
        info = np.zeros(1, dtype=_ffi.SCATTER_INFO)
        self._check(self._lib.blok_hip_volume_scatter_info(self._ctx, _ffi.ptr(info)))
        return info

    def volume_scatter_download(self, first=None, count=None, page: int = 1 << 22) -> np.ndarray:
        """Records [first, first + count) of the last scatter's table (INSTANCE, sorted by column), or with both None the whole table."""
        if first is None and count is None:
            first, count = 0, int(self.volume_scatter_info()["n_placed"][0])
        return self._paged(self._lib.blok_hip_volume_scatter_download, np.zeros(int(count or 0), dtype=INSTANCE), int(first or 0), page)

    def volume_scatter_device(self):
        """(device address, count) of the last scatter's table where it lies, for the *_instanced_device entries (which skip instances that
        fail their limits: check a downloaded table with check_instances).  Valid until the next scatter, column field or volume."""
        table, n = C.c_void_p(0), C.c_uint64(0)
        self._check(self._lib.blok_hip_volume_scatter_device(self._ctx, C.byref(table), C.byref(n)))
        return int(table.value or 0), int(n.value)

    def volume_reduce(self, lo=None, hi=None, levels: int = 1, flags: int = 0) -> np.ndarray:
        """Reduces a region of the resident volume (world voxels, half open; both None = the whole box) to `levels` coarser levels, each
        cell of level j holding the counts of filled and of exposed voxels of its 2^j cube and a voted material id (blok_hip.h:
        blok_hip_volume_reduce; flags: _ffi.LOD_VOTE_EXPOSED), kept on the device until the next reduce.  Returns the info, one
        _ffi.LOD_INFO record; volume_lod_download fetches the planes, volume_lod_model makes a level a model."""
        info = np.zeros(1, dtype=_ffi.LOD_INFO)
        self._check(self._lib.blok_hip_volume_reduce(self._ctx, _vec3(lo), _vec3(hi), int(levels), int(flags), _ffi.ptr(info)))
        return info

    def terrain_reduce(self, params, lo, hi, levels: int = 1, flags: int = 0) -> np.ndarray:
        """Reduces the terrain function (params a blok_amd.terrain.TerrainParams with flags 0) over the world region [lo, hi) to `levels`
        coarser levels without a volume (blok_hip.h: blok_hip_terrain_reduce; flags: _ffi.LOD_VOTE_EXPOSED, _ffi.LOD_SEAMLESS).  Fills the
        snapshot volume_reduce fills: volume_lod_info, volume_lod_download and volume_lod_model work behind it.  Returns the info."""
        info = np.zeros(1, dtype=_ffi.LOD_INFO)
        self._check(self._lib.blok_hip_terrain_reduce(self._ctx, C.byref(params), _vec3(lo), _vec3(hi), int(levels), int(flags), _ffi.ptr(info)))
        return info

    def volume_automaton(self, rule, lo=None, hi=None):
        """Steps a neighbour-count rule (one _ffi.AUTOMATON_RULE record; blok_amd.automaton makes them) over a region of the resident
        volume (world voxels, half open; both None = the whole box), in place (blok_hip.h: blok_hip_volume_automaton).  Returns (info,
        step_counts): one _ffi.AUTOMATON_INFO record, and a [steps][2] uint64 array of the cells born and died per step, zero past
        info["steps_run"]; the next volume_rebuild installs the world."""
        rule = np.ascontiguousarray(rule, dtype=_ffi.AUTOMATON_RULE).reshape(1)
        info = np.zeros(1, dtype=_ffi.AUTOMATON_INFO)
        counts = np.zeros((max(int(rule["steps"][0]), 1), 2), dtype=np.uint64)
        self._check(self._lib.blok_hip_volume_automaton(self._ctx, _vec3(lo), _vec3(hi), _ffi.ptr(rule), _ffi.ptr(counts), _ffi.ptr(info)))
        return info, counts

    def volume_lod_info(self) -> np.ndarray:
        info = np.zeros(1, dtype=_ffi.LOD_INFO)
        self._check(self._lib.blok_hip_volume_lod_info(self._ctx, _ffi.ptr(info)))
        return info

    def volume_lod_download(self, level: int, plane: int = 0, first=None, count=None, page: int = 1 << 24) -> np.ndarray:
        """A plane of a level (1-based) of the last reduce — 0: n (uint16), 1: e (uint16), 2: the ids (uint32) — fetched `page` cells at a
        time: cells [first, first + count) in index order, or with both None the whole plane shaped [z][y][x]."""
        dtype = np.uint32 if int(plane) == 2 else np.uint16
        if first is None and count is None:
            cext = [int(c) for c in self.volume_lod_info()["level"][0][max(int(level), 1) - 1]["cext"]] if 1 <= int(level) <= _ffi.LOD_MAX_LEVELS else [0, 0, 0]
            out = self._paged(self._lib.blok_hip_volume_lod_download, np.zeros(cext[0] * cext[1] * cext[2], dtype=dtype), 0, page, int(level), int(plane))
            return out.reshape(cext[2], cext[1], cext[0])
        return self._paged(self._lib.blok_hip_volume_lod_download, np.zeros(int(count or 0), dtype=dtype), int(first or 0), page, int(level), int(plane))

    def volume_lod_model(self, level: int, min_count: int = 1) -> int:
        """The cells of a level of the last reduce with n >= min_count as a new model, in the lattice whose voxel (0, 0, 0) is the level's
        first cell, each voxel's material the cell's voted id (blok_hip.h: blok_hip_volume_lod_model).  Returns the model id; the voxel
        count is in last_capture_voxels."""
        model, n = C.c_uint32(0), C.c_uint64(0)
        self._check(self._lib.blok_hip_volume_lod_model(self._ctx, int(level), int(min_count), C.byref(model), C.byref(n)))
        self.last_capture_voxels = int(n.value)
        return int(model.value)

    def volume_rebuild(self, materials=None) -> WorldStats:
        mats = np.zeros(0, dtype=MATERIAL) if materials is None else np.ascontiguousarray(materials, dtype=MATERIAL)
        self._check(self._lib.blok_hip_volume_rebuild(self._ctx, _ffi.ptr(mats) if len(mats) else None, len(mats)))
        return self.world_stats()

    # -- image-space chain: denoiser, TAA, sharpen on device planes ----------------------------
    def denoise_settings(self) -> "_ffi.DenoiseSettings":
        s = _ffi.DenoiseSettings()
        self._lib.blok_denoise_settings_default(C.byref(s))
        return s

    def denoise_device(self, color_ptr: int, world_pos_ptr: int, normal_roughness_ptr: int, prev_view_proj, frame_count: int,
                       out_color_ptr: int, motion_ptr: int = 0, settings=None, stream: int = 0):
        """Denoiser::denoise for one frame over float4 device planes (as trace_paths_device writes them)."""
        planes = _ffi.GBuffer(color_ptr, world_pos_ptr, normal_roughness_ptr, 0)
        m = (C.c_float * 16)(*[float(v) for v in np.asarray(prev_view_proj, dtype=np.float32).reshape(-1)])
        self._check(self._lib.blok_hip_denoise_device(self._ctx, C.byref(planes), motion_ptr or None, m, int(frame_count),
                                                      C.byref(settings) if settings is not None else None, out_color_ptr,
                                                      stream or None))

    def denoise_state(self):
        """Host copies of (history colour, moments, history length, variance, motion vectors) after the last frame."""
        h, w = self.height, self.width
        out = (np.zeros((h, w, 4), np.float32), np.zeros((h, w, 2), np.float32), np.zeros((h, w), np.float32),
               np.zeros((h, w), np.float32), np.zeros((h, w, 2), np.float32))
        self._check(self._lib.blok_hip_denoise_state(self._ctx, *[_ffi.ptr(a) for a in out]))
        return out

    def taa_device(self, color_ptr: int, out_color_ptr: int, frame_count: int, feedback_min: float = 0.93, feedback_max: float = 0.98,
                   motion_ptr: int = 0, stream: int = 0):
        self._check(self._lib.blok_hip_taa_device(self._ctx, color_ptr, motion_ptr or None, feedback_min, feedback_max,
                                                  int(frame_count), out_color_ptr, stream or None))

    def sharpen_device(self, rgba8_ptr: int, out_rgba8_ptr: int, strength: float = 0.5, stream: int = 0):
        self._check(self._lib.blok_hip_sharpen_device(self._ctx, rgba8_ptr, strength, out_rgba8_ptr, stream or None))

    def draw_frame_rt(self, cam: np.ndarray, spp: int = 8, max_bounces: int = 2, settings=None):
        """Renderer::drawFrame's ray-tracing path in one call: path trace -> denoise -> TAA -> tonemap -> sharpen.
        Returns (RGBA8 (h, w) uint32, frames rendered so far)."""
        cam = np.ascontiguousarray(cam, dtype=CAMERA)
        out = np.zeros((self.height, self.width), dtype=np.uint32)
        frames = C.c_uint32()
        self._check(self._lib.blok_hip_draw_frame_rt(self._ctx, _ffi.ptr(cam), spp, max_bounces,
                                                     C.byref(settings) if settings is not None else None, _ffi.ptr(out), C.byref(frames)))
        return out, frames.value

    def camera_view_proj(self, cam: np.ndarray) -> np.ndarray:
        cam = np.ascontiguousarray(cam, dtype=CAMERA)
        m = (C.c_float * 16)()
        self._lib.blok_camera_view_proj(_ffi.ptr(cam), m)
        return np.array(m, dtype=np.float32)

    def post_reset(self):
        self._check(self._lib.blok_hip_post_reset(self._ctx))

    def set_path_start(self, resume_from_anchor=False, wave_tile_beam=True):
        """Where the path kernel's walks start (blok_hip_set_path_start): from the pixel's latest hit's ancestors, behind the wave tile's own
        beam; frames are identical in every combination."""
        self._check(self._lib.blok_hip_set_path_start(self._ctx, int(bool(resume_from_anchor)), int(bool(wave_tile_beam))))

    def set_ray_batching(self, mode):
        """Path kernel scheduling (never changes a result): 0 / False = off, 1 = one kind of ray at a time, 2 / True (default) = one
        kind at a time and the oldest sample first."""
        self._check(self._lib.blok_hip_set_ray_batching(self._ctx, 2 if mode is True else int(mode)))

    def set_sun_map(self, enabled: bool):
        """Shadow rays stop at the last occluder of their sun-direction column (never changes a result); default on."""
        self._check(self._lib.blok_hip_set_sun_map(self._ctx, int(bool(enabled))))

    def sun_map(self, want_map: bool = True):
        """Read-back of the shadow rays' last-occluder map (blok_hip_debug.h: blok_hip_sun_map_download): (info, map) with info one
        _ffi.SUN_MAP_INFO record and map the float32 texels shaped [nv][nu], or None without a map or with want_map False."""
        info = np.zeros(1, dtype=_ffi.SUN_MAP_INFO)
        self._check(self._lib.blok_hip_sun_map_download(self._ctx, _ffi.ptr(info), None, 0))
        if not want_map or not int(info["has_map"][0]):
            return info, None
        texels = np.zeros((int(info["nv"][0]), int(info["nu"][0])), dtype=np.float32)
        self._check(self._lib.blok_hip_sun_map_download(self._ctx, _ffi.ptr(info), _ffi.ptr(texels), texels.size))
        return info, texels

    def set_beam(self, beam_tile_pixels: int):
        """Beam pre-pass granularity of the frame kernels in pixels (0 = off, default 32); never changes a result."""
        self._check(self._lib.blok_hip_set_beam(self._ctx, beam_tile_pixels))
        self._beam_tile = int(beam_tile_pixels)

    def set_taa_jitter(self, jitter_px=None):
        """Sub-pixel TAA jitter (pixels, each within +-0.5) of the primary rays of all following frames; None = off."""
        if jitter_px is None:
            self._check(self._lib.blok_hip_set_taa_jitter(self._ctx, None))
        else:
            j = (C.c_float * 2)(float(jitter_px[0]), float(jitter_px[1]))
            self._check(self._lib.blok_hip_set_taa_jitter(self._ctx, j))

    def set_rt_taa_jitter(self, enabled: bool):
        """draw_frame_rt applies jitter entry (frame mod 16) by itself (default on = PostProcess::Settings::enableTAA)."""
        self._check(self._lib.blok_hip_set_rt_taa_jitter(self._ctx, 1 if enabled else 0))

    def beam_prepass(self, cam, rect=None, want_visits=False):
        """The pre-pass alone: (t0, visits) per beam tile of the rectangle, row-major (blok_hip.h: blok_hip_beam_prepass)."""
        x0, y0, w, h = rect or (0, 0, self.width, self.height)
        tile = self._beam_tile
        n = ((w + tile - 1) // tile) * ((h + tile - 1) // tile)
        t0 = np.zeros(n, dtype=np.float32)
        visits = np.zeros(n, dtype=np.uint32) if want_visits else None
        cam = np.ascontiguousarray(cam)
        self._check(self._lib.blok_hip_beam_prepass(self._ctx, C.c_void_p(cam.ctypes.data), x0, y0, w, h, C.c_void_p(t0.ctypes.data),
                                                    C.c_void_p(visits.ctypes.data) if want_visits else None, n))
        return t0, visits

    def trace_wave_tiles_device(self, cam, tiles, t0, hits_ptr=0, rgba_ptr=0, rect=None, stream=0):
        """Walks the listed 8x8-pixel wave tiles of the rectangle in list order (blok_hip.h: blok_hip_trace_wave_tiles_device)."""
        x0, y0, w, h = rect or (0, 0, self.width, self.height)
        tiles = np.ascontiguousarray(tiles, dtype=np.uint32)
        t0 = None if t0 is None else np.ascontiguousarray(t0, dtype=np.float32)
        cam = np.ascontiguousarray(cam)
        self._check(self._lib.blok_hip_trace_wave_tiles_device(self._ctx, C.c_void_p(cam.ctypes.data), x0, y0, w, h, C.c_void_p(tiles.ctypes.data),
                                                               C.c_void_p(t0.ctypes.data) if t0 is not None else None, len(tiles),
                                                               C.c_void_p(hits_ptr) if hits_ptr else None, C.c_void_p(rgba_ptr) if rgba_ptr else None,
                                                               C.c_void_p(stream) if stream else None))

    def set_debug_wave_clocks(self, dev_ptr):
        self._check(self._lib.blok_hip_set_debug_wave_clocks(self._ctx, C.c_void_p(dev_ptr) if dev_ptr else None))

    def set_tile_ordering(self, resort_every_n_frames):
        """Longest-first scheduling of the walk from earlier frames' per-wave clocks, re-sorted asynchronously every N frames
        (default 8; 0 / False = off; True = 8); applied only to launches that have the chip to themselves; never changes a result."""
        n = 8 if resort_every_n_frames is True else int(resort_every_n_frames or 0)
        self._check(self._lib.blok_hip_set_tile_ordering(self._ctx, n))

    def set_rank_tile_ordering(self, enabled: bool):
        """Longest-first order and live prefix for a rank's tile launches too (a view at rest); never changes a frame."""
        self._check(self._lib.blok_hip_set_rank_tile_ordering(self._ctx, int(bool(enabled))))

    def set_moving_order(self, enabled: bool):
        """Longest-first scheduling for a camera in motion: the previous frame's clocks, dilated, carried to this view by a whole-tile
        shift (default on; launches alone on the device only); never changes a result."""
        self._check(self._lib.blok_hip_set_moving_order(self._ctx, 1 if enabled else 0))

    def debug_class_order(self, cost, radius, beam=None):
        """Test hook: (order, rank_of, live, depth sums) of blok_hip_debug_class_order for a 2-D array of per-wave-tile costs."""
        cost = np.ascontiguousarray(cost, dtype=np.uint32)
        ty, tx = cost.shape
        order = np.zeros(tx * ty, dtype=np.uint32); rank = np.zeros(tx * ty, dtype=np.uint32)
        live = C.c_uint32(0); sums = np.zeros(3, dtype=np.float32)
        b = None if beam is None else np.ascontiguousarray(beam, dtype=np.float32)
        self._check(self._lib.blok_hip_debug_class_order(self._ctx, C.c_void_p(cost.ctypes.data), tx, ty, int(radius), C.c_void_p(b.ctypes.data) if b is not None else None,
                                                         0 if b is None else len(b), C.c_void_p(order.ctypes.data), C.c_void_p(rank.ctypes.data), C.byref(live), C.c_void_p(sums.ctypes.data)))
        return order, rank, live.value, sums

    def debug_force_order_shift(self, shift=None):
        """Test hook: every ordered launch applies this (x, y) whole-tile shift to its order; None = off."""
        self._check(self._lib.blok_hip_debug_force_order_shift(self._ctx, 0 if shift is None else 1, *(shift or (0, 0))))

    def last_fallback_tiles(self) -> int:
        """Diagnostic: wave tiles the search waves of the latest prefix launch walked themselves (after a synchronise)."""
        return int(self._lib.blok_hip_last_fallback_tiles(self._ctx))

    def last_order_use(self):
        """Diagnostic: (0 row-major | 1 order of this view | 2 order carried from another view, shift_x, shift_y) of the latest rectangle launch."""
        sx, sy = C.c_int32(0), C.c_int32(0)
        return self._lib.blok_hip_last_order_use(self._ctx, C.byref(sx), C.byref(sy)), sx.value, sy.value

    def set_joint_prefix_limit(self, max_walk_waves: int):
        """Diagnostic: cap on the walk waves of a joint launch; the rest is walked by the search waves (same frame)."""
        self._check(self._lib.blok_hip_set_joint_prefix_limit(self._ctx, max_walk_waves))

    def set_list_classes(self, enabled: bool):
        """List launches: order the walk by the previous frame's measured cost, in four classes (default on); never changes a result."""
        self._check(self._lib.blok_hip_set_list_classes(self._ctx, 1 if enabled else 0))

    def last_launch_kind(self) -> int:
        """Which kernels the latest rectangle / tile launch was issued as (blok_hip.h: blok_hip_last_launch_kind)."""
        return int(self._lib.blok_hip_last_launch_kind(self._ctx))

    def set_miss_writer(self, in_walk: bool):
        """Empty tiles' miss pixels: written by the walk launch's waves (True, default) or by the pre-pass (blok_hip.h)."""
        self._check(self._lib.blok_hip_set_miss_writer(self._ctx, 1 if in_walk else 0))

    def set_beam_cache(self, mode):
        """Keep the beam bounds of a view at rest from launch to launch (blok_hip_debug.h): 5 or True (default) = with, from the view's K-th
        hit on, a finer bound per wave tile, then its rays packed into a list, each restarted where its own counted walk ended, at the tree
        node that walk ends in; 4 = restarted there from the root; 3 = the list
        sorted by measured length and walked from the finer bounds; 2 = without the packed walk; 1 = the beam tiles' bounds alone; 0 or
        False = every launch searches.  Never changes a result."""
        self._check(self._lib.blok_hip_set_beam_cache(self._ctx, (5 if mode else 0) if isinstance(mode, bool) else int(mode)))

    def set_beam_refine_after(self, hits: int):
        """K: the hit of a kept view behind whose walk its finer bounds are searched, once (0 = the default; blok_hip_debug.h)."""
        self._check(self._lib.blok_hip_set_beam_refine_after(self._ctx, hits))

    def set_beam_list_after(self, hits: int):
        """N: the launch from the finer bounds that counts a kept view's rays for its packed list (0 = the default; blok_hip_debug.h)."""
        self._check(self._lib.blok_hip_set_beam_list_after(self._ctx, hits))

    def beam_cache_list_builds(self) -> int:
        """Diagnostic: launches so far that counted and issued the build of a view's packed list."""
        n = C.c_uint64(0)
        self._check(self._lib.blok_hip_beam_cache_list_builds(self._ctx, C.byref(n)))
        return int(n.value)

    def pack_area(self) -> int:
        """Side of the packed list's areas in pixels (blok_hip_debug.h: blok_hip_pack_area)."""
        return int(self._lib.blok_hip_pack_area())

    def beam_cache_list_state(self) -> int:
        """What the latest rectangle launch had to do with a packed list: 0 nothing, 1 it counted and issued the build, 2 it walked packed.
        Waits for nothing."""
        state = C.c_int(0)
        self._check(self._lib.blok_hip_beam_cache_download_list(self._ctx, C.byref(state), None, None, None, 0, None, 0, None, 0))
        return int(state.value)

    def beam_cache_list(self, w: int, h: int):
        """(state, n_groups, entries, table, trips) of the latest rectangle launch's packed list (blok_hip_debug.h:
        blok_hip_beam_cache_download_list), for its rectangle of w x h pixels: entries (areas, area^2) uint32, table (areas * area^2 / 64,) uint32,
        trips (h, w) uint8; None for state 0."""
        state, areas, groups = C.c_int(0), C.c_uint32(0), C.c_uint32(0)
        self._check(self._lib.blok_hip_beam_cache_download_list(self._ctx, C.byref(state), C.byref(areas), None, None, 0, None, 0, None, 0))
        if not state.value:
            return None
        stretch = self.pack_area() ** 2                  # trace_kernels.h: kPackStretch entries and kPackGroups = stretch / 64 words per area
        entries = np.zeros((int(areas.value), stretch), dtype=np.uint32)
        table = np.zeros(int(areas.value) * (stretch // 64), dtype=np.uint32)
        trips = np.zeros((h, w), dtype=np.uint8)
        self._check(self._lib.blok_hip_beam_cache_download_list(self._ctx, C.byref(state), C.byref(areas), C.byref(groups), _ffi.ptr(entries), entries.size,
                                                                 _ffi.ptr(table), table.size, _ffi.ptr(trips), trips.size))
        return int(state.value), int(groups.value), entries, table, trips

    def beam_cache_starts_state(self) -> int:
        """What the latest rectangle launch had to do with a list's starts: 0 nothing, 1 it counted them or walked from them, 2 it walked
        packed under another start key.  Waits for nothing."""
        state = C.c_int(0)
        self._check(self._lib.blok_hip_beam_cache_download_starts(self._ctx, C.byref(state), None, 0, None, 0))
        return int(state.value)

    def beam_cache_starts(self, w: int, h: int):
        """(starts, restarts) of the latest rectangle launch's packed list (blok_hip_debug.h: blok_hip_beam_cache_download_starts), for its
        rectangle of w x h pixels: starts (areas, area^2) float32 in list order, restarts (h, w) uint8."""
        state, areas = C.c_int(0), C.c_uint32(0)
        self._check(self._lib.blok_hip_beam_cache_download_list(self._ctx, C.byref(state), C.byref(areas), None, None, 0, None, 0, None, 0))
        starts = np.zeros((int(areas.value), self.pack_area() ** 2), dtype=np.float32)
        restarts = np.zeros((h, w), dtype=np.uint8)
        self._check(self._lib.blok_hip_beam_cache_download_starts(self._ctx, None, _ffi.ptr(starts), starts.size, _ffi.ptr(restarts), restarts.size))
        return starts, restarts

    def beam_cache_start_counters(self):
        """(packed launches that walked from the starts, packed launches that found another start key)."""
        used, other = C.c_uint64(0), C.c_uint64(0)
        self._check(self._lib.blok_hip_beam_cache_start_counters(self._ctx, C.byref(used), C.byref(other)))
        return int(used.value), int(other.value)

    def beam_cache_has_nodes(self) -> bool:
        """Does the latest rectangle launch's packed list carry node words (mode 5)?  Waits for nothing."""
        has = C.c_int(0)
        self._check(self._lib.blok_hip_beam_cache_download_nodes(self._ctx, C.byref(has), None, 0, None, 0))
        return bool(has.value)

    def beam_cache_nodes(self, w: int, h: int):
        """(entry words, pixel words) of the latest rectangle launch's packed list (blok_hip_debug.h: blok_hip_beam_cache_download_nodes), for its
        rectangle of w x h pixels: entry words (areas, area^2) uint32 in list order, pixel words (h, w) uint32 of the latest count launch."""
        state, areas = C.c_int(0), C.c_uint32(0)
        self._check(self._lib.blok_hip_beam_cache_download_list(self._ctx, C.byref(state), C.byref(areas), None, None, 0, None, 0, None, 0))
        entry_words = np.zeros((int(areas.value), self.pack_area() ** 2), dtype=np.uint32)
        pixel_words = np.zeros((h, w), dtype=np.uint32)
        self._check(self._lib.blok_hip_beam_cache_download_nodes(self._ctx, None, _ffi.ptr(entry_words), entry_words.size, _ffi.ptr(pixel_words), pixel_words.size))
        return entry_words, pixel_words

    def beam_cache_node_counter(self) -> int:
        """Packed launches so far that re-entered their rays at the node words (packed_frame_node_kernel)."""
        n = C.c_uint64(0)
        self._check(self._lib.blok_hip_beam_cache_node_counters(self._ctx, C.byref(n)))
        return int(n.value)

    def set_packed_fill(self, units_per_wave: int):
        """How a packed launch writes the miss pixels of its empty wave tiles (blok_hip_debug.h): 0 = a fill launch in front of the walk
        launch; k >= 1 = one launch whose walk workgroups also write at most k fill units of 64 pixels each.  Never changes a result."""
        self._check(self._lib.blok_hip_set_packed_fill(self._ctx, int(units_per_wave)))

    def packed_fill_counters(self):
        """(packed launches issued as one launch, workgroups of those launches that only filled)."""
        frames, tail = C.c_uint64(0), C.c_uint64(0)
        self._check(self._lib.blok_hip_packed_fill_counters(self._ctx, C.byref(frames), C.byref(tail)))
        return int(frames.value), int(tail.value)

    def beam_cache_refines(self) -> int:
        """Diagnostic: launches so far that issued a view's finer searches behind their walk."""
        n = C.c_uint64(0)
        self._check(self._lib.blok_hip_beam_cache_refines(self._ctx, C.byref(n)))
        return int(n.value)

    def beam_cache_fine_state(self) -> int:
        """What the latest rectangle launch had to do with its view's finer bounds: 0 nothing, 1 it issued their searches, 2 it walked from
        them.  Waits for nothing."""
        state = C.c_int(0)
        self._check(self._lib.blok_hip_beam_cache_download_fine(self._ctx, C.byref(state), None, None, 0))
        return int(state.value)

    def beam_cache_fine(self):
        """(state, t0) of the latest rectangle launch's finer bounds (blok_hip_debug.h: blok_hip_beam_cache_download_fine): state 0 none,
        1 it issued their searches behind its walk, 2 it walked from them; t0 one start parameter per 8 x 8 wave tile of the rectangle,
        row-major, or None for state 0."""
        state, n = C.c_int(0), C.c_uint32(0)
        self._check(self._lib.blok_hip_beam_cache_download_fine(self._ctx, C.byref(state), C.byref(n), None, 0))
        if not state.value:
            return 0, None
        t0 = np.zeros(int(n.value), dtype=np.float32)
        self._check(self._lib.blok_hip_beam_cache_download_fine(self._ctx, C.byref(state), C.byref(n), _ffi.ptr(t0), len(t0)))
        return int(state.value), t0

    def beam_cache_counters(self):
        """Diagnostic: (hits, fills) — launches so far that walked from kept beam bounds, and that searched into a slot."""
        hits, fills = C.c_uint64(0), C.c_uint64(0)
        self._check(self._lib.blok_hip_beam_cache_counters(self._ctx, C.byref(hits), C.byref(fills)))
        return int(hits.value), int(fills.value)

    def beam_cache_last(self):
        """(action, t0) of the latest rectangle launch (blok_hip_debug.h: blok_hip_beam_cache_download): action 0 it searched, 1 it searched
        into a slot, 2 it walked from a slot; t0 that slot's start parameters per beam tile, row-major, or None for action 0."""
        action, n = C.c_int(0), C.c_uint32(0)
        self._check(self._lib.blok_hip_beam_cache_download(self._ctx, C.byref(action), C.byref(n), None, 0))
        if not action.value:
            return 0, None
        t0 = np.zeros(int(n.value), dtype=np.float32)
        self._check(self._lib.blok_hip_beam_cache_download(self._ctx, C.byref(action), C.byref(n), _ffi.ptr(t0), len(t0)))
        return int(action.value), t0

    def beam_cache_last_action(self) -> int:
        """What the latest rectangle launch did about the kept beam bounds: 0 it searched, 1 it searched into a slot, 2 it walked from a slot.
        Waits for nothing."""
        action = C.c_int(0)
        self._check(self._lib.blok_hip_beam_cache_download(self._ctx, C.byref(action), None, None, 0))
        return int(action.value)

    def set_beam_budget(self, max_node_visits: int):
        """Node visits a beam search may spend (0 = default); running out is answered conservatively, never changes a result."""
        self._check(self._lib.blok_hip_set_beam_budget(self._ctx, max_node_visits))

    def set_voxel_size(self, voxel_size: float):
        """ChunkManager's voxelSize for the next add_world: a power of two in [1/256, 256] (default 1)."""
        self._check(self._lib.blok_hip_set_voxel_size(self._ctx, float(voxel_size)))

    def set_dense_dda(self, enabled: bool):
        """Dense-grid path: when on at add_dense, rectangle traces walk the uploaded grid itself (tiles + LDS occupancy bits)
        with a two-level DDA instead of the derived tree; records are identical."""
        self._check(self._lib.blok_hip_set_dense_dda(self._ctx, 1 if enabled else 0))

    def set_fused(self, enabled: bool):
        """Launch form (blok_hip.h): 0 two launches, 1 persistent grid with queues, 2 joint launch, 3 automatic (default); never changes a result."""
        self._check(self._lib.blok_hip_set_fused(self._ctx, int(enabled)))      # False/0, True/1 or 2 (joint launch, blok_hip.h)

    def frame_queue_stalls(self) -> int:
        """Waves of one-launch frames that ever gave up waiting for a queue entry (0 in a working system); synchronises."""
        n = C.c_uint32(0)
        self._check(self._lib.blok_hip_frame_queue_stalls(self._ctx, C.byref(n)))
        return int(n.value)

    def reset_accum(self):
        self._check(self._lib.blok_hip_reset_accum(self._ctx))

    def _check(self, rc: int):
        if rc != 0:
            raise BlokError(rc, self._lib.blok_hip_last_error(self._ctx).decode())

    # -- world -----------------------------------------------------------------------------
    def add_world(self, world) -> WorldStats:
        """world: blok_amd.world.PackedWorld (nodes, sub_chunks, materials)."""
        nodes = np.ascontiguousarray(world.nodes, dtype=SVO_NODE)
        subs = np.ascontiguousarray(world.sub_chunks, dtype=SUB_CHUNK)
        mats = np.ascontiguousarray(world.materials, dtype=MATERIAL)
        self._check(self._lib.blok_hip_upload_world(self._ctx, _ffi.ptr(nodes), len(nodes), _ffi.ptr(subs), len(subs),
                                                    _ffi.ptr(mats), len(mats)))
        return self.world_stats()

    update_world = add_world

    def add_dense(self, material_ids: np.ndarray, origin=(0, 0, 0), materials: np.ndarray | None = None) -> WorldStats:
        """material_ids[z][y][x], 0 = empty."""
        ids = np.ascontiguousarray(material_ids, dtype=np.uint32)
        nz, ny, nx = ids.shape
        mats = np.zeros(1, dtype=MATERIAL) if materials is None else np.ascontiguousarray(materials, dtype=MATERIAL)
        o = (C.c_int32 * 3)(*origin)
        self._check(self._lib.blok_hip_upload_dense(self._ctx, _ffi.ptr(ids), nx, ny, nz, o, _ffi.ptr(mats), len(mats)))
        return self.world_stats()

    def set_host_build(self, enabled: bool):
        self._check(self._lib.blok_hip_set_host_build(self._ctx, int(enabled)))

    def built_on_device(self) -> bool:
        return bool(self._lib.blok_hip_world_built_on_device(self._ctx))

    def download_tree(self):
        """(nodes as (n, 4) uint32, material ids) of the device-resident structure."""
        st = self.world_stats()
        nodes = np.zeros((st.n_tree_nodes, 4), dtype=np.uint32)
        mats = np.zeros(max(st.n_voxels, 1), dtype=np.uint32)
        self._check(self._lib.blok_hip_download_tree(self._ctx, _ffi.ptr(nodes), len(nodes), _ffi.ptr(mats), len(mats)))
        return nodes, mats[:st.n_voxels]

    def world_stats(self) -> WorldStats:
        s = WorldStats()
        self._check(self._lib.blok_hip_world_stats(self._ctx, C.byref(s)))
        return s

    # -- trace -----------------------------------------------------------------------------
    def draw_frame(self, cam: np.ndarray, rect=None) -> np.ndarray:
        """Primary first-hit records of the frame (or of rect = (x0, y0, w, h)), shape (h, w)."""
        x0, y0, w, h = rect if rect is not None else (0, 0, self.width, self.height)
        cam = np.ascontiguousarray(cam, dtype=CAMERA)
        hits = np.zeros(w * h, dtype=HIT)
        self._check(self._lib.blok_hip_trace_primary(self._ctx, _ffi.ptr(cam), x0, y0, w, h, _ffi.ptr(hits)))
        return hits.reshape(h, w)

    def draw_frame_device(self, cam: np.ndarray, hits_ptr: int = 0, rgba_ptr: int = 0, rect=None, stream: int = 0):
        """Asynchronous, device-resident outputs (either pointer may be 0, not both)."""
        x0, y0, w, h = rect if rect is not None else (0, 0, self.width, self.height)
        cam = np.ascontiguousarray(cam, dtype=CAMERA)
        self._check(self._lib.blok_hip_trace_primary_device(self._ctx, _ffi.ptr(cam), x0, y0, w, h,
                                                            C.c_void_p(hits_ptr), C.c_void_p(rgba_ptr),
                                                            C.c_void_p(stream)))

    def tiles_for_rank(self, tile: int, rank: int, n_ranks: int) -> int:
        return int(_ffi.hip_lib().blok_hip_tiles_for_rank(self.width, self.height, tile, rank, n_ranks))

    def draw_tiles_device(self, cam: np.ndarray, tile: int, rank: int, n_ranks: int, hits_ptr: int = 0,
                          rgba_ptr: int = 0, stream: int = 0):
        cam = np.ascontiguousarray(cam, dtype=CAMERA)
        self._check(self._lib.blok_hip_trace_tiles_device(self._ctx, _ffi.ptr(cam), tile, rank, n_ranks,
                                                          C.c_void_p(hits_ptr), C.c_void_p(rgba_ptr),
                                                          C.c_void_p(stream)))

    def untile_device(self, gathered_ptr: int, elem_bytes: int, tile: int, n_ranks: int, tiles_per_rank_max: int,
                      out_ptr: int, stream: int = 0):
        self._check(self._lib.blok_hip_untile_device(self._ctx, C.c_void_p(gathered_ptr), elem_bytes, tile, n_ranks,
                                                     tiles_per_rank_max, C.c_void_p(out_ptr), C.c_void_p(stream)))

    def compact_tiles_device(self, rgba_tiles_ptr: int, tile: int, n_tiles: int, out_ptr: int, stream: int = 0):
        """Dense RGBA8 tiles of this rank -> {count, {local tile index, pixels} per tile with a non-sky pixel} (blok_hip.h)."""
        self._check(self._lib.blok_hip_compact_tiles_device(self._ctx, C.c_void_p(rgba_tiles_ptr), tile, n_tiles, C.c_void_p(out_ptr), C.c_void_p(stream)))

    def scatter_tiles_device(self, gathered_ptr: int, n_ranks: int, rank_stride_words: int, tile: int, max_records: int, out_ptr: int, stream: int = 0):
        """Root: sky-filled frame + the compacted records of every rank (blok_hip.h)."""
        self._check(self._lib.blok_hip_scatter_tiles_device(self._ctx, C.c_void_p(gathered_ptr), n_ranks, rank_stride_words, tile, max_records,
                                                            C.c_void_p(out_ptr), C.c_void_p(stream)))

    # several frames per call (blok_hip.h: BLOK_MAX_TILE_FRAMES): cams is an array of 1..8 cameras
    def draw_tile_frames_device(self, cams: np.ndarray, tile: int, rank: int, n_ranks: int, frame_stride_tiles: int, hits_ptr: int = 0,
                                rgba_ptr: int = 0, stream: int = 0):
        cams = np.ascontiguousarray(cams, dtype=CAMERA).reshape(-1)
        self._check(self._lib.blok_hip_trace_tile_frames_device(self._ctx, _ffi.ptr(cams), len(cams), tile, rank, n_ranks, frame_stride_tiles,
                                                                C.c_void_p(hits_ptr), C.c_void_p(rgba_ptr), C.c_void_p(stream)))

    def untile_frames_device(self, gathered_ptr: int, elem_bytes: int, tile: int, n_ranks: int, tiles_per_rank_max: int, n_frames: int,
                             frame_stride_tiles: int, out_ptr: int, stream: int = 0):
        self._check(self._lib.blok_hip_untile_frames_device(self._ctx, C.c_void_p(gathered_ptr), elem_bytes, tile, n_ranks, tiles_per_rank_max,
                                                            n_frames, frame_stride_tiles, C.c_void_p(out_ptr), C.c_void_p(stream)))

    def compact_tile_frames_device(self, rgba_tiles_ptr: int, tile: int, n_tiles: int, n_frames: int, frame_stride_tiles: int, out_ptr: int,
                                   stream: int = 0):
        """n_frames frames of dense RGBA8 tiles -> counts + records interleaved by frame (blok_hip.h)."""
        self._check(self._lib.blok_hip_compact_tile_frames_device(self._ctx, C.c_void_p(rgba_tiles_ptr), tile, n_tiles, n_frames, frame_stride_tiles,
                                                                  C.c_void_p(out_ptr), C.c_void_p(stream)))

    def scatter_tile_frames_device(self, gathered_ptr: int, n_ranks: int, rank_stride_words: int, tile: int, max_records: int, n_frames: int,
                                   out_ptr: int, tile_state_ptr: int = 0, stream: int = 0):
        self._check(self._lib.blok_hip_scatter_tile_frames_device(self._ctx, C.c_void_p(gathered_ptr), n_ranks, rank_stride_words, tile, max_records,
                                                                  n_frames, C.c_void_p(out_ptr), C.c_void_p(tile_state_ptr), C.c_void_p(stream)))

    def exchange_code_bits(self) -> int:
        """16 if pixels can travel as 16-bit (material, face) codes with this world's material table, else 0 (blok_hip.h)."""
        return int(self._lib.blok_hip_exchange_code_bits(self._ctx))

    def compact_hit_tile_frames_device(self, hit_tiles_ptr: int, tile: int, n_tiles: int, n_frames: int, frame_stride_tiles: int, out_ptr: int,
                                       stream: int = 0):
        self._check(self._lib.blok_hip_compact_hit_tile_frames_device(self._ctx, C.c_void_p(hit_tiles_ptr), tile, n_tiles, n_frames, frame_stride_tiles,
                                                                      C.c_void_p(out_ptr), C.c_void_p(stream)))

    def scatter_code_tile_frames_device(self, gathered_ptr: int, n_ranks: int, rank_stride_words: int, tile: int, max_records: int, n_frames: int,
                                        out_ptr: int, tile_state_ptr: int = 0, stream: int = 0):
        self._check(self._lib.blok_hip_scatter_code_tile_frames_device(self._ctx, C.c_void_p(gathered_ptr), n_ranks, rank_stride_words, tile, max_records,
                                                                       n_frames, C.c_void_p(out_ptr), C.c_void_p(tile_state_ptr), C.c_void_p(stream)))

    def trace_rays(self, rays: np.ndarray) -> np.ndarray:
        rays = np.ascontiguousarray(rays, dtype=RAY)
        hits = np.zeros(len(rays), dtype=HIT)
        self._check(self._lib.blok_hip_trace_rays(self._ctx, _ffi.ptr(rays), len(rays), _ffi.ptr(hits)))
        return hits

    # -- instanced voxel models (blok_hip.h) ------------------------------------------------------------------------
    def model_create(self, xyz, material_ids) -> int:
        """Uploads a model (n voxels of its local lattice, one material id each); returns its id.  May synchronise the device."""
        xyz = np.ascontiguousarray(xyz, dtype=np.int32).reshape(-1, 3)
        mats = np.ascontiguousarray(material_ids, dtype=np.uint32).reshape(-1)
        if len(mats) != len(xyz):
            raise ValueError("one material id per voxel")
        out = C.c_uint32()
        self._check(self._lib.blok_hip_model_create(self._ctx, _ffi.ptr(xyz), _ffi.ptr(mats), len(mats), C.byref(out)))
        return int(out.value)

    def model_destroy(self, model: int):
        self._check(self._lib.blok_hip_model_destroy(self._ctx, int(model)))

    def model_set_scale(self, model: int, scale_log2: int):
        """One model voxel becomes a cube of 2**scale_log2 world voxels (0..8; blok_hip.h: "Scaled models").  Blocks; the previous-frame
        table of draw_frame_rt_instanced_motion is forgotten."""
        if scale_log2 < 0:
            raise ValueError("scale_log2 must be >= 0")
        self._check(self._lib.blok_hip_model_set_scale(self._ctx, int(model), int(scale_log2)))

    def model_scale(self, model: int) -> int:
        out = C.c_uint32()
        self._check(self._lib.blok_hip_model_scale(self._ctx, int(model), C.byref(out)))
        return int(out.value)

    # emissive models as lights (blok_amd/lights.py has the entries and their host twins)
    def model_lights(self, model: int):
        from . import lights
        return lights.model_lights(self, model)

    def model_lights_info(self, model: int):
        from . import lights
        return lights.model_lights_info(self, model)

    def model_lights_download(self, model: int, first=None, count=None, page: int = 1 << 22):
        from . import lights
        return lights.model_lights_download(self, model, first, count, page)

    def model_lights_clear(self, model: int):
        from . import lights
        lights.model_lights_clear(self, model)

    def instance_lights_info(self, instances):
        from . import lights
        return lights.instance_lights_info(self, instances)

    def model_download(self, model: int):
        """Diagnostic (blok_hip_debug.h: blok_hip_download_model): (nodes as (n, 4) uint32, material ids, info) of a model as it lies in
        device memory; info is a dict of levels, origin, lo, hi."""
        info = _ffi.ModelInfo()
        self._check(self._lib.blok_hip_download_model(self._ctx, int(model), None, 0, None, 0, C.byref(info)))
        nodes = np.zeros((int(info.n_nodes), 4), dtype=np.uint32)
        mats = np.zeros(int(info.n_materials), dtype=np.uint32)
        self._check(self._lib.blok_hip_download_model(self._ctx, int(model), _ffi.ptr(nodes), len(nodes), _ffi.ptr(mats) if len(mats) else None, len(mats), None))
        return nodes, mats, {"levels": int(info.levels), "origin": tuple(info.origin), "lo": tuple(info.lo), "hi": tuple(info.hi)}

    def check_instances(self, instances: np.ndarray):
        inst = np.ascontiguousarray(instances, dtype=INSTANCE).reshape(-1)
        self._check(self._lib.blok_hip_check_instances(self._ctx, _ffi.ptr(inst), len(inst)))

    def _placed_frame(self, cam: np.ndarray, instances, rect):
        """What the blocking primary frames over placed models prepare alike: the rectangle, the camera, the instance table and the outputs."""
        x0, y0, w, h = rect if rect is not None else (0, 0, self.width, self.height)
        cam = np.ascontiguousarray(cam, dtype=CAMERA)
        inst = np.ascontiguousarray(instances if instances is not None else [], dtype=INSTANCE).reshape(-1)
        return (x0, y0, w, h), cam, inst, np.zeros(w * h, dtype=HIT), np.zeros(w * h, dtype=np.uint32), np.zeros(w * h, dtype=np.uint32)

    def _placed_rays(self, rays: np.ndarray, instances):
        """... and the blocking rays: the rays, the instance table and the outputs."""
        rays = np.ascontiguousarray(rays, dtype=RAY)
        inst = np.ascontiguousarray(instances if instances is not None else [], dtype=INSTANCE).reshape(-1)
        return rays, inst, np.zeros(len(rays), dtype=HIT), np.zeros(len(rays), dtype=np.uint32)

    @staticmethod
    def _table(records: np.ndarray):
        return _ffi.ptr(records) if len(records) else None

    def trace_primary_instanced(self, cam: np.ndarray, instances: np.ndarray, rect=None):
        """(hits (h, w), instance ids (h, w), RGBA8 (h, w)) of the frame (or rect) over the world plus `instances` (INSTANCE records)."""
        (x0, y0, w, h), cam, inst, hits, ids, rgba = self._placed_frame(cam, instances, rect)
        self._check(self._lib.blok_hip_trace_primary_instanced(self._ctx, _ffi.ptr(cam), x0, y0, w, h, self._table(inst), len(inst),
                                                               _ffi.ptr(hits), _ffi.ptr(rgba), _ffi.ptr(ids)))
        return hits.reshape(h, w), ids.reshape(h, w), rgba.reshape(h, w)

    def trace_primary_instanced_device(self, cam: np.ndarray, instances_ptr: int, n_instances: int, hits_ptr: int = 0, rgba_ptr: int = 0,
                                       ids_ptr: int = 0, rect=None, stream: int = 0):
        """Asynchronous: device instance table and outputs (any output pointer may be 0, not all)."""
        x0, y0, w, h = rect if rect is not None else (0, 0, self.width, self.height)
        cam = np.ascontiguousarray(cam, dtype=CAMERA)
        self._check(self._lib.blok_hip_trace_primary_instanced_device(self._ctx, _ffi.ptr(cam), x0, y0, w, h, C.c_void_p(instances_ptr),
                                                                      int(n_instances), C.c_void_p(hits_ptr), C.c_void_p(rgba_ptr),
                                                                      C.c_void_p(ids_ptr), C.c_void_p(stream)))

    def trace_rays_instanced(self, rays: np.ndarray, instances: np.ndarray):
        """(records, instance ids) of explicit rays over the world plus `instances`."""
        rays, inst, hits, ids = self._placed_rays(rays, instances)
        self._check(self._lib.blok_hip_trace_rays_instanced(self._ctx, _ffi.ptr(rays), len(rays), self._table(inst), len(inst),
                                                            _ffi.ptr(hits), _ffi.ptr(ids)))
        return hits, ids

    # -- posed models (blok_hip.h, "Posed models"): instanced models under any rotation, scale, mirror or shear ------------------------------
    def check_poses(self, poses: np.ndarray):
        p = np.ascontiguousarray(poses, dtype=POSE).reshape(-1)
        self._check(self._lib.blok_hip_check_poses(self._ctx, _ffi.ptr(p) if len(p) else None, len(p)))

    def trace_primary_posed(self, cam: np.ndarray, instances, poses, rect=None):
        """(hits (h, w), ids (h, w), RGBA8 (h, w)) of the frame (or rect) over the world, `instances` (INSTANCE records) and `poses` (POSE
        records, blok_amd.pose).  A pixel a pose wins has id POSE_ID | index, the pose's local voxel and local face."""
        (x0, y0, w, h), cam, inst, hits, ids, rgba = self._placed_frame(cam, instances, rect)
        p = np.ascontiguousarray(poses if poses is not None else [], dtype=POSE).reshape(-1)
        self._check(self._lib.blok_hip_trace_primary_posed(self._ctx, _ffi.ptr(cam), x0, y0, w, h, self._table(inst), len(inst),
                                                           self._table(p), len(p), _ffi.ptr(hits), _ffi.ptr(rgba), _ffi.ptr(ids)))
        return hits.reshape(h, w), ids.reshape(h, w), rgba.reshape(h, w)

    def trace_primary_posed_device(self, cam: np.ndarray, instances_ptr: int, n_instances: int, poses_ptr: int, n_poses: int, hits_ptr: int = 0,
                                   rgba_ptr: int = 0, ids_ptr: int = 0, rect=None, stream: int = 0):
        """Asynchronous: device tables and outputs (any output pointer may be 0, not all)."""
        x0, y0, w, h = rect if rect is not None else (0, 0, self.width, self.height)
        cam = np.ascontiguousarray(cam, dtype=CAMERA)
        self._check(self._lib.blok_hip_trace_primary_posed_device(self._ctx, _ffi.ptr(cam), x0, y0, w, h, C.c_void_p(instances_ptr), int(n_instances),
                                                                  C.c_void_p(poses_ptr), int(n_poses), C.c_void_p(hits_ptr), C.c_void_p(rgba_ptr),
                                                                  C.c_void_p(ids_ptr), C.c_void_p(stream)))

    def trace_rays_posed(self, rays: np.ndarray, instances, poses):
        """(records, ids) of explicit rays over the world, `instances` and `poses`: every pose is tested for every ray."""
        rays, inst, hits, ids = self._placed_rays(rays, instances)
        p = np.ascontiguousarray(poses if poses is not None else [], dtype=POSE).reshape(-1)
        self._check(self._lib.blok_hip_trace_rays_posed(self._ctx, _ffi.ptr(rays), len(rays), self._table(inst), len(inst),
                                                        self._table(p), len(p), _ffi.ptr(hits), _ffi.ptr(ids)))
        return hits, ids

    def trace_rays_posed_device(self, rays_ptr: int, n: int, instances_ptr: int, n_instances: int, poses_ptr: int, n_poses: int, hits_ptr: int = 0,
                                ids_ptr: int = 0, stream: int = 0):
        self._check(self._lib.blok_hip_trace_rays_posed_device(self._ctx, C.c_void_p(rays_ptr), int(n), C.c_void_p(instances_ptr), int(n_instances),
                                                               C.c_void_p(poses_ptr), int(n_poses), C.c_void_p(hits_ptr), C.c_void_p(ids_ptr),
                                                               C.c_void_p(stream)))

    def trace_paths_instanced(self, cam: np.ndarray, instances: np.ndarray, spp: int = 8, max_bounces: int = 2, frame_index: int = 0, rect=None):
        """trace_paths over the world plus `instances` (INSTANCE records): the planes dict plus "ids", the instance of each pixel's
        first hit ((h, w) uint32, INSTANCE_NONE for the world or the sky)."""
        x0, y0, w, h = rect if rect is not None else (0, 0, self.width, self.height)
        cam = np.ascontiguousarray(cam, dtype=CAMERA)
        inst = np.ascontiguousarray(instances, dtype=INSTANCE).reshape(-1)
        planes = {k: np.zeros((h, w, 4), dtype=np.float32) for k in ("color", "world_pos", "normal_roughness", "albedo_metallic")}
        planes["ids"] = np.zeros((h, w), dtype=np.uint32)
        g = GBuffer(*[planes[k].ctypes.data for k in ("color", "world_pos", "normal_roughness", "albedo_metallic")])
        self._check(self._lib.blok_hip_trace_paths_instanced(self._ctx, _ffi.ptr(cam), x0, y0, w, h, spp, max_bounces, frame_index,
                                                             _ffi.ptr(inst), len(inst), C.byref(g), _ffi.ptr(planes["ids"])))
        return planes

    def trace_paths_instanced_device(self, cam: np.ndarray, instances_ptr: int, n_instances: int, color_ptr: int = 0, world_pos_ptr: int = 0,
                                     normal_roughness_ptr: int = 0, albedo_metallic_ptr: int = 0, ids_ptr: int = 0, spp: int = 8,
                                     max_bounces: int = 2, frame_index: int = 0, rect=None, stream: int = 0):
        """Asynchronous: device instance table, float4 device planes and id plane (any may be 0)."""
        x0, y0, w, h = rect if rect is not None else (0, 0, self.width, self.height)
        cam = np.ascontiguousarray(cam, dtype=CAMERA)
        g = GBuffer(color_ptr, world_pos_ptr, normal_roughness_ptr, albedo_metallic_ptr)
        self._check(self._lib.blok_hip_trace_paths_instanced_device(self._ctx, _ffi.ptr(cam), x0, y0, w, h, spp, max_bounces, frame_index,
                                                                    C.c_void_p(instances_ptr), int(n_instances), C.byref(g),
                                                                    C.c_void_p(ids_ptr), C.c_void_p(stream)))

    def trace_paths_instanced_ref_device(self, cam: np.ndarray, instances_ptr: int, n_instances: int, color_ptr: int = 0, world_pos_ptr: int = 0,
                                         normal_roughness_h_ptr: int = 0, albedo_metallic_u8_ptr: int = 0, motion_h_ptr: int = 0,
                                         prev_view_proj=None, ids_ptr: int = 0, spp: int = 8, max_bounces: int = 2, frame_index: int = 0,
                                         rect=None, stream: int = 0):
        """trace_paths_ref_device over the world plus a device instance table; ids_ptr: the id plane (may be 0)."""
        x0, y0, w, h = rect if rect is not None else (0, 0, self.width, self.height)
        cam = np.ascontiguousarray(cam, dtype=CAMERA)
        g = _ffi.GBufferRef(color_ptr, world_pos_ptr, normal_roughness_h_ptr, albedo_metallic_u8_ptr, motion_h_ptr)
        m = None if prev_view_proj is None else (C.c_float * 16)(*[float(v) for v in np.asarray(prev_view_proj, dtype=np.float32).reshape(-1)])
        self._check(self._lib.blok_hip_trace_paths_instanced_ref_device(self._ctx, _ffi.ptr(cam), x0, y0, w, h, spp, max_bounces, frame_index,
                                                                        C.c_void_p(instances_ptr), int(n_instances), m, C.byref(g),
                                                                        C.c_void_p(ids_ptr), C.c_void_p(stream)))

    def draw_frame_rt_instanced(self, cam: np.ndarray, instances: np.ndarray, spp: int = 8, max_bounces: int = 2, settings=None):
        """draw_frame_rt with the path pass over the world plus `instances`: (RGBA8 (h, w) uint32, frames rendered so far)."""
        cam = np.ascontiguousarray(cam, dtype=CAMERA)
        inst = np.ascontiguousarray(instances, dtype=INSTANCE).reshape(-1)
        out = np.zeros((self.height, self.width), dtype=np.uint32)
        frames = C.c_uint32()
        self._check(self._lib.blok_hip_draw_frame_rt_instanced(self._ctx, _ffi.ptr(cam), spp, max_bounces,
                                                               C.byref(settings) if settings is not None else None, _ffi.ptr(inst), len(inst),
                                                               _ffi.ptr(out), C.byref(frames)))
        return out, frames.value

    # -- posed models in the path-traced frame (blok_hip.h, "Path-traced frames with poses") ------------------------------------------------
    def trace_paths_posed(self, cam: np.ndarray, instances, poses, spp: int = 8, max_bounces: int = 2, frame_index: int = 0, rect=None):
        """trace_paths_instanced with `poses` (POSE records) behind the instances: the planes dict plus "ids" (POSE_ID | index where a pose
        wins the first hit).  A posed hit's normal is its face's own world normal."""
        x0, y0, w, h = rect if rect is not None else (0, 0, self.width, self.height)
        cam = np.ascontiguousarray(cam, dtype=CAMERA)
        inst = np.ascontiguousarray(instances if instances is not None else [], dtype=INSTANCE).reshape(-1)
        p = np.ascontiguousarray(poses if poses is not None else [], dtype=POSE).reshape(-1)
        planes = {k: np.zeros((h, w, 4), dtype=np.float32) for k in ("color", "world_pos", "normal_roughness", "albedo_metallic")}
        planes["ids"] = np.zeros((h, w), dtype=np.uint32)
        g = GBuffer(*[planes[k].ctypes.data for k in ("color", "world_pos", "normal_roughness", "albedo_metallic")])
        self._check(self._lib.blok_hip_trace_paths_posed(self._ctx, _ffi.ptr(cam), x0, y0, w, h, spp, max_bounces, frame_index, self._table(inst),
                                                         len(inst), self._table(p), len(p), C.byref(g), _ffi.ptr(planes["ids"])))
        return planes

    def trace_paths_posed_device(self, cam: np.ndarray, instances_ptr: int, n_instances: int, poses_ptr: int, n_poses: int, color_ptr: int = 0,
                                 world_pos_ptr: int = 0, normal_roughness_ptr: int = 0, albedo_metallic_ptr: int = 0, ids_ptr: int = 0,
                                 spp: int = 8, max_bounces: int = 2, frame_index: int = 0, rect=None, stream: int = 0):
        """Asynchronous: device tables, float4 device planes and id plane (any may be 0)."""
        x0, y0, w, h = rect if rect is not None else (0, 0, self.width, self.height)
        cam = np.ascontiguousarray(cam, dtype=CAMERA)
        g = GBuffer(color_ptr, world_pos_ptr, normal_roughness_ptr, albedo_metallic_ptr)
        self._check(self._lib.blok_hip_trace_paths_posed_device(self._ctx, _ffi.ptr(cam), x0, y0, w, h, spp, max_bounces, frame_index,
                                                                C.c_void_p(instances_ptr), int(n_instances), C.c_void_p(poses_ptr), int(n_poses),
                                                                C.byref(g), C.c_void_p(ids_ptr), C.c_void_p(stream)))

    def trace_paths_posed_ref_device(self, cam: np.ndarray, instances_ptr: int, n_instances: int, poses_ptr: int, n_poses: int, color_ptr: int = 0,
                                     world_pos_ptr: int = 0, normal_roughness_h_ptr: int = 0, albedo_metallic_u8_ptr: int = 0, motion_h_ptr: int = 0,
                                     prev_view_proj=None, ids_ptr: int = 0, spp: int = 8, max_bounces: int = 2, frame_index: int = 0,
                                     rect=None, stream: int = 0):
        """trace_paths_instanced_ref_device with a device pose table behind the instances."""
        x0, y0, w, h = rect if rect is not None else (0, 0, self.width, self.height)
        cam = np.ascontiguousarray(cam, dtype=CAMERA)
        g = _ffi.GBufferRef(color_ptr, world_pos_ptr, normal_roughness_h_ptr, albedo_metallic_u8_ptr, motion_h_ptr)
        m = None if prev_view_proj is None else (C.c_float * 16)(*[float(v) for v in np.asarray(prev_view_proj, dtype=np.float32).reshape(-1)])
        self._check(self._lib.blok_hip_trace_paths_posed_ref_device(self._ctx, _ffi.ptr(cam), x0, y0, w, h, spp, max_bounces, frame_index,
                                                                    C.c_void_p(instances_ptr), int(n_instances), C.c_void_p(poses_ptr), int(n_poses),
                                                                    m, C.byref(g), C.c_void_p(ids_ptr), C.c_void_p(stream)))

    def draw_frame_rt_posed(self, cam: np.ndarray, instances, poses, spp: int = 8, max_bounces: int = 2, settings=None):
        """draw_frame_rt_instanced with the path pass over the world, `instances` and `poses`: (RGBA8 (h, w) uint32, frames rendered so far)."""
        cam = np.ascontiguousarray(cam, dtype=CAMERA)
        inst = np.ascontiguousarray(instances if instances is not None else [], dtype=INSTANCE).reshape(-1)
        p = np.ascontiguousarray(poses if poses is not None else [], dtype=POSE).reshape(-1)
        out = np.zeros((self.height, self.width), dtype=np.uint32)
        frames = C.c_uint32()
        self._check(self._lib.blok_hip_draw_frame_rt_posed(self._ctx, _ffi.ptr(cam), spp, max_bounces, C.byref(settings) if settings is not None else None,
                                                           self._table(inst), len(inst), self._table(p), len(p), _ffi.ptr(out), C.byref(frames)))
        return out, frames.value

    def draw_frame_rt_instanced_motion(self, cam: np.ndarray, instances: np.ndarray, spp: int = 8, max_bounces: int = 2, settings=None):
        """draw_frame_rt_instanced with object motion: the context keeps the previous frame's table, and an instance whose index, model
        and usability carry over from it is reprojected where it was.  (RGBA8 (h, w) uint32, frames rendered so far)."""
        cam = np.ascontiguousarray(cam, dtype=CAMERA)
        inst = np.ascontiguousarray(instances, dtype=INSTANCE).reshape(-1)
        out = np.zeros((self.height, self.width), dtype=np.uint32)
        frames = C.c_uint32()
        self._check(self._lib.blok_hip_draw_frame_rt_instanced_motion(self._ctx, _ffi.ptr(cam), spp, max_bounces,
                                                                      C.byref(settings) if settings is not None else None, _ffi.ptr(inst),
                                                                      len(inst), _ffi.ptr(out), C.byref(frames)))
        return out, frames.value

    def instance_motion_device(self, world_pos_ptr: int, ids_ptr: int, cur_ptr: int, n_cur: int, prev_ptr: int, n_prev: int, prev_view_proj,
                               motion_h_ptr: int = 0, motion_ptr: int = 0, rect=None, stream: int = 0):
        """Asynchronous: the object motion of the rectangle's pixels whose first hit is a tracked instance, into an RG16F and/or a float2
        plane (w*h, the rectangle's own, like the world-position and id planes); other pixels are left untouched."""
        x0, y0, w, h = rect if rect is not None else (0, 0, self.width, self.height)
        m = None if prev_view_proj is None else (C.c_float * 16)(*[float(v) for v in np.asarray(prev_view_proj, dtype=np.float32).reshape(-1)])
        self._check(self._lib.blok_hip_instance_motion_device(self._ctx, x0, y0, w, h, C.c_void_p(world_pos_ptr), C.c_void_p(ids_ptr),
                                                              C.c_void_p(cur_ptr), int(n_cur), C.c_void_p(prev_ptr), int(n_prev), m,
                                                              C.c_void_p(motion_h_ptr), C.c_void_p(motion_ptr), C.c_void_p(stream)))

    def denoise_instanced_ref_device(self, color_ptr: int, world_pos_ptr: int, normal_roughness_h_ptr: int, motion_h_ptr: int, prev_view_proj,
                                     frame_count: int, out_color_ptr: int, ids_ptr: int, cur_ptr: int, n_cur: int, prev_ptr: int, n_prev: int,
                                     settings=None, stream: int = 0):
        """denoise_ref_device for a frame with instances: the id plane and this / the previous frame's device tables."""
        planes = _ffi.GBufferRef(color_ptr, world_pos_ptr, normal_roughness_h_ptr, 0, motion_h_ptr)
        m = (C.c_float * 16)(*[float(v) for v in np.asarray(prev_view_proj, dtype=np.float32).reshape(-1)])
        self._check(self._lib.blok_hip_denoise_instanced_ref_device(self._ctx, C.byref(planes), m, int(frame_count),
                                                                    C.byref(settings) if settings is not None else None, C.c_void_p(ids_ptr),
                                                                    C.c_void_p(cur_ptr), int(n_cur), C.c_void_p(prev_ptr), int(n_prev),
                                                                    out_color_ptr, stream or None))

    # -- object motion for posed models (blok_hip.h, "Object motion for posed models") ------------------------------------------------------
    def draw_frame_rt_posed_motion(self, cam: np.ndarray, instances, poses, spp: int = 8, max_bounces: int = 2, settings=None):
        """draw_frame_rt_posed with object motion: the context keeps the previous frame's instance and pose tables, and a pose (or instance)
        whose index, model and usability carry over from them is reprojected where it was.  (RGBA8 (h, w) uint32, frames rendered so far)."""
        cam = np.ascontiguousarray(cam, dtype=CAMERA)
        inst = np.ascontiguousarray(instances if instances is not None else [], dtype=INSTANCE).reshape(-1)
        p = np.ascontiguousarray(poses if poses is not None else [], dtype=POSE).reshape(-1)
        out = np.zeros((self.height, self.width), dtype=np.uint32)
        frames = C.c_uint32()
        self._check(self._lib.blok_hip_draw_frame_rt_posed_motion(self._ctx, _ffi.ptr(cam), spp, max_bounces,
                                                                  C.byref(settings) if settings is not None else None, self._table(inst), len(inst),
                                                                  self._table(p), len(p), _ffi.ptr(out), C.byref(frames)))
        return out, frames.value

    def posed_motion_device(self, world_pos_ptr: int, ids_ptr: int, cur_ptr: int, n_cur: int, prev_ptr: int, n_prev: int, cur_poses_ptr: int,
                            n_cur_poses: int, prev_poses_ptr: int, n_prev_poses: int, prev_view_proj, motion_h_ptr: int = 0, motion_ptr: int = 0,
                            rect=None, stream: int = 0):
        """Asynchronous: instance_motion_device for a frame with poses: the object motion of the rectangle's pixels whose first hit is a
        tracked instance or a tracked pose; other pixels are left untouched."""
        x0, y0, w, h = rect if rect is not None else (0, 0, self.width, self.height)
        m = None if prev_view_proj is None else (C.c_float * 16)(*[float(v) for v in np.asarray(prev_view_proj, dtype=np.float32).reshape(-1)])
        self._check(self._lib.blok_hip_posed_motion_device(self._ctx, x0, y0, w, h, C.c_void_p(world_pos_ptr), C.c_void_p(ids_ptr),
                                                           C.c_void_p(cur_ptr), int(n_cur), C.c_void_p(prev_ptr), int(n_prev),
                                                           C.c_void_p(cur_poses_ptr), int(n_cur_poses), C.c_void_p(prev_poses_ptr), int(n_prev_poses), m,
                                                           C.c_void_p(motion_h_ptr), C.c_void_p(motion_ptr), C.c_void_p(stream)))

    def denoise_posed_ref_device(self, color_ptr: int, world_pos_ptr: int, normal_roughness_h_ptr: int, motion_h_ptr: int, prev_view_proj,
                                 frame_count: int, out_color_ptr: int, ids_ptr: int, cur_ptr: int, n_cur: int, prev_ptr: int, n_prev: int,
                                 cur_poses_ptr: int, n_cur_poses: int, prev_poses_ptr: int, n_prev_poses: int, settings=None, stream: int = 0):
        """denoise_instanced_ref_device for a frame with poses: the id plane, and this / the previous frame's device tables of both kinds."""
        planes = _ffi.GBufferRef(color_ptr, world_pos_ptr, normal_roughness_h_ptr, 0, motion_h_ptr)
        m = None if prev_view_proj is None else (C.c_float * 16)(*[float(v) for v in np.asarray(prev_view_proj, dtype=np.float32).reshape(-1)])
        self._check(self._lib.blok_hip_denoise_posed_ref_device(self._ctx, C.byref(planes), m, int(frame_count),
                                                                C.byref(settings) if settings is not None else None, C.c_void_p(ids_ptr),
                                                                C.c_void_p(cur_ptr), int(n_cur), C.c_void_p(prev_ptr), int(n_prev),
                                                                C.c_void_p(cur_poses_ptr), int(n_cur_poses), C.c_void_p(prev_poses_ptr), int(n_prev_poses),
                                                                C.c_void_p(out_color_ptr), C.c_void_p(stream)))

    def debug_pose_motion_records(self, cur: np.ndarray, prev: np.ndarray) -> np.ndarray:
        """The POSE_MOTION records the prepare kernel builds for host table `cur` against `prev` (unchecked) with this context's models."""
        c = np.ascontiguousarray(cur, dtype=POSE).reshape(-1)
        p = np.ascontiguousarray(prev, dtype=POSE).reshape(-1)
        out = np.zeros(len(c), dtype=_ffi.POSE_MOTION)
        self._check(self._lib.blok_hip_debug_pose_motion_records(self._ctx, self._table(c), len(c), self._table(p), len(p), self._table(out)))
        return out

    def debug_build_tlas(self, instances_ptr: int, n_instances: int) -> np.ndarray:
        """The instance BVH of a device table (tlas_core.h: TlasNode), as an (nodes, 8) int32 array."""
        count = C.c_uint32()
        cap = 2 * (1 << max(0, int(n_instances) - 1).bit_length())
        out = np.zeros((cap, 8), dtype=np.int32)
        self._check(self._lib.blok_hip_debug_build_tlas(self._ctx, C.c_void_p(instances_ptr), int(n_instances), _ffi.ptr(out), cap, C.byref(count)))
        return out[:count.value]

    def debug_build_pose_tlas(self, cam: np.ndarray, poses_ptr: int, n_poses: int) -> np.ndarray:
        """The pose BVH of a device pose table for a launch from `cam` (pose_tlas_core.h), as an (nodes, 8) int32 array."""
        count = C.c_uint32()
        cap = 2 * (1 << max(0, int(n_poses) - 1).bit_length())
        out = np.zeros((cap, 8), dtype=np.int32)
        cam = np.ascontiguousarray(cam, dtype=CAMERA)
        self._check(self._lib.blok_hip_debug_build_pose_tlas(self._ctx, _ffi.ptr(cam), C.c_void_p(poses_ptr), int(n_poses), _ffi.ptr(out), cap, C.byref(count)))
        return out[:count.value]

    def set_pose_tlas(self, enabled=True):
        """Posed path launches with (default) or without the pose BVH: the frames are identical."""
        self._check(self._lib.blok_hip_set_pose_tlas(self._ctx, int(bool(enabled))))

    def trace_paths(self, cam: np.ndarray, spp: int = 8, max_bounces: int = 2, frame_index: int = 0, rect=None):
        """raygen.rgen's sample/bounce loop: dict of (h, w, 4) float32 planes
        color, world_pos, normal_roughness, albedo_metallic."""
        x0, y0, w, h = rect if rect is not None else (0, 0, self.width, self.height)
        cam = np.ascontiguousarray(cam, dtype=CAMERA)
        planes = {k: np.zeros((h, w, 4), dtype=np.float32) for k in ("color", "world_pos", "normal_roughness", "albedo_metallic")}
        g = GBuffer(*[planes[k].ctypes.data for k in ("color", "world_pos", "normal_roughness", "albedo_metallic")])
        self._check(self._lib.blok_hip_trace_paths(self._ctx, _ffi.ptr(cam), x0, y0, w, h, spp, max_bounces, frame_index,
                                                   C.byref(g)))
        return planes

    def trace_paths_device(self, cam: np.ndarray, color_ptr: int, spp: int = 8, max_bounces: int = 2,
                           frame_index: int = 0, rect=None, world_pos_ptr: int = 0, normal_roughness_ptr: int = 0,
                           albedo_metallic_ptr: int = 0, stream: int = 0):
        x0, y0, w, h = rect if rect is not None else (0, 0, self.width, self.height)
        cam = np.ascontiguousarray(cam, dtype=CAMERA)
        g = GBuffer(color_ptr, world_pos_ptr, normal_roughness_ptr, albedo_metallic_ptr)
        self._check(self._lib.blok_hip_trace_paths_device(self._ctx, _ffi.ptr(cam), x0, y0, w, h, spp, max_bounces,
                                                          frame_index, C.byref(g), C.c_void_p(stream)))

    def trace_paths_ref_device(self, cam: np.ndarray, color_ptr: int = 0, world_pos_ptr: int = 0, normal_roughness_h_ptr: int = 0,
                               albedo_metallic_u8_ptr: int = 0, motion_h_ptr: int = 0, prev_view_proj=None, spp: int = 8,
                               max_bounces: int = 2, frame_index: int = 0, rect=None, stream: int = 0):
        """Path-traced frame with the G-buffer in the reference's image formats (RGBA32F x 2, RGBA16F, RGBA8, RG16F motion)."""
        x0, y0, w, h = rect if rect is not None else (0, 0, self.width, self.height)
        cam = np.ascontiguousarray(cam, dtype=CAMERA)
        g = _ffi.GBufferRef(color_ptr, world_pos_ptr, normal_roughness_h_ptr, albedo_metallic_u8_ptr, motion_h_ptr)
        m = None if prev_view_proj is None else (C.c_float * 16)(*[float(v) for v in np.asarray(prev_view_proj, dtype=np.float32).reshape(-1)])
        self._check(self._lib.blok_hip_trace_paths_ref_device(self._ctx, _ffi.ptr(cam), x0, y0, w, h, spp, max_bounces, frame_index,
                                                              m, C.byref(g), C.c_void_p(stream)))

    def denoise_ref_device(self, color_ptr: int, world_pos_ptr: int, normal_roughness_h_ptr: int, motion_h_ptr: int, prev_view_proj,
                           frame_count: int, out_color_ptr: int, settings=None, stream: int = 0):
        """Denoiser::denoise for one frame over reference-format planes (as trace_paths_ref_device writes them)."""
        planes = _ffi.GBufferRef(color_ptr, world_pos_ptr, normal_roughness_h_ptr, 0, motion_h_ptr)
        m = (C.c_float * 16)(*[float(v) for v in np.asarray(prev_view_proj, dtype=np.float32).reshape(-1)])
        self._check(self._lib.blok_hip_denoise_ref_device(self._ctx, C.byref(planes), m, int(frame_count),
                                                          C.byref(settings) if settings is not None else None, out_color_ptr, stream or None))

    def draw_frame_accumulate(self, cam: np.ndarray, spp_per_frame: int = 1, max_bounces: int = 2):
        """Progressive frame of the compute backend (CudaTracer::drawFrame): returns (RGBA8 (h, w) uint32, frames accumulated)."""
        cam = np.ascontiguousarray(cam, dtype=CAMERA)
        out = np.zeros((self.height, self.width), dtype=np.uint32)
        frames = C.c_uint32()
        self._check(self._lib.blok_hip_draw_frame_accumulate(self._ctx, _ffi.ptr(cam), spp_per_frame, max_bounces,
                                                             _ffi.ptr(out), C.byref(frames)))
        return out, frames.value

    def accum_download(self) -> np.ndarray:
        out = np.zeros((self.height, self.width, 4), dtype=np.float32)
        self._check(self._lib.blok_hip_accum_download(self._ctx, _ffi.ptr(out)))
        return out

    def tonemap(self, hdr: np.ndarray, exposure: float = 1.0, saturation_boost: float = 1.15, operator: int = 1) -> np.ndarray:
        """tonemap.comp: (..., 4) float32 HDR -> (...) uint32 RGBA8 (reference defaults)."""
        hdr = np.ascontiguousarray(hdr, dtype=np.float32)
        out = np.zeros(hdr.shape[:-1], dtype=np.uint32)
        self._check(self._lib.blok_hip_tonemap(self._ctx, _ffi.ptr(hdr), out.size, exposure, saturation_boost, operator,
                                               _ffi.ptr(out)))
        return out

    def tonemap_device(self, hdr_ptr: int, out_rgba8_ptr: int, n_pixels: int = 0, exposure: float = 1.0, saturation_boost: float = 1.15,
                       operator: int = 1, stream: int = 0):
        self._check(self._lib.blok_hip_tonemap_device(self._ctx, hdr_ptr, n_pixels or self.width * self.height, exposure,
                                                      saturation_boost, operator, out_rgba8_ptr, stream or None))

    def shade_rgba8(self, cam: np.ndarray, rect=None) -> np.ndarray:
        x0, y0, w, h = rect if rect is not None else (0, 0, self.width, self.height)
        cam = np.ascontiguousarray(cam, dtype=CAMERA)
        out = np.zeros(w * h, dtype=np.uint32)
        self._check(self._lib.blok_hip_shade_rgba8(self._ctx, _ffi.ptr(cam), x0, y0, w, h, _ffi.ptr(out)))
        return out.reshape(h, w)

    # -- timing ----------------------------------------------------------------------------
    def release_stream(self, stream: int):
        """Before destroying a HIP stream that was passed to *_device entries: the context drops its per-stream scratch and markers."""
        self._check(self._lib.blok_hip_release_stream(self._ctx, C.c_void_p(stream)))

    def set_timing(self, enabled: bool):
        self._check(self._lib.blok_hip_set_timing(self._ctx, int(enabled)))

    def last_kernel_ms(self) -> float:
        ms = C.c_float()
        self._check(self._lib.blok_hip_last_kernel_ms(self._ctx, C.byref(ms)))
        return ms.value
