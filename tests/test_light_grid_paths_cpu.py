"""CPU: the lit path loop under a light grid (path_core.h: grid_light_sample, shade_pixel<…, kGrid>) through the host shim
tests/host_harness/light_grid_paths_shim.cpp: the sampler against a numpy float32 restatement bit for bit — both strategies, inlist true and
false on the global branch, a point without a cell, m >> 24 equal to s - 1 and to s — and the frame equalities: the grid flag off gives
the lit body's bytes, and a grid in which every cell lists every light gives the lit body's frame within 16 * 2^-24 of the pixel."""
from __future__ import annotations

import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from blok_amd import lights as LT
from blok_amd import world as W
from blok_amd._ffi import INSTANCE, LIGHT, MATERIAL, POSE
from tests import light_grid_cases as GC
from tests import light_grid_reference as GR
from tests import lights_reference as LR
from tests.test_lit_paths_cpu import FLAGS, GLOW2, LitShim, PLANES, ROOM_CAM, ROOT, SRC, _ptr, materials, room, room_table, voxels_of

f32 = np.float32


class GridShim:
    def __init__(self, out):
        subprocess.run(["g++", *FLAGS, "-shared", "-o", os.fspath(out), os.fspath(SRC / "light_grid_paths_shim.cpp"), os.fspath(ROOT / "blok_amd/csrc/hip/tree_build.cpp")], check=True)
        L = C.CDLL(os.fspath(out))
        L.is_model.restype = C.c_void_p
        L.is_model.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.POINTER(C.c_char_p)]
        L.is_free.argtypes = [C.c_void_p]
        L.gp_render.argtypes = ([C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p, C.c_uint32, C.c_void_p, C.c_uint32, C.c_float, C.c_void_p, C.c_void_p] + [C.c_uint32] * 6 +
                                [C.c_void_p, C.c_uint32, C.c_void_p, C.c_uint32, C.c_float, C.c_int] + [C.c_void_p] * 4 + [C.c_void_p] * 5)
        L.gp_light_sample.restype = C.c_int
        L.gp_light_sample.argtypes = [C.c_void_p, C.c_uint32, C.c_uint32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint32, C.c_float, C.c_void_p, C.c_void_p,
                                      C.c_uint32, C.c_float, C.c_float, C.c_uint32, C.c_void_p, C.c_void_p, C.c_void_p]
        self.lib = L

    tree = LitShim.tree

    def render(self, world, cam, mats, w, h, spp, bounces, frame, table, grid=None, vs=1.0, models=(), inst=None, poses=None):
        planes = {k: np.zeros((h, w, 4), dtype=f32) for k in PLANES}
        ids = np.zeros((h, w), dtype=np.uint32)
        handles = (C.c_void_p * max(1, len(models)))(*[m.value for m in models])
        inst = np.ascontiguousarray(inst if inst is not None else [], dtype=INSTANCE).reshape(-1)
        poses = np.ascontiguousarray(poses if poses is not None else [], dtype=POSE).reshape(-1)
        table = np.ascontiguousarray(table, dtype=LIGHT)
        faces = int((table["du"].astype(np.int64) * table["dv"]).sum())
        owned = np.zeros(2048, dtype=np.uint32)
        for i in LR.material_index(table["material"], len(mats)):
            owned[i >> 5] |= np.uint32(1 << (i & 31))
        g = grid if grid is not None else (None, None, None, None)
        self.lib.gp_render(world, handles, len(models), _ptr(inst), len(inst), _ptr(poses), len(poses), vs, _ptr(np.ascontiguousarray(cam)), _ptr(mats), len(mats), w, h, spp, bounces, frame, _ptr(table), len(table),
                           _ptr(owned), faces, float(f32(faces) * f32(vs) * f32(vs)), 1 if grid is not None else 0, *[_ptr(a) for a in g],
                           *[_ptr(planes[k]) for k in PLANES], _ptr(ids))
        planes["ids"] = ids
        return planes


@pytest.fixture(scope="module")
def shim(tmp_path_factory):
    return GridShim(tmp_path_factory.mktemp("grid") / "liblight_grid_paths_shim.so")


def numpy_grid_sample(table, grid, mats, vs, hit_pos, n, r, u1, u2, m):
    """DESIGN.md §34 in float32, every operation rounded separately: (has, q, le, g, what, ray) with what = (local, inlist, A_g) and
    ray = (origin, direction, distance) of the sample's shadow ray."""
    start, faces, items, info = grid
    c, reach, s = int(info["cell_log2"][0]), int(info["reach"][0]), int(info["share"][0])
    lo, dim = info["cell_lo"][0].astype(np.int64), info["dim"][0].astype(np.int64)
    vs = f32(vs)
    hit_pos, n = np.asarray(hit_pos, dtype=f32), np.asarray(n, dtype=f32)
    x = hit_pos + n * f32(0.001)
    v = np.floor(x / vs)
    a_g, cell, gabs = 0, None, None
    if np.all(np.abs(v) < f32(2.0 ** 30)):
        gabs = v.astype(np.int64) >> c
        rel = gabs - lo
        if np.all((rel >= 0) & (rel < dim)):
            cell = int((rel[2] * dim[1] + rel[1]) * dim[0] + rel[0])
            a_g = int(faces[cell])
    a_dom = int((table["du"].astype(np.int64) * table["dv"]).sum())
    local = a_g > 0 and (int(m) >> 24) < s
    if local:
        p = LR.pick_of(r, a_g)
        seg = items[start[cell]:start[cell + 1]]
        k = int(np.searchsorted(seg["lcum"].astype(np.int64), p, side="right")) - 1
        light, off, inlist = table[int(seg["light"][k])], p - int(seg["lcum"][k]), True
    else:
        pick = LR.pick_of(r, a_dom)
        i = LR.find_light(table, pick)
        light, off = table[i], pick - int(table["cum"][i])
        inlist = False
        if a_g > 0:
            cmin, cmax = GR.cell_ranges(table[i:i + 1], c)
            inlist = bool(GR.listed(cmin, cmax, reach, gabs)[0])
    w_loc = (f32(s) / f32(256.0)) / f32(a_g) if inlist else f32(0.0)
    w_glob = (f32(256 - s) / f32(256.0) if a_g > 0 else f32(1.0)) / f32(a_dom)
    area_eff = (vs * vs) / (w_loc + w_glob)
    q, nl = LR.sample_point(light, off, u1, u2, vs)
    g, org, dr, dist = LR.geometry(hit_pos, n, q, nl, area_eff)
    le = mats["emission"][int(LR.material_index(np.array([light["material"]]), len(mats))[0])]
    return bool(g > 0), q, le, f32(g), (local, inlist, a_g), (org, dr, dist)


def test_sampler_equals_the_numpy_restatement_bit_for_bit(shim):
    """Two clusters and a grid of c = 3, reach 0, so that a shading cell lists some lights and not others; shading points in a listing
    cell, in an empty cell of the box, outside the box and beyond 2^30 voxels; vs 1 and 0.5; m >> 24 at s - 1 and at s."""
    case = next(c for c in GC.table() if c.name == "two distant clusters")
    table = case.lights
    mats = materials()
    seen = set()
    rng = np.random.default_rng(34)
    q, le, g = np.zeros(3, dtype=f32), np.zeros(3, dtype=f32), np.zeros(1, dtype=f32)
    for vs in (1.0, 0.5):
        for reach, share in ((0, 192), (1, 1), (1, 255)):
            grid = LT.host_build_grid(table, 3, reach, share)
            points = [((6.2, 2.5, 7.1), (0, -1, 0)), ((7.5, 3.0, 6.0), (0, 1, 0)), ((100.0, 2.0, 20.0), (0, 1, 0)), ((206.0, 1.0, 46.5), (1, 0, 0)),
                      ((-300.0, 4.0, 4.0), (0, 1, 0)), ((3.0e9, 4.0, 4.0), (0, 1, 0)), ((4.0, -2.0e9, 4.0), (0, 1, 0))]
            for pos, nrm in points:
                hit_pos, n = np.array(pos, dtype=f32) * f32(vs), np.array(nrm, dtype=f32)
                for m in (0, (share - 1) << 24 | 0xFFFFFF, share << 24, 0xFFFFFFFF):
                    for _ in range(6):
                        r, u1, u2 = int(rng.integers(0, 2 ** 32)), f32(rng.random()), f32(rng.random())
                        has = shim.lib.gp_light_sample(_ptr(table), len(table), int((table["du"].astype(np.int64) * table["dv"]).sum()), _ptr(grid[0]), _ptr(grid[1]), _ptr(grid[2]),
                                                       _ptr(grid[3]), _ptr(mats), len(mats), vs, _ptr(hit_pos), _ptr(n), r, float(u1), float(u2), m, _ptr(q), _ptr(le), _ptr(g))
                        whas, wq, wle, wg, what, _ = numpy_grid_sample(table, grid, mats, vs, hit_pos, n, r, u1, u2, m)
                        assert bool(has) == whas, (pos, m, what)
                        if whas:
                            assert q.tobytes() == wq.tobytes() and g[0].tobytes() == wg.tobytes() and le.tobytes() == np.asarray(wle, dtype=f32).tobytes(), (pos, m, what, g[0], wg)
                        seen.add((what[0], what[1], what[2] > 0, (m >> 24) - share if m not in (0, 0xFFFFFFFF) else None))
    print(sorted(seen, key=str))
    kinds = {k[:3] for k in seen}
    assert (True, True, True) in kinds, "local"
    assert (False, True, True) in kinds and (False, False, True) in kinds, "global with inlist true and false"
    assert (False, False, False) in kinds, "a point without a cell"
    assert any(k[0] and k[3] == -1 for k in seen) and any(not k[0] and k[2] and k[3] == 0 for k in seen), "m >> 24 at s - 1 is local, at s global"


def test_flag_off_is_the_lit_body_and_a_grid_that_lists_everything_is_the_lit_frame(shim):
    """The 14^3 room and its one ceiling light, c = 4, reach 0: one cell that lists the light, and every shading point lies in it.  Then
    A_g = A and lcum = cum, so both strategies pick the lit body's face from r, and at 1 spp and 1 bounce nothing behind the fourth draw
    reaches the pixel.  area_eff = (vs * vs) / (w_loc + w_glob) against area_world = (float(A) * vs) * vs: the two quotients s / 256 and
    (256 - s) / 256 are exact, each division by float(A) rounds once (2), their sum once (3), the quotient once (4), against the two
    roundings of area_world that it replaces (6 in all, each 2^-24 relative at most); the product with area_eff and the one with 1 / pi
    carry the difference, the multiplication into `pending` and the final add to the pixel round once more each: 16 * 2^-24 of the pixel
    bounds it with room to spare."""
    d, m = room()
    xyz, ids = voxels_of(d, m)
    mats = materials()
    table = room_table(GLOW2)
    w, h = 24, 18
    cam = W.camera_look_at(*ROOM_CAM, 70.0, w, h)
    world = shim.tree(xyz, ids)
    grid = LT.host_build_grid(table, 4, 0, 192)
    assert int(grid[3]["n_cells"][0]) == 1 and int(grid[1][0]) == 16
    lit = shim.render(world, cam, mats, w, h, 1, 1, 3, table)
    for k in PLANES:
        assert np.isfinite(lit[k]).all()
    under = shim.render(world, cam, mats, w, h, 1, 1, 3, table, grid)
    for k in PLANES[1:]:
        assert under[k].tobytes() == lit[k].tobytes(), k
    a, b = lit["color"][..., :3].astype(np.float64), under["color"][..., :3].astype(np.float64)
    worst = float((np.abs(a - b) / np.maximum(np.abs(a), 1e-30)).max())
    print(f"worst relative difference {worst:.3g} = {worst * 2 ** 24:.2f} * 2^-24; {int((a != b).any(-1).sum())} of {w * h} pixels not bit-equal")
    assert (a > 0).any() and np.all(np.abs(a - b) <= 16.0 * 2.0 ** -24 * np.abs(a))
    # more samples and bounces: the fourth draw moves the stream, the frames differ, the G-buffer does not
    lit2, under2 = shim.render(world, cam, mats, w, h, 2, 3, 3, table), shim.render(world, cam, mats, w, h, 2, 3, 3, table, grid)
    assert (lit2["color"] != under2["color"]).any() and np.isfinite(under2["color"]).all()
    for k in PLANES[1:]:
        assert under2[k].tobytes() == lit2[k].tobytes(), k
    shim.lib.is_free(world)


def test_flag_off_gives_the_lit_shims_bytes(shim, tmp_path):
    lit_shim = LitShim(tmp_path / "liblit_paths_shim.so")
    d, m = room()
    xyz, ids = voxels_of(d, m)
    mats = materials()
    table = room_table(GLOW2)
    w, h = 16, 12
    cam = W.camera_look_at(*ROOM_CAM, 70.0, w, h)
    world, world2 = shim.tree(xyz, ids), lit_shim.tree(xyz, ids)
    a = shim.render(world, cam, mats, w, h, 2, 3, 5, table)
    b = lit_shim.render(world2, [], None, None, cam, mats, w, h, 2, 3, 5, table=table)
    for k in PLANES:
        assert a[k].tobytes() == b[k].tobytes(), k
    shim.lib.is_free(world)
    lit_shim.lib.is_free(world2)
