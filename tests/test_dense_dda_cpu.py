"""CPU: the dense-grid kernel's per-ray body (blok_amd/csrc/hip/dense_core.h: two-level DDA over the tiled id grid) compiled for the
host by tests/host_harness/dense_shim.cpp, against the oracle, at the places where a DDA goes wrong: grids of one tile and one cell,
extents around a tile edge, grids at the int16 coordinate limits, rays built to tie two or three far planes over and over, rays that
start inside a filled cell or on lattice planes / tile faces / tile corners, short and late intervals.  Every case runs with both
occupancy-word accessors (the kernel's LDS copy and the global array) and compares every record of every ray bit for bit; the hit /
miss floors are figures the oracle alone reaches (it reports 1.2 to 1.5 times each floor)."""
import itertools
import os
import subprocess
import sys
from pathlib import Path

import numpy as np
import pytest

from blok_amd import world as W
from tests import harness_ffi as H
from tests import oracle_ffi as O
from tests.conftest import SEED, edge_case_rays, make_scene_world, random_rays, records_equal

ROOT = Path(__file__).resolve().parent.parent
DIMS = (1, 7, 8, 9, 17)
FILLS = ("empty", "corners", "sparse", "half", "solid", "big_ids")
ORIGINS = ((0, 0, 0), (-13, -8, -21))            # the negative one: a tile-aligned axis, two that are not
NEAR_ZERO_DIRS = [(1e-7, -1, 1e-7), (-1e-7, -1, 0), (0.5, -0.5, 1e-6), (1, -0.001, 0), (0, -0.001, 1), (1, -1e-3, 1)]   # edge_case_rays()
SIGNS = list(itertools.product((1.0, -1.0), repeat=3))

_lib = None          # the sanitizer run points this at the ASan+UBSan build of the shim


def host_dense(ids, origin, global_bits):
    return H.HostDense(ids, origin, global_bits=global_bits, lib=_lib)


def oracle_world(ids, origin):
    """The grid's voxels through ChunkManager -> the packed world the oracle walks."""
    z, y, x = np.nonzero(ids)
    xyz = (np.stack([x, y, z], axis=1) + np.asarray(origin)).astype(np.int32)
    cm = W.ChunkManager(128, 1.0)
    if len(xyz):
        cm.set_voxels(xyz, np.ascontiguousarray(ids[z, y, x], dtype=np.uint32))
    cm.rebuild_dirty_chunks()
    return cm.pack_chunks_to_gpu_svo()


def oracle_trace(ids, origin, rays):
    n_voxels = int(np.count_nonzero(ids))
    if n_voxels == 0:
        miss = np.zeros(len(rays), dtype=O.HIT)                  # miss.rmiss:25-27, what the oracle writes for a ray that reports nothing
        miss["t"], miss["face"] = -1.0, 0xFF
        return miss
    pw = oracle_world(ids, origin)
    if n_voxels <= 64:                                           # the tiny worlds: every voxel against every ray
        return O.trace_bruteforce(pw.nodes, pw.sub_chunks, rays)[0]
    return O.Lattice(pw.nodes, pw.sub_chunks).trace(rays)[0]


def check(ids, origin, rays, ref=None):
    """Both accessors against the oracle on every ray; returns (hits, misses) of the oracle."""
    ref = oracle_trace(ids, origin, rays) if ref is None else ref
    for global_bits in (False, True):
        got = host_dense(ids, origin, global_bits).trace_rays(rays)
        eq = records_equal(got, ref)
        assert eq.all(), (ids.shape, origin, global_bits, int((~eq).sum()), rays[~eq][:3], got[~eq][:3], ref[~eq][:3])
    hits = int(ref["hit"].sum())
    return hits, len(rays) - hits


def octants(rays):
    d = rays["dir"]
    full = (d != 0).all(axis=1)
    return {tuple(np.sign(v)) for v in d[full]}


def make_rays(org, d, tmin=0.001, tmax=10000.0, normalise=True):
    org = np.asarray(org, dtype=np.float64).reshape(-1, 3)
    d = np.asarray(d, dtype=np.float64).reshape(-1, 3)
    if normalise:
        d = d / np.maximum(np.linalg.norm(d, axis=1, keepdims=True), 1e-30)
    rays = np.zeros(len(org), dtype=O.RAY)
    rays["org"], rays["dir"] = org.astype(np.float32), d.astype(np.float32)
    rays["tmin"], rays["tmax"] = tmin, tmax
    return rays


def fill_grid(shape_zyx, fill, rng):
    nz, ny, nx = shape_zyx
    if fill == "empty":
        return np.zeros(shape_zyx, np.uint32)
    if fill == "corners":
        g = np.zeros(shape_zyx, np.uint32)
        for k, (z, y, x) in enumerate(itertools.product((0, nz - 1), (0, ny - 1), (0, nx - 1))):
            g[z, y, x] = 10 + k
        return g
    if fill == "solid":
        return rng.integers(1, 300, size=shape_zyx).astype(np.uint32)
    if fill == "big_ids":
        return np.where(rng.random(shape_zyx) < 0.2, rng.integers(65536, 2 ** 32, size=shape_zyx, dtype=np.uint64), 0).astype(np.uint32)
    p = 0.03 if fill == "sparse" else 0.5
    return np.where(rng.random(shape_zyx) < p, rng.integers(1, 300, size=shape_zyx), 0).astype(np.uint32)


def tie_rays(lo, hi, rng, count):
    """Origins on integer points — lattice planes, tile faces / edges / corners (grid corner + multiples of 8), the grid's own corners —
    and directions along exact diagonals (components of equal magnitude, or zero): the far planes of two or three axes tie at every cell."""
    lo, hi = np.asarray(lo), np.asarray(hi)
    org = rng.integers(lo - 3, hi + 4, size=(count, 3)).astype(np.float64)
    snap = rng.random((count, 3)) < 0.4
    tiles = lo + 8 * rng.integers(0, (hi - lo + 7) // 8 + 1, size=(count, 3))
    org[snap] = tiles[snap]
    corner = rng.random(count) < 0.15
    org[corner] = np.where(rng.random((int(corner.sum()), 3)) < 0.5, lo, hi)
    a = np.float32(1.0 / np.sqrt(3.0))
    b = np.float32(1.0 / np.sqrt(2.0))
    dirs = [(sx * a, sy * a, sz * a) for sx, sy, sz in SIGNS]
    dirs += [(sx * b, sy * b, 0) for sx in (1, -1) for sy in (1, -1)] + [(sx * b, 0, sz * b) for sx in (1, -1) for sz in (1, -1)]
    dirs += [(0, sy * b, sz * b) for sy in (1, -1) for sz in (1, -1)]
    dirs += [(1, 0, 0), (-1, 0, 0), (0, 1, 0), (0, -1, 0), (0, 0, 1), (0, 0, -1)]
    d = np.array(dirs, dtype=np.float64)[rng.integers(0, len(dirs), size=count)]
    towards = rng.random(count) < 0.5                          # half of them: the diagonal whose signs point at the grid's middle
    mid = 0.5 * (lo + hi)
    s = np.where(mid - org >= 0, 1.0, -1.0)
    d[towards] = np.abs(d[towards]) * s[towards]
    return make_rays(org, d, normalise=False)


def grid_rays(shape_zyx, origin, seed, count=160):
    """Random rays at and around the grid (a third from inside, a tenth pointing away), near-zero direction components, tie rays, and
    short / late intervals of some of them."""
    rng = np.random.default_rng(seed)
    nz, ny, nx = shape_zyx
    lo = np.asarray(origin, dtype=np.float64)
    ext = np.array([nx, ny, nz], dtype=np.float64)
    hi = lo + ext
    reach = ext.max() + 4.0
    org = rng.uniform(lo - reach, hi + reach, size=(count, 3))
    inside = rng.random(count) < 0.33
    org[inside] = rng.uniform(lo, hi, size=(int(inside.sum()), 3))
    tgt = rng.uniform(lo, hi, size=(count, 3))
    d = tgt - org
    away = rng.random(count) < 0.1
    d[away] *= -1.0
    # every octant, whatever the draw: eight rays through the middle
    mid = 0.5 * (lo + hi)
    oct_d = np.array(SIGNS) * rng.uniform(0.2, 1.0, size=(8, 3))
    rays = [make_rays(org, d), make_rays(mid - oct_d * reach, oct_d)]
    nz_org = rng.uniform(lo - 2.0, hi + 2.0, size=(len(NEAR_ZERO_DIRS) * 2, 3))
    nz_org[:, 1] = hi[1] + rng.uniform(0.0, 3.0, size=len(nz_org))                 # above the grid: those directions point down
    nz_org[::2, 0] = np.floor(nz_org[::2, 0]) + 0.5
    rays.append(make_rays(nz_org, np.array(NEAR_ZERO_DIRS * 2)))
    ties = tie_rays(lo.astype(np.int64), hi.astype(np.int64), rng, count)
    rays.append(ties)
    short = np.concatenate([rays[0][: count // 4], ties[: count // 4]])
    short["tmax"] = rng.uniform(0.5, reach, size=len(short)).astype(np.float32)
    late = np.concatenate([rays[0][count // 4: count // 2], ties[count // 4: count // 2]])
    late["tmin"] = rng.uniform(0.5, 2.5 * reach, size=len(late)).astype(np.float32)
    return np.concatenate(rays + [short, late])


# ---- scene64 -------------------------------------------------------------------------------------------------------------------------------
def test_scene64_edge_case_and_random_rays(scene64):
    cm, pw = scene64
    ids = W.scene_dense(64, SEED)
    rays = np.concatenate([edge_case_rays(), random_rays(64, 5000, 21)])
    assert octants(rays) == set(SIGNS)
    ref, ctr = O.Lattice(pw.nodes, pw.sub_chunks).trace(rays)
    hits, misses = check(ids, (0, 0, 0), rays, ref)
    assert hits == ctr["hits"] and hits > 3500 and misses > 650, (hits, misses)


@pytest.mark.parametrize("pose", [0, 1, 2])
def test_scene64_primary_rays(scene64, pose):
    cm, pw = scene64
    ids = W.scene_dense(64, SEED)
    cam = W.scene_camera(64, pose, 160, 120, SEED)
    ref, ctr = O.Lattice(pw.nodes, pw.sub_chunks).trace(O.primary_rays(cam, 160, 120))
    for global_bits in (False, True):
        assert records_equal(host_dense(ids, (0, 0, 0), global_bits).trace_primary(cam, 160, 120), ref).all(), global_bits
    assert ctr["hits"] > 5500 and ctr["rays"] - ctr["hits"] > 50, ctr


def test_scene64_jittered_primary_rays(scene64):
    """The kernel's pixel -> ray mapping with a TAA jitter, frame index 5: the oracle's rays under the same clip-space jitter."""
    cm, pw = scene64
    ids = W.scene_dense(64, SEED)
    cam = W.scene_camera(64, 1, 131, 77, SEED)
    j = W.taa_jitter(5)
    clip = (np.float32(2.0) * np.float32(j[0]) / np.float32(131), np.float32(2.0) * np.float32(j[1]) / np.float32(77))
    lat = O.Lattice(pw.nodes, pw.sub_chunks)
    plain, _ = lat.trace(O.primary_rays(cam, 131, 77))
    O.set_jitter_clip(j, 131, 77)
    try:
        ref, ctr = lat.trace(O.primary_rays(cam, 131, 77))
    finally:
        O.set_jitter_clip(None)
    assert not records_equal(ref, plain).all()                   # the jitter reaches the rays
    for global_bits in (False, True):
        assert records_equal(host_dense(ids, (0, 0, 0), global_bits).trace_primary(cam, 131, 77, jitter_clip=clip), ref).all(), global_bits
    assert ctr["hits"] > 5000 and ctr["rays"] - ctr["hits"] > 20, ctr


# ---- extents around a tile edge, every combination -------------------------------------------------------------------------------------------
# floors per fill level over the 125 shapes of one origin (hits, misses): the oracle reports 1.2 to 1.4 times as many (62 500 rays each)
SWEEP_FLOORS = {"empty": (0, 60000), "corners": (4000, 45000), "sparse": (4500, 45000), "half": (22000, 26000), "solid": (25000, 22000),
                "big_ids": (16000, 32000)}


def sweep(fill, origin, dims=DIMS):
    rng = np.random.default_rng(FILLS.index(fill) * 7 + (origin[0] != 0))
    hits = misses = 0
    seen = set()
    for k, (nx, ny, nz) in enumerate(itertools.product(dims, repeat=3)):
        ids = fill_grid((nz, ny, nx), fill, rng)
        rays = grid_rays(ids.shape, origin, 1000 + k)
        seen |= octants(rays)
        h, m = check(ids, origin, rays)
        hits += h
        misses += m
    assert seen == set(SIGNS)
    return hits, misses


@pytest.mark.parametrize("origin", ORIGINS, ids=["origin0", "negative"])
@pytest.mark.parametrize("fill", FILLS)
def test_every_extent_combination(fill, origin):
    hits, misses = sweep(fill, origin)
    if fill == "empty":
        assert hits == 0
    assert hits >= SWEEP_FLOORS[fill][0] and misses >= SWEEP_FLOORS[fill][1], (fill, origin, hits, misses)


# ---- int16 limits ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("origin,shape_zyx", [((-32768, -32768, -32768), (9, 17, 12)), ((32768 - 12, 32768 - 17, 32768 - 9), (9, 17, 12)),
                                              ((-32768, 32768 - 8, -4), (8, 8, 24))], ids=["lowest", "highest", "mixed"])
def test_grids_at_the_coordinate_limits(origin, shape_zyx):
    rng = np.random.default_rng(3)
    hits = misses = 0
    seen = set()
    for fill in ("corners", "half", "solid"):
        ids = fill_grid(shape_zyx, fill, rng)
        rays = grid_rays(shape_zyx, origin, 77, count=400)
        seen |= octants(rays)
        h, m = check(ids, origin, rays)
        hits += h
        misses += m
    assert seen == set(SIGNS)
    assert hits > 1000 and misses > 1600, (hits, misses)


# ---- ties, starts inside cells, intervals: one grid built for them ----------------------------------------------------------------------------
def tie_grid():
    """33 x 17 x 25 cells at (-8, 3, -16): a shell of filled cells round every tile corner region plus 8 % noise, so that diagonal rays meet
    filled cells right behind tile faces, edges and corners."""
    rng = np.random.default_rng(41)
    nz, ny, nx = 25, 17, 33
    g = np.where(rng.random((nz, ny, nx)) < 0.08, rng.integers(1, 200, size=(nz, ny, nx)), 0).astype(np.uint32)
    for z, y, x in itertools.product(range(7, nz, 8), range(7, ny, 8), range(7, nx, 8)):
        g[z:z + 2, y:y + 2, x:x + 2] = 500 + x                  # the eight cells round an interior tile corner
    g[12, 8, 4:12] = 700                                         # a bar across a tile face, x = 4..11
    return g, (-8, 3, -16)


def test_rays_built_to_tie():
    ids, origin = tie_grid()
    nz, ny, nx = ids.shape
    lo = np.array(origin)
    hi = lo + (nx, ny, nz)
    rng = np.random.default_rng(8)
    rays = tie_rays(lo, hi, rng, 6000)
    # through tile corners exactly: origins a whole number of diagonal steps before an interior tile corner, all eight diagonals
    a = np.float32(1.0 / np.sqrt(3.0))
    corners = np.array([lo + 8 * np.array(c) for c in itertools.product((1, 2, 3, 4), (1, 2), (1, 2, 3))], dtype=np.float64)
    through = [make_rays(corners - np.array(s) * k, np.tile(np.array(s) * a, (len(corners), 1)), normalise=False)
               for s in SIGNS for k in (1, 5, 8, 13, 40)]
    rays = np.concatenate([rays] + through)
    assert octants(rays) == set(SIGNS)
    hits, misses = check(ids, origin, rays)
    assert hits > 2500 and misses > 2500, (hits, misses)


def test_starts_inside_cells_and_intervals():
    ids, origin = tie_grid()
    nz, ny, nx = ids.shape
    lo = np.array(origin, dtype=np.float64)
    rng = np.random.default_rng(19)
    z, y, x = np.nonzero(ids)
    filled = np.stack([x, y, z], axis=1) + lo
    ze, ye, xe = np.nonzero(ids == 0)
    empty = np.stack([xe, ye, ze], axis=1) + lo
    n = 1500
    d = rng.normal(size=(n, 3))
    # origin strictly inside a filled cell: reported at t == tmin
    pick = filled[rng.integers(0, len(filled), size=n)]
    inside = make_rays(pick + rng.uniform(0.05, 0.95, size=(n, 3)), d)
    inside["tmin"][n // 2:] = rng.uniform(0.0, 0.04, size=n - n // 2).astype(np.float32)
    ref_inside = oracle_trace(ids, origin, inside)
    assert (ref_inside["hit"] == 1).all() and (ref_inside["t"] == inside["tmin"]).all()
    # origin on the min corner / faces of a filled cell (lattice planes), and of an empty one
    on_planes = make_rays(np.concatenate([pick[: n // 2], empty[rng.integers(0, len(empty), size=n // 2)]])
                          + np.where(rng.random((n, 3)) < 0.5, 0.0, 0.5), d)
    # tmax: ends inside the first reported cell (still a hit), inside an empty cell before it, and before the grid
    far = make_rays(pick + 0.5 - 60.0 * d / np.linalg.norm(d, axis=1, keepdims=True), d)
    t_hit = oracle_trace(ids, origin, far)
    assert t_hit["hit"].mean() > 0.9                                               # aimed at a filled cell's centre from outside
    ends_in_cell = far.copy(); ends_in_cell["tmax"] = np.where(t_hit["hit"] == 1, t_hit["t"] + np.float32(0.01), 5.0)
    ends_before = far.copy(); ends_before["tmax"] = np.where(t_hit["hit"] == 1, t_hit["t"] - np.float32(0.3), 5.0)
    ends_at = far.copy(); ends_at["tmax"] = np.where(t_hit["hit"] == 1, t_hit["t"], 5.0)      # tmax == entry: an empty interval
    before_grid = far.copy(); before_grid["tmax"] = 10.0
    beyond = far.copy(); beyond["tmin"] = 200.0                                    # tmin beyond the grid
    within = far.copy(); within["tmin"] = rng.uniform(40.0, 80.0, size=n).astype(np.float32)   # tmin inside the grid, any cell
    rays = np.concatenate([inside, on_planes, far, ends_in_cell, ends_before, ends_at, before_grid, beyond, within])
    assert octants(rays) == set(SIGNS)
    ref = oracle_trace(ids, origin, rays)
    sl = np.cumsum([0] + [n] * 9)
    part = {name: ref[sl[k]:sl[k + 1]] for k, name in enumerate(["inside", "on_planes", "far", "ends_in_cell", "ends_before", "ends_at", "before_grid",
                                                                  "beyond", "within"])}
    assert part["ends_in_cell"]["hit"].mean() > 0.9 and (part["before_grid"]["hit"] == 0).all() and (part["beyond"]["hit"] == 0).all()
    assert part["ends_before"]["hit"].sum() < part["far"]["hit"].sum() and part["ends_at"]["hit"].sum() < part["far"]["hit"].sum()
    hits, misses = check(ids, origin, rays, ref)
    assert hits > 5000 and misses > 5000, (hits, misses)


def test_ties_step_x_then_y_then_z():
    """The order in which tied far planes are crossed (x, then y, then z, as in the tree kernel) shows in no record: the cells in between
    have empty intervals whichever comes first.  It is pinned here through the harness's step log: a ray from a grid corner along an exact
    space diagonal ties all three planes at every tile and every cell on its way to the one filled voxel in the opposite corner."""
    a = np.float32(1.0 / np.sqrt(3.0))
    b = np.float32(1.0 / np.sqrt(2.0))
    for origin in ORIGINS:
        lo = np.array(origin, dtype=np.float64)
        for s in SIGNS:
            s = np.array(s)
            ids = np.zeros((24, 24, 24), np.uint32)
            far = np.where(s > 0, 23, 0)
            ids[far[2], far[1], far[0]] = 77
            ray = make_rays(lo + np.where(s > 0, 0, 24), s * a, normalise=False)
            ref = oracle_trace(ids, origin, ray)
            assert ref[0]["hit"] == 1 and tuple(ref[0]["voxel"]) == tuple((lo + far).astype(int))
            for global_bits in (False, True):
                rec, steps = host_dense(ids, origin, global_bits).trace_steps(ray[0])
                assert records_equal(np.array([rec]), ref).all()
                assert steps.tolist() == [0, 1, 2] * 9, (origin, s, steps)           # 2 empty tiles, then 7 cells of the last tile, each x, y, z
            # two planes tie (x and z; y never steps: direction 0 from y + 0.5)
            ids[:] = 0
            ids[far[2], 3, far[0]] = 78
            start = lo + np.where(s > 0, 0, 24)
            start[1] = lo[1] + 3.5
            ray = make_rays(start, (s[0] * b, 0.0, s[2] * b), normalise=False)
            ref = oracle_trace(ids, origin, ray)
            assert ref[0]["hit"] == 1
            rec, steps = host_dense(ids, origin, False).trace_steps(ray[0])
            assert records_equal(np.array([rec]), ref).all() and steps.tolist() == [0, 2] * 9, (origin, s, steps)


def test_single_tile_and_one_cell_thick_grids():
    """count == 1 in the tile-level bisection on one, two or three axes: 1 x 1 x 1 to 8 x 8 x 8 cells in one tile, slabs one cell thick."""
    rng = np.random.default_rng(2)
    hits = misses = 0
    for shape_zyx, origin in [((1, 1, 1), (0, 0, 0)), ((1, 1, 1), (-1, -1, -1)), ((8, 8, 8), (-8, 0, 8)), ((5, 3, 2), (2, -3, 1)),
                              ((1, 40, 1), (0, -20, 0)), ((1, 1, 40), (-7, 5, 5)), ((40, 1, 1), (3, 3, -33)), ((1, 23, 37), (-9, -9, -9)),
                              ((26, 1, 19), (100, 0, -100))]:
        for fill in ("solid", "half"):
            ids = fill_grid(shape_zyx, fill, rng)
            ids.flat[0] = 7
            h, m = check(ids, origin, grid_rays(shape_zyx, origin, 5, count=300))
            hits += h
            misses += m
    assert hits > 5500 and misses > 7000, (hits, misses)


def test_the_tiler_pads_with_empty_cells():
    """The cells beyond nx, ny, nz inside the last tiles hold 0 whatever lies next to the grid in memory: a solid grid cut out of a larger
    solid array (so a tiler reading past a row would pick up ids), rays through the padding only."""
    big = np.full((20, 20, 20), 9, np.uint32)
    ids = np.ascontiguousarray(big[:9, :7, :17])
    org = np.array([[17.5, 3.5, 30.0], [20.0, 7.5, 4.5], [-5.0, 7.5, 9.5], [17.2, 7.2, 9.2], [16.9, 6.9, 15.9]])
    d = np.array([[0, 0, -1], [-1, 0, 0], [1, 0, 0], [1, 1, 1], [-1e-3, -1e-3, -1]], dtype=np.float64)
    rays = make_rays(org, d)
    hits, misses = check(ids, (0, 0, 0), rays)
    assert misses == 4 and hits == 1                             # the last one grazes down the padding into the grid's top face


# ---- sanitizers ---------------------------------------------------------------------------------------------------------------------------
def test_dense_body_under_address_and_ub_sanitizers():
    """ASan + UBSan run of the body and the host tiler (the kernel itself has never run under a sanitizer): this file's own tests, a
    representative subset, with the shim's sanitizer build."""
    lib = H.build_dense(sanitize=True)
    code = f"""
import sys
sys.path.insert(0, {str(ROOT)!r})
from tests import harness_ffi as H
from tests.conftest import make_scene_world
import tests.test_dense_dda_cpu as T
T._lib = H.load_dense({str(lib)!r})
scene = make_scene_world(64)
T.test_scene64_edge_case_and_random_rays(scene)
T.test_scene64_primary_rays(scene, 1)
for fill in ("corners", "half", "solid"):
    print(fill, T.sweep(fill, (-13, -8, -21), dims=(1, 8, 9)))
T.test_grids_at_the_coordinate_limits((-32768, -32768, -32768), (9, 17, 12))
T.test_grids_at_the_coordinate_limits((32768 - 12, 32768 - 17, 32768 - 9), (9, 17, 12))
T.test_rays_built_to_tie()
T.test_ties_step_x_then_y_then_z()
T.test_starts_inside_cells_and_intervals()
T.test_single_tile_and_one_cell_thick_grids()
T.test_the_tiler_pads_with_empty_cells()
print('done')
"""
    env = dict(os.environ)
    env["LD_PRELOAD"] = subprocess.run(["g++", "-print-file-name=libasan.so"], capture_output=True, text=True).stdout.strip()
    env["ASAN_OPTIONS"] = "detect_leaks=0"
    proc = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, env=env, timeout=1500)
    assert proc.returncode == 0, proc.stdout[-1000:] + proc.stderr[-3000:]
    assert "done" in proc.stdout and "runtime error" not in proc.stderr and "AddressSanitizer" not in proc.stderr
