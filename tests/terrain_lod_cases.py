"""Shared by the tests of terrain_reduce (blok_terrain_reduce on the host, HipTracer.terrain_reduce on the device): the case table, and the
reference every comparison uses — terrain.eval_box into arrays, then lod.reduce_host over them, which tests/test_lod_cpu.py pins to the
numpy model of the reduce.  Without SEAMLESS the arrays are the region's own box; with it they are the region grown by one voxel on every
side, reduced over the region with the flag taken off, and the info's flags put back.  References are computed once and shared."""
from __future__ import annotations

import functools

import numpy as np

from blok_amd import lod as HL
from blok_amd import terrain as HT
from tests import terrain_cases as TC

VOTE_EXPOSED, SEAMLESS = HL.VOTE_EXPOSED, HL.SEAMLESS
ALL_FLAGS = (0, VOTE_EXPOSED, SEAMLESS, VOTE_EXPOSED | SEAMLESS)
ALL_LEVELS = (1, 3, 5)
# = terrain_lod::kTileX, kSlab, kTileZ (csrc/common/terrain_lod_core.h): the voxels of a workgroup's tile along x, y and z
TILE = (64, 64, 16)
FAR = (1 << 30) - 70

LARGE = {
    "large_a": ((-37, -41, -29), (59, 39, 35)),
    "large_b": ((-8, -24, -8), (8, 30, 8)),
    "large_c": ((1, -33, -65), (130, 31, -1)),
}


def _edge_cases():
    """Per axis a region whose extent is the tile's edge - 1, + 0 and + 1 at an odd origin, small on the other axes."""
    out = {}
    base_lo, base_hi = (-31, -15, -9), (-25, 1, -3)          # (rows that cross the surface)
    for axis, name in enumerate("xyz"):
        for d in (-1, 0, 1):
            lo, hi = list(base_lo), list(base_hi)
            hi[axis] = lo[axis] + TILE[axis] + d
            out[f"edge_{name}{TILE[axis] + d}"] = (tuple(lo), tuple(hi))
    return out


REGIONS = dict(LARGE)
REGIONS.update({
    "column": ((-3, -20, 5), (-2, 28, 6)),
    "above": ((-10, 29, -10), (23, 61, 9)),              # wholly above the surface: all zeros
    "deep": ((5, -215, -7), (45, -160, 20)),             # wholly below y = -150: no surface, caves and ore alone
    "one_x": ((-5, -30, 3), (-4, 20, 40)),
    "one_y": ((-20, -5, -9), (21, -4, 12)),
    "one_z": ((3, -30, -5), (40, 20, -4)),
    "empty_y": ((0, 0, 0), (8, 0, 8)),
    "far_x": ((FAR, -30, 11), (1 << 30, 12, 30)),
})
REGIONS.update(_edge_cases())
VARIANT_REGION = ((-13, -40, -11), (20, 30, 14))
VARIANTS = {"no_caves": dict(cave_octaves=0), "no_ore": dict(ore_threshold=65536), "surface_is_soil": dict(surface_material=2)}


def cases():
    """(name, params overrides, lo, hi)."""
    return [(name, {}, lo, hi) for name, (lo, hi) in REGIONS.items()] + [(name, kw, *VARIANT_REGION) for name, kw in VARIANTS.items()]


CASES = cases()
CASE_IDS = [c[0] for c in CASES]


def params_of(kw):
    return TC.params(**kw)[0]


@functools.lru_cache(maxsize=None)
def _arrays(kw_items, lo, hi, grow):
    p = params_of(dict(kw_items))
    d, m, _ = HT.eval_box(p, tuple(c - grow for c in lo), tuple(c + grow for c in hi))
    d.setflags(write=False)
    m.setflags(write=False)
    return d, m


@functools.lru_cache(maxsize=None)
def _reference(kw_items, lo, hi, levels, flags):
    grow = 1 if flags & SEAMLESS else 0
    d, m = _arrays(kw_items, lo, hi, grow)
    if grow:
        planes, info = HL.reduce_host(d, m, tuple(c - 1 for c in lo), lo, hi, levels, flags & VOTE_EXPOSED)
        info["flags"] = flags
    else:
        planes, info = HL.reduce_host(d, m, lo, None, None, levels, flags)
    for level in planes:
        for plane in level:
            plane.setflags(write=False)
    info.setflags(write=False)
    return planes, info


def reference(kw, lo, hi, levels, flags):
    """(levels, info) of the composition, shared and read-only."""
    return _reference(tuple(sorted(kw.items())), tuple(lo), tuple(hi), int(levels), int(flags))


def voxel_ids(kw, lo, hi):
    """The material ids of the region's filled voxels (the reference's arrays)."""
    d, m = _arrays(tuple(sorted(kw.items())), tuple(lo), tuple(hi), 0)
    return m[d > 0]


def same(got, want, tag=""):
    """(levels, info) pairs equal byte for byte."""
    assert got[1].tobytes() == want[1].tobytes(), f"{tag}: info {got[1]} != {want[1]}"
    assert len(got[0]) == len(want[0])
    for j, (g, w) in enumerate(zip(got[0], want[0]), start=1):
        for plane, (a, b) in enumerate(zip(g, w)):
            assert a.dtype == b.dtype and a.shape == b.shape, f"{tag}: level {j} plane {plane}: {a.dtype} {a.shape} != {b.dtype} {b.shape}"
            assert a.tobytes() == b.tobytes(), f"{tag}: level {j} plane {plane}: {int((a != b).sum())} of {a.size} cells differ"


def check_reference_tells_the_flags_apart():
    """Conditions on the reference alone, so that a product that ignores a flag cannot pass: on the three large regions all four material
    ids occur, VOTE_EXPOSED changes the id plane at every level up to 3, and SEAMLESS changes the e plane at level 1."""
    for name, (lo, hi) in LARGE.items():
        assert set(np.unique(voxel_ids({}, lo, hi)).tolist()) == {1, 2, 3, 4}, name
        plain, voted = reference({}, lo, hi, 3, 0)[0], reference({}, lo, hi, 3, VOTE_EXPOSED)[0]
        for j in range(3):
            assert (plain[j][2] != voted[j][2]).any(), (name, j + 1)
        assert (reference({}, lo, hi, 1, 0)[0][0][1] != reference({}, lo, hi, 1, SEAMLESS)[0][0][1]).any(), name
