"""Shared by the terrain tests: the parameter set of the contract's quoted values, as a TerrainParams record and as the dict the numpy
reference takes, and seeded prior content for a box."""
from __future__ import annotations

import numpy as np

from blok_amd import _ffi

FIELDS = [f for f, _ in _ffi.TerrainParams._fields_]
ISSUE = dict(seed=0xB10C0001, base_height=-20, amplitude=48, height_cell_log2=5, height_octaves=4, cave_cell_log2=4, cave_octaves=2,
             cave_threshold=24000, cave_roof=3, soil_depth=3, ore_cell_log2=3, ore_threshold=52000, surface_material=1, soil_material=2,
             rock_material=3, ore_material=4, density=1.5, flags=0)


def params(**kw):
    d = dict(ISSUE, **kw)
    p = _ffi.TerrainParams()
    for k, v in d.items():
        setattr(p, k, v)
    return p, d


def prior(shape_zyx, seed=3):
    rng = np.random.default_rng(seed)
    d = np.where(rng.random(shape_zyx) < 0.1, rng.uniform(0.1, 2.0, shape_zyx), 0.0).astype(np.float32)
    return d, np.where(d > 0, rng.integers(5, 9, shape_zyx), 0).astype(np.uint32)
