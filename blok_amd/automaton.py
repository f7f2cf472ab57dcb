"""Neighbour-count rules on the CPU (blok_automaton_voxels): the host build of HipTracer.volume_automaton, the rule record, and the
presets as plain data.  A rule is one _ffi.AUTOMATON_RULE record: `survive` and `birth` are bit sets over the count of filled neighbours
(bit n: a filled cell with n filled neighbours stays / an empty cell with n becomes filled)."""
from __future__ import annotations

import ctypes as C

import numpy as np

from . import _ffi
from ._ffi import BlokError

BOX_IS_SOLID = _ffi.AUTOMATON_BOX_IS_SOLID
FIXED_MATERIAL = _ffi.AUTOMATON_FIXED_MATERIAL
RULE = _ffi.AUTOMATON_RULE
INFO = _ffi.AUTOMATON_INFO
NEIGHBOURHOODS = (6, 18, 26)


def _vec(v):
    return None if v is None else (C.c_int32 * 3)(*[int(c) for c in v])


def at_least(k: int, n: int) -> int:
    """The bit set of the counts k .. n of a neighbourhood of n cells."""
    return sum(1 << c for c in range(max(int(k), 0), int(n) + 1))


def bits(counts) -> int:
    """The bit set of the listed counts."""
    return sum(1 << int(c) for c in set(counts))


def rule(neighbourhood: int, survive: int, birth: int, steps: int = 1, density: float = 1.0, material: int = 0, box_is_solid: bool = False,
         fixed_material: bool = False) -> np.ndarray:
    r = np.zeros(1, dtype=RULE)
    r["neighbourhood"], r["survive"], r["birth"], r["steps"] = int(neighbourhood), int(survive), int(birth), int(steps)
    r["flags"] = (BOX_IS_SOLID if box_is_solid else 0) | (FIXED_MATERIAL if fixed_material else 0)
    r["density"], r["material"] = float(density), int(material)
    return r


# ---- presets ---------------------------------------------------------------------------------------------------------------------------------
def smooth(steps: int = 1, **kw) -> np.ndarray:
    """The majority of the 26 neighbours: survive at 13 or more, born at 14 or more."""
    return rule(26, at_least(13, 26), at_least(14, 26), steps, **kw)


def despeckle(**kw) -> np.ndarray:
    """Drops the voxels without a face neighbour."""
    return rule(6, at_least(1, 6), 0, **kw)


def fill_pits(steps: int = 1, **kw) -> np.ndarray:
    """Fills the empty cells with five or six filled face neighbours."""
    return rule(6, at_least(0, 6), at_least(5, 6), steps, **kw)


def dilate(neighbourhood: int = 6, steps: int = 1, **kw) -> np.ndarray:
    return rule(neighbourhood, at_least(0, neighbourhood), at_least(1, neighbourhood), steps, **kw)


def erode(neighbourhood: int = 6, steps: int = 1, **kw) -> np.ndarray:
    """A filled cell with an empty neighbour goes (the outside of the box is empty unless box_is_solid)."""
    return rule(neighbourhood, 1 << neighbourhood, 0, steps, **kw)


def life(survive_set, birth_set, neighbourhood: int = 26, steps: int = 1, **kw) -> np.ndarray:
    """A Life-like rule from the two lists of counts, e.g. life((4, 5), (5,)) for "4555"."""
    return rule(neighbourhood, bits(survive_set), bits(birth_set), steps, **kw)


def check(r) -> str:
    """The text of the rule `r` fails (blok_automaton_check), or '' for a rule that passes."""
    r = np.ascontiguousarray(r, dtype=RULE).reshape(1)
    err = C.create_string_buffer(128)
    return "" if _ffi.host_lib().blok_automaton_check(_ffi.ptr(r), err, len(err)) == 0 else err.value.decode()


def automaton_host(density, material_ids, r, origin=(0, 0, 0), lo=None, hi=None):
    """blok_automaton_voxels over [z][y][x] arrays of a box at world `origin`; the region in world voxels (both corners None = the whole
    box).  Returns (density, material_ids, info, step_counts): new arrays, one INFO record, a [steps][2] uint64 array (born, died)."""
    d = np.array(density, dtype=np.float32, order="C")
    m = np.array(material_ids, dtype=np.uint32, order="C")
    assert d.ndim == 3 and m.shape == d.shape, "the arrays are [z][y][x] over the whole box"
    nz, ny, nx = d.shape
    info = np.zeros(1, dtype=INFO)
    counts, r_ptr = None, None
    if r is not None:
        r = np.ascontiguousarray(r, dtype=RULE).reshape(1)
        r_ptr = _ffi.ptr(r)
        counts = np.zeros((min(max(int(r["steps"][0]), 1), 255), 2), dtype=np.uint64)
    rc = _ffi.host_lib().blok_automaton_voxels(_ffi.ptr(d) if d.size else None, _ffi.ptr(m) if m.size else None, _vec(origin), nx, ny, nz, _vec(lo), _vec(hi), r_ptr,
                                               None if counts is None else _ffi.ptr(counts), _ffi.ptr(info))
    if rc != 0:
        raise BlokError(rc, "blok_automaton_voxels")
    return d, m, info, counts
