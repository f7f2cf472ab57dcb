"""The content and the case table of the automaton tests (tests/test_automaton_cpu.py, tests/test_automaton_gpu.py) — TESTS ONLY.
A case is a box with its content, a region (world voxels, None = the whole box) and a rule; the expected result is
tests/automaton_reference.py's, computed once per case and shared."""
from __future__ import annotations

import functools

import numpy as np

from blok_amd import automaton as A
from tests import automaton_reference as R
from tests import limit_cases as LC

HOUSE_ORIGIN, HOUSE_SHAPE = (-37, -21, 13), (88, 52, 44)          # odd origin, x across a 64-cell boundary
LONG_SHAPE = (272, 12, 12)                                         # a row of 68 bricks: a wave seam falls inside it
RAGGED_SHAPE = (20, 24, 41)                                        # a ragged last brick along z
LIMIT_SHAPE = (40, 36, 33)
SLAB_SHAPE = (40, 48, 24)                                          # thick slabs: bricks whose 27 words are all ones, or all 0 (every cell at count 0, or at the neighbourhood's size)
BOXES = {"house": (HOUSE_ORIGIN, HOUSE_SHAPE), "long": ((-131, 5, -9), LONG_SHAPE), "ragged": ((3, -5, 7), RAGGED_SHAPE),
         "high": (LC.limit_origin("HIGH", LIMIT_SHAPE), LIMIT_SHAPE), "slabs": ((-9, 3, 11), SLAB_SHAPE)}
SEED = 20261


def tie_cell(shape):
    """Box-local (x, y, z) of the planted tie, in the empty slab (boxes with 25 rows or more along y hold it)."""
    return shape[0] // 3, (28 if shape == SLAB_SHAPE else (2 * shape[1]) // 3) + 2, shape[2] // 3


@functools.lru_cache(maxsize=None)
def content(shape, seed=SEED):
    """[z][y][x] (density, ids) of a box of `shape` (x, y, z): 45 % noise with ids 5 .. 8; a slab of filled and a slab of empty rows along y;
    NaN, negative and zero densities among the empty cells and non-zero stale ids in a fifth of them; and, where the slab is thick enough, an
    empty cell (tie_cell) in the empty slab whose only two neighbours carry the ids 8 and 5."""
    nx, ny, nz = shape
    rng = np.random.default_rng(seed)
    filled = rng.random((nz, ny, nx)) < 0.45
    y0, y1 = ny // 6, ny // 6 + max(ny // 5, 2)
    e0, e1 = (2 * ny) // 3, (2 * ny) // 3 + max(ny // 5, 2)
    if shape == SLAB_SHAPE:                                        # five bricks of rock below, five of air above, noise between
        y0, y1, e0, e1 = 0, 20, 28, ny
    filled[:, y0:y1, :] = True                                     # all filled
    filled[:, e0:e1, :] = False                                    # all empty
    ids = np.where(filled, rng.integers(5, 9, filled.shape), 0).astype(np.uint32)
    d = np.where(filled, rng.choice(np.array([1.0, 0.25, 3.5], np.float32), filled.shape), 0).astype(np.float32)
    kinds = rng.integers(0, 4, filled.shape)
    d = np.where(~filled & (kinds == 1), np.float32(np.nan), d)
    d = np.where(~filled & (kinds == 2), np.float32(-1.5), d)
    d = np.where(~filled & (kinds == 3), np.float32(-0.0), d).astype(np.float32)
    stale = ~filled & (rng.random(filled.shape) < 0.2)
    ids = np.where(stale, rng.integers(1, 10, filled.shape), ids).astype(np.uint32)      # below, among and above the ids that vote
    x, y, z = tie_cell(shape)
    if e1 - e0 >= 5:
        d[z, y, x - 1], ids[z, y, x - 1] = 1.0, 8
        d[z, y + 1, x], ids[z, y + 1, x] = 1.0, 5
    d.setflags(write=False); ids.setflags(write=False)
    return d, ids


def world(origin, local):
    return tuple(int(origin[a]) + int(local[a]) for a in range(3))


def regions(box):
    """name -> (lo, hi), box-local, of the box."""
    nx, ny, nz = BOXES[box][1]
    if box == "house":
        return {"whole": None, "inner": ((4, 4, 4), (84, 48, 40)), "unaligned": ((5, 6, 7), (81, 46, 39)), "cell": ((33, 17, 9), (34, 18, 10)),
                "column": ((64, 0, 8), (68, ny, 12)), "empty": ((10, 10, 10), (10, 20, 20))}
    hi = tuple(max(v for v in range(n) if v % 4 == a + 1) for a, n in enumerate((nx, ny, nz)))
    return {"whole": None, "unaligned": ((5, 2, 3), hi)}           # lo, hi = 1, 2, 3 mod 4 on the three axes


def majority(nb, solid):
    return A.rule(nb, A.at_least((nb + 1) // 2, nb), A.at_least(nb // 2 + 1, nb), box_is_solid=solid)


# name -> rule; the kernel path a rule is here for stands beside it
def house_rules():
    rules = {
        "smooth": A.smooth(1), "smooth x3": A.smooth(3),
        "despeckle": A.despeckle(), "despeckle x5": A.rule(6, A.at_least(1, 6), 0, steps=5),      # stops at step 2
        "fill pits x2": A.fill_pits(2),
        "life 4555 x8": A.life((4, 5), (5,), steps=8),
        "births at 0": A.rule(6, A.at_least(0, 6), 1, material=77),                            # no-voter births, a write of every isolated empty cell
        "births at 0, solid": A.rule(26, A.at_least(0, 26), A.bits((0, 26)), material=78, box_is_solid=True),
        "nobody survives": A.rule(26, 0, 0),
        "nothing happens": A.rule(6, A.at_least(0, 6), 0, steps=4),                            # a fixed point: steps_run 1, nothing written
        "fixed material": A.rule(18, A.at_least(6, 18), A.at_least(8, 18), steps=2, material=0xFFFFFFFF, fixed_material=True),
    }
    for nb in A.NEIGHBOURHOODS:
        if nb == 6:                                                                            # (18 and 26 dilate the regions and the other boxes)
            rules[f"dilate {nb}"] = A.dilate(nb, density=2.5)
        rules[f"erode {nb}"] = A.erode(nb)
        for solid in (False, True):                                                            # outside-solid bricks and ragged ends
            rules[f"majority {nb}{' solid' if solid else ''}"] = majority(nb, solid)
    return rules


FIXED_POINTS = {"nothing happens"}
VOTING = lambda r: int(r["birth"][0]) != 0 and not (int(r["flags"][0]) & A.FIXED_MATERIAL)
TOGGLE = A.rule(6, 0, A.at_least(0, 6), steps=3)                  # a filled cell dies, an empty one is born: every step changes a one-cell region


@functools.lru_cache(maxsize=None)
def table():
    """The cases, in an order that keeps a box's cases together: dicts of name, box, origin, shape, lo, hi (world, or None), rule."""
    out = []

    def add(box, rule_name, rule, region_name):
        origin, shape = BOXES[box]
        reg = regions(box)[region_name]
        lo, hi = (None, None) if reg is None else (world(origin, reg[0]), world(origin, reg[1]))
        out.append({"name": f"{box}/{region_name}/{rule_name}", "box": box, "origin": origin, "shape": shape, "lo": lo, "hi": hi, "rule": rule,
                    "rule_name": rule_name, "region": region_name})

    for name, rule in house_rules().items():
        add("house", name, rule, "whole")
    for region in ("inner", "unaligned", "column", "empty"):                                   # the region cut inside a brick: unaligned, column
        add("house", "smooth x2", A.smooth(2), region)
        add("house", "dilate 18", A.dilate(18), region)
    add("house", "toggle x3", TOGGLE, "cell")
    for box in ("long", "ragged", "high"):                                                     # the wave seam; the ragged brick; the lattice's end
        for region in ("whole", "unaligned"):
            add(box, "smooth x2", A.smooth(2), region)
            add(box, "majority 18 solid", majority(18, True), region)
            add(box, "dilate 26", A.dilate(26), region)
            add(box, "erode 6", A.erode(6), region)
    for region in ("whole", "unaligned"):                                                      # bricks of 27 equal words, at both counts
        for name in ("smooth x3", "births at 0, solid", "nobody survives", "majority 18 solid", "dilate 6", "erode 26"):
            add("slabs", name, house_rules()[name], region)
    return out


def cases_of(box):
    return [c for c in table() if c["box"] == box]


@functools.lru_cache(maxsize=None)
def _expected(name):
    c = next(c for c in table() if c["name"] == name)
    d, m = content(c["shape"])
    got = R.run(d, m, c["origin"], c["lo"], c["hi"], c["rule"])
    for a in got[:4]:
        a.setflags(write=False)
    return got


def expected(c):
    """(d, m, info, step_counts, ties) of the reference, computed once per case."""
    return _expected(c["name"])
