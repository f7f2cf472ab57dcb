"""GPU: the shadow rays' last-occluder map (beam.h: prism_far; api.hip: rebuild_sun_map, update_sun_map) as NUMBERS, texel by texel,
against tests/bounds_reference.py — not through the frames it leaves unchanged.

Two invariants.  VALID, always: map >= lo - delta at every texel, lo = the largest far(voxel) over the voxels a correct search must keep.
TIGHT, for a fresh map and for every texel the tightening bands have passed: also map <= hi + delta, hi over the voxels a correct search
may keep, and map == -kBeamNone exactly where that set is empty.  delta is derived in tests/bounds_reference.py (8 ulp of the largest plane
value: 6e-5 for a 64-cube near the origin, 0.031 at the ends of the int16 lattice); every test prints the largest deviation from the
nearer bound it saw, in voxels and in units of its delta.

Measured on an MI355X, largest deviation beyond the nearer reference bound: fresh maps 9.5e-6 voxel (64^3 scene, 0.16 delta), 6.2e-6
(64-cube volume, 0.10 delta), 3.0e-5 (256-cube, 0.12 delta); after the bands have drained 4.0e-5 (0.16 delta).  Loose texels after one
filling edit stand 4 - 84 voxels above hi, as the raise intends.
What these tests found on their first run: 16 of the 4962 bound-holding texels of the 64^3 scene stood up to 18.99 voxels ABOVE hi, 6 of a
small volume up to 4.55, 5 at either end of the lattice up to 21.9 — beam_search widened the stacked low candidate word as the signed int
the readlane builtin returns, so a word with bit 31 set made all 32 high lanes candidates of a revisited node (beam.h, fixed with this
module).  Conservative, hence invisible to every image test."""
from __future__ import annotations

import numpy as np
import pytest

from blok_amd import _ffi
from blok_amd import stamp as ST
from blok_amd import world as W
from tests import bounds_reference as B
from tests import limit_cases as LC
from tests.conftest import SEED

pytestmark = pytest.mark.gpu

LAYOUTS = pytest.mark.parametrize("keyed", [True, False], ids=["keyed", "general"])
NONE32 = np.float32(-B.K_BEAM_NONE)
ORIGIN = (-37, 5, -90)


def tracer(keyed=True):
    from blok_amd.tracer import HipTracer
    t = HipTracer(64, 64).init()
    t.set_volume_layout(keyed)
    return t


@pytest.fixture(scope="module")
def mats():
    return W.scene_materials(SEED)


def sparse_content(shape, seed, fill=0.004, top=None):
    """[z][y][x] density and ids: a random sprinkle below `top` (box-local y), a filled cell in each of the box's eight corners' columns
    at the bottom, never changed."""
    nx, ny, nz = shape
    rng = np.random.default_rng(seed)
    f = rng.random((nz, ny, nx)) < fill
    if top is not None:
        f[:, top:, :] = False
    for z in (0, nz - 1):
        for x in (0, nx - 1):
            f[z, 0, x] = True
    d = f.astype(np.float32)
    m = np.where(f, 1 + rng.integers(0, 200, size=f.shape), 0).astype(np.uint32)
    return d, m


def filled(t, origin):
    d, _ = t.volume_download()
    with np.errstate(invalid="ignore"):
        return B.voxels_of(d > 0, origin)


class Verdict:
    """The map as downloaded, held against the reference for `voxels`."""

    def __init__(self, t, voxels):
        info, self.texels = t.sun_map()
        self.info = info[0]
        assert int(self.info["has_map"]) == 1 and self.texels is not None
        st = t.world_stats()
        self.cube = B.cube_of(None, [int(c) for c in st.origin], int(st.levels))
        self.delta = B.sun_delta(self.info, *self.cube)
        self.lo, self.hi = B.sun_map_bounds(voxels, self.info, self.delta)
        self.map = self.texels.astype(np.float64)
        self.below = self.lo - self.map                                 # > delta: invalid
        self.above = np.where(self.hi > -B.K_BEAM_NONE, self.map - self.hi, 0.0)      # > delta: not tight

    def report(self, tag, where=None):
        w = np.ones(self.map.shape, bool) if where is None else where
        worst_below = float(self.below[w].max(initial=-np.inf))
        finite = w & (self.map < B.K_BEAM_NONE)
        worst_above = float(self.above[finite].max(initial=-np.inf))
        dev = max(worst_below, worst_above, 0.0)
        print(f"[sun map] {tag}: {self.map.shape[1]} x {self.map.shape[0]} texels of {float(self.info['texel']):g}, delta {self.delta:.3g}; "
              f"largest deviation beyond the nearer bound {dev:.3g} voxel = {dev / self.delta:.2f} delta"
              f" (map - lo >= {-worst_below:.3g}, map - hi <= {worst_above:.3g})")

    def assert_valid(self, tag, where=None):
        w = np.ones(self.map.shape, bool) if where is None else where
        bad = w & ~(self.below <= self.delta)
        assert not bad.any(), (tag, "texels too low", int(bad.sum()), np.argwhere(bad)[:4].tolist(), float(self.below[bad].max()))

    def assert_tight(self, tag, where=None):
        w = np.ones(self.map.shape, bool) if where is None else where
        self.report(tag, w)
        self.assert_valid(tag, w)
        empty = self.hi <= -B.K_BEAM_NONE
        bad = w & ~empty & ~(self.above <= self.delta)
        assert not bad.any(), (tag, "texels too high", int(bad.sum()), np.argwhere(bad)[:4].tolist(), float(self.above[bad].max()))
        assert (self.texels[w & empty] == NONE32).all(), (tag, "a texel no voxel can reach holds a bound")
        assert (self.texels[w & (self.lo > -B.K_BEAM_NONE)] > NONE32).all(), tag

    def reached(self, lo, hi, margin_texels=0):
        """Mask of the texels whose prism, grown by kBeamSlack + delta and by `margin_texels` texels, meets the box [lo, hi) of world voxels."""
        corners = np.array([[(hi if (c >> a) & 1 else lo)[a] for a in range(3)] for c in range(8)], dtype=np.float64)
        u, v, _ = B.frame_vectors(self.info)
        grow = B.K_BEAM_SLACK + self.delta + margin_texels * float(self.info["texel"])
        nv, nu = self.map.shape
        iu0, iu1 = B.texel_range(np.array([(corners @ u).min()]), np.array([(corners @ u).max()]), float(self.info["u0"]), float(self.info["texel"]), nu, grow)
        iv0, iv1 = B.texel_range(np.array([(corners @ v).min()]), np.array([(corners @ v).max()]), float(self.info["v0"]), float(self.info["texel"]), nv, grow)
        m = np.zeros((nv, nu), bool)
        m[int(iv0[0]):int(iv1[0]) + 1, int(iu0[0]):int(iu1[0]) + 1] = True
        return m


# ---- fresh maps are tight at every texel --------------------------------------------------------------------------------------------------
def test_fresh_map_of_the_scene_is_tight(scene64):
    cm, pw = scene64
    t = tracer()
    t.add_world(pw)
    v = Verdict(t, B.voxels_of(W.scene_dense(64, SEED) != 0, (0, 0, 0)))
    assert float(v.info["texel"]) == 1.0 and int(v.info["loose_edits"]) == 0 and int(v.info["tighten_pending"]) == 0
    v.assert_tight("64^3 scene")
    t.shutdown()


@LAYOUTS
def test_fresh_map_of_a_resident_volume_is_tight(keyed, mats):
    shape = (50, 41, 45)
    d, m = sparse_content(shape, 11, fill=0.02)
    t = tracer(keyed)
    t.volume_create(ORIGIN, shape, 128, 1.0)
    t.volume_upload(d, m)
    t.volume_rebuild(mats)
    Verdict(t, B.voxels_of(d > 0, ORIGIN)).assert_tight(f"volume at {ORIGIN}")
    t.shutdown()


@pytest.mark.parametrize("which", ["LOW", "HIGH"])
def test_fresh_map_at_the_ends_of_the_lattice_is_tight(which, mats):
    """Where the plane values are largest (about 57 000: delta is 8 ulp = 0.031 voxel) and the reference's two sets differ the most."""
    origin = LC.limit_origin(which, LC.SHAPE)
    d, m = sparse_content(LC.SHAPE, 12, fill=0.003)
    d[-1, -1, -1], m[-1, -1, -1] = 1.0, 3                            # the corner on the lattice's end (HIGH) / the box's far corner
    t = tracer()
    t.volume_create(origin, LC.SHAPE, 128, 1.0)
    t.volume_upload(d, m)
    t.volume_rebuild(mats)
    Verdict(t, B.voxels_of(d > 0, origin)).assert_tight(f"box at the {which} end")
    t.shutdown()


def test_a_world_of_voxel_size_two_has_no_map(mats):
    cm = W.ChunkManager(128, 2.0)
    rng = np.random.default_rng(4)
    xyz = rng.integers(-20, 30, size=(300, 3)).astype(np.int32)
    cm.set_voxels(xyz, rng.integers(1, 200, size=len(xyz)).astype(np.uint32))
    cm.rebuild_dirty_chunks()
    t = tracer()
    t.set_voxel_size(2.0)
    t.add_world(cm.pack_chunks_to_gpu_svo(mats))
    info, texels = t.sun_map()
    assert int(info["has_map"][0]) == 0 and texels is None and int(info["nu"][0]) == 0
    t.shutdown()
    t = tracer()                                                      # and no world at all
    info, texels = t.sun_map()
    assert int(info["has_map"][0]) == 0 and texels is None
    t.shutdown()


def test_coarse_texels_are_tight_and_cover_the_cube(mats):
    """1100 cells along x: the tree's cube is 4096, its projection wider than 2048 texels of one voxel."""
    shape, origin = (1100, 6, 7), (-500, 3, -2)
    rng = np.random.default_rng(6)
    f = np.zeros(shape[::-1], bool)
    for x0 in (0, 540, 1100 - 12):                                   # both ends and the middle
        f[:, :, x0:x0 + 12] = rng.random((shape[2], shape[1], 12)) < 0.25
    f[0, 0, 0] = f[-1, -1, -1] = True
    assert 200 < int(f.sum()) < 600
    t = tracer()
    t.volume_create(origin, shape, 128, 1.0)
    t.volume_upload(f.astype(np.float32), f.astype(np.uint32) * 5)
    st = t.volume_rebuild(mats)
    assert int(st.levels) == 6
    v = Verdict(t, B.voxels_of(f, origin))
    assert float(v.info["texel"]) > 1.0
    u, w, _ = B.frame_vectors(v.info)
    corners = v.cube[0] + B.CORNERS * v.cube[1]
    for axis, x0, n in ((u, "u0", "nu"), (w, "v0", "nv")):
        i = np.floor((corners @ axis - float(v.info[x0])) / float(v.info["texel"]))
        assert i.min() >= 0 and i.max() <= int(v.info[n]) - 1, (x0, i.min(), i.max(), int(v.info[n]))
    v.assert_tight("1100 x 6 x 7 box, cube 4096")
    t.shutdown()


# ---- a filling edit leaves the map valid everywhere, at once -----------------------------------------------------------------------------
CUBE = (64, 64, 64)                                                   # the box is the tree's cube: its corners project onto the map's rim
TOP = 20                                                              # the base content stays below this height; the edits build above it


def corner_lo(corner, size):
    """World low corner of a box of `size` cells flush in corner number `corner` (bit a set: the high end of axis a) of the cube."""
    return tuple(ORIGIN[a] + (CUBE[a] - size[a] if (corner >> a) & 1 else 0) for a in range(3))


def box_cells(lo, size):
    g = np.stack(np.meshgrid(*[np.arange(lo[a], lo[a] + size[a]) for a in range(3)], indexing="ij"), axis=-1).reshape(-1, 3)
    return g.astype(np.int32)


def edit_upload(t, d, m):
    """A whole-box upload of taller geometry: a tower in the corner (high x, high y, high z)."""
    d, m = d.copy(), m.copy()
    d[-3:, TOP:, -3:], m[-3:, TOP:, -3:] = 1.0, 7
    t.volume_upload(d, m)
    return ORIGIN, tuple(ORIGIN[a] + CUBE[a] for a in range(3))


def edit_set_voxels(t, d, m):
    size = (2, 30, 3)
    lo = corner_lo(0b010, size)                                       # low x, high y, low z
    cells = box_cells(lo, size)
    t.volume_set_voxels(cells, np.full(len(cells), 9, np.uint32), np.ones(len(cells), np.float32))
    return lo, tuple(lo[a] + size[a] for a in range(3))


def edit_brush(t, d, m):
    c = (ORIGIN[0] + CUBE[0] - 2.5, ORIGIN[1] + CUBE[1] - 2.5, ORIGIN[2] + 2.5)      # high x, high y, low z: its box ends on three faces
    t.volume_apply_brush(c, 2.49, 1.0, 0)
    return tuple(int(np.floor(x - 2.49)) for x in c), tuple(int(np.floor(x + 2.49)) + 1 for x in c)


def edit_stamp(t, d, m):
    size = (3, 40, 2)
    g = box_cells((0, 0, 0), size)
    model = t.model_create(g, np.full(len(g), 7, dtype=np.uint32))
    lo = corner_lo(0b110, size)                                       # low x, high y, high z
    assert t.volume_stamp_models(ST.placement(lo, model=model), _ffi.STAMP_SET, 1.0) == len(g)
    return lo, tuple(lo[a] + size[a] for a in range(3))


def edit_grow(t, d, m):
    size = (8, 12, 8)
    lo = corner_lo(0b111, size)
    hi = tuple(lo[a] + size[a] for a in range(3))
    seed = np.array([[hi[0] - 3, hi[1] - 4, hi[2] - 3]], np.int32)
    t.volume_set_voxels(seed, [5], [1.0])                             # (part of the same edit: one rebuild follows both)
    t.volume_distance_field(lo, hi, max_radius=3)
    assert t.volume_edit_by_distance(_ffi.DISTANCE_GROW, 8, 1.0, 7) > 50
    return lo, hi


def edit_flood(t, d, m):
    size = (4, 25, 5)
    lo = corner_lo(0b011, size)                                       # high x, high y, low z ... the column under the box's top face
    hi = tuple(lo[a] + size[a] for a in range(3))
    t.volume_flood_field(lo, hi, seeds=[lo], max_steps=64)
    assert t.volume_edit_by_flood(_ffi.FLOOD_FILL, 64, 1.0, 7) == size[0] * size[1] * size[2]
    return lo, hi


EDITS = {"upload": edit_upload, "set_voxels": edit_set_voxels, "brush": edit_brush, "stamp": edit_stamp, "grow": edit_grow, "flood": edit_flood}


def unchanged_outside(before, after, box, tag):
    """The texels the edit's box cannot reach — not even through the one texel of margin update_sun_map takes on every side — hold the
    very bits they held."""
    far_from_it = ~after.reached(*box, margin_texels=1)
    assert far_from_it.any() or box[0] == ORIGIN, tag
    assert (after.texels[far_from_it].view(np.uint32) == before.texels[far_from_it].view(np.uint32)).all(), (tag, "a texel out of the edit's reach changed")


@LAYOUTS
@pytest.mark.parametrize("kind", list(EDITS))
def test_a_filling_edit_leaves_the_map_valid_at_once(keyed, kind, mats):
    d, m = sparse_content(CUBE, 21, fill=0.01, top=TOP)
    t = tracer(keyed)
    t.volume_create(ORIGIN, CUBE, 128, 1.0)
    t.volume_upload(d, m)
    st = t.volume_rebuild(mats)
    assert int(st.levels) == 3 and tuple(int(c) for c in st.origin) == ORIGIN
    before = Verdict(t, B.voxels_of(d > 0, ORIGIN))
    before.assert_tight("base")
    box = EDITS[kind](t, d, m)
    t.volume_rebuild(mats)
    after = Verdict(t, filled(t, ORIGIN))
    assert (after.lo > before.lo + 1.0).any(), "the edit must add something taller than what stood there"
    after.report(f"after {kind}")
    after.assert_valid(kind)
    assert int(after.info["tighten_pending"]) == 0
    if kind == "upload":                                              # a fill of the whole box is a new world to the map
        assert int(after.info["loose_edits"]) == 0
        after.assert_tight("whole-box upload")
    else:
        assert int(after.info["loose_edits"]) == 1
        unchanged_outside(before, after, box, kind)
        assert (after.texels != before.texels).any()
    t.shutdown()


@LAYOUTS
def test_a_restore_that_fills_leaves_the_map_valid_at_once(keyed, mats):
    d, m = sparse_content(CUBE, 22, fill=0.01, top=TOP)
    size = (3, 35, 3)
    lo = corner_lo(0b101, (3, CUBE[1], 3))                            # high x, high z; the tower stands on the floor against two faces
    hi = (lo[0] + size[0], lo[1] + size[1], lo[2] + size[2])
    tower = box_cells(lo, size)
    t = tracer(keyed)
    t.volume_create(ORIGIN, CUBE, 128, 1.0)
    t.volume_upload(d, m)
    t.volume_set_voxels(tower, np.full(len(tower), 7, np.uint32), np.ones(len(tower), np.float32))
    t.volume_rebuild(mats)
    t.volume_encode_bricks(lo, hi)
    t.volume_set_voxels(tower, np.zeros(len(tower), np.uint32), np.zeros(len(tower), np.float32))
    t.volume_rebuild(mats)
    before = Verdict(t, filled(t, ORIGIN))
    before.assert_valid("tower taken away")
    t.volume_restore_bricks()
    t.volume_rebuild(mats)
    after = Verdict(t, filled(t, ORIGIN))
    assert (after.lo > before.lo + 1.0).any()
    after.report("after restore")
    after.assert_valid("restore")
    assert int(after.info["loose_edits"]) == 2
    unchanged_outside(before, after, (lo, hi), "restore")
    t.shutdown()


def test_an_edit_whose_footprint_starts_within_the_slack_of_a_texel_border(mats):
    """The one texel of margin update_sun_map takes around an edit's box is needed: a voxel whose (u, v) footprint begins less than
    kBeamSlack above a texel border is inside that neighbour's grown prism too.  Single-voxel edits chosen for that, on the u axis at the
    footprint's low edge and on the v axis at its high edge, each the tallest thing far and wide."""
    d, m = sparse_content(CUBE, 23, fill=0.01, top=TOP)
    t = tracer()
    t.volume_create(ORIGIN, CUBE, 128, 1.0)
    t.volume_upload(d, m)
    t.volume_rebuild(mats)
    base = Verdict(t, B.voxels_of(d > 0, ORIGIN))
    y = ORIGIN[1] + CUBE[1] - 1
    cells = box_cells((ORIGIN[0] + 8, y, ORIGIN[2] + 8), (48, 1, 48))
    umin, umax, vmin, vmax, _ = B.sun_footprints(cells, base.info)
    band = (base.delta + 0.005, B.K_BEAM_SLACK - base.delta - 0.005)
    frac_lo = (umin - float(base.info["u0"])) % 1.0                   # how far above a texel border the footprint begins
    frac_hi = (-(vmax - float(base.info["v0"]))) % 1.0                # how far below one it ends
    picks = [cells[(frac_lo > band[0]) & (frac_lo < band[1])][0], cells[(frac_hi > band[0]) & (frac_hi < band[1])][-1]]
    for k, cell in enumerate(picks):
        t.volume_set_voxels(cell.reshape(1, 3), [4], [1.0])
        t.volume_rebuild(mats)
        v = Verdict(t, filled(t, ORIGIN))
        v.report(f"voxel {cell.tolist()} a hair above a texel border")
        v.assert_valid(f"border voxel {k}")
    t.shutdown()


# ---- the tightening cycle -----------------------------------------------------------------------------------------------------------------
BIG = (250, 150, 250)                                                 # the tree's cube is 256: the map about 354 x 437 texels, the box's part of it about 343 x 364
LOOSE_EDITS, BAND_TEXELS = 32, 32768


def scattered_edit(k, rng):
    """Two or three voxels near corner k mod 8 of the BIG box, a few cells in from it."""
    corner = k % 8
    base = [ORIGIN[a] + (BIG[a] - 1 - int(rng.integers(0, 6)) if (corner >> a) & 1 else int(rng.integers(0, 6))) for a in range(3)]
    cells = np.array([base, [base[0], base[1] - 1 if (corner >> 1) & 1 else base[1] + 1, base[2]]], np.int32)
    return cells


def box_of(cells):
    return tuple(int(c) for c in cells.min(axis=0)), tuple(int(c) + 1 for c in cells.max(axis=0))


@LAYOUTS
def test_the_tightening_cycle(keyed, mats):
    """32 loose edits, then the bands: valid after every rebuild, the bookkeeping as api.hip documents it, and tight again when the
    pending rectangle has drained — except where the 32nd call's own raise came after its band."""
    rng = np.random.default_rng(31)
    d, m = sparse_content(BIG, 30, fill=0.00003)
    t = tracer(keyed)
    t.volume_create(ORIGIN, BIG, 128, 1.0)
    t.volume_upload(d, m)
    st = t.volume_rebuild(mats)
    assert int(st.levels) == 4
    voxels = {tuple(v) for v in B.voxels_of(d > 0, ORIGIN).tolist()}
    assert 150 < len(voxels) < 400
    as_array = lambda: np.array(sorted(voxels), dtype=np.int64)
    fresh = Verdict(t, as_array())
    fresh.assert_tight("fresh 256-cube map")
    nv, nu = fresh.map.shape
    assert 340 <= nu <= 460 and 420 <= nv <= 460 and nu * nv > 4 * BAND_TEXELS             # (256 |u|_1 = 351 by 256 |v|_1 = 435, and the margins)
    boxes, last_box = [], None
    # an empty place for the edits that change nothing, and a voxel of the base content that the clearing edit takes away
    empty_at = (ORIGIN[0] + 100.5, ORIGIN[1] + 140.5, ORIGIN[2] + 90.5)
    assert not any(abs(v[0] - empty_at[0]) < 3 and abs(v[1] - empty_at[1]) < 3 and abs(v[2] - empty_at[2]) < 3 for v in voxels)
    for k in range(1, LOOSE_EDITS + 1):
        if k == 16:                                                   # a clearing edit in the middle of the cycle
            gone = scattered_cells[0]                                 # what the edit before put there: a SUBTRACT brush over that one voxel
            t.volume_apply_brush(tuple(float(c) + 0.5 for c in gone), 0.4, 0.0, 1)
            boxes.append(box_of(gone.reshape(1, 3)))
            t.volume_rebuild(mats)
            voxels = {tuple(v) for v in filled(t, ORIGIN).tolist()}
            assert tuple(int(c) for c in gone) not in voxels
        else:
            scattered_cells = scattered_edit(k, rng)
            t.volume_set_voxels(scattered_cells, np.full(len(scattered_cells), 6, np.uint32), np.ones(len(scattered_cells), np.float32))
            voxels |= {tuple(int(c) for c in cell) for cell in scattered_cells}
            boxes.append(box_of(scattered_cells))
            last_box = boxes[-1]
            t.volume_rebuild(mats)
        v = Verdict(t, as_array())
        v.assert_valid(f"loose edit {k}")
        assert int(v.info["loose_edits"]) == k % LOOSE_EDITS, k
        assert int(v.info["tighten_pending"]) == (1 if k == LOOSE_EDITS else 0), k
    v.report("after the 32nd edit")
    assert {tuple(c) for c in filled(t, ORIGIN).tolist()} == voxels
    # the rectangle, less the first band (searched by the 32nd call itself), contains the texels of every edit's box
    u0, u1, v0, v1 = (int(v.info[key]) for key in ("pending_u0", "pending_u1", "pending_v0", "pending_v1"))
    rows = max(1, BAND_TEXELS // (u1 - u0 + 1))
    for box in boxes:
        iv, iu = np.nonzero(v.reached(*box))
        assert u0 <= iu.min() and iu.max() <= u1 and v0 - rows <= iv.min() and iv.max() <= v1, (box, (u0, u1, v0, v1))
    rect = np.zeros((nv, nu), bool)
    rect[v0 - rows:v1 + 1, u0:u1 + 1] = True
    assert (u1 - u0 + 1) * (v1 - v0 + 1) > 2 * BAND_TEXELS, "the rectangle must need several bands"
    # edits that change no voxel and fill nothing: a band of rows per edit
    n_bands = 1
    while int(v.info["tighten_pending"]):
        assert n_bands < 40
        t.volume_apply_brush(empty_at, 1.2, 0.0, 1)
        t.volume_rebuild(mats)
        w = Verdict(t, as_array())
        w.assert_valid(f"band {n_bands}")
        if v1 - v0 + 1 <= rows:
            assert int(w.info["tighten_pending"]) == 0
        else:
            v0 += rows
            assert int(w.info["tighten_pending"]) == 1
            assert (int(w.info["pending_u0"]), int(w.info["pending_u1"]), int(w.info["pending_v0"]), int(w.info["pending_v1"])) == (u0, u1, v0, v1)
        assert int(w.info["loose_edits"]) == n_bands
        n_bands += 1
        v = w
    assert n_bands >= 3
    assert {tuple(c) for c in filled(t, ORIGIN).tolist()} == voxels
    # drained: tight everywhere, except where the 32nd call raised after it searched
    raised = v.reached(*last_box, margin_texels=1)
    v.assert_tight("drained, outside the last raise", ~raised)
    v.assert_valid("drained, the last raise", raised)
    corners = np.array([[(last_box[1] if (c >> a) & 1 else last_box[0])[a] for a in range(3)] for c in range(8)], dtype=np.float64)
    far = float((corners @ B.frame_vectors(v.info)[2]).max())
    bound = far + 1.0e-3 * abs(far) + 0.01
    bound += B.ulp32(bound)
    assert (v.map[raised] <= np.maximum(v.hi[raised] + v.delta, bound)).all()
    assert (v.texels[~rect].view(np.uint32) == fresh.texels[~rect].view(np.uint32)).all(), "texels outside the rectangle were never touched"
    # a lattice change mid-cycle: a whole new map owes nothing
    for k in range(LOOSE_EDITS - int(v.info["loose_edits"]) + 1):
        cells = scattered_edit(k, rng)
        t.volume_set_voxels(cells, np.full(len(cells), 6, np.uint32), np.ones(len(cells), np.float32))
        t.volume_rebuild(mats)
    info, _ = t.sun_map(want_map=False)
    assert int(info["tighten_pending"][0]) == 1 and int(info["loose_edits"][0]) == 1
    d2, m2 = t.volume_download()
    t.volume_upload(d2, m2)                                           # a fill of the whole box: searched anew (rebuild_sun_map)
    t.volume_rebuild(mats)
    final = Verdict(t, filled(t, ORIGIN))
    assert int(final.info["tighten_pending"]) == 0 and int(final.info["loose_edits"]) == 0
    final.assert_tight("after rebuild_sun_map")
    t.shutdown()
