"""GPU: the resident volume (blok_hip_volume_*, gpu_build.hip) against a plain model of it, after every edit of long edit sequences.

Every check compares the downloaded dense arrays with tests/volume_tree_reference.py's DenseModel byte for byte, and the rebuilt tree —
nodes and material ids — with reference_tree of the model, byte for byte; the model and the reference are pinned to the oracle and to
the host builder in tests/test_volume_tree_reference_cpu.py.  Every test runs with the keyed layout allowed and refused (small boxes
fall back to the general one by themselves; nothing here asserts which was chosen).  The cases: boxes of 1 to 7 levels with ragged last
bricks, edits that end on 4-, 16- and 64-voxel boundaries and on the box's faces, the state a keyed volume carries across rebuilds
(dirty bytes, material offsets of the previous build, ping-pong arrays, reallocations), both refresh paths of keyed_refresh (the
switch is at 65 536 bricks / 4096 level-2 cells in an edit's range) with data, and frames of the final states against the oracle.

Not covered: a KEYED volume of 6 or 7 levels.  The keyed layout is chosen for such a box only when it holds at least 64^5 / 8 = 2^27
bricks (2^33 voxels), which no test can fill, edit and compare in seconds; boxes of 6 and 7 levels are tested in the general layout."""
import numpy as np
import pytest

from blok_amd import world as W
from tests import oracle_ffi as O
from tests.conftest import SEED, records_equal
from tests.volume_tree_reference import DenseModel, OutsideBox, box_levels, brick_table, reference_tree

pytestmark = pytest.mark.gpu

FW, FH = 96, 64                       # frames of section (e)
ORIGIN = (-7, 3, -20)
LAYOUTS = pytest.mark.parametrize("keyed", [True, False], ids=["keyed", "general"])


@pytest.fixture(scope="module")
def tr():
    from blok_amd.tracer import HipTracer
    t = HipTracer(FW, FH).init()
    yield t
    t.shutdown()


@pytest.fixture(scope="module")
def mats():
    return W.scene_materials(SEED)


def _first_difference(got: np.ndarray, ref: np.ndarray) -> str:
    if got.shape != ref.shape:
        return f"shape {got.shape} for {ref.shape}"
    rows = np.flatnonzero((got != ref).reshape(len(ref), -1).any(axis=1))
    i = int(rows[0])
    return f"{len(rows)} of {len(ref)} entries differ, the first at {i}: {got[i].tolist()} for {ref[i].tolist()}"


def check(tr, model, tag, mats=None):
    """Dense arrays == the model's; the rebuilt tree == reference_tree(model); world_stats agree.  Returns the reference."""
    d, m = tr.volume_download()
    assert d.tobytes() == model.density.tobytes(), (tag, "density", _first_difference(d.view(np.uint32).ravel(), model.density.view(np.uint32).ravel()))
    assert m.tobytes() == model.ids.tobytes(), (tag, "ids", _first_difference(m.ravel(), model.ids.ravel()))
    st = tr.volume_rebuild(mats)
    levels = box_levels(model.shape_xyz)
    ref_nodes, ref_mats = reference_tree(model.filled, model.ids, levels)
    if len(ref_mats) == 0:                                     # an empty world is the host builder's: one empty node, one level, no origin of its own
        assert (st.n_voxels, st.n_tree_nodes, st.levels) == (0, 1, 1), tag
    else:
        assert (st.n_voxels, st.n_tree_nodes, st.levels, tuple(st.origin)) == (len(ref_mats), len(ref_nodes), levels, model.origin), tag
    nodes, ids = tr.download_tree()
    assert nodes.tobytes() == ref_nodes.tobytes(), (tag, "nodes", _first_difference(nodes, ref_nodes))
    assert ids.tobytes() == ref_mats.tobytes(), (tag, "materials", _first_difference(ids, ref_mats))
    return ref_nodes, ref_mats


class Pair:
    """The same edits to the volume and to the model.  Without a tracer: the model alone (what a sequence does is then known from the
    reference alone — the step counts of section (c), the oracle's frame counts of section (e))."""

    def __init__(self, tr, origin, shape, keyed=True, mats=None):
        self.tr, self.mats, self.model = tr, mats, DenseModel(origin, shape)
        self.history = []                                      # brick tables of the checked states
        self.counts = (0, 0, 0)
        if tr is not None:
            tr.set_volume_layout(keyed)
            tr.volume_create(origin, shape, 128, 1.0)

    def local(self, xyz):
        return np.asarray(xyz, dtype=np.int64).reshape(-1, 3) + np.asarray(self.model.origin)

    def upload(self, density, ids):
        self.model.upload(density, ids)
        if self.tr is not None:
            self.tr.volume_upload(density, ids)

    def set_voxels(self, xyz, ids=None, density=None):
        self.model.set_voxels(xyz, ids, density)
        if self.tr is not None:
            self.tr.volume_set_voxels(xyz, ids, density)

    def brush(self, center, radius, value, mode):
        self.model.brush(center, radius, value, mode)
        if self.tr is not None:
            self.tr.volume_apply_brush(center, radius, value, mode)

    def refused(self, what, *args):
        """An edit that leaves the box: the model refuses it, the volume raises BlokError, and the next check finds nothing written."""
        from blok_amd._ffi import BlokError
        with pytest.raises(OutsideBox):
            getattr(self.model, what)(*args)
        if self.tr is not None:
            with pytest.raises(BlokError):
                (self.tr.volume_set_voxels if what == "set_voxels" else self.tr.volume_apply_brush)(*args)

    def took(self, path, tag):
        """Section (d): exactly one refresh since the last call, and in a keyed volume on `path` — 0 an edit's (a wave per brick, the
        pyramid in one workgroup), 1 an upload's (a lane per brick, a launch per level)."""
        if self.tr is None:
            return
        now = self.tr.volume_refresh_counts()
        delta = tuple(a - b for a, b in zip(now, self.counts))
        self.counts = now
        assert sum(delta) == 1 and (delta[2] == 1 or delta[path] == 1), (tag, delta)

    def check(self, tag, table=False):
        if table:
            self.history.append(brick_table(self.model.filled, self.model.ids))
        if self.tr is not None:
            check(self.tr, self.model, tag, self.mats)

    def name_every_filled_voxel(self):
        """Section (e): every filled voxel gets a nonzero id, in one set_voxels call (a voxel of id 0 is not a surface to the oracle)."""
        z, y, x = np.nonzero(self.model.filled)
        ids = self.model.ids[z, y, x]
        ids = np.where(ids == 0, 1 + (x + 3 * y + 5 * z) % 200, ids).astype(np.uint32)
        self.set_voxels(self.local(np.stack([x, y, z], 1)), ids, self.model.density[z, y, x])


def random_fill(rng, shape_xyz, fraction):
    """(density, ids) [z][y][x]: `fraction` of the voxels filled with densities in (0, 1]; the empty ones hold zeros of both signs,
    negative densities and NaNs, and every voxel — empty ones too — an id in 1..255."""
    shp = tuple(reversed(shape_xyz))
    empty = np.array([0.0, -0.0, -1.0, np.nan, -np.inf, 0.0], dtype=np.float32)[rng.integers(0, 6, shp)]
    density = np.where(rng.random(shp) < fraction, (1.0 - rng.random(shp)).astype(np.float32), empty).astype(np.float32)
    return density, rng.integers(1, 256, shp).astype(np.uint32)


# ---- (a) extents and level counts -----------------------------------------------------------------------------------------------------
# levels 1..7, ragged last bricks on every axis, level-2 pyramids of 1, 64, 4096 and 262 144 cells
BOXES = [(1, 1, 1), (4, 4, 4), (3, 2, 4), (5, 5, 5), (16, 16, 16), (16, 1, 7), (17, 3, 64), (64, 64, 64), (65, 9, 6), (256, 5, 5), (257, 8, 8),
         (1025, 4, 4), (4097, 1, 2)]


@LAYOUTS
@pytest.mark.parametrize("shape", BOXES, ids=lambda s: "x".join(map(str, s)))
def test_boxes_of_every_level_count(tr, mats, keyed, shape):
    rng = np.random.default_rng(sum(shape))
    for origin in (ORIGIN, (0, 0, 0)):
        assert all(o + n <= 32768 for o, n in zip(origin, shape))
        p = Pair(tr, origin, shape, keyed, mats)
        p.check((origin, "created"))                           # nothing filled: one empty node
        p.upload(*random_fill(rng, shape, 0.3))
        p.check((origin, "30 % fill"))
        p.upload(np.ones(tuple(reversed(shape)), dtype=np.float32), rng.integers(1, 256, tuple(reversed(shape))).astype(np.uint32))
        p.check((origin, "solid"))
        p.upload(None, None)
        corners = [[x, y, z] for z in (0, shape[2] - 1) for y in (0, shape[1] - 1) for x in (0, shape[0] - 1)]
        p.set_voxels(p.local(corners), np.arange(11, 19), None)      # (coincident corners of a thin box: the last write wins)
        p.check((origin, "corners only"))


# ---- (b) edit boxes on boundaries ------------------------------------------------------------------------------------------------------
def boundary_sequence(p: Pair):
    nx, ny, nz = p.model.shape_xyz
    o = np.asarray(p.model.origin, dtype=np.float64)
    hi = o + (nx, ny, nz)
    rng = np.random.default_rng(70)
    p.upload(*random_fill(rng, (nx, ny, nz), 0.05))
    p.check("5 % fill")
    # single voxels either side of the 4-, 16- and 64-voxel boundaries and on the far faces, one axis at a time
    singles = [[x, 9, 77] for x in (3, 4, 15, 16, 63, 64, 69)] + [[21, y, 77] for y in (3, 4, 15, 16, 36)] + [[21, 9, z] for z in (3, 4, 15, 16, 63, 64, 69, 127, 128, 129)]
    for k, v in enumerate(singles):
        p.set_voxels(p.local([v]), [20 + k], [0.5])
        p.check(("fill", v))
    for k, v in enumerate(singles):
        p.set_voxels(p.local([v]), [90 + k], [(0.0, -0.0, -1.0, np.nan)[k % 4]])
        p.check(("empty", v))
    p.set_voxels(p.local([[0, 0, 0], [nx - 1, ny - 1, nz - 1]]), [201, 202], [1.0, 0.25])
    p.check("opposite corners")
    p.brush(tuple(o + 4.5), 4.5, 1.0, 0)                       # floor(c - r) = the low faces exactly
    p.check("brush on the low faces")
    p.brush(tuple(hi - 4.5), 4.49, 0.75, 0)                    # floor(c + r) + 1 = the high faces exactly
    p.check("brush on the high faces")
    p.refused("brush", tuple(hi - 4.5), 4.5, 1.0, 0)           # one voxel further
    p.check("refused brush")
    p.brush(tuple(o + (32, 16, 64)), 8.0, 1.0, 0)              # integer centre and radius: [24, 41) x [8, 25) x [56, 73), starts on brick boundaries
    p.check("integer brush")
    p.brush(tuple(o + (20, 20, 80)), 16.0, -0.0, 1)            # [4, 37) x [4, 37 = ny) x [64, 97): a 64-voxel boundary and the high y face
    p.check("integer brush, subtract")
    p.brush(tuple(o + (48, 16, 32)), 15.0, 0.5, 0)             # [33, 64) x [1, 32) x [17, 48): ends on the 64-voxel boundary in x
    p.check("integer brush ending at 64")
    p.refused("set_voxels", p.local([[5, 5, 5], [nx, 5, 5]]), [1, 2], [1.0, 1.0])
    p.refused("set_voxels", p.local([[5, 5, 5], [5, -1, 5]]), [1, 2], [1.0, 1.0])
    p.check("refused set_voxels")


# ---- (c) stale state across rebuilds ---------------------------------------------------------------------------------------------------
def stale_sequence(p: Pair, repeats: int = 10):
    nx, ny, nz = p.model.shape_xyz
    o = np.asarray(p.model.origin, dtype=np.float64)
    rng = np.random.default_rng(96)
    m = p.model
    brick = np.array([[x, y, z] for z in range(4) for y in range(4) for x in range(4)])

    def chk(tag):
        p.check(tag, table=True)

    p.upload(*random_fill(rng, (nx, ny, nz), 0.1))
    chk("10 % fill")
    z, y, x = (int(c[len(c) // 2]) for c in np.nonzero(m.filled))                 # a filled voxel in the middle of the box
    p.set_voxels(p.local([[x, y, z]]), [int(m.ids[z, y, x]) % 255 + 1], [m.density[z, y, x]])
    chk("an id under an unchanged mask")
    p.set_voxels(p.local([[x, y, z]]), None, [m.density[z, y, x]])
    chk("a filled voxel of id 0")
    z, y, x = (int(c[len(c) // 2]) for c in np.nonzero(~m.filled))
    p.set_voxels(p.local([[x, y, z]]), None, [0.5])
    chk("density without an id")
    # a brick emptied and refilled with other ids: a rebuild in between, then none
    at = brick + (40, 40, 40)
    keep = m.filled[at[:, 2], at[:, 1], at[:, 0]]
    assert 0 < keep.sum() < 64
    p.set_voxels(p.local(at), np.full(64, 7), np.zeros(64, dtype=np.float32))
    chk("brick emptied")
    p.set_voxels(p.local(at[keep]), 100 + np.arange(keep.sum()), None)
    chk("brick refilled")
    p.set_voxels(p.local(at), np.full(64, 8), np.full(64, -0.0, dtype=np.float32))
    p.set_voxels(p.local(at[keep]), 150 + np.arange(keep.sum()), None)
    chk("brick emptied and refilled between two rebuilds")
    # the lowest-key corner gains and loses voxels: every other brick's material offset moves
    low = brick[~m.filled[brick[:, 2], brick[:, 1], brick[:, 0]]]
    assert len(low) >= 12
    for k in range(3):
        p.set_voxels(p.local(low[4 * k:4 * k + 4]), [30 + k] * 4, None)
        chk(("lowest-key corner gains voxels", k))
    for k in range(3):
        p.set_voxels(p.local(low[4 * k:4 * k + 4 - k]), None, np.zeros(4 - k, dtype=np.float32))
        chk(("lowest-key corner loses voxels", k))
    chk("no edit")
    # rebuilds in a row, edits alternating between two far corners (the ping-pong tree / material arrays), an id changing elsewhere
    z, y, x = (int(c[len(c) // 3]) for c in np.nonzero(m.filled))
    for k in range(repeats):
        corner = (0, 0, 0) if k % 2 == 0 else (nx - 4, ny - 4, 0)
        v = brick[(5 * k) % 64] + corner
        p.set_voxels(p.local([v, [x, y, z]]), [60 + k, 70 + k], [0.0 if m.filled[v[2], v[1], v[0]] else 1.0, m.density[z, y, x]])
        chk(("alternating corners", k))
    # one brick -> more than 5000 bricks in one edit, and back (the reallocations)
    d = np.zeros((nz, ny, nx), dtype=np.float32)
    d[44:48, 40:44, 48:52] = 1.0
    p.upload(d, rng.integers(1, 256, d.shape).astype(np.uint32))
    chk("one brick")
    many = np.array([[4 * bx + 1, 4 * by + 2, 4 * bz + 3] for bz in range(nz // 4) for by in range(ny // 4) for bx in range(nx // 4) if (bx + by + bz) % 2 == 0])
    assert len(many) > 5000
    p.set_voxels(p.local(many), 1 + np.arange(len(many)) % 255, None)
    chk("more than 5000 bricks")
    p.set_voxels(p.local(many), None, np.zeros(len(many), dtype=np.float32))
    chk("one brick again")
    # emptied by brushes alone, rebuilt empty, refilled in a third of the bricks
    p.brush(tuple(o + (50.0, 42.0, 46.0)), 6.0, 0.0, 1)
    chk("emptied by a brush")
    third = np.array([[4 * bx + (bx + k) % 4, 4 * by + k, 4 * bz + 2] for bz in range(nz // 4) for by in range(ny // 4) for bx in range(nx // 4) if (bx + by + bz) % 3 == 0
                      for k in range(3)])
    p.set_voxels(p.local(third), 1 + np.arange(len(third)) % 255, None)
    chk("a third of the bricks")
    density, ids = random_fill(rng, (nx, ny, nz), 0.08)
    p.upload(None, ids)
    chk("ids alone")
    p.upload(density, None)
    chk("density alone")


def stale_counts(history):
    """(steps in which some brick keeps its mask and ids while its material offset moves, steps in which some brick's ids change under
    an unchanged mask), from the brick tables of consecutive checked states."""
    moved = renamed = 0
    for before, after in zip(history, history[1:]):
        same = [b for b in before.keys() & after.keys() if before[b][0] == after[b][0]]
        moved += any(before[b][1] == after[b][1] and before[b][2] != after[b][2] for b in same)
        renamed += any(before[b][1] != after[b][1] for b in same)
    return moved, renamed


# ---- (d) both refresh paths ------------------------------------------------------------------------------------------------------------
def refresh_paths_sequence(p: Pair):
    """160^3: a whole-box range is 40^3 = 64 000 bricks and 10^3 level-2 cells, the wave-per-brick path with the one-workgroup pyramid;
    168^3: 42^3 = 74 088 bricks, the lane-per-brick path with a launch per level."""
    n = p.model.shape_xyz[0]
    o = np.asarray(p.model.origin, dtype=np.float64)
    rng = np.random.default_rng(n)
    whole = 0 if (n // 4) ** 3 <= 65536 else 1                 # keyed_refresh's rule for a range of the whole box
    p.upload(*random_fill(rng, (n, n, n), 0.02))
    p.took(whole, "upload")
    p.check("2 % fill")
    p.set_voxels(p.local([[0, 0, 0], [n - 1, n - 1, n - 1]]), [3, 4], [1.0, 0.5])
    p.took(whole, "opposite corners")
    p.check("opposite corners")
    p.brush(tuple(o + n / 2 + 0.25), 9.5, 1.0, 0)
    p.took(0, "brush in the middle")
    p.check("brush in the middle")
    p.upload(*random_fill(rng, (n, n, n), 0.03))
    p.took(whole, "another fill")
    p.check("another fill")
    if n == 168:
        p.brush(tuple(o + 84.0), 83.0, 0.0, 1)                 # [1, 168) per axis: 42^3 bricks from a brush — it hollows the fill
        p.took(1, "brush over the whole box")
        p.check("brush over the whole box")
        p.brush(tuple(o + 84.0), 40.0, 1.0, 0)                 # 21^3 bricks: the other path again, a solid ball
        p.took(0, "ball")
        p.check("ball")


# ---- (e) frames ------------------------------------------------------------------------------------------------------------------------
def cameras(model):
    """Outside the box; inside an empty voxel (the one nearest to the middle of the layer two voxels under the top face), looking level
    towards the low corner: the upper half of the frame leaves through the top face; and on the plane of the box's low x face, looking
    along it."""
    o = np.asarray(model.origin, dtype=np.float64)
    n = np.asarray(model.shape_xyz, dtype=np.float64)
    mid = o + n / 2
    z, y, x = np.nonzero(~model.filled)
    i = int(np.argmin((x + 0.5 - n[0] / 2) ** 2 + (y + 0.5 - (n[1] - 2.5)) ** 2 + (z + 0.5 - n[2] / 2) ** 2))
    inside = o + (x[i] + 0.5, y[i] + 0.5, z[i] + 0.5)
    return [W.camera_look_at(tuple(mid + (0.9 * n[0], 0.8 * n[1], -1.1 * n[2])), tuple(mid), 60.0, FW, FH),
            W.camera_look_at(tuple(inside), (o[0], inside[1], o[2]), 70.0, FW, FH),
            W.camera_look_at((o[0], mid[1], o[2] - 0.4 * n[2]), (o[0], mid[1], o[2] + n[2]), 60.0, FW, FH)]


def oracle_frames(model):
    """[(records, hits)] of the three cameras from the oracle's own world of the model's filled voxels."""
    z, y, x = np.nonzero(model.filled)
    ow = O.OracleWorld(128, 1.0)
    ow.set_voxels(np.stack([x, y, z], 1) + np.asarray(model.origin), model.ids[z, y, x])
    ow.rebuild()
    lat = O.Lattice(*ow.pack())
    out = []
    for cam in cameras(model):
        ref, ctr = lat.trace(O.primary_rays(cam, FW, FH), threads=8)
        out.append((cam, ref, int(ctr["hits"])))
    return out


def check_frames(p: Pair, tag, floors):
    """floors: per camera (hits, misses), about 0.7 of what the oracle alone reports for this state (printed below; FW * FH = 6144 rays)."""
    p.name_every_filled_voxel()
    p.check((tag, "every filled voxel named"))
    for k, (cam, ref, hits) in enumerate(oracle_frames(p.model)):
        print(f"{tag} camera {k}: oracle hits {hits}, misses {FW * FH - hits}")
        assert hits >= floors[k][0] and FW * FH - hits >= floors[k][1], (tag, k, hits)
        if p.tr is not None:
            got = p.tr.draw_frame(cam).reshape(-1)
            same = records_equal(got, ref)
            assert same.all(), (tag, k, f"{int((~same).sum())} of {len(ref)} records differ, the first at pixel {int(np.flatnonzero(~same)[0])}")


# (hits, misses) per camera at about 0.7 of what the oracle alone reports for the model's final states, of 96 x 64 = 6144 rays:
#   boundaries (799, 5345) (4520, 1624) (1615, 4529);  stale (1804, 4340) (5234, 910) (3069, 3075);  paths (1786, 4358) (3310, 2834) (2907, 3237)
FLOORS = {"boundaries": [(560, 3740), (3160, 1135), (1130, 3170)], "stale": [(1260, 3040), (3660, 640), (2150, 2150)], "paths": [(1250, 3050), (2320, 1980), (2030, 2270)]}


@LAYOUTS
def test_edit_boxes_on_boundaries(tr, mats, keyed):
    p = Pair(tr, ORIGIN, (70, 37, 130), keyed, mats)
    assert box_levels(p.model.shape_xyz) == 4
    boundary_sequence(p)
    check_frames(p, "boundaries", FLOORS["boundaries"])


@LAYOUTS
def test_state_carried_across_rebuilds(tr, mats, keyed):
    p = Pair(tr, ORIGIN, (96, 80, 96), keyed, mats)
    stale_sequence(p)
    moved, renamed = stale_counts(p.history)
    print(f"steps with a brick unchanged at a moved offset: {moved}; with ids changed under an unchanged mask: {renamed}")
    assert moved >= 20 and renamed >= 5                        # (21 and 13) from the reference's voxels alone: the sequence does exercise the take-over
    check_frames(p, "stale", FLOORS["stale"])


@LAYOUTS
@pytest.mark.parametrize("n", [160, 168])
def test_both_refresh_paths(tr, mats, keyed, n):
    p = Pair(tr, ORIGIN, (n, n, n), keyed, mats)
    assert ((n // 4) ** 3 <= 65536) == (n == 160) and (n // 16 + 1) ** 3 <= 4096 and box_levels((n, n, n)) == 4      # which side of the switch a whole-box range falls
    refresh_paths_sequence(p)
    if n == 168:
        check_frames(p, "paths", FLOORS["paths"])


# ---- (f) creation refusals -------------------------------------------------------------------------------------------------------------
REFUSED = {"extent 16385": ((0, 0, 0), (16385, 1, 1), 1.0), "origin + extent > 32768": ((32760, 0, 0), (16, 4, 4), 1.0), "origin + extent > 32768 in z": ((0, 0, 32767), (1, 1, 2), 1.0),
           "origin < -32768": ((0, -32769, 0), (4, 4, 4), 1.0), "zero x": ((0, 0, 0), (0, 4, 4), 1.0), "zero y": ((0, 0, 0), (4, 0, 4), 1.0), "zero z": ((0, 0, 0), (4, 4, 0), 1.0),
           "voxel size 0.5": ((0, 0, 0), (4, 4, 4), 0.5)}


@LAYOUTS
@pytest.mark.parametrize("case", list(REFUSED))
def test_creation_refusals(tr, mats, keyed, case):
    from blok_amd._ffi import BlokError
    origin, shape, voxel_size = REFUSED[case]
    tr.set_volume_layout(keyed)
    with pytest.raises(BlokError):
        tr.volume_create(origin, shape, 128, voxel_size)
    p = Pair(tr, ORIGIN, (5, 5, 5), keyed, mats)
    p.upload(*random_fill(np.random.default_rng(5), (5, 5, 5), 0.4))
    p.check("after a refused creation")
