"""GPU: the beam pre-pass's start parameters (beam.h: beam_start, beam_search<true>) as NUMBERS, tile by tile, against
tests/bounds_reference.py — not through the frames they leave unchanged.

With a visit budget far above any search neither coarsening nor exhaustion can occur, and every tile must satisfy
t0_lo - eps <= t0 <= t0_hi + eps, with kBeamNone exactly where no voxel may be kept and never where one must be.  Under a budget the
answer may only be lower: 0 <= t0 <= t0_hi + eps.  delta and eps are derived in tests/bounds_reference.py; every test prints the largest
deviation from the nearer bound it saw, in world units and in units of the tile's eps.

Measured on an MI355X, unlimited budget, largest deviation beyond the nearer reference bound over 3954 tiles per world: 2.1e-5 (64^3 scene,
0.07 eps), 1.6e-4 (odd world, 0.09 eps), 4.0e-5 / 1.6e-4 (voxel sizes 0.5 / 2, 0.06 eps), 4.0e-5 (HIGH box, 0.11 eps); under budgets the
largest excess over t0_hi is 0.10 eps.  Default budget on the 64^3 scene: 3180 of 3180 tiles exact, no search beyond 96 visits (asserted).
The bounds a resting view keeps are read out of the slot its launch walked from and are the bits of a fresh search.
What these tests found on their first run: 2 - 3 of 390 tiles per view held a t0 of 1.8 to 26 BELOW t0_lo (64^3 scene, tiles 142, 168,
223: 73.355, 73.908, 101.773 against 83.369, 83.361, 103.576; 34 - 46 visits where 18 - 22 suffice) — beam_search widened the stacked low
candidate word as the signed int the readlane builtin returns, so a word with bit 31 set made all 32 high lanes candidates of a
revisited node (beam.h, fixed with this module).  Conservative, hence invisible to every image test; with it the bounds were not monotone
in the budget either."""
from __future__ import annotations

import numpy as np
import pytest

from blok_amd import world as W
from tests import bounds_reference as B
from tests import limit_cases as LC
from tests.conftest import SEED, make_scene_world

pytestmark = pytest.mark.gpu

W_PX, H_PX = 203, 117                                                 # partial tiles at the right and bottom edges for every tile size
RECTS = [(0, 0, W_PX, H_PX), (37, 19, 101, 55)]
TILES = (8, 16, 32, 64)
UNLIMITED = 1 << 20


class World:
    """One context with a world installed, and what the reference needs of it."""

    def __init__(self, name):
        from blok_amd.tracer import HipTracer
        self.name = name
        self.t = t = HipTracer(W_PX, H_PX).init()
        self.vs = 1.0
        mats = W.scene_materials(SEED)
        if name == "scene 64":
            t.add_world(make_scene_world(64)[1])
            self.voxels = B.voxels_of(W.scene_dense(64, SEED) != 0, (0, 0, 0))
        elif name == "odd world" or name.startswith("voxel size"):
            self.vs = float(name.split()[-1]) if name.startswith("voxel size") else 1.0
            xyz, ids = B.odd_world_voxels()
            if self.vs != 1.0:
                xyz, ids = xyz[::3], ids[::3]
                t.set_voxel_size(self.vs)
            cm = W.ChunkManager(128, self.vs)
            cm.set_voxels(xyz, ids); cm.rebuild_dirty_chunks()
            t.add_world(cm.pack_chunks_to_gpu_svo(mats))
            self.voxels = np.unique(xyz.astype(np.int64), axis=0)
        else:                                                         # a resident volume at the HIGH end of the lattice
            self.origin = LC.limit_origin("HIGH", LC.SHAPE)
            rng = np.random.default_rng(8)
            f = rng.random(LC.SHAPE[::-1]) < 0.004
            f[-1, -1, -1] = f[0, 0, 0] = True
            f[10:40, 30, 20:70] = True                               # a one-voxel floor
            self.d, self.m = f.astype(np.float32), f.astype(np.uint32) * 3
            t.volume_create(self.origin, LC.SHAPE, 128, 1.0)
            t.volume_upload(self.d, self.m)
            t.volume_rebuild(mats)
            self.voxels = B.voxels_of(f, self.origin)
        self.mats = mats
        st = t.world_stats()
        assert int(st.n_voxels) == len(self.voxels)
        self.cube = B.cube_of(None, [int(c) for c in st.origin], int(st.levels))
        t.set_beam_cache(False)                                       # (beam_prepass searches whatever this says: it never looks at the slots)
        self.lo = self.voxels.min(axis=0).astype(np.float64)
        self.hi = self.voxels.max(axis=0).astype(np.float64) + 1.0
        self.centre, self.radius = 0.5 * (self.lo + self.hi), 0.5 * float(np.linalg.norm(self.hi - self.lo))

    def cam(self, eye, target, fov):
        return W.camera_look_at(tuple(float(c) * self.vs for c in eye), tuple(float(c) * self.vs for c in target), fov, W_PX, H_PX)

    def cameras(self):
        """{tag: camera}, positions given in voxel units: outside, inside a filled voxel, grazing a face of the tree's cube, looking away,
        and the narrowest and the widest field of view."""
        c, r = self.centre, self.radius
        inside = self.voxels[len(self.voxels) // 2].astype(np.float64) + (0.5, 0.25, 0.75)
        face_x = self.cube[0][0]                                      # the cube's low x face
        far_voxel = self.voxels[np.argmax(np.abs(self.voxels - c).sum(axis=1))].astype(np.float64) + 0.5
        return {"outside": self.cam(c + (1.3 * r, 0.9 * r, -1.5 * r), c, 60.0),
                "inside a voxel": self.cam(inside, c + (3.0, -2.0, 1.0), 70.0),
                "grazing": self.cam((face_x, c[1] + 0.3, self.cube[0][2] - 0.2 * r), (face_x, c[1] - 0.2 * r, c[2] + r), 50.0),
                "away": self.cam(c + (1.3 * r, 0.9 * r, -1.5 * r), c + (2.6 * r, 1.8 * r, -3.0 * r), 60.0),
                "4 degrees": self.cam(far_voxel + (2.0 * r, 0.7 * r, 1.1 * r), far_voxel, 4.0),
                "150 degrees": self.cam(c + (0.2 * r, 1.1 * r, 0.3 * r), c, 150.0)}

    def bounds(self, cam, rect, tile):
        return B.beam_tile_bounds(self.voxels, cam, W_PX, H_PX, rect, tile, self.vs, B.beam_delta(cam, self.vs, *self.cube))


_worlds = {}


@pytest.fixture
def world(request):
    name = request.param
    if name not in _worlds:
        _worlds[name] = World(name)
    return _worlds[name]


@pytest.fixture(scope="module", autouse=True)
def shut_down():
    yield
    for w in _worlds.values():
        w.t.shutdown()
    _worlds.clear()


WORLDS = pytest.mark.parametrize("world", ["scene 64", "odd world", "voxel size 0.5", "voxel size 2.0", "HIGH box"], indirect=True)


class Worst:
    def __init__(self):
        self.dev, self.in_eps, self.tiles, self.none = 0.0, 0.0, 0, 0

    def take(self, got, lo, hi, eps):
        g = got.astype(np.float64)
        live = g < B.K_BEAM_NONE
        self.tiles += len(g); self.none += int((~live).sum())
        d = np.maximum(np.where(lo < B.K_BEAM_NONE, lo - g, 0.0), np.where(hi < B.K_BEAM_NONE, g - hi, 0.0))[live]
        if len(d):
            k = int(np.argmax(d))
            if d[k] > self.dev:
                self.dev, self.in_eps = float(d[k]), float(d[k] / eps[live][k])


def exact(got, lo, hi, eps, tag):
    g = got.astype(np.float64)
    none = g >= B.K_BEAM_NONE
    assert (none[lo >= B.K_BEAM_NONE]).all(), (tag, "a bound where no voxel can be kept")
    assert (~none[hi < B.K_BEAM_NONE]).all(), (tag, "none where a voxel must be kept")
    bad = ~none & ~((lo - eps <= g) & (g <= hi + eps))
    assert not bad.any(), (tag, np.nonzero(bad)[0][:4].tolist(), g[bad][:4].tolist(), lo[bad][:4].tolist(), hi[bad][:4].tolist(), eps[bad][:4].tolist())


@WORLDS
def test_unlimited_searches_are_exact(world):
    t = world.t
    t.set_beam_budget(UNLIMITED)
    worst = Worst()
    for tag, cam in world.cameras().items():
        for tile in TILES:
            t.set_beam(tile)
            for rect in RECTS:
                got, visits = t.beam_prepass(cam, rect, want_visits=True)
                lo, hi, eps = world.bounds(cam, rect, tile)
                assert len(got) == len(lo) and (visits < UNLIMITED // 4).all()
                worst.take(got, lo, hi, eps)
                exact(got, lo, hi, eps, (world.name, tag, tile, rect))
                if tag == "inside a voxel":
                    assert (got == 0.0).all(), (tag, tile, rect)
                if tag == "away":
                    assert (got >= np.float32(B.K_BEAM_NONE)).all(), (tag, tile, rect)
        live = got < np.float32(B.K_BEAM_NONE)
        print(f"[beam] {world.name}, {tag}: {int(live.sum())} of {len(got)} tiles of the last rectangle live")
    print(f"[beam] {world.name}: {worst.tiles} tiles ({worst.none} none), largest deviation beyond the nearer bound {worst.dev:.3g} = {worst.in_eps:.2f} eps")
    assert worst.none > 0 and worst.none < worst.tiles
    t.set_beam_budget(0); t.set_beam(32)


@WORLDS
def test_budgets_only_lower_the_bound(world):
    t = world.t
    worst = Worst()
    for tag, cam in world.cameras().items():
        for tile in (8, 32):
            t.set_beam(tile)
            rect = RECTS[0]
            lo, hi, eps = world.bounds(cam, rect, tile)
            t.set_beam_budget(UNLIMITED)
            full, _ = t.beam_prepass(cam, rect, want_visits=True)
            previous = None
            for budget in (1, 2, 8, 64, 0):                          # 0 = the default, 256
                t.set_beam_budget(budget)
                got, visits = t.beam_prepass(cam, rect, want_visits=True)
                g = got.astype(np.float64)
                assert (visits <= (budget or 256)).all(), (tag, tile, budget, int(visits.max()))
                assert (g >= 0.0).all()
                assert (g[hi < B.K_BEAM_NONE] < B.K_BEAM_NONE).all(), (tag, tile, budget, "none where a voxel must be kept")
                live = g < B.K_BEAM_NONE
                assert (g[live] <= hi[live] + eps[live]).all(), (tag, tile, budget)
                assert (g <= full.astype(np.float64) + eps).all(), (tag, tile, budget, "above the unlimited search")
                worst.take(got, np.full(len(g), B.K_BEAM_NONE), hi, eps)
                if previous is not None:                              # monotone in the budget
                    assert (previous <= g + eps).all(), (world.name, tag, tile, budget, float((previous - g).max()))
                previous = g
            assert (previous <= full.astype(np.float64) + eps).all()
    print(f"[beam] {world.name}, budgets: largest excess over t0_hi {worst.dev:.3g} = {worst.in_eps:.2f} eps")
    t.set_beam_budget(0); t.set_beam(32)


@pytest.mark.parametrize("world", ["scene 64"], indirect=True)
def test_default_budget_on_the_scene(world):
    """How many tiles the default budget (256 visits; coarsening from the 98th evaluation on, beam.h: kBeamCoarsen1) leaves exact on the
    64^3 scene.  A search that spent at most 96 visits took the very path of the unlimited one: its answer is the same bits."""
    t = world.t
    n = n_exact = n_short = 0
    for tag, cam in world.cameras().items():
        for tile in TILES:
            t.set_beam(tile)
            t.set_beam_budget(UNLIMITED)
            full, full_visits = t.beam_prepass(cam, RECTS[0], want_visits=True)
            t.set_beam_budget(0)
            got, visits = t.beam_prepass(cam, RECTS[0], want_visits=True)
            short = visits <= 96
            assert np.array_equal(full_visits[short], visits[short])
            assert (got[short].view(np.uint32) == full[short].view(np.uint32)).all(), (tag, tile)
            n += len(got); n_short += int(short.sum()); n_exact += int((got.view(np.uint32) == full.view(np.uint32)).sum())
    print(f"[beam] scene 64, default budget: {n_exact} of {n} tiles exact; {n_short} searches of at most 96 visits")
    assert n_short == n and n_exact == n                              # (scene, cameras and tiles are fixed: none comes near the 98th evaluation)
    t.set_beam(32)


def kept_bounds(t, cam):
    """Frames of one view until a launch walks from kept bounds (the view is admitted at its second launch, which searches into a slot; the
    third walks from it): the floats of the slot that launch read, and that the counters say so."""
    hits0, fills0 = t.beam_cache_counters()
    for _ in range(4):
        t.draw_frame(cam)
        action, kept = t.beam_cache_last()
        if action == 2:
            break
    hits, fills = t.beam_cache_counters()
    assert action == 2 and hits > hits0 and fills == fills0 + 1, (action, (hits0, fills0), (hits, fills))
    return kept


@pytest.mark.parametrize("world", ["HIGH box"], indirect=True)
def test_kept_bounds_are_what_a_search_returns(world):
    """The bounds a launch WALKS from when the cache is on, read out of the slot (blok_hip_beam_cache_download), are the bits of a fresh
    search — before an edit, and after an edit and a rebuild, where stale bounds would be the old ones.  (beam_prepass itself never looks
    at the slots; it searches whatever set_beam_cache says, so the module's set_beam_cache(False) changes nothing for it.)"""
    t = world.t
    cam = world.cameras()["outside"]
    t.set_beam(32); t.set_beam_budget(0)
    before, _ = t.beam_prepass(cam, RECTS[0], want_visits=True)
    again, _ = t.beam_prepass(cam, RECTS[0], want_visits=True)
    assert np.array_equal(before.view(np.uint32), again.view(np.uint32))
    t.set_beam_cache(True)
    try:
        kept = kept_bounds(t, cam)
        assert np.array_equal(kept.view(np.uint32), before.view(np.uint32))
        # an edit and a rebuild: a tower in front of the camera
        o = world.origin
        cells = np.array([[o[0] + 90, o[1] + y, o[2] + 5] for y in range(30, 75)], np.int32)
        t.volume_set_voxels(cells, np.full(len(cells), 4, np.uint32), np.ones(len(cells), np.float32))
        t.volume_rebuild(world.mats)
        t.draw_frame(cam)
        assert t.beam_cache_last()[0] != 2, "the first launch over a new tree must not walk from bounds of the old one"
        fresh, _ = t.beam_prepass(cam, RECTS[0], want_visits=True)
        assert not np.array_equal(fresh.view(np.uint32), before.view(np.uint32)), "the tower must change some tile's bound"
        kept = kept_bounds(t, cam)
        assert np.array_equal(kept.view(np.uint32), fresh.view(np.uint32))
    finally:
        t.set_beam_cache(False)
        t.volume_upload(world.d, world.m)                             # the world back for whoever comes next
        t.volume_rebuild(world.mats)
