"""The edits that reach the shadow rays' last-occluder map (api.hip: update_sun_map) through gpu_volume_commit, as one table — TESTS ONLY.
Every writer tells the commit a box and a bit (gpu_build.h: Edit::MayFill); a writer that under-reports either keeps every array, tree and
first hit right and loses shadows.  A case is one edit of one family, spelled once as a list of steps and run twice: on a tracer
(Case.on_device) and on numpy arrays through the family's own reference (Case.on_model).  It declares the world box the edit may write
(None: the whole map is searched anew, as behind a scroll, or behind a fill whose committed box is the whole volume) and its class:

    fills            a tight map of the world before is too low for the world after (tests/test_sun_map_writers_cpu.py proves it);
    clears           filled cells become empty, none the other way: the map must stay as it is, bit for bit;
    writes_nothing   the arrays stay byte-equal.

The box is the one of tests/test_sun_map_gpu.py: the 64-cube at ORIGIN, which is the tree's cube, so that a box on a face of the volume
projects onto the rim of the map, where update_sun_map clamps its texel ranges.  The base content stays below TOP and the filling edits
build above it.  A clearing edit needs something to clear: its case adds solid boxes to the base content (Case.base), below TOP except
for the brush, which stays at the corner of edit_brush.  Coordinates are written box-local and moved to the world by
`shift` (the tightening cycle runs the same cases in a larger box, at two places far apart)."""
from __future__ import annotations

import numpy as np

from blok_amd import _ffi
from blok_amd import affine as A
from blok_amd import automaton as AU
from blok_amd import stamp as ST
from tests import affine_reference as AR
from tests import automaton_reference as AUR
from tests import columns_reference as CR
from tests import components_reference as KR
from tests import distance_reference as DR
from tests import flood_reference as FR
from tests import scroll_reference as SCR
from tests import shapes_reference as SHR
from tests import stamp_reference as SR
from tests import terrain_reference as TR
from tests import voxelize_meshes as VM
from tests import voxelize_reference as VR
from tests.terrain_cases import ISSUE
from tests.test_sun_map_gpu import CUBE, ORIGIN, TOP, corner_lo, sparse_content
from tests.volume_tree_reference import DenseModel

BASE_SEED = 41
FILLS, CLEARS, WRITES_NOTHING = "fills", "clears", "writes_nothing"


def box_model(size, first=7):
    g = np.stack(np.meshgrid(*[np.arange(n) for n in size], indexing="ij"), axis=-1).reshape(-1, 3).astype(np.int32)
    return g, (first + np.arange(len(g)) % 5).astype(np.uint32)


# column: the 3 x 40 x 2 model of edit_stamp; lying: the same on its side (long along x); pillar: what the scatter table places
MODELS = {"column": box_model((3, 40, 2)), "lying": box_model((40, 3, 2), 20), "pillar": box_model((2, 12, 2), 40)}
MODEL_IDS = {name: k for k, name in enumerate(MODELS)}                # model_create numbers a fresh context's models from 0, in this order


def create_models(t):
    ids = {name: t.model_create(*model) for name, model in MODELS.items()}
    assert ids == MODEL_IDS, ids
    return ids


class World:
    """The model's side: density and ids [z][y][x] of the volume's box at `origin`."""

    def __init__(self, d, m, origin):
        self.d, self.m, self.origin = np.ascontiguousarray(d), np.ascontiguousarray(m), tuple(int(c) for c in origin)

    @property
    def shape(self):
        return self.d.shape[::-1]

    def copy(self):
        return World(self.d.copy(), self.m.copy(), self.origin)

    def filled(self):
        with np.errstate(invalid="ignore"):
            return self.d > 0

    def slices(self, lo, hi):
        return tuple(slice(lo[a] - self.origin[a], hi[a] - self.origin[a]) for a in (2, 1, 0))


def terrain_params(d):
    p = _ffi.TerrainParams()
    for k, v in d.items():
        setattr(p, k, v)
    return p


def same_model(t, got, xyz, mm, tag):
    """The model `got` is the one model_create builds from the reference's list."""
    want = t.model_create(xyz, mm)
    gn, gm, gi = t.model_download(got)
    wn, wm, wi = t.model_download(want)
    assert gi == wi and gn.tobytes() == wn.tobytes() and gm.tobytes() == wm.tobytes(), (tag, gi, wi)


# ---- one step on the model: (world, args) -> what the entry returns ------------------------------------------------------------------------
def m_shapes(w, shapes):
    return SHR.apply(w.d, w.m, w.origin, shapes)


def m_affine(w, model, forward, lo, hi, mode, value):
    return AR.stamp(w.d, w.m, w.origin, *MODELS[model], A.from_matrix(np.asarray(forward, dtype=np.float64)), lo, hi, mode, value)


def m_stamp(w, model, place, mode, value):
    return SR.stamp(w.d, w.m, w.origin, *MODELS[model], place, mode, value)


def scatter_records(params, rows):
    return CR.params(**params), CR.entries([(MODEL_IDS[name], weight, anchor, sink) for name, weight, anchor, sink in rows])


def m_scatter(w, params, rows, value):
    top, material, info = CR.field(w.d, w.m, w.origin)
    table, counts = CR.scatter(top, material, info, *scatter_records(params, rows))
    name_of = {v: k for k, v in MODEL_IDS.items()}
    n = 0
    for rec in table:
        place = (tuple(int(c) for c in rec["offset"]), tuple(int(c) for c in rec["axis"]), int(rec["flip"]))
        n += SR.stamp(w.d, w.m, w.origin, *MODELS[name_of[int(rec["model"])]], place, SR.SET, value)
    return table, counts, n


def m_automaton(w, rule, lo, hi):
    w.d, w.m, info, counts, _ = AUR.run(w.d, w.m, w.origin, lo, hi, rule)
    return info, counts


def m_terrain(w, params, lo, hi):
    sl = w.slices(lo, hi)
    w.d[sl], w.m[sl] = TR.eval_box(params, lo, hi, w.d[sl], w.m[sl])
    return TR.written(params, lo, hi)


def m_voxelize(w, mesh, material, density, solid):
    filled, ids = VR.voxelize(*mesh, w.origin, w.shape, material=material, solid=solid)
    w.d[filled] = np.float32(density)
    w.m[filled] = ids[filled]
    return int(filled.sum())


def m_flood(w, lo, hi, seeds, K, flags, material, edits):
    steps, info = FR.field(w.d, w.m, w.origin, lo, hi, seeds, K, flags, material)
    return info, [FR.edit(w.d, w.m, steps, info, op, d, np.float32(value), mat, w.origin) for op, d, value, mat in edits]


def m_distance(w, lo, hi, radius, flags, op, d2, density, material):
    dist, info = DR.field(w.d, w.origin, lo, hi, radius, flags)
    return info, DR.edit(w.d, w.m, dist, info, op, d2, density, material, origin=w.origin)


def dense_of(w):
    model = DenseModel(w.origin, w.shape)
    model.density, model.ids = w.d, w.m
    return model


def m_brush(w, centre, radius, value, mode):
    model = dense_of(w)
    model.brush(centre, radius, value, mode)
    w.d, w.m = model.density, model.ids


def m_set_voxels(w, xyz, ids, density):
    model = dense_of(w)
    model.set_voxels(xyz, ids, density)
    w.d, w.m = model.density, model.ids


def m_capture(w, lo, hi):
    out = SR.capture(w.d, w.m, w.origin, lo, hi)
    SR.cut(w.d, w.m, w.origin, lo, hi)
    return out


def m_component(w, lo, hi):
    """Labels the region and cuts its largest component."""
    labels, records = KR.label(w.d, w.origin, lo, hi)
    rec = records[int(np.argmax(records["n_voxels"]))]
    snapshot = (labels, lo, hi)
    xyz, mm, _ = KR.members(w.d, w.m, w.origin, snapshot, rec)
    KR.clear_members(w.d, w.m, w.origin, snapshot, rec)
    return int(rec["label"]), xyz, mm, tuple(int(c) for c in rec["lo"])


def m_scroll(w, delta, terrain):
    info = SCR.info(w.d, w.m, w.origin, delta)
    exposed = SCR.plan(w.origin, w.shape, delta)["exposed"]
    w.d, w.m = SCR.scroll(w.d, w.m, delta)
    w.origin = tuple(o + s for o, s in zip(w.origin, delta))
    return info, [m_terrain(w, terrain, lo, hi) for lo, hi in exposed]


# ---- the same step on the device: (tracer, model ids, the reference's result, args) -> what the entry returned ----------------------------
def d_shapes(t, ids, want, shapes):
    return t.volume_apply_shapes(SHR.record(shapes))


def d_affine(t, ids, want, model, forward, lo, hi, mode, value):
    return t.volume_stamp_affine(A.from_matrix(np.asarray(forward, dtype=np.float64), ids[model]), lo, hi, mode, value)


def d_stamp(t, ids, want, model, place, mode, value):
    return t.volume_stamp_models(ST.placement(*place, model=ids[model]), mode, value)


def d_scatter(t, ids, want, params, rows, value):
    t.volume_column_field()
    counts = t.volume_scatter_models(*scatter_records(params, rows))
    table = t.volume_scatter_download()
    return table, counts, t.volume_stamp_models(table, _ffi.STAMP_SET, value)


def d_automaton(t, ids, want, rule, lo, hi):
    return t.volume_automaton(rule, lo, hi)


def d_terrain(t, ids, want, params, lo, hi):
    return t.volume_generate_terrain(terrain_params(params), lo, hi)


def d_voxelize(t, ids, want, mesh, material, density, solid):
    return t.volume_voxelize_mesh(*mesh, material=material, density=density, solid=solid)


def d_flood(t, ids, want, lo, hi, seeds, K, flags, material, edits):
    info = t.volume_flood_field(lo, hi, seeds=seeds, max_steps=K, flags=flags, material=material)
    return info, [t.volume_edit_by_flood(op, d, value, mat) for op, d, value, mat in edits]


def d_distance(t, ids, want, lo, hi, radius, flags, op, d2, density, material):
    info = t.volume_distance_field(lo, hi, max_radius=radius, to_empty=bool(flags & DR.TO_EMPTY), box_is_solid=bool(flags & DR.BOX_IS_SOLID))
    return info, t.volume_edit_by_distance(op, d2, density, material)


def d_brush(t, ids, want, centre, radius, value, mode):
    return t.volume_apply_brush(centre, radius, value, mode)


def d_set_voxels(t, ids, want, xyz, ids_, density):
    return t.volume_set_voxels(xyz, ids_, density)


def d_capture(t, ids, want, lo, hi):
    got = t.volume_capture_model(lo, hi, cut=True)
    assert t.last_capture_voxels == len(want[1]) > 0
    same_model(t, got, *want, "capture_model CUT")
    return want


def d_component(t, ids, want, lo, hi):
    label, xyz, mm, at = want
    t.volume_label_components(lo, hi)
    got, origin = t.volume_capture_component(label, cut=True)
    assert t.last_capture_voxels == len(mm) > 0
    same_model(t, got, xyz, mm, "capture_component CUT")
    return label, xyz, mm, origin


def d_scroll(t, ids, want, delta, terrain):
    from blok_amd import scroll as S
    info = t.volume_scroll(delta)
    return info, [t.volume_generate_terrain(terrain_params(terrain), lo, hi) for lo, hi in S.boxes(info, "exposed")]


STEPS = {"shapes": (m_shapes, d_shapes), "affine": (m_affine, d_affine), "stamp": (m_stamp, d_stamp), "scatter": (m_scatter, d_scatter),
         "automaton": (m_automaton, d_automaton), "terrain": (m_terrain, d_terrain), "voxelize": (m_voxelize, d_voxelize), "flood": (m_flood, d_flood),
         "distance": (m_distance, d_distance), "brush": (m_brush, d_brush), "set_voxels": (m_set_voxels, d_set_voxels), "capture": (m_capture, d_capture),
         "component": (m_component, d_component), "scroll": (m_scroll, d_scroll)}


def norm(x):
    """A result as nested tuples of ints and bytes (tests/volume_life.py: norm)."""
    if isinstance(x, np.ndarray):
        return (x.dtype.itemsize, np.ascontiguousarray(x).tobytes())
    if isinstance(x, (tuple, list)):
        return tuple(norm(v) for v in x)
    if isinstance(x, (np.integer, np.bool_)):
        return int(x)
    return x


class Case:
    """name; family (the entry it goes through); cls; box ((lo, hi) world voxels, or None for the whole map); steps [(kind, args)];
    base [(lo, hi)] boxes filled solid (density 1, id 3) in the base content; lattice_moves: the edit scrolls the box."""

    def __init__(self, name, family, cls, box, steps, base=(), lattice_moves=False):
        self.name, self.family, self.cls, self.box, self.steps, self.base, self.lattice_moves = name, family, cls, box, steps, tuple(base), lattice_moves

    def __repr__(self):
        return self.name

    def on_model(self, w):
        """The edit on the arrays, through the family's reference.  Returns the entries' results."""
        return [STEPS[kind][0](w, **args) for kind, args in self.steps]

    def on_device(self, t, ids, want):
        """The edit on the tracer's volume.  `want`: what on_model returned (a capture is compared where it is made)."""
        return [STEPS[kind][1](t, ids, w, **args) for (kind, args), w in zip(self.steps, want)]

    def world(self, origin=ORIGIN, shape=CUBE, seed=BASE_SEED, fill=0.01):
        """The base content for this case: the sprinkle below TOP and the case's own solid boxes."""
        d, m = sparse_content(shape, seed, fill=fill, top=TOP)
        w = World(d, m, origin)
        for lo, hi in self.base:
            sl = w.slices(lo, hi)
            w.d[sl], w.m[sl] = 1.0, 3
        return w


def changed(before, after):
    """(cells that became filled, cells that became empty) between two worlds over the same box."""
    assert before.origin == after.origin
    return int((~before.filled() & after.filled()).sum()), int((before.filled() & ~after.filled()).sum())


def table(shift=(0, 0, 0)):
    """The cases, their box-local coordinates moved to ORIGIN + shift."""
    o = tuple(ORIGIN[a] + shift[a] for a in range(3))
    P = lambda x, y, z: (o[0] + x, o[1] + y, o[2] + z)                                # a box-local cell, or corner, in the world
    B = lambda lo, size: (P(*lo), P(*(lo[a] + size[a] for a in range(3))))            # the world box of `size` cells at box-local `lo`
    at = lambda corner, size: tuple(c + s for c, s in zip(corner_lo(corner, size), shift))
    corner_box = lambda corner, size: (at(corner, size), tuple(c + n for c, n in zip(at(corner, size), size)))
    join = lambda *boxes: (tuple(min(b[0][a] for b in boxes) for a in range(3)), tuple(max(b[1][a] for b in boxes) for a in range(3)))
    clip = lambda box: (tuple(max(box[0][a], o[a]) for a in range(3)), tuple(min(box[1][a], o[a] + CUBE[a]) for a in range(3)))
    half = lambda cell: [2 * c + 1 for c in cell]                                      # a cell's centre in half-voxel units
    COLUMN = (3, 40, 2)

    def shape_box(*shapes):
        """The cells whose centres lie in the shapes' extents (shapes_reference.extent), cut with the volume."""
        boxes = []
        for s in shapes:
            e = [SHR.extent(s, k) for k in range(3)]
            boxes.append((tuple(-((1 - e[k][0]) // 2) for k in range(3)), tuple((e[k][1] - 1) // 2 + 1 for k in range(3))))
        return clip(join(*boxes))

    cases = []
    add = lambda *a, **kw: cases.append(Case(*a, **kw))

    # ---- apply_shapes ----
    s = [SHR.vbox(*corner_box(0b011, COLUMN), SHR.SET, material=5)]
    add("shapes SET column", "apply_shapes", FILLS, shape_box(*s), [("shapes", dict(shapes=s))])
    s = [SHR.shape(SHR.ELLIPSOID, SHR.KEEP, half(P(8, 52, 57)), r=(14, 22, 12), material=6, value=0.75)]
    add("shapes KEEP ellipsoid", "apply_shapes", FILLS, shape_box(*s), [("shapes", dict(shapes=s))])
    s = [SHR.shape(SHR.CAPSULE, SHR.ADD, half(P(60, 28, 30)), half(P(60, 59, 34)), r=(8, 0, 0), material=4, value=1.5)]
    add("shapes ADD capsule", "apply_shapes", FILLS, shape_box(*s), [("shapes", dict(shapes=s))])
    # two commit groups at opposite corners: the rebuild joins their boxes, and the join is the whole volume — a new world to the map
    s = [SHR.vbox(*corner_box(0b001, (20, 20, 20)), SHR.ERASE), SHR.vbox(*corner_box(0b110, COLUMN), SHR.SET, material=5)]
    add("shapes ERASE and SET in two far groups", "apply_shapes", FILLS, None, [("shapes", dict(shapes=s))])
    s = [SHR.vbox(*corner_box(0b010, COLUMN), SHR.SET, material=5), SHR.vbox(*B((0, 20, 0), (6, 10, 4)), SHR.SUBTRACT, value=0.0)]
    add("shapes SET under a SUBTRACT, one group", "apply_shapes", FILLS, shape_box(*s), [("shapes", dict(shapes=s))])
    a = P(0, 40, 30)
    s = [SHR.shape(SHR.CYLINDER, SHR.SET, (2 * a[0], 2 * a[1] + 1, 2 * a[2] + 1), (2 * a[0], 2 * a[1] + 81, 2 * a[2] + 1), r=(8, 0, 0), material=8)]
    add("shapes SET cylinder half outside", "apply_shapes", FILLS, shape_box(*s), [("shapes", dict(shapes=s))])
    s = [SHR.vbox(*B((0, 0, 40), (24, 20, 24)), SHR.ERASE), SHR.vbox(*B((20, 0, 0), (20, 20, 20)), SHR.PAINT, material=9),
         SHR.vbox(*B((0, 0, 0), (30, 20, 30)), SHR.REPLACE, material=2, match=9), SHR.vbox(*B((40, 0, 40), (24, 20, 24)), SHR.SUBTRACT, value=0.0),
         SHR.vbox(*B((30, 30, 30), (10, 20, 10)), SHR.ADD, value=0.0)]
    add("shapes that cannot fill", "apply_shapes", CLEARS, shape_box(*s), [("shapes", dict(shapes=s))])

    # ---- stamp_affine: the column lying along x in model space ----
    up = AR.rot(0.0, 0.0, 90.0)                                                       # model x -> world y, model y -> world -x
    region = B((8, 16, 58), (8, 48, 6))
    add("affine SET lattice rotation", "stamp_affine", FILLS, region,
        [("affine", dict(model="lying", forward=AR.forward(up, P(13, 20, 62)), lo=region[0], hi=region[1], mode=SR.SET, value=1.0))])
    # no region: in a 64-cube the host cull's one coarse tile is the whole volume, and so is the committed box
    add("affine KEEP twice the size", "stamp_affine", FILLS, None,
        [("affine", dict(model="lying", forward=AR.forward(2.0 * up, P(40, 4, 0)), lo=None, hi=None, mode=SR.KEEP, value=0.5))])
    region = B((30, 10, 40), (34, 54, 24))
    add("affine SET tilted", "stamp_affine", FILLS, region,
        [("affine", dict(model="lying", forward=AR.forward(AR.rot(20.0, 10.0, 70.0), [float(c) for c in P(50, 18, 50)]), lo=region[0], hi=region[1], mode=SR.SET,
                         value=1.25))])
    region = B((52, 40, 0), (12, 24, 6))
    add("affine SET cut in half by the region", "stamp_affine", FILLS, region,
        [("affine", dict(model="lying", forward=AR.forward(up, P(60, 20, 0)), lo=region[0], hi=region[1], mode=SR.SET, value=1.0))])
    region = B((0, 0, 0), (44, 4, 4))
    add("affine ERASE", "stamp_affine", CLEARS, region,
        [("affine", dict(model="lying", forward=AR.forward(np.eye(3), P(0, 0, 0)), lo=region[0], hi=region[1], mode=SR.ERASE, value=1.0))],
        base=[B((0, 0, 0), (40, 3, 2))])

    # ---- stamp_models ----
    box = B((61, 0, 62), COLUMN)
    add("stamp KEEP", "stamp_models", FILLS, box, [("stamp", dict(model="column", place=(box[0], (0, 1, 2), 0), mode=SR.KEEP, value=0.5))])
    box = B((0, 0, 62), COLUMN)
    add("stamp ERASE", "stamp_models", CLEARS, box, [("stamp", dict(model="column", place=(box[0], (0, 1, 2), 0), mode=SR.ERASE, value=1.0))],
        base=[B((0, 0, 62), (3, TOP, 2))])
    add("stamp of a scatter table", "stamp_models", FILLS, B((0, 0, 0), (64, TOP + 12, 64)),
        [("scatter", dict(params=dict(seed=5, flags=CR.ANY_MATERIAL, cell_log2=2), rows=[("pillar", 1, (0, 0, 0), 0)], value=1.0))])

    # ---- automaton ----
    region = B((22, TOP - 4, 0), (18, 12, 12))
    add("automaton dilate above a seed column", "automaton", FILLS, region,
        [("automaton", dict(rule=AU.dilate(6, steps=3, material=9), lo=region[0], hi=region[1]))],
        base=[B((28, 0, 0), (6, TOP, 6))])
    region = B((40, 56, 52), (12, 8, 12))
    add("automaton dilate, the box is solid", "automaton", FILLS, region,
        [("automaton", dict(rule=AU.dilate(6, steps=3, material=9, box_is_solid=True), lo=region[0], hi=region[1]))])
    region = B((0, 0, 0), (64, TOP, 32))
    add("automaton erode", "automaton", CLEARS, region,
        [("automaton", dict(rule=AU.erode(6, steps=2), lo=region[0], hi=region[1]))])

    # ---- terrain ----
    land = lambda flags, base: dict(ISSUE, flags=flags, amplitude=8, base_height=o[1] + base)
    region = B((44, 10, 0), (20, 40, 16))
    add("terrain ADD", "terrain", FILLS, region, [("terrain", dict(params=land(TR.ADD, 30), lo=region[0], hi=region[1]))])
    # a flat top: the highest voxel written stands in the measured box's own far corner along the sun, where the raise takes its depth —
    # over rolling heights that corner is air, and a box one layer short still reaches above every voxel
    region = B((30, 24, 50), (12, 30, 14))
    add("terrain ADD with a flat top", "terrain", FILLS, region,
        [("terrain", dict(params=dict(land(TR.ADD, 40), amplitude=0), lo=region[0], hi=region[1]))])
    region = B((0, 0, 40), (16, 48, 24))
    add("terrain replace", "terrain", FILLS, region, [("terrain", dict(params=land(0, 28), lo=region[0], hi=region[1]))])
    region = B((20, 40, 20), (16, 24, 16))
    add("terrain ADD below the region's floor", "terrain", WRITES_NOTHING, region, [("terrain", dict(params=land(TR.ADD, 10), lo=region[0], hi=region[1]))])

    # ---- voxelize ----
    lo, hi = P(60, 20, 60), P(64, 50, 64)
    mesh = VM.box([c + 0.25 for c in lo], [c - 0.25 for c in hi])
    add("voxelize a prism against two faces", "voxelize", FILLS, (lo, hi), [("voxelize", dict(mesh=mesh, material=6, density=1.0, solid=True))])

    # ---- flood ----
    region = B((30, TOP - 2, 59), (4, 27, 5))                                           # a seed under a lid, the 4 x 25 x 5 shaft above it
    add("flood FILL_UNREACHED a sealed shaft", "flood", FILLS, region,
        [("flood", dict(lo=region[0], hi=region[1], seeds=np.array([region[0]], np.int32), K=64, flags=0, material=0, edits=[(FR.FILL_UNREACHED, 0, 1.0, 7)]))],
        base=[B((30, TOP - 1, 59), (4, 1, 5))])
    region = B((38, 0, 0), (16, 6, 12))
    add("flood PAINT and CLEAR", "flood", CLEARS, region,
        [("flood", dict(lo=region[0], hi=region[1], seeds=np.array([P(40, 0, 0)], np.int32), K=64, flags=FR.THROUGH_FILLED, material=0,
                        edits=[(FR.PAINT, 64, 1.0, 33), (FR.CLEAR, 64, 1.0, 0)]))],
        base=[B((40, 0, 0), (12, 4, 10))])

    # ---- distance ----
    for name, op, x0 in (("SHRINK", DR.SHRINK, 10), ("HOLLOW", DR.HOLLOW, 50)):
        region = B((x0 - 2, 0, 50), (16, 14, 14))
        add(f"distance {name}", "distance", CLEARS, region,
            [("distance", dict(lo=region[0], hi=region[1], radius=3, flags=DR.TO_EMPTY, op=op, d2=1, density=1.0, material=0))], base=[B((x0, 0, 52), (12, 12, 12))])

    # ---- brush: both documented modes, value 0 and 1, at the corner of edit_brush; the class is what the reference does to the arrays ----
    centre = tuple(float(c) for c in (P(64, 64, 0)[0] - 2.5, P(64, 64, 0)[1] - 2.5, P(64, 64, 0)[2] + 2.5))
    box = B((59, 59, 0), (5, 5, 5))
    for mode, mode_name in ((0, "ADD"), (1, "SUBTRACT")):
        for value in (0.0, 1.0):
            case = Case(f"brush {mode_name} {value:g}", "brush", None, box, [("brush", dict(centre=centre, radius=2.49, value=value, mode=mode))],
                        base=[box] if mode == 1 else [])
            before = case.world(origin=o)
            after = before.copy()
            case.on_model(after)
            born, died = changed(before, after)
            same = after.d.tobytes() == before.d.tobytes() and after.m.tobytes() == before.m.tobytes()
            case.cls = FILLS if born else CLEARS if died else WRITES_NOTHING
            assert case.cls != WRITES_NOTHING or same, case
            cases.append(case)

    # ---- capture ----
    region = B((0, 0, 18), (10, 8, 12))
    add("capture_model CUT", "capture", CLEARS, region, [("capture", dict(lo=region[0], hi=region[1]))], base=[B((0, 0, 20), (8, 6, 8))])
    region = B((50, 0, 26), (14, 10, 16))
    add("capture_component CUT", "capture", CLEARS, region, [("component", dict(lo=region[0], hi=region[1]))], base=[B((56, 0, 30), (8, 6, 8))])

    # ---- scroll: the lattice moves, the map is searched anew ----
    column = [SHR.vbox(*corner_box(0b111, COLUMN), SHR.SET, material=5)]
    for delta in ((4, 0, 0), (0, -8, 4)):
        step = ("scroll", dict(delta=delta, terrain=land(0, 30)))
        add(f"scroll {delta} with terrain", "scroll", FILLS, None, [step], lattice_moves=True)
        add(f"scroll {delta} behind a SET column", "scroll", FILLS, None, [("shapes", dict(shapes=column)), step], lattice_moves=True)
    return cases


CASES = table()
BY_NAME = {c.name: c for c in CASES}
assert len(BY_NAME) == len(CASES)
FAMILIES = tuple(dict.fromkeys(c.family for c in CASES))
