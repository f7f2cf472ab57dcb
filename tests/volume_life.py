"""Mixed lives of the resident volume — TESTS ONLY.  One numpy model of a volume, `Life`, that composes the families' own references (it
holds no arithmetic of its own), and `schedule`, a seeded generator of lives in which every family of writers is followed by every family
of readers with no rebuild in between, edits of several families pool before one rebuild, and snapshots are consumed long after they were
taken, across scrolls and across writes into their regions.  tests/test_volume_life_cpu.py asserts the schedules' conditions and drives
the host builds through them; tests/test_volume_life_gpu.py drives the device.

A step is a dict: kind ("writer", "reader", "rebuild", "deferred"), family, tag, args.  Regions, seeds and placements are world voxels.
WRITE[family](life, **args) changes the model and returns what the entry returns; READ[family](d, m, origin, **args) is pure."""
from __future__ import annotations

import functools

import numpy as np

from blok_amd import _ffi
from blok_amd import affine as A
from tests import affine_reference as AR
from tests import bricks_reference as BR
from tests import columns_reference as CR
from tests import components_reference as KR
from tests import distance_reference as DR
from tests import flood_reference as FR
from tests import lod_reference as LR
from tests import quads_reference as QR
from tests import scroll_reference as SCR
from tests import shapes_reference as SHR
from tests import stamp_reference as SR
from tests import sweep_reference as SWR
from tests import terrain_reference as TR
from tests import voxelize_meshes as VM
from tests import voxelize_reference as VR
from tests.terrain_cases import ISSUE, prior
from tests.volume_tree_reference import DenseModel

ORIGIN, SHAPE = (-37, -21, 13), (88, 52, 44)
N_LIVES = 6
SEED = 0x11FE
WRITERS = ("upload", "set_voxels", "brush", "voxelize", "terrain", "stamp_models", "stamp_affine", "apply_shapes", "capture_cut", "component_cut",
           "restore", "edit_by_distance", "edit_by_flood", "scroll")
READERS = ("distance", "flood", "columns", "lod", "bricks", "quads", "components", "sweep", "capture")
CONSUMERS = ("edit_by_distance", "edit_by_flood", "restore", "component_cut", "scatter")
SNAPSHOT_OF = {"edit_by_distance": "distance", "edit_by_flood": "flood", "restore": "bricks", "component_cut": "components", "scatter": "columns"}
KINDS = ("quads", "bricks", "distance", "flood", "columns", "lod", "components")      # what a context holds at once
FOLLOWS_THE_BOX = ("distance", "flood", "columns", "components")                      # dropped by a scroll that cuts their region; the others stay
DROPPED = "dropped"
MODELS = dict(AR.MODELS)
MODELS["twin"] = (MODELS["block"][0], MODELS["block"][1] + np.uint32(7))              # the same voxels: a SET over the block changes ids only
SCATTER = (CR.params(seed=5, flags=_ffi.SCATTER_ANY_MATERIAL, cell_log2=1), CR.entries([(1, 3, (0, 0, 0), 0), (2, 1, (1, 0, 1), 1)]))


def content(seed=3):
    """terrain_cases.prior with the negative and NaN densities of test_stamp_gpu.prior_with_empties."""
    d, m = prior(SHAPE[::-1], seed=seed)
    d[::3, ::2, ::5] = -0.5
    d[1::7, ::3, ::2] = np.nan
    return np.ascontiguousarray(d), np.ascontiguousarray(m)


def norm(x):
    """A result as nested tuples of ints and bytes: equal results are equal objects (an array by its element size and bytes: the builds
    differ in how they shape a plane, not in what it holds)."""
    if isinstance(x, np.ndarray):
        return (x.dtype.itemsize, np.ascontiguousarray(x).tobytes())
    if isinstance(x, (tuple, list)):
        return tuple(norm(v) for v in x)
    if isinstance(x, (np.integer, np.bool_)):
        return int(x)
    return x


# ---- readers: pure functions of the arrays ------------------------------------------------------------------------------------------------
def read_columns(d, m, origin, lo, hi, axis, flags):
    top, material, info = CR.field(d, m, origin, lo, hi, axis, flags)
    if axis == 1 and not flags & CR.FROM_LOW:
        return top, material, info, *CR.scatter(top, material, info, *SCATTER)
    return top, material, info


READ = {
    "distance": lambda d, m, origin, lo, hi, radius, flags: DR.field(d, origin, lo, hi, radius, flags),
    "flood": lambda d, m, origin, lo, hi, seeds, K, flags, material: FR.field(d, m, origin, lo, hi, seeds, K, flags, material),
    "columns": read_columns,
    "lod": lambda d, m, origin, lo, hi, levels, flags: LR.reduce(d, m, origin, lo, hi, levels, flags),
    "bricks": lambda d, m, origin, lo, hi, flags: BR.encode(d, m, origin, lo, hi, flags),
    "quads": lambda d, m, origin, lo, hi, ignore: QR.extract(d, m, origin, lo, hi, ignore),
    "components": lambda d, m, origin, lo, hi: KR.label(d, origin, lo, hi),
    "sweep": lambda d, m, origin, table, direction, max_distance, flags: [SWR.sweep(d, origin, MODELS[name][0], place, direction, max_distance, flags)
                                                                          for name, place in table],
    "capture": lambda d, m, origin, lo, hi: SR.capture(d, m, origin, lo, hi),
}
KEEPS_A_SNAPSHOT = {"distance", "flood", "columns", "lod", "bricks", "quads", "components"}


class Life:
    """The model: density and ids [z][y][x], the box's origin, and per snapshot kind what the context holds: {"args", "want"} or DROPPED."""

    def __init__(self, seed=3):
        self.origin, self.shape = ORIGIN, SHAPE
        self.d, self.m = content(seed)
        self.snaps = {}

    @property
    def hi(self):
        return tuple(o + n for o, n in zip(self.origin, self.shape))

    def copy(self):
        out = object.__new__(Life)
        out.origin, out.shape, out.d, out.m, out.snaps = self.origin, self.shape, self.d.copy(), self.m.copy(), dict(self.snaps)
        return out

    def dense(self):
        """A DenseModel on these arrays (its edits replace or write them: take them back with `adopt`)."""
        model = DenseModel(self.origin, self.shape)
        model.density, model.ids = self.d, self.m
        return model

    def adopt(self, model):
        self.d, self.m = model.density, model.ids

    def apply(self, step):
        """One step on the model; returns the reference's result."""
        if step["kind"] == "rebuild":
            return None
        if step["kind"] == "reader":
            want = READ[step["family"]](self.d, self.m, self.origin, **step["args"])
            if step["family"] in KEEPS_A_SNAPSHOT:
                self.snaps[step["family"]] = {"args": step["args"], "want": want}
            return want
        return WRITE[step["family"]](self, **step["args"])

    def region_of(self, kind):
        """The world region a held snapshot was taken over."""
        a = self.snaps[kind]["args"]
        return tuple(a["lo"]), tuple(a["hi"])


# ---- writers ------------------------------------------------------------------------------------------------------------------------------
def write_upload(life, seed):
    life.d, life.m = content(seed)


def write_set_voxels(life, xyz, ids, density):
    model = life.dense()
    model.set_voxels(xyz, ids, density)
    life.adopt(model)


def write_brush(life, centre, radius, value, mode):
    model = life.dense()
    model.brush(centre, radius, value, mode)
    life.adopt(model)


def write_voxelize(life, mesh, material, density, solid):
    pos, tri = mesh
    filled, ids = VR.voxelize(pos, tri, life.origin, life.shape, material=material, solid=solid)
    life.d[filled] = np.float32(density)
    life.m[filled] = ids[filled]
    return int(filled.sum())


def terrain_dict(flags, base_height):
    return dict(ISSUE, flags=flags, base_height=base_height)


def write_terrain(life, params, lo, hi):
    sl = tuple(slice(lo[a] - life.origin[a], hi[a] - life.origin[a]) for a in (2, 1, 0))
    life.d[sl], life.m[sl] = TR.eval_box(params, lo, hi, life.d[sl], life.m[sl])
    return TR.written(params, lo, hi)


def write_stamp_models(life, table, mode, value):
    return sum(SR.stamp(life.d, life.m, life.origin, *MODELS[name], place, mode, value) for name, place in table)


def affine_record(forward):
    return A.from_matrix(np.asarray(forward, dtype=np.float64))


def write_stamp_affine(life, table, lo, hi, mode, value):
    return sum(AR.stamp(life.d, life.m, life.origin, *MODELS[name], affine_record(forward), lo, hi, mode, value) for name, forward in table)


def write_apply_shapes(life, shapes):
    return SHR.apply(life.d, life.m, life.origin, shapes)


def write_capture_cut(life, lo, hi):
    out = SR.capture(life.d, life.m, life.origin, lo, hi)
    SR.cut(life.d, life.m, life.origin, lo, hi)
    return out


def write_component_cut(life, label, cut=True):
    labels, records = life.snaps["components"]["want"]
    rec = records[records["label"] == label][0]
    snapshot = (labels, *life.region_of("components"))
    xyz, mm, _ = KR.members(life.d, life.m, life.origin, snapshot, rec)
    if cut:
        KR.clear_members(life.d, life.m, life.origin, snapshot, rec)
    return xyz, mm, tuple(int(c) for c in rec["lo"])


def write_restore(life, dst, keep_others, stream=None):
    """dst None: where it was taken.  stream None: the context's own snapshot (restore_bricks), else host arrays (decode_bricks)."""
    s = life.snaps["bricks"]["want"] if stream is None else stream
    life.d, life.m = BR.decode(life.d, life.m, life.origin, s, dst, BR.KEEP_OTHERS if keep_others else 0)
    life.d, life.m = np.ascontiguousarray(life.d), np.ascontiguousarray(life.m)


def write_edit_by_distance(life, op, d2, density, material):
    return DR.edit(life.d, life.m, *life.snaps["distance"]["want"], op, d2, density, material, origin=life.origin)


def write_edit_by_flood(life, op, d, density, material):
    return FR.edit(life.d, life.m, *life.snaps["flood"]["want"], op, d, np.float32(density), material, life.origin)


def write_scroll(life, delta, terrain=None):
    """The move, then terrain generated into each exposed box when asked.  Snapshots that follow the box are dropped when their region
    does not lie wholly in the new box (scroll_reference.inside)."""
    info = SCR.info(life.d, life.m, life.origin, delta)
    new_origin = tuple(o + s for o, s in zip(life.origin, delta))
    stays = SCR.inside(life.origin, life.shape, new_origin)
    for kind in FOLLOWS_THE_BOX:
        if life.snaps.get(kind, DROPPED) is not DROPPED:
            lo, hi = life.region_of(kind)
            sl = tuple(slice(lo[a] - life.origin[a], hi[a] - life.origin[a]) for a in (2, 1, 0))
            if not stays[sl].all():
                life.snaps[kind] = DROPPED
    life.d, life.m = SCR.scroll(life.d, life.m, delta)
    life.origin = new_origin
    counts = []
    if terrain is not None:
        for lo, hi in SCR.plan(tuple(o - s for o, s in zip(new_origin, delta)), life.shape, delta)["exposed"]:
            counts.append(write_terrain(life, terrain, lo, hi))
    return info, counts


def write_scatter(life):
    top, material, info = life.snaps["columns"]["want"][:3]
    return CR.scatter(top, material, info, *SCATTER)


WRITE = {"upload": write_upload, "set_voxels": write_set_voxels, "brush": write_brush, "voxelize": write_voxelize, "terrain": write_terrain,
         "stamp_models": write_stamp_models, "stamp_affine": write_stamp_affine, "apply_shapes": write_apply_shapes, "capture_cut": write_capture_cut,
         "component_cut": write_component_cut, "restore": write_restore, "edit_by_distance": write_edit_by_distance,
         "edit_by_flood": write_edit_by_flood, "scroll": write_scroll, "scatter": write_scatter}


# ---- what a step did, from the arrays alone -----------------------------------------------------------------------------------------------
def filled(d):
    with np.errstate(invalid="ignore"):
        return d > 0


def changed_cells(before, after):
    """Bool [z][y][x]: the cells whose two words differ.  `before` is read at the origin the box has afterwards (a scroll is judged against
    the arrays it found, as a move that left them where they were would leave them)."""
    return (before[0].view(np.uint32) != after[0].view(np.uint32)) | (before[1] != after[1])


def box_of(mask, origin):
    z, y, x = np.nonzero(mask)
    return (tuple(int(c.min()) + o for c, o in zip((x, y, z), origin)), tuple(int(c.max()) + 1 + o for c, o in zip((x, y, z), origin)))


def brick_occupancy(d):
    """Bool per box-local 4^3 brick (ragged last bricks padded)."""
    f = filled(d)
    pad = [(0, -n % 4) for n in f.shape]
    f = np.pad(f, pad)
    nz, ny, nx = f.shape
    return f.reshape(nz // 4, 4, ny // 4, 4, nx // 4, 4).any(axis=(1, 3, 5))


def emptied_bricks(before, after):
    return int((brick_occupancy(before) & ~brick_occupancy(after)).sum())


def bricks_in_an_empty_64_cell(before, after):
    """As test_masks_and_tree_follow_mixed_edits counts `seen`: bricks now filled in a slab x0 .. x0 + 64 of the box that held nothing."""
    now, n = brick_occupancy(after), 0
    for x0 in range(0, before.shape[2], 64):
        if not filled(before[:, :, x0:x0 + 64]).any():
            n += int(now[:, :, x0 // 4:(x0 + 64) // 4].sum())
    return n


# ---- drawing parameters -------------------------------------------------------------------------------------------------------------------
def region_near(life, rng, box, max_ext=(48, 32, 32), min_ext=(9, 7, 5)):
    """A region of at most max_ext cells inside the volume's box that holds a cell of `box`."""
    lo, hi = [], []
    for a in range(3):
        c = int(rng.integers(box[0][a], box[1][a]))
        ext = int(rng.integers(min_ext[a], min(max_ext[a], life.shape[a]) + 1))
        l = int(np.clip(c - int(rng.integers(0, ext)), life.origin[a], life.hi[a] - ext))
        lo.append(l); hi.append(l + ext)
    return tuple(lo), tuple(hi)


def central_region(life, rng):
    """A region at least 12 cells from every face of the box: a scroll by up to 12 cells keeps it."""
    lo = tuple(life.origin[a] + 12 + int(rng.integers(0, 5)) for a in range(3))
    hi = tuple(min(life.hi[a] - 12 - int(rng.integers(0, 5)), lo[a] + (48, 32, 32)[a]) for a in range(3))
    return lo, hi


def point_in(rng, lo, hi):
    return tuple(int(rng.integers(lo[a], hi[a])) for a in range(3))


def draw_reader(family, life, rng, box, cells=None, ids=False):
    """args of one reader whose region meets `box`; ids: a variant that reads material ids."""
    lo, hi = region_near(life, rng, box)
    if family == "distance":
        return dict(lo=lo, hi=hi, radius=int(rng.integers(2, 6)), flags=int(rng.choice(DR.ALL_FLAGS)))
    if family == "flood":
        sl = tuple(slice(lo[a] - life.origin[a], hi[a] - life.origin[a]) for a in (2, 1, 0))
        flags = FR.seed_face(int(rng.integers(0, 6))) | FR.seed_face(int(rng.integers(0, 6)))
        material = 0
        if ids or rng.random() < 0.3:
            flags |= FR.THROUGH_FILLED
            if ids or rng.random() < 0.5:
                flags |= FR.SAME_MATERIAL
                present, counts = np.unique(life.m[sl][filled(life.d[sl])], return_counts=True)
                material = int(present[counts.argmax()]) if present.size else 0      # the region's most common id
        seeds = np.array([point_in(rng, lo, hi) for _ in range(3)], dtype=np.int32)
        return dict(lo=lo, hi=hi, seeds=seeds, K=int(rng.integers(8, 41)), flags=flags, material=material)
    if family == "columns":
        return dict(lo=lo, hi=hi, axis=int(rng.integers(0, 3)), flags=int(rng.integers(0, 2)) * CR.FROM_LOW)
    if family == "lod":
        return dict(lo=lo, hi=hi, levels=int(rng.integers(1, 4)), flags=int(rng.integers(0, 2)) * LR.VOTE_EXPOSED)
    if family == "bricks":
        return dict(lo=lo, hi=hi, flags=int(rng.integers(0, 2)) * BR.FILLED_ONLY)
    if family == "quads":
        return dict(lo=lo, hi=hi, ignore=False if ids else bool(rng.integers(0, 2)))
    if family in ("components", "capture"):
        return dict(lo=lo, hi=hi)
    assert family == "sweep"
    z, y, x = np.nonzero(cells)
    table = []
    for name in ("small", "block"):
        k = int(rng.integers(0, len(x)))
        v = MODELS[name][0][int(rng.integers(0, len(MODELS[name][0])))]
        offset = tuple(int(c) + o - int(s) for c, o, s in zip((x[k], y[k], z[k]), life.origin, v))      # a model voxel lands on a changed cell
        table.append((name, (offset, (0, 1, 2), 0)))
    return dict(table=table, direction=int(rng.integers(0, 6)), max_distance=int(rng.integers(5, 60)), flags=int(rng.integers(0, 2)) * SWR.BOX_IS_SOLID)


READS_IDS = {"columns", "lod", "bricks", "quads", "flood", "capture"}


def shape_of(kind, op, centre, rng):
    c2 = [2 * c + 1 for c in centre]
    kw = dict(material=int(rng.integers(1, 9)), match=int(rng.integers(5, 9)), value=float(rng.choice([0.25, 0.75, 1.5])))
    if kind == SHR.BOX:
        return SHR.shape(kind, op, [c - int(rng.integers(5, 19)) for c in c2], [c + int(rng.integers(5, 19)) for c in c2], **kw)
    if kind == SHR.ELLIPSOID:
        return SHR.shape(kind, op, c2, r=[int(rng.integers(6, 20)) for _ in range(3)], **kw)
    b = [c + int(rng.integers(-16, 17)) for c in c2]
    return SHR.shape(kind, op, c2, b, r=[int(rng.integers(5, 13)), 0, 0], **kw)


def draw_writer(family, life, rng, mode, focus=None):
    """(args, tag) of one writer of the family in its mode number `mode`; focus: a world region the edit should land in."""
    lo, hi = (life.origin, life.hi) if focus is None else focus
    at_lo = [max(l, o + 6) for l, o in zip(lo, life.origin)]      # six cells from every face: the largest brush stays in the box
    at = point_in(rng, at_lo, [max(min(h, e - 6), l + 1) for h, e, l in zip(hi, life.hi, at_lo)])
    if family == "upload":
        seed = int(rng.integers(4, 1000))
        return dict(seed=seed), f"upload seed {seed}"
    if family == "set_voxels":
        n = int(rng.integers(20, 200))
        xyz = np.clip(np.asarray(at) + rng.integers(-5, 6, size=(n, 3)), life.origin, np.asarray(life.hi) - 1).astype(np.int32)
        density = rng.choice(np.array([0.0, -1.0, 0.5, 1.0, 2.0], np.float32), n).astype(np.float32)
        return dict(xyz=xyz, ids=rng.integers(1, 250, n).astype(np.uint32), density=density), f"set_voxels {n}"
    if family == "brush":
        add = mode % 2 == 0
        centre = tuple(float(c) + 0.5 for c in at)
        return dict(centre=centre, radius=float(rng.choice([2.5, 4.0, 5.5])), value=1.0 if add else 0.0, mode=0 if add else 1), "brush " + ("add" if add else "dig")
    if family == "voxelize":
        solid = bool(mode % 2)
        c, r = [float(v) + float(rng.random()) for v in at], float(rng.uniform(3.5, 6.0))
        mesh = VM.octahedron(c, r) if rng.random() < 0.5 else VM.box([v - r for v in c], [v + r for v in c])
        return dict(mesh=mesh, material=int(rng.integers(1, 250)), density=1.5, solid=solid), "voxelize " + ("solid" if solid else "surface")
    if family == "terrain":
        flags = (0, 1, 4, 3, 5, 0)[mode % 6]
        rlo, rhi = region_near(life, rng, (at, tuple(c + 1 for c in at)))
        base = life.origin[1] + int(rng.integers(10, 30))
        return dict(params=terrain_dict(flags, base), lo=rlo, hi=rhi), "terrain " + {0: "solid", 1: "shell", 3: "closed shell", 4: "additive", 5: "additive shell"}[flags]
    if family == "stamp_models":
        m = (SR.SET, SR.KEEP, SR.ERASE)[mode % 3]
        table = []
        for name in rng.choice(["small", "large", "block", "sparse"], size=2, replace=False):
            axis, flip = SR.ORIENTATIONS[int(rng.integers(0, len(SR.ORIENTATIONS)))]
            offset = at if name != "sparse" else tuple(int(c) - 30 for c in at)
            table.append((str(name), (tuple(int(c) + int(rng.integers(-3, 4)) for c in offset), axis, flip)))
        return dict(table=table, mode=m, value=float(rng.choice([0.5, 1.0, 2.0]))), "stamp_models " + ("SET", "KEEP", "ERASE")[m]
    if family == "stamp_affine":
        m = (SR.SET, SR.KEEP, SR.ERASE)[mode % 3]
        name = str(rng.choice(["small", "large", "block", "sparse"]))
        scale = {"small": 3.0, "large": 0.8, "block": 1.7, "sparse": 0.3}[name] * float(rng.uniform(0.8, 1.3))
        forward = AR.forward(scale * AR.rot(float(rng.uniform(0, 360)), float(rng.uniform(-40, 40)), float(rng.uniform(-40, 40))), [float(c) + 0.37 for c in at])
        whole = rng.random() < 0.5
        rlo, rhi = (None, None) if whole else region_near(life, rng, (at, tuple(c + 1 for c in at)), max_ext=(80, 40, 36), min_ext=(30, 20, 16))
        return dict(table=[(name, forward)], lo=rlo, hi=rhi, mode=m, value=float(rng.choice([0.5, 1.25]))), "stamp_affine " + ("SET", "KEEP", "ERASE")[m]
    if family == "apply_shapes":
        shapes = [shape_of(SHR.KINDS[(mode + k) % 4], SHR.OPS[(4 * mode + k) % 7], [c + int(rng.integers(-4, 5)) for c in at], rng) for k in range(4)]
        return dict(shapes=shapes), "apply_shapes " + " ".join(("SET", "KEEP", "ERASE", "PAINT", "REPLACE", "ADD", "SUBTRACT")[s["op"]] for s in shapes)
    if family == "capture_cut":
        rlo, rhi = region_near(life, rng, (at, tuple(c + 1 for c in at)), max_ext=(30, 20, 20))
        return dict(lo=rlo, hi=rhi), "capture CUT"
    if family == "component_cut":
        labels, records = life.snaps["components"]["want"]
        snapshot = (labels, *life.region_of("components"))
        order = np.argsort(records["n_voxels"])[::-1]
        for k in order[int(rng.integers(0, 3)):]:
            if len(KR.members(life.d, life.m, life.origin, snapshot, records[k])[1]):
                return dict(label=int(records[k]["label"])), "capture_component CUT"
        return None, "no component is left"
    if family == "restore":
        ext = [int(e) for e in life.snaps["bricks"]["want"][0]["ext"][0]]
        if mode % 3 == 0:
            return dict(dst=None, keep_others=False), "restore_bricks in place"
        dst = tuple(int(rng.integers(life.origin[a], life.hi[a] - ext[a] + 1)) for a in range(3))
        if (dst[0] - life.origin[0]) % 4 == 0:
            dst = (dst[0] + (1 if dst[0] + 1 + ext[0] <= life.hi[0] else -1),) + dst[1:]
        keep = bool(rng.integers(0, 2))
        if mode % 3 == 1:
            return dict(dst=dst, keep_others=keep), "restore_bricks moved off the brick grid"
        d0, m0 = content(seed=11)
        src_lo = tuple(ORIGIN[a] + int(rng.integers(0, SHAPE[a] - ext[a] + 1)) for a in range(3))
        stream = BR.encode(d0, m0, ORIGIN, src_lo, tuple(src_lo[a] + ext[a] for a in range(3)), BR.FILLED_ONLY if keep else 0)
        return dict(dst=dst, keep_others=keep, stream=stream), "decode_bricks of a host stream"
    if family == "edit_by_distance":
        info = life.snaps["distance"]["want"][1]
        op = DR.GROW if not int(info["flags"][0]) & DR.TO_EMPTY else (DR.SHRINK, DR.HOLLOW)[mode % 2]
        d2 = int(rng.integers(1, int(info["max_radius"][0]) ** 2 + 1)) if op != DR.HOLLOW else int(rng.integers(1, 4))
        return dict(op=op, d2=d2, density=0.75, material=int(rng.integers(1, 250))), "edit_by_distance " + ("GROW", "SHRINK", "HOLLOW")[op]
    if family == "edit_by_flood":
        info = life.snaps["flood"]["want"][1]
        if int(info["flags"][0]) & FR.THROUGH_FILLED:
            op = (FR.PAINT, FR.CLEAR)[mode % 2]
        else:
            op = (FR.FILL, FR.FILL_UNREACHED)[mode % 2]
        d = int(rng.integers(1, int(info["max_steps"][0]) + 1))
        return dict(op=op, d=d, density=1.25, material=int(rng.integers(1, 250))), "edit_by_flood " + ("FILL", "FILL_UNREACHED", "PAINT", "CLEAR")[op]
    assert family == "scroll"
    delta = [0, 0, 0]
    for a in ([int(rng.integers(0, 3))] if mode % 2 else range(3)):
        drift = life.origin[a] - ORIGIN[a]
        step = int(rng.choice([4, 8])) * (1 if rng.random() < 0.5 else -1)
        delta[a] = step if abs(drift + step) <= 12 else -step
    terrain = terrain_dict(0, life.origin[1] + 20) if mode % 3 == 0 else None
    return dict(delta=tuple(delta), terrain=terrain), f"scroll {tuple(delta)}" + (" with terrain" if terrain else "")


def distance_flags_for(mode):
    return 0 if mode % 3 == 0 else DR.TO_EMPTY


# ---- the generator --------------------------------------------------------------------------------------------------------------------------
class Builder:
    def __init__(self, index):
        self.index, self.rng = index, np.random.default_rng(SEED + index)
        self.life, self.steps = Life(), []
        self.age = {}                                             # writers since each snapshot was taken
        self.last_box = (self.life.origin, self.life.hi)
        self.last_cells = None
        self.occurrences = {}
        self.last_tag = "upload"

    def add(self, kind, family, args, tag, **extra):
        step = dict(kind=kind, family=family, args=args, tag=tag, **extra)
        if kind == "reader":
            step["after"] = self.last_tag
        else:
            self.last_tag = tag
        self.life.apply(step)
        self.steps.append(step)
        if kind == "reader" and family in KEEPS_A_SNAPSHOT:
            self.age[family] = 0
        if kind in ("writer", "deferred") and family != "scatter":
            for k in self.age:
                self.age[k] += 1
        return step

    def reader(self, family, ids=False, args=None, **extra):
        if args is None:
            args = draw_reader(family, self.life, self.rng, self.last_box, self.last_cells, ids)
        return self.add("reader", family, args, READER_TAGS[family](args), **extra)

    def need(self, family, mode, force=False):
        """Takes the snapshot a consumer needs when the context holds none that fits (force: anyway)."""
        kind = SNAPSHOT_OF[family]
        held = DROPPED if force else self.life.snaps.get(kind, DROPPED)
        args = None
        if family == "edit_by_distance":
            flags = distance_flags_for(mode)
            if held is DROPPED or (int(held["want"][1]["flags"][0]) & DR.TO_EMPTY) != flags:
                args = dict(draw_reader("distance", self.life, self.rng, self.last_box), flags=flags | int(self.rng.integers(0, 2)) * DR.BOX_IS_SOLID)
        elif family == "edit_by_flood":
            through = FR.THROUGH_FILLED if mode % 3 == 2 else 0
            if held is DROPPED or (int(held["want"][1]["flags"][0]) & FR.THROUGH_FILLED) != through:
                args = draw_reader("flood", self.life, self.rng, self.last_box)
                args["flags"] = (args["flags"] & ~(FR.THROUGH_FILLED | FR.SAME_MATERIAL)) | through
        elif held is DROPPED:
            args = draw_reader(kind, self.life, self.rng, self.last_box)
        if family == "restore" and args is None and not self.bricks_fit():
            args = draw_reader("bricks", self.life, self.rng, self.last_box)
        if args is not None:
            self.reader(kind, args=args)

    def bricks_fit(self):
        lo, hi = self.life.region_of("bricks")
        return all(self.life.origin[a] <= lo[a] and hi[a] <= self.life.hi[a] for a in range(3))

    def writer(self, family, readers=(), mode=None, focus=None, ids_only=False, must=None, retake=False):
        """One writer whose parameters are redrawn until it changes the volume and every reader of `readers` (family, reads ids) sees it.
        retake: a consumer whose snapshot leaves it nothing to do may take a new one."""
        if mode is None:
            mode = self.index + self.occurrences.get(family, 0)
        self.occurrences[family] = self.occurrences.get(family, 0) + 1
        if family in SNAPSHOT_OF:
            self.need(family, mode)
        for attempt in range(90):
            if retake and family in SNAPSHOT_OF and attempt % 10 == 9:
                self.last_box = (self.life.origin, self.life.hi)
                self.need(family, mode, force=True)
            args, tag = draw_writer(family, self.life, self.rng, mode, focus)
            if args is None:
                self.need(family, mode, force=True)
                continue
            trial = self.life.copy()
            before = (self.life.d, self.life.m)
            trial.apply(dict(kind="writer", family=family, args=args))
            cells = changed_cells(before, (trial.d, trial.m))
            if not cells.any() or (must is not None and not must(before, (trial.d, trial.m), cells)):
                continue
            if ids_only and (filled(before[0]) != filled(trial.d)).any():
                continue
            box = box_of(cells, trial.origin)
            drawn = []
            for reader, ids in readers:
                for _ in range(8):
                    rargs = draw_reader(reader, trial, self.rng, box, cells, ids)
                    if reader == "capture" and not filled(trial.d[tuple(slice(rargs["lo"][a] - trial.origin[a], rargs["hi"][a] - trial.origin[a]) for a in (2, 1, 0))]).any():
                        continue
                    if norm(READ[reader](*before, trial.origin, **rargs)) != norm(READ[reader](trial.d, trial.m, trial.origin, **rargs)):
                        drawn.append((reader, rargs))
                        break
            if len(drawn) == len(readers):
                break
        else:
            raise AssertionError(f"life {self.index}: no {family} (mode {mode}) changes what {readers} read")
        age = self.age.get(SNAPSHOT_OF.get(family), 0)
        own = family in SNAPSHOT_OF and not (family == "restore" and args.get("stream") is not None)
        step = self.add("deferred" if own and age >= 2 else "writer", family, args, tag, ids_only=ids_only)
        self.last_box, self.last_cells = box, cells
        for reader, rargs in drawn:
            self.reader(reader, args=rargs, pair=family)
        return step

    def rebuild(self):
        self.add("rebuild", "rebuild", {}, "rebuild")


READER_TAGS = {
    "distance": lambda a: f"distance_field R {a['radius']} flags {a['flags']}",
    "flood": lambda a: f"flood_field K {a['K']} flags {a['flags']:#x}",
    "columns": lambda a: f"column_field along {'xyz'[a['axis']]}" + (" from low" if a["flags"] else ""),
    "lod": lambda a: f"reduce {a['levels']} levels flags {a['flags']}",
    "bricks": lambda a: f"encode_bricks flags {a['flags']}",
    "quads": lambda a: "extract_quads" + (" ignoring material" if a["ignore"] else ""),
    "components": lambda a: "label_components",
    "sweep": lambda a: f"sweep_models direction {a['direction']}",
    "capture": lambda a: "capture_model",
}


def readers_of(writer_index, life_index):
    """The readers that follow writer family number `writer_index` in life `life_index`: over the six lives, all nine."""
    return [READERS[r] for r in range(len(READERS)) if (r + writer_index) % N_LIVES == life_index]


@functools.lru_cache(maxsize=None)
def _schedule(index):
    b = Builder(index)
    rng, life = b.rng, b.life
    # condition g: a writer that empties whole bricks, then one that fills bricks of a 64-cell that holds nothing
    slab = (tuple(o + (64 if a == 0 else 0) for a, o in enumerate(life.origin)), life.hi)
    b.add("writer", "apply_shapes", dict(shapes=[SHR.vbox(*slab, SHR.ERASE)]), "apply_shapes ERASE the far 64-cell")
    b.writer(("stamp_models", "voxelize", "terrain", "stamp_affine", "set_voxels", "brush")[index], mode=0 if index != 2 else 2,
             focus=(tuple(c + 6 for c in slab[0]), tuple(c - 6 for c in slab[1])), must=lambda before, after, cells: bricks_in_an_empty_64_cell(before[0], after[0]) > 0)
    # condition f: every snapshot kind held at once
    for kind in KINDS:
        args = draw_reader(kind, life, rng, central_region(life, rng))
        if kind == "columns":
            args.update(axis=1, flags=0)
        b.reader(kind, args=args)
    b.rebuild()
    # condition a: every writer family, each followed by this life's share of the readers; condition c: three families pool before a rebuild
    for n, w in enumerate(range(index, index + len(WRITERS))):
        family = WRITERS[(3 * w) % len(WRITERS)]
        mode = None
        if family == "edit_by_flood":
            mode = (0, 1, 5)[index % 3]                           # FILL, FILL_UNREACHED, CLEAR: PAINT changes ids only (below)
        if family == "restore":
            mode = 1 + index % 2                                  # moved, or a host stream: in place it is the consumer of life 2 (below)
        b.writer(family, [(r, False) for r in readers_of(WRITERS.index(family), index)], mode=mode, retake=True)
        if n % 3 == 2:
            b.rebuild()
    b.rebuild()
    # a writer that changes ids only, read by a reader of ids; a reader of occupancy must see no change
    which = index % 4
    if which == 3:
        at = point_in(rng, tuple(c + 8 for c in life.origin), tuple(c - 8 for c in life.hi))
        place = (at, (0, 1, 2), 0)
        b.add("writer", "stamp_models", dict(table=[("block", place)], mode=SR.SET, value=1.0), "stamp_models SET the block")
        before = life.copy()
        b.add("writer", "stamp_models", dict(table=[("twin", place)], mode=SR.SET, value=1.0), "stamp_models SET the twin", ids_only=True)
        cells = changed_cells((before.d, before.m), (life.d, life.m))
        b.last_box, b.last_cells = box_of(cells, life.origin), cells
        ids_reader = READERS[3 + index % 3]
        for _ in range(20):
            args = draw_reader(ids_reader, life, rng, b.last_box, cells, True)
            if norm(READ[ids_reader](before.d, before.m, life.origin, **args)) != norm(READ[ids_reader](life.d, life.m, life.origin, **args)):
                break
        b.reader(ids_reader, args=args, pair="stamp_models")
    else:
        if which == 2:
            b.writer("edit_by_flood", [("lod", True)], mode=2, ids_only=True)
        else:
            for _ in range(60):
                at = point_in(rng, tuple(c + 8 for c in life.origin), tuple(c - 8 for c in life.hi))
                shapes = [shape_of(SHR.KINDS[(index + k) % 4], (SHR.PAINT, SHR.REPLACE)[which], at, rng) for k in range(2)]
                trial = life.copy()
                if SHR.apply(trial.d, trial.m, trial.origin, shapes) and (trial.m != life.m).any():
                    break
            cells = changed_cells((life.d, life.m), (trial.d, trial.m))
            before = life.copy()
            b.add("writer", "apply_shapes", dict(shapes=shapes), "apply_shapes " + ("PAINT", "REPLACE")[which], ids_only=True)
            b.last_box, b.last_cells = box_of(cells, life.origin), cells
            ids_reader = ("bricks", "quads")[which]
            for _ in range(20):
                args = draw_reader(ids_reader, life, rng, b.last_box, cells, True)
                if norm(READ[ids_reader](before.d, before.m, life.origin, **args)) != norm(READ[ids_reader](life.d, life.m, life.origin, **args)):
                    break
            b.reader(ids_reader, args=args, pair="apply_shapes")
    b.reader(("distance", "components", "sweep")[index % 3], equality_only=True)
    # conditions d and e: a snapshot, a write inside its region, a scroll that keeps it, a later small edit, its consumer, one rebuild
    consumer = CONSUMERS[index % len(CONSUMERS)]
    kind = SNAPSHOT_OF[consumer]
    region = central_region(life, rng)
    args = draw_reader(kind, life, rng, region)
    args.update(lo=region[0], hi=region[1])
    if kind == "columns":
        args.update(axis=1, flags=0)
    if kind == "distance":
        args.update(flags=DR.TO_EMPTY, radius=4)
    if kind == "flood":
        args.update(flags=FR.ALL_FACES, material=0, seeds=None)
    b.reader(kind, args=args)
    inside = (tuple(c + 4 for c in region[0]), tuple(c - 4 for c in region[1]))
    b.rebuild()
    b.writer("brush", mode=0, focus=inside)
    b.writer("scroll", mode=index)
    assert life.snaps[kind] is not DROPPED
    b.writer("set_voxels", focus=inside)
    if consumer == "scatter":
        b.add("deferred", "scatter", {}, "scatter_models")
    else:
        step = b.writer(consumer, mode={"edit_by_distance": 1 + index % 2, "edit_by_flood": index % 2, "restore": 0}.get(consumer, 0))
        assert step["kind"] == "deferred"
    b.rebuild()
    return tuple(b.steps)


def schedule(life_index, keyed=True):
    """The steps of life `life_index`.  Both brick layouts live the same lives: a result that differs between them is a finding."""
    return list(_schedule(int(life_index)))


def replay(steps):
    """Yields (index, step, (d, m, origin) before the step, the life after it, the reference's result)."""
    life = Life()
    for i, step in enumerate(steps):
        before = (life.d.copy(), life.m.copy(), life.origin)
        want = life.apply(step)
        yield i, step, before, life, want


def label(life_index, i, step):
    """What a failure reads as: "life 2, step 31: after stamp_affine KEEP, column_field along z"."""
    return f"life {life_index}, step {i}: " + (f"after {step['after']}, " if "after" in step else "") + step["tag"]
