"""CPU: the walk loop after its second pass over the generated code (trace_core.h: walk_loop, enter_axis, child_index, the single step of
walk_resume), against the oracle, on rays chosen where the changed instructions decide something:

  * enter_axis selects the probed corner instead of adding a selected increment: rays that enter a node exactly AT an interior plane, so
    that a probe's T equals the entry parameter (the comparison is <=);
  * the step advances ONE picked coordinate and puts it back with three selects: rays lying in node planes and on voxel edges, whose far
    planes tie between two or three axes (x, then y, then z);
  * the level is carried as the digit offset 2 * lvl and the loop's exits are one predicate: rays that leave the world on the step that would
    ascend past the root (through faces, edges and corners of the world box), rays whose interval ends inside the world, rays with a direction
    component below 1e-6 (the safe inverse);
  * the capped loop (the path kernel's tail pool): caps of 1, 2 and 7 trips, a cut walk started again from the root at the tCur it returned.

Two worlds: 64^3 (three levels) holding a few bricks, and the 256^3 scene (four levels) with its terrain shell.  Every record must equal the
oracle's field for field.  The last test runs the same rays through a program of its own built with ASan + UBSan (tests/host_harness/
walk_diet.cpp); nothing loaded into Python is sanitized."""
import ctypes as C
import os
import subprocess
from pathlib import Path

import numpy as np
import pytest

from blok_amd import world as W
from tests import oracle_ffi as O
from tests.conftest import records_equal

ROOT = Path(__file__).resolve().parent.parent
SRC = ROOT / "tests" / "host_harness"
CAPS = (1, 2, 7)
FLAGS = ["-O1", "-g", "-std=c++20", "-ffp-contract=off", "-Wall", f"-I{ROOT / 'include'}", f"-I{ROOT / 'blok_amd/csrc/hip'}", f"-I{SRC}"]
SOURCES = [os.fspath(SRC / "walk_diet.cpp"), os.fspath(ROOT / "blok_amd/csrc/hip/tree_build.cpp")]


# ---- the shim ---------------------------------------------------------------------------------------------------------------------------
def _build_shim() -> Path:
    out = SRC / "libwalk_diet.so"
    deps = [SRC / "walk_diet.cpp", SRC / "host_harness_shims.h"] + [ROOT / "blok_amd/csrc/hip" / n for n in ("trace_core.h", "trace_kernels.h", "tree_build.cpp", "tree.h")]
    if not out.exists() or any(d.stat().st_mtime > out.stat().st_mtime for d in deps):
        subprocess.run(["g++", *FLAGS, "-fPIC", "-shared", "-o", os.fspath(out), *SOURCES], check=True)
    return out


class Walker:
    """The walk over the tree the product's host builder makes of a packed world."""

    def __init__(self, pw):
        L = C.CDLL(os.fspath(_build_shim()))
        L.wd_build.restype = C.c_void_p
        L.wd_build.argtypes = [C.c_void_p, C.c_size_t, C.c_void_p, C.c_size_t, C.POINTER(C.c_char_p)]
        L.wd_free.argtypes = [C.c_void_p]
        L.wd_levels.restype = C.c_uint32
        L.wd_levels.argtypes = [C.c_void_p]
        L.wd_origin.argtypes = [C.c_void_p, C.c_void_p]
        L.wd_trace.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_uint32, C.c_void_p, C.POINTER(C.c_uint64), C.POINTER(C.c_uint32)]
        why = C.c_char_p()
        self.L = L
        self.h = L.wd_build(C.c_void_p(pw.nodes.ctypes.data), len(pw.nodes), C.c_void_p(pw.sub_chunks.ctypes.data), len(pw.sub_chunks), C.byref(why))
        assert self.h, why.value.decode()
        self.h = C.c_void_p(self.h)
        self.levels = int(L.wd_levels(self.h))
        o = (C.c_int32 * 3)()
        L.wd_origin(self.h, o)
        self.origin = np.array(list(o), dtype=np.float64)

    def __del__(self):
        if getattr(self, "h", None):
            self.L.wd_free(self.h)
            self.h = None

    def trace(self, rays, cap=0):
        """(records, cuts): cap 0 = the plain loop; otherwise the capped loop with restarts, and how often a walk was cut."""
        rays = np.ascontiguousarray(rays)
        out = np.zeros(len(rays), dtype=O.HIT)
        cuts, backwards = C.c_uint64(), C.c_uint32()
        self.L.wd_trace(self.h, C.c_void_p(rays.ctypes.data), len(rays), cap, C.c_void_p(out.ctypes.data), C.byref(cuts), C.byref(backwards))
        assert backwards.value == 0, "a cut walk returned a parameter below the one it started from"
        return out, int(cuts.value)


# ---- the worlds -------------------------------------------------------------------------------------------------------------------------
def bricks64():
    """64^3, three levels: full bricks in two opposite corners (they pin the tree to [0, 64)^3), a checkerboard brick, a plate across the
    centre planes of the root, single voxels on either side of node planes."""
    xyz, mat = [], []

    def box(lo, hi, m, keep=lambda x, y, z: True):
        for z in range(lo[2], hi[2]):
            for y in range(lo[1], hi[1]):
                for x in range(lo[0], hi[0]):
                    if keep(x, y, z):
                        xyz.append((x, y, z)); mat.append(m)

    box((0, 0, 0), (4, 4, 4), 1)
    box((60, 60, 60), (64, 64, 64), 2)
    box((16, 32, 20), (20, 36, 24), 3, lambda x, y, z: (x + y + z) % 2 == 0)
    box((24, 24, 31), (40, 40, 33), 4)
    box((28, 12, 44), (36, 20, 52), 5, lambda x, y, z: (x // 2 + y // 2 + z // 2) % 2 == 0)      # around the root's plane x = 32 and the level-1 plane y = 16
    box((44, 40, 4), (52, 56, 8), 6)
    box((8, 44, 40), (12, 60, 60), 7, lambda x, y, z: z % 4 != 3)
    for k, p in enumerate([(15, 15, 15), (16, 16, 16), (31, 32, 47), (47, 48, 15), (32, 0, 32), (63, 0, 0), (0, 63, 31), (48, 47, 48)]):
        xyz.append(p); mat.append(8 + k)
    cm = W.ChunkManager(128, 1.0)
    cm.set_voxels(np.array(xyz, dtype=np.int32), np.array(mat, dtype=np.uint32))
    cm.rebuild_dirty_chunks()
    return cm.pack_chunks_to_gpu_svo(W.scene_materials()), np.array(xyz, dtype=np.float64)


@pytest.fixture(scope="module")
def worlds(scene256):
    """name -> (walker, rays, the oracle's records): computed once, shared by every test, never changed."""
    out = {}
    bricks, brick_voxels = bricks64()
    cm256 = scene256[0]
    for name, pw in (("bricks64", bricks), ("scene256", scene256[1])):
        wk = Walker(pw)
        n = 4 ** wk.levels
        if name == "bricks64":
            filled = brick_voxels
        else:                                      # filled voxels of the scene: probe lattice points of the terrain's height range
            probe = np.random.default_rng(5).integers(0, n, size=(4000, 3))
            filled = np.array([q for q in probe if cm256.get_voxel_material(tuple(int(v) for v in q)) != 0], dtype=np.float64)
        rays = chosen_rays(wk.origin, n, filled, seed=len(name))
        ref, ctr = O.Lattice(pw.nodes, pw.sub_chunks).trace(rays, threads=4)
        for a in (rays, ref):
            a.setflags(write=False)
        out[name] = (wk, rays, ref, ctr, pw)
    assert out["bricks64"][0].levels == 3 and out["scene256"][0].levels == 4
    return out


# ---- the rays ---------------------------------------------------------------------------------------------------------------------------
def _ray(o, d, tmin, tmax):
    return (tuple(np.float32(o)), np.float32(tmin), tuple(np.float32(d)), np.float32(tmax))


def _unit(d):
    d = np.asarray(d, dtype=np.float64)
    return (d / np.linalg.norm(d)).astype(np.float32)


def _T(plane, o, d):
    """T(a, plane) as the kernel and the reference evaluate it (intersect.rint:48-49,79,179-180), in binary32."""
    d = np.float32(d)
    inv = np.float32(1.0) / (np.float32(1e-6) if abs(d) < np.float32(1e-6) else d)
    return np.float32(np.float32(np.float32(plane) - np.float32(o)) * inv)


def chosen_rays(origin, n, filled, seed):
    """A few hundred rays over a world [origin, origin + n)^3 with node planes every 4, 16, 64 voxels."""
    rng = np.random.default_rng(seed)
    rows = []
    sizes = [s for s in (1, 4, 16, 64) if s < n]
    axis_dirs = [(1, 0, 0), (-1, 0, 0), (0, 1, 0), (0, -1, 0), (0, 0, 1), (0, 0, -1)]
    tie_dirs = [(1, 1, 0), (1, -1, 0), (0, 1, 1), (-1, 0, 1), (1, 1, 1), (-1, -1, -1), (1, -1, 1), (-1, 1, 1)]
    # (a) in node planes and on voxel edges: origins on lattice points of a level (inside and outside the world), directions along axes and
    #     diagonals with equal components — the far planes of two or three axes tie at every step
    for _ in range(140):
        s = sizes[rng.integers(len(sizes))]
        o = origin + rng.integers(-1, n // s + 2, size=3) * float(s)
        d = (axis_dirs + tie_dirs)[rng.integers(len(axis_dirs) + len(tie_dirs))]
        rows.append(_ray(o, _unit(d), 0.0 if rng.random() < 0.5 else 0.001, 10000.0))
    # (b) entering a node exactly at an interior plane: tmin is T of an interior plane of some node (k * s, k = 1, 2, 3 inside a node of size
    #     4 s) on one axis, computed as the walk computes it, so a probe of enter_axis compares EQUAL to the entry parameter; with equal
    #     components the same holds on two or three axes at once
    for _ in range(140):
        s = sizes[rng.integers(len(sizes))]
        d = _unit((axis_dirs + tie_dirs)[rng.integers(len(axis_dirs) + len(tie_dirs))])
        a = int(np.flatnonzero(d)[rng.integers(np.count_nonzero(d))])
        o = origin + rng.integers(0, n, size=3).astype(np.float64)
        o[a] = origin[a] + (-3.0 if d[a] > 0 else n + 3.0)
        node = rng.integers(0, max(n // (4 * s), 1)) * 4 * s
        plane = origin[a] + node + s * int(rng.integers(1, 4))
        rows.append(_ray(o, d, max(float(_T(plane, o[a], d[a])), 0.0), 10000.0))
    # (c) a direction component below 1e-6 in magnitude (replaced by +1e-6 in the inverse), zero and negative ones included
    for _ in range(100):
        o = origin + rng.uniform(-0.25 * n, 1.25 * n, size=3)
        d = rng.normal(size=3)
        k = rng.integers(1, 3)
        for a in rng.permutation(3)[:k]:
            d[a] = rng.choice([0.0, 1e-7, -1e-7, 9.9e-7, -9.9e-7, 1e-12, -0.0])
        if not np.any(np.abs(d) > 1e-3):
            continue
        d = d / np.linalg.norm(d)
        rows.append(_ray(o, d.astype(np.float32), 0.001, 10000.0))
    # (d) leaving the world: through faces, along edges and through the corners of the box (the stepped coordinate reaches the world's far
    #     plane, alone or tied with others), from inside and from outside; and intervals that end inside the world
    far = origin + n
    for _ in range(120):
        kind = rng.integers(4)
        if kind == 0:                                                  # corner to corner and along the box's edges
            c = rng.integers(0, 2, size=3)
            o = np.where(c, far + 1.0, origin - 1.0)
            d = np.where(c, -1.0, 1.0) * rng.choice([1.0, 0.0], size=3, p=[0.7, 0.3])
            if not np.any(d):
                d = np.where(c, -1.0, 1.0)
            o = np.where(d == 0, np.where(c, far, origin), o)
        elif kind == 1:                                                # from inside, any direction: most leave without a report
            o = origin + rng.uniform(0, n, size=3)
            d = rng.normal(size=3)
        elif kind == 2:                                                # skimming a face of the box just inside it
            a = rng.integers(3)
            o = origin + rng.uniform(-0.2 * n, 1.2 * n, size=3)
            o[a] = (origin[a] if rng.random() < 0.5 else far[a]) + rng.choice([0.0, 1e-3, -1e-3, 0.5, -0.5])
            d = rng.normal(size=3)
            d[a] *= 1e-3
        else:                                                          # an interval that ends inside the world
            o = origin + rng.uniform(-0.1 * n, 1.1 * n, size=3)
            d = rng.normal(size=3)
        tmax = 10000.0 if kind != 3 else float(rng.uniform(0.5, 0.6 * n))
        rows.append(_ray(o, _unit(d), 0.001 if kind != 1 else 0.0, tmax))
    # (e) aimed at filled voxels — their centres, corners and edge midpoints — so that walks end in a report reached through descents, ties at
    #     the voxel's own planes included
    for _ in range(160):
        v = filled[rng.integers(len(filled))]
        target = v + rng.choice([0.0, 0.5, 1.0], size=3)
        o = origin + rng.uniform(-0.3 * n, 1.3 * n, size=3) if rng.random() < 0.7 else origin + rng.integers(-1, n // 4 + 2, size=3) * 4.0
        if np.allclose(o, target):
            continue
        rows.append(_ray(o, _unit(target - o), 0.001, 10000.0))
    return np.array(rows, dtype=O.RAY)


def _differences(got, ref, rays):
    bad = np.flatnonzero(~records_equal(got, ref))
    fields = [f for f in O.HIT.names if bad.size and not np.array_equal(got[f][bad], ref[f][bad])]
    return f"{bad.size} records differ in {fields}; first: ray {rays[bad[:1]]} got {got[bad[:1]]} want {ref[bad[:1]]}" if bad.size else ""


# ---- the tests --------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["bricks64", "scene256"])
def test_chosen_rays_equal_the_oracle_field_for_field(worlds, name):
    wk, rays, ref, ctr, _ = worlds[name]
    assert len(rays) >= 500
    hits, misses = int(ref["hit"].sum()), int((ref["hit"] == 0).sum())
    print(f"{name}: {len(rays)} rays, {hits} report a voxel, {misses} do not")
    assert hits >= 60 and misses >= 100            # both ends of the loop are exercised: a report, and the world or the interval left
    got, _ = wk.trace(rays)
    for f in O.HIT.names:
        assert np.array_equal(got[f], ref[f]), (f, _differences(got, ref, rays))
    assert records_equal(got, ref).all()


def test_the_chosen_rays_tie_and_probe_equal(worlds):
    """What makes the rays worth walking, from the rays and the formula of T alone: far planes that tie between axes, and entry parameters
    equal to an interior plane's T."""
    wk, rays, _, _, _ = worlds["bricks64"]
    ties = probes = tiny = 0
    for r in rays:
        d, o = r["dir"], r["org"]
        tiny += bool(np.any(np.abs(d) < np.float32(1e-6)))
        big = np.flatnonzero(np.abs(d) > 0.1)
        if len(big) >= 2:                      # two axes whose planes at equal distance from the origin have equal T
            p = np.float32(7.0)
            ties += _T(o[big[0]] + np.sign(d[big[0]]) * p, o[big[0]], d[big[0]]) == _T(o[big[1]] + np.sign(d[big[1]]) * p, o[big[1]], d[big[1]])
        for a in range(3):
            probes += any(_T(wk.origin[a] + q, o[a], d[a]) == r["tmin"] for q in range(1, 64) if q % 16) if r["tmin"] > 0.5 else 0
    print(f"ties {ties}, entry parameters on an interior plane {probes}, rays with a component below 1e-6: {tiny}")
    assert ties >= 50 and probes >= 50 and tiny >= 50


@pytest.mark.parametrize("cap", CAPS)
@pytest.mark.parametrize("name", ["bricks64", "scene256"])
def test_capped_loop_restarted_from_the_returned_parameter(worlds, name, cap):
    wk, rays, ref, _, _ = worlds[name]
    got, cuts = wk.trace(rays, cap=cap)
    print(f"{name}, cap {cap}: {cuts} cuts over {len(rays)} rays")
    assert cuts >= len(rays) // 4                  # the caps bite
    for f in O.HIT.names:
        assert np.array_equal(got[f], ref[f]), (f, _differences(got, ref, rays))


def test_walk_under_address_and_ub_sanitizers(worlds, tmp_path):
    """A program of its own over the same worlds, rays and expected records, the plain loop and every cap."""
    exe = tmp_path / "walk_diet_main"
    subprocess.run(["g++", *FLAGS, "-DWALK_DIET_MAIN", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-fno-omit-frame-pointer",
                    "-o", os.fspath(exe), *SOURCES], check=True)
    caps = np.array((0,) + CAPS, dtype=np.uint32)
    for name, (wk, rays, ref, _, pw) in worlds.items():
        case = tmp_path / f"{name}.case"
        with open(case, "wb") as f:
            f.write(np.array([len(pw.nodes), len(pw.sub_chunks), len(rays), len(caps)], dtype=np.uint64).tobytes())
            for a in (pw.nodes, pw.sub_chunks, rays, ref, caps):
                f.write(np.ascontiguousarray(a).tobytes())
        run = subprocess.run([os.fspath(exe), os.fspath(case)], capture_output=True, text=True)
        assert run.returncode == 0, run.stdout + run.stderr
        assert run.stderr == "", run.stderr
        lines = run.stdout.splitlines()
        assert len(lines) == len(caps) and all(f"rays {len(rays)} differ 0 " in l and l.endswith("backwards 0") for l in lines), run.stdout
