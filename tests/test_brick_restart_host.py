"""A listed ray of a view at rest re-enters at the node its restarted walk ends in (blok_amd/csrc/hip/trace_core.h: restart_node_word,
walk_enter_node; beam_cache.h: mode 5), on the host, through tests/host_harness/node_restart_shim.cpp — the one-trip entry compiled by g++ from
the header text the kernels compile.  For every ray of tests/test_own_start_host.py's frames over the 64^3 scene the counted host walk leaves
(t_last, node, level); the entry then either settles the ray with a record byte-equal to the walk from the root at tmin = t_last, or says
"not settled".  The words are checked as numbers against a descent of the tree by the voxel's digits.

A spoilt word.  The entry cannot tell a wrong node or a wrong level BELOW the tree's from a right one — the word is state kept under the
view's key, like the start — so the deliberately wrong levels here are the ones it can and must refuse: every level the tree has not
(`levels` .. 7).  Those, and the 0xFFFFFFFF word, say "not settled" for every ray and load nothing but nodes[0] or the word's own node.  No GPU."""
import ctypes as C
import os
import subprocess
from pathlib import Path

import numpy as np
import pytest

from tests.test_own_start_host import HT, WD, cameras, tile_bounds

ROOT = Path(__file__).resolve().parent.parent
SRC = ROOT / "tests" / "host_harness" / "node_restart_shim.cpp"
HIP = ROOT / "blok_amd" / "csrc" / "hip"
DEPS = [SRC, HIP / "trace_core.h", HIP / "trace_kernels.h", HIP / "tree_build.cpp", HIP / "tree.h", ROOT / "tests" / "host_harness" / "host_harness_shims.h"]
LIB = ROOT / "tests" / "host_harness" / "libnode_restart_shim.so"
FLAGS = ["-O1", "-g", "-std=c++20", "-ffp-contract=off", "-Wall", "-Wextra", "-Werror", f"-I{ROOT / 'include'}", f"-I{HIP}", f"-I{SRC.parent}"]

NONE = 0xFFFFFFFF
HIT = np.dtype([("t", "<f4"), ("material_id", "<u4"), ("voxel", "<i2", 3), ("face", "u1"), ("hit", "u1")])


def shim():
    if not LIB.exists() or LIB.stat().st_mtime < max(d.stat().st_mtime for d in DEPS):
        subprocess.run(["g++", *FLAGS, "-fPIC", "-shared", "-o", os.fspath(LIB), os.fspath(SRC), os.fspath(HIP / "tree_build.cpp")], check=True)
    L = C.CDLL(os.fspath(LIB))
    L.nr_build.restype = C.c_void_p
    L.nr_build.argtypes = [C.c_void_p, C.c_size_t, C.c_void_p, C.c_size_t, C.POINTER(C.c_char_p)]
    L.nr_adopt.restype = C.c_void_p
    L.nr_adopt.argtypes = [C.c_void_p, C.c_size_t, C.c_void_p, C.c_size_t, C.c_void_p, C.c_uint32]
    L.nr_free.argtypes = [C.c_void_p]
    L.nr_levels.restype = C.c_uint32
    L.nr_levels.argtypes = [C.c_void_p]
    L.nr_tree_nodes.restype = C.c_void_p
    L.nr_tree_nodes.argtypes = [C.c_void_p, C.POINTER(C.c_size_t), C.c_void_p]
    L.nr_run.restype = C.c_uint32
    L.nr_run.argtypes = [C.c_void_p, C.c_void_p] + [C.c_uint32] * 6 + [C.c_void_p, C.c_void_p, C.c_int] + [C.c_void_p] * 7
    return L


class HostWorld:
    """A tree in the shim: built from a packed world by the host builder, or adopted as a device's download."""

    def __init__(self, L, handle):
        self.L, self.h = L, handle
        self.levels = int(L.nr_levels(C.c_void_p(handle)))
        n, origin = C.c_size_t(0), np.zeros(3, dtype=np.int32)
        p = L.nr_tree_nodes(C.c_void_p(handle), C.byref(n), C.c_void_p(origin.ctypes.data))
        self.nodes = np.ctypeslib.as_array(C.cast(p, C.POINTER(C.c_uint32)), shape=(n.value, 4)).copy()
        self.origin = origin

    @classmethod
    def build(cls, L, packed):
        why = C.c_char_p()
        h = L.nr_build(C.c_void_p(packed.nodes.ctypes.data), len(packed.nodes), C.c_void_p(packed.sub_chunks.ctypes.data), len(packed.sub_chunks), C.byref(why))
        assert h, why.value
        return cls(L, h)

    @classmethod
    def adopt(cls, L, nodes, materials, origin, levels):
        nodes, materials, origin = np.ascontiguousarray(nodes, dtype=np.uint32), np.ascontiguousarray(materials, dtype=np.uint32), np.ascontiguousarray(origin, dtype=np.int32)
        return cls(L, L.nr_adopt(C.c_void_p(nodes.ctypes.data), len(nodes), C.c_void_p(materials.ctypes.data), len(materials), C.c_void_p(origin.ctypes.data), levels))

    def close(self):
        self.L.nr_free(C.c_void_p(self.h))

    def run(self, cam, frame, rect, tstart=None, spoil=0, jitter_clip=None):
        """-> dict of per-pixel arrays (h, w): word, start, restarts, cell (h, w, 3), settled, entry and root records; and the node loads
        that were out of range."""
        (fw, fh), (x0, y0, w, h) = frame, rect
        cam = np.ascontiguousarray(cam)
        out = dict(word=np.zeros((h, w), dtype=np.uint32), start=np.zeros((h, w), dtype=np.float32), restarts=np.zeros((h, w), dtype=np.uint8),
                   cell=np.zeros((h, w, 3), dtype=np.int32), settled=np.zeros((h, w), dtype=np.uint8), entry=np.zeros((h, w), dtype=HIT), root=np.zeros((h, w), dtype=HIT))
        ts = None if tstart is None else np.ascontiguousarray(tstart, dtype=np.float32)
        jc = None if jitter_clip is None else np.ascontiguousarray(jitter_clip, dtype=np.float32)
        bad = self.L.nr_run(C.c_void_p(self.h), C.c_void_p(cam.ctypes.data), fw, fh, x0, y0, w, h, None if ts is None else C.c_void_p(ts.ctypes.data),
                            None if jc is None else C.c_void_p(jc.ctypes.data), spoil, *[C.c_void_p(out[k].ctypes.data) for k in ("word", "start", "restarts", "cell", "settled", "entry", "root")])
        return out, int(bad)


def descend(nodes, levels, cell, level):
    """The node whose children are the level-`level` cells, reached from the root by the digits of `cell` (tree coordinates), and the bit of the
    cell in it: (index, bit, occupied) — index None when a cell on the way is empty."""
    index = 0
    for lvl in range(levels - 1, level - 1, -1):
        bit = ((int(cell[0]) >> 2 * lvl) & 3) | (((int(cell[1]) >> 2 * lvl) & 3) << 2) | (((int(cell[2]) >> 2 * lvl) & 3) << 4)
        lo, hi, base = int(nodes[index, 0]), int(nodes[index, 1]), int(nodes[index, 2])
        mask = lo | (hi << 32)
        if lvl == level:
            return index, bit, bool((mask >> bit) & 1)
        if not (mask >> bit) & 1:
            return None, bit, False
        index = base + bin(mask & ((1 << bit) - 1)).count("1")
    raise AssertionError("level above the tree")


def word_errors(words, is_hit, voxels, cells, listed, nodes, origin, levels):
    """Everything that is wrong with per-pixel node words, as strings.  words (h, w) uint32; is_hit (h, w) bool and voxels (h, w, 3) world voxels
    from the frame's records; cells (h, w, 3): the start voxel of every ray's restarted interval in tree coordinates (the shim's); listed
    (h, w) bool: the pixels whose words count."""
    bad = []
    has = words != NONE
    level = (words >> 29).astype(int)
    index = (words & 0x1FFFFFFF).astype(int)
    if (listed & is_hit & ~has).any():
        bad.append(f"{int((listed & is_hit & ~has).sum())} hit pixels without a word")
    if (listed & is_hit & has & (level != 0)).any():
        bad.append(f"{int((listed & is_hit & has & (level != 0)).sum())} hit pixels whose word's level is not 0")
    if (listed & has & ((level >= levels) | (index >= len(nodes)))).any():
        bad.append("words whose level or index the tree has not")
        return bad
    wrong_node = wrong_bit = occupied_miss = 0
    for y, x in np.argwhere(listed & has):
        cell = voxels[y, x].astype(int) - origin if is_hit[y, x] else cells[y, x]
        want, bit, occupied = descend(nodes, levels, cell, int(level[y, x]))
        if want != int(index[y, x]):
            wrong_node += 1
        elif is_hit[y, x] and not occupied:
            wrong_bit += 1
        elif not is_hit[y, x] and occupied:
            occupied_miss += 1
    if wrong_node:
        bad.append(f"{wrong_node} words whose node is not the one the tree's descent by the cell's digits reaches")
    if wrong_bit:
        bad.append(f"{wrong_bit} hit pixels whose voxel's bit is not set in the word's node")
    if occupied_miss:
        bad.append(f"{occupied_miss} miss pixels whose cell at the word's level is occupied in the word's node")
    return bad


@pytest.fixture(scope="module")
def world(scene64):
    L = shim()
    w = HostWorld.build(L, scene64[1])
    yield w
    w.close()


@pytest.mark.parametrize("bounds", [False, True], ids=["from_tmin", "from_the_tiles_bounds"])
@pytest.mark.parametrize("name", ["from_outside", "inside_the_world_box", "inside_a_solid_voxel", "grazing"])
def test_the_entry_settles_with_the_walks_record_or_says_not_settled(world, scene64, name, bounds):
    cam = cameras(scene64)[name]
    plain, _ = world.run(cam, (WD, HT), (0, 0, WD, HT))
    tstart = None
    if bounds:
        hit = plain["root"]["hit"] == 1
        tstart = tile_bounds(np.where(hit, plain["root"]["t"], np.inf).astype(np.float32))
    got, out_of_range = world.run(cam, (WD, HT), (0, 0, WD, HT), tstart=tstart)
    assert out_of_range == 0
    settled, has = got["settled"] == 1, got["word"] != NONE
    same = got["entry"].view(np.uint8).reshape(HT, WD, 16) == got["root"].view(np.uint8).reshape(HT, WD, 16)
    assert same.all(axis=2)[settled].all(), f"{int((~same.all(axis=2) & settled).sum())} settled rays whose record is not the walk's from the root"
    assert np.array_equal(got["root"].view(np.uint8), plain["root"].view(np.uint8)), "the walk from a ray's own start is not the walk from tmin"
    assert np.array_equal(settled, has), f"{int((has & ~settled).sum())} rays with a word that their last trip does not settle; {int((settled & ~has).sum())} settled without one"
    assert np.array_equal(has, got["restarts"] != 0), "a ray has a word exactly when it made a trip"
    is_hit = got["root"]["hit"] == 1
    print(f"{name}: {int(settled.sum())} of {WD * HT} rays settled, {int(is_hit.sum())} hits; word levels {np.bincount((got['word'][has] >> 29).astype(int), minlength=world.levels).tolist()}")
    assert settled.sum() > 1000 and is_hit[settled].sum() > 1000
    errors = word_errors(got["word"], is_hit, got["root"]["voxel"], got["cell"], np.ones((HT, WD), dtype=bool), world.nodes, world.origin, world.levels)
    assert not errors, "; ".join(errors)
    assert (got["start"][is_hit].view(np.uint32) == got["root"]["t"][is_hit].view(np.uint32)).all()


@pytest.mark.parametrize("spoil", [1, 2], ids=["a_level_the_tree_has_not", "no_word"])
def test_a_spoilt_word_is_not_settled_and_reads_nothing_out_of_range(world, scene64, spoil):
    for name, cam in cameras(scene64).items():
        got, out_of_range = world.run(cam, (WD, HT), (0, 0, WD, HT), spoil=spoil)
        assert out_of_range == 0, name
        assert not got["settled"].any(), f"{name}: {int(got['settled'].sum())} rays settled by a spoilt word"
        assert (got["word"] != NONE).sum() > 1000, f"{name}: nothing was spoilt"


def test_the_checks_catch_a_word_of_the_neighbouring_node_and_a_level_off_by_one(world, scene64):
    cam = cameras(scene64)["from_outside"]
    got, _ = world.run(cam, (WD, HT), (0, 0, WD, HT))
    is_hit = got["root"]["hit"] == 1
    everything = np.ones((HT, WD), dtype=bool)
    y, x = np.argwhere(is_hit)[len(np.argwhere(is_hit)) // 2]
    for spoilt, text in ((got["word"][y, x] + 1, "is not the one the tree's descent"), (got["word"][y, x] | (1 << 29), "level is not 0")):
        words = got["word"].copy()
        words[y, x] = spoilt
        assert any(text in s for s in word_errors(words, is_hit, got["root"]["voxel"], got["cell"], everything, world.nodes, world.origin, world.levels))


def test_the_entry_runs_clean_under_the_sanitizers(tmp_path):
    """The shim as a stand-alone program (its own main) over a generated 64^3 world and a 4^3 one of one level, built with the address and
    undefined-behaviour sanitizers: every settled record is the walk's, no spoilt word settles, nothing is read out of range."""
    exe = tmp_path / "node_restart_asan"
    subprocess.run(["g++", *FLAGS, "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-DNODE_RESTART_SHIM_MAIN", "-o", os.fspath(exe), os.fspath(SRC),
                    os.fspath(HIP / "tree_build.cpp")], check=True)
    r = subprocess.run([os.fspath(exe)], capture_output=True, text=True)
    assert r.returncode == 0 and " 0 mismatches" in r.stdout, r.stdout + r.stderr
