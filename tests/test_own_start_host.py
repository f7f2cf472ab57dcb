"""A listed ray of a view at rest restarts where its own counted walk ended (blok_amd/csrc/hip/beam_cache.h: BeamStartKey, plan_beam_starts;
trace_core.h: walk_loop), on the host.  Part 1, through the walk compiled for the host (tests/host_harness): a walk from the root with
per-pixel t0 = every hit's own t gives the records of the walk from the wave tiles' bounds, byte for byte, in exactly `levels` trips per hit
ray — from outside the world, from inside its box, from inside a solid voxel (the hit is at tmin) and for a grazing view whose rays leave
through the world's far side.  Part 2, through a shim: the policy of the starts — mode 4's states, the start key, every drop.  No GPU."""
import ctypes as C
import os
import subprocess
from pathlib import Path

import numpy as np
import pytest

from blok_amd import world as W

ROOT = Path(__file__).resolve().parent.parent
SRC = ROOT / "tests" / "host_harness" / "own_start_shim.cpp"
HDR = ROOT / "blok_amd" / "csrc" / "hip" / "beam_cache.h"
LIB = ROOT / "tests" / "host_harness" / "libown_start_shim.so"

WD, HT = 200, 136                                         # tests/test_beam_list_gpu.py's frame


def solid_voxel(scene64):
    """The centre of a filled voxel: a ray that starts inside it reports it at tmin, whichever way it looks."""
    from tests.conftest import SEED
    found = np.argwhere(W.scene_dense(64, SEED) != 0)        # [z, y, x], the scene of scene64
    z, y, x = found[len(found) // 2]
    return float(x) + 0.5, float(y) + 0.5, float(z) + 0.5


def cameras(scene64):
    sx, sy, sz = solid_voxel(scene64)
    a = np.radians(48.0)
    return {
        "from_outside": W.camera_look_at((32.0 + 95.0 * np.cos(a), 51.0, 32.0 + 95.0 * np.sin(a)), (32.0, 18.0, 32.0), 60.0, WD, HT),
        "inside_the_world_box": W.camera_look_at((30.3, 52.7, 33.1), (9.0, 11.0, 14.0), 70.0, WD, HT),
        "inside_a_solid_voxel": W.camera_look_at((sx + 0.13, sy - 0.21, sz + 0.07), (sx + 9.0, sy + 4.0, sz - 7.0), 60.0, WD, HT),
        "grazing": W.camera_look_at((-21.0, 31.3, 29.0), (120.0, 29.0, 41.0), 50.0, WD, HT),
    }


@pytest.fixture(scope="module")
def host(scene64):
    from tests import harness_ffi as H
    hk = H.HostKernel(scene64[1].nodes, scene64[1].sub_chunks)
    L = H.lib()
    L.hh_trace_rect_stats2.argtypes = [C.c_void_p] * 2 + [C.c_uint32] * 6 + [C.c_void_p] * 4

    def run(cam, ts):
        cam = np.ascontiguousarray(cam)
        out, it = np.zeros(WD * HT, dtype=H.HIT), np.zeros(WD * HT, dtype=np.uint32)
        L.hh_trace_rect_stats2(hk.h, C.c_void_p(cam.ctypes.data), WD, HT, 0, 0, WD, HT, None if ts is None else C.c_void_p(ts.ctypes.data), None,
                               C.c_void_p(out.ctypes.data), C.c_void_p(it.ctypes.data))
        return out, it.reshape(HT, WD)
    return run, hk.levels


def tile_bounds(t):
    """scripts/packed_walk_estimate.py's ideal bounds: per 8 x 8 wave tile grown by one pixel, the nearest hit less two voxels; a tile without a
    hit there starts at 0 (the host has no searches: any lower bound will do, and 0 is one)."""
    h, w = t.shape
    pad = np.pad(t, 1, constant_values=np.inf)
    near = np.full((h // 8, w // 8), np.inf, dtype=np.float32)
    for dy in range(10):
        for dx in range(10):
            near = np.minimum(near, pad[dy:dy + h:8, dx:dx + w:8])
    return np.where(np.isfinite(near), np.maximum(near - 2, 0), 0.0).astype(np.float32).repeat(8, axis=0).repeat(8, axis=1)


@pytest.mark.parametrize("name", ["from_outside", "inside_the_world_box", "inside_a_solid_voxel", "grazing"])
def test_a_walk_from_every_hits_own_t_gives_the_same_records_in_levels_trips(host, scene64, name):
    run, levels = host
    cam = cameras(scene64)[name]
    plain, it0 = run(cam, None)
    hit = (plain["hit"] == 1).reshape(HT, WD)
    t = np.where(hit, plain["t"].reshape(HT, WD), np.inf).astype(np.float32)
    bounds = np.ascontiguousarray(tile_bounds(t))
    from_tiles, it1 = run(cam, bounds)
    assert np.array_equal(plain.view(np.uint8), from_tiles.view(np.uint8)), "the wave tiles' bounds are no lower bounds"
    own = np.ascontiguousarray(np.where(hit, t, bounds).astype(np.float32))
    restarted, it2 = run(cam, own)
    print(f"{name}: {int(hit.sum())} hits of {WD * HT}, trips per hit ray {it1[hit].mean() if hit.any() else 0:.2f} from the tiles' bounds, {it2[hit].mean() if hit.any() else 0:.2f} restarted; levels {levels}")
    assert np.array_equal(restarted.view(np.uint8), from_tiles.view(np.uint8)), f"{int((restarted != from_tiles).sum())} records differ"
    assert hit.sum() > 1000 and (name == "inside_a_solid_voxel" or (~hit).sum() > 1000)
    assert (it2[hit] == levels).all(), f"restarted hit rays with other than {levels} trips: {np.bincount(it2[hit]).tolist()}"
    assert name == "inside_a_solid_voxel" or it1[hit].mean() > levels, "the restart saves nothing in this view: it says nothing"
    if name == "inside_a_solid_voxel":
        assert hit.all() and len(np.unique(plain["t"])) == 1, "the camera is not inside a solid voxel: the hits are not all at tmin"
    if name == "grazing":
        assert (it0[~hit] > 2 * levels).sum() > 1000, "no rays that cross the world and leave through its far side"


# ---- the policy ----------------------------------------------------------------------------------------------------------------------

SEARCH, FILL, HIT = range(3)
COUNT, PACKED, COUNT_OWN, USE, OTHER = 64, 128, 256, 1 << 9, 2 << 9
COUNTED = (0, 0, 0x3A83126F, 0x461C4000)                 # jitter x, jitter y, tmin, tmax as bits


@pytest.fixture(scope="module")
def lib():
    if not LIB.exists() or LIB.stat().st_mtime < max(SRC.stat().st_mtime, HDR.stat().st_mtime):
        subprocess.run(["g++", "-O1", "-std=c++20", "-fPIC", "-Wall", "-Wextra", "-Werror", f"-I{HDR.parent}", "-shared", "-o", os.fspath(LIB), os.fspath(SRC)], check=True)
    L = C.CDLL(os.fspath(LIB))
    L.own_start_new.restype = C.c_void_p
    L.own_start_new.argtypes = [C.c_int]
    for name in ("own_start_delete", "own_start_reset", "own_start_settle", "own_start_mode"):
        getattr(L, name).argtypes = [C.c_void_p]
    for name in ("own_start_list_state", "own_start_has", "own_start_set_mode"):
        getattr(L, name).argtypes = [C.c_void_p, C.c_int]
    L.own_start_launch.argtypes = [C.c_void_p, C.POINTER(C.c_uint32), C.POINTER(C.c_uint32), C.c_int, C.c_int, C.POINTER(C.c_int)]
    return L


class Cache:
    """K = 1 and N = 1 throughout: a view's launches are a search, a fill, the hit that refines, the hit that counts."""

    def __init__(self, L, own=True):
        self.L, self.s, self.n = L, L.own_start_new(1 if own else 0), L.own_start_key_words()

    def close(self):
        self.L.own_start_delete(self.s)

    def ask(self, v, key=COUNTED, done=False, issued=1):
        slot = C.c_int(-7)
        words = (C.c_uint32 * self.n)(*[0x3F800000 + 977 * v + i for i in range(self.n)])
        return self.L.own_start_launch(self.s, words, (C.c_uint32 * 4)(*key), 1 if done else 0, issued, C.byref(slot)), slot.value

    def listed(self, v, key=COUNTED):
        """View v from nothing to its adopted list, counted under `key` -> its slot."""
        assert self.ask(v, key)[0] == SEARCH
        assert self.ask(v, key)[0] == FILL
        flags, slot = self.ask(v, key)
        assert flags == HIT and not self.has(slot)
        assert self.ask(v, key) == (HIT | COUNT | (COUNT_OWN if self.L.own_start_mode(self.s) else 0), slot)
        assert self.ask(v, key, done=True)[0] & PACKED
        return slot

    def has(self, slot):
        return bool(self.L.own_start_has(self.s, slot))


@pytest.fixture()
def make(lib):
    made = []

    def factory(own=True):
        made.append(Cache(lib, own))
        return made[-1]
    yield factory
    for c in made:
        c.close()


def test_mode_4_counts_the_starts_with_the_list_and_packed_hits_of_the_counted_rays_use_them(make):
    c = make()
    slot = c.listed(0)
    assert c.has(slot)
    for _ in range(5):
        assert c.ask(0) == (HIT | PACKED | USE, slot)


def test_mode_3_has_a_list_and_no_starts(make):
    c = make(own=False)
    slot = c.listed(0)
    assert not c.has(slot)
    for key in (COUNTED, (1, 0, COUNTED[2], COUNTED[3])):
        assert c.ask(0, key) == (HIT | PACKED, slot)


@pytest.mark.parametrize("word", range(4), ids=["jitter_x", "jitter_y", "tmin", "tmax"])
def test_one_bit_of_the_start_key_walks_the_same_list_from_the_finer_bounds_and_the_starts_stay(make, lib, word):
    c = make()
    slot = c.listed(0)
    other = list(COUNTED); other[word] ^= 1
    for _ in range(3):
        assert c.ask(0, other) == (HIT | PACKED | OTHER, slot)                # the list, not its starts; no second count
    assert c.has(slot) and lib.own_start_list_state(c.s, slot) == 3
    assert c.ask(0) == (HIT | PACKED | USE, slot)                             # the counted values return
    minus_zero = list(COUNTED); minus_zero[0] = 0x80000000
    assert c.ask(0, minus_zero) == (HIT | PACKED | OTHER, slot)               # bit for bit: -0 is not 0


def test_the_start_key_is_the_count_launchs_whatever_the_launches_before_it_had(make):
    c = make()
    jittered = (0x3E800000, 0xBE800000, COUNTED[2], COUNTED[3])
    assert c.ask(0)[0] == SEARCH and c.ask(0)[0] == FILL and c.ask(0)[0] == HIT
    flags, slot = c.ask(0, jittered)
    assert flags == HIT | COUNT | COUNT_OWN
    assert c.ask(0, done=True) == (HIT | PACKED | OTHER, slot)
    assert c.ask(0, jittered) == (HIT | PACKED | USE, slot)


def test_a_build_that_could_not_be_issued_leaves_no_starts(make):
    c = make()
    assert c.ask(0)[0] == SEARCH and c.ask(0)[0] == FILL and c.ask(0)[0] == HIT
    flags, slot = c.ask(0, issued=0)
    assert flags == HIT | COUNT | COUNT_OWN and not c.has(slot)
    assert c.ask(0) == (HIT | COUNT | COUNT_OWN, slot) and c.has(slot)


def test_a_refill_an_eviction_a_clear_and_a_settle_drop_the_starts_with_the_list(make, lib):
    c = make()
    slots = {v: c.listed(v) for v in range(4)}
    assert sorted(slots.values()) == [0, 1, 2, 3] and all(c.has(k) for k in range(4))
    assert c.ask(4)[0] == SEARCH
    assert c.ask(4) == (FILL, slots[0]) and not c.has(slots[0])               # an eviction
    assert all(c.has(slots[v]) for v in (1, 2, 3))
    assert c.ask(0)[0] == SEARCH
    assert c.ask(0) == (FILL, slots[1]) and not c.has(slots[1])               # a refill
    lib.own_start_reset(c.s)                                                  # a clear (a world or tree version is another key: a refill)
    assert not any(c.has(k) for k in range(4)) and lib.own_start_mode(c.s) == 1
    assert c.ask(0)[0] == SEARCH and c.ask(0)[0] == FILL and c.ask(0)[0] == HIT
    flags, slot = c.ask(0)
    assert flags == HIT | COUNT | COUNT_OWN and c.has(slot)
    lib.own_start_settle(c.s)                                                 # behind a wait for the device an unadopted list is not kept
    assert lib.own_start_list_state(c.s, slot) == 0
    assert c.ask(0) == (HIT | COUNT | COUNT_OWN, slot)                        # counted again: the starts are that launch's


def test_the_mode_switched_off_in_mid_life_new_lists_have_no_starts(make, lib):
    c = make()
    a = c.listed(0)
    lib.own_start_set_mode(c.s, 0); lib.own_start_reset(c.s)                  # (blok_hip_set_beam_cache clears the slots)
    b = c.listed(0)
    assert not c.has(b) and c.ask(0) == (HIT | PACKED, b) and a == b


def test_the_policy_walk_runs_clean_under_the_sanitizers(tmp_path):
    """The shim as a stand-alone program (its own main), built with the address and undefined-behaviour sanitizers."""
    exe = tmp_path / "own_start_policy_asan"
    subprocess.run(["g++", "-O1", "-g", "-std=c++20", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-DOWN_START_SHIM_MAIN",
                    f"-I{HDR.parent}", "-o", os.fspath(exe), os.fspath(SRC)], check=True)
    r = subprocess.run([os.fspath(exe)], capture_output=True, text=True)
    assert r.returncode == 0 and "0 mismatches" in r.stdout, r.stdout + r.stderr
