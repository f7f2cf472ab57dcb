"""The beam cache's decisions as a table (blok_amd/csrc/hip/beam_cache.h: BeamKey, plan_beam_cache), on the host: a view is admitted when
its key arrives a second time in a row, hits from the third launch on, takes an empty slot or the one used longest ago, and every field
of the key decides on its own.  No GPU."""
import ctypes as C
import os
import subprocess
from pathlib import Path

import pytest

ROOT = Path(__file__).resolve().parent.parent
SRC = ROOT / "tests" / "host_harness" / "beam_cache_shim.cpp"
HDR = ROOT / "blok_amd" / "csrc" / "hip" / "beam_cache.h"
LIB = ROOT / "tests" / "host_harness" / "libbeam_cache_shim.so"

SEARCH, FILL, HIT = range(3)
# BeamKey, field by field (beam_cache.h): the camera's 14 floats, then one word each
FIELDS = [f"cam[{i}]" for i in range(14)] + ["x0", "y0", "w", "h", "frame_w", "frame_h", "beam_tile", "beam_budget", "tuning", "ray_mode", "levels",
                                             "origin[0]", "origin[1]", "origin[2]", "voxel_bits", "nodes_lo", "nodes_hi", "world_version", "tree_version"]


@pytest.fixture(scope="module")
def lib():
    if not LIB.exists() or LIB.stat().st_mtime < max(SRC.stat().st_mtime, HDR.stat().st_mtime):
        subprocess.run(["g++", "-O1", "-std=c++20", "-fPIC", "-Wall", "-Wextra", "-Werror", f"-I{HDR.parent}", "-shared", "-o", os.fspath(LIB), os.fspath(SRC)], check=True)
    L = C.CDLL(os.fspath(LIB))
    L.beam_cache_new.restype = C.c_void_p
    L.beam_cache_delete.argtypes = [C.c_void_p]
    L.beam_cache_reset.argtypes = [C.c_void_p]
    L.beam_cache_plan.argtypes = [C.c_void_p, C.POINTER(C.c_uint32), C.POINTER(C.c_int)]
    assert L.beam_cache_key_words() == len(FIELDS) and L.beam_cache_slots() == 4
    return L


class Cache:
    def __init__(self, L):
        self.L, self.s = L, L.beam_cache_new()

    def close(self):
        self.L.beam_cache_delete(self.s)

    def reset(self):
        self.L.beam_cache_reset(self.s)

    def ask(self, key):
        slot = C.c_int(-7)
        words = (C.c_uint32 * len(FIELDS))(*key)
        return self.L.beam_cache_plan(self.s, words, C.byref(slot)), slot.value


def view(v):
    return [0x3F800000 + 977 * v + i for i in range(len(FIELDS))]


@pytest.fixture()
def cache(lib):
    c = Cache(lib)
    yield c
    c.close()


def test_a_view_is_admitted_on_its_second_launch_in_a_row_and_hits_from_the_third(cache):
    assert cache.ask(view(0)) == (SEARCH, -1)
    action, slot = cache.ask(view(0))
    assert action == FILL and 0 <= slot < 4
    for _ in range(5):
        assert cache.ask(view(0)) == (HIT, slot)


def test_a_camera_in_motion_never_fills_and_never_evicts(cache):
    slots = {}
    for v in range(4):                                   # four views at rest take the four slots
        cache.ask(view(v)); slots[v] = cache.ask(view(v))[1]
    assert sorted(slots.values()) == [0, 1, 2, 3]
    for v in range(100, 200):                            # an orbit: no key twice
        assert cache.ask(view(v)) == (SEARCH, -1)
    for v in range(4):
        assert cache.ask(view(v)) == (HIT, slots[v])


def test_a_key_seen_before_but_not_in_the_previous_launch_is_not_admitted(cache):
    for _ in range(6):                                   # two views alternating from the start: never twice in a row
        assert cache.ask(view(0))[0] == SEARCH and cache.ask(view(1))[0] == SEARCH
    # each rests for two launches once: both are kept, and alternating hits from then on
    assert cache.ask(view(0))[0] == SEARCH and cache.ask(view(0))[0] == FILL
    assert cache.ask(view(1))[0] == SEARCH and cache.ask(view(1))[0] == FILL
    for _ in range(6):
        assert cache.ask(view(0))[0] == HIT and cache.ask(view(1))[0] == HIT


def test_the_slot_used_longest_ago_is_replaced(cache):
    slot = {}
    for v in range(4):
        cache.ask(view(v)); slot[v] = cache.ask(view(v))[1]
    for v in (0, 2, 3):                                  # view 1 is now the one used longest ago
        assert cache.ask(view(v)) == (HIT, slot[v])
    assert cache.ask(view(4)) == (SEARCH, -1)
    assert cache.ask(view(4)) == (FILL, slot[1])
    assert cache.ask(view(1)) == (SEARCH, -1)            # evicted: admitted afresh, into the next slot used longest ago (view 0's)
    assert cache.ask(view(1)) == (FILL, slot[0])
    for v in (2, 3, 4, 1):
        assert cache.ask(view(v))[0] == HIT
    assert cache.ask(view(0))[0] == SEARCH


def test_an_empty_slot_is_taken_before_any_view_is_replaced(cache):
    cache.ask(view(0)); first = cache.ask(view(0))[1]
    cache.ask(view(1)); second = cache.ask(view(1))[1]
    assert first != second
    assert cache.ask(view(0)) == (HIT, first)


def test_clearing_empties_the_slots_and_forgets_the_previous_key(cache):
    cache.ask(view(0)); cache.ask(view(0))
    assert cache.ask(view(0))[0] == HIT
    cache.reset()
    assert cache.ask(view(0))[0] == SEARCH               # not FILL: the launch before the reset does not count
    assert cache.ask(view(0))[0] == FILL


@pytest.mark.parametrize("field", range(len(FIELDS)), ids=FIELDS)
def test_every_field_of_the_key_decides_on_its_own(cache, field):
    key = view(3)
    cache.ask(key); cache.ask(key)
    assert cache.ask(key)[0] == HIT
    for bit in (0, 31):                                  # one ulp of a camera float; a sign
        other = list(key); other[field] ^= 1 << bit
        assert cache.ask(other) == (SEARCH, -1), FIELDS[field]
        assert cache.ask(key)[0] == HIT


def test_the_policy_walk_runs_clean_under_the_sanitizers(tmp_path):
    """The shim as a stand-alone program (its own main), built with the address and undefined-behaviour sanitizers."""
    exe = tmp_path / "beam_cache_policy_asan"
    subprocess.run(["g++", "-O1", "-g", "-std=c++20", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-DBEAM_CACHE_SHIM_MAIN",
                    f"-I{HDR.parent}", "-o", os.fspath(exe), os.fspath(SRC)], check=True)
    r = subprocess.run([os.fspath(exe)], capture_output=True, text=True)
    assert r.returncode == 0 and "0 mismatches" in r.stdout, r.stdout + r.stderr
