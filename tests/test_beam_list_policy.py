"""The state of a kept view's packed list as a table (blok_amd/csrc/hip/beam_cache.h: plan_beam_list, beam_list_commit, beam_list_drop,
beam_list_settle), on the host: the list follows its slot through fill, hit, refine, count, build, adoption, refill, eviction, clear and a
build that could not be issued; one build is in flight at a time, and one that finishes for a slot that was dropped meanwhile is adopted
by nobody.  No GPU."""
import ctypes as C
import os
import subprocess
from pathlib import Path

import pytest

ROOT = Path(__file__).resolve().parent.parent
SRC = ROOT / "tests" / "host_harness" / "beam_list_shim.cpp"
HDR = ROOT / "blok_amd" / "csrc" / "hip" / "beam_cache.h"
LIB = ROOT / "tests" / "host_harness" / "libbeam_list_shim.so"

SEARCH, FILL, HIT = range(3)
REFINE, FINE, COUNT, PACKED = 16, 32, 64, 128
NONE, NOW, BUILDING, READY = range(4)


def adopted(slot):
    return (slot + 1) << 8


@pytest.fixture(scope="module")
def lib():
    if not LIB.exists() or LIB.stat().st_mtime < max(SRC.stat().st_mtime, HDR.stat().st_mtime):
        subprocess.run(["g++", "-O1", "-std=c++20", "-fPIC", "-Wall", "-Wextra", "-Werror", f"-I{HDR.parent}", "-shared", "-o", os.fspath(LIB), os.fspath(SRC)], check=True)
    L = C.CDLL(os.fspath(LIB))
    L.beam_list_new.restype = C.c_void_p
    for name in ("beam_list_delete", "beam_list_reset", "beam_list_settle", "beam_list_after", "beam_list_building"):
        getattr(L, name).argtypes = [C.c_void_p]
    L.beam_list_set_after.argtypes = [C.c_void_p, C.c_uint]
    L.beam_list_state.argtypes = [C.c_void_p, C.c_int]
    L.beam_list_launch.argtypes = [C.c_void_p, C.POINTER(C.c_uint32), C.c_int, C.c_int, C.c_int, C.POINTER(C.c_int)]
    return L


class Cache:
    """K = 1 throughout: a view's launches are a search, a fill, the hit that refines, then hits from the finer bounds."""

    def __init__(self, L, after):
        self.L, self.s, self.n = L, L.beam_list_new(), L.beam_list_key_words()
        L.beam_list_set_after(self.s, after)

    def close(self):
        self.L.beam_list_delete(self.s)

    def ask(self, v, done=False, eligible=True, issued=1):
        """One launch of view v; done: the event behind the build in flight has been seen complete.  -> (flags, slot)."""
        slot = C.c_int(-7)
        words = (C.c_uint32 * self.n)(*[0x3F800000 + 977 * v + i for i in range(self.n)])
        return self.L.beam_list_launch(self.s, words, 1 if eligible else 0, 1 if done else 0, issued, C.byref(slot)), slot.value

    def refined(self, v):
        """View v from nothing to its finer bounds -> its slot."""
        assert self.ask(v)[0] == SEARCH
        action, slot = self.ask(v)
        assert action == FILL and self.state(slot) == NONE
        assert self.ask(v) == (HIT | REFINE, slot)
        return slot

    def state(self, slot):
        return self.L.beam_list_state(self.s, slot)

    def building(self):
        """-1, or the slot of the build in flight (+ 256 when that slot has been dropped since)."""
        return self.L.beam_list_building(self.s)


@pytest.fixture()
def make(lib):
    made = []

    def factory(after=1):
        made.append(Cache(lib, after))
        return made[-1]
    yield factory
    for c in made:
        c.close()


def test_the_default_is_the_measured_sixteen_hits_and_a_clear_keeps_the_setting(lib, make):
    assert lib.beam_list_default_after() == 16               # the count launch and the build over a packed frame's gain
    c = make(5)
    lib.beam_list_reset(c.s)
    assert lib.beam_list_after(c.s) == 5


@pytest.mark.parametrize("after", [1, 2, 5])
def test_fill_hit_refine_count_build_adopt(make, after):
    c = make(after)
    slot = c.refined(0)
    for _ in range(after - 1):
        assert c.ask(0) == (HIT | FINE, slot) and c.state(slot) == NONE
    assert c.ask(0) == (HIT | FINE | COUNT, slot)             # it walks from the finer bounds as the others do, and counts
    assert c.state(slot) == BUILDING and c.building() == slot
    for _ in range(3):
        assert c.ask(0) == (HIT | FINE, slot)                 # no launch waits for the build, none counts again
    assert c.ask(0, done=True) == (HIT | FINE | PACKED | adopted(slot), slot)      # the first launch that finds it finished
    assert c.state(slot) == READY and c.building() == -1
    for _ in range(2 * after + 3):
        assert c.ask(0, done=True) == (HIT | FINE | PACKED, slot)                 # never a second build


def test_between_the_plan_and_the_commit_the_state_is_count_now(make):
    c = make()
    slot = c.refined(0)
    assert c.ask(0, issued=-1) == (HIT | FINE | COUNT, slot)  # (-1: the shim leaves the commit out)
    assert c.state(slot) == NOW and c.building() == -1
    assert c.ask(0, issued=-1) == (HIT | FINE, slot)          # asked again before the commit: neither a second count nor a list


def test_a_build_that_could_not_be_issued_leaves_no_list_and_counts_again(make):
    c = make(2)
    slot = c.refined(0)
    assert c.ask(0) == (HIT | FINE, slot)
    assert c.ask(0, issued=0) == (HIT | FINE | COUNT, slot)
    assert c.state(slot) == NONE and c.building() == -1
    assert c.ask(0) == (HIT | FINE, slot)                     # N hits again
    assert c.ask(0) == (HIT | FINE | COUNT, slot) and c.state(slot) == BUILDING


def test_a_geometry_the_packed_walk_does_not_apply_to_never_counts(make):
    c = make()
    slot = c.refined(0)
    for _ in range(5):
        assert c.ask(0, eligible=False) == (HIT | FINE, slot)
    assert c.state(slot) == NONE
    assert c.ask(0) == (HIT | FINE | COUNT, slot)             # switched on later: its first eligible hit


def test_a_view_that_is_not_refined_has_no_list(make):
    c = make()
    for v in range(100, 130):                                 # a camera in motion
        assert c.ask(v) == (SEARCH, -1)
    assert all(c.state(k) == NONE for k in range(4)) and c.building() == -1


def test_one_build_at_a_time_the_second_view_waits_its_turn(make):
    c = make()
    a = c.refined(0)
    assert c.ask(0) == (HIT | FINE | COUNT, a)
    b = c.refined(1)
    assert c.ask(1) == (HIT | FINE, b) and c.state(b) == NONE                     # view 0's build is in flight: view 1 walks on as it is
    assert c.ask(1, done=True) == (HIT | FINE | COUNT | adopted(a), b)            # the launch that sees it finished adopts it for view 0 and counts for itself
    assert c.state(a) == READY and c.state(b) == BUILDING and c.building() == b
    assert c.ask(0) == (HIT | FINE | PACKED, a)
    assert c.ask(1, done=True) == (HIT | FINE | PACKED | adopted(b), b)


def test_a_refill_an_eviction_and_a_clear_drop_the_list(make, lib):
    c = make()
    slots = {}
    for v in range(4):                                        # four views at rest, all with their lists
        slots[v] = c.refined(v)
        assert c.ask(v) == (HIT | FINE | COUNT, slots[v])
        assert c.ask(v, done=True) == (HIT | FINE | PACKED | adopted(slots[v]), slots[v])
    assert sorted(slots.values()) == [0, 1, 2, 3] and all(c.state(k) == READY for k in range(4))
    # a fifth view evicts the one used longest ago (view 0): the list goes with the finer bounds, and the slot earns a new one
    assert c.ask(4) == (SEARCH, -1)
    assert c.ask(4) == (FILL, slots[0]) and c.state(slots[0]) == NONE
    assert c.ask(4) == (HIT | REFINE, slots[0])
    assert c.ask(4) == (HIT | FINE | COUNT, slots[0])
    assert c.ask(4, done=True) == (HIT | FINE | PACKED | adopted(slots[0]), slots[0])
    for v in (2, 3):
        assert c.ask(v) == (HIT | FINE | PACKED, slots[v])   # the others keep theirs
    # view 0 comes back: a refill of view 1's slot
    assert c.ask(0) == (SEARCH, -1)
    assert c.ask(0) == (FILL, slots[1]) and c.state(slots[1]) == NONE
    lib.beam_list_reset(c.s)
    assert all(c.state(k) == NONE for k in range(4))
    slot = c.refined(0)
    assert c.ask(0) == (HIT | FINE | COUNT, slot)


@pytest.mark.parametrize("how", ["refill", "clear"])
def test_a_build_that_finishes_for_a_dropped_slot_is_adopted_by_nobody_and_blocks_until_it_has_finished(make, lib, how):
    c = make()
    slot = c.refined(0)
    assert c.ask(0) == (HIT | FINE | COUNT, slot) and c.building() == slot
    if how == "clear":
        lib.beam_list_reset(c.s)
    else:                                                     # four other views: the last of them evicts view 0
        for v in range(1, 5):
            c.ask(v); last = c.ask(v)
        assert last == (FILL, slot)
    assert c.state(slot) == NONE and c.building() == slot + 256
    # whoever holds the slot now is refined, and does not count while the stale build still writes the slot's (and the context's) buffers
    v = 0 if how == "clear" else 4
    if how == "clear":
        assert c.refined(0) == slot
    else:
        assert c.ask(4) == (HIT | REFINE, slot)
    assert c.ask(v) == (HIT | FINE, slot) and c.state(slot) == NONE and c.building() == slot + 256
    assert c.ask(v, done=True) == (HIT | FINE | COUNT, slot)  # finished: nothing adopted; the slot's own build starts
    assert c.state(slot) == BUILDING and c.building() == slot
    assert c.ask(v, done=True) == (HIT | FINE | PACKED | adopted(slot), slot)


def test_behind_a_wait_for_the_device_no_build_is_in_flight_and_an_unadopted_list_is_not_kept(make, lib):
    c = make()
    slot = c.refined(0)
    assert c.ask(0) == (HIT | FINE | COUNT, slot)
    lib.beam_list_settle(c.s)
    assert c.state(slot) == NONE and c.building() == -1
    assert c.ask(0) == (HIT | FINE | COUNT, slot)             # counted again at once


def test_the_list_walk_runs_clean_under_the_sanitizers(tmp_path):
    """The shim as a stand-alone program (its own main), built with the address and undefined-behaviour sanitizers."""
    exe = tmp_path / "beam_list_policy_asan"
    subprocess.run(["g++", "-O1", "-g", "-std=c++20", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-DBEAM_LIST_SHIM_MAIN",
                    f"-I{HDR.parent}", "-o", os.fspath(exe), os.fspath(SRC)], check=True)
    r = subprocess.run([os.fspath(exe)], capture_output=True, text=True)
    assert r.returncode == 0 and "0 mismatches" in r.stdout, r.stdout + r.stderr
