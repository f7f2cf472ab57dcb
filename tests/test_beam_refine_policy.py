"""When a kept view's finer bounds are searched, as a table (blok_amd/csrc/hip/beam_cache.h: plan_beam_refine, beam_refine_commit), on the
host: "refine now" is said exactly once per fill, on the view's K-th hit; never for a view that is searched but not admitted; the state
starts over with every refill, eviction and clear; K = 1, and a K no view ever reaches.  No GPU."""
import ctypes as C
import os
import subprocess
from pathlib import Path

import pytest

ROOT = Path(__file__).resolve().parent.parent
SRC = ROOT / "tests" / "host_harness" / "beam_refine_shim.cpp"
HDR = ROOT / "blok_amd" / "csrc" / "hip" / "beam_cache.h"
LIB = ROOT / "tests" / "host_harness" / "libbeam_refine_shim.so"

SEARCH, FILL, HIT = range(3)
REFINE, FINE = 16, 32
NONE, NOW, DONE = range(3)


@pytest.fixture(scope="module")
def lib():
    if not LIB.exists() or LIB.stat().st_mtime < max(SRC.stat().st_mtime, HDR.stat().st_mtime):
        subprocess.run(["g++", "-O1", "-std=c++20", "-fPIC", "-Wall", "-Wextra", "-Werror", f"-I{HDR.parent}", "-shared", "-o", os.fspath(LIB), os.fspath(SRC)], check=True)
    L = C.CDLL(os.fspath(LIB))
    L.beam_refine_new.restype = C.c_void_p
    L.beam_refine_delete.argtypes = [C.c_void_p]
    L.beam_refine_reset.argtypes = [C.c_void_p]
    L.beam_refine_set_after.argtypes = [C.c_void_p, C.c_uint]
    L.beam_refine_after.argtypes = [C.c_void_p]
    L.beam_refine_state.argtypes = [C.c_void_p, C.c_int]
    L.beam_refine_launch.argtypes = [C.c_void_p, C.POINTER(C.c_uint32), C.c_int, C.c_int, C.POINTER(C.c_int)]
    return L


class Cache:
    def __init__(self, L, after):
        self.L, self.s, self.n = L, L.beam_refine_new(), L.beam_refine_key_words()
        L.beam_refine_set_after(self.s, after)

    def close(self):
        self.L.beam_refine_delete(self.s)

    def reset(self):
        self.L.beam_refine_reset(self.s)

    def view(self, v):
        return [0x3F800000 + 977 * v + i for i in range(self.n)]

    def ask(self, v, eligible=True, issued=1):
        """One launch of view v -> (action | REFINE | FINE, slot)."""
        slot = C.c_int(-7)
        words = (C.c_uint32 * self.n)(*self.view(v))
        return self.L.beam_refine_launch(self.s, words, 1 if eligible else 0, issued, C.byref(slot)), slot.value

    def state(self, slot):
        return self.L.beam_refine_state(self.s, slot)


@pytest.fixture()
def make(lib):
    made = []

    def factory(after):
        made.append(Cache(lib, after))
        return made[-1]
    yield factory
    for c in made:
        c.close()


def test_the_default_is_the_measured_sixteen_hits_and_a_clear_keeps_the_setting(lib):
    c = Cache(lib, 5)
    try:
        assert lib.beam_refine_default_after() == 16      # the searches' duration over a frame's gain, the worse of poses A and B
        fresh = lib.beam_refine_new()
        assert lib.beam_refine_after(fresh) == 16
        lib.beam_refine_delete(fresh)
        c.reset()
        assert lib.beam_refine_after(c.s) == 5
    finally:
        c.close()


@pytest.mark.parametrize("after", [1, 2, 3, 8])
def test_refine_is_planned_exactly_once_per_fill_on_the_kth_hit(make, after):
    c = make(after)
    assert c.ask(0) == (SEARCH, -1)
    action, slot = c.ask(0)
    assert action == FILL and c.state(slot) == NONE          # a fill never refines, whatever K
    for _ in range(after - 1):
        assert c.ask(0) == (HIT, slot) and c.state(slot) == NONE
    assert c.ask(0) == (HIT | REFINE, slot)                   # the K-th hit: it still walks from the coarse bounds
    assert c.state(slot) == DONE
    for _ in range(3 * after + 5):
        assert c.ask(0) == (HIT | FINE, slot)                 # never a second time


def test_between_the_plan_and_the_commit_the_state_is_refine_now(make):
    c = make(1)
    c.ask(0); slot = c.ask(0)[1]
    assert c.ask(0, issued=-1) == (HIT | REFINE, slot)       # (-1: the shim leaves the commit out)
    assert c.state(slot) == NOW
    assert c.ask(0, issued=-1) == (HIT, slot)                 # asked again before the commit: neither a second refinement nor the finer bounds
    assert c.state(slot) == NOW


def test_a_view_that_is_searched_but_not_admitted_never_refines(make):
    c = make(1)
    for v in range(100, 160):                                 # a camera in motion: no key twice
        assert c.ask(v) == (SEARCH, -1)
    for _ in range(10):                                       # two views taking turns from the start: never twice in a row
        assert c.ask(0) == (SEARCH, -1) and c.ask(1) == (SEARCH, -1)
    assert all(c.state(k) == NONE for k in range(4))


def test_a_geometry_that_cannot_be_refined_never_is(make):
    c = make(1)
    c.ask(0, eligible=False); slot = c.ask(0, eligible=False)[1]
    for _ in range(6):
        assert c.ask(0, eligible=False) == (HIT, slot)
    assert c.state(slot) == NONE


def test_a_refill_an_eviction_and_a_clear_start_the_state_over(make):
    c = make(2)
    slots = {}
    for v in range(4):                                        # four views at rest, all refined
        c.ask(v); slots[v] = c.ask(v)[1]
        assert c.ask(v) == (HIT, slots[v]) and c.ask(v) == (HIT | REFINE, slots[v]) and c.ask(v) == (HIT | FINE, slots[v])
    assert sorted(slots.values()) == [0, 1, 2, 3] and all(c.state(k) == DONE for k in range(4))
    # a fifth view evicts the one used longest ago (view 0): its slot starts over, and counts its own hits
    assert c.ask(4) == (SEARCH, -1)
    assert c.ask(4) == (FILL, slots[0]) and c.state(slots[0]) == NONE
    assert c.ask(4) == (HIT, slots[0])
    assert c.ask(4) == (HIT | REFINE, slots[0])
    assert c.ask(4) == (HIT | FINE, slots[0])
    for v in (2, 3):
        assert c.ask(v) == (HIT | FINE, slots[v])            # the others keep theirs
    # view 0 comes back: admitted afresh into view 1's slot (used longest ago), a refill of a refined slot
    assert c.ask(0) == (SEARCH, -1)
    assert c.ask(0) == (FILL, slots[1]) and c.state(slots[1]) == NONE
    assert c.ask(0) == (HIT, slots[1]) and c.ask(0) == (HIT | REFINE, slots[1])
    c.reset()
    assert all(c.state(k) == NONE for k in range(4))
    assert c.ask(0) == (SEARCH, -1) and c.ask(0)[0] == FILL
    assert c.ask(0)[0] == HIT and c.ask(0)[0] == HIT | REFINE      # two hits again, not one: the count started over as well


def test_k_larger_than_the_hits_a_view_ever_gets(make):
    c = make(1000)
    c.ask(0); slot = c.ask(0)[1]
    for _ in range(999):
        assert c.ask(0) == (HIT, slot)
    assert c.state(slot) == NONE
    c.ask(1); c.ask(1)                                        # the camera moves on; the view was never refined and paid nothing
    assert c.ask(0) == (HIT | REFINE, slot)                   # ... and had it stayed: its thousandth hit


def test_a_launch_that_could_not_issue_its_searches_leaves_the_slot_coarse_and_counts_again(make):
    c = make(2)
    c.ask(0); slot = c.ask(0)[1]
    assert c.ask(0) == (HIT, slot)
    assert c.ask(0, issued=0) == (HIT | REFINE, slot) and c.state(slot) == NONE
    assert c.ask(0) == (HIT, slot)
    assert c.ask(0) == (HIT | REFINE, slot) and c.state(slot) == DONE


def test_the_refine_walk_runs_clean_under_the_sanitizers(tmp_path):
    """The shim as a stand-alone program (its own main), built with the address and undefined-behaviour sanitizers."""
    exe = tmp_path / "beam_refine_policy_asan"
    subprocess.run(["g++", "-O1", "-g", "-std=c++20", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-DBEAM_REFINE_SHIM_MAIN",
                    f"-I{HDR.parent}", "-o", os.fspath(exe), os.fspath(SRC)], check=True)
    r = subprocess.run([os.fspath(exe)], capture_output=True, text=True)
    assert r.returncode == 0 and "0 mismatches" in r.stdout, r.stdout + r.stderr
