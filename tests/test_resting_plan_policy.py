"""What one launch over a kept view does, as ONE value (blok_amd/csrc/hip/beam_cache.h: plan_resting_launch, RestingWalk, commit_resting_launch),
on the host through a shim: the value over the modes, the list's states, the start key, the two eligibilities and a failed issue; the node
words are declined exactly when a launch told to count them cannot keep them, and a declined slot walks from its starts for good.  The
value is also checked against the four plans it was made from, as the launch code read them before there was a value.  No GPU."""
import ctypes as C
import itertools
import os
import subprocess
from pathlib import Path

import pytest

ROOT = Path(__file__).resolve().parent.parent
SRC = ROOT / "tests" / "host_harness" / "resting_plan_shim.cpp"
HDR = ROOT / "blok_amd" / "csrc" / "hip" / "beam_cache.h"
LIB = ROOT / "tests" / "host_harness" / "libresting_plan_shim.so"

NOT_HIT, COARSE, FINE, COUNT, COUNT_STARTS, COUNT_NODES, PACKED_FINE, PACKED_STARTS, PACKED_NODES = range(9)
SEARCH, FILL, HIT = range(3)
NONE, NOW, BUILDING, READY = range(4)
REFINE_OK, LIST_OK, BUILT, WORDS = 1, 2, 4, 8             # the facts
COUNTED = (0, 0, 0x3A83126F, 0x461C4000)                 # jitter x, jitter y, tmin, tmax as bits
JITTERED = (0x3E800000, 0xBE800000, 0x3A83126F, 0x461C4000)
MODES = [(0, 0), (0, 1), (1, 0), (1, 1)]                 # own_starts, node_restart


@pytest.fixture(scope="module")
def lib():
    if not LIB.exists() or LIB.stat().st_mtime < max(SRC.stat().st_mtime, HDR.stat().st_mtime):
        subprocess.run(["g++", "-O1", "-std=c++20", "-fPIC", "-Wall", "-Wextra", "-Werror", f"-I{HDR.parent}", "-shared", "-o", os.fspath(LIB), os.fspath(SRC)], check=True)
    L = C.CDLL(os.fspath(LIB))
    L.resting_plan_new.restype = C.c_void_p
    L.resting_plan_new.argtypes = [C.c_int, C.c_int, C.c_uint]
    for name in ("resting_plan_delete", "resting_plan_reset", "resting_plan_settle"):
        getattr(L, name).argtypes = [C.c_void_p]
    for name in ("resting_plan_set_node_restart", "resting_plan_refine_state", "resting_plan_list_state", "resting_plan_has_starts", "resting_plan_has_nodes"):
        getattr(L, name).argtypes = [C.c_void_p, C.c_int]
    L.resting_plan_launch.argtypes = [C.c_void_p, C.POINTER(C.c_uint32), C.POINTER(C.c_uint32), C.c_int, C.c_int, C.c_int, C.POINTER(C.c_int)]
    return L


def ladder(bits, node_restart):
    """The value as the launch code used to derive it from the four plans and the policy's node state."""
    has_nodes = bits >> 16 & 1
    action, use_fine, count_now, use_list = (bits >> 4) & 3, (bits >> 7) & 1, (bits >> 8) & 1, (bits >> 9) & 1
    count_own, use = (bits >> 10) & 1, (bits >> 11) & 3
    if action != HIT:
        return NOT_HIT
    if use_list:
        return PACKED_FINE if use != 1 else PACKED_NODES if node_restart and has_nodes else PACKED_STARTS
    if count_now:
        return COUNT if not count_own else COUNT_NODES if has_nodes else COUNT_STARTS
    return FINE if use_fine else COARSE


class Cache:
    """K = 1: a view's launches are a search, a fill, the hit that refines, N - 1 hits from the finer bounds, the hit that counts."""

    def __init__(self, L, own, nodes, after=1):
        self.L, self.s, self.n, self.node_restart = L, L.resting_plan_new(own, nodes, after), L.resting_plan_key_words(), bool(nodes)

    def close(self):
        self.L.resting_plan_delete(self.s)

    def ask(self, v, facts=REFINE_OK | LIST_OK | WORDS, key=COUNTED, refine_issued=1, list_issued=1):
        """One launch of view v -> (the value, the slot); the value is the ladder's over the plans of the same launch."""
        slot = C.c_int(-7)
        words = (C.c_uint32 * self.n)(*[0x3F800000 + 977 * v + i for i in range(self.n)])
        bits = self.L.resting_plan_launch(self.s, words, (C.c_uint32 * 4)(*key), facts, refine_issued, list_issued, C.byref(slot))
        assert bits & 15 == ladder(bits, self.node_restart), hex(bits)
        self.bits = bits
        return bits & 15, slot.value

    def refined(self, v, facts=REFINE_OK | LIST_OK | WORDS):
        assert self.ask(v, facts)[0] == NOT_HIT and self.bits >> 4 & 3 == SEARCH
        assert self.ask(v, facts)[0] == NOT_HIT and self.bits >> 4 & 3 == FILL
        walk, slot = self.ask(v, facts)
        assert walk == COARSE and self.bits >> 6 & 1 and self.L.resting_plan_refine_state(self.s, slot) == 2
        return slot

    def listed(self, v, facts=REFINE_OK | LIST_OK | WORDS, key=COUNTED):
        """View v from nothing to its adopted list (N = 1), counted under `key` with `facts` -> (its slot, the count's value, the adopting hit's)."""
        slot = self.refined(v, facts)
        count = self.ask(v, facts, key)
        assert count[1] == slot and self.list(slot) == BUILDING
        packed = self.ask(v, facts | BUILT, key)
        assert packed[1] == slot and self.list(slot) == READY and self.bits >> 13 & 7 == slot + 1
        return slot, count[0], packed[0]

    def list(self, slot):
        return self.L.resting_plan_list_state(self.s, slot)

    def starts(self, slot):
        return bool(self.L.resting_plan_has_starts(self.s, slot))

    def nodes(self, slot):
        return bool(self.L.resting_plan_has_nodes(self.s, slot))


@pytest.fixture()
def make(lib):
    made = []

    def factory(own=1, nodes=1, after=1):
        made.append(Cache(lib, own, nodes, after))
        return made[-1]
    yield factory
    for c in made:
        c.close()


def expected(own, nodes, can):
    words = own and nodes and can
    return (COUNT, PACKED_FINE) if not own else (COUNT_NODES, PACKED_NODES) if words else (COUNT_STARTS, PACKED_STARTS)


@pytest.mark.parametrize("own,nodes,can", [m + (c,) for m in MODES for c in (0, 1)])
def test_the_value_over_the_modes_and_whether_node_words_can_be_kept(make, own, nodes, can):
    c = make(own, nodes)
    facts = REFINE_OK | LIST_OK | (WORDS if can else 0)
    slot, count, packed = c.listed(0, facts)
    assert (count, packed) == expected(own, nodes, can)
    assert c.starts(slot) == bool(own) and c.nodes(slot) == bool(own and nodes and can)
    for _ in range(3):
        assert c.ask(0, facts) == (packed, slot)


@pytest.mark.parametrize("own,nodes", MODES)
def test_the_value_in_every_state_of_the_list(make, own, nodes):
    c = make(own, nodes, after=2)
    count, packed = expected(own, nodes, 1)
    slot = c.refined(0)
    assert c.list(slot) == NONE and c.ask(0) == (FINE, slot)                  # None, before the N-th hit from the finer bounds
    assert c.ask(0, refine_issued=-1, list_issued=-1) == (count, slot) and c.list(slot) == NOW
    assert c.ask(0, refine_issued=-1, list_issued=-1) == (FINE, slot) and c.list(slot) == NOW      # (a launch between the plan and the commit: another stream)
    c.L.resting_plan_reset(c.s)
    slot = c.refined(0)
    assert c.ask(0) == (FINE, slot) and c.ask(0) == (count, slot) and c.list(slot) == BUILDING
    assert c.ask(0) == (FINE, slot) and c.list(slot) == BUILDING               # the event not yet seen complete
    assert c.ask(0, REFINE_OK | LIST_OK | WORDS | BUILT) == (packed, slot) and c.list(slot) == READY
    assert c.ask(0) == (packed, slot)


@pytest.mark.parametrize("own,nodes,can", [m + (c,) for m in MODES for c in (0, 1)])
def test_another_start_key_walks_packed_from_the_finer_bounds_and_the_counted_key_returns(make, own, nodes, can):
    c = make(own, nodes)
    facts = REFINE_OK | LIST_OK | (WORDS if can else 0)
    slot, _, packed = c.listed(0, facts)
    for other in (JITTERED, (0, 0, 0x3F800000, COUNTED[3]), (0, 0, COUNTED[2], 0x42C80000), (0x80000000, 0, COUNTED[2], COUNTED[3])):
        assert c.ask(0, facts, other) == (PACKED_FINE, slot)
        assert c.bits >> 11 & 3 == (2 if own else 0)
    assert c.ask(0, facts) == (packed, slot)                                  # own starts or node words again
    assert c.starts(slot) == bool(own) and c.nodes(slot) == bool(own and nodes and can) and c.list(slot) == READY


@pytest.mark.parametrize("own,nodes", MODES)
def test_a_launch_that_is_not_eligible_walks_from_what_it_may(make, own, nodes):
    c = make(own, nodes)
    assert c.ask(0, LIST_OK)[0] == NOT_HIT and c.ask(0, LIST_OK)[0] == NOT_HIT
    for _ in range(3):
        walk, slot = c.ask(0, LIST_OK | WORDS)
        assert walk == COARSE and not c.bits >> 6 & 1 and c.L.resting_plan_refine_state(c.s, slot) == 0      # no finer bounds: never refined, never counted
    assert c.ask(0, REFINE_OK | WORDS) == (COARSE, slot) and c.bits >> 6 & 1                                 # the hit that refines
    for _ in range(3):
        assert c.ask(0, REFINE_OK | WORDS) == (FINE, slot) and c.list(slot) == NONE                          # no packed walk: never counted
    count, packed = expected(own, nodes, 1)
    assert c.ask(0) == (count, slot)
    assert c.ask(0, REFINE_OK | LIST_OK | WORDS | BUILT) == (packed, slot)
    assert c.ask(0, REFINE_OK | WORDS) == (FINE, slot)                        # a list, and a launch it does not apply to
    assert c.ask(0, LIST_OK | WORDS) == (COARSE, slot)
    assert c.ask(0) == (packed, slot) and c.list(slot) == READY


@pytest.mark.parametrize("own,nodes", MODES)
def test_an_issue_that_fails_at_the_refine_or_at_the_build_is_asked_again(make, own, nodes):
    c = make(own, nodes)
    count, packed = expected(own, nodes, 1)
    assert c.ask(0)[0] == NOT_HIT and c.ask(0)[0] == NOT_HIT
    walk, slot = c.ask(0, refine_issued=0, list_issued=0)
    assert walk == COARSE and c.bits >> 6 & 1 and c.L.resting_plan_refine_state(c.s, slot) == 0
    assert c.ask(0) == (COARSE, slot) and c.bits >> 6 & 1 and c.L.resting_plan_refine_state(c.s, slot) == 2
    assert c.ask(0, refine_issued=1, list_issued=0) == (count, slot)
    assert c.list(slot) == NONE and not c.starts(slot) and not c.nodes(slot)
    assert c.ask(0) == (count, slot) and c.list(slot) == BUILDING and c.starts(slot) == bool(own) and c.nodes(slot) == bool(own and nodes)
    assert c.ask(0, REFINE_OK | LIST_OK | WORDS | BUILT) == (packed, slot)


@pytest.mark.parametrize("own,nodes,can", [m + (c,) for m in MODES for c in (0, 1)])
def test_the_node_words_are_declined_by_the_launch_told_to_count_them_that_cannot_keep_them_and_by_no_other(make, own, nodes, can):
    c = make(own, nodes)
    facts = REFINE_OK | LIST_OK | (WORDS if can else 0)
    slot = c.refined(0, REFINE_OK | LIST_OK)                                  # launches that count nothing decline nothing
    assert not c.nodes(slot)
    walk, _ = c.ask(0, facts)
    told = bool(own and nodes)                                                # plan_beam_starts set nodes[slot]: the launch was told to count them
    assert c.bits >> 10 & 1 == own and c.nodes(slot) == (told and bool(can)) and c.starts(slot) == bool(own)
    assert walk == expected(own, nodes, can)[0]
    for f in (REFINE_OK | LIST_OK, REFINE_OK | LIST_OK | BUILT, REFINE_OK | LIST_OK, REFINE_OK, 0):      # none of these counts: whatever the fact says, the words stay
        c.ask(0, f)
        assert c.nodes(slot) == (told and bool(can))


def test_a_declined_slot_walks_from_its_starts_for_good_and_the_next_list_is_asked_again(make):
    c = make()
    slot, count, packed = c.listed(0, REFINE_OK | LIST_OK)
    assert (count, packed) == (COUNT_STARTS, PACKED_STARTS) and c.starts(slot) and not c.nodes(slot)
    for _ in range(3):
        assert c.ask(0) == (PACKED_STARTS, slot)                              # node words that could be kept NOW revive nothing
    assert c.ask(0, key=JITTERED) == (PACKED_FINE, slot) and c.ask(0) == (PACKED_STARTS, slot)
    other, count, packed = c.listed(1)                                         # another view, its own list: counted with node words
    assert other != slot and (count, packed) == (COUNT_NODES, PACKED_NODES) and c.nodes(other) and not c.nodes(slot)
    c.L.resting_plan_reset(c.s)                                                # the slot's next list (a clear; a refill does the same)
    again, count, packed = c.listed(0)
    assert (count, packed) == (COUNT_NODES, PACKED_NODES) and c.nodes(again)


def test_mode_5_switched_off_over_a_list_with_node_words_walks_from_the_starts(make):
    c = make()
    slot, _, packed = c.listed(0)
    assert packed == PACKED_NODES
    c.L.resting_plan_set_node_restart(c.s, 0); c.node_restart = False
    assert c.ask(0) == (PACKED_STARTS, slot) and c.nodes(slot)
    c.L.resting_plan_set_node_restart(c.s, 1); c.node_restart = True
    assert c.ask(0) == (PACKED_NODES, slot)


def test_the_full_table_against_the_plans_it_is_made_from(make):
    """Every mode x every combination of the facts x both start keys, launch after launch over two views: Cache.ask checks each value."""
    seen = set()
    for own, nodes in MODES:
        for issued in (1, 0):
            c = make(own, nodes)
            for facts, key in itertools.product(range(16), (COUNTED, JITTERED)):
                for v in (0, 0, 1, 1, 0, 0, 0):
                    seen.add(c.ask(v, facts, key, refine_issued=issued, list_issued=issued)[0])
            for facts, key in itertools.product(reversed(range(16)), (COUNTED, JITTERED)):
                for v in (0, 0, 0, 1, 1, 1):
                    seen.add(c.ask(v, facts, key)[0])
    assert seen == set(range(9))


def test_the_policy_walk_runs_clean_under_the_sanitizers(tmp_path):
    """The shim as a stand-alone program (its own main), built with the address and undefined-behaviour sanitizers."""
    exe = tmp_path / "resting_plan_policy_asan"
    subprocess.run(["g++", "-O1", "-g", "-std=c++20", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-DRESTING_PLAN_SHIM_MAIN",
                    f"-I{HDR.parent}", "-o", os.fspath(exe), os.fspath(SRC)], check=True)
    r = subprocess.run([os.fspath(exe)], capture_output=True, text=True)
    assert r.returncode == 0 and "0 mismatches" in r.stdout, r.stdout + r.stderr
