"""CPU: the host build of the neighbour-count rules (blok_automaton_voxels, blok_amd/automaton.py) against the numpy model of the contract
(tests/automaton_reference.py) over the whole case table of the GPU tests (tests/automaton_cases.py): arrays bit for bit, info and per-step
counts; cross-checks against the distance and components references; the properties of the rule; the conditions that keep the table from
being vacuous, asserted from the model alone; and the whole-brick arithmetic of csrc/common/automaton_core.h, run beside the host build's
cell loop by a program of its own under ASan and UBSan."""
from __future__ import annotations

import os
import subprocess
from pathlib import Path

import numpy as np
import pytest

from blok_amd import _ffi
from blok_amd import automaton as A
from blok_amd._ffi import BlokError
from tests import automaton_cases as K
from tests import automaton_reference as R
from tests import components_reference as CR
from tests import distance_reference as DR

ROOT = Path(__file__).resolve().parent.parent
BLOK_ERR_INVALID_ARG, BLOK_ERR_UNSUPPORTED = -1, -5


def host_of(c):
    d, m = K.content(c["shape"])
    return A.automaton_host(d, m, c["rule"], c["origin"], c["lo"], c["hi"])


def same(got, want, tag):
    """(d, m, info, step_counts) equal bit for bit."""
    for name, g, w in zip(("density", "ids", "info", "step counts"), got[:4], want[:4]):
        assert g.dtype == w.dtype and g.shape == w.shape, (tag, name, g.dtype, g.shape, w.dtype, w.shape)
        assert g.tobytes() == w.tobytes(), f"{tag}: {name}: {g if name == 'info' else int((g.view(np.uint32) != w.view(np.uint32)).sum())} differ(s) from {w if name == 'info' else 'the model'}"


def test_abi_is_at_least_1_19_and_the_records_have_their_sizes():
    assert _ffi.hip_lib().blok_hip_abi_version() >= (1 << 16) | 19
    assert _ffi.AUTOMATON_RULE.itemsize == 32 and _ffi.AUTOMATON_INFO.itemsize == 64 and R.INFO == _ffi.AUTOMATON_INFO
    assert _ffi.AUTOMATON_INFO.fields["n_born"][1] == 40


# ---- host build against the model ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("box", list(K.BOXES))
def test_host_build_matches_the_model(box):
    cases = K.cases_of(box)
    assert len(cases) >= 8
    for c in cases:
        same(host_of(c), K.expected(c), c["name"])


def test_presets_are_the_rules_the_header_names():
    s = A.smooth(4)[0]
    assert (int(s["neighbourhood"]), int(s["survive"]), int(s["birth"]), int(s["steps"])) == (26, sum(1 << n for n in range(13, 27)), sum(1 << n for n in range(14, 27)), 4)
    assert (int(A.despeckle()[0]["neighbourhood"]), int(A.despeckle()[0]["survive"]), int(A.despeckle()[0]["birth"])) == (6, 0b1111110, 0)
    assert (int(A.fill_pits(2)[0]["survive"]), int(A.fill_pits(2)[0]["birth"])) == (0b1111111, 0b1100000)
    assert int(A.life((4, 5), (5,))[0]["survive"]) == 0b110000 and int(A.life((4, 5), (5,))[0]["birth"]) == 0b100000
    assert A.at_least(3, 6) == 0b1111000 and A.check(A.smooth()) == "" and "steps" in A.check(A.smooth(0))


# ---- against the references the repository already has ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("nb,d2", [(6, 1), (18, 2), (26, 3)])
def test_dilate_and_erode_are_grow_and_shrink_of_the_distance_field(nb, d2):
    origin, shape = K.BOXES["high"]
    d0, m0 = K.content(shape)
    d, m = d0.copy(), m0.copy()
    dist, info = DR.field(d0, origin, None, None, 2, 0)
    n = DR.edit(d, m, dist, info, DR.GROW, d2, 2.5, 41, origin)
    hd, hm, hinfo, _ = A.automaton_host(d0, m0, A.dilate(nb, density=2.5, material=41, fixed_material=True), origin)
    assert n == int(hinfo["n_born"][0]) > 1000 and hd.tobytes() == d.tobytes() and hm.tobytes() == m.tobytes()
    d, m = d0.copy(), m0.copy()
    dist, info = DR.field(d0, origin, None, None, 2, DR.TO_EMPTY)
    n = DR.edit(d, m, dist, info, DR.SHRINK, d2, origin=origin)
    hd, hm, hinfo, _ = A.automaton_host(d0, m0, A.erode(nb), origin)
    assert n == int(hinfo["n_died"][0]) > 1000 and hd.tobytes() == d.tobytes() and hm.tobytes() == m.tobytes()


def test_despeckle_kills_exactly_the_components_of_one_voxel():
    origin, shape = K.BOXES["house"]
    d0, m0 = K.content(shape)
    labels, records = CR.label(d0, origin)
    alone = np.zeros(d0.size, bool)
    alone[records["label"][records["n_voxels"] == 1].astype(np.int64)] = True      # (a component's label is the index of one of its cells: of its only one)
    hd, _, hinfo, _ = A.automaton_host(d0, m0, A.despeckle(), origin)
    died = (R.filled_of(d0) & ~R.filled_of(hd)).reshape(-1)
    assert int(alone.sum()) == int(hinfo["n_died"][0]) > 100 and (died == alone).all()


# ---- properties --------------------------------------------------------------------------------------------------------------------------------
def case(name):
    return next(c for c in K.table() if c["name"] == name)


def test_the_call_stops_after_the_first_step_that_changes_nothing():
    _, _, info, counts = host_of(case("house/whole/despeckle x5"))
    assert int(info["steps_run"][0]) == 2 and int(counts[0][1]) > 0 and not counts[1:].any()      # after the first step no survivor is alone
    _, _, info, counts = host_of(case("house/whole/nothing happens"))
    assert int(info["steps_run"][0]) == 1 and not counts.any() and int(info["n_filled"][0]) == int(R.filled_of(K.content(K.HOUSE_SHAPE)[0]).sum())


def small(cells, shape=(5, 5, 5)):
    """[z][y][x] arrays of a small box from {(x, y, z): (density, id)}."""
    d, m = np.zeros(shape[::-1], np.float32), np.zeros(shape[::-1], np.uint32)
    for (x, y, z), (value, ident) in cells.items():
        d[z, y, x], m[z, y, x] = value, ident
    return d, m


def both(d, m, r, **kw):
    """The host build's result, after it has been found equal to the model's."""
    got = A.automaton_host(d, m, r, **kw)
    want = R.run(d, m, kw.get("origin", (0, 0, 0)), kw.get("lo"), kw.get("hi"), r)
    same(got, want, "small")
    return got


def test_a_tie_goes_to_the_smallest_id():
    c = case("house/whole/dilate 6")
    x, y, z = K.tie_cell(c["shape"])
    d0, m0 = K.content(c["shape"])
    assert not d0[z, y, x] > 0 and sorted(int(m0[q]) for q in ((z, y, x - 1), (z, y + 1, x))) == [5, 8]
    hd, hm, _, _ = host_of(c)
    assert float(hd[z, y, x]) == 2.5 and int(hm[z, y, x]) == 5
    d, m = small({(1, 2, 2): (1.0, 9), (3, 2, 2): (1.0, 4), (2, 1, 2): (1.0, 9), (2, 3, 2): (1.0, 4)})
    assert int(both(d, m, A.dilate(6))[1][2, 2, 2]) == 4


def test_the_stale_ids_of_empty_cells_do_not_vote():
    cells = {(1, 2, 2): (1.0, 7)}
    cells.update({q: (value, 3) for q, value in (((3, 2, 2), 0.0), ((2, 1, 2), -2.0), ((2, 3, 2), float("nan")), ((2, 2, 1), -0.0), ((2, 2, 3), 0.0))})
    d, m = small(cells)
    hd, hm, _, _ = both(d, m, A.dilate(6))
    assert int(hm[2, 2, 2]) == 7 and float(hd[2, 2, 2]) == 1.0
    assert hd.view(np.uint32)[2, 1, 2] == d.view(np.uint32)[2, 1, 2] and int(hm[2, 1, 2]) == 3 and int(hm[1, 2, 2]) == 3      # an empty cell without a filled neighbour is not born and keeps its bits


def test_a_dying_voter_still_votes():
    d, m = small({(2, 2, 2): (1.0, 9)})
    hd, hm, info, _ = both(d, m, A.rule(6, 0, 1 << 1, material=55))      # everything filled dies; born beside exactly one filled cell
    assert not hd[2, 2, 2] > 0 and int(hm[2, 2, 2]) == 0
    assert [int(hm[q]) for q in ((2, 2, 1), (2, 2, 3), (2, 1, 2), (2, 3, 2), (1, 2, 2), (3, 2, 2))] == [9] * 6
    assert (int(info["n_born"][0]), int(info["n_died"][0])) == (6, 1)


def test_cells_outside_the_region_stay_frozen_bit_for_bit():
    c = case("house/unaligned/smooth x2")
    d0, m0 = K.content(c["shape"])
    hd, hm, info, _ = A.automaton_host(d0, m0, A.smooth(3), c["origin"], c["lo"], c["hi"])
    l, h = R.local_region(d0.shape, c["origin"], c["lo"], c["hi"])
    outside = np.ones(d0.shape, bool)
    outside[l[2]:h[2], l[1]:h[1], l[0]:h[0]] = False
    assert int(info["steps_run"][0]) == 3
    assert (hd.view(np.uint32)[outside] == d0.view(np.uint32)[outside]).all() and (hm[outside] == m0[outside]).all()
    # after ONE step (over three a cell may be born and die again, which writes it): the empty cells of the region that stayed empty keep
    # their NaN, their -1.5 and their stale ids
    hd, hm, _, _ = A.automaton_host(d0, m0, A.smooth(1), c["origin"], c["lo"], c["hi"])
    kept = ~outside & ~R.filled_of(d0) & ~R.filled_of(hd)
    assert (hd.view(np.uint32)[kept] == d0.view(np.uint32)[kept]).all() and (hm[kept] == m0[kept]).all() and np.isnan(hd[kept]).any() and (hm[kept] != 0).any()


def test_a_translated_box_gives_the_same_result():
    c = case("house/unaligned/smooth x2")
    want = host_of(c)
    for shift in ((1, -3, 5), (-32731, 31, 7)):
        moved = lambda p: tuple(int(p[a]) + shift[a] for a in range(3))
        got = A.automaton_host(*K.content(c["shape"]), c["rule"], moved(c["origin"]), moved(c["lo"]), moved(c["hi"]))
        assert got[0].tobytes() == want[0].tobytes() and got[1].tobytes() == want[1].tobytes() and got[3].tobytes() == want[3].tobytes()
        assert [int(v) for v in got[2]["lo"][0]] == list(moved(c["lo"]))


def bad_rules():
    ok = dict(neighbourhood=26, survive=1 << 13, birth=1 << 14, steps=1, density=1.0)
    for change in (dict(neighbourhood=8), dict(neighbourhood=0), dict(survive=1 << 27), dict(neighbourhood=6, survive=1 << 7, birth=0), dict(birth=1 << 27),
                   dict(neighbourhood=18, survive=0, birth=1 << 19), dict(steps=0), dict(steps=256), dict(density=0.0), dict(density=-1.0), dict(density=float("nan")),
                   dict(density=float("inf"))):
        yield change, A.rule(**dict(ok, **change))
    for field, value in (("flags", 4), ("reserved", 1)):
        r = A.rule(**ok)
        r[field] = value
        yield {field: value}, r


def test_every_error_leaves_the_arrays_unchanged():
    origin, shape = K.BOXES["ragged"]
    d0, m0 = K.content(shape)

    def refused(status, r, **kw):
        d, m = d0.copy(), m0.copy()
        rc = _ffi.host_lib().blok_automaton_voxels(_ffi.ptr(d), _ffi.ptr(m), A._vec(origin), *shape, A._vec(kw.get("lo")), A._vec(kw.get("hi")),
                                                   None if r is None else _ffi.ptr(r), None, None)
        assert rc == status, (kw, r)
        assert d.tobytes() == d0.tobytes() and m.tobytes() == m0.tobytes()
        if r is not None:
            with pytest.raises(BlokError) as e:
                A.automaton_host(d0, m0, r, origin, **kw)
            assert e.value.status == status

    n = 0
    for change, r in bad_rules():
        refused(BLOK_ERR_INVALID_ARG, r)
        assert A.check(r) != "", change
        n += 1
    assert n == 14
    refused(BLOK_ERR_INVALID_ARG, None)
    ok = A.smooth()
    hi = tuple(origin[a] + shape[a] for a in range(3))
    refused(BLOK_ERR_INVALID_ARG, ok, lo=origin)
    refused(BLOK_ERR_INVALID_ARG, ok, hi=hi)
    refused(BLOK_ERR_INVALID_ARG, ok, lo=(origin[0] + 2, origin[1], origin[2]), hi=(origin[0] + 1, hi[1], hi[2]))
    refused(BLOK_ERR_UNSUPPORTED, ok, lo=(origin[0] - 1, origin[1], origin[2]), hi=hi)
    refused(BLOK_ERR_UNSUPPORTED, ok, lo=origin, hi=(hi[0], hi[1], hi[2] + 1))
    assert A.automaton_host(d0, m0, A.rule(26, 0, 0, density=float("nan")), origin)[2]["n_died"][0] > 0      # without births the density is not looked at


# ---- the table is not vacuous: from the model alone -------------------------------------------------------------------------------------------
NO_TIE_EXPECTED = {"births at 0", "births at 0, solid", "toggle x3"}      # born cells without a voter; a region of one cell


def test_the_table_exercises_what_it_is_there_for():
    names = [c["name"] for c in K.table()]
    assert len(set(names)) == len(names) >= 50
    for c in K.table():
        d, m, info, counts, ties = K.expected(c)
        changed = int(info["n_born"][0]) + int(info["n_died"][0])
        if c["region"] == "empty":
            assert changed == 0 and int(info["steps_run"][0]) == 0
        elif c["rule_name"] in K.FIXED_POINTS:
            assert changed == 0 and int(info["steps_run"][0]) == 1
        else:
            assert changed > 0, c["name"]
            if c["rule_name"].startswith(("smooth", "life")):
                assert counts[0][0] > 0 and counts[0][1] > 0, c["name"]
            if K.VOTING(c["rule"]) and c["rule_name"] not in NO_TIE_EXPECTED:
                assert sum(ties) > 0, c["name"]
    born_without_voter = K.expected(case("house/whole/births at 0"))
    assert int((born_without_voter[1] == 77).sum()) == int(born_without_voter[2]["n_born"][0]) > 1000
    assert int(K.expected(case("house/whole/despeckle x5"))[2]["steps_run"][0]) == 2
    # the slab box holds bricks whose 27 words are all ones, and bricks whose 27 are all 0: every cell of such a brick has the count 0, or the neighbourhood's size
    f = R.filled_of(K.content(K.SLAB_SHAPE)[0])
    nz, ny, nx = (n // 4 for n in f.shape)
    bricks = f.reshape(nz, 4, ny, 4, nx, 4)
    for uniform in (bricks.all(axis=(1, 3, 5)), ~bricks.any(axis=(1, 3, 5))):
        assert np.lib.stride_tricks.sliding_window_view(uniform, (3, 3, 3)).all(axis=(3, 4, 5)).any()
    d0, m0 = K.content(K.HOUSE_SHAPE)
    empty = ~R.filled_of(d0)
    assert np.isnan(d0[empty]).any() and (d0[empty] < 0).any() and 0.15 < float((m0[empty] != 0).mean()) < 0.25


# ---- the whole-brick arithmetic, and the sanitizers --------------------------------------------------------------------------------------------
def _checksum(raw: bytes) -> int:
    w = np.frombuffer(raw, dtype=np.uint32).astype(np.uint64)
    return int((w * np.arange(1, w.size + 1, dtype=np.uint64)).sum(dtype=np.uint64))


def test_brick_arithmetic_equals_the_cell_loop_under_address_and_ub_sanitizers(tmp_path):
    """A program of its own (tests/host_harness/automaton_main.cpp) over case files: the whole table and three refusals.  Per case it runs
    the host build's cell loop and the whole-brick arithmetic of automaton_core.h — what the decide kernel runs — over every brick of the
    region, and reports whether they agree bit for bit; the cell loop's result is compared with the model here.  Nothing loaded into Python
    is sanitized."""
    exe = tmp_path / "automaton_main"
    subprocess.run(["g++", "-O1", "-g", "-std=c++20", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    "-fno-omit-frame-pointer", f"-I{ROOT / 'include'}", "-o", os.fspath(exe), os.fspath(ROOT / "tests/host_harness/automaton_main.cpp"),
                    os.fspath(ROOT / "blok_amd/csrc/host/automaton.cpp")], check=True)
    jobs = [(c, 0) for c in K.table()]
    first = K.table()[0]
    o = first["origin"]
    jobs += [(dict(first, rule=A.rule(7, 0, 0)), BLOK_ERR_INVALID_ARG), (dict(first, rule=A.smooth(256)), BLOK_ERR_INVALID_ARG),
             (dict(first, lo=(o[0] - 1, o[1], o[2]), hi=(o[0] + 4, o[1] + 4, o[2] + 4)), BLOK_ERR_UNSUPPORTED)]
    files, want = [], []
    for i, (c, status) in enumerate(jobs):
        path = tmp_path / f"case{i}.bin"
        region = [1] + list(c["lo"]) + list(c["hi"]) if c["lo"] is not None else [0] * 7
        header = np.array(list(c["shape"]) + list(c["origin"]) + region, dtype=np.int32)
        d0, m0 = K.content(c["shape"])
        path.write_bytes(header.tobytes() + c["rule"].tobytes() + d0.tobytes() + m0.tobytes())
        files.append(os.fspath(path))
        if status:
            want.append(f"{status} 0 0 0 0 {_checksum(d0.tobytes())} {_checksum(m0.tobytes())} 0 -1")
        else:
            d, m, info, counts, _ = K.expected(c)
            i0 = info[0]
            want.append(f"0 {int(i0['steps_run'])} {int(i0['n_born'])} {int(i0['n_died'])} {int(i0['n_filled'])} {_checksum(d.tobytes())} {_checksum(m.tobytes())} "
                        f"{_checksum(counts.tobytes())} {-1 if c['region'] == 'empty' else 1}")
    run = subprocess.run([os.fspath(exe)] + files, capture_output=True, text=True)
    assert run.returncode == 0 and run.stderr == "", run.stdout + run.stderr
    got = run.stdout.splitlines()
    assert len(got) == len(want)
    for (c, _), g, w in zip(jobs, got, want):
        assert g == w, (c["name"], g, w)
