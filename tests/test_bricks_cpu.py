"""CPU: the sparse brick stream (include/blok_hip.h: blok_hip_volume_encode_bricks).  The numpy reference (tests/bricks_reference.py) pinned
to hand-written streams; the host build (blok_bricks_encode / _decode, which shares bricks_core.h with the kernels) pinned to the
reference byte for byte over the content of the GPU tests; the validation table; the .bvol file; and what makes the shared scene worth
running, asserted from the reference alone.  No GPU."""
from __future__ import annotations

import os
import subprocess
from pathlib import Path

import numpy as np
import pytest

from blok_amd import _ffi
from blok_amd import bricks as B
from blok_amd._ffi import BlokError
from tests import bricks_reference as R

ROOT = Path(__file__).resolve().parent.parent
BLOK_ERR_INVALID_ARG, BLOK_ERR_UNSUPPORTED = -1, -5
ONE, ONE_HALF, QUARTER, MINUS_ZERO, MINUS_HALF, NAN = 0x3F800000, 0x3FC00000, 0x3E800000, 0x80000000, 0xBF000000, 0x7FC00000


def f32(pattern):
    return np.array([pattern], dtype=np.uint32).view(np.float32)[0]


def both(d, m, origin=(0, 0, 0), lo=None, hi=None, flags=0):
    """The reference's stream, after the host build has been found equal to it."""
    ref = R.encode(d, m, origin, lo, hi, flags)
    got = B.encode_host(d, m, origin, lo, hi, flags)
    assert R.same_stream(ref, got)
    return ref


def fields(stream):
    info, records, dp, mp = stream
    return ([(int(r["mask"]), int(r["brick"]), int(r["kind"]), int(r["density"]), int(r["material"])) for r in records], dp.tolist(), mp.tolist(),
            tuple(int(info[k][0]) for k in ("n_bricks", "n_density", "n_material", "n_voxels")))


# ---- hand-written streams, the numbers spelled out -------------------------------------------------------------------------------------
def test_one_voxel_at_the_last_cell_of_a_5_9_2_region():
    # box 8 x 12 x 4 at (10, 20, 30); region [11, 16) x [22, 31) x [31, 33): ext (5, 9, 2), nb (2, 3, 1)
    d, m = np.zeros((4, 12, 8), np.float32), np.zeros((4, 12, 8), np.uint32)
    d[2, 10, 5], m[2, 10, 5] = 1.0, 7                        # world (15, 30, 32) = region cell (4, 8, 1): brick (1, 2, 0), cell (0, 0, 1)
    s = both(d, m, (10, 20, 30), (11, 22, 31), (16, 31, 33))
    assert fields(s) == ([(1 << 16, 1 + 2 * (2 + 3 * 0), 3, ONE, 7)], [], [], (1, 0, 0, 1))
    assert s[0]["lo"][0].tolist() == [11, 22, 31] and s[0]["ext"][0].tolist() == [5, 9, 2] and int(s[0]["version"][0]) == 1


def test_a_full_uniform_brick_has_no_payload():
    d, m = np.full((4, 4, 4), 1.5, np.float32), np.full((4, 4, 4), 3, np.uint32)
    assert fields(both(d, m)) == ([((1 << 64) - 1, 0, 3, ONE_HALF, 3)], [], [], (1, 0, 0, 64))


def test_kinds_1_2_and_0_with_payload_in_bit_order():
    d, m = np.zeros((4, 4, 8), np.float32), np.zeros((4, 4, 8), np.uint32)
    # brick 0: cells (1, 0, 0) bit 1, (0, 2, 0) bit 8, (3, 3, 3) bit 63
    for (x, y, z), dv, mv in (((1, 0, 0), 1.0, 5), ((0, 2, 0), 1.0, 6), ((3, 3, 3), 1.0, 5)):
        d[z, y, x], m[z, y, x] = dv, mv
    mask = (1 << 1) | (1 << 8) | (1 << 63)
    assert fields(both(d, m)) == ([(mask, 0, 1, ONE, 0)], [], [5, 6, 5], (1, 0, 3, 3))                       # one density, two ids
    m[m > 0] = 4
    d[0, 2, 0] = 0.25
    assert fields(both(d, m)) == ([(mask, 0, 2, 0, 4)], [ONE, QUARTER, ONE], [], (1, 3, 0, 3))              # two densities, one id
    m[3, 3, 3] = 9
    assert fields(both(d, m)) == ([(mask, 0, 0, 0, 0)], [ONE, QUARTER, ONE], [4, 4, 9], (1, 3, 3, 3))       # both mixed
    # a second brick of kind 0 starts at the running sums; a uniform brick in between adds nothing to them
    d[0, 0, 4], m[0, 0, 4] = 1.5, 2
    d[1, 1, 5], m[1, 1, 5] = 1.5, 2
    d2, m2 = np.concatenate([d, d[:, :, :4]], axis=2), np.concatenate([m, m[:, :, :4]], axis=2)
    assert fields(both(d2, m2)) == ([(mask, 0, 0, 0, 0), (1 | 1 << 21, 1, 3, ONE_HALF, 2), (mask, 2, 0, 3, 3)],
                                    [ONE, QUARTER, ONE] * 2, [4, 4, 9] * 2, (3, 6, 6, 8))


def test_odd_densities_and_bare_ids_are_stored_by_default_and_dropped_by_filled_only():
    d, m = np.zeros((4, 4, 4), np.float32), np.zeros((4, 4, 4), np.uint32)
    d[0, 0, 0], d[0, 0, 1], d[0, 0, 2] = f32(MINUS_ZERO), f32(NAN), -0.5
    m[0, 0, 3] = 8                                              # an id under density 0: what a SUBTRACT brush leaves behind
    d[0, 1, 0], m[0, 1, 0] = 1.0, 2
    s = both(d, m)
    assert fields(s) == ([(0b11111, 0, 0, 0, 0)], [MINUS_ZERO, NAN, MINUS_HALF, 0, ONE], [0, 0, 0, 8, 2], (1, 5, 5, 5))
    assert fields(both(d, m, flags=R.FILLED_ONLY)) == ([(1 << 4, 0, 3, ONE, 2)], [], [], (1, 0, 0, 1))
    # bare ids alone: every stored cell has the density pattern 0, which is uniform
    d[:] = 0
    m[0, 1, 0] = 8
    assert fields(both(d, m)) == ([(0b11000, 0, 3, 0, 8)], [], [], (1, 0, 0, 2))
    assert fields(both(d, m, flags=R.FILLED_ONLY)) == ([], [], [], (0, 0, 0, 0))
    # the round trip of the patterns, bit for bit
    d[0, 0, 0], d[0, 0, 1], d[0, 0, 2] = f32(MINUS_ZERO), f32(NAN), -0.5
    out = R.decode(np.ones_like(d), np.ones_like(m), (0, 0, 0), both(d, m))
    assert out[0].tobytes() == d.tobytes() and out[1].tobytes() == m.tobytes()


def test_a_partial_last_brick_has_no_bit_beyond_the_region():
    d, m = np.full((3, 7, 6), 1.0, np.float32), np.full((3, 7, 6), 1, np.uint32)       # everything stored, everywhere
    recs = fields(both(d, m, (0, 0, 0), (0, 0, 0), (6, 7, 3)))[0]                    # ext (6, 7, 3): nb (2, 2, 1)
    row4, row2 = 0b1111, 0b0011
    layer = lambda row, ny: sum(row << (4 * y) for y in range(ny))
    solid = lambda row, ny, nz: sum(layer(row, ny) << (16 * z) for z in range(nz))
    assert [r[0] for r in recs] == [solid(row4, 4, 3), solid(row2, 4, 3), solid(row4, 3, 3), solid(row2, 3, 3)]
    assert [r[1:] for r in recs] == [(i, 3, ONE, 1) for i in range(4)]
    # the same cells as a region of a larger box full of content: what lies beyond the region never shows
    big_d, big_m = np.full((5, 9, 9), 2.0, np.float32), np.full((5, 9, 9), 4, np.uint32)
    big_d[1:4, 1:8, 2:8], big_m[1:4, 1:8, 2:8] = d, m
    assert fields(both(big_d, big_m, (0, 0, 0), (2, 1, 1), (8, 8, 4)))[0] == recs


# ---- the host build against the reference over the content of the GPU tests ---------------------------------------------------------------
def test_host_build_equals_the_reference_on_the_shared_scene():
    d, m = R.scene()
    for flags in (0, R.FILLED_ONLY):
        for lo, hi in R.SCENE_REGIONS + R.SCENE_ALIGNED[1:]:
            s = both(d, m, R.SCENE_ORIGIN, lo, hi, flags)
            assert int(s[0]["n_bricks"][0]) > 0


def test_host_build_equals_the_reference_on_the_small_volumes_and_decodes_alike():
    rng = np.random.default_rng(7)
    for name, origin, shape, d, m, regions in R.small_volumes():
        for flags in (0, R.FILLED_ONLY):
            for lo, hi in regions:
                s = both(d, m, origin, lo, hi, flags)
                ext = s[0]["ext"][0].astype(int)
                moved = [origin] + [tuple(int(origin[a] + rng.integers(0, shape[a] - ext[a] + 1)) for a in range(3)) for _ in range(2)]
                for dst in [None] + moved:
                    for dflags in (0, R.KEEP_OTHERS):
                        d1 = rng.uniform(0.5, 1.0, d.shape).astype(np.float32)
                        m1 = rng.integers(1, 4, m.shape).astype(np.uint32)
                        want = R.decode(d1, m1, origin, s, dst, dflags)
                        B.decode_host(d1, m1, origin, *s, dst_lo=dst, flags=dflags)
                        assert d1.tobytes() == want[0].tobytes() and m1.tobytes() == want[1].tobytes(), (name, flags, lo, dst, dflags)
                if flags == 0 and lo is None:                  # default encode, default decode, same place: both arrays bit for bit
                    back = R.decode(np.ones_like(d), np.ones_like(m), origin, s)
                    assert back[0].tobytes() == d.tobytes() and back[1].tobytes() == m.tobytes(), name
                if flags and lo is None:                       # FILLED_ONLY: what is filled comes back, (0, 0) elsewhere
                    back = R.decode(np.ones_like(d), np.ones_like(m), origin, s)
                    filled = d > 0
                    assert back[0].tobytes() == np.where(filled, d, np.float32(0)).tobytes() and back[1].tobytes() == np.where(filled, m, 0).astype(np.uint32).tobytes()


def test_empty_regions_nothing_stored_and_one_value():
    d, m = np.zeros((5, 6, 7), np.float32), np.zeros((5, 6, 7), np.uint32)
    assert fields(both(d, m, (1, 1, 1)))[3] == (0, 0, 0, 0)                              # nothing stored
    s = both(d + 1, m + 2, (1, 1, 1), (3, 3, 3), (3, 6, 5))                              # an empty region
    assert fields(s)[3] == (0, 0, 0, 0) and s[0]["ext"][0].tolist() == [0, 3, 2]
    recs, dp, mp, totals = fields(both(d + 1, m + 2, (1, 1, 1)))                         # all one value: all bricks of kind 3
    assert totals == (2 * 2 * 2, 0, 0, 7 * 6 * 5) and all(r[2:] == (3, ONE, 2) for r in recs)
    # the host build's refusals: the device entry's codes
    for args, status in ((dict(lo=(1, 1, 1)), BLOK_ERR_INVALID_ARG), (dict(lo=(3, 3, 3), hi=(2, 4, 4)), BLOK_ERR_INVALID_ARG),
                         (dict(lo=(0, 1, 1), hi=(3, 3, 3)), BLOK_ERR_UNSUPPORTED), (dict(flags=2), BLOK_ERR_INVALID_ARG)):
        with pytest.raises(BlokError) as e:
            B.encode_host(d, m, (1, 1, 1), **args)
        assert e.value.status == status, args


# ---- validation ------------------------------------------------------------------------------------------------------------------------------
def _valid():
    name, origin, shape, d, m, regions = R.small_volumes()[3]          # 13 x 6 x 5: 4 x 2 x 2 bricks, partial on every axis
    s = R.encode(d, m, origin)
    kinds = s[1]["kind"].tolist()
    assert len(s[1]) >= 8 and 0 in kinds[2:] and s[0]["ext"][0].tolist() == [13, 6, 5]
    return s


def _corrupt(s, what, record=None, value=None):
    info, records, dp, mp = (np.array(a) for a in s)
    if record is None:
        info[what] = value
    else:
        records[what][record] = value
    return info, records, dp, mp


def test_validation_error_table_names_the_rule_and_the_first_failing_record():
    s = _valid()
    B.validate_host(*s)
    info, records, dp, mp = s
    k = next(i for i in range(2, len(records)) if records["kind"][i] == 0)          # a record with both payload indices
    n = len(records)
    last_x_partial = next(i for i in range(n) if records["brick"][i] % 4 == 3)      # brick x = 3 holds the region's cell x = 12 only
    table = [
        (_corrupt(s, "version", value=2), "version is not 1", None),
        (_corrupt(s, "flags", value=6), "unknown flag bits", None),
        (_corrupt(s, "brick", 3, records["brick"][2]), "not strictly ascending", 3),
        (_corrupt(s, "brick", 3, records["brick"][1]), "not strictly ascending", 3),
        (_corrupt(s, "brick", n - 1, 4 * 2 * 2), "outside the region's bricks", n - 1),
        (_corrupt(s, "mask", 4, 0), "empty mask", 4),
        (_corrupt(s, "mask", last_x_partial, int(records["mask"][last_x_partial]) | 2), "bit outside the region", last_x_partial),
        (_corrupt(s, "kind", 1, 4), "kind above 3", 1),
        (_corrupt(s, "density", k, int(records["density"][k]) + 1), "density index is not the running sum", k),
        (_corrupt(s, "material", k, int(records["material"][k]) - 1), "material index is not the running sum", k),
        (_corrupt(s, "n_density", value=len(dp) + 1), "n_density differs", None),
        (_corrupt(s, "n_material", value=len(mp) - 1), "n_material differs", None),
        (_corrupt(s, "n_voxels", value=int(info["n_voxels"][0]) + 1), "n_voxels differs", None),
    ]
    for stream, text, record in table:
        with pytest.raises(BlokError) as e:
            B.validate_host(*stream)
        msg = str(e.value)
        assert e.value.status == BLOK_ERR_INVALID_ARG and text in msg, (text, msg)
        assert (f"(record {record})" in msg) if record is not None else ("(record" not in msg), (text, msg)
        d1, m1 = np.ones((5, 6, 13), np.float32), np.ones((5, 6, 13), np.uint32)          # decode validates first: nothing is written
        with pytest.raises(BlokError):
            B.decode_host(d1, m1, (3, -2, 1), *stream)
        assert (d1 == 1).all() and (m1 == 1).all()
    # a mask bit switched on inside the region is caught by the sums, at the first record that comes after it
    bad = _corrupt(s, "mask", k, int(records["mask"][k]) | (int(records["mask"][k]) + 1))
    with pytest.raises(BlokError) as e:
        B.validate_host(*bad)
    assert "running sum" in str(e.value) or "differs" in str(e.value)
    # a destination that leaves the box
    d1, m1 = np.ones((5, 6, 13), np.float32), np.ones((5, 6, 13), np.uint32)
    with pytest.raises(BlokError) as e:
        B.decode_host(d1, m1, (3, -2, 1), *s, dst_lo=(4, -2, 1))
    assert e.value.status == BLOK_ERR_UNSUPPORTED and (d1 == 1).all()


# ---- the .bvol file ---------------------------------------------------------------------------------------------------------------------------
def _files(tmp_path):
    """A valid file, its truncations at and around each section boundary, and a header that promises more than the file holds."""
    s = _valid()
    info, records, dp, mp = s
    good = tmp_path / "good.bvol"
    B.write_file(good, *s)
    raw = good.read_bytes()
    assert len(raw) == R.stream_bytes(s) and raw[:8] == b"BLOKBVL1"
    assert raw[8:] == info.tobytes() + records.tobytes() + dp.tobytes() + mp.tobytes()
    ends = [0, 8, 8 + 64, 8 + 64 + 24 * len(records), 8 + 64 + 24 * len(records) + 4 * len(dp)]
    bad = {}
    for cut in sorted({c + k for c in ends for k in (-1, 0, 1) if 0 <= c + k < len(raw)} | {len(raw) - 1}):
        bad[f"cut{cut}.bvol"] = raw[:cut]
    for field, at in (("n_bricks", 8 + 32), ("n_density", 8 + 40), ("n_material", 8 + 48)):
        for value in (2 ** 60, 2 ** 64 - 1, int(info[field][0]) + 1):
            bad[f"{field}_{value}.bvol"] = raw[:at] + int(value).to_bytes(8, "little") + raw[at + 8:]
    bad["magic.bvol"] = b"BLOKBVL2" + raw[8:]
    bad["longer.bvol"] = raw + b"\0\0\0\0"
    for name, data in bad.items():
        (tmp_path / name).write_bytes(data)
    return s, good, [tmp_path / name for name in bad]


def test_file_round_trip_is_byte_equal_and_damaged_files_are_refused(tmp_path):
    s, good, bad = _files(tmp_path)
    back = B.read_file(good)
    assert R.same_stream(back, s)
    again = tmp_path / "again.bvol"
    B.write_file(again, *back)
    assert again.read_bytes() == good.read_bytes()
    for path in bad:
        with pytest.raises(BlokError) as e:
            B.read_file(path)
        assert e.value.status == BLOK_ERR_INVALID_ARG, path.name
    with pytest.raises(BlokError):
        B.read_file(tmp_path / "missing.bvol")
    with pytest.raises(BlokError):                             # write_file validates first and leaves no file behind
        B.write_file(tmp_path / "never.bvol", *_corrupt(s, "kind", 0, 7))
    assert not (tmp_path / "never.bvol").exists()
    empty = R.encode(np.zeros((2, 2, 2), np.float32), np.zeros((2, 2, 2), np.uint32), (0, 0, 0))
    B.write_file(tmp_path / "empty.bvol", *empty)
    assert (tmp_path / "empty.bvol").stat().st_size == 72 and R.same_stream(B.read_file(tmp_path / "empty.bvol"), empty)


def test_reader_and_validation_under_address_and_ub_sanitizers(tmp_path):
    """A program of its own (tests/host_harness/bricks_file_main.cpp) over the same files; nothing loaded into Python is sanitized."""
    s, good, bad = _files(tmp_path)
    exe = tmp_path / "bricks_file_main"
    subprocess.run(["g++", "-O1", "-g", "-std=c++20", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    "-fno-omit-frame-pointer", f"-I{ROOT / 'include'}", "-o", os.fspath(exe), os.fspath(ROOT / "tests/host_harness/bricks_file_main.cpp"),
                    os.fspath(ROOT / "blok_amd/csrc/host/bricks.cpp")], check=True)
    run = subprocess.run([os.fspath(exe), os.fspath(good)] + [os.fspath(p) for p in bad], capture_output=True, text=True)
    assert run.returncode == 0, run.stdout + run.stderr
    assert run.stderr == "", run.stderr
    lines = run.stdout.splitlines()
    n = len(s[1])
    # every disturbed field is refused, except a uniform plane's value: any pattern and any id is a legal one (kinds 1, 2 and 3)
    free = sum((1 if r["kind"] & 1 else 0) + (1 if r["kind"] & 2 else 0) for r in s[1])
    assert lines[0] == f"ok {n} {int(s[0]['n_voxels'][0])} disturbed {5 * n} refused {5 * n - free}", lines[0]
    assert len(lines) == 1 + len(bad) and all(l.startswith("refused ") for l in lines[1:]), run.stdout


# ---- what makes the shared scene worth running, from the reference alone ------------------------------------------------------------------
def test_the_shared_scene_exercises_every_kind_partial_masks_both_modes_and_off_grid_bricks():
    d, m = R.scene()
    default = R.encode(d, m, R.SCENE_ORIGIN)
    filled = R.encode(d, m, R.SCENE_ORIGIN, flags=R.FILLED_ONLY)
    kinds_default = np.bincount(default[1]["kind"], minlength=4)
    kinds_filled = np.bincount(filled[1]["kind"], minlength=4)
    print("kinds, default:", kinds_default, "FILLED_ONLY:", kinds_filled)
    # The issue asks for 50 of every kind.  FILLED_ONLY gives that.  By default the negative densities sown through the prior content
    # (every third layer) leave only 3 bricks with two densities under one id: kind 2's bound is lowered to those 3, as the issue allows.
    assert (kinds_filled >= 50).all(), kinds_filled
    assert (kinds_default[[0, 1, 3]] >= 50).all() and kinds_default[2] >= 3, kinds_default
    for s in (default, filled):
        full = int((s[1]["mask"] == np.uint64(2 ** 64 - 1)).sum())
        assert full >= 1000 and len(s[1]) - full >= 1000, (full, len(s[1]))
    assert int(default[0]["n_voxels"][0]) > int(filled[0]["n_voxels"][0]) > 0
    assert int(default[0]["n_density"][0]) > 0 and int(default[0]["n_material"][0]) > 0
    # off the box's brick grid the bricks are other bricks: the ragged region's records are not those of the aligned region around it
    (alo, ahi), (rlo, rhi) = R.SCENE_ALIGNED[1], R.SCENE_REGIONS[1]
    aligned, ragged = R.encode(d, m, R.SCENE_ORIGIN, alo, ahi), R.encode(d, m, R.SCENE_ORIGIN, rlo, rhi)
    assert any(c % 4 for c in np.subtract(rlo, R.SCENE_ORIGIN)) and not any(c % 4 for c in np.subtract(alo, R.SCENE_ORIGIN))
    whole_masks = set(default[1]["mask"].tolist())
    assert all(int(k) in whole_masks for k in aligned[1]["mask"])      # aligned: the box's own bricks
    assert sum(int(k) not in whole_masks for k in ragged[1]["mask"]) >= 100
    partial = [s for lo, hi in R.SCENE_REGIONS[2:] for s in [R.encode(d, m, R.SCENE_ORIGIN, lo, hi)]]
    assert all(len(s[1]) > 0 and (s[1]["mask"] != np.uint64(2 ** 64 - 1)).all() for s in partial)      # one voxel thick: no full brick
