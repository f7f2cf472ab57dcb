"""CPU: object motion for posed models (include/blok_hip.h, "Object motion for posed models").

The shared core (blok_amd/csrc/common/pose_motion_core.h), the per-pixel map and id dispatch (blok_amd/csrc/hip/pose_motion.h) and the posed
mode of the temporal pass (post_core.h) are compiled for the host through this test's own shim (tests/host_harness/pose_motion_shim.cpp) and
held against tests/pose_motion_reference.py: the record against numpy float64 and the map against numpy float32, both bit for bit; the map
against the lattice map of instance_motion.h and against a float64 round trip within §31's bound; the posed temporal pass against the existing
one on hand-built frames."""
from __future__ import annotations

import ctypes as C
import math
import os
import subprocess
from pathlib import Path

import numpy as np
import pytest

from blok_amd import _ffi
from blok_amd import pose as P
from blok_amd._ffi import INSTANCE, INSTANCE_NONE, POSE, POSE_ID, POSE_MOTION
from tests import instance_oracle as IO
from tests import pose_cases as PC
from tests import pose_motion_reference as R

ROOT = Path(__file__).resolve().parents[1]
SRC = ROOT / "tests" / "host_harness"
FLAGS = ["-std=c++20", "-ffp-contract=off", "-Wall", f"-I{ROOT / 'include'}", f"-I{ROOT / 'blok_amd/csrc/hip'}", f"-I{SRC}"]
N_PLANES = 15
f32, f64 = np.float32, np.float64


class Settings(C.Structure):
    _fields_ = [(k, C.c_float) for k in ("temporal_alpha", "moment_alpha", "variance_clip_gamma", "depth_threshold", "normal_threshold", "phi_color",
                                         "phi_normal", "phi_depth")] + [("atrous_iterations", C.c_int), ("variance_boost", C.c_float),
                                                                        ("min_history_length", C.c_int)]


def default_settings():
    return Settings(0.05, 0.2, 1.5, 0.1, 0.95, 0.5, 128.0, 0.1, 4, 1.5, 4)


@pytest.fixture(scope="module")
def shim(tmp_path_factory):
    out = tmp_path_factory.mktemp("pose_motion_shim") / "libpose_motion_shim.so"
    subprocess.run(["g++", "-O1", "-fPIC", *FLAGS, "-shared", "-o", os.fspath(out), os.fspath(SRC / "pose_motion_shim.cpp")], check=True)
    L = C.CDLL(os.fspath(out))
    for name in ("pm_record", "pm_prepare", "pm_map", "pm_lattice_map", "pm_states", "pm_temporal", "pm_motion"):
        getattr(L, name).restype = None
    L.pm_record.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_void_p]
    L.pm_prepare.argtypes = [C.c_void_p, C.c_uint32, C.c_void_p, C.c_uint32, C.c_void_p, C.c_void_p, C.c_uint32, C.c_void_p]
    L.pm_map.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p, C.c_void_p]
    L.pm_lattice_map.argtypes = [C.c_void_p, C.c_void_p, C.c_float, C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p, C.c_void_p]
    L.pm_states.argtypes = [C.c_void_p, C.c_size_t, C.c_void_p, C.c_uint32, C.c_void_p, C.c_uint32, C.c_void_p, C.c_void_p, C.c_uint32, C.c_void_p,
                            C.c_uint32, C.c_void_p]
    L.pm_temporal.argtypes = [C.c_uint32, C.c_uint32, C.c_uint32, C.c_void_p, C.POINTER(Settings), C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint32,
                              C.c_void_p, C.c_uint32, C.c_void_p, C.c_void_p, C.c_uint32, C.c_float, C.c_void_p, C.c_uint32]
    return L


def _p(a):
    return None if a is None else C.c_void_p(a.ctypes.data)


def one(pose):
    return np.array([pose], dtype=POSE).reshape(1)


def shim_record(L, cur, prev, usable=True):
    out = np.zeros(1, dtype=POSE_MOTION)
    c, q = one(cur), (None if prev is None else one(prev))            # (held until the call returns)
    L.pm_record(_p(c), _p(q), int(usable), _p(out))
    return out


def shim_map(L, rec, p, n, through=False):
    p, n = np.ascontiguousarray(p, dtype=f32), np.ascontiguousarray(n, dtype=f32)
    op, on = np.zeros_like(p), np.zeros_like(n)
    L.pm_map(_p(rec), int(through), _p(p), _p(n), len(p), _p(op), _p(on))
    return op, on


# ------------------------------------------------------------------------------------------------ the cases
def far(pose, shift):
    q = pose.copy()
    q["pivot"] = (np.asarray(pose["pivot"], f64) + np.asarray(shift, f64)).astype(f32)
    return q


def case_poses():
    """The poses of tests/pose_cases.py at both voxel sizes (yaw, compound turns at scale 1.5, 0.5, 4 and 2, a mirror, a shear, a rank-2 map,
    lattice poses; three of the overflow case's seventy), each also with a far pivot, all naming model 0 so that every pair is tracked or
    not by its floats alone."""
    out = []
    for vs in (1.0, 0.5):
        for case in PC.table(vs):
            for q in case.poses[:3]:
                q = q.copy()
                q["model"] = 0
                out.append(q)
    uniq = {q.tobytes(): q for q in out}
    out = list(uniq.values())
    out += [far(q, s) for q, s in zip(out[:6], [(500000.0, -300000.25, 800000.5), (-1e6, 7.0, 3.0), (12345.678, 0.0, -999999.0)] * 2)]
    return out


def causes():
    """name -> (cur, prev or None, model_usable, expected state): every way to be untracked, and the near misses that stay tracked."""
    base = P.rotation(0, 0.3, 0.1, -0.2, 1.5, (8.0, 1.0, 8.0), (40.0, 70.0, 44.0))[0]
    moved = P.rotation(0, 0.5, 0.1, -0.2, 1.5, (8.0, 1.0, 8.0), (41.0, 72.0, 44.0))[0]
    out = {"moving": (moved, base, True, 2), "unmoved": (base, base, True, 1), "beyond n_prev": (moved, None, True, 0),
           "model not usable": (moved, base, False, 0)}
    other = base.copy(); other["model"] = 1
    out["another model"] = (moved, other, True, 0)
    for side in ("cur", "prev"):
        for what, field, value in (("nan", "local", np.nan), ("inf", "pivot", np.inf), ("big m", "m", 1025.0), ("big pivot", "pivot", 2.0 ** 20 + 1.0),
                                   ("big local", "local", -(2.0 ** 20) - 1.0)):
            bad = (moved if side == "cur" else base).copy()
            if field == "m":
                bad["m"][1][2] = value
            else:
                bad[field][1] = value
            out[f"{side}: {what}"] = (bad, base, True, 0) if side == "cur" else (moved, bad, True, 0)
    negzero = base.copy(); negzero["local"] = (0.0, 0.0, 0.0)
    poszero = negzero.copy(); negzero["local"][2] = -0.0
    out["-0.0 against +0.0"] = (negzero, poszero, True, 2)
    flat = base.copy(); flat["m"][2] = (0.0, 0.0, 0.0)
    out["singular prev"] = (moved, flat, True, 0)
    out["singular cur"] = (flat, base, True, 2)
    out["singular unmoved"] = (flat, flat, True, 1)                  # the identity needs no inverse
    for name, e, state in (("just below the floor", 2.0 ** -20, 0), ("just above the floor", 2.0 ** -20 * (1.0 + 2.0 ** -10), 2)):
        thin = base.copy(); thin["m"] = [[1.0, 0.0, 0.0], [0.0, 1.0, 0.0], [0.0, 1.0, e]]      # det = e, row norms 1, 1, sqrt(1 + e^2)
        out[f"prev {name}"] = (moved, thin, True, state)
    tiny = base.copy(); tiny["m"] = np.eye(3) * 1e-17                # invertible; A ~ 1e20 is finite, its cofactors ~ 1e40 are not
    big = base.copy(); big["m"] = np.eye(3) * 1000.0
    out["overflow"] = (big, tiny, True, 0)
    small = base.copy(); small["m"] = np.eye(3) * 1e-6
    out["no overflow"] = (big, small, True, 2)
    return out


# ------------------------------------------------------------------------------------------------ the record
def test_record_of_every_pair_of_case_poses_equals_numpy_float64(shim):
    poses = case_poses()
    assert len(poses) >= 20
    states = np.zeros(3, int)
    for a in poses:
        for b in poses:
            got, want = shim_record(shim, a, b), R.record(a, b)
            assert got.tobytes() == want.tobytes(), (a, b, got, want)
            states[int(got["state"][0])] += 1
            assert (int(got["state"][0]) == 1) == (a.tobytes() == b.tobytes())
    assert states[1] == len(poses) and states[2] > 300 and states[0] >= len(poses) - 1        # (the rank-2 pose as prev)
    # the shipped host helper is the same core
    for a, b in zip(poses, poses[1:] + poses[:1]):
        assert P.motion_record(a, b).tobytes() == R.record(a, b).tobytes()
        assert P.motion_record(a, None).tobytes() == R.record(a, None).tobytes()


def test_every_cause_of_an_untracked_pose(shim):
    for name, (cur, prev, usable, state) in causes().items():
        got, want = shim_record(shim, cur, prev, usable), R.record(cur, prev, usable)
        assert int(got["state"][0]) == state, name
        assert got.tobytes() == want.tobytes(), name
        assert P.motion_record(cur, prev, usable).tobytes() == want.tobytes(), name
        if state != 2:
            assert got.tobytes()[4:] == bytes(124), name


def test_prepare_body_applies_the_index_and_model_rules(shim):
    c = causes()
    cur = np.array([c["moving"][0]] * 6, dtype=POSE)
    prev = np.array([c["moving"][1]] * 5, dtype=POSE)
    cur[1]["model"] = prev[1]["model"] = 1                          # another live model: tracked
    cur[2]["model"] = prev[2]["model"] = 2                          # a destroyed model
    cur[3]["model"] = prev[3]["model"] = 3                          # a model whose box leaves the int16 lattice
    cur[4]["model"] = prev[4]["model"] = 9                          # beyond the store
    lohi = np.array([[0, 0, 0, 16, 2, 16], [0, 0, 0, 3, 3, 3], [0, 0, 0, 16, 2, 16], [0, 0, 0, 40000, 1, 1]], dtype=np.int32)
    alive = np.array([1, 1, 0, 1], dtype=np.uint8)
    out = np.zeros(6, dtype=POSE_MOTION)
    shim.pm_prepare(_p(cur), 6, _p(prev), 5, _p(lohi), _p(alive), 4, _p(out))
    assert out["state"].tolist() == [2, 2, 0, 0, 0, 0]             # index 5 >= n_prev: it appeared this frame
    assert out[0].tobytes() == R.record(cur[0], prev[0])[0].tobytes()
    # the id dispatch: poses by their record, one past the table, an instance id with no tables, the world
    ids = np.array([POSE_ID | 0, POSE_ID | 2, POSE_ID | 6, 0, INSTANCE_NONE], dtype=np.uint32)
    st = np.zeros(len(ids), dtype=np.uint8)
    shim.pm_states(_p(ids), len(ids), None, 0, None, 0, _p(lohi), _p(alive), 4, _p(out), 6, _p(st))
    assert st.tolist() == [1, 2, 2, 2, 0]


# ------------------------------------------------------------------------------------------------ the per-pixel map
def test_map_equals_numpy_float32(shim):
    rng = np.random.default_rng(21)
    poses = case_poses()
    n_moving = 0
    for a in poses:
        for b in poses[::3]:
            rec = R.record(a, b)
            if int(rec["state"][0]) != 2:
                continue
            n_moving += 1
            centre = np.asarray(a["pivot"], f64)
            p = np.concatenate([centre + rng.uniform(-40, 40, (8, 3)), rng.uniform(-3, 3, (2, 3)), rng.uniform(-1e6, 1e6, (2, 3))]).astype(f32)
            nrm = rng.normal(size=(len(p), 3))
            nrm = (nrm / np.linalg.norm(nrm, axis=1, keepdims=True)).astype(f32)
            nrm[0] = 0.0                                             # !(qq > 0): the normal comes back as it is
            got_p, got_n = shim_map(shim, rec, p, nrm)
            assert got_p.tobytes() == R.map_point(rec[0], p).tobytes()
            assert got_n.tobytes() == R.map_normal(rec[0], nrm).tobytes()
            assert got_n[0].tobytes() == nrm[0].tobytes()
            through = shim_map(shim, rec, p, nrm, through=True)
            assert through[0].tobytes() == got_p.tobytes() and through[1].tobytes() == got_n.tobytes()
    assert n_moving > 100
    # state 1: the identity with no arithmetic (-0.0 stays -0.0)
    p = np.array([[-0.0, 0.0, -0.0], [1e-30, -3.5, 7.25]], dtype=f32)
    rec = R.record(poses[0], poses[0])
    got_p, got_n = shim_map(shim, rec, p, p, through=True)
    assert got_p.tobytes() == p.tobytes() and got_n.tobytes() == p.tobytes()


@pytest.mark.parametrize("vs", [1.0, 0.5])
def test_lattice_poses_agree_with_the_lattice_map(shim, vs):
    """All 48 x 48 orientation pairs as poses made by blok_pose_from_instance: p_prev within §31's bound (plus the half ulp of map_point's own
    single rounding) of instance_motion.h's map_point; n_prev equal to map_normal on the six axis normals."""
    rng = np.random.default_rng(31 if vs == 1.0 else 32)
    axis_normals = np.array([(1, 0, 0), (-1, 0, 0), (0, 1, 0), (0, -1, 0), (0, 0, 1), (0, 0, -1)], dtype=f32)
    worst = 0.0
    for pc, fc in IO.SIGNED_PERMUTATIONS:
        for pp_, fp in IO.SIGNED_PERMUTATIONS:
            cur = np.array([IO.instance(0, rng.integers(-3000, 3000, 3), pc, fc)], dtype=INSTANCE)
            prev = np.array([IO.instance(0, rng.integers(-3000, 3000, 3), pp_, fp)], dtype=INSTANCE)
            rec = shim_record(shim, P.from_instance(cur, vs)[0], P.from_instance(prev, vs)[0])
            assert int(rec["state"][0]) == 2 or cur.tobytes() == prev.tobytes()
            if int(rec["state"][0]) != 2:
                continue
            p = ((cur["offset"][0] + rng.uniform(-20, 20, (6, 3))) * vs).astype(f32)
            got_p, got_n = shim_map(shim, rec, p, np.resize(axis_normals, (6, 3)))
            want_p, want_n = np.zeros_like(p), np.zeros_like(p)
            shim.pm_lattice_map(_p(cur), _p(prev), vs, _p(p), _p(axis_normals), 6, _p(want_p), _p(want_n))
            err = np.abs(got_p.astype(f64) - want_p.astype(f64)).max(axis=1)
            bound = R.prev_bound(rec[0], p) + R.U * np.abs(want_p.astype(f64)).max(axis=1)
            assert (err <= bound).all(), (pc, fc, pp_, fp, err, bound)
            worst = max(worst, float((err / bound).max()))
            assert np.array_equal(got_n, want_n), (pc, fc, pp_, fp)
    print(f"vs {vs}: worst error / bound {worst:.3f}")


@pytest.mark.parametrize("degrees", [7.0, 30.0, 90.0])
def test_round_trip_through_the_previous_pose(shim, degrees):
    """Points on the plate's faces, seen under cur, mapped to the previous frame, land within §31's bound of prev's forward image of their
    local point (float64)."""
    rng = np.random.default_rng(int(degrees))
    ext = np.array([16.0, 2.0, 16.0])
    worst = 0.0
    for position in ((40.0, 70.0, 44.0), (-3000.5, 900.25, 12000.0)):
        prev = P.rotation(0, math.radians(20.0), 0.0, 0.0, 1.5, tuple(ext / 2), position)[0]
        cur = P.rotation(0, math.radians(20.0 + degrees), math.radians(degrees / 3), 0.0, 1.5, tuple(ext / 2), tuple(c + d for c, d in zip(position, (1.0, 2.5, -0.5))))[0]
        rec = shim_record(shim, cur, prev)
        assert int(rec["state"][0]) == 2
        local = rng.uniform(0.0, 1.0, (60, 3)) * ext
        for k in range(60):                                          # onto one of the six faces
            local[k, (k // 2) % 3] = ext[(k // 2) % 3] * (k % 2)
        mc, mp = np.asarray(cur["m"], f64), np.asarray(prev["m"], f64)
        world = np.asarray(cur["pivot"], f64) + np.linalg.solve(mc, (local - np.asarray(cur["local"], f64)).T).T
        p = world.astype(f32)
        local_of_p = (p.astype(f64) - np.asarray(cur["pivot"], f64)) @ mc.T + np.asarray(cur["local"], f64)
        want = np.asarray(prev["pivot"], f64) + np.linalg.solve(mp, (local_of_p - np.asarray(prev["local"], f64)).T).T
        got, _ = shim_map(shim, rec, p, np.zeros_like(p))
        err = np.abs(got.astype(f64) - want).max(axis=1)
        bound = R.prev_bound(rec[0], p)
        assert (err <= bound).all(), (degrees, position, err.max(), bound.min())
        worst = max(worst, float((err / bound).max()))
        assert np.abs(got.astype(f64) - p).max() > 0.5               # the pose did move
    print(f"{degrees} degrees: worst error / bound {worst:.3f}")


# ------------------------------------------------------------------------------------------------ the temporal pass
W = H = 32
DEPTH_EYE = 60.0                                                 # camera plane at y = 60, looking down -y
EXT = (12.0, 1.0, 12.0)


def ortho_view_proj():
    """uv = (x / W, z / H): pixel (px, py) sees world (px + 0.5, *, py + 0.5); column-major."""
    m = np.zeros(16, dtype=f32)
    m[0] = 2.0 / W; m[12] = -1.0
    m[9] = 2.0 / H; m[13] = -1.0
    m[15] = 1.0
    return m


def plate_pose(yaw_degrees, centre):
    return P.rotation(0, math.radians(yaw_degrees), 0.0, 0.0, 1.0, tuple(e / 2 for e in EXT), centre)[0]


def plate_frame(pose, seed):
    """Ground at y = 0 everywhere and the 12 x 1 x 12 plate under `pose` (a yaw: its top face stays level), seen from above."""
    rng = np.random.default_rng(seed)
    px, py = np.meshgrid(np.arange(W), np.arange(H))
    top = float(pose["pivot"][1]) + EXT[1] / 2
    w = np.stack([px + 0.5, np.full(px.shape, top), py + 0.5], -1).reshape(-1, 3)
    local = (w - np.asarray(pose["pivot"], f64)) @ np.asarray(pose["m"], f64).T + np.asarray(pose["local"], f64)
    on = ((local[:, 0] >= 0) & (local[:, 0] < EXT[0]) & (local[:, 2] >= 0) & (local[:, 2] < EXT[2])).reshape(H, W)
    y = np.where(on, top, 0.0)
    wp = np.stack([px + 0.5, y, py + 0.5, DEPTH_EYE - y], -1).astype(f32)
    nr = np.zeros((H, W, 4), f32)
    nr[..., 1] = 1.0
    nr[..., 3] = 0.5
    col = np.where(on[..., None], [0.8, 0.2, 0.2, 1.0], [0.2, 0.7, 0.3, 1.0]).astype(f32)
    col[..., :3] *= rng.uniform(0.9, 1.1, (H, W, 1)).astype(f32)
    ids = np.where(on, POSE_ID | 0, INSTANCE_NONE).astype(np.uint32)
    return col, wp, nr, ids, on


class Temporal:
    """One temporal pass per call over a ping-pong history, through the shim (posed when ids are given)."""

    def __init__(self, L):
        self.L = L
        n = W * H
        self.hist = [dict(color=np.zeros((n, 4), f32), moments=np.zeros((n, 2), f32), wp=np.zeros((n, 4), f32),
                          hl=np.zeros(n, np.uint16), un=np.zeros((n, 4), f32)) for _ in range(2)]
        self.motion = np.zeros((n, 2), np.uint16)
        self.cur = 0
        self.lohi = np.array([[0, 0, 0, 12, 1, 12]], dtype=np.int32)
        self.alive = np.ones(1, np.uint8)

    def run(self, frame, col, wp, nr, ids=None, records=None):
        h, p = self.hist[self.cur], self.hist[self.cur ^ 1]
        planes = [col, wp, nr, None, p["color"], p["moments"], p["wp"], p["hl"], p["un"],
                  h["color"], h["moments"], h["wp"], h["un"], h["hl"], self.motion]
        arr = (C.c_void_p * N_PLANES)(*[None if a is None else a.ctypes.data for a in planes])
        s = default_settings()
        records = np.zeros(0, POSE_MOTION) if records is None else np.ascontiguousarray(records, dtype=POSE_MOTION)
        self.L.pm_temporal(W, H, frame, _p(ortho_view_proj()), C.byref(s), arr, _p(ids), None, 0, None, 0, _p(self.lohi), _p(self.alive), 1, 1.0,
                           _p(records) if len(records) else None, len(records))
        self.cur ^= 1
        return {k: v.copy() for k, v in h.items()} | {"motion": self.motion.copy()}


def turned_frames():
    """The plate turned by 10 degrees about its centre and lifted 3 voxels from frame 0 to frame 1, over a static camera."""
    pa, pb = plate_pose(0.0, (14.0, 9.5, 14.0)), plate_pose(10.0, (14.0, 12.5, 14.0))
    return plate_frame(pa, 1), plate_frame(pb, 2), pa, pb


def equal_states(x, y):
    return all(x[k].tobytes() == y[k].tobytes() for k in x)


def test_posed_pass_without_pose_pixels_or_motion_is_the_existing_pass(shim):
    a, b, pa, pb = turned_frames()
    none_ids = [np.full((H, W), INSTANCE_NONE, np.uint32)] * 2
    moving = [R.record(pa, None), R.record(pb, pa)]
    still = [R.record(pb, None), R.record(pb, pb)]
    a_still = plate_frame(pb, 1)
    # every id NONE (with a moving table), and the plate's ids with an unmoved table: the existing pass, every plane bit for bit
    for frames, ids, records in (((a, b), none_ids, moving), ((a_still, b), [a_still[3], b[3]], still)):
        plain, posed = Temporal(shim), Temporal(shim)
        for k, (f, i) in enumerate(zip(frames, ids)):
            want = plain.run(k, *f[:3])
            got = posed.run(k, *f[:3], ids=i, records=records[k])
            assert equal_states(got, want), k
        assert (want["hl"].view(np.float16) == 2.0).any()


def test_a_turned_and_lifted_plate_keeps_its_history(shim):
    a, b, pa, pb = turned_frames()
    plain, posed = Temporal(shim), Temporal(shim)
    plain.run(0, *a[:3]); posed.run(0, *a[:3], ids=a[3], records=R.record(pa, None))
    want = plain.run(1, *b[:3])
    rec = R.record(pb, pa)
    assert int(rec["state"][0]) == 2
    got = posed.run(1, *b[:3], ids=b[3], records=rec)
    on = b[4].reshape(-1)
    # interior: plate pixels of frame 1 whose point lay at least 1.5 voxels inside the plate one frame earlier
    was = R.map_point(rec[0], b[1].reshape(-1, 4)[:, :3]).astype(f64)
    local = (was - np.asarray(pa["pivot"], f64)) @ np.asarray(pa["m"], f64).T + np.asarray(pa["local"], f64)
    interior = on & (local[:, 0] > 1.5) & (local[:, 0] < EXT[0] - 1.5) & (local[:, 2] > 1.5) & (local[:, 2] < EXT[2] - 1.5)
    assert interior.sum() > 40
    hl_plain = want["hl"].view(np.float16).astype(f32)
    hl_posed = got["hl"].view(np.float16).astype(f32)
    assert (hl_plain[on] == 1.0).all()                           # camera-only: the plate's points moved by 3 voxels
    assert (hl_posed[interior] == 2.0).all()                     # object motion: reprojected where they were
    mo = got["motion"].view(np.float16).astype(f32)
    assert (np.abs(mo[interior]).max(axis=1) > 1e-3).mean() > 0.5
    for k in ("color", "moments", "hl", "un", "wp"):
        assert got[k][~on].tobytes() == want[k][~on].tobytes(), k
    assert got["motion"][~on].tobytes() == want["motion"][~on].tobytes()
    assert got["wp"].tobytes() == want["wp"].tobytes()
    # an untracked pose (state 0) takes no history even where nothing moved
    still = Temporal(shim)
    still.run(0, *b[:3], ids=b[3], records=R.record(pb, None))
    none = still.run(1, *b[:3], ids=b[3], records=R.record(pb, None))
    assert (none["hl"][on].view(np.float16) == 1.0).all() and (none["hl"][~on].view(np.float16) == 2.0).all()


# ------------------------------------------------------------------------------------------------ sanitizers, ABI
def test_shim_under_address_and_ub_sanitizers(tmp_path):
    """The shim as a stand-alone program (its own main) replays every cause and case pose through the prepare body, the map, the posed temporal
    pass and the motion pass.  Nothing loaded into Python is sanitized."""
    exe = tmp_path / "pose_motion_main"
    subprocess.run(["g++", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-fno-omit-frame-pointer", *FLAGS,
                    "-DPOSE_MOTION_SHIM_MAIN", "-o", os.fspath(exe), os.fspath(SRC / "pose_motion_shim.cpp")], check=True)
    rows = [(c, p if p is not None else c) for c, p, _, _ in causes().values()]
    poses = case_poses()
    rows += list(zip(poses, poses[1:] + poses[:1]))
    cur = np.array([r[0] for r in rows], dtype=POSE)
    prev = np.array([r[1] for r in rows], dtype=POSE)[:-2]            # the last two: beyond n_prev
    rng = np.random.default_rng(2)
    pts = rng.uniform(-100, 100, (16, 3)).astype(f32)
    nrm = rng.normal(size=(16, 3)).astype(f32)
    path = tmp_path / "cases.bin"
    with open(path, "wb") as f:
        f.write(np.array([len(cur), len(prev), len(pts)], dtype=np.uint32).tobytes())
        f.write(cur.tobytes()); f.write(prev.tobytes()); f.write(pts.tobytes()); f.write(nrm.tobytes())
    done = subprocess.run([os.fspath(exe), os.fspath(path)], capture_output=True, text=True)
    assert done.returncode == 0, done.stdout + done.stderr
    assert "moving" in done.stdout


def test_abi_and_symbols():
    lib = _ffi.hip_lib()
    assert lib.blok_hip_abi_version() >= (1 << 16) | 24
    for name in ("blok_hip_posed_motion_device", "blok_hip_denoise_posed_device", "blok_hip_denoise_posed_ref_device",
                 "blok_hip_draw_frame_rt_posed_motion", "blok_hip_debug_pose_motion_records"):
        assert hasattr(lib, name), name
    assert hasattr(_ffi.host_lib(), "blok_pose_motion_record")
