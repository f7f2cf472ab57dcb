"""CPU: object motion of moving instances (blok_amd/csrc/hip/instance_motion.h) and the instanced temporal pass (post_core.h).

The headers are compiled for the host through this test's own shim (tests/host_harness/motion_shim.cpp): the map from this frame's
instance placement to the previous one against a numpy float32 restatement, the tracking rule, and the instanced temporal pass against the
existing one on hand-built frames."""
from __future__ import annotations

import ctypes as C
import os
import subprocess
from pathlib import Path

import numpy as np
import pytest

from blok_amd._ffi import INSTANCE, INSTANCE_NONE
from tests import instance_oracle as IO

ROOT = Path(__file__).resolve().parent.parent
SRC = ROOT / "tests" / "host_harness"
N_PLANES = 15


class Settings(C.Structure):
    _fields_ = [(k, C.c_float) for k in ("temporal_alpha", "moment_alpha", "variance_clip_gamma", "depth_threshold", "normal_threshold",
                                         "phi_color", "phi_normal", "phi_depth")] + \
               [("atrous_iterations", C.c_int), ("variance_boost", C.c_float), ("min_history_length", C.c_int)]


def default_settings():
    return Settings(0.05, 0.2, 1.5, 0.1, 0.95, 0.5, 128.0, 0.1, 4, 1.5, 4)


@pytest.fixture(scope="module")
def shim(tmp_path_factory):
    out = tmp_path_factory.mktemp("motion_shim") / "libmotion_shim.so"
    subprocess.run(["g++", "-O1", "-std=c++20", "-fPIC", "-ffp-contract=off", "-Wall", f"-I{ROOT / 'include'}",
                    f"-I{ROOT / 'blok_amd/csrc/hip'}", f"-I{SRC}", "-shared", "-o", os.fspath(out), os.fspath(SRC / "motion_shim.cpp")], check=True)
    L = C.CDLL(os.fspath(out))
    L.ms_map.argtypes = [C.c_void_p, C.c_void_p, C.c_float, C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p, C.c_void_p]
    L.ms_tracked.argtypes = [C.c_void_p, C.c_uint32, C.c_void_p, C.c_uint32, C.c_void_p, C.c_void_p, C.c_uint32, C.c_void_p]
    L.ms_temporal.argtypes = [C.c_uint32, C.c_uint32, C.c_uint32, C.c_void_p, C.POINTER(Settings), C.c_void_p, C.c_void_p, C.c_void_p,
                              C.c_uint32, C.c_void_p, C.c_uint32, C.c_void_p, C.c_void_p, C.c_uint32, C.c_float]
    return L


def _p(a):
    return None if a is None else C.c_void_p(a.ctypes.data)


def shim_map(L, cur, prev, vs, p, n):
    cur = np.array([cur], dtype=INSTANCE)
    prev = np.array([prev], dtype=INSTANCE)
    p = np.ascontiguousarray(p, dtype=np.float32)
    n = np.ascontiguousarray(n, dtype=np.float32)
    op, on = np.zeros_like(p), np.zeros_like(n)
    L.ms_map(_p(cur), _p(prev), vs, _p(p), _p(n), len(p), _p(op), _p(on))
    return op, on


def numpy_map(cur, prev, vs, p, n):
    """instance_motion.h restated in float32: p_prev[b] = fl(c p[a] + float(prev.offset[b] - c cur.offset[a]) vs), n_prev[b] = c n[a]."""
    same = (list(cur["offset"]) == list(prev["offset"]) and list(cur["axis"]) == list(prev["axis"]) and int(cur["flip"]) == int(prev["flip"]))
    if same:
        return p.copy(), n.copy()
    pp, nn = np.zeros_like(p), np.zeros_like(n)
    for b in range(3):
        k = list(prev["axis"]).index(b)
        a = int(cur["axis"][k])
        neg = ((int(cur["flip"]) ^ int(prev["flip"])) >> k) & 1
        c = -1 if neg else 1
        d = np.float32(int(prev["offset"][b]) - c * int(cur["offset"][a]))
        pa = -p[:, a] if neg else p[:, a]
        pp[:, b] = pa + d * np.float32(vs)
        nn[:, b] = -n[:, a] if neg else n[:, a]
    return pp, nn


def world_voxels(inst, mx):
    """An instance's model voxels in world coordinates (tests/test_instance_paths_gpu.py: world_voxels)."""
    out = np.zeros_like(mx)
    flip = int(inst["flip"])
    for k in range(3):
        a = int(inst["axis"][k])
        o = int(inst["offset"][a])
        out[:, a] = (o - 1 - mx[:, k]) if (flip >> k) & 1 else (o + mx[:, k])
    return out


def face_normal(inst, k, n):
    """§11's face rule: local face 2k + n is world face 2 axis[k] + (n ^ flip_k); face 2a is +axis a, 2a + 1 is -axis a."""
    a = int(inst["axis"][k])
    f = n ^ ((int(inst["flip"]) >> k) & 1)
    v = np.zeros(3, dtype=np.float32)
    v[a] = -1.0 if f else 1.0
    return v


# ------------------------------------------------------------------------------------------------ the map
@pytest.mark.parametrize("vs", [1.0, 0.5])
def test_map_of_every_orientation_pair_equals_numpy(shim, vs):
    rng = np.random.default_rng(11 if vs == 1.0 else 12)
    n_pts = 12
    for pc, fc in IO.SIGNED_PERMUTATIONS:
        for pp_, fp in IO.SIGNED_PERMUTATIONS:
            cur = IO.instance(0, rng.integers(-30000, 30000, 3), pc, fc)
            prev = IO.instance(0, rng.integers(-30000, 30000, 3), pp_, fp)
            p = np.concatenate([rng.uniform(-30000, 30000, (n_pts // 2, 3)), rng.uniform(-3, 3, (n_pts // 2, 3))]).astype(np.float32)
            nrm = rng.normal(size=(n_pts, 3)).astype(np.float32)
            got_p, got_n = shim_map(shim, cur, prev, vs, p, nrm)
            want_p, want_n = numpy_map(cur, prev, vs, p, nrm)
            assert got_p.tobytes() == want_p.tobytes(), (pc, fc, pp_, fp)
            assert got_n.tobytes() == want_n.tobytes(), (pc, fc, pp_, fp)


def test_equal_placements_return_the_point_bit_for_bit(shim):
    rng = np.random.default_rng(5)
    p = np.array([[-0.0, 0.0, -0.0], [1e-30, -3.5, 7.25], [-20000.125, 12.0, 0.1]], dtype=np.float32)
    nrm = np.array([[-0.0, 1.0, 0.0], [0.6, -0.8, 0.0], [0.0, 0.0, -1.0]], dtype=np.float32)
    for axis, flip in IO.SIGNED_PERMUTATIONS:
        inst = IO.instance(3, rng.integers(-100, 100, 3), axis, flip)
        other = inst.copy()
        other["model"] = 4                                       # the model is not part of the placement
        got_p, got_n = shim_map(shim, inst, other, 1.0, p, nrm)
        assert got_p.tobytes() == p.tobytes() and got_n.tobytes() == nrm.tobytes()
    # a translation by zero through the arithmetic would turn -0 into +0: the identity does no arithmetic
    moved = IO.instance(0, (1, 0, 0))
    got_p, _ = shim_map(shim, IO.instance(0, (0, 0, 0)), moved, 1.0, p, nrm)
    assert got_p[0, 0] == 1.0 and np.signbit(got_p[0, 1]) == 0


@pytest.mark.parametrize("vs", [1.0, 0.5])
def test_a_model_voxel_centre_maps_to_the_same_voxel_centre(shim, vs):
    rng = np.random.default_rng(3)
    mx = rng.integers(0, 32, (40, 3)).astype(np.int64)
    for _ in range(300):
        cur = IO.instance(0, rng.integers(-500, 500, 3), *IO.SIGNED_PERMUTATIONS[rng.integers(48)])
        prev = IO.instance(0, rng.integers(-500, 500, 3), *IO.SIGNED_PERMUTATIONS[rng.integers(48)])
        p = ((world_voxels(cur, mx) + 0.5) * vs).astype(np.float32)
        want = ((world_voxels(prev, mx) + 0.5) * vs).astype(np.float32)
        got, _ = shim_map(shim, cur, prev, vs, p, np.zeros_like(p))
        assert got.tobytes() == want.tobytes()


def test_mapped_face_normals_follow_the_face_rule(shim):
    for pc, fc in IO.SIGNED_PERMUTATIONS:
        for pp_, fp in IO.SIGNED_PERMUTATIONS:
            cur, prev = IO.instance(0, (5, -2, 9), pc, fc), IO.instance(0, (-7, 1, 0), pp_, fp)
            faces = [(k, n) for k in range(3) for n in range(2)]
            nrm = np.array([face_normal(cur, k, n) for k, n in faces], dtype=np.float32)
            want = np.array([face_normal(prev, k, n) for k, n in faces], dtype=np.float32)
            _, got = shim_map(shim, cur, prev, 1.0, np.zeros_like(nrm), nrm)
            assert np.array_equal(got, want), (pc, fc, pp_, fp)


# ------------------------------------------------------------------------------------------------ tracking
def test_tracking_rule(shim):
    lohi = np.array([[0, 0, 0, 8, 8, 8], [0, 0, 0, 4, 4, 4], [0, 0, 0, 2, 2, 2]], dtype=np.int32)
    alive = np.array([1, 1, 1], dtype=np.uint8)
    cur = np.array([IO.instance(0, (10, 0, 0)), IO.instance(1, (0, 20, 0)), IO.instance(0, (3, 3, 3)), IO.instance(2, (1, 1, 1)),
                    IO.instance(1, (4, 4, 4)), IO.instance(1, (9, 9, 9))], dtype=INSTANCE)
    prev = cur[:5].copy()
    prev[0]["offset"] = (7, 0, 0)                                # moved: tracked
    prev[1]["axis"] = (2, 0, 1)                                  # turned: tracked
    prev[2]["model"] = 1                                         # a different model: untracked
    prev[3]["offset"] = (40000, 0, 0)                            # outside the lattice: unusable, untracked
    prev[4]["flip"] = 9                                          # malformed: unusable, untracked
    out = np.zeros(len(cur), dtype=np.uint8)
    shim.ms_tracked(_p(cur), len(cur), _p(prev), len(prev), _p(lohi), _p(alive), 3, _p(out))
    assert out.tolist() == [1, 1, 0, 0, 0, 0]                   # index 5 >= n_prev: appeared this frame
    alive[0] = 0                                                  # a destroyed model: untracked
    shim.ms_tracked(_p(cur), len(cur), _p(prev), len(prev), _p(lohi), _p(alive), 3, _p(out))
    assert out.tolist() == [0, 1, 0, 0, 0, 0]
    shim.ms_tracked(_p(cur), len(cur), _p(prev), len(prev), _p(lohi), _p(alive), 1, _p(out))
    assert out.tolist() == [0] * 6                               # model id beyond the store


# ------------------------------------------------------------------------------------------------ the temporal pass
W = H = 32
DEPTH_EYE = 60.0                                                 # camera plane at y = 60, looking down -y


def ortho_view_proj():
    """uv = (x / W, z / H): pixel (px, py) sees world (px + 0.5, *, py + 0.5); column-major."""
    m = np.zeros(16, dtype=np.float32)
    m[0] = 2.0 / W; m[12] = -1.0
    m[9] = 2.0 / H; m[13] = -1.0
    m[15] = 1.0
    return m


def plate_frame(x0, top, seed, x1=None):
    """Ground at y = 0 everywhere, a 12 x 12 plate with its top face at y = top over pixels [x0, x0 + 12) x [8, 20)."""
    rng = np.random.default_rng(seed)
    px, py = np.meshgrid(np.arange(W), np.arange(H))
    on = (px >= x0) & (px < x0 + 12) & (py >= 8) & (py < 20)
    y = np.where(on, top, 0.0)
    wp = np.stack([px + 0.5, y, py + 0.5, DEPTH_EYE - y], -1).astype(np.float32)
    nr = np.zeros((H, W, 4), np.float32)
    nr[..., 1] = 1.0
    nr[..., 3] = 0.5
    col = np.where(on[..., None], [0.8, 0.2, 0.2, 1.0], [0.2, 0.7, 0.3, 1.0]).astype(np.float32)
    col[..., :3] *= rng.uniform(0.9, 1.1, (H, W, 1)).astype(np.float32)
    ids = np.where(on, 0, INSTANCE_NONE).astype(np.uint32)
    return col, wp, nr, ids, on


class Temporal:
    """One temporal pass per call over a ping-pong history, through the shim (instanced when ids are given)."""

    def __init__(self, L):
        self.L = L
        n = W * H
        self.hist = [dict(color=np.zeros((n, 4), np.float32), moments=np.zeros((n, 2), np.float32), wp=np.zeros((n, 4), np.float32),
                          hl=np.zeros(n, np.uint16), un=np.zeros((n, 4), np.float32)) for _ in range(2)]
        self.motion = np.zeros((n, 2), np.uint16)
        self.cur = 0
        self.lohi = np.array([[0, 0, 0, 12, 1, 12]], dtype=np.int32)
        self.alive = np.ones(1, np.uint8)

    def run(self, frame, col, wp, nr, ids=None, cur=None, prev=None, vs=1.0):
        h, p = self.hist[self.cur], self.hist[self.cur ^ 1]
        planes = [col, wp, nr, None, p["color"], p["moments"], p["wp"], p["hl"], p["un"],
                  h["color"], h["moments"], h["wp"], h["un"], h["hl"], self.motion]
        arr = (C.c_void_p * N_PLANES)(*[None if a is None else a.ctypes.data for a in planes])
        s = default_settings()
        cur = np.zeros(0, INSTANCE) if cur is None else np.ascontiguousarray(cur, dtype=INSTANCE)
        prev = np.zeros(0, INSTANCE) if prev is None else np.ascontiguousarray(prev, dtype=INSTANCE)
        self.L.ms_temporal(W, H, frame, _p(ortho_view_proj()), C.byref(s), arr, _p(ids), _p(cur), len(cur), _p(prev), len(prev),
                           _p(self.lohi), _p(self.alive), 1, vs)
        self.cur ^= 1
        return {k: v.copy() for k, v in h.items()} | {"motion": self.motion.copy()}


def frames():
    """The plate moving by (3, 3, 0) voxels from frame 0 to frame 1, over a static camera."""
    a = plate_frame(4, 10.0, 1)
    b = plate_frame(7, 13.0, 2)
    ta, tb = IO.instance(0, (4, 9, 8)), IO.instance(0, (7, 12, 8))
    return a, b, np.array([ta], INSTANCE), np.array([tb], INSTANCE)


def equal_states(x, y):
    return all(x[k].tobytes() == y[k].tobytes() for k in x)


def test_instanced_pass_without_instance_pixels_or_motion_is_the_existing_pass(shim):
    a, b, ta, tb = frames()
    none_ids = [np.full((H, W), INSTANCE_NONE, np.uint32)] * 2
    # every id NONE (with moving tables), and the plate's ids with an unmoved table: the existing pass, every plane bit for bit
    for ids, tables in ((none_ids, (ta, tb)), ([a[3], b[3]], (tb, tb))):
        plain, inst = Temporal(shim), Temporal(shim)
        for k, (f, i) in enumerate(zip((a, b), ids)):
            want = plain.run(k, *f[:3])
            got = inst.run(k, *f[:3], ids=i, cur=tables[k], prev=tables[0] if k else None)
            assert equal_states(got, want), k


def test_a_moving_plate_keeps_its_history(shim):
    a, b, ta, tb = frames()
    plain, inst = Temporal(shim), Temporal(shim)
    plain.run(0, *a[:3]); inst.run(0, *a[:3], ids=a[3], cur=ta)
    want = plain.run(1, *b[:3])
    got = inst.run(1, *b[:3], ids=b[3], cur=tb, prev=ta)
    on = b[4].reshape(-1)
    interior = np.zeros((H, W), bool)
    interior[9:19, 8:18] = True                                   # >= 1 pixel inside the plate's footprint
    interior = interior.reshape(-1)
    hl_plain = want["hl"].view(np.float16).astype(np.float32)
    hl_inst = got["hl"].view(np.float16).astype(np.float32)
    assert (hl_plain[interior] == 1.0).all()                     # camera-only: the plate's points moved by more than 2 voxels
    assert (hl_inst[interior] == 2.0).all()                      # object motion: reprojected where they were
    # the object motion: 3 pixels in u (exact in binary16), 0 in v; the ground is the existing pass' bits
    mo = got["motion"].view(np.float16).astype(np.float32)
    assert np.array_equal(mo[on], np.tile([3.0 / W, 0.0], (on.sum(), 1)).astype(np.float32))
    for k in ("color", "moments", "hl", "un", "wp"):
        assert got[k][~on].tobytes() == want[k][~on].tobytes(), k
    assert got["motion"][~on].tobytes() == want["motion"][~on].tobytes()
    # the stored history geometry is the current frame's
    assert got["wp"].tobytes() == want["wp"].tobytes()


def test_an_untracked_instance_uses_no_history(shim):
    a, _, ta, _ = frames()
    plain, inst = Temporal(shim), Temporal(shim)
    plain.run(0, *a[:3]); inst.run(0, *a[:3], ids=a[3], cur=ta)
    want = plain.run(1, *a[:3])                                   # nothing moved: the plate accepts history in the existing pass
    changed = ta.copy()
    changed[0]["model"] = 1                                       # ... but it changed model
    got = inst.run(1, *a[:3], ids=a[3], cur=ta, prev=changed)
    on = a[4].reshape(-1)
    assert (want["hl"][on].view(np.float16) == 2.0).all()
    assert (got["hl"][on].view(np.float16) == 1.0).all()
    assert np.array_equal(got["color"][on][:, :3], a[0].reshape(-1, 4)[on][:, :3])       # the output is the current colour
    assert got["hl"][~on].tobytes() == want["hl"][~on].tobytes()
