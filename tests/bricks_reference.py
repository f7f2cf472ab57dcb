"""The sparse brick stream's contract in numpy — TESTS ONLY, written from the header text (include/blok_hip.h: blok_hip_volume_encode_bricks)
and independent of blok_amd/csrc/common/bricks_core.h: boolean slicing per brick, np.unique for uniformity, Python integers for masks,
decode as plain array assignment.  Also the content the brick tests share."""
from __future__ import annotations

import numpy as np

from blok_amd import _ffi
from blok_amd import terrain as T
from tests.distance_reference import moved
from tests.terrain_cases import ISSUE, prior

FILLED_ONLY, KEEP_OTHERS = 1, 1


def bits(density) -> np.ndarray:
    return np.ascontiguousarray(density, dtype=np.float32).view(np.uint32)


def encode(density, ids, origin, lo=None, hi=None, flags=0):
    """density, ids: [z][y][x] over the box at world `origin`; region in world voxels, half open (both None = the whole box).
    Returns (info, records, density payload, material payload) in the library's dtypes."""
    density, ids = np.asarray(density, dtype=np.float32), np.asarray(ids, dtype=np.uint32)
    nz, ny, nx = density.shape
    lo = tuple(origin) if lo is None else tuple(int(c) for c in lo)
    hi = tuple(o + n for o, n in zip(origin, (nx, ny, nz))) if hi is None else tuple(int(c) for c in hi)
    l = [lo[a] - origin[a] for a in range(3)]
    ext = [hi[a] - lo[a] for a in range(3)]
    assert all(e >= 0 for e in ext) and all(l[a] >= 0 and l[a] + ext[a] <= (nx, ny, nz)[a] for a in range(3))
    d = bits(density)[l[2]:l[2] + ext[2], l[1]:l[1] + ext[1], l[0]:l[0] + ext[0]]
    m = ids[l[2]:l[2] + ext[2], l[1]:l[1] + ext[1], l[0]:l[0] + ext[0]]
    f = density[l[2]:l[2] + ext[2], l[1]:l[1] + ext[1], l[0]:l[0] + ext[0]]
    with np.errstate(invalid="ignore"):
        stored = (f > 0) if flags & FILLED_ONLY else ((d != 0) | (m != 0))
    nb = [(e + 3) // 4 for e in ext]
    records, dpay, mpay, n_voxels = [], [], [], 0
    bit_of = (np.arange(4)[None, None, :] + 4 * np.arange(4)[None, :, None] + 16 * np.arange(4)[:, None, None])      # [z][y][x] of a brick
    if all(ext):
        for bz in range(nb[2]):
            for by in range(nb[1]):
                for bx in range(nb[0]):
                    sl = (slice(4 * bz, 4 * bz + 4), slice(4 * by, 4 * by + 4), slice(4 * bx, 4 * bx + 4))
                    s = stored[sl]
                    if not s.any():
                        continue
                    b = bit_of[:s.shape[0], :s.shape[1], :s.shape[2]][s]      # the stored cells' bits, ascending: z, then y, then x
                    assert (np.diff(b) > 0).all()
                    mask = sum(1 << int(k) for k in b)
                    dv, mv = d[sl][s], m[sl][s]
                    kind = (1 if len(np.unique(dv)) == 1 else 0) | (2 if len(np.unique(mv)) == 1 else 0)
                    records.append((mask, bx + nb[0] * (by + nb[1] * bz), kind, int(dv[0]) if kind & 1 else sum(map(len, dpay)),
                                    int(mv[0]) if kind & 2 else sum(map(len, mpay))))
                    if not kind & 1:
                        dpay.append(dv)
                    if not kind & 2:
                        mpay.append(mv)
                    n_voxels += len(b)
    dp = np.concatenate(dpay).astype(np.uint32) if dpay else np.zeros(0, np.uint32)
    mp = np.concatenate(mpay).astype(np.uint32) if mpay else np.zeros(0, np.uint32)
    info = np.zeros(1, dtype=_ffi.BRICKS_INFO)
    info["version"], info["flags"], info["lo"], info["ext"] = 1, flags, lo, ext
    info["n_bricks"], info["n_density"], info["n_material"], info["n_voxels"] = len(records), len(dp), len(mp), n_voxels
    return info, np.array(records, dtype=_ffi.BRICK_RECORD).reshape(-1), dp, mp


def decode(density, ids, origin, stream, dst_lo=None, flags=0):
    """New arrays: `stream` written into [dst_lo, dst_lo + ext) (None = where it was taken) of the box's arrays."""
    info, records, dp, mp = stream
    d, m = bits(density).copy(), np.array(ids, dtype=np.uint32)
    ext = [int(e) for e in info["ext"][0]]
    lo = [int(c) for c in (info["lo"][0] if dst_lo is None else dst_lo)]
    l = [lo[a] - origin[a] for a in range(3)]
    assert all(l[a] >= 0 and l[a] + ext[a] <= d.shape[2 - a] for a in range(3))
    if not flags & KEEP_OTHERS:
        d[l[2]:l[2] + ext[2], l[1]:l[1] + ext[1], l[0]:l[0] + ext[0]] = 0
        m[l[2]:l[2] + ext[2], l[1]:l[1] + ext[1], l[0]:l[0] + ext[0]] = 0
    nb = [(e + 3) // 4 for e in ext]
    for r in records:
        brick, mask = int(r["brick"]), int(r["mask"])
        bx, by, bz = brick % nb[0], (brick // nb[0]) % nb[1], brick // (nb[0] * nb[1])
        rank = 0
        for b in range(64):
            if not (mask >> b) & 1:
                continue
            x, y, z = l[0] + 4 * bx + (b & 3), l[1] + 4 * by + ((b >> 2) & 3), l[2] + 4 * bz + (b >> 4)
            d[z, y, x] = r["density"] if r["kind"] & 1 else dp[int(r["density"]) + rank]
            m[z, y, x] = r["material"] if r["kind"] & 2 else mp[int(r["material"]) + rank]
            rank += 1
    return d.view(np.float32), m


def same_stream(a, b) -> bool:
    dt = (_ffi.BRICKS_INFO, _ffi.BRICK_RECORD, np.uint32, np.uint32)
    return all(np.ascontiguousarray(x, dtype=t).tobytes() == np.ascontiguousarray(y, dtype=t).tobytes() for x, y, t in zip(a, b, dt))


def stream_bytes(stream) -> int:
    """The size of the stream's .bvol file."""
    info, records, dp, mp = stream
    return 8 + 64 + 24 * len(records) + 4 * len(dp) + 4 * len(mp)


# ---- the content the CPU and GPU tests share ----------------------------------------------------------------------------------------------
SCENE_ORIGIN, SCENE_SHAPE = (-40, -44, -24), (96, 80, 64)
# the ragged regions of tests/test_quads_gpu.py (world voxels): unaligned in every axis, and one voxel thick in z, y and x
_SCENE_REGIONS = [(None, None), ((-31, -39, -13), (38, 21, 30)), ((-8, -20, 0), (24, 4, 1)), ((-40, 3, -24), (56, 4, 40)), ((17, -44, -20), (18, 36, 33))]
_SCENE_ALIGNED = [(None, None), ((-32, -40, -16), (40, 20, 32))]      # corners on the box's brick grid


def scene_regions(origin=SCENE_ORIGIN):
    """The ragged regions over the box SCENE_SHAPE at `origin`: the same box-local cells."""
    return moved(_SCENE_REGIONS, origin, SCENE_ORIGIN)


def scene_aligned(origin=SCENE_ORIGIN):
    return moved(_SCENE_ALIGNED, origin, SCENE_ORIGIN)


SCENE_REGIONS, SCENE_ALIGNED = scene_regions(), scene_aligned()
_scene = {}


def scene(origin=SCENE_ORIGIN):
    """The shared scene of the box at `origin`, computed once and never written to: prior() content with negative and NaN densities, the
    ISSUE terrain added on top (ADD: only where nothing is filled).  The terrain is a function of the world coordinate; its base height
    moves with the box's floor, so that its surface crosses the box wherever the box lies."""
    origin = tuple(origin)
    if origin not in _scene:
        nx, ny, nz = SCENE_SHAPE
        d, m = prior((nz, ny, nx))
        d[::3, ::2, ::5] = -0.5
        d[1::7, ::3, ::2] = np.nan
        p = _ffi.TerrainParams()
        for k, v in dict(ISSUE, flags=4, base_height=ISSUE["base_height"] + origin[1] - SCENE_ORIGIN[1]).items():
            setattr(p, k, v)
        hi = tuple(o + n for o, n in zip(origin, SCENE_SHAPE))
        d, m, _ = T.eval_box(p, origin, hi, d, m)
        d.setflags(write=False); m.setflags(write=False)
        _scene[origin] = (d, m)
    return _scene[origin]


def small_volumes():
    """(name, origin, shape_xyz, density, ids, regions): the small shapes of the GPU tests, each at the size where a path can go wrong."""
    out = []
    rng = np.random.default_rng(29)

    def content(shape, p=0.45):
        s = shape[::-1]
        d = np.where(rng.random(s) < p, rng.choice(np.array([0.25, 1.0, 1.5], np.float32), s), 0.0).astype(np.float32)
        d[::3, ::2, ::5] = -0.5
        d[rng.random(s) < 0.02] = np.nan
        d[rng.random(s) < 0.02] = -0.0
        m = np.where(d > 0, rng.integers(5, 8, s), 0).astype(np.uint32)
        m[rng.random(s) < 0.03] = 9                            # ids under whatever density is there, 0 included
        return d, m
    # nx % 4 == 0 and regions none of whose corners is a multiple of 4: dword loads
    o, shape = (-7, 3, -2), (24, 13, 9)
    d, m = content(shape)
    regions = [(None, None)] + [(tuple(a + c for a, c in zip(o, lo)), tuple(a + c for a, c in zip(o, hi)))
                                for lo, hi in (((1, 1, 1), (22, 11, 7)), ((5, 2, 3), (19, 10, 6)), ((17, 1, 5), (23, 13, 9)), ((2, 6, 1), (3, 7, 2)))]
    out.append(("24x13x9", o, shape, d, m, regions))
    out.append(("26x8x8", (0, 0, 0), (26, 8, 8), *content((26, 8, 8)), [(None, None), ((4, 0, 0), (26, 8, 8))]))      # nx % 4 != 0
    # 66 bricks along x: a full wave and a partial one per brick row, on the vector path; and a region starting on x = 8
    out.append(("264x8x8", (-100, 0, 0), (264, 8, 8), *content((264, 8, 8), 0.2), [(None, None), ((-92, 0, 4), (164, 7, 8))]))
    for shape in ((13, 6, 5), (1, 2, 3), (5, 9, 2)):
        out.append(("x".join(map(str, shape)), (3, -2, 1), shape, *content(shape), [(None, None)]))
    return out
