"""What the beam pre-pass and the shadow rays' last-occluder map must hold, as numbers — TESTS ONLY, numpy, float64, no GPU.

Written from the comments of blok_amd/csrc/hip/beam.h, not from the kernel's arithmetic: both features are one search over the 64-tree
for "the filled voxels that meet a region of four half-spaces, each pushed out by kBeamSlack; a cell is culled only if its farthest corner
is strictly behind one", and the answer is an extreme of a linear function over those voxels.  Here the voxels are a plain list of world
coordinates (tree units) and the region test is applied to every one of them.

A float32 search cannot decide a voxel whose farthest corner lies within its own rounding error of a pushed-out plane, so every reference
comes as a pair: the `inner` set is cut with kBeamSlack - delta (voxels every correct search must keep), the `outer` set with
kBeamSlack + delta (voxels a correct search may keep).  A correct answer lies between the two extremes, give or take the error of the
extreme value itself.

delta, derived (eps = 2^-24, ulp(M) = the float32 spacing at M, M = the largest magnitude a plane value or one of its partial sums can
take in the case: with unit normals, at most the Euclidean norm of the per-axis largest |coordinate - ref| over the tree's cube — c only
brings a value back towards zero, the planes pass through the cube's neighbourhood):
  * root: p = fma(n.x, ox, fma(n.y, oy, n.z oz)) + c is four roundings of at most ulp(M) / 2: 2 ulp(M).  (The beam's ox = origin - eye
    is a rounding of its own per axis: 1 ulp(M) more, BEAM_ULPS = SUN_ULPS + 1; the sun map's ref is 0 and its origin an integer.)
  * per-lane steps a = dot(n, child) carry three roundings, 1.5 ulp(|a|); a step is s a with s a power of four, so the top level adds
    1.5 ulp(M) and every level below a quarter of the one above: 2 ulp(M) together.
  * descent: one fused step g = fma(s, a, p) per level, ulp(M) / 2 each, at most 7 levels: 3.5 ulp(M).
  * the corner: fma(s, far, g), ulp(M) / 2.
  SUN_ULPS = 2 + 2 + 3.5 + 0.5 = 8 ulp(M) — beam.h's "a few ulp of the coordinate magnitude".  The same bound holds for the depth value
  the search returns, with M taken for the depth plane.
The beam's planes are built on the device, so their normals carry an error that grows with the distance from the eye:
  * a corner direction p = fwd + right u + up v: inv_w by a 1 ulp reciprocal (2 eps relative), px inv_w (eps), the - 1 (eps absolute), the
    two factors tan_half_fov and aspect (eps each): |du| <= 6.1 eps ta, ta = tan_half_fov aspect (1 + 2 / w), likewise dv with
    t = tan_half_fov (1 + 2 / h); the two fused steps per component add 2 eps |p|: |dp| <= E(p) = eps (6.1 (ta + t) + 2 |p|).
  * side = p x q without fusing: per component two rounded products and a rounded difference,
    |dc| <= E(p) |q| + E(q) |p| + 3.5 eps |p| |q| + eps |c|, and the direction of c is off by |dc| / |c| radians — |c| = |p| |q| sin(angle
    between the two corner rays), which is what makes narrow tiles at narrow fields of view the worst case.
  * normalising: the dot product (3 eps), halved by the root, the 1 ulp rsq (2 eps) and the product (eps): a scale error of 4.5 eps.
  So plane k is off by at most e_k |x - eye| at the point x, e_k = |dc| / |c| + 4.5 eps, and the cut for plane k at voxel x is
  kBeamSlack -+ (BEAM_ULPS ulp(M) + e_k r(x)), r(x) = the distance of the voxel's farthest corner from the eye.  The depth along the central
  direction (no cancellation: e_mid = E(p) / |p| + 4.5 eps) is off by BEAM_ULPS ulp(M) + e_mid r(x), and the closing formula adds three roundings.
Nothing here is fitted to what the kernels return; the GPU test modules print the largest deviation from the nearer bound they saw.

Coordinates: voxels are (n, 3) integer world coordinates of their low corners in tree units (voxel (x, y, z) covers [x, x+1]^3)."""
from __future__ import annotations

import numpy as np

K_BEAM_SLACK = float(np.float32(0.05))
K_BEAM_NONE = float(np.float32(3.0e38))
EPS = 2.0 ** -24
SUN_ULPS = 8.0
BEAM_ULPS = 9.0
CORNERS = np.array([[(c >> a) & 1 for a in range(3)] for c in range(8)], dtype=np.float64)


def ulp32(x) -> float:
    return float(np.spacing(np.float32(abs(float(x)))))


def voxels_of(filled: np.ndarray, origin) -> np.ndarray:
    """World coordinates (n, 3) int64 of the True cells of a dense [z][y][x] array whose cell (0, 0, 0) is `origin`."""
    z, y, x = np.nonzero(np.asarray(filled))
    return np.stack([x, y, z], axis=1).astype(np.int64) + np.asarray(origin, dtype=np.int64)


def cube_of(voxels: np.ndarray, origin=None, levels=None):
    """(origin, edge) of the tree's cube: as given (world_stats), or the smallest power-of-four cube from the voxels' low corner."""
    if origin is not None and levels is not None:
        return np.asarray(origin, dtype=np.float64), float(4 ** int(levels))
    lo, hi = voxels.min(axis=0), voxels.max(axis=0) + 1
    edge = 4.0
    while edge < float((hi - lo).max()):
        edge *= 4.0
    return lo.astype(np.float64), edge


def _magnitude(cube_origin, edge, ref) -> float:
    o = np.asarray(cube_origin, dtype=np.float64) - np.asarray(ref, dtype=np.float64)
    return float(np.linalg.norm(np.maximum(np.abs(o), np.abs(o + edge))))


# ---- the shadow rays' last-occluder map ---------------------------------------------------------------------------------------------------
def sun_delta(info, cube_origin, edge) -> float:
    """delta of the map's side planes and of its values: SUN_ULPS ulp(M), M over the cube and one texel beyond it (the map's margin)."""
    return SUN_ULPS * ulp32(_magnitude(cube_origin, edge, (0.0, 0.0, 0.0)) + 2.0 * float(info["texel"]))


def frame_vectors(info):
    """(u, v, s) of a map's frame: the float32 values, exactly, as float64."""
    return tuple(np.asarray(info[k], dtype=np.float32).reshape(3).astype(np.float64) for k in ("u", "v", "s"))


def sun_footprints(voxels, info):
    """Per voxel: (u_min, u_max, v_min, v_max, far) — the (u, v) bounding rectangle of its eight corners and the largest s . corner."""
    u, v, s = frame_vectors(info)
    x = np.asarray(voxels, dtype=np.float64).reshape(-1, 3)
    pu, pv, ps = x @ u, x @ v, x @ s
    return (pu + np.minimum(u, 0).sum(), pu + np.maximum(u, 0).sum(), pv + np.minimum(v, 0).sum(), pv + np.maximum(v, 0).sum(),
            ps + np.maximum(s, 0).sum())


def texel_range(lo, hi, x0, texel, n, grow):
    """Texels i (clamped to the map; first > last where none) whose [x0 + i texel, x0 + (i + 1) texel] grown by `grow` meets [lo, hi]."""
    first = np.ceil((lo - grow - x0) / texel).astype(np.int64) - 1
    last = np.floor((hi + grow - x0) / texel).astype(np.int64)
    return np.maximum(first, 0), np.minimum(last, n - 1)


def _sun_one(voxels, info, grow):
    nu, nv = int(info["nu"]), int(info["nv"])
    u0, v0, texel = float(info["u0"]), float(info["v0"]), float(info["texel"])
    out = np.full(nu * nv, -K_BEAM_NONE, dtype=np.float64)
    if len(voxels) == 0:
        return out.reshape(nv, nu)
    umin, umax, vmin, vmax, far = sun_footprints(voxels, info)
    iu0, iu1 = texel_range(umin, umax, u0, texel, nu, grow)
    iv0, iv1 = texel_range(vmin, vmax, v0, texel, nv, grow)
    for dv in range(int(max((iv1 - iv0).max() + 1, 0))):
        for du in range(int(max((iu1 - iu0).max() + 1, 0))):
            iu, iv = iu0 + du, iv0 + dv
            ok = (iu <= iu1) & (iv <= iv1)
            np.maximum.at(out, iv[ok] * nu + iu[ok], far[ok])
    return out.reshape(nv, nu)


def sun_map_bounds(voxels, info, delta):
    """(lo, hi) [nv][nu] float64: the largest far(voxel) over inner(texel) and over outer(texel), -K_BEAM_NONE where the set is empty."""
    return _sun_one(voxels, info, K_BEAM_SLACK - delta), _sun_one(voxels, info, K_BEAM_SLACK + delta)


def sun_map_bounds_brute(voxels, info, delta):
    """The same by a loop over every texel and every voxel's eight corners: the pin of sun_map_bounds."""
    u, v, s = frame_vectors(info)
    nu, nv = int(info["nu"]), int(info["nv"])
    u0, v0, texel = float(info["u0"]), float(info["v0"]), float(info["texel"])
    lo = np.full((nv, nu), -K_BEAM_NONE)
    hi = np.full((nv, nu), -K_BEAM_NONE)
    for x in np.asarray(voxels, dtype=np.float64).reshape(-1, 3):
        corners = x + CORNERS
        cu, cv, far = corners @ u, corners @ v, (corners @ s).max()
        for iv in range(nv):
            for iu in range(nu):
                u_lo, v_lo = u0 + iu * texel, v0 + iv * texel
                for out, grow in ((lo, K_BEAM_SLACK - delta), (hi, K_BEAM_SLACK + delta)):
                    # a cell is culled only if its farthest corner is behind a side plane by more than the slack
                    culled = (cu.max() - u_lo < -grow or u_lo + texel - cu.min() < -grow or cv.max() - v_lo < -grow or v_lo + texel - cv.min() < -grow)
                    if not culled:
                        out[iv, iu] = max(out[iv, iu], far)
    return lo, hi


def sun_texel_lookup(info, origins):
    """path_core.h's texel lookup in float32 for ray origins (n, 3) float32: (inside, iu, iv)."""
    f = np.float32
    o = np.asarray(origins, dtype=np.float32).reshape(-1, 3)

    def dot(a):                                                       # vdot: x x + y y + z z in float32, left to right
        a = np.asarray(info[a], dtype=np.float32).reshape(3)
        return (a[0] * o[:, 0] + a[1] * o[:, 1]) + a[2] * o[:, 2]
    inv = f(1.0) / f(info["texel"])
    fu, fv = (dot("u") - f(info["u0"])) * inv, (dot("v") - f(info["v0"])) * inv
    inside = (fu >= 0) & (fv >= 0) & (fu < f(int(info["nu"]))) & (fv < f(int(info["nv"])))
    return inside, np.where(inside, fu, 0).astype(np.int64), np.where(inside, fv, 0).astype(np.int64)


def sun_capped_tmax(info, texels, origins, tmin, tmax):
    """The shadow rays' interval as path_core.h caps it: t_last = map - s . o in float32, cap = t_last + 0.05 + 1e-4 |t_last|, tmax =
    min(tmax, cap); returns (tmax', empty) with empty where cap <= tmin."""
    f = np.float32
    o = np.asarray(origins, dtype=np.float32).reshape(-1, 3)
    s = np.asarray(info["s"], dtype=np.float32).reshape(3)
    inside, iu, iv = sun_texel_lookup(info, o)
    last = np.asarray(texels, dtype=np.float32)[iv, iu]
    t_last = last - ((s[0] * o[:, 0] + s[1] * o[:, 1]) + s[2] * o[:, 2])
    cap = t_last + f(0.05) + f(1.0e-4) * np.abs(t_last)
    cap = np.where(inside, cap, f(tmax)).astype(np.float32)
    return np.minimum(f(tmax), cap).astype(np.float32), inside & (cap <= f(tmin))


# ---- beam tiles -------------------------------------------------------------------------------------------------------------------------
def tile_rects(rect, tile):
    """[(px, py, px_end, py_end)] of the rectangle's beam tiles, row-major: frame pixels [px, px_end) x [py, py_end)."""
    x0, y0, w, h = rect
    return [(x, y, min(x + tile, x0 + w), min(y + tile, y0 + h)) for y in range(y0, y0 + h, tile) for x in range(x0, x0 + w, tile)]


_camera_memo = {}


def camera_vectors(cam):
    """(pos, fwd, right, up, tan_half_fov, aspect) of a camera record in float64 (read-only arrays; the latest record is remembered)."""
    c = np.asarray(cam).reshape(-1)[0]
    key = c.tobytes()
    if key not in _camera_memo:
        _camera_memo.clear()
        g = lambda k: np.asarray(c[k], dtype=np.float64)
        vectors = (g("pos"), g("fwd"), g("right"), g("up"))
        for a in vectors:
            a.setflags(write=False)
        _camera_memo[key] = (*vectors, float(c["tan_half_fov"]), float(c["aspect"]))
    return _camera_memo[key]


def pixel_dir(cam, px, py, frame_w, frame_h):
    """Un-normalised direction through continuous pixel coordinates (px, py) of the frame."""
    _, fwd, right, up, t, a = camera_vectors(cam)
    u = (2.0 * px / frame_w - 1.0) * t * a
    v = (1.0 - 2.0 * py / frame_h) * t
    return fwd + right * u + up * v


def tile_planes(cam, frame_w, frame_h, tile_rect):
    """beam_start's region for one tile: (normals (4, 3) unit and oriented towards the centre, mid (3,) unit, e (4,), e_mid) with e the
    bound of each normal's error per unit distance from the eye (module docstring)."""
    px, py, px_end, py_end = (float(v) for v in tile_rect)
    _, _, _, _, t, a = camera_vectors(cam)
    raw = pixel_dir(cam, 0.5 * (px + px_end), 0.5 * (py + py_end), frame_w, frame_h)
    mid = raw / np.linalg.norm(raw)
    spread = 6.1 * (t * a * (1.0 + 2.0 / frame_w) + t * (1.0 + 2.0 / frame_h))
    err = lambda p: EPS * (spread + 2.0 * np.sqrt(p @ p))
    # the rectangle grown by one pixel on every side; corner i: x high for i = 1, 2; y high for i = 2, 3
    corner = [pixel_dir(cam, px_end + 1.0 if i in (1, 2) else px - 1.0, py_end + 1.0 if i >= 2 else py - 1.0, frame_w, frame_h) for i in range(4)]
    normals, e = np.zeros((4, 3)), np.zeros(4)
    for k in range(4):
        p, q = corner[k], corner[(k + 1) & 3]
        c = np.array([p[1] * q[2] - p[2] * q[1], p[2] * q[0] - p[0] * q[2], p[0] * q[1] - p[1] * q[0]])
        lp, lq, lc = np.sqrt(p @ p), np.sqrt(q @ q), np.sqrt(c @ c)
        n = c / lc
        normals[k] = n if n @ mid >= 0.0 else -n
        e[k] = (err(p) * lq + err(q) * lp + 3.5 * EPS * lp * lq + EPS * lc) / lc + 4.5 * EPS
    return normals, mid, e, err(raw) / np.linalg.norm(raw) + 4.5 * EPS


def beam_delta(cam, voxel_size, cube_origin, edge) -> float:
    """The distance-independent part of the beam's delta: BEAM_ULPS ulp(M), M over the cube as seen from the eye (voxel units)."""
    eye = camera_vectors(cam)[0] / float(voxel_size)
    return BEAM_ULPS * ulp32(_magnitude(cube_origin, edge, eye))


def _t0_of(best, voxel_size):
    return np.where(best >= K_BEAM_NONE, K_BEAM_NONE, np.maximum(best * (1.0 - 1.0e-4) - 2.0 * K_BEAM_SLACK, 0.0) * voxel_size)


def beam_tile_bounds(voxels, cam, frame_w, frame_h, rect, tile, voxel_size, delta0):
    """Per beam tile of the rectangle, row-major: (t0_lo, t0_hi, eps) float64.  t0_lo comes from the outer set and t0_hi from the inner
    set (K_BEAM_NONE where the set is empty); eps is the error of a correct float32 answer against either: delta of the depth carried
    through t0 = max(best (1 - 1e-4) - 2 kBeamSlack, 0) voxel_size, plus that formula's own three roundings."""
    x = np.asarray(voxels, dtype=np.float64).reshape(-1, 3)
    eye = camera_vectors(cam)[0] / float(voxel_size)
    rel = x - eye                                                     # low corners from the eye, voxel units
    reach = np.linalg.norm(np.maximum(np.abs(rel), np.abs(rel + 1.0)), axis=1)     # the farthest corner's distance: r(x)
    rects = tile_rects(rect, tile)
    lo, hi, eps = (np.zeros(len(rects)) for _ in range(3))
    planes = [tile_planes(cam, frame_w, frame_h, r) for r in rects]
    augmented = np.concatenate([rel, np.ones((len(rel), 1)), reach[:, None]], axis=1)
    chunk = 64                                                        # tiles per product: (voxels, 4 * chunk) values at a time
    for first in range(0, len(rects), chunk):
        some = planes[first:first + chunk]
        n_all = np.concatenate([p[0] for p in some])                  # (4 c, 3)
        e_all = np.concatenate([p[2] for p in some])
        # far corner's plane value + r(x) e_k in one product: [x, 1, r(x)] . [n_k, sum of n_k's positive parts, e_k]
        rows = np.concatenate([n_all, np.maximum(n_all, 0.0).sum(axis=1)[:, None], e_all[:, None]], axis=1)
        outer_all = (augmented @ rows.T >= -(K_BEAM_SLACK + delta0)).reshape(len(rel), len(some), 4).all(axis=2)
        for j, (normals, mid, e, e_mid) in enumerate(some):
            i = first + j
            left = np.nonzero(outer_all[:, j])[0]                     # the outer cut; the inner set lies inside it
            kept, kept_reach = rel[left], reach[left]
            far = kept @ normals.T + np.maximum(normals, 0.0).sum(axis=1)             # (n, 4)
            inner = (far >= -(K_BEAM_SLACK - (delta0 + kept_reach[:, None] * e[None, :]))).all(axis=1)
            outer = np.ones(len(left), bool)
            depth = np.maximum(kept @ mid + np.minimum(mid, 0.0).sum(), 0.0)          # nearest corner along mid; negative counts as 0
            best_in = depth[inner].min() if inner.any() else K_BEAM_NONE
            best_out = depth[outer].min() if outer.any() else K_BEAM_NONE
            lo[i], hi[i] = _t0_of(best_out, voxel_size), _t0_of(best_in, voxel_size)
            finite = [b for b in (best_in, best_out) if b < K_BEAM_NONE]
            far_best = max(finite) if finite else 0.0
            # a voxel at depth d along mid inside the frustum lies within d / cos(half diagonal) of the eye; its own reach bounds that
            r_best = float(kept_reach.max()) if outer.any() else 0.0
            eps[i] = (delta0 + e_mid * r_best + 3.0 * EPS * far_best) * voxel_size
    return lo, hi, eps


def beam_tile_bounds_brute(voxels, cam, frame_w, frame_h, rect, tile, voxel_size, delta0):
    """beam_tile_bounds by a loop over every tile, voxel, plane and corner: its pin."""
    eye = camera_vectors(cam)[0] / float(voxel_size)
    rects = tile_rects(rect, tile)
    lo, hi = np.zeros(len(rects)), np.zeros(len(rects))
    for i, r in enumerate(rects):
        normals, mid, e, _ = tile_planes(cam, frame_w, frame_h, r)
        best = {"in": K_BEAM_NONE, "out": K_BEAM_NONE}
        for x in np.asarray(voxels, dtype=np.float64).reshape(-1, 3):
            corners = x + CORNERS - eye
            reach = np.linalg.norm(corners, axis=1).max()
            depth = max((corners @ mid).min(), 0.0)
            for key, sign in (("in", -1.0), ("out", 1.0)):
                if all((corners @ normals[k]).max() >= -(K_BEAM_SLACK + sign * (delta0 + e[k] * reach)) for k in range(4)):
                    best[key] = min(best[key], depth)
        lo[i], hi[i] = _t0_of(np.float64(best["out"]), voxel_size), _t0_of(np.float64(best["in"]), voxel_size)
    return lo, hi


# ---- scenes the CPU and the GPU modules share -----------------------------------------------------------------------------------------------
def sun_frame(cube_origin, edge):
    """The map's frame for a tree cube, laid out as DESIGN.md describes it (one SUN_MAP_INFO-like dict of float32 values): s the shader's
    sun, u = normalize(s x Y), v = s x u, texels of one voxel (coarser beyond 2048 of them), one texel of margin below the cube's projection
    and one above.  For the CPU tests, which have no product to report a frame; any frame that covers the cube serves there."""
    f = np.float32
    s = np.array([0.5, 0.8, 0.3], dtype=np.float32)
    s = (s / np.sqrt((s * s).sum(dtype=np.float32))).astype(np.float32)
    sd = s.astype(np.float64)
    u = np.array([-sd[2], 0.0, sd[0]])
    u /= np.linalg.norm(u)
    v = np.cross(sd, u)
    u32, v32 = u.astype(np.float32), v.astype(np.float32)
    corners = np.asarray(cube_origin, dtype=np.float64) + CORNERS * float(edge)
    pu, pv = corners @ u32.astype(np.float64), corners @ v32.astype(np.float64)
    texel = max(1.0, np.ceil(max(pu.max() - pu.min(), pv.max() - pv.min()) / 2048.0))
    u0, v0 = np.floor(pu.min()) - texel, np.floor(pv.min()) - texel
    return {"u": u32, "v": v32, "s": s, "u0": f(u0), "v0": f(v0), "texel": f(texel),
            "nu": int(np.ceil((pu.max() - u0) / texel)) + 1, "nv": int(np.ceil((pv.max() - v0) / texel)) + 1}


def odd_world_voxels():
    """(xyz, material ids) of the world of tests/test_gpu_parity.py::test_beam_prepass_random_cameras_and_odd_worlds: it straddles the
    origin, with an isolated voxel far from the rest on either side and a one-voxel-thick wall."""
    rng = np.random.default_rng(2024)
    pts = rng.integers(-40, 40, size=(6000, 3)).astype(np.int32)
    wall = np.array([(x, y, 17) for x in range(-60, 60) for y in range(-30, 30)], dtype=np.int32)
    far = np.array([(-200, 90, -170), (211, -3, 140)], dtype=np.int32)
    xyz = np.concatenate([pts, wall, far])
    return xyz, rng.integers(1, 200, size=len(xyz)).astype(np.uint32)


def random_cameras(count, width, height, seed):
    """[(eye, target, fov)] as that test draws them: anywhere from deep inside the volume to far outside, any orientation, 4 .. 150 degrees."""
    rng = np.random.default_rng(seed)
    out = []
    for k in range(count):
        scale = (30.0, 80.0, 400.0)[k % 3]
        eye = rng.normal(0.0, scale, 3)
        target = eye + rng.normal(0.0, 1.0, 3) if k % 5 else rng.normal(0.0, 20.0, 3)
        if np.linalg.norm(target - eye) < 1e-3:
            target = eye + (1.0, 0.0, 0.0)
        out.append((tuple(float(c) for c in eye), tuple(float(c) for c in target), float(rng.uniform(4.0, 150.0))))
    return out
