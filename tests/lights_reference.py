"""TEST INFRASTRUCTURE: the light table and the light sample of include/blok_hip.h ("emissive voxels as lights") restated in
numpy, independent of the C++ (blok_amd/csrc/common/lights_core.h, path_core.h: light_sample).  Integer work in Python ints / uint64, float
work in float32 with every operation rounded once."""
from __future__ import annotations

import numpy as np

from blok_amd._ffi import LIGHT

f32 = np.float32
U32 = 0xFFFFFFFF
K_LIGHT_EPS = f32(0.004)
K_INV_PI = f32(0.31830988618)


def material_index(ids, n_materials: int):
    c = np.minimum(np.asarray(ids, dtype=np.int64), 65535)
    return np.where(c < n_materials, c, 0)


def emissive(materials) -> np.ndarray:
    """dot(emission, 1) > 0.01 in float32, summed left to right (raygen.rgen:158-160)."""
    e = np.asarray(materials["emission"], dtype=f32)
    return ((e[..., 0] + e[..., 1]) + e[..., 2]) > f32(0.01)


def from_quads(quads, materials):
    """The table blok_hip_lights_from_quads / blok_lights_from_quads build: (LIGHT records, A, owned material indices)."""
    glow = emissive(materials)
    idx = material_index(quads["material"], len(materials))
    keep = glow[idx] if len(quads) else np.zeros(0, dtype=bool)
    kept = quads[keep]
    out = np.zeros(len(kept), dtype=LIGHT)
    for k in ("lo", "du", "dv", "material", "face"):
        out[k] = kept[k]
    area = kept["du"].astype(np.uint64) * kept["dv"].astype(np.uint64)
    cum = np.concatenate([[0], np.cumsum(area, dtype=np.uint64)]).astype(np.uint64)
    total = int(cum[-1])
    assert total <= U32
    out["cum"] = cum[:-1].astype(np.uint32)
    return out, total, np.unique(idx[keep])


def pick_of(r: int, n_faces: int) -> int:
    return (int(r) * int(n_faces)) >> 32


def find_light(table, pick: int) -> int:
    """The last light whose cum is <= pick."""
    return int(np.searchsorted(table["cum"].astype(np.int64), int(pick), side="right")) - 1


def sample_point(light, off: int, u1, u2, vs):
    """(q, nl): the point of cell `off` of the light at the offsets u1, u2, and the light's normal."""
    du = int(light["du"])
    iu, iv = off % du, off // du
    face = int(light["face"])
    a = face >> 1
    u_ax, v_ax = (1 if a == 0 else 0), (1 if a == 2 else 2)
    lo = [int(c) for c in light["lo"]]
    vs = f32(vs)
    q = np.zeros(3, dtype=f32)
    q[a] = f32(lo[a]) * vs
    q[u_ax] = (f32(lo[u_ax] + iu) + f32(u1)) * vs
    q[v_ax] = (f32(lo[v_ax] + iv) + f32(u2)) * vs
    nl = np.zeros(3, dtype=f32)
    nl[a] = f32(-1.0) if face & 1 else f32(1.0)
    return q, nl


def dot3(a, b):
    a, b = np.asarray(a, dtype=f32), np.asarray(b, dtype=f32)
    return (a[..., 0] * b[..., 0] + a[..., 1] * b[..., 1]) + a[..., 2] * b[..., 2]


def geometry(hit_pos, n, q, nl, area_world):
    """DESIGN.md §32 c for one point: (g, x, dir, d); g = 0 means no term and no ray."""
    hit_pos, n, q, nl = (np.asarray(v, dtype=f32) for v in (hit_pos, n, q, nl))
    x = hit_pos + n * f32(0.001)
    w = q - x
    d2 = dot3(w, w)
    d = np.sqrt(d2)
    with np.errstate(all="ignore"):
        dr = w / d
    cos_s = max(dot3(n, dr), f32(0.0))
    cos_l = max(-dot3(nl, dr), f32(0.0))
    if not (cos_s > 0 and cos_l > 0 and d > f32(2.0) * K_LIGHT_EPS):
        return f32(0.0), x, dr, d
    g = (((cos_s * cos_l) / d2) * f32(area_world)) * K_INV_PI
    assert g.dtype == f32
    return g, x, dr, d


# ---- the shader's random numbers (raygen.rgen:77-99), vectorised over pixels in uint32 ----
def pcg(state):
    """(new state, output) of one pcg step on a uint32 array."""
    with np.errstate(over="ignore"):
        old = state.astype(np.uint32)
        new = old * np.uint32(747796405) + np.uint32(2891336453)
        word = ((old >> ((old >> np.uint32(28)) + np.uint32(4))) ^ old) * np.uint32(277803737)
        return new, (word >> np.uint32(22)) ^ word


def random_float(state):
    state, r = pcg(state)
    return state, r.astype(f32) / f32(4294967295.0)


def init_rng(px, py, width: int, frame: int, sample: int):
    with np.errstate(over="ignore"):
        seed = (np.asarray(px, dtype=np.uint32) + np.asarray(py, dtype=np.uint32) * np.uint32(width)).astype(np.uint32)
        seed = seed ^ (np.uint32(frame) * np.uint32(747796405))
        seed = seed ^ (np.uint32(sample) * np.uint32(1664525))
    seed, _ = pcg(seed)
    seed, _ = pcg(seed)
    return seed
