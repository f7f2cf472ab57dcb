"""Object motion for posed models (include/blok_hip.h, "Object motion for posed models") restated in numpy: the motion record
in float64, the per-pixel map in float32, the object motion of a frame from its own planes, and §31's error bound.  The references of
tests/test_pose_motion_cpu.py and tests/test_pose_motion_gpu.py."""
from __future__ import annotations

import numpy as np

from blok_amd._ffi import INSTANCE_NONE, POSE, POSE_ID, POSE_MOTION

f32, f64 = np.float32, np.float64
U = 2.0 ** -24                      # half an ulp, relative
K_PREV = 16                         # §31: |p_prev - exact| <= K_PREV * U * magnitude(record, point)
DET_FLOOR_SQUARED = f64(2.0 ** -40)
MAX_M, MAX_POINT = 1024.0, 1048576.0


def floats_fine(p) -> bool:
    m, pivot, local = np.asarray(p["m"], f32), np.asarray(p["pivot"], f32), np.asarray(p["local"], f32)
    if not (np.isfinite(m).all() and np.isfinite(pivot).all() and np.isfinite(local).all()):
        return False
    return bool((np.abs(m) <= MAX_M).all() and (np.abs(pivot) <= MAX_POINT).all() and (np.abs(local) <= MAX_POINT).all())


def adjugate(m):
    """(adj, det) of a (3, 3) float64 matrix, in the header's term order, every operation a separate float64 one."""
    m = [[f64(v) for v in row] for row in m]
    (m00, m01, m02), (m10, m11, m12), (m20, m21, m22) = m
    c = [[m11 * m22 - m12 * m21, m02 * m21 - m01 * m22, m01 * m12 - m02 * m11],
         [m12 * m20 - m10 * m22, m00 * m22 - m02 * m20, m02 * m10 - m00 * m12],
         [m10 * m21 - m11 * m20, m01 * m20 - m00 * m21, m00 * m11 - m01 * m10]]
    det = (m00 * c[0][0] + m01 * c[1][0]) + m02 * c[2][0]
    return c, det


def record(cur, prev, model_usable=True) -> np.ndarray:
    """One POSE_MOTION record; prev None: the pose's index lies beyond the previous table."""
    out = np.zeros(1, dtype=POSE_MOTION)
    if prev is None or not model_usable or int(prev["model"]) != int(cur["model"]):
        return out
    if not (floats_fine(cur) and floats_fine(prev)):
        return out
    if np.asarray(cur, dtype=POSE).tobytes() == np.asarray(prev, dtype=POSE).tobytes():
        out["state"] = 1
        return out
    with np.errstate(all="ignore"):
        m = np.asarray(prev["m"], f32).astype(f64)
        M = np.asarray(cur["m"], f32).astype(f64)
        C, det = adjugate(m)
        s = [(m[k, 0] * m[k, 0] + m[k, 1] * m[k, 1]) + m[k, 2] * m[k, 2] for k in range(3)]
        if not (det * det > DET_FLOOR_SQUARED * ((s[0] * s[1]) * s[2])):
            return out
        inv_det = f64(1.0) / det
        inv = [[C[j][k] * inv_det for k in range(3)] for j in range(3)]
        A = [[(inv[i][0] * M[0, j] + inv[i][1] * M[1, j]) + inv[i][2] * M[2, j] for j in range(3)] for i in range(3)]
        dl = [f64(cur["local"][j]) - f64(prev["local"][j]) for j in range(3)]
        c = [(inv[i][0] * dl[0] + inv[i][1] * dl[1]) + inv[i][2] * dl[2] for i in range(3)]
        adj_a, det_a = adjugate(A)
        sign = f64(-1.0) if det_a < 0 else f64(1.0)
        a32 = np.array(A, f64).astype(f32)
        c32 = np.array(c, f64).astype(f32)
        n32 = np.array([[(-adj_a[j][i] if sign < 0 else adj_a[j][i]) for j in range(3)] for i in range(3)], f64).astype(f32)
    if not (np.isfinite(a32).all() and np.isfinite(c32).all() and np.isfinite(n32).all()):
        return out
    out["state"] = 2
    out["a"][0], out["c"][0], out["n"][0] = a32, c32, n32
    out["pivot_cur"][0], out["pivot_prev"][0] = cur["pivot"], prev["pivot"]
    return out


def map_point(R, p):
    """p_prev of (n, 3) float32 points under a state-2 record, every operation a separate float32 one."""
    p = np.asarray(p, f32)
    a, c, pc, pp = (np.asarray(R[k], f32).reshape(s) for k, s in (("a", (3, 3)), ("c", 3), ("pivot_cur", 3), ("pivot_prev", 3)))
    with np.errstate(all="ignore"):
        r = p - pc[None, :]
        q = np.stack([((a[i, 0] * r[:, 0] + a[i, 1] * r[:, 1]) + a[i, 2] * r[:, 2]) + c[i] for i in range(3)], axis=1)
        return (pp[None, :] + q).astype(f32)


def map_normal(R, n):
    n = np.asarray(n, f32)
    m = np.asarray(R["n"], f32).reshape(3, 3)
    with np.errstate(all="ignore"):
        v = np.stack([(m[i, 0] * n[:, 0] + m[i, 1] * n[:, 1]) + m[i, 2] * n[:, 2] for i in range(3)], axis=1).astype(f32)
        qq = (v[:, 0] * v[:, 0] + v[:, 1] * v[:, 1]) + v[:, 2] * v[:, 2]
        ok = qq > 0
        out = n.copy()
        out[ok] = v[ok] / np.sqrt(qq[ok])[:, None]
    return out.astype(f32)


def magnitude(R, p):
    """§31's magnitude of the map of points p under a state-2 record: max(|a|_inf |r|_inf, |c|_inf, |q|_inf, |pivot_prev|_inf), per point,
    in float64."""
    a, c, pc, pp = (np.asarray(R[k], f32).astype(f64).reshape(s) for k, s in (("a", (3, 3)), ("c", 3), ("pivot_cur", 3), ("pivot_prev", 3)))
    r = np.asarray(p, f32).astype(f64) - pc
    q = r @ a.T + c
    row = np.abs(a).sum(axis=1).max()
    return np.maximum.reduce([row * np.abs(r).max(axis=1), np.full(len(r), np.abs(c).max()), np.abs(q).max(axis=1), np.full(len(r), np.abs(pp).max())])


def prev_bound(R, p):
    return K_PREV * U * magnitude(R, p)


def project_prev(M, q):
    M = np.asarray(M, f32)
    x, y, z = q[:, 0], q[:, 1], q[:, 2]
    cx = ((M[0] * x + M[4] * y) + M[8] * z) + M[12]
    cy = ((M[1] * x + M[5] * y) + M[9] * z) + M[13]
    cw = ((M[3] * x + M[7] * y) + M[11] * z) + M[15]
    return (cx / cw) * f32(0.5) + f32(0.5), (cy / cw) * f32(0.5) + f32(0.5)


def pose_object_motion(world_pos, ids, records, prev_vp, x0, y0, frame_w, frame_h):
    """(tracked mask, float32 motion (h, w, 2)) of the pose pixels of a frame from its own planes: cu - project_prev(prev_view_proj, p_prev)."""
    h, w = ids.shape
    tracked = np.zeros((h, w), bool)
    mo = np.zeros((h, w, 2), f32)
    posed = (ids != INSTANCE_NONE) & ((ids & POSE_ID) != 0)
    for i in np.unique(ids[posed] & ~np.uint32(POSE_ID)):
        i = int(i)
        if i >= len(records) or int(records[i]["state"]) == 0:
            continue
        sel = ids == (POSE_ID | i)
        p = world_pos[sel][:, :3].astype(f32)
        q = p if int(records[i]["state"]) == 1 else map_point(records[i], p)
        with np.errstate(all="ignore"):
            pu, pv = project_prev(prev_vp, q)
            yy, xx = np.nonzero(sel)
            mo[sel, 0] = ((xx + x0).astype(f32) + f32(0.5)) / f32(frame_w) - pu
            mo[sel, 1] = ((yy + y0).astype(f32) + f32(0.5)) / f32(frame_h) - pv
        tracked |= sel
    return tracked, mo
