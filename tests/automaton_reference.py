"""The numpy model of blok_hip_volume_automaton's contract (include/blok_hip.h) — TESTS ONLY, numpy alone, no code in common with the host
build (blok_amd/csrc/host/automaton.cpp) or the kernels.  The box is padded by one cell with the outside state, the count of a cell is the
sum of up to 26 shifted views, the rule is a table lookup, and the id of a born cell is np.unique over its voters: the cells of the
neighbourhood that lie inside the box and were filled before the step."""
from __future__ import annotations

import itertools

import numpy as np

BOX_IS_SOLID, FIXED_MATERIAL = 1, 2
INFO = np.dtype([("version", "<u4"), ("flags", "<u4"), ("lo", "<i4", 3), ("ext", "<u4", 3), ("steps_run", "<u4"), ("reserved", "<u4"), ("n_born", "<u8"),
                 ("n_died", "<u8"), ("n_filled", "<u8")])
# (dx, dy, dz) of the 26 neighbours; a neighbourhood is the offsets at squared distance <= 1, 2, 3
OFFSETS = [o for o in itertools.product((-1, 0, 1), repeat=3) if o != (0, 0, 0)]
REACH = {6: 1, 18: 2, 26: 3}


def offsets_of(neighbourhood):
    return [o for o in OFFSETS if o[0] * o[0] + o[1] * o[1] + o[2] * o[2] <= REACH[neighbourhood]]


def filled_of(d):
    with np.errstate(invalid="ignore"):
        return np.asarray(d, dtype=np.float32) > 0                # NaN, zeros of either sign and negative densities are empty


def local_region(shape_zyx, origin, lo, hi):
    nz, ny, nx = shape_zyx
    l = [0, 0, 0] if lo is None else [int(lo[a]) - int(origin[a]) for a in range(3)]
    h = [nx, ny, nz] if hi is None else [int(hi[a]) - int(origin[a]) for a in range(3)]
    assert all(0 <= l[a] <= h[a] <= (nx, ny, nz)[a] for a in range(3)), "the region lies in the box"
    return l, h


def step(d, m, l, h, neighbourhood, survive, birth, flags, density, material):
    """One synchronous step over the box-local region [l, h).  Returns (d, m, stats): new arrays, and the cells born, died, and born with
    a tie among their voters' ids."""
    filled = filled_of(d)
    nz, ny, nx = filled.shape
    state = np.full((nz + 2, ny + 2, nx + 2), bool(flags & BOX_IS_SOLID))
    state[1:-1, 1:-1, 1:-1] = filled
    votes = np.zeros(state.shape, bool)                            # filled before the step and inside the box
    votes[1:-1, 1:-1, 1:-1] = filled
    ids = np.zeros(state.shape, np.uint32)
    ids[1:-1, 1:-1, 1:-1] = m
    offs = offsets_of(neighbourhood)
    count = np.zeros(filled.shape, np.int64)
    for dx, dy, dz in offs:
        count += state[1 + dz:1 + dz + nz, 1 + dy:1 + dy + ny, 1 + dx:1 + dx + nx]
    stays = np.array([(survive >> n) & 1 for n in range(27)], bool)
    comes = np.array([(birth >> n) & 1 for n in range(27)], bool)
    region = np.zeros(filled.shape, bool)
    region[l[2]:h[2], l[1]:h[1], l[0]:h[0]] = True
    born = region & ~filled & comes[count]
    died = region & filled & ~stays[count]
    out_d, out_m = np.array(d, dtype=np.float32), np.array(m, dtype=np.uint32)
    out_d[died], out_m[died] = 0.0, 0
    out_d[born] = np.float32(density)
    n_ties = 0
    if flags & FIXED_MATERIAL:
        out_m[born] = material
    else:
        z, y, x = np.nonzero(born)
        voter = np.stack([votes[z + 1 + dz, y + 1 + dy, x + 1 + dx] for dx, dy, dz in offs], axis=1) if len(z) else np.zeros((0, len(offs)), bool)
        cast = np.stack([ids[z + 1 + dz, y + 1 + dy, x + 1 + dx] for dx, dy, dz in offs], axis=1) if len(z) else np.zeros((0, len(offs)), np.uint32)
        chosen = np.full(len(z), material, np.uint32)              # nobody votes: the rule's id
        for i in np.nonzero(voter.any(axis=1))[0]:
            values, n = np.unique(cast[i][voter[i]], return_counts=True)      # sorted: the first of the most voted is the smallest
            chosen[i] = values[np.argmax(n)]
            n_ties += int((n == n.max()).sum() > 1)
        out_m[z, y, x] = chosen
    return out_d, out_m, {"born": int(born.sum()), "died": int(died.sum()), "ties": n_ties}


def run(d, m, origin, lo, hi, rule):
    """The whole call.  rule: a mapping or record with the fields of blok_automaton_rule.  Returns (d, m, info, step_counts, ties): new
    arrays, one INFO record, a [steps][2] uint64 array of (born, died), and the born cells with a tied vote per step run."""
    get = lambda k: rule[k][0] if isinstance(rule, np.ndarray) else rule[k]
    nb, survive, birth, flags, steps = int(get("neighbourhood")), int(get("survive")), int(get("birth")), int(get("flags")), int(get("steps"))
    density, material = np.float32(get("density")), int(get("material"))
    d, m = np.array(d, dtype=np.float32), np.array(m, dtype=np.uint32)
    l, h = local_region(d.shape, origin, lo, hi)
    info = np.zeros(1, dtype=INFO)
    info["version"], info["flags"] = 1, flags
    info["lo"][0] = [int(origin[a]) + l[a] for a in range(3)]
    info["ext"][0] = [h[a] - l[a] for a in range(3)]
    counts = np.zeros((steps, 2), np.uint64)
    ties = []
    if all(h[a] > l[a] for a in range(3)):
        for k in range(steps):
            d, m, stats = step(d, m, l, h, nb, survive, birth, flags, density, material)
            info["steps_run"] = k + 1
            if stats["born"] == 0 and stats["died"] == 0:
                break
            counts[k] = stats["born"], stats["died"]
            ties.append(stats["ties"])
        info["n_born"], info["n_died"] = int(counts[:, 0].sum()), int(counts[:, 1].sum())
        info["n_filled"] = int(filled_of(d)[l[2]:h[2], l[1]:h[1], l[0]:h[0]].sum())
    return d, m, info, counts, ties
