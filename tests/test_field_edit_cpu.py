"""CPU: the cases of tests/field_edit_cases.py — all seven ops of edit_by_distance and edit_by_flood over regions 65, 64 and 1 cells wide —
from the numpy models of the two contracts alone: first that the cases can tell a broken edit from a working one, then that the host
build (blok_distance_edit, blok_flood_edit: the per-cell step the kernel shares, csrc/common/field_edit_core.h) gives the models' arrays
and counts byte for byte.  tests/test_field_edit_gpu.py holds the device to the same arrays."""
import numpy as np
import pytest

from blok_amd import distance as D
from blok_amd import flood as F
from tests import field_edit_cases as E
from tests import flood_reference as FR


def written(family, op, width):
    """Bool [z][y][x] over the region: the cells the references' edit changes or — where it writes what was there — would write: every
    written cell gets VALUE or 0 for a density that was neither, or MATERIAL or 0 for an id that was neither."""
    d, m = E.noise()
    _, info, d2, m2, n = E.expected(family, op, width)
    l = [int(info["lo"][0][a]) - E.ORIGIN[a] for a in range(3)]
    ext = [int(e) for e in info["ext"][0]]
    cut = (slice(l[2], l[2] + ext[2]), slice(l[1], l[1] + ext[1]), slice(l[0], l[0] + ext[0]))
    outside = np.ones(d.shape, bool)
    outside[cut] = False
    assert (d2[outside].tobytes(), m2[outside].tobytes()) == (d[outside].tobytes(), m[outside].tobytes()), "an edit stays in its region"
    w = (d2[cut].view(np.uint32) != d[cut].view(np.uint32)) | (m2[cut] != m[cut])
    assert int(w.sum()) == n, "every write of these cases changes its cell"
    return w


def test_the_noise_is_what_the_cases_say():
    d, m = E.noise()
    assert d.shape == m.shape == E.SHAPE[::-1]
    share = float((d > 0).mean())
    print(f"filled share {share:.3f}")
    assert 0.4 < share < 0.6
    assert set(np.unique(m[d > 0])) == {1, 2, 3} and not m[~(d > 0)].any()
    assert not (d == np.float32(E.VALUE)).any() and not (m == E.MATERIAL).any()
    assert all(c % 4 for c in E.CORNER), "the regions start off the brick grid"


@pytest.mark.parametrize("family,op,name", E.OPS, ids=[o[2] for o in E.OPS])
def test_every_op_writes_some_cells_of_the_wide_region_and_leaves_some(family, op, name):
    """A kernel that writes nothing, or everything, cannot pass."""
    w = written(family, op, 65)
    print(f"{name}: writes {int(w.sum())} of {w.size} cells, {int(w[:, :, 64].sum())} of them at x = 64")
    assert 0 < int(w.sum()) < w.size


def test_paint_changes_an_id_and_no_density():
    d, m = E.noise()
    _, _, d2, m2, n = E.expected("flood", FR.PAINT, 65)
    assert n > 0 and d2.tobytes() == d.tobytes() and int((m2 != m).sum()) == n


@pytest.mark.parametrize("family", ["distance", "flood"])
def test_a_write_lands_in_the_lone_lane_of_the_second_segment(family):
    """A kernel that drops the tail of a row cannot pass."""
    hits = {name: int(written(f, op, 65)[:, :, 64].sum()) for f, op, name in E.OPS if f == family}
    print(hits)
    assert any(hits.values())


@pytest.mark.parametrize("family,op,width", E.CASES, ids=E.IDS)
def test_the_host_build_gives_the_references_arrays(family, op, width):
    d, m = E.noise()
    field, info, d_want, m_want, n_want = E.expected(family, op, width)
    d2, m2 = d.copy(), m.copy()
    if family == "distance":
        n = D.distance_edit_host(d2, m2, E.ORIGIN, field, info, op, E.D2, E.VALUE, E.MATERIAL)
    else:
        n = F.flood_edit_host(d2, m2, E.ORIGIN, field, info, op, E.D, E.VALUE, E.MATERIAL)
    print(f"host wrote {n}, reference {n_want}; {int((d2.view(np.uint32) != d_want.view(np.uint32)).sum())} densities and {int((m2 != m_want).sum())} ids differ")
    assert n == n_want
    assert d2.tobytes() == d_want.tobytes() and m2.tobytes() == m_want.tobytes()
