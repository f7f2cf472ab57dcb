"""GPU: blok_hip_volume_edit_by_distance and blok_hip_volume_edit_by_flood — one kernel template over the op's rule (csrc/hip/field_edit.h) —
on the cases of tests/field_edit_cases.py, in both brick layouts: the returned count, then volume_download() against the numpy models of
the two contracts byte for byte (tests/test_field_edit_cpu.py shows from the models alone that a kernel which writes nothing, everything,
or drops the lone lane of a row's second segment cannot pass), the snapshot unchanged by the edit, and on the wide region the rebuilt tree:
the refresh ran over the edited box."""
import numpy as np
import pytest

from blok_amd import world as W
from tests import field_edit_cases as E
from tests.conftest import SEED
from tests.test_volume_rebuild_gpu import check
from tests.volume_tree_reference import DenseModel

pytestmark = pytest.mark.gpu

LAYOUTS = pytest.mark.parametrize("keyed", [True, False], ids=["keyed", "general"])


@pytest.fixture(scope="module")
def tr():
    from blok_amd.tracer import HipTracer
    t = HipTracer(96, 64).init()
    yield t
    t.shutdown()


@pytest.fixture(scope="module")
def mats():
    return W.scene_materials(SEED)


@LAYOUTS
@pytest.mark.parametrize("family,op,width", E.CASES, ids=E.IDS)
def test_the_edit_gives_the_references_arrays(tr, mats, keyed, family, op, width):
    d, m = E.noise()
    field, info, d_want, m_want, n_want = E.expected(family, op, width)
    lo, hi = E.region(width)
    tr.set_volume_layout(keyed)
    tr.volume_create(E.ORIGIN, E.SHAPE)
    tr.volume_upload(d, m)
    if family == "distance":
        radius, flags = E.field_args(family, op, width)
        got_info = tr.volume_distance_field(lo, hi, radius, to_empty=bool(flags))
        download, edit, threshold = tr.volume_distance_download, tr.volume_edit_by_distance, E.D2
    else:
        got_info = tr.volume_flood_field(lo, hi, *E.field_args(family, op, width))
        download, edit, threshold = tr.volume_flood_download, tr.volume_edit_by_flood, E.D
    before = download()
    assert before.tobytes() == field.tobytes() and got_info.tobytes() == info.tobytes(), "the snapshot is the reference's"
    n = edit(op, threshold, E.VALUE, E.MATERIAL)
    d_got, m_got = tr.volume_download()
    print(f"device wrote {n}, reference {n_want}; {int((d_got.view(np.uint32) != d_want.view(np.uint32)).sum())} densities and "
          f"{int((m_got != m_want).sum())} ids differ")
    assert n == n_want
    assert d_got.tobytes() == d_want.tobytes() and m_got.tobytes() == m_want.tobytes()
    assert download().tobytes() == before.tobytes(), "the edit leaves its snapshot alone"
    if width == E.WIDTHS[0]:                                      # once per op and layout
        model = DenseModel(E.ORIGIN, E.SHAPE)
        model.upload(d_want, m_want)
        check(tr, model, "edited", mats)
