"""The host model of the pond inventory (tests/ponds_model.py) against hand-written answers and against scipy.ndimage.label.
CPU only.  tests/test_ponds.py holds the device against this model, so the model has to be right on its own evidence."""
import numpy as np
import pytest

from ponds_model import POND_DTYPE, inventory, pond_cells

Q = 2.0 ** -24


def padded(rows):
    """file-raster rows (lists) -> padded float array"""
    a = np.array(rows, dtype=np.float64)
    out = np.zeros((a.shape[0] + 2, a.shape[1] + 2))
    out[1:-1, 1:-1] = a
    return out


def valid_like(w, nodata=()):
    v = np.zeros(w.shape, dtype=bool)
    v[1:-1, 1:-1] = True
    for r, c in nodata:
        v[r, c] = False
    return v


def row(table, k):
    return tuple(table[k][n].item() for n in POND_DTYPE.names)


def test_corner_contact_is_one_pond():
    w = padded([[1.0, 0.0],
                [0.0, 2.0]])
    labels, table = inventory(valid_like(w), w, 0.5)
    assert labels.tolist() == [[0, 0, 0, 0], [0, 1, 0, 0], [0, 0, 1, 0], [0, 0, 0, 0]]
    assert row(table, 0) == (1, 1, 2, 3 << 24, 2.0, 1, 2, 1, 2)


def test_anti_diagonal_contact_is_one_pond():
    w = padded([[0.0, 1.0],
                [1.0, 0.0]])
    labels, table = inventory(valid_like(w), w, 0.0)
    assert labels[1:-1, 1:-1].tolist() == [[0, 1], [1, 0]]
    assert row(table, 0) == (1, 2, 2, 2 << 24, 1.0, 1, 2, 1, 2)


def test_u_whose_arms_meet_in_the_last_row():
    w = padded([[1, 0, 0, 0, 1],
                [1, 0, 0, 0, 1],
                [1, 0, 3, 0, 1],
                [1, 1, 1, 1, 1]])
    labels, table = inventory(valid_like(w), w, 0.0)
    # the right arm starts as its own run and must end up in pond 1; the island in the middle touches the bottom row diagonally
    assert labels[1:-1, 1:-1].tolist() == [[1, 0, 0, 0, 1], [1, 0, 0, 0, 1], [1, 0, 1, 0, 1], [1, 1, 1, 1, 1]]
    assert len(table) == 1
    assert row(table, 0) == (1, 1, 12, (11 + 3) << 24, 3.0, 1, 4, 1, 5)


def test_two_ponds_are_numbered_by_first_cell():
    w = padded([[0, 0, 0, 2],
                [1, 0, 0, 2],
                [1, 0, 0, 0]])
    labels, table = inventory(valid_like(w), w, 0.0)
    assert labels[1:-1, 1:-1].tolist() == [[0, 0, 0, 1], [2, 0, 0, 1], [2, 0, 0, 0]]
    assert row(table, 0) == (1, 4, 2, 4 << 24, 2.0, 1, 2, 4, 4)
    assert row(table, 1) == (2, 1, 2, 2 << 24, 1.0, 2, 3, 1, 1)


def test_nodata_column_cuts_a_pond_and_water_on_nodata_is_ignored():
    w = padded([[1, 1, 5, 1, 1],
                [1, 1, 5, 1, 1]])
    v = valid_like(w, nodata=[(1, 3), (2, 3)])
    labels, table = inventory(v, w, 0.0)
    assert labels[1:-1, 1:-1].tolist() == [[1, 1, 0, 2, 2], [1, 1, 0, 2, 2]]
    assert table["cells"].tolist() == [4, 4]
    assert table["max_depth"].tolist() == [1.0, 1.0]        # the 5 m on NODATA never counts
    assert table["volume_q"].tolist() == [4 << 24, 4 << 24]


def test_depth_equal_to_min_depth_is_dry():
    w = padded([[0.001, 0.0010000000000000002, 0.001]])
    labels, table = inventory(valid_like(w), w, 0.001)
    assert labels[1:-1, 1:-1].tolist() == [[0, 1, 0]]
    assert table["cells"].tolist() == [1]
    assert (table["first_row"][0], table["first_col"][0]) == (1, 2)


def test_border_and_nan_are_never_pond_cells():
    w = np.full((4, 5), 1.0)
    w[1, 2] = np.nan
    v = np.ones((4, 5), dtype=bool)       # even a DEM that claims a valid border
    wet = pond_cells(v, w, 0.0)
    assert wet.tolist() == [[False] * 5, [False, True, False, True, False], [False, True, True, True, False], [False] * 5]
    labels, table = inventory(v, w, 0.0)
    assert len(table) == 1 and table["cells"][0] == 5


def test_rint_ties_in_volume_q_go_to_even():
    # 0.5, 1.5, 2.5 quanta -> 0, 2, 2; 3.5 -> 4; just above a tie rounds up
    depths = [0.5 * Q, 1.5 * Q, 2.5 * Q, 3.5 * Q, 0.5 * Q * (1 + 2.0 ** -52)]
    w = padded([depths])
    labels, table = inventory(valid_like(w), w, 0.0)
    assert len(table) == 1 and table["cells"][0] == 5
    assert table["volume_q"][0] == 0 + 2 + 2 + 4 + 1
    assert table["max_depth"][0] == 3.5 * Q


def test_subnormal_depths_are_wet_and_exact():
    tiny = np.nextafter(0.0, 1.0)
    w = padded([[tiny, 3.25]])
    labels, table = inventory(valid_like(w), w, 0.0)
    assert table["cells"].tolist() == [2]
    assert table["volume_q"][0] == int(3.25 * 2 ** 24)
    assert table["max_depth"][0] == 3.25


def test_all_dry_gives_an_empty_table():
    w = padded([[0.0, 0.0], [0.0, 0.0]])
    labels, table = inventory(valid_like(w), w, 0.0)
    assert not labels.any() and labels.dtype == np.int32
    assert len(table) == 0 and table.dtype == POND_DTYPE


def canonical(labels):
    """renumber any labelling by first cell in row-major order"""
    flat = labels.ravel()
    nz = np.flatnonzero(flat)
    _, first = np.unique(flat[nz], return_index=True)
    order = np.argsort(first)
    lut = np.zeros(flat.max() + 1, dtype=np.int32)
    lut[np.unique(flat[nz])[order]] = np.arange(1, len(order) + 1)
    return lut[labels]


@pytest.mark.parametrize("shape,density,seed", [((40, 57), 0.30, 1), ((64, 130), 0.41, 2), ((129, 67), 0.60, 3), ((200, 300), 0.41, 4)])
def test_against_scipy_label(shape, density, seed):
    ndi = pytest.importorskip("scipy.ndimage")
    rng = np.random.default_rng(seed)
    w = np.zeros((shape[0] + 2, shape[1] + 2))
    w[1:-1, 1:-1] = np.where(rng.random(shape) < density, rng.random(shape) * 4.0, 0.0)
    v = valid_like(w)
    v[1:-1, 1:-1] &= rng.random(shape) > 0.05
    labels, table = inventory(v, w, 0.001)
    wet = pond_cells(v, w, 0.001)
    ref, n = ndi.label(wet, structure=np.ones((3, 3), dtype=int))
    assert n == len(table)
    assert (canonical(ref) == labels).all()
    idx = np.arange(1, n + 1)
    lab = canonical(ref)
    assert (table["cells"] == np.bincount(lab.ravel(), minlength=n + 1)[1:]).all()
    assert (table["max_depth"] == ndi.maximum(w, lab, idx)).all()
    q = np.rint(w * 2.0 ** 24).astype(np.int64)
    assert (table["volume_q"].astype(np.int64) == ndi.sum_labels(q, lab, idx).astype(np.int64)).all()
    objs = ndi.find_objects(lab)
    for k, sl in enumerate(objs):
        assert (table["row_min"][k], table["row_max"][k] + 1, table["col_min"][k], table["col_max"][k] + 1) == \
            (sl[0].start, sl[0].stop, sl[1].start, sl[1].stop)
        r0 = sl[0].start
        assert table["first_row"][k] == r0 and table["first_col"][k] == np.flatnonzero(lab[r0] == k + 1)[0]
