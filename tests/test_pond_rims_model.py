"""The host model of the pond rims (tests/pond_rims_model.py) against answers written out by hand: the yardstick of
tests/test_pond_rims.py has to be right before anything is held against it.  Labels come from tests/ponds_model.py."""
import numpy as np

from helpers import pad
from pond_rims_model import RIM_DTYPE, assert_same_rims, depth_from_key, depth_key, device_dem, rims
from ponds_model import inventory

MISS = -99999.0
WET = 0.001
INF = float("inf")


def model(dem, w, min_depth=WET):
    bd, bw = pad(np.asarray(dem, dtype=np.float64), np.asarray(w, dtype=np.float64), MISS)
    labels, table = inventory(bd > MISS, bw, min_depth)
    return labels, rims(labels, device_dem(bd, MISS), bw, len(table))


def rows(*r):
    return np.array(list(r), dtype=RIM_DTYPE)


def bowl(ring=20.0):
    dem = np.full((5, 5), 30.0)
    dem[1:4, 1:4] = ring
    dem[2, 2] = 10.0
    w = np.zeros((5, 5))
    w[2, 2] = 1.0
    return dem, w


def test_keys_order_doubles_and_come_back():
    v = np.array([-INF, -3.5, -5e-324, -0.0, 0.0, 5e-324, 1.0, 100.25, INF])
    k = depth_key(v)
    assert (k[1:] > k[:-1]).all()
    assert (depth_from_key(k).view(np.uint64) == v.view(np.uint64)).all()


def test_four_ponds_share_the_centre_cell():
    w = np.zeros((3, 3))
    w[::2, ::2] = 0.5
    labels, t = model(np.full((3, 3), 100.0), w)
    assert labels.max() == 4
    # padded coordinates; of the three rim cells of each pond the one with the smallest row-major index
    assert_same_rims(t, rows((100.5, 100.5, 100.0, 1, 2, 3, 5), (100.5, 100.5, 100.0, 1, 2, 3, 5),
                             (100.5, 100.5, 100.0, 2, 1, 3, 5), (100.5, 100.5, 100.0, 2, 2, 3, 5)))


def test_a_bowl_with_one_lowest_rim_cell():
    dem, w = bowl()
    dem[3, 2] = 15.0
    _, t = model(dem, w)
    assert_same_rims(t, rows((11.0, 11.0, 15.0, 4, 3, 8, 0)))
    assert t["rim_level"][0] - t["surface_max"][0] == 4.0           # freeboard


def test_a_tie_goes_to_the_smallest_index():
    _, t = model(*bowl())
    assert_same_rims(t, rows((11.0, 11.0, 20.0, 2, 2, 8, 0)))


def test_water_below_the_threshold_counts_on_the_rim():
    dem, w = bowl(21.0)
    dem[1, 2] = 20.0
    w[1, 2] = 0.0005
    labels, t = model(dem, w)
    assert labels[2, 3] == 0
    assert_same_rims(t, rows((11.0, 11.0, 20.0 + 0.0005, 2, 3, 8, 0)))


def test_nan_negative_and_zero_water_fall_to_the_dem():
    dem, w = bowl()
    dem[2, 1], w[2, 1] = 19.0, np.nan
    _, t = model(dem, w)
    assert_same_rims(t, rows((11.0, 11.0, 19.0, 3, 2, 8, 0)))
    w[2, 1] = -4.0
    assert_same_rims(model(dem, w)[1], rows((11.0, 11.0, 19.0, 3, 2, 8, 0)))
    w[2, 1] = -0.0
    assert_same_rims(model(dem, w)[1], rows((11.0, 11.0, 19.0, 3, 2, 8, 0)))


def test_minus_zero_sorts_below_plus_zero():
    dem, w = bowl(0.0)
    dem[2, 2] = -10.0
    dem[3, 3] = -0.0                                   # the last ring cell in index order, and still the lowest
    _, t = model(dem, w)
    assert_same_rims(t, rows((-9.0, -9.0, -0.0, 4, 4, 8, 0)))
    assert np.signbit(t["rim_level"][0])


def test_a_pond_enclosed_by_nodata_has_walls_and_no_rim():
    dem = np.full((3, 3), MISS)
    dem[1, 1] = 50.0
    w = np.full((3, 3), 0.25)                          # water on NODATA never makes a pond cell
    _, t = model(dem, w)
    assert_same_rims(t, rows((50.25, 50.25, INF, -1, -1, 0, 8)))
    assert t["rim_level"][0] - t["surface_max"][0] == INF


def test_all_wet_has_the_border_for_its_walls():
    R, C = 4, 6
    dem = 100.0 + np.arange(R * C).reshape(R, C)
    _, t = model(dem, np.full((R, C), 0.5))
    assert_same_rims(t, rows((100.5, 123.5, INF, -1, -1, 0, 2 * (R + C) + 4)))


def test_a_cell_is_a_rim_cell_of_at_most_four_ponds_and_once_each():
    w = np.zeros((9, 11))
    w[::2, ::2] = 0.5
    labels, t = model(np.full((9, 11), 100.0), w)
    n = labels.max()
    assert n == 30
    # a lattice cell in the interior has 8 dry neighbours, each counted once for it; one on the edge 5 and 3 walls, a corner 3 and 5
    corner, edge, interior = (3, 5), (5, 3), (8, 0)
    got = sorted(zip(t["rim_cells"].tolist(), t["wall_cells"].tolist()))
    assert got == sorted([corner] * 4 + [edge] * (2 * 3 + 2 * 4) + [interior] * (3 * 4))
    # memberships per dry cell: between two lattice cells 2, between four 4
    assert int(t["rim_cells"].sum()) == 4 * 3 + 14 * 5 + 12 * 8
