"""The host model of the pond catchments (tests/pond_catchments_model.py) against answers written by hand: the model is the
yardstick of the device tests, so it is held to the definitions of include/wdpm_pond_catchments.h here, case by case.  The identity
sum(pond cells) + sum(catch_cells) + unponded_cells == cells with a level is asserted inside the model on every call."""
import numpy as np

from helpers import pad
from pond_catchments_model import catchments, descent_length
from pond_rims_model import device_dem
from ponds_model import inventory

MISS = -99999.0
N = MISS
INF = np.inf


def run(dem, w, min_depth=0.001):
    dem, w = np.atleast_2d(np.asarray(dem, dtype=np.float64)), np.atleast_2d(np.asarray(w, dtype=np.float64))
    bd, bw = pad(dem, w, MISS)
    labels, ponds = inventory(bd > MISS, bw, min_depth)
    basin, table, stats = catchments(labels, device_dem(bd, MISS), bw, ponds)
    assert (basin[0] == -1).all() and (basin[-1] == -1).all() and (basin[:, 0] == -1).all() and (basin[:, -1] == -1).all()
    return basin[1:-1, 1:-1].tolist(), table, stats, (labels, device_dem(bd, MISS), bw)


def row(table, k):
    return tuple(table[k].tolist())


def test_a_ramp_into_a_pond():
    basin, t, s, raw = run([5, 4, 3, 2, 1], [0, 0, 0, 0, 0.5])
    assert basin == [[1, 1, 1, 1, 1]]
    assert row(t, 0) == (4, 1, 5.0, 1, 1, 1, 5)
    assert s == dict(slope_cells=4, pit_cells=0, unponded_cells=0, ponds=1)
    assert descent_length(*raw) == 4        # the fourth step enters the pond


def test_a_ridge_between_two_ponds_ties_to_the_smaller_index():
    basin, t, s, _ = run([1, 2, 3, 2, 1], [0.5, 0, 0, 0, 0.5])
    assert basin == [[1, 1, 1, 2, 2]]       # the ridge cell sees 2 m on both sides: left is the smaller index
    assert row(t, 0) == (2, 1, 3.0, 1, 1, 1, 3) and row(t, 1) == (1, 1, 2.0, 1, 1, 4, 5)
    assert s == dict(slope_cells=3, pit_cells=0, unponded_cells=0, ponds=2)
    # a column of the same: up is the smaller index
    basin, t, _, _ = run([[1], [2], [3], [2], [1]], [[0.5], [0], [0], [0], [0.5]])
    assert basin == [[1], [1], [1], [2], [2]] and row(t, 0) == (2, 1, 3.0, 1, 3, 1, 1)
    # up-right against left: the row above comes first
    basin, _, _, _ = run([[9, 9, 1], [1, 3, 9]], [[0, 0, 0.5], [0.5, 0, 0]])
    assert basin[1][1] == 1 and basin[1][0] == 2


def test_every_cell_of_a_flat_is_a_pit():
    basin, t, s, _ = run(np.full((3, 3), 7.0), np.zeros((3, 3)))
    assert basin == [[0] * 3] * 3 and len(t) == 0
    assert s == dict(slope_cells=9, pit_cells=9, unponded_cells=9, ponds=0)
    # a pond at a pond's own level is not strictly lower either
    basin, t, s, _ = run([1, 2, 2], [1, 0, 0])
    assert basin == [[1, 0, 0]] and row(t, 0) == (0, 0, -INF, 1, 1, 1, 1) and s["pit_cells"] == 2


def test_a_film_below_the_threshold_turns_a_descent_round():
    dem = [1, 2.0003, 2.0005, 2.0004, 1]
    basin, t, _, _ = run(dem, [0.5, 0, 0, 0, 0.5])
    assert basin == [[1, 1, 1, 2, 2]] and row(t, 0)[:3] == (2, 1, 2.0005)
    basin, t, s, _ = run(dem, [0.5, 0.0005, 0, 0, 0.5])          # 0.5 mm on the second cell: not a pond cell, but it stands higher
    assert basin == [[1, 1, 2, 2, 2]]
    assert row(t, 0) == (1, 1, 2.0003 + 0.0005, 1, 1, 1, 2) and row(t, 1) == (2, 1, 2.0005, 1, 1, 3, 5)
    # NaN and negative water fall to the DEM
    basin, _, _, _ = run(dem, [0.5, np.nan, 0, 0, 0.5])
    assert basin == [[1, 1, 1, 2, 2]]
    basin, _, _, _ = run(dem, [0.5, -3.0, 0, 0, 0.5])
    assert basin == [[1, 1, 1, 2, 2]]


def test_minus_zero_lies_below_plus_zero():
    basin, t, s, _ = run([0.0, -0.0, -5], [0, 0, 1])
    assert basin == [[1, 1, 1]] and s["pit_cells"] == 0 and row(t, 0)[:2] == (2, 1)
    assert t["head_level"][0] == 0 and not np.signbit(t["head_level"][0])
    basin, t, s, _ = run([-0.0, 0.0, 7], [0, 0, 0])
    assert basin == [[0, 0, 0]] and s == dict(slope_cells=3, pit_cells=1, unponded_cells=3, ponds=0)
    basin, t, s, _ = run([0.0, -0.0, 0.0], [0, 0, 0])
    assert s["pit_cells"] == 1


def test_nodata_walls():
    basin, t, s, raw = run([[9, 8, 7], [N, N, 6], [3, 4, 5]], [[0, 0, 0], [0, 0, 0], [0.5, 0, 0]])
    assert basin == [[1, 1, 1], [-1, -1, 1], [1, 1, 1]]          # round the wall: 9 8 6 4 and in
    assert row(t, 0) == (6, 1, 9.0, 1, 3, 1, 3) and s == dict(slope_cells=6, pit_cells=0, unponded_cells=0, ponds=1)
    assert descent_length(*raw) == 4
    basin, t, s, _ = run([5, N, 1], [0, 0, 0.5])                 # nothing with a level beside it: a pit
    assert basin == [[0, -1, 1]] and row(t, 0) == (0, 0, -INF, 1, 1, 3, 3)
    assert s == dict(slope_cells=1, pit_cells=1, unponded_cells=1, ponds=1)
    basin, _, _, _ = run([5, np.nan, 1], [0, 0, 0.5])            # a NaN elevation is a wall as well
    assert basin == [[0, -1, 1]]


def test_a_descent_over_corners_only():
    basin, t, s, _ = run([[9, 20, 20], [20, 8, 20], [20, 20, 7]], [[0, 0, 0], [0, 0, 0], [0, 0, 0.5]])
    assert basin == [[1] * 3] * 3
    assert row(t, 0) == (8, 3, 20.0, 1, 3, 1, 3)                # the corner's three neighbours enter the pond
    assert s == dict(slope_cells=8, pit_cells=0, unponded_cells=0, ponds=1)


def test_no_pond_and_all_pond():
    basin, t, s, _ = run([3, 2, 1], [0, 0, 0])
    assert basin == [[0, 0, 0]] and len(t) == 0 and s == dict(slope_cells=3, pit_cells=1, unponded_cells=3, ponds=0)
    basin, t, s, _ = run(np.full((2, 2), 4.0), np.ones((2, 2)))
    assert basin == [[1, 1], [1, 1]] and row(t, 0) == (0, 0, -INF, 1, 2, 1, 2)
    assert s == dict(slope_cells=0, pit_cells=0, unponded_cells=0, ponds=1)
