"""The host model of the pond outlets (tests/pond_outlets_model.py) against answers written by hand and against a plain double
loop: the model is the yardstick of the device tests, so it is held to the definitions of include/wdpm_pond_outlets.h here, case
by case.  The two statements the header makes about every call - pour_level >= rim_level, and the basin an outlet leads to spills
no higher - are asserted on every case and on random rasters."""
import numpy as np
import pytest

from helpers import pad
from pond_catchments_model import OFFSETS, catchments, levels
from pond_outlets_model import TooDeep, assert_invariants, outlets
from pond_rims_model import depth_from_key, device_dem, rims
from ponds_model import inventory

MISS = -99999.0
N = MISS
INF = np.inf
Q = 2 ** 24
NONE = (INF, -1, -1, -1, -1, -1, 0, 0, 0, 0)


def run(dem, w, min_depth=0.001):
    dem, w = np.atleast_2d(np.asarray(dem, dtype=np.float64)), np.atleast_2d(np.asarray(w, dtype=np.float64))
    bd, bw = pad(dem, w, MISS)
    labels, ponds = inventory(bd > MISS, bw, min_depth)
    ddem = device_dem(bd, MISS)
    basin, _, _ = catchments(labels, ddem, bw, ponds)
    table, stats = outlets(labels, ddem, bw, ponds)
    assert_invariants(table, rims(labels, ddem, bw, len(ponds)))
    return basin[1:-1, 1:-1].tolist(), table, stats


def row(table, k):
    """(pour_level, from_row, from_col, to_row, to_col, to_basin, reserved, divide_cells, fill_cells, fill_q), padded coordinates"""
    return tuple(table[k].tolist())


def test_two_ponds_that_are_each_others_outlet():
    basin, t, s = run([1, 2, 3, 2, 1], [0.5, 0, 0, 0, 0.5])
    assert basin == [[1, 1, 1, 2, 2]]
    # the only pair of the two basins is (3 m, 2 m): both spill at 3 m; 1.5 m and 2 m lie below it
    assert row(t, 0) == (3.0, 1, 3, 1, 4, 2, 0, 1, 2, int(2.5 * Q))
    assert row(t, 1) == (3.0, 1, 4, 1, 3, 1, 0, 1, 2, int(2.5 * Q))
    assert s == dict(ponds=2, no_outlet=0, to_land=0, divide_cells=2)


def test_a_chain_of_three():
    basin, t, s = run([1, 5, 2, 6, 3], [0.5, 0, 0.5, 0, 0.5])
    assert basin == [[1, 1, 2, 2, 3]]
    assert row(t, 0) == (5.0, 1, 2, 1, 3, 2, 0, 1, 1, int(3.5 * Q))
    assert row(t, 1) == (5.0, 1, 3, 1, 2, 1, 0, 2, 1, int(2.5 * Q))       # its other pass, over 6 m into pond 3, is higher
    assert row(t, 2) == (6.0, 1, 5, 1, 4, 2, 0, 1, 1, int(2.5 * Q))       # a pond cell as `from`
    assert s == dict(ponds=3, no_outlet=0, to_land=0, divide_cells=4)


def test_an_outlet_onto_land_that_ends_in_a_pit():
    basin, t, s = run([1, 2, 3, 2.5, 2.75], [0.5, 0, 0, 0, 0])
    assert basin == [[1, 1, 1, 0, 0]]
    assert row(t, 0) == (3.0, 1, 3, 1, 4, 0, 0, 1, 2, int(2.5 * Q))
    assert s == dict(ponds=1, no_outlet=0, to_land=1, divide_cells=1)


def test_a_pond_at_its_pour_level_fills_nothing():
    basin, t, s = run([1, 2, 1], [1, 0, 1])
    assert basin == [[1, 0, 2]]                                           # the middle cell has no lower neighbour: a pit
    assert row(t, 0) == (2.0, 1, 1, 1, 2, 0, 0, 1, 0, 0) and row(t, 1) == (2.0, 1, 3, 1, 2, 0, 0, 1, 0, 0)
    assert s == dict(ponds=2, no_outlet=0, to_land=2, divide_cells=2)


def test_ties_go_to_the_smallest_from_and_then_to_neighbour_order():
    basin, t, s = run([[1, 3, 1], [1, 3, 1]], [[0.5, 0, 0.5], [0.5, 0, 0.5]])
    assert basin == [[1, 1, 2], [1, 1, 2]]
    # four pairs at 3 m either way.  Pond 1: from (1, 2), whose right neighbour comes before its down-right one
    assert row(t, 0) == (3.0, 1, 2, 1, 3, 2, 0, 2, 2, 3 * Q)
    # pond 2: from (1, 3), whose left neighbour comes before its down-left one
    assert row(t, 1) == (3.0, 1, 3, 1, 2, 1, 0, 2, 2, 3 * Q)
    # a lower pair further down the raster wins over an earlier, higher one: (2, 2)'s pairs stand at 2.5 m, up-right before right
    basin, t, _ = run([[1, 3, 1], [1, 2.5, 1]], [[0.5, 0, 0.5], [0.5, 0, 0.5]])
    assert basin == [[1, 1, 2], [1, 1, 2]]
    assert row(t, 0)[:6] == (2.5, 2, 2, 1, 3, 2) and row(t, 0)[7:] == (2, 2, 2 * Q)
    # with a lower pond on the right the middle column drains there: pond cells as `from`, (1, 1) before (2, 1); (2, 2) looks up-left
    # before left
    basin, t, _ = run([[1, 3, 1], [1, 2.5, 1]], [[0.5, 0, 0.25], [0.5, 0, 0.25]])
    assert basin == [[1, 2, 2], [1, 2, 2]]
    assert row(t, 0)[:6] == (2.5, 1, 1, 2, 2, 2) and row(t, 1)[:6] == (2.5, 2, 2, 1, 1, 1)


def test_signed_zeros():
    basin, t, s = run([-1, -0.0, 0.0, -1], [0.5, 0, 0, 0.5])
    assert basin == [[1, 1, 2, 2]]
    assert t["pour_level"][0] == 0 and not np.signbit(t["pour_level"][0]) and not np.signbit(t["pour_level"][1])
    assert row(t, 0)[1:] == (1, 2, 1, 3, 2, 0, 1, 2, Q // 2)              # -0.5 and -0.0 lie below +0.0; the latter adds nothing
    assert row(t, 1)[1:] == (1, 3, 1, 2, 1, 0, 1, 1, Q // 2)              # +0.0 is not below itself
    basin, t, s = run([-1, 0.0, -0.0, -1], [0.5, 0, 0, 0.5])
    assert basin == [[1, 1, 2, 2]] and not np.signbit(t["pour_level"]).any()


def test_no_outlet():
    basin, t, s = run([5, 4, 3, 2, 1], [0, 0, 0, 0, 0.5])                # one basin over everything
    assert basin == [[1] * 5] and row(t, 0) == NONE and s == dict(ponds=1, no_outlet=1, to_land=0, divide_cells=0)
    basin, t, s = run([5, N, 1], [0, 0, 0.5])                             # walled in by NODATA and the border
    assert basin == [[0, -1, 1]] and row(t, 0) == NONE
    basin, t, s = run([1, N, 1], [0.5, 0, 0.5])                           # a NODATA ridge is no pass
    assert row(t, 0) == NONE and row(t, 1) == NONE and s == dict(ponds=2, no_outlet=2, to_land=0, divide_cells=0)
    basin, t, s = run([1, np.nan, 1], [0.5, 0, 0.5])                      # nor is a NaN elevation
    assert row(t, 0) == NONE and row(t, 1) == NONE
    basin, t, s = run([3, 2, 1], [0, 0, 0])                               # no pond, no row
    assert len(t) == 0 and s == dict(ponds=0, no_outlet=0, to_land=0, divide_cells=0)


def test_a_bowl_computed_by_hand():
    """a 5 x 5 bowl around one pond cell beside a plain that ends in a pit: rings at 2 and 3 m, the pass in the outer ring's one notch"""
    dem = np.full((5, 8), 9.0)
    y, x = np.mgrid[0:5, 0:5]
    dem[:, :5] = np.maximum(abs(y - 2), abs(x - 2)) + 1.0
    dem[2, 2] = 0.0
    dem[2, 4] = 2.5                     # the notch in the outer ring
    dem[:, 5:] = [2.25, 2.0, 1.75]      # the plain falls away from the bowl; its last column is all pits
    water = np.zeros((5, 8))
    water[2, 2] = 0.5
    basin, t, s = run(dem, water)
    assert [r[:5] for r in basin] == [[1] * 5] * 5 and all(v == 0 for r in basin for v in r[5:])
    # pairs across columns 5 | 6 (padded): the notch at 2.5 m is the lowest `from`, its up-right neighbour the first `to`
    assert row(t, 0)[:7] == (2.5, 3, 5, 2, 6, 0, 0)
    assert t["divide_cells"][0] == 5
    # below 2.5 m: the pond's surface at 0.5 m and the eight cells of the inner ring at 2 m
    assert t["fill_cells"][0] == 9 and t["fill_q"][0] == int((2.0 + 8 * 0.5) * Q)


def test_films_and_nan_water_count_like_the_catchments_levels():
    basin, t, _ = run([1, 2, 3, 2, 1], [0.5, 0.0005, np.nan, -3.0, 0.5])
    assert basin == [[1, 1, 2, 2, 2]]                                     # the film lifts its cell above the one beyond the ridge
    assert t["pour_level"][0] == 3.0 and t["fill_cells"][0] == 2
    assert t["fill_q"][0] == int(np.rint((3.0 - 1.5) * Q)) + int(np.rint((3.0 - (2 + 0.0005)) * Q))


def test_rint_rounds_half_to_even():
    half = 0.5 / Q
    for k, want in ((1, 0), (3, 2), (5, 2)):                             # 0.5, 1.5, 2.5 quanta below the outlet
        _, t, _ = run([0, 2 - k * half, 2, 1, 0], [0.5, 0, 0, 0, 0.5])
        assert t["pour_level"][0] == 2.0 and t["fill_cells"][0] == 2 and t["fill_q"][0] == int(1.5 * Q) + want, (k, t[0])


def test_a_600_m_pit_fails():
    with pytest.raises(TooDeep):
        run([0, 600, 1], [0.5, 0, 0])
    _, t, _ = run([0, 500, 1], [0.5, 0, 0])
    assert t["fill_q"][0] == int(499.5 * Q)
    with pytest.raises(TooDeep):                                          # exactly 512 m
        run([0, 512.5, 1], [0.5, 0, 0])


# ---- the model against a plain double loop, and the invariants, on random rasters ---------------------------------------------------
def plain(basin, key, n):
    rows, ncp = basin.shape
    best = [None] * n
    divide = [0] * n
    for r in range(rows):
        for c in range(ncp):
            k = basin[r, c]
            if k <= 0:
                continue
            on = False
            for i, (dr, dc) in enumerate(OFFSETS):
                rr, cc = r + dr, c + dc
                if not (0 <= rr < rows and 0 <= cc < ncp) or basin[rr, cc] < 0 or basin[rr, cc] == k:
                    continue
                on = True
                cand = (int(max(key[r, c], key[rr, cc])), r * ncp + c, i, rr, cc)
                if best[k - 1] is None or cand[:3] < best[k - 1][:3]:
                    best[k - 1] = cand
            divide[k - 1] += on
    return best, divide


@pytest.mark.parametrize("seed", range(6))
def test_random_rasters(seed):
    rng = np.random.default_rng(seed)
    R, Cc = 9 + seed, 14 - seed
    dem = np.round(rng.random((R, Cc)) * 3, 1 if seed % 2 else 2) + 10.0
    dem[rng.random((R, Cc)) < 0.08] = MISS
    water = np.where(rng.random((R, Cc)) < 0.25, 0.05 + rng.random((R, Cc)), 0.0)
    water[rng.random((R, Cc)) < 0.05] = 0.0005
    bd, bw = pad(dem, water, MISS)
    labels, ponds = inventory(bd > MISS, bw, 0.001)
    ddem = device_dem(bd, MISS)
    basin, _, _ = catchments(labels, ddem, bw, ponds)
    table, stats = outlets(labels, ddem, bw, ponds)
    n = len(ponds)
    assert n >= 2
    assert_invariants(table, rims(labels, ddem, bw, n))
    _, key = levels(labels, ddem, bw)
    best, divide = plain(basin, key, n)
    for k in range(n):
        if best[k] is None:
            assert row(table, k) == NONE
            continue
        h, a, _, rr, cc = best[k]
        pour = float(depth_from_key(np.uint64(h)))
        assert row(table, k)[:8] == (pour, a // bd.shape[1], a % bd.shape[1], rr, cc, basin[rr, cc], 0, divide[k])
        mine = (basin == k + 1) & (key < np.uint64(h))
        lv = depth_from_key(key[mine])
        assert table["fill_cells"][k] == int(mine.sum()) and table["fill_q"][k] == sum(int(np.rint((pour - v) * Q)) for v in lv.tolist())
    assert stats["no_outlet"] == sum(b is None for b in best) and stats["divide_cells"] == sum(divide)
