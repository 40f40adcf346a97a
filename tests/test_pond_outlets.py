"""The pond outlets on the device (include/wdpm_pond_outlets.h, wdpm_amd/csrc/wdpm_pond_outlets.hip) against the host model
(tests/pond_outlets_model.py, itself held against hand-written answers and a plain double loop in tests/test_pond_outlets_model.py).

Every case compares the WHOLE outlet table and the counts for equality - integers by value, doubles by bit pattern; the definitions
are exact, there is no tolerance; holds labels, pond table, rim table, basin raster and catchment table of the same call, bit for
bit, against a label_catchments() of a twin context; asserts the two statements the header makes about every call (pour_level >=
rim_level; the basin an outlet leads to spills no higher); and asserts that no guard byte around the handle's buffers changed.
Shapes are file cells: 46 x 70 is two segments, 67 x 193 one block row of four, 131 x 385 seven segments over two blocks; a wave
owns a 64-column segment, so padded column 63 is lane 63 and padded column 64 lane 0 of the next.
"""
import numpy as np
import pytest

from helpers import find_drain, n_bit_diff, pad, rough_dem
from pond_catchments_model import catchments
from pond_outlets_model import TooDeep, assert_invariants, assert_same_outlets, outlets
from pond_rims_model import device_dem
from ponds_model import inventory

pytestmark = pytest.mark.gpu
MISS = -99999.0
WET = 0.001
THRES = 0.005 / 1000
SHAPES = [(46, 70), (67, 193), (131, 385)]
Q = 2 ** 24
NONE = (np.inf, -1, -1, -1, -1, -1, 0, 0, 0, 0)
DIRECTIONS = [(-1, -1), (-1, 0), (-1, 1), (0, -1), (0, 1), (1, -1), (1, 0), (1, 1)]


def lesser(p):
    """what a label_catchments() leaves as well"""
    return p.labels(), p.table(), p.rims(), p.basins(), p.catchments()


def hold_against_model(bd, miss, water, md, p, n):
    """the outlet table and its counts of handle p against the model of the same water; returns (table, stats, basins)"""
    table, stats, basins = p.outlets(), p.outlet_stats(), p.basins()
    ref_labels, ref_ponds = inventory(bd > miss, water, md)
    assert n == len(ref_ponds) == stats["ponds"] == len(table)
    dem = device_dem(bd, miss)
    ref_basin, _, _ = catchments(ref_labels, dem, water, ref_ponds)
    assert (basins == ref_basin).all()
    assert_same_outlets(table, stats, *outlets(ref_labels, dem, water, ref_ponds, basin=ref_basin))
    assert_invariants(table, p.rims())
    return table, stats, basins


def outlets_on_device(hip, bd, bw, thresholds=(WET,), rows_per_wave=None):
    """Upload padded rasters, label with outlets at each threshold on ONE handle, hold the outlet table against the model and
    everything else the call leaves against the label_catchments() of a twin context.  Returns what the last threshold left."""
    from wdpm_amd.ponds import OUTLET_DTYPE, Ponds
    R, Cc = bd.shape[0] - 2, bd.shape[1] - 2
    kw = dict(module="add", nrows=R, ncols=Cc, missingvalue=MISS)
    with hip.context(**kw) as ctx, hip.context(**kw) as twin:
        ctx.upload(bd, bw)
        twin.upload(bd, bw)
        with Ponds(ctx) as p, Ponds(twin) as q:
            for md in thresholds:
                n = p.label_outlets(md)
                assert p.outlets().dtype == OUTLET_DTYPE
                got = hold_against_model(bd, MISS, ctx.download_water(), md, p, n)
                assert q.label_catchments(md) == n
                for mine, theirs in zip(lesser(p), lesser(q)):
                    assert mine.tobytes() == theirs.tobytes()
                assert p.catchment_stats() == q.catchment_stats()
                if rows_per_wave is not None:
                    assert p.stats()["rows_per_wave"] == rows_per_wave, p.stats()
            assert p.guard_bad() == 0
    return got


def check(hip, dem, water, **kw):
    return outlets_on_device(hip, *pad(np.atleast_2d(np.asarray(dem, dtype=np.float64)), np.atleast_2d(np.asarray(water, dtype=np.float64)),
                                       MISS), **kw)


def row(table, k):
    return tuple(table[k].tolist())


def grid(R, Cc):
    """padded row and column of every file cell"""
    return np.mgrid[1:R + 1, 1:Cc + 1]


# ---- pair geometry -------------------------------------------------------------------------------------------------------------------
def lines_scene(R, Cc, dr, dc, seed=0):
    """A rough plateau near 1000 m that holds short lines of low cells along direction (dr, dc), far from each other, each with one
    pair (a, b) that is by far the lowest pass of both its ponds:
        kind 0:  pond (1.5 m) | a (3 m, drains back) | b (2.5 m, drains on) | pond (1.5 m)      a is a cell of the catchment
        kind 1:  a (a pond cell, surface 3 m) | b (2.5 m) | pond (1.5 m)                        a is a pond cell
    with a on lane 63 and b on lane 0 of the next segment or the other way round (straight and diagonal), a on both sides of a seam
    for the directions along it, and a on padded column 1 / ncp - 2 and padded row 1 / rows - 2.  Returns the file rasters and the
    pairs as padded (a row, a col, b row, b col)."""
    rng = np.random.default_rng(seed + 100 + 17 * (3 * dr + dc))
    dem = 1000.0 + np.round(rng.random((R, Cc)) * 8) / 4
    water = np.zeros((R, Cc))
    ncp = Cc + 2
    want = []                                # (padded a row, padded a col, kind)
    rows = iter(range(6, R - 6, 6))
    for i, seam in enumerate(range(64, ncp, 64)):
        for ac in ([seam - 1] if dc > 0 else [seam] if dc < 0 else [seam - 1, seam]):
            ar = next(rows, None)
            if ar is not None:
                want.append((ar, ac, i % 2))
    ar = next(rows, None)
    if ar is not None:
        want.append((ar, 1 if dc >= 0 else Cc, 1))                     # padded column 1 or ncp - 2
    want.append((1 if dr >= 0 else R, 20 if dc >= 0 else 30, 1))       # padded row 1 or rows - 2
    pairs = []
    for ar, ac, kind in want:
        cells = [(ar + k * dr, ac + k * dc) for k in ((-1, 0, 1, 2) if kind == 0 else (0, 1, 2))]
        if not all(1 <= r <= R and 1 <= c <= Cc for r, c in cells):
            continue
        levels = ((1.0, 0.5), (3.0, 0.0), (2.5, 0.0), (1.0, 0.5)) if kind == 0 else ((2.5, 0.5), (2.5, 0.0), (1.0, 0.5))
        for (r, c), (e, d) in zip(cells, levels):
            dem[r - 1, c - 1], water[r - 1, c - 1] = e, d
        pairs.append((ar, ac, ar + dr, ac + dc))
    return dem, water, pairs


def check_lines(hip, R, Cc, dr, dc, **kw):
    dem, water, pairs = lines_scene(R, Cc, dr, dc)
    table, stats, basins = check(hip, dem, water, **kw)
    assert len(pairs) >= 3
    for ar, ac, br, bc in pairs:
        k, j = basins[ar, ac], basins[br, bc]
        assert k > 0 and j > 0 and k != j
        assert row(table, k - 1)[:6] == (3.0, ar, ac, br, bc, j) and row(table, j - 1)[:6] == (3.0, br, bc, ar, ac, k)
    return pairs


@pytest.mark.parametrize("R,Cc", SHAPES)
@pytest.mark.parametrize("dr,dc", DIRECTIONS)
def test_outlet_pairs_in_the_eight_directions(hip, R, Cc, dr, dc):
    pairs = check_lines(hip, R, Cc, dr, dc)
    cols = {(ac, bc) for _, ac, _, bc in pairs}
    if dc > 0:
        assert (63, 64) in cols and any(ac == 1 for ac, _ in cols)
    if dc < 0:
        assert (64, 63) in cols and any(ac == Cc for ac, _ in cols)
    assert any(ar == (1 if dr >= 0 else R) for ar, _, _, _ in pairs)


@pytest.mark.parametrize("rpw", [1, 2, 3, 64])
@pytest.mark.parametrize("dr,dc", [(-1, -1), (-1, 0), (-1, 1), (1, -1), (1, 0), (1, 1)])
def test_pairs_across_strip_seams(hip, monkeypatch, dr, dc, rpw):
    """the same lines with every row, every second and every third row the first of a strip; 64 rows: one strip and a short one"""
    monkeypatch.setenv("WDPM_PONDS_ROWS_PER_WAVE", str(rpw))
    check_lines(hip, 67, 193, dr, dc, rows_per_wave=rpw)


# ---- what a and b are, ties, no outlet, the fill: the hand-written answers of tests/test_pond_outlets_model.py ------------------------
def test_two_ponds_that_are_each_others_outlet(hip):
    t, s, _ = check(hip, [1, 2, 3, 2, 1], [0.5, 0, 0, 0, 0.5])
    assert row(t, 0) == (3.0, 1, 3, 1, 4, 2, 0, 1, 2, int(2.5 * Q)) and row(t, 1) == (3.0, 1, 4, 1, 3, 1, 0, 1, 2, int(2.5 * Q))
    assert s == dict(ponds=2, no_outlet=0, to_land=0, divide_cells=2)


def test_a_chain_of_three(hip):
    t, s, _ = check(hip, [1, 5, 2, 6, 3], [0.5, 0, 0.5, 0, 0.5])
    assert row(t, 0) == (5.0, 1, 2, 1, 3, 2, 0, 1, 1, int(3.5 * Q))
    assert row(t, 1) == (5.0, 1, 3, 1, 2, 1, 0, 2, 1, int(2.5 * Q))
    assert row(t, 2) == (6.0, 1, 5, 1, 4, 2, 0, 1, 1, int(2.5 * Q))       # a pond cell as `from`


def test_a_pond_cell_of_another_basin_as_to(hip):
    """the ridge cell drains to the lower pond on its right: pond 1 spills from a pond cell, pond 2 into one"""
    t, s, basins = check(hip, [1, 3, 1], [0.5, 0, 0.25])
    assert basins[1, 1:-1].tolist() == [1, 2, 2]
    assert row(t, 0) == (3.0, 1, 1, 1, 2, 2, 0, 1, 1, int(1.5 * Q)) and row(t, 1) == (3.0, 1, 2, 1, 1, 1, 0, 1, 1, int(1.75 * Q))


def test_an_outlet_onto_land_that_ends_in_a_pit(hip):
    t, s, _ = check(hip, [1, 2, 3, 2.5, 2.75], [0.5, 0, 0, 0, 0])
    assert row(t, 0) == (3.0, 1, 3, 1, 4, 0, 0, 1, 2, int(2.5 * Q)) and s == dict(ponds=1, no_outlet=0, to_land=1, divide_cells=1)


def test_a_pond_at_its_pour_level_fills_nothing(hip):
    t, s, _ = check(hip, [1, 2, 1], [1, 0, 1])
    assert row(t, 0) == (2.0, 1, 1, 1, 2, 0, 0, 1, 0, 0) and row(t, 1) == (2.0, 1, 3, 1, 2, 0, 0, 1, 0, 0)


def test_ties(hip):
    t, _, _ = check(hip, [[1, 3, 1], [1, 3, 1]], [[0.5, 0, 0.5], [0.5, 0, 0.5]])
    assert row(t, 0) == (3.0, 1, 2, 1, 3, 2, 0, 2, 2, 3 * Q)              # the smallest `from`, then right before down-right
    assert row(t, 1) == (3.0, 1, 3, 1, 2, 1, 0, 2, 2, 3 * Q)              # left before down-left
    t, _, _ = check(hip, [[1, 3, 1], [1, 2.5, 1]], [[0.5, 0, 0.25], [0.5, 0, 0.25]])
    assert row(t, 0)[:6] == (2.5, 1, 1, 2, 2, 2) and row(t, 1)[:6] == (2.5, 2, 2, 1, 1, 1)


@pytest.mark.parametrize("R,Cc", SHAPES)
def test_ties_everywhere(hip, R, Cc):
    """two levels only and a pond in every sixth cell: every divide is a run of equal heights across lanes, seams and strips"""
    rng = np.random.default_rng(R)
    dem = np.where(rng.random((R, Cc)) < 0.5, 7.0, 7.25)
    water = np.where(rng.random((R, Cc)) < 0.16, 0.125, 0.0)
    dem[water > 0] = 6.0
    t, s, _ = check(hip, dem, water)
    assert len(t) > 20 and s["divide_cells"] > len(t) and set(np.unique(t["pour_level"][t["from_row"] >= 0])) <= {6.125, 7.0, 7.25}


def test_signed_zeros(hip):
    t, _, _ = check(hip, [-1, -0.0, 0.0, -1], [0.5, 0, 0, 0.5])
    assert t["pour_level"][0] == 0 and not np.signbit(t["pour_level"]).any()
    assert row(t, 0)[1:] == (1, 2, 1, 3, 2, 0, 1, 2, Q // 2) and row(t, 1)[1:] == (1, 3, 1, 2, 1, 0, 1, 1, Q // 2)
    rng = np.random.default_rng(3)
    dem = np.where(rng.random((46, 70)) < 0.5, 0.0, -0.0)
    water = np.where(rng.random((46, 70)) < 0.05, 0.4, 0.0)
    dem[water > 0] = -5.0
    t, _, _ = check(hip, dem, water)
    has = t["from_row"] >= 0
    assert has.sum() > 5 and (t["pour_level"][has] == 0).all() and np.signbit(t["pour_level"][has]).any()


def bowl(R, Cc):
    r, c = grid(R, Cc)
    d2 = (r - R // 2) ** 2 + (c - Cc // 2) ** 2
    return 50.0 + d2 / 64.0, np.where(d2 <= 9, 0.01, 0.0)


@pytest.mark.parametrize("R,Cc", SHAPES)
def test_no_outlet(hip, monkeypatch, R, Cc):
    monkeypatch.setenv("WDPM_PONDS_ROWS_PER_WAVE", "16")
    t, s, basins = check(hip, *bowl(R, Cc), rows_per_wave=16)             # one basin over everything
    assert (basins[1:-1, 1:-1] == 1).all() and row(t, 0) == NONE and s == dict(ponds=1, no_outlet=1, to_land=0, divide_cells=0)
    # two bowls with a NODATA ridge between them, each walled in by it and the border
    dem, water = bowl(R, Cc)
    r, c = grid(R, Cc)
    wall = Cc // 3
    d2 = (r - R // 2) ** 2 + (c - 5) ** 2
    dem = np.where(c < wall, 50.0 + d2 / 64.0, dem)
    water = np.where(c < wall, np.where(d2 <= 2, 0.01, 0.0), water)
    dem[:, wall - 1] = MISS
    t, s, basins = check(hip, dem, water, rows_per_wave=16)
    assert len(t) == 2 and row(t, 0) == NONE and row(t, 1) == NONE and s["no_outlet"] == 2 and set(np.unique(basins)) == {-1, 1, 2}
    t, s, _ = check(hip, dem, np.zeros((R, Cc)))                          # no pond at all: an empty table
    assert len(t) == 0 and s == dict(ponds=0, no_outlet=0, to_land=0, divide_cells=0)


def hand_bowl():
    dem = np.full((5, 8), 9.0)
    y, x = np.mgrid[0:5, 0:5]
    dem[:, :5] = np.maximum(abs(y - 2), abs(x - 2)) + 1.0
    dem[2, 2] = 0.0
    dem[2, 4] = 2.5
    dem[:, 5:] = [2.25, 2.0, 1.75]
    water = np.zeros((5, 8))
    water[2, 2] = 0.5
    return dem, water


def test_a_bowl_computed_by_hand(hip):
    t, s, _ = check(hip, *hand_bowl())
    assert row(t, 0) == (2.5, 3, 5, 2, 6, 0, 0, 5, 9, int((2.0 + 8 * 0.5) * Q))


@pytest.mark.parametrize("R,Cc", SHAPES)
def test_films_and_nan_water_in_the_basins(hip, R, Cc):
    rng = np.random.default_rng(R)
    dem = rough_dem(R, Cc, R, step=0.25)
    water = np.where(dem < np.quantile(dem, 0.2), 0.3, 0.0)
    film = (water == 0) & (rng.random((R, Cc)) < 0.3)
    water[film] = rng.random(int(film.sum())) * WET            # at most the threshold: slope cells at WET, pond cells at 0
    water[rng.random((R, Cc)) < 0.01] = np.nan
    water[rng.random((R, Cc)) < 0.01] = -0.5
    t, s, _ = check(hip, dem, water, thresholds=(WET, 0.0))
    assert len(t) > 3 and int(t["fill_cells"].sum()) > 0


def test_a_600_m_pit_fails_and_the_handle_stays_usable(hip):
    import wdpm_amd
    from wdpm_amd.ponds import Ponds
    R, Cc = 46, 70
    dem, water = lines_scene(R, Cc, 0, 1)[:2]
    ok_d, ok_w = pad(dem, water, MISS)
    deep = dem.copy()
    deep[30, 40:44] = [0.0, 600.0, 1.0, 700.0]                  # a pond 600 m below the only way out of its walls
    deep[29, 39:45] = deep[31, 39:45] = 700.0
    deep[30, 39] = 700.0
    pit_w = water.copy()
    pit_w[30, 40] = 0.5
    bd, bw = pad(deep, pit_w, MISS)
    labels, ponds = inventory(bd > MISS, bw, WET)
    with pytest.raises(TooDeep):
        outlets(labels, device_dem(bd, MISS), bw, ponds)
    with hip.context(module="add", nrows=R, ncols=Cc, missingvalue=MISS) as ctx:
        ctx.upload(bd, bw)
        with Ponds(ctx) as p:
            with pytest.raises(wdpm_amd.WdpmError, match="wdpm_outlets_label.*512 m"):
                p.label_outlets(WET)
            p.n = len(ponds)
            for ask in (p.outlets, p.outlet_stats):
                with pytest.raises(wdpm_amd.WdpmError, match="no outlet table"):
                    ask()
            with pytest.raises(wdpm_amd.WdpmError):
                p.table()
            n = p.label_catchments(WET)                          # the lesser call has nothing to say about depths below outlets
            assert n == len(ponds) and len(p.catchments()) == n
            ctx.upload(ok_d, ok_w)                               # and the handle labels another water as if nothing had happened
            n = p.label_outlets(WET)
            hold_against_model(ok_d, MISS, ok_w, WET, p, n)
            assert p.guard_bad() == 0


# ---- rows that are skipped -----------------------------------------------------------------------------------------------------------
def ramp(R, Cc):
    """a plane that falls towards the last column, whose last two columns are one pond: one basin, every row skipped"""
    r, c = grid(R, Cc)
    return 1000.0 - 0.5 * c, np.where(c >= Cc - 1, 0.25, 0.0)


@pytest.mark.parametrize("R,Cc", SHAPES)
def test_rows_without_a_pass(hip, R, Cc):
    t, s, basins = check(hip, rough_dem(R, Cc, 1), np.full((R, Cc), 0.5))          # the settled all-wet raster
    assert row(t, 0) == NONE and len(t) == 1
    t, s, basins = check(hip, *ramp(R, Cc))
    assert row(t, 0) == NONE and (basins[1:-1, 1:-1] == 1).all()


@pytest.mark.parametrize("col", [63, 64, 126, 127, 128, 129], ids=lambda c: "col%d" % c)
@pytest.mark.parametrize("wet", [False, True], ids=["ramp", "wet"])
def test_one_foreign_cell_stops_the_skip(hip, wet, col):
    """One dry pit cell (basin 0) in an otherwise single basin, at padded column `col` of 67 x 193: lane 63, lane 0, and either side
    of the next seam - where it lies in the segment, or is the cell beside it.  The rows around it hold the raster's only passes.
    In the all-wet raster the pit is one foreign cell among pond cells; on the ramp the few cells just up the slope drain into it."""
    R, Cc = 67, 193
    dem, water = ramp(R, Cc) if not wet else (np.full((R, Cc), 100.0), np.full((R, Cc), 0.5))
    ar = 32
    dem[ar - 1, col - 1] -= 2.0                                  # lower than all around it, and dry
    water[ar - 1, col - 1] = 0.0
    t, s, basins = check(hip, dem, water)
    assert basins[ar, col] == 0 and len(t) == 1 and t["to_basin"][0] == 0 and s["divide_cells"] >= 8
    if wet:
        assert (basins[1:-1, 1:-1] == 1).sum() == R * Cc - 1
        assert row(t, 0) == (100.5, ar - 1, col - 1, ar, col, 0, 0, 8, 0, 0)


# ---- noise, thin rasters ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("density", [0.30, 0.41, 0.60])
def test_noise(hip, density):
    """water at three densities on rough ground, 3 % NODATA with water on it, at two thresholds on one handle"""
    R, Cc = 131, 385
    rng = np.random.default_rng(int(density * 100))
    dem = rough_dem(R, Cc, int(density * 100))
    depth = 0.002 + rng.random((R, Cc)) * 0.02
    depth[rng.random((R, Cc)) < 0.10] = 3.0
    water = np.where(rng.random((R, Cc)) < density, depth, 0.0)
    dem[rng.random((R, Cc)) < 0.03] = MISS
    t, s, _ = check(hip, dem, water, thresholds=(WET, 0.01))
    assert len(t) > 10 and s["divide_cells"] > 0 and s["no_outlet"] < len(t)


def noise_case():
    rng = np.random.default_rng(8)
    dem = rough_dem(131, 385, 8, step=0.125)
    water = np.where(rng.random((131, 385)) < 0.41, 0.002 + rng.random((131, 385)), 0.0)
    dem[rng.random((131, 385)) < 0.03] = MISS
    return dem, water


@pytest.mark.parametrize("rpw", [1, 2, 3, 64])
def test_noise_with_rows_per_wave_forced(hip, monkeypatch, rpw):
    monkeypatch.setenv("WDPM_PONDS_ROWS_PER_WAVE", str(rpw))
    check(hip, *noise_case(), rows_per_wave=rpw)


@pytest.mark.parametrize("R,Cc", [(1, 1), (131, 1), (3, 700), (1, 200)])
def test_thin_rasters(hip, R, Cc):
    rng = np.random.default_rng(R * Cc)
    dem = rough_dem(R, Cc, R + Cc, step=0.25)
    t, s, _ = check(hip, dem, np.zeros((R, Cc)))                                    # no pond
    assert len(t) == 0
    t, s, _ = check(hip, dem, np.full((R, Cc), 0.5))                                # all pond
    assert len(t) == 1 and row(t, 0) == NONE
    if R * Cc > 1:
        t, s, _ = check(hip, dem, np.where(rng.random((R, Cc)) < 0.3, 0.3, 0.0), thresholds=(WET, 0.25))


# ---- the handle -----------------------------------------------------------------------------------------------------------------------
def test_handle_state(hip):
    import wdpm_amd
    from wdpm_amd.ponds import OUTLET_DTYPE, Ponds, bind
    R, Cc = 46, 70
    dem = rough_dem(R, Cc, 5)
    water = np.where(np.random.default_rng(5).random((R, Cc)) < 0.3, 0.3, 0.0)
    bd, bw = pad(dem, water, MISS)
    dll = bind(hip)
    with hip.context(module="add", nrows=R, ncols=Cc, missingvalue=MISS) as ctx:
        ctx.upload(bd, bw)
        with Ponds(ctx) as p:
            with pytest.raises(wdpm_amd.WdpmError, match="label_outlets\\(\\) has not succeeded"):
                p.outlets()
            with pytest.raises(wdpm_amd.WdpmError, match="no outlet table"):            # nothing labelled yet
                p.n = 0
                p.outlets(capacity=10)
            n = p.label_outlets(WET)
            want, stats, _ = hold_against_model(bd, MISS, bw, WET, p, n)
            assert n >= 4
            for name, call in (("label", p.label), ("label_rims", p.label_rims), ("label_catchments", p.label_catchments)):
                assert call(WET) == n                                                   # each lesser label call takes the table away
                for ask in (p.outlets, p.outlet_stats):
                    with pytest.raises(wdpm_amd.WdpmError, match="no outlet table"):
                        ask()
                assert p.label_outlets(WET) == n and p.outlets().tobytes() == want.tobytes() and p.outlet_stats() == stats
            buf = np.full(n * OUTLET_DTYPE.itemsize, 0xAB, dtype=np.uint8)
            assert dll.wdpm_outlets_table(p._h, buf.ctypes.data, n - 1) != 0            # one too small: fails ...
            assert b"capacity" in dll.wdpm_last_error() and b"wdpm_outlets_table" in dll.wdpm_last_error()
            assert (buf == 0xAB).all()                                                  # ... and writes nothing
            assert dll.wdpm_outlets_table(p._h, buf.ctypes.data, n) == 0
            assert buf.tobytes() == want.tobytes() and p.outlets(capacity=n + 7).tobytes() == want.tobytes()
            with pytest.raises(wdpm_amd.WdpmError, match="wdpm_outlets_label"):
                p.label_outlets(float("nan"))
            with pytest.raises(wdpm_amd.WdpmError, match="wdpm_outlets_label"):
                p.label_outlets(-1.0)
            with pytest.raises(wdpm_amd.WdpmError, match="records no events"):
                p.outlet_phase_ms()
            assert p.label_outlets(5.0) == 0                                            # no pond at this threshold: an empty table
            assert len(p.outlets()) == 0 and p.outlet_stats() == dict(ponds=0, no_outlet=0, to_land=0, divide_cells=0)
            assert p.label_outlets(WET) == n and p.outlets().tobytes() == want.tobytes()
            ctx.run_block(1, THRES)                                                     # the water moves on: a label call of the new
            assert p.label(WET) >= 0                                                    # water leaves no outlet table either
            with pytest.raises(wdpm_amd.WdpmError, match="no outlet table"):
                p.outlets()
            n2 = p.label_outlets(WET)
            hold_against_model(bd, MISS, ctx.download_water(), WET, p, n2)
            assert p.guard_bad() == 0


def test_phase_times(hip, monkeypatch):
    from wdpm_amd.ponds import OUTLET_PHASES, Ponds
    monkeypatch.setenv("WDPM_PONDS_TIMING", "1")
    dem, water = noise_case()
    bd, bw = pad(dem, water, MISS)
    with hip.context(module="add", nrows=131, ncols=385, missingvalue=MISS) as ctx:
        ctx.upload(bd, bw)
        with Ponds(ctx) as p:
            p.label_outlets(WET)
            ms = p.outlet_phase_ms()
            assert tuple(ms) == OUTLET_PHASES == ("passes", "locate") and all(0 < v < 1000 for v in ms.values()), ms
            assert set(p.catchment_phase_ms()) == {"receivers", "jump", "tally"} and len(p.phase_ms()) == 6


# ---- real water, and the context is left as it was ------------------------------------------------------------------------------------
def real_case(hip, module):
    dem = hip.synth_dem(385, 131)[:131, :385].copy()
    dem[40:60, 100:140] = MISS
    bd, _ = pad(dem, np.zeros_like(dem), MISS)
    bw = np.where(bd > MISS, 0.1, 0.0)
    kw = dict(module=module, nrows=131, ncols=385, missingvalue=MISS)
    if module == "drain":
        dr, dc = find_drain(bd)
        kw.update(drainrow=dr, draincol=dc)
    return bd, bw, kw


@pytest.mark.parametrize("module", ["add", "drain"])
def test_real_water_and_state_neutrality(hip, module):
    """Two blocks of real iterations; outlets (the owed drain() of the drain module applied by the call) against the model; a third
    block with another outlet call between begin_block and its first iteration.  The third block is, bit for bit, what a twin
    context computes that never took an inventory."""
    import wdpm_amd
    from wdpm_amd.ponds import Ponds
    bd, bw, kw = real_case(hip, module)
    with hip.context(**kw) as a, hip.context(**kw) as b:
        for c in (a, b):
            c.upload(bd, bw)
            c.totaldrain = 0.0
            c.run_block(100, THRES)
            c.run_block(100, THRES)
        with Ponds(a) as p:
            n = p.label_outlets(WET)
            t, s, _ = hold_against_model(bd, MISS, a.download_water(), WET, p, n)
            assert n >= 1 and s["divide_cells"] > 0
            a.begin_block(THRES)
            a.expect_max_diff()
            n2 = p.label_outlets(0.0)
            got = p.outlets(), p.outlet_stats(), p.basins(), p.rims()
            flushed = a.download_water()
            a.iterate(100)
            md_a = a.max_diff()
            hold_against_model(bd, MISS, flushed, 0.0, p, n2)
            assert p.guard_bad() == 0
        md_b = b.run_block(100, THRES)
        assert md_a == md_b
        assert n_bit_diff(a.download_water(), b.download_water()) == 0
        assert a.totaldrain == b.totaldrain
        for c in (a, b):
            assert c.get_option(wdpm_amd.capi.OPT_GUARD_BAD) == 0


def test_basin5(hip, basin5):
    """basin5 after an add of 300 mm and 300 iterations: the outlet table against the model"""
    from wdpm_amd.ponds import Ponds
    dem, hdr = basin5
    miss = hdr["NODATA_value"] if "NODATA_value" in hdr else hdr[[k for k in hdr if k.lower().startswith("nodata")][0]]
    R, Cc = dem.shape
    bd, _ = pad(dem, np.zeros_like(dem), miss)
    bw = np.where(bd > miss, 0.3, 0.0)
    with hip.context(module="add", nrows=R, ncols=Cc, missingvalue=miss) as ctx:
        ctx.upload(bd, bw)
        ctx.run_block(300, THRES)
        with Ponds(ctx) as p:
            n = p.label_outlets(WET)
            t, s, _ = hold_against_model(bd, miss, ctx.download_water(), WET, p, n)
            assert n >= 1 and s["divide_cells"] > 0 and p.guard_bad() == 0
