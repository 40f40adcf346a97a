"""The one check of the pond catchments over row blocks (include/wdpm_group_pond_catchments.h) and the patterns that need a row-block
boundary, shared by tests/test_group_pond_catchments.py (N ranks on one GPU) and tests/test_group_pond_catchments_multi_gpu.py (one
rank per GPU).

Every check is equality: the basin raster, the catchment table and the counts against tests/pond_catchments_model.catchments on the
labels the group returns, the water the group downloads and device_dem of the uploaded DEM (integers by value, head_level by bit
pattern); labels, pond table and rim table of the same call, bit for bit, against the label_rims() of a twin group that holds the same
rasters; the identity sum(pond cells) + sum(catch_cells) + unponded_cells == cells with a level; and no guard byte changed.  Patterns
are placed with rowblock.partition (padded rows; file = padded - 1)."""
import numpy as np

import group_pond_rims_cases as rc
import group_ponds_cases as gc
from group_pond_rims_cases import ramp_dem
from group_ponds_cases import MISS, WET
from helpers import pad
from pond_catchments_model import assert_same_catchments, catchments
from pond_rims_model import device_dem
from ponds_model import assert_same, inventory

ROUND_CAP = 40
BATCH = 4
DIRECTIONS = [(-1, -1), (-1, 0), (-1, 1), (0, -1), (0, 1), (1, -1), (1, 0), (1, 1)]


def check_catchments(grp, p, bd, md, twin=None):
    """label_catchments at md on the group's current water; returns (labels, pond table, basins, catchment table, stats).  `twin`:
    a GroupPonds on a group with the same rasters, whose label_rims() must leave the same labels, pond table and rim table."""
    from wdpm_amd.ponds import CATCH_DTYPE
    n = p.label_catchments(md)
    labels, table, rims, basin, catch, stats = p.labels(), p.table(), p.rims(), p.basins(), p.catchments(), p.catchment_stats()
    water = grp.download_water()
    ref_labels, ref_table = inventory(bd > MISS, water, md)
    assert n == len(ref_table) == stats["ponds"] == p.stats()["ponds"], (n, len(ref_table), stats)
    assert_same(labels, table, ref_labels, ref_table)
    dem = device_dem(bd, MISS)
    assert catch.dtype == CATCH_DTYPE
    assert_same_catchments(basin, catch, stats, *catchments(labels, dem, water, table))
    assert int(table["cells"].sum()) + int(catch["catch_cells"].sum()) + stats["unponded_cells"] == int((dem < np.inf).sum())
    assert stats["slope_cells"] == int(catch["catch_cells"].sum()) + stats["unponded_cells"]
    assert BATCH <= stats["rounds"] <= ROUND_CAP and stats["rounds"] % BATCH == 0, stats
    assert stats["ranks"] == grp.size and 0 <= stats["crossings"] <= stats["exits"] and stats["remote"] >= 0 and stats["resolve_ms"] >= 0, stats
    if grp.size == 1:
        assert stats["exits"] == stats["crossings"] == stats["remote"] == 0, stats
    if twin is not None:
        assert twin.label_rims(md) == n
        assert labels.tobytes() == twin.labels().tobytes() and table.tobytes() == twin.table().tobytes()
        assert rims.tobytes() == twin.rims().tobytes() and p.rims_stats()["slots"] == twin.rims_stats()["slots"]
        assert twin.guard_bad() == 0
    assert p.guard_bad() == 0
    return labels, table, basin, catch, stats


class CatchCase:
    """Two groups with one handle each for several DEMs and waters of one shape: the one under test and its twin."""

    def __init__(self, hip, R, Cc, devices, every=1):
        from wdpm_amd.ponds import GroupPonds
        from wdpm_amd.rowblock import Group
        self.R, self.Cc, self.n = R, Cc, len(devices)
        kw = {} if every is None else dict(exchange_every=every)
        self.grp = Group(hip, "add", R, Cc, MISS, list(devices), **kw)
        self.twin_grp = Group(hip, "add", R, Cc, MISS, list(devices), **kw)
        self.ponds = GroupPonds(self.grp)
        self.twin = GroupPonds(self.twin_grp)

    def __enter__(self):
        return self

    def __exit__(self, *a):
        self.ponds.close()
        self.twin.close()
        self.grp.close()
        self.twin_grp.close()

    def check(self, water, dem=None, nodata=None, thresholds=(WET,)):
        """water and dem in file layout; returns what check_catchments returns for the last threshold"""
        assert water.shape == (self.R, self.Cc)
        if dem is None:
            dem = ramp_dem(self.R, self.Cc, nodata=nodata)
        elif nodata is not None:
            dem = np.where(nodata, MISS, dem)
        self.bd, bw = pad(dem, water, MISS)
        self.grp.upload(self.bd, bw)
        self.twin_grp.upload(self.bd, bw)
        out = None
        for md in thresholds:
            out = check_catchments(self.grp, self.ponds, self.bd, md, self.twin)
        return out


def grid(R, Cc):
    """padded row and column of every file cell"""
    return np.mgrid[1:R + 1, 1:Cc + 1]


def boundaries(slabs):
    """the last owned padded row above every row-block boundary"""
    return [s.own_hi for s in slabs[:-1]]


# ---- ramps across every boundary ---------------------------------------------------------------------------------------------
def run_ramps(case, directions=DIRECTIONS, pits=((1, 0), (-1, 1))):
    """A plane that falls half a metre per cell towards one of the eight neighbours, the two lowest lines under water: every
    descent runs across lanes 0 / 63, columns 1 / ncp - 2 and every row-block boundary, and on the straight directions three
    neighbours tie.  With three ranks and more a rank between the pond and the far end drains to a pond it neither owns nor
    borders on.  Without water the lowest line is a line of pits, and every exit ends in one."""
    R, Cc, n = case.R, case.Cc, case.n
    r, c = grid(R, Cc)
    for dr, dc in directions:
        down = dr * r + dc * c
        dem = 1000.0 - 0.5 * down
        _, table, basin, catch, stats = case.check(np.where(down >= down.max() - 1, 0.3, 0.0), dem)
        assert stats["pit_cells"] == 0 and stats["unponded_cells"] == 0 and (basin[1:-1, 1:-1] > 0).all(), stats
        if dr != 0:
            assert stats["exits"] > 0 and stats["crossings"] > 0, stats
            if n >= 3:
                assert stats["remote"] > 0, stats
        if (dr, dc) in pits:
            _, table, basin, catch, stats = case.check(np.zeros((R, Cc)), dem)
            assert len(table) == 0 and stats["unponded_cells"] == R * Cc and stats["pit_cells"] >= 1 and stats["exits"] > 0, stats
            assert stats["remote"] == 0 and (basin[1:-1, 1:-1] == 0).all()


# ---- a receiver that is a pond cell of the neighbour's row -------------------------------------------------------------------
def run_pond_cell_across(case, slabs):
    """Two cells with a level in a raster of NODATA, one above the other across a boundary: a pond cell and a slope cell whose
    receiver it is.  The slope cell's owner counts the inflow, and no descent exits."""
    R, Cc = case.R, case.Cc
    for hi in sorted({boundaries(slabs)[0], boundaries(slabs)[-1]}):
        for c in rc.target_columns(Cc):
            for pond_below in (True, False):
                pond_row, slope_row = (hi + 1, hi) if pond_below else (hi, hi + 1)
                dem = np.full((R, Cc), MISS)
                w = np.zeros((R, Cc))
                dem[pond_row - 1, c - 1] = 10.0
                w[pond_row - 1, c - 1] = 0.5
                dem[slope_row - 1, c - 1] = 20.0
                _, table, basin, catch, stats = case.check(w, dem)
                assert len(table) == 1 and stats["slope_cells"] == 1 and stats["exits"] == 0 and stats["crossings"] == 0, stats
                assert catch["inflow_cells"][0] == 1 and catch["catch_cells"][0] == 1 and basin[slope_row, c] == 1, catch
                assert (catch["row_min"][0], catch["row_max"][0], catch["head_level"][0]) == (hi, hi + 1, 20.0), catch


# ---- descents that cross a boundary again and again ----------------------------------------------------------------------------
def run_zigzag(case, slabs, steps=7):
    """A channel of single cells in a raster of NODATA that steps diagonally from one side of a boundary to the other, `steps`
    cells long, into a pond cell: every cell but the last exits, and each of them is a seam cell."""
    R, Cc = case.R, case.Cc
    for hi in sorted({boundaries(slabs)[0], boundaries(slabs)[-1]}):
        for c0 in (2, 60) if Cc >= 70 else (1,):
            if c0 + steps > Cc:
                continue
            dem = np.full((R, Cc), MISS)
            w = np.zeros((R, Cc))
            for k in range(steps):
                dem[hi - 1 + k % 2, c0 - 1 + k] = 500.0 - k
            pr, pc = hi + steps % 2, c0 + steps
            dem[pr - 1, pc - 1] = 100.0
            w[pr - 1, pc - 1] = 0.25
            _, table, basin, catch, stats = case.check(w, dem)
            assert len(table) == 1 and catch["catch_cells"][0] == steps and catch["inflow_cells"][0] == 1, catch
            assert stats["exits"] == stats["crossings"] == steps - 1 >= 3, stats
            assert catch["head_level"][0] == 500.0 and (catch["col_min"][0], catch["col_max"][0]) == (c0, pc), catch


def run_snake(case, slabs):
    """A channel in a raster of NODATA down one column through every rank, round in the last rank's rows and up another column into
    a pond cell in the first rank: only what lies above the pond's rank on the way up ends without an exit."""
    R, Cc, n = case.R, case.Cc, case.n
    if Cc < 6:
        return
    a = 2
    dem = np.full((R, Cc), MISS)
    w = np.zeros((R, Cc))
    path = [(r, a) for r in range(1, R + 1)] + [(R, a + 1)] + [(r, a + 2) for r in range(R, 1, -1)]
    for k, (r, c) in enumerate(path):
        dem[r - 1, c - 1] = 5000.0 - 0.125 * k
    dem[0, a + 1] = 100.0                                  # padded (1, a + 2): the pond
    w[0, a + 1] = 0.5
    _, table, basin, catch, stats = case.check(w, dem)
    assert len(table) == 1 and catch["catch_cells"][0] == len(path) and stats["unponded_cells"] == 0, (catch, stats)
    own = [min(s.own_hi, R) - max(s.own_lo, 1) + 1 for s in slabs]       # file rows per rank
    assert min(own) >= 2                                                 # what the counts below take for granted
    # The nodes are the cells of a rank's first owned row (ranks 1 .. n - 1) and of its last one (ranks 0 .. n - 2).  Down column a
    # every one of them exits - those of the last rank through its own first row, after the turn; up column a + 2 all but rank 0's.
    assert stats["crossings"] == (2 * n - 2) + (2 * n - 3) == 4 * n - 5, stats
    # every cell of the way down and of the turn, and what the ranks below the first hold of the way up
    assert stats["exits"] == R + 1 + sum(own[1:]), (stats, own)


def serpentine(R, Cc):
    """a channel that snakes through every other row between high walls and ends in one pond cell (file layout)"""
    dem = 20000.0 + np.arange(R)[:, None] + np.zeros((R, Cc))
    water = np.zeros((R, Cc))
    k, r, c, step = 0, 0, 0, 1
    while True:
        dem[r, c] = 10000.0 - 0.125 * k
        k += 1
        if 0 <= c + step < Cc:
            c += step
            continue
        if r + 2 >= R:
            break
        dem[r + 1, c] = 10000.0 - 0.125 * k
        k += 1
        r += 2
        step = -step
    dem[r, c] -= 1.0
    water[r, c] = 0.5
    return dem, water, k


# ---- ties whose candidates lie in different ranks ------------------------------------------------------------------------------
def run_ties(case, slabs):
    """X in a rank's first owned row; up-right of it, in the rank above, and left of it, in its own row, two cells at one level, each
    with a pond of its own behind it: up-right has the smaller padded index, so X drains across the boundary."""
    R, Cc = case.R, case.Cc
    for hi in sorted({boundaries(slabs)[0], boundaries(slabs)[-1]}):
        for c in (62, 63, 64) if Cc >= 70 else (4,):
            for level in (5.0, 0.0, -0.0):
                dem = np.full((R, Cc), MISS)
                w = np.zeros((R, Cc))
                cell = lambda r, col, v: dem.__setitem__((r - 1, col - 1), v)
                cell(hi + 1, c, 10.0)                      # X
                cell(hi, c + 1, level)                     # up-right, in the rank above
                cell(hi + 1, c - 1, level)                 # left, in X's own row
                cell(hi - 1, c + 2, -20.0)
                w[hi - 2, c + 1] = 1.0                     # the pond behind up-right
                cell(hi + 2, c - 2, -20.0)
                w[hi + 1, c - 3] = 1.0                     # the pond behind left
                labels, table, basin, catch, stats = case.check(w, dem)
                assert len(table) == 2 and basin[hi + 1, c] == labels[hi - 1, c + 2] == 1, (basin[hi + 1, c], labels[hi - 1, c + 2])
                assert stats["exits"] == 1 and (catch["catch_cells"] == [2, 1]).all(), (stats, catch)


# ---- levels on the seam rows: signed zeros, films, NaN water, flats, pits ------------------------------------------------------
def run_seam_levels(case, slabs):
    R, Cc = case.R, case.Cc
    rng = np.random.default_rng(R * Cc + case.n)
    dem = ramp_dem(R, Cc, seed=3)
    w = np.zeros((R, Cc))
    for hi in boundaries(slabs):
        for row in (hi, hi + 1):                               # padded rows either side of the boundary
            dem[row - 1, :] = rng.choice([0.0, -0.0, 0.25, -0.25], Cc)
            kind = rng.random(Cc)
            w[row - 1, :] = np.where(kind < 0.2, WET, np.where(kind < 0.4, WET / 2, np.where(kind < 0.5, np.nan, np.where(kind < 0.6, 0.3, 0.0))))
    _, table, basin, catch, stats = case.check(w, dem, thresholds=(WET, 0.0))
    assert len(table) > 0 and stats["pit_cells"] > 0 and stats["exits"] > 0, stats
    # flats along both rows of every boundary, the land above and below falling towards them: every cell of a flat is a pit
    dem = ramp_dem(R, Cc, seed=4) + 50.0
    for hi in boundaries(slabs):
        dem[hi - 1:hi + 1, :] = 7.0
    _, table, basin, catch, stats = case.check(np.zeros((R, Cc)), dem)
    assert stats["pit_cells"] >= 2 * Cc * len(boundaries(slabs)) and stats["exits"] == 0, stats
    # ... and lone pits on both rows
    for hi in boundaries(slabs):
        dem[hi - 1:hi + 1, :] = 7.0 + 0.5 * (np.arange(Cc) % 3)
    _, table, basin, catch, stats = case.check(np.zeros((R, Cc)), dem)
    assert stats["pit_cells"] > 0


def run_nodata_wall(case, slabs):
    """NODATA all along the last owned row above every boundary: no descent crosses"""
    R, Cc = case.R, case.Cc
    w, nodata = rc.noise(R, Cc, 0.30, 17)
    for hi in boundaries(slabs):
        nodata[hi - 1, :] = True
    _, table, basin, catch, stats = case.check(w, nodata=nodata)
    assert len(table) > 3 and stats["exits"] == 0 and stats["crossings"] == 0 and stats["remote"] == 0, stats


def run_odd_ranks(case, slabs):
    """a rank that is all NODATA, a rank without any pond, an empty raster, all wet"""
    R, Cc = case.R, case.Cc
    mid = slabs[1] if len(slabs) > 2 else slabs[-1]
    rows = slice(max(mid.own_lo, 1) - 1, min(mid.own_hi, R))
    w, nodata = rc.noise(R, Cc, 0.41, 23)
    nodata[rows, :] = True
    _, table, *_ = case.check(w, nodata=nodata)
    assert len(table) > 3
    w, nodata = rc.noise(R, Cc, 0.41, 29)
    w[rows, :] = 0.0
    _, table, basin, catch, stats = case.check(w, nodata=nodata)
    assert len(table) > 3 and stats["exits"] > 0
    _, table, basin, catch, stats = case.check(np.zeros((R, Cc)))
    assert len(table) == 0 and len(catch) == 0 and stats["remote"] == 0 and stats["unponded_cells"] == R * Cc
    assert len(case.ponds.catchments(capacity=0)) == 0
    _, table, basin, catch, stats = case.check(np.full((R, Cc), 0.5))
    assert len(table) == 1 and stats["slope_cells"] == 0 and catch["catch_cells"][0] == 0 and np.isneginf(catch["head_level"][0]), catch
    assert (basin[1:-1, 1:-1] == 1).all() and stats["exits"] == 0


def run_cone(case, slabs):
    """one small pond in the second rank at the foot of a cone that is the whole raster: head level and box extremes lie in other
    ranks than its cells"""
    R, Cc = case.R, case.Cc
    r, c = grid(R, Cc)
    r0, c0 = slabs[1].own_lo + 1, min(70, Cc) // 2 + 1
    dem = 100.0 + 0.5 * np.maximum(np.abs(r - r0), np.abs(c - c0)) + 0.001 * np.abs(c - c0)
    w = np.zeros((R, Cc))
    w[r0 - 1, c0 - 1] = 0.2
    _, table, basin, catch, stats = case.check(w, dem)
    assert len(table) == 1 and catch["catch_cells"][0] == R * Cc - 1 and stats["exits"] > 0
    assert (catch["row_min"][0], catch["row_max"][0], catch["col_min"][0], catch["col_max"][0]) == (1, R, 1, Cc), catch
    assert catch["head_level"][0] == dem.max()


def run_shared_slots(case):
    """local ponds joined through another rank (arms, comb), catchments on either side of them: the shared slot takes both"""
    R, Cc, n = case.R, case.Cc, case.n
    for flip in (False, True):
        w = gc.arms(R, Cc)
        _, table, basin, catch, stats = case.check(w[::-1].copy() if flip else w)
        assert case.ponds.stats()["merged"] == 2 * (n - 1) and catch["catch_cells"].sum() > 0
        w, teeth = gc.comb(R, Cc)
        case.check(w[::-1].copy() if flip else w)
        assert case.ponds.stats()["merged"] == (n - 1) * teeth


def run_noise(case, densities=(0.30, 0.41, 0.60), thresholds=(WET, 0.01)):
    for d in densities:
        w, nodata = rc.noise(case.R, case.Cc, d, int(d * 100) + case.R + case.n)
        _, table, basin, catch, stats = case.check(w, nodata=nodata, thresholds=thresholds)
        assert len(table) > 10 and stats["exits"] > 0 and stats["pit_cells"] > 0, stats
