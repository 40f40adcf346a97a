"""The one check of the pond rims over row blocks (include/wdpm_group_pond_rims.h) and the patterns that need a row-block boundary,
shared by tests/test_group_pond_rims.py (N ranks on one GPU) and tests/test_group_pond_rims_multi_gpu.py (one rank per GPU).

Every check is equality: the rim table against tests/pond_rims_model.rims on the labels the group returns, the water the group
downloads and device_dem of the uploaded DEM (integers by value, doubles by bit pattern), next to the label raster and the pond
table of the same call against tests/ponds_model.inventory.  The DEM is never flat: a ramp plus seeded steps, so that levels
differ and a pattern says where the lowest lies.  Patterns are placed with rowblock.partition (padded rows; file = padded - 1)."""
import numpy as np

import group_ponds_cases as gc
from group_ponds_cases import MISS, WET
from helpers import pad
from pond_rims_model import assert_same_rims, device_dem, rims
from ponds_model import assert_same, inventory


def ramp_dem(R, Cc, seed=0, nodata=None):
    """100 m and up: a ramp down the rows and along the columns plus steps of a quarter metre; NODATA where asked"""
    r, c = np.mgrid[0:R, 0:Cc]
    dem = 100.0 + 0.125 * r + 0.0625 * (c % 7) + 0.25 * np.random.default_rng(seed + R * Cc).integers(0, 4, (R, Cc))
    if nodata is not None:
        dem[nodata] = MISS
    return dem


def check_rims(grp, p, bd, md):
    """label_rims at md on the group's current water; returns (labels, rim table, pond stats, rim stats)"""
    from wdpm_amd.ponds import RIM_DTYPE
    n = p.label_rims(md)
    labels, table, stats, got, rstats = p.labels(), p.table(), p.stats(), p.rims(), p.rims_stats()
    water = grp.download_water()
    ref_labels, ref_table = inventory(bd > MISS, water, md)
    assert n == len(ref_table) == stats["ponds"], (n, len(ref_table), stats)
    assert_same(labels, table, ref_labels, ref_table)
    ranks = [p.rank_stats(i) for i in range(grp.size)]
    assert stats["ranks"] == grp.size and stats["local_ponds"] == sum(r["ponds"] for r in ranks), (stats, ranks)
    assert stats["ponds"] == stats["local_ponds"] - stats["merged"], stats
    assert got.dtype == RIM_DTYPE
    assert_same_rims(got, rims(labels, device_dem(bd, MISS), water, n))
    assert rstats["ranks"] == grp.size and rstats["foreign"] >= 0 and rstats["merge_ms"] >= 0, rstats
    assert rstats["slots"] == stats["local_ponds"] + rstats["foreign"], (rstats, stats)
    assert p.guard_bad() == 0
    return labels, got, stats, rstats


class RimCase:
    """One group and one handle for several DEMs and waters of one shape."""

    def __init__(self, hip, R, Cc, devices, every=1):
        from wdpm_amd.ponds import GroupPonds
        from wdpm_amd.rowblock import Group
        self.R, self.Cc, self.n = R, Cc, len(devices)
        kw = {} if every is None else dict(exchange_every=every)
        self.grp = Group(hip, "add", R, Cc, MISS, list(devices), **kw)
        self.ponds = GroupPonds(self.grp)

    def __enter__(self):
        return self

    def __exit__(self, *a):
        self.ponds.close()
        self.grp.close()

    def check(self, water, dem=None, nodata=None, thresholds=(WET,)):
        """water and dem in file layout; returns what check_rims returns for the last threshold"""
        assert water.shape == (self.R, self.Cc)
        if dem is None:
            dem = ramp_dem(self.R, self.Cc, nodata=nodata)
        self.bd, bw = pad(dem, water, MISS)
        self.grp.upload(self.bd, bw)
        out = None
        for md in thresholds:
            out = check_rims(self.grp, self.ponds, self.bd, md)
        return out


def pond_at(labels, table, r, c):
    """the rim row of the pond that holds padded cell (r, c)"""
    assert labels[r, c] > 0, (r, c)
    return table[labels[r, c] - 1]


def target_columns(Cc):
    """padded columns: lanes 0 and 63 of a segment, the raster's first and last file column"""
    return [64, 63, 1, Cc]


# ---- a foreign pond whose lowest rim cell lies across the boundary -----------------------------------------------------------
def run_foreign(case, slabs):
    """A pond of two rows wholly in the rank above boundary b, touching its last owned row; the lowest cell of its rim is in the
    first owned row of the rank below, at padded column c.  Then mirrored: the pond below, the rim cell above."""
    R, Cc = case.R, case.Cc
    for b in sorted({0, len(slabs) - 2}):
        hi = slabs[b].own_hi                      # padded; rank b + 1 begins at hi + 1
        for c in target_columns(Cc):
            for down in (True, False):
                pond_rows = (hi - 1, hi) if down else (hi + 1, hi + 2)
                rim_row = hi + 1 if down else hi
                if min(pond_rows) < 1 or max(pond_rows) > R:
                    continue
                cols = [k for k in (c - 1, c, c + 1) if 1 <= k <= Cc]
                w = np.zeros((R, Cc))
                dem = ramp_dem(R, Cc, seed=c)
                for r in pond_rows:
                    w[r - 1, [k - 1 for k in cols]] = 0.5 + 0.01 * r
                dem[rim_row - 1, c - 1] = 10.0    # far below everything else
                labels, t, stats, rs = case.check(w, dem)
                row = pond_at(labels, t, pond_rows[0], c)
                assert stats["ponds"] == 1 and (row["rim_row"], row["rim_col"], row["rim_level"]) == (rim_row, c, 10.0), (row, b, c, down)
                assert rs["foreign"] > 0, rs


# ---- a neighbour cell that touches one pond from both sides of a boundary, and four ponds at one cell -------------------------
def run_counted_once_and_four_ponds(case, slabs):
    R, Cc = case.R, case.Cc
    hi = slabs[0].own_hi
    for c in (20, 63, 64) if Cc >= 66 else (3,):
        if Cc < c + 3:
            continue
        w = np.zeros((R, Cc))
        for r in (hi, hi + 2):                    # rank 0's last row, rank 1's second; joined round the right of (hi + 1, c)
            w[r - 1, c - 2:c + 1] = 0.25
        w[hi + 1 - 1, c + 2 - 1] = 0.25
        labels, t, stats, _ = case.check(w)
        assert stats["ponds"] == 1 and labels[hi + 1, c] == 0
        # the model's count, spelled out: the box of 5 x 6 cells round the pond, less its 7 cells and the two corners on the right
        assert t["rim_cells"][0] + t["wall_cells"][0] == 5 * 6 - 7 - 2, t
    if Cc >= 66:
        for x_row, x_col in ((hi + 1, 64), (hi, 63)):     # a cell on the boundary and on the segment seam at once
            w = np.zeros((R, Cc))
            depth = 0.125
            for r in (x_row - 1, x_row + 1):
                for c in (x_col - 1, x_col + 1):
                    w[r - 1, c - 1] = depth
                    depth += 0.125
            dem = ramp_dem(R, Cc, seed=7)
            dem[x_row - 1, x_col - 1] = 20.0
            labels, t, stats, rs = case.check(w, dem)
            assert stats["ponds"] == 4 and stats["merged"] == 0 and rs["foreign"] >= 2, (stats, rs)
            assert all((row["rim_row"], row["rim_col"], row["rim_level"]) == (x_row, x_col, 20.0) for row in t), t


# ---- ties across ranks, signed zeros, walls only -------------------------------------------------------------------------------
def run_ties(case, slabs):
    R, Cc = case.R, case.Cc
    hi = slabs[0].own_hi
    c0 = min(30, Cc - 4)
    for upper, lower in ((5.0, 5.0), (0.0, -0.0), (-0.0, 0.0), (-0.0, -0.0)):
        w = np.zeros((R, Cc))
        w[hi - 1:hi + 1, c0:c0 + 3] = 0.5         # padded rows hi and hi + 1: a pond on both sides of the boundary
        dem = ramp_dem(R, Cc, seed=11)
        dem[hi - 2, c0 + 1] = upper               # padded (hi - 1, c0 + 2), in rank 0
        dem[hi + 1, c0 + 1] = lower               # padded (hi + 2, c0 + 2), in rank 1
        labels, t, stats, _ = case.check(w, dem)
        want_lower = np.signbit(lower) and not np.signbit(upper)
        assert stats["ponds"] == 1 and t["rim_row"][0] == (hi + 2 if want_lower else hi - 1) and t["rim_col"][0] == c0 + 2, (t, upper, lower)
        assert np.signbit(t["rim_level"][0]) == np.signbit(lower if want_lower else upper)
    # a cell in rank 0's last row, walled in by NODATA on both sides of the boundary: +inf, -1, -1
    w = np.zeros((R, Cc))
    nodata = np.zeros((R, Cc), dtype=bool)
    nodata[hi - 2:hi + 1, c0:c0 + 3] = True
    nodata[hi - 1, c0 + 1] = False
    w[hi - 1, c0 + 1] = 0.75
    w[nodata] = 0.3                               # water on NODATA is no pond
    labels, t, stats, rs = case.check(w, nodata=nodata)
    assert stats["ponds"] == 1 and t["rim_cells"][0] == 0 and t["wall_cells"][0] == 8 and rs["foreign"] == 1, (t, rs)
    assert np.isposinf(t["rim_level"][0]) and t["rim_row"][0] == -1 and t["rim_col"][0] == -1


# ---- ponds that lean on the raster's first and last row ------------------------------------------------------------------------
def run_border_walls(case):
    R, Cc = case.R, case.Cc
    w = np.zeros((R, Cc))
    w[0, :] = 0.5
    w[R - 1, 2:] = 0.25
    labels, t, stats, _ = case.check(w)
    assert stats["ponds"] == 2
    # the border row above (with both corners) and two cells of either side column; below, one side column only
    assert t["wall_cells"][0] == (Cc + 2) + 4 and t["wall_cells"][1] == Cc + 2, t


# ---- shared slots, one pond through every rank ---------------------------------------------------------------------------------
def run_shared_slots(case):
    R, Cc, n = case.R, case.Cc, case.n
    for flip in (False, True):
        w = gc.arms(R, Cc)
        _, _, s, _ = case.check(w[::-1].copy() if flip else w)
        assert s["merged"] == 2 * (n - 1), s
        w, teeth = gc.comb(R, Cc)
        _, _, s, _ = case.check(w[::-1].copy() if flip else w)
        assert s["merged"] == (n - 1) * teeth, (s, teeth)


def run_serpentine(case, slabs):
    """one pond through every rank, with a dry channel along the last owned row of every other rank: the rows either side of it
    are wet all along and the channel stops short of the left end, so the pond stays one and every channel cell touches it from
    above, in its own rank, and from below, in the next"""
    R, Cc = case.R, case.Cc
    w = gc.serpentine_transposed(R, Cc)
    for s in slabs[:-1:2]:
        w[s.own_hi - 2, :] = 0.5
        w[s.own_hi, :] = 0.75
        w[s.own_hi - 1, 4:] = 0.0
    _, t, stats, _ = case.check(w)
    assert stats["ponds"] == 1 and stats["merged"] == stats["local_ponds"] - 1 and t["rim_cells"][0] > Cc, (stats, t)


# ---- noise ---------------------------------------------------------------------------------------------------------------------
def noise(R, Cc, density, seed):
    """the water of group_ponds_cases.noise (films of a few tenths of a millimetre among it), 3 % NODATA with water on it"""
    w, _ = gc.noise(R, Cc, density, seed)
    rng = np.random.default_rng(seed + 1)
    film = rng.random((R, Cc)) < 0.05
    w[film] = rng.random(int(film.sum())) * WET           # 0 < w <= min_depth: dry for the labels, counted into a rim level
    return w, rng.random((R, Cc)) < 0.03


def run_noise(case, densities=(0.30, 0.41, 0.60), thresholds=(WET, 0.01)):
    for d in densities:
        w, nodata = noise(case.R, case.Cc, d, int(d * 100) + case.R + case.n)
        _, t, s, rs = case.check(w, nodata=nodata, thresholds=thresholds)
        assert s["ponds"] > 10 and s["stitch_unions"] > 0 and (t["wall_cells"] > 0).any(), s
        if d < 0.5:
            assert rs["foreign"] > 0, rs
